"""The chunk entries (include/cld_mi355x.h) without a GPU: the header declares
them, the library exports them, the bindings exist, the records have their
documented sizes, and the argument checks -- those of the two device entries
come before cld_init -- give CLD_EINVAL / CLD_ENOSPC with nothing written."""
import ctypes
import os
import re

import numpy as np

import cld_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, NOSPC = cld_amd.EINVAL, cld_amd.ENOSPC
DECLS = {"cld_chunk_work_bytes": r"\bsize_t\s+cld_chunk_work_bytes\s*\(\s*size_t\s+n\s*,\s*uint64_t\s+chunk_cap\s*\)\s*;",
         "cld_chunk_totals": r"\bint\s+cld_chunk_totals\s*\(\s*const\s+uint64_t\s*\*\s*offsets\b",
         "cld_chunk_totals_device": r"\bint\s+cld_chunk_totals_device\s*\(\s*int\s+device\b",
         "cld_gather_chunks": r"\bint\s+cld_gather_chunks\s*\(\s*const\s+uint8_t\s*\*\s*buf\b",
         "cld_gather_chunks_device": r"\bint\s+cld_gather_chunks_device\s*\(\s*int\s+device\b"}


class Chunk(ctypes.Structure):                      # cld_chunk as the header writes it
    _fields_ = [("offset", ctypes.c_int32), ("bytes", ctypes.c_int32), ("lang1", ctypes.c_uint16), ("pad", ctypes.c_uint16)]


def test_header_library_and_bindings():
    src = open(os.path.join(ROOT, "include", "cld_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+CLD_CHUNKS_SPACE\s+1u\b", code) and cld_amd.CHUNKS_SPACE == 1
    assert re.search(r"#define\s+CLD_GROUP_BINS\s+615u\b", code)
    lib = ctypes.CDLL(cld_amd.LIB_PATH)
    for name, decl in DECLS.items():
        assert re.search(decl, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in cld_amd.EXPORTS
    for f in ("chunk_totals", "gather_chunks", "chunk_totals_device", "gather_chunks_device", "chunk_work_bytes"):
        assert callable(getattr(cld_amd, f))
    # the records the entries read: 12-byte chunks, 64-bit offsets
    assert ctypes.sizeof(Chunk) == 12 == cld_amd.CHUNK_DTYPE.itemsize
    assert [cld_amd.CHUNK_DTYPE.fields[f][1] for f in ("offset", "bytes", "lang1", "pad")] == \
        [Chunk.offset.offset, Chunk.bytes.offset, Chunk.lang1.offset, Chunk.pad.offset] == [0, 4, 8, 10]
    assert re.search(r"typedef\s+struct\s+cld_chunk\s*\{\s*int32_t\s+offset;\s*int32_t\s+bytes;\s*uint16_t\s+lang1;\s*"
                     r"uint16_t\s+pad;\s*\}\s*cld_chunk;", code)
    # the workspace: 8 bytes per chunk and a fixed part, whatever n is
    fixed = cld_amd.chunk_work_bytes(0, 0) - 8
    assert 0 < fixed <= 4 << 20
    for n, cap in ((1, 1), (5, 1000), (1 << 20, 77), (3, 0xFFFFFFFF)):
        assert cld_amd.chunk_work_bytes(n, cap) == fixed + 8 * (cap + 1)


def host_buffers(n, cap):
    """Host arrays standing in for device memory: the checks under test return before any of it is read."""
    return {"buf": np.zeros(64, np.uint8), "offs": np.zeros(n + 1, np.uint64), "chunks": np.zeros(cap, cld_amd.CHUNK_DTYPE),
            "coffs": np.zeros(n + 1, np.uint64), "select": np.zeros(615, np.uint8), "counts": np.zeros(615, np.uint64),
            "bytes": np.zeros(615, np.uint64), "out": np.zeros(64, np.uint8), "ooffs": np.zeros(n + 1, np.uint64),
            "work": np.zeros(cld_amd.chunk_work_bytes(n, cap) // 8 + 1, np.uint64)}


def test_totals_argument_errors():
    L, n, cap = cld_amd.lib(), 9, 20
    h = host_buffers(n, cap)
    p = {k: v.ctypes.data for k, v in h.items()}
    wb = cld_amd.chunk_work_bytes(n, cap)
    host, dev = L.cld_chunk_totals, L.cld_chunk_totals_device
    big = 1 << 40
    for args in ((p["offs"], 1 << 31, p["chunks"], cap, p["coffs"]),          # n > INT32_MAX
                 (p["offs"], n, p["chunks"], 1 << 32, p["coffs"]),            # chunk_cap > UINT32_MAX
                 (p["offs"], n, p["chunks"], cap, None),                      # no chunk_offsets
                 (None, 0, None, 0, None),                                    # ... not even for no documents
                 (None, n, p["chunks"], cap, p["coffs"]),                     # no offsets
                 (p["offs"], n, None, cap, p["coffs"])):                      # chunks that exist nowhere
        assert host(*args, p["counts"], p["bytes"]) == E
        assert dev(0, *args, p["counts"], p["bytes"], p["work"], big, None) == E
    ok = (p["offs"], n, p["chunks"], cap, p["coffs"], p["counts"], p["bytes"])
    assert dev(0, *ok, None, wb, None) == E
    assert dev(0, *ok, p["work"] + 4, wb, None) == E
    for short in (0, 1, wb - 1):
        assert dev(0, *ok, p["work"], short, None) == NOSPC
    assert all(not v.view(np.uint8).any() for v in h.values())


def test_gather_argument_errors():
    L, n, cap = cld_amd.lib(), 9, 20
    h = host_buffers(n, cap)
    p = {k: v.ctypes.data for k, v in h.items()}
    wb = cld_amd.chunk_work_bytes(n, cap)
    host, dev = L.cld_gather_chunks, L.cld_gather_chunks_device
    big = 1 << 40
    good = dict(buf=p["buf"], offs=p["offs"], n=n, chunks=p["chunks"], cap=cap, coffs=p["coffs"], select=p["select"],
                flags=0, out=p["out"], out_cap=64, ooffs=p["ooffs"])
    order = ("buf", "offs", "n", "chunks", "cap", "coffs", "select", "flags", "out", "out_cap", "ooffs")

    def both(work=p["work"], work_bytes=big, **change):
        a = [dict(good, **change)[k] for k in order]
        return host(*a), dev(0, *a, work, work_bytes, None)

    assert both(n=1 << 31) == (E, E)
    assert both(cap=1 << 32) == (E, E)
    assert both(select=None) == (E, E)
    assert both(coffs=None) == (E, E)
    assert both(out=None) == (E, E)                                           # a capacity, no buffer
    assert both(n=0, buf=None, offs=None, chunks=None, cap=0, out=None, ooffs=None) == (E, E)   # ... for no documents too
    assert both(n=0, coffs=None) == (E, E) and both(n=0, select=None) == (E, E)
    for bit in (2, 4, 0x10, 0x80000000):
        assert both(flags=bit) == (E, E) and both(flags=bit | cld_amd.CHUNKS_SPACE) == (E, E)
        assert both(flags=bit, n=0) == (E, E)
    assert both(offs=None) == (E, E) and both(ooffs=None) == (E, E) and both(chunks=None) == (E, E)
    assert both(buf=None) == (E, E)
    a = [good[k] for k in order]
    assert dev(0, *a, None, big, None) == E and dev(0, *a, p["work"] + 4, big, None) == E      # no workspace, a misaligned one
    assert dev(0, *a[:-1], p["ooffs"] + 4, p["work"], big, None) == E
    for out, out_cap in ((p["out"], 64), (None, 0)):                          # the sizing pass needs its workspace too
        for short in (0, wb - 1):
            assert both(work_bytes=short, out=out, out_cap=out_cap)[1] == NOSPC
    assert both(work_bytes=wb, n=1 << 31)[1] == E
    # (the host calls that passed the checks ran on zeros: every vector is empty, nothing is written but zeros)
    assert all(not v.view(np.uint8).any() for v in h.values())
