"""The line entries (include/cld_mi355x.h) without a GPU: the header declares
them, the library exports them, the bindings exist, the status record has its
documented size, the workspace stays within its bound, and the argument checks
-- those of the two device entries come before cld_init -- give CLD_EINVAL /
CLD_ENOSPC with nothing written."""
import ctypes
import os
import re

import numpy as np

import cld_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, NOSPC = cld_amd.EINVAL, cld_amd.ENOSPC
DECLS = {"cld_lines_work_bytes": r"\bsize_t\s+cld_lines_work_bytes\s*\(\s*size_t\s+n\s*,\s*uint64_t\s+buf_bytes\s*\)\s*;",
         "cld_split_lines": r"\bint\s+cld_split_lines\s*\(\s*const\s+uint8_t\s*\*\s*buf\b",
         "cld_split_lines_device": r"\bint\s+cld_split_lines_device\s*\(\s*int\s+device\b",
         "cld_lines_to_chunks": r"\bint\s+cld_lines_to_chunks\s*\(\s*const\s+cld_result\s*\*\s*line_results\b",
         "cld_lines_to_chunks_device": r"\bint\s+cld_lines_to_chunks_device\s*\(\s*int\s+device\b"}
PATTERN = 0x5A


class Status(ctypes.Structure):                     # cld_lines_status as the header writes it
    _fields_ = [("total_lines", ctypes.c_uint64), ("max_line_bytes", ctypes.c_uint64)]


def test_header_library_and_bindings():
    src = open(os.path.join(ROOT, "include", "cld_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+CLD_LINES_JOIN_BLANK\s+1u\b", code) and cld_amd.LINES_JOIN_BLANK == 1
    lib = ctypes.CDLL(cld_amd.LIB_PATH)
    for name, decl in DECLS.items():
        assert re.search(decl, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in cld_amd.EXPORTS
    for f in ("split_lines", "split_lines_device", "lines_to_chunks", "lines_to_chunks_device", "lines_work_bytes"):
        assert callable(getattr(cld_amd, f))
    assert ctypes.sizeof(Status) == 16 == cld_amd.LINES_STATUS_DTYPE.itemsize
    assert [cld_amd.LINES_STATUS_DTYPE.fields[f][1] for f in ("total_lines", "max_line_bytes")] == [0, 8]
    assert re.search(r"typedef\s+struct\s+cld_lines_status\s*\{\s*uint64_t\s+total_lines;\s*uint64_t\s+max_line_bytes;\s*\}"
                     r"\s*cld_lines_status;", code)
    kernels = open(os.path.join(ROOT, "language-detector_amd", "csrc", "cld_kernels.h")).read()
    assert re.search(r"kLinesTile\s*=\s*%d\b" % cld_amd.LINES_TILE, kernels)
    assert re.search(r"kLinesWgs\s*=\s*kGroupWgs\b", kernels) and cld_amd.LINES_WGS == cld_amd.GROUP_WGS


def test_workspace_bound():
    """At most 8 (n + 1) + buf_bytes / 64 + 4 MB, whatever line_cap is (it is no argument); enough for a word per tile."""
    for n in (0, 1, 1000, 1 << 20, (1 << 31) - 1):
        for nb in (0, 1, 1023, 1024, 1 << 20, (1 << 32) + 5, 1 << 38):
            wb = cld_amd.lines_work_bytes(n, nb)
            assert wb % 8 == 0 and 8 * (nb // cld_amd.LINES_TILE + 3) <= wb <= 8 * (n + 1) + nb // 64 + (4 << 20)
            assert wb == 8 * (nb // 1024 + 3) + 73728           # the formula the header states


def buffers(n, cap):
    """Host arrays standing in for device memory, filled with a pattern: the checks under test return before
    any of it is read or written."""
    h = {"buf": np.zeros(64, np.uint8), "offs": np.zeros(n + 1, np.uint64), "lo": np.zeros(cap + 1, np.uint64),
         "ld": np.zeros(cap, np.uint32), "dl": np.zeros(n + 1, np.uint64), "st": np.zeros(2, np.uint64),
         "res": np.zeros(cap, cld_amd.RESULT_DTYPE), "chunks": np.zeros(cap, cld_amd.CHUNK_DTYPE),
         "work": np.zeros(cld_amd.lines_work_bytes(n, 64) // 8 + 1, np.uint64)}
    for v in h.values():
        v.view(np.uint8)[:] = PATTERN
    return h


def untouched(h):
    return all((v.view(np.uint8) == PATTERN).all() for v in h.values())


def test_split_argument_errors():
    L, n, cap = cld_amd.lib(), 9, 20
    h = buffers(n, cap)
    p = {k: v.ctypes.data for k, v in h.items()}
    wb = cld_amd.lines_work_bytes(n, 64)
    host, dev = L.cld_split_lines, L.cld_split_lines_device
    big = 1 << 40
    good = dict(buf=p["buf"], offs=p["offs"], n=n, flags=0, lo=p["lo"], ld=p["ld"], cap=cap, dl=p["dl"], st=p["st"])

    def device(work=p["work"], work_bytes=big, buf_bytes=64, **change):
        a = dict(good, **change)
        return dev(0, a["buf"], a["offs"], a["n"], buf_bytes, a["flags"], a["lo"], a["ld"], a["cap"], a["dl"], a["st"],
                   work, work_bytes, None)

    def both(**change):
        a = dict(good, **change)
        return host(a["buf"], a["offs"], a["n"], a["flags"], a["lo"], a["ld"], a["cap"], a["dl"], a["st"]), device(**change)

    assert both(n=1 << 31) == (E, E)                                          # n > INT32_MAX
    assert both(cap=1 << 31) == (E, E) and both(cap=1 << 40) == (E, E)        # the line batch must be a legal n
    for bit in (2, 4, 0x100, 0x80000000):                                     # unknown flag bits
        assert both(flags=bit) == (E, E) and both(flags=bit | cld_amd.LINES_JOIN_BLANK) == (E, E)
        assert both(flags=bit, n=0) == (E, E)
    assert both(lo=None) == (E, E) and both(lo=None, n=0) == (E, E)           # a capacity, no line_offsets
    assert both(offs=None) == (E, E) and both(dl=None) == (E, E)
    assert both(offs=p["offs"] + 4) == (E, E) and both(dl=p["dl"] + 4) == (E, E)
    a = [good[k] for k in ("flags", "lo", "ld", "cap", "dl", "st")]
    assert dev(0, p["buf"], p["offs"], n, 64, *a, None, big, None) == E       # no workspace, a misaligned one
    assert dev(0, p["buf"], p["offs"], n, 64, *a, p["work"] + 4, big, None) == E
    assert dev(0, None, p["offs"], n, 64, *a, p["work"], big, None) == E      # bytes, no buffer
    for lo, cap_ in ((p["lo"], cap), (None, 0)):                              # the sizing pass needs its workspace too
        for short in (0, 1, wb - 1):
            assert device(work_bytes=short, lo=lo, cap=cap_) == NOSPC
    assert device(work_bytes=wb - 1, buf_bytes=1 << 30) == NOSPC
    assert device(work_bytes=wb, n=1 << 31) == E
    assert untouched(h)
    # the host entry with a text and no buffer
    offs = np.array([0, 5], np.uint64)
    dl = np.zeros(2, np.uint64)
    assert host(None, offs.ctypes.data, 1, 0, None, None, 0, dl.ctypes.data, None) == E


def test_lines_to_chunks_argument_errors():
    L, n, cap = cld_amd.lib(), 9, 20
    h = buffers(n, cap)
    p = {k: v.ctypes.data for k, v in h.items()}
    host, dev = L.cld_lines_to_chunks, L.cld_lines_to_chunks_device
    good = dict(res=p["res"], lo=p["lo"], ld=p["ld"], cap=cap, offs=p["offs"], n=n, dl=p["dl"], flags=0, chunks=p["chunks"])
    order = ("res", "lo", "ld", "cap", "offs", "n", "dl", "flags", "chunks")

    def both(**change):
        a = [dict(good, **change)[k] for k in order]
        return host(*a), dev(0, *a, None)

    assert both(n=1 << 31) == (E, E) and both(cap=1 << 31) == (E, E)
    for bit in (4, 8, 0x80000000):
        assert both(flags=bit) == (E, E) and both(flags=bit | cld_amd.GROUP_TOP1) == (E, E) and both(flags=bit, n=0) == (E, E)
    for k in ("res", "lo", "ld", "offs", "dl", "chunks"):
        assert both(**{k: None}) == (E, E), k
    assert both(dl=None, n=0) == (E, E)
    assert untouched(h)
