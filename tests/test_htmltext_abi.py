"""The HTML text entries (include/cld_mi355x.h) without a GPU: the header declares
them, the library exports them, the bindings exist, the status record has its
documented layout, the block-tag list is the one the tests restate, and the
argument checks -- those of the two device entries come before cld_init -- give
CLD_EINVAL with nothing written.  The n == 0 cases of the host entries."""
import ctypes
import os
import re

import numpy as np
import pytest

import cld_amd
import htmltext_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = cld_amd.EINVAL
DECLS = {"cld_html_text": r"\bint\s+cld_html_text\s*\(\s*const\s+uint8_t\s*\*\s*buf\b",
         "cld_html_text_device": r"\bint\s+cld_html_text_device\s*\(\s*int\s+device\b",
         "cld_chunks_to_page": r"\bint\s+cld_chunks_to_page\s*\(\s*const\s+uint64_t\s*\*\s*offsets\b",
         "cld_chunks_to_page_device": r"\bint\s+cld_chunks_to_page_device\s*\(\s*int\s+device\b"}
PATTERN = 0x5A


class Status(ctypes.Structure):                     # cld_htmltext_status as the header writes it
    _fields_ = [("text_bytes", ctypes.c_uint64), ("tags", ctypes.c_uint64), ("entities", ctypes.c_uint32),
                ("dropped", ctypes.c_uint32)]


def test_header_library_and_bindings():
    src = open(os.path.join(ROOT, "include", "cld_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+CLD_HTMLTEXT_BLOCK_LF\s+1u\b", code) and cld_amd.HTMLTEXT_BLOCK_LF == 1
    lib = ctypes.CDLL(cld_amd.LIB_PATH)
    for name, decl in DECLS.items():
        assert re.search(decl, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in cld_amd.EXPORTS
    for f in ("html_text", "html_text_device", "chunks_to_page", "chunks_to_page_device"):
        assert callable(getattr(cld_amd, f))
    assert ctypes.sizeof(Status) == 24 == cld_amd.HTMLTEXT_STATUS_DTYPE.itemsize
    assert [cld_amd.HTMLTEXT_STATUS_DTYPE.fields[f][1] for f in ("text_bytes", "tags", "entities", "dropped")] == [0, 8, 16, 20]
    assert re.search(r"typedef\s+struct\s+cld_htmltext_status\s*\{\s*uint64_t\s+text_bytes;\s*uint64_t\s+tags;\s*"
                     r"uint32_t\s+entities;\s*uint32_t\s+dropped;\s*\}\s*cld_htmltext_status;", code)
    # the block-tag list is part of the header
    m = re.search(r"#define\s+CLD_HTMLTEXT_BLOCK_TAGS\s*\\\n((?:\s*\"[^\"]*\"\s*\\?\n)+)", code)
    assert m and "".join(re.findall(r'"([^"]*)"', m.group(1))).split() == hc.BLOCK_TAGS
    assert len(hc.BLOCK_TAGS) == 44 and max(map(len, hc.BLOCK_TAGS)) == 10
    kernels = open(os.path.join(ROOT, "language-detector_amd", "csrc", "cld_kernels.h")).read()
    assert re.search(r"kHtmlTextStage\s*=\s*%d\b" % cld_amd.HTMLTEXT_STAGE, kernels)
    assert re.search(r"kHtmlTextCands\s*=\s*%d\b" % cld_amd.HTMLTEXT_CANDS, kernels)


def buffers(n, cap):
    """Host arrays standing in for device memory, filled with a pattern: the checks under test return before
    any of it is read or written."""
    h = {"buf": np.zeros(64, np.uint8), "offs": np.zeros(n + 1, np.uint64), "out": np.zeros(64, np.uint8),
         "tl": np.zeros(n, np.int32), "pos": np.zeros(64, np.uint32), "st": np.zeros(3, np.uint64),
         "chunks": np.zeros(cap, cld_amd.CHUNK_DTYPE), "coffs": np.zeros(n + 1, np.uint64),
         "page": np.zeros(cap, cld_amd.CHUNK_DTYPE)}
    for v in h.values():
        v.view(np.uint8)[:] = PATTERN
    return h


def untouched(h):
    return all((v.view(np.uint8) == PATTERN).all() for v in h.values())


def test_html_text_argument_errors():
    L, n = cld_amd.lib(), 5
    h = buffers(n, 8)
    p = {k: v.ctypes.data for k, v in h.items()}
    host, dev = L.cld_html_text, L.cld_html_text_device
    good = dict(buf=p["buf"], offs=p["offs"], n=n, flags=0, out=p["out"], tl=p["tl"], pos=p["pos"], st=p["st"])

    def device(buf_bytes=64, **change):
        a = dict(good, **change)
        return dev(0, a["buf"], a["offs"], a["n"], buf_bytes, a["flags"], a["out"], a["tl"], a["pos"], a["st"], None)

    def both(**change):
        a = dict(good, **change)
        return host(a["buf"], a["offs"], a["n"], a["flags"], a["out"], a["tl"], a["pos"], a["st"]), device(**change)

    assert both(n=1 << 31) == (E, E)                                          # n > INT32_MAX
    for bit in (2, 4, 0x100, 0x80000000):                                     # unknown flag bits
        assert both(flags=bit) == (E, E) and both(flags=bit | cld_amd.HTMLTEXT_BLOCK_LF) == (E, E)
        assert both(flags=bit, n=0) == (E, E)
    assert both(offs=None) == (E, E)
    assert device(buf=None) == E and device(out=None) == E                    # bytes, no buffer
    assert device(buf=None, n=0) == E and device(out=None, n=0) == E          # ... whatever n is
    assert device(offs=p["offs"] + 4) == E and device(tl=p["tl"] + 2) == E and device(pos=p["pos"] + 1) == E
    assert device(st=p["st"] + 4) == E
    assert untouched(h)
    # the host entry with pages and no buffer
    offs = np.array([0, 5], np.uint64)
    out = np.zeros(5, np.uint8)
    assert host(None, offs.ctypes.data, 1, 0, out.ctypes.data, None, None, None) == E
    assert host(out.ctypes.data, offs.ctypes.data, 1, 0, None, None, None, None) == E


def test_html_text_no_pages():
    st = np.full(3, 0x5A5A5A5A5A5A5A5A, np.uint64)
    offs = np.array([7], np.uint64)
    assert cld_amd.lib().cld_html_text(None, None, 0, cld_amd.HTMLTEXT_BLOCK_LF, None, None, None, st.ctypes.data) == 0
    assert not st.any()
    assert cld_amd.lib().cld_html_text(None, offs.ctypes.data, 0, 0, None, None, None, None) == 0
    got = cld_amd.html_text(np.zeros(0, np.uint8), np.array([0, 0, 0], np.uint64), pos=True)     # empty pages only
    assert list(got["text_len"]) == [0, 0] and hc.status_list(got["status"]) == [0, 0, 0, 0]


def test_chunks_to_page_argument_errors_and_no_documents():
    L, n, cap = cld_amd.lib(), 5, 8
    h = buffers(n, cap)
    p = {k: v.ctypes.data for k, v in h.items()}
    host, dev = L.cld_chunks_to_page, L.cld_chunks_to_page_device
    good = dict(offs=p["offs"], n=n, pos=p["pos"], chunks=p["chunks"], cap=cap, coffs=p["coffs"], page=p["page"])
    order = ("offs", "n", "pos", "chunks", "cap", "coffs", "page")

    def both(**change):
        a = [dict(good, **change)[k] for k in order]
        return host(*a), dev(0, *a, None)

    assert both(n=1 << 31) == (E, E) and both(cap=1 << 32) == (E, E)          # as cld_chunk_totals
    for k in ("offs", "chunks", "coffs", "pos", "page"):
        assert both(**{k: None}) == (E, E), k
    assert both(coffs=None, n=0) == (E, E)
    assert untouched(h)
    # no documents, no chunks: nothing to do, nothing touched (the host entry; the device entry needs its context)
    assert host(None, 0, None, None, 0, p["coffs"], None) == 0
    assert host(p["offs"], n, None, None, 0, p["coffs"], None) == 0
    assert untouched(h)


def chunk_inputs(seed=5):
    """Pages with a pos that is partly hostile, and vectors with negative bytes, offsets outside the document,
    chunks past chunk_cap, empty and inverted ranges."""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 40, 64, 300, 0, 17]
    offs = np.zeros(len(lens) + 1, np.uint64)
    offs[0] = 9
    offs[1:] = 9 + np.cumsum(lens)
    pos = np.zeros(int(offs[-1]) + 5, np.uint32)
    for a, L in zip(offs[:-1], lens):
        a = int(a)
        pos[a:a + L] = np.sort(rng.integers(0, L + 1, size=L))
    pos[int(offs[4]) + 10] = 5000                                    # above L: clamped
    pos[int(offs[4]) + 200] = 3                                      # goes down: bytes 0, never negative
    pos[int(offs[2]) + 5] = 0xFFFFFFFF
    counts = [2, 3, 9, 0, 40, 4, 6]
    coffs = np.zeros(len(lens) + 1, np.uint64)
    coffs[1:] = np.cumsum(counts)
    total = int(coffs[-1])
    ch = np.zeros(total, cld_amd.CHUNK_DTYPE)
    ch["offset"] = rng.integers(-20, 330, size=total)
    ch["bytes"] = rng.integers(-30, 120, size=total)
    ch["lang1"] = rng.integers(0, 700, size=total)
    ch["pad"] = 0x7777
    ch["offset"][:4] = [0, -2147483648, 2147483647, 2147483647]
    ch["bytes"][:4] = [2147483647, 2147483647, 2147483647, -2147483648]
    return offs, pos, ch, coffs


@pytest.mark.parametrize("cap_less", [0, 7, 1000])
def test_chunks_to_page_host_equals_definition(cap_less):
    offs, pos, ch, coffs = chunk_inputs()
    cap = max(len(ch) - cap_less, 0)
    want = hc.expected_to_page(offs, pos, ch, coffs, cap)
    got = cld_amd.chunks_to_page(offs, pos, ch[:cap] if cap else ch[:1], coffs, chunk_cap=cap)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    if cap:
        assert (got["bytes"] >= 0).all() and (got["offset"] >= 0).all() and not got["pad"].any()
        # in place
        buf = ch[:cap].copy()
        rc = cld_amd.lib().cld_chunks_to_page(offs.ctypes.data, len(offs) - 1, pos.ctypes.data, buf.ctypes.data, cap,
                                              coffs.ctypes.data, buf.ctypes.data)
        assert rc == 0 and np.array_equal(buf.view(np.uint8), want.view(np.uint8))
