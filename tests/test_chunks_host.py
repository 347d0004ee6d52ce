"""cld_chunk_totals and cld_gather_chunks, the host references of the chunk entries
(no GPU), against numpy on the synthetic cases of chunk_cases.py; the numpy
reference itself against plain Python slicing on the small ones."""
import numpy as np
import pytest

import chunk_cases as cc
import cld_amd

SELECTS = cc.select_sets()
SPACE = cld_amd.CHUNKS_SPACE
CASES = {"hostile": cc.hostile_case, "capped": cc.capped_case, "lengths": cc.lengths_case,
         "one_chunk": lambda: cc.layout_case(1, "mixed", 1), "ones_65": lambda: cc.layout_case(65, "ones", 2),
         "one_513": lambda: cc.layout_case(513, "one", 3), "mixed_513": lambda: cc.layout_case(513, "mixed", 4),
         "inverted_63": lambda: cc.layout_case(63, "inverted", 5), "inverted_5000": lambda: cc.layout_case(5000, "inverted", 6),
         "mixed_200003": lambda: cc.layout_case(200003, "mixed", 7),
         # vectors that together hold nine times the chunks there are: the host entries take every instance
         "overlap": cc.overlap_case}


@pytest.mark.parametrize("name", list(CASES))
def test_host_entries_equal_numpy(name):
    c = CASES[name]()
    want = cc.expected_totals(c)
    got = cld_amd.chunk_totals(c["offs"], c["chunks"], c["coffs"], chunk_cap=c["cap"])
    for f in want:
        cc.assert_same(got[f], want[f], "%s: %s" % (name, f))
    small = len(c["chunks"]) <= 6000 and name != "lengths"
    for sel, select in SELECTS.items():
        for flags in (0, SPACE):
            what = "%s, select %s, flags %d" % (name, sel, flags)
            data, offs = cc.expected_gather(c, select, flags)
            if small:
                s, so = cc.slow_gather(c, select, flags)
                cc.assert_same(data, s, what + ": numpy against Python slicing")
                cc.assert_same(offs, so, what + ": numpy against Python slicing, offsets")
            hb, ho = cld_amd.gather_chunks(c["buf"], c["offs"], c["chunks"], c["coffs"], select, flags, chunk_cap=c["cap"])
            cc.assert_same(ho, offs, what + ": offsets")
            cc.assert_same(hb, data, what + ": bytes")
            if sel == "one" and flags == 0:
                assert len(data) == int(want["chunk_bytes"][3]), "the totals size one language's buffer exactly"
            if sel == "all" and flags == 0:
                assert len(data) == int(want["chunk_bytes"].sum())


def test_host_capacity():
    """out_offsets hold the true totals whatever the capacity; nothing at or past out_buf + out_cap is written."""
    c = cc.layout_case(513, "mixed", 4)
    data, offs = cc.expected_gather(c, SELECTS["but26"], SPACE)
    total = len(data)
    n = len(c["offs"]) - 1
    L = cld_amd.lib()
    sel = SELECTS["but26"]
    for cap in (total, total - 1, total // 2, 1):
        out = np.full(total + 64, 0x5A, np.uint8)
        oo = np.zeros(n + 1, np.uint64)
        rc = L.cld_gather_chunks(c["buf"].ctypes.data, c["offs"].ctypes.data, n, c["chunks"].ctypes.data, c["cap"],
                                 c["coffs"].ctypes.data, sel.ctypes.data, SPACE, out.ctypes.data, cap, oo.ctypes.data)
        assert rc == 0
        cc.assert_same(oo, offs, "capacity %d: offsets" % cap)
        cc.assert_same(out[:cap], data[:cap], "capacity %d: bytes" % cap)
        assert (out[cap:] == 0x5A).all(), "capacity %d: bytes past the capacity were written" % cap
    oo = np.zeros(n + 1, np.uint64)
    assert L.cld_gather_chunks(c["buf"].ctypes.data, c["offs"].ctypes.data, n, c["chunks"].ctypes.data, c["cap"],
                               c["coffs"].ctypes.data, sel.ctypes.data, SPACE, None, 0, oo.ctypes.data) == 0
    cc.assert_same(oo, offs, "the sizing pass")


def test_host_optional_totals_and_no_documents():
    c = cc.hostile_case()
    want = cc.expected_totals(c)
    n = len(c["offs"]) - 1
    L = cld_amd.lib()
    args = (c["offs"].ctypes.data, n, c["chunks"].ctypes.data, c["cap"], c["coffs"].ctypes.data)
    counts, nbytes = np.full(cc.BINS, 7, np.uint64), np.full(cc.BINS, 7, np.uint64)
    assert L.cld_chunk_totals(*args, counts.ctypes.data, None) == 0 and L.cld_chunk_totals(*args, None, nbytes.ctypes.data) == 0
    assert L.cld_chunk_totals(*args, None, None) == 0
    cc.assert_same(counts, want["chunk_counts"], "counts alone")
    cc.assert_same(nbytes, want["chunk_bytes"], "bytes alone")
    # n == 0: zeros where the pointers are not NULL, out_offsets[0] = 0
    co = np.zeros(1, np.uint64)
    counts[:], nbytes[:] = 7, 7
    assert L.cld_chunk_totals(None, 0, None, 0, co.ctypes.data, counts.ctypes.data, nbytes.ctypes.data) == 0
    assert not counts.any() and not nbytes.any()
    assert L.cld_chunk_totals(None, 0, None, 0, co.ctypes.data, None, None) == 0
    oo = np.full(1, 7, np.uint64)
    sel = cc.select_sets()["all"]
    assert L.cld_gather_chunks(None, None, 0, None, 0, co.ctypes.data, sel.ctypes.data, 0, None, 0, oo.ctypes.data) == 0
    assert list(oo) == [0]
    assert L.cld_gather_chunks(None, None, 0, None, 0, co.ctypes.data, sel.ctypes.data, 0, None, 0, None) == 0
    got = cld_amd.chunk_totals(np.zeros(1, np.uint64), np.zeros(0, cld_amd.CHUNK_DTYPE), np.zeros(1, np.uint64))
    assert not got["chunk_counts"].any() and not got["chunk_bytes"].any()
