"""cld_split_lines and cld_lines_to_chunks, the host references (no GPU), against
numpy written from the definitions (line_cases.py).  Every comparison is exact."""
import numpy as np
import pytest

import cld_amd
import line_cases as lc

JOIN = lc.JOIN
LF = lc.LF


def check_split(buf, offs, flags, what):
    want = lc.expected_split(buf, offs, flags)
    lc.check_invariants(buf, offs, flags, want)
    got = cld_amd.split_lines(buf, offs, flags)
    for k in ("line_offsets", "doc_lines", "line_doc"):
        lc.assert_same(got[k], want[k], "%s, flags %d: %s" % (what, flags, k))
    assert int(got["status"]["total_lines"]) == want["total"] and int(got["status"]["max_line_bytes"]) == want["longest"], what
    return want


def pack(docs, lead=0):
    body = np.frombuffer(b"".join(docs), np.uint8)
    return lc.pack([len(d) for d in docs], body, lead=lead)


def test_random_small_batches():
    rng = np.random.default_rng(5)
    differ = 0
    for t in range(400):
        n = int(rng.integers(1, 7))
        lens = rng.integers(0, 14, n) * (rng.random(n) < 0.7)
        body = rng.choice(np.array([LF, LF, 0x20, 0x0D, 0x00, 0x41, 0x42, 0x21, 0x20], np.uint8), int(lens.sum()))
        buf, offs = lc.pack(list(lens), body, lead=int(rng.integers(0, 9)))
        a = check_split(buf, offs, 0, "random %d" % t)
        b = check_split(buf, offs, JOIN, "random %d" % t)
        differ += a["total"] != b["total"]
    assert differ > 50, "CLD_LINES_JOIN_BLANK should act on many of these"


@pytest.mark.parametrize("flags", (0, JOIN))
def test_edges(flags):
    # all LF: every byte is a line without the flag; with it each document is one line
    buf, offs = pack([b"\n\n\n", b"", b"\n", b"\n\n"])
    w = check_split(buf, offs, flags, "all LF")
    assert w["total"] == (3 if flags else 6) and list(w["doc_lines"]) == ([0, 1, 1, 2, 3] if flags else [0, 3, 3, 4, 6])
    # no LF: one line per non-empty document
    buf, offs = pack([b"abc", b"", b"", b"de\r", b"\x00"], lead=7)
    w = check_split(buf, offs, flags, "no LF")
    assert w["total"] == 3 and list(w["line_doc"]) == [0, 3, 4] and list(w["doc_lines"]) == [0, 1, 1, 1, 2, 3]
    assert int(offs[0]) == 7 and int(w["line_offsets"][0]) == 7
    # LF as a document's first byte, as its last byte, and both; CR and NUL are no line ends
    buf, offs = pack([b"\nab", b"ab\n", b"\nab\n", b"a\r\nb\x00c\n\n"], lead=3)
    w = check_split(buf, offs, flags, "LF first and last")
    assert list(np.diff(w["doc_lines"].astype(np.int64))) == ([1, 1, 1, 3] if flags else [2, 1, 2, 3])
    # only empty documents: no line, and line_offsets is the one boundary
    buf, offs = pack([b"", b"", b""], lead=4)
    w = check_split(buf, offs, flags, "empty documents")
    assert w["total"] == 0 and list(w["line_offsets"]) == [4] and not w["doc_lines"].any() and w["longest"] == 0
    # blank lines join the line after them; at a document's end they form one line; a document boundary cuts a run
    buf, offs = pack([b"x\n \n\t\ny\n\n \n", b" \n\nz"])
    w = check_split(buf, offs, flags, "blank runs")
    if flags:
        assert [bytes(buf[a:b]) for a, b in zip(w["line_offsets"][:-1].astype(int), w["line_offsets"][1:].astype(int))] == \
            [b"x\n", b" \n\t\ny\n", b"\n \n", b" \n\nz"]
    else:
        assert w["total"] == 9


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_layouts_and_capacities(layout):
    buf, offs = lc.layout_case(3 * lc.TILE + 11, layout, seed=len(layout))
    for flags in (0, JOIN):
        want = check_split(buf, offs, flags, layout)
        m = want["total"]
        assert m >= 1
        for cap in sorted({m, m - 1, m // 2, 1} - {0} | {m + 3}):
            got = cld_amd.split_lines(buf, offs, flags, line_cap=cap)
            k = min(m, cap)
            lc.assert_same(got["line_offsets"], want["line_offsets"][:k + 1], "%s, capacity %d: line_offsets" % (layout, cap))
            lc.assert_same(got["line_doc"], want["line_doc"][:k], "%s, capacity %d: line_doc" % (layout, cap))
            lc.assert_same(got["doc_lines"], want["doc_lines"], "%s, capacity %d: doc_lines" % (layout, cap))
            assert int(got["status"]["total_lines"]) == m
        # nothing past the extents: guard words behind a short capacity; line_doc and the status left out; the sizing pass
        cap = max(m // 2, 1)
        lo, ld = np.full(cap + 9, 77, np.uint64), np.full(cap + 8, 77, np.uint32)
        dl, n = np.zeros(len(offs), np.uint64), len(offs) - 1
        L = cld_amd.lib()
        assert L.cld_split_lines(buf.ctypes.data, offs.ctypes.data, n, flags, lo.ctypes.data, ld.ctypes.data, cap,
                                 dl.ctypes.data, None) == 0
        assert (lo[min(m, cap) + 1:] == 77).all() and (ld[min(m, cap):] == 77).all()
        lo[:] = 77
        assert L.cld_split_lines(buf.ctypes.data, offs.ctypes.data, n, flags, lo.ctypes.data, None, cap, dl.ctypes.data,
                                 None) == 0
        lc.assert_same(lo[:min(m, cap) + 1], want["line_offsets"][:min(m, cap) + 1], "line_doc left out")
        st = np.zeros(1, cld_amd.LINES_STATUS_DTYPE)
        dl[:] = 0
        assert L.cld_split_lines(buf.ctypes.data, offs.ctypes.data, n, flags, None, None, 0, dl.ctypes.data,
                                 st.ctypes.data) == 0
        assert int(st[0]["total_lines"]) == m
        lc.assert_same(dl, want["doc_lines"], "the sizing pass: doc_lines")


def test_no_documents():
    dl, st = np.full(1, 9, np.uint64), np.full(2, 9, np.uint64)
    lo = np.full(2, 9, np.uint64)
    assert cld_amd.lib().cld_split_lines(None, None, 0, JOIN, lo.ctypes.data, None, 1, dl.ctypes.data, st.ctypes.data) == 0
    assert dl[0] == 0 and not st.any() and (lo == 9).all()


@pytest.mark.parametrize("gflags", (0, cld_amd.GROUP_TOP1, cld_amd.GROUP_RELIABLE_ONLY,
                                    cld_amd.GROUP_TOP1 | cld_amd.GROUP_RELIABLE_ONLY))
def test_lines_to_chunks(gflags):
    buf, offs = lc.layout_case(2 * lc.TILE + 5, "mixed", seed=3)
    s = lc.expected_split(buf, offs, JOIN)
    m = s["total"]
    res = lc.random_results(m, seed=gflags)
    assert len(set(res["is_reliable"])) == 2 and (res["lang3"][:, 0] != res["summary_lang"]).any()
    want = lc.expected_chunks(res, s["line_offsets"], s["line_doc"], offs, s["doc_lines"], gflags)
    got = cld_amd.lines_to_chunks(res, s["line_offsets"], s["line_doc"], offs, s["doc_lines"], gflags)
    lc.assert_same(got.view(np.uint8), want.view(np.uint8), "chunks, group flags %d" % gflags)
    assert not got["pad"].any() and (got["bytes"] > 0).all()
    # the vectors tile each document: chunk_offsets are doc_lines itself
    for i in range(len(offs) - 1):
        v = got[int(s["doc_lines"][i]):int(s["doc_lines"][i + 1])]
        assert int(v["bytes"].sum()) == int(offs[i + 1] - offs[i])
        assert list(v["offset"]) == list(np.cumsum(v["bytes"]) - v["bytes"])
    # a short capacity
    cap = m // 2
    got = cld_amd.lines_to_chunks(res, s["line_offsets"], s["line_doc"], offs, s["doc_lines"], gflags, line_cap=cap)
    lc.assert_same(got.view(np.uint8), want[:cap].view(np.uint8), "chunks, capacity %d" % cap)


def test_lines_to_chunks_foreign_documents_and_saturation():
    """line_doc entries >= n give {0, 0, key, 0}; offsets and lengths past INT32_MAX saturate (no byte is read)."""
    offs = np.array([5, 100, 2 ** 33, 2 ** 40], np.uint64)
    lo = np.array([5, 100, 2 ** 31 + 99, 2 ** 31 + 100, 2 ** 33, 2 ** 33 + 7, 2 ** 40, 3], np.uint64)
    ld = np.array([0, 1, 1, 1, 2, 2, 3], np.uint32)
    ld_foreign = np.array([0, 3, 1, 0xFFFFFFFF, 2, 7, 1], np.uint32)
    dl = np.array([0, 1, 4, 7], np.uint64)
    res = lc.random_results(7, seed=1)
    for line_doc in (ld, ld_foreign):
        want = lc.expected_chunks(res, lo, line_doc, offs, dl, 0)
        got = cld_amd.lines_to_chunks(res, lo, line_doc, offs, dl, 0)
        lc.assert_same(got.view(np.uint8), want.view(np.uint8), "chunks")
    got = cld_amd.lines_to_chunks(res, lo, ld, offs, dl, 0)
    assert list(got["offset"][:4]) == [0, 0, lc.I32MAX, lc.I32MAX] and list(got["bytes"][:5]) == [95, lc.I32MAX, 1, lc.I32MAX, 7]
    assert got["bytes"][5] == lc.I32MAX and got["bytes"][6] == 0          # (line 6 is of document 3 >= n)
    got = cld_amd.lines_to_chunks(res, lo, ld_foreign, offs, dl, 0)
    for j in (1, 3, 5):
        assert (got["offset"][j], got["bytes"][j], got["pad"][j]) == (0, 0, 0) and got["lang1"][j] == res["summary_lang"][j]
