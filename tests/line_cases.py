"""The expectations of the line entries, in numpy, written from the definitions in
include/cld_mi355x.h ("A batch split into lines") and not from the C++: the
boundary set B, CLD_LINES_JOIN_BLANK, line_offsets / doc_lines / line_doc / the
status, and the chunks cld_lines_to_chunks makes of per-line results.  Also the
batches the host and GPU tests share.  Everything is integers: every comparison
is exact."""
import numpy as np

import cld_amd

JOIN = cld_amd.LINES_JOIN_BLANK
TILE = cld_amd.LINES_TILE
WGS = cld_amd.LINES_WGS
I32MAX = 2 ** 31 - 1
LF = 0x0A


def expected_split(buf, offs, flags=0):
    """-> dict of line_offsets uint64[m + 1], doc_lines uint64[n + 1], line_doc uint32[m], total, longest."""
    buf = np.asarray(buf, np.uint8)
    offs = np.asarray(offs, np.uint64).astype(np.int64)
    n = len(offs) - 1
    assert n >= 1 and (np.diff(offs) >= 0).all()
    own = np.unique(offs)                                    # the distinct values of offsets
    after_lf = offs[0] + np.flatnonzero(buf[offs[0]:offs[n]] == LF) + 1
    pure = after_lf[~np.isin(after_lf, own)]                 # LF boundaries that are no value of offsets
    if flags & JOIN and len(pure):
        raw = np.union1d(own, after_lf)                      # the unflagged B
        p = pure - 1
        start = raw[np.searchsorted(raw, p, side="right") - 1]   # the largest element of it that is <= p
        above = np.concatenate([[0], np.cumsum(buf > 0x20)])
        pure = pure[above[p + 1] - above[start] > 0]         # dropped: no byte above 0x20 in [start, p]
    lo = np.union1d(own, pure)
    m = len(lo) - 1
    return {"line_offsets": lo.astype(np.uint64),
            "doc_lines": np.searchsorted(lo, offs, side="left").astype(np.uint64),
            "line_doc": (np.searchsorted(offs, lo[:m], side="right") - 1).astype(np.uint32),
            "total": m, "longest": int(np.diff(lo).max()) if m else 0}


def check_invariants(buf, offs, flags, s):
    """The properties section 1 of the contract states, asserted directly on a split s."""
    buf = np.asarray(buf, np.uint8)
    offs = np.asarray(offs, np.uint64).astype(np.int64)
    lo, dl, ld = s["line_offsets"].astype(np.int64), s["doc_lines"].astype(np.int64), s["line_doc"].astype(np.int64)
    n, m = len(offs) - 1, len(lo) - 1
    assert lo[0] == offs[0] and lo[m] == offs[n] and (np.diff(lo) > 0).all()
    assert dl[n] == m and (lo[dl] == offs).all()
    assert (np.diff(dl) == 0)[np.diff(offs) == 0].all(), "an empty document has a line"
    assert (offs[ld] <= lo[:m]).all() and (lo[1:] <= offs[ld + 1]).all(), "a line crosses a document"
    assert (dl[ld] <= np.arange(m)).all() and (np.arange(m) < dl[ld + 1]).all()
    last = np.zeros(m, bool)
    last[dl[1:][np.diff(dl) > 0] - 1] = True
    assert (buf[lo[1:][~last] - 1] == LF).all(), "a line that is not its document's last lacks its LF"
    above = np.concatenate([[0], np.cumsum(buf > 0x20)])
    lfs = np.concatenate([[0], np.cumsum(buf == LF)])
    if flags & JOIN:
        assert (above[lo[1:]] - above[lo[:m]] > 0)[~last].all(), "a joined line that is not the last is blank"
    else:
        assert (lfs[np.maximum(lo[1:] - 1, lo[:m])] - lfs[lo[:m]] == 0).all(), "an LF inside a line"


def expected_chunks(results, line_offsets, line_doc, offs, doc_lines, gflags=0, cap=None):
    """cld_lines_to_chunks from its definition -> CHUNK_DTYPE[min(doc_lines[n], cap)]."""
    n = len(offs) - 1
    cap = len(line_doc) if cap is None else cap
    m = min(int(doc_lines[n]), cap)
    res = np.asarray(results, cld_amd.RESULT_DTYPE)[:m]
    key = (res["lang3"][:, 0] if gflags & cld_amd.GROUP_TOP1 else res["summary_lang"]).astype(np.int64)
    if gflags & cld_amd.GROUP_RELIABLE_ONLY:
        key = np.where(res["is_reliable"] == 0, cld_amd.UNKNOWN_LANGUAGE, key)
    out = np.zeros(m, cld_amd.CHUNK_DTYPE)
    out["lang1"] = key
    lo = np.asarray(line_offsets, np.uint64)[:m + 1].astype(np.int64)        # (the tests stay below 2^63)
    i = np.asarray(line_doc, np.uint32)[:m].astype(np.int64)
    own = i < n                                              # a line of a document >= n: {0, 0, key, 0}
    start = np.asarray(offs, np.uint64).astype(np.int64)[np.minimum(i, n - 1)]
    out["offset"] = np.where(own, np.clip(lo[:m] - start, 0, I32MAX), 0)
    out["bytes"] = np.where(own, np.clip(lo[1:] - lo[:m], 0, I32MAX), 0)
    return out


def random_results(m, seed):
    """m results with keys on both sides of every flag: reliable or not, lang3[0] differing from the summary."""
    rng = np.random.default_rng(seed)
    res = np.zeros(m, cld_amd.RESULT_DTYPE)
    res["summary_lang"] = rng.choice([0, 3, 26, 41, 613, 614, 0xFFFF], m)
    res["lang3"][:, 0] = rng.choice([1, 3, 9, 26, 500], m)
    res["is_reliable"] = rng.integers(0, 2, m)
    return res


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s values, want %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: %d differ, first at %d: %s, want %s" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------- batches

LAYOUTS = ("tweets", "one", "mixed", "alllf", "nolf")
LEAD = 37                      # bytes of the buffer before offsets[0], LF among them
TAIL = 21                      # and behind offsets[n]


def text(rng, nbytes, lf=0.03):
    """Letters, blanks (0x20, tab, CR, NUL), bytes above 0x7F, LF; and blank runs with LFs in them."""
    t = rng.choice(np.array([0x41, 0x62, 0x7A, 0xC3, 0xA9, 0x21, 0x20, 0x20, 0x09, 0x0D, 0x00], np.uint8), nbytes)
    t[rng.random(nbytes) < lf] = LF
    for _ in range(nbytes // 300 + 1):
        a, k = int(rng.integers(0, nbytes)), int(rng.integers(1, 40))
        t[a:a + k] = rng.choice(np.array([0x20, LF, 0x0D, LF], np.uint8), len(t[a:a + k]))
    return t


def cut(rng, nbytes, layout):
    """Document lengths summing to nbytes."""
    if layout == "one":
        return [nbytes]
    lens = []
    while sum(lens) < nbytes:
        if layout == "tweets":
            lens.append(int(rng.integers(1, 141)))
        else:
            lens.append(0 if rng.random() < 0.35 else int(rng.integers(1, 3000)))
    lens[-1] -= sum(lens) - nbytes
    if layout != "tweets":
        lens += [0, 0]
        lens = [0] + lens
    return lens


def pack(lens, body, rng=None, lead=LEAD):
    """-> (the whole buffer: lead bytes, the text, TAIL bytes; offsets[0] == lead)."""
    edge = np.array([LF, 0x41, LF, LF, 0x20], np.uint8)
    buf = np.concatenate([np.resize(edge, lead), np.asarray(body, np.uint8), np.resize(edge, TAIL)])
    offs = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    assert int(offs[-1]) == lead + len(body)
    return buf, offs


def layout_case(nbytes, layout, seed, lead=LEAD):
    rng = np.random.default_rng(seed)
    if layout == "alllf":
        body = np.full(nbytes, LF, np.uint8)
        lens = cut(rng, nbytes, "mixed" if nbytes > 40 else "one")
    elif layout == "nolf":
        body = text(rng, nbytes, lf=0.0)
        body[body == LF] = 0x20
        lens = cut(rng, nbytes, "mixed" if nbytes > 40 else "one")
    else:
        body = text(rng, nbytes)
        lens = cut(rng, nbytes, layout)
    return pack(lens, body, lead=lead)


def seam_case(lead_align=0):
    """LFs and document boundaries exactly at tile seams and at a range seam.  With the text's first byte at
    a 16-byte aligned address (the tests place it so) tile t is text bytes [t * TILE, (t + 1) * TILE).
    The text has 2 * WGS tiles, the last one ragged: two tiles per range."""
    nt = 2 * WGS - 1
    body = np.full(nt * TILE + 77, 0x61, np.uint8)
    for t in (1, 2, 5, 6):
        body[t * TILE - 1] = LF                  # the last byte of a tile
    for t in (3, 5, 9):
        body[t * TILE] = LF                      # the first byte of a tile (tile 5: both)
    body[2 * 7 * TILE - 1] = LF                  # the last byte of a range
    body[2 * 9 * TILE] = LF                      # the first byte of a range
    body[2 * 20 * TILE - 1] = LF                 # a document that ends with its LF at a range seam
    bounds = sorted({4 * TILE, 8 * TILE, 2 * 11 * TILE, 2 * 20 * TILE, 2 * 30 * TILE + 1, 2 * 31 * TILE - 1})
    lens = np.diff([0] + bounds + [len(body)])
    return pack(list(lens), body, lead=16 * 3 + lead_align)


def join_cases():
    """name -> (buf, offs): blank runs where the carry of CLD_LINES_JOIN_BLANK has to travel.  Text bytes [t * TILE,
    (t + 1) * TILE) are tile t, two tiles per range (2 * WGS tiles, the last one ragged)."""
    size = (2 * WGS - 1) * TILE + 9
    blank = np.array([0x20, 0x20, LF, 0x09, LF, 0x0D, 0x20], np.uint8)

    def body():
        b = np.full(size, 0x62, np.uint8)
        b[np.arange(500, size, 997)] = LF
        return b

    cases = {}
    b = body()                                   # longer than 3 tiles, text before and after
    b[TILE + 11:5 * TILE - 3] = np.resize(blank, 4 * TILE - 14)
    cases["long_run"] = pack([size], b, lead=32)
    b = body()                                   # across a range seam (tiles 13 | 14)
    b[14 * TILE - 90:14 * TILE + 70] = np.resize(blank, 160)
    cases["range_seam"] = pack([size], b, lead=32)
    b = body()                                   # ends at a document's end: the blank lines form one line
    b[6 * TILE - 300:6 * TILE + 40] = np.resize(blank, 340)
    cases["doc_end"] = pack([6 * TILE + 40, size - 6 * TILE - 40], b, lead=32)
    b = body()                                   # a whole blank tile, text in the next one
    b[8 * TILE:9 * TILE] = np.resize(blank, TILE)
    b[9 * TILE:9 * TILE + 5] = 0x63
    cases["next_tile"] = pack([size], b, lead=32)
    b = body()                                   # cut by a document boundary: the carry resets, the run is two lines
    b[3 * TILE - 200:4 * TILE + 300] = np.resize(blank, TILE + 500)
    cases["cut_by_doc"] = pack([3 * TILE + 100, size - 3 * TILE - 100], b, lead=32)
    b = body()                                   # the text begins with a blank run of tiles
    b[:2 * TILE + 5] = np.resize(blank, 2 * TILE + 5)
    cases["at_start"] = pack([size], b, lead=32)
    return cases


def dense_case(seed=7):
    """Documents of 1..3 bytes over more than two tiles (hundreds of document starts in a tile, far more than
    the 64 offsets a wave probes at once), 300 empty documents in a row in the middle of them, 70 more further
    on, then one document for the rest."""
    rng = np.random.default_rng(seed)
    size = 3 * TILE + 50
    body = text(rng, size, lf=0.05)
    lens = []
    for upto, empties in ((TILE + 300, 300), (2 * TILE + 600, 70)):
        while sum(lens) < upto:
            lens.append(int(rng.integers(1, 4)))
        lens += [0] * empties
    lens.append(size - sum(lens))
    return pack(lens, body)


def ranges_size():
    """Text bytes that use most of the WGS ranges of tiles and leave a ragged last one: 3 tiles per range."""
    return (3 * WGS - 41) * TILE + 333
