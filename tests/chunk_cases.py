"""Inputs and numpy expectations shared by test_chunks_host.py and test_gpu_chunks.py:
synthetic batches with chunk vectors (no detection needed) and what numpy makes of
them, straight from the definitions in include/cld_mi355x.h.  Neither the host
entries nor the kernels compute an expected value."""
import numpy as np

import cld_amd

BINS = cld_amd.GROUP_BINS
I32MAX = 0x7FFFFFFF
LANGS = np.array([0, 26, 3, 41, 613, 614, 0xFFFF], dtype=np.uint16)
PIECE_LENGTHS = (0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025)
BIG_PIECE = (1 << 20) + 3


def select_sets():
    """name -> select[BINS]: one bin, all, none, everything but UNKNOWN_LANGUAGE (26)."""
    one = np.zeros(BINS, np.uint8)
    one[3] = 1
    but26 = np.full(BINS, 0x80, np.uint8)        # (any nonzero byte keeps)
    but26[26] = 0
    return {"one": one, "all": np.ones(BINS, np.uint8), "none": np.zeros(BINS, np.uint8), "but26": but26}


def make_chunks(rows):
    c = np.zeros(len(rows), dtype=cld_amd.CHUNK_DTYPE)
    for k, (off, nbytes, lang) in enumerate(rows):
        c[k] = (off, nbytes, lang, 0xABCD)       # (pad holds noise: nobody reads it)
    return c


def case(docs, vectors, cap=None, coffs=None):
    """docs: bytes each; vectors: a list of (offset, bytes, lang1) rows per document."""
    buf, offs = cld_amd.pack(docs)
    chunks = make_chunks([r for v in vectors for r in v])
    if coffs is None:
        coffs = np.zeros(len(docs) + 1, np.uint64)
        np.cumsum([len(v) for v in vectors], out=coffs[1:])
    return {"buf": np.asarray(buf, np.uint8), "offs": np.asarray(offs, np.uint64), "chunks": chunks,
            "coffs": np.asarray(coffs, np.uint64), "cap": len(chunks) if cap is None else cap}


def layout_case(total, layout, seed):
    """`total` chunks in all, dealt to documents by `layout`:
      ones      every document holds one chunk
      one       one document holds every chunk, empty documents and vectors around it
      mixed     vectors of 0..40 chunks (fewer in a small batch), runs of empty vectors between full ones
      inverted  mixed, with chunk_offsets that go down: the first entry is past every chunk (document 0
                has an inverted, so empty, vector), one vector in the middle is inverted and the next
                starts lower than the last one ended (its first chunks belong to two documents), a
                stretch of chunks belongs to nobody, and the last entry is below the one before it
    Most chunks tile a stretch of their document in order, some with gaps; one in eight has random
    words (negative, past the end, overlapping)."""
    rng = np.random.default_rng(seed)
    if layout == "ones":
        vl = np.ones(total, np.int64)
    elif layout == "one":
        vl = np.zeros(5, np.int64)
        vl[2] = total
    else:
        vl = []
        while sum(vl) < total:
            vl += [0] * int(rng.integers(0, 4)) if rng.random() < 0.3 else [int(rng.integers(1, max(5, min(41, total // 8))))]
        vl[-1] -= sum(vl) - total
        vl = np.array(vl + [0, 0], np.int64)
    n = len(vl)
    coffs = np.zeros(n + 1, np.int64)
    np.cumsum(vl, out=coffs[1:])
    nchunks = total
    if layout == "inverted":
        k = n // 2
        while coffs[k] < 2:
            k += 1
        assert 1 <= k <= n - 3, "too few vectors for this layout"
        unused = 7                                   # chunks total .. total + 7 are nobody's ...
        nchunks = total + unused
        coffs[0] = nchunks + 5                       # document 0: inverted
        vl[0] = 0
        coffs[k + 1] = coffs[k] - 2                  # document k: inverted; k + 1 starts 2 chunks before k did
        vl[k] = 0
        vl[k + 1] = coffs[k + 2] - coffs[k + 1]
        coffs[n] = coffs[n - 1] - 1                  # the last: inverted (its vector was empty before)
        assert vl[n - 1] == 0
        assert vl.sum() <= nchunks                   # (... so the instances still fit the capacity)
    # documents: letters; lengths so that most vectors fit them
    dl = vl * 9 + rng.integers(0, 30, n)
    if layout != "one":
        dl[rng.integers(0, n, max(1, n // 50))] = 0  # some empty documents, their chunks hang in the air
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(dl, out=offs[1:])
    buf = rng.integers(0x61, 0x7B, int(offs[n]), dtype=np.uint8)
    ch = np.zeros(nchunks, cld_amd.CHUNK_DTYPE)
    nb = rng.integers(0, 14, nchunks)
    gap = np.where(rng.random(nchunks) < 0.25, rng.integers(1, 4, nchunks), 0)
    # a chunk's offset: the running sum of bytes and gaps since its vector's first chunk (by chunk index)
    first = np.zeros(nchunks, np.int64)
    a, b = np.minimum(coffs[:-1], nchunks), np.minimum(coffs[1:], nchunks)
    for i in np.nonzero(b > a)[0]:
        first[a[i]:b[i]] = a[i]
    run = np.cumsum(nb + gap) - (nb + gap)
    ch["offset"] = run - run[first] + gap
    ch["bytes"] = nb
    wild = rng.random(nchunks) < 0.125
    ch["offset"][wild] = rng.integers(-20, 400, int(wild.sum()))
    ch["bytes"][wild] = rng.integers(-5, 60, int(wild.sum()))
    ch["lang1"] = LANGS[rng.integers(0, len(LANGS), nchunks)]
    ch["pad"] = 0xABCD
    return {"buf": buf, "offs": offs, "chunks": ch, "coffs": coffs.astype(np.uint64), "cap": nchunks}


def lengths_case():
    """Every piece length of PIECE_LENGTHS at every source alignment 0..15, then one piece of BIG_PIECE
    bytes, one chunk per piece, a few pieces per document; between them dropped chunks (bin 26)."""
    rng = np.random.default_rng(7)
    docs, vectors = [], []
    for ln in PIECE_LENGTHS:
        v, at = [], 0
        for align in range(16):
            at = (at + 15) // 16 * 16 + align
            v.append((at, ln, 3))
            at += ln
            if align % 3 == 0:
                v.append((at, 5, 26))
                at += 5
        docs.append(rng.integers(0x61, 0x7B, at + 9, dtype=np.uint8).tobytes())
        vectors.append(v)
    docs.append(rng.integers(0x61, 0x7B, BIG_PIECE + 20, dtype=np.uint8).tobytes())
    vectors.append([(0, 7, 3), (7, 6, 26), (13, BIG_PIECE, 41), (13 + BIG_PIECE, 7, 3)])
    return case(docs, vectors)


def hostile_case():
    """Chunk words no detector writes, and every neighbour relation of CLD_CHUNKS_SPACE."""
    rng = np.random.default_rng(9)
    L = 40
    docs = [rng.integers(0x61, 0x7B, k, dtype=np.uint8).tobytes() for k in (L, L, 0, L, 25, L)]
    K, D = 3, 26                                     # a kept and a dropped language under "but26" and "one"
    vectors = [
        # offsets and lengths outside the document, overflow of offset + bytes
        [(-1, 5, K), (L, 5, K), (L + 1, 5, K), (I32MAX, 5, K), (4, -1, K), (4, 0, K), (4, I32MAX, K),
         (I32MAX, I32MAX, K), (-I32MAX - 1, I32MAX, K), (-I32MAX - 1, -I32MAX - 1, K), (-3, 10, 41)],
        # overlapping and repeated chunks, the languages at the clamp
        [(0, 20, K), (10, 20, K), (10, 20, K), (10, 20, K), (0, L, 613), (0, L, 614), (0, L, 0xFFFF), (39, 1, 615)],
        # an empty document with chunks
        [(0, 5, K), (-1, 2, K), (0, 0, D)],
        # CLD_CHUNKS_SPACE: kept first; adjacent kept; non-adjacent kept; dropped between two kept;
        # an empty kept-language piece between two adjacent kept chunks
        [(0, 5, K), (5, 4, K), (12, 3, K), (15, 5, D), (20, 5, K), (25, 0, K), (25, 5, K), (30, 5, 41), (35, 5, K)],
        # a dropped chunk first, then kept ones; a chunk that reaches past the end
        [(0, 5, D), (5, 5, K), (10, 5, K), (20, 50, K)],
        [],
    ]
    c = case(docs, vectors)
    # one more document whose offsets go down (a length of 0), with two chunks
    c["chunks"] = np.concatenate([c["chunks"], make_chunks([(0, 5, K), (3, 30, K)])])
    c["offs"] = np.append(c["offs"], c["offs"][-1] - np.uint64(30))
    c["coffs"] = np.append(c["coffs"], c["coffs"][-1] + np.uint64(2))
    c["cap"] += 2
    return c


def capped_case():
    """chunk_cap below chunk_offsets[n]: the cut falls inside document 2's vector."""
    c = layout_case(300, "mixed", seed=31)
    vl = np.diff(c["coffs"].astype(np.int64))
    i = int(np.nonzero(vl >= 5)[0][2])
    c["cap"] = int(c["coffs"][i]) + 2
    assert c["coffs"][i] < c["cap"] < c["coffs"][i + 1] <= c["coffs"][-1]
    return c


def overlap_case():
    """Vectors that overlap so much that together they hold more chunks than there are: chunk_offsets
    goes back to 0 for every other document.  The documented limit of cld_gather_chunks_device: it places
    the first chunk_cap chunk instances in document order (the cut falls inside a vector here); the
    totals and the host entries take them all."""
    c = layout_case(600, "mixed", seed=41)
    co = c["coffs"].astype(np.int64)
    co[2::2] = 0                                     # documents 1, 3, 5, ... are empty, 2, 4, 6, ... start at chunk 0
    co[-1] = 0
    c["coffs"] = co.astype(np.uint64)
    doc, _, _ = instances(c)
    assert len(doc) > 3 * c["cap"] and doc[c["cap"] - 1] == doc[c["cap"]], "the cut should fall inside a vector"
    return c


# ---------------------------------------------------------------- numpy

def instances(c, limit=None):
    """Every chunk of every vector in document order: (document, chunk index, first of its vector);
    limit: only the first `limit` of them (what cld_gather_chunks_device places where overlapping
    vectors hold more than chunk_cap chunks together)."""
    n, cap = len(c["offs"]) - 1, c["cap"]
    co = np.minimum(c["coffs"], np.uint64(cap)).astype(np.int64)
    a = co[:-1]
    vl = np.maximum(co[1:] - a, 0)
    doc = np.repeat(np.arange(n), vl)
    k = np.arange(int(vl.sum())) - np.repeat(np.cumsum(vl) - vl, vl)
    return doc[:limit], (np.repeat(a, vl) + k)[:limit], (k == 0)[:limit]


def pieces(c, limit=None):
    doc, ci, first = instances(c, limit)
    o = c["offs"].astype(np.int64)
    ln = np.maximum(o[1:] - o[:-1], 0)[doc]
    off = c["chunks"]["offset"][ci].astype(np.int64)
    s = np.clip(off, 0, ln)
    e = np.clip(off + c["chunks"]["bytes"][ci].astype(np.int64), s, ln)
    bins = np.minimum(c["chunks"]["lang1"][ci].astype(np.int64), cld_amd.NUM_LANGUAGES)
    return doc, first, s, e, bins


def expected_totals(c):
    _, _, s, e, bins = pieces(c)
    counts = np.bincount(bins, minlength=BINS).astype(np.uint64)
    nbytes = np.zeros(BINS, np.int64)
    np.add.at(nbytes, bins, e - s)
    return {"chunk_counts": counts, "chunk_bytes": nbytes.astype(np.uint64)}


def expected_gather(c, select, flags, limit=None):
    """(bytes, out_offsets) of the whole output (limit: see instances)."""
    doc, first, s, e, bins = pieces(c, limit)
    n = len(c["offs"]) - 1
    kept = (np.asarray(select)[bins] != 0) & (e > s)
    space = np.zeros(len(kept), bool)
    if flags & cld_amd.CHUNKS_SPACE and len(kept):
        joins = np.zeros(len(kept), bool)            # the chunk before is a kept piece ending where this one starts
        joins[1:] = kept[:-1] & (e[:-1] == s[1:])
        space = kept & ~first & ~joins
    ln = np.where(kept, e - s, 0)
    outlen = ln + space
    per_doc = np.zeros(n, np.int64)
    np.add.at(per_doc, doc, outlen)
    out_offs = np.zeros(n + 1, np.uint64)
    np.cumsum(per_doc, out=out_offs[1:])
    at = np.cumsum(outlen) - outlen + space          # where each piece's bytes start in the output
    total = int(outlen.sum())
    out = np.full(total, 0x20, np.uint8)
    idx = np.nonzero(kept)[0]
    lk = ln[idx]
    within = np.arange(int(lk.sum())) - np.repeat(np.cumsum(lk) - lk, lk)
    src = np.repeat(c["offs"].astype(np.int64)[doc[idx]] + s[idx], lk) + within
    out[np.repeat(at[idx], lk) + within] = c["buf"][src]
    return out, out_offs


def slow_gather(c, select, flags):
    """The same by Python slicing, chunk by chunk (small cases: it checks expected_gather itself)."""
    out, offs = bytearray(), [0]
    buf = bytes(c["buf"])
    for i in range(len(c["offs"]) - 1):
        lo, hi = int(c["offs"][i]), int(c["offs"][i + 1])
        doc = buf[lo:hi] if hi > lo else b""
        a, b = int(c["coffs"][i]), min(int(c["coffs"][i + 1]), c["cap"])
        prev = None
        for k in range(a, b):
            off, nb, lang = int(c["chunks"]["offset"][k]), int(c["chunks"]["bytes"][k]), int(c["chunks"]["lang1"][k])
            s = min(max(off, 0), len(doc))
            e = min(max(off + nb, s), len(doc))
            kept = bool(select[min(lang, 614)]) and e > s
            if kept:
                if flags & cld_amd.CHUNKS_SPACE and k != a and not (prev is not None and prev == s):
                    out += b" "
                out += doc[s:e]
            prev = e if kept else None
        offs.append(len(out))
    return np.frombuffer(bytes(out), np.uint8), np.array(offs, np.uint64)


def assert_same(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s%s, numpy %s%s" % (what, g.dtype, g.shape, w.dtype, w.shape)
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, "%s: differs at %d places; first at %d: got %d, numpy %d" % (what, len(bad), bad[0], g[bad[0]],
                                                                                        w[bad[0]])
