"""CLD_FLAG_SCRUB_UTF8 and cld_scrub_utf8_batch / _device on the GPU, judged by
the reference alone (oracle/_ref/librefcld2.so).

Bytes: the reference's loop (test_scrub_host.ref_scrub: SpanInterchangeValid,
a space over the byte at the valid prefix, again) gives the expected copy and
the expected counts.  Results: the reference's unchecked entries on the looped
text, which is interchange-valid, so the reference is defined on it.

The device entries run in child processes (scrub_device_child.py) in which
torch owns the GPU and the buffers.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus
import docflags_cases as dc
from test_gpu_check_utf8 import (BASE, assert_prefixes, assert_results, boundary_family, long_documents, ref_lib,   # noqa: F401
                                 span_valid)
from test_gpu_corrupt import BAD, docs_for
from test_gpu_html_hints import random_hints
from test_scrub_host import ref_scrub
from test_valid_prefix_host import BOUNDARY, encode, ref_prefixes, rejected_code_point

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCRUB = 0x20
LANE = 16
TEXT = BASE * 4


def text(k):
    """Exactly k bytes of interchange-valid text."""
    t = TEXT[:k]
    while t and (t[-1] & 0xC0 == 0x80 or t[-1] >= 0xC0):   # end on a character boundary
        t = t[:-1]
    return t + b"a" * (k - len(t))


class Layout:
    """Documents packed back to back with their batch offsets known, so that a byte can be put
    at a chosen address modulo the lane (16) or the tile (device buffers start tile-aligned)."""

    def __init__(self):
        self.docs, self.pos = [], 0

    def add(self, *docs):
        for d in docs:
            self.docs.append(d)
            self.pos += len(d)

    def align(self, m):
        """A filler document (of the short or the long shape, as it comes) up to the next multiple of m."""
        if self.pos % m:
            self.add(text(-self.pos % m))

    def place(self, seq, k, edge, total):
        """A document of `total` bytes with byte k of seq at its offset `edge`."""
        head = text(edge - k)
        self.add(head + seq + text(total - len(head) - len(seq)))


def splits(seq, junction=None):
    """Where an edge cuts seq: before every byte and behind the last; for a pair only around its junction."""
    if junction is None:
        return range(len(seq) + 1)
    return [k for k in (junction - 1, junction, junction + 1) if 0 <= k <= len(seq)]


def edge_family(tile):
    """Every BAD sequence, and every pair of them back to back, across a lane's byte 15/16, a tile's
    last/first byte, the 64-byte step of the one-wave shape, the 256/257-byte switch between the
    shapes, and a document end (long | long: one lane stores the end of one document and the
    start of the next; short | long, long | short and short | short: the two shapes meet)."""
    lay = Layout()
    seqs = [(s, None) for s in BAD] + [(a + b, len(a)) for a in BAD for b in BAD]
    for seq, j in seqs:
        for k in splits(seq, j):
            lay.align(tile)
            lay.place(seq, k, 10 * LANE, 20 * LANE)                    # byte 15 | 16 of a lane, in a long document
            lay.align(tile)
            lay.place(seq, k, tile, tile + 20 * LANE)                  # last | first byte of a tile
            if j is None:
                lay.align(tile)
                lay.add(text(700))                                     # ... in a document that starts mid-tile
                lay.place(seq, k, tile - 700, tile)
            lay.align(LANE)
            lay.place(seq, k, 64, 64 + 50)                             # the one-wave shape's step of 64 bytes
        for total in (256, 257):                                       # the longest short document, the shortest long one
            lay.align(LANE)
            lay.add(text(total - len(seq)) + seq)
            lay.add(text(100) + seq + text(total - 100 - len(seq)))
        for k in [k for k in splits(seq, j) if 0 < k < len(seq)]:      # a document end inside the sequence
            shapes = ((300, 300), (40, 300)) if j is not None else ((300, 300), (40, 300), (300, 40), (40, 40))
            for a, b in shapes:
                lay.align(LANE)
                lay.add(text(a) + seq[:k], seq[k:] + text(b))
    return lay


def tiny_run(seed=7, n=400):
    """Documents of 0 to 5 bytes, weighted towards the bytes at which a rule changes."""
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(BOUNDARY, np.uint8)
    return [pool[rng.integers(0, len(pool), int(rng.integers(0, 6)))].tobytes() for _ in range(n)]


def build_byte_batch(gpu, lib):
    """Case 1's batch, packed, with the reference loop's copy and counts."""
    tile = gpu.VALID_TILE
    lay = Layout()
    lay.add(*docs_for(31, 600))
    lay.add(*boundary_family(tile))
    lay.add(*[b"ab" + encode(cp) + b"cd" for cp in range(0x110000) if rejected_code_point(cp)])
    fam = edge_family(tile)
    lay.align(tile)
    lay.add(*fam.docs)
    # several documents in one lane's 16 bytes, between the end of a long document and the start of the next
    lay.add(text(300) + b"\xe4\xb8", *tiny_run(), b"\x80" + text(300))
    longs, _ = long_documents(tile)
    lay.align(tile)
    lay.add(*longs)                                                    # tile-aligned (each is a multiple of the tile)
    lay.add(b"abc", *longs)                                            # and after an odd pad
    docs = lay.docs
    assert len(fam.docs) > 5000 and sum(len(d) <= 5 for d in docs) > 400
    span = span_valid(lib)
    looped = [ref_scrub(span, d) for d in docs]
    buf, offs = gpu.pack(docs)
    want = np.frombuffer(b"".join(t for t, _ in looped), dtype=np.uint8)
    counts = np.array([c for _, c in looped], dtype=np.int32)
    assert len(want) == len(buf) and int((counts > 0).sum()) > 5000 and int((counts == 0).sum()) > 2000
    return docs, buf, offs, want, counts


@pytest.fixture(scope="module")
def byte_batch(gpu, ref_lib):   # noqa: F811
    return build_byte_batch(gpu, ref_lib)                              # (computed once)


def assert_bytes(got, cnt, batch, what):
    docs, buf, offs, want, counts = batch
    if not np.array_equal(got, want):
        p = int(np.nonzero(got != want)[0][0])
        d = int(np.searchsorted(offs, p, side="right")) - 1
        raise AssertionError("%s: byte %d differs (document %d of %d bytes, its byte %d): got %#x, the loop %#x, "
                             "input %#x" % (what, p, d, len(docs[d]), p - int(offs[d]), got[p], want[p], buf[p]))
    if cnt is not None:
        bad = np.nonzero(cnt != counts)[0]
        assert len(bad) == 0, "%s: %d counts differ; first: document %d (%d bytes) got %d, the loop changed %d" % (
            what, len(bad), bad[0], len(docs[bad[0]]), cnt[bad[0]], counts[bad[0]])


def test_bytes_and_counts_host_entry(gpu, byte_batch):
    docs, buf, offs, want, counts = byte_batch
    before = buf.copy()
    got, cnt = gpu.scrub_utf8_batch(buf=buf, offsets=offs)
    assert np.array_equal(buf, before), "the input buffer was written"
    assert_bytes(got, cnt, byte_batch, "scrub_utf8_batch")
    got, cnt = gpu.scrub_utf8_batch(buf=buf, offsets=offs, replaced=False)
    assert cnt is None
    assert_bytes(got, None, byte_batch, "scrub_utf8_batch without counts")
    # a batch that starts inside the buffer: out_buf is indexed from its first document on
    a, b = 2000, 9000
    got, cnt = gpu.scrub_utf8_batch(buf=buf, offsets=offs[a:b + 1])
    assert np.array_equal(got, want[int(offs[a]):int(offs[b])]) and np.array_equal(cnt, counts[a:b])
    assert len(gpu.scrub_utf8_batch([])[0]) == 0


def run_child(tmp, mode, buf, offs, **env_more):
    """A child that ends abnormally fails the test that needs it, and nothing else is started."""
    np.savez(tmp / (mode + "_in.npz"), buf=buf, offs=offs)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p), **env_more)
    r = subprocess.run([sys.executable, os.path.join(HERE, "scrub_device_child.py"), mode, str(tmp / (mode + "_in.npz")),
                        str(tmp / (mode + "_out.npz"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "scrub_device_child.py %s ended with %d: %s" % (mode, r.returncode, r.stderr[-3000:])
    return np.load(tmp / (mode + "_out.npz"))


def test_bytes_and_counts_device_entry(gpu, byte_batch, tmp_path):
    docs, buf, offs, want, counts = byte_batch
    got = run_child(tmp_path, "bytes", buf, offs)
    for key in ("aligned", "bytewise", "shifted", "stream"):
        assert_bytes(got[key + "_out"], got[key + "_replaced"], byte_batch, "scrub_utf8_device (%s)" % key)
    assert_bytes(got["nocount_out"], None, byte_batch, "scrub_utf8_device without counts")
    assert (got["nocount_replaced"] == -7).all()


# ---------------------------------------------------------------- scoring

@pytest.fixture(scope="module")
def score_batch(gpu, ref_tables):
    """Case 2's documents, their looped text and which of them the loop changed, on both table sets."""
    label, ref = ref_tables
    span = span_valid(ref.lib)
    docs = docs_for(33, 600)
    looped = [ref_scrub(span, d) for d in docs]
    lbuf, loffs = gpu.pack([t for t, _ in looped])
    changed = np.array([c > 0 for _, c in looped])
    assert 300 < int(changed.sum()) < len(docs) - 300                  # both kinds in numbers
    return label, ref, span, docs, lbuf, loffs, changed


def test_detect_batch(gpu, score_batch):
    label, ref, span, docs, lbuf, loffs, changed = score_batch
    buf, offs = gpu.pack(docs)
    before = buf.copy()
    got = gpu.detect_batch(buf=buf, offsets=offs, flags=SCRUB)
    assert np.array_equal(buf, before)
    assert_results(got, ref.detect_batch(lbuf, loffs, threads=16), "detect_batch(SCRUB) (%s)" % label)


def test_detect_batch_prepared_text(gpu, score_batch):
    """With the service's preparation the scrub applies to the prepared text, as the check does."""
    label, ref, span, docs, _, _, _ = score_batch
    both = gpu.FLAG_STRIP_EXTRAS | gpu.FLAG_CSTRING
    pb, po = gpu.prepare_batch(docs, flags=both)
    prepared = [bytes(pb[po[i]:po[i + 1]]) for i in range(len(docs))]
    looped = [ref_scrub(span, d) for d in prepared]
    assert sum(c > 0 for _, c in looped) > 300
    lbuf, loffs = gpu.pack([t for t, _ in looped])
    assert_results(gpu.detect_batch(docs, flags=SCRUB | both), ref.detect_batch(lbuf, loffs, threads=16),
                   "detect_batch(SCRUB | STRIP_EXTRAS | CSTRING) (%s)" % label)


def test_detect_batch_ex_hints_and_flags(gpu, score_batch):
    label, ref, span, docs, lbuf, loffs, changed = score_batch
    hints = random_hints(gpu, len(docs), seed=71)
    assert_results(gpu.detect_batch_ex(docs, hints=hints, flags=SCRUB), ref.detect_batch(lbuf, loffs, hints=hints, threads=16),
                   "detect_batch_ex(hints, SCRUB) (%s)" % label)
    assert_results(gpu.detect_batch_ex(docs, flags=SCRUB | 0x4100), ref.detect_batch(lbuf, loffs, threads=16, flags=0x4100),
                   "detect_batch_ex(SCRUB | 0x4100) (%s)" % label)


def test_detect_batch_ex_html(gpu, score_batch):
    label, ref, span, docs, _, _, _ = score_batch
    pages = [b"<p>" + d.replace(b" ", b" <b>x</b> ", 2) + b" &eacute;t&eacute; &#x1F600;</p>" for d in docs[:300]]
    # ... and pages whose lang= attribute holds an ill-formed byte: the scan reads the scrubbed text
    pages += [b"<html lang=\"f\xffr\"><p>" + d + b"</p>" for d in docs[300:330]]
    pages += [b"<html lang=fr\x80><p>" + d + b"</p>" for d in docs[330:360]]
    looped = [ref_scrub(span, p) for p in pages]
    assert 30 < sum(c > 0 for _, c in looped) and sum(c == 0 for _, c in looped) > 30
    lbuf, loffs = gpu.pack([t for t, _ in looped])
    want = ref.detect_batch(lbuf, loffs, plain=np.zeros(len(pages), np.uint8), threads=16)
    assert_results(gpu.detect_batch_ex(pages, html=True, flags=SCRUB), want, "detect_batch_ex(html, SCRUB) (%s)" % label)


def assert_vectors(res, chunks, coffs, want, what):
    wres, wch, wco = want
    assert_results(res, wres, what)
    assert np.array_equal(np.asarray(coffs, np.uint64), wco), what + ": chunk_offsets"
    for f in ("offset", "bytes", "lang1"):
        bad = np.nonzero(chunks[f] != wch[f])[0]
        assert len(bad) == 0, "%s: chunk field %s differs at chunk %d (document %d)" % (
            what, f, bad[0], int(np.searchsorted(wco, bad[0], side="right")) - 1)


def test_detect_batch_vec(gpu, score_batch):
    label, ref, span, docs, lbuf, loffs, changed = score_batch
    res, chunks, coffs = gpu.detect_batch_vec(docs, flags=SCRUB)
    assert_vectors(res, chunks, coffs, ref.detect_batch_vec(lbuf, loffs, threads=16), "detect_batch_vec(SCRUB) (%s)" % label)
    assert int(coffs[-1]) > len(docs)


def test_detect_batch_docflags_with_prefixes(gpu, score_batch):
    """Document 804 of this batch (random bytes, repaired, scored as HTML | ScoreAsQuads) is the
    page on which the parallel span builders first met an undecodable '&' after a single letter
    of another script (tests/test_gpu_html_stale_script.py has that case on its own)."""
    label, ref, span, docs, lbuf, loffs, changed = score_batch
    words = dc.assign_modes(len(docs), seed=72)
    want = dc.reference_rows(ref, lbuf, loffs, words)
    vps = ref_prefixes(span, docs)                                     # of the documents as given
    lens = np.array([len(d) for d in docs])
    assert np.array_equal(vps < lens, changed)
    got, gvp = gpu.detect_batch_docflags(docs, doc_flags=words, flags=SCRUB, valid_prefix=True)
    assert_prefixes(gvp, vps, docs, "detect_batch_docflags(SCRUB) (%s)" % label)
    assert_results(got, want, "detect_batch_docflags(SCRUB, mixed words) (%s)" % label)
    # without the array, and without the words (the forwarded call): the same
    again = gpu.detect_batch_docflags(docs, doc_flags=words, flags=SCRUB)
    assert again.tobytes() == got.tobytes()
    got0, gvp0 = gpu.detect_batch_docflags(docs, flags=SCRUB, valid_prefix=True)
    assert_prefixes(gvp0, vps, docs, "detect_batch_docflags(SCRUB, no words) (%s)" % label)
    assert_results(got0, ref.detect_batch(lbuf, loffs, threads=16), "detect_batch_docflags(SCRUB, no words) (%s)" % label)


def test_device_entries(gpu, score_batch, tmp_path):
    """cld_detect_batch_device_ex and cld_detect_batch_device_vec on torch tensors (the child
    starts on the table set the reference has loaded)."""
    label, ref, span, docs, lbuf, loffs, changed = score_batch
    n_changed = int(changed.sum())
    buf, offs = gpu.pack(docs)
    got = run_child(tmp_path, "score", buf, offs,
                    CLD_MI355X_TABLES=gpu.Q0_TABLES if label == "q0" else os.environ["CLD_MI355X_TABLES"])
    assert_results(got["ex_out"], ref.detect_batch(lbuf, loffs, threads=16), "detect_batch_device_ex(SCRUB)")
    want = ref.detect_batch_vec(lbuf, loffs, threads=16)
    vps = ref_prefixes(span, docs)
    for key in ("vec", "vecnovp"):
        what = "detect_batch_device_vec(SCRUB) (%s)" % key
        assert_vectors(got[key + "_out"], got[key + "_chunks"], got[key + "_coffs"], want, what)
        st = got[key + "_status"][0]
        assert int(st["rejected_docs"]) == n_changed and n_changed > 300, what
        assert int(st["failed_docs"]) == 0 and int(st["total_chunks"]) == int(want[2][-1]), what
    assert_prefixes(got["vec_vp"], vps, docs, "detect_batch_device_vec(SCRUB)")
    assert (got["vecnovp_vp"].view(np.uint8) == 0xA5).all()            # NULL: not wanted, nothing written


# ---------------------------------------------------------------- routing

def test_kernels_route_on_the_repaired_bytes(gpu):
    docs = docs_for(34, 600)
    gpu.detect_batch(docs)
    unflagged = int(gpu.last_stats(0).general_docs)
    flagged_res = gpu.detect_batch(docs, flags=SCRUB)
    flagged = int(gpu.last_stats(0).general_docs)
    scrubbed = [gpu.scrub_utf8_host(d)[0] for d in docs]
    plain_res = gpu.detect_batch(scrubbed)
    assert int(gpu.last_stats(0).general_docs) == flagged
    assert flagged < unflagged                                         # the ill-formed ones left the sequential source
    assert flagged_res.tobytes() == plain_res.tobytes()


def test_clean_batch_is_untouched(gpu):
    buf, offs = corpus.c2(2000)
    out, replaced = gpu.scrub_utf8_batch(buf=buf, offsets=offs)
    assert np.array_equal(out, buf[int(offs[0]):int(offs[-1])]) and not replaced.any()
    assert gpu.detect_batch(buf=buf, offsets=offs, flags=SCRUB).tobytes() == gpu.detect_batch(buf=buf, offsets=offs).tobytes()


def test_detect_language_scrubbed(gpu, ref_tables):
    label, ref = ref_tables
    span = span_valid(ref.lib)
    b2, o2 = corpus.c2(60, seed=35)
    texts = [bytes(b2[o2[i]:o2[i + 1]]) for i in range(60)]
    texts = [(t[:len(t) // 2] + BAD[i % 19] + t[len(t) // 2:]) if i % 2 else t for i, t in enumerate(texts)]   # (BAD[19] is NUL)
    for t in texts:
        assert b"\0" not in t
        want, changed = ref_scrub(span, t)
        lang = int(ref.detect_batch(*gpu.pack([want]))["summary_lang"][0])
        # (detect_language's mapping of UNKNOWN, compact_lang_det.cc:91-93)
        code = "en" if lang == gpu.UNKNOWN_LANGUAGE else gpu.language_code(lang)
        assert gpu.detect_language_scrubbed(t) == (code, changed), t
