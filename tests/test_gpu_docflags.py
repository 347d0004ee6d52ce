"""cld_detect_batch_docflags / cld_detect_batch_vec_docflags: is_plain_text and
CLD2's ScoreAsQuads / BestEffort per document within one batch, on every
scoring path (k_wave, the fused k_long, the staged path with span-parallel
groups, the sequential span source, the HTML rewrite, vector mode), against
the reference CLD2 itself called once per document mode (docflags_cases.py).

Each case first asserts, from the reference alone, that every non-zero mode
changes some document's result: a batch on which the modes do nothing cannot
pass.  Synthetic Q1 tables (the suite's default).  Needs an MI355X."""
import ctypes
import os

import numpy as np
import pytest

import docflags_cases as dc
import refcld
from test_gpu_check_utf8 import REJECTED, one_bad
from test_gpu_parity import FIELDS, assert_same
from test_valid_prefix_host import SPAN_VALID

pytestmark = pytest.mark.gpu
CHECK = 8


@pytest.fixture(scope="module")
def ref(gpu):
    refcld.verify_build()
    return refcld.instance(os.environ["CLD_MI355X_TABLES"])


@pytest.fixture(scope="module")
def cases(gpu, golden):
    """The documents and mode words of cases 1, 3 and 5, which vector mode, the UTF-8 check and the identities draw on."""
    return {"short": dc.short_documents(golden) + (None,), "staged": dc.staged_documents(golden) + (None,),
            "mix": dc.html_mix(gpu, golden, False)}


def run_case(gpu, ref, docs, words, hints, what):
    buf, offs = gpu.pack(docs)
    assert not np.isin(buf, (0xC0, 0xC1, 0xF5, 0xF6, 0xF7)).any()
    want = dc.reference_rows(ref, buf, offs, words, hints)
    dc.assert_modes_matter(ref, buf, offs, words, want, hints, what)
    got = gpu.detect_batch_docflags(buf=buf, offsets=offs, hints=hints, doc_flags=words)
    st = gpu.last_stats(0)
    assert_same(got, want, what)
    return st


def test_short_documents(gpu, ref, cases):
    docs, words, _ = cases["short"]
    assert 450 <= len(docs) <= 550 and max(len(d) for d in docs) <= 256
    st = run_case(gpu, ref, docs, words, None, "short documents")
    assert st.short_docs > len(docs) // 2                  # k_wave's documents


def test_fused_long_kernel(gpu, ref, golden):
    docs, words = dc.fused_pages(golden)
    assert len(docs) == 48 and min(len(d) for d in docs) > 256
    st = run_case(gpu, ref, docs, words, None, "fused k_long")
    assert st.long_docs + st.general_docs == 48


def test_staged_path(gpu, ref, cases):
    docs, words, _ = cases["staged"]
    st = run_case(gpu, ref, docs, words, None, "staged path")
    assert st.long_docs > 64


def test_sequential_span_source(gpu, ref, golden):
    docs, words = dc.sequential_documents(golden)
    st = run_case(gpu, ref, docs, words, None, "sequential span source")
    assert st.general_docs > 0


@pytest.mark.parametrize("with_hints", [False, True], ids=["no_hints", "hints"])
def test_html_and_plain_documents_mixed(gpu, ref, golden, with_hints):
    docs, words, hints = dc.html_mix(gpu, golden, with_hints)
    html = (words & dc.HTML) != 0
    assert 100 < int(html[:300].sum()) < 200 and html[300:].all() and b"" in docs
    run_case(gpu, ref, docs, words, hints, "html / plain mix")
    # the lang= scan runs for the documents flagged HTML, and only for them: with the
    # HTML bit taken from a page whose attribute lies in the window, its prior goes
    buf, offs = gpu.pack(docs)
    plain_words = words & ~np.uint32(dc.HTML)
    got = gpu.detect_batch_docflags(buf=buf, offsets=offs, hints=hints, doc_flags=plain_words)
    assert_same(got, dc.reference_rows(ref, buf, offs, plain_words, hints), "the same documents, all plain")


def vector_batch(cases):
    rng = np.random.default_rng(0xD0C7)
    docs, words = [], []
    for key, k in (("short", 80), ("staged", 60), ("mix", 60)):
        d, w, _ = cases[key]
        for i in np.sort(rng.choice(len(d), size=k, replace=False)):
            docs.append(d[i])
            words.append(w[i])
    return docs, np.array(words, dtype=np.uint32)


def test_vector_mode(gpu, ref, cases):
    docs, words = vector_batch(cases)
    assert len(docs) == 200 and len(np.unique(words)) == 8
    buf, offs = gpu.pack(docs)
    res, chunks, coffs = gpu.detect_batch_vec_docflags(buf=buf, offsets=offs, doc_flags=words)
    want, vec = dc.reference_vectors(ref, buf, offs, words)
    assert_same(res, want, "vector mode")
    counts = np.array([len(v) for v in vec], dtype=np.int64)
    assert np.array_equal(np.diff(coffs.astype(np.int64)), counts) and coffs[0] == 0
    assert counts.sum() > len(docs)
    for i, v in enumerate(vec):
        have = chunks[int(coffs[i]):int(coffs[i + 1])]
        for f in ("offset", "bytes", "lang1"):
            assert np.array_equal(have[f], v[f]), "document %d (mode %#x): chunk field %s" % (i, words[i], f)
    # and the modes reach vector mode: the flags-0 plain vectors differ somewhere
    base, bvec = dc.reference_vectors(ref, buf, offs, np.zeros(len(docs), np.uint32))
    assert dc.differs(want, base).sum() >= 10


def test_check_utf8_with_mixed_doc_flags(gpu, ref, cases):
    docs, words = vector_batch(cases)
    docs = list(docs)
    bad = [3, 4, 17, 81, 95, 140, 141, 160, 199]           # short ones, long ones and pages
    for i in bad:
        assert len(docs[i]) > 4
        docs[i] = one_bad(docs[i], len(docs[i]) // 2)
    buf, offs = gpu.pack(docs)
    assert not np.isin(buf, (0xC0, 0xC1, 0xF5, 0xF6, 0xF7)).any()
    span = getattr(ref.lib, SPAN_VALID)
    span.argtypes, span.restype = [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    vps = np.array([span(d, len(d)) for d in docs], dtype=np.int32)
    lens = np.array([len(d) for d in docs])
    rejected = np.nonzero(vps < lens)[0].tolist()          # (a few C5 documents end inside a character)
    assert set(bad) <= set(rejected) and len(rejected) < 30
    rows = dc.reference_rows(ref, buf, offs, words)
    want = np.zeros(len(docs), dtype=gpu.RESULT_DTYPE)
    for f in FIELDS:
        want[f] = rows[f]
        for i in rejected:
            want[f][i] = REJECTED[f]
    got, gvp = gpu.detect_batch_docflags(buf=buf, offsets=offs, doc_flags=words, flags=CHECK, valid_prefix=True)
    assert np.array_equal(gvp, vps)
    assert_same(got, want, "CHECK_UTF8 with mixed doc_flags")
    # without the prefix array: the same results
    again = gpu.detect_batch_docflags(buf=buf, offsets=offs, doc_flags=words, flags=CHECK)
    assert again.tobytes() == got.tobytes()


def test_identities(gpu, cases):
    """Bitwise, on every result field: all-zero words are cld_detect_batch_ex; uniform words X are
    cld_detect_batch_ex(flags = X); flags = A with words B is words A | B; the debug bits do nothing."""
    docs, words, hints = [], [], None
    for key, k in (("short", 500), ("mix", 413), ("staged", 120)):
        d, w, _ = cases[key]
        docs += d[:k]
        words += list(w[:k])
    words = np.array(words, dtype=np.uint32)
    n = len(docs)
    buf, offs = gpu.pack(docs)
    hints = dc.random_hints(gpu, n, 0xD0C8)
    for h in (None, hints):
        base = gpu.detect_batch_ex(buf=buf, offsets=offs, hints=h)
        assert gpu.detect_batch_docflags(buf=buf, offsets=offs, hints=h, doc_flags=np.zeros(n, np.uint32)).tobytes() == \
            base.tobytes()
        assert gpu.detect_batch_docflags(buf=buf, offsets=offs, hints=h, doc_flags=None).tobytes() == base.tobytes()
    changed = 0
    for x in dc.MODE_WORDS[1:]:
        ex = gpu.detect_batch_ex(buf=buf, offsets=offs, hints=hints, html=bool(x & dc.HTML), flags=int(x & dc.CLD2))
        uni = gpu.detect_batch_docflags(buf=buf, offsets=offs, hints=hints, doc_flags=np.full(n, x, np.uint32))
        assert uni.tobytes() == ex.tobytes(), "uniform words %#x" % x
        changed += ex.tobytes() != base.tobytes()
    assert changed == 7
    mixed = gpu.detect_batch_docflags(buf=buf, offsets=offs, hints=hints, doc_flags=words)
    assert mixed.tobytes() != base.tobytes()
    for a in (dc.HTML, dc.QUADS, dc.BEST | dc.HTML, dc.QUADS | dc.BEST):
        one = gpu.detect_batch_docflags(buf=buf, offsets=offs, hints=hints, doc_flags=words, flags=a)
        two = gpu.detect_batch_docflags(buf=buf, offsets=offs, hints=hints, doc_flags=words | np.uint32(a))
        assert one.tobytes() == two.tobytes(), "flags %#x" % a
    noisy = words | np.uint32(0x3E00)                      # CLD_FLAG_DEBUG_MASK: accepted and ignored
    assert gpu.detect_batch_docflags(buf=buf, offsets=offs, hints=hints, doc_flags=noisy).tobytes() == mixed.tobytes()
    # vector mode: all-zero words and no words are cld_detect_batch_vec
    v0 = gpu.detect_batch_vec(buf=buf, offsets=offs, hints=hints)
    for df in (None, np.zeros(n, np.uint32)):
        v1 = gpu.detect_batch_vec_docflags(buf=buf, offsets=offs, hints=hints, doc_flags=df)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(v0, v1))
