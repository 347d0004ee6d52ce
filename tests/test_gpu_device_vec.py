"""cld_detect_batch_device_vec: the ResultChunkVector on the device-resident
interface (cld_vec.hip: k_vec_plan, k_vec_finish, the chunk-parallel gather),
with CLD_FLAG_CHECK_UTF8, hints and HTML, against cld_detect_batch_vec on the
same input -- which test_gpu_vector.py pins to the oracle and the reference --
and, for one batch, against the reference's own vectors.  Everything is
compared bit for bit: the result fields, chunk_offsets and the chunks.

The device entry runs in child processes (device_vec_child.py) in which torch
owns the GPU and the buffers; a child leaves its outputs in an .npz file and
the tests here assert on that.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus
import refcld
from test_gpu_check_utf8 import one_bad
from test_gpu_html_hints import random_hints
from test_gpu_parity import EDGE, FIELDS, assert_same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64          # device_vec_child.py: chunks behind d_chunks
PATTERN = 0xA5      #   and the byte they (and every output) are filled with before a call
SCAN_BLOCK = 1024   # cld_strip.hip kScanBlock, the scan's tile
SCAN_COUNTS = (1, 63, 64, 65, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1)
BAD_LEADS = (0xC0, 0xC1, 0xF5, 0xF6, 0xF7)
# paragraphs in scripts that each belong to one language (scored by the script alone), so neighbours never merge
PARAGRAPHS = ["Ελληνικά κείμενο εδώ και τώρα ", "ภาษาไทยข้อความที่นี่ตอนนี้ ", "ქართული ტექსტი აქ და ახლა ",
              "հայերեն տեքստ այստեղ և հիմա "]


def docs_of(buf, offs):
    return [bytes(buf[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]


def many_chunks(k):
    """A document of k short paragraphs in alternating scripts."""
    return "".join(PARAGRAPHS[i % len(PARAGRAPHS)] for i in range(k)).encode()


def scan_batch(tweets, count):
    """count documents; empty ones first, last and (where there is room) in a run of 70."""
    docs = [tweets[i % len(tweets)] for i in range(count)]
    if count >= 63:
        docs[0] = docs[-1] = b""
    if count >= SCAN_BLOCK - 1:
        docs[500:570] = [b""] * 70
    return docs


def check_batch(tweets, pages):
    """Valid documents with ill-formed ones at 0, n - 1, mid-batch and a few more places (none with the
    lead bytes the reference is undefined on)."""
    docs = tweets[:300] + pages[:20] + tweets[300:380]
    n = len(docs)
    for i in (0, n - 1, n // 2, 7, 8, 9, 310, 311):
        d = docs[i] if len(docs[i]) > 4 else b"plain text here"
        docs[i] = one_bad(d, len(d) // 2)
    assert not any(b in BAD_LEADS for d in docs for b in d)
    return docs


@pytest.fixture(scope="module")
def inputs(gpu):
    """Every batch the children run: the first child's calls, the second's, and the host-side
    arguments (hints, html) of the calls that have them."""
    calls, failing, host = {}, {}, {}

    def add(where, key, buf, offs, flags=0, hints=None, **more):
        where[key + "_buf"], where[key + "_offs"], where[key + "_flags"] = buf, offs, np.uint32(flags)
        if hints is not None:
            where[key + "_rec"], where[key + "_text"] = gpu.pack_hints(hints, len(offs) - 1)
        for k, v in more.items():
            where["%s_%s" % (key, k)] = np.uint8(v)
        host[key] = (hints, bool(flags & gpu.FLAG_HTML), flags & ~gpu.FLAG_HTML)

    add(calls, "v0", *corpus.c2(3000))
    c5b, c5o = corpus.c5(300)
    add(calls, "v1", c5b, c5o)
    add(calls, "v2", *corpus.c3(30, boiler_frac=0.5))
    hb, ho = corpus.html(300, seed=12)
    add(calls, "v3", hb, ho, gpu.FLAG_HTML, random_hints(gpu, 300, seed=61))
    add(calls, "v4", *gpu.pack(EDGE))
    rb, ro = corpus.c5(500, seed=15)
    for k, flags in enumerate((0, gpu.FLAG_SCORE_AS_QUADS, gpu.FLAG_BEST_EFFORT)):
        add(calls, "r%d" % k, rb, ro, flags)
    tweets = docs_of(*corpus.c2(700, seed=62))
    for k, count in enumerate(SCAN_COUNTS):
        add(calls, "g%d" % k, *gpu.pack(scan_batch(tweets, count)))
    # documents of hundreds and of more than a thousand chunks among short ones; also the capacity batch
    big = tweets[:40] + [many_chunks(300)] + tweets[40:90] + [b"", many_chunks(1300)] + tweets[90:100]
    add(calls, "b0", *gpu.pack(big), caps=1)
    add(calls, "z0", *gpu.pack([b""] * 200))                              # no document has a chunk
    add(calls, "c0", *gpu.pack(check_batch(tweets, docs_of(c5b, c5o))), gpu.FLAG_CHECK_UTF8)
    add(calls, "s0", *corpus.c2(500, seed=63))
    add(calls, "s1", *corpus.c5(100, seed=64))
    fb, fo = corpus.c5(200, seed=17)
    add(failing, "f0", fb, fo, big=0)
    add(failing, "f1", fb, fo, big=1)
    return calls, failing, host


def run_child(tmp, name, data, **env_more):
    """A child that ends abnormally fails every test that needs it, and nothing else is started."""
    np.savez(tmp / (name + "_in.npz"), **data)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p), **env_more)
    r = subprocess.run([sys.executable, os.path.join(HERE, "device_vec_child.py"), str(tmp / (name + "_in.npz")),
                        str(tmp / (name + "_out.npz"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "device_vec_child.py (%s) ended with %d: %s" % (name, r.returncode, r.stderr[-3000:])
    return np.load(tmp / (name + "_out.npz"))


@pytest.fixture(scope="module")
def child(inputs, tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("device_vec"), "calls", inputs[0])


@pytest.fixture(scope="module")
def host_answers(gpu, inputs):
    """cld_detect_batch_vec per key, computed once."""
    memo = {}

    def get(key, where=0):
        if key not in memo:
            hints, html, flags = inputs[2][key]
            memo[key] = gpu.detect_batch_vec(buf=inputs[where][key + "_buf"], offsets=inputs[where][key + "_offs"],
                                             hints=hints, html=html, flags=flags)
        return memo[key]
    return get


def assert_vectors(got, prefix, want, what, cap=None, pad=True):
    """The child's outputs under prefix against (results, chunks, chunk_offsets); cap: the room the call had;
    pad: the chunks' padding word is compared too (the host entry's is what the kernel wrote)."""
    res, chunks, coffs = want
    total = int(coffs[-1])
    cap = total if cap is None else cap
    assert_same(got[prefix + "out"], res, what)
    assert np.array_equal(got[prefix + "coffs"], coffs), what + ": chunk offsets"
    st = got[prefix + "status"][0]
    assert (int(st["total_chunks"]), int(st["failed_docs"])) == (total, 0), (what, st)
    if prefix + "chunks" in got.files:
        have = got[prefix + "chunks"]
        assert len(have) == cap + GUARD
        k = min(cap, total)
        for f in ("offset", "bytes", "lang1") + (("pad",) if pad else ()):
            assert np.array_equal(have[f][:k], chunks[f][:k]), "%s: chunks, field %s" % (what, f)
        assert (have[k:].view(np.uint8) == PATTERN).all(), what + ": bytes behind the chunks were written"


def assert_device_equals_host(child, host_answers, key, what):
    want = host_answers(key)
    assert_vectors(child, key + "_", want, what)
    # the sizing pass: the same results, offsets and status without a chunk buffer
    assert_vectors(child, key + "_size_", want, what + " (sizing pass)")
    assert child[key + "_status"].tobytes() == child[key + "_size_status"].tobytes()
    return want


@pytest.mark.parametrize("key,what", [("v0", "c2"), ("v1", "c5"), ("v2", "c3 boilerplate"), ("v3", "html with hints"),
                                      ("v4", "edge")])
def test_corpora(child, host_answers, key, what):
    res, chunks, coffs = assert_device_equals_host(child, host_answers, key, what)
    assert int(coffs[-1]) > 0


def test_hints_and_html_change_answers(gpu, child, inputs):
    """(so the comparison of v3 is one of hinted HTML results, not of a path that ignored both)"""
    buf, offs = inputs[0]["v3_buf"], inputs[0]["v3_offs"]
    plain = gpu.detect_batch_vec(buf=buf, offsets=offs)[0]
    no_hints = gpu.detect_batch_vec(buf=buf, offsets=offs, html=True)[0]
    got = child["v3_out"]
    assert (plain["text_bytes"] != got["text_bytes"]).any() and (no_hints["lang3"] != got["lang3"]).any()


def test_matches_reference_directly(gpu, child, inputs):
    ref = refcld.instance(gpu.SYNTH_TABLES)
    refcld.verify_build()
    buf, offs = inputs[0]["r0_buf"], inputs[0]["r0_offs"]
    assert not np.isin(buf, BAD_LEADS).any()
    outs = []
    for k, flags in enumerate((0, gpu.FLAG_SCORE_AS_QUADS, gpu.FLAG_BEST_EFFORT)):
        res, chunks, coffs = ref.detect_batch_vec(buf, offs, threads=16, flags=flags)
        assert_vectors(child, "r%d_" % k, (res, chunks, coffs), "c5 vs the reference, flags %#x" % flags, pad=False)
        outs.append(child["r%d_out" % k])
    assert any((outs[0][f] != outs[2][f]).any() for f in FIELDS)          # the flags reached the kernels


@pytest.mark.parametrize("k", range(len(SCAN_COUNTS)), ids=["n%d" % c for c in SCAN_COUNTS])
def test_scan_and_gather_document_counts(child, host_answers, inputs, k):
    key = "g%d" % k
    offs = inputs[0][key + "_offs"]
    assert len(offs) - 1 == SCAN_COUNTS[k]
    res, chunks, coffs = assert_device_equals_host(child, host_answers, key, "%d documents" % SCAN_COUNTS[k])
    counts = np.diff(coffs.astype(np.int64))
    assert ((counts > 0) == (np.diff(offs.astype(np.int64)) > 0)).all()    # every tweet has a chunk, no empty document
    if SCAN_COUNTS[k] >= 63:
        assert counts[0] == 0 and counts[-1] == 0
    if SCAN_COUNTS[k] >= SCAN_BLOCK - 1:
        assert (counts[500:570] == 0).all()                                # a run longer than a wavefront


def test_long_vectors_and_capacity(child, host_answers):
    want = assert_device_equals_host(child, host_answers, "b0", "long vectors")
    res, chunks, coffs = want
    counts = np.diff(coffs.astype(np.int64))
    assert 256 < counts[40] <= 1024 < counts[92], (counts[40], counts[92])   # the input has the vectors it is meant to
    total = int(coffs[-1])
    assert child["b0_caps"].tolist() == [total, total - 1, 1, 0]
    for cap in (total - 1, 1):
        prefix = "b0_cap%d_" % cap
        assert_vectors(child, prefix, want, "chunk_cap %d of %d" % (cap, total), cap=cap)
        assert child[prefix + "status"].tobytes() == child["b0_status"].tobytes()


def test_no_chunks_at_all(child, host_answers):
    res, chunks, coffs = assert_device_equals_host(child, host_answers, "z0", "empty documents")
    assert int(coffs[-1]) == 0 and len(chunks) == 0
    n0 = child["n0"]                                                       # n == 0: offsets[0] = 0 and a zero status
    assert len(n0) == 24 and not n0.any()


def test_check_utf8(gpu, child, inputs):
    buf, offs = inputs[0]["c0_buf"], inputs[0]["c0_offs"]
    n = len(offs) - 1
    lens = np.diff(offs.astype(np.int64))
    res_c, vp = gpu.detect_batch_checked(buf=buf, offsets=offs)
    want = gpu.detect_batch_vec(buf=buf, offsets=offs, flags=gpu.FLAG_CHECK_UTF8)
    rejected = vp < lens
    assert rejected[0] and rejected[n - 1] and rejected[n // 2] and 8 <= rejected.sum() < n // 4
    assert_same(want[0], res_c, "host: vec(CHECK) vs checked")
    counts = np.diff(want[2].astype(np.int64))
    assert (counts[rejected] == 0).all() and counts[~rejected].sum() > 300
    for prefix in ("c0_", "c0_size_", "c0_novp_"):
        assert_vectors(child, prefix, want, "CHECK_UTF8 " + prefix)
        assert int(child[prefix + "status"]["rejected_docs"][0]) == int(rejected.sum())
        got = child[prefix + "out"][rejected]
        assert (got["summary_lang"] == gpu.UNKNOWN_LANGUAGE).all() and (got["lang3"] == gpu.UNKNOWN_LANGUAGE).all()
        assert not got["text_bytes"].any() and not got["is_reliable"].any() and not got["percent3"].any()
    for prefix in ("c0_", "c0_size_"):
        assert np.array_equal(child[prefix + "vp"], vp), prefix + ": valid prefixes"
    assert "c0_novp_vp" not in child.files
    for key in ("v0", "b0"):                                               # without the flag nothing is counted
        assert int(child[key + "_status"]["rejected_docs"][0]) == 0


def test_two_batches_back_to_back_on_a_stream(child, host_answers):
    for key in ("s0", "s1"):
        assert_vectors(child, key + "_", host_answers(key), key + " on a torch stream")


def test_failed_documents(gpu, inputs, host_answers, tmp_path_factory):
    """One-chunk pool regions (CLD_VEC_POOL_SMALL=1, read once per process: a child of its own): with
    big_regions 0 every document of two chunks and more outgrows its region and comes back failed, the
    rest complete; with big_regions 1 the whole batch is the host's answer."""
    got = run_child(tmp_path_factory.mktemp("device_vec_small"), "small", inputs[1], CLD_VEC_POOL_SMALL="1")
    want = host_answers("f0", where=1)
    res, chunks, coffs = want
    assert_vectors(got, "f1_", want, "big_regions = 1")
    counts = np.diff(coffs.astype(np.int64))
    failed = counts >= 2
    assert failed.sum() >= 10 and (~failed).sum() >= 10
    for prefix in ("f0_", "f0_size_"):
        out, st = got[prefix + "out"], got[prefix + "status"][0]
        kept = np.where(failed, 0, counts)
        assert np.array_equal(np.diff(got[prefix + "coffs"].astype(np.int64)), kept) and got[prefix + "coffs"][0] == 0
        assert (int(st["failed_docs"]), int(st["total_chunks"]), int(st["rejected_docs"])) == (failed.sum(), kept.sum(), 0)
        assert_same(out[~failed], res[~failed], "documents that fit")
        bad = out[failed]
        assert (bad["summary_lang"] == gpu.LANG_FAILED).all() and (bad["lang3"] == gpu.UNKNOWN_LANGUAGE).all()
        assert not bad["percent3"].any() and not bad["normalized3"].any() and not bad["text_bytes"].any()
        assert not bad["is_reliable"].any()
    idx = coffs[:-1].astype(np.int64)[kept == 1]                          # (a document that fit has one chunk or none)
    assert got["f0_chunks"][:kept.sum()].tobytes() == chunks[idx].tobytes()
    assert (got["f0_chunks"][kept.sum():].view(np.uint8) == PATTERN).all()
