"""cld_detect_batch_device_docflags / cld_detect_batch_device_vec_docflags: the
per-document modes on the device-resident interface, where the words stay in
HBM and the ApplyHints kernel turns them into routing bits (cld_hints.hip).
Against the host _docflags entries on the same input, bit for bit, and against
the reference CLD2 itself (docflags_cases.py).

The device entries run in a child process (device_docflags_child.py) in which
torch owns the GPU and the buffers; the child leaves its outputs in an .npz
file and the tests here assert on that.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import docflags_cases as dc
import refcld
from test_gpu_docflags import vector_batch
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64          # device_docflags_child.py: chunks behind d_chunks
PATTERN = 0xA5      #   and the byte every output is filled with before a call
STRAY = 0xFFFFFFFF & ~(dc.HTML | dc.CLD2)             # every bit but CLD_FLAG_HTML / SCORE_AS_QUADS / BEST_EFFORT


@pytest.fixture(scope="module")
def ref(gpu):
    refcld.verify_build()
    return refcld.instance(os.environ["CLD_MI355X_TABLES"])


@pytest.fixture(scope="module")
def inputs(gpu, golden):
    """Every call of the child by key, and per key what the host entry is called with: (docs, words, hints, flags, vec)."""
    calls, host = {}, {}

    def add(key, docs, words, hints=None, flags=0, vec=False, stray=False):
        buf, offs = gpu.pack(docs)
        calls[key + "_buf"], calls[key + "_offs"] = buf, offs
        calls[key + "_flags"], calls[key + "_vec"] = np.uint32(flags), np.uint8(vec)
        if words is not None:
            calls[key + "_words"] = np.asarray(words, np.uint32) | np.uint32(STRAY if stray else 0)
        if hints is not None:
            calls[key + "_rec"], calls[key + "_text"] = gpu.pack_hints(hints, len(docs))
        host[key] = (buf, offs, words, hints, flags, vec)

    cases = {"short": dc.short_documents(golden) + (None,), "staged": dc.staged_documents(golden) + (None,),
             "mix": dc.html_mix(gpu, golden, True)}
    add("d1", *cases["short"])
    add("d3", *cases["staged"])
    add("d5", *cases["mix"])
    add("d5q", *cases["mix"], flags=dc.QUADS)                   # a batch-wide flag under the words
    vd, vw = vector_batch(cases)
    add("v6", vd, vw, vec=True)
    add("h1", cases["short"][0], cases["short"][1], stray=True)
    add("h6", vd, vw, vec=True, stray=True)
    add("s1", *cases["short"])                                   # back to back on one torch stream
    add("s5", *cases["mix"])
    add("s6", vd, vw, vec=True)
    # d_doc_flags NULL: cld_detect_batch_device_hints / cld_detect_batch_device_vec
    add("n5", cases["mix"][0], None, cases["mix"][2], flags=dc.HTML | dc.BEST)
    add("n1", cases["short"][0], None)
    add("n6", vd, None, vec=True, flags=dc.HTML)
    return calls, host


@pytest.fixture(scope="module")
def child(inputs, tmp_path_factory):
    """A child that ends abnormally fails every test of the module, and nothing else is started."""
    tmp = tmp_path_factory.mktemp("device_docflags")
    np.savez(tmp / "in.npz", **inputs[0])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, os.path.join(HERE, "device_docflags_child.py"), str(tmp / "in.npz"),
                        str(tmp / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "device_docflags_child.py ended with %d: %s" % (r.returncode, r.stderr[-3000:])
    return np.load(tmp / "out.npz")


@pytest.fixture(scope="module")
def host_answers(gpu, inputs):
    """The host _docflags entry per key, computed once."""
    memo = {}

    def get(key):
        if key not in memo:
            buf, offs, words, hints, flags, vec = inputs[1][key]
            f = gpu.detect_batch_vec_docflags if vec else gpu.detect_batch_docflags
            memo[key] = f(buf=buf, offsets=offs, hints=hints, doc_flags=words, flags=flags)
        return memo[key]
    return get


def assert_vectors(got, prefix, want, what, with_chunks=True):
    res, chunks, coffs = want
    total = int(coffs[-1])
    assert_same(got[prefix + "out"], res, what)
    assert np.array_equal(got[prefix + "coffs"], coffs), what + ": chunk offsets"
    st = got[prefix + "status"][0]
    assert (int(st["total_chunks"]), int(st["failed_docs"]), int(st["rejected_docs"])) == (total, 0, 0), (what, st)
    if with_chunks:
        have = got[prefix + "chunks"]
        assert len(have) == total + GUARD
        for f in ("offset", "bytes", "lang1"):
            assert np.array_equal(have[f][:total], chunks[f]), "%s: chunks, field %s" % (what, f)
        assert (have[total:].view(np.uint8) == PATTERN).all(), what + ": bytes behind the chunks were written"
    else:
        assert prefix + "chunks" not in got.files


@pytest.mark.parametrize("key,what", [("d1", "short documents"), ("d3", "staged path"), ("d5", "html / plain mix, hints"),
                                      ("d5q", "html / plain mix under CLD_FLAG_SCORE_AS_QUADS")])
def test_device_entry_equals_host_and_reference(gpu, ref, child, inputs, host_answers, key, what):
    buf, offs, words, hints, flags, _ = inputs[1][key]
    want = dc.reference_rows(ref, buf, offs, np.asarray(words) | np.uint32(flags), hints)
    if not flags:
        dc.assert_modes_matter(ref, buf, offs, words, want, hints, what)
    assert_same(child[key + "_out"], host_answers(key), what + ": device entry vs host entry")
    assert_same(child[key + "_out"], want, what)


def test_device_vector_entry_equals_host_and_reference(gpu, ref, child, inputs, host_answers):
    buf, offs, words, _, _, _ = inputs[1]["v6"]
    want = host_answers("v6")
    assert_vectors(child, "v6_", want, "vector mode")
    assert_vectors(child, "v6_size_", want, "vector mode, sizing pass", with_chunks=False)     # chunk_cap 0
    assert child["v6_status"].tobytes() == child["v6_size_status"].tobytes()
    rres, vec = dc.reference_vectors(ref, buf, offs, words)
    assert_same(child["v6_out"], rres, "vector mode vs the reference")
    coffs = child["v6_coffs"].astype(np.int64)
    assert np.array_equal(np.diff(coffs), [len(v) for v in vec])
    for i, v in enumerate(vec):
        have = child["v6_chunks"][coffs[i]:coffs[i + 1]]
        for f in ("offset", "bytes", "lang1"):
            assert np.array_equal(have[f], v[f]), "document %d: chunk field %s" % (i, f)


def test_stray_bits_are_masked(child, inputs):
    """Words with every other bit set -- preparation flags, CLD_FLAG_CHECK_UTF8, the debug bits, unknown
    high bits -- equal the masked words: the kernel keeps the three bits it knows."""
    assert (inputs[0]["h1_words"] & np.uint32(STRAY) == np.uint32(STRAY)).all()
    assert np.array_equal(inputs[0]["h1_words"] & np.uint32(dc.HTML | dc.CLD2), inputs[0]["d1_words"])
    assert child["h1_out"].tobytes() == child["d1_out"].tobytes()
    for k in ("out", "coffs", "chunks", "status", "size_out", "size_coffs", "size_status"):
        assert child["h6_" + k].tobytes() == child["v6_" + k].tobytes(), k


def test_calls_back_to_back_on_a_torch_stream(child, host_answers):
    assert child["s1_out"].tobytes() == child["d1_out"].tobytes()
    assert_same(child["s1_out"], host_answers("s1"), "short documents on a torch stream")
    assert child["s5_out"].tobytes() == child["d5_out"].tobytes()
    assert_vectors(child, "s6_", host_answers("s6"), "vector mode on a torch stream")


def test_null_doc_flags_is_the_existing_entry(gpu, child, inputs):
    for key in ("n1", "n5"):
        assert child[key + "_out"].tobytes() == child[key + "_base_out"].tobytes(), key
    buf, offs, _, hints, flags, _ = inputs[1]["n5"]
    want = gpu.detect_batch_ex(buf=buf, offsets=offs, hints=hints, html=True, flags=flags & dc.CLD2)
    assert_same(child["n5_out"], want, "NULL words, results entry")
    for k in ("out", "coffs", "chunks", "status", "size_out", "size_coffs", "size_status"):
        assert child["n6_" + k].tobytes() == child["n6_base_" + k].tobytes(), k
    buf, offs = inputs[1]["n6"][:2]
    assert_vectors(child, "n6_", gpu.detect_batch_vec(buf=buf, offsets=offs, html=True), "NULL words, vector entry")
