"""The checked entry points (CLD_FLAG_CHECK_UTF8, cld_detect_batch_checked,
cld_valid_prefix_*, detect_language_checked) against the reference's own
SpanInterchangeValid, DetectLanguageCheckUTF8 and
ExtDetectLanguageSummaryCheckUTF8 (compact_lang_det.cc:44-56, :317-355;
oracle/_ref/librefcld2.so).  With the check in front no scored document holds
an ill-formed byte, so the reference is defined on every byte string and
judges random bytes and the leads C0 / C1 / F5-F7 itself.  Needs an MI355X."""
import ctypes
import os

import numpy as np
import pytest

import corpus
import refcld
from test_gpu_corrupt import corrupt, docs_for
from test_valid_prefix_host import SPAN_VALID, code_point_docs, ref_prefixes, two_byte_docs
from valid_fuzz import FIELDS

pytestmark = pytest.mark.gpu

EXT_CHECKED = ("_ZN4CLD233ExtDetectLanguageSummaryCheckUTF8EPKcibPKNS_8CLDHintsEiPNS_8LanguageEPiPdPSt6vectorINS_"
               "11ResultChunkESaISA_EES7_PbS7_")
DL_CHECKED = "_ZN4CLD223DetectLanguageCheckUTF8EPKcibPbPi"
BASE = "héllo wörld 中文 😀 ".encode() * 40
CHECK = 8
REJECTED = {"lang3": [26, 26, 26], "summary_lang": 26, "percent3": [0, 0, 0], "is_reliable": 0, "text_bytes": 0,
            "normalized3": [0.0, 0.0, 0.0]}


def one_bad(d, p):
    """d with byte p replaced: BF where it was ASCII, 'A' elsewhere."""
    d = bytearray(d)
    d[p] = 0xBF if d[p] < 0x80 else 0x41
    return bytes(d)


def boundary_family(tile):
    cuts = sorted(set(list(range(0, 141)) + [255, 256, 257, 1023, 1024, 1025, tile - 1, tile, tile + 1]))
    docs = []
    for L in cuts:
        cut = BASE[:L]
        docs.append(cut)
        docs += [one_bad(cut, p) for p in range(L)]
    return docs


def span_valid(lib):
    f = getattr(lib, SPAN_VALID)
    f.argtypes = [ctypes.c_char_p, ctypes.c_int]
    f.restype = ctypes.c_int
    return f


@pytest.fixture(scope="module")
def ref_lib():
    refcld.verify_build()
    # (SpanInterchangeValid reads no tables: whichever instance is loaded serves, and none is reloaded here)
    return (refcld._loaded.get("ref") or refcld.instance(os.environ["CLD_MI355X_TABLES"])).lib


@pytest.fixture(scope="module")
def prefix_batch(gpu, ref_lib):
    """Case 1's batch, packed, with the reference's prefixes (computed once)."""
    docs = docs_for(31, 600) + boundary_family(gpu.VALID_TILE) + code_point_docs() + two_byte_docs()
    buf, offs = gpu.pack(docs)
    return docs, buf, offs, ref_prefixes(span_valid(ref_lib), docs)


def assert_prefixes(got, want, docs, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d of %d prefixes differ; first: document %d (%d bytes) got %d, reference %d" % (
        what, len(bad), len(docs), bad[0], len(docs[bad[0]]), got[bad[0]], want[bad[0]])


def test_prefixes_short_and_medium(gpu, prefix_batch):
    docs, buf, offs, want = prefix_batch
    assert_prefixes(gpu.valid_prefix_batch(buf=buf, offsets=offs), want, docs, "valid_prefix_batch")


def long_documents(tile):
    n = 3 << 20                                            # above kLongDocCap (1 MiB), a multiple of the tile
    good = (BASE * (n // len(BASE) + 1))[:n - 8]
    while good[-1] & 0xC0 == 0x80 or good[-1] >= 0xC0:     # end on a character boundary
        good = good[:-1]
    good = good + b"a" * (n - len(good))
    three = one_bad(one_bad(one_bad(good, 5 * tile + 17), 900 * tile + 3), 2000 * tile + 1023)
    docs = [good] + [one_bad(good, p) for p in (0, tile - 1, tile, tile + 1, 2 * tile - 2, n - 1)]
    docs += [good[:-3] + b"\xf0\x9f\x98", three]
    return docs, three


def test_prefixes_long_documents(gpu, ref_lib):
    tile = gpu.VALID_TILE
    longs, three = long_documents(tile)
    b2, o2 = corpus.c2(64, seed=9)
    tweets = [bytes(b2[o2[i]:o2[i + 1]]) for i in range(64)]
    # the long documents start tile-aligned (offset 0); after the tweets and an odd pad, three of them again unaligned
    docs = longs + tweets + [b"abc"] + [longs[3], longs[5], three]
    want = ref_prefixes(span_valid(ref_lib), docs)
    assert want[len(longs) - 1] // tile == 5               # the first of the three errors (three tiles) wins
    buf, offs = gpu.pack(docs)
    assert_prefixes(gpu.valid_prefix_batch(buf=buf, offsets=offs), want, docs, "long documents")


def ref_checked(lib, doc, plain=True, flags=0):
    """The reference's ExtDetectLanguageSummaryCheckUTF8 with default hints and a NULL
    vector -> (valid_prefix, result dict); the result is None where the reference
    returned before scoring (it leaves the other outputs unwritten there)."""
    f = getattr(lib, EXT_CHECKED)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_bool, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    hints = refcld.Hints(None, b"", 23, 26)
    l3 = (ctypes.c_int * 3)()
    p3 = (ctypes.c_int * 3)()
    n3 = (ctypes.c_double * 3)()
    tb, rel, vp = ctypes.c_int(0), ctypes.c_bool(True), ctypes.c_int(-1)
    lang = f(doc, len(doc), plain, ctypes.byref(hints), flags, l3, p3, n3, None, ctypes.byref(tb), ctypes.byref(rel),
             ctypes.byref(vp))
    if vp.value < len(doc):
        assert lang == 26 and not rel.value
        return vp.value, None
    return vp.value, {"lang3": list(l3), "summary_lang": lang, "percent3": list(p3), "is_reliable": int(rel.value),
                      "text_bytes": tb.value, "normalized3": list(n3)}


def expected(gpu, lib, docs, plain=True, flags=0):
    want = np.zeros(len(docs), dtype=gpu.RESULT_DTYPE)
    vps = np.zeros(len(docs), dtype=np.int32)
    for i, d in enumerate(docs):
        vps[i], r = ref_checked(lib, d, plain, flags)
        for f in FIELDS:
            want[f][i] = (REJECTED if r is None else r)[f]
    return want, vps


def assert_results(got, want, what):
    for f in FIELDS:
        bad = np.nonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))[0]
        assert len(bad) == 0, "%s: field %s differs on %d documents; first %d: got %s, want %s" % (
            what, f, len(bad), bad[0], got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def result_batch(gpu, ref_tables):
    """Case 3's batch with the reference's checked results for flags 0 (on the tables in use)."""
    label, ref = ref_tables
    docs = docs_for(32, 600)
    want, vps = expected(gpu, ref.lib, docs)
    return label, ref, docs, want, vps


@pytest.mark.parametrize("flags", [0, 0x100, 0x4000])
def test_checked_results(gpu, result_batch, flags):
    label, ref, docs, want, vps = result_batch
    if flags:
        want, vps = expected(gpu, ref.lib, docs, flags=flags)
    lens = np.array([len(d) for d in docs])
    assert 100 < int(np.sum(vps < lens)) < len(docs) - 100      # both kinds in numbers
    got, gvp = gpu.detect_batch_checked(docs, flags=flags)
    assert_prefixes(gvp, vps, docs, "detect_batch_checked (%s, flags %#x)" % (label, flags))
    assert_results(got, want, "detect_batch_checked (%s, flags %#x)" % (label, flags))


def test_rejected_documents_are_not_scored(gpu, result_batch):
    label, ref, docs, want, vps = result_batch
    valid = [d for d, v in zip(docs, vps) if v == len(d)]
    gpu.detect_batch(valid)
    g0 = int(gpu.last_stats(0).general_docs)
    gpu.detect_batch(docs)
    assert int(gpu.last_stats(0).general_docs) > g0            # unchecked: the malformed ones take the sequential source
    gpu.detect_batch_checked(docs)
    assert int(gpu.last_stats(0).general_docs) == g0


def test_flag_on_detect_batch(gpu, result_batch):
    label, ref, docs, want, vps = result_batch
    assert_results(gpu.detect_batch(docs, flags=CHECK), want, "detect_batch(CHECK) (%s)" % label)
    # with the service's preparation the check applies to the prepared text
    both = gpu.FLAG_STRIP_EXTRAS | gpu.FLAG_CSTRING
    pb, po = gpu.prepare_batch(docs, flags=both)
    assert_results(gpu.detect_batch(docs, flags=CHECK | both), gpu.detect_batch(buf=pb, offsets=po, flags=CHECK),
                   "detect_batch(CHECK | STRIP_EXTRAS | CSTRING) (%s)" % label)


def test_flag_on_detect_batch_vec(gpu, result_batch):
    label, ref, docs, want, vps = result_batch
    docs, vps = docs[:300], vps[:300]
    res, chunks, coffs = gpu.detect_batch_vec(docs, flags=CHECK)
    assert 30 < int(np.sum(vps < np.array([len(d) for d in docs]))) < 270
    for i, d in enumerate(docs):
        have = [(int(c["offset"]), int(c["bytes"]), int(c["lang1"])) for c in chunks[coffs[i]:coffs[i + 1]]]
        if vps[i] < len(d):
            assert have == [], "rejected document %d has a vector" % i
            for f in FIELDS:
                assert np.array_equal(res[i][f], np.asarray(REJECTED[f], dtype=res[i][f].dtype)), (i, f)
            continue
        rb, cb = ref.detect_vec(d)
        assert have == [(int(c["offset"]), int(c["bytes"]), int(c["lang1"])) for c in cb], "vector of document %d" % i
        for f in FIELDS:
            assert np.array_equal(np.asarray(res[i][f], dtype=np.float64), np.asarray(rb[f], dtype=np.float64)), (i, f)


def test_flag_on_detect_batch_ex_html(gpu, result_batch):
    label, ref, docs, _, _ = result_batch
    pages = [b"<p>" + d.replace(b" ", b" <b>x</b> ", 2) + b" &eacute;t&eacute; &#x1F600;</p>" for d in docs[:300]]
    want, vps = expected(gpu, ref.lib, pages, plain=False)
    assert 30 < int(np.sum(vps < np.array([len(p) for p in pages]))) < 270
    assert_results(gpu.detect_batch_ex(pages, html=True, flags=CHECK), want, "detect_batch_ex(html, CHECK) (%s)" % label)
    got, gvp = gpu.detect_batch_checked(pages, html=True)
    assert_prefixes(gvp, vps, pages, "detect_batch_checked(html)")
    assert_results(got, want, "detect_batch_checked(html) (%s)" % label)


DEVICE_ENTRY = """
import sys
import numpy as np
import torch
torch.cuda.set_device(0)                 # torch first: the library then shares its HIP runtime (as in bench.py)
import cld_amd
cld_amd.init_device(0)
buf, offs = np.load(sys.argv[1]), np.load(sys.argv[2])
n = len(offs) - 1
dev = torch.device("cuda", 0)
d_buf = torch.from_numpy(buf).to(dev)
d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
d_vp = torch.full((n,), -7, dtype=torch.int32, device=dev)
cld_amd.valid_prefix_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_vp.data_ptr(), None)
torch.cuda.synchronize()
s = torch.cuda.Stream()
d_vp2 = torch.full((n,), -7, dtype=torch.int32, device=dev)
cld_amd.valid_prefix_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_vp2.data_ptr(), s.cuda_stream)
s.synchronize()
assert torch.equal(d_vp, d_vp2)
cld_amd.valid_prefix_device(0, None, None, 0, None, None)
np.save(sys.argv[3], np.stack([d_vp.cpu().numpy(), cld_amd.valid_prefix_batch(buf=buf, offsets=offs)]))
"""


def test_device_entry_on_torch_tensors(gpu, prefix_batch, tmp_path):
    """cld_valid_prefix_device on torch tensors, in a process of its own where torch
    initialises the GPU first (this one has the library's runtime loaded already)."""
    import subprocess
    import sys
    docs, buf, offs, want = prefix_batch
    np.save(tmp_path / "buf.npy", buf)
    np.save(tmp_path / "offs.npy", offs)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, "-c", DEVICE_ENTRY, str(tmp_path / "buf.npy"), str(tmp_path / "offs.npy"),
                        str(tmp_path / "vp.npy")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    dev_vp, host_vp = np.load(tmp_path / "vp.npy")
    assert_prefixes(dev_vp, host_vp, docs, "valid_prefix_device against the host entry")
    assert_prefixes(dev_vp, want, docs, "valid_prefix_device")


def test_entry_errors(gpu):
    # the prefixes index the documents as given: no preparation flags on the checked entry
    for bad in (gpu.FLAG_STRIP_EXTRAS, gpu.FLAG_CSTRING):
        with pytest.raises(gpu.CldError, match="%d" % gpu.EINVAL):
            gpu.detect_batch_checked([b"some text"], flags=bad)
    res, vp = gpu.detect_batch_checked([])
    assert len(res) == 0 and len(vp) == 0
    assert len(gpu.valid_prefix_batch([])) == 0
    gpu.valid_prefix_device(0, None, None, 0, None, None)
    assert len(gpu.detect_batch([], flags=CHECK)) == 0


def test_detect_language_checked(gpu, ref_tables):
    label, ref = ref_tables
    f = getattr(ref.lib, DL_CHECKED)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_bool, ctypes.c_void_p, ctypes.c_void_p]
    b2, o2 = corpus.c2(200, seed=33)
    rng = np.random.default_rng(33)
    texts = [bytes(b2[o2[i]:o2[i + 1]]) for i in range(200)]
    texts = [corrupt(rng, t) if i % 2 else t for i, t in enumerate(texts)]
    texts = [t.split(b"\0")[0] for t in texts]                 # C strings
    rejected = 0
    for t in texts:
        rel, vp = ctypes.c_bool(True), ctypes.c_int(-1)
        lang = f(t, len(t), True, ctypes.byref(rel), ctypes.byref(vp))
        code, gvp = gpu.detect_language_checked(t)
        assert (code, gvp) == (gpu.language_code(lang), vp.value), t
        rejected += vp.value < len(t)
    assert 20 < rejected < 180
