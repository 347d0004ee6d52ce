"""k_wave's two instantiations against each other and the oracle.

A batch with no routing bytes, priors, rewritten pages or stage profile runs
k_wave<.., PLAIN>; anything else the general one.  The families of
test_gpu_wave_stages.py go through both: through detect_batch (plain), and
through detect_batch_docflags with one appended BestEffort document, whose
routing byte makes the runtime hand k_wave a routing array (its result is
dropped).  Every result field of the two must be equal and equal to the
oracle's, and both must finish the same number of documents in k_wave
(BatchStats.short_docs), so neither can pass by handing documents to k_long.
Then a mixed batch (plain, hinted and HTML documents together) and the edges
of k_wave's XCD slice arithmetic.  Needs an MI355X."""
import numpy as np
import pytest

from test_gpu_parity import FIELDS, assert_same
from test_gpu_wave_stages import FAMILIES, TINY, document_level, large, run_plain, window_edges

pytestmark = pytest.mark.gpu

# the appended document of the general runs: k_wave finishes it (one Latin span)
EXTRA = b"the quick brown fox jumps over the lazy dog and runs away into the forest"


def run_general(gpu, docs):
    """docs through the general instantiation: (results of docs, short_docs without the appended document)."""
    buf, offs = gpu.pack(list(docs) + [EXTRA])
    df = np.zeros(len(docs) + 1, dtype=np.uint32)
    df[-1] = gpu.FLAG_BEST_EFFORT
    got = gpu.detect_batch_docflags(buf=buf, offsets=offs, doc_flags=df)
    short = int(gpu.last_stats(0).short_docs)
    # the appended document alone, the same way: what it adds to short_docs
    b1, o1 = gpu.pack([EXTRA])
    gpu.detect_batch_docflags(buf=b1, offsets=o1, doc_flags=df[-1:])
    extra = int(gpu.last_stats(0).short_docs)
    assert extra == 1, "the appended document must be one k_wave finishes"
    return got[:-1], short - extra


def both(gpu, oracle, docs, what):
    buf, offs = gpu.pack(docs)
    ref = oracle.detect_batch(buf, offs, threads=16)
    plain = gpu.detect_batch(buf=buf, offsets=offs)
    short_p = int(gpu.last_stats(0).short_docs)
    general, short_g = run_general(gpu, docs)
    assert_same(plain, ref, what + ", plain")
    assert_same(general, ref, what + ", general")
    for f in FIELDS:
        assert np.array_equal(plain[f], general[f]), "%s: %s differs between the instantiations" % (what, f)
    print("short_docs %s: plain %d general %d of %d" % (what, short_p, short_g, len(docs)))
    assert short_p == short_g, what
    return short_p


@pytest.mark.parametrize("name", [n for n in FAMILIES if n != "small_html"])
def test_family_both_instantiations(gpu, oracle, name):
    docs = FAMILIES[name]()
    step = TINY - 1                      # with the appended document: batches of at most 1024
    for a in range(0, len(docs), step):
        both(gpu, oracle, docs[a:a + step], "%s, batch at %d" % (name, a))
    both(gpu, oracle, large(docs), "%s, large batch" % name)


def test_mixed_batch(gpu, oracle):
    docs = document_level()
    plain = gpu.detect_batch(docs=docs)
    page = (b"<html><head><title>Une page</title></head><body><p>Ceci est une page en fran&ccedil;ais avec "
            b"quelques mots de plus pour la d&eacute;tection de la langue.</p></body></html>")
    hinted = b"confirmar senha e nome de usuario para entrar no sistema"
    n = len(docs)
    hints = [gpu.Hints.make()] * n + [gpu.Hints.make("pt", "br"), gpu.Hints.make()]   # (make(): no hint)
    df = np.zeros(n + 2, dtype=np.uint32)
    df[-1] = gpu.FLAG_HTML
    got = gpu.detect_batch_docflags(docs=docs + [hinted, page], hints=hints, doc_flags=df)
    for f in FIELDS:
        assert np.array_equal(got[f][:n], plain[f]), "mixed batch: %s of the plain documents differs" % f
    buf, offs = gpu.pack(docs)
    assert_same(plain, oracle.detect_batch(buf, offs, threads=16), "mixed batch, plain run")
    assert int(got[n]["summary_lang"]) != gpu.LANG_FAILED and int(got[n + 1]["summary_lang"]) != gpu.LANG_FAILED


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1023, 1024, 1025])
def test_grid_edges(gpu, oracle, n):
    edges = window_edges()
    # a 256-byte document (k_wave's capacity), an empty one and a 257-byte one (k_long's)
    fixed = [(b"abcdefg hijklmn " * 16)[:256], b"", (b"abcdefg hijklmn " * 17)[:257]]
    assert [len(d) for d in fixed] == [256, 0, 257]
    # spread over the batch (a batch of one holds the first only), window_edges() cycled as the rest
    docs = [edges[(5 * k) % len(edges)] for k in range(n)]
    for j, d in enumerate(fixed[:n]):
        docs[(j * n) // 3] = d
    what = "grid edges, n = %d" % n
    short_p = run_plain(gpu, oracle, docs, what)
    buf, offs = gpu.pack(docs)
    general, short_g = run_general(gpu, docs)
    assert_same(general, oracle.detect_batch(buf, offs, threads=16), what + ", general")
    assert short_p == short_g, what
