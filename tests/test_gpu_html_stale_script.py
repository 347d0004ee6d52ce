"""HTML mode: an undecodable '&' right after a single letter of another script.

The reference's letters loop (getonescriptspan.cc:876-931) lets one letter of
another script through when the next byte is Common, and a raw '&' is.  If the
'&' then decodes to nothing, the loop meets it with that letter's script still
in hand, and the script of the letter after the '&' decides whether the span
breaks there -- "ҪΪ&r" is two spans, " ҫϊ " and " r ", 9 bytes, where the
rewritten page "ҪΪr" alone would be one of 7.  The parallel span builders hand
such pages to the sequential span source.  Judge: the reference
(oracle/_ref/librefcld2.so) on the same pages, which are valid UTF-8, results
and chunk vectors.  Needs an MI355X."""
import itertools
import os

import numpy as np
import pytest

import refcld
from test_gpu_check_utf8 import assert_results

pytestmark = pytest.mark.gpu

# one letter each: Cyrillic, Greek, Latin, Armenian, Georgian, and a combining mark (Inherited)
LETTERS = ["Ҫ", "Ϊ", "r", "Ք", "ქ", "́"]
AMPS = ["&", "&&", "&zz;", "&#;", "& "]                  # undecodable, each dropped byte by byte or in part
TAILS = ["", "x", " ", "й", "&amp;", "<b>"]


def pages():
    out = [b"\xd2\xaa\xce\xaa&r"]                          # the page the scrub tests met
    for a, b, c in itertools.product(LETTERS[:5], LETTERS, LETTERS):
        for amp, tail in itertools.product(AMPS, TAILS):
            out.append((a + b + amp + c + tail).encode())
    # the same in pages of the long-document kernels: the span's own text in front and behind
    front = {"Ҫ": "қазақ тілі мен әдебиеті туралы мәтін ", "Ϊ": "ελληνικά κείμενο εδώ και τώρα ", "r": "plain english words here ",
             "Ք": "հայերեն տեքստ այստեղ և հիմա ", "ქ": "ქართული ტექსტი აქ და ახლა "}
    for a, b, c in itertools.product(LETTERS[:5], LETTERS[:5], LETTERS):
        for amp in AMPS[:3]:
            out.append((front[a] * 12 + a + b + amp + c + " " + front[a] * 3).encode())
    return out


@pytest.fixture(scope="module")
def batch(gpu):
    refcld.verify_build()
    ref = refcld.instance(os.environ["CLD_MI355X_TABLES"])
    docs = pages()
    buf, offs = gpu.pack(docs)
    assert sum(len(d) <= 256 for d in docs) > 5000 and sum(len(d) > 256 for d in docs) > 400
    return ref, docs, buf, offs


def test_results(gpu, batch):
    ref, docs, buf, offs = batch
    want = ref.detect_batch(buf, offs, plain=np.zeros(len(docs), np.uint8), threads=16)
    assert int(want["text_bytes"][0]) == 9
    assert_results(gpu.detect_batch_ex(buf=buf, offsets=offs, html=True), want, "html pages")
    assert_results(gpu.detect_batch_ex(buf=buf, offsets=offs, html=True, flags=0x100),
                   ref.detect_batch(buf, offs, plain=np.zeros(len(docs), np.uint8), threads=16, flags=0x100),
                   "html pages, ScoreAsQuads")


def test_vectors(gpu, batch):
    ref, docs, buf, offs = batch
    res, chunks, coffs = gpu.detect_batch_vec(buf=buf, offsets=offs, html=True)
    wres, wch, wco = ref.detect_batch_vec(buf, offs, plain=np.zeros(len(docs), np.uint8), threads=16)
    assert_results(res, wres, "html pages, vector mode")
    assert np.array_equal(np.asarray(coffs, np.uint64), wco)
    for f in ("offset", "bytes", "lang1"):
        bad = np.nonzero(chunks[f] != wch[f])[0]
        assert len(bad) == 0, "chunk field %s differs at chunk %d (page %r)" % (
            f, bad[0], docs[int(np.searchsorted(wco, bad[0], side="right")) - 1])
