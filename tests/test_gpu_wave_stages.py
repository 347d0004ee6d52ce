"""k_wave's stages at the smallest shapes where they can go wrong: the fused
span + lowercase pass (window edges, every lowerable code point, several
spans per document, the ent lookahead of rewritten HTML), the hit stages
(word counts around the 64-entry register boundary, long words, repeats),
one to three chunks, and the document level (one language, close pairs,
three languages, unreliable junk, hints and CLD2's flags).

Every family is documents of at most 256 bytes, run once in batches of at
most 1024 documents (run_tiny: k_wave alone) and once as a larger batch
(k_route + k_wave), every field compared with the oracle.  So that no family
can pass by leaving k_wave, the number of documents k_wave finishes
(BatchStats.short_docs) must equal what the commit before the span /
lowercase fusion gives for the same seeded batch.  Needs an MI355X."""
import numpy as np
import pytest

import corpus
from test_gpu_html_hints import priors_for, random_hints
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
CAP = 256
TINY = 1024


def _fit(words, cap=CAP):
    """The longest prefix of words (joined by spaces) of at most cap bytes."""
    out, n = [], 0
    for w in words:
        if n + len(w) + (1 if out else 0) > cap:
            break
        n += len(w) + (1 if out else 0)
        out.append(w)
    return b" ".join(out)


def _cut(b, n):
    """b cut to at most n bytes on a character boundary."""
    while n > 0 and n < len(b) and (b[n] & 0xC0) == 0x80:
        n -= 1
    return b[:n]


def _words(rng, lang, k):
    ws = corpus.vocab()[lang]
    return [ws[int(i)] for i in rng.integers(0, len(ws), size=k)]


def _synth(rng, lo, hi, n):
    """A word of n random code points of [lo, hi)."""
    return "".join(chr(int(c)) for c in rng.integers(lo, hi, size=n)).encode("utf-8")


def window_edges():
    rng = np.random.default_rng(101)
    docs = []
    # vocabulary text cut on a character boundary at every length 0..256
    for lang in ("en", "fr", "cs", "tr", "ru"):
        text = b" ".join(_words(rng, lang, 120))
        docs += [_cut(text, n) for n in range(CAP + 1)]
    # a gap, a 2-byte and a 3-byte letter placed around each 64-byte window edge
    ascii_text = b" ".join(w for w in _words(rng, "en", 200) if w.isascii())
    tokens = [b"12, ", b"3.", b" ", "é".encode(), "É".encode(), "ḁ".encode(), "Ḁ".encode(),
              "д".encode(), "中".encode(), b" 7 ", "éḁ".encode()]
    for edge in (64, 128, 192):
        for at in range(edge - 4, edge + 2):
            for t in tokens:
                for base in (0, 37):
                    docs.append(_cut(ascii_text[base:base + at] + t + ascii_text[base + at:], CAP))
    # a run that ends exactly at byte 64 / 128 / 192 / 256, and a document that ends inside a run
    letters = b"abcdefghijklmnopqrstuvwxyz"
    for edge in (64, 128, 192, 256):
        run = bytes(letters[i % 26] for i in range(edge))
        docs += [run, run[:-1], run[:-1] + b" ", run[:-1] + b"1", (run + b" and more words here")[:CAP],
                 (run + b"1 and more words here")[:CAP], (run[:-2] + "é".encode() + b" tail")[:CAP]]
    return docs


LOWER_RANGES = [(0x41, 0x5B), (0xC0, 0x250), (0x370, 0x400), (0x400, 0x530), (0x1E00, 0x1F00), (0x2100, 0x2150),
                (0xFF21, 0xFF3B)]


def lowering():
    rng = np.random.default_rng(102)
    docs = []
    fill = _words(rng, "en", 64) + _words(rng, "ru", 64)
    k = 0
    for lo, hi in LOWER_RANGES:
        for cp in range(lo, hi):
            ch = chr(cp)
            a, b = fill[k % 128].decode(), fill[(k + 7) % 128].decode()
            k += 1
            docs.append(("%s a%sb %s%s %s%s %s %sx" % (a, ch, ch, ch, ch, b, b, ch)).encode("utf-8"))
    # length-changing lowerings next to window edges
    for ch in ("İ", "ẞ", "K", "Å", "Ω"):
        for n in (20, 30, 31, 62, 63, 64):
            docs.append(_cut(((ch + " ") * n + "and the end").encode("utf-8"), CAP))
            docs.append(_cut(("x" * n + ch + "y " + ch * 40).encode("utf-8"), CAP))
    # 4-byte letters: the unfused span + lowercase pair
    for ch in ("\U00010330", "\U00010400", "\U00010428", "\U0001D400", "\U00020000", "\U0001F600"):
        docs.append(("some words %s%s and %sab more words" % (ch, ch, ch)).encode("utf-8"))
        docs.append(("des mots %s encore" % ch).encode("utf-8") * 3)
    return docs


def several_spans():
    rng = np.random.default_rng(103)
    pools = corpus.cjk_pools()

    def word(script):
        if script == "Latn":
            return _words(rng, "en", 1)[0]
        if script == "Cyrl":
            return _words(rng, "ru", 1)[0]
        if script == "Arab":
            return _words(rng, "ar", 1)[0]
        if script == "Deva":
            return _words(rng, "hi", 1)[0]
        if script == "Grek":
            return _synth(rng, 0x3B1, 0x3CA, int(rng.integers(2, 8)))
        if script == "Geor":
            return _synth(rng, 0x10D0, 0x10F1, int(rng.integers(2, 8)))
        pool = pools["ko" if script == "Hang" else "zh"]
        return b"".join(pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 5))))

    scripts = ["Latn", "Cyrl", "Grek", "Arab", "Deva", "Hang", "Hani", "Geor"]
    docs = []
    for nspans in range(2, 13):
        for rep in range(60):
            seq, prev = [], None
            for _ in range(nspans):
                s = scripts[int(rng.integers(0, len(scripts)))]
                while s == prev:
                    s = scripts[int(rng.integers(0, len(scripts)))]
                seq.append(s)
                prev = s
            if rep % 10 == 0:                       # a scored Latin span, then RTypeNone/One, then CJK
                seq[:3] = ["Latn", "Geor" if rep % 20 else "Grek", "Hani"]
                seq = seq[:max(3, nspans)]
            per = 1 if nspans > 6 else int(rng.integers(1, 4))
            sep = b" " if rep % 3 else b""           # with no separator the scripts touch
            docs.append(_cut(sep.join(b" ".join(word(s) for _ in range(per)) for s in seq), CAP))
    return docs


def word_shapes():
    rng = np.random.default_rng(104)
    L = "abcdefghijklmnopqrstuvwxyz"
    docs = []
    # one-letter words around the 64-entry register boundary; 129 words do not fit k_wave
    for n in (63, 64, 65, 127, 128, 129):
        for rep in range(8):
            docs.append(" ".join(L[int(i)] for i in rng.integers(0, 26, size=n)).encode())
        docs.append(" ".join(L[i % 26] for i in range(n)).encode())
        docs.append(_cut(" ".join("é" if i % 5 == 0 else L[i % 26] for i in range(n)).encode("utf-8"), CAP))
    # words of 5..40 letters: more than four chain entries per word
    for n in range(5, 41):
        for rep in range(4):
            ws = ["".join(L[int(i)] for i in rng.integers(0, 26, size=n)) for _ in range(1 + 200 // n)]
            if rep == 3:
                ws = [w[: n // 2] + "é" + w[n // 2:] for w in ws]
            docs.append(_fit([w.encode("utf-8") for w in ws]))
        docs.append(_fit([w * (1 + n // len(w)) for w in _words(rng, "de", 12)]))
    # repeated words and pairs, placed so the repeat falls on words 60..67
    pats = [["la"] * 3, ["a", "b", "a", "b"], ["a", "b", "a"], ["to", "to"], ["abcd"] * 3, ["le", "la", "le", "la", "le"]]
    for at in range(58, 68):
        for pat in pats:
            for rep in range(2):
                fill = [L[int(rng.integers(0, 26))] + (L[int(rng.integers(0, 26))] if rng.random() < 0.3 else "")
                        for _ in range(at)]
                docs.append(_fit([w.encode() for w in fill + pat + ["x", "yz", "la", "a"]]))
    # the same with vocabulary words, the repeat near the end of the document
    for rep in range(60):
        ws = _words(rng, "fr", int(rng.integers(3, 30)))
        ws += [ws[-1], ws[-1]] if rep % 2 else [ws[-2], ws[-1], ws[-2], ws[-1]] if len(ws) > 1 else ws
        docs.append(_fit(ws))
    return docs


def chunk_counts():
    rng = np.random.default_rng(105)
    docs = []
    for n in range(5, 61):
        for lang in ("en", "fr", "de", "es", "pl", "tr", "ru", "id"):
            ws = sorted(_words(rng, lang, 4 * n), key=len)[:n] if n > 30 else _words(rng, lang, n)
            rng.shuffle(ws)
            docs.append(_fit(ws))
    return docs


def _mix(rng, langs, total):
    ws = []
    for lang in langs:
        ws.append(_fit(_words(rng, lang, 40), total // len(langs) - 1))
    return _fit(ws)


def document_level():
    rng = np.random.default_rng(106)
    docs = []
    b, o = corpus.c2(250, seed=1061)                                   # one language
    docs += [bytes(b[o[i]:o[i + 1]]) for i in range(250)]
    close = [("id", "ms"), ("cs", "sk"), ("hr", "sr"), ("bs", "hr"), ("no", "da"), ("gl", "es"), ("rw", "lg")]
    for i in range(250):                                               # two close languages, half and half
        docs.append(_mix(rng, close[i % len(close)], int(rng.integers(60, CAP + 1))))
    three = ["en", "fr", "de", "ru", "tr", "fi", "hu", "pl", "ar", "hi", "id", "ms", "cs", "sk"]
    for i in range(250):                                               # three languages
        ls = [three[int(k)] for k in rng.choice(len(three), size=3, replace=False)]
        docs.append(_mix(rng, ls, int(rng.integers(90, CAP + 1))))
    b, o = corpus.c2n(250, seed=1062)                                  # shifted junk: unreliable
    docs += [bytes(b[o[i]:o[i + 1]]) for i in range(250)]
    return [_cut(d, CAP) for d in docs]


def small_html():
    rng = np.random.default_rng(107)
    ents = ["&eacute;", "&Eacute;", "&amp;", "&lt;", "&gt;", "&nbsp;", "&#233;", "&#xE9;", "&#1044;", "&#x434;", "&#945;",
            "&#x4e2d;", "&bogus;", "&", "&#65;", "&uuml;", "&#304;", "&#x1F600;", "&ntilde"]
    tags = ["<p>", "</p>", "<b>", "</b>", "<br>", "<i>", "</i>", "<a href='x'>", "</a>"]
    docs = []
    for k in range(700):
        lang = ("fr", "es", "de", "ru", "en", "tr")[k % 6]
        out = []
        for w in _words(rng, lang, int(rng.integers(2, 24))):
            w = w.decode()
            r = rng.random()
            e = ents[int(rng.integers(0, len(ents)))]
            if r < 0.15:
                w = e + w                            # an entity directly before a letter
            elif r < 0.30:
                w = w + e                            # directly after
            elif r < 0.45:
                w = w[:1] + e + w[1:]                # inside a word
            elif r < 0.50:
                w = "α" + e + w                      # a lookahead from another script onto an entity
            elif r < 0.60:
                w = tags[int(rng.integers(0, len(tags)))] + w
            out.append(w)
        docs.append(_cut(" ".join(out).encode("utf-8"), CAP))
    return docs


FAMILIES = {"window_edges": window_edges, "lowering": lowering, "several_spans": several_spans,
            "word_shapes": word_shapes, "chunk_counts": chunk_counts, "document_level": document_level,
            "small_html": small_html}

# BatchStats.short_docs (documents k_wave finished) for (the batches of <= 1024
# summed, the one large batch), recorded with the library of the commit before
# the span / lowercase fusion on these same seeded batches.  What is missing
# from the family's size: empty documents, the 129 one-letter words (257
# bytes), and the documents load_document hands on.
PARENT_SHORT_DOCS = {
    "window_edges": (1702, 1702),
    "lowering": (1308, 1308),
    "several_spans": (659, 1318),
    "word_shapes": (395, 1185),
    "chunk_counts": (446, 1338),
    "document_level": (1000, 2000),
    "small_html": (700, 1400),
}


def large(docs):
    """The family as one batch of more than TINY documents."""
    out = list(docs)
    while len(out) <= TINY:
        out += docs
    return out


def run_plain(gpu, oracle, docs, what, flags=0):
    buf, offs = gpu.pack(docs)
    got = gpu.detect_batch(buf=buf, offsets=offs, flags=flags)
    short = int(gpu.last_stats(0).short_docs)
    if flags:
        ref = oracle.detect_batch_ex(buf, offs, threads=16, flags=flags)
    else:
        ref = oracle.detect_batch(buf, offs, threads=16)
    assert_same(got, ref, what)
    return short


def run_html(gpu, oracle, docs, what):
    buf, offs = gpu.pack(docs)
    n = len(docs)
    got = gpu.detect_batch_ex(buf=buf, offsets=offs, html=True)
    short = int(gpu.last_stats(0).short_docs)
    pr = priors_for(gpu, buf, offs, True, None)
    assert_same(got, oracle.detect_batch_ex(buf, offs, plain=np.zeros(n, np.uint8), priors=pr, threads=16), what)
    return short


def run_family(gpu, oracle, name):
    """(short_docs of the small batches summed, short_docs of the large batch)."""
    docs = FAMILIES[name]()
    assert max(len(d) for d in docs) <= CAP + 1 and 200 <= len(docs) <= 4000
    run = run_html if name == "small_html" else run_plain
    small = sum(run(gpu, oracle, docs[a:a + TINY], "%s, batch at %d" % (name, a)) for a in range(0, len(docs), TINY))
    return small, run(gpu, oracle, large(docs), "%s, large batch" % name)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_family(gpu, oracle, name):
    got = run_family(gpu, oracle, name)
    print("short_docs %s: %s" % (name, got))
    assert got == PARENT_SHORT_DOCS[name]


def test_document_level_hints_and_flags(gpu, oracle):
    docs = document_level()
    buf, offs = gpu.pack(docs)
    n = len(docs)
    hints = random_hints(gpu, n, seed=108)
    got = gpu.detect_batch_ex(buf=buf, offsets=offs, hints=hints)
    pr = priors_for(gpu, buf, offs, False, hints)
    assert_same(got, oracle.detect_batch_ex(buf, offs, priors=pr, threads=16), "document level, hints")
    for flags in (gpu.FLAG_BEST_EFFORT, gpu.FLAG_SCORE_AS_QUADS, gpu.FLAG_BEST_EFFORT | gpu.FLAG_SCORE_AS_QUADS):
        got = gpu.detect_batch_ex(buf=buf, offsets=offs, hints=hints, flags=flags)
        assert_same(got, oracle.detect_batch_ex(buf, offs, priors=pr, threads=16, flags=flags),
                    "document level, hints, flags %#x" % flags)
        for part in (docs[:TINY], large(docs)):
            run_plain(gpu, oracle, part, "document level, flags %#x" % flags, flags=flags)
