"""k_wave's lane bits and the quad stage's class bytes at the smallest shapes
where they can go wrong.

The quad stage classifies every byte of the lowered span once (advance, space
or vowel, space) and makes GetQuadHits' step for every position from those
classes, 64 positions a window; the span pass and the hit stages take a lane's
bit of a wave-uniform mask by inverse ballot.  The families below put what a
step reads on either side of a window seam of the lowered text (positions
63/64/65, 127/128/129: a document that starts with a letter has its byte i at
lowered position i + 1 while every character keeps its length), at the end of
the text, and put span starts, breaks and ends on the first and last lanes of
a window of the document.

Every family is documents of at most 256 bytes, run in batches of at most
1024 (k_wave alone) and as one larger batch (k_route + k_wave), through the
plain and the general instantiation (test_gpu_wave_plain.both): every field
equal to the oracle and to each other.  BatchStats.short_docs must equal what
the commit before this change gives for the same seeded batches, so nothing
passes by handing documents to k_long.  Needs an MI355X."""
import itertools
import re

import numpy as np
import pytest

import cldt
import corpus
from test_gpu_html_hints import priors_for
from test_gpu_parity import assert_same
from test_gpu_wave_plain import both
from test_gpu_wave_stages import CAP, TINY, _cut, _fit, _words, large

pytestmark = pytest.mark.gpu

E2, E3 = "é", "ḁ"                       # a 2-byte and a 3-byte Latin letter (both lower to themselves)
SEAMS = (64, 128, 192)


def _filler(rng, n=400):
    """ASCII lower-case words, at least n bytes."""
    out = b""
    while len(out) < n:
        out += b" ".join(w for w in _words(rng, "en", 40) if w.isascii() and w.islower()) + b" "
    return out


def step_seams():
    """Words, quads and vowel skips over the seams of the lowered text: a
    token of 1-, 2- and 3-byte letters (consonant runs, vowel runs, mixed)
    placed at every offset from 6 before to 3 after each seam, so each of its
    characters -- a 3-byte one included -- is cut by the seam at some offset."""
    rng = np.random.default_rng(201)
    fill = _filler(rng)
    tokens = ["strngth", "aeiouae", "b" + E2 + "c" + E3 + "d", E3 * 5, E2 * 6, "a" + E3 + "e" + E2 + "i" + E3,
              "q " + E3 + " r", "x" + E3, E3 + "x y", "bcd" + E2 + "fgh" + E3 + "jkl", "ab cd ef gh", "o u i"]
    docs = []
    for seam in SEAMS:
        for at in range(seam - 7, seam + 3):          # (lowered position at + 1)
            for t in tokens:
                for base in (0, 11):
                    head = fill[base:base + at]
                    docs.append(_cut(head + t.encode("utf-8") + b" " + fill[base + at:], CAP))
    return docs


def limit_edges():
    """The end of the text: every last word of up to five letters over a
    consonant, a vowel, a 2-byte and a 3-byte letter, so a quad's fourth
    character, or its second plus the vowel step, lands on the end offset, one
    before it and in the padding; then texts that end at a multiple of 64 and a
    byte either side."""
    rng = np.random.default_rng(202)
    fill = _filler(rng)
    docs = []
    alphabet = ["b", "a", E2, E3]
    for n in range(1, 6):
        for w in itertools.product(alphabet, repeat=n):
            word = "".join(w).encode("utf-8")
            docs.append(b"xyz " + word)
            if n >= 4:
                docs.append(b"the end " + word + b".")
    tails = ["b", "a", "ab", "ba", "abc", "bcda", "abcde", E3, "a" + E3, E3 + E2 + "b", "bcdfgh"]
    for end in (64, 128, 192, 256):
        for total in range(end - 3, min(end + 3, CAP + 1)):   # the document's length; the text ends one further
            for t in tails:
                tb = t.encode("utf-8")
                for base in (0, 5):
                    head = fill[base:base + total - len(tb) - 1]
                    docs.append(head + b" " + tb)
    return docs


def single_letters():
    """One-letter words: at a window's first and last lane (the offset moves
    them over the seam), and runs of them, so the list of spaces fills to
    around 64 and 128 entries."""
    rng = np.random.default_rng(203)
    L = "abcdefghijklmnopqrstuvwxyz"
    docs = []
    for n in (61, 62, 63, 64, 65, 66, 124, 125, 126, 127, 128):
        for lead in ("", "x", "xy", "xyz"):
            ws = [L[int(i)] for i in rng.integers(0, 26, size=n)]
            if lead:
                ws[0] = lead
            d = " ".join(ws).encode()
            if len(d) <= CAP:
                docs.append(d)
        # 2- and 3-byte one-character words among them
        ws = [E2 if i % 7 == 3 else E3 if i % 11 == 5 else L[i % 26] for i in range(n)]
        docs.append(_cut(" ".join(ws).encode("utf-8"), CAP))
    # a one-byte word first and last in each window, longer words between
    fill = _filler(rng)
    for seam in SEAMS:
        for at in range(seam - 4, seam + 3):
            for base in (0, 7):
                docs.append(_cut(fill[base:base + at] + b" a b " + fill[base + at:], CAP))
                docs.append(_cut(fill[base:base + at] + (" %s a %s " % (E3, E2)).encode("utf-8") + fill[base + at:], CAP))
    return docs


def lane_bits():
    """Span starts, breaks (a Common character) and ends (a letter of another
    script) on lanes 0, 1, 62 and 63 of each window of the document; a
    separator next to a kept character; two spans in one window; a document
    that ends inside a run on lane 63."""
    rng = np.random.default_rng(204)
    text = _filler(rng)
    cyr = " ".join(w.decode() for w in _words(rng, "ru", 30)).encode("utf-8")
    lanes = sorted({64 * w + l for w in range(4) for l in (0, 1, 62, 63)})
    docs = []
    for q in lanes:
        # (ordinary words, so that k_wave finishes the document; a letter on either side of byte q)
        base = next(b for b in range(40)
                    if q == 0 or (text[b + q - 1:b + q + 1].isalpha() and text[b + q - 2:b + q - 1].isalpha()))
        fill = text[base:]
        # the span starts at byte q, after digits and spaces
        docs.append(_cut(b"1" * q + fill[:40] + b" " + fill[40:90], CAP))
        docs.append(_cut((b"12 " * 90)[:q] + fill, CAP))
        # (k_wave's span pass reads the document's own bytes, 64 a window: byte q is lane q % 64)
        assert q == 0 or fill[q - 1:q + 1].isalpha()
        assert docs[-2][q:q + 1].isalpha() and docs[-1][q:q + 1].isalpha()
        assert q == 0 or not (docs[-2][q - 1:q].isalpha() or docs[-1][q - 1:q].isalpha())
        for brk in (b"1", b",", b" ", b", ", b"12"):
            # a break at byte q, inside a run
            docs.append(_cut(fill[:q] + brk + fill[q:], CAP))
            assert docs[-1][q:q + 1] == brk[:1] and (q + len(brk) >= CAP or docs[-1][q + len(brk):q + len(brk) + 1].isalpha())
        for other in ("д", "дом", "α"):
            # the span ends at byte q: another script's letter stop; the Latin text after it is a third span
            o = other.encode("utf-8")
            docs.append(_cut(fill[:q] + o + fill[q:q + 20], CAP))
            assert docs[-1][q:q + 2] == o[:2] or q + 2 > CAP      # (cut at the capacity: the span ends with the document)
            docs.append(_cut(fill[:q] + b" " + o + b" " + cyr, CAP))
            docs.append(_cut(fill[:q] + b"1" + o + fill[q:], CAP))
    for end in (64, 128, 192, 256):
        for base in range(0, 12, 3):                   # (the last byte a letter: the document ends inside a run)
            docs += [text[base:base + end - 1] + b"z", text[base:base + end - 2] + E2.encode("utf-8")]
            assert len(docs[-1]) == len(docs[-2]) == end   # (the last byte on lane 63)
    # short spans in turn: several starts and ends in one window
    for k in range(40):
        parts = []
        for j in range(int(rng.integers(2, 9))):
            ws = _words(rng, "ru" if (j + k) % 2 else "en", int(rng.integers(1, 4)))
            parts.append(b" ".join(ws))
        docs.append(_cut((b" " if k % 2 else b"").join(parts), CAP))
    return docs


SEAM_WORDS = 70                          # words of a hit_registers document: one chain entry each


def _short_words():
    """ASCII lower-case vocabulary words of (two, three) letters: one quad chain entry each."""
    ws = {w for v in corpus.vocab().values() for w in v if 2 <= len(w) <= 3 and w.isascii() and w.islower()}
    return sorted(w for w in ws if len(w) == 2), sorted(w for w in ws if len(w) == 3)


def hit_registers():
    """Hit and word registers at their 64-entry seam.  Every document is
    SEAM_WORDS vocabulary words of two or three letters, so word i is chain
    entry i and entry 64 opens the second register of both the quad chain and
    the word list; all different but for a repeat (a a, a a a, a b a b, a b a)
    that starts at word 60..65, so it lies before, across and after the seam.
    test_hit_register_shapes checks on the oracle's hits that the kept bits
    and the dropped repeats are where this says."""
    rng = np.random.default_rng(205)
    two, three = _short_words()
    docs = []
    for at in range(60, 66):
        for pat in ([0, 0], [0, 0, 0], [0, 1, 0, 1], [0, 1, 0]):
            for rep in range(3):
                # 30 words of two letters and 42 of three, all different, in random order: at most 256 bytes
                ws = [two[int(i)] for i in rng.permutation(len(two))[:30]]
                ws += [three[int(i)] for i in rng.permutation(len(three))[:SEAM_WORDS + 2 - 30]]
                ws = [ws[int(i)] for i in rng.permutation(len(ws))]
                a, ws = sorted(ws[:2], key=len), ws[2:]
                ws[at:at + len(pat)] = [a[k] for k in pat]
                assert len(ws) == SEAM_WORDS and len(set(ws)) == SEAM_WORDS - len(pat) + len(set(pat))
                docs.append(b" ".join(ws))
                assert len(docs[-1]) <= CAP
    for lang in sorted(corpus.vocab()):
        for n in (6, 20, 45):
            docs.append(_fit(_words(rng, lang, n)))
    return docs


FAMILIES = {"step_seams": step_seams, "limit_edges": limit_edges, "single_letters": single_letters,
            "lane_bits": lane_bits, "hit_registers": hit_registers}

# BatchStats.short_docs of the plain instantiation for (the batches of at most
# 1023 summed, the one large batch), recorded with the library of the commit
# before this change on these same seeded batches, in the GPU call that ran
# this file on the new library.
PARENT_SHORT_DOCS = {
    "step_seams": (720, 1440),
    "limit_edges": (3128, 3128),
    "single_letters": (129, 1032),
    "lane_bits": (328, 1312),
    "hit_registers": (283, 1132),
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_family(gpu, oracle, name):
    docs = FAMILIES[name]()
    assert max(len(d) for d in docs) <= CAP and 100 <= len(docs) <= 4000
    step = TINY - 1                      # with both()'s appended document: batches of at most 1024
    small = sum(both(gpu, oracle, docs[a:a + step], "%s, batch at %d" % (name, a)) for a in range(0, len(docs), step))
    got = (small, both(gpu, oracle, large(docs), "%s, large batch" % name))
    print("short_docs %s: %s of %d" % (name, got, len(docs)))
    assert got == PARENT_SHORT_DOCS[name]


def _trace(oracle, doc):
    """The oracle's trace of one plain document: (offsets of the kept base
    hits, one set of key groups (key >> 2) per chunk over the chunk's linear
    langprobs, the seed included)."""
    _, _, lines = oracle.detect(doc, trace=True)
    hits, linear, starts, mode = [], [], [], None
    for ln in lines:
        m = re.match(r"Q\[\d+\](\d+),", ln)
        if m:
            hits.append(int(m.group(1)))
        if ln.startswith("linear "):
            mode = "linear"
        elif ln.startswith("chunkstart "):
            mode = "starts"
        elif ln.startswith("summary "):
            mode = None
        elif mode == "linear":
            m = re.match(r"\[\d+\]\d+,[A-Za-z]=([0-9a-f]{8})$", ln)
            if m:
                linear.append(int(m.group(1), 16))
        elif mode == "starts":
            m = re.match(r"\[\d+\](\d+)$", ln)
            if m:
                starts.append(int(m.group(1)))
    groups = []
    for a, b in zip(starts, starts[1:]):
        groups.append({k >> 2 for lp in linear[a:b] for k in ((lp >> 8) & 255, (lp >> 16) & 255, lp >> 24) if k})
    return hits, groups


def test_hit_register_shapes(oracle):
    """The seam documents of hit_registers() are what its docstring says, on
    the oracle's kept hits: word i is chain entry i (one quad a word), every
    first occurrence is a kept hit -- so registers 0 and 1 have kept bits on
    lanes 0 and 63 and on lanes 0..5 -- and of a repeat exactly the words that
    equal one of the last two kept ones are dropped, on either side of entry 64."""
    docs = hit_registers()[:6 * 4 * 3]
    seen = set()
    for d in docs:
        ws = d.split(b" ")
        assert len(ws) == SEAM_WORDS and all(len(cldt.word_quads(w)) == 1 for w in ws)
        offs = np.cumsum([1] + [len(w) + 1 for w in ws])[:-1]          # (the span text opens with a space)
        hits, _ = _trace(oracle, d)
        kept = [i for i, o in enumerate(offs) if int(o) in hits]
        assert len(kept) == len(hits)
        want, last2 = [], []
        for i, w in enumerate(ws):
            if w in last2:
                continue
            want.append(i)
            last2 = (last2 + [w])[-2:]
        assert kept == want, d
        assert {0, 63, 64}.issubset(kept) or 63 not in want or 64 not in want
        dropped = sorted(set(range(SEAM_WORDS)) - set(kept))
        assert dropped and 60 <= dropped[0] <= 69
        seen |= set(dropped)
        seen.add(("kept", 63 in kept, 64 in kept))
    # repeats dropped on lanes 62, 63 of the first register and 0, 1 of the second; documents that keep both seam lanes
    assert {62, 63, 64, 65}.issubset(seen) and ("kept", True, True) in seen and ("kept", True, False) in seen


GROUP63 = ("zzp", "zzh", "tlh", "zze")     # the Latin per-script numbers 252..255: key group 63


def key_group_docs(oracle):
    """Documents whose every chunk has only key group 0 in use (per-script
    numbers 1-3: en, da, nl; the Latin seed is en): words of those vocabularies
    alone and two to six together, kept when the oracle's linear langprobs say so.  No langprob
    of the scoring tables has a key above 251, so group 63 comes in by a
    language hint alone: its prior boost is one langprob of key 252..255."""
    rng = np.random.default_rng(206)

    def only_group_0(d):
        _, groups = _trace(oracle, d)
        return bool(groups) and all(g == {0} for g in groups)

    v = corpus.vocab()
    singles = [w for w in sorted(set(v["en"]) | set(v["da"]) | set(v["nl"])) if only_group_0(w)]
    docs = list(singles)
    for k in range(300):                     # two to six of those words: their pairs and octagrams must stay in the group too
        d = _fit([singles[int(i)] for i in rng.integers(0, len(singles), size=2 + k % 5)])
        if d not in docs and only_group_0(d):
            docs.append(d)
    return docs


# (documents key_group_docs keeps, short_docs of the hinted batch, of the plain batches summed, of the large plain batch)
KEY_GROUPS_PARENT = (426, 426, 426, 1278)


def test_key_groups_0_and_63(gpu, oracle):
    """Chunks whose in-use key groups are exactly 0 and 63: score_round's
    lane_bit(gm) with the first and the last lane set and the lanes between
    idle.  Only the general instantiation can get there (a hint makes the
    prior); the plain one runs the same documents with group 0 alone."""
    docs = key_group_docs(oracle)
    ids = [i for i in range(512) if oracle.code(i) in GROUP63]
    assert len(ids) == 4 and len(docs) >= 40
    buf, offs = gpu.pack(docs)
    hints = [gpu.Hints.make(language=ids[i % 4]) for i in range(len(docs))]
    pr = priors_for(gpu, buf, offs, False, hints)
    # the prior boosts: one Latin langprob whose only key is in group 63, nothing else
    assert all(((int(p[0]) >> 8) & 255) >> 2 == 63 and int(p[0]) >> 16 == 0 and not p[1:].any() for p in pr)
    got = gpu.detect_batch_ex(buf=buf, offsets=offs, hints=hints)
    short_h = int(gpu.last_stats(0).short_docs)
    assert_same(got, oracle.detect_batch_ex(buf, offs, priors=pr, threads=16), "key groups 0 and 63, hinted")
    small = both(gpu, oracle, docs, "key group 0")
    res = (len(docs), short_h, small, both(gpu, oracle, large(docs), "key group 0, large batch"))
    print("short_docs key_groups: %s" % (res,))
    assert res == KEY_GROUPS_PARENT
