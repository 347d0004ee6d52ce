"""k_wave's hit stages at the smallest shapes where they can go wrong: the
octa stage's word ends (taken from the quad stage's word list, the 8-character
cap from two hops of the quad step record), the quad chain around its 64- and
128-entry registers, the base emissions the quad stage writes at the probe
(their count around 64, 128 and the 160-entry capacity, and none at all with
the Q0 table), the repeat filter across the register seam, and the CJK
streams, which write their base emissions through the same helper.

As test_gpu_wave_stages.py: documents of at most 256 bytes, every family once
in batches of at most 1024 documents (run_tiny: k_wave alone) and once as one
larger batch, every field compared with the oracle, and BatchStats.short_docs
equal to what the commit before this stage layout gives on the same seeded
batch, so nothing passes by handing documents on to k_long and the capacity
hand-ons stay where they were.  Needs an MI355X."""
import os

import numpy as np
import pytest

import corpus
from test_gpu_wave_stages import CAP, TINY, _cut, _fit, _words, large, run_plain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1 = "abcdefghijklmnopqrstuvwxyz"
L2 = "àáâãäåæçèéêëìíîïñòóôõöøùúûüýāăąćčďēęěğīłńňőœřśşšťūůűźżž"
L3 = "ḁḃḅḇḉḋḍḏḑḓḕḗḙḛḝḟḡḣḥḧḩḫḭḯḱḳḵḷḹḻḽḿṁṃṅṇṉṋṍṏṑṓṕṗṙṛṝṟṡṣṥṧṩṫṭṯṱṳṵṷṹṻṽṿẁẃẅẇẉẋẍẏẑẓẕạảấầẩẫậắằẳẵặẹẻẽếềểễệỉịọỏốồổỗộớờởỡợụủứừửữựỳỵỷỹ"
WIDTH = {1: L1, 2: L2, 3: L3}


def _letter(rng, width):
    s = WIDTH[width]
    return s[int(rng.integers(0, len(s)))]


def word_ends():
    rng = np.random.default_rng(201)
    docs = []
    fill = _words(rng, "en", 400)

    def place(w, k):
        f = [fill[(k * 7 + i) % 400] for i in range(60)]
        two = fill[(k * 3 + 1) % 400]
        return [w, w + b" " + two, two + b" " + w, two + b" " + w + b" " + fill[(k * 5 + 2) % 400],   # 1, 2, 3 words
                _fit([w] + f), _fit([f[0], w] + f[1:]),                                               # first, second
                _cut(_fit(f, CAP - len(w) - 1) + b" " + w, CAP)]                                      # last

    # synthetic words of 1..12 characters: the 8th and 9th characters take each
    # byte width, the others all one width or a mix
    k = 0
    for n in range(1, 13):
        for w8 in (1, 2, 3):
            for w9 in (1, 2, 3):
                for base in (1, 2, 3, 0):
                    ws = [base or int(rng.integers(1, 4)) for _ in range(n)]
                    if n >= 8:
                        ws[7] = w8
                    if n >= 9:
                        ws[8] = w9
                    if n < 8 and (w8, w9) != (1, 1) and base:
                        continue                       # (the same word again)
                    w = "".join(_letter(rng, x) for x in ws)
                    if k % 5 == 0:
                        w = w.upper()                  # lowered in the span pass, some with another length
                    docs += place(w.encode("utf-8"), k)
                    k += 1
    # vocabulary words (they hit the octa tables) of every character length,
    # 1-, 2- and 3-byte scripts, as they are and grown by one and two letters
    v = corpus.vocab()
    for lang in ("de", "fi", "hu", "cs", "tr", "pl", "ru", "uk", "hi"):
        by_len = {}
        for w in v.get(lang, []):
            by_len.setdefault(len(w.decode("utf-8")), []).append(w)
        for n in sorted(by_len):
            ws = by_len[n]
            for rep in range(3 if n in (7, 8, 9) else 1):
                w = ws[int(rng.integers(0, len(ws)))]
                for grown in (w, w + w[-1:].decode("utf-8", "ignore").encode() if w[-1] < 0x80 else w,
                              w + "é".encode(), w + "ḁx".encode()):
                    others = [ws[int(rng.integers(0, len(ws)))] for _ in range(2)] + _words(rng, lang, 30)
                    docs += [grown, _fit([grown] + others), _fit([others[0], grown] + others[1:]),
                             _cut(_fit(others, CAP - len(grown) - 1) + b" " + grown, CAP)]
    return [d for d in docs if len(d) <= CAP]


def chain_sizes():
    """k words of m ASCII letters over the whole grid that fits.  The chain entry
    count crosses 64 from both sides and reaches 128 from below only: a chain
    step covers at least two bytes (two characters, or a one-letter word and its
    space), so 256 bytes hold at most 128 entries and no document of this
    size can reach quad_hits' n > NB hand-on."""
    rng = np.random.default_rng(202)
    vowels, cons = "aeiou", "bcdfghjklmnpqrstvwxyz"
    docs = []
    for m in range(1, 41):
        for k in range(1, 300):
            if k * (m + 1) - 1 > CAP:
                break
            # random letters; then words that start on vowels (the chain steps one further there)
            docs.append(" ".join("".join(L1[int(i)] for i in rng.integers(0, 26, size=m)) for _ in range(k)).encode())
            if (k + m) % 2 == 0:
                docs.append(" ".join("".join((vowels if (j + i) % 3 else cons)[int(rng.integers(0, 5))]
                                             for j in range(m)) for i in range(k)).encode())
    for k in (63, 64, 65, 127, 128):                     # word counts at the register boundaries
        for m in (1, 2, 3):
            if k * (m + 1) - 1 <= CAP:
                docs.append(" ".join(L1[(i * 7 + m) % 26] * m for i in range(k)).encode())
    return docs


# Two-letter words whose quad hit carries two langprobs in the synthetic Q1
# table, and some that carry one (found with the oracle's trace).  Three
# different words in rotation pass the repeat filter, which compares a hit
# with the last two kept ones only.
TWO_LANGPROBS = ["hq", "ia", "iq"]
ONE_LANGPROB = ["af", "aj", "ak", "av", "ba", "bh", "bo", "br", "ca", "cy", "dk", "eg"]


def capacity_docs():
    """Documents with e base emissions for every e from 40 to 170: e // 2 hits
    of two langprobs and e % 2 of one, three bytes a word.  Past NE = 160 the
    document is handed on; the hit count stays under NB = 128 throughout."""
    docs = []
    for e in range(40, 171):
        ws = [TWO_LANGPROBS[i % 3] for i in range(e // 2)]
        if e % 2:
            ws.insert(len(ws) // 2, ONE_LANGPROB[e % len(ONE_LANGPROB)])
        docs.append(" ".join(ws).encode())
    # the same counts reached with one-langprob hits mixed in: more hits per emission
    for e in range(120, 171):
        n1 = 170 - e                                # 0..50 one-langprob hits
        n2 = (e - n1) // 2
        if n2 < 0 or (n1 + n2) * 3 - 1 > CAP:
            continue
        ws = [TWO_LANGPROBS[i % 3] for i in range(n2)]
        for i in range(n1):
            ws.insert((i * 2 + 1) % (len(ws) + 1), ONE_LANGPROB[i % len(ONE_LANGPROB)])
        docs.append(" ".join(ws).encode())
    return docs


def base_emissions(oracle, doc):
    """Base emissions of a one-span Latin document, from the oracle's trace: the
    quad entries of its linear hit list, less the seed that opens it."""
    _, _, lines = oracle.detect(doc, trace=True)
    return sum(1 for x in lines if ",Q=" in x) - sum(1 for x in lines if x.startswith("linear"))


def emission_counts():
    rng = np.random.default_rng(203)
    v = corpus.vocab()
    docs = capacity_docs()
    for lang in corpus.C2_LANGS:
        ws = _words(rng, lang, 80)
        short = sorted(set(v[lang]), key=lambda w: (len(w), w))[:120]
        rng.shuffle(short)
        for k in range(1, 130):
            for pool in (ws, short):
                if k <= len(pool) and len(b" ".join(pool[:k])) <= CAP:
                    docs.append(b" ".join(pool[:k]))
    return docs


def repeat_seam():
    rng = np.random.default_rng(204)
    v = corpus.vocab()
    short = [w for lang in corpus.C2_LANGS for w in v[lang] if w.isascii() and len(w) == 2]
    three = [w for lang in corpus.C2_LANGS for w in v[lang] if w.isascii() and len(w) == 3]
    assert len(set(short)) >= 8 and len(set(three)) >= 8
    docs = []
    # one chain entry and one word per list entry: the repeat falls on entries 62..66
    for at in range(58, 68):
        for rep in range(6):
            a, b, c = (short[int(i)] for i in rng.integers(0, len(short), size=3))
            t = three[int(rng.integers(0, len(three)))]
            for pat in ([a, a], [a, a, a], [a, b, a, b], [a, b, a], [t, t], [a, b, c, a, b, c], [a, b, b, a]):
                fill = [short[int(i)] for i in rng.integers(0, len(short), size=at)]
                docs.append(_fit(fill + pat + [b, t, c, a]))
    # a repeated quad inside long words: several chain entries per word, the seam mid-word
    for at in range(20, 31):
        for rep in range(4):
            ws = [three[int(i)] for i in rng.integers(0, len(three), size=at)]
            w = "".join(L1[int(i)] for i in rng.integers(0, 26, size=4))
            docs.append(_fit([x for x in ws] + [(w * 6).encode(), (w * 3).encode(), ws[0], ws[1]]))
    return docs


def cjk_streams():
    rng = np.random.default_rng(205)
    pools = corpus.cjk_pools()
    docs = []
    for lang in ("zh", "ja", "ko"):
        pool = pools[lang]
        for n in range(1, 81):
            for rep in range(2):
                chars = [pool[int(i)] for i in rng.integers(0, len(pool), size=n)]
                if rep:
                    chars[n // 2:n // 2] = chars[:2]        # a repeated pair
                t = b"".join(chars)
                docs.append(_cut(t, CAP))
                docs.append(_cut(b" ".join(_words(rng, "en", 1 + n % 5)) + b" " + t, CAP))
                if n % 4 == 0:                              # words of two to six characters
                    parts, i = [], 0
                    while i < len(chars):
                        j = i + int(rng.integers(2, 7))
                        parts.append(b"".join(chars[i:j]))
                        i = j
                    docs.append(_cut(b" ".join(parts), CAP))
    return docs


FAMILIES = {"word_ends": word_ends, "chain_sizes": chain_sizes, "emission_counts": emission_counts,
            "repeat_seam": repeat_seam, "cjk_streams": cjk_streams}

# BatchStats.short_docs (the batches of <= 1024 summed, the one large batch),
# recorded with the parent commit's library on these same seeded batches.
PARENT_SHORT_DOCS = {
    "word_ends": (3144, 3144),
    "chain_sizes": (1246, 1246),
    "emission_counts": (1375, 1375),        # 21 short of the family: the 20 past NE = 160 and one more
    "emission_counts/q0": (1388, 1388),
    "repeat_seam": (464, 1392),
    "cjk_streams": (1080, 1080),
}


def run_family(gpu, oracle, name):
    docs = FAMILIES[name]()
    assert max(len(d) for d in docs) <= CAP and 200 <= len(docs) <= 4000, (name, len(docs))
    small = sum(run_plain(gpu, oracle, docs[a:a + TINY], "%s, batch at %d" % (name, a))
                for a in range(0, len(docs), TINY))
    return small, run_plain(gpu, oracle, large(docs), "%s, large batch" % name)


@pytest.mark.parametrize("name", [n for n in FAMILIES if n != "emission_counts"])
def test_family(gpu, oracle, name):
    got = run_family(gpu, oracle, name)
    print("short_docs %s: %s" % (name, got))
    assert got == PARENT_SHORT_DOCS[name]


def test_emission_counts(gpu, oracle, ref_tables):
    """With the synthetic Q1 table (base emissions up to the capacity) and with
    the product's Q0 table (no base hit at all: the nb <= 0 chunk plan)."""
    label, _ = ref_tables
    key = "emission_counts" if label == "q1" else "emission_counts/q0"
    if label == "q1":
        # the family does reach the counts it is about: every count around the
        # 64- and 128-entry boundaries and from 150 to 170, ten past the capacity
        have = {base_emissions(oracle, d) for d in capacity_docs()}
        want = set(range(60, 69)) | set(range(124, 133)) | set(range(150, 171))
        print("base emissions reached: %d..%d, missing %s" % (min(have), max(have), sorted(want - have)))
        assert want <= have
    from oracle import Oracle
    try:
        if label == "q0":
            oracle = Oracle(os.path.join(ROOT, "language-detector_amd", "data", "cld2_q0.cldt"))
        got = run_family(gpu, oracle, "emission_counts")
    finally:
        Oracle()                                   # the oracle's tables are process-global
    print("short_docs %s: %s" % (key, got))
    assert got == PARENT_SHORT_DOCS[key]
