"""k_wave's deferred tail: the plain instantiation hands each document's chunks
on as records and k_wtail, one lane per document, makes the chunk summaries,
the DocTote and the document level (cld_wtail.hip).

Every batch below runs twice, each time in a child process (wave_tail_child.py)
because the switches are read once per process: with CLD_WAVE_TAIL=1 (records
and k_wtail) and with CLD_WAVE_TAIL=0 (the tail in the wave), both with
CLD_TINY=0 so that small batches take the same kernels as large ones.  Each
batch is checked against the oracle, the two paths against each other, and
BatchStats.short_docs of the two must agree -- except where a document needs
more records than a slot holds (kTailRecs = 31): the deferred path hands that
one on, which is the point of the case.

Documents come from the vocabularies the stage tests use (test_gpu_wave_stages.py).
Shapes, counted with the oracle's trace where they matter: 1, 2 and the most
chunks a 256-byte Latin span reaches; 31 and 32 records in one document; a
document of more than 256 text bytes whose first pass is not good.  Needs an
MI355X."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cldt
import corpus
from test_gpu_hit_stages import ONE_LANGPROB, TWO_LANGPROBS
from test_gpu_parity import assert_same
from test_gpu_wave_stages import CAP, _cut, _fit, _mix, _words

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TAIL_RECS = 31                      # kTailRecs (cld_kernels.h)
BEST_EFFORT, QUADS = 0x4000, 0x0100


def records(oracle, doc):
    """DocTote::Add calls of the document's first pass (one per scored chunk and
    per unscored span): the records k_wave leaves for it."""
    _, _, lines = oracle.detect(doc, trace=True)
    return next(int(x.split()[0]) for x in lines if x.endswith("chunks scored"))


def recursed(oracle, doc):
    _, _, lines = oracle.detect(doc, trace=True)
    return any(x.startswith("recurse") for x in lines)


def sentences(rng, n):
    langs = corpus.C2_LANGS
    return [_fit(_words(rng, langs[i % len(langs)], int(rng.integers(3, 30)))) for i in range(n)]


def grid_edges(n):
    """n documents for the lane-per-document grid; the last one is unlike its neighbours."""
    rng = np.random.default_rng(300 + n)
    docs = sentences(rng, n)
    docs[-1] = _cut(b" ".join(_words(rng, "ru", 6) + _words(rng, "en", 6) + _words(rng, "hi", 4)), CAP)
    return docs


def chunk_shapes(oracle):
    """One span with one chunk, with two, and at the most chunks a 256-byte Latin
    document reaches; then one-record documents next to the longest ones."""
    rng = np.random.default_rng(311)
    by_count = {}
    for k in range(1, 120):
        for pool in (_words(rng, "en", 120), sorted(set(corpus.vocab()["en"]), key=lambda w: (len(w), w))[:120]):
            d = _fit(pool[:k])
            by_count.setdefault(records(oracle, d), d)
    # two-letter words that each carry a quad hit: 85 of them fill 256 bytes, the
    # most base hits a document of this size collects from words that all hit
    hitting = TWO_LANGPROBS + ONE_LANGPROB
    for k in range(20, 86):
        d = " ".join(hitting[i % len(hitting)] for i in range(k)).encode()
        by_count.setdefault(records(oracle, d), d)
    most = max(by_count)
    print("chunks per one-span Latin document reached: %s" % sorted(by_count))
    # 85 hits make chunks of 20, 20, 20 and 25 (ChunkAll keeps a tail under 30 whole)
    assert 1 in by_count and 2 in by_count and most == 4
    docs = [by_count[c] for c in sorted(by_count)]
    docs += [by_count[1] if i % 2 else by_count[most] for i in range(70)]     # lanes of one wave diverge
    return docs


def alternating(oracle):
    """Latin and Cyrillic words in turn: documents of exactly kTailRecs records and of one more."""
    rng = np.random.default_rng(312)
    lat = [w for w in corpus.vocab()["en"] if 2 <= len(w) <= 3] + [b"ab", b"to"]
    cyr = [w for w in corpus.vocab()["ru"] if len(w) <= 6] + ["да".encode("utf-8"), "он".encode("utf-8")]
    found = {}
    for spans in range(TAIL_RECS - 4, TAIL_RECS + 8):
        for rep in range(8):
            d = b" ".join((lat if i % 2 == 0 else cyr)[int(rng.integers(0, len(lat if i % 2 == 0 else cyr)))]
                          for i in range(spans))
            if len(d) <= CAP:
                found.setdefault(records(oracle, d), d)
    assert TAIL_RECS in found and TAIL_RECS + 1 in found, sorted(found)
    fill = sentences(rng, 6)
    return fill[:3] + [found[TAIL_RECS], found[TAIL_RECS + 1], found[TAIL_RECS]] + fill[3:], 1


def span_scoring(oracle, doc):
    """Per script span of the document's first pass: True where the span was scored
    (it has a hit buffer), False where it went to the DocTote as it stands
    (RTypeNone / RTypeOne)."""
    _, _, lines = oracle.detect(doc, trace=True)
    out = []
    for x in lines:
        if x.startswith("span "):
            out.append(False)
        elif x.startswith("hitbuffer") and out:
            out[-1] = True
        elif x.endswith("chunks scored"):
            break
    return out


def unscored_between(oracle):
    """A span of an RTypeOne / RTypeNone script between two scored spans, the
    middle one shown unscored by the oracle's trace."""
    rng = np.random.default_rng(313)
    docs, mids = [], set()
    for mid in ("γειά σου κόσμε", "ქართული ენა", "ᏣᎳᎩ ᎦᏬᏂᎯᏍᏗ", "ไทย ภาษา"):
        for a, b in (("en", "fr"), ("ru", "en"), ("de", "ru")):
            d = _cut(b" ".join(_words(rng, a, 5)) + b" " + mid.encode("utf-8") + b" " +
                     b" ".join(_words(rng, b, 5)), CAP)
            if span_scoring(oracle, d) == [True, False, True]:
                docs.append(d)
                mids.add(mid)
    print("unscored middle spans: %d documents, %d scripts" % (len(docs), len(mids)))
    assert len(docs) >= 6 and len(mids) >= 2
    return docs


DUMP_LINE = re.compile(r"\[\s*\d+\]\s+(\S+)\s+(-?\d+)B\s+(-?\d+)p\s+(-?\d+)R")
CLDT_CLOSEST_ALT, CLDT_CLOSE_SET = 27, 28             # cldt_format.h


class Totes:
    """The document level's inputs as the oracle's trace shows them (DocTote::Dump,
    before RefineScoredClosePairs), with the close sets and closest alternatives
    of the table blob, to say which branches of the document level a document takes."""

    def __init__(self, oracle):
        blob = cldt.Blob.load(os.environ["CLD_MI355X_TABLES"])
        self.oracle = oracle
        self.close = list(blob.u8(CLDT_CLOSE_SET))
        self.alt = list(blob.u16(CLDT_CLOSEST_ALT))
        self.ids = {oracle.code(i): i for i in range(len(self.close))}

    def slots(self, doc):
        """[language id, bytes, score, reliability] per slot in use, in slot order."""
        _, _, lines = self.oracle.detect(doc, trace=True)
        out, on = [], False
        for x in lines:
            if x.startswith("DocTote::Dump"):
                on = True
            elif on and x.endswith("chunks scored"):
                break
            elif on:
                m = DUMP_LINE.match(x.strip())
                out.append([self.ids[m.group(1)], int(m.group(2)), int(m.group(3)), int(m.group(4))])
        return out

    def close_merges(self, slots):
        """RefineScoredClosePairs on the slots: [(language merged away, language kept)]."""
        merges, gone = [], set()
        for i, s in enumerate(slots):
            cs = self.close[s[0]]
            if cs == 0 or i in gone:
                continue
            for j in range(i + 1, len(slots)):
                if j not in gone and self.close[slots[j][0]] == cs:
                    frm, to = (i, j) if s[1] < slots[j][1] else (j, i)
                    for f in (1, 2, 3):
                        slots[to][f] += slots[frm][f]
                    gone.add(frm)
                    merges.append((slots[frm][0], slots[to][0]))
                    break
        slots[:] = [s for i, s in enumerate(slots) if i not in gone]
        return merges

    def removal(self, doc):
        """What RemoveUnreliableLanguages does to the document's top language:
        "merge" (unreliable, its closest alternative is in the tote), "drop"
        (unreliable, no alternative there), or None."""
        slots = self.slots(doc)
        self.close_merges(slots)
        if not slots:
            return None
        top = max(slots, key=lambda s: s[1])
        if top[1] <= 0 or top[3] // top[1] >= 41:
            return None
        alt = self.alt[top[0]] if top[0] < len(self.alt) else None
        there = any(s[0] == alt and s[1] > 0 for s in slots if s is not top)
        return "merge" if there else "drop"


def close_sets(oracle):
    """Two close-set languages in one document, each the larger one in some
    document (RefineScoredClosePairs merges the smaller into the larger); junk
    text whose top language is unreliable, alone (RemoveUnreliableLanguages
    drops it) and beside words of that language's closest alternative (it
    merges the two).  Which of these a document does is read from the oracle's
    trace, not hoped for."""
    rng = np.random.default_rng(314)
    t = Totes(oracle)
    docs, directions = [], set()
    for a, b in (("id", "ms"), ("cs", "sk"), ("hr", "sr"), ("bs", "hr"), ("no", "da"), ("gl", "es")):
        for share in (0.25, 0.5, 0.75):
            for rep in range(3):
                total = int(rng.integers(100, CAP + 1))
                d = _cut(_fit(_words(rng, a, 40), int(total * share)) + b" " +
                         _fit(_words(rng, b, 40), int(total * (1 - share))), CAP)
                docs.append(d)
                directions |= set(t.close_merges(t.slots(d)))
    both = sorted((x, y) for x, y in directions if x < y and (y, x) in directions)
    print("close pairs merged in both directions: %s" % [(oracle.code(x), oracle.code(y)) for x, y in both])
    assert both
    jb, jo = corpus.c2n(300, seed=3141)
    junk = [bytes(jb[jo[i]:jo[i + 1]]) for i in range(300)]
    vocab = corpus.vocab()
    did = {"merge": 0, "drop": 0}
    for j in junk:
        slots = t.slots(j)
        if t.removal(j) != "drop" or did["drop"] >= 20 and did["merge"] >= 20:
            continue
        top = max(slots, key=lambda s: s[1])[0]
        alt = oracle.code(t.alt[top]) if top < len(t.alt) else None
        if did["drop"] < 20:
            docs.append(j)
            did["drop"] += 1
        # the same junk beside words of its top language's closest alternative,
        # where that is a language of another close set (or the pair would merge first)
        if alt in vocab and (t.close[top] == 0 or t.close[top] != t.close[t.ids[alt]]):
            for k in (2, 3, 4, 6):
                d = _cut(j[:CAP - 60] + b" " + b" ".join(_words(rng, alt, k)), CAP)
                if t.removal(d) == "merge" and did["merge"] < 20:
                    docs.append(d)
                    did["merge"] += 1
                    break
    print("unreliable top language: %s" % did)
    assert did["merge"] >= 1 and did["drop"] >= 1
    return docs


def not_good(oracle):
    """Documents whose lowered text passes 256 bytes (capital I with dot grows when
    lowered) in two or three languages: some are not good after the first pass
    and reach the re-queue list from k_wtail."""
    rng = np.random.default_rng(315)
    docs = []
    for rep in range(40):
        ls = [("tr", "en"), ("tr", "de", "fr"), ("en", "fr", "ru"), ("id", "tr", "pl")][rep % 4]
        d = _cut(_mix(rng, ls, CAP).replace(b"i", "İ".encode("utf-8"), 12), CAP)
        docs.append(d)
    jb, jo = corpus.c2n(400, seed=3151)
    docs += [bytes(jb[jo[i]:jo[i] + CAP]) for i in range(0, 400, 10)]       # junk across tweets, 256 bytes
    docs = [_cut(d, CAP) for d in docs]
    n = sum(recursed(oracle, d) for d in docs)
    print("documents not good after the first pass: %d of %d" % (n, len(docs)))
    assert n >= 1
    return docs


def empties():
    """Empty documents mixed with over-CAP ones and ordinary ones.  No HTML-routed
    document: routing bytes make the batch a general one (enqueue() defers the
    tail only with special == null), so k_wtail never sees such a batch; the
    existing HTML tests cover that instantiation."""
    rng = np.random.default_rng(316)
    s = sentences(rng, 8)
    over = b" ".join(_words(rng, "en", 80))[:CAP + 40]
    return [b"", s[0], b"", b"", over, s[1], b"", s[2], over, b""] + s[3:] + [b""]


@pytest.fixture(scope="module")
def cases(gpu, oracle):
    """key -> (docs, flags, documents only the deferred path hands on)."""
    c = {}
    for n in (1, 63, 64, 65, 129):
        c["grid%03d" % n] = (grid_edges(n), 0, 0)
    c["chunks"] = (chunk_shapes(oracle), 0, 0)
    docs, over = alternating(oracle)
    c["slotcap"] = (docs, 0, over)
    c["unscored"] = (unscored_between(oracle), 0, 0)
    c["close"] = (close_sets(oracle), 0, 0)
    c["notgood"] = (not_good(oracle), 0, 0)
    c["empty"] = (empties(), 0, 0)
    c["close_be"] = (c["close"][0], BEST_EFFORT, 0)
    c["notgood_be"] = (c["notgood"][0], BEST_EFFORT, 0)
    c["unscored_q"] = (c["unscored"][0], QUADS, 0)
    c["close_beq"] = (c["close"][0], BEST_EFFORT | QUADS, 0)
    return c


@pytest.fixture(scope="module")
def runs(gpu, cases, tmp_path_factory):
    """Both children's outputs: {1: deferred tail, 0: tail in the wave}."""
    tmp = tmp_path_factory.mktemp("wave_tail")
    inp = {}
    for key, (docs, flags, _) in cases.items():
        inp[key + "_buf"], inp[key + "_offs"] = gpu.pack(docs)
        inp[key + "_flags"] = np.uint32(flags)
    np.savez(tmp / "in.npz", **inp)
    out = {}
    for tail in (1, 0):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p), CLD_TINY="0",
                   CLD_WAVE_TAIL=str(tail))
        r = subprocess.run([sys.executable, os.path.join(HERE, "wave_tail_child.py"), str(tmp / "in.npz"),
                            str(tmp / ("out%d.npz" % tail))], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "wave_tail_child.py (tail %d) ended with %d: %s" % (tail, r.returncode, r.stderr[-3000:])
        out[tail] = np.load(tmp / ("out%d.npz" % tail))
    return inp, out


KEYS = ["grid001", "grid063", "grid064", "grid065", "grid129", "chunks", "slotcap", "unscored", "close", "notgood",
        "empty", "close_be", "notgood_be", "unscored_q", "close_beq"]


@pytest.mark.parametrize("key", KEYS)
def test_tail(oracle, cases, runs, key):
    inp, out = runs
    docs, flags, over = cases[key]
    buf, offs = inp[key + "_buf"], inp[key + "_offs"]
    ref = oracle.detect_batch_ex(buf, offs, threads=16, flags=flags) if flags else oracle.detect_batch(buf, offs, threads=16)
    assert_same(out[1][key + "_out"], ref, "%s, deferred tail" % key)
    assert_same(out[0][key + "_out"], ref, "%s, tail in the wave" % key)
    assert_same(out[1][key + "_out"], out[0][key + "_out"], "%s, deferred against in-wave" % key)
    s1, s0 = int(out[1][key + "_short"]), int(out[0][key + "_short"])
    print("short_docs %s: deferred %d, in the wave %d of %d" % (key, s1, s0, len(docs)))
    assert s1 == s0 - over
    if key == "slotcap":
        assert s0 == len(docs)                          # the wave itself finishes all of them
    if key in ("notgood", "notgood_be"):
        # exactly the documents the oracle sends to a second pass reached the re-queue list
        assert s0 == len(docs) - sum(recursed(oracle, d) for d in docs) < len(docs)
    if key == "empty":
        assert s0 == len(docs) - 2                      # all but the two over-CAP documents
