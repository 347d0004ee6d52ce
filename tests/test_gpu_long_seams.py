"""The long-document path at the smallest shapes where its seams can go wrong:
the routing thresholds of k_lspan, the group seams of span-parallel documents
and the boost-ring lookback that rebuilds a group's entering rings, the 2 KB
and 6 KB text windows, and the 1000-hit rounds.

Every family is seeded documents of 257 bytes to about 48 KB built from
corpus.vocab(), in batches of a few hundred documents at most, run in two
forms: staged (more than 64 long documents in the batch, padded with one-span
300-byte filler: k_lspan / k_lscore / k_lgroup / k_lfinish / k_lrep) and fused
(lists of at most 64: k_long alone).  Every result field is compared with the
oracle, and so that no family can pass by leaving its kernel, the route
counts (cld_last_route_stats) must equal what long_route_model works out from
the oracle's traces and the thresholds the source comments state -- none of
them is copied from a GPU run.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus
import long_route_model as lrm
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUADS, BEST = 0x0100, 0x4000                      # CLD_FLAG_SCORE_AS_QUADS, CLD_FLAG_BEST_EFFORT

# languages whose vocabulary carries distinct-boost hits in the suite's Q1 table, per ring class,
# and same-class languages that carry none
# ("sr" is left out of its close set: its vocabulary mixes Cyrillic and Latin words, which would cut spans)
EMIT = {0: [("cs", "sk"), ("da", "no"), ("es", "gl", "pt"), ("hr", "bs")], 1: [("hi", "ne", "bh", "mr")]}
QUIET = {0: ("en", "de", "fr"), 1: ("ru", "uk")}
CLOSE = {0: ("cs", "sk", "da", "no", "es", "gl", "pt", "hr", "bs", "en"), 1: ("ru", "uk", "bg", "mk", "be")}
# what stands between two spans of a class: the other class, RTypeOne scripts (Greek, Georgian), CJK, a single letter
SEPS = {0: ("ru", "el", "zh", "ar", "ko", "ka", "я"), 1: ("ar", "en", "el", "zh", "ka", "fa", "a")}


def _words(rng, lang, k):
    ws = corpus.vocab()[lang]
    return [ws[int(i)] for i in rng.integers(0, len(ws), size=k)]


def _synth(rng, lo, hi, n):
    return "".join(chr(int(c)) for c in rng.integers(lo, hi, size=n)).encode("utf-8")


def text(rng, kind, k):
    """k words of one script: a vocabulary language, Greek ("el") or Georgian
    ("ka") letters, CJK characters ("zh", "ko"), or the single letter given."""
    if kind == "el":
        return b" ".join(_synth(rng, 0x3B1, 0x3CA, int(rng.integers(3, 8))) for _ in range(k))
    if kind == "ka":
        return b" ".join(_synth(rng, 0x10D0, 0x10F1, int(rng.integers(3, 8))) for _ in range(k))
    if kind in ("zh", "ko"):
        pool = corpus.cjk_pools()[kind]
        return b"".join(pool[int(i)] for i in rng.integers(0, len(pool), size=2 * k))
    if kind not in corpus.vocab():
        return kind.encode("utf-8")
    return b" ".join(_words(rng, kind, k))


def mixed(rng, langs, k):
    return b" ".join(_words(rng, langs[int(rng.integers(len(langs)))], 1)[0] for _ in range(k))


def filler(rng, n):
    """One-span English documents of 257..320 bytes."""
    out = []
    for _ in range(n):
        t = b" ".join(_words(rng, "en", 80))
        cut = int(rng.integers(290, 320))
        while t[cut - 1:cut] == b" ":
            cut -= 1
        out.append(t[:cut])
    return out


class Runner:
    """Runs families in both batch forms and keeps the traces."""

    def __init__(self, gpu, oracle):
        self.gpu, self.oracle, self.cache = gpu, oracle, {}
        self.fill = filler(np.random.default_rng(900), 70)

    def trace(self, doc, flags=0):
        key = (doc, flags & QUADS)                # (BestEffort acts after the passes are decided)
        if key not in self.cache:
            self.cache[key] = lrm.trace(self.oracle, doc, flags & QUADS)
        return self.cache[key]

    def parity(self, docs, what, flags=0):
        buf, offs = self.gpu.pack(docs)
        got = self.gpu.detect_batch(buf=buf, offsets=offs, flags=flags)
        ref = self.oracle.detect_batch_ex(buf, offs, threads=8, flags=flags)
        assert_same(got, ref, what)
        st = self.gpu.last_stats(0)
        assert st.general_docs == 0, (what, list(st.long_requeue))
        return ref, st, self.gpu.last_route_stats(0).as_dict()

    def expect(self, docs, flags=0, wide=()):
        tr = [self.trace(d, flags) if len(d) > lrm.WAVE_CAP else None for d in docs]
        return lrm.expected_routes(docs, tr, wide=wide), tr

    def staged(self, docs, what, flags=0, wide=None, fill=None):
        """One batch of more than 64 long documents.  wide: {index: certain}
        -- documents that may (False) or must (True) meet the staged window's
        limit; the route counts are then bounded by both readings."""
        docs = list(docs) + list(self.fill if fill is None else fill)
        ref, st, rt = self.parity(docs, what + " staged", flags)
        wide = wide or {}
        lo, tr = self.expect(docs, flags, wide={i for i, sure in wide.items() if sure})
        hi, _ = self.expect(docs, flags, wide=set(wide))
        for f in lrm.FIELDS:
            a, b = sorted((lo[f], hi[f]))
            assert a <= rt[f] <= b, (what, f, rt, lo, hi)
        assert rt["long_list"] > lrm.SMALL_LIST
        assert list(st.passes[:3]) == [int((ref["passes"] == k).sum()) for k in (1, 2, 3)], (what, list(st.passes))
        return rt, tr

    def fused(self, docs, what, flags=0):
        """Lists of at most 64 long documents: the fused kernel alone."""
        for a in range(0, len(docs), lrm.SMALL_LIST):
            part = docs[a:a + lrm.SMALL_LIST]
            _, _, rt = self.parity(part, "%s fused %d" % (what, a), flags)
            want, _ = self.expect(part, flags)
            assert {f: rt[f] for f in lrm.FIELDS} == want, (what, a, rt)
            assert rt["store_units"] == 0

    def both(self, docs, what, flags=0, wide=None):
        rt, tr = self.staged(docs, what, flags, wide)
        self.fused(docs, what, flags)
        return rt, tr


@pytest.fixture(scope="module")
def run(gpu, oracle):
    return Runner(gpu, oracle)


# ------------------------------------------------------------ 1. route thresholds
def span_doc(rng, nsp, pair=("en", "ru"), min_bytes=300):
    """nsp spans: words of two scripts in turn, as many per span as min_bytes needs."""
    per = 1
    while True:
        d = b" ".join(text(rng, pair[j % 2], per) for j in range(nsp))
        if len(d) >= min_bytes:
            return d
        per += 1


SPAN_COUNTS = (1, 2, 32, 33, 47, 48, 49, 50, 63, 64, 65, 80, 81, 96, 97, 200)


def test_route_thresholds_by_span_count(run):
    """kHeavySpans (32), kParMin (48) and every group count from 4 to 13: a
    document of nsp spans is split exactly when nsp > 48, into ceil(nsp / 16) groups."""
    rng = np.random.default_rng(901)
    docs, nsps = [], []
    for pair in (("en", "ru"), ("cs", "hi"), ("ar", "de")):
        for n in SPAN_COUNTS:
            docs.append(span_doc(rng, n, pair))
            nsps.append(n)
    rt, tr = run.both(docs, "span counts")
    assert [tr[i].nsp for i in range(len(docs))] == nsps            # the builder's own claim
    assert rt["staged_split1"] == sum(n > 48 for n in nsps)
    assert rt["groups1"] == sum(-(-n // 16) for n in nsps if n > 48)
    assert rt["staged_whole"] == sum(n <= 48 for n in nsps) + len(run.fill)
    assert rt["to_fused"] == 0


@pytest.mark.parametrize("n", [63, 64, 65, 66])
def test_route_thresholds_by_list_length(run, n):
    """The host path skips the staged launches for a list of at most 64 long
    documents (every staged field 0) and takes them from 65 on; short
    documents in the batch do not count."""
    rng = np.random.default_rng(902)
    docs = filler(rng, n - 2) + [span_doc(rng, 60), span_doc(rng, 20)] + [b"short words", b"", b" ".join(_words(rng, "en", 30))[:200]]
    _, _, rt = run.parity(docs, "list of %d" % n)
    want, _ = run.expect(docs)
    assert {f: rt[f] for f in lrm.FIELDS} == want, rt
    assert rt["long_list"] == n
    if n <= 64:
        assert all(rt[f] == 0 for f in lrm.FIELDS[1:]) and rt["store_units"] == 0
    else:
        assert (rt["staged_whole"], rt["staged_split1"], rt["groups1"], rt["to_fused"]) == (n - 1, 1, 4, 0)
        assert rt["store_units"] > 0


DEVICE_CHILD = r'''
import sys, numpy as np, torch
torch.cuda.set_device(0)
import cld_amd
cld_amd.init_device(0)
dev = torch.device("cuda", 0)
inp = np.load(sys.argv[1])
out = {}
for key in sorted(k[:-4] for k in inp.files if k.endswith("_buf")):
    buf, offs = inp[key + "_buf"], inp[key + "_offs"]
    n = len(offs) - 1
    tb = torch.from_numpy(np.concatenate([buf, np.zeros(8, np.uint8)])).to(dev)
    to = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_out = torch.zeros(n * 40 + 8, dtype=torch.uint8, device=dev)
    cld_amd.detect_batch_device(0, tb.data_ptr(), to.data_ptr(), n, d_out.data_ptr(), None)
    torch.cuda.synchronize()
    rt = cld_amd.last_route_stats(0)
    out[key + "_out"] = d_out.cpu().numpy()[:n * 40].view(cld_amd.RESULT_DTYPE)
    out[key + "_rt"] = np.array([getattr(rt, f) for f in cld_amd.RouteStats.FIELDS], dtype=np.uint64)
np.savez(sys.argv[2], **out)
'''


def test_route_thresholds_device_resident(gpu, oracle, tmp_path):
    """A device-resident call cannot count its long documents on the host:
    the staged kernels are launched and k_lspan itself hands a list of at most
    64 to the fused kernel (to_fused == long_list), none of one of 65."""
    rng = np.random.default_rng(903)
    inp, batches = {}, {}
    for n in (63, 64, 65, 66):
        docs = filler(rng, n - 2) + [span_doc(rng, 60), span_doc(rng, 20)] + [b"short words", b" ".join(_words(rng, "en", 30))[:200]]
        buf, offs = gpu.pack(docs)
        inp["b%d_buf" % n], inp["b%d_offs" % n] = buf, offs
        batches[n] = docs
    np.savez(tmp_path / "in.npz", **inp)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(os.path.join(ROOT, p) for p in ("language-detector_amd", "oracle")))
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env=env, capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = np.load(tmp_path / "out.npz")
    for n, docs in batches.items():
        buf, offs = gpu.pack(docs)
        assert_same(out["b%d_out" % n], oracle.detect_batch(buf, offs, threads=8), "device list of %d" % n)
        rt = dict(zip(gpu.RouteStats.FIELDS, (int(v) for v in out["b%d_rt" % n])))
        tr = [lrm.trace(oracle, d) if len(d) > lrm.WAVE_CAP else None for d in docs]
        want = lrm.expected_routes(docs, tr, device_resident=True)
        assert {f: rt[f] for f in lrm.FIELDS} == want, (n, rt)
        assert rt["long_list"] == n and rt["to_fused"] == (n if n <= 64 else 0)


def test_route_thresholds_page_batches(run):
    """Batches whose long documents average 8 KB or more split only documents
    of more than kParMinPages (2000) spans; the same documents among 300-byte
    filler all split."""
    rng = np.random.default_rng(904)
    nsps = (49, 500, 1999, 2000, 2001, 2100)
    docs = [span_doc(rng, n) for n in nsps]
    pages = [b" ".join(_words(rng, "en", 2200))[:12288].rstrip() for _ in range(66)]
    assert lrm.page_batch(docs + pages) and not lrm.page_batch(docs + run.fill)
    rt, tr = run.staged(docs, "page batch", fill=pages)
    assert [tr[i].nsp for i in range(len(nsps))] == list(nsps)
    assert (rt["staged_split1"], rt["groups1"]) == (2, 126 + 132)
    rt, _ = run.staged(docs, "page documents among filler")
    assert (rt["staged_split1"], rt["groups1"]) == (6, sum(-(-n // 16) for n in nsps))
    run.fused(docs, "page documents")


def test_route_thresholds_span_table(run):
    """kMaxSpans: the span table holds 4096 entries and k_lspan hands a
    document on once it is full, so 4095 spans are stored and split, 4096 and
    4097 go to the fused kernel."""
    rng = np.random.default_rng(905)
    docs = [span_doc(rng, n, pair) for n in (4095, 4096, 4097) for pair in (("en", "ru"), ("hi", "cs"))]
    rt, tr = run.both(docs, "span table")
    assert [tr[i].nsp for i in range(6)] == [4095, 4095, 4096, 4096, 4097, 4097]
    assert (rt["staged_split1"], rt["groups1"], rt["to_fused"]) == (2, 2 * 256, 4)


# ------------------------------------------------------------ 2. group seams and the ring lookback
class Words:
    """The vocabulary split by what a word does to the boost ring: `loud`
    words each emit one distinct boost, `mute` words none (each word traced
    alone by the oracle)."""

    def __init__(self, run):
        self.loud, self.mute = {}, {}
        for lang in sorted({l for g in EMIT[0] + EMIT[1] for l in g} | set(QUIET[0] + QUIET[1] + CLOSE[1]) |
                           {"nl", "it", "ar", "fa"}):
            self.loud[lang], self.mute[lang] = [], []
            for w in corpus.vocab()[lang]:
                t = run.trace(w)
                if t.nsp == 1:
                    (self.loud if t.spans[0].distinct else self.mute)[lang].append(w)

    def take(self, rng, table, langs, k):
        out = []
        for _ in range(k):
            ws = table[langs[int(rng.integers(len(langs)))]]
            out.append(ws[int(rng.integers(len(ws)))])
        return b" ".join(out)


def big_span(rng, W, cls, group, head, tail):
    """A span of more than 1000 quad hits (two rounds, text wider than the 2 KB
    window): `head` emitting words first, mute text for the rest, and `tail`
    emitting words at its very end (the last round's distinct hits)."""
    quiet = ("en", "de", "fr", "nl", "it") if cls == 0 else ("ru", "uk", "be")
    body = [W.take(rng, W.loud, group, head), W.take(rng, W.mute, quiet, 600)]
    if tail:
        body.append(W.take(rng, W.loud, group, tail))
    return b" ".join(body)


LEAN_SEPS = {0: ("я", "el", "ж", "ka"), 1: ("a", "el", "x", "ka")}


def seam_doc(rng, W, cls, nsp, dist, spread, big=0, lean=False):
    """A document of nsp spans whose spans of class cls stand at the even
    indices, what SEPS[cls] lists between them.  dist: where the distinct
    emissions that a seam (span 16 g) must find lie -- "prev" (the class's span
    right before the seam), "group" (the first span of the previous group, or
    the one before it), "far" (behind 16 to 40 mute spans of the class),
    "zero" (span 0 only), "none".  spread: "one" (one span with exactly four),
    "four" (four spans with one each, other spans between), "five" (five to
    seven over two spans: the oldest must drop).  Everything else is mute, so a
    group scores with exactly the ring the lookback rebuilt: the class's spans
    after every seam are mixtures of one close set, which the ring's boosts
    decide.  big: the index of a two-round span (big_span), 0 for none.  lean:
    nearly all text is of the one close set and the separators are a letter or
    a short RTypeOne word, so that pass 1 is good enough and its result final."""
    group = EMIT[cls][int(rng.integers(len(EMIT[cls])))]
    seams = list(range(16, nsp, 16))
    emit_at = {}

    def emit(j, k):
        if 0 <= j < nsp:
            emit_at[j] = k

    for j0 in seams:
        if dist == "prev":
            base = j0 - 2
        elif dist == "group":
            base = j0 - 16 if rng.random() < 0.5 else j0 - 18
        elif dist == "far":
            base = j0 - 2 * int(rng.integers(16, 41))
        else:
            break
        if base < 0:
            continue
        if spread == "one":
            emit(base, 4)
        elif spread == "four":
            for k in range(4):
                emit(base - 2 * k, 1)
        else:
            emit(base, int(rng.integers(2, 4)))
            emit(base - 2, int(rng.integers(3, 5)))
        if dist == "far":
            break                                 # one emitting place: every later seam looks back to it
    if dist == "zero":
        emit(0, 4)
    close = group if cls == 0 else (CLOSE[1] if rng.random() < 0.6 else group)
    out = []
    for j in range(nsp):
        if j % 2 and lean:
            out.append(text(rng, LEAN_SEPS[cls][int(rng.integers(4))], 1))
        elif j % 2:
            kind = SEPS[cls][int(rng.integers(len(SEPS[cls])))]
            out.append(W.take(rng, W.mute, (kind,), 2) if kind in W.mute else text(rng, kind, int(rng.integers(1, 3))))
        elif j in emit_at:
            loud = W.take(rng, W.loud, group, emit_at[j]).split(b" ")
            mute = W.take(rng, W.mute, group, int(rng.integers(0, 3))).split()
            out.append(b" ".join(loud[:1] + mute + loud[1:]))
        elif big and j == big:
            out.append(big_span(rng, W, cls, group, 6, int(rng.integers(0, 3))))
        elif any(0 <= j - j0 < 6 for j0 in seams):
            out.append(W.take(rng, W.mute, close, int(rng.integers(3, 9))))
        else:
            out.append(W.take(rng, W.mute, group if lean else QUIET[cls], int(rng.integers(1, 3)) + 3 * lean))
    return b" ".join(out)


def seam_family(run, seed, big=False):
    if not hasattr(run, "words"):
        run.words = Words(run)
    rng = np.random.default_rng(seed)
    docs = []
    for cls in (0, 1):
        for nsp in (49, 64, 65, 97, 130):
            for dist in ("prev", "group", "far", "zero", "none"):
                for spread in ("one", "four", "five"):
                    if dist in ("zero", "none") and spread != "one":
                        continue
                    for lean in (False, True):
                        at = 2 * int(rng.integers(4, nsp // 2 - 1)) if big else 0
                        docs.append(seam_doc(rng, run.words, cls, nsp, dist, spread, at, lean))
    return docs


def check_lookback(tr, n):
    """The family does what it is for: at least half of its documents enter a
    group other than group 0 with a ring that is not empty, at least a tenth
    take an emission from further back than the previous group."""
    filled = far = 0
    for t in tr[:n]:
        a, b = lrm.ring_lookback(t)
        filled += a > 0
        far += b > 0
    assert 2 * filled >= n and 10 * far >= n, (filled, far, n)


@pytest.mark.parametrize("flags", [0, QUADS, BEST], ids=["plain", "quads", "besteffort"])
def test_group_seams_and_ring_lookback(run, flags):
    """Emission distance x spread x span counts 49 / 64 / 65 / 97 / 130 (last
    groups of 1, 16, 1, 1 and 2 spans) for both ring classes, separators that
    the walk must skip (the other class, RTypeOne scripts, CJK, single
    letters); also with ScoreAsQuads (RTypeOne scripts are then scored and
    walked) and BestEffort."""
    docs = seam_family(run, 910)
    rt, tr = run.both(docs, "seams %#x" % flags, flags)
    assert all(t.nsp > 48 for t in tr[:len(docs)])
    assert rt["staged_split1"] == len(docs) and rt["to_fused"] == 0
    assert rt["staged_split2"] > len(docs) // 10 and rt["groups2"] > 0          # pass 2 (Repeats) over groups
    check_lookback(tr, len(docs))


def test_group_seams_with_two_round_lookback_spans(run):
    """A span of more than 1000 quad hits in the lookback and among the scored
    spans: two hit rounds, the last with zero to two distinct hits, and text
    wider than the 2 KB window (tb + 48 > 2048: read from the store)."""
    docs = seam_family(run, 911, big=True)[::3]
    rt, tr = run.both(docs, "two-round lookback")
    bigs = [max(t.spans, key=lambda s: s.tb) for t in tr[:len(docs)]]
    ok = [s for s in bigs if len(s.rounds) == 2 and s.tb + 48 > lrm.ST_WINDOW and s.rounds[1][3] < 4]
    assert 2 * len(ok) >= len(docs), (len(ok), len(docs))
    assert rt["staged_split1"] + rt["to_fused"] == len(docs) and rt["staged_split1"] >= len(ok)
    check_lookback(tr, len(docs))


# ------------------------------------------------------------ 3. window edges
def exact_span(rng, lang, tb):
    """One span of exactly tb text bytes (the scanner's count: the text and its two framing spaces)."""
    t = b" ".join(_words(rng, lang, tb // 3 + 8))
    cut = tb - 2
    while (t[cut] & 0xC0) == 0x80:                # (asked for on a character boundary)
        cut -= 1
    t = bytearray(t[:cut])
    if t[-1:] == b" ":
        t[-1:] = b"x"
    return bytes(t) + b" " * (tb - 2 - cut)


def test_window_edges(run):
    """Spans around the staged window (tb + 48 of 2047 / 2048 / 2049: the
    last that is scored from LDS, the first two read from the store), a word
    straddling byte 2048, the fused window (6127 / 6128 / 6129), alone, as a
    lookback span and as a scored span of a group."""
    rng = np.random.default_rng(920)
    docs, want_tb = [], []
    for edge in (lrm.ST_WINDOW, lrm.FUSED_WINDOW):
        for d in (-1, 0, 1):
            for lang in ("en", "fr"):
                tb = edge - 48 + d
                s = exact_span(rng, lang, tb)
                docs.append(s)
                want_tb.append(tb)
                for at in (14, 16):                     # a group's last lookback span, its first scored span
                    parts = [text(rng, ("cs", "ru")[j % 2], 2) for j in range(60)]
                    parts[at] = s
                    docs.append(b" ".join(parts))
                    want_tb.append(tb)
    for at in (2040, 2046, 2047, 2048):
        pre = b" ".join(_words(rng, "en", 700))[:at - 6].rstrip()
        docs.append(pre + b" " * (at - 5 - len(pre)) + b"straddling " + b" ".join(_words(rng, "en", 40)))
        want_tb.append(None)
    rt, tr = run.both(docs, "window edges")
    for t, tb in zip(tr, want_tb):
        assert tb is None or max(s.tb for s in t.spans) == tb, (tb, [s.tb for s in t.spans][:20])
    assert rt["to_fused"] == 0


def test_window_wider_blocks_fall_back_to_the_fused_kernel(run):
    """Single words of 1990 to 3000 bytes, alone and with a few words after
    them.  A block of the hit stages wider than the staged kernels' 2 KB window
    cannot be scored through it: the scoring stage hands the document to the
    fused kernel (to_fused, never the sequential span source).  Which widths
    that is follows from the window (long_route_model.wide_block): a span of
    tb + 48 <= 2048 text bytes lies in LDS whole and cannot fall; a longer one
    of at most 64 words is one block of tb + 24 bytes, which the window holds up
    to 2033.  So spans of up to 2009 text bytes (words of up to 2007 bytes)
    stay on the staged path -- not, as one might expect, only those below 1990
    -- and from 2010 on they fall, every one."""
    rng = np.random.default_rng(921)
    docs = []
    for w in (1990, 1997, 1998, 1999, 2000, 2003, 2006, 2007, 2008, 2009, 2030, 2047, 2048, 2049, 2060, 3000):
        for tail in (0, 3):
            word = bytes(rng.integers(97, 123, size=w).astype(np.uint8))
            docs.append(word + (b" " + b" ".join(_words(rng, "en", tail)) if tail else b""))
    tbs = [run.trace(d).spans[0].tb for d in docs]
    assert all(run.trace(d).nsp == 1 for d in docs) and tbs[::2] == [len(d) + 2 for d in docs[::2]]
    assert {2000, 2001, 2009, 2010} <= set(tbs)                     # both edges of the rule, each side
    wide = {i: True for i, tb in enumerate(tbs) if lrm.wide_block(tb, 4)}
    rt, _ = run.both(docs, "wide words", wide=wide)
    assert rt["to_fused"] == len(wide) and rt["staged_whole"] == len(docs) + len(run.fill)


def test_window_squeeze_documents_reach_the_fused_kernel(run):
    """Spans of 2047 and 2048 text bytes do not take CheapSqueezeTriggerTest
    and spans of 2049 and more do (2048 < text_bytes): repetitive text there
    restarts with Squeeze, which only the fused kernel runs.  k_lspan hands such
    a document on without a reason slot (the Why slots are the fused kernel's
    own hand-ons), so what can be held to the trace is to_fused, one per
    restart, and the pass counts."""
    rng = np.random.default_rng(922)
    docs = []
    menu = corpus.BOILERPLATE.replace(b"| ", b"")       # (letters and spaces only: every byte is text)
    for tb in (2047, 2048, 2049, 2050, 2100, 4000):
        reps = menu * (tb // len(menu) + 2)
        docs.append(reps[:tb - 3].rstrip().ljust(tb - 3, b"x") + b"z")
        docs.append((b"a b c d e f g h " * 400)[:tb - 3] + b"z")
    docs += [d + b" " + text(rng, "ru", 20) for d in docs]
    rt, tr = run.both(docs, "squeeze edge")
    sq = [t.squeeze1 for t in tr[:len(docs)]]
    assert [t.spans[0].tb for t in tr[:4]] == [2047, 2047, 2048, 2048] and not any(sq[:4])
    assert all(sq[4:12]) and all(sq[16:]) and rt["to_fused"] == sum(sq)


# ------------------------------------------------------------ 4. hit rounds
def hits_span(run, rng, kind, target):
    """One span whose base hits (quadgrams, or CJK unigrams), counted by the
    oracle's trace over all its rounds, number exactly target."""
    cjk = kind in ("zh", "ko")
    join = b"" if cjk else b" "
    pool = corpus.cjk_pools()[kind] if cjk else corpus.vocab()[kind]
    unit = lambda: pool[int(rng.integers(len(pool)))]
    units = [unit() for _ in range(2 * target)]
    hits = lambda parts: run.trace(join.join(parts)).spans[0].quads
    lo, hi = 1, len(units)                        # the longest prefix of at most target hits
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if hits(units[:mid]) <= target:
            lo = mid
        else:
            hi = mid - 1
    parts = units[:lo]
    for _ in range(6):
        have = hits(parts)
        for _ in range(40):
            if have == target:
                return join.join(parts)
            cand = parts + [unit()]
            got = hits(cand)
            if got <= target:
                parts, have = cand, got
        parts = parts[:-3]                            # no word fits: back off and take other words
    raise AssertionError("no span of %d hits from %s" % (target, kind))


def test_hit_rounds(run):
    """A hit round holds 1000 base hits: spans of 999, 1000, 1001, 1999, 2000
    and 2001 of them (one, two and three rounds), quadgram and CJK, scored
    whole, as a member of a group, and fused."""
    rng = np.random.default_rng(930)
    docs, want = [], []
    for kind in ("en", "ru", "zh"):
        for target in (999, 1000, 1001, 1999, 2000, 2001):
            s = hits_span(run, rng, kind, target)
            docs.append(s)
            other = ("hi", "cs") if kind != "en" else ("ru", "hi")
            parts = [text(rng, other[j % 2], 2) for j in range(52)]
            parts[20] = s
            docs.append(b" ".join(parts))
            want += [target] * 2
    rt, tr = run.both(docs, "hit rounds")
    rounds = set()
    for t, target in zip(tr, want):
        s = max(t.spans, key=lambda s: s.quads)
        assert s.quads == target and target // 1000 <= len(s.rounds) <= target // 1000 + 1, (target, s.quads, s.rounds)
        rounds.add(len(s.rounds))
    assert rounds == {1, 2, 3}
    assert rt["staged_split1"] == len(docs) // 2 - sum(t.squeeze1 for t in tr[1:len(docs):2])


# ------------------------------------------------------------ 5. vector mode
def test_vector_mode_over_the_same_documents(run):
    """Families 2 to 4 once through cld_detect_batch_vec (k_long<VEC>), chunk
    for chunk against the oracle's vectors."""
    from test_gpu_vector import check
    rng = np.random.default_rng(940)
    docs = seam_family(run, 910)[::7] + seam_family(run, 911, big=True)[::29]
    for edge in (lrm.ST_WINDOW, lrm.FUSED_WINDOW):
        docs += [exact_span(rng, "en", edge - 48 + d) for d in (-1, 0, 1)]
    docs += [bytes(rng.integers(97, 123, size=w).astype(np.uint8)) + b" " + text(rng, "en", 30) for w in (2000, 2048, 2060)]
    docs += [hits_span(run, rng, kind, t) for kind in ("en", "zh") for t in (1000, 1001)]
    buf, offs = run.gpu.pack(docs)
    check(run.gpu, run.oracle, buf, offs, "long seams, vector mode")
    st, rt = run.gpu.last_stats(0), run.gpu.last_route_stats(0).as_dict()
    assert st.general_docs == 0 and rt["long_list"] == len(docs)
    assert all(rt[f] == 0 for f in lrm.FIELDS[1:])                 # (k_long<VEC> takes the whole list)
