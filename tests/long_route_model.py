"""What the long-document path must do with a batch, worked out from the
reference side alone: the oracle's trace of each document (one `span <script>
<bytes>` line per script span, one `hitbuffer <script> base/delta/distinct b d
x` line per hit round of a scored span followed by the round's linearised hits,
`[i]offset,D=langprob` for a distinct one, `restart squeeze`, `recurse`) and the
routing rules written in the kernels' source comments.

  * a document of more than 256 bytes is on the long list (k_wave's cap);
  * a long list of at most SMALL_LIST documents goes whole to the fused
    k_long: on the host path the staged launches are skipped (every staged
    field reads 0), on a device-resident call k_lspan hands the list over
    (to_fused == long_list);
  * otherwise k_lspan stores pass 1's spans, except for a document that takes
    the Squeeze restart in pass 1 or has MAX_SPANS spans or more: fused;
  * a stored document of more than PAR_MIN spans is split into groups of
    PAR_G spans -- more than PAR_MIN_PAGES spans where the long documents of
    the batch average 8 KB or more (whole KB, capped at 63, as k_len_hist
    buckets them);
  * a stored document whose pass 1 is not good enough (`recurse`) takes pass
    2, split again if it was split;
  * a document with a span block wider than the staged kernels' 2 KB window
    is handed to the fused kernel by the scoring stage (callers name those
    documents: the trace does not show block widths; wide_block() is the rule
    for a span of at most 64 words).

Left out, because nothing at these sizes and default settings can reach them:
k_lspan's other whole-batch routes (CLD_LONG_HEAVY_KB, documents over the fused
kernel's 1 MB cap), the span cache's 512 KB, a store without room (the default
is 8 GB), a full group list (its capacity is at least 65,536 groups, so that
fallback is not tested here) and records that outgrow their room.

The kernels' span count equals the trace's by construction of the documents
used here: plain text, every span shorter than the 40 KB script buffer, so
neither side cuts a span, and the trace prints every span the scanner
returns, the unscored ones (RTypeNone / RTypeOne, one byte) included."""
import ctypes

import numpy as np

from oracle import TRACE_FN

WAVE_CAP = 256
SMALL_LIST = 64
PAR_MIN, PAR_G, PAR_MIN_PAGES, HEAVY_SPANS, MAX_SPANS = 48, 16, 2000, 32, 4096
ST_WINDOW, FUSED_WINDOW = 2048, 6128
FIELDS = ("long_list", "staged_whole", "staged_split1", "groups1", "staged_pass2", "staged_split2", "groups2",
          "to_fused")


class Span:
    __slots__ = ("script", "tb", "rounds")

    def __init__(self, script, tb):
        self.script, self.tb, self.rounds = script, tb, []

    @property
    def quads(self):
        return sum(r[0] for r in self.rounds)

    @property
    def distinct(self):                           # distinct-boost emissions (ring entries), all rounds
        return sum(r[3] for r in self.rounds)

    @property
    def cls(self):                                # the boost ring it shares: 0 Latin, 1 every other script
        return 0 if self.script == "Latn" else 1


class Trace:
    """passes: the span lists of the oracle's passes, in order (a pass cut
    short by the Squeeze restart included); squeeze1: pass 1 took the restart;
    recurse: the first complete pass was not good enough."""

    def __init__(self):
        self.passes, self.squeeze1, self.recurse = [[]], False, False

    @property
    def spans(self):
        return self.passes[0]

    @property
    def nsp(self):
        return len(self.passes[0])


def trace(oracle, doc, flags=0):
    t = Trace()

    def line(_a, s):
        c = s[:1]
        if c == b"s" and s[:5] == b"span ":
            _, script, tb = s.split()
            t.passes[-1].append(Span(script.decode(), int(tb)))
        elif c == b"h" and s[:10] == b"hitbuffer ":
            w = s.split()
            t.passes[-1][-1].rounds.append([int(w[3]), int(w[4]), int(w[5]), 0])
        elif c == b"[" and b",D=" in s:
            t.passes[-1][-1].rounds[-1][3] += 1
        elif c == b"r" and s[:7] == b"restart":
            t.squeeze1 |= len(t.passes) == 1
            t.passes.append([])
        elif c == b"r" and s[:7] == b"recurse":
            t.recurse = True
            t.passes.append([])

    cb = TRACE_FN(line)
    oracle.lib.cldo_set_flags.argtypes = [ctypes.c_void_p, ctypes.c_int]
    oracle.lib.cldo_set_flags(oracle.ctx, int(flags))
    oracle.lib.cldo_set_trace(oracle.ctx, cb, None)
    try:
        oracle.detect(bytes(doc))
    finally:
        oracle.lib.cldo_set_trace(oracle.ctx, TRACE_FN(0), None)
        oracle.lib.cldo_set_flags(oracle.ctx, 0)
    return t


class Facts:
    """What expected_routes reads of a Trace, from the oracle's first-pass
    record alone (Oracle.first_pass): for batches too large to trace."""

    def __init__(self, oracle, doc, flags=0):
        self.nsp, self.max_tb, self.squeeze1, self.recurse = oracle.first_pass(doc, flags)


def page_batch(docs):
    """k_lspan's page-batch test over the long documents of the batch."""
    kb = [min(len(d) >> 10, 63) for d in docs if len(d) > WAVE_CAP]
    return bool(kb) and sum(kb) >= 8 * len(kb)


def wide_block(tb, words):
    """Whether the staged scoring stage must hand on a span of tb text bytes
    and at most 64 words.  A span of tb + 48 <= 2048 bytes is copied into the
    LDS window whole.  A longer one is read through the window block by block;
    the widest block is the word-list stage's, 64 words and 24 bytes of
    lookahead -- here the whole span, [1, tb + 24) -- loaded from the 16-byte
    boundary at or below 32 bytes before its start (0 here) into a window that
    holds 2048 - 15 bytes from there."""
    assert words <= 64
    return tb + 48 > ST_WINDOW and tb + 24 > ST_WINDOW - 15


def expected_routes(docs, traces, device_resident=False, wide=()):
    """The route counts of one batch (one chunk of the host path).  traces[i]:
    trace() of docs[i], needed for the long ones only; wide: indices of the
    documents that hold a block wider than the staged window."""
    want = dict.fromkeys(FIELDS, 0)
    longs = [i for i, d in enumerate(docs) if len(d) > WAVE_CAP]
    want["long_list"] = len(longs)
    if len(longs) <= SMALL_LIST:
        if device_resident:
            want["to_fused"] = len(longs)
        return want
    par_min = PAR_MIN_PAGES if page_batch(docs) else PAR_MIN
    for i in longs:
        t = traces[i]
        if t.squeeze1 or t.nsp >= MAX_SPANS:
            want["to_fused"] += 1
            continue
        split = t.nsp > par_min
        ng = -(-t.nsp // PAR_G)
        if split:
            want["staged_split1"] += 1
            want["groups1"] += ng
        else:
            want["staged_whole"] += 1
        if i in wide:
            want["to_fused"] += 1
            continue
        if t.recurse:
            want["staged_pass2"] += 1
            if split:
                want["staged_split2"] += 1
                want["groups2"] += ng
    return want


def ring_lookback(t, flags=0):
    """Over the groups g > 0 of a split document: (entering rings that are not
    empty, entering rings holding an emission from before the previous group).
    A group needs the ring of a class when one of its spans of that class is
    scored (has hit rounds); the ring holds the last four distinct emissions of
    the earlier spans of the class."""
    sp = t.spans
    filled = far = 0
    for j0 in range(PAR_G, len(sp), PAR_G):
        for cls in (0, 1):
            if not any(s.cls == cls and s.rounds for s in sp[j0:j0 + PAR_G]):
                continue
            got, oldest = 0, None
            for j in range(j0 - 1, -1, -1):
                if sp[j].cls == cls and sp[j].distinct:
                    got += sp[j].distinct
                    oldest = j
                    if got >= 4:
                        break
            filled += got > 0
            far += oldest is not None and oldest < j0 - PAR_G
    return filled, far


def pack(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=offs[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs
