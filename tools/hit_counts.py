"""Word and quad-chain counts per document of a corpus config, on the CPU: what
k_wave's hit stages iterate over (words per span, chain entries per word and
per span, the share of spans that need the second 64-entry register).

hit_counts.py [CONFIG [DOCS]]   (default c2 20000)

The text is lowered and split the way a single-script span is (letters kept,
everything else a single space); the chain follows GetQuadHits' step
(cldutil.cc:340-400) on the UTF-8 bytes.  Base / delta / distinct hits, base
emissions, spans and chunks per document come from the oracle's trace (the
hit buffers, the linear list and the chunk starts it prints), on the tables
of CLD_MI355X_TABLES or the synthetic Q1."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "language-detector_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import corpus  # noqa: E402
from oracle import DEFAULT_TABLES, Oracle  # noqa: E402

VOWELS = set(b"AEIOUaeiou")


def adv_but_space(c):
    return 0 if c <= 0x20 else 1 if c < 0xC0 else 2 if c < 0xE0 else 3 if c < 0xF0 else 4


def chain_entries(text, start, limit):
    """Entries of the quad chain over text[start:limit] (text ends in spaces)."""
    n, p = 0, start
    while p < limit:
        if text[p] == 0x20:
            p += 1
            continue
        n += 1
        a1 = p + adv_but_space(text[p])
        a2 = a1 + adv_but_space(text[a1])
        c2 = text[a2]
        a3 = a2 + adv_but_space(c2)
        a4 = a3 + adv_but_space(text[a3])
        nx = a2 + (1 if (c2 <= 0x20 or c2 in VOWELS or (c2 & 0xC0) == 0x80) else 0)
        if text[a4] == 0x20 or a2 >= limit or nx >= limit:
            while p < limit and text[p] != 0x20:      # the word's chain ends: on to the next word
                p += 1
        else:
            p = nx
    return n


def traced(o, doc):
    """(spans, base hits, delta hits, distinct hits, base emissions, chunks) of one document."""
    _, _, lines = o.detect(doc, trace=True)
    spans = base = delta = dist = em = chunks = 0
    for x in lines:
        if x.startswith("hitbuffer"):
            spans += 1
            b, d, t = x.split()[-3:]
            base += int(b); delta += int(d); dist += int(t)
        elif x.startswith("chunkstart"):
            chunks += int(x.split()[1])
        elif ",Q=" in x or (",U=" in x and not x.endswith("=00000000")):
            em += 1
    return spans, base, delta, dist, em - spans, chunks          # (a seed opens every span's list)


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    buf, offs = corpus.GENERATORS[cfg](n)
    buf = bytes(np.asarray(buf))
    words, chain = [], []
    for i in range(n):
        s = buf[offs[i]:offs[i + 1]].decode("utf-8", "replace").lower()
        ws = [w for w in re.split(r"[\W\d_]+", s) if w]
        text = (" " + " ".join(ws) + "    ").encode("utf-8") + b"\0" * 16
        limit = len(text) - 16 - 3
        words.append(len(ws) + 1)                     # GetOctaHits also takes the empty word at the end
        chain.append(chain_entries(text, 1, limit))
    words, chain = np.array(words), np.array(chain)
    print("%s, %d documents (one Latin span each assumed)" % (cfg, n))
    for name, v in (("words (octa stage)", words), ("chain entries (quad stage)", chain)):
        print("  %-28s mean %.1f  p50 %d  p99 %d  max %d  > 64: %.2f %%  > 128: %.3f %%" %
              (name, v.mean(), np.percentile(v, 50), np.percentile(v, 99), v.max(), 100.0 * (v > 64).mean(),
               100.0 * (v > 128).mean()))
    print("  chain entries per word       mean %.2f" % (chain.sum() / max(1, (words - 1).sum())))
    o = Oracle(os.environ.get("CLD_MI355X_TABLES", DEFAULT_TABLES))
    t = np.array([traced(o, buf[offs[i]:offs[i + 1]]) for i in range(n)])
    for k, name in enumerate(("scored spans", "base hits", "delta hits", "distinct hits", "base emissions", "chunks")):
        v = t[:, k]
        print("  %-28s mean %.2f  p50 %d  p99 %d  max %d  > 64: %.2f %%  > 128: %.3f %%" %
              (name, v.mean(), np.percentile(v, 50), np.percentile(v, 99), v.max(), 100.0 * (v > 64).mean(),
               100.0 * (v > 128).mean()))
    print("  chunks per scored span       mean %.2f" % (t[:, 5].sum() / max(1, t[:, 0].sum())))


if __name__ == "__main__":
    main()
