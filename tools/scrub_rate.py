"""Rates of CLD_FLAG_SCRUB_UTF8 beside the two older choices (GPU box).  One
JSON line per corpus, also written to profiles/scrub_rate.jsonl.

cld_detect_batch end to end from host buffers with flags 0,
CLD_FLAG_CHECK_UTF8 and CLD_FLAG_SCRUB_UTF8, alternated call by call, on
tools/messy_rate.py's corrupted corpus (seed 101, 12000 per config) and on the
same corpus clean: docs/s (median, with the fastest and the slowest call),
general_docs (documents on the sequential span source) and the number of
documents answered with a language (summary_lang neither UNKNOWN nor failed).

    python tools/scrub_rate.py [--reps N] [--small] [--once FLAGS] [--out PATH]

--once FLAGS: no timing; three calls with that flags word on the clean corpus
(the run a kernel profiler wraps to price the prepare step alone).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("language-detector_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import cld_amd  # noqa: E402
import corpus  # noqa: E402

NAMES = {0: "unchecked", cld_amd.FLAG_CHECK_UTF8: "checked", cld_amd.FLAG_SCRUB_UTF8: "scrubbed"}


def corpora(small):
    import test_gpu_corrupt as tc
    seed, n_each = 101, (1200 if small else 12000)
    clean = []
    for cfg, n in (("c2", n_each), ("c3", max(8, n_each // 40)), ("c4", n_each // 2), ("c5", n_each)):
        b, o = corpus.GENERATORS[cfg](n, seed=seed)
        clean += [bytes(b[o[i]:o[i + 1]]) for i in range(n)]
    rng = np.random.default_rng(seed)
    return [tc.corrupt(rng, d) for d in clean], clean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a tenth of the sizes")
    ap.add_argument("--once", type=lambda v: int(v, 0), default=None, help="three untimed calls with these flags, clean corpus")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub_rate.jsonl"))
    a = ap.parse_args()
    cld_amd.init_device(0, tables=cld_amd.SYNTH_TABLES)
    messy, clean = corpora(a.small)
    if a.once is not None:
        buf, offs = cld_amd.pack(clean)
        for _ in range(3):
            cld_amd.detect_batch(buf=buf, offsets=offs, flags=a.once)
        return
    lines = []
    for name, docs in (("corrupted", messy), ("clean", clean)):
        buf, offs = cld_amd.pack(docs)
        lens = np.diff(offs).astype(np.int64)
        times = {f: [] for f in NAMES}
        seq, answered = {}, {}
        for flags in times:                                 # warm-up, and the counts (the same in every call)
            for _ in range(2):
                res = cld_amd.detect_batch(buf=buf, offsets=offs, flags=flags)
            seq[flags] = int(cld_amd.last_stats(0).general_docs)
            lang = res["summary_lang"]
            answered[flags] = int(np.count_nonzero((lang != cld_amd.UNKNOWN_LANGUAGE) & (lang != cld_amd.LANG_FAILED)))
        for _ in range(a.reps):                             # alternated: all three see the same card state
            for flags in times:
                t = time.perf_counter()
                cld_amd.detect_batch(buf=buf, offsets=offs, flags=flags)
                times[flags].append((time.perf_counter() - t) * 1e3)
        vp = cld_amd.valid_prefix_batch(buf=buf, offsets=offs)
        _, replaced = cld_amd.scrub_utf8_batch(buf=buf, offsets=offs)
        row = {"measure": "detect_batch", "corpus": name, "docs": len(docs), "bytes": len(buf), "reps": a.reps,
               "not_interchange_valid": int(np.count_nonzero(vp != lens)),
               "repaired": int(np.count_nonzero(replaced)), "replaced_bytes": int(replaced.sum())}
        for flags, label in NAMES.items():
            t = np.asarray(times[flags])
            m = float(np.median(t))
            row.update({label + "_ms": round(m, 2), label + "_ms_min": round(float(t.min()), 2),
                        label + "_ms_max": round(float(t.max()), 2), label + "_docs_per_s": round(len(docs) / m * 1e3),
                        label + "_general_docs": seq[flags], label + "_answered": answered[flags]})
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
