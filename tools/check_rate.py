"""Rates of the checked entry points (GPU box).  One JSON line per measurement.

validator   cld_valid_prefix_device over HBM-resident C2 (1M tweets) and C3
            (100K 16 KB pages), timed with device events, beside a torch
            device-to-device copy of the same buffer timed the same way and
            alternated with it in this process: the copy is the one-pass floor
            of that card that day (it reads and writes the bytes once each).
corpus      cld_detect_batch end to end from host buffers with and without
            CLD_FLAG_CHECK_UTF8, alternated, on tools/messy_rate.py's corrupted
            corpus (seed 101, 12000 per config) and on the same corpus clean,
            with general_docs (documents on the sequential span source).

    python tools/check_rate.py [--part validator|corpus|all] [--reps N] [--small]
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


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def validator(reps, small):
    import torch
    dev = torch.device("cuda", 0)
    for cfg, n in (("c2", 50_000 if small else 1_000_000), ("c3", 5_000 if small else 100_000)):
        buf, offs = corpus.GENERATORS[cfg](n)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        d_buf = torch.from_numpy(buf).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_vp = torch.empty(n, dtype=torch.int32, device=dev)
        d_copy = torch.empty_like(d_buf)
        st = torch.cuda.Stream()                            # (a stream of its own: NULL means the runtime's stream to the library)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def timed(fn):
            with torch.cuda.stream(st):
                ev[0].record()
                fn()
                ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1])

        check = lambda: cld_amd.valid_prefix_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_vp.data_ptr(), st.cuda_stream)
        copy = lambda: d_copy.copy_(d_buf)
        for _ in range(3):
            timed(check), timed(copy)
        t_check, t_copy = [], []
        for _ in range(reps):                               # alternated: both see the same card state
            t_check.append(timed(check))
            t_copy.append(timed(copy))
        torch.cuda.synchronize()
        vp = d_vp.cpu().numpy()
        lens = np.diff(offs).astype(np.int64)
        gb = len(buf) / 1e9
        mc, mp = median(t_check), median(t_copy)
        print(json.dumps({"measure": "validator", "corpus": cfg, "docs": n, "bytes": len(buf), "reps": reps,
                          "check_ms": round(mc, 4), "check_ms_min": round(min(t_check), 4),
                          "check_ms_max": round(max(t_check), 4), "check_GBps": round(gb / (mc / 1e3), 1),
                          "copy_ms": round(mp, 4), "copy_read_GBps": round(gb / (mp / 1e3), 1),
                          "check_over_copy_read": round(mp / mc, 3),
                          "rejected": int(np.count_nonzero(vp != lens))}), flush=True)


def corpora(reps, small):
    import test_gpu_corrupt as tc
    seed, n_each = 101, (1200 if small else 12000)
    clean = []
    for cfg, n in (("c2", n_each), ("c3", max(8, n_each // 40)), ("c4", n_each // 2), ("c5", n_each)):
        b, o = corpus.GENERATORS[cfg](n, seed=seed)
        clean += [bytes(b[o[i]:o[i + 1]]) for i in range(n)]
    rng = np.random.default_rng(seed)
    messy = [tc.corrupt(rng, d) for d in clean]
    for name, docs in (("corrupted", messy), ("clean", clean)):
        buf, offs = cld_amd.pack(docs)
        times = {0: [], cld_amd.FLAG_CHECK_UTF8: []}
        seq = {}
        for flags in times:
            for _ in range(2):
                cld_amd.detect_batch(buf=buf, offsets=offs, flags=flags)
            seq[flags] = int(cld_amd.last_stats(0).general_docs)
        for _ in range(reps):                               # alternated
            for flags in times:
                t = time.perf_counter()
                cld_amd.detect_batch(buf=buf, offsets=offs, flags=flags)
                times[flags].append((time.perf_counter() - t) * 1e3)
        vp = cld_amd.valid_prefix_batch(buf=buf, offsets=offs)
        m0, m1 = median(times[0]), median(times[cld_amd.FLAG_CHECK_UTF8])
        print(json.dumps({"measure": "detect_batch", "corpus": name, "docs": len(docs), "bytes": len(buf), "reps": reps,
                          "rejected": int(np.count_nonzero(vp != np.diff(offs).astype(np.int64))),
                          "unchecked_ms": round(m0, 2), "unchecked_ms_min": round(min(times[0]), 2),
                          "unchecked_ms_max": round(max(times[0]), 2), "unchecked_docs_per_s": round(len(docs) / m0 * 1e3),
                          "checked_ms": round(m1, 2), "checked_ms_min": round(min(times[cld_amd.FLAG_CHECK_UTF8]), 2),
                          "checked_ms_max": round(max(times[cld_amd.FLAG_CHECK_UTF8]), 2),
                          "checked_docs_per_s": round(len(docs) / m1 * 1e3),
                          "unchecked_general_docs": seq[0], "checked_general_docs": seq[cld_amd.FLAG_CHECK_UTF8]}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("validator", "corpus", "all"), default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a tenth of the sizes (a profiler run)")
    a = ap.parse_args()
    if a.part in ("validator", "all"):                      # torch first: the library then shares its HIP runtime
        import torch
        torch.cuda.set_device(0)
    cld_amd.init_device(0, tables=cld_amd.SYNTH_TABLES)
    if a.part in ("validator", "all"):
        validator(a.reps, a.small)
    if a.part in ("corpus", "all"):
        corpora(a.reps, a.small)


if __name__ == "__main__":
    main()
