"""ApplyHints on the GPU against ApplyHints on the host, on the same HTML pages.

  python tools/hints_rate.py [--docs 100000] [--threads 16] [--runs 15]

Kernel: cld_hint_boosts_device (cld_hints.hip) on corpus.html(docs) resident in
HBM, timed by HIP events on its stream: the median of `runs` after 5 warm-up
calls.  Host: cld_hint_priors per page on `threads` threads, each with a
contiguous share like apply_hints() (tools/hint_host_bench.cpp, wall time,
median of `runs` after one warm-up pass).  One JSON line each."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "language-detector_amd"))
os.environ.setdefault("CLD_MI355X_TABLES", os.path.join(ROOT, "language-detector_amd", "data", "cld2_synth_q1.cldt"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=15)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)                 # torch first: the library then shares its HIP runtime (as in bench.py)
    import cld_amd
    import corpus
    cld_amd.init_device(0)
    buf, offs = corpus.html(a.docs)
    buf, offs = np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(offs, np.uint64)
    n = len(offs) - 1
    dev = torch.device("cuda", 0)
    d_buf = torch.from_numpy(buf).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    pri = torch.zeros((n, 14), dtype=torch.int16, device=dev)
    boo = torch.zeros((n, 16), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    ms = []
    for r in range(a.runs + 5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(s)
        cld_amd.hint_boosts_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, None, None, 0, False, pri.data_ptr(),
                                   boo.data_ptr(), s.cuda_stream)
        t1.record(s)
        s.synchronize()
        if r >= 5:
            ms.append(t0.elapsed_time(t1))
    ms.sort()
    print(json.dumps({"what": "k_apply_hints", "docs": n, "bytes": int(len(buf)),
                      "with_priors": int((boo != 0).any(dim=1).sum().item()), "kernel_ms_median": ms[len(ms) // 2],
                      "kernel_ms_min": ms[0], "kernel_ms_max": ms[-1], "runs": len(ms)}), flush=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "build/hint_host_bench"], check=True)
    with tempfile.TemporaryDirectory() as d:
        buf.tofile(os.path.join(d, "buf"))
        offs.tofile(os.path.join(d, "offs"))
        subprocess.run([os.path.join(ROOT, "tools", "build", "hint_host_bench"), cld_amd.LIB_PATH, os.path.join(d, "buf"),
                        os.path.join(d, "offs"), str(a.threads), str(a.runs)], check=True)


if __name__ == "__main__":
    main()
