"""The two vector entries on the same batches.

  python tools/device_vec_rate.py host   [--binding DIR]     cld_detect_batch_vec alone, no torch
  python tools/device_vec_rate.py device                     both entries

cld_detect_batch_vec (host buffers: upload, kernels, download) by wall clock around
the blocking call; cld_detect_batch_device_vec (batch and outputs resident in HBM)
by events on the torch stream it is enqueued on.  Medians after 3 warm-up calls,
one JSON line per batch.  The device entry's outputs are compared with the host
entry's at every size timed.  --binding DIR imports cld_amd from DIR: another
commit's binding, with that commit's library in CLD_MI355X_LIB.  For the kernel
times run `device --reps 3` under rocprofv3 --kernel-trace --stats: k_vec_gather
is the host entry's gather, k_vec_gather_chunks the device entry's.

Batches: corpus.c5(2000) and corpus.c2(3000) (the sizes of tests/test_gpu_vector.py),
c2 at 200 K and, with `device`, the gather's two extremes: a million tweets of about
one chunk each, and one document of 15,000 one-script paragraphs (15,000 chunks)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAGRAPHS = ["Ελληνικά κείμενο εδώ και τώρα ", "ภาษาไทยข้อความที่นี่ตอนนี้ ", "ქართული ტექსტი აქ და ახლა ",
              "հայերեն տեքստ այստեղ և հիմա "]


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["host", "device"])
    ap.add_argument("--binding", default=None)
    ap.add_argument("--reps", type=int, default=0, help="timed calls per batch (default: 20, 5 for the large ones)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "language-detector_amd"))
    if a.binding:
        sys.path.insert(0, a.binding)
    if a.mode == "device":
        import torch
        torch.cuda.set_device(0)               # torch first: the library then shares its HIP runtime
    import cld_amd
    import corpus
    cld_amd.init_device(0, tables=os.path.join(ROOT, "language-detector_amd", "data", "cld2_synth_q1.cldt"))
    L = cld_amd.lib()
    batches = [("c5_2000", lambda: corpus.c5(2000), 20), ("c2_3000", lambda: corpus.c2(3000), 20),
               ("c2_200000", lambda: corpus.c2(200000), 5)]
    if a.mode == "device":
        one = "".join(PARAGRAPHS[i % 4] for i in range(15000)).encode()
        assert len(one) < (1 << 20) - 64       # the parallel span builder's documents
        batches += [("c2_1000000", lambda: corpus.c2(1000000), 3), ("one_doc_15000_paragraphs", lambda: cld_amd.pack([one]), 2)]
    for name, make, reps in batches:
        reps = a.reps or reps
        buf, offs = make()
        n = len(offs) - 1
        res, chunks, coffs = cld_amd.detect_batch_vec(buf=buf, offsets=offs)
        total = int(coffs[-1])
        row = {"batch": name, "lib": os.environ.get("CLD_MI355X_LIB", "tree"), "docs": n, "bytes": int(offs[-1]),
               "chunks": total}
        out = np.zeros(n, cld_amd.RESULT_DTYPE)
        ch = np.zeros(max(total, 1), cld_amd.CHUNK_DTYPE)
        co = np.zeros(n + 1, np.uint64)
        t = []
        for _ in range(3 + reps):
            t0 = time.perf_counter()
            rc = L.cld_detect_batch_vec(buf.ctypes.data, offs.ctypes.data, n, None, 0, out.ctypes.data, ch.ctypes.data,
                                        total, co.ctypes.data)
            t.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        row["host_wall"] = stats(t[3:])
        if a.mode == "device":
            dev = torch.device("cuda", 0)
            d_buf = torch.from_numpy(buf).to(dev)
            d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
            d_out = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
            d_ch = torch.zeros(max(total, 1) * 12, dtype=torch.uint8, device=dev)
            d_co = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_st = torch.zeros(16, dtype=torch.uint8, device=dev)
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            t = []
            for _ in range(3 + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                cld_amd.detect_batch_device_vec(0, d_buf.data_ptr(), d_offs.data_ptr(), n, len(buf), d_out.data_ptr(),
                                                d_ch.data_ptr(), total, d_co.data_ptr(), d_st.data_ptr(),
                                                stream_ptr=stream.cuda_stream)
                e1.record(stream)
                stream.synchronize()
                t.append(e0.elapsed_time(e1))
            row["device_events"] = stats(t[3:])
            st = d_st.cpu().numpy().view(cld_amd.VEC_STATUS_DTYPE)[0]
            assert int(st["total_chunks"]) == total and int(st["failed_docs"]) == 0
            assert np.array_equal(d_co.cpu().numpy().view(np.uint64), coffs)
            assert d_ch.cpu().numpy()[:total * 12].tobytes() == chunks.tobytes()
            assert d_out.cpu().numpy().tobytes() == res.tobytes()
            row["equal_to_host"] = True
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
