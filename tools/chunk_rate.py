"""The copy rate of cld_gather_chunks_device (all bins selected) beside cld_gather_docs_device packing the
same number of output bytes (the leading documents whose bytes add up to at most the pieces' total: all
of them where the vectors tile their pages), on one resident batch of C3-like pages: HIP events on a torch stream, 10 warm-up calls,
then the median, minimum and maximum of 50.  Prints one JSON line.  usage: chunk_rate.py [pages]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "language-detector_amd"))
os.environ.setdefault("CLD_MI355X_TABLES", os.path.join(ROOT, "language-detector_amd", "data", "cld2_synth_q1.cldt"))
torch.cuda.set_device(0)
import cld_amd  # noqa: E402
import corpus  # noqa: E402

cld_amd.init_device(0)
dev = torch.device("cuda", 0)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
buf, offs = corpus.GENERATORS["c3"](N)
buf, offs = np.asarray(buf, np.uint8), np.asarray(offs, np.uint64)
n, nb = len(offs) - 1, len(buf)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
z = lambda k: torch.zeros(max(k, 1), dtype=torch.uint8, device=dev)
d_buf, d_offs = up(buf), up(offs)
d_res, d_coffs, d_st = z(n * 40), z((n + 1) * 8), z(16)
torch.cuda.synchronize()
cld_amd.detect_batch_device_vec(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_res.data_ptr(), None, 0, d_coffs.data_ptr(),
                                d_st.data_ptr())
torch.cuda.synchronize()
cap = int(d_st.cpu().numpy().view(cld_amd.VEC_STATUS_DTYPE)["total_chunks"][0])
d_chunks = z(cap * 12)
cld_amd.detect_batch_device_vec(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_res.data_ptr(), d_chunks.data_ptr(), cap,
                                d_coffs.data_ptr(), d_st.data_ptr())
torch.cuda.synchronize()
sel = up(np.ones(cld_amd.GROUP_BINS, np.uint8))
wb = cld_amd.chunk_work_bytes(n, cap)
w = z(wb)
oo = z((n + 1) * 8)
s = torch.cuda.Stream()
cld_amd.gather_chunks_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_chunks.data_ptr(), cap, d_coffs.data_ptr(),
                             sel.data_ptr(), None, 0, oo.data_ptr(), w.data_ptr(), wb, stream_ptr=s.cuda_stream)
torch.cuda.synchronize()
total = int(oo.cpu().numpy().view(np.uint64)[-1])
d_out = z(total)
m = int(np.searchsorted(offs, np.uint64(total), side="right")) - 1      # documents 0..m hold at most `total` bytes
docs_bytes = int(offs[m])
idx = up(np.arange(m, dtype=np.uint32))
gwb = cld_amd.group_work_bytes(m)
gw = z(gwb)
d_out2 = z(docs_bytes)
oo2 = z((m + 1) * 8)


def chunks_call():
    cld_amd.gather_chunks_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_chunks.data_ptr(), cap, d_coffs.data_ptr(),
                                 sel.data_ptr(), d_out.data_ptr(), total, oo.data_ptr(), w.data_ptr(), wb,
                                 stream_ptr=s.cuda_stream)


def docs_call():
    cld_amd.gather_docs_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, idx.data_ptr(), m, d_out2.data_ptr(), docs_bytes,
                               oo2.data_ptr(), gw.data_ptr(), gwb, stream_ptr=s.cuda_stream)


def timed(f, warm=10, reps=50):
    for _ in range(warm):
        f()
    s.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        f()
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


tc, td = timed(chunks_call), timed(docs_call)
r = {"pages": n, "input_bytes": nb, "chunks": cap, "chunks_out_bytes": total, "docs_gathered": m, "docs_out_bytes": docs_bytes,
     "gather_chunks_ms_median_min_max": tc, "gather_docs_ms_median_min_max": td,
     "gather_chunks_GBps": total / tc[0] / 1e6, "gather_docs_GBps": docs_bytes / td[0] / 1e6}
r["ratio_chunks_over_docs_rate"] = r["gather_chunks_GBps"] / r["gather_docs_GBps"]
r["ratio_chunks_over_docs_time"] = tc[0] / td[0]
print(json.dumps(r))
