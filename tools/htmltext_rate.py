"""The time of cld_html_text_device -- with and without d_pos, with and without CLD_HTMLTEXT_BLOCK_LF -- on
pages of about 16 KB in the style of corpus.html, resident in HBM; beside it cld_gather_docs_device copying
the same bytes (the copy floor: every byte read once and written once) and the whole HTML-mode detection of
the same pages (cld_detect_batch_device_hints with CLD_FLAG_HTML), of which the private rewrite is the first
step.  251 distinct pages repeated to the batch size (a prime, so that a wave striding over the batch meets
them all).  HIP events on a torch stream, 10 warm-up calls, then the median, minimum and maximum of 30 (the
detection: 2 and 5).  Prints one JSON line.
usage: htmltext_rate.py [pages]"""
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
PAGES = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
DISTINCT = 251                 # a prime: the grid strides over the pages by a multiple of 256
LF = cld_amd.HTMLTEXT_BLOCK_LF

one, o = corpus.html(DISTINCT, seed=0xC1D20016, lo=16000, hi=16768, emoji=0.25)
one, lens = np.asarray(one, np.uint8), np.diff(np.asarray(o, np.int64))
reps = -(-PAGES // DISTINCT)
offs = np.concatenate([[0], np.cumsum(np.tile(lens, reps))])[:PAGES + 1].astype(np.uint64)
nb = int(offs[-1])

up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
z = lambda k: torch.zeros(max(k, 1), dtype=torch.uint8, device=dev)
d_buf = up(one).repeat(reps)[:nb].contiguous()
d_offs = up(offs)
n = PAGES
s = torch.cuda.Stream()
d_out, d_pos, d_tl, d_st = z(nb), z(4 * nb), z(4 * n), z(24)


def timed(f, warm=10, reps=30):
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


r = {"pages": n, "bytes": nb, "mean_page_bytes": nb / n}
for flags in (0, LF):
    for pos in (False, True):
        def text():
            cld_amd.html_text_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_out.data_ptr(), flags=flags,
                                     d_text_len_ptr=d_tl.data_ptr(), d_pos_ptr=d_pos.data_ptr() if pos else None,
                                     d_status_ptr=d_st.data_ptr(), stream_ptr=s.cuda_stream)
        r["text_f%d_%s_ms_median_min_max" % (flags, "pos" if pos else "nopos")] = timed(text)
st = d_st.cpu().numpy().view(cld_amd.HTMLTEXT_STATUS_DTYPE)[0]
r.update({f: int(st[f]) for f in ("text_bytes", "tags", "entities", "dropped")})

idx = up(np.arange(n, dtype=np.uint32))
gwb = cld_amd.group_work_bytes(n)
gw, oo = z(gwb), z((n + 1) * 8)


def gather():
    cld_amd.gather_docs_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, idx.data_ptr(), n, d_out.data_ptr(), nb,
                               oo.data_ptr(), gw.data_ptr(), gwb, stream_ptr=s.cuda_stream)


r["gather_docs_ms_median_min_max"] = timed(gather)
for k in ("text_f0_nopos", "text_f1_nopos", "text_f0_pos", "text_f1_pos"):
    r[k + "_over_gather_time"] = r[k + "_ms_median_min_max"][0] / r["gather_docs_ms_median_min_max"][0]

d_res = z(n * 40)


def detect_html():
    cld_amd.detect_batch_device_hints(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_res.data_ptr(), flags=cld_amd.FLAG_HTML,
                                      stream_ptr=s.cuda_stream)


r["detect_html_ms_median_min_max"] = timed(detect_html, warm=2, reps=5)
print(json.dumps(r))
