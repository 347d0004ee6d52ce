"""The time of cld_split_lines_device (both flag values) beside cld_gather_docs_device packing the same
bytes -- both read every byte of the text once -- on two resident batches over one buffer: pages of about
16 KB made of LF-joined corpus.c2 tweets, and the same tweets as documents of about 100 bytes.  Then, for
the pages, the two ways to per-part languages side by side: split -> cld_detect_batch_device on the lines,
and cld_detect_batch_device_vec on the pages (they answer different questions: a line's own result against
a slice of the page's result).  HIP events on a torch stream, 10 warm-up calls, then the median, minimum
and maximum of 50 (the two detections: 3 and 9).  Prints one JSON line.  usage: line_rate.py [pages]"""
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
PAGES = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
PAGE = 16384
JOIN = cld_amd.LINES_JOIN_BLANK

# 65536 distinct tweets, each with an LF behind it, repeated until the pages are full
tb, to = corpus.GENERATORS["c2"](65536)
tb, to = np.asarray(tb, np.uint8), np.asarray(to, np.int64)
assert not (tb == 0x0A).any()
lens = np.diff(to) + 1
one = np.zeros(int(lens.sum()), np.uint8)
ends = np.cumsum(lens)
keep = np.ones(len(one), bool)
keep[ends - 1] = False
one[keep] = tb
one[ends - 1] = 0x0A
per_page = int(round(PAGE / lens.mean()))
tweets = PAGES * per_page
reps = -(-tweets // len(lens))
buf = np.tile(one, reps)
t_offs = np.concatenate([[0], np.cumsum(np.tile(lens, reps))])[:tweets + 1].astype(np.uint64)
buf = buf[:int(t_offs[-1])]
p_offs = t_offs[::per_page].copy()
nb = len(buf)
assert len(p_offs) == PAGES + 1 and int(p_offs[-1]) == nb

up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
z = lambda k: torch.zeros(max(k, 1), dtype=torch.uint8, device=dev)
d_buf = up(buf)
s = torch.cuda.Stream()
batches = {"pages": (up(p_offs), PAGES), "tweets": (up(t_offs), tweets)}
d_lo, d_ld, d_st = z((tweets + 1) * 8), z(tweets * 4), z(16)
wb = cld_amd.lines_work_bytes(tweets, nb)
w = z(wb)
d_out = z(nb)


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


r = {"pages": PAGES, "tweets": tweets, "bytes": nb, "workspace_bytes": wb}
for name, (d_offs, n) in batches.items():
    d_dl = z((n + 1) * 8)
    for flags in (0, JOIN):
        def split():
            cld_amd.split_lines_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_lo.data_ptr(), d_ld.data_ptr(), tweets,
                                       d_dl.data_ptr(), w.data_ptr(), wb, flags=flags, d_status_ptr=d_st.data_ptr(),
                                       stream_ptr=s.cuda_stream)
        r["%s_split_f%d_ms_median_min_max" % (name, flags)] = timed(split)
        st = d_st.cpu().numpy().view(cld_amd.LINES_STATUS_DTYPE)[0]
        r["%s_lines_f%d" % (name, flags)] = int(st["total_lines"])
        assert int(st["total_lines"]) == tweets                  # (every line holds a tweet: the flag drops nothing)
    idx = up(np.arange(n, dtype=np.uint32))
    gwb = cld_amd.group_work_bytes(n)
    gw, oo = z(gwb), z((n + 1) * 8)

    def gather():
        cld_amd.gather_docs_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, idx.data_ptr(), n, d_out.data_ptr(), nb,
                                   oo.data_ptr(), gw.data_ptr(), gwb, stream_ptr=s.cuda_stream)
    r["%s_gather_docs_ms_median_min_max" % name] = timed(gather)
    r["%s_split_over_gather_time" % name] = r["%s_split_f0_ms_median_min_max" % name][0] / \
        r["%s_gather_docs_ms_median_min_max" % name][0]

# the two ways to per-part languages of the pages
d_offs, n = batches["pages"]
d_dl, d_res = z((n + 1) * 8), z(tweets * 40)


def split_detect():
    cld_amd.split_lines_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_lo.data_ptr(), d_ld.data_ptr(), tweets,
                               d_dl.data_ptr(), w.data_ptr(), wb, flags=JOIN, stream_ptr=s.cuda_stream)
    cld_amd.detect_batch_device(0, d_buf.data_ptr(), d_lo.data_ptr(), tweets, d_res.data_ptr(), stream_ptr=s.cuda_stream)


r["pages_split_detect_lines_ms_median_min_max"] = timed(split_detect, warm=3, reps=9)
d_pres, d_coffs, d_vst = z(n * 40), z((n + 1) * 8), z(16)
cld_amd.detect_batch_device_vec(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_pres.data_ptr(), None, 0, d_coffs.data_ptr(),
                                d_vst.data_ptr(), stream_ptr=s.cuda_stream)
s.synchronize()
cap = int(d_vst.cpu().numpy().view(cld_amd.VEC_STATUS_DTYPE)["total_chunks"][0])
d_chunks = z(cap * 12)


def vec():
    cld_amd.detect_batch_device_vec(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_pres.data_ptr(), d_chunks.data_ptr(), cap,
                                    d_coffs.data_ptr(), d_vst.data_ptr(), stream_ptr=s.cuda_stream)


r["pages_detect_vec_ms_median_min_max"] = timed(vec, warm=3, reps=9)
r["pages_vec_chunks"] = cap
print(json.dumps(r))
