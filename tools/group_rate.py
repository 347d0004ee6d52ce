"""Times of cld_group_by_language_device and cld_gather_docs_device beside their
yardsticks (GPU box).  One JSON line per corpus and measure, also written to
profiles/group_rate.jsonl.

The corpora are the 1 M tweets of C2 and the 100 K pages of C3, detected on the
device first (cld_detect_batch_device); everything timed runs on results and
text that are already in HBM.  Times are HIP-event times on one stream, after
a warm-up, per call: the median of --reps calls with the fastest and the
slowest beside it.  Ours and the yardstick alternate call by call, so both see
the same card state.

  group    ours (counts, byte totals, order and group offsets in one call)
           beside torch.sort(keys, stable=True) + torch.bincount(keys, minlength=615)
           on the key tensor of the same results (extracted beforehand, not
           timed), for int16, int32 and int64 keys.  The outputs are compared.
  gather   the largest language's documents (a slice of d_order), and every
           document in language order, beside a device-to-device copy of the
           same byte count (the ceiling) and beside what a caller does without
           the entries: download the results, group and select on the host
           with numpy, upload the selection (host clock around a synchronise).

    python tools/group_rate.py [--reps N] [--small] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("language-detector_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
torch.cuda.set_device(0)
import cld_amd  # noqa: E402
import corpus  # noqa: E402

BINS = cld_amd.GROUP_BINS
dev = torch.device("cuda", 0)


def timed(fn, stream, inner):
    """`inner` calls of fn between two events on the stream -> ms per call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(inner):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, reps, stream, warmup=5, inner=1):
    """{name: fn} -> {name: [ms per call] * reps}, the functions in turn within every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, stream, inner))
    return t


def stats(row, label, ms):
    ms = np.asarray(ms)
    row.update({label + "_ms": round(float(np.median(ms)), 4), label + "_ms_min": round(float(ms.min()), 4),
                label + "_ms_max": round(float(ms.max()), 4)})
    return float(np.median(ms))


def host_select(buf, offs, sel):
    """The selected documents packed, by numpy: one index array for short documents, slices for pages."""
    lens = (offs[sel + 1] - offs[sel]).astype(np.int64)
    out_offs = np.zeros(len(sel) + 1, np.int64)
    np.cumsum(lens, out=out_offs[1:])
    if len(sel) and out_offs[-1] // len(sel) >= 1024:
        o = offs.astype(np.int64)
        return np.concatenate([buf[o[i]:o[i + 1]] for i in sel]), out_offs.astype(np.uint64)
    src = np.repeat(offs[sel].astype(np.int64) - out_offs[:-1], lens) + np.arange(out_offs[-1])
    return buf[src], out_offs.astype(np.uint64)


def measure(name, buf, offs, reps, lines):
    n, nb = len(offs) - 1, len(buf)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    d_buf = torch.from_numpy(buf).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_res = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cld_amd.detect_batch_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_res.data_ptr(), sp)
    torch.cuda.synchronize()

    # ---- group
    wb = cld_amd.group_work_bytes(n)
    d_work = torch.empty(wb, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(BINS, dtype=torch.int64, device=dev)
    d_bytes = torch.zeros(BINS, dtype=torch.int64, device=dev)
    d_goffs = torch.zeros(BINS + 1, dtype=torch.int64, device=dev)
    d_order = torch.zeros(n, dtype=torch.int32, device=dev)

    def ours():
        cld_amd.group_by_language_device(0, d_res.data_ptr(), n, d_counts.data_ptr(), d_work.data_ptr(), wb,
                                         d_offsets_ptr=d_offs.data_ptr(), d_bin_bytes_ptr=d_bytes.data_ptr(),
                                         d_order_ptr=d_order.data_ptr(), d_group_offsets_ptr=d_goffs.data_ptr(),
                                         stream_ptr=sp)

    keys16 = d_res.view(torch.int16).view(n, 20)[:, 3].clone()                # summary_lang (< 614 in these corpora)
    keys16.clamp_(max=cld_amd.NUM_LANGUAGES)
    keys = {"int16": keys16, "int32": keys16.to(torch.int32), "int64": keys16.to(torch.int64)}
    assert int(keys16.min()) >= 0
    for k in list(keys):                                                      # (a key type torch has no kernel for is left out)
        try:
            torch.bincount(keys[k], minlength=BINS), torch.sort(keys[k], stable=True)
        except RuntimeError as e:
            print("torch on %s keys: %s" % (k, str(e).splitlines()[0]), flush=True)
            del keys[k]
    theirs = {}

    def torch_pair(k):
        def f():
            theirs[k] = (torch.sort(keys[k], stable=True)[1], torch.bincount(keys[k], minlength=BINS))
        return f

    fns = {"ours": ours}
    fns.update({"torch_" + k: torch_pair(k) for k in keys})
    t = alternate(fns, reps, stream, inner=10)
    torch.cuda.synchronize()
    for k, (order, counts) in theirs.items():
        assert torch.equal(order.to(torch.int32), d_order) and torch.equal(counts, d_counts), "group differs from torch (%s)" % k
    row = {"measure": "group", "corpus": name, "docs": n, "bytes": nb, "reps": reps, "calls_per_rep": 10,
           "languages": int((d_counts > 0).sum()), "work_bytes": wb}
    m = stats(row, "ours", t["ours"])
    best = min(stats(row, "torch_sort_bincount_" + k, t["torch_" + k]) for k in keys)
    row["ours_over_fastest_torch"] = round(m / best, 3)
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)

    # ---- gather
    counts, goffs, bin_bytes = (x.cpu().numpy().astype(np.int64) for x in (d_counts, d_goffs, d_bytes))
    big = int(np.argmax(bin_bytes))
    for what, at, m_docs, total in (("largest_language", int(goffs[big]), int(counts[big]), int(bin_bytes[big])),
                                    ("every_document_by_language", 0, n, nb)):
        d_out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        d_oo = torch.zeros(m_docs + 1, dtype=torch.int64, device=dev)
        d_src = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        gw = cld_amd.group_work_bytes(m_docs)

        def gather():
            cld_amd.gather_docs_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_order.data_ptr() + 4 * at, m_docs,
                                       d_out.data_ptr(), total, d_oo.data_ptr(), d_work.data_ptr(), gw, stream_ptr=sp)

        def copy():
            d_src.copy_(d_out)

        t = alternate({"gather": gather, "copy": copy}, reps, stream)
        torch.cuda.synchronize()
        assert int(d_oo[m_docs]) == total

        # what a caller does without the entries (the text is still on the host)
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = d_res.cpu().numpy().view(cld_amd.RESULT_DTYPE)
            bins = np.minimum(res["summary_lang"], cld_amd.NUM_LANGUAGES)
            sel = np.argsort(bins, kind="stable") if m_docs == n else np.nonzero(bins == big)[0]
            sbuf, soffs = host_select(buf, offs, sel)
            d_sel, d_soffs = torch.from_numpy(sbuf).to(dev), torch.from_numpy(soffs.view(np.int64)).to(dev)
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(d_sel, d_out[:total]) and torch.equal(d_soffs, d_oo), "gather differs from the host's selection"
        row = {"measure": "gather", "corpus": name, "selection": what, "docs": m_docs, "bytes": total, "reps": reps}
        g = stats(row, "ours", t["gather"])
        c = stats(row, "device_copy", t["copy"])
        h = stats(row, "host_download_select_upload", host_ms)
        row.update({"ours_over_device_copy": round(g / c, 2), "host_over_ours": round(h / g, 1),
                    "ours_gb_per_s": round(total / g / 1e6, 1), "device_copy_gb_per_s": round(total / c / 1e6, 1)})
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del d_out, d_src, d_oo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--small", action="store_true", help="a hundredth of the sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_rate.jsonl"))
    a = ap.parse_args()
    cld_amd.init_device(0, tables=cld_amd.SYNTH_TABLES)
    lines = []
    side = torch.cuda.Stream()                # (not the default stream: the entries take NULL for the runtime's own)
    for name, n in (("c2", 1_000_000), ("c3", 100_000)):
        buf, offs = corpus.GENERATORS[name](n // 100 if a.small else n)
        with torch.cuda.stream(side):
            measure(name, np.ascontiguousarray(buf), np.ascontiguousarray(offs, dtype=np.uint64), a.reps, lines)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
