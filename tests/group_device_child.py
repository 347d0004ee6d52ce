"""Child process of test_gpu_group.py: torch initialises the GPU first (the
library then shares its HIP runtime, as in bench.py), the inputs go to HBM as
torch tensors and the device entries run on them.

argv: mode, input .npz, output .npz.
  group   cld_group_by_language_device on every case <k> of the input (res<k>: the
          results as bytes, offs<k>, flags<k>: the flag sets to run).  Every output
          starts as PATTERN and has GUARD words either side; the workspace starts as
          garbage; d_results is compared before and after.  On the case named by
          `variants`: a torch stream, each optional output left out, the same call
          twice, a workspace one byte short, and n == 0.
  gather  cld_gather_docs_device on <buf, offs> with every index set idx_<name> and
          the capacities caps_<name>; source and output five bytes off a 256-byte
          boundary.
  e2e     cld_detect_batch_device on <buf, offs>, the group entry on the device
          results, a gather for every bin that is not empty, and
          cld_detect_batch_device on each gathered batch."""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
import cld_amd  # noqa: E402

cld_amd.init_device(0)
dev = torch.device("cuda", 0)
mode = sys.argv[1]
inp = np.load(sys.argv[2])
out = {}
GUARD = 64                     # words either side of a group output, of an offsets array
BGUARD = 256                   # bytes either side of a gathered buffer
PATTERN = 0x5A
BINS = cld_amd.GROUP_BINS


def filled(nbytes):
    return torch.full((max(nbytes, 1),), PATTERN, dtype=torch.uint8, device=dev)


def upload(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


class Guarded:
    """count words of `size` bytes in HBM between two guards, all PATTERN."""

    def __init__(self, count, size):
        self.count, self.size = count, size
        self.t = filled((count + 2 * GUARD) * size)
        self.ptr = self.t.data_ptr() + GUARD * size

    def get(self, what):
        """The words as numpy; the guards must be intact."""
        h = self.t.cpu().numpy()
        lo, hi = GUARD * self.size, (GUARD + self.count) * self.size
        assert (h[:lo] == PATTERN).all() and (h[hi:hi + GUARD * self.size] == PATTERN).all(), what + ": a guard was written"
        return h[lo:hi].view({4: np.uint32, 8: np.uint64}[self.size]).copy()

    def untouched(self):
        return bool((self.t == PATTERN).all())


def work(nbytes):
    return torch.full((max(nbytes, 8),), 0xC3, dtype=torch.uint8, device=dev)


if mode == "group":
    def run(d_res, d_offs, n, flags, skip=(), stream=None, short=0):
        o = {"counts": Guarded(BINS, 8), "bin_bytes": Guarded(BINS, 8), "order": Guarded(n, 4),
             "group_offsets": Guarded(BINS + 1, 8)}
        wb = cld_amd.group_work_bytes(n) - short
        w = work(wb)
        before = d_res.clone()
        torch.cuda.synchronize()             # (torch filled the tensors on its own stream, not the library's)
        p = {k: (None if k in skip else v.ptr) for k, v in o.items()}
        cld_amd.group_by_language_device(0, d_res.data_ptr(), n, p["counts"], w.data_ptr(), wb, flags=flags,
                                         d_offsets_ptr=d_offs.data_ptr(), d_bin_bytes_ptr=p["bin_bytes"],
                                         d_order_ptr=p["order"], d_group_offsets_ptr=p["group_offsets"], stream_ptr=stream)
        torch.cuda.synchronize()
        assert torch.equal(d_res, before), "d_results was written"
        for k in skip:
            assert o[k].untouched(), "%s was written though it was left out" % k
        return {k: v.get(k) for k, v in o.items() if k not in skip}, o

    for k in range(int(inp["cases"])):
        res, offs = inp["res%d" % k], inp["offs%d" % k]
        n = len(offs) - 1
        d_res, d_offs = upload(res), upload(offs)
        for flags in inp["flags%d" % k]:
            got, _ = run(d_res, d_offs, n, int(flags))
            for f, v in got.items():
                out["c%d_f%d_%s" % (k, flags, f)] = v
        if k == int(inp["variants"]):
            s = torch.cuda.Stream()
            got, _ = run(d_res, d_offs, n, 0, stream=s.cuda_stream)
            for f, v in got.items():
                out["stream_" + f] = v
            for skip in ("bin_bytes", "order", "group_offsets"):
                got, _ = run(d_res, d_offs, n, 0, skip=(skip,))
                for f, v in got.items():
                    out["no_%s_%s" % (skip, f)] = v
            got, _ = run(d_res, d_offs, n, 0, skip=("bin_bytes", "order", "group_offsets"))
            out["only_counts"] = got["counts"]
            out["again_order"] = run(d_res, d_offs, n, 0)[0]["order"]
            try:
                run(d_res, d_offs, n, 0, short=1)
                out["short_rc"] = np.array(0)
            except cld_amd.CldError as e:
                out["short_rc"] = np.array(int(str(e).rsplit(":", 1)[1]))
            # (run() has checked nothing: it raised before; the outputs of a fresh call must stay PATTERN)
            o = {"counts": Guarded(BINS, 8), "order": Guarded(n, 4)}
            w = work(8)
            torch.cuda.synchronize()
            rc = cld_amd.lib().cld_group_by_language_device(0, d_res.data_ptr(), n, 0, None, o["counts"].ptr, None,
                                                            o["order"].ptr, None, w.data_ptr(),
                                                            cld_amd.group_work_bytes(n) - 1, None)
            torch.cuda.synchronize()
            out["short_rc2"] = np.array(rc)
            out["short_untouched"] = np.array(all(v.untouched() for v in o.values()) and bool((w == 0xC3).all()))
    z = {"counts": Guarded(BINS, 8), "bin_bytes": Guarded(BINS, 8), "group_offsets": Guarded(BINS + 1, 8)}
    d_offs = upload(np.zeros(1, np.uint64))  # (the byte totals are asked for: the offsets of no documents)
    torch.cuda.synchronize()
    cld_amd.group_by_language_device(0, None, 0, z["counts"].ptr, None, 0, d_offsets_ptr=d_offs.data_ptr(),
                                     d_bin_bytes_ptr=z["bin_bytes"].ptr, d_group_offsets_ptr=z["group_offsets"].ptr)
    torch.cuda.synchronize()
    for k, v in z.items():
        out["empty_" + k] = v.get("n == 0 " + k)
    cld_amd.group_by_language_device(0, None, 0, None, None, 0)

elif mode == "gather":
    buf, offs = inp["buf"], inp["offs"]
    n_src, nb = len(offs) - 1, len(buf)
    d_in = filled(nb + 512)
    d_in[5:5 + nb] = torch.from_numpy(buf).to(dev)
    d_offs = upload(offs)
    before = d_in.clone()
    for name in [k[4:] for k in inp.files if k.startswith("idx_")]:
        idx = inp["idx_" + name]
        m = len(idx)
        d_idx = upload(idx) if m else filled(4)
        wb = cld_amd.group_work_bytes(m)
        for cap in inp["caps_" + name]:
            cap = int(cap)
            total = int(inp["total_" + name])
            d_o = filled(total + 2 * BGUARD + 512)
            assert d_in.data_ptr() % 256 == 0 and d_o.data_ptr() % 256 == 0
            oo = Guarded(m + 1, 8)
            w = work(wb)
            torch.cuda.synchronize()
            lo = BGUARD + 5
            sizing = cap < 0                                   # (-1 in the input: out_cap 0 and no buffer)
            cld_amd.gather_docs_device(0, d_in.data_ptr() + 5, d_offs.data_ptr(), n_src, d_idx.data_ptr(), m,
                                       None if sizing else d_o.data_ptr() + lo, 0 if sizing else cap, oo.ptr,
                                       w.data_ptr(), wb)
            torch.cuda.synchronize()
            h = d_o.cpu().numpy()
            hi = lo + (0 if sizing else min(cap, total))
            what = "%s, capacity %d" % (name, cap)
            assert (h[:lo] == PATTERN).all() and (h[hi:] == PATTERN).all(), what + ": bytes outside the capacity were written"
            out["%s_%d_buf" % (name, cap)] = h[lo:hi]
            out["%s_%d_offs" % (name, cap)] = oo.get(what)
    assert torch.equal(d_in, before), "the source was written"
    oo = Guarded(1, 8)
    torch.cuda.synchronize()
    cld_amd.gather_docs_device(0, None, None, 0, None, 0, None, 0, oo.ptr, None, 0)
    torch.cuda.synchronize()
    out["empty_offs"] = oo.get("m == 0")

else:
    buf, offs = inp["buf"], inp["offs"]
    n, nb = len(offs) - 1, len(buf)
    d_buf, d_offs = upload(buf), upload(offs)
    d_res = filled(n * 40)
    torch.cuda.synchronize()
    cld_amd.detect_batch_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_res.data_ptr())
    o = {"counts": Guarded(BINS, 8), "bin_bytes": Guarded(BINS, 8), "order": Guarded(n, 4),
         "group_offsets": Guarded(BINS + 1, 8)}
    wb = cld_amd.group_work_bytes(n)
    w = work(wb)
    torch.cuda.synchronize()
    # the library's own stream carries the detection and the group: no host wait in between
    cld_amd.group_by_language_device(0, d_res.data_ptr(), n, o["counts"].ptr, w.data_ptr(), wb,
                                     d_offsets_ptr=d_offs.data_ptr(), d_bin_bytes_ptr=o["bin_bytes"].ptr,
                                     d_order_ptr=o["order"].ptr, d_group_offsets_ptr=o["group_offsets"].ptr)
    torch.cuda.synchronize()
    out["results"] = d_res.cpu().numpy()[:n * 40]
    h = {k: v.get(k) for k, v in o.items()}
    out.update(h)
    for b in np.nonzero(h["counts"])[0]:
        m, at, nbytes = int(h["counts"][b]), int(h["group_offsets"][b]), int(h["bin_bytes"][b])
        d_o = filled(nbytes + 2 * BGUARD)
        oo = Guarded(m + 1, 8)
        d_r = filled(m * 40)
        torch.cuda.synchronize()
        cld_amd.gather_docs_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, o["order"].ptr + 4 * at, m,
                                   d_o.data_ptr() + BGUARD, nbytes, oo.ptr, w.data_ptr(), wb)
        cld_amd.detect_batch_device(0, d_o.data_ptr() + BGUARD, oo.ptr, m, d_r.data_ptr())
        torch.cuda.synchronize()
        g = d_o.cpu().numpy()
        assert (g[:BGUARD] == PATTERN).all() and (g[BGUARD + nbytes:] == PATTERN).all(), "bin %d: guard bytes written" % b
        out["bin%d_buf" % b] = g[BGUARD:BGUARD + nbytes]
        out["bin%d_offs" % b] = oo.get("bin %d" % b)
        out["bin%d_results" % b] = d_r.cpu().numpy()[:m * 40]

np.savez(sys.argv[3], **out)
