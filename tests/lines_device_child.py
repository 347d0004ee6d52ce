"""Child process of test_gpu_lines.py: torch initialises the GPU first (the
library then shares its HIP runtime, as in bench.py), the inputs go to HBM as
torch tensors and the line device entries run on them.

argv: mode, input .npz, output .npz.
  cases   every case <k> of the input (buf<k>, offs<k>, res<k> as bytes: one result per
          line, gflags<k>, hostile<k>): one cld_split_lines_device per row of runs<k> =
          (flags, line_cap or -1 for the sizing pass, the alignment 0..15 of d_buf +
          offsets[0], line_doc wanted, status wanted) -> r<k>_<row>_lo / _ld / _dl / _st,
          then cld_lines_to_chunks_device on what it wrote (_ch) where there is a
          line_doc.  The buffer sits between guard bytes, buf_bytes is its exact length;
          every output starts as PATTERN between guards and must still be PATTERN past
          the extents the contract names, the workspace starts as garbage; every input
          is compared before and after.  A hostile case is only run: guards and rc.  On
          the case named by `variants`: a torch stream, the same call twice, a workspace
          one byte short, and n == 0.
  e2e     split with CLD_LINES_JOIN_BLANK (sizing pass, then with room),
          cld_detect_batch_device on the line batch, cld_lines_to_chunks_device, the
          chunk totals and a gather for the four bins with the most bytes, and
          cld_group_by_language_device over the line results with the line offsets."""
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
GUARD = 64                     # words either side of an array of words
BGUARD = 256                   # bytes either side of the text
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

    def get(self, what, written=None):
        """The words as numpy; the guards, and the words from `written` on, must be intact."""
        h = self.t.cpu().numpy()
        lo, hi = GUARD * self.size, (GUARD + self.count) * self.size
        assert (h[:lo] == PATTERN).all() and (h[hi:hi + GUARD * self.size] == PATTERN).all(), what + ": a guard was written"
        if written is not None:
            assert (h[lo + written * self.size:hi] == PATTERN).all(), what + ": words past the extent were written"
        return h[lo:hi].view({4: np.uint32, 8: np.uint64}[self.size]).copy()

    def untouched(self):
        return bool((self.t == PATTERN).all())


def work(nbytes):
    return torch.full((max(nbytes, 8),), 0xC3, dtype=torch.uint8, device=dev)


class Batch:
    """A batch in HBM, d_buf + offsets[0] at a chosen alignment."""

    def __init__(self, buf, offs):
        self.n, self.nb = len(offs) - 1, len(buf)
        self.buf, self.offs0 = np.ascontiguousarray(buf), int(offs[0])
        self.d_offs = upload(offs)
        self.wb = cld_amd.lines_work_bytes(self.n, self.nb)
        self.place(0)

    def place(self, align):
        self.d_in = filled(self.nb + 2 * BGUARD + 32)
        assert self.d_in.data_ptr() % 256 == 0
        self.lo = BGUARD + (align - self.offs0) % 16
        if self.nb:
            self.d_in[self.lo:self.lo + self.nb] = torch.from_numpy(self.buf).to(dev)
        self.ptr = self.d_in.data_ptr() + self.lo
        assert (self.ptr + self.offs0) % 16 == align
        self.before = [self.d_in.clone(), self.d_offs.clone()]

    def unchanged(self):
        return torch.equal(self.d_in, self.before[0]) and torch.equal(self.d_offs, self.before[1])

    def split(self, flags, cap, align, want_doc=True, want_status=True, stream=None, hostile=False, what=""):
        """-> dict of lo, ld, dl, st (those that were asked for) and the device arrays for the chunk step."""
        self.place(align)
        sizing = cap < 0
        g = {"dl": Guarded(self.n + 1, 8)}
        if not sizing:
            g["lo"] = Guarded(cap + 1, 8)
            if want_doc:
                g["ld"] = Guarded(cap, 4)
        if want_status:
            g["st"] = Guarded(2, 8)
        w = work(self.wb)
        torch.cuda.synchronize()             # (torch filled the tensors on its own stream, not the library's)
        cld_amd.split_lines_device(0, self.ptr, self.d_offs.data_ptr(), self.n, self.nb, g["lo"].ptr if "lo" in g else None,
                                   g["ld"].ptr if "ld" in g else None, 0 if sizing else cap, g["dl"].ptr, w.data_ptr(),
                                   self.wb, flags=flags, d_status_ptr=g["st"].ptr if "st" in g else None, stream_ptr=stream)
        torch.cuda.synchronize()
        got = {"dl": g["dl"].get(what + " doc_lines")}
        k = None if hostile or sizing else min(int(got["dl"][self.n]), cap)
        if "lo" in g:
            got["lo"] = g["lo"].get(what + " line_offsets", None if hostile else k + 1)
        if "ld" in g:
            got["ld"] = g["ld"].get(what + " line_doc", k)
        if "st" in g:
            got["st"] = g["st"].get(what + " status")
        assert self.unchanged(), what + ": an input was written"
        return got, g

    def chunks(self, g, cap, res, gflags, m, what):
        d_res = filled(cap * 40)
        k = min(m, cap)
        if k:
            d_res[:k * 40] = upload(res[:k])
        ch = Guarded(cap * 3, 4)
        torch.cuda.synchronize()
        cld_amd.lines_to_chunks_device(0, d_res.data_ptr(), g["lo"].ptr, g["ld"].ptr, cap, self.d_offs.data_ptr(), self.n,
                                       g["dl"].ptr, ch.ptr, flags=gflags)
        torch.cuda.synchronize()
        return ch.get(what + " chunks", k * 3)[:k * 3]


if mode == "cases":
    for k in range(int(inp["cases"])):
        b = Batch(inp["buf%d" % k], inp["offs%d" % k])
        hostile = bool(inp["hostile%d" % k])
        res = inp["res%d" % k].view(cld_amd.RESULT_DTYPE)
        gflags = int(inp["gflags%d" % k])
        runs = [tuple(int(x) for x in row) for row in inp["runs%d" % k]]
        for r, (flags, cap, align, want_doc, want_status) in enumerate(runs):
            what = "case %d, run %d" % (k, r)
            got, g = b.split(flags, cap, align, bool(want_doc), bool(want_status), hostile=hostile, what=what)
            for f, v in got.items():
                out["r%d_%d_%s" % (k, r, f)] = v
            if "ld" in g and not hostile:
                out["r%d_%d_ch" % (k, r)] = b.chunks(g, cap, res, gflags, int(got["dl"][b.n]), what)
        if k == int(inp["variants"]):
            flags, cap, align, _, _ = runs[0]
            s = torch.cuda.Stream()
            got, _ = b.split(flags, cap, align, stream=s.cuda_stream, what="on a torch stream")
            for f, v in got.items():
                out["stream_" + f] = v
            got, _ = b.split(flags, cap, align, what="again")
            for f, v in got.items():
                out["again_" + f] = v
            # a workspace one byte short: CLD_ENOSPC and nothing written, not even to the workspace
            o = {"lo": Guarded(cap + 1, 8), "ld": Guarded(cap, 4), "dl": Guarded(b.n + 1, 8), "st": Guarded(2, 8)}
            w = work(b.wb)
            torch.cuda.synchronize()
            out["short_rc"] = np.array(cld_amd.lib().cld_split_lines_device(
                0, b.ptr, b.d_offs.data_ptr(), b.n, b.nb, flags, o["lo"].ptr, o["ld"].ptr, cap, o["dl"].ptr, o["st"].ptr,
                w.data_ptr(), b.wb - 1, None))
            torch.cuda.synchronize()
            out["short_untouched"] = np.array(all(v.untouched() for v in o.values()) and bool((w == 0xC3).all()))
    z = {"lo": Guarded(1, 8), "dl": Guarded(1, 8), "st": Guarded(2, 8)}
    torch.cuda.synchronize()
    cld_amd.split_lines_device(0, None, None, 0, 0, z["lo"].ptr, None, 0, z["dl"].ptr, None, 0,
                               flags=cld_amd.LINES_JOIN_BLANK, d_status_ptr=z["st"].ptr)
    cld_amd.split_lines_device(0, None, None, 0, 0, None, None, 0, None, None, 0)
    torch.cuda.synchronize()
    out["empty_dl"], out["empty_st"] = z["dl"].get("n == 0 doc_lines"), z["st"].get("n == 0 status")
    out["empty_lo_untouched"] = np.array(z["lo"].untouched())

else:
    buf, offs = inp["buf"], inp["offs"]
    n, nb = len(offs) - 1, len(buf)
    JOIN = cld_amd.LINES_JOIN_BLANK
    d_buf, d_offs = upload(buf), upload(offs)
    dl, st = Guarded(n + 1, 8), Guarded(2, 8)
    wb = cld_amd.lines_work_bytes(n, nb)
    w = work(wb)
    torch.cuda.synchronize()
    cld_amd.split_lines_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, None, None, 0, dl.ptr, w.data_ptr(), wb,
                               flags=JOIN, d_status_ptr=st.ptr)
    torch.cuda.synchronize()
    m = int(st.get("sizing status")[0])
    lo, ld, ch = Guarded(m + 1, 8), Guarded(m, 4), Guarded(m * 3, 4)
    d_res = filled(m * 40)
    torch.cuda.synchronize()
    # the library's own stream carries the split, the detection and the bridge: no host wait in between
    cld_amd.split_lines_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, lo.ptr, ld.ptr, m, dl.ptr, w.data_ptr(), wb,
                               flags=JOIN, d_status_ptr=st.ptr)
    cld_amd.detect_batch_device(0, d_buf.data_ptr(), lo.ptr, m, d_res.data_ptr())
    cld_amd.lines_to_chunks_device(0, d_res.data_ptr(), lo.ptr, ld.ptr, m, d_offs.data_ptr(), n, dl.ptr, ch.ptr)
    o = {"counts": Guarded(BINS, 8), "bytes": Guarded(BINS, 8)}
    cwb = cld_amd.chunk_work_bytes(n, m)
    cw = work(cwb)
    cld_amd.chunk_totals_device(0, d_offs.data_ptr(), n, ch.ptr, m, dl.ptr, cw.data_ptr(), cwb,
                                d_chunk_counts_ptr=o["counts"].ptr, d_chunk_bytes_ptr=o["bytes"].ptr)
    gr = {"counts": Guarded(BINS, 8), "bin_bytes": Guarded(BINS, 8)}
    gwb = cld_amd.group_work_bytes(m)
    gw = work(gwb)
    cld_amd.group_by_language_device(0, d_res.data_ptr(), m, gr["counts"].ptr, gw.data_ptr(), gwb, d_offsets_ptr=lo.ptr,
                                     d_bin_bytes_ptr=gr["bin_bytes"].ptr)
    torch.cuda.synchronize()
    out["lo"], out["ld"], out["dl"], out["st"] = lo.get("line_offsets"), ld.get("line_doc"), dl.get("doc_lines"), st.get("status")
    out["results"] = d_res.cpu().numpy()[:m * 40]
    out["chunks"] = ch.get("chunks")
    out["chunk_counts"], out["chunk_bytes"] = o["counts"].get("counts"), o["bytes"].get("bytes")
    out["group_counts"], out["group_bin_bytes"] = gr["counts"].get("group counts"), gr["bin_bytes"].get("bin_bytes")
    bins = [int(b) for b in np.argsort(out["chunk_bytes"], kind="stable")[::-1][:4] if out["chunk_bytes"][b] > 0]
    out["bins"] = np.array(bins)
    for b in bins:
        sel = np.zeros(BINS, np.uint8)
        sel[b] = 1
        d_sel = upload(sel)
        nbytes = int(out["chunk_bytes"][b])
        oo = Guarded(n + 1, 8)
        d_o = filled(nbytes + 2 * BGUARD)
        torch.cuda.synchronize()
        cld_amd.gather_chunks_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, ch.ptr, m, dl.ptr, d_sel.data_ptr(),
                                     d_o.data_ptr() + BGUARD, nbytes, oo.ptr, cw.data_ptr(), cwb)
        torch.cuda.synchronize()
        g = d_o.cpu().numpy()
        assert (g[:BGUARD] == PATTERN).all() and (g[BGUARD + nbytes:] == PATTERN).all(), "bin %d: guard bytes written" % b
        out["bin%d_buf" % b] = g[BGUARD:BGUARD + nbytes]
        out["bin%d_offs" % b] = oo.get("bin %d offsets" % b)

np.savez(sys.argv[3], **out)
