"""Child process of test_gpu_chunks.py: torch initialises the GPU first (the
library then shares its HIP runtime, as in bench.py), the inputs go to HBM as
torch tensors and the chunk device entries run on them.

argv: mode, input .npz, output .npz.
  cases   every case <k> of the input (buf<k>, offs<k>, chunks<k> as bytes, coffs<k>,
          cap<k>): cld_chunk_totals_device (t<k>_counts, t<k>_bytes), then one
          cld_gather_chunks_device per row of runs<k> = (select id, flags, out_cap or
          -1 for the sizing pass, bytes to allocate, output alignment 0..15), with
          select<id> (g<k>_<row>_buf, g<k>_<row>_offs).  The documents sit five bytes off
          a 256-byte boundary between guard bytes; d_chunks holds cap<k> chunks and
          guard bytes behind them; every output starts as PATTERN between guards, the
          workspace as garbage; every input is compared before and after.  On the case
          named by `variants`: a torch stream, each optional output left out, the same
          call twice, a workspace one byte short, and n == 0.
  e2e     cld_detect_batch_device_vec on <buf, offs> (sizing pass, then with room), the
          totals, then for the bins with the most bytes and both flag values a sizing
          gather, the gather and cld_detect_batch_device on the gathered batch."""
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
GUARD = 64                     # words either side of a totals array, of an offsets array
BGUARD = 256                   # bytes either side of the documents, of a gathered buffer
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


class Batch:
    """A batch and its vectors in HBM."""

    def __init__(self, buf, offs, chunks, coffs, cap):
        self.n, self.cap, nb = len(offs) - 1, cap, len(buf)
        self.d_in = filled(nb + 2 * BGUARD + 16)
        self.lo = BGUARD + 5
        assert self.d_in.data_ptr() % 256 == 0
        if nb:
            self.d_in[self.lo:self.lo + nb] = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)
        self.d_offs, self.d_coffs = upload(offs), upload(coffs)
        self.d_chunks = filled(cap * 12 + 12 * GUARD)            # (chunks past the capacity: guard bytes)
        if cap:
            self.d_chunks[:cap * 12] = upload(chunks[:cap])
        self.inputs = (self.d_in, self.d_offs, self.d_coffs, self.d_chunks)
        self.before = [t.clone() for t in self.inputs]
        self.wb = cld_amd.chunk_work_bytes(self.n, cap)

    def unchanged(self):
        return all(torch.equal(a, b) for a, b in zip(self.inputs, self.before))

    def totals(self, skip=(), stream=None, short=0):
        o = {"counts": Guarded(BINS, 8), "bytes": Guarded(BINS, 8)}
        w = work(self.wb - short)
        torch.cuda.synchronize()             # (torch filled the tensors on its own stream, not the library's)
        p = {k: (None if k in skip else v.ptr) for k, v in o.items()}
        cld_amd.chunk_totals_device(0, self.d_offs.data_ptr(), self.n, self.d_chunks.data_ptr(), self.cap,
                                    self.d_coffs.data_ptr(), w.data_ptr(), self.wb - short,
                                    d_chunk_counts_ptr=p["counts"], d_chunk_bytes_ptr=p["bytes"], stream_ptr=stream)
        torch.cuda.synchronize()
        for k in skip:
            assert o[k].untouched(), "%s was written though it was left out" % k
        return {k: v.get(k) for k, v in o.items() if k not in skip}

    def gather(self, d_sel, flags, cap, alloc, align, stream=None, short=0, what=""):
        """-> (the bytes written, out_offsets); cap < 0: the sizing pass."""
        d_o = filled(alloc + 2 * BGUARD + 16)
        assert d_o.data_ptr() % 256 == 0
        oo = Guarded(self.n + 1, 8)
        w = work(self.wb - short)
        lo = BGUARD + align
        sizing = cap < 0
        torch.cuda.synchronize()
        cld_amd.gather_chunks_device(0, self.d_in.data_ptr() + self.lo, self.d_offs.data_ptr(), self.n,
                                     self.d_chunks.data_ptr(), self.cap, self.d_coffs.data_ptr(), d_sel.data_ptr(),
                                     None if sizing else d_o.data_ptr() + lo, 0 if sizing else cap, oo.ptr,
                                     w.data_ptr(), self.wb - short, flags=flags, stream_ptr=stream)
        torch.cuda.synchronize()
        offs = oo.get(what)
        h = d_o.cpu().numpy()
        hi = lo + (0 if sizing else min(cap, int(offs[-1]), alloc))
        assert (h[:lo] == PATTERN).all() and (h[hi:] == PATTERN).all(), what + ": bytes outside the capacity were written"
        return h[lo:hi], offs


if mode == "cases":
    selects = {int(k[6:]): upload(inp[k]) for k in inp.files if k.startswith("select")}
    for k in range(int(inp["cases"])):
        b = Batch(inp["buf%d" % k], inp["offs%d" % k], inp["chunks%d" % k].view(cld_amd.CHUNK_DTYPE), inp["coffs%d" % k],
                  int(inp["cap%d" % k]))
        t = b.totals()
        out["t%d_counts" % k], out["t%d_bytes" % k] = t["counts"], t["bytes"]
        runs = inp["runs%d" % k]
        for r, (sel, flags, cap, alloc, align) in enumerate(runs):
            what = "case %d, run %d" % (k, r)
            out["g%d_%d_buf" % (k, r)], out["g%d_%d_offs" % (k, r)] = b.gather(selects[int(sel)], int(flags), int(cap),
                                                                              int(alloc), int(align), what=what)
        if k == int(inp["variants"]):
            sel, flags, cap, alloc, align = (int(x) for x in runs[0])
            s = torch.cuda.Stream()
            t = b.totals(stream=s.cuda_stream)
            out["stream_counts"], out["stream_bytes"] = t["counts"], t["bytes"]
            out["stream_buf"], out["stream_offs"] = b.gather(selects[sel], flags, cap, alloc, align, stream=s.cuda_stream)
            out["only_counts"] = b.totals(skip=("bytes",))["counts"]
            out["only_bytes"] = b.totals(skip=("counts",))["bytes"]
            b.totals(skip=("counts", "bytes"))
            out["again_buf"], out["again_offs"] = b.gather(selects[sel], flags, cap, alloc, align)
            # a workspace one byte short: CLD_ENOSPC and nothing written, not even to the workspace
            o = {"counts": Guarded(BINS, 8), "bytes": Guarded(BINS, 8), "offs": Guarded(b.n + 1, 8)}
            d_o = filled(alloc + 16)
            w = work(b.wb)
            torch.cuda.synchronize()
            L = cld_amd.lib()
            out["short_rc_totals"] = np.array(L.cld_chunk_totals_device(
                0, b.d_offs.data_ptr(), b.n, b.d_chunks.data_ptr(), b.cap, b.d_coffs.data_ptr(), o["counts"].ptr,
                o["bytes"].ptr, w.data_ptr(), b.wb - 1, None))
            out["short_rc_gather"] = np.array(L.cld_gather_chunks_device(
                0, b.d_in.data_ptr() + b.lo, b.d_offs.data_ptr(), b.n, b.d_chunks.data_ptr(), b.cap, b.d_coffs.data_ptr(),
                selects[sel].data_ptr(), flags, d_o.data_ptr(), alloc, o["offs"].ptr, w.data_ptr(), b.wb - 1, None))
            torch.cuda.synchronize()
            out["short_untouched"] = np.array(all(v.untouched() for v in o.values()) and bool((w == 0xC3).all()) and
                                              bool((d_o == PATTERN).all()))
        assert b.unchanged(), "case %d: an input was written" % k
    z = {"counts": Guarded(BINS, 8), "bytes": Guarded(BINS, 8), "offs": Guarded(1, 8)}
    d_co = upload(np.zeros(1, np.uint64))
    torch.cuda.synchronize()
    cld_amd.chunk_totals_device(0, None, 0, None, 0, d_co.data_ptr(), None, 0, d_chunk_counts_ptr=z["counts"].ptr,
                                d_chunk_bytes_ptr=z["bytes"].ptr)
    cld_amd.gather_chunks_device(0, None, None, 0, None, 0, d_co.data_ptr(), selects[0].data_ptr(), None, 0, z["offs"].ptr,
                                 None, 0)
    cld_amd.chunk_totals_device(0, None, 0, None, 0, d_co.data_ptr(), None, 0)
    torch.cuda.synchronize()
    for k, v in z.items():
        out["empty_" + k] = v.get("n == 0 " + k)

else:
    buf, offs = inp["buf"], inp["offs"]
    n, nb = len(offs) - 1, len(buf)
    d_buf, d_offs = upload(buf), upload(offs)
    d_res, d_coffs, d_st = filled(n * 40), filled((n + 1) * 8), filled(16)
    torch.cuda.synchronize()
    cld_amd.detect_batch_device_vec(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_res.data_ptr(), None, 0,
                                    d_coffs.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    cap = int(d_st.cpu().numpy()[:16].view(cld_amd.VEC_STATUS_DTYPE)["total_chunks"][0])
    d_chunks = filled(cap * 12 + 12 * GUARD)
    torch.cuda.synchronize()
    cld_amd.detect_batch_device_vec(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_res.data_ptr(), d_chunks.data_ptr(),
                                    cap, d_coffs.data_ptr(), d_st.data_ptr())
    # the library's own stream carries the detection and the totals: no host wait in between
    o = {"counts": Guarded(BINS, 8), "bytes": Guarded(BINS, 8)}
    wb = cld_amd.chunk_work_bytes(n, cap)
    w = work(wb)
    cld_amd.chunk_totals_device(0, d_offs.data_ptr(), n, d_chunks.data_ptr(), cap, d_coffs.data_ptr(), w.data_ptr(), wb,
                                d_chunk_counts_ptr=o["counts"].ptr, d_chunk_bytes_ptr=o["bytes"].ptr)
    torch.cuda.synchronize()
    out["results"] = d_res.cpu().numpy()[:n * 40]
    out["coffs"] = d_coffs.cpu().numpy()[:(n + 1) * 8].view(np.uint64)
    out["chunks"] = d_chunks.cpu().numpy()[:cap * 12]
    out["status"] = d_st.cpu().numpy()[:16]
    out["chunk_counts"], out["chunk_bytes"] = o["counts"].get("counts"), o["bytes"].get("bytes")
    bins = [int(b) for b in np.argsort(out["chunk_bytes"], kind="stable")[::-1][:4] if out["chunk_bytes"][b] > 0]
    out["bins"] = np.array(bins)
    for b in bins:
        sel = np.zeros(BINS, np.uint8)
        sel[b] = 1
        d_sel = upload(sel)
        for flags in (0, cld_amd.CHUNKS_SPACE):
            oo = Guarded(n + 1, 8)
            torch.cuda.synchronize()
            cld_amd.gather_chunks_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_chunks.data_ptr(), cap,
                                         d_coffs.data_ptr(), d_sel.data_ptr(), None, 0, oo.ptr, w.data_ptr(), wb, flags=flags)
            torch.cuda.synchronize()
            nbytes = int(oo.get("sizing")[-1])
            if flags == 0:
                assert nbytes == int(out["chunk_bytes"][b]), "bin %d: the totals do not size the buffer" % b
            d_o = filled(nbytes + 2 * BGUARD)
            d_r = filled(n * 40)
            torch.cuda.synchronize()
            cld_amd.gather_chunks_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, d_chunks.data_ptr(), cap,
                                         d_coffs.data_ptr(), d_sel.data_ptr(), d_o.data_ptr() + BGUARD, nbytes, oo.ptr,
                                         w.data_ptr(), wb, flags=flags)
            cld_amd.detect_batch_device(0, d_o.data_ptr() + BGUARD, oo.ptr, n, d_r.data_ptr())
            torch.cuda.synchronize()
            g = d_o.cpu().numpy()
            assert (g[:BGUARD] == PATTERN).all() and (g[BGUARD + nbytes:] == PATTERN).all(), "bin %d: guard bytes written" % b
            key = "bin%d_f%d_" % (b, flags)
            out[key + "buf"] = g[BGUARD:BGUARD + nbytes]
            out[key + "offs"] = oo.get(key)
            out[key + "results"] = d_r.cpu().numpy()[:n * 40]

np.savez(sys.argv[3], **out)
