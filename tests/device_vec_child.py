"""Child process of test_gpu_device_vec.py: torch initialises the GPU first (the
library then shares its HIP runtime, as in bench.py), every input goes to HBM
as a torch tensor, and cld_detect_batch_device_vec runs on them.

argv: input .npz, output .npz.  The input holds calls by key:
  <key>_buf, <key>_offs, <key>_flags [, <key>_rec, <key>_text] [, <key>_big] [, <key>_caps]
Every call is made twice: the sizing pass (chunk_cap 0, d_chunks NULL), whose
answers go to <key>_size_*, then with room for status.total_chunks chunks and a
guard region of GUARD chunks behind them (<key>_out, _coffs, _chunks [with the
guard], _status, and _vp with CLD_FLAG_CHECK_UTF8; <key>_novp_*: the same call
with d_valid_prefix NULL).  <key>_caps: also with chunk_cap total - 1 and 1
(<key>_cap<k>_*).  Keys starting with "s" are enqueued back to back on one
torch stream, with one synchronise after the last."""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
import cld_amd  # noqa: E402

cld_amd.init_device(0)
dev = torch.device("cuda", 0)
inp = np.load(sys.argv[1])
out = {}
GUARD = 64
PATTERN = 0xA5
CHECK = cld_amd.FLAG_CHECK_UTF8


def up(a):
    """numpy array -> (tensor in HBM, its address); an empty one still gets an address."""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([b, np.zeros(1, np.uint8)])).to(dev)
    return t, t.data_ptr()


def filled(nbytes):
    return torch.full((max(nbytes, 1),), PATTERN, dtype=torch.uint8, device=dev)


class Call:
    """One batch in HBM and the arguments that go with it."""

    def __init__(self, key):
        self.key = key
        self.buf, self.offs = inp[key + "_buf"], inp[key + "_offs"]
        self.n = len(self.offs) - 1
        self.flags = int(inp[key + "_flags"])
        self.big = bool(inp[key + "_big"]) if key + "_big" in inp else False
        self.tb, self.pb = up(self.buf)
        self.to, self.po = up(self.offs)
        self.prec = self.ptext = None
        self.tbytes = 0
        if key + "_rec" in inp:
            self.tr, self.prec = up(inp[key + "_rec"])
            self.tt, self.ptext = up(inp[key + "_text"])
            self.tbytes = len(inp[key + "_text"])

    def enqueue(self, cap, with_chunks=True, with_vp=True, stream=None):
        """-> the output tensors, every byte of them PATTERN before the call."""
        n = self.n
        t = {"out": filled(n * 40), "coffs": filled((n + 1) * 8), "status": filled(16),
             "chunks": filled((cap + GUARD) * 12) if with_chunks else None,
             "vp": filled(n * 4) if (self.flags & CHECK) and with_vp else None}
        cld_amd.detect_batch_device_vec(0, self.pb, self.po, n, len(self.buf), t["out"].data_ptr(),
                                        t["chunks"].data_ptr() if with_chunks else None, cap, t["coffs"].data_ptr(),
                                        t["status"].data_ptr(), self.prec, self.ptext, self.tbytes, self.flags,
                                        self.big, t["vp"].data_ptr() if t["vp"] is not None else None, stream)
        return t

    def save(self, prefix, t, cap):
        n = self.n
        h = {k: v.cpu().numpy() for k, v in t.items() if v is not None}
        out[prefix + "out"] = h["out"][:n * 40].view(cld_amd.RESULT_DTYPE)
        out[prefix + "coffs"] = h["coffs"][:(n + 1) * 8].view(np.uint64)
        out[prefix + "status"] = h["status"][:16].view(cld_amd.VEC_STATUS_DTYPE)
        if "chunks" in h:
            out[prefix + "chunks"] = h["chunks"][:(cap + GUARD) * 12].view(cld_amd.CHUNK_DTYPE)
        if "vp" in h:
            out[prefix + "vp"] = h["vp"][:n * 4].view(np.int32)
        return out[prefix + "status"]

    def size(self):
        t = self.enqueue(0, with_chunks=False)
        torch.cuda.synchronize()
        return int(self.save(self.key + "_size_", t, 0)["total_chunks"][0])


keys = sorted(k[:-4] for k in inp.files if k.endswith("_buf"))
for key in (k for k in keys if not k.startswith("s")):
    c = Call(key)
    total = c.size()
    t = c.enqueue(total)
    torch.cuda.synchronize()
    c.save(key + "_", t, total)
    if c.flags & CHECK:
        t = c.enqueue(total, with_vp=False)
        torch.cuda.synchronize()
        c.save(key + "_novp_", t, total)
    if key + "_caps" in inp:
        for cap in (total - 1, 1):
            t = c.enqueue(cap)
            torch.cuda.synchronize()
            c.save("%s_cap%d_" % (key, cap), t, cap)
        out[key + "_caps"] = np.array([total, total - 1, 1, 0])

# two batches back to back on one torch stream, one synchronise
calls = [Call(k) for k in keys if k.startswith("s")]
if calls:
    totals = [c.size() for c in calls]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):                    # (the output tensors are made on the stream that fills them)
        ts = [c.enqueue(total, stream=stream.cuda_stream) for c, total in zip(calls, totals)]
    stream.synchronize()
    for c, t, total in zip(calls, ts, totals):
        c.save(c.key + "_", t, total)

# n == 0: CLD_OK, d_chunk_offsets[0] = 0 and a zero status; with NULL pointers nothing is written
co, st = filled(8), filled(16)
cld_amd.detect_batch_device_vec(0, None, None, 0, 0, None, None, 0, co.data_ptr(), st.data_ptr())
cld_amd.detect_batch_device_vec(0, None, None, 0, 0, None, None, 0, None, None)
torch.cuda.synchronize()
out["n0"] = np.concatenate([co.cpu().numpy(), st.cpu().numpy()])

np.savez(sys.argv[2], **out)
