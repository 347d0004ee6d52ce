"""Child process of test_gpu_device_docflags.py: torch initialises the GPU first
(the library then shares its HIP runtime, as in bench.py), every input goes to
HBM as a torch tensor, and cld_detect_batch_device_docflags /
cld_detect_batch_device_vec_docflags run on them.

argv: input .npz, output .npz.  The input holds calls by key:
  <key>_buf, <key>_offs, <key>_flags, <key>_vec (0: results, 1: with chunk vectors)
  [, <key>_words] [, <key>_rec, <key>_text]
A results call leaves <key>_out.  A vector call is made twice: the sizing pass
(chunk_cap 0, d_chunks NULL; <key>_size_out, _size_coffs, _size_status), then
with room for status.total_chunks chunks and GUARD more behind them (<key>_out,
_coffs, _chunks, _status).  A key without <key>_words passes d_doc_flags NULL,
and the entry the call is forwarded to runs on the same input as well
(<key>_base_*).  Keys starting with "s" are enqueued back to back on one torch
stream, with one synchronise after the last."""
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
        self.vec = bool(inp[key + "_vec"])
        self.tb, self.pb = up(self.buf)
        self.to, self.po = up(self.offs)
        self.pw = self.prec = self.ptext = None
        self.tbytes = 0
        if key + "_words" in inp:
            assert inp[key + "_words"].dtype == np.uint32 and len(inp[key + "_words"]) == self.n
            self.tw, self.pw = up(inp[key + "_words"])
        if key + "_rec" in inp:
            self.tr, self.prec = up(inp[key + "_rec"])
            self.tt, self.ptext = up(inp[key + "_text"])
            self.tbytes = len(inp[key + "_text"])

    def enqueue(self, cap=0, with_chunks=True, stream=None, base=False):
        """-> the output tensors, every byte of them PATTERN before the call.  base: through the
        entry a call without words is forwarded to."""
        n = self.n
        t = {"out": filled(n * 40)}
        if not self.vec:
            if base:
                cld_amd.detect_batch_device_hints(0, self.pb, self.po, n, len(self.buf), t["out"].data_ptr(), self.prec,
                                                  self.ptext, self.tbytes, self.flags, stream)
            else:
                cld_amd.detect_batch_device_docflags(0, self.pb, self.po, n, len(self.buf), t["out"].data_ptr(),
                                                     self.pw, self.prec, self.ptext, self.tbytes, self.flags, stream)
            return t
        t.update(coffs=filled((n + 1) * 8), status=filled(16),
                 chunks=filled((cap + GUARD) * 12) if with_chunks else None)
        pc = t["chunks"].data_ptr() if with_chunks else None
        if base:
            cld_amd.detect_batch_device_vec(0, self.pb, self.po, n, len(self.buf), t["out"].data_ptr(), pc, cap,
                                            t["coffs"].data_ptr(), t["status"].data_ptr(), self.prec, self.ptext,
                                            self.tbytes, self.flags, False, None, stream)
        else:
            cld_amd.detect_batch_device_vec_docflags(0, self.pb, self.po, n, len(self.buf), t["out"].data_ptr(), pc, cap,
                                                     t["coffs"].data_ptr(), t["status"].data_ptr(), self.pw, self.prec,
                                                     self.ptext, self.tbytes, self.flags, False, None, stream)
        return t

    def save(self, prefix, t, cap=0):
        n = self.n
        h = {k: v.cpu().numpy() for k, v in t.items() if v is not None}
        out[prefix + "out"] = h["out"][:n * 40].view(cld_amd.RESULT_DTYPE)
        if self.vec:
            out[prefix + "coffs"] = h["coffs"][:(n + 1) * 8].view(np.uint64)
            out[prefix + "status"] = h["status"][:16].view(cld_amd.VEC_STATUS_DTYPE)
            if "chunks" in h:
                out[prefix + "chunks"] = h["chunks"][:(cap + GUARD) * 12].view(cld_amd.CHUNK_DTYPE)

    def size(self, base=False):
        """The sizing pass of a vector call -> total_chunks."""
        t = self.enqueue(0, with_chunks=False, base=base)
        torch.cuda.synchronize()
        prefix = self.key + ("_base_size_" if base else "_size_")
        self.save(prefix, t)
        return int(out[prefix + "status"]["total_chunks"][0])

    def run(self, base=False):
        total = self.size(base) if self.vec else 0
        t = self.enqueue(total, base=base)
        torch.cuda.synchronize()
        self.save(self.key + ("_base_" if base else "_"), t, total)


keys = sorted(k[:-4] for k in inp.files if k.endswith("_buf"))
for key in (k for k in keys if not k.startswith("s")):
    c = Call(key)
    c.run()
    if c.pw is None:
        c.run(base=True)

# calls back to back on one torch stream, one synchronise
calls = [Call(k) for k in keys if k.startswith("s")]
if calls:
    totals = [c.size() if c.vec else 0 for c in calls]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):                    # (the output tensors are made on the stream that fills them)
        ts = [c.enqueue(total, stream=stream.cuda_stream) for c, total in zip(calls, totals)]
    stream.synchronize()
    for c, t, total in zip(calls, ts, totals):
        c.save(c.key + "_", t, total)

np.savez(sys.argv[2], **out)
