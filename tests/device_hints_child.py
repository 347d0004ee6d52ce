"""Child process of test_gpu_device_hints.py: torch initialises the GPU first
(the library then shares its HIP runtime, as in bench.py), every input goes to
HBM as a torch tensor, and the device entry points run on them.

argv: input .npz, output .npz.  The input holds numbered calls:
  k<i>_buf, k<i>_offs, k<i>_plain [, k<i>_rec, k<i>_text]   cld_hint_boosts_device
  d<i>_buf, d<i>_offs, d<i>_flags [, d<i>_rec, d<i>_text]   cld_detect_batch_device_hints
  p<i>_buf, p<i>_offs                                        cld_detect_batch_device
The output holds k<i>_priors [n, 14], k<i>_boosts [n, 16], d<i>_out and p<i>_out
(cld_result records)."""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
import cld_amd  # noqa: E402

cld_amd.init_device(0)
dev = torch.device("cuda", 0)
inp = np.load(sys.argv[1])
out = {}


def up(a):
    """numpy array -> (tensor in HBM, its address); an empty one still gets an address."""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([b, np.zeros(1, np.uint8)])).to(dev)
    return t, t.data_ptr()


def hint_args(key):
    if key + "_rec" not in inp:
        return None, None, None, 0
    rec, text = inp[key + "_rec"], inp[key + "_text"]
    tr, pr = up(rec)
    tt, pt = up(text)
    return (tr, tt), pr, pt, len(text)


stream = torch.cuda.Stream()
for key in sorted(k[:-4] for k in inp.files if k.startswith("k") and k.endswith("_buf")):
    buf, offs, plain = inp[key + "_buf"], inp[key + "_offs"], bool(inp[key + "_plain"])
    n = len(offs) - 1
    tb, pb = up(buf)
    to, po = up(offs)
    keep, prec, ptext, tbytes = hint_args(key)
    res = []
    for sp in (None, stream.cuda_stream):
        pri = torch.full((n, 14), -7, dtype=torch.int16, device=dev)
        boo = torch.full((n, 16), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        cld_amd.hint_boosts_device(0, pb, po, n, prec, ptext, tbytes, plain, pri.data_ptr(), boo.data_ptr(), sp)
        torch.cuda.synchronize()
        res.append((pri.cpu().numpy(), boo.cpu().numpy().view(np.uint32)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), key + ": streams differ"
    out[key + "_priors"], out[key + "_boosts"] = res[0]
    # either output alone
    pri = torch.full((n, 14), -7, dtype=torch.int16, device=dev)
    boo = torch.full((n, 16), -7, dtype=torch.int32, device=dev)
    cld_amd.hint_boosts_device(0, pb, po, n, prec, ptext, tbytes, plain, pri.data_ptr(), None, None)
    cld_amd.hint_boosts_device(0, pb, po, n, prec, ptext, tbytes, plain, None, boo.data_ptr(), None)
    torch.cuda.synchronize()
    assert np.array_equal(pri.cpu().numpy(), res[0][0]) and np.array_equal(boo.cpu().numpy().view(np.uint32), res[0][1])

# n = 0: nothing is read
cld_amd.hint_boosts_device(0, None, None, 0)
cld_amd.detect_batch_device_hints(0, None, None, 0, 0, None)


def results(t, n):
    return t.cpu().numpy()[:n * 40].view(cld_amd.RESULT_DTYPE)


for key in sorted(k[:-4] for k in inp.files if k[0] in "dp" and k.endswith("_buf")):
    buf, offs = inp[key + "_buf"], inp[key + "_offs"]
    n = len(offs) - 1
    tb, pb = up(buf)
    to, po = up(offs)
    d_out = torch.zeros(n * 40 + 8, dtype=torch.uint8, device=dev)
    if key[0] == "p":
        cld_amd.detect_batch_device(0, pb, po, n, d_out.data_ptr(), None)
    else:
        keep, prec, ptext, tbytes = hint_args(key)
        cld_amd.detect_batch_device_hints(0, pb, po, n, len(buf), d_out.data_ptr(), prec, ptext, tbytes,
                                          int(inp[key + "_flags"]), stream.cuda_stream if key.endswith("s") else None)
    torch.cuda.synchronize()
    out[key + "_out"] = results(d_out, n)

np.savez(sys.argv[2], **out)
