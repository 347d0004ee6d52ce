"""Child process of test_gpu_scrub.py: torch initialises the GPU first (the
library then shares its HIP runtime, as in bench.py), the inputs go to HBM as
torch tensors and the device entries run on them.

argv: mode, input .npz, output .npz.
  bytes   cld_scrub_utf8_device on <buf, offs>: d_out in step with d_buf (one
          16-byte store per lane), d_out one byte off (byte stores), both five
          bytes off a 256-byte boundary (tiles cut the batch elsewhere), on a
          torch stream, without the counts, and n == 0.  Every output starts as
          PATTERN and has GUARD bytes either side.
  score   cld_detect_batch_device_ex and cld_detect_batch_device_vec (big
          regions, with and without d_valid_prefix) with CLD_FLAG_SCRUB_UTF8."""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
import cld_amd  # noqa: E402

cld_amd.init_device(0)
dev = torch.device("cuda", 0)
mode = sys.argv[1]
inp = np.load(sys.argv[2])
buf, offs = inp["buf"], inp["offs"]
n, nb = len(offs) - 1, len(buf)
out = {}
GUARD = 256
PATTERN = 0xA5
SCRUB = cld_amd.FLAG_SCRUB_UTF8


def filled(nbytes):
    return torch.full((max(nbytes, 1),), PATTERN, dtype=torch.uint8, device=dev)


d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)

if mode == "bytes":
    def run(key, in_off, out_off, counts=True, stream=None):
        """The batch at d_in + in_off, the copy at d_o + GUARD + out_off (both tensors tile-aligned)."""
        d_in = filled(nb + 64)
        d_in[in_off:in_off + nb] = torch.from_numpy(buf).to(dev)
        before = d_in.clone()
        d_o = filled(nb + 2 * GUARD + 64)
        d_r = torch.full((n,), -7, dtype=torch.int32, device=dev)
        assert d_in.data_ptr() % 1024 == 0 and d_o.data_ptr() % 1024 == 0
        torch.cuda.synchronize()             # (torch filled the tensors on its own stream, not the library's)
        cld_amd.scrub_utf8_device(0, d_in.data_ptr() + in_off, d_offs.data_ptr(), n, d_o.data_ptr() + GUARD + out_off,
                                  d_r.data_ptr() if counts else None, stream)
        torch.cuda.synchronize()
        assert torch.equal(d_in, before), key + ": the input was written"
        h = d_o.cpu().numpy()
        lo, hi = GUARD + out_off, GUARD + out_off + nb
        assert (h[:lo] == PATTERN).all() and (h[hi:] == PATTERN).all(), key + ": bytes outside the batch were written"
        out[key + "_out"] = h[lo:hi]
        out[key + "_replaced"] = d_r.cpu().numpy()

    run("aligned", 0, 0)
    run("bytewise", 0, 1)
    run("shifted", 5, 5)
    s = torch.cuda.Stream()
    run("stream", 0, 0, stream=s.cuda_stream)
    run("nocount", 0, 0, counts=False)
    cld_amd.scrub_utf8_device(0, None, None, 0, None, None, None)
else:
    d_buf = torch.from_numpy(buf).to(dev)
    before = d_buf.clone()
    d_out = filled(n * 40)
    torch.cuda.synchronize()                 # (torch filled the tensors on its own stream, not the library's)
    rc = cld_amd.lib().cld_detect_batch_device_ex(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_out.data_ptr(), SCRUB,
                                                  None)
    assert rc == 0, "cld_detect_batch_device_ex: %d" % rc
    torch.cuda.synchronize()
    out["ex_out"] = d_out.cpu().numpy()[:n * 40].view(cld_amd.RESULT_DTYPE)

    def vec(key, with_vp):
        t = {"out": filled(n * 40), "coffs": filled((n + 1) * 8), "status": filled(16), "vp": filled(n * 4)}
        torch.cuda.synchronize()
        cld_amd.detect_batch_device_vec(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, t["out"].data_ptr(), None, 0,
                                        t["coffs"].data_ptr(), t["status"].data_ptr(), flags=SCRUB, big_regions=True,
                                        d_valid_prefix_ptr=t["vp"].data_ptr() if with_vp else None)
        torch.cuda.synchronize()
        total = int(t["status"].cpu().numpy()[:16].view(cld_amd.VEC_STATUS_DTYPE)["total_chunks"][0])
        t["chunks"] = filled(total * 12)
        torch.cuda.synchronize()
        cld_amd.detect_batch_device_vec(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, t["out"].data_ptr(),
                                        t["chunks"].data_ptr(), total, t["coffs"].data_ptr(), t["status"].data_ptr(),
                                        flags=SCRUB, big_regions=True,
                                        d_valid_prefix_ptr=t["vp"].data_ptr() if with_vp else None)
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in t.items()}
        out[key + "_out"] = h["out"][:n * 40].view(cld_amd.RESULT_DTYPE)
        out[key + "_coffs"] = h["coffs"][:(n + 1) * 8].view(np.uint64)
        out[key + "_status"] = h["status"][:16].view(cld_amd.VEC_STATUS_DTYPE)
        out[key + "_chunks"] = h["chunks"][:total * 12].view(cld_amd.CHUNK_DTYPE)
        out[key + "_vp"] = h["vp"][:n * 4].view(np.int32)

    vec("vec", True)
    vec("vecnovp", False)
    assert torch.equal(d_buf, before), "the input was written"

np.savez(sys.argv[3], **out)
