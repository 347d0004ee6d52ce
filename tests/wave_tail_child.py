"""Child process of test_gpu_wave_tail.py: the plain batches of the input .npz
through cld_detect_batch, in a process of its own because the two switches it
is started under are read once per process -- CLD_TINY=0 (so that batches of
any size take enqueue()'s k_wave and not the request-sized path, which keeps
the tail in the wave) and CLD_WAVE_TAIL (1: k_wave's deferred instantiation
and k_wtail; 0: the tail in the wave).

argv: input .npz, output .npz.  Per key: <key>_buf, <key>_offs, <key>_flags in;
<key>_out (the results) and <key>_short (BatchStats.short_docs) out."""
import sys

import numpy as np

import cld_amd

cld_amd.init()
inp = np.load(sys.argv[1])
out = {}
for key in sorted(k[:-4] for k in inp.files if k.endswith("_buf")):
    res = cld_amd.detect_batch(buf=inp[key + "_buf"], offsets=inp[key + "_offs"], flags=int(inp[key + "_flags"]))
    out[key + "_out"] = res
    out[key + "_short"] = np.int64(cld_amd.last_stats(0).short_docs)
np.savez(sys.argv[2], **out)
