"""Inputs and numpy expectations shared by test_group_host.py and test_gpu_group.py:
synthetic cld_result arrays (no detection needed) and what numpy makes of them."""
import numpy as np

import cld_amd

BINS = cld_amd.GROUP_BINS
FLAG_SETS = (0, cld_amd.GROUP_TOP1, cld_amd.GROUP_RELIABLE_ONLY, cld_amd.GROUP_TOP1 | cld_amd.GROUP_RELIABLE_ONLY)
CLAMP_KEYS = (613, 614, 615, 0xFFFE, 0xFFFF)


def results_for(keys, seed=0, top1=None, reliable=None):
    """RESULT_DTYPE records with summary_lang = keys; lang3[0] = top1 (default: another language than
    the summary's for every third document), is_reliable = reliable (default: 0 for every fourth);
    the fields the entries must not read hold noise."""
    keys = np.asarray(keys, dtype=np.uint16)
    n = len(keys)
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=cld_amd.RESULT_DTYPE)
    r.view(np.uint8)[:] = rng.integers(0, 256, n * 40, dtype=np.uint8)
    r["summary_lang"] = keys
    idx = np.arange(n)
    r["lang3"][:, 0] = np.where(idx % 3 == 1, (keys.astype(np.uint32) * 7 + 5) % 620, keys) if top1 is None else top1
    r["is_reliable"] = (idx % 4 != 2) if reliable is None else reliable
    return r


def lengths_for(n, seed=0):
    """Document offsets: lengths 0..299, a few long ones, so that the byte totals need 64 bits only by their sum."""
    rng = np.random.default_rng(seed + 1)
    ln = rng.integers(0, 300, n).astype(np.uint64)
    if n:
        ln[rng.integers(0, n, min(n, 5))] += np.uint64(3 << 30)
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(ln, out=offs[1:])
    return offs


def key_sets(n, seed=0):
    """name -> summary_lang keys of n documents."""
    rng = np.random.default_rng(seed + 2)
    sets = {"random": rng.integers(0, 614, n),
            "every_bin": (np.arange(n) * 7 + 3) % BINS,            # n == BINS: every bin exactly once
            "one_key": np.full(n, 41),
            "clamp": np.array(CLAMP_KEYS)[rng.integers(0, len(CLAMP_KEYS), n)],
            "few": np.array([0, 26, 3, 613, 614])[rng.integers(0, 5, n)]}
    # a wave (64 documents) of 64 distinct keys, then a wave of one key, in turn
    i = np.arange(n)
    sets["waves"] = np.where((i // 64) % 2 == 0, (i % 64) * 9 + 11, 77)
    # runs of one key, of lengths around a wave and a workgroup step, which cross both kinds of boundary
    runs = np.array([1, 2, 63, 64, 65, 130, 511, 512, 513, 700, 1500])[rng.integers(0, 11, n // 200 + 2)]
    sets["runs"] = np.repeat(rng.integers(0, 615, len(runs)), runs)[:n]
    assert len(sets["runs"]) == n
    return {k: v.astype(np.uint16) for k, v in sets.items()}


def expected(results, offsets, flags):
    """counts, group_offsets, order, bin_bytes (None without offsets) by numpy."""
    key = (results["lang3"][:, 0] if flags & cld_amd.GROUP_TOP1 else results["summary_lang"]).astype(np.int64)
    if flags & cld_amd.GROUP_RELIABLE_ONLY:
        key = np.where(results["is_reliable"] == 0, 26, key)
    bins = np.minimum(key, cld_amd.NUM_LANGUAGES)
    counts = np.bincount(bins, minlength=BINS).astype(np.uint64)
    goffs = np.zeros(BINS + 1, dtype=np.uint64)
    np.cumsum(counts, out=goffs[1:])
    order = np.argsort(bins, kind="stable").astype(np.uint32)
    bin_bytes = None
    if offsets is not None:
        bin_bytes = np.zeros(BINS, dtype=np.uint64)
        np.add.at(bin_bytes, bins, np.diff(offsets))
    return {"counts": counts, "group_offsets": goffs, "order": order, "bin_bytes": bin_bytes}


def assert_group(got, want, what):
    for f in ("counts", "group_offsets", "order", "bin_bytes"):
        if want.get(f) is None or f not in got:
            continue
        g, w = np.asarray(got[f]), want[f]
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s%s" % (what, f, g.dtype, g.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %s differs at %d places; first at %d: got %d, numpy %d" % (
            what, f, len(bad), bad[0], g[bad[0]], w[bad[0]])
