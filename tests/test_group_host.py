"""cld_group_by_language, the host reference of the group entries (no GPU),
against numpy: np.bincount, a stable np.argsort, np.cumsum and np.add.at over
synthetic cld_result arrays.  Everything is integers: every comparison is exact."""
import numpy as np
import pytest

import cld_amd
import group_cases as gc

SIZES = (0, 1, 2, 70001)


@pytest.mark.parametrize("n", SIZES)
def test_key_sets_against_numpy(n):
    offs = gc.lengths_for(n)
    for name, keys in gc.key_sets(n).items():
        res = gc.results_for(keys)
        before = res.copy()
        for flags in gc.FLAG_SETS:
            got = cld_amd.group_by_language(res, offsets=offs, flags=flags)
            gc.assert_group(got, gc.expected(res, offs, flags), "%s, n %d, flags %d" % (name, n, flags))
            assert int(got["group_offsets"][gc.BINS]) == n
        assert np.array_equal(res.view(np.uint8), before.view(np.uint8)), "the results were written"


def test_every_bin_exactly_once():
    keys = gc.key_sets(gc.BINS)["every_bin"]
    assert sorted(keys) == list(range(gc.BINS))
    res = gc.results_for(keys, top1=keys, reliable=1)
    got = cld_amd.group_by_language(res)
    assert (got["counts"] == 1).all() and np.array_equal(got["group_offsets"], np.arange(gc.BINS + 1, dtype=np.uint64))
    assert np.array_equal(keys[got["order"]], np.arange(gc.BINS))


def test_clamp_to_the_last_bin():
    keys = np.array(gc.CLAMP_KEYS * 3, dtype=np.uint16)
    res = gc.results_for(keys, top1=keys, reliable=1)
    got = cld_amd.group_by_language(res)
    assert got["counts"][613] == 3 and got["counts"][614] == 12 and got["counts"][:613].sum() == 0
    assert list(got["order"][3:]) == [i for i in range(15) if i % 5 != 0]      # stable within the bin


def test_top1_and_reliable_only_change_the_key():
    res = gc.results_for(np.array([5, 5, 5, 5], np.uint16), top1=[5, 9, 5, 9], reliable=[1, 1, 0, 0])
    c = lambda flags: {int(b): int(k) for b, k in enumerate(cld_amd.group_by_language(res, flags=flags)["counts"]) if k}
    assert c(0) == {5: 4}
    assert c(cld_amd.GROUP_TOP1) == {5: 2, 9: 2}
    assert c(cld_amd.GROUP_RELIABLE_ONLY) == {5: 2, 26: 2}
    assert c(cld_amd.GROUP_TOP1 | cld_amd.GROUP_RELIABLE_ONLY) == {5: 1, 9: 1, 26: 2}


def test_optional_outputs_and_argument_errors():
    n = 1000
    res = gc.results_for(gc.key_sets(n)["random"])
    offs = gc.lengths_for(n)
    want = gc.expected(res, offs, 0)
    L = cld_amd.lib()
    new = lambda: {"counts": np.full(gc.BINS, 7, np.uint64), "bin_bytes": np.full(gc.BINS, 7, np.uint64),
                   "order": np.full(n, 7, np.uint32), "group_offsets": np.full(gc.BINS + 1, 7, np.uint64)}

    def call(a, flags=0, offsets=offs, skip=()):
        p = {k: (None if k in skip else v.ctypes.data) for k, v in a.items()}
        return L.cld_group_by_language(res.ctypes.data, n, flags, None if offsets is None else offsets.ctypes.data,
                                       p["counts"], p["bin_bytes"], p["order"], p["group_offsets"])

    for skip in ("bin_bytes", "order", "group_offsets"):
        a = new()
        assert call(a, skip=(skip,)) == 0
        assert (a.pop(skip) == 7).all()
        gc.assert_group(a, want, "without " + skip)
    a = new()
    assert call(a, offsets=None, skip=("bin_bytes",)) == 0                    # no byte totals: no offsets needed
    gc.assert_group({k: v for k, v in a.items() if k != "bin_bytes"}, want, "without offsets")
    a = new()
    assert call(a, offsets=None) == cld_amd.EINVAL                            # bin_bytes without offsets
    for bit in (4, 8, 0x80000000):
        assert call(a, flags=bit) == cld_amd.EINVAL and call(a, flags=bit | cld_amd.GROUP_TOP1) == cld_amd.EINVAL
    assert call(a, skip=("counts",)) == cld_amd.EINVAL
    assert all((v == 7).all() for v in a.values()), "a rejected call wrote an output"
    assert L.cld_group_by_language(None, n, 0, None, a["counts"].ctypes.data, None, None, None) == cld_amd.EINVAL
    assert L.cld_group_by_language(res.ctypes.data, 1 << 31, 0, None, a["counts"].ctypes.data, None, None,
                                   None) == cld_amd.EINVAL
    with pytest.raises(cld_amd.CldError, match="%d" % cld_amd.EINVAL):
        cld_amd.group_by_language(res, flags=4)


def test_work_bytes_is_monotone_and_bounded():
    sizes = [0, 1, 2, 511, 512, 513, 70001, 131072, 131073, 1 << 20, 1 << 24, (1 << 31) - 1]
    w = [cld_amd.group_work_bytes(n) for n in sizes]
    assert all(a <= b for a, b in zip(w, w[1:])) and w[-1] <= 16 << 20 and w[1] > 0
