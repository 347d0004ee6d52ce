"""The device-resident vector interface without a GPU: the layout of
cld_vec_status (include/cld_mi355x.h) and the argument checks of
cld_detect_batch_device_vec that come before any GPU is touched."""
import numpy as np
import pytest


def call(L, flags=0, chunks=None, chunk_cap=0, valid_prefix=None):
    """cld_detect_batch_device_vec on an empty batch; the pointers that are given point at host memory
    nobody reads (the checks come first)."""
    return L.cld_detect_batch_device_vec(0, None, None, 0, 0, None, None, 0, flags, 0, None, chunks, chunk_cap, None,
                                         valid_prefix, None, None)


def test_vec_status_layout():
    import cld_amd
    d = cld_amd.VEC_STATUS_DTYPE
    assert d.itemsize == 16
    assert {k: d.fields[k][1] for k in d.names} == {"total_chunks": 0, "failed_docs": 8, "rejected_docs": 12}
    assert (d.fields["total_chunks"][0].itemsize, d.fields["failed_docs"][0].itemsize,
            d.fields["rejected_docs"][0].itemsize) == (8, 4, 4)
    assert "cld_detect_batch_device_vec" in cld_amd.EXPORTS


@pytest.mark.parametrize("flags", [1, 2, 1 | 8, 0x10000, 1 << 31],
                         ids=["strip_extras", "cstring", "strip_extras_check_utf8", "unknown", "unknown31"])
def test_detect_batch_device_vec_rejects_flags(flags):
    """Preparation flags other than the check and unknown bits: CLD_EINVAL before cld_init, so also where no GPU is."""
    import cld_amd
    assert (cld_amd.FLAG_STRIP_EXTRAS, cld_amd.FLAG_CSTRING, cld_amd.FLAG_CHECK_UTF8) == (1, 2, 8)
    assert call(cld_amd.lib(), flags=flags) == cld_amd.EINVAL
    with pytest.raises(cld_amd.CldError, match="%d" % cld_amd.EINVAL):
        cld_amd.detect_batch_device_vec(0, None, None, 0, 0, None, None, 0, None, None, flags=flags)


def test_detect_batch_device_vec_rejects_pointers():
    import cld_amd
    L = cld_amd.lib()
    word = np.zeros(4, np.int32)
    # a valid-prefix array without CLD_FLAG_CHECK_UTF8 (also next to other accepted flags)
    assert call(L, flags=0, valid_prefix=word.ctypes.data) == cld_amd.EINVAL
    assert call(L, flags=cld_amd.FLAG_HTML | cld_amd.FLAG_BEST_EFFORT, valid_prefix=word.ctypes.data) == cld_amd.EINVAL
    # room for chunks without a place for them
    assert call(L, chunks=None, chunk_cap=1) == cld_amd.EINVAL
    assert call(L, flags=cld_amd.FLAG_CHECK_UTF8, chunks=None, chunk_cap=1 << 40) == cld_amd.EINVAL
