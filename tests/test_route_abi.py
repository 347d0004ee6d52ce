"""cld_last_route_stats (include/cld_mi355x.h) without a GPU: the header
declares the call and its record, the library exports it, the binding mirrors
the record field for field, and the argument checks hold.  (That each field
reads the right device counter is held by tests/test_gpu_long_seams.py, which
compares every field with counts worked out from the oracle.)"""
import ctypes
import os
import re

import cld_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["long_list", "staged_whole", "staged_split1", "groups1", "staged_pass2", "staged_split2", "groups2",
          "to_fused", "store_units", "spec_taken"]


def _code(path):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, path)).read(), flags=re.S)


def test_header_library_and_binding():
    code = _code("include/cld_mi355x.h")
    m = re.search(r"typedef\s+struct\s+cld_route_stats\s*\{(.*?)\}\s*cld_route_stats\s*;", code, flags=re.S)
    assert m, "cld_route_stats is not declared"
    body = m.group(1)
    decl = re.findall(r"uint64_t\s+([^;]+);", body)
    names = [n.strip() for part in decl for n in part.split(",")]
    assert names == FIELDS + ["reserved[6]"]
    assert re.search(r"\bint\s+cld_last_route_stats\s*\(\s*int\s+device\s*,\s*cld_route_stats\s*\*\s*st\s*\)\s*;", code)
    # cld_batch_stats keeps its layout: the benchmark and its mock read it
    assert ctypes.sizeof(cld_amd.BatchStats) == 19 * 8
    assert ctypes.sizeof(cld_amd.RouteStats) == 16 * 8
    assert [f for f, _ in cld_amd.RouteStats._fields_] == FIELDS + ["reserved"]
    assert [getattr(cld_amd.RouteStats, f).offset for f in FIELDS] == [8 * i for i in range(10)]
    assert cld_amd.RouteStats.reserved.offset == 80 and cld_amd.RouteStats.reserved.size == 48
    assert hasattr(ctypes.CDLL(cld_amd.LIB_PATH), "cld_last_route_stats")
    assert "cld_last_route_stats" in cld_amd.EXPORTS and callable(cld_amd.last_route_stats)
    assert list(cld_amd.RouteStats().as_dict()) == FIELDS


def test_argument_errors_and_the_answer_before_any_batch():
    """No device has been initialised in this process (nothing here calls
    cld_init): every device number is CLD_EINVAL, like cld_last_batch_stats,
    and the caller's record is left alone."""
    L = cld_amd.lib()
    st = cld_amd.RouteStats()
    ctypes.memset(ctypes.byref(st), 0xA5, ctypes.sizeof(st))
    for dev in (-1, 0, 1, 1 << 20):
        assert L.cld_last_route_stats(dev, ctypes.byref(st)) == cld_amd.EINVAL
        assert L.cld_last_batch_stats(dev, ctypes.byref(cld_amd.BatchStats())) == cld_amd.EINVAL
    assert L.cld_last_route_stats(0, None) == cld_amd.EINVAL
    assert bytes(st) == b"\xA5" * ctypes.sizeof(st)
    try:
        cld_amd.last_route_stats(0)
    except cld_amd.CldError as e:
        assert "cld_last_route_stats" in str(e)
    else:
        raise AssertionError("last_route_stats(0) before cld_init did not raise")
