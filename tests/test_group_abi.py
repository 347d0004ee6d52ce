"""The group entries (include/cld_mi355x.h) without a GPU: the header declares
them, the library exports them, the bindings exist, and the argument checks of
the two device entries that come before cld_init give CLD_EINVAL / CLD_ENOSPC."""
import ctypes
import os
import re

import numpy as np

import cld_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, NOSPC = cld_amd.EINVAL, cld_amd.ENOSPC
DECLS = {"cld_group_work_bytes": r"\bsize_t\s+cld_group_work_bytes\s*\(\s*size_t\s+n\s*\)\s*;",
         "cld_group_by_language": r"\bint\s+cld_group_by_language\s*\(\s*const\s+cld_result\s*\*\s*results\b",
         "cld_group_by_language_device": r"\bint\s+cld_group_by_language_device\s*\(\s*int\s+device\b",
         "cld_gather_docs_device": r"\bint\s+cld_gather_docs_device\s*\(\s*int\s+device\b"}


def test_header_library_and_bindings():
    src = open(os.path.join(ROOT, "include", "cld_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, value in (("CLD_NUM_LANGUAGES", "614u"), ("CLD_GROUP_BINS", "615u"), ("CLD_GROUP_TOP1", "1u"),
                        ("CLD_GROUP_RELIABLE_ONLY", "2u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    assert (cld_amd.NUM_LANGUAGES, cld_amd.GROUP_BINS, cld_amd.GROUP_TOP1, cld_amd.GROUP_RELIABLE_ONLY) == (614, 615, 1, 2)
    lib = ctypes.CDLL(cld_amd.LIB_PATH)
    for name, decl in DECLS.items():
        assert re.search(decl, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in cld_amd.EXPORTS
    for f in ("group_by_language", "group_by_language_device", "gather_docs_device", "group_work_bytes"):
        assert callable(getattr(cld_amd, f))
    # the Python copy of the decomposition is the kernels' (csrc/cld_kernels.h)
    hdr = open(os.path.join(ROOT, "language-detector_amd", "csrc", "cld_kernels.h")).read()
    assert re.search(r"kGroupWgs\s*=\s*%d\s*;" % cld_amd.GROUP_WGS, hdr)
    assert re.search(r"kGroupTile\s*=\s*%d\s*;" % cld_amd.GROUP_TILE, hdr)
    assert [cld_amd.group_range(n) for n in (1, 512, 131072, 131073, 200003, 1 << 20)] == [512, 512, 512, 1024, 1024, 4096]


def host_buffers(n):
    """Host arrays standing in for device memory: the checks under test return before any of it is read."""
    return {"res": np.zeros(n, cld_amd.RESULT_DTYPE), "offs": np.zeros(n + 1, np.uint64),
            "counts": np.zeros(615, np.uint64), "bytes": np.zeros(615, np.uint64), "order": np.zeros(n, np.uint32),
            "goffs": np.zeros(616, np.uint64), "work": np.zeros(cld_amd.group_work_bytes(n) // 8 + 1, np.uint64)}


def test_group_device_argument_errors():
    L, n = cld_amd.lib(), 9
    h = host_buffers(n)
    p = {k: v.ctypes.data for k, v in h.items()}
    wb = cld_amd.group_work_bytes(n)
    group = L.cld_group_by_language_device
    for bit in (4, 0x10, 0x80000000):
        assert group(0, p["res"], n, bit, p["offs"], p["counts"], p["bytes"], p["order"], p["goffs"], p["work"], wb,
                     None) == E
        assert group(0, None, 0, bit | cld_amd.GROUP_TOP1, None, None, None, None, None, None, 0, None) == E
    assert group(0, p["res"], n, 0, None, p["counts"], p["bytes"], p["order"], p["goffs"], p["work"], wb, None) == E
    assert group(0, None, 0, 0, None, None, p["bytes"], None, None, None, 0, None) == E     # bin_bytes without offsets
    assert group(0, None, n, 0, p["offs"], p["counts"], None, None, None, p["work"], wb, None) == E
    assert group(0, p["res"], n, 0, p["offs"], None, None, None, None, p["work"], wb, None) == E
    assert group(0, p["res"], n, 0, p["offs"], p["counts"], None, None, None, None, wb, None) == E
    assert group(0, p["res"], n, 0, p["offs"], p["counts"], None, None, None, p["work"] + 4, wb, None) == E
    assert group(0, p["res"], 1 << 31, 0, p["offs"], p["counts"], None, None, None, p["work"], 1 << 40, None) == E
    for short in (0, 1, wb - 1):
        assert group(0, p["res"], n, 0, p["offs"], p["counts"], p["bytes"], p["order"], p["goffs"], p["work"], short,
                     None) == NOSPC
    assert all(not v.view(np.uint8).any() for v in h.values())


def test_gather_device_argument_errors():
    L, n = cld_amd.lib(), 9
    h = host_buffers(n)
    p = {k: v.ctypes.data for k, v in h.items()}
    wb = cld_amd.group_work_bytes(n)
    buf = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint8)
    b, o = buf.ctypes.data, out.ctypes.data
    gather = L.cld_gather_docs_device
    assert gather(0, None, p["offs"], n, p["order"], n, o, 64, p["goffs"], p["work"], wb, None) == E
    assert gather(0, b, None, n, p["order"], n, o, 64, p["goffs"], p["work"], wb, None) == E
    assert gather(0, b, p["offs"], n, None, n, o, 64, p["goffs"], p["work"], wb, None) == E
    assert gather(0, b, p["offs"], n, p["order"], n, None, 64, p["goffs"], p["work"], wb, None) == E   # a capacity, no buffer
    assert gather(0, b, p["offs"], n, p["order"], n, o, 64, None, p["work"], wb, None) == E
    assert gather(0, b, p["offs"], n, p["order"], n, o, 64, p["goffs"], None, wb, None) == E
    assert gather(0, b, p["offs"], n, p["order"], n, o, 64, p["goffs"], p["work"] + 1, wb, None) == E
    assert gather(0, b, p["offs"], n, p["order"], 1 << 31, o, 64, p["goffs"], p["work"], 1 << 40, None) == E
    assert gather(0, b, p["offs"], 1 << 31, p["order"], n, o, 64, p["goffs"], p["work"], wb, None) == E
    assert gather(0, None, None, 0, None, 0, None, 64, None, None, 0, None) == E
    for cap, ob in ((64, o), (0, None)):                                       # the sizing pass needs its workspace too
        for short in (0, wb - 1):
            assert gather(0, b, p["offs"], n, p["order"], n, ob, cap, p["goffs"], p["work"], short, None) == NOSPC
    assert all(not v.view(np.uint8).any() for v in h.values()) and not out.any()
