"""CLD_FLAG_SCRUB_UTF8 and the cld_scrub_utf8_* / detect_language_scrubbed
entries (include/cld_mi355x.h) without a GPU: the header declares them, the
library exports them, the bindings exist, and the argument checks that come
before cld_init give CLD_EINVAL -- the flag next to CLD_FLAG_CHECK_UTF8 in any
entry that takes both, in cld_detect_batch_checked, in a doc_flags word, and in
the two device entries that take no preparation flag."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = [b"le chat noir", b"der \xffHund", b"", b"<p lang=fr>bon\xc0jour</p>"]
N = len(DOCS)
DECLS = {"cld_scrub_utf8_host": r"\bint32_t\s+cld_scrub_utf8_host\s*\(\s*const\s+uint8_t\s*\*\s*doc\s*,\s*size_t\s+len\s*,"
                                r"\s*uint8_t\s*\*\s*out\s*\)\s*;",
         "cld_scrub_utf8_batch": r"\bint\s+cld_scrub_utf8_batch\s*\(",
         "cld_scrub_utf8_device": r"\bint\s+cld_scrub_utf8_device\s*\(\s*int\s+device\b",
         "detect_language_scrubbed": r"\bconst\s+char\s*\*\s*detect_language_scrubbed\s*\(\s*const\s+char\s*\*\s*text\s*,"
                                     r"\s*int\s*\*\s*replaced_bytes\s*\)\s*;"}


@pytest.fixture(scope="module")
def batch():
    import cld_amd
    buf, offs = cld_amd.pack(DOCS)
    out = np.zeros(N, dtype=cld_amd.RESULT_DTYPE)
    return cld_amd, cld_amd.lib(), buf, offs, out


def test_header_library_and_bindings():
    import cld_amd
    src = open(os.path.join(ROOT, "include", "cld_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+CLD_FLAG_SCRUB_UTF8\s+0x20u\b", code)
    assert cld_amd.FLAG_SCRUB_UTF8 == 0x20
    lib = ctypes.CDLL(cld_amd.LIB_PATH)
    for name, decl in DECLS.items():
        assert re.search(decl, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in cld_amd.EXPORTS
    for f in ("scrub_utf8_host", "scrub_utf8_batch", "scrub_utf8_device", "detect_language_scrubbed"):
        assert callable(getattr(cld_amd, f))
    # the reference's caution travels with the flag and with the pass (compact_lang_det.h:76-79)
    assert len(re.findall(r"U\+FFFD", src)) >= 2
    # cld_vec_status keeps its 16 bytes
    assert cld_amd.VEC_STATUS_DTYPE.itemsize == 16


def test_scrub_and_check_together_are_einval(batch):
    cld_amd, L, buf, offs, out = batch
    S, C, E = cld_amd.FLAG_SCRUB_UTF8, cld_amd.FLAG_CHECK_UTF8, cld_amd.EINVAL
    b, o, r = buf.ctypes.data, offs.ctypes.data, out.ctypes.data
    vp = np.zeros(N, np.int32)
    ch = np.zeros(64, dtype=cld_amd.CHUNK_DTYPE)
    co = np.zeros(N + 1, np.uint64)
    words = np.zeros(N, np.uint32)
    for more in (0, cld_amd.FLAG_BEST_EFFORT):
        both = S | C | more
        assert L.cld_detect_batch(b, o, N, r, both) == E
        assert L.cld_detect_batch(b, o, N, r, both | cld_amd.FLAG_STRIP_EXTRAS) == E
        assert L.cld_detect_batch_ex(b, o, N, None, both, r) == E
        assert L.cld_detect_batch_ex(b, o, N, None, both | cld_amd.FLAG_HTML, r) == E
        assert L.cld_detect_batch_vec(b, o, N, None, both, r, ch.ctypes.data, 64, co.ctypes.data) == E
        assert L.cld_detect_batch_docflags(b, o, N, None, words.ctypes.data, both, r, vp.ctypes.data) == E
        assert L.cld_detect_batch_docflags(b, o, N, None, None, both, r, None) == E
        assert L.cld_detect_batch_vec_docflags(b, o, N, None, words.ctypes.data, both, r, ch.ctypes.data, 64,
                                               co.ctypes.data) == E
        assert L.cld_detect_batch_device_ex(0, None, None, 0, 0, None, both, None) == E
        assert L.cld_detect_batch_device_vec(0, None, None, 0, 0, None, None, 0, both, 0, None, None, 0, None, None,
                                             None, None) == E
        assert L.cld_detect_batch_device_vec_docflags(0, None, None, 0, 0, None, None, 0, words.ctypes.data, both, 0,
                                                      None, None, 0, None, None, None, None) == E
        # the checked entry forces the check on: the flag is the same contradiction there
        assert L.cld_detect_batch_checked(b, o, N, None, S | more, r, vp.ctypes.data) == E
    with pytest.raises(cld_amd.CldError, match="%d" % E):
        cld_amd.detect_batch(DOCS, flags=S | C)
    with pytest.raises(cld_amd.CldError, match="%d" % E):
        cld_amd.detect_batch_checked(DOCS, flags=S)


@pytest.mark.parametrize("at", [0, N - 1])
def test_flag_in_a_doc_flags_word_is_einval(batch, at):
    cld_amd, L, buf, offs, out = batch
    S, E = cld_amd.FLAG_SCRUB_UTF8, cld_amd.EINVAL
    ch = np.zeros(64, dtype=cld_amd.CHUNK_DTYPE)
    co = np.zeros(N + 1, np.uint64)
    for word in (S, S | cld_amd.FLAG_HTML, S | cld_amd.FLAG_BEST_EFFORT):
        words = np.zeros(N, np.uint32)
        words[at] = word
        for flags in (0, S, cld_amd.FLAG_CHECK_UTF8):
            assert L.cld_detect_batch_docflags(buf.ctypes.data, offs.ctypes.data, N, None, words.ctypes.data, flags,
                                               out.ctypes.data, None) == E
            assert L.cld_detect_batch_vec_docflags(buf.ctypes.data, offs.ctypes.data, N, None, words.ctypes.data, flags,
                                                   out.ctypes.data, ch.ctypes.data, 64, co.ctypes.data) == E


def test_device_entries_without_preparation_flags_reject_it(batch):
    cld_amd, L = batch[0], batch[1]
    S, E = cld_amd.FLAG_SCRUB_UTF8, cld_amd.EINVAL
    word = np.zeros(4, np.uint32)
    for flags in (S, S | cld_amd.FLAG_HTML):
        assert L.cld_detect_batch_device_hints(0, None, None, 0, 0, None, None, 0, None, flags, None) == E
        assert L.cld_detect_batch_device_docflags(0, None, None, 0, 0, None, None, 0, word.ctypes.data, None, flags,
                                                  None) == E
        assert L.cld_detect_batch_device_docflags(0, None, None, 0, 0, None, None, 0, None, None, flags, None) == E


def test_pass_alone_argument_errors(batch):
    cld_amd, L, buf, offs, out = batch
    E = cld_amd.EINVAL
    ob = np.zeros(max(len(buf), 1), np.uint8)
    cnt = np.zeros(N, np.int32)
    assert L.cld_scrub_utf8_batch(None, None, 0, None, None) == 0                      # n == 0: CLD_OK, no GPU asked
    assert L.cld_scrub_utf8_batch(None, offs.ctypes.data, N, ob.ctypes.data, cnt.ctypes.data) == E
    assert L.cld_scrub_utf8_batch(buf.ctypes.data, None, N, ob.ctypes.data, cnt.ctypes.data) == E
    assert L.cld_scrub_utf8_batch(buf.ctypes.data, offs.ctypes.data, N, None, cnt.ctypes.data) == E
    down = offs.copy()
    down[1], down[2] = down[2], down[1]
    assert down[2] < down[1]
    assert L.cld_scrub_utf8_batch(buf.ctypes.data, down.ctypes.data, N, ob.ctypes.data, None) == E
    big = np.array([0, 1 << 31], np.uint64)                                            # a document over INT32_MAX bytes
    assert L.cld_scrub_utf8_batch(buf.ctypes.data, big.ctypes.data, 1, ob.ctypes.data, None) == E
    assert L.cld_scrub_utf8_device(0, None, offs.ctypes.data, N, ob.ctypes.data, None, None) == E
    assert L.cld_scrub_utf8_device(0, buf.ctypes.data, None, N, ob.ctypes.data, None, None) == E
    assert L.cld_scrub_utf8_device(0, buf.ctypes.data, offs.ctypes.data, N, None, None, None) == E
    assert L.cld_scrub_utf8_device(0, buf.ctypes.data, offs.ctypes.data, 1 << 31, ob.ctypes.data, None, None) == E
    # a flagged batch with such a document, as with the check
    for f in (cld_amd.FLAG_SCRUB_UTF8, cld_amd.FLAG_SCRUB_UTF8 | cld_amd.FLAG_HTML):
        assert L.cld_detect_batch_ex(buf.ctypes.data, big.ctypes.data, 1, None, f, out.ctypes.data) == E
    assert L.cld_detect_batch(buf.ctypes.data, big.ctypes.data, 1, out.ctypes.data, cld_amd.FLAG_SCRUB_UTF8) == E
    assert len(cld_amd.scrub_utf8_batch([])[0]) == 0


def test_valid_prefix_goes_with_either_flag(batch):
    """cld_detect_batch_docflags takes the array with the scrub flag as with the check:
    no CLD_EINVAL from the argument checks (without a GPU the call then fails in cld_init)."""
    cld_amd, L, buf, offs, out = batch
    vp = np.zeros(N, np.int32)
    words = np.zeros(N, np.uint32)
    assert L.cld_detect_batch_docflags(buf.ctypes.data, offs.ctypes.data, N, None, words.ctypes.data, 0, out.ctypes.data,
                                       vp.ctypes.data) == cld_amd.EINVAL
    assert L.cld_detect_batch_docflags(None, None, 0, None, None, cld_amd.FLAG_SCRUB_UTF8, None, None) == 0
    assert L.cld_detect_batch_device_vec(0, None, None, 0, 0, None, None, 0, 0, 0, None, None, 0, None, vp.ctypes.data,
                                         None, None) == cld_amd.EINVAL
