"""The four _docflags entries (per-document is_plain_text and CLD2 flags within
one batch, include/cld_mi355x.h) without a GPU: the header declares them, the
library exports them, and the argument checks that come before cld_init --
a doc_flags word outside CLD_FLAG_HTML and the reference's public flags, a
valid_prefix array without CLD_FLAG_CHECK_UTF8, the vector entry's argument
errors -- give CLD_EINVAL."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cld_detect_batch_docflags", "cld_detect_batch_vec_docflags", "cld_detect_batch_device_docflags",
         "cld_detect_batch_device_vec_docflags")
DOCS = [b"le chat noir", b"der Hund", b"", b"<p lang=fr>bonjour</p>"]
# STRIP_EXTRAS, CSTRING, CHECK_UTF8, each also next to accepted bits, and bits nobody defines
BAD_WORDS = {"strip_extras": 1, "cstring": 2, "check_utf8": 8, "html_and_cstring": 4 | 2,
             "best_effort_and_check_utf8": 0x4000 | 8, "unknown16": 0x10, "unknown": 0x10000, "unknown31": 1 << 31}
GOOD_WORDS = (0, 4, 0x0100, 0x4000, 0x4104, 0x3E00, 0x7F04)     # (0x3E00: the ignored debug-output bits)


@pytest.fixture(scope="module")
def batch():
    import cld_amd
    buf, offs = cld_amd.pack(DOCS)
    out = np.zeros(len(DOCS), dtype=cld_amd.RESULT_DTYPE)
    return cld_amd, cld_amd.lib(), buf, offs, out


def host(batch, words, flags=0, valid_prefix=None):
    cld_amd, L, buf, offs, out = batch
    df = np.asarray(words, dtype=np.uint32)
    return L.cld_detect_batch_docflags(buf.ctypes.data, offs.ctypes.data, len(DOCS), None, df.ctypes.data, flags,
                                       out.ctypes.data, valid_prefix)


def host_vec(batch, words, flags=0, chunks=True, chunk_cap=64, chunk_offsets=True):
    cld_amd, L, buf, offs, out = batch
    df = np.asarray(words, dtype=np.uint32)
    ch = np.zeros(64, dtype=cld_amd.CHUNK_DTYPE)
    co = np.zeros(len(DOCS) + 1, dtype=np.uint64)
    return L.cld_detect_batch_vec_docflags(buf.ctypes.data, offs.ctypes.data, len(DOCS), None, df.ctypes.data, flags,
                                           out.ctypes.data, ch.ctypes.data if chunks else None, chunk_cap,
                                           co.ctypes.data if chunk_offsets else None)


def test_header_declares_and_library_exports_the_entries():
    import cld_amd
    src = open(os.path.join(ROOT, "include", "cld_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(cld_amd.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in cld_amd.EXPORTS
    # every entry takes the per-document words
    for name, arg in zip(NAMES, ("doc_flags", "doc_flags", "d_doc_flags", "d_doc_flags")):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert re.search(r"const\s+uint32_t\s*\*\s*%s\b" % arg, decl), name
    for f in ("detect_batch_docflags", "detect_batch_vec_docflags", "detect_batch_device_docflags",
              "detect_batch_device_vec_docflags"):
        assert callable(getattr(cld_amd, f))


@pytest.mark.parametrize("word", list(BAD_WORDS.values()), ids=list(BAD_WORDS))
@pytest.mark.parametrize("at", [0, len(DOCS) - 1])
def test_host_entries_reject_doc_flags_words(batch, word, at):
    cld_amd = batch[0]
    words = [GOOD_WORDS[i % len(GOOD_WORDS)] for i in range(len(DOCS))]
    words[at] = words[at] | word
    assert host(batch, words) == cld_amd.EINVAL
    assert host(batch, words, flags=cld_amd.FLAG_CHECK_UTF8 | cld_amd.FLAG_HTML) == cld_amd.EINVAL
    assert host_vec(batch, words) == cld_amd.EINVAL
    with pytest.raises(cld_amd.CldError, match="%d" % cld_amd.EINVAL):
        cld_amd.detect_batch_docflags(DOCS, doc_flags=words)
    with pytest.raises(cld_amd.CldError, match="%d" % cld_amd.EINVAL):
        cld_amd.detect_batch_vec_docflags(DOCS, doc_flags=words)


def test_valid_prefix_needs_the_check_flag(batch):
    cld_amd = batch[0]
    vp = np.zeros(len(DOCS), dtype=np.int32)
    good = list(GOOD_WORDS[:len(DOCS)])
    for flags in (0, cld_amd.FLAG_HTML | cld_amd.FLAG_BEST_EFFORT):
        assert host(batch, good, flags=flags, valid_prefix=vp.ctypes.data) == cld_amd.EINVAL
    # also where doc_flags is NULL (the call that would be forwarded)
    cld, L, buf, offs, out = batch
    assert L.cld_detect_batch_docflags(buf.ctypes.data, offs.ctypes.data, len(DOCS), None, None, 0, out.ctypes.data,
                                       vp.ctypes.data) == cld_amd.EINVAL


@pytest.mark.parametrize("flags", [1, 2, 0x10000, 1 << 31], ids=["strip_extras", "cstring", "unknown", "unknown31"])
def test_entries_reject_flags(batch, flags):
    """`flags` keeps the set of the entry each one extends (checked before cld_init)."""
    cld_amd, L = batch[0], batch[1]
    good = list(GOOD_WORDS[:len(DOCS)])
    assert host(batch, good, flags=flags) == cld_amd.EINVAL
    assert host_vec(batch, good, flags=flags) == cld_amd.EINVAL
    word = np.zeros(4, np.uint32)
    assert L.cld_detect_batch_device_docflags(0, None, None, 0, 0, None, None, 0, word.ctypes.data, None, flags,
                                              None) == cld_amd.EINVAL
    assert L.cld_detect_batch_device_vec_docflags(0, None, None, 0, 0, None, None, 0, word.ctypes.data, flags, 0, None,
                                                  None, 0, None, None, None, None) == cld_amd.EINVAL


def test_device_entry_rejects_check_utf8_and_vector_pointers(batch):
    cld_amd, L = batch[0], batch[1]
    word = np.zeros(4, np.uint32)
    # cld_detect_batch_device_hints takes no preparation flag, CLD_FLAG_CHECK_UTF8 included
    assert L.cld_detect_batch_device_docflags(0, None, None, 0, 0, None, None, 0, word.ctypes.data, None,
                                              cld_amd.FLAG_CHECK_UTF8, None) == cld_amd.EINVAL
    # cld_detect_batch_device_vec's: a valid-prefix array without the flag, room for chunks without a place for them
    vp = np.zeros(4, np.int32)
    assert L.cld_detect_batch_device_vec_docflags(0, None, None, 0, 0, None, None, 0, word.ctypes.data, 0, 0, None,
                                                  None, 0, None, vp.ctypes.data, None, None) == cld_amd.EINVAL
    assert L.cld_detect_batch_device_vec_docflags(0, None, None, 0, 0, None, None, 0, word.ctypes.data, 0, 0, None,
                                                  None, 1, None, None, None, None) == cld_amd.EINVAL


def test_vector_entry_argument_errors(batch):
    cld_amd = batch[0]
    good = list(GOOD_WORDS[:len(DOCS)])
    assert host_vec(batch, good, chunk_offsets=False) == cld_amd.EINVAL
    assert host_vec(batch, good, chunks=False, chunk_cap=1) == cld_amd.EINVAL
    cld, L, buf, offs, out = batch
    co = np.zeros(len(DOCS) + 1, dtype=np.uint64)
    df = np.asarray(good, dtype=np.uint32)
    # the batch checks of every host entry: no offsets, no result array
    assert L.cld_detect_batch_vec_docflags(buf.ctypes.data, None, len(DOCS), None, df.ctypes.data, 0, out.ctypes.data,
                                           None, 0, co.ctypes.data) == cld_amd.EINVAL
    assert L.cld_detect_batch_docflags(buf.ctypes.data, offs.ctypes.data, len(DOCS), None, df.ctypes.data, 0, None,
                                       None) == cld_amd.EINVAL


def test_wrapper_wants_one_word_per_document():
    import cld_amd
    with pytest.raises(ValueError):
        cld_amd.detect_batch_docflags(DOCS, doc_flags=[0, 4])
    with pytest.raises(ValueError):
        cld_amd.detect_batch_vec_docflags(DOCS, doc_flags=np.zeros((len(DOCS), 2), np.uint32))
