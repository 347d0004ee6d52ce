"""Python host binding of libcld_mi355x.so (the C ABI in include/cld_mi355x.h).

Mirrors the reference's caller-facing interface for this path:
  detect_language(text) -> ISO code       main.go:77-81 Detect_language / wrapper.cc:7-16
  detect_batch(docs)    -> cld_result[]   one DetectLanguageSummaryV2 per document
  prepare_batch(docs, flags)              handlers.go:150-151: StripExtras (handlers.go:198-210)
                                          + the cgo C-string cut, as a GPU kernel
  load_data_from_file(path)               CLD2::loadDataFromFile (run-time tables)
  detect_batch_checked(docs)              ExtDetectLanguageSummaryCheckUTF8 per document
                                          (compact_lang_det.cc:317-355) -> (results, valid prefixes)
  detect_language_checked(text)           DetectLanguageCheckUTF8 (compact_lang_det.cc:44-56)
  valid_prefix_batch(docs)                SpanInterchangeValid per document, as a GPU kernel
  detect_batch(docs, flags=FLAG_SCRUB_UTF8)   ill-formed bytes repaired (each error position of the
                                          check becomes a space) and every document scored
  scrub_utf8_batch(docs)                  that repair alone, as a GPU kernel -> (buffer, replaced)
  group_by_language(results)              counts, stable order and group offsets per language (host reference)
  group_by_language_device / gather_docs_device   the same over results in HBM, and the chosen
                                          documents packed into a new device batch
  chunk_totals / gather_chunks            per-language totals over chunk vectors, and the pieces in chosen
                                          languages packed into a new batch (host references)
  chunk_totals_device / gather_chunks_device      the same over a batch and its vectors in HBM
  split_lines / lines_to_chunks           a batch's lines as a new offsets array over the same text, and
                                          per-line results as one chunk vector per document (host references)
  split_lines_device / lines_to_chunks_device     the same over a batch in HBM: line-level detection
  html_text / chunks_to_page              the text of HTML pages (tags to separators, entities decoded), page-aligned,
                                          with each byte's position in its page; chunk vectors on the text
                                          carried back to byte ranges of the page (host references)
  html_text_device / chunks_to_page_device        the same over pages in HBM: HTML in front of the line,
                                          chunk and group entries
  detect_language_scrubbed(text)          the repair on the host, then detect_language
There is no CPU fallback: if the HIP library or a GPU is missing, calls raise.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CLD_MI355X_LIB") or os.path.join(HERE, "build", "libcld_mi355x.so")
# Product default: Q0, the empty quadgram table (cld_version() says "quad=empty-Q0").
# Tests and the benchmark opt into the synthetic Q1 table through CLD_MI355X_TABLES.
Q0_TABLES = os.path.join(HERE, "data", "cld2_q0.cldt")
SYNTH_TABLES = os.path.join(HERE, "data", "cld2_synth_q1.cldt")
FLAG_STRIP_EXTRAS = 1      # include/cld_mi355x.h CLD_FLAG_STRIP_EXTRAS
FLAG_CSTRING = 2           # include/cld_mi355x.h CLD_FLAG_CSTRING
FLAG_HTML = 4              # include/cld_mi355x.h CLD_FLAG_HTML (cld_detect_batch_ex)
FLAG_CHECK_UTF8 = 8        # include/cld_mi355x.h CLD_FLAG_CHECK_UTF8: documents that are not interchange-valid are not scored
FLAG_SCRUB_UTF8 = 0x20     # include/cld_mi355x.h CLD_FLAG_SCRUB_UTF8: error positions of the check become 0x20, every document is scored
VALID_TILE = 1024          # csrc/cld_kernels.h kValidTile: the check's tile (documents over VALID_SHORT_MAX bytes)
VALID_SHORT_MAX = 256      # csrc/cld_kernels.h kValidShortMax
FLAG_SCORE_AS_QUADS = 0x0100   # CLD_FLAG_SCORE_AS_QUADS = kCLDFlagScoreAsQuads (compact_lang_det.h:343)
FLAG_BEST_EFFORT = 0x4000      # CLD_FLAG_BEST_EFFORT = kCLDFlagBestEffort (compact_lang_det.h:349)
UNKNOWN_ENCODING = 23      # encodings.h UNKNOWN_ENCODING
UNKNOWN_LANGUAGE = 26      # generated_language.h UNKNOWN_LANGUAGE
LANG_FAILED = 0xFFFF       # include/cld_mi355x.h CLD_LANG_FAILED: a document without a result
EIO, ENOMEM, ENOSPC, EINVAL = -5, -12, -28, -22   # include/cld_mi355x.h error codes
NUM_LANGUAGES = 614        # include/cld_mi355x.h CLD_NUM_LANGUAGES: Language values 0..613
GROUP_BINS = 615           # include/cld_mi355x.h CLD_GROUP_BINS: bin 614 takes every key >= 614 (LANG_FAILED too)
GROUP_TOP1 = 1             # include/cld_mi355x.h CLD_GROUP_TOP1: the key is lang3[0], not summary_lang
GROUP_RELIABLE_ONLY = 2    # include/cld_mi355x.h CLD_GROUP_RELIABLE_ONLY: unreliable documents get key UNKNOWN_LANGUAGE
GROUP_WGS = 256            # csrc/cld_kernels.h kGroupWgs: the group entries cut a batch into at most this many ranges
GROUP_TILE = 512           # csrc/cld_kernels.h kGroupTile: documents per step of a range's workgroup
CHUNKS_SPACE = 1           # include/cld_mi355x.h CLD_CHUNKS_SPACE: a 0x20 before a kept piece that does not continue the one before

RESULT_DTYPE = np.dtype([("lang3", "<u2", 3), ("summary_lang", "<u2"), ("percent3", "i1", 3),
                         ("is_reliable", "u1"), ("text_bytes", "<i4"), ("normalized3", "<f8", 3)])
assert RESULT_DTYPE.itemsize == 40

# Every symbol include/cld_mi355x.h declares (checked by tests/test_capi.py)
EXPORTS = ("detect_language", "cld_init", "cld_init_device", "cld_shutdown", "cld_detect_batch",
           "cld_detect_batch_device", "cld_plan_shards", "cld_kernel_time", "cld_language_code",
           "cld_language_name", "cld_last_batch_stats", "cld_version", "cld_stage_cycles",
           "cld_load_data_from_file", "cld_load_data_from_raw_address", "cld_unload_data",
           "cld_is_data_dynamic", "cld_export_tables", "cld_convert_data_file",
           "cld_detect_batch_device_ex", "cld_prepare_batch", "cld_host_alloc", "cld_host_free",
           "cld_kernel_times", "cld_detect_batch_ex", "cld_hint_priors", "cld_detect_batch_vec",
           "cld_detect_batch_checked", "cld_valid_prefix_host", "cld_valid_prefix_batch",
           "cld_valid_prefix_device", "detect_language_checked", "cld_hint_boosts_device",
           "cld_detect_batch_device_hints", "cld_detect_batch_device_vec", "cld_detect_batch_docflags",
           "cld_detect_batch_vec_docflags", "cld_detect_batch_device_docflags",
           "cld_detect_batch_device_vec_docflags", "cld_scrub_utf8_host", "cld_scrub_utf8_batch",
           "cld_scrub_utf8_device", "detect_language_scrubbed", "cld_group_work_bytes", "cld_group_by_language",
           "cld_group_by_language_device", "cld_gather_docs_device", "cld_last_route_stats", "cld_chunk_work_bytes",
           "cld_chunk_totals", "cld_chunk_totals_device", "cld_gather_chunks", "cld_gather_chunks_device",
           "cld_lines_work_bytes", "cld_split_lines", "cld_split_lines_device", "cld_lines_to_chunks",
           "cld_lines_to_chunks_device", "cld_html_text", "cld_html_text_device", "cld_chunks_to_page",
           "cld_chunks_to_page_device")
CHUNK_DTYPE = np.dtype([("offset", "<i4"), ("bytes", "<i4"), ("lang1", "<u2"), ("pad", "<u2")])   # cld_chunk
LINES_JOIN_BLANK = 1       # include/cld_mi355x.h CLD_LINES_JOIN_BLANK: blank lines join the line after them
LINES_TILE = 1024          # csrc/cld_kernels.h kLinesTile: the text bytes one wave of the split reads
LINES_WGS = 256            # csrc/cld_kernels.h kLinesWgs: the split scans its tiles in at most this many ranges
LINES_STATUS_DTYPE = np.dtype([("total_lines", "<u8"), ("max_line_bytes", "<u8")])   # cld_lines_status
HTMLTEXT_BLOCK_LF = 1      # include/cld_mi355x.h CLD_HTMLTEXT_BLOCK_LF: a block tag's separator byte is 0x0A, not 0x20
HTMLTEXT_STAGE = 2048      # csrc/cld_kernels.h kHtmlTextStage: pages up to this size are staged in LDS, longer ones read in place
HTMLTEXT_CANDS = 256       # csrc/cld_kernels.h kHtmlTextCands: '<' / '&' candidates per segment of a page
# include/cld_mi355x.h cld_htmltext_status
HTMLTEXT_STATUS_DTYPE = np.dtype([("text_bytes", "<u8"), ("tags", "<u8"), ("entities", "<u4"), ("dropped", "<u4")])
assert HTMLTEXT_STATUS_DTYPE.itemsize == 24


class Hints(ctypes.Structure):
    """CLDHints (compact_lang_det.h:134-139) = include/cld_mi355x.h cld_hints."""
    _fields_ = [("content_language_hint", ctypes.c_char_p), ("tld_hint", ctypes.c_char_p),
                ("encoding_hint", ctypes.c_int32), ("language_hint", ctypes.c_int32)]

    @classmethod
    def make(cls, content_language=None, tld=None, encoding=UNKNOWN_ENCODING, language=UNKNOWN_LANGUAGE):
        enc = lambda v: v.encode() if isinstance(v, str) else v
        return cls(enc(content_language), enc(tld), encoding, language)


# include/cld_mi355x.h cld_hints_dev: CLDHints without pointers, for hints that live in device memory
HINTS_DEV_DTYPE = np.dtype([("content_language_off", "<u4"), ("content_language_len", "<u4"), ("tld", "S4"),
                            ("encoding_hint", "<i4"), ("language_hint", "<i4")])
assert HINTS_DEV_DTYPE.itemsize == 20


# include/cld_mi355x.h cld_vec_status: what cld_detect_batch_device_vec leaves in d_status
VEC_STATUS_DTYPE = np.dtype([("total_chunks", "<u8"), ("failed_docs", "<u4"), ("rejected_docs", "<u4")])
assert VEC_STATUS_DTYPE.itemsize == 16


def pack_hints(hints, n=None):
    """list of Hints (None: no hint for that document) -> (HINTS_DEV_DTYPE[n], uint8 text):
    the records cld_hint_boosts_device / cld_detect_batch_device_hints take, and the
    buffer their content-language texts lie in, each followed by a NUL.  A TLD longer
    than 3 bytes keeps its first 4, which marks it as ignored (as the reference ignores it)."""
    if n is not None and len(hints) != n:
        raise ValueError("need one Hints per document")
    rec = np.zeros(len(hints), dtype=HINTS_DEV_DTYPE)
    rec["encoding_hint"] = UNKNOWN_ENCODING
    rec["language_hint"] = UNKNOWN_LANGUAGE
    text = bytearray()
    for i, h in enumerate(hints):
        if h is None:
            continue
        cl = h.content_language_hint or b""
        if cl:
            rec["content_language_off"][i] = len(text)
            rec["content_language_len"][i] = len(cl)
            text += cl + b"\0"
        rec["tld"][i] = (h.tld_hint or b"")[:4]
        rec["encoding_hint"][i] = h.encoding_hint
        rec["language_hint"][i] = h.language_hint
    return rec, np.frombuffer(bytes(text), dtype=np.uint8)


class BatchStats(ctypes.Structure):
    _fields_ = [("docs", ctypes.c_uint64), ("short_docs", ctypes.c_uint64), ("general_docs", ctypes.c_uint64),
                ("passes", ctypes.c_uint64 * 4), ("short_ms", ctypes.c_double), ("general_ms", ctypes.c_double),
                ("long_docs", ctypes.c_uint64), ("long_ms", ctypes.c_double),
                ("long_requeue", ctypes.c_uint64 * 8)]


class RouteStats(ctypes.Structure):
    """include/cld_mi355x.h cld_route_stats: which long-document kernels scored the last batch."""
    FIELDS = ("long_list", "staged_whole", "staged_split1", "groups1", "staged_pass2", "staged_split2", "groups2",
              "to_fused", "store_units", "spec_taken")
    _fields_ = [(f, ctypes.c_uint64) for f in FIELDS] + [("reserved", ctypes.c_uint64 * 6)]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f in self.FIELDS}


class CldError(RuntimeError):
    pass


class PartialBatchError(CldError):
    """CLD_EIO from a batch call: every result is complete except the documents
    in `failed` (summary_lang == LANG_FAILED), which the GPU could not score even
    alone.  `value` is what the call would have returned."""

    def __init__(self, what, value, failed):
        super().__init__("%s: %d document(s) without a result" % (what, int(np.count_nonzero(failed))))
        self.value = value
        self.failed = failed


def build():
    subprocess.run(["make", "-s", "-C", HERE], check=True)


_lib = None


def lib():
    """Load the in-tree HIP library (never a fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CldError("libcld_mi355x.so is not built (run __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        L.detect_language.argtypes = [ctypes.c_char_p]
        L.detect_language.restype = ctypes.c_char_p
        L.cld_init.argtypes = [ctypes.c_char_p, ctypes.c_int]
        L.cld_detect_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32]
        L.cld_detect_batch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_void_p]
        L.cld_language_code.restype = ctypes.c_char_p
        L.cld_language_name.restype = ctypes.c_char_p
        L.cld_version.restype = ctypes.c_char_p
        L.cld_last_batch_stats.argtypes = [ctypes.c_int, ctypes.POINTER(BatchStats)]
        L.cld_last_route_stats.argtypes = [ctypes.c_int, ctypes.POINTER(RouteStats)]
        L.cld_init_device.argtypes = [ctypes.c_char_p, ctypes.c_int]
        L.cld_plan_shards.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        L.cld_kernel_time.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
        L.cld_kernel_times.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
        L.cld_prepare_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                        ctypes.c_void_p, ctypes.c_void_p]
        L.cld_detect_batch_device_ex.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                 ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        L.cld_load_data_from_file.argtypes = [ctypes.c_char_p]
        L.cld_load_data_from_raw_address.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.cld_export_tables.argtypes = [ctypes.c_char_p]
        L.cld_convert_data_file.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
        L.cld_host_alloc.argtypes = [ctypes.c_size_t]
        L.cld_host_alloc.restype = ctypes.c_void_p
        L.cld_host_free.argtypes = [ctypes.c_void_p]
        L.cld_detect_batch_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                          ctypes.c_uint32, ctypes.c_void_p]
        L.cld_detect_batch_vec.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                           ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.c_void_p]
        L.cld_hint_priors.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(Hints),
                                      ctypes.c_void_p, ctypes.c_void_p]
        L.cld_detect_batch_checked.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                               ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.cld_valid_prefix_host.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        L.cld_valid_prefix_host.restype = ctypes.c_int32
        L.cld_valid_prefix_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.cld_valid_prefix_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_void_p]
        L.cld_hint_boosts_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.cld_detect_batch_device_hints.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                    ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                    ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        L.cld_detect_batch_device_vec.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                  ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p]
        vp, sz, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64
        L.cld_detect_batch_docflags.argtypes = [vp, vp, sz, vp, vp, u32, vp, vp]
        L.cld_detect_batch_vec_docflags.argtypes = [vp, vp, sz, vp, vp, u32, vp, vp, sz, vp]
        L.cld_detect_batch_device_docflags.argtypes = [ctypes.c_int, vp, vp, sz, u64, vp, vp, u64, vp, vp, u32, vp]
        L.cld_detect_batch_device_vec_docflags.argtypes = [ctypes.c_int, vp, vp, sz, u64, vp, vp, u64, vp, u32,
                                                           ctypes.c_int, vp, vp, u64, vp, vp, vp, vp]
        L.detect_language_checked.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
        L.detect_language_checked.restype = ctypes.c_char_p
        L.cld_scrub_utf8_host.argtypes = [vp, sz, vp]
        L.cld_scrub_utf8_host.restype = ctypes.c_int32
        L.cld_scrub_utf8_batch.argtypes = [vp, vp, sz, vp, vp]
        L.cld_scrub_utf8_device.argtypes = [ctypes.c_int, vp, vp, sz, vp, vp, vp]
        L.detect_language_scrubbed.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
        L.detect_language_scrubbed.restype = ctypes.c_char_p
        L.cld_group_work_bytes.argtypes = [sz]
        L.cld_group_work_bytes.restype = sz
        L.cld_group_by_language.argtypes = [vp, sz, u32, vp, vp, vp, vp, vp]
        L.cld_group_by_language_device.argtypes = [ctypes.c_int, vp, sz, u32, vp, vp, vp, vp, vp, vp, sz, vp]
        L.cld_gather_docs_device.argtypes = [ctypes.c_int, vp, vp, sz, vp, sz, vp, u64, vp, vp, sz, vp]
        L.cld_chunk_work_bytes.argtypes = [sz, u64]
        L.cld_chunk_work_bytes.restype = sz
        L.cld_chunk_totals.argtypes = [vp, sz, vp, u64, vp, vp, vp]
        L.cld_chunk_totals_device.argtypes = [ctypes.c_int, vp, sz, vp, u64, vp, vp, vp, vp, sz, vp]
        L.cld_gather_chunks.argtypes = [vp, vp, sz, vp, u64, vp, vp, u32, vp, u64, vp]
        L.cld_gather_chunks_device.argtypes = [ctypes.c_int, vp, vp, sz, vp, u64, vp, vp, u32, vp, u64, vp, vp, sz, vp]
        L.cld_lines_work_bytes.argtypes = [sz, u64]
        L.cld_lines_work_bytes.restype = sz
        L.cld_split_lines.argtypes = [vp, vp, sz, u32, vp, vp, u64, vp, vp]
        L.cld_split_lines_device.argtypes = [ctypes.c_int, vp, vp, sz, u64, u32, vp, vp, u64, vp, vp, vp, sz, vp]
        L.cld_lines_to_chunks.argtypes = [vp, vp, vp, u64, vp, sz, vp, u32, vp]
        L.cld_lines_to_chunks_device.argtypes = [ctypes.c_int, vp, vp, vp, u64, vp, sz, vp, u32, vp, vp]
        L.cld_html_text.argtypes = [vp, vp, sz, u32, vp, vp, vp, vp]
        L.cld_html_text_device.argtypes = [ctypes.c_int, vp, vp, sz, u64, u32, vp, vp, vp, vp, vp]
        L.cld_chunks_to_page.argtypes = [vp, sz, vp, vp, u64, vp, vp]
        L.cld_chunks_to_page_device.argtypes = [ctypes.c_int, vp, sz, vp, vp, u64, vp, vp, vp]
        _lib = L
    return _lib


def load_data_from_file(path):
    """CLD2::loadDataFromFile (compact_lang_det.h:393): scoring tables from a cld2_data_file00."""
    rc = lib().cld_load_data_from_file(path.encode())
    if rc != 0:
        raise CldError("cld_load_data_from_file(%s) failed: %d" % (path, rc))


def load_data_from_raw_address(data):
    """CLD2::loadDataFromRawAddress (compact_lang_det.h:406) over a bytes-like image."""
    b = bytes(data)
    rc = lib().cld_load_data_from_raw_address(ctypes.c_char_p(b), len(b))
    if rc != 0:
        raise CldError("cld_load_data_from_raw_address failed: %d" % rc)


def unload_data():
    rc = lib().cld_unload_data()
    if rc != 0:
        raise CldError("cld_unload_data failed: %d" % rc)


def is_data_dynamic():
    return bool(lib().cld_is_data_dynamic())


def export_tables(path):
    rc = lib().cld_export_tables(path.encode())
    if rc != 0:
        raise CldError("cld_export_tables failed: %d" % rc)


def convert_data_file(data_file, out_cldt, base_cldt=None):
    """cld2_data_file00 + base CLDT -> CLDT file (host only, no GPU)."""
    rc = lib().cld_convert_data_file(data_file.encode(), base_cldt.encode() if base_cldt else None,
                                     out_cldt.encode())
    if rc != 0:
        raise CldError("cld_convert_data_file(%s) failed: %d" % (data_file, rc))


def init(tables=None, n_devices=0):
    rc = lib().cld_init(tables.encode() if tables else None, n_devices)
    if rc != 0:
        raise CldError("cld_init failed: %d" % rc)


def init_device(device, tables=None):
    """One process per GPU: bind the runtime to HIP device `device` (context 0)."""
    rc = lib().cld_init_device(tables.encode() if tables else None, device)
    if rc != 0:
        raise CldError("cld_init_device(%d) failed: %d" % (device, rc))


def plan_shards(offsets, nshards):
    """Contiguous document shards of equal estimated kernel cost (cld_plan_shards; host-only, no GPU)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    cuts = np.zeros(nshards + 1, dtype=np.uint64)
    rc = lib().cld_plan_shards(offsets.ctypes.data, len(offsets) - 1, nshards, cuts.ctypes.data)
    if rc != 0:
        raise CldError("cld_plan_shards failed: %d" % rc)
    return cuts.astype(np.int64)


def kernel_time(ctx=0):
    """(short_ms, general_ms, launches) summed over batches since the last call."""
    a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    rc = lib().cld_kernel_time(ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n))
    if rc != 0:
        raise CldError("cld_kernel_time failed: %d" % rc)
    return a.value, b.value, n.value


def kernel_times(ctx=0):
    """([wave_ms, long_ms, general_ms], launches) summed over batches since the last call."""
    ms = (ctypes.c_double * 3)()
    n = ctypes.c_int()
    rc = lib().cld_kernel_times(ctx, ms, ctypes.byref(n))
    if rc != 0:
        raise CldError("cld_kernel_times failed: %d" % rc)
    return [ms[0], ms[1], ms[2]], n.value


def stage_cycles(ctx=0):
    """Per-stage cycle sums of the wavefront kernel (CLD_PROFILE_STAGES=1)."""
    c = np.zeros(16, dtype=np.uint64)
    rc = lib().cld_stage_cycles(ctx, ctypes.c_void_p(c.ctypes.data))
    if rc != 0:
        raise CldError("cld_stage_cycles failed: %d" % rc)
    return c


def pack(docs):
    """list of str/bytes -> (uint8 buffer, uint64 offsets[n+1])."""
    bs = [d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in bs], out=offs[1:])
    buf = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, np.uint8)
    return buf, offs


def detect_batch(docs=None, buf=None, offsets=None, flags=0, out=None):
    """One DetectLanguageSummaryV2 per document; flags = FLAG_STRIP_EXTRAS | FLAG_CSTRING
    prepares each text as POST / does before detecting (handlers.go:150-151);
    FLAG_CHECK_UTF8 rejects and FLAG_SCRUB_UTF8 repairs what is not interchange-valid
    UTF-8 (one of the two); FLAG_SCORE_AS_QUADS / FLAG_BEST_EFFORT are CLD2's own flags.  out: an
    existing contiguous RESULT_DTYPE array of n entries to fill (a caller that
    reuses its result buffer, as a service would), else a new one."""
    if docs is not None:
        buf, offsets = pack(docs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    if out is None:
        out = np.zeros(n, dtype=RESULT_DTYPE)
    elif out.dtype != RESULT_DTYPE or out.shape != (n,) or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
        raise ValueError("out must be a writeable contiguous array of %d RESULT_DTYPE entries" % n)
    if n == 0:
        return out
    bptr = buf.ctypes.data if buf.size else ctypes.addressof(ctypes.c_uint8(0))
    rc = lib().cld_detect_batch(bptr, offsets.ctypes.data, n, out.ctypes.data, flags)
    if rc == EIO:
        raise PartialBatchError("cld_detect_batch", out, out["summary_lang"] == LANG_FAILED)
    if rc != 0:
        raise CldError("cld_detect_batch failed: %d" % rc)
    return out


def detect_batch_ex(docs=None, buf=None, offsets=None, hints=None, html=False, flags=0):
    """ExtDetectLanguageSummary per document (compact_lang_det.h:324-335):
    html=True scores every document as HTML (is_plain_text = false); hints is
    None or one Hints per document; flags: FLAG_SCORE_AS_QUADS / FLAG_BEST_EFFORT and
    FLAG_CHECK_UTF8 or FLAG_SCRUB_UTF8."""
    if docs is not None:
        buf, offsets = pack(docs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    out = np.zeros(n, dtype=RESULT_DTYPE)
    if n == 0:
        return out
    harr = None
    if hints is not None:
        if len(hints) != n:
            raise ValueError("need one Hints per document")
        harr = (Hints * n)(*hints)
    bptr = buf.ctypes.data if buf.size else ctypes.addressof(ctypes.c_uint8(0))
    rc = lib().cld_detect_batch_ex(bptr, offsets.ctypes.data, n, ctypes.cast(harr, ctypes.c_void_p) if harr else None,
                                   (FLAG_HTML if html else 0) | flags, out.ctypes.data)
    if rc == EIO:
        raise PartialBatchError("cld_detect_batch_ex", out, out["summary_lang"] == LANG_FAILED)
    if rc != 0:
        raise CldError("cld_detect_batch_ex failed: %d" % rc)
    return out


def detect_batch_vec(docs=None, buf=None, offsets=None, hints=None, html=False, chunk_cap=None, flags=0):
    """ExtDetectLanguageSummary with a ResultChunkVector per document:
    (results, chunks [CHUNK_DTYPE], chunk_offsets[n+1]); document i's vector is
    chunks[chunk_offsets[i]:chunk_offsets[i+1]].  flags as for detect_batch_ex."""
    if docs is not None:
        buf, offsets = pack(docs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    out = np.zeros(n, dtype=RESULT_DTYPE)
    coffs = np.zeros(n + 1, dtype=np.uint64)
    if n == 0:
        return out, np.zeros(0, dtype=CHUNK_DTYPE), coffs
    harr = None
    if hints is not None:
        if len(hints) != n:
            raise ValueError("need one Hints per document")
        harr = (Hints * n)(*hints)
    cap = chunk_cap if chunk_cap is not None else 4 * n + 1024
    bptr = buf.ctypes.data if buf.size else ctypes.addressof(ctypes.c_uint8(0))
    for _ in range(2):                                     # second try with the exact size
        chunks = np.zeros(max(cap, 1), dtype=CHUNK_DTYPE)
        rc = lib().cld_detect_batch_vec(bptr, offsets.ctypes.data, n,
                                        ctypes.cast(harr, ctypes.c_void_p) if harr else None,
                                        (FLAG_HTML if html else 0) | flags, out.ctypes.data, chunks.ctypes.data, cap,
                                        coffs.ctypes.data)
        if rc == 0:
            return out, chunks[:int(coffs[-1])], coffs
        if rc == EIO:                                      # some document got no vector (an empty one)
            raise PartialBatchError("cld_detect_batch_vec", (out, chunks[:int(coffs[-1])], coffs),
                                    out["summary_lang"] == LANG_FAILED)
        if rc != ENOSPC or chunk_cap is not None:
            break
        cap = int(coffs[-1])
    raise CldError("cld_detect_batch_vec failed: %d" % rc)


def hint_priors(doc=b"", html=False, hints=None):
    """Host-only ApplyHints (compact_lang_det_impl.cc:1587-1684): (priors, boosts16).
    priors: the trimmed CLDLangPriors as int16 (weight << 10) + language;
    boosts16: prior boosts latn[4] othr[4], whacks latn[4] othr[4] as langprobs."""
    b = doc.encode() if isinstance(doc, str) else bytes(doc)
    p = np.zeros(14, dtype=np.int16)
    q = np.zeros(16, dtype=np.uint32)
    cb = ctypes.create_string_buffer(b, len(b) + 1)
    rc = lib().cld_hint_priors(cb, len(b), 0 if html else 1, ctypes.byref(hints) if hints is not None else None,
                               p.ctypes.data, q.ctypes.data)
    if rc < 0:
        raise CldError("cld_hint_priors failed: %d" % rc)
    return p[:rc].copy(), q


def detect_batch_device(device, d_buf_ptr, d_offsets_ptr, n, d_out_ptr, stream_ptr=None):
    rc = lib().cld_detect_batch_device(device, d_buf_ptr, d_offsets_ptr, n, d_out_ptr, stream_ptr)
    if rc != 0:
        raise CldError("cld_detect_batch_device failed: %d" % rc)


def hint_boosts_device(device, d_buf_ptr, d_offsets_ptr, n, d_hints_ptr=None, d_hint_text_ptr=None, hint_text_bytes=0,
                       plain=True, d_priors14_ptr=None, d_boosts16_ptr=None, stream_ptr=None):
    """cld_hint_boosts_device: ApplyHints as a GPU kernel, every pointer in device memory
    (d_hints_ptr: HINTS_DEV_DTYPE records, see pack_hints); asynchronous on the stream.
    d_priors14_ptr: int16[n, 14], d_boosts16_ptr: uint32[n, 16]; either may be None."""
    rc = lib().cld_hint_boosts_device(device, d_buf_ptr, d_offsets_ptr, n, d_hints_ptr, d_hint_text_ptr,
                                      hint_text_bytes, 1 if plain else 0, d_priors14_ptr, d_boosts16_ptr, stream_ptr)
    if rc != 0:
        raise CldError("cld_hint_boosts_device failed: %d" % rc)


def detect_batch_device_hints(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_out_ptr, d_hints_ptr=None,
                              d_hint_text_ptr=None, hint_text_bytes=0, flags=0, stream_ptr=None):
    """cld_detect_batch_device_hints: detect_batch_ex for device-resident input.  flags:
    FLAG_HTML, FLAG_SCORE_AS_QUADS, FLAG_BEST_EFFORT; asynchronous on the stream."""
    rc = lib().cld_detect_batch_device_hints(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_hints_ptr,
                                             d_hint_text_ptr, hint_text_bytes, d_out_ptr, flags, stream_ptr)
    if rc != 0:
        raise CldError("cld_detect_batch_device_hints failed: %d" % rc)


def detect_batch_device_vec(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_out_ptr, d_chunks_ptr, chunk_cap,
                            d_chunk_offsets_ptr, d_status_ptr, d_hints_ptr=None, d_hint_text_ptr=None,
                            hint_text_bytes=0, flags=0, big_regions=False, d_valid_prefix_ptr=None, stream_ptr=None):
    """cld_detect_batch_device_vec: detect_batch_vec for device-resident input, asynchronous on
    the stream.  d_out_ptr: RESULT_DTYPE[n], d_chunk_offsets_ptr: uint64[n + 1], d_status_ptr: one
    VEC_STATUS_DTYPE record, d_chunks_ptr: CHUNK_DTYPE[chunk_cap] (None with chunk_cap 0: the
    sizing pass -- read total_chunks from the status, allocate, call again).  flags: FLAG_HTML,
    FLAG_CHECK_UTF8 or FLAG_SCRUB_UTF8 (d_valid_prefix_ptr: int32[n] or None; rejected_docs of the
    status counts the rejected / the repaired documents), FLAG_SCORE_AS_QUADS, FLAG_BEST_EFFORT.
    Documents counted in failed_docs (summary_lang == LANG_FAILED, empty vector) are redone
    with big_regions=True or through detect_batch_vec."""
    rc = lib().cld_detect_batch_device_vec(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_hints_ptr,
                                           d_hint_text_ptr, hint_text_bytes, flags, 1 if big_regions else 0,
                                           d_out_ptr, d_chunks_ptr, chunk_cap, d_chunk_offsets_ptr,
                                           d_valid_prefix_ptr, d_status_ptr, stream_ptr)
    if rc != 0:
        raise CldError("cld_detect_batch_device_vec failed: %d" % rc)


def _doc_flags(doc_flags, n):
    """doc_flags of the _docflags entries: None, or one uint32 word per document."""
    if doc_flags is None:
        return None
    a = np.ascontiguousarray(doc_flags, dtype=np.uint32)
    if a.shape != (n,):
        raise ValueError("need one doc_flags word per document")
    return a


def detect_batch_docflags(docs=None, buf=None, offsets=None, hints=None, doc_flags=None, flags=0, valid_prefix=False):
    """cld_detect_batch_docflags: detect_batch_ex with is_plain_text and CLD2's flags per
    document -- document i is scored with flags | doc_flags[i] (FLAG_HTML, FLAG_SCORE_AS_QUADS,
    FLAG_BEST_EFFORT; doc_flags: uint32[n] or None).  flags as for detect_batch_ex; with
    FLAG_CHECK_UTF8 or FLAG_SCRUB_UTF8 and valid_prefix=True -> (results, valid_prefix int32[n]),
    the prefixes of the documents as given."""
    if docs is not None:
        buf, offsets = pack(docs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    out = np.zeros(n, dtype=RESULT_DTYPE)
    vp = np.zeros(n, dtype=np.int32) if valid_prefix else None
    df = _doc_flags(doc_flags, n)
    harr = None
    if hints is not None:
        if len(hints) != n:
            raise ValueError("need one Hints per document")
        harr = (Hints * n)(*hints) if n else None
    bptr = buf.ctypes.data if buf.size else ctypes.addressof(ctypes.c_uint8(0))
    rc = lib().cld_detect_batch_docflags(bptr, offsets.ctypes.data, n,
                                         ctypes.cast(harr, ctypes.c_void_p) if harr else None,
                                         df.ctypes.data if df is not None and n else None, flags, out.ctypes.data,
                                         vp.ctypes.data if vp is not None else None)
    value = (out, vp) if valid_prefix else out
    if rc == EIO:
        raise PartialBatchError("cld_detect_batch_docflags", value, out["summary_lang"] == LANG_FAILED)
    if rc != 0:
        raise CldError("cld_detect_batch_docflags failed: %d" % rc)
    return value


def detect_batch_vec_docflags(docs=None, buf=None, offsets=None, hints=None, doc_flags=None, chunk_cap=None, flags=0):
    """cld_detect_batch_vec_docflags: detect_batch_vec with is_plain_text and CLD2's flags per
    document (doc_flags: uint32[n] or None, as for detect_batch_docflags)."""
    if docs is not None:
        buf, offsets = pack(docs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    out = np.zeros(n, dtype=RESULT_DTYPE)
    coffs = np.zeros(n + 1, dtype=np.uint64)
    if n == 0:
        return out, np.zeros(0, dtype=CHUNK_DTYPE), coffs
    df = _doc_flags(doc_flags, n)
    harr = None
    if hints is not None:
        if len(hints) != n:
            raise ValueError("need one Hints per document")
        harr = (Hints * n)(*hints)
    cap = chunk_cap if chunk_cap is not None else 4 * n + 1024
    bptr = buf.ctypes.data if buf.size else ctypes.addressof(ctypes.c_uint8(0))
    for _ in range(2):                                     # second try with the exact size
        chunks = np.zeros(max(cap, 1), dtype=CHUNK_DTYPE)
        rc = lib().cld_detect_batch_vec_docflags(bptr, offsets.ctypes.data, n,
                                                 ctypes.cast(harr, ctypes.c_void_p) if harr else None,
                                                 df.ctypes.data if df is not None else None, flags, out.ctypes.data,
                                                 chunks.ctypes.data, cap, coffs.ctypes.data)
        if rc == 0:
            return out, chunks[:int(coffs[-1])], coffs
        if rc == EIO:                                      # some document got no vector (an empty one)
            raise PartialBatchError("cld_detect_batch_vec_docflags", (out, chunks[:int(coffs[-1])], coffs),
                                    out["summary_lang"] == LANG_FAILED)
        if rc != ENOSPC or chunk_cap is not None:
            break
        cap = int(coffs[-1])
    raise CldError("cld_detect_batch_vec_docflags failed: %d" % rc)


def detect_batch_device_docflags(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_out_ptr, d_doc_flags_ptr=None,
                                 d_hints_ptr=None, d_hint_text_ptr=None, hint_text_bytes=0, flags=0, stream_ptr=None):
    """cld_detect_batch_device_docflags: detect_batch_device_hints with d_doc_flags_ptr, uint32[n]
    in device memory (None: exactly that call); the kernel masks each word to FLAG_HTML |
    FLAG_SCORE_AS_QUADS | FLAG_BEST_EFFORT."""
    rc = lib().cld_detect_batch_device_docflags(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_hints_ptr,
                                                d_hint_text_ptr, hint_text_bytes, d_doc_flags_ptr, d_out_ptr, flags,
                                                stream_ptr)
    if rc != 0:
        raise CldError("cld_detect_batch_device_docflags failed: %d" % rc)


def detect_batch_device_vec_docflags(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_out_ptr, d_chunks_ptr,
                                     chunk_cap, d_chunk_offsets_ptr, d_status_ptr, d_doc_flags_ptr=None,
                                     d_hints_ptr=None, d_hint_text_ptr=None, hint_text_bytes=0, flags=0,
                                     big_regions=False, d_valid_prefix_ptr=None, stream_ptr=None):
    """cld_detect_batch_device_vec_docflags: detect_batch_device_vec with d_doc_flags_ptr,
    uint32[n] in device memory (None: exactly that call)."""
    rc = lib().cld_detect_batch_device_vec_docflags(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_hints_ptr,
                                                    d_hint_text_ptr, hint_text_bytes, d_doc_flags_ptr, flags,
                                                    1 if big_regions else 0, d_out_ptr, d_chunks_ptr, chunk_cap,
                                                    d_chunk_offsets_ptr, d_valid_prefix_ptr, d_status_ptr, stream_ptr)
    if rc != 0:
        raise CldError("cld_detect_batch_device_vec_docflags failed: %d" % rc)


def last_stats(device=0):
    st = BatchStats()
    rc = lib().cld_last_batch_stats(device, ctypes.byref(st))
    if rc != 0:
        raise CldError("cld_last_batch_stats failed: %d" % rc)
    return st


def last_route_stats(device=0):
    """The routes the last batch's long documents took (RouteStats; cld_last_route_stats)."""
    st = RouteStats()
    rc = lib().cld_last_route_stats(device, ctypes.byref(st))
    if rc != 0:
        raise CldError("cld_last_route_stats failed: %d" % rc)
    return st


def detect_language(text):
    """main.go:77-81 / wrapper.cc:7-16: NUL-terminated text -> ISO code ('en' for unknown)."""
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    return lib().detect_language(b).decode()


def detect_language_checked(text):
    """DetectLanguageCheckUTF8 (compact_lang_det.cc:44-56) -> (ISO code, valid_prefix_bytes):
    a text that is not interchange-valid UTF-8 is not scored and gets 'un'."""
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    vp = ctypes.c_int(0)
    code = lib().detect_language_checked(b, ctypes.byref(vp)).decode()
    return code, vp.value


def detect_language_scrubbed(text):
    """detect_language of the text with every error position of the UTF-8 check replaced
    by a space (FLAG_SCRUB_UTF8, on the host) -> (ISO code, replaced_bytes)."""
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    r = ctypes.c_int(0)
    code = lib().detect_language_scrubbed(b, ctypes.byref(r)).decode()
    return code, r.value


def scrub_utf8_host(doc):
    """scrub(doc) on the host (cld_scrub_utf8_host, no GPU) -> (bytes, replaced): doc with each
    byte at an error position of the interchange-valid check replaced by 0x20."""
    b = doc.encode("utf-8") if isinstance(doc, str) else bytes(doc)
    out = ctypes.create_string_buffer(max(len(b), 1))
    rc = lib().cld_scrub_utf8_host(b, len(b), out)
    if rc < 0:
        raise CldError("cld_scrub_utf8_host failed: %d" % rc)
    return out.raw[:len(b)], rc


def scrub_utf8_batch(docs=None, buf=None, offsets=None, replaced=True):
    """scrub() per document on the GPU (cld_scrub_utf8_batch) -> (uint8 buffer of
    offsets[n] - offsets[0] bytes, indexed like the input from its first document on,
    replaced int32[n] or None).  The input is not written."""
    if docs is not None:
        buf, offsets = pack(docs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    out = np.zeros(int(offsets[n] - offsets[0]) if n > 0 else 0, dtype=np.uint8)
    cnt = np.zeros(n, dtype=np.int32) if replaced else None
    bptr = buf.ctypes.data if buf.size else ctypes.addressof(ctypes.c_uint8(0))
    optr = out.ctypes.data if out.size else ctypes.addressof(ctypes.c_uint8(0))
    rc = lib().cld_scrub_utf8_batch(bptr, offsets.ctypes.data, n, optr, cnt.ctypes.data if replaced else None)
    if rc != 0:
        raise CldError("cld_scrub_utf8_batch failed: %d" % rc)
    return out, cnt


def scrub_utf8_device(device, d_buf_ptr, d_offsets_ptr, n, d_out_ptr, d_replaced_ptr=None, stream_ptr=None):
    """cld_scrub_utf8_device: every pointer in device memory (d_out indexed like d_buf,
    d_replaced int32[n] or None); asynchronous on the stream."""
    rc = lib().cld_scrub_utf8_device(device, d_buf_ptr, d_offsets_ptr, n, d_out_ptr, d_replaced_ptr, stream_ptr)
    if rc != 0:
        raise CldError("cld_scrub_utf8_device failed: %d" % rc)


def group_range(n):
    """Documents per workgroup range of the group entries for n documents (csrc/cld_kernels.h cld_group_range)."""
    per = -(-n // GROUP_WGS)
    return max(GROUP_TILE, -(-per // GROUP_TILE) * GROUP_TILE)


def group_work_bytes(n):
    """cld_group_work_bytes: the workspace either device entry needs for n documents."""
    return int(lib().cld_group_work_bytes(n))


def group_by_language(results, offsets=None, flags=0):
    """cld_group_by_language (the host reference, no GPU) over a RESULT_DTYPE array -> dict of
    counts uint64[GROUP_BINS], group_offsets uint64[GROUP_BINS + 1], order uint32[n] (document
    indices sorted by (bin, index)) and, with offsets, bin_bytes uint64[GROUP_BINS].
    flags: GROUP_TOP1 | GROUP_RELIABLE_ONLY."""
    results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
    n = len(results)
    got = {"counts": np.zeros(GROUP_BINS, np.uint64), "group_offsets": np.zeros(GROUP_BINS + 1, np.uint64),
           "order": np.zeros(n, np.uint32)}
    optr = bptr = None
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(offsets) != n + 1:
            raise ValueError("need n + 1 offsets")
        got["bin_bytes"] = np.zeros(GROUP_BINS, np.uint64)
        optr, bptr = offsets.ctypes.data, got["bin_bytes"].ctypes.data
    rc = lib().cld_group_by_language(results.ctypes.data, n, flags, optr, got["counts"].ctypes.data, bptr,
                                     got["order"].ctypes.data, got["group_offsets"].ctypes.data)
    if rc != 0:
        raise CldError("cld_group_by_language failed: %d" % rc)
    return got


def group_by_language_device(device, d_results_ptr, n, d_counts_ptr, d_work_ptr, work_bytes, flags=0,
                             d_offsets_ptr=None, d_bin_bytes_ptr=None, d_order_ptr=None, d_group_offsets_ptr=None,
                             stream_ptr=None):
    """cld_group_by_language_device: every pointer in device memory (results cld_result[n],
    counts / bin_bytes uint64[GROUP_BINS], order uint32[n], group_offsets uint64[GROUP_BINS + 1],
    a workspace of group_work_bytes(n)); asynchronous on the stream."""
    rc = lib().cld_group_by_language_device(device, d_results_ptr, n, flags, d_offsets_ptr, d_counts_ptr,
                                            d_bin_bytes_ptr, d_order_ptr, d_group_offsets_ptr, d_work_ptr, work_bytes,
                                            stream_ptr)
    if rc != 0:
        raise CldError("cld_group_by_language_device failed: %d" % rc)


def gather_docs_device(device, d_buf_ptr, d_offsets_ptr, n_src, d_index_ptr, m, d_out_buf_ptr, out_cap,
                       d_out_offsets_ptr, d_work_ptr, work_bytes, stream_ptr=None):
    """cld_gather_docs_device: documents d_index[0..m) of the device batch packed into
    (d_out_buf, d_out_offsets uint64[m + 1]); out_cap 0 with no buffer sizes the output.
    A workspace of group_work_bytes(m); asynchronous on the stream."""
    rc = lib().cld_gather_docs_device(device, d_buf_ptr, d_offsets_ptr, n_src, d_index_ptr, m, d_out_buf_ptr, out_cap,
                                      d_out_offsets_ptr, d_work_ptr, work_bytes, stream_ptr)
    if rc != 0:
        raise CldError("cld_gather_docs_device failed: %d" % rc)


def chunk_work_bytes(n, chunk_cap):
    """cld_chunk_work_bytes: the workspace either chunk device entry needs: 8 * (chunk_cap + 1) bytes and a fixed part."""
    return int(lib().cld_chunk_work_bytes(n, chunk_cap))


def _chunk_args(offsets, chunks, chunk_offsets, chunk_cap):
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    chunk_offsets = np.ascontiguousarray(chunk_offsets, dtype=np.uint64)
    chunks = np.ascontiguousarray(chunks, dtype=CHUNK_DTYPE)
    if len(offsets) < 1 or len(chunk_offsets) != len(offsets):
        raise ValueError("need n + 1 offsets and n + 1 chunk offsets")
    cap = len(chunks) if chunk_cap is None else int(chunk_cap)
    if cap > len(chunks):
        raise ValueError("chunk_cap is more than the chunks given")
    return offsets, chunks, chunk_offsets, cap


def chunk_totals(offsets, chunks, chunk_offsets, chunk_cap=None):
    """cld_chunk_totals (the host reference, no GPU) over a batch's offsets and its vectors (a CHUNK_DTYPE
    array and chunk_offsets, as detect_batch_vec returns them; chunk_cap: the chunks that exist, default
    all given) -> dict of chunk_counts and chunk_bytes, uint64[GROUP_BINS] each."""
    offsets, chunks, chunk_offsets, cap = _chunk_args(offsets, chunks, chunk_offsets, chunk_cap)
    got = {"chunk_counts": np.zeros(GROUP_BINS, np.uint64), "chunk_bytes": np.zeros(GROUP_BINS, np.uint64)}
    rc = lib().cld_chunk_totals(offsets.ctypes.data, len(offsets) - 1, chunks.ctypes.data, cap, chunk_offsets.ctypes.data,
                                got["chunk_counts"].ctypes.data, got["chunk_bytes"].ctypes.data)
    if rc != 0:
        raise CldError("cld_chunk_totals failed: %d" % rc)
    return got


def gather_chunks(buf, offsets, chunks, chunk_offsets, select, flags=0, chunk_cap=None, out_cap=None):
    """cld_gather_chunks (the host reference, no GPU): the pieces of every document whose bin is set in
    select (GROUP_BINS bytes, nonzero: keep) packed into a new batch -> (buffer, offsets uint64[n + 1]).
    flags: CHUNKS_SPACE.  out_cap: the buffer's size (default: the sizing pass first, then all of it);
    the offsets are the true totals either way."""
    offsets, chunks, chunk_offsets, cap = _chunk_args(offsets, chunks, chunk_offsets, chunk_cap)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    select = np.ascontiguousarray(select, dtype=np.uint8)
    if len(select) != GROUP_BINS:
        raise ValueError("select holds one byte per bin")
    n = len(offsets) - 1
    out_offsets = np.zeros(n + 1, np.uint64)

    def call(out, out_bytes):
        rc = lib().cld_gather_chunks(buf.ctypes.data, offsets.ctypes.data, n, chunks.ctypes.data, cap,
                                     chunk_offsets.ctypes.data, select.ctypes.data, flags,
                                     out.ctypes.data if out_bytes else None, out_bytes, out_offsets.ctypes.data)
        if rc != 0:
            raise CldError("cld_gather_chunks failed: %d" % rc)

    if out_cap is None:
        call(None, 0)
        out_cap = int(out_offsets[n])
    out = np.zeros(out_cap, np.uint8)
    call(out, out_cap)
    return out[:min(out_cap, int(out_offsets[n]))], out_offsets


def chunk_totals_device(device, d_offsets_ptr, n, d_chunks_ptr, chunk_cap, d_chunk_offsets_ptr, d_work_ptr, work_bytes,
                        d_chunk_counts_ptr=None, d_chunk_bytes_ptr=None, stream_ptr=None):
    """cld_chunk_totals_device: every pointer in device memory (the batch's offsets, cld_chunk[chunk_cap],
    chunk_offsets uint64[n + 1], counts / bytes uint64[GROUP_BINS], a workspace of
    chunk_work_bytes(n, chunk_cap)); asynchronous on the stream."""
    rc = lib().cld_chunk_totals_device(device, d_offsets_ptr, n, d_chunks_ptr, chunk_cap, d_chunk_offsets_ptr,
                                       d_chunk_counts_ptr, d_chunk_bytes_ptr, d_work_ptr, work_bytes, stream_ptr)
    if rc != 0:
        raise CldError("cld_chunk_totals_device failed: %d" % rc)


def gather_chunks_device(device, d_buf_ptr, d_offsets_ptr, n, d_chunks_ptr, chunk_cap, d_chunk_offsets_ptr, d_select_ptr,
                         d_out_buf_ptr, out_cap, d_out_offsets_ptr, d_work_ptr, work_bytes, flags=0, stream_ptr=None):
    """cld_gather_chunks_device: the pieces in the selected bins (d_select: GROUP_BINS bytes) of the device
    batch packed into (d_out_buf, d_out_offsets uint64[n + 1]); out_cap 0 with no buffer sizes the output.
    flags: CHUNKS_SPACE.  A workspace of chunk_work_bytes(n, chunk_cap); asynchronous on the stream."""
    rc = lib().cld_gather_chunks_device(device, d_buf_ptr, d_offsets_ptr, n, d_chunks_ptr, chunk_cap,
                                        d_chunk_offsets_ptr, d_select_ptr, flags, d_out_buf_ptr, out_cap,
                                        d_out_offsets_ptr, d_work_ptr, work_bytes, stream_ptr)
    if rc != 0:
        raise CldError("cld_gather_chunks_device failed: %d" % rc)


def lines_work_bytes(n, buf_bytes):
    """cld_lines_work_bytes: the workspace cld_split_lines_device needs: one word per LINES_TILE bytes and a fixed part."""
    return int(lib().cld_lines_work_bytes(n, buf_bytes))


def split_lines(buf, offsets, flags=0, line_cap=None):
    """cld_split_lines (the host reference, no GPU): the batch's lines, each with its LF, as a new offsets
    array over the same buffer -> dict of line_offsets uint64[min(m, line_cap) + 1], line_doc
    uint32[min(m, line_cap)], doc_lines uint64[n + 1] and status (a LINES_STATUS_DTYPE record).
    flags: LINES_JOIN_BLANK.  line_cap: the room for lines (default: the sizing pass first, then all of
    them); doc_lines and status are the true values either way."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) < 1:
        raise ValueError("need n + 1 offsets")
    n = len(offsets) - 1
    doc_lines = np.zeros(n + 1, np.uint64)
    status = np.zeros(1, LINES_STATUS_DTYPE)

    def call(lo, ld, cap):
        rc = lib().cld_split_lines(buf.ctypes.data, offsets.ctypes.data, n, flags, lo.ctypes.data if lo is not None else None,
                                   ld.ctypes.data if ld is not None else None, cap, doc_lines.ctypes.data,
                                   status.ctypes.data)
        if rc != 0:
            raise CldError("cld_split_lines failed: %d" % rc)

    if line_cap is None:
        call(None, None, 0)
        line_cap = int(status[0]["total_lines"])
    line_offsets = np.zeros(line_cap + 1, np.uint64)
    line_doc = np.zeros(max(line_cap, 1), np.uint32)
    call(line_offsets, line_doc, line_cap)
    m = min(int(status[0]["total_lines"]), line_cap)
    return {"line_offsets": line_offsets[:m + 1], "line_doc": line_doc[:m], "doc_lines": doc_lines, "status": status[0]}


def split_lines_device(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_line_offsets_ptr, d_line_doc_ptr, line_cap,
                       d_doc_lines_ptr, d_work_ptr, work_bytes, flags=0, d_status_ptr=None, stream_ptr=None):
    """cld_split_lines_device: every pointer in device memory (line_offsets uint64[line_cap + 1], line_doc
    uint32[line_cap] or None, doc_lines uint64[n + 1], status a LINES_STATUS_DTYPE record or None, a
    workspace of lines_work_bytes(n, buf_bytes)); line_cap 0 with no line_offsets sizes the output.
    flags: LINES_JOIN_BLANK.  Asynchronous on the stream."""
    rc = lib().cld_split_lines_device(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, flags, d_line_offsets_ptr,
                                      d_line_doc_ptr, line_cap, d_doc_lines_ptr, d_status_ptr, d_work_ptr, work_bytes,
                                      stream_ptr)
    if rc != 0:
        raise CldError("cld_split_lines_device failed: %d" % rc)


def lines_to_chunks(line_results, line_offsets, line_doc, offsets, doc_lines, flags=0, line_cap=None):
    """cld_lines_to_chunks (the host reference, no GPU): the results of a line batch (RESULT_DTYPE, one per
    line) as one CHUNK_DTYPE vector per document of the original batch; the vectors' chunk offsets are
    doc_lines itself.  flags: GROUP_TOP1 | GROUP_RELIABLE_ONLY.  line_cap: the lines that exist (default:
    all of line_doc) -> CHUNK_DTYPE[min(doc_lines[n], line_cap)]."""
    line_results = np.ascontiguousarray(line_results, dtype=RESULT_DTYPE)
    line_offsets = np.ascontiguousarray(line_offsets, dtype=np.uint64)
    line_doc = np.ascontiguousarray(line_doc, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    doc_lines = np.ascontiguousarray(doc_lines, dtype=np.uint64)
    if len(offsets) < 1 or len(doc_lines) != len(offsets):
        raise ValueError("need n + 1 offsets and n + 1 doc_lines")
    cap = len(line_doc) if line_cap is None else int(line_cap)
    if cap > len(line_doc) or cap > len(line_results) or cap + 1 > len(line_offsets) + (cap == 0):
        raise ValueError("line_cap is more than the lines given")
    n = len(offsets) - 1
    m = min(int(doc_lines[n]), cap)
    chunks = np.zeros(max(m, 1), CHUNK_DTYPE)
    rc = lib().cld_lines_to_chunks(line_results.ctypes.data, line_offsets.ctypes.data, line_doc.ctypes.data, cap,
                                   offsets.ctypes.data, n, doc_lines.ctypes.data, flags, chunks.ctypes.data)
    if rc != 0:
        raise CldError("cld_lines_to_chunks failed: %d" % rc)
    return chunks[:m]


def lines_to_chunks_device(device, d_line_results_ptr, d_line_offsets_ptr, d_line_doc_ptr, line_cap, d_offsets_ptr, n,
                           d_doc_lines_ptr, d_chunks_ptr, flags=0, stream_ptr=None):
    """cld_lines_to_chunks_device: every pointer in device memory (results cld_result[line_cap], line_offsets
    uint64[line_cap + 1], line_doc uint32[line_cap], the original batch's offsets and doc_lines uint64[n + 1],
    chunks cld_chunk[line_cap]); asynchronous on the stream."""
    rc = lib().cld_lines_to_chunks_device(device, d_line_results_ptr, d_line_offsets_ptr, d_line_doc_ptr, line_cap,
                                          d_offsets_ptr, n, d_doc_lines_ptr, flags, d_chunks_ptr, stream_ptr)
    if rc != 0:
        raise CldError("cld_lines_to_chunks_device failed: %d" % rc)


def html_text(buf, offsets, flags=0, pos=False):
    """cld_html_text (the host reference, no GPU): the text of every HTML page of the batch, page-aligned ->
    dict of out (uint8, indexed like buf: page i's text at offsets[i], then 0x20 to the page's end), text_len
    int32[n], status (an HTMLTEXT_STATUS_DTYPE record) and, with pos=True, pos (uint32 per output byte: its
    position in its page, the page's length at the padding).  flags: HTMLTEXT_BLOCK_LF."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) < 1:
        raise ValueError("need n + 1 offsets")
    n = len(offsets) - 1
    size = max(len(buf), int(offsets.max()))
    got = {"out": np.zeros(size, np.uint8), "text_len": np.zeros(n, np.int32), "status": np.zeros(1, HTMLTEXT_STATUS_DTYPE)}
    if pos:
        got["pos"] = np.zeros(size, np.uint32)
    rc = lib().cld_html_text(buf.ctypes.data, offsets.ctypes.data, n, flags, got["out"].ctypes.data,
                             got["text_len"].ctypes.data, got["pos"].ctypes.data if pos else None,
                             got["status"].ctypes.data)
    if rc != 0:
        raise CldError("cld_html_text failed: %d" % rc)
    got["status"] = got["status"][0]
    return got


def html_text_device(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, d_out_ptr, flags=0, d_text_len_ptr=None,
                     d_pos_ptr=None, d_status_ptr=None, stream_ptr=None):
    """cld_html_text_device: every pointer in device memory (out uint8[buf_bytes], indexed like the pages and
    not overlapping them; text_len int32[n], pos uint32[buf_bytes], status an HTMLTEXT_STATUS_DTYPE record,
    each or None); no workspace; asynchronous on the stream.  flags: HTMLTEXT_BLOCK_LF."""
    rc = lib().cld_html_text_device(device, d_buf_ptr, d_offsets_ptr, n, buf_bytes, flags, d_out_ptr, d_text_len_ptr,
                                    d_pos_ptr, d_status_ptr, stream_ptr)
    if rc != 0:
        raise CldError("cld_html_text_device failed: %d" % rc)


def chunks_to_page(offsets, pos, chunks, chunk_offsets, chunk_cap=None):
    """cld_chunks_to_page (the host reference, no GPU): chunk vectors that index the text of html_text
    (CHUNK_DTYPE and chunk_offsets, as for chunk_totals) rewritten to index the pages, through pos ->
    CHUNK_DTYPE[chunk_cap]; chunks that do not exist stay zero."""
    offsets, chunks, chunk_offsets, cap = _chunk_args(offsets, chunks, chunk_offsets, chunk_cap)
    pos = np.ascontiguousarray(pos, dtype=np.uint32)
    out = np.zeros(max(cap, 1), CHUNK_DTYPE)
    rc = lib().cld_chunks_to_page(offsets.ctypes.data, len(offsets) - 1, pos.ctypes.data, chunks.ctypes.data, cap,
                                  chunk_offsets.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise CldError("cld_chunks_to_page failed: %d" % rc)
    return out[:cap]


def chunks_to_page_device(device, d_offsets_ptr, n, d_pos_ptr, d_chunks_ptr, chunk_cap, d_chunk_offsets_ptr,
                          d_out_chunks_ptr, stream_ptr=None):
    """cld_chunks_to_page_device: every pointer in device memory (the pages' offsets, pos as html_text_device
    wrote it, cld_chunk[chunk_cap] on the text, chunk_offsets uint64[n + 1], the output cld_chunk[chunk_cap],
    which may be the input); asynchronous on the stream."""
    rc = lib().cld_chunks_to_page_device(device, d_offsets_ptr, n, d_pos_ptr, d_chunks_ptr, chunk_cap,
                                         d_chunk_offsets_ptr, d_out_chunks_ptr, stream_ptr)
    if rc != 0:
        raise CldError("cld_chunks_to_page_device failed: %d" % rc)


def valid_prefix_host(doc):
    """SpanInterchangeValid (compact_lang_det_impl.cc:72-80) of one document, on the host (no GPU)."""
    b = doc.encode("utf-8") if isinstance(doc, str) else bytes(doc)
    rc = lib().cld_valid_prefix_host(b, len(b))
    if rc < 0:
        raise CldError("cld_valid_prefix_host failed: %d" % rc)
    return rc


def valid_prefix_batch(docs=None, buf=None, offsets=None):
    """SpanInterchangeValid per document on the GPU (cld_valid_prefix_batch) -> int32[n]."""
    if docs is not None:
        buf, offsets = pack(docs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    vp = np.zeros(n, dtype=np.int32)
    bptr = buf.ctypes.data if buf.size else ctypes.addressof(ctypes.c_uint8(0))
    rc = lib().cld_valid_prefix_batch(bptr, offsets.ctypes.data, n, vp.ctypes.data)
    if rc != 0:
        raise CldError("cld_valid_prefix_batch failed: %d" % rc)
    return vp


def valid_prefix_device(device, d_buf_ptr, d_offsets_ptr, n, d_valid_prefix_ptr, stream_ptr=None):
    """cld_valid_prefix_device: every pointer in device memory; asynchronous on the stream."""
    rc = lib().cld_valid_prefix_device(device, d_buf_ptr, d_offsets_ptr, n, d_valid_prefix_ptr, stream_ptr)
    if rc != 0:
        raise CldError("cld_valid_prefix_device failed: %d" % rc)


def detect_batch_checked(docs=None, buf=None, offsets=None, hints=None, html=False, flags=0):
    """ExtDetectLanguageSummaryCheckUTF8 per document (compact_lang_det.cc:317-355) ->
    (results, valid_prefix int32[n]).  Document i was scored iff valid_prefix[i] is its
    length; else results[i] is the reference's "rejected" result (UNKNOWN, zeros)."""
    if docs is not None:
        buf, offsets = pack(docs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    out = np.zeros(n, dtype=RESULT_DTYPE)
    vp = np.zeros(n, dtype=np.int32)
    harr = None
    if hints is not None:
        if len(hints) != n:
            raise ValueError("need one Hints per document")
        harr = (Hints * n)(*hints) if n else None
    bptr = buf.ctypes.data if buf.size else ctypes.addressof(ctypes.c_uint8(0))
    rc = lib().cld_detect_batch_checked(bptr, offsets.ctypes.data, n,
                                        ctypes.cast(harr, ctypes.c_void_p) if harr else None,
                                        (FLAG_HTML if html else 0) | flags, out.ctypes.data, vp.ctypes.data)
    if rc == EIO:
        raise PartialBatchError("cld_detect_batch_checked", (out, vp), out["summary_lang"] == LANG_FAILED)
    if rc != 0:
        raise CldError("cld_detect_batch_checked failed: %d" % rc)
    return out, vp


def version():
    return lib().cld_version().decode()


def host_array(n, dtype):
    """numpy array of n elements in pinned host memory (cld_host_alloc): a
    cld_detect_batch on such buffers skips the staging copy.  The memory is
    released with the array."""
    dtype = np.dtype(dtype)
    nbytes = max(1, n * dtype.itemsize)
    p = lib().cld_host_alloc(nbytes)
    if not p:
        raise CldError("cld_host_alloc(%d) failed" % nbytes)
    raw = (ctypes.c_uint8 * nbytes).from_address(p)
    arr = np.frombuffer(raw, dtype=np.uint8)[:n * dtype.itemsize].view(dtype)
    import weakref
    weakref.finalize(raw, lib().cld_host_free, p)
    return arr


def language_code(lang):
    return lib().cld_language_code(int(lang)).decode()


ENGLISH, UNKNOWN_LANGUAGE = 0, 26     # generated_language.h Language enum values


def result_code(r):
    """compact_lang_det.cc:91-93 + wrapper.cc:14: the ISO code detect_language() returns
    for a cld_result (UNKNOWN -> ENGLISH)."""
    lang = int(r["summary_lang"])
    return language_code(ENGLISH if lang == UNKNOWN_LANGUAGE else lang)


def language_name(lang):
    return lib().cld_language_name(int(lang)).decode()


def prepare_batch(docs=None, buf=None, offsets=None, flags=FLAG_STRIP_EXTRAS | FLAG_CSTRING):
    """handlers.go:150-151 text preparation on the GPU (cld_prepare_batch):
    StripExtras (handlers.go:198-210) and/or the cgo C-string cut.  -> (buf, offsets)."""
    if docs is not None:
        buf, offsets = pack(docs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    out = np.zeros(int(offsets[-1] - offsets[0]) + n + 1, dtype=np.uint8)
    oo = np.zeros(n + 1, dtype=np.uint64)
    bptr = buf.ctypes.data if buf.size else ctypes.addressof(ctypes.c_uint8(0))
    rc = lib().cld_prepare_batch(bptr, offsets.ctypes.data, n, flags, out.ctypes.data, oo.ctypes.data)
    if rc != 0:
        raise CldError("cld_prepare_batch failed: %d" % rc)
    return out[:int(oo[-1])], oo


def strip_extras(text):
    """handlers.go:198-210 StripExtras for one text (GPU kernel, no C-string cut)."""
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    out, oo = prepare_batch([b], flags=FLAG_STRIP_EXTRAS)
    r = bytes(out[:int(oo[1])])
    return r.decode("utf-8", "surrogateescape") if isinstance(text, str) else r
