/*
 * cld_mi355x.h -- C ABI of the MI355X-native CLD2-compatible language
 * detector (libcld_mi355x.so).  Plain C types only: no HIP or torch types.
 *
 * Drop-in for the reference's cgo boundary:
 *   detect_language()          replaces wrapper.h:8 / wrapper.cc:7-16
 *                              (called from main.go:77-81, handlers.go:151)
 * Batch boundary (new, same semantics per document):
 *   cld_detect_batch()         one DetectLanguageSummaryV2 per document
 *                              (compact_lang_det_impl.cc:1707-2106) with
 *                              plain text, no hints, flags 0 -- exactly what
 *                              wrapper.cc:9-12 asks CLD2 for.
 */
#ifndef CLD_MI355X_H_
#define CLD_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-document result: the out-parameters of DetectLanguageSummaryV2
 * (compact_lang_det_impl.cc:1707-1720).  40 bytes, naturally aligned. */
typedef struct cld_result {
  uint16_t lang3[3];        /* top-3 Language enum values; UNKNOWN_LANGUAGE (26) if absent */
  uint16_t summary_lang;    /* V2 return value (UNKNOWN is NOT mapped to ENGLISH here)     */
  int8_t percent3[3];       /* percent of text bytes per language                          */
  uint8_t is_reliable;      /* 0/1                                                         */
  int32_t text_bytes;       /* letters-only text bytes scored                              */
  double normalized3[3];    /* (score << 10) / bytes per language                          */
} cld_result;

/* Error codes (negative errno style) */
#define CLD_OK 0
#define CLD_EINVAL (-22)
#define CLD_ENODEV (-19)
#define CLD_ENOMEM (-12)
#define CLD_EIO (-5)
#define CLD_EFAULT (-14)  /* a HIP runtime call failed (device error) */
#define CLD_ENOSPC (-28)  /* cld_detect_batch_vec: chunk_cap too small for the vectors */

/* summary_lang of a document the GPU could not score.  Such a document is
 * redone alone once; if it fails again the call returns CLD_EIO and every
 * other document's result is complete (lang3 = UNKNOWN, percent3 0,
 * text_bytes 0 for the failed one).  The kernels have no such case short of
 * a device fault: it exists so one bad document never costs a batch. */
#define CLD_LANG_FAILED 0xFFFF

/* cld_detect_batch flags: the service's text preparation, applied on the GPU
 * before detection (handlers.go:150-151).
 *   CLD_FLAG_STRIP_EXTRAS  StripExtras (handlers.go:198-210): keep the
 *                          strings.Fields words (unicode.IsSpace separators)
 *                          that start with neither "@" nor "http", each
 *                          followed by one ' '.
 *   CLD_FLAG_CSTRING       cut each document at its first NUL byte, as the
 *                          cgo hand-off does (main.go:77-81: C.CString, then
 *                          strlen in wrapper.cc:8).
 * STRIP_EXTRAS | CSTRING = exactly the text Detect_language() sees for one
 * request item of POST / (handlers.go:150-151). */
#define CLD_FLAG_STRIP_EXTRAS 1u
#define CLD_FLAG_CSTRING 2u
/* is_plain_text = false: the documents are HTML -- tags, comments, <script>
 * and <style> bodies are skipped and entities decoded by the span scanner
 * (getonescriptspan.cc:150-541, 592-1027), lang= attributes in the first 8 KB
 * become hints (compact_lang_det_impl.cc:1596-1611). */
#define CLD_FLAG_HTML 4u
/* The reference's checked entry points (DetectLanguageCheckUTF8,
 * compact_lang_det.h:168 / compact_lang_det.cc:44-56;
 * ExtDetectLanguageSummaryCheckUTF8, compact_lang_det.h:295 /
 * compact_lang_det.cc:317-355): each document first goes through
 * SpanInterchangeValid (compact_lang_det_impl.cc:72-80), and one that is not
 * interchange-valid UTF-8 from its first byte to its last is not scored.  It
 * gets the result those entries return before they score anything:
 * lang3 = {26, 26, 26} (UNKNOWN_LANGUAGE), summary_lang 26, percent3 0,
 * normalized3 0.0, text_bytes 0, is_reliable 0 -- and in vector mode an empty
 * chunk vector.  The unchecked entries are for input proven valid
 * (compact_lang_det.h:74): on ill-formed bytes the reference is undefined
 * (lead bytes C0, C1, F5-F7 index past its tables), and here such a document
 * takes the slowest path, the sequential span source.  Pass this flag for
 * input nobody has validated -- crawled pages, user text.
 * Interchange valid = well-formed UTF-8 (no overlong forms, no surrogates,
 * nothing above U+10FFFF) without the C0 controls other than TAB LF FF CR
 * (NUL is rejected), U+007F-U+009F, U+FDD0-U+FDEF and U+nFFFE / U+nFFFF.
 * With STRIP_EXTRAS / CSTRING the check applies to the prepared text, the
 * buffer CLD2 would be handed.  The flag belongs to the preparation flags:
 * a batch that carries it takes the streamed path (a GPU pass over the text
 * in front of the kernels), never the one-launch path of request-sized
 * batches nor the coalescer's tiny groups.  The check is a GPU kernel
 * (cld_valid.hip); documents longer than INT32_MAX bytes give CLD_EINVAL.
 * To have such documents repaired and scored instead of rejected, see
 * CLD_FLAG_SCRUB_UTF8 below. */
#define CLD_FLAG_CHECK_UTF8 8u
/* Repair instead of reject, what compact_lang_det.h:73-79 and :161-173 tell a
 * caller of the checked entries to do with the bytes they refuse: every
 * document is scored as the unchecked entry scores scrub(document), where
 *   scrub(doc) = doc with each byte at an error position of the check
 *                replaced by 0x20
 * -- the result of the usual loop "call DetectLanguageCheckUTF8, overwrite the
 * byte at valid_prefix_bytes with a space, call again" run to its end, in one
 * GPU pass (an error position's verdict depends on bytes p-3 .. p+3 with bytes
 * outside the document read as 0, and overwriting one with a space changes no
 * other position's verdict).  The length does not change, so chunk offsets and
 * valid prefixes still index the document as given; NUL is an error position
 * and becomes a space; the caller's buffer is never written.  scrub(doc) is
 * interchange-valid, so every document is scored where the reference is
 * defined and on the parallel kernels.  Accepted wherever
 * CLD_FLAG_CHECK_UTF8 is, as a preparation flag like it (the streamed path; per
 * batch, never in a doc_flags word: CLD_EINVAL), applied after STRIP_EXTRAS /
 * CSTRING and before an HTML page is rewritten or scanned for lang=.
 * CLD_FLAG_SCRUB_UTF8 | CLD_FLAG_CHECK_UTF8 in one call is CLD_EINVAL (so is
 * the flag in cld_detect_batch_checked), and so is a document longer than
 * INT32_MAX bytes.  Where an entry takes a valid_prefix array with the check it
 * takes it with this flag: it receives SpanInterchangeValid of the document as
 * given, which equals its length iff nothing was replaced.
 * Caution, the reference's own (compact_lang_det.h:76-79): the scrubbed text
 * is what the detector scores, nothing more.  Text that is passed on to other
 * software should go through a converter that turns ill-formed sequences into
 * U+FFFD instead -- deleting bytes or turning them into spaces can create
 * security holes there. */
#define CLD_FLAG_SCRUB_UTF8 0x20u
/* The reference's public result-affecting flags, with the reference's values
 * (compact_lang_det.h:343-349), accepted in the `flags` word of every batch
 * entry point and applied to every document of the batch:
 *   CLD_FLAG_SCORE_AS_QUADS  kCLDFlagScoreAsQuads: scripts normally scored by
 *                            their script alone (RTypeOne/None: Greek, Thai,
 *                            ...) are quadgram-scored instead
 *                            (scoreonescriptspan.cc:1318-1320)
 *   CLD_FLAG_BEST_EFFORT     kCLDFlagBestEffort: no unreliable-language removal
 *                            and no UNKNOWN summary for a small top percent
 *                            (compact_lang_det_impl.cc:1998-2000, :1493)
 * The reference's debug-output flags (kCLDFlagHtml, Cr, Verbose, Quiet, Echo:
 * CLD_FLAG_DEBUG_MASK) only write diagnostics to stderr there; they are
 * accepted and ignored. */
#define CLD_FLAG_SCORE_AS_QUADS 0x0100u
#define CLD_FLAG_BEST_EFFORT 0x4000u
#define CLD_FLAG_DEBUG_MASK 0x3E00u

/* ResultChunk (compact_lang_det.h:147-153): one piece of a document in one
 * language; offset/bytes index the document as given; lang1 is a Language
 * enum, UNKNOWN_LANGUAGE (26) for unreliable or too-short pieces. */
typedef struct cld_chunk {
  int32_t offset;
  int32_t bytes;
  uint16_t lang1;
  uint16_t pad;
} cld_chunk;

/* CLDHints (compact_lang_det.h:134-139): per-document priors. */
typedef struct cld_hints {
  const char* content_language_hint;  /* "mi,en" boosts Maori and English; NULL / "" for none */
  const char* tld_hint;               /* "id" boosts Indonesian; NULL / "" for none */
  int32_t encoding_hint;              /* Encoding enum (encodings.h); CLD_UNKNOWN_ENCODING for none */
  int32_t language_hint;              /* Language enum; 26 (UNKNOWN_LANGUAGE) for none */
} cld_hints;
#define CLD_UNKNOWN_ENCODING 23

/* wrapper.h:8 -- returns a static ISO code; never NULL; UNKNOWN -> "en"
 * (compact_lang_det.cc:91-93).  Input is NUL-terminated, length = strlen
 * (wrapper.cc:8).  Thread-safe; concurrent callers are coalesced into GPU
 * micro-batches by the runtime. */
const char* detect_language(const char* text);

/* DetectLanguageCheckUTF8 (compact_lang_det.h:168, compact_lang_det.cc:44-56)
 * with is_plain_text = true: *valid_prefix_bytes (NULL: not wanted) receives
 * the number of leading interchange-valid bytes of text; if that is less than
 * strlen(text) the text is not scored and the code of UNKNOWN_LANGUAGE ("un";
 * not mapped to "en", as there) is returned -- the check runs on the host
 * (cld_valid_prefix_host) and a rejected text never reaches the GPU.
 * Otherwise detect_language(text). */
const char* detect_language_checked(const char* text, int* valid_prefix_bytes);

/* detect_language(scrub(text)) (CLD_FLAG_SCRUB_UTF8): the scrub runs on the
 * host over a private copy (cld_scrub_utf8_host; text is not written), so an
 * ill-formed text gets a language instead of "un".  *replaced_bytes (NULL: not
 * wanted) receives the number of bytes replaced by a space, 0 for an
 * interchange-valid text. */
const char* detect_language_scrubbed(const char* text, int* replaced_bytes);

/* Optional explicit initialisation.  tables_path NULL -> $CLD_MI355X_TABLES or
 * the blob shipped next to the library.  n_devices <= 0 -> all visible GPUs.
 * Returns CLD_OK or a negative error.  Called implicitly by the entry points. */
int cld_init(const char* tables_path, int n_devices);
void cld_shutdown(void);

/* Initialise on exactly one GPU (HIP ordinal `device`); context index 0.
 * One process per GPU (torch.distributed / bench.py) uses this. */
int cld_init_device(const char* tables_path, int device);

/* Cost-balanced document shards: cuts[0..nshards] (cuts[0]=0, cuts[nshards]=n)
 * such that shard k = documents [cuts[k], cuts[k+1]), each holding about
 * 1/nshards of the estimated kernel cost (a document of <= 256 bytes: 480
 * units, a longer one: 41/8 units per byte + 2500; measured per-document
 * kernel times in units of 10 ps).  Host-only helper used by
 * cld_detect_batch's multi-GPU split and by multi-process callers. */
int cld_plan_shards(const uint64_t* offsets, size_t n, int nshards, size_t* cuts);

/* Sum of kernel durations (HIP events on the stream the kernels ran on) of
 * every batch enqueued on context `ctx` since the previous call; resets.
 * short_ms = wavefront kernel; general_ms = the long-document kernels (k_long, both instantiations). */
int cld_kernel_time(int ctx, double* short_ms, double* general_ms, int* launches);

/* Same accounting split per kernel stage: ms[0] the wavefront kernel (k_wave),
 * (with HTML pages: the GPU rewrite of the pages into plain text, k_html_rewrite,
 * is counted in ms[0]), ms[1] the long-document stage (length ordering + k_long on the
 * parallel span builder), ms[2] k_long's documents on the sequential span source (its SEQ
 * instantiation, cld_seq.hip).  Sums since the previous call of either
 * function; resets. */
int cld_kernel_times(int ctx, double* ms3, int* launches);

/* Diagnostics: per-stage shader-clock cycle sums on context `ctx` since the
 * previous call; 16 entries.  [0..7] short-document wavefront kernel (0 load,
 * 1 span, 2 lower, 3 quad/uni, 4 octa/bi, 5 score, 6 document level);
 * [8..15] long-document kernel (8 classify, 9 span+lowercase, 10 squeeze
 * test, 11 repeats, 12 word lists + quad chain, 13 quad hits, 14 octa/uni/bi
 * hits, 15 linearize/chunk/score).  All zero unless the runtime was started
 * with CLD_PROFILE_STAGES=1.  Resets. */
int cld_stage_cycles(int ctx, uint64_t* cycles16);

/* Batch detection.  Documents are [buf + offsets[i], buf + offsets[i+1]),
 * i < n (offsets has n+1 entries, non-decreasing).  Each document is scored
 * as if followed by NUL bytes, i.e. exactly like detect_language() on a
 * NUL-terminated copy of it (embedded NULs are kept, as with
 * CLD2::DetectLanguage(buffer, length, ...)).  `out` is caller-allocated
 * (n entries).  Host buffers; not retained after return.  Blocks until the
 * results are in `out`.  Documents are sharded across the initialised GPUs
 * by estimated cost; each shard streams through the GPU in chunks of <= 64 MB /
 * 512K documents (pinned staging, upload / kernels / download overlapped on
 * three streams).  A batch whose mean document is longer than 256 bytes goes
 * in chunks of <= 256 MB / 2M documents instead: each of a context's two chunk
 * slots then holds up to 256 MB of text plus 48 B per document in device
 * memory, and as much pinned host staging unless the caller's buffers are
 * pinned (CLD_CHUNK_MB scales both).  Request-sized calls (< 16 MB of text)
 * from concurrent callers are coalesced into one GPU batch; a batch of at
 * most 1024 documents of <= 256 bytes takes one upload, one kernel and one
 * download.  flags: 0 or CLD_FLAG_STRIP_EXTRAS / CLD_FLAG_CSTRING /
 * CLD_FLAG_CHECK_UTF8 or CLD_FLAG_SCRUB_UTF8, and CLD_FLAG_SCORE_AS_QUADS /
 * CLD_FLAG_BEST_EFFORT (above).  Thread-safe. */
int cld_detect_batch(const uint8_t* buf, const uint64_t* offsets, size_t n,
                     cld_result* out, uint32_t flags);

/* ExtDetectLanguageSummary (compact_lang_det.h:324-335 / impl.cc:1707) over a
 * batch: `hints` is NULL or one cld_hints per document (CLDHints); flags is
 * the reference's `flags` argument -- CLD_FLAG_SCORE_AS_QUADS,
 * CLD_FLAG_BEST_EFFORT, the ignored debug flags -- plus CLD_FLAG_HTML for
 * is_plain_text = false (all documents are HTML) and CLD_FLAG_CHECK_UTF8 or
 * CLD_FLAG_SCRUB_UTF8.
 * Results are the same fields as cld_detect_batch.  Host buffers; blocks. */
int cld_detect_batch_ex(const uint8_t* buf, const uint64_t* offsets, size_t n, const cld_hints* hints,
                        uint32_t flags, cld_result* out);

/* ExtDetectLanguageSummaryCheckUTF8 (compact_lang_det.h:295,
 * compact_lang_det.cc:317-355) over a batch: cld_detect_batch_ex with
 * CLD_FLAG_CHECK_UTF8 forced on, plus valid_prefix[i] (n entries) =
 * SpanInterchangeValid of document i, its number of leading interchange-valid
 * bytes -- the document was scored iff that equals its length; else out[i] is
 * the "rejected" result (CLD_FLAG_CHECK_UTF8 above).  One upload serves the
 * check and the scoring.  flags: CLD_FLAG_HTML and the public CLD2 flags;
 * CLD_FLAG_STRIP_EXTRAS / CLD_FLAG_CSTRING give CLD_EINVAL, because the
 * prefixes index the documents as given, and so does CLD_FLAG_SCRUB_UTF8 (this
 * entry rejects, that flag repairs; for the prefixes of a scrubbed batch see
 * cld_detect_batch_docflags).  A document longer than INT32_MAX
 * bytes gives CLD_EINVAL; n == 0 CLD_OK; CLD_EIO as for cld_detect_batch. */
int cld_detect_batch_checked(const uint8_t* buf, const uint64_t* offsets, size_t n, const cld_hints* hints,
                             uint32_t flags, cld_result* out, int32_t* valid_prefix);

/* SpanInterchangeValid (compact_lang_det_impl.cc:72-80) alone.
 *   cld_valid_prefix_host    one document on the host, no GPU: its number of
 *                            leading interchange-valid bytes (CLD_EINVAL if
 *                            len > INT32_MAX).  A truncated character at the
 *                            end counts from its lead byte.
 *   cld_valid_prefix_batch   host buffers, on GPU 0 (like cld_prepare_batch),
 *                            in pieces of <= 256 MB; blocks until
 *                            valid_prefix[0..n) is on the host.
 *   cld_valid_prefix_device  every pointer in device memory of GPU `device`,
 *                            enqueued on `stream` (NULL: the runtime's);
 *                            asynchronous, uses none of the context's scratch.
 *                            The caller keeps documents <= INT32_MAX bytes.
 * Documents of <= 256 bytes take one wavefront each; longer ones are checked
 * in 1 KB tiles, one wavefront per tile, 16 bytes per lane, whatever their
 * length.  n == 0: CLD_OK. */
int32_t cld_valid_prefix_host(const uint8_t* doc, size_t len);
int cld_valid_prefix_batch(const uint8_t* buf, const uint64_t* offsets, size_t n, int32_t* valid_prefix);
int cld_valid_prefix_device(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n,
                            int32_t* d_valid_prefix, void* stream);

/* scrub() of CLD_FLAG_SCRUB_UTF8 alone, modelled on the three above.
 *   cld_scrub_utf8_host    one document on the host, no GPU: out[0..len)
 *                          receives scrub(doc); out may equal doc.  Returns
 *                          the number of replaced bytes (CLD_EINVAL if
 *                          len > INT32_MAX or a pointer is NULL with len > 0).
 *   cld_scrub_utf8_batch   host buffers, on GPU 0, in pieces of <= 256 MB;
 *                          out_buf holds offsets[n] - offsets[0] bytes indexed
 *                          like the input from its first document on (byte j
 *                          of document i at out_buf[offsets[i] - offsets[0] +
 *                          j]); replaced[0..n) (NULL: not wanted) the number
 *                          of replaced bytes per document.  Blocks.
 *   cld_scrub_utf8_device  every pointer in device memory of GPU `device`,
 *                          enqueued on `stream` (NULL: the runtime's);
 *                          asynchronous, uses none of the context's scratch.
 *                          d_out is indexed by d_offsets like d_buf (bytes
 *                          outside [d_offsets[0], d_offsets[n]) are not
 *                          written) and must not overlap it; d_replaced
 *                          (NULL: not wanted) as above.  Where d_out - d_buf
 *                          is a multiple of 16 each lane of a tile stores its
 *                          16 bytes at once, otherwise byte by byte.  The
 *                          caller keeps documents <= INT32_MAX bytes.
 * The input is never written.  The pass reads each byte once and writes each
 * byte once, in the two shapes of the check.  n == 0: CLD_OK.
 * The caution at CLD_FLAG_SCRUB_UTF8 holds here above all: the output is what
 * the detector scores; text that goes on to other software should be
 * converted to U+FFFD instead (compact_lang_det.h:76-79). */
int32_t cld_scrub_utf8_host(const uint8_t* doc, size_t len, uint8_t* out);
int cld_scrub_utf8_batch(const uint8_t* buf, const uint64_t* offsets, size_t n, uint8_t* out_buf, int32_t* replaced);
int cld_scrub_utf8_device(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n, uint8_t* d_out,
                          int32_t* d_replaced, void* stream);

/* A batch of results grouped by language, and the chosen documents packed into
 * a new batch: what a caller does with the results of a crawl shard, without
 * leaving the GPU (the reference service counts its answers per language,
 * handlers.go:163 incLanguageCount).
 *
 * The key of a document is summary_lang, or lang3[0] with CLD_GROUP_TOP1;
 * with CLD_GROUP_RELIABLE_ONLY a document with is_reliable == 0 gets the key
 * UNKNOWN_LANGUAGE (26).  Its bin is min(key, CLD_NUM_LANGUAGES): bin 614
 * collects every key that is no Language value, CLD_LANG_FAILED among them.
 * Any other bit in group_flags: CLD_EINVAL.
 *   counts[CLD_GROUP_BINS]             documents per bin
 *   bin_bytes[CLD_GROUP_BINS]          (NULL: not wanted; needs offsets, else
 *                                      CLD_EINVAL) the sum of offsets[i + 1] -
 *                                      offsets[i] over each bin's documents
 *   order[n]                           (NULL: not wanted) the document indices
 *                                      sorted by (bin, index): a stable sort
 *   group_offsets[CLD_GROUP_BINS + 1]  (NULL: not wanted) the exclusive prefix
 *                                      sum of counts, group_offsets[615] == n:
 *                                      bin b's documents are order[group_offsets[b]
 *                                      .. group_offsets[b + 1]), ascending
 *   cld_group_by_language         the host reference, no GPU.
 *   cld_group_by_language_device  every pointer in device memory of GPU
 *                                 `device` (8-byte aligned where it holds 64-bit
 *                                 words or results), enqueued on `stream` (NULL:
 *                                 the runtime's); asynchronous, waits for nothing
 *                                 on the host, uses none of the context's scratch
 *                                 and may run from several threads at once, each
 *                                 with a workspace of its own: d_work holds
 *                                 work_bytes >= cld_group_work_bytes(n) bytes
 *                                 (a smaller one: CLD_ENOSPC, nothing enqueued)
 *                                 and is free again when the call's work on the
 *                                 stream is done.  d_results is only read.
 *                                 order is the same
 *                                 from run to run: no atomic decides a position.
 *   cld_gather_docs_device        documents d_index[0..m) of the batch (d_buf,
 *                                 d_offsets[0..n_src]) packed back to back:
 *                                 d_out_offsets[0..m] = the exclusive prefix sum
 *                                 of their lengths, always the true totals, and
 *                                 d_out_buf[0, min(d_out_offsets[m], out_cap))
 *                                 their bytes; nothing at or past d_out_buf +
 *                                 out_cap is written (out_cap == 0, d_out_buf
 *                                 NULL: the sizing pass).  An index may repeat;
 *                                 an index >= n_src is an empty document.  The
 *                                 output is a batch for every cld_detect_batch_device*
 *                                 entry, with buf_bytes = d_out_offsets[m].
 *                                 d_out_buf and d_buf must not overlap.  The
 *                                 usual d_index is a slice of d_order: d_order +
 *                                 group_offsets[L], m = counts[L], and bin_bytes[L]
 *                                 sizes d_out_buf exactly.  Workspace and stream
 *                                 as above, cld_group_work_bytes(m).
 * cld_group_work_bytes does not grow past a few MB: both entries cut their
 * work into a fixed number of workgroup ranges.  n or m (or n_src) above
 * INT32_MAX: CLD_EINVAL.  n == 0 / m == 0: CLD_OK, with zero counts, byte
 * totals and group offsets, and d_out_offsets[0] = 0, written where those
 * pointers are not NULL. */
#define CLD_NUM_LANGUAGES 614u      /* Language enum values 0..613 (generated_language.h) */
#define CLD_GROUP_BINS    615u      /* bin 614: every key >= 614, CLD_LANG_FAILED (0xFFFF) among them */
#define CLD_GROUP_TOP1          1u  /* key = lang3[0]; default: summary_lang */
#define CLD_GROUP_RELIABLE_ONLY 2u  /* is_reliable == 0  ->  key UNKNOWN_LANGUAGE (26) */
size_t cld_group_work_bytes(size_t n);
int cld_group_by_language(const cld_result* results, size_t n, uint32_t group_flags, const uint64_t* offsets,
                          uint64_t* counts, uint64_t* bin_bytes, uint32_t* order, uint64_t* group_offsets);
int cld_group_by_language_device(int device, const cld_result* d_results, size_t n, uint32_t group_flags,
                                 const uint64_t* d_offsets, uint64_t* d_counts, uint64_t* d_bin_bytes,
                                 uint32_t* d_order, uint64_t* d_group_offsets, void* d_work, size_t work_bytes,
                                 void* stream);
int cld_gather_docs_device(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n_src,
                           const uint32_t* d_index, size_t m, uint8_t* d_out_buf, uint64_t out_cap,
                           uint64_t* d_out_offsets, void* d_work, size_t work_bytes, void* stream);

/* ExtDetectLanguageSummary with a ResultChunkVector per document
 * (compact_lang_det.h:324-335): the same results as cld_detect_batch_ex plus
 * each document's chunk vector -- pieces of the document as given, in one
 * language each (SummaryBufferToVector / SharpenBoundaries / OffsetMap,
 * scoreonescriptspan.cc:389-548, 671-845; offsetmap.cc).  Vector mode changes
 * scoring the way the reference's does (SharpenBoundaries moves chunk bytes,
 * Squeeze/RepWords overwrite instead of cutting), so `out` can differ from
 * cld_detect_batch_ex's for the same document, exactly as there.
 * chunk_offsets[n+1] receives document i's chunks as
 * chunks[chunk_offsets[i] .. chunk_offsets[i+1]).  If chunk_cap is too small
 * the call returns CLD_ENOSPC with out and chunk_offsets complete and chunks
 * holding the first chunk_cap entries (CLD_ENOMEM: device memory ran out).  A document whose vector outgrows its
 * working region is redone alone with 8x the room; should that fail too, it
 * gets an empty vector and the call returns CLD_EIO with every other
 * document's result and vector complete.  Every document runs the sequential
 * kernel (not a high-throughput path, as in the reference).
 * CLD_FLAG_CHECK_UTF8: a rejected document gets an empty vector.
 * CLD_FLAG_SCRUB_UTF8: the vector is that of scrub(document), whose offsets
 * are the document's own. */
int cld_detect_batch_vec(const uint8_t* buf, const uint64_t* offsets, size_t n, const cld_hints* hints,
                         uint32_t flags, cld_result* out, cld_chunk* chunks, size_t chunk_cap,
                         uint64_t* chunk_offsets);

/* Host-only (no GPU): the ApplyHints result for one document.  priors: the
 * CLDLangPriors (OneCLDLangPrior = (weight << 10) + Language, at most 14)
 * after TrimCLDLangPriors(4); boosts16: prior boosts latn[4], othr[4] and
 * close-language whacks latn[4], othr[4] as langprobs.  Returns the prior
 * count, or a negative error.  doc may be NULL unless is_plain_text = 0. */
int cld_hint_priors(const uint8_t* doc, size_t len, int is_plain_text, const cld_hints* hints,
                    int16_t* priors14, uint32_t* boosts16);

/* Same, with every pointer in device memory of GPU `device` and work
 * enqueued on `stream` (a hipStream_t, NULL = the runtime's stream for that
 * device).  Asynchronous: returns once the kernels are enqueued.  Used by the
 * benchmark to time the path with inputs already resident in HBM. */
int cld_detect_batch_device(int device, const uint8_t* d_buf, const uint64_t* d_offsets,
                            size_t n, cld_result* d_out, void* stream);

/* cld_detect_batch_device with flags (preparation flags, CLD_FLAG_CHECK_UTF8
 * or CLD_FLAG_SCRUB_UTF8 among them, and CLD2 flags, as for cld_detect_batch).  buf_bytes bounds
 * d_offsets[n] (the prepared copy is staged in a device buffer of
 * buf_bytes + n bytes).  Asynchronous like cld_detect_batch_device. */
int cld_detect_batch_device_ex(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n,
                               uint64_t buf_bytes, cld_result* d_out, uint32_t flags, void* stream);

/* CLDHints (compact_lang_det.h:134-139) for callers whose hints live in device
 * memory: no pointers. */
typedef struct cld_hints_dev {
  uint32_t content_language_off;  /* into the hint text buffer                              */
  uint32_t content_language_len;  /* 0: none; read up to its first NUL, as strlen would;    */
                                  /* a range past hint_text_bytes is clipped to the buffer  */
  char     tld[4];                /* NUL-padded; tld[0] == 0: none; tld[3] != 0: ignored,   */
                                  /* as the reference ignores a TLD longer than 3           */
                                  /* (SetCLDTLDHint, compact_lang_det_hint_code.cc:1446)    */
  int32_t  encoding_hint;         /* CLD_UNKNOWN_ENCODING for none                          */
  int32_t  language_hint;         /* 26 for none                                            */
} cld_hints_dev;                  /* 20 bytes */

/* ApplyHints alone (compact_lang_det_impl.cc:1587-1684; cld_hint_priors for a
 * batch in device memory, a GPU kernel: cld_hints.hip).  Every pointer in
 * device memory of GPU `device`; asynchronous on `stream` (NULL: the
 * runtime's); uses none of the context's scratch.  d_hints NULL: no hints.
 * is_plain_text 0: the lang= scan of each document's first 8 KB.
 * d_priors14 (14 per document, after TrimCLDLangPriors(4), zero-padded) and
 * d_boosts16 (16 per document, as cld_hint_priors' boosts16): either may be
 * NULL.  Bit-identical to cld_hint_priors on the same bytes and hints.
 * CLD_EINVAL for tables without the hint sections; n == 0: CLD_OK. */
int cld_hint_boosts_device(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n,
                           const cld_hints_dev* d_hints, const uint8_t* d_hint_text,
                           uint64_t hint_text_bytes, int is_plain_text,
                           int16_t* d_priors14, uint32_t* d_boosts16, void* stream);

/* cld_detect_batch_ex (ExtDetectLanguageSummary, compact_lang_det.h:324-335)
 * for device-resident input: d_hints is NULL or one cld_hints_dev per
 * document; flags = CLD_FLAG_HTML and the public CLD2 flags (debug flags
 * ignored).  Preparation flags, CLD_FLAG_CHECK_UTF8 and CLD_FLAG_SCRUB_UTF8
 * included, give CLD_EINVAL.  buf_bytes bounds d_offsets[n], as in
 * cld_detect_batch_device_ex.  ApplyHints runs on the GPU in front of the
 * scoring kernels; without hints and without CLD_FLAG_HTML the call is
 * cld_detect_batch_device.  Asynchronous. */
int cld_detect_batch_device_hints(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n,
                                  uint64_t buf_bytes, const cld_hints_dev* d_hints,
                                  const uint8_t* d_hint_text, uint64_t hint_text_bytes,
                                  cld_result* d_out, uint32_t flags, void* stream);

/* cld_detect_batch_vec for device-resident input: every pointer is device
 * memory of GPU `device`, the call is asynchronous on `stream` (NULL: the
 * runtime's), nothing inside it waits for the GPU, and it returns once its
 * kernels are enqueued.  d_out, d_chunk_offsets[0..n] and d_chunks are what
 * cld_detect_batch_vec gives for the same documents, hints and flags.
 *   flags        CLD_FLAG_HTML, the public CLD2 flags (debug flags ignored)
 *                and CLD_FLAG_CHECK_UTF8 or CLD_FLAG_SCRUB_UTF8 (both:
 *                CLD_EINVAL); CLD_FLAG_STRIP_EXTRAS /
 *                CLD_FLAG_CSTRING and unknown bits give CLD_EINVAL (chunk
 *                offsets and prefixes index the documents as given).
 *   d_hints      NULL or one cld_hints_dev per document (their texts in
 *                d_hint_text); ApplyHints runs on the GPU, as in
 *                cld_detect_batch_device_hints.
 *   CHECK_UTF8   a rejected document gets the "rejected" result and an empty
 *                vector; d_valid_prefix (NULL: not wanted; n entries)
 *                receives SpanInterchangeValid per document, as
 *                cld_detect_batch_checked gives it.  d_valid_prefix without
 *                the flag is CLD_EINVAL.  The caller keeps documents
 *                <= INT32_MAX bytes.
 *   SCRUB_UTF8   every document is scored as scrub(document), hints' lang=
 *                scan included; d_valid_prefix as with CHECK_UTF8 (of the
 *                document as given: its length iff nothing was replaced), and
 *                d_status->rejected_docs counts the repaired documents.
 *   capacity     d_chunk_offsets always holds the true totals, d_chunks
 *                receives the first chunk_cap chunks and nothing is written
 *                past d_chunks + chunk_cap.  chunk_cap 0 with d_chunks NULL is
 *                the sizing pass: read d_status->total_chunks, allocate, call
 *                again.
 *   buf_bytes    bounds d_offsets[n], as in cld_detect_batch_device_ex: it
 *                sizes the working memory on the host (which never reads the
 *                offsets).  CLD_ENOMEM, synchronously, if that does not fit.
 *   big_regions  0: a document of len bytes builds its vector in a region of
 *                len + len/4 + 8 chunks; else 8 len + 256, the two sizes
 *                cld_detect_batch_vec uses.  That entry redoes a document
 *                whose vector outgrows its region; here the host is not
 *                asked, so such a document gets an empty vector, summary_lang
 *                CLD_LANG_FAILED (lang3 UNKNOWN, zeros otherwise) and a count
 *                in d_status->failed_docs, and every other document is
 *                complete.  Redo those with big_regions = 1 or through
 *                cld_detect_batch_vec.
 * n == 0: CLD_OK, with d_chunk_offsets[0] = 0 and a zero status written where
 * the pointers are not NULL.  n > 0x7FFFFFFF and tables without the HTML or
 * hint sections (when asked for): CLD_EINVAL.  Calls enqueued back to back
 * run one after another on the context's working memory.
 * cld_last_batch_stats is not updated by this entry: nothing is read back. */
typedef struct cld_vec_status {   /* 16 bytes, written by the last kernel of the call */
  uint64_t total_chunks;          /* = d_chunk_offsets[n]; > chunk_cap means the CLD_ENOSPC case */
  uint32_t failed_docs;           /* documents whose vector outgrew its pool region (above)    */
  uint32_t rejected_docs;         /* CLD_FLAG_CHECK_UTF8 / SCRUB_UTF8: documents not           */
                                  /* interchange-valid (rejected, or repaired and scored)      */
} cld_vec_status;

int cld_detect_batch_device_vec(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n,
                                uint64_t buf_bytes, const cld_hints_dev* d_hints,
                                const uint8_t* d_hint_text, uint64_t hint_text_bytes, uint32_t flags,
                                int big_regions, cld_result* d_out, cld_chunk* d_chunks,
                                uint64_t chunk_cap, uint64_t* d_chunk_offsets,
                                int32_t* d_valid_prefix, cld_vec_status* d_status, void* stream);

/* ---- Per-document is_plain_text and CLD2 flags within one batch.
 * ExtDetectLanguageSummary takes is_plain_text and flags per call
 * (compact_lang_det.h:324-335); the entries above take one value of each for
 * the whole batch.  The four _docflags entries take one more array,
 * doc_flags[n], one word per document, so that a batch of n documents stays n
 * independent calls of the reference -- a crawl shard of text/html and
 * text/plain records, some of them wanting best-effort answers, is one batch.
 * Document i is scored as the reference scores it with
 *   is_plain_text = !((flags | doc_flags[i]) & CLD_FLAG_HTML)
 *   flags         = (flags | doc_flags[i]) & (CLD_FLAG_SCORE_AS_QUADS | CLD_FLAG_BEST_EFFORT)
 * (kCLDFlagScoreAsQuads, scoreonescriptspan.cc:1318-1320; kCLDFlagBestEffort,
 * compact_lang_det_impl.cc:1998-2000, :1493; the lang= scan of the first 8 KB,
 * impl.cc:1596-1611, runs for the documents that are HTML and only for them).
 * A bit set in `flags` holds for every document; a word can add bits, never
 * take one away.  The debug-output bits (CLD_FLAG_DEBUG_MASK) are accepted
 * and ignored in the words as in `flags`.  `flags` keeps the meaning it has
 * in the entry each one extends, CLD_FLAG_CHECK_UTF8 included; hints stay per
 * document.  The preparation flags and the UTF-8 check are per batch only.
 * doc_flags == NULL: exactly the entry it extends (the call is forwarded).
 *
 * Host entries: a word with any bit outside CLD_FLAG_HTML |
 * CLD_FLAG_SCORE_AS_QUADS | CLD_FLAG_BEST_EFFORT | CLD_FLAG_DEBUG_MASK
 * (CLD_FLAG_STRIP_EXTRAS, CLD_FLAG_CSTRING, CLD_FLAG_CHECK_UTF8,
 * CLD_FLAG_SCRUB_UTF8, unknown bits)
 * gives CLD_EINVAL, before any GPU work.  Words that are all zero cost
 * nothing: the call is then cld_detect_batch_ex's.  Otherwise the batch
 * carries one routing byte per document to the GPU (as a hinted batch does),
 * and when some document is HTML the HTML working memory of
 * cld_detect_batch_ex: per chunk two bytes per text byte, ten where a chunk
 * holds 40928 bytes or more.
 *
 *   cld_detect_batch_docflags      cld_detect_batch_ex; with CLD_FLAG_CHECK_UTF8
 *                                  in flags also cld_detect_batch_checked:
 *                                  valid_prefix (NULL: not wanted; n entries)
 *                                  receives SpanInterchangeValid per document.
 *                                  With CLD_FLAG_SCRUB_UTF8 it receives the
 *                                  same (of the documents as given) and every
 *                                  document is scored.
 *                                  valid_prefix without the flag: CLD_EINVAL.
 *   cld_detect_batch_vec_docflags  cld_detect_batch_vec, with its errors
 *                                  (chunk_offsets NULL, chunk_cap > 0 without
 *                                  chunks: CLD_EINVAL; CLD_ENOSPC; CLD_EIO). */
int cld_detect_batch_docflags(const uint8_t* buf, const uint64_t* offsets, size_t n, const cld_hints* hints,
                              const uint32_t* doc_flags, uint32_t flags, cld_result* out, int32_t* valid_prefix);
int cld_detect_batch_vec_docflags(const uint8_t* buf, const uint64_t* offsets, size_t n, const cld_hints* hints,
                                  const uint32_t* doc_flags, uint32_t flags, cld_result* out, cld_chunk* chunks,
                                  size_t chunk_cap, uint64_t* chunk_offsets);

/* The same for device-resident input: cld_detect_batch_device_hints and
 * cld_detect_batch_device_vec with d_doc_flags[n] in device memory of GPU
 * `device`; every other argument, the asynchrony and the errors are theirs
 * (flags: CLD_FLAG_HTML and the public CLD2 flags; the vector entry also
 * CLD_FLAG_CHECK_UTF8 or CLD_FLAG_SCRUB_UTF8).  d_doc_flags == NULL forwards to them.
 * The host never reads the words, so it cannot reject one: the ApplyHints
 * kernel (cld_hints.hip) masks each word to CLD_FLAG_HTML |
 * CLD_FLAG_SCORE_AS_QUADS | CLD_FLAG_BEST_EFFORT and ignores every other bit,
 * stray high bits included.  For the same reason the host cannot know whether
 * any document is HTML, so with d_doc_flags the call is set up as an HTML
 * batch is: the tables must hold the HTML and hint sections (CLD_EINVAL
 * otherwise), ApplyHints always runs, the 16 langprobs per document always go
 * along (64 n bytes, plus n routing bytes), and the HTML working memory is
 * sized from buf_bytes -- 2 buf_bytes, and 8 buf_bytes more in the vector
 * entry or where buf_bytes >= 40928 (each rewritten byte's page offset).
 * CLD_ENOMEM, synchronously, if that does not fit. */
int cld_detect_batch_device_docflags(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n,
                                     uint64_t buf_bytes, const cld_hints_dev* d_hints, const uint8_t* d_hint_text,
                                     uint64_t hint_text_bytes, const uint32_t* d_doc_flags, cld_result* d_out,
                                     uint32_t flags, void* stream);
int cld_detect_batch_device_vec_docflags(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n,
                                         uint64_t buf_bytes, const cld_hints_dev* d_hints, const uint8_t* d_hint_text,
                                         uint64_t hint_text_bytes, const uint32_t* d_doc_flags, uint32_t flags,
                                         int big_regions, cld_result* d_out, cld_chunk* d_chunks, uint64_t chunk_cap,
                                         uint64_t* d_chunk_offsets, int32_t* d_valid_prefix, cld_vec_status* d_status,
                                         void* stream);

/* A batch split by the language of its chunks: per-language totals over the
 * chunk vectors of a batch, and the pieces in chosen languages packed into a
 * new batch -- "which part of the text is in which language"
 * (compact_lang_det.h:147-153) acted on without leaving the GPU.
 *
 * The batch is buf, offsets[0..n]; its vectors are chunks, chunk_offsets[0..n]
 * as cld_detect_batch_vec / cld_detect_batch_device_vec write them, and
 * chunk_cap is the number of entries chunks really holds.
 *   document i   has len = offsets[i + 1] - offsets[i] bytes, 0 if that is
 *                negative, and the vector chunks[chunk_offsets[i] ..
 *                min(chunk_offsets[i + 1], chunk_cap)), empty if that range is
 *                empty or inverted.  Chunks at or past chunk_cap do not exist
 *                (the CLD_ENOSPC case of the vector entries: the offsets hold the
 *                true totals, memory the first chunk_cap chunks).
 *   the piece    of a chunk is the byte range [s, e) of its document, s =
 *                clamp(offset, 0, len), e = clamp((int64)offset + bytes, s, len).
 *                Negative bytes, offsets outside the document, overlapping and
 *                repeated chunks are legal input: no chunk word makes an entry
 *                read a byte outside [offsets[i], offsets[i + 1]) or write
 *                outside its output.
 *   the bin      of a chunk is min(lang1, CLD_NUM_LANGUAGES), the CLD_GROUP_BINS
 *                bins of the group entries.
 * cld_chunk_totals (the host reference, no GPU) / cld_chunk_totals_device:
 *   chunk_counts[CLD_GROUP_BINS]  (NULL: not wanted) the chunks per bin; every
 *                                 existing chunk counts, an empty piece too
 *   chunk_bytes[CLD_GROUP_BINS]   (NULL: not wanted) the sum of e - s per bin
 * cld_gather_chunks (the host reference, no GPU) / cld_gather_chunks_device:
 *   select[CLD_GROUP_BINS]        one byte per bin, nonzero: keep
 *   output document i is the concatenation, in vector order, of the pieces of
 *   document i whose bin is selected and which are not empty (the kept pieces);
 *   the output batch has n documents, many of them possibly empty.  With
 *   CLD_CHUNKS_SPACE a kept piece is preceded by one 0x20 unless its chunk is
 *   the first of its document's vector, or the chunk before it in the vector
 *   is itself a kept piece that ends exactly where this one starts: words are
 *   not glued across a removed stretch, and a leading space is harmless to the
 *   detector.  Any other flag bit: CLD_EINVAL.  With flags == 0 and one
 *   selected bin L the output holds chunk_bytes[L] bytes: the totals size
 *   out_buf exactly.
 *   out_offsets[0..n] is always the exclusive prefix sum of the true output
 *   lengths; out_buf[0, min(out_offsets[n], out_cap)) receives the bytes and
 *   nothing at or past out_buf + out_cap is written (out_cap == 0 with out_buf
 *   NULL: the sizing pass).  The output must not overlap buf.  It is a batch
 *   for every cld_detect_batch_device* entry, buf_bytes = out_offsets[n].
 * The device entries: every pointer in device memory of GPU `device` (8-byte
 * aligned where it holds 64-bit words, 4-byte aligned chunks), enqueued on
 * `stream` (NULL: the runtime's); asynchronous, the host waits for nothing and
 * reads no device word; none of the context's scratch is used.  d_work holds
 * work_bytes >= cld_chunk_work_bytes(n, chunk_cap) bytes (a smaller one:
 * CLD_ENOSPC, nothing enqueued) and is free again when the call's work on the
 * stream is done.  cld_chunk_work_bytes is 8 * (chunk_cap + 1) bytes -- the
 * output position of every chunk's piece -- plus a fixed 2.4 MB (the totals'
 * per-range counts and bytes over the bins; the scans' per-range sums); n does
 * not enter.  The output is the same from run to run: no atomic decides a
 * position or a byte.  Inputs are only read.
 * chunk_offsets may be anything; vectors of two documents overlap only where
 * it goes down and up again.  cld_gather_chunks_device holds one position per
 * chunk, so where overlapping vectors hold more than chunk_cap (or
 * CLD_CHUNKS_MAX) chunks together it takes the first chunk_cap of them in
 * document order and the rest do not exist; the other three entries take them
 * all.
 * CLD_EINVAL: n > INT32_MAX, chunk_cap > UINT32_MAX, NULL chunk_offsets, NULL
 * select, out_cap > 0 with NULL out_buf, and with n > 0 a NULL offsets,
 * out_offsets or workspace, NULL chunks with chunk_cap > 0, or NULL buf with
 * out_cap > 0.  n == 0: CLD_OK, with zero totals and out_offsets[0] = 0 written
 * where those pointers are not NULL. */
#define CLD_CHUNKS_SPACE 1u             /* one 0x20 before a kept piece that does not continue the one before it */
#define CLD_CHUNKS_MAX 0xFFF00000ull    /* chunks one cld_gather_chunks_device call can place */
size_t cld_chunk_work_bytes(size_t n, uint64_t chunk_cap);
int cld_chunk_totals(const uint64_t* offsets, size_t n, const cld_chunk* chunks, uint64_t chunk_cap,
                     const uint64_t* chunk_offsets, uint64_t* chunk_counts, uint64_t* chunk_bytes);
int cld_chunk_totals_device(int device, const uint64_t* d_offsets, size_t n, const cld_chunk* d_chunks,
                            uint64_t chunk_cap, const uint64_t* d_chunk_offsets, uint64_t* d_chunk_counts,
                            uint64_t* d_chunk_bytes, void* d_work, size_t work_bytes, void* stream);
int cld_gather_chunks(const uint8_t* buf, const uint64_t* offsets, size_t n, const cld_chunk* chunks,
                      uint64_t chunk_cap, const uint64_t* chunk_offsets, const uint8_t* select, uint32_t flags,
                      uint8_t* out_buf, uint64_t out_cap, uint64_t* out_offsets);
int cld_gather_chunks_device(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n,
                             const cld_chunk* d_chunks, uint64_t chunk_cap, const uint64_t* d_chunk_offsets,
                             const uint8_t* d_select, uint32_t flags, uint8_t* d_out_buf, uint64_t out_cap,
                             uint64_t* d_out_offsets, void* d_work, size_t work_bytes, void* stream);

/* A batch split into lines, for line-level detection without leaving the GPU:
 * each line of a page is one independent document for the detect entries (a
 * crawl pipeline's usual question is the language of each line or paragraph).
 * The split is zero-copy: a line keeps its terminating LF, so the lines tile
 * the text exactly and the line batch is the same buf with a new offsets array.
 *
 * The batch is buf, offsets[0..n], non-decreasing as for every entry; its text
 * is T = [offsets[0], offsets[n]).
 *   boundaries   B is the set of distinct values of offsets[0..n], plus p + 1
 *                for every p in T with buf[p] == 0x0A.  No other byte is
 *                special: CR stays in its line, NUL is an ordinary byte.
 *   lines        are the consecutive pairs of sorted B, m = |B| - 1 of them.  A
 *                line includes its LF; a document's last line may lack one; an
 *                empty document has no line; no line crosses a document.
 *   CLD_LINES_JOIN_BLANK  an LF boundary p + 1 that is not a value of offsets is
 *                dropped when the raw line it ends is blank: the raw line runs
 *                from the largest element of the unflagged B that is <= p
 *                through p, and is blank when it has no byte above 0x20.  Blank
 *                lines therefore join the line after them, blank lines at a
 *                document's end form one line, and every line of a document
 *                except its last holds a byte above 0x20.  Any other flag bit:
 *                CLD_EINVAL.
 *   line_offsets[0..m]  sorted B: line_offsets[0] == offsets[0], line_offsets[m]
 *                == offsets[n].  (buf, line_offsets, m) is a batch for every
 *                cld_detect_batch_device*, group and gather entry.
 *   doc_lines[0..n]  the number of elements of B below offsets[i]: document i's
 *                lines are [doc_lines[i], doc_lines[i + 1]),
 *                line_offsets[doc_lines[i]] == offsets[i], doc_lines[n] == m.
 *   line_doc[0..m)  (NULL: not wanted) the document of each line.
 *   status       (NULL: not wanted) total_lines = m and max_line_bytes, the
 *                longest line.
 * Capacity, as for the chunk vectors: line_offsets holds line_cap + 1 words and
 * line_doc line_cap; doc_lines and status always receive the true values;
 * line_offsets[j] is written for j <= min(m, line_cap), line_doc[j] for j <
 * min(m, line_cap), and nothing past those extents.  line_cap == 0 with
 * line_offsets NULL is the sizing pass: read total_lines, allocate, call again.
 * line_cap > INT32_MAX is CLD_EINVAL: the line batch must be a legal n for the
 * detect entries.
 * cld_split_lines is the host reference, no GPU.  cld_split_lines_device:
 * every pointer in device memory of GPU `device` (8-byte aligned where it holds
 * 64-bit words), enqueued on `stream` (NULL: the runtime's); asynchronous, the
 * host waits for nothing and reads no device word; none of the context's
 * scratch is used, so it may run from several threads, each with a workspace of
 * its own.  buf_bytes bounds d_offsets[n]: every offset is clamped to it, so no
 * offsets word makes a kernel read outside d_buf[0, buf_bytes) or write outside
 * the extents above; where the offsets go down the values are unspecified and
 * the bounds still hold.  The output is the same from run to run: no atomic
 * decides a position (the longest line is an integer maximum).  d_work holds
 * work_bytes >= cld_lines_work_bytes(n, buf_bytes) bytes (a smaller one:
 * CLD_ENOSPC, nothing enqueued) and is free again when the call's work on the
 * stream is done: cld_lines_work_bytes is 8 * (buf_bytes / 1024 + 3) + 73728 --
 * one word per 1 KB tile of the text, the per-range sums and a word per wave --
 * whatever n and line_cap are.
 * CLD_EINVAL: n > INT32_MAX, line_cap > INT32_MAX, unknown flag bits, line_cap
 * > 0 with NULL line_offsets; with n > 0 a NULL or not 8-byte aligned offsets,
 * doc_lines or workspace (the host entry has no workspace); with n > 0 and
 * buf_bytes > 0 a NULL buf (the host entry: with offsets[n] > offsets[0]).
 * n == 0: CLD_OK, with doc_lines[0] = 0 and a zero status; line_offsets[0] is
 * left alone, there is no offsets[0] to copy.
 *
 * cld_lines_to_chunks (host) / cld_lines_to_chunks_device turn the results of
 * the line batch into one cld_chunk vector per document of the original batch,
 * so cld_chunk_totals* and cld_gather_chunks* work at line granularity and keep
 * document identity.  chunks[j] is written for j < min(doc_lines[n], line_cap);
 * with i = line_doc[j]: offset = line_offsets[j] - offsets[i] saturated to
 * [0, INT32_MAX], bytes = the line's length saturated to INT32_MAX, lang1 = the
 * key of line_results[j] exactly as cld_group_by_language defines it
 * (group_flags: CLD_GROUP_TOP1, CLD_GROUP_RELIABLE_ONLY; other bits:
 * CLD_EINVAL), pad = 0; i >= n gives {0, 0, key, 0}.  The chunk offsets of
 * these vectors are doc_lines itself and chunk_cap is line_cap: nothing is
 * copied.  One lane per line, no workspace; stream and device as above.
 * CLD_EINVAL: n or line_cap > INT32_MAX, NULL doc_lines; with n > 0 and
 * line_cap > 0 a NULL line_results, line_offsets, line_doc, offsets or chunks. */
#define CLD_LINES_JOIN_BLANK 1u         /* blank lines join the line after them */
typedef struct cld_lines_status {
  uint64_t total_lines;                 /* m = doc_lines[n]; > line_cap: call again with more room */
  uint64_t max_line_bytes;              /* the longest line */
} cld_lines_status;
size_t cld_lines_work_bytes(size_t n, uint64_t buf_bytes);
int cld_split_lines(const uint8_t* buf, const uint64_t* offsets, size_t n, uint32_t flags, uint64_t* line_offsets,
                    uint32_t* line_doc, uint64_t line_cap, uint64_t* doc_lines, cld_lines_status* status);
int cld_split_lines_device(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n, uint64_t buf_bytes,
                           uint32_t flags, uint64_t* d_line_offsets, uint32_t* d_line_doc, uint64_t line_cap,
                           uint64_t* d_doc_lines, cld_lines_status* d_status, void* d_work, size_t work_bytes,
                           void* stream);
int cld_lines_to_chunks(const cld_result* line_results, const uint64_t* line_offsets, const uint32_t* line_doc,
                        uint64_t line_cap, const uint64_t* offsets, size_t n, const uint64_t* doc_lines,
                        uint32_t group_flags, cld_chunk* chunks);
int cld_lines_to_chunks_device(int device, const cld_result* d_line_results, const uint64_t* d_line_offsets,
                               const uint32_t* d_line_doc, uint64_t line_cap, const uint64_t* d_offsets, size_t n,
                               const uint64_t* d_doc_lines, uint32_t group_flags, cld_chunk* d_chunks, void* stream);

/* The text of HTML pages, with a map back to the page: what the group, chunk
 * and line entries above need in front of them when the batch is HTML (they
 * take their batch as plain text), without leaving the GPU.
 *
 * text(page) is what the reference's span scanner reads of a page in HTML mode
 * (is_plain_text = false) before it looks at letters or scripts: one
 * left-to-right walk (getonescriptspan.cc:150-203, 393-468, 503-541) over the
 * page bytes [0, L), from p = 0:
 *   '<'          a '<' the walk reaches starts a tag of t =
 *                ScanToPossibleLetter(page + p, L - p) bytes, t >= 1: comments,
 *                <script>...</script> and <style>...</style> bodies and quoted
 *                attributes exactly as the reference's tag parser consumes
 *                them.  It emits one separator byte, 0x20 -- or 0x0A under
 *                CLD_HTMLTEXT_BLOCK_LF when the tag is a block tag -- with
 *                source position p; the walk continues at p + t.
 *   '&'          a '&' the walk reaches is read by EntityToBuffer.  A decodable
 *                entity consumes tlen bytes and emits its plen decoded UTF-8
 *                bytes, byte k with source position p + k.  An undecodable '&'
 *                consumes one byte and emits nothing: the scanner drops it and
 *                the run of letters goes on ("AT&T" reads "ATT"), so that the
 *                text scores as the page scores.
 *   other bytes  emit themselves, with source position p.
 * Nothing is read outside the page: a tag left open at the page's end consumes
 * to L and no further, an entity is cut at L.
 * No growth: a decoded entity never holds more bytes than it consumed (the
 * shortest forms are "&#9" 3 -> 1, "&lt" 4 -> 2, "&ni;" 4 -> 3, "&#65536"
 * 7 -> 4), so text_len <= L and the source positions are strictly increasing.
 * Block tags: the bytes after '<' or '</' spell one of CLD_HTMLTEXT_BLOCK_TAGS,
 * ASCII case-insensitive, followed by a byte that is not an ASCII letter or
 * digit, or by the page end.  Comments and every other tag give a space.  Space
 * and LF are both non-letters to the detector: the flag changes no detection
 * result, it gives cld_split_lines* the lines of the text.
 * Every page is extracted whatever its bytes are (tags and entities are a
 * matter of bytes; the well-formedness of the UTF-8 around them plays no part).
 *
 * The output is page-aligned -- no sizing pass, no workspace:
 *   out          page i's text is out[offsets[i] .. offsets[i] + text_len[i]);
 *                the rest of the page's range is filled with 0x20.  (out,
 *                offsets, n) is at once a batch for every
 *                cld_detect_batch_device*, group, gather and line entry:
 *                trailing spaces add nothing to any span.  out must not overlap
 *                buf.
 *   text_len[n]  (NULL: not wanted) the bytes of each page's text.
 *   pos          (NULL: not wanted) one uint32_t per output byte, indexed like
 *                out: that byte's source position within its page, and L at the
 *                padding.
 *   status       (NULL: not wanted) the sums over the batch.
 * Bytes outside [offsets[0], offsets[n]) are not written, in either array.
 * cld_html_text is the host reference, no GPU; it reads the entity sections of
 * the table blob on the host, as cld_hint_priors reads the hint sections.
 * Tables without the HTML sections: CLD_EINVAL, from both entries.
 * cld_html_text_device: every pointer in device memory of GPU `device` (8-byte
 * aligned offsets, 4-byte aligned text_len and pos, 8-byte aligned status),
 * enqueued on `stream` (NULL: the runtime's); asynchronous, the host reads no
 * device word; none of the context's scratch is used and there is no
 * workspace.  buf_bytes bounds d_offsets[n]: every offset is clamped to it, so
 * no offsets word makes a kernel read outside d_buf[0, buf_bytes) or write
 * outside the same range of d_out / d_pos; where the offsets go down the values
 * are unspecified and the bounds still hold.  The caller keeps pages <=
 * INT32_MAX bytes.  The status is written by the call's last kernel; the
 * counts are integer sums, so the output is the same from run to run.  One
 * wavefront takes one page.
 * CLD_EINVAL: unknown flag bits; n > INT32_MAX; with n > 0 a NULL offsets; a
 * NULL buf or out with buf_bytes > 0, whatever n is (the host entry has no
 * buf_bytes: with n > 0 and offsets[n] > offsets[0]).  Otherwise n == 0: CLD_OK
 * and a zero status.
 *
 * cld_chunks_to_page (the host reference, no GPU) / cld_chunks_to_page_device
 * take chunk vectors that index the text -- from cld_detect_batch_device_vec on
 * the text batch, or from cld_lines_to_chunks_device with doc_lines as chunk
 * offsets -- and rewrite them to index the page.  Documents and vectors are
 * read exactly as cld_chunk_totals defines them (the chunk_cap rule, the piece
 * [s, e) clipped to [0, L)).  With P(x) = min(pos[offsets[i] + x], L) for x < L
 * and P(L) = L, out_chunks[c] = {offset = P(s), bytes = max(P(e) - P(s), 0),
 * lang1, pad = 0} for every existing chunk c of every document.  Pieces that
 * tile the text therefore tile the page: a piece ends where the next text
 * byte's source begins, so it takes the markup that follows it.  pos values
 * are clamped: a hostile pos gives wrong numbers and no access outside the
 * arrays.  out_chunks may be chunks itself.  The device entry: one wavefront
 * per document, lanes over its chunks; no workspace; stream and device as above.
 * CLD_EINVAL: as cld_chunk_totals, and NULL pos or out_chunks where there is
 * a chunk to write (n > 0 and chunk_cap > 0). */
#define CLD_HTMLTEXT_BLOCK_LF 1u        /* a block tag's separator byte is 0x0A */
#define CLD_HTMLTEXT_BLOCK_TAGS \
  "address article aside blockquote body br dd div dl dt fieldset figcaption figure footer form " \
  "h1 h2 h3 h4 h5 h6 head header hr html li main nav ol option p pre script section style table tbody td " \
  "tfoot th thead title tr ul"
typedef struct cld_htmltext_status {
  uint64_t text_bytes;                  /* sum of text_len */
  uint64_t tags;                        /* tags reached */
  uint32_t entities;                    /* entities decoded */
  uint32_t dropped;                     /* undecodable '&' dropped */
} cld_htmltext_status;
int cld_html_text(const uint8_t* buf, const uint64_t* offsets, size_t n, uint32_t flags, uint8_t* out,
                  int32_t* text_len, uint32_t* pos, cld_htmltext_status* status);
int cld_html_text_device(int device, const uint8_t* d_buf, const uint64_t* d_offsets, size_t n, uint64_t buf_bytes,
                         uint32_t flags, uint8_t* d_out, int32_t* d_text_len, uint32_t* d_pos,
                         cld_htmltext_status* d_status, void* stream);
int cld_chunks_to_page(const uint64_t* offsets, size_t n, const uint32_t* pos, const cld_chunk* chunks,
                       uint64_t chunk_cap, const uint64_t* chunk_offsets, cld_chunk* out_chunks);
int cld_chunks_to_page_device(int device, const uint64_t* d_offsets, size_t n, const uint32_t* d_pos,
                              const cld_chunk* d_chunks, uint64_t chunk_cap, const uint64_t* d_chunk_offsets,
                              cld_chunk* d_out_chunks, void* stream);

/* The preparation step alone, on GPU 0 (host buffers): out_buf receives the
 * prepared documents back to back (capacity >= offsets[n]-offsets[0] + n
 * bytes), out_offsets[0..n] their offsets.  flags: CLD_FLAG_STRIP_EXTRAS and/or
 * CLD_FLAG_CSTRING.  Blocks until the result is on the host. */
int cld_prepare_batch(const uint8_t* buf, const uint64_t* offsets, size_t n, uint32_t flags,
                      uint8_t* out_buf, uint64_t* out_offsets);

/* Pinned host memory for callers of cld_detect_batch.  Documents, offsets and
 * results that live in such memory skip the runtime's staging copy: they are
 * DMA'd straight from/to it (the batch HTTP endpoint keeps its request and
 * response buffers here).  Any other host memory works too and is staged
 * through the runtime's own pinned chunk buffers.  NULL on failure. */
void* cld_host_alloc(size_t bytes);
void cld_host_free(void* p);

/* LanguageCode / LanguageName (lang_script.cc:212-217, :205-210). */
const char* cld_language_code(int lang);
const char* cld_language_name(int lang);

/* Counters of the most recent batch on this thread's last device call. */
typedef struct cld_batch_stats {
  uint64_t docs;
  uint64_t short_docs;       /* finished by the short-document (wavefront) kernel */
  uint64_t general_docs;     /* finished by the sequential any-length kernel      */
  uint64_t passes[4];        /* documents needing 1, 2, 3 passes; [3] = errors     */
  double short_ms, general_ms; /* kernel time from HIP events                     */
  uint64_t long_docs;        /* finished by the long-document wavefront kernel    */
  double long_ms;
  uint64_t long_requeue[8];  /* why k_long handed documents on: 1 length, 2 scanner
                                state, 3 span/lowercase, 4 Squeeze restart, 5 capacity */
} cld_batch_stats;
int cld_last_batch_stats(int device, cld_batch_stats* st);

/* Which long-document kernels scored the batch cld_last_batch_stats speaks of
 * (read-only; the list counts the staged kernels keep on the device, summed
 * over the chunks of a host batch like cld_batch_stats).  A long document is
 * one k_wave did not finish.  The staged path stores its pass-1 spans and
 * scores it whole (k_lscore) or, with many spans, in groups of 16 spans
 * (k_lgroup / k_lfinish); what it cannot take -- the Squeeze restart, a block
 * wider than its 2 KB window, no room in the store or the group list, records
 * that outgrew their room -- the fused k_long redoes from scratch.
 *   long_list      documents on the long list
 *   staged_whole   stored, pass 1 scored whole
 *   staged_split1  stored, pass 1 scored in groups;  groups1: the groups asked
 *                  for, those of a document that found no room in the group
 *                  list included (groups2 likewise)
 *   staged_pass2   stored documents whose pass 1 was not good enough (whole
 *                  and split ones); staged_split2 / groups2: the split ones
 *                  among them and their pass-2 groups
 *   to_fused       documents the staged kernels handed to the fused k_long,
 *                  at any stage (a list of at most 64 long documents that
 *                  reaches the staged kernels goes there whole)
 *   store_units    16-byte units of the span store asked for (over the
 *                  store's size: it ran out)
 *   spec_taken     speculative pass-2 results the fused kernel took
 * long_list == staged_whole + staged_split1 + (documents handed on by the
 * span stage); to_fused also counts the later stages' hand-ons.
 * Where the runtime skipped the staged launches altogether -- the host path
 * with at most 64 documents of more than 256 bytes in a chunk, none of them
 * over the fused kernel's 1 MB cap or CLD_LONG_SMALL_KB; the vector entries;
 * diagnostics; CLD_LONG_STAGED=0 -- every field from staged_whole to store_units reads 0
 * and the fused kernel scored the whole list.  A call k_wave finished alone
 * reads all zeros.  CLD_EINVAL: no such device (before cld_init), st NULL.
 * Not updated by the device-resident vector and group entries. */
typedef struct cld_route_stats {
  uint64_t long_list, staged_whole, staged_split1, groups1, staged_pass2, staged_split2, groups2, to_fused,
      store_units, spec_taken;
  uint64_t reserved[6];
} cld_route_stats;
int cld_last_route_stats(int device, cld_route_stats* st);

/* ---- Run-time table loading (CLD2 dynamic data, cld2_dynamic_data.h:22-147).
 * A "cld2_data_file00" image carries the scoring tables of ScoringTables
 * (CJK unigram machine, kAvgDeltaOctaScore, compat/deltabi/distinctbi/quad/
 * quad2/deltaocta/distinctocta); the other tables stay the built-in ones.
 * Loading re-uploads the tables to every initialised GPU (after draining
 * in-flight work) and applies to every later call.  Not to be called
 * concurrently with detection calls (the reference's loaders are not either).
 *
 *   cld_load_data_from_file         replaces CLD2::loadDataFromFile
 *                                   (compact_lang_det.h:393, impl.cc:108-121)
 *   cld_load_data_from_raw_address  replaces CLD2::loadDataFromRawAddress
 *                                   (compact_lang_det.h:406, impl.cc:123-136)
 *   cld_unload_data                 replaces CLD2::unloadData (compact_lang_det.h:413);
 *                                   here it restores the built-in tables
 *   cld_is_data_dynamic             1 while data-file tables are in use
 *                                   (cf. CLD2::isDataDynamic, compact_lang_det.h:426)
 * They return CLD_OK or CLD_EINVAL (malformed file: bad marker, header or
 * file size mismatch as in cld2_dynamic_data_loader.cc:41-146, or a block /
 * indirect index outside the file); a failed load keeps the tables in use. */
int cld_load_data_from_file(const char* path);
int cld_load_data_from_raw_address(const void* raw, uint32_t length);
int cld_unload_data(void);
int cld_is_data_dynamic(void);

/* Host-only helpers (no GPU): write the tables in use as a CLDT blob, and
 * convert a cld2 data file over a base CLDT (NULL = the built-in one) into a
 * CLDT file -- the form the test oracle reads. */
int cld_export_tables(const char* out_cldt_path);
int cld_convert_data_file(const char* cld2_data_file, const char* base_cldt, const char* out_cldt_path);

/* Build / table identity string: "cld-mi355x <ver> tables=<path> quad=<q>
 * quad_build=<date>" where q says which quadgram table is live: "empty-Q0"
 * (the default: the reference's placeholder pattern, no quadgram scoring),
 * "synthetic-Q1" (the test/bench table, opted into via CLD_MI355X_TABLES) or
 * "other" (e.g. a real table from cld_load_data_from_file). */
const char* cld_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CLD_MI355X_H_ */
