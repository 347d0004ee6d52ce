// cld_kernels.h -- launch interface between the host runtime and the kernels.
#ifndef CLD_KERNELS_H_
#define CLD_KERNELS_H_
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "cld_device.h"

// Wavefront-per-document bucket (cld_wave.hip)
constexpr int kWaveCap = 256;
#ifndef WAVE_WPB
#define WAVE_WPB 1
#endif
constexpr int kWaveWPB = WAVE_WPB;   // waves (documents) per workgroup
// Largest kLgProbV2Tbl score byte the packed wave tote accepts (runtime checks the blob)
constexpr int kMaxLgProbScore = 16;
// k_wave's deferred tail (plain batches): the wave leaves each document a slot
// of 16-byte words in a record buffer and k_wtail (cld_wtail.hip), one lane
// per document, makes the chunk summaries, the DocTote and the document level.
//   word 0, the header, written by the wave for every document of the batch:
//     x = records that follow, or kTailNone (k_wtail leaves the document alone:
//         skipped or re-queued by the wave, or empty and already written)
//     y = total text bytes
//   words 1..x, in DocTote::Add order:
//     a scored chunk     x = key1 | key2 << 8 (per-script numbers, 0xFF: none)
//                        y = score1 | score2 << 16
//                        z = lo | hi << 16 (the chunk's offsets as SetChunkSummary reads them)
//                        w = grams | ulscript << 16
//     an unscored span   x = kTailSpan, y = language, z = text bytes
//                        (RTypeNone / RTypeOne: Add(language, bytes, bytes, 100))
// A document with more than kTailRecs records is re-queued by the wave.
constexpr int kTailRecs = 31;
constexpr size_t kTailSlotBytes = 16 * (1 + kTailRecs);
constexpr uint32_t kTailNone = 0xFFFFFFFFu, kTailSpan = 0x10000u;


// Device counter slots (three 64-byte lines, zeroed per batch)
// kCtrRequeue/kCtrDequeue: the k_long list (documents longer than k_wave takes,
// the ones it hands on, HTML pages the rewrite did not take);
// kCtrSpecial: those HTML pages.  (kCtrRequeue2 / kCtrDequeue2: unused.)
enum { kCtrRequeue = 0, kCtrDequeue = 1, kCtrPass1 = 2, kCtrPass2 = 3, kCtrPass3 = 4, kCtrError = 5,
       kCtrRequeue2 = 6, kCtrDequeue2 = 7, kCtrWhy = 8 /* 8 slots: k_long re-queue reasons */,
       kCtrSpecial = 16, kCtrSpecTake = 17 /* k_long: speculative pass-2 results taken */,
       kCtrSpecDone = 18 /* k_long: waves finished (speculating launches) */,
       // staged long-document path (k_lspan / k_lscore / k_lrep): list counts and dequeue cursors
       kCtrStFall = 19 /* to the fused k_long */, kCtrStDqSpan = 20, kCtrStOk = 21 /* spans stored */,
       kCtrStDqS1 = 22, kCtrStP2 = 23 /* pass 2 */, kCtrStDqRep = 24, kCtrStDqS2 = 25, kCtrStDqFall = 26,
       kCtrStPool = 27 /* store 16-byte units taken */,
       // span-parallel documents: group lists and document lists of passes 1 and 2
       kCtrStG1 = 28, kCtrStDqG1 = 29, kCtrStPar1 = 30, kCtrStDqF1 = 31,
       kCtrStG2 = 32, kCtrStDqG2 = 33, kCtrStPar2 = 34, kCtrStDqF2 = 35,
       // heavy (many-span) entries of the stored and pass-2 lists, filled from the top
       kCtrStOkH = 36, kCtrStP2H = 37,
       kCtrSeq = 38 /* k_long: documents scored on the sequential span source (cld_seq.hip) */, kCtrSlots = 48 };
// Per-document routing bits of cld_detect_batch_ex (special[i])
// kSpecialRewritten: an HTML document k_html_rewrite turned into plain text
// (hbuf / hflag); k_long scores the original page if it needs the sequential
// span source.  kSpecialNoVec (vec mode): a rewritten page whose offset map the
// parallel span builder cannot reproduce (cld_html.hip); k_long<VEC> scans the
// original page with the sequential span source.
// kSpecialQuads / kSpecialBestEffort (the _docflags entries): the document's
// own kCLDFlagScoreAsQuads / kCLDFlagBestEffort, on top of the batch's cflags.
enum : uint8_t { kSpecialHtml = 1, kSpecialPriors = 2, kSpecialRewritten = 4, kSpecialNoVec = 8,
                 kSpecialQuads = 16, kSpecialBestEffort = 32 };
// The CLD2 flags a routing byte carries (0 for a byte without the two bits,
// so a batch without per-document flags scores with cflags alone), and back.
constexpr uint32_t cld_special_cflags(uint32_t sp) {
  return ((sp & kSpecialQuads) << 4) | ((sp & kSpecialBestEffort) << 9);
}
constexpr uint8_t cld_cflags_special(uint32_t flags) {
  return (uint8_t)(((flags & CLD_FLAG_SCORE_AS_QUADS) >> 4) | ((flags & CLD_FLAG_BEST_EFFORT) >> 9));
}
static_assert(cld_special_cflags(kSpecialQuads) == CLD_FLAG_SCORE_AS_QUADS &&
                  cld_special_cflags(kSpecialBestEffort) == CLD_FLAG_BEST_EFFORT &&
                  cld_cflags_special(CLD_FLAG_SCORE_AS_QUADS | CLD_FLAG_BEST_EFFORT) ==
                      (kSpecialQuads | kSpecialBestEffort),
              "routing bits <-> CLD2 flags");
// k_long: waves per workgroup
constexpr int kLongWPB = 4;

extern "C" {
// ResultChunkVector mode: k_route_vec lists every document under
// counters[kCtrRequeue]; k_long<VEC> then scores them with one VecSlot per
// resident wave (vslots: n_slots * cld_vec_slot_bytes()); document i builds
// its vector in pool[pool_off[i] .. pool_off[i+1]) and writes its size (or
// -1: it outgrew its region, or has no result) to n_chunks[i].
size_t cld_vec_slot_bytes();
hipError_t cld_launch_route_vec(int n, uint32_t* counters, uint32_t* long_list, hipStream_t s);
hipError_t cld_launch_long_vec(const DevTables* d_T, const uint8_t* buf, const uint64_t* offs, const uint32_t* list,
                               cld_result* out, uint8_t* slots, uint8_t* vslots, int n_slots, uint32_t* seq_list,
                               uint32_t* counters, uint32_t cflags, const uint8_t* special, const uint32_t* priors,
                               const uint8_t* hbuf, const uint8_t* hflag, const uint32_t* hpos, const uint32_t* hgap,
                               cld_chunk* pool, const uint64_t* pool_off, int32_t* n_chunks, hipStream_t s);
hipError_t cld_launch_vec_gather(const cld_chunk* pool, const uint64_t* pool_off, const int32_t* n_chunks,
                                 const uint64_t* pos, int n, cld_chunk* dst, hipStream_t s);
// The device-resident vector path (cld_vec.hip; cld_detect_batch_device_vec),
// the host steps of cld_detect_batch_vec as kernels:
// cld_launch_vec_plan: region[i] = document i's pool region in chunks, for
// cld_launch_scan_lengths to turn into pool_off -- len + len/4 + 8, with
// kVecRegionsBig 8 len + 256, with kVecRegionsOne (the CLD_VEC_POOL_SMALL
// test hook) 1.
// cld_launch_vec_finish, after k_long<VEC> and the UTF-8 fixup: counts[i] =
// max(n_chunks[i], 0) for the scan into the chunk offsets; a document with
// n_chunks -1 gets the CLD_LANG_FAILED result and is counted in
// status->failed_docs; valid_prefix (nullable; over offs, the documents as
// given): documents the check rejected are counted in status->rejected_docs.
// status is zeroed by the caller.
// cld_launch_vec_gather_chunks: the first min(chunk_offs[n], cap) chunks from
// the pool regions to dst in document order, work split over output
// positions; writes status->total_chunks = chunk_offs[n].
enum { kVecRegionsSmall = 0, kVecRegionsBig = 1, kVecRegionsOne = 2 };
hipError_t cld_launch_vec_plan(const uint64_t* offs, int n, int mode, uint64_t* region, hipStream_t s);
hipError_t cld_launch_vec_finish(const uint64_t* offs, int n, const int32_t* n_chunks, const int32_t* valid_prefix,
                                 cld_result* out, uint32_t unknown_language, uint64_t* counts, cld_vec_status* status,
                                 hipStream_t s);
hipError_t cld_launch_vec_gather_chunks(const cld_chunk* pool, const uint64_t* pool_off, const uint64_t* chunk_offs,
                                        int n, cld_chunk* dst, uint64_t cap, cld_vec_status* status, hipStream_t s);
// special (nullable): per-document kSpecial* bits; HTML documents are appended
// to special_list under counters[special_ctr] instead of being scored, hinted
// ones (kSpecialPriors) are scored with their 16 ApplyHints langprobs
// (priors + 16 * i; k_long reads the same two arrays).
// cflags (every launcher): the caller's public CLD2 flags, CLD_FLAG_SCORE_AS_QUADS /
// CLD_FLAG_BEST_EFFORT (compact_lang_det.h:343, :349), the same for every document;
// a document whose routing byte carries kSpecialQuads / kSpecialBestEffort is
// scored with cflags | cld_special_cflags(special[i]).
// tail_recs (nullable; n * kTailSlotBytes, 16-byte aligned, not zeroed): a plain
// batch -- special, priors, hbuf, hflag and prof all null -- runs k_wave's
// deferred instantiation and then k_wtail over it; null keeps the tail in the
// wave, as every other batch does.
hipError_t cld_launch_wave(const DevTables* T, const uint8_t* buf, const uint64_t* offs, int n,
                           cld_result* out, uint32_t* requeue_list, uint32_t* counters,
                           unsigned long long* prof, const uint8_t* special, uint32_t* special_list,
                           int special_ctr, uint32_t cflags, const uint32_t* priors, const uint8_t* hbuf,
                           const uint8_t* hflag, uint32_t* hist2, uint8_t* tail_recs, hipStream_t s);
// k_wave alone, without k_route: the caller guarantees every document is at
// most kWaveCap bytes (run_tiny's request-sized batches).  Documents the wave
// kernel cannot finish are listed under counters[kCtrRequeue], or, with
// requeue_list == nullptr (counters unused), marked in their result:
// summary_lang = kWaveRequeued.
constexpr uint16_t kWaveRequeued = 0xFFFE;
// kMaxScriptBytes (cld_prims.hip): rewritten HTML pages this long and
// longer carry page offsets (hpos / hgap) for the span soft limit
constexpr int kHtmlSoftMin = 40928;
// lng::kDocCap (cld_long.hip): the fused k_long takes documents up to this
// many bytes less 64; longer ones need the staged path's big-document regions
constexpr uint64_t kLongDocCap = 1u << 20;
hipError_t cld_launch_wave_only(const DevTables* T, const uint8_t* buf, const uint64_t* offs, int n, cld_result* out,
                                uint32_t* requeue_list, uint32_t* counters, uint32_t cflags, hipStream_t s);
// HTML documents of the batch (special & kSpecialHtml) rewritten into plain
// text (cld_html.hip): hbuf / hflag are indexed like buf (offs); special is
// updated in place (kSpecialHtml -> kSpecialRewritten for each rewritten page);
// prof (nullable, CLD_PROFILE_STAGES=1): cycles of step 2 summed into prof[0].
// hpos (nullable): per rewritten byte, its page offset (vec mode's MapBack;
// the span soft limit of pages of kMaxScriptBytes and more); hgap (with hpos):
// at a byte that follows dropped '&'s, where they began.  Written for pages of
// hpos_min bytes and more (vec mode 0, plain kMaxScriptBytes).
hipError_t cld_launch_html_rewrite(const DevTables* d_T, const uint8_t* buf, const uint64_t* offs, int n,
                                   uint8_t* special, uint8_t* hbuf, uint8_t* hflag, uint32_t* hpos, uint32_t* hgap,
                                   int hpos_min, unsigned long long* prof, hipStream_t s);
size_t cld_wave_smem_bytes();
// (hist2: zeroed by k_route when cld_launch_wave was given it: zeroed = true)
hipError_t cld_launch_order_long(const uint64_t* offs, const uint32_t* list, const uint32_t* counters,
                                 uint8_t* key, uint32_t* hist2, uint32_t* sorted, bool zeroed, hipStream_t s);
size_t cld_long_slot_bytes();
size_t cld_cpt_entries();
hipError_t cld_build_cpt(const DevTables* T, uint64_t* out, hipStream_t s);
size_t cld_keytab_entries();
hipError_t cld_build_keytab(const DevTables* T, uint64_t* out, hipStream_t s);
// ind -> tote adds for the seven scoring tables, back to back in `out`
// (compat, deltabi, distinctbi, quad, quad2, deltaocta, distinctocta order);
// sets each table's `adds` pointer in *T.
size_t cld_adds_entries(const DevTables* T);
hipError_t cld_build_adds(DevTables* T, uint64_t* out, hipStream_t s);
int cld_long_waves_per_simd();
size_t cld_strip_scratch_bytes(int n);
hipError_t cld_launch_strip_offsets(const uint8_t* buf, const uint64_t* offs, int n, uint32_t flags,
                                    uint64_t* out_offs, void* scratch, hipStream_t s);
hipError_t cld_launch_strip_write(const uint8_t* buf, const uint64_t* offs, int n, uint32_t flags,
                                  const uint64_t* out_offs, uint8_t* out, hipStream_t s);
// Exclusive scan of n lengths (scratch[0..n), written by the caller) into
// out_offs[0..n]; scratch as for cld_launch_strip_offsets.
hipError_t cld_launch_scan_lengths(int n, uint64_t* out_offs, void* scratch, hipStream_t s);
// The interchange-valid UTF-8 check (cld_valid.hip; SpanInterchangeValid,
// compact_lang_det_impl.cc:72-80).  Documents of at most kValidShortMax bytes
// take one wave each, longer ones go in tiles of kValidTile bytes at
// kValidTile-aligned addresses.  bytes_hint: offs[n] - offs[0] where the host
// knows it (it sizes the tile kernels' grid), else 0.
constexpr int kValidShortMax = 256;
constexpr int kValidTile = 1024;
hipError_t cld_launch_valid_prefix(const uint8_t* buf, const uint64_t* offs, int n, int32_t* valid_prefix,
                                   uint64_t bytes_hint, hipStream_t s);
// CLD_FLAG_SCRUB_UTF8 / cld_scrub_utf8_*: out[offs[i] + j] = byte j of document
// i with every error position of the check replaced by 0x20 (out is indexed
// like buf and does not overlap it; one 16-byte store per lane of a tile where
// out - buf is a multiple of 16, byte stores otherwise).  replaced[i]
// (nullable): the number of replaced bytes; valid_prefix[i] (nullable): the
// first of them, SpanInterchangeValid of the document as given.
hipError_t cld_launch_scrub(const uint8_t* buf, const uint64_t* offs, int n, uint8_t* out, int32_t* replaced,
                            int32_t* valid_prefix, uint64_t bytes_hint, hipStream_t s);
// CLD_FLAG_CHECK_UTF8: len[i] = document i's length when valid_prefix[i] says
// the whole of it is valid, else 0; the valid documents copied to out at
// out_offs (the scan of len); the reference's "rejected" result written over
// out[i] (and 0 over n_chunks[i], nullable) for every other document.
hipError_t cld_launch_valid_lens(const uint64_t* offs, int n, const int32_t* valid_prefix, uint64_t* len,
                                 hipStream_t s);
hipError_t cld_launch_valid_copy(const uint8_t* buf, const uint64_t* offs, int n, const uint64_t* out_offs,
                                 uint8_t* out, uint64_t bytes_hint, hipStream_t s);
hipError_t cld_launch_valid_fixup(const uint64_t* offs, int n, const int32_t* valid_prefix, cld_result* out,
                                  int32_t* n_chunks, uint32_t unknown_language, hipStream_t s);
// cld_group_by_language_device / cld_gather_docs_device (cld_group.hip).  Both
// cut their n items into at most kGroupWgs contiguous ranges of
// cld_group_range(n) items, a multiple of kGroupTile, one workgroup each, so
// `work` (kGroupWorkBytes, 8-byte aligned, not zeroed) does not grow with n:
// per-range histograms (u32) and byte totals (u64) over the bins, the counts;
// the gather keeps its per-range sums there.  n, m <= INT32_MAX.
// cld_launch_group: counts, bin_bytes (with offs), order, group_offsets each
// nullable.  cld_launch_gather: out_offs[0..m] always, out[0, min(total, cap))
// when cap > 0.
constexpr int kGroupWgs = 256;
constexpr int kGroupTile = 512;
constexpr size_t kGroupWorkBytes = (size_t)kGroupWgs * CLD_GROUP_BINS * (sizeof(uint32_t) + sizeof(uint64_t)) +
                                   (CLD_GROUP_BINS + 1) * sizeof(uint64_t);
inline uint32_t cld_group_range(uint32_t n) {
  const uint32_t per = n / kGroupWgs + (n % kGroupWgs != 0);
  return per <= (uint32_t)kGroupTile ? (uint32_t)kGroupTile : (per + kGroupTile - 1) / kGroupTile * kGroupTile;
}
hipError_t cld_launch_group(const cld_result* res, uint32_t n, uint32_t flags, const uint64_t* offs, uint64_t* counts,
                            uint64_t* bin_bytes, uint32_t* order, uint64_t* group_offsets, void* work, hipStream_t s);
hipError_t cld_launch_gather(const uint8_t* buf, const uint64_t* offs, uint32_t n_src, const uint32_t* index, uint32_t m,
                             uint8_t* out, uint64_t cap, uint64_t* out_offs, void* work, hipStream_t s);
// cld_chunk_totals_device / cld_gather_chunks_device (cld_chunks.hip).  `work`
// (cld_chunk_work(chunk_cap) bytes, 8-byte aligned, not zeroed): a fixed part
// -- the totals' per-range counts and bytes over the bins, u64 each, for the
// at most kGroupWgs ranges of cld_chunk_doc_range(n) documents; the gather's
// instance count and per-range sums -- then chunk_cap + 1 u64, the gather's
// output position of every chunk's piece.  n <= INT32_MAX, chunk_cap <=
// UINT32_MAX.  cld_launch_chunk_totals: counts, bytes each nullable.
// cld_launch_chunk_gather: out_offs[0..n] always, out[0, min(total, cap)) when
// cap > 0.
constexpr size_t kChunkWorkFixed = (size_t)kGroupWgs * 2 * CLD_GROUP_BINS * sizeof(uint64_t);
inline size_t cld_chunk_work(uint64_t chunk_cap) { return kChunkWorkFixed + (size_t)(chunk_cap + 1) * sizeof(uint64_t); }
inline uint32_t cld_chunk_doc_range(uint32_t n) {
  const uint32_t per = n / kGroupWgs + (n % kGroupWgs != 0);
  return per ? per : 1;
}
hipError_t cld_launch_chunk_totals(const uint64_t* offs, uint32_t n, const cld_chunk* chunks, const uint64_t* chunk_offs,
                                   uint64_t chunk_cap, uint64_t* counts, uint64_t* bytes, void* work, hipStream_t s);
hipError_t cld_launch_chunk_gather(const uint8_t* buf, const uint64_t* offs, uint32_t n, const cld_chunk* chunks,
                                   const uint64_t* chunk_offs, uint64_t chunk_cap, const uint8_t* select, uint32_t flags,
                                   uint8_t* out, uint64_t out_cap, uint64_t* out_offs, void* work, hipStream_t s);
// cld_split_lines_device / cld_lines_to_chunks_device (cld_lines.hip).  The
// text is read in tiles of kLinesTile bytes, one wave each; the tile words are
// scanned over at most kLinesWgs ranges of tiles.  `work` (cld_lines_work(buf_bytes)
// bytes, 8-byte aligned, not zeroed): a fixed part -- the per-range maxima and
// sums, the longest line of each of at most kLinesWaves waves -- then one u64
// per tile and one more.  buf_bytes
// bounds offs[n]; the text has at most buf_bytes / kLinesTile + 2 tiles (a
// 16-byte skew and a ragged end).  n, line_cap <= INT32_MAX.
// cld_launch_split_lines: line_offsets, line_doc, status each nullable;
// max_wgs (0: as many as stay resident): a cap on the workgroups of the two
// text kernels, so that a test gives every wave a run of many tiles at a
// small size.
constexpr int kLinesTile = 1024;
constexpr int kLinesWgs = kGroupWgs;
constexpr int kLinesWaves = 8192;
constexpr size_t kLinesWorkFixed = 8192 + kLinesWaves * sizeof(uint64_t);
inline size_t cld_lines_work(uint64_t buf_bytes) {
  return kLinesWorkFixed + (size_t)(buf_bytes / kLinesTile + 3) * sizeof(uint64_t);
}
hipError_t cld_launch_split_lines(const uint8_t* buf, const uint64_t* offs, uint32_t n, uint64_t buf_bytes, uint32_t flags,
                                  uint64_t* line_offsets, uint32_t* line_doc, uint64_t line_cap, uint64_t* doc_lines,
                                  cld_lines_status* status, void* work, uint32_t max_wgs, hipStream_t s);
hipError_t cld_launch_lines_to_chunks(const cld_result* res, const uint64_t* line_offsets, const uint32_t* line_doc,
                                      uint64_t line_cap, const uint64_t* offs, uint32_t n, const uint64_t* doc_lines,
                                      uint32_t group_flags, cld_chunk* chunks, hipStream_t s);
// cld_html_text_device / cld_chunks_to_page_device (cld_htmltext.hip).  One wave
// per page: pages of at most kHtmlTextStage bytes are staged in LDS, longer ones
// read in place; a page is walked in segments of whole 64-byte windows holding
// at most kHtmlTextCands '<' / '&' candidates.  No workspace.  buf_bytes bounds
// offs[n]; n <= INT32_MAX.  cld_launch_html_text: text_len, pos, status each
// nullable; status is zeroed on the stream, then summed into by the kernel;
// max_wgs (0: 2048): a cap on the workgroups, so that a test makes every wave
// take several pages at a small size.
constexpr int kHtmlTextStage = 2048;
constexpr int kHtmlTextCands = 256;
hipError_t cld_launch_html_text(const DevTables* d_T, const uint8_t* buf, const uint64_t* offs, uint32_t n,
                                uint64_t buf_bytes, uint32_t flags, uint8_t* out, int32_t* text_len, uint32_t* pos,
                                cld_htmltext_status* status, uint32_t max_wgs, hipStream_t s);
hipError_t cld_launch_chunks_to_page(const uint64_t* offs, uint32_t n, const uint32_t* pos, const cld_chunk* chunks,
                                     uint64_t chunk_cap, const uint64_t* chunk_offs, cld_chunk* out, hipStream_t s);
// ApplyHints (cld_hints.hip; compact_lang_det_impl.cc:1587-1684), one wave
// per document: priors14 (14 per document, trimmed to 4, zero-padded),
// boosts16 (the 16 langprobs enqueue() takes as `priors`) and special (the
// routing byte: kSpecialHtml unless plain, kSpecialPriors when a langprob is
// non-zero); each nullable.  hints (nullable): one record per document, its
// content-language text in hint_text[0, hint_text_bytes).  plain 0: the lang=
// scan of each document's first 8 KB.  doc_flags (nullable): one word per
// document, masked to CLD_FLAG_HTML | SCORE_AS_QUADS | BEST_EFFORT: document i
// is HTML (scan, kSpecialHtml) when plain is 0 or its word says so, and its
// two CLD2 flags go into special as kSpecialQuads / kSpecialBestEffort.
// H by value to the kernel.
hipError_t cld_launch_apply_hints(const DevHints* H, const uint8_t* buf, const uint64_t* offs, int n,
                                  const cld_hints_dev* hints, const uint8_t* hint_text, uint64_t hint_text_bytes,
                                  int plain, const uint32_t* doc_flags, int16_t* priors14, uint32_t* boosts16,
                                  uint8_t* special, hipStream_t s);
// fault_doc (k_long): test hook, batch index of a document made to fail
// (0xFFFFFFFF: none): it gets no result (summary CLD_LANG_FAILED).
// seq_list (n entries, counters[kCtrRequeue2]): the documents k_long hands to
// its SEQ instantiation (the sequential span source, cld_seq.hip), which the
// launch runs right after it.
// d_T: the device's DevTables copy in HBM (k_long reads the table set through
// it: holding the by-value kernel argument in registers made the kernel spill
// it to scratch and reload table fields from there at every probe)
hipError_t cld_launch_long(const DevTables* d_T, const uint8_t* buf, const uint64_t* offs, const uint32_t* list,
                           cld_result* out, uint8_t* slots, int n_slots, uint32_t* seq_list,
                           uint32_t* counters, uint32_t* trace, uint32_t* dbg, uint32_t dbg_doc,
                           unsigned long long* prof, uint32_t cflags, const uint8_t* special,
                           const uint32_t* priors, const uint8_t* hbuf, const uint8_t* hflag, const uint32_t* hpos,
                           const uint32_t* hgap, uint32_t fault_doc, cld_result* spec_out, uint32_t* spec_take,
                           int ctr_total, int ctr_deq, hipEvent_t mid, hipStream_t s);
// spec_out / spec_take (nullable: no speculation): cld_long_spec_docs(n_slots)
// results and u32 entries, k_long's speculative pass-2 results for the
// longest documents of a small batch.
size_t cld_long_spec_docs(int n_slots);
// Staged long-document path (cld_long.hip, "staged long-document path"):
// k_lspan over `list` (counters[kCtrRequeue] documents) stores pass 1's spans
// in `pool` (meta[k]: the region of list entry k) and lists the entries it
// took (ok_list) and the documents it did not (fall_list, for the fused
// k_long: cld_launch_long with kCtrStFall / kCtrStDqFall); k_lscore scores
// pass 1 (to p2_list when not good enough), k_lrep runs Repeats over those,
// k_lscore<pass 2> finishes them.  small_total: a list this short goes whole
// to the fused kernel, in order (its speculation is for small batches), and
// so does a list holding a document of heavy_kb KB or more (hist: k_len_hist's
// length buckets; nullable; heavy_kb 0: no such rule).
// n_waves: resident waves the staged kernels may use (slots).
int cld_staged_waves_per_simd();
// par_lists (span-parallel documents): two u32 document lists of n entries
// each (passes 1, 2), then two u64 group lists of gcap entries each.
hipError_t cld_launch_staged(const DevTables* d_T, const uint8_t* buf, const uint64_t* offs, const uint32_t* list,
                             cld_result* out, uint8_t* slots, int n_waves, uint8_t* pool, uint64_t pool_bytes,
                             uint64_t* meta, uint32_t* ok_list, uint32_t* p2_list, uint32_t* fall_list,
                             uint32_t* counters, uint32_t cflags, const uint8_t* special,
                             const uint32_t* priors, const uint8_t* hbuf, const uint8_t* hflag, const uint32_t* hpos,
                             const uint32_t* hgap, uint32_t fault_doc, uint32_t small_total, const uint32_t* hist,
                             uint32_t heavy_kb, uint32_t* par_lists, size_t n, size_t gcap, hipStream_t s);
}
#endif
