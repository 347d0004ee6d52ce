/*
 * cld_oracle.c -- TEST INFRASTRUCTURE ONLY.  Never linked into the product.
 *
 * A plain-C, single-threaded-per-call restatement of the CLD2 plain-text
 * DetectLanguage path the reference service calls (wrapper.cc:7-16 ->
 * compact_lang_det.cc:59-95 -> compact_lang_det_impl.cc:1707-2106).  It is the
 * parity CHECKER for the HIP path (tests/, __graft_entry__.smoke()) and the
 * CPU baseline leg of bench.py.  Each function cites the reference lines it
 * restates.  It reads every table from the same CLDT blob the GPU path loads,
 * so "same tables in -> same bytes out" is what parity means.
 *
 * Pinning: the reference itself cannot be built here --
 * its production quadgram table cld2_generated_quadchrome_2.cc is a missing
 * blob and the task rules forbid building it against a stand-in.  This
 * restatement is therefore pinned by the reference's own artefacts:
 *   - cld2/docs/CLD2UnitTestOutput.html DocTote dumps + summaries for every
 *     script-only and CJK unit-test document (exact, real tables),
 *   - cld2/docs/CLD2UnitTestOutputVerbose.html hit / linear / chunk-summary
 *     dumps (stage-level pins for the quadgram documents),
 *   - main_test.go known-answer strings whose path does not need quadgrams.
 * Quadgram-scored scripts with the real table are "parity unpinned" here.
 *
 * Invalid UTF-8 is outside the reference contract (wrapper.cc passes
 * unchecked bytes; the reference then reads uninitialised heap).  Here every
 * out-of-range table read returns 0 and bytes past the document read as NUL,
 * exactly as the HIP path does, so the two agree on any input.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cld_oracle.h"
#include "../language-detector_amd/csrc/cldt_format.h"

/* ------------------------------------------------------------ constants */
/* utf8statetable.h:46-63 */
enum {
  kExitDstSpaceFull = 239, kExitIllegalStructure, kExitOK, kExitReject,
  kExitReplace1, kExitReplace2, kExitReplace3, kExitReplace21, kExitReplace31,
  kExitReplace32, kExitReplaceOffset1, kExitReplaceOffset2, kExitReplace1S0,
  kExitSpecial, kExitDoAgain, kExitRejectAlt, kExitNone
};

/* getonescriptspan.h:29-33 */
#define kMaxScriptBuffer 40960
#define kMaxScriptLowerBuffer ((kMaxScriptBuffer * 3) / 2)
#define kMaxScriptBytes (kMaxScriptBuffer - 32)
#define kWithinScriptTail 32
/* scoreonescriptspan.h:89-93 */
#define kMaxBoosts 4
#define kChunksizeQuads 20
#define kChunksizeUnis 50
#define kMaxScoringHits 1000
#define kMaxSummaries (kMaxScoringHits / kChunksizeQuads)
/* compact_lang_det_impl.cc:203-239 */
#define kCheapSqueezeTestThresh 4096
#define kCheapSqueezeTestLen 256
#define kSpacesTriggerPercent 25
#define kPredictTriggerPercent 67
#define kChunksizeDefault 48
#define kSpacesThreshPercent 25
#define kPredictThreshPercent 40
#define kMaxSpaceScan 32
#define kGoodLang1Percent 70
#define kGoodLang1and2Percent 93
#define kShortTextThresh 256
#define kPredictionTableSize 4096
#define kNonEnBoilerplateMinPercent 17
#define kNonFIGSBoilerplateMinPercent 20
#define kGoodFirstMinPercent 26
#define kGoodFirstReliableMinPercent 51
#define kIgnoreMaxPercent 20
#define kKeepMinPercent 2
#define kMinReliableKeepPercent 41   /* :981 */
#define kUnreliablePercentThreshold 75   /* scoreonescriptspan.cc:33 */
#define kGoodSecondT1T2MinBytes 15   /* :1405 */
/* compact_lang_det_impl.h:31-38 */
#define kCLDFlagFinish 1
#define kCLDFlagSqueeze 2
#define kCLDFlagRepeats 4
#define kCLDFlagTop40 8
#define kCLDFlagShort 16
#define kCLDFlagUseWords 64
/* compact_lang_det.h:343, :349 (the public result-affecting flags) */
#define kCLDFlagScoreAsQuads 0x0100
#define kCLDFlagBestEffort 0x4000
/* cldutil.cc:43-44 */
#define kMinGramCount 3
#define kMaxGramCount 16
#define kUnusedKey 0xFFFF

enum { UNIHIT = 0, QUADHIT = 1, DELTAHIT = 2, DISTINCTHIT = 3 };
enum { RTypeNone = 0, RTypeOne = 1, RTypeMany = 2, RTypeCJK = 3 };

/* --------------------------------------------------------------- tables */
typedef struct {
  uint32_t state0, state0_size, total_size, shift, n_remap, n_rstr;
  const uint8_t* t8; const uint16_t* t16;
  const uint8_t* remap; const uint8_t* rstr;
} sm_t;

typedef struct {
  uint32_t size_one, size, key_mask, n_ind, n_buckets;
  const uint32_t* b; const uint32_t* ind;
} tbl_t;

static struct {
  uint8_t* blob; size_t blob_size; int loaded;
  cldt_meta meta;
  sm_t script, lower, scan, uni;
  tbl_t compat, deltabi, distinctbi, quad, quad2, deltaocta, distinctocta;
  const int16_t* expected; uint32_t n_expected;
  const uint8_t* lgprob;
  const uint8_t* l2p; uint32_t l2p_size;
  const uint16_t* p2l_latn; const uint16_t* p2l_othr;
  const uint8_t* rtype; const uint16_t* deflang; uint32_t n_scripts, n_langs;
  const uint16_t* closest; uint32_t n_closest;
  const uint8_t* close_set;
  const uint8_t* codes; /* string section */
  const uint8_t* names;
  const uint8_t* script_codes;
  /* HTML mode (optional sections) */
  const uint8_t* ent_names; const int32_t* ent_values; uint32_t n_ent;
  const uint32_t* cp1252;
} T;

static const uint8_t* find_section(uint32_t id, uint64_t* size) {
  const cldt_file_header* fh = (const cldt_file_header*)T.blob;
  const cldt_section* s = (const cldt_section*)(T.blob + fh->section_table_offset);
  for (uint32_t i = 0; i < fh->n_sections; ++i)
    if (s[i].id == id) { if (size) *size = s[i].size; return T.blob + s[i].offset; }
  return NULL;
}

static int load_sm(uint32_t id, sm_t* sm) {
  uint64_t size;
  const uint8_t* p = find_section(id, &size);
  if (!p) return -1;
  const cldt_sm_header* h = (const cldt_sm_header*)p;
  sm->state0 = h->state0; sm->state0_size = h->state0_size;
  sm->total_size = h->total_size; sm->shift = h->entry_shift;
  const uint8_t* q = p + sizeof(*h);
  if (h->bytes_per_entry == 2) { sm->t16 = (const uint16_t*)q; sm->t8 = NULL; return 0; }
  sm->t8 = q; sm->t16 = NULL;
  size_t off = sizeof(*h) + h->total_size;
  off = (off + 15) & ~(size_t)15;
  sm->remap = p + off; sm->n_remap = h->n_remap;
  sm->rstr = p + off + 4 * (size_t)h->n_remap; sm->n_rstr = h->n_remap_string;
  return 0;
}

static int load_tbl(uint32_t id, tbl_t* t) {
  const uint8_t* p = find_section(id, NULL);
  if (!p) return -1;
  const cldt_table_header* h = (const cldt_table_header*)p;
  t->size_one = h->size_one; t->size = h->size; t->key_mask = h->key_mask;
  t->n_ind = h->n_ind; t->n_buckets = h->n_buckets_stored;
  t->b = (const uint32_t*)(p + sizeof(*h));
  t->ind = t->b + 4 * (size_t)h->n_buckets_stored;
  return 0;
}

int cldo_load(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return -1;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  free(T.blob); memset(&T, 0, sizeof(T));
  T.blob = (uint8_t*)malloc((size_t)n);
  if (fread(T.blob, 1, (size_t)n, f) != (size_t)n) { fclose(f); return -2; }
  fclose(f);
  T.blob_size = (size_t)n;
  const cldt_file_header* fh = (const cldt_file_header*)T.blob;
  if (fh->magic != CLDT_MAGIC || fh->version != CLDT_VERSION) return -3;
  uint64_t sz = 0;
  const uint8_t* p = find_section(CLDT_META, NULL);
  if (!p) return -4;
  memcpy(&T.meta, p, sizeof(T.meta));
  if (load_sm(CLDT_SCRIPT_PROP, &T.script) || load_sm(CLDT_LOWER_REPL, &T.lower) ||
      load_sm(CLDT_SCAN_NOT, &T.scan) || load_sm(CLDT_CJK_UNI_PROP, &T.uni)) return -5;
  if (load_tbl(CLDT_CJK_COMPAT, &T.compat) || load_tbl(CLDT_DELTA_BI, &T.deltabi) ||
      load_tbl(CLDT_DISTINCT_BI, &T.distinctbi) || load_tbl(CLDT_QUAD, &T.quad) ||
      load_tbl(CLDT_QUAD2, &T.quad2) || load_tbl(CLDT_DELTA_OCTA, &T.deltaocta) ||
      load_tbl(CLDT_DISTINCT_OCTA, &T.distinctocta)) return -6;
  T.expected = (const int16_t*)find_section(CLDT_EXPECTED_SCORE, &sz); T.n_expected = (uint32_t)(sz / 2);
  T.lgprob = find_section(CLDT_LGPROB, NULL);
  T.l2p = find_section(CLDT_LANG_TO_PLANG, &sz); T.l2p_size = (uint32_t)sz;
  T.p2l_latn = (const uint16_t*)find_section(CLDT_PLANG_TO_LANG_LATN, NULL);
  T.p2l_othr = (const uint16_t*)find_section(CLDT_PLANG_TO_LANG_OTHR, NULL);
  T.rtype = find_section(CLDT_ULSCRIPT_RTYPE, &sz); T.n_scripts = (uint32_t)sz;
  T.deflang = (const uint16_t*)find_section(CLDT_ULSCRIPT_DEFAULT_LANG, NULL);
  T.closest = (const uint16_t*)find_section(CLDT_CLOSEST_ALT, &sz); T.n_closest = (uint32_t)(sz / 2);
  T.close_set = find_section(CLDT_CLOSE_SET, &sz); T.n_langs = (uint32_t)sz;
  T.codes = find_section(CLDT_LANG_CODES, NULL);
  T.names = find_section(CLDT_LANG_NAMES, NULL);
  T.script_codes = find_section(CLDT_ULSCRIPT_CODES, NULL);
  T.ent_names = find_section(CLDT_ENTITY_NAMES, NULL);
  T.ent_values = (const int32_t*)find_section(CLDT_ENTITY_VALUES, &sz); T.n_ent = (uint32_t)(sz / 4);
  T.cp1252 = (const uint32_t*)find_section(CLDT_CP1252_FIX, NULL);
  if (!T.expected || !T.lgprob || !T.l2p || !T.p2l_latn || !T.p2l_othr || !T.rtype ||
      !T.deflang || !T.closest || !T.close_set || !T.codes) return -7;
  T.loaded = 1;
  return 0;
}

static const char* str_at(const uint8_t* sec, uint32_t i) {
  uint32_t n = *(const uint32_t*)sec;
  if (i >= n) return "";
  const uint32_t* offs = (const uint32_t*)(sec + 4);
  return (const char*)(sec + 4 + 4 * (n + 1) + offs[i]);
}

/* LanguageCode (lang_script.cc:212-217): out-of-range -> UNKNOWN_LANGUAGE */
const char* cldo_language_code(int lang) {
  if (lang < 0 || (uint32_t)lang >= T.meta.num_languages) lang = (int)T.meta.unknown_language;
  return str_at(T.codes, (uint32_t)lang);
}
const char* cldo_language_name(int lang) {
  if (lang < 0 || (uint32_t)lang >= T.meta.num_languages) lang = (int)T.meta.unknown_language;
  return str_at(T.names, (uint32_t)lang);
}
static const char* script_code(int s) {
  if (s < 0 || (uint32_t)s >= T.n_scripts) s = 0;
  return str_at(T.script_codes, (uint32_t)s);
}

/* ------------------------------------------------------ lang/script maps */
/* lang_script.cc:154-160 */
static int rtype_of(int ulscript) {
  if (ulscript < 0 || (uint32_t)ulscript >= T.n_scripts) ulscript = 0;
  return T.rtype[ulscript];
}
/* lang_script.cc:314-318 */
static int default_language(int ulscript) {
  if (ulscript < 0 || (uint32_t)ulscript >= T.n_scripts) return (int)T.meta.unknown_language;
  return T.deflang[ulscript];
}
/* lang_script.cc:320-326 */
static uint8_t per_script_number(int ulscript, int lang) {
  if (ulscript < 0 || (uint32_t)ulscript >= T.n_scripts) return 0;
  if (T.rtype[ulscript] == RTypeNone) return 1;
  if (lang < 0 || (uint32_t)lang >= T.l2p_size) return 0;
  return T.l2p[lang];
}
/* lang_script.cc:328-341 */
static int from_per_script_number(int ulscript, uint8_t ps) {
  if (ulscript < 0 || (uint32_t)ulscript >= T.n_scripts) return (int)T.meta.unknown_language;
  if (T.rtype[ulscript] == RTypeNone || T.rtype[ulscript] == RTypeOne) return T.deflang[ulscript];
  if ((uint32_t)ulscript == T.meta.ulscript_latin) return T.p2l_latn[ps];
  return T.p2l_othr[ps];
}
/* lang_script.cc:261-310 (stored per language by the table extractor) */
static int close_set(int lang) {
  if (lang < 0 || (uint32_t)lang >= T.n_langs) return 0;
  return T.close_set[lang];
}
/* lang_script.cc:552-557 */
static int lscript4(int ulscript) {
  if ((uint32_t)ulscript == T.meta.ulscript_latin) return 0;
  if ((uint32_t)ulscript == T.meta.ulscript_cyrillic) return 1;
  if ((uint32_t)ulscript == T.meta.ulscript_arabic) return 2;
  return 3;
}

/* ------------------------------------------------------------ offset map */
/* OffsetMap (offsetmap.cc:43-453): a list of copy / insert / delete ranges
 * from A (the original text) to A' (the text built from it), coded one byte
 * per range as the reference codes it (2-bit op, 6-bit length, prefix bytes
 * for longer lengths; adjacent copies merged by Flush).  Only built in
 * ResultChunkVector mode, where MapBack takes chunk offsets in the lowered
 * span text back to document offsets. */
enum { OM_PREFIX = 0, OM_COPY = 1, OM_INSERT = 2, OM_DELETE = 3 };
typedef struct {
  uint8_t* d; int n, cap;             /* diffs_ */
  int pend_op, pend_len;              /* pending_op_, pending_length_ */
  int max_a, max_ap;                  /* max_aoffset_, max_aprimeoffset_ */
} offmap_t;
static void om_push(offmap_t* m, int op, int len) {          /* Emit :203-206 */
  if (m->n == m->cap) { m->cap = m->cap ? 2 * m->cap : 256; m->d = (uint8_t*)realloc(m->d, (size_t)m->cap); }
  m->d[m->n++] = (uint8_t)((op << 6) | (len & 0x3F));
}
static void om_clear(offmap_t* m) {                          /* Clear :43-55 */
  m->n = 0; m->pend_op = OM_COPY; m->pend_len = 0; m->max_a = 0; m->max_ap = 0;
}
static void om_flush(offmap_t* m) {                          /* Flush :158-187 */
  if (m->pend_len == 0) return;
  if (m->pend_op == OM_COPY && m->n > 0) {
    uint8_t c = m->d[m->n - 1];
    if ((c >> 6) == OM_COPY && (c & 0x3F) + m->pend_len <= 0x3F) {
      m->d[m->n - 1] = (uint8_t)(c + m->pend_len);
      m->pend_len = 0;
      return;
    }
  }
  if (m->pend_len > 0x3F) {
    int nz = 0;
    for (int shift = 30; shift > 0; shift -= 6) {
      int prefix = (m->pend_len >> shift) & 0x3F;
      if (prefix > 0 || nz) { om_push(m, OM_PREFIX, prefix); nz = 1; }
    }
  }
  om_push(m, m->pend_op, m->pend_len & 0x3F);
  m->pend_len = 0;
}
static void om_copy(offmap_t* m, int bytes) {                /* Copy :107-118 */
  if (bytes == 0) return;
  m->max_a += bytes; m->max_ap += bytes;
  if (m->pend_op == OM_COPY) m->pend_len += bytes;
  else { om_flush(m); m->pend_op = OM_COPY; m->pend_len = bytes; }
}
static void om_insert(offmap_t* m, int bytes) {              /* Insert :122-138 */
  if (bytes == 0) return;
  m->max_ap += bytes;
  if (m->pend_op == OM_INSERT) m->pend_len += bytes;
  else if (bytes == 1 && m->pend_op == OM_DELETE && m->pend_len == 1) m->pend_op = OM_COPY;
  else { om_flush(m); m->pend_op = OM_INSERT; m->pend_len = bytes; }
}
static void om_delete(offmap_t* m, int bytes) {              /* Delete :141-156 */
  if (bytes == 0) return;
  m->max_a += bytes;
  if (m->pend_op == OM_DELETE) m->pend_len += bytes;
  else if (bytes == 1 && m->pend_op == OM_INSERT && m->pend_len == 1) m->pend_op = OM_COPY;
  else { om_flush(m); m->pend_op = OM_DELETE; m->pend_len = bytes; }
}
static void om_maybe_flush_all(offmap_t* m) {                /* MaybeFlushAll / FlushAll :190-200 */
  if (0 < m->pend_len || m->n == 0) { om_copy(m, 1); om_flush(m); }
}
static void om_reset(offmap_t* m) { om_maybe_flush_all(m); }  /* Reset :94-104 (window state is implicit) */
/* MapBack :428-452.  The reference walks a window left/right; the range it
 * settles on is the one of non-zero A' width holding aprime, so a scan from
 * the left gives the same answer. */
static int om_map_back(offmap_t* m, int ap) {
  om_maybe_flush_all(m);
  if (ap < 0) return 0;
  if (m->max_ap <= ap) return (ap - m->max_ap) + m->max_a;
  int lo_a = 0, lo_ap = 0, i = 0;
  while (i < m->n) {
    int op = OM_PREFIX, len = 0;
    while (i < m->n && op == OM_PREFIX) {                    /* ParseNext :316-330 */
      uint8_t c = m->d[i++];
      op = c >> 6;
      len = (len << 6) + (c & 0x3F);
    }
    if (op == OM_PREFIX) break;
    int hi_a = lo_a + (op == OM_INSERT ? 0 : len), hi_ap = lo_ap + (op == OM_DELETE ? 0 : len);
    if (ap < hi_ap) {
      int a = ap - (lo_ap - lo_a);
      return a >= hi_a ? hi_a : a;
    }
    lo_a = hi_a; lo_ap = hi_ap;
  }
  return (ap - m->max_ap) + m->max_a;     /* SetRight (not reached for well-formed maps) */
}

/* ResultChunk (compact_lang_det.h:147-153) and its vector */
typedef struct { int32_t offset, bytes; uint16_t lang1, pad; } rchunk_t;
typedef struct { rchunk_t* v; int n, cap; } rvec_t;
static void rvec_push(rvec_t* r, rchunk_t c) {
  if (r->n == r->cap) { r->cap = r->cap ? 2 * r->cap : 64; r->v = (rchunk_t*)realloc(r->v, sizeof(rchunk_t) * (size_t)r->cap); }
  r->v[r->n++] = c;
}

/* --------------------------------------------------- UTF-8 state machines */
static int utf8_len(uint8_t c) {            /* kUTF8LenTbl, utf8statetable.h:266-277 */
  return c < 0xC0 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4;
}
static uint32_t t16(const sm_t* sm, int64_t i) {
  return (i < 0 || i >= (int64_t)sm->total_size) ? 0 : sm->t16[i];
}
static int32_t t8(const sm_t* sm, int64_t i) {
  return (i < 0 || i >= (int64_t)sm->total_size) ? 0 : sm->t8[i];
}

/* GetUTF8LetterScriptNum -> UTF8GenericPropertyTwoByte
 * getonescriptspan.cc:1083-1088, utf8statetable.cc:362-411 */
static int script_num(const uint8_t* s) {
  int srclen = utf8_len(s[0]);
  const sm_t* sm = &T.script;
  int64_t b = sm->state0;
  uint8_t c = s[0];
  uint32_t e;
  if (c < 0x80) return (int)t16(sm, b + c);
  if ((c & 0xE0) == 0xC0 && srclen >= 2) {
    e = t16(sm, b + c); e = t16(sm, b + ((int64_t)e << sm->shift) + s[1]);
  } else if ((c & 0xF0) == 0xE0 && srclen >= 3) {
    e = t16(sm, b + c); e = t16(sm, b + ((int64_t)e << sm->shift) + s[1]);
    e = t16(sm, b + ((int64_t)e << sm->shift) + s[2]);
  } else if ((c & 0xF8) == 0xF0 && srclen >= 4) {
    e = t16(sm, b + c); e = t16(sm, b + ((int64_t)e << sm->shift) + s[1]);
    e = t16(sm, b + ((int64_t)e << sm->shift) + s[2]);
    e = t16(sm, b + ((int64_t)e << sm->shift) + s[3]);
  } else {
    e = 0;
  }
  return (int)(uint8_t)e;   /* the API returns uint8 (utf8statetable.h:186) */
}

/* UTF8GenericPropertyBigOneByte on the CJK unigram machine, with srclen =
 * kAdvanceOneChar[lead] as GetUniHits passes it (cldutil.cc:221-226,
 * utf8statetable.cc:271-320). */
static int uni_prop(const uint8_t* s, int srclen) {
  const sm_t* sm = &T.uni;
  int64_t b0 = sm->state0;
  uint8_t c = s[0];
  int32_t e;
  int sh = (int)sm->shift;
  if (c < 0x80) return t8(sm, b0 + c);
  if ((c & 0xE0) == 0xC0 && srclen >= 2) {
    e = t8(sm, b0 + c); e = t8(sm, b0 + ((int64_t)e << sh) + s[1]);
  } else if ((c & 0xF0) == 0xE0 && srclen >= 3) {
    e = t8(sm, b0 + c);
    int64_t tb = b0 + ((int64_t)e << (sh + 4));
    e = (int8_t)t8(sm, tb + s[1]);
    tb = tb + ((int64_t)e << sh);
    e = t8(sm, tb + s[2]);
  } else if ((c & 0xF8) == 0xF0 && srclen >= 4) {
    e = t8(sm, b0 + c); e = t8(sm, b0 + ((int64_t)e << sh) + s[1]);
    int64_t tb = b0 + ((int64_t)e << (sh + 4));
    e = (int8_t)t8(sm, tb + s[2]);
    tb = tb + ((int64_t)e << sh);
    e = t8(sm, tb + s[3]);
  } else {
    e = 0;
  }
  return (uint8_t)e;
}

static int in_state_zero(const sm_t* sm, int64_t tbl) {
  return (uint64_t)(tbl - sm->state0) < sm->state0_size;
}

/* ScanToLetterOrSpecial -> UTF8GenericScan(utf8scannot_lettermarkspecial)
 * getonescriptspan.cc:480-485, utf8statetable.cc:460-554.  The 8-byte fast
 * loop is omitted: the extractor proved it only skips bytes whose state0
 * entry is 0 (stay in state 0, no exit), so the byte loop is equivalent. */
static int scan_to_letter_or_special(const uint8_t* isrc, int len) {
  if (len <= 0) return 0;
  const sm_t* sm = &T.scan;
  const uint8_t* src = isrc;
  const uint8_t* lim = isrc + len;
  int64_t tb0 = sm->state0;
  int e = 0;
  for (;;) {
    int64_t tb = tb0;
    e = 0;
    while (src < lim) {
      uint8_t c = *src;
      e = t8(sm, tb + c);
      src++;
      if (e >= kExitIllegalStructure) break;
      tb = tb0 + ((int64_t)e << sm->shift);
    }
    if (e >= kExitIllegalStructure) {
      src--;
      if (!in_state_zero(sm, tb)) {
        do { src--; } while (src > isrc && (src[0] & 0xC0) == 0x80);
      }
    } else if (!in_state_zero(sm, tb)) {
      e = kExitIllegalStructure;
      do { src--; } while (src > isrc && (src[0] & 0xC0) == 0x80);
    } else {
      e = kExitOK;
    }
    if (e != kExitDoAgain) break;
  }
  return (int)(src - isrc);
}

/* UTF8GenericReplace(utf8repl_lettermarklower), utf8statetable.cc:608-867
 * and the kExitDoAgain driver loop :1138-1169, with the offset map
 * (map2uplow_) when om != NULL.  Returns bytes filled. */
static int lower_replace(const uint8_t* isrc, int ilen, uint8_t* odst, int olen, int plain, offmap_t* om) {
  const sm_t* sm = &T.lower;
  int total_filled = 0;
  const uint8_t* in = isrc; int inlen = ilen;
  uint8_t* out = odst; int outlen = olen;
  for (;;) {
    int sh = (int)sm->shift;
    int nEntries = 1 << sh;
    const uint8_t* src = in;
    const uint8_t* copystart = in;
    const uint8_t* srclimit = in + inlen;
    uint8_t* dst = out;
    uint8_t* dstlimit = out + outlen;
    int e = 0;
    if ((dstlimit - dst) < (srclimit - src)) { e = kExitDstSpaceFull; goto done_nobackup; }
    {
      int64_t tb0 = sm->state0;
      int64_t tb = tb0;
      uint8_t c = 0;
    do_state_table:
      tb = tb0;
      e = 0;       /* utf8statetable.cc:645-649 re-declares e = 0 here */
      c = 0;
    do_state_table_newe:
      while (src < srclimit) {
        c = *src;
        e = t8(sm, tb + c);
        *dst = c;
        src++; dst++;
        if (e >= kExitIllegalStructure) break;
        tb = tb0 + ((int64_t)e << sh);
      }
      if (e >= kExitIllegalStructure) {
        int offset = 0;
        switch (e) {
          case kExitReplace31:
            dst -= 2;
            if (om) { om_copy(om, (int)(src - copystart) - 2); om_delete(om, 2); copystart = src; }
            dst[-1] = (uint8_t)t8(sm, tb + c + nEntries * 1); goto do_state_table;
          case kExitReplace32:
            dst--;
            if (om) { om_copy(om, (int)(src - copystart) - 1); om_delete(om, 1); copystart = src; }
            dst[-2] = (uint8_t)t8(sm, tb + c + nEntries * 2);
            dst[-1] = (uint8_t)t8(sm, tb + c + nEntries * 1); goto do_state_table;
          case kExitReplace21:
            dst--;
            if (om) { om_copy(om, (int)(src - copystart) - 1); om_delete(om, 1); copystart = src; }
            dst[-1] = (uint8_t)t8(sm, tb + c + nEntries * 1); goto do_state_table;
          case kExitReplace3:
            dst[-3] = (uint8_t)t8(sm, tb + c + nEntries * 3);
            /* fallthrough */
          case kExitReplace2:
            dst[-2] = (uint8_t)t8(sm, tb + c + nEntries * 2);
            /* fallthrough */
          case kExitReplace1:
            dst[-1] = (uint8_t)t8(sm, tb + c + nEntries * 1); goto do_state_table;
          case kExitReplace1S0:
            dst[-1] = (uint8_t)t8(sm, tb + c + 256 * 1); goto do_state_table;
          case kExitReplaceOffset2:
            if (nEntries != 256 && in_state_zero(sm, tb)) offset += (uint8_t)t8(sm, tb + c + 256 * 2) << 8;
            else offset += (uint8_t)t8(sm, tb + c + nEntries * 2) << 8;
            /* fallthrough */
          case kExitSpecial:
          case kExitReplaceOffset1: {
            if (nEntries != 256 && in_state_zero(sm, tb)) offset += (uint8_t)t8(sm, tb + c + 256 * 1);
            else offset += (uint8_t)t8(sm, tb + c + nEntries * 1);
            if ((uint32_t)offset >= sm->n_remap) { e = kExitIllegalStructure; break; }
            const uint8_t* re = sm->remap + 4 * (size_t)offset;
            int del_len = re[0] & ~0x80;
            int add_len = re[1] & ~0x80;
            /* kHtmlPlaintextFlag pair: plain text uses this entry, HTML the next (:755-762) */
            if ((re[1] & 0x80) && !plain && (uint32_t)offset + 1 < sm->n_remap) {
              re += 4;
              add_len = re[1] & ~0x80;
            }
            int string_offset = re[2] | (re[3] << 8);
            uint8_t* newdst = dst - del_len + add_len;
            if ((dstlimit - newdst) < (srclimit - src)) { e = kExitDstSpaceFull; break; }
            dst -= del_len;
            for (int k = 0; k < add_len; ++k)
              dst[k] = ((uint32_t)(string_offset + k) < sm->n_rstr) ? sm->rstr[string_offset + k] : 0;
            dst += add_len;
            if (om) {
              if (add_len > del_len) {
                om_copy(om, (int)(src - copystart)); om_insert(om, add_len - del_len); copystart = src;
              } else if (add_len < del_len) {
                om_copy(om, (int)(src - copystart) + add_len - del_len); om_delete(om, del_len - add_len);
                copystart = src;
              }
            }
            if (re[0] & 0x80) {
              int ne = ((uint32_t)(string_offset + add_len) < sm->n_rstr) ? sm->rstr[string_offset + add_len] : 0;
              tb = tb0 + ((int64_t)ne << sh);
              goto do_state_table_newe;
            }
            if (e == kExitRejectAlt) break;
            if (e != kExitSpecial) goto do_state_table;
            goto do_state_table;   /* DoSpecialFixup is a no-op (:597-601) */
          }
          default:
            break;
        }
        src--; dst--;
        if (!in_state_zero(sm, tb)) {
          do { src--; dst--; } while (src > in && (src[0] & 0xC0) == 0x80);
        }
      } else if (!in_state_zero(sm, tb)) {
        e = kExitIllegalStructure;
        do { src--; dst--; } while (src > in && (src[0] & 0xC0) == 0x80);
      } else {
        e = kExitOK;
      }
    }
    if (om && src > copystart) { om_copy(om, (int)(src - copystart)); copystart = src; }
  done_nobackup:;
    int consumed = (int)(src - in), filled = (int)(dst - out);
    total_filled += filled;
    if (e != kExitDoAgain) break;
    in += consumed; inlen -= consumed; out += filled; outlen -= filled;
  }
  return total_filled;
}

/* ------------------------------------------------------------ HTML mode */
/* IsSpecial (getonescriptspan.cc:470-477): < > & */
static int is_special(uint8_t c) { return c == '<' || c == '>' || c == '&'; }

/* ScanToPossibleLetter (getonescriptspan.cc:150-203, 503-541): the cheap tag
 * parser, restated as a transition function over the reference's byte
 * classes.  It advances over <tag>, <!-- ... -->, <script ...> ... </script>
 * and <style ...> ... </style> (quotes inside tags respected, CR/LF ends a
 * quoted string); state 0 / 1 exit (1 = '<' seen inside a tag).  Pinned
 * against the reference's own function by tests/test_html_hints.py. */
enum { TC_LT, TC_GT, TC_EX, TC_HY, TC_QU, TC_AP, TC_SL, TC_S, TC_C, TC_R, TC_I, TC_P, TC_T, TC_Y, TC_L, TC_E,
       TC_CR, TC_NL, TC_PL };
static int tag_class(uint8_t c) {
  switch (c) {
    case '<': return TC_LT; case '>': return TC_GT; case '!': return TC_EX; case '-': return TC_HY;
    case '"': return TC_QU; case '\'': return TC_AP; case '/': return TC_SL; case '\n': case '\r': return TC_CR;
    case '&': case '@': case '`': return TC_PL;
    default: break;
  }
  if ((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z')) {
    switch (c | 0x20) {
      case 's': return TC_S; case 'c': return TC_C; case 'r': return TC_R; case 'i': return TC_I;
      case 'p': return TC_P; case 't': return TC_T; case 'y': return TC_Y; case 'l': return TC_L;
      case 'e': return TC_E; default: return TC_PL;
    }
  }
  return c >= 0xC0 ? TC_PL : TC_NL;
}
/* inside "<...": '<' is an error exit, '>' ends the tag, quotes open strings */
static int tag_common(int k, int other) {
  return k == TC_LT ? 1 : k == TC_GT ? 2 : k == TC_QU ? 10 : k == TC_AP ? 11 : other;
}
static int tag_next(int s, int k) {
#define TAG_COMMON(other) return tag_common(k, other)
  switch (s) {
    case 0: case 2: return k == TC_LT ? 3 : (k >= TC_S && k <= TC_E) || k == TC_PL ? 0 : 2;
    case 3: if (k == TC_EX) return 4; if (k == TC_S) return 13; if (k == TC_HY || k == TC_SL) return 9; TAG_COMMON(9);
    case 4: if (k == TC_HY) return 5; TAG_COMMON(9);
    case 5: if (k == TC_HY) return 6; TAG_COMMON(9);
    case 6: return k == TC_HY ? 7 : 6;
    case 7: return k == TC_HY ? 8 : 6;
    case 8: return k == TC_GT ? 2 : k == TC_HY ? 8 : 6;
    case 9: TAG_COMMON(9);
    case 10: return k == TC_QU ? 9 : k == TC_CR ? 12 : 10;
    case 11: return k == TC_AP ? 9 : k == TC_CR ? 12 : 11;
    case 12: return k == TC_LT ? 1 : k == TC_GT ? 2 : 12;
    case 13: if (k == TC_C) return 14; if (k == TC_T) return 28; TAG_COMMON(9);
    case 14: if (k == TC_R) return 15; TAG_COMMON(9);
    case 15: if (k == TC_I) return 16; TAG_COMMON(9);
    case 16: if (k == TC_P) return 17; TAG_COMMON(9);
    case 17: if (k == TC_T) return 18; TAG_COMMON(9);
    case 18: if (k == TC_GT || k == TC_CR || k == TC_NL) return 19; TAG_COMMON(9);
    case 19: return k == TC_LT ? 20 : 19;
    case 20: return k == TC_SL ? 21 : 19;
    case 21: return k == TC_S ? 22 : (k == TC_CR || k == TC_NL) ? 21 : 19;
    case 22: return k == TC_C ? 23 : 19;
    case 23: return k == TC_R ? 24 : 19;
    case 24: return k == TC_I ? 25 : 19;
    case 25: return k == TC_P ? 26 : 19;
    case 26: return k == TC_T ? 27 : 19;
    case 27: return k == TC_GT ? 2 : 19;
    case 28: if (k == TC_Y) return 29; TAG_COMMON(9);
    case 29: if (k == TC_L) return 30; TAG_COMMON(9);
    case 30: if (k == TC_E) return 31; TAG_COMMON(9);
    case 31: if (k == TC_GT || k == TC_CR || k == TC_NL) return 32; TAG_COMMON(9);
    case 32: return k == TC_LT ? 33 : 32;
    case 33: return k == TC_SL ? 34 : 32;
    case 34: return k == TC_S ? 35 : (k == TC_CR || k == TC_NL) ? 34 : 32;
    case 35: return k == TC_T ? 36 : 32;
    case 36: return k == TC_Y ? 37 : 32;
    case 37: return k == TC_L ? 38 : 32;
    case 38: return k == TC_E ? 39 : 32;
    case 39: return k == TC_GT ? 2 : 32;
    default: return 1;
  }
#undef TAG_COMMON
}
static int scan_to_possible_letter(const uint8_t* isrc, int len) {
  const uint8_t* src = isrc;
  const uint8_t* lim = isrc + len;
  int s = 0, e = 0;
  while (src < lim) {
    e = tag_next(s, tag_class(*src++));
    if (e <= 1) { --src; break; }      /* kMaxExitStateLettersMarksOnly: overshot by one byte */
    s = e;
  }
  if (src >= lim) return len;           /* fell off the end: pretend the last byte was '>' */
  if (e != 0 && e != 2) {               /* '<' inside a tag: just past the first, unmatched '<' */
    int off = (int)(src - isrc) - 1;
    while (0 < off && isrc[off] != '<') --off;
    return off + 1;
  }
  return (int)(src - isrc);
}

/* FixUnicodeValue (fixunicodevalue.cc) */
static int32_t fix_unicode_value(int32_t uv) {
  uint32_t u = (uint32_t)uv;
  if (u < 0x100) return T.cp1252 ? (int32_t)T.cp1252[u] : uv;
  if (u < 0xD800) return uv;
  if ((u & ~0x0Fu) == 0xFDD0 || (u & ~0x0Fu) == 0xFDE0 || (u & 0xFFFEu) == 0xFFFE) return 0xFFFD;
  if (0xE000 <= u && u <= 0x10FFFF) return uv;
  return 0xFFFD;
}
static int is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
static int is_xdigit(uint8_t c) { return is_digit(c) || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'); }
static int is_alnum(uint8_t c) { return is_digit(c) || ((c | 0x20) >= 'a' && (c | 0x20) <= 'z'); }
static int xdigit_val(uint8_t c) { return is_digit(c) ? c - '0' : (c | 0x20) - 'a' + 10; }
/* strto32_base10 / _base16 (getonescriptspan.cc:325-391), quirks kept: a
 * 9-digit decimal or an 8-digit hex >= 0x80000000 is U+FFFD */
static int32_t entity_number(const uint8_t* p, const uint8_t* lim, int hex, const uint8_t** endp) {
  *endp = p;
  while (p < lim && *p == '0') ++p;
  if (p == lim || !(hex ? is_xdigit(*p) : is_digit(*p))) return -1;
  const uint8_t* e = p;
  while (e < lim && (hex ? is_xdigit(*e) : is_digit(*e))) ++e;
  *endp = e;
  const int n = (int)(e - p);
  int fits = hex ? (n < 8 || (n == 8 && p[0] < '8')) : (n < 9 || (n == 10 && memcmp(p, "2147483647", 10) <= 0));
  if (!fits) return 0xFFFD;
  int32_t v = 0;
  for (; p < e; ++p) v = hex ? (int32_t)(((uint32_t)v << 4) + (uint32_t)xdigit_val(*p)) : v * 10 + (*p - '0');
  return fix_unicode_value(v);
}
/* LookupEntity (:292-300): binary search over the sorted entity names */
static int32_t lookup_entity(const uint8_t* name, int n) {
  if (n >= 16 || !T.ent_names) return -1;
  char key[16];
  memcpy(key, name, (size_t)n); key[n] = 0;
  int lo = 0, hi = (int)T.n_ent;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    int c = strcmp(str_at(T.ent_names, (uint32_t)mid), key);
    if (c < 0) lo = mid + 1; else if (c > 0) hi = mid; else return T.ent_values[mid];
  }
  return -1;
}
/* ReadEntity (:393-451): value, or -1 with *consumed = 1 */
static int32_t read_entity(const uint8_t* src, int srcn, int* consumed) {
  const uint8_t* end = src + srcn;
  if (srcn == 0 || *src != '&') { *consumed = 0; return -1; }
  *consumed = 1;
  const uint8_t* st = src + 1;
  const uint8_t* en;
  int32_t v;
  if (st < end && *st == '#') {
    if (st + 2 >= end) return -1;
    if (st[1] == 'x' || st[1] == 'X') v = entity_number(st + 2, end, 1, &en);
    else v = entity_number(st + 1, end, 0, &en);
    if (v == -1 || en > end) return -1;
  } else {
    for (en = st; en < end && is_alnum(*en); ++en) {}
    v = lookup_entity(st, (int)(en - st));
    if (v < 0) return -1;
    if (v >= 256 && !(en < end && *en == ';')) return -1;
  }
  if (en < end && *en == ';') ++en;
  *consumed = (int)(en - src);
  return v;
}
/* runetochar (:249-286) */
static int rune_to_utf8(uint8_t* s, uint32_t c) {
  if (c <= 0x7F) { s[0] = (uint8_t)c; return 1; }
  if (c <= 0x7FF) { s[0] = (uint8_t)(0xC0 | (c >> 6)); s[1] = (uint8_t)(0x80 | (c & 0x3F)); return 2; }
  if (c > 0x10FFFF) c = 0xFFFD;
  if (c <= 0xFFFF) {
    s[0] = (uint8_t)(0xE0 | (c >> 12)); s[1] = (uint8_t)(0x80 | ((c >> 6) & 0x3F)); s[2] = (uint8_t)(0x80 | (c & 0x3F));
    return 3;
  }
  s[0] = (uint8_t)(0xF0 | (c >> 18)); s[1] = (uint8_t)(0x80 | ((c >> 12) & 0x3F));
  s[2] = (uint8_t)(0x80 | ((c >> 6) & 0x3F)); s[3] = (uint8_t)(0x80 | (c & 0x3F));
  return 4;
}
/* EntityToBuffer (:454-468): take / put byte counts */
static void entity_to_buffer(const uint8_t* src, int len, uint8_t* dst, int* tlen, int* plen) {
  int32_t v = read_entity(src, len, tlen);
  if (v > 0) {
    *plen = rune_to_utf8(dst, (uint32_t)v);
  } else {
    *tlen = 1;
    *plen = 0;
  }
}

/* ------------------------------------------------------------- scanner */
typedef struct {
  const uint8_t* buf;       /* document, followed by >= 8 NUL bytes */
  int next, remaining;      /* next_byte_ - start_byte_, byte_length_ */
  uint8_t* sbuf;            /* script_buffer_       kMaxScriptBuffer + pad */
  uint8_t* lbuf;            /* script_buffer_lower_ kMaxScriptLowerBuffer + pad */
  int plain;                /* is_plain_text_ */
  offmap_t* map_orig;       /* map2original_ (ResultChunkVector mode only, else NULL) */
  offmap_t* map_low;        /* map2uplow_ */
} scanner_t;

typedef struct {
  uint8_t* text;
  int text_bytes, offset, ulscript;
} span_t;

/* ScriptScanner::SkipToFrontOfSpan, getonescriptspan.cc:592-642 */
static int skip_to_front_of_span(const uint8_t* src, int len, int* script, int plain) {
  int sc = 0, skip = 0, tlen = 0, plen = 0;
  while (skip < len) {
    skip += scan_to_letter_or_special(src + skip, len - skip);
    if (skip >= len) { *script = sc; return len; }
    if (!plain && is_special(src[skip])) {
      if (src[skip] == '<') {
        tlen = scan_to_possible_letter(src + skip, len - skip);
        sc = 0;
      } else if (src[skip] == '>') {
        tlen = 1;
        sc = 0;
      } else {                                  /* '&': expand, no advance */
        uint8_t tmp[8] = {0};
        entity_to_buffer(src + skip, len - skip, tmp, &tlen, &plen);
        if (plen > 0) sc = script_num(tmp);
      }
    } else {
      tlen = utf8_len(src[skip]);
      sc = script_num(src + skip);
    }
    if (sc != 0) break;
    skip += tlen;
  }
  *script = sc;
  return skip;
}

/* ScriptScanner::GetOneScriptSpan, getonescriptspan.cc:799-1027; HTML mode
 * (plain == 0) skips tags and decodes entities into the span. */
static int get_one_script_span(scanner_t* ss, span_t* span) {
  const int common = (int)T.meta.ulscript_common, inherited = (int)T.meta.ulscript_inherited;
  const int plain = ss->plain;
  offmap_t* mo = ss->map_orig;     /* map2original_ (:833-1023), ResultChunkVector mode only */
  span->text = ss->sbuf; span->text_bytes = 0; span->offset = ss->next; span->ulscript = 0;
  int put_soft_limit = kMaxScriptBytes - kWithinScriptTail;
  if (kMaxScriptBytes <= ss->remaining && ss->remaining < 2 * kMaxScriptBytes)
    put_soft_limit = ss->remaining / 2;
  int spanscript, sc = 0, tlen = 0, plen = 0;
  uint8_t* sb = ss->sbuf;
  sb[0] = ' '; sb[1] = 0;
  int take = 0, put = 1;
  if (mo) { om_clear(mo); om_delete(mo, span->offset); }
  int skip = skip_to_front_of_span(ss->buf + ss->next, ss->remaining, &spanscript, plain);
  ss->next += skip; ss->remaining -= skip;
  if (mo) {
    if (skip != 1) { om_delete(mo, skip); om_insert(mo, 1); }
    else om_copy(mo, 1);
  }
  if (ss->remaining <= 0) { if (mo) om_reset(mo); return 0; }
  span->ulscript = spanscript;
  const uint8_t* nb = ss->buf + ss->next;
  int bl = ss->remaining;
  while (take < bl) {
    int need_break = 0;
    while (take < bl) {
      if (!plain && is_special(nb[take])) {
        if (nb[take] == '<' || nb[take] == '>') { sc = 0; break; }
        entity_to_buffer(nb + take, bl - take, sb + put, &tlen, &plen);   /* '&': copy entity, no advance */
        if (plen > 0) sc = script_num(sb + put);
      } else {
        tlen = plen = utf8_len(nb[take]);
        if (take < bl - 3) memcpy(sb + put, nb + take, 4);
        else memcpy(sb + put, nb + take, (size_t)plen);
        sc = script_num(nb + take);
      }
      if (sc != spanscript && sc != inherited) {
        if (sc == common) {
          need_break = 1;
        } else {
          int sc2 = script_num(nb + take + tlen);
          if (sc2 != common && sc2 != spanscript) need_break = 1;
        }
      }
      if (need_break) break;
      take += tlen; put += plen;
      if (mo) {
        if (tlen == plen) om_copy(mo, tlen);
        else if (tlen < plen) { om_copy(mo, tlen); om_insert(mo, plen - tlen); }
        else { om_copy(mo, plen); om_delete(mo, tlen - plen); }
      }
      if (put >= kMaxScriptBytes) break;
    }
    while (take < bl) {
      tlen = scan_to_letter_or_special(nb + take, bl - take);
      take += tlen;
      if (mo) om_delete(mo, tlen);
      if (take >= bl) break;
      if (!plain && is_special(nb[take])) {
        if (nb[take] == '<') {
          tlen = scan_to_possible_letter(nb + take, bl - take);
          sc = 0;
        } else if (nb[take] == '>') {
          tlen = 1;
          sc = 0;
        } else {                                /* '&': expand, no advance */
          entity_to_buffer(nb + take, bl - take, sb + put, &tlen, &plen);
          if (plen > 0) sc = script_num(sb + put);
        }
      } else {
        tlen = utf8_len(nb[take]);
        sc = script_num(nb + take);
      }
      if (sc != 0) break;
      take += tlen;
      if (mo) om_delete(mo, tlen);
    }
    sb[put++] = ' ';
    if (mo) om_insert(mo, 1);
    if (sc != spanscript && sc != inherited) break;
    if (put >= put_soft_limit) break;
  }
  /* back up to a character boundary: the map is not adjusted (:998-1004) */
  while (0 < take && take < bl && (nb[take] & 0xC0) == 0x80) { --take; --put; }
  ss->next += take; ss->remaining -= take;
  sb[put + 0] = ' '; sb[put + 1] = ' '; sb[put + 2] = ' '; sb[put + 3] = 0;
  if (mo) { om_insert(mo, 4); om_reset(mo); }
  span->text_bytes = put;
  return 1;
}

/* ScriptScanner::LowerScriptSpan getonescriptspan.cc:1033-1054 */
static void lower_script_span(scanner_t* ss, span_t* span) {
  if (ss->map_low) om_clear(ss->map_low);
  int filled = lower_replace(span->text, span->text_bytes + 3, ss->lbuf, kMaxScriptLowerBuffer, ss->plain,
                             ss->map_low);
  ss->lbuf[filled] = 0;
  /* bytes past `filled` are never semantically read (masked hash loads,
   * NUL-stopped advances); keep them NUL so invalid input is deterministic */
  ss->lbuf[filled + 1] = 0; ss->lbuf[filled + 2] = 0; ss->lbuf[filled + 3] = 0;
  span->text = ss->lbuf;
  span->text_bytes = filled - 3;
  if (ss->map_low) om_reset(ss->map_low);
}

/* ----------------------------------------------------------- squeezing */
/* compact_lang_det_impl.cc:491-504 */
static int backscan_to_space(const uint8_t* src, int limit) {
  int n = 0;
  if (limit > kMaxSpaceScan) limit = kMaxSpaceScan;
  while (n < limit) { if (src[-n - 1] == ' ') return n; ++n; }
  n = 0;
  while (n < limit) { if ((src[-n] & 0xC0) != 0x80) return n; ++n; }
  return 0;
}
/* :509-522 */
static int forwardscan_to_space(const uint8_t* src, int limit) {
  int n = 0;
  if (limit > kMaxSpaceScan) limit = kMaxSpaceScan;
  while (n < limit) { if (src[n] == ' ') return n + 1; ++n; }
  n = 0;
  while (n < limit) { if ((src[n] & 0xC0) != 0x80) return n; ++n; }
  return 0;
}
/* :541-580 */
static int count_predicted_bytes(const uint8_t* src, int src_len, int* hash, int* tbl) {
  int p_count = 0;
  const uint8_t* lim = src + src_len;
  int h = *hash;
  while (src < lim) {
    int c = src[0], incr = 1;
    if (c < 0xC0) {
    } else if ((c & 0xE0) == 0xC0) { c = (c << 8) | src[1]; incr = 2; }
    else if ((c & 0xF0) == 0xE0) { c = (c << 16) | (src[1] << 8) | src[2]; incr = 3; }
    else { c = (int)(((uint32_t)c << 24) | ((uint32_t)src[1] << 16) | ((uint32_t)src[2] << 8) | src[3]); incr = 4; }
    src += incr;
    int p = tbl[h];
    tbl[h] = c;
    if (c == p) p_count += incr;
    h = ((h << 4) ^ c) & 0xFFF;
  }
  *hash = h;
  return p_count;
}
/* :586-595 */
static int count_spaces4(const uint8_t* src, int src_len) {
  int s = 0;
  for (int i = 0; i < (src_len & ~3); i += 4)
    s += (src[i] == ' ') + (src[i + 1] == ' ') + (src[i + 2] == ' ') + (src[i + 3] == ' ');
  return s;
}
/* :610-692 */
static int cheap_rep_words_inplace(uint8_t* isrc, int src_len, int* hash, int* tbl) {
  const uint8_t* src = isrc;
  const uint8_t* lim = isrc + src_len;
  uint8_t* dst = isrc;
  int h = *hash;
  uint8_t* word_dst = dst;
  int good = 0, wlen = 0;
  while (src < lim) {
    int c = src[0], incr = 1;
    *dst++ = (uint8_t)c;
    if (c == ' ') {
      if (good * 2 > wlen) dst = word_dst;
      word_dst = dst; good = 0; wlen = 0;
    }
    if (c < 0xC0) {
    } else if ((c & 0xE0) == 0xC0) { *dst++ = src[1]; c = (c << 8) | src[1]; incr = 2; }
    else if ((c & 0xF0) == 0xE0) { *dst++ = src[1]; *dst++ = src[2]; c = (c << 16) | (src[1] << 8) | src[2]; incr = 3; }
    else {
      *dst++ = src[1]; *dst++ = src[2]; *dst++ = src[3];
      c = (int)(((uint32_t)c << 24) | ((uint32_t)src[1] << 16) | ((uint32_t)src[2] << 8) | src[3]); incr = 4;
    }
    src += incr;
    wlen += incr;
    int p = tbl[h];
    tbl[h] = c;
    if (c == p) good += incr;
    h = ((h << 4) ^ c) & 0xFFF;
  }
  *hash = h;
  if ((dst - isrc) < (src_len - 3)) { dst[0] = ' '; dst[1] = ' '; dst[2] = ' '; dst[3] = 0; }
  else if ((dst - isrc) < src_len) { dst[0] = ' '; }
  return (int)(dst - isrc);
}
/* :785-865 */
static int cheap_squeeze_inplace(uint8_t* isrc, int src_len, int ichunksize, int* tbl) {
  uint8_t* src = isrc;
  uint8_t* dst = src;
  uint8_t* lim = src + src_len;
  int skipping = 0, hash = 0;
  memset(tbl, 0, kPredictionTableSize * sizeof(int));
  int chunksize = ichunksize ? ichunksize : kChunksizeDefault;
  int space_thresh = (chunksize * kSpacesThreshPercent) / 100;
  int predict_thresh = (chunksize * kPredictThreshPercent) / 100;
  while (src < lim) {
    int remaining = (int)(lim - src);
    int len = remaining < chunksize ? remaining : chunksize;
    while ((src[len] & 0xC0) == 0x80) ++len;
    int space_n = count_spaces4(src, len);
    int predb_n = count_predicted_bytes(src, len, &hash, tbl);
    if (space_n >= space_thresh || predb_n >= predict_thresh) {
      if (!skipping) {
        int n = backscan_to_space(dst, (int)(dst - isrc));
        dst -= n;
        if (dst == isrc) *dst++ = ' ';
        skipping = 1;
      }
    } else {
      if (skipping) {
        int n = forwardscan_to_space(src, len);
        src += n; remaining -= n; len -= n;
        skipping = 0;
      }
      if (len > 0) { memmove(dst, src, (size_t)len); dst += len; }
    }
    src += len;
  }
  if ((dst - isrc) < (src_len - 3)) { dst[0] = ' '; dst[1] = ' '; dst[2] = ' '; dst[3] = 0; }
  else if ((dst - isrc) < src_len) { dst[0] = ' '; }
  return (int)(dst - isrc);
}
/* CheapRepWordsInplaceOverwrite :697-765 (ResultChunkVector mode): well-
 * predicted words become '.' runs in place, the length is kept */
static int cheap_rep_words_inplace_overwrite(uint8_t* isrc, int src_len, int* hash, int* tbl) {
  const uint8_t* src = isrc;
  const uint8_t* lim = isrc + src_len;
  uint8_t* dst = isrc;
  int h = *hash;
  uint8_t* word_dst = dst;
  int good = 0, wlen = 0;
  while (src < lim) {
    int c = src[0], incr = 1;
    *dst++ = (uint8_t)c;
    if (c == ' ') {
      if (good * 2 > wlen)
        for (uint8_t* p = word_dst; p < dst - 1; ++p) *p = '.';
      word_dst = dst; good = 0; wlen = 0;
    }
    if (c < 0xC0) {
    } else if ((c & 0xE0) == 0xC0) { *dst++ = src[1]; c = (c << 8) | src[1]; incr = 2; }
    else if ((c & 0xF0) == 0xE0) { *dst++ = src[1]; *dst++ = src[2]; c = (c << 16) | (src[1] << 8) | src[2]; incr = 3; }
    else {
      *dst++ = src[1]; *dst++ = src[2]; *dst++ = src[3];
      c = (int)(((uint32_t)c << 24) | ((uint32_t)src[1] << 16) | ((uint32_t)src[2] << 8) | src[3]); incr = 4;
    }
    src += incr;
    wlen += incr;
    int p = tbl[h];
    tbl[h] = c;
    if (c == p) good += incr;
    h = ((h << 4) ^ c) & 0xFFF;
  }
  *hash = h;
  if ((dst - isrc) < (src_len - 3)) { dst[0] = ' '; dst[1] = ' '; dst[2] = ' '; dst[3] = 0; }
  else if ((dst - isrc) < src_len) { dst[0] = ' '; }
  return (int)(dst - isrc);
}
/* CheapSqueezeInplaceOverwrite :869-939 */
static int cheap_squeeze_inplace_overwrite(uint8_t* isrc, int src_len, int ichunksize, int* tbl) {
  uint8_t* src = isrc;
  uint8_t* dst = src;
  uint8_t* lim = src + src_len;
  int skipping = 0, hash = 0;
  memset(tbl, 0, kPredictionTableSize * sizeof(int));
  int chunksize = ichunksize ? ichunksize : kChunksizeDefault;
  int space_thresh = (chunksize * kSpacesThreshPercent) / 100;
  int predict_thresh = (chunksize * kPredictThreshPercent) / 100;
  ++src; ++dst;                                   /* always keep the leading space */
  while (src < lim) {
    int remaining = (int)(lim - src);
    int len = remaining < chunksize ? remaining : chunksize;
    while ((src[len] & 0xC0) == 0x80) ++len;
    int space_n = count_spaces4(src, len);
    int predb_n = count_predicted_bytes(src, len, &hash, tbl);
    if (space_n >= space_thresh || predb_n >= predict_thresh) {
      if (!skipping) {
        int n = backscan_to_space(dst, (int)(dst - isrc));
        for (uint8_t* p = dst - n; p < dst; ++p) *p = '.';
        skipping = 1;
      }
      for (uint8_t* p = dst; p < dst + len; ++p) *p = '.';
      dst[len - 1] = ' ';
    } else {
      if (skipping) {
        int n = forwardscan_to_space(src, len);
        for (uint8_t* p = dst; p < dst + n - 1; ++p) *p = '.';
        skipping = 0;
      }
    }
    dst += len;
    src += len;
  }
  if ((dst - isrc) < (src_len - 3)) { dst[0] = ' '; dst[1] = ' '; dst[2] = ' '; dst[3] = 0; }
  else if ((dst - isrc) < src_len) { dst[0] = ' '; }
  return (int)(dst - isrc);
}
/* :952-971 */
static int cheap_squeeze_trigger_test(const uint8_t* src, int src_len, int testsize, int* tbl) {
  if (src_len < testsize) return 0;
  int space_thresh = (testsize * kSpacesTriggerPercent) / 100;
  int predict_thresh = (testsize * kPredictTriggerPercent) / 100;
  int hash = 0;
  memset(tbl, 0, kPredictionTableSize * sizeof(int));
  if (count_spaces4(src, testsize) >= space_thresh) return 1;
  return count_predicted_bytes(src, testsize, &hash, tbl) >= predict_thresh;
}

/* --------------------------------------------------------------- totes */
typedef struct {            /* tote.h:33-61 */
  uint64_t in_use;
  int score_count;
  uint16_t score[256];
} tote_t;

static void tote_reinit(tote_t* t) { t->in_use = 0; t->score_count = 0; }
/* tote.cc:52-61 */
static void tote_add(tote_t* t, uint8_t key, int delta) {
  int g = key >> 2;
  uint64_t m = 1ULL << g;
  if (!(t->in_use & m)) { memset(&t->score[g * 4], 0, 8); t->in_use |= m; }
  t->score[key] = (uint16_t)(t->score[key] + delta);
}
/* tote.cc:65-101 */
static void tote_top3(const tote_t* t, int* key3) {
  key3[0] = key3[1] = key3[2] = -1;
  int s3[3] = {-1, -1, -1};
  uint64_t m = t->in_use;
  int base = 0;
  while (m) {
    if (m & 1) {
      for (int i = 0; i < 4; ++i) {
        int v = t->score[base + i];
        if (v > s3[2]) {
          int at = 2;
          if (v > s3[1]) {
            s3[2] = s3[1]; key3[2] = key3[1]; at = 1;
            if (v > s3[0]) { s3[1] = s3[0]; key3[1] = key3[0]; at = 0; }
          }
          s3[at] = v; key3[at] = base + i;
        }
      }
    }
    m >>= 1; base += 4;
  }
}
/* GetScore(-1) reads the uint16 before score_[] (tote.h:52-58): the high
 * half of the int score_count_ (in_use_mask_ at 0, byte_count_ at 8,
 * score_count_ at 12, the union at 16; little-endian), 0 for any count below
 * 65536.  A chunk whose tote stays empty gets there: ScoreAsQuads on text
 * whose spans score no langprob (malformed bytes, tests/test_gpu_corrupt.py);
 * the GPU takes 0 as well. */
static int tote_score(const tote_t* t, int key) {
  if (key < 0) return t->score_count >= 65536 ? (t->score_count >> 16) & 0xFFFF : 0;
  return t->score[key];
}

typedef struct {            /* tote.h:65-107 */
  int incr_count, sorted;
  uint16_t key[24];
  int value[24], score[24], rel[24];
} doctote_t;

static void doctote_init(doctote_t* d) {
  memset(d, 0, sizeof(*d));
  for (int i = 0; i < 24; ++i) d->key[i] = kUnusedKey;
}
/* tote.cc:127-175 */
static void doctote_add(doctote_t* d, uint16_t k, int bytes, int score, int rel) {
  ++d->incr_count;
  int s0 = k & 15, s1 = s0 ^ 8, s2 = (k & 7) + 16;
  int s = -1;
  if (d->key[s0] == k) s = s0;
  else if (d->key[s1] == k) s = s1;
  else if (d->key[s2] == k) s = s2;
  if (s >= 0) {
    d->value[s] += bytes; d->score[s] += score; d->rel[s] += rel * bytes;
    return;
  }
  int a;
  if (d->key[s0] == kUnusedKey) a = s0;
  else if (d->key[s1] == kUnusedKey) a = s1;
  else if (d->key[s2] == kUnusedKey) a = s2;
  else {
    a = s0;
    if (d->value[s1] < d->value[a]) a = s1;
    if (d->value[s2] < d->value[a]) a = s2;
  }
  d->key[a] = k; d->value[a] = bytes; d->score[a] = score; d->rel[a] = rel * bytes;
}
/* tote.cc:178-202 */
static int doctote_find(const doctote_t* d, uint16_t k) {
  if (d->sorted) {
    for (int s = 0; s < 24; ++s) if (d->key[s] == k) return s;
    return -1;
  }
  int s0 = k & 15;
  if (d->key[s0] == k) return s0;
  if (d->key[s0 ^ 8] == k) return s0 ^ 8;
  if (d->key[(k & 7) + 16] == k) return (k & 7) + 16;
  return -1;
}
/* tote.cc:221-250 */
static void doctote_sort(doctote_t* d, int n) {
  for (int s = 0; s < n; ++s) {
    if (d->key[s] == kUnusedKey) d->value[s] = -1;
    for (int s2 = s + 1; s2 < 24; ++s2) {
      if (d->key[s2] == kUnusedKey) d->value[s2] = -1;
      if (d->value[s] < d->value[s2]) {
        uint16_t tk = d->key[s]; d->key[s] = d->key[s2]; d->key[s2] = tk;
        int t = d->value[s]; d->value[s] = d->value[s2]; d->value[s2] = t;
        t = d->score[s]; d->score[s] = d->score[s2]; d->score[s2] = t;
        t = d->rel[s]; d->rel[s] = d->rel[s2]; d->rel[s2] = t;
      }
    }
  }
  d->sorted = 1;
}

/* ------------------------------------------------------------- scoring */
typedef struct { int n; uint32_t lp[kMaxBoosts]; } boosts_t;

typedef struct {
  int ulscript;
  boosts_t distinct_latn, distinct_othr;   /* ScoringContext::distinct_boost */
  uint32_t prior_boost[2][kMaxBoosts];     /* ScoringContext::langprior_boost latn / othr (ApplyHints) */
  uint32_t prior_whack[2][kMaxBoosts];     /* ScoringContext::langprior_whack latn / othr */
} ctx_t;

typedef struct { int offset, indirect; } hit_t;
typedef struct { uint16_t offset, type; uint32_t langprob; } linear_t;

typedef struct {           /* scoreonescriptspan.h:169-214 */
  int next_base, next_delta, next_distinct, next_linear, next_chunk_start, lowest_offset;
  hit_t base[kMaxScoringHits + 1], delta[kMaxScoringHits + 1], distinct[kMaxScoringHits + 1];
  linear_t linear[4 * kMaxScoringHits + 1];
  int chunk_start[kMaxSummaries + 1];
} hitbuf_t;

typedef struct {           /* scoreonescriptspan.h:240-252 */
  uint16_t offset, chunk_start, lang1, lang2, score1, score2, bytes, grams, ulscript;
  uint8_t rel_delta, rel_score;
} chunksum_t;

struct cldo_ctx {
  scanner_t ss;
  hitbuf_t hb;
  int predict[kPredictionTableSize];
  int sqz_tbl[kPredictionTableSize];
  uint8_t* docbuf; int docbuf_cap;
  cldo_trace_fn trace; void* trace_arg;
  int trace_text;                              /* also trace each lowered span's bytes (hex) */
  int plain;                                   /* is_plain_text (HTML mode when 0) */
  uint32_t priors[16];                         /* ApplyHints result: boost latn[4] othr[4], whack latn[4] othr[4] */
  rvec_t* vec;                                 /* ResultChunkVector being built, or NULL */
  offmap_t map_orig, map_low;                  /* the scanner's maps (vec mode) */
  int cflags;                                  /* the caller's flags (ExtDetectLanguageSummary `flags`) */
  /* what the first pass of the last document did (cldo_first_pass): spans the scanner returned,
   * the longest span's text bytes, the Squeeze restart taken, a second pass asked for */
  int p1_spans, p1_max_tb, p1_squeeze, p1_recurse;
};

static void tracef(struct cldo_ctx* c, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#include <stdarg.h>
static void tracef(struct cldo_ctx* c, const char* fmt, ...) {
  if (!c->trace) return;
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
  c->trace(c->trace_arg, buf);
}

/* QuadHashV2 / QuadHashV2Mix, cldutil_shared.cc:167-202 */
static const uint32_t kWordMask0[4] = {0xFFFFFFFF, 0x000000FF, 0x0000FFFF, 0x00FFFFFF};
static uint32_t ld32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint32_t quad_hash_v2(const uint8_t* w, int n) {
  if (n == 0) return 0;
  uint32_t pre = 0;
  if (w[-1] == ' ') pre |= 0x00004444;
  if (w[n] == ' ') pre |= 0x44440000;
  uint32_t w0, w1, w2;
  if (n <= 4) {
    w0 = ld32(w) & kWordMask0[n & 3]; w0 ^= w0 >> 3;
    return w0 ^ pre;
  } else if (n <= 8) {
    w0 = ld32(w); w0 ^= w0 >> 3;
    w1 = ld32(w + 4) & kWordMask0[n & 3]; w1 ^= w1 << 4;
    return (w0 ^ pre) + w1;
  }
  w0 = ld32(w); w0 ^= w0 >> 3;
  w1 = ld32(w + 4); w1 ^= w1 << 4;
  w2 = ld32(w + 8) & kWordMask0[n & 3]; w2 ^= w2 << 2;
  return (w0 ^ pre) + w1 + w2;
}
/* BiHashV2, cldutil_shared.cc:107-122 */
static uint32_t bi_hash_v2(const uint8_t* w, int n) {
  if (n == 0) return 0;
  uint32_t w0, w1;
  if (n <= 4) { w0 = ld32(w) & kWordMask0[n & 3]; return w0 ^ (w0 >> 3); }
  w0 = ld32(w); w0 ^= w0 >> 3;
  w1 = ld32(w + 4) & kWordMask0[n & 3]; w1 ^= w1 << 18;
  return w0 + w1;
}
/* OctaHash40 / Mix, cldutil_shared.cc:234-354 */
static uint64_t octa_hash40(const uint8_t* w, int n) {
  if (n == 0) return 0;
  uint64_t pre = 0;
  if (w[-1] == ' ') pre |= 0x00004444;
  if (w[n] == ' ') pre |= 0x44440000;
  uint64_t w0, w1, sum;
  int q = (n - 1) >> 2;
  if (q > 5) q = 5;
  /* word i (0-based) mix: 0:^>>3  1:^<<4  2:^<<2  3:^>>8  4:^>>4  5:^>>6 */
  w0 = ld32(w);
  if (q == 0) w0 &= kWordMask0[n & 3];
  sum = w0;
  w0 = w0 ^ (w0 >> 3);
  for (int i = 1; i <= q; ++i) {
    w1 = ld32(w + 4 * i);
    if (i == q) w1 &= kWordMask0[n & 3];
    sum += w1;
    switch (i) {
      case 1: w1 = w1 ^ (w1 << 4); break;
      case 2: w1 = w1 ^ (w1 << 2); break;
      case 3: w1 = w1 ^ (w1 >> 8); break;
      case 4: w1 = w1 ^ (w1 >> 4); break;
      default: w1 = w1 ^ (w1 >> 6); break;
    }
    w0 += w1;
  }
  sum += sum >> 17;
  sum += sum >> 9;
  sum = (sum & 0xFF) << 32;
  return (w0 ^ pre) + sum;
}
/* PairHash, cldutil_shared.cc:384-386 */
static uint64_t pair_hash(uint64_t a, uint64_t b) { return ((a >> 13) | (a << (64 - 13))) + b; }

/* QuadHashV3Lookup4 / OctaHashV3Lookup4, cldutil_shared.h:380-454 */
static uint32_t lookup4(const tbl_t* t, uint32_t subscr, uint32_t key) {
  if (t->n_buckets == 0) return 0;
  const uint32_t* b = t->b + 4 * (size_t)subscr;
  for (int k = 0; k < 4; ++k) if (((key ^ b[k]) & t->key_mask) == 0) return b[k];
  return 0;
}
static uint32_t quad_lookup(const tbl_t* t, uint32_t h) {
  uint32_t sub = (h + (h >> 12)) & (t->size - 1);
  return lookup4(t, sub, h & t->key_mask);
}
static uint32_t octa_lookup(const tbl_t* t, uint64_t h) {
  uint32_t sub = (uint32_t)((h + (h >> 12)) & (uint64_t)(t->size - 1));
  uint32_t key = (uint32_t)(h >> 4) & t->key_mask;
  return lookup4(t, sub, key);
}
static uint32_t ind_at(const tbl_t* t, uint32_t i) { return i < t->n_ind ? t->ind[i] : 0; }

static int adv_but_space(uint8_t c) { return c <= 0x20 ? 0 : c < 0xC0 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4; }
static int adv_space_vowel(uint8_t c) {
  return (c <= 0x20 || c == 'A' || c == 'E' || c == 'I' || c == 'O' || c == 'U' ||
          c == 'a' || c == 'e' || c == 'i' || c == 'o' || c == 'u' || (c >= 0x80 && c < 0xC0));
}
static int adv_one_char(uint8_t c) { return c < 0xC0 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4; }

/* GetQuadHits cldutil.cc:315-405 */
static int get_quad_hits(const uint8_t* text, int letter_offset, int letter_limit, hitbuf_t* hb) {
  const uint8_t* src = text + letter_offset;
  const uint8_t* lim = text + letter_limit;
  int nb = hb->next_base;
  int npq = 0;
  uint32_t pq[2] = {0, 0};
  if (src[0] == ' ') ++src;
  while (src < lim) {
    const uint8_t* e = src;
    e += adv_but_space(e[0]); e += adv_but_space(e[0]);
    const uint8_t* mid = e;
    e += adv_but_space(e[0]); e += adv_but_space(e[0]);
    int len = (int)(e - src);
    uint32_t h = quad_hash_v2(src, len);
    if (h != pq[0] && h != pq[1]) {
      uint32_t flag = 0;
      const tbl_t* hit = &T.quad;
      uint32_t probs = quad_lookup(&T.quad, h);
      if (probs == 0 && T.quad2.size != 0) {
        flag = 0x80000000u; hit = &T.quad2;
        probs = quad_lookup(&T.quad2, h);
      }
      if (probs != 0) {
        pq[npq] = h; npq = (npq + 1) & 1;
        hb->base[nb].offset = (int)(src - text);
        hb->base[nb].indirect = (int)((probs & ~hit->key_mask) | flag);
        ++nb;
      }
    }
    src = (e[0] == ' ') ? e : mid;
    if (src < lim) src += adv_space_vowel(src[0]);
    else src = lim;
    if (nb >= kMaxScoringHits) break;
  }
  hb->next_base = nb;
  hb->base[nb].offset = (int)(src - text);
  hb->base[nb].indirect = 0;
  return (int)(src - text);
}

/* GetOctaHits cldutil.cc:416-533 */
static void get_octa_hits(const uint8_t* text, int letter_offset, int letter_limit, hitbuf_t* hb) {
  const uint8_t* src = text + letter_offset;
  const uint8_t* lim = text + letter_limit + 1;
  int nd = hb->next_delta, nx = hb->next_distinct;
  int npo = 0;
  uint64_t po[2] = {0, 0};
  int charcount = 0;
  if (src[0] == ' ') ++src;
  const uint8_t* prior_word_start = src;
  const uint8_t* word_start = src;
  const uint8_t* word_end = word_start;
  while (src < lim) {
    if (src[0] == ' ') {
      int len = (int)(word_end - word_start);
      uint64_t wh = octa_hash40(word_start, len);
      if (wh != po[0] && wh != po[1]) {
        po[npo] = wh; npo = 1 - npo;
        uint64_t tph = po[npo];
        if (tph != 0 && tph != wh) {
          uint32_t probs = octa_lookup(&T.distinctocta, pair_hash(tph, wh));
          if (probs) {
            hb->distinct[nx].offset = (int)(prior_word_start - text);
            hb->distinct[nx].indirect = (int)(probs & ~T.distinctocta.key_mask);
            ++nx;
          }
        }
        uint32_t probs = octa_lookup(&T.distinctocta, wh);
        if (probs) {
          hb->distinct[nx].offset = (int)(word_start - text);
          hb->distinct[nx].indirect = (int)(probs & ~T.distinctocta.key_mask);
          ++nx;
        }
        probs = octa_lookup(&T.deltaocta, wh);
        if (probs) {
          hb->delta[nd].offset = (int)(word_start - text);
          hb->delta[nd].indirect = (int)(probs & ~T.deltaocta.key_mask);
          ++nd;
        }
      }
      charcount = 0;
      prior_word_start = word_start;
      word_start = src + 1;
      word_end = word_start;
    } else {
      ++charcount;
    }
    src += utf8_len(src[0]);
    if (charcount <= 8) word_end = src;
    if (nd >= kMaxScoringHits) break;
    if (nx >= kMaxScoringHits - 1) break;
  }
  hb->next_delta = nd; hb->next_distinct = nx;
  int dummy = (int)(src - text);
  hb->delta[nd].offset = dummy; hb->delta[nd].indirect = 0;
  hb->distinct[nx].offset = dummy; hb->distinct[nx].indirect = 0;
}

/* GetUniHits cldutil.cc:201-244 */
static int get_uni_hits(const uint8_t* text, int letter_offset, int letter_limit, hitbuf_t* hb) {
  const uint8_t* src = text + letter_offset;
  const uint8_t* lim = text + letter_limit;
  int nb = hb->next_base;
  if (src[0] == ' ') ++src;
  while (src < lim) {
    const uint8_t* us = src;
    int len = adv_one_char(us[0]);
    src += len;
    int propval = uni_prop(us, len);
    if (propval > 0) {
      hb->base[nb].offset = (int)(src - text);
      hb->base[nb].indirect = propval;
      ++nb;
    }
    if (nb >= kMaxScoringHits) break;
  }
  hb->next_base = nb;
  hb->base[nb].offset = (int)(src - text);
  hb->base[nb].indirect = 0;
  return (int)(src - text);
}

/* GetBiHits cldutil.cc:248-310 */
static void get_bi_hits(const uint8_t* text, int letter_offset, int letter_limit, hitbuf_t* hb) {
  const uint8_t* src = text + letter_offset;
  const uint8_t* lim = text + letter_limit;
  int nd = hb->next_delta, nx = hb->next_distinct;
  while (src < lim) {
    int len = adv_one_char(src[0]);
    int len2 = adv_one_char(src[len]) + len;
    if (6 <= len2) {
      uint32_t bh = bi_hash_v2(src, len2);
      uint32_t probs = quad_lookup(&T.deltabi, bh);
      if (probs) {
        hb->delta[nd].offset = (int)(src - text);
        hb->delta[nd].indirect = (int)(probs & ~T.deltabi.key_mask);
        ++nd;
      }
      probs = quad_lookup(&T.distinctbi, bh);
      if (probs) {
        hb->distinct[nx].offset = (int)(src - text);
        hb->distinct[nx].indirect = (int)(probs & ~T.distinctbi.key_mask);
        ++nx;
      }
    }
    src += len;
    if (nd >= kMaxScoringHits) break;
    if (nx >= kMaxScoringHits - 1) break;
  }
  hb->next_delta = nd; hb->next_distinct = nx;
  int dummy = (int)(src - text);
  hb->delta[nd].offset = dummy; hb->delta[nd].indirect = 0;
  hb->distinct[nx].offset = dummy; hb->distinct[nx].indirect = 0;
}

/* MakeLangProb cldutil.cc:610-614 with kLgProbV2TblBackmap (cldutil_shared.h:310-313) */
static uint32_t make_lang_prob(int lang, int qprob) {
  static const uint8_t backmap[13] = {0, 0, 1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 66};
  uint32_t ps = per_script_number((int)T.meta.ulscript_latin, lang);
  return (ps << 8) | backmap[qprob];
}

/* LinearizeAll scoreonescriptspan.cc:856-975 */
static void linearize_all(const ctx_t* cx, int score_cjk, hitbuf_t* hb) {
  const tbl_t *base_obj, *base_obj2, *delta_obj, *distinct_obj;
  uint16_t base_hit;
  if (score_cjk) {
    base_obj = &T.compat; base_obj2 = &T.compat; delta_obj = &T.deltabi;
    distinct_obj = &T.distinctbi; base_hit = UNIHIT;
  } else {
    base_obj = &T.quad; base_obj2 = &T.quad2; delta_obj = &T.deltaocta;
    distinct_obj = &T.distinctocta; base_hit = QUADHIT;
  }
  int bl = hb->next_base, dl = hb->next_delta, xl = hb->next_distinct;
  int bi = 0, di = 0, xi = 0, li = 0;
  hb->linear[li].offset = (uint16_t)hb->lowest_offset;
  hb->linear[li].type = base_hit;
  hb->linear[li].langprob = make_lang_prob(default_language(cx->ulscript), 1);
  ++li;
  while (bi < bl || di < dl || xi < xl) {
    int boff = hb->base[bi].offset, doff = hb->delta[di].offset, xoff = hb->distinct[xi].offset;
    if (di < dl && doff <= boff && doff <= xoff) {
      uint32_t lp = ind_at(delta_obj, (uint32_t)hb->delta[di].indirect);
      ++di;
      if (lp > 0) { hb->linear[li].offset = (uint16_t)doff; hb->linear[li].type = DELTAHIT; hb->linear[li].langprob = lp; ++li; }
    } else if (xi < xl && xoff <= boff && xoff <= doff) {
      uint32_t lp = ind_at(distinct_obj, (uint32_t)hb->distinct[xi].indirect);
      ++xi;
      if (lp > 0) { hb->linear[li].offset = (uint16_t)xoff; hb->linear[li].type = DISTINCTHIT; hb->linear[li].langprob = lp; ++li; }
    } else {
      uint32_t ind = (uint32_t)hb->base[bi].indirect;
      const tbl_t* lb = base_obj;
      if (ind & 0x80000000u) { lb = base_obj2; ind &= ~0x80000000u; }
      ++bi;
      if (ind < lb->size_one) {
        uint32_t lp = ind_at(lb, ind);
        if (lp > 0) { hb->linear[li].offset = (uint16_t)boff; hb->linear[li].type = base_hit; hb->linear[li].langprob = lp; ++li; }
      } else {
        ind += ind - lb->size_one;
        uint32_t lp = ind_at(lb, ind), lp2 = ind_at(lb, ind + 1);
        if (lp > 0) { hb->linear[li].offset = (uint16_t)boff; hb->linear[li].type = base_hit; hb->linear[li].langprob = lp; ++li; }
        if (lp2 > 0) { hb->linear[li].offset = (uint16_t)boff; hb->linear[li].type = base_hit; hb->linear[li].langprob = lp2; ++li; }
      }
    }
  }
  hb->next_linear = li;
  hb->linear[li].offset = (uint16_t)hb->base[hb->next_base].offset;
  hb->linear[li].langprob = 0;
}

/* ChunkAll scoreonescriptspan.cc:978-1031 */
static void chunk_all(int score_cjk, hitbuf_t* hb) {
  int chunksize = score_cjk ? kChunksizeUnis : kChunksizeQuads;
  uint16_t base_hit = score_cjk ? UNIHIT : QUADHIT;
  int li = 0, lend = hb->next_linear, ncs = 0, left = hb->next_base;
  while (left > 0) {
    int blen = chunksize;
    if (left < chunksize + (chunksize >> 1)) blen = left;
    else if (left < 2 * chunksize) blen = (left + 1) >> 1;
    hb->chunk_start[ncs++] = li;
    int cnt = 0;
    while (cnt < blen && li < lend) {
      if (hb->linear[li].type == base_hit) ++cnt;
      ++li;
    }
    left -= blen;
  }
  if (ncs == 0) hb->chunk_start[ncs++] = 0;
  hb->next_chunk_start = ncs;
  hb->chunk_start[ncs] = hb->next_linear;
}

/* ProcessProbV2Tote cldutil.cc:128-138 */
static void add_lang_prob(uint32_t lp, tote_t* t) {
  const uint8_t* e = T.lgprob + 8 * (lp & 0xFF);
  uint8_t k1 = (lp >> 8) & 0xFF, k2 = (lp >> 16) & 0xFF, k3 = (lp >> 24) & 0xFF;
  if (k1) tote_add(t, k1, e[5]);
  if (k2) tote_add(t, k2, e[6]);
  if (k3) tote_add(t, k3, e[7]);
}

/* ReliabilityDelta cldutil.cc:553-571 */
static int reliability_delta(int v1, int v2, int grams) {
  int maxr = 100;
  if (grams < 8) maxr = 12 * grams;
  int thr = (grams * 5) >> 3;
  if (thr < kMinGramCount) thr = kMinGramCount;
  else if (thr > kMaxGramCount) thr = kMaxGramCount;
  int d = v1 - v2;
  if (d >= thr) return maxr;
  if (d <= 0) return 0;
  int r = (100 * d) / thr;
  return r < maxr ? r : maxr;
}
/* ReliabilityExpected cldutil.cc:585-605 (the path's only floating point) */
static int reliability_expected(int actual, int expected) {
  if (expected == 0) return 100;
  if (actual == 0) return 0;
  double ratio;
  if (expected > actual) ratio = (1.0 * expected) / actual;
  else ratio = (1.0 * actual) / expected;
  if (ratio <= 1.5) return 100;
  if (ratio > 4.0) return 0;
  double num = 100.0 * (4.0 - ratio);
  return (int)(num / (4.0 - 1.5));
}

/* SetChunkSummary scoreonescriptspan.cc:60-96 */
static void set_chunk_summary(int ulscript, int first_linear, int offset, int len,
                              const tote_t* t, chunksum_t* cs) {
  int key3[3];
  tote_top3(t, key3);
  int lang1 = from_per_script_number(ulscript, (uint8_t)key3[0]);
  int lang2 = from_per_script_number(ulscript, (uint8_t)key3[1]);
  int actual = 0;
  if (len > 0) actual = (int)((uint32_t)tote_score(t, key3[0]) << 10) / len;
  int esub = lang1 * 4 + lscript4(ulscript);
  int expected = (esub >= 0 && (uint32_t)esub < T.n_expected) ? T.expected[esub] : 0;
  cs->offset = (uint16_t)offset;
  cs->chunk_start = (uint16_t)first_linear;
  cs->lang1 = (uint16_t)lang1;
  cs->lang2 = (uint16_t)lang2;
  cs->score1 = (uint16_t)tote_score(t, key3[0]);
  cs->score2 = (uint16_t)(key3[1] < 0 ? 0 : tote_score(t, key3[1]));
  cs->bytes = (uint16_t)len;
  cs->grams = (uint16_t)t->score_count;
  cs->ulscript = (uint16_t)ulscript;
  cs->rel_delta = (uint8_t)reliability_delta(cs->score1, cs->score2, cs->grams);
  int c1 = close_set(lang1);
  if (c1 != 0 && c1 == close_set(lang2)) cs->rel_delta = 100;
  cs->rel_score = (uint8_t)reliability_expected(actual, expected);
}

/* ScoreOneChunk :208-259, ScoreBoosts :125-152, AddDistinctBoost2 :112-121.
 * langprior boost/whack rings stay empty on the wrapper path (no hints). */
static void score_one_chunk(ctx_t* cx, const hitbuf_t* hb, int ci, int ulscript, chunksum_t* cs) {
  tote_t t;
  tote_reinit(&t);
  int f = hb->chunk_start[ci], fn = hb->chunk_start[ci + 1];
  boosts_t* db = ((uint32_t)cx->ulscript == T.meta.ulscript_latin) ? &cx->distinct_latn : &cx->distinct_othr;
  for (int i = f; i < fn; ++i) {
    uint32_t lp = hb->linear[i].langprob;
    add_lang_prob(lp, &t);
    if (hb->linear[i].type <= QUADHIT) t.score_count++;
    if (hb->linear[i].type == DISTINCTHIT) { db->lp[db->n] = lp; db->n = (db->n + 1) & (kMaxBoosts - 1); }
  }
  /* ScoreBoosts (scoreonescriptspan.cc:125-152): prior boosts, distinct boosts, then whacks */
  const int so = ((uint32_t)cx->ulscript == T.meta.ulscript_latin) ? 0 : 1;
  for (int k = 0; k < kMaxBoosts; ++k) if (cx->prior_boost[so][k] > 0) add_lang_prob(cx->prior_boost[so][k], &t);
  for (int k = 0; k < kMaxBoosts; ++k) if (db->lp[k] > 0) add_lang_prob(db->lp[k], &t);
  for (int k = 0; k < kMaxBoosts; ++k)
    if (cx->prior_whack[so][k] > 0) t.score[(cx->prior_whack[so][k] >> 8) & 0xFF] = 0;   /* ZeroPSLang :39-42 */
  int lo = hb->linear[f].offset, hi = hb->linear[fn].offset;
  set_chunk_summary(ulscript, f, lo, hi - lo, &t, cs);
}

static void trace_chunk(struct cldo_ctx* c, int i, const chunksum_t* cs) {
  tracef(c, "[%d] %d lin[%d] %s.%d %s.%d %dB %d# %s %dRd %dRs", i, cs->offset, cs->chunk_start,
         cldo_language_code(cs->lang1), cs->score1, cldo_language_code(cs->lang2), cs->score2,
         cs->bytes, cs->grams, script_code(cs->ulscript), cs->rel_delta, cs->rel_score);
}

/* ------------------------------------------------- ResultChunkVector */
static int same_close_set(int l1, int l2) {                  /* SameCloseSet scoreonescriptspan.cc:44-56 */
  int c1 = close_set(l1);
  return c1 != 0 && c1 == close_set(l2);
}
/* GetLangScore cldutil.cc:141-152 */
static int get_lang_score(uint32_t lp, uint8_t pslang) {
  const uint8_t* e = T.lgprob + 8 * (lp & 0xFF);
  int r = 0;
  if (((lp >> 8) & 0xFF) == pslang) r += e[5];
  if (((lp >> 16) & 0xFF) == pslang) r += e[6];
  if (((lp >> 24) & 0xFF) == pslang) r += e[7];
  return r;
}
/* BetterBoundary scoreonescriptspan.cc:671-720 (debug output omitted) */
static int better_boundary(const hitbuf_t* hb, uint8_t ps0, uint8_t ps1, int lin0, int lin1, int lin2) {
  if (lin2 - lin0 <= 8) return lin1;
  int running = 0, diff[8];
  for (int i = lin0; i < lin0 + 8; ++i) {
    int j = i & 7;
    uint32_t lp = hb->linear[i].langprob;
    diff[j] = get_lang_score(lp, ps0) - get_lang_score(lp, ps1);
    if (i < lin0 + 4) running += diff[j]; else running -= diff[j];
  }
  int best_value = 0, best = lin1;
  for (int i = lin0; i < lin2 - 8; ++i) {
    int j = i & 7;
    if (best_value < running) {
      int plus = 0, minus = 0;
      for (int kk = 0; kk < 8; ++kk) { if (diff[kk] > 0) plus = 1; if (diff[kk] < 0) minus = 1; }
      if (plus && minus) { best_value = running; best = i + 4; }
    }
    uint32_t lp = hb->linear[i + 8].langprob;
    int nd = get_lang_score(lp, ps0) - get_lang_score(lp, ps1);
    int md = diff[(i + 4) & 7], od = diff[j];
    diff[j] = nd;
    running -= od; running += 2 * md; running -= nd;
  }
  return best;
}
/* SharpenBoundaries :764-829; sb[n] is the dummy end entry */
static void sharpen_boundaries(const hitbuf_t* hb, int ulscript, chunksum_t* sb, int n) {
  int prior_linear = sb[0].chunk_start;
  uint16_t prior_lang = sb[0].lang1;
  for (int i = 1; i < n; ++i) {
    chunksum_t* cs = &sb[i];
    uint16_t this_lang = cs->lang1;
    if (this_lang == prior_lang) { prior_linear = cs->chunk_start; continue; }
    int this_linear = cs->chunk_start, next_linear = sb[i + 1].chunk_start;
    if (same_close_set(prior_lang, this_lang)) { prior_linear = this_linear; prior_lang = this_lang; continue; }
    uint8_t ps0 = per_script_number(ulscript, prior_lang), ps1 = per_script_number(ulscript, this_lang);
    int better = better_boundary(hb, ps0, ps1, prior_linear, this_linear, next_linear);
    int old_off = hb->linear[this_linear].offset, new_off = hb->linear[better].offset;
    cs->chunk_start = (uint16_t)better;
    cs->offset = (uint16_t)new_off;
    cs->bytes = (uint16_t)(cs->bytes - (new_off - old_off));
    sb[i - 1].bytes = (uint16_t)(sb[i - 1].bytes + (new_off - old_off));
    prior_linear = better;
    prior_lang = this_lang;
  }
}
/* ScriptScanner::MapBack getonescriptspan.cc:1076-1078 */
static int scanner_map_back(struct cldo_ctx* c, int t) {
  return om_map_back(&c->map_orig, om_map_back(&c->map_low, t));
}
/* ItemToVector :322-355 (kMaxResultChunkBytes = 0x7fffffff) */
static void item_to_vector(rvec_t* vec, int new_lang, int mapped_offset, int mapped_len) {
  if (vec->n > 0) {
    rchunk_t* prior = &vec->v[vec->n - 1];
    if (new_lang == prior->lang1) { prior->bytes = (mapped_offset + mapped_len) - prior->offset; return; }
  }
  rchunk_t rc = {mapped_offset, mapped_len, (uint16_t)new_lang, 0};
  rvec_push(vec, rc);
}
/* SummaryBufferToVector :386-495 */
static void summary_buffer_to_vector(struct cldo_ctx* c, const chunksum_t* sb, int n) {
  rvec_t* vec = c->vec;
  const uint8_t* buf = c->ss.buf;
  const int unk = (int)T.meta.unknown_language;
  for (int i = 0; i < n; ++i) {
    const chunksum_t* cs = &sb[i];
    int unmapped_offset = cs->offset, unmapped_len = cs->bytes;
    int mapped_offset = scanner_map_back(c, unmapped_offset);
    if (mapped_offset > 0) {
      int prior_size = vec->n > 0 ? vec->v[vec->n - 1].bytes : 0;
      int n_limit = prior_size - 3 < mapped_offset ? prior_size - 3 : mapped_offset;
      if (n_limit > 12) n_limit = 12;
      const uint8_t* us = buf + mapped_offset;
      int k = 0;
      while (k < n_limit && us[-k - 1] >= 0x41) ++k;
      if (k >= n_limit) k = 0;
      if (k < n_limit) {
        uint8_t ch = us[-k - 1];
        if (ch == '\'' || ch == '"' || ch == '#' || ch == '@') ++k;
      }
      if (k > 0) {
        vec->v[vec->n - 1].bytes -= k;
        mapped_offset -= k;
      }
    }
    int mapped_len = scanner_map_back(c, unmapped_offset + unmapped_len) - mapped_offset;
    int new_lang = cs->lang1;
    int delta_bad = cs->rel_delta < kUnreliablePercentThreshold;
    int score_bad = cs->rel_score < kUnreliablePercentThreshold;
    uint16_t prior_lang = vec->n > 0 ? vec->v[vec->n - 1].lang1 : (uint16_t)unk;
    if (prior_lang == cs->lang1) delta_bad = 0;
    if (same_close_set(cs->lang1, prior_lang)) { new_lang = prior_lang; delta_bad = 0; }
    if (same_close_set(cs->lang1, cs->lang2) && prior_lang == cs->lang2) { new_lang = prior_lang; delta_bad = 0; }
    uint16_t next_lang = (i + 1 >= n) ? (uint16_t)unk : sb[i + 1].lang1;
    if (delta_bad && prior_lang == cs->lang2 && next_lang == cs->lang2) { new_lang = prior_lang; delta_bad = 0; }
    if (delta_bad || score_bad) new_lang = unk;
    item_to_vector(vec, new_lang, mapped_offset, mapped_len);
  }
}
/* JustOneItemToVector :499-530 */
static void just_one_item_to_vector(struct cldo_ctx* c, int lang1, int unmapped_offset, int unmapped_len) {
  int mapped_offset = scanner_map_back(c, unmapped_offset);
  int mapped_len = scanner_map_back(c, unmapped_offset + unmapped_len) - mapped_offset;
  item_to_vector(c->vec, lang1, mapped_offset, mapped_len);
}

/* ProcessHitBuffer :1067-1116 (vec == NULL) */
static void process_hit_buffer(struct cldo_ctx* c, ctx_t* cx, const span_t* span, int score_cjk,
                               hitbuf_t* hb, doctote_t* dt) {
  if (c->trace) {
    tracef(c, "hitbuffer %s base/delta/distinct %d %d %d", script_code(span->ulscript),
           hb->next_base, hb->next_delta, hb->next_distinct);
    for (int i = 0; i < hb->next_base; ++i) tracef(c, "Q[%d]%d,%d", i, hb->base[i].offset, hb->base[i].indirect);
    for (int i = 0; i < hb->next_delta; ++i) tracef(c, "DL[%d]%d,%d", i, hb->delta[i].offset, hb->delta[i].indirect);
    for (int i = 0; i < hb->next_distinct; ++i) tracef(c, "D[%d]%d,%d", i, hb->distinct[i].offset, hb->distinct[i].indirect);
  }
  linearize_all(cx, score_cjk, hb);
  chunk_all(score_cjk, hb);
  if (c->trace) {
    tracef(c, "linear %d", hb->next_linear);
    for (int i = 0; i <= hb->next_linear; ++i)
      tracef(c, "[%d]%d,%c=%08x", i, hb->linear[i].offset,
             i < hb->next_linear ? "UQLD"[hb->linear[i].type & 3] : 'U', hb->linear[i].langprob);
    tracef(c, "chunkstart %d", hb->next_chunk_start);
    for (int i = 0; i <= hb->next_chunk_start; ++i) tracef(c, "[%d]%d", i, hb->chunk_start[i]);
  }
  chunksum_t sb[kMaxSummaries + 1];
  int n = 0;
  for (int i = 0; i < hb->next_chunk_start; ++i) {
    chunksum_t cs;
    score_one_chunk(cx, hb, i, span->ulscript, &cs);
    if (n < kMaxSummaries) sb[n++] = cs;
  }
  /* the dummy entry off the end (ScoreAllHits :289-297) */
  memset(&sb[n], 0, sizeof(sb[n]));
  sb[n].offset = hb->linear[hb->next_linear].offset;
  sb[n].chunk_start = (uint16_t)hb->next_linear;
  if (c->vec) sharpen_boundaries(hb, cx->ulscript, sb, n);
  if (c->trace) {
    tracef(c, "summary %d", n);
    for (int i = 0; i < n; ++i) trace_chunk(c, i, &sb[i]);
  }
  /* SummaryBufferToDocTote :305-315 */
  for (int i = 0; i < n; ++i) {
    int rel = sb[i].rel_delta < sb[i].rel_score ? sb[i].rel_delta : sb[i].rel_score;
    doctote_add(dt, sb[i].lang1, sb[i].bytes, sb[i].score1, rel);
  }
  if (c->vec) summary_buffer_to_vector(c, sb, n);
}

/* SpliceHitBuffer :1118-1127 */
static void splice(hitbuf_t* hb, int next_offset) {
  hb->next_base = hb->next_delta = hb->next_distinct = hb->next_linear = hb->next_chunk_start = 0;
  hb->lowest_offset = next_offset;
}
static void hitbuf_init(hitbuf_t* hb) {        /* ScoringHitBuffer::init (.h:187-207) */
  hb->next_base = hb->next_delta = hb->next_distinct = hb->next_linear = hb->next_chunk_start = 0;
  hb->lowest_offset = 0;
  hb->base[0].offset = hb->base[0].indirect = 0;
  hb->delta[0].offset = hb->delta[0].indirect = 0;
  hb->distinct[0].offset = hb->distinct[0].indirect = 0;
  hb->linear[0].offset = 0; hb->linear[0].langprob = 0;
  hb->chunk_start[0] = 0;
}

/* ScoreOneScriptSpan :1302-1333 and its three cases :1132-1277 */
static void score_one_script_span(struct cldo_ctx* c, ctx_t* cx, const span_t* span, doctote_t* dt) {
  int rt = rtype_of(span->ulscript);
  if ((c->cflags & kCLDFlagScoreAsQuads) && rt != RTypeCJK) rt = RTypeMany;   /* :1318-1320 */
  if (c->trace) tracef(c, "span %s %d", script_code(span->ulscript), span->text_bytes);
  if (rt == RTypeNone || rt == RTypeOne) {
    int bytes = span->text_bytes;
    doctote_add(dt, (uint16_t)default_language(span->ulscript), bytes, bytes, 100);
    if (c->vec) just_one_item_to_vector(c, default_language(span->ulscript), 1, bytes - 1);
    return;
  }
  hitbuf_t* hb = &c->hb;
  hitbuf_init(hb);
  int cjk = (rt == RTypeCJK);
  int off = 1;
  hb->lowest_offset = off;
  int limit = span->text_bytes;
  while (off < limit) {
    int next;
    if (cjk) {
      next = get_uni_hits(span->text, off, limit, hb);
      get_bi_hits(span->text, off, next, hb);
    } else {
      next = get_quad_hits(span->text, off, limit, hb);
      get_octa_hits(span->text, off, next, hb);
    }
    process_hit_buffer(c, cx, span, cjk, hb, dt);
    splice(hb, next);
    off = next;
  }
}

/* ------------------------------------------------------ doc-level passes */
/* MoveLang1ToLang2's ResultChunkVector half (compact_lang_det_impl.cc:1122-1147) */
static void move_lang1_to_lang2_vec(rvec_t* vec, int lang1, int lang2) {
  if (!vec) return;
  int k = 0;
  uint16_t prior_lang = (uint16_t)T.meta.unknown_language;
  for (int i = 0; i < vec->n; ++i) {
    rchunk_t* rc = &vec->v[i];
    if (rc->lang1 == lang1) rc->lang1 = (uint16_t)lang2;
    if (rc->lang1 == prior_lang && k > 0) {
      vec->v[k - 1].bytes += rc->bytes;
    } else {
      vec->v[k] = vec->v[i];
      ++k;
    }
    prior_lang = rc->lang1;
  }
  vec->n = k;
}
/* RefineScoredClosePairs + MoveLang1ToLang2 compact_lang_det_impl.cc:1105-1203 */
static void refine_scored_close_pairs(doctote_t* d, rvec_t* vec) {
  for (int s = 0; s < 24; ++s) {
    int cs = close_set(d->key[s]);
    if (cs == 0) continue;
    for (int s2 = s + 1; s2 < 24; ++s2) {
      if (close_set(d->key[s2]) == cs) {
        int from, to;
        if (d->value[s] < d->value[s2]) { from = s; to = s2; } else { from = s2; to = s; }
        const int from_lang = d->key[from], to_lang = d->key[to];
        d->value[to] += d->value[from];
        d->score[to] += d->score[from];
        d->rel[to] += d->rel[from];
        d->key[from] = kUnusedKey; d->score[from] = 0; d->rel[from] = 0;
        move_lang1_to_lang2_vec(vec, from_lang, to_lang);
        break;
      }
    }
  }
}

/* RemoveUnreliableLanguages :997-1101 (SetScore/SetReliability exactly as
 * written there: the merged entry's *score* field receives newbytes) */
static void remove_unreliable_languages(doctote_t* d) {
  for (int s = 0; s < 24; ++s) {
    int lang = d->key[s];
    if (lang == kUnusedKey) continue;
    int bytes = d->value[s], reli = d->rel[s];
    if (bytes == 0) continue;
    int rp = reli / bytes;
    if (rp >= kMinReliableKeepPercent) continue;
    int alt = (int)T.meta.unknown_language;
    if ((uint32_t)lang <= T.meta.hawaiian && (uint32_t)lang < T.n_closest) alt = T.closest[lang];
    if (alt == (int)T.meta.unknown_language) continue;
    int as = doctote_find(d, (uint16_t)alt);
    if (as < 0) continue;
    int bytes2 = d->value[as], reli2 = d->rel[as];
    if (bytes2 == 0) continue;
    int rp2 = reli2 / bytes2;
    int to = as, from = s;
    if (rp2 < rp || (rp2 == rp && lang < alt)) { to = s; from = as; }
    int np = rp > rp2 ? rp : rp2;
    if (np < kMinReliableKeepPercent) np = kMinReliableKeepPercent;
    int nb = bytes + bytes2;
    int nr = np * nb;
    d->key[from] = kUnusedKey; d->score[from] = 0; d->rel[from] = 0;
    d->score[to] = nb; d->rel[to] = nr;
  }
  for (int s = 0; s < 24; ++s) {
    if (d->key[s] == kUnusedKey) continue;
    int bytes = d->value[s], reli = d->rel[s];
    if (bytes == 0) continue;
    if (reli / bytes >= kMinReliableKeepPercent) continue;
    d->key[s] = kUnusedKey; d->score[s] = 0; d->rel[s] = 0;
  }
}

/* GetNormalizedScore :1269-1273 + ExtractLangEtc :1276-1384 */
static double normalized_score(int bytecount, int score) {
  if (bytecount <= 0) return 0.0;
  return (double)((int32_t)((uint32_t)score << 10) / bytecount);
}
static void extract_lang_etc(const doctote_t* d, int total_text_bytes, int* rp3, int* lang3,
                             int* pct3, double* ns3, int* text_bytes, int* is_reliable) {
  const int unk = (int)T.meta.unknown_language;
  int bc[3] = {0, 0, 0};
  for (int i = 0; i < 3; ++i) { rp3[i] = 0; lang3[i] = unk; pct3[i] = 0; ns3[i] = 0.0; }
  *text_bytes = total_text_bytes;
  *is_reliable = 0;
  for (int i = 0; i < 3; ++i) {
    int k = d->key[i];
    if (k != kUnusedKey && k != unk) {
      lang3[i] = k;
      bc[i] = d->value[i];
      rp3[i] = d->rel[i] / (bc[i] ? bc[i] : 1);
      ns3[i] = normalized_score(bc[i], d->score[i]);
    }
  }
  int t12 = bc[0] + bc[1], t123 = t12 + bc[2];
  if (total_text_bytes < t123) { total_text_bytes = t123; *text_bytes = total_text_bytes; }
  int div = total_text_bytes > 1 ? total_text_bytes : 1;
  pct3[0] = (bc[0] * 100) / div;
  pct3[1] = (t12 * 100) / div;
  pct3[2] = (t123 * 100) / div;
  pct3[2] -= pct3[1];
  pct3[1] -= pct3[0];
  if (pct3[1] < pct3[2]) { ++pct3[1]; --pct3[2]; }
  if (pct3[0] < pct3[1]) { ++pct3[0]; --pct3[1]; }
  *text_bytes = total_text_bytes;
  int k0 = d->key[0];
  if (k0 != kUnusedKey && k0 != unk) {
    int bcount = d->value[0];
    int r = d->rel[0] / (bcount ? bcount : 1);
    *is_reliable = (r >= kMinReliableKeepPercent);
  } else {
    *is_reliable = 0;
  }
  int ignore = 100 - (pct3[0] + pct3[1] + pct3[2]);
  if (ignore > kIgnoreMaxPercent) *is_reliable = 0;
}

static int is_figs(int l) {
  return l == (int)T.meta.french || l == (int)T.meta.italian || l == (int)T.meta.german ||
         l == (int)T.meta.spanish;
}
static int is_efigs(int l) { return l == (int)T.meta.english || is_figs(l); }

/* CalcSummaryLang :1414-1522 */
static void calc_summary_lang(int total_text_bytes, const int* lang3, const int* pct3,
                              int* summary, int* is_reliable, int flags) {
  const int unk = (int)T.meta.unknown_language, en = (int)T.meta.english;
  int slot_count = 3;
  int active[3] = {0, 1, 2};
  int ignore = 0;
  int ret_pct = pct3[0];
  *summary = lang3[0];
  *is_reliable = 1;
  if (pct3[0] < kKeepMinPercent) *is_reliable = 0;
  for (int i = 0; i < 3; ++i) {
    if (lang3[i] == (int)T.meta.tg_unknown_language) {
      ignore += pct3[i];
      for (int j = i + 1; j < 3; ++j) active[j - 1] = active[j];
      --slot_count;
      ret_pct = (pct3[0] * 100) / (101 - ignore);
      *summary = lang3[active[0]];
      if (pct3[active[0]] < kKeepMinPercent) *is_reliable = 0;
    }
  }
  int second_bytes = (total_text_bytes * pct3[active[1]]) / 100;
  int minbytes = kGoodSecondT1T2MinBytes;
  int l0 = lang3[active[0]], l1 = lang3[active[1]];
  if (l0 == en && l1 != en && l1 != unk && pct3[active[1]] >= kNonEnBoilerplateMinPercent &&
      second_bytes >= minbytes) {
    ignore += pct3[active[0]];
    ret_pct = (pct3[active[1]] * 100) / (101 - ignore);
    *summary = l1;
    if (pct3[active[1]] < kKeepMinPercent) *is_reliable = 0;
  } else if (is_figs(l0) && !is_efigs(l1) && l1 != unk &&
             pct3[active[1]] >= kNonFIGSBoilerplateMinPercent && second_bytes >= minbytes) {
    ignore += pct3[active[0]];
    ret_pct = (pct3[active[1]] * 100) / (101 - ignore);
    *summary = l1;
    if (pct3[active[1]] < kKeepMinPercent) *is_reliable = 0;
  } else if (l1 == en && l0 != en) {
    ignore += pct3[active[1]];
    ret_pct = (pct3[active[0]] * 100) / (101 - ignore);
  } else if (is_figs(l1) && !is_efigs(l0)) {
    ignore += pct3[active[1]];
    ret_pct = (pct3[active[0]] * 100) / (101 - ignore);
  }
  if (ret_pct < kGoodFirstMinPercent && !(flags & kCLDFlagBestEffort)) {
    *summary = unk; *is_reliable = 0;
  }
  if (ret_pct < kGoodFirstReliableMinPercent) *is_reliable = 0;
  ignore = 100 - (pct3[0] + pct3[1] + pct3[2]);
  if (ignore > kIgnoreMaxPercent) *is_reliable = 0;
  if (slot_count == 0) { *summary = unk; *is_reliable = 0; }
}

static void trace_doctote(struct cldo_ctx* c, const doctote_t* d) {
  if (!c->trace) return;
  tracef(c, "DocTote::Dump");
  for (int s = 0; s < 24; ++s)
    if (d->key[s] != kUnusedKey)
      tracef(c, "[%2d] %3s %6dB %5dp %4dR,", s, cldo_language_code(d->key[s]), d->value[s], d->score[s], d->rel[s]);
  tracef(c, "  %d chunks scored", d->incr_count);
}

/* DetectLanguageSummaryV2 :1707-2106 with plain text, empty hints,
 * allow_extended_lang=false and resultchunkvector=NULL; the recursion is
 * unrolled into a pass loop with identical flag transitions. */
static int detect_summary_v2(struct cldo_ctx* c, const uint8_t* buf, int len, cldo_result* r) {
  const int unk = (int)T.meta.unknown_language;
  int flags = c->cflags & (kCLDFlagScoreAsQuads | kCLDFlagBestEffort);   /* the caller's flags (:1707) */
  r->passes = 0;
  c->p1_spans = c->p1_max_tb = c->p1_squeeze = c->p1_recurse = 0;
  for (;;) {
    r->passes++;
    for (int i = 0; i < 3; ++i) { r->lang3[i] = (uint16_t)unk; r->percent3[i] = 0; r->normalized3[i] = 0.0; }
    r->text_bytes = 0; r->is_reliable = 0; r->summary_lang = (uint16_t)unk;
    if (len == 0) return unk;
    doctote_t dt; doctote_init(&dt);
    ctx_t cx; memset(&cx, 0, sizeof(cx));
    memcpy(cx.prior_boost, c->priors, 8 * sizeof(uint32_t));
    memcpy(cx.prior_whack, c->priors + 8, 8 * sizeof(uint32_t));
    scanner_t* ss = &c->ss;
    ss->buf = buf; ss->next = 0; ss->remaining = len; ss->plain = c->plain;
    ss->map_orig = c->vec ? &c->map_orig : NULL;
    ss->map_low = c->vec ? &c->map_low : NULL;
    if (c->vec) c->vec->n = 0;              /* resultchunkvector->clear() (:1730-1732) */
    int hash = 0;
    if (flags & kCLDFlagRepeats) memset(c->predict, 0, sizeof(c->predict));
    int total = 0, restart = 0;
    span_t span;
    while (get_one_script_span(ss, &span)) {
      lower_script_span(ss, &span);
      if (c->trace && c->trace_text) {
        static const char hx[] = "0123456789abcdef";
        char* h = (char*)malloc(2 * (size_t)span.text_bytes + 1);
        for (int i = 0; i < span.text_bytes; ++i) {
          h[2 * i] = hx[span.text[i] >> 4];
          h[2 * i + 1] = hx[span.text[i] & 15];
        }
        h[2 * span.text_bytes] = 0;
        if (c->trace) {                        /* direct: longer than tracef's line buffer */
          char* line = (char*)malloc(2 * (size_t)span.text_bytes + 32);
          sprintf(line, "lowered %d %s", flags, h);
          c->trace(c->trace_arg, line);
          free(line);
        }
        free(h);
      }
      if (flags & kCLDFlagSqueeze) {
        span.text_bytes = c->vec ? cheap_squeeze_inplace_overwrite(span.text, span.text_bytes, 0, c->sqz_tbl)
                                 : cheap_squeeze_inplace(span.text, span.text_bytes, 0, c->sqz_tbl);
      } else if ((kCheapSqueezeTestThresh >> 1) < span.text_bytes && !(flags & kCLDFlagFinish)) {
        if (cheap_squeeze_trigger_test(span.text, span.text_bytes, kCheapSqueezeTestLen, c->sqz_tbl)) {
          flags |= kCLDFlagSqueeze; restart = 1;
          if (r->passes == 1) c->p1_squeeze = 1;
          if (c->trace) tracef(c, "restart squeeze");
          break;
        }
      }
      if (flags & kCLDFlagRepeats)
        span.text_bytes = c->vec ? cheap_rep_words_inplace_overwrite(span.text, span.text_bytes, &hash, c->predict)
                                 : cheap_rep_words_inplace(span.text, span.text_bytes, &hash, c->predict);
      cx.ulscript = span.ulscript;
      if (r->passes == 1) {
        c->p1_spans++;
        if (span.text_bytes > c->p1_max_tb) c->p1_max_tb = span.text_bytes;
      }
      score_one_script_span(c, &cx, &span, &dt);
      total += span.text_bytes;
    }
    if (restart) continue;
    trace_doctote(c, &dt);
    refine_scored_close_pairs(&dt, c->vec);
    int rp3[3], lang3[3], pct3[3], tb, rel;
    double ns3[3];
    doctote_sort(&dt, 3);
    extract_lang_etc(&dt, total, rp3, lang3, pct3, ns3, &tb, &rel);
    int good = 0;
    if (flags & kCLDFlagFinish) good = 1;
    else if (total <= kShortTextThresh) good = 1;
    else if (rel && pct3[0] >= kGoodLang1Percent) good = 1;
    else if (rel && pct3[0] + pct3[1] >= kGoodLang1and2Percent) good = 1;
    if (good) {
      if (!(flags & kCLDFlagBestEffort)) remove_unreliable_languages(&dt);   /* :1998-2000 */
      doctote_sort(&dt, 3);
      extract_lang_etc(&dt, total, rp3, lang3, pct3, ns3, &tb, &rel);
      int summary;
      calc_summary_lang(total, lang3, pct3, &summary, &rel, flags);
      for (int i = 0; i < 3; ++i) {
        r->lang3[i] = (uint16_t)lang3[i]; r->percent3[i] = pct3[i]; r->normalized3[i] = ns3[i];
        r->reliable_percent3[i] = rp3[i];
      }
      r->text_bytes = tb; r->is_reliable = (uint8_t)rel; r->summary_lang = (uint16_t)summary;
      if (c->vec && c->vec->n > 0) {         /* FinishResultVector(0, buffer_length) (:1688-1702) */
        rchunk_t* rc = &c->vec->v[0];
        if (rc->offset > 0) { int diff = rc->offset; rc->offset -= diff; rc->bytes += diff; }
        rchunk_t* rc2 = &c->vec->v[c->vec->n - 1];
        int hi2 = rc2->offset + rc2->bytes;
        if (hi2 < len) rc2->bytes += len - hi2;
      }
      if (c->trace) {
        char line[256]; int o = 0;
        for (int i = 0; i < 3; ++i)
          if (lang3[i] != unk) o += snprintf(line + o, sizeof(line) - o, "%s.%dR(%d%%) ", cldo_language_code(lang3[i]), rp3[i], pct3[i]);
        snprintf(line + o, sizeof(line) - o, "%d bytes = %s%c", total, cldo_language_name(summary), rel ? ' ' : '*');
        tracef(c, "%s", line);
      }
      return summary;
    }
    if (c->trace) tracef(c, "recurse total=%d", total);
    c->p1_recurse = 1;
    flags |= kCLDFlagTop40 | kCLDFlagRepeats | kCLDFlagFinish;
    if (total < kShortTextThresh) flags |= kCLDFlagShort | kCLDFlagUseWords;
  }
}

/* ---------------------------------------------------------------- API */
cldo_ctx* cldo_ctx_new(void) {
  cldo_ctx* c = (cldo_ctx*)calloc(1, sizeof(cldo_ctx));
  c->plain = 1;
  c->ss.sbuf = (uint8_t*)calloc(kMaxScriptBuffer + 64, 1);
  c->ss.lbuf = (uint8_t*)calloc(kMaxScriptLowerBuffer + 64, 1);
  return c;
}
void cldo_ctx_free(cldo_ctx* c) {
  if (!c) return;
  free(c->map_orig.d); free(c->map_low.d);
  free(c->ss.sbuf); free(c->ss.lbuf); free(c->docbuf); free(c);
}
void cldo_set_trace(cldo_ctx* c, cldo_trace_fn fn, void* arg) { c->trace = fn; c->trace_arg = arg; }
void cldo_set_trace_text(cldo_ctx* c, int on) { c->trace_text = on; }
void cldo_set_flags(cldo_ctx* c, int flags) { c->cflags = flags; }
void cldo_first_pass(const cldo_ctx* c, int out[4]) {
  out[0] = c->p1_spans; out[1] = c->p1_max_tb; out[2] = c->p1_squeeze; out[3] = c->p1_recurse;
}

/* The document is copied into a buffer followed by 16 NUL bytes, matching
 * the NUL-terminated C string the reference wrapper receives. */
int cldo_detect(cldo_ctx* c, const char* text, int len, cldo_result* r) {
  if (!T.loaded) return -1;
  if (len < 0) len = 0;
  if (c->docbuf_cap < len + 16) {
    free(c->docbuf);
    c->docbuf_cap = len + 16 + 4096;
    c->docbuf = (uint8_t*)malloc((size_t)c->docbuf_cap);
  }
  memcpy(c->docbuf, text, (size_t)len);
  memset(c->docbuf + len, 0, 16);
  memset(r, 0, sizeof(*r));
  return detect_summary_v2(c, c->docbuf, len, r);
}

/* ExtDetectLanguageSummary with a ResultChunkVector (compact_lang_det.h:261-294):
 * up to cap chunks copied to out; returns the vector size (may exceed cap),
 * or a negative error. */
int cldo_detect_vec(cldo_ctx* c, const char* text, int len, int is_plain_text, const uint32_t* priors,
                    cldo_result* r, cldo_rchunk* out, int cap) {
  rvec_t vec = {NULL, 0, 0};
  c->vec = &vec;
  int lang = cldo_detect_ex(c, text, len, is_plain_text, priors, r);
  c->vec = NULL;
  if (lang < 0) { free(vec.v); return lang; }
  for (int i = 0; i < vec.n && i < cap; ++i) {
    out[i].offset = vec.v[i].offset; out[i].bytes = vec.v[i].bytes; out[i].lang1 = vec.v[i].lang1; out[i].pad = 0;
  }
  int n = vec.n;
  free(vec.v);
  return n;
}

/* wrapper.cc:7-16 + compact_lang_det.cc:91-93 (UNKNOWN -> ENGLISH) */
const char* cldo_detect_language(cldo_ctx* c, const char* text) {
  cldo_result r;
  int lang = cldo_detect(c, text, (int)strlen(text), &r);
  if (lang < 0) return NULL;
  if (lang == (int)T.meta.unknown_language) lang = (int)T.meta.english;
  return cldo_language_code(lang);
}

int cldo_meta(int which) {
  switch (which) {
    case 0: return (int)T.meta.num_languages;
    case 1: return (int)T.meta.unknown_language;
    case 2: return (int)T.meta.english;
    default: return -1;
  }
}

/* Batch: n documents, threads > 1 splits them over pthreads (CPU baseline). */
#include <pthread.h>
typedef struct {
  const char* buf; const uint64_t* offs; int lo, hi; cldo_result* out;
  const uint8_t* plain; const uint32_t* priors; int flags;
} job_t;
int cldo_detect_batch_ex(const char* buf, const uint64_t* offsets, int n, const uint8_t* plain,
                         const uint32_t* priors, cldo_result* out, int threads);
/* DetectLanguageSummaryV2 with is_plain_text and the ApplyHints result
 * (compact_lang_det_impl.cc:1587-1684) given: priors = 16 langprobs, boost
 * latn[4] othr[4], whack latn[4] othr[4] (NULL: none). */
int cldo_detect_ex(cldo_ctx* c, const char* text, int len, int is_plain_text, const uint32_t* priors,
                   cldo_result* r) {
  c->plain = is_plain_text ? 1 : 0;
  if (priors) memcpy(c->priors, priors, sizeof(c->priors));
  else memset(c->priors, 0, sizeof(c->priors));
  int lang = cldo_detect(c, text, len, r);
  c->plain = 1;
  memset(c->priors, 0, sizeof(c->priors));
  return lang;
}
static void* run_job(void* a) {
  job_t* j = (job_t*)a;
  cldo_ctx* c = cldo_ctx_new();
  c->cflags = j->flags;
  for (int i = j->lo; i < j->hi; ++i)
    cldo_detect_ex(c, j->buf + j->offs[i], (int)(j->offs[i + 1] - j->offs[i]),
                   j->plain ? j->plain[i] : 1, j->priors ? j->priors + 16 * (size_t)i : NULL, &j->out[i]);
  cldo_ctx_free(c);
  return NULL;
}
int cldo_detect_batch(const char* buf, const uint64_t* offsets, int n, cldo_result* out, int threads) {
  return cldo_detect_batch_ex(buf, offsets, n, NULL, NULL, out, threads);
}
int cldo_detect_batch_ex(const char* buf, const uint64_t* offsets, int n, const uint8_t* plain,
                         const uint32_t* priors, cldo_result* out, int threads) {
  return cldo_detect_batch_flags(buf, offsets, n, plain, priors, out, threads, 0);
}
int cldo_detect_batch_flags(const char* buf, const uint64_t* offsets, int n, const uint8_t* plain,
                            const uint32_t* priors, cldo_result* out, int threads, int flags) {
  if (!T.loaded) return -1;
  if (threads < 1) threads = 1;
  if (threads > 256) threads = 256;
  pthread_t th[256];
  job_t jobs[256];
  for (int t = 0; t < threads; ++t) {
    jobs[t].buf = buf; jobs[t].offs = offsets; jobs[t].out = out; jobs[t].plain = plain; jobs[t].priors = priors;
    jobs[t].flags = flags;
    jobs[t].lo = (int)((int64_t)n * t / threads); jobs[t].hi = (int)((int64_t)n * (t + 1) / threads);
    pthread_create(&th[t], NULL, run_job, &jobs[t]);
  }
  for (int t = 0; t < threads; ++t) pthread_join(th[t], NULL);
  return 0;
}

/* Stage-level entry for pinning against CLD2UnitTestOutputVerbose.html:
 * ChunkAll + ScoreOneChunk over a linear buffer exactly as dumped there
 * (linear[0] = the default-language seed).  `ring` is the distinct-boost ring
 * of the span's script class {n, lp0..lp3}, carried in and out. */
int cldo_score_linear(int ulscript, int score_cjk, int next_base, const uint16_t* offsets,
                      const uint8_t* types, const uint32_t* langprobs, int n_linear,
                      int dummy_offset, uint32_t* ring, cldo_chunk* out, int max_out) {
  static __thread hitbuf_t hb;
  if (n_linear > 4 * kMaxScoringHits || next_base > kMaxScoringHits) return -1;
  for (int i = 0; i < n_linear; ++i) {
    hb.linear[i].offset = offsets[i]; hb.linear[i].type = types[i]; hb.linear[i].langprob = langprobs[i];
  }
  hb.next_linear = n_linear;
  hb.linear[n_linear].offset = (uint16_t)dummy_offset; hb.linear[n_linear].langprob = 0;
  hb.next_base = next_base;
  chunk_all(score_cjk, &hb);
  ctx_t cx; memset(&cx, 0, sizeof(cx));
  cx.ulscript = ulscript;
  boosts_t* db = ((uint32_t)ulscript == T.meta.ulscript_latin) ? &cx.distinct_latn : &cx.distinct_othr;
  if (ring) { db->n = (int)ring[0]; for (int k = 0; k < 4; ++k) db->lp[k] = ring[1 + k]; }
  int n = 0;
  for (int i = 0; i < hb.next_chunk_start && n < max_out; ++i) {
    chunksum_t cs;
    score_one_chunk(&cx, &hb, i, ulscript, &cs);
    out[n].offset = cs.offset; out[n].chunk_start = cs.chunk_start; out[n].lang1 = cs.lang1;
    out[n].lang2 = cs.lang2; out[n].score1 = cs.score1; out[n].score2 = cs.score2;
    out[n].bytes = cs.bytes; out[n].grams = cs.grams; out[n].ulscript = cs.ulscript;
    out[n].rel_delta = cs.rel_delta; out[n].rel_score = cs.rel_score;
    ++n;
  }
  if (ring) { ring[0] = (uint32_t)db->n; for (int k = 0; k < 4; ++k) ring[1 + k] = db->lp[k]; }
  return n;
}

/* As cldo_score_linear but with chunk boundaries given (the dumped
 * DumpChunkStart array), for linear buffers the reference dump truncates. */
int cldo_score_chunks(int ulscript, const uint16_t* offsets, const uint8_t* types,
                      const uint32_t* langprobs, int n_linear, const int* chunk_starts,
                      int n_chunks, uint32_t* ring, cldo_chunk* out) {
  static __thread hitbuf_t hb;
  if (n_linear > 4 * kMaxScoringHits || n_chunks > kMaxSummaries) return -1;
  for (int i = 0; i < n_linear; ++i) {
    hb.linear[i].offset = offsets[i]; hb.linear[i].type = types[i]; hb.linear[i].langprob = langprobs[i];
  }
  for (int i = 0; i <= n_chunks; ++i) {
    if (chunk_starts[i] >= n_linear) return -2;
    hb.chunk_start[i] = chunk_starts[i];
  }
  hb.next_chunk_start = n_chunks;
  ctx_t cx; memset(&cx, 0, sizeof(cx));
  cx.ulscript = ulscript;
  boosts_t* db = ((uint32_t)ulscript == T.meta.ulscript_latin) ? &cx.distinct_latn : &cx.distinct_othr;
  if (ring) { db->n = (int)ring[0]; for (int k = 0; k < 4; ++k) db->lp[k] = ring[1 + k]; }
  for (int i = 0; i < n_chunks; ++i) {
    chunksum_t cs;
    score_one_chunk(&cx, &hb, i, ulscript, &cs);
    out[i].offset = cs.offset; out[i].chunk_start = cs.chunk_start; out[i].lang1 = cs.lang1;
    out[i].lang2 = cs.lang2; out[i].score1 = cs.score1; out[i].score2 = cs.score2;
    out[i].bytes = cs.bytes; out[i].grams = cs.grams; out[i].ulscript = cs.ulscript;
    out[i].rel_delta = cs.rel_delta; out[i].rel_score = cs.rel_score;
  }
  if (ring) { ring[0] = (uint32_t)db->n; for (int k = 0; k < 4; ++k) ring[1 + k] = db->lp[k]; }
  return n_chunks;
}

/* Table-property probes used by tests (not part of the restated path). */
/* Test hooks for the hash pins (oracle/hashcheck/, tests/test_hash_pins.py):
 * kind 0 QuadHashV2 (cldutil_shared.cc:196), 1 BiHashV2 (:107),
 * 2 OctaHash40 (:348).  w[-1] and w[n] are read, as the reference does. */
uint64_t cldo_gram_hash(int kind, const char* w, int n) {
  const uint8_t* p = (const uint8_t*)w;
  if (kind == 0) return quad_hash_v2(p, n);
  if (kind == 1) return bi_hash_v2(p, n);
  return octa_hash40(p, n);
}
uint64_t cldo_pair_hash(uint64_t a, uint64_t b) { return pair_hash(a, b); }
/* QuadHashV3Lookup4 / OctaHashV3Lookup4 on one of the loaded tables, named
 * by its CLDT section id; returns the matching bucket keyvalue or 0. */
uint32_t cldo_probe(int section, uint64_t h) {
  switch (section) {
    case CLDT_CJK_COMPAT: return quad_lookup(&T.compat, (uint32_t)h);
    case CLDT_DELTA_BI: return quad_lookup(&T.deltabi, (uint32_t)h);
    case CLDT_DISTINCT_BI: return quad_lookup(&T.distinctbi, (uint32_t)h);
    case CLDT_QUAD: return quad_lookup(&T.quad, (uint32_t)h);
    case CLDT_QUAD2: return quad_lookup(&T.quad2, (uint32_t)h);
    case CLDT_DELTA_OCTA: return octa_lookup(&T.deltaocta, h);
    case CLDT_DISTINCT_OCTA: return octa_lookup(&T.distinctocta, h);
    default: return 0;
  }
}

/* Test hooks for the HTML-mode pins (tests/test_html_hints.py): the span
 * scanner + lowercaser alone (one callback line "<ulscript> <hex>" per span),
 * the tag parser and the entity reader. */
int cldo_scan_spans(const char* text, int len, int is_plain_text, cldo_trace_fn fn, void* arg) {
  if (!T.loaded) return -1;
  cldo_ctx* c = cldo_ctx_new();
  uint8_t* doc = (uint8_t*)calloc((size_t)len + 16, 1);
  memcpy(doc, text, (size_t)len);
  scanner_t* ss = &c->ss;
  ss->buf = doc; ss->next = 0; ss->remaining = len; ss->plain = is_plain_text ? 1 : 0;
  span_t span;
  int n = 0;
  while (get_one_script_span(ss, &span)) {
    lower_script_span(ss, &span);
    char* line = (char*)malloc(2 * (size_t)span.text_bytes + 32);
    int o = sprintf(line, "%d ", span.ulscript);
    for (int i = 0; i < span.text_bytes; ++i) o += sprintf(line + o, "%02x", span.text[i]);
    fn(arg, line);
    free(line);
    ++n;
  }
  free(doc);
  cldo_ctx_free(c);
  return n;
}
int cldo_scan_tag(const char* text, int len) { return scan_to_possible_letter((const uint8_t*)text, len); }
int cldo_read_entity(const char* text, int len, int* consumed) {
  return read_entity((const uint8_t*)text, len, consumed);
}

int cldo_lower(const char* in, int len, char* out, int olen) {
  return lower_replace((const uint8_t*)in, len, (uint8_t*)out, olen, 1, NULL);
}
int cldo_script_num(const char* s) { return script_num((const uint8_t*)s); }

/* ------------------------------------------------ service text preparation
 * handlers.go:150-151: textStr = StripExtras(textStr); Detect_language(textStr)
 *   StripExtras  handlers.go:198-210 -- for each word of strings.Fields(text)
 *                not HasPrefix "@" / "http": result += word + " "
 *   Detect_language main.go:77-81 -- C.CString + strlen (wrapper.cc:8): the
 *                text ends at its first NUL.
 * strings.Fields (Go 1.x strings.go) splits on unicode.IsSpace runes while
 * ranging over the string rune by rune; the rune decoder is Go's
 * utf8.DecodeRuneInString: an invalid or truncated sequence yields U+FFFD with
 * width 1.  Restated sequentially, rune by rune (the HIP kernel uses a
 * byte-parallel formulation; this is its independent check). */
static int go_decode_rune(const uint8_t* s, int64_t n, int64_t i, uint32_t* r) {
  const uint32_t b0 = s[i];
  if (b0 < 0x80) { *r = b0; return 1; }
  int w = 0;
  uint32_t lo = 0x80, hi = 0xBF;
  if (b0 >= 0xC2 && b0 <= 0xDF) w = 2;
  else if (b0 == 0xE0) { w = 3; lo = 0xA0; }
  else if (b0 >= 0xE1 && b0 <= 0xEC) w = 3;
  else if (b0 == 0xED) { w = 3; hi = 0x9F; }
  else if (b0 >= 0xEE && b0 <= 0xEF) w = 3;
  else if (b0 == 0xF0) { w = 4; lo = 0x90; }
  else if (b0 >= 0xF1 && b0 <= 0xF3) w = 4;
  else if (b0 == 0xF4) { w = 4; hi = 0x8F; }
  if (w == 0 || i + w > n) { *r = 0xFFFD; return 1; }
  const uint32_t b1 = s[i + 1];
  if (b1 < lo || b1 > hi) { *r = 0xFFFD; return 1; }
  for (int k = 2; k < w; ++k)
    if (s[i + k] < 0x80 || s[i + k] > 0xBF) { *r = 0xFFFD; return 1; }
  if (w == 2) *r = ((b0 & 0x1F) << 6) | (b1 & 0x3F);
  else if (w == 3) *r = ((b0 & 0x0F) << 12) | ((b1 & 0x3F) << 6) | (s[i + 2] & 0x3F);
  else *r = ((b0 & 0x07) << 18) | ((b1 & 0x3F) << 12) | ((s[i + 2] & 0x3F) << 6) | (s[i + 3] & 0x3F);
  return w;
}

static int go_is_space(uint32_t r) {   /* unicode.IsSpace */
  if (r <= 0xFF) return r == ' ' || (r >= '\t' && r <= '\r') || r == 0x85 || r == 0xA0;
  return r == 0x1680 || (r >= 0x2000 && r <= 0x200A) || r == 0x2028 || r == 0x2029 || r == 0x202F ||
         r == 0x205F || r == 0x3000;
}

/* One document -> prepared bytes in out (capacity n + 1); returns the length. */
static int64_t prepare_one(const uint8_t* s, int64_t n, int strip, int cstr, uint8_t* out) {
  int64_t o = 0;
  if (!strip) {
    memcpy(out, s, (size_t)n);
    o = n;
  } else {
    int64_t i = 0;
    while (i < n) {
      uint32_t r;
      int w = go_decode_rune(s, n, i, &r);
      if (go_is_space(r)) { i += w; continue; }
      const int64_t ws = i;                     /* a word: runes up to the next space */
      while (i < n) {
        w = go_decode_rune(s, n, i, &r);
        if (go_is_space(r)) break;
        i += w;
      }
      const int64_t wl = i - ws;
      const int drop = s[ws] == '@' || (wl >= 4 && memcmp(s + ws, "http", 4) == 0);
      if (!drop) { memcpy(out + o, s + ws, (size_t)wl); o += wl; out[o++] = ' '; }
    }
  }
  if (cstr) {
    const uint8_t* z = memchr(out, 0, (size_t)o);
    if (z) o = z - out;
  }
  return o;
}

int cldo_prepare_batch(const char* buf, const uint64_t* offsets, int n, int flags, char* out,
                       uint64_t* out_offsets) {
  uint64_t o = 0;
  out_offsets[0] = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t len = (int64_t)(offsets[i + 1] - offsets[i]);
    o += (uint64_t)prepare_one((const uint8_t*)buf + offsets[i], len, flags & 1, flags & 2, (uint8_t*)out + o);
    out_offsets[i + 1] = o;
  }
  return 0;
}
