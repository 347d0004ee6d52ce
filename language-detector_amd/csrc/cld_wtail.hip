// cld_wtail.hip -- k_wtail: the tail of k_wave's deferred instantiation, one
// lane per document.
//
// Everything after a span's chunks have their top two keys -- SetChunkSummary,
// the DocTote adds, the document level -- runs in k_wave on 1 to 24 of a
// wavefront's 64 lanes, and a wave64 instruction costs the same whether one
// lane is live or all.  Here the wave leaves each document's chunks as records
// (layout in cld_kernels.h) and 64 documents share a wavefront: the same
// sequential arithmetic as the reference, executed once per 64 documents.
// The code below is the sequential form (DocTote::add / sort3 of cld_prims.hip,
// the document level as oracle/cld_oracle.c states it), with the lane's
// DocTote in LDS, lane-minor: slot s of field f sits at [f][s][lane], so the
// 64 lanes of an access fall on 64 consecutive words and never share a bank.
// No scratch: nothing here is a dynamically indexed private array.
//
// Which slots are in use is a 24-bit mask in a register (`u`), not kUnusedKey
// in the key field: a slot outside the mask is never read, so the tote needs
// no initialisation, and every loop over the 24 slots visits the slots in use
// only (one to three for most documents) in the same ascending order.  Where
// the reference gives an unused slot the value -1 (Sort), the mask says so.

namespace cld {
namespace wtail {

constexpr int kSlots = 24;
enum { fKey = 0, fVal = 1, fScore = 2, fRel = 3, kFields = 4 };
using Tote = int[kFields][kSlots][64];

__device__ __forceinline__ bool used(uint32_t u, int s) { return (u >> s) & 1; }
__device__ __forceinline__ uint32_t above(uint32_t u, int s) { return u & ~((2u << s) - 1u); }   // slots > s in use

// DocTote::Add (tote.cc:127-175)
__device__ __forceinline__ void add(Tote& t, int ln, uint32_t& u, int k, int bytes, int sc, int r) {
  const int s0 = k & 15, s1 = s0 ^ 8, s2 = (k & 7) + 16;
  const int k0 = used(u, s0) ? t[fKey][s0][ln] : (int)kUnusedKey, k1 = used(u, s1) ? t[fKey][s1][ln] : (int)kUnusedKey,
            k2 = used(u, s2) ? t[fKey][s2][ln] : (int)kUnusedKey;
  int a = k0 == k ? s0 : k1 == k ? s1 : k2 == k ? s2 : -1;
  if (a >= 0) {
    t[fVal][a][ln] += bytes; t[fScore][a][ln] += sc; t[fRel][a][ln] += r * bytes;
    return;
  }
  if (k0 == kUnusedKey) a = s0;
  else if (k1 == kUnusedKey) a = s1;
  else if (k2 == kUnusedKey) a = s2;
  else {
    a = s0;
    if (t[fVal][s1][ln] < t[fVal][a][ln]) a = s1;
    if (t[fVal][s2][ln] < t[fVal][a][ln]) a = s2;
  }
  u |= 1u << a;
  t[fKey][a][ln] = k; t[fVal][a][ln] = bytes; t[fScore][a][ln] = sc; t[fRel][a][ln] = r * bytes;
}

// DocTote::Sort(3) (tote.cc:221-250): pass s swaps slot s with every later slot
// whose value beats its current one, strictly.  An unused slot counts as -1 and
// so never beats anything; an unused slot s takes the first later slot in use.
__device__ __forceinline__ void sort3(Tote& t, int ln, uint32_t& u) {
  for (int s = 0; s < 3; ++s) {
    int vs = used(u, s) ? t[fVal][s][ln] : -1;
    for (uint32_t m = above(u, s); m; m &= m - 1) {
      const int s2 = __builtin_ctz(m), v2 = t[fVal][s2][ln];
      if (!(vs < v2)) continue;
      if (used(u, s)) {
#pragma unroll
        for (int f = 0; f < kFields; ++f) {
          const int x = t[f][s][ln];
          t[f][s][ln] = t[f][s2][ln];
          t[f][s2][ln] = x;
        }
      } else {
#pragma unroll
        for (int f = 0; f < kFields; ++f) t[f][s][ln] = t[f][s2][ln];
        u = (u | 1u << s) & ~(1u << s2);
      }
      vs = v2;
    }
  }
}

// RefineScoredClosePairs (compact_lang_det_impl.cc:1105-1147): slot s, in
// order, merges with the first later slot of its close set, the smaller into
// the larger (whose slot keeps its value field, as there).
__device__ __forceinline__ void refine_close_pairs(const DevTables& T, Tote& t, int ln, uint32_t& u) {
  for (uint32_t m = u; m; m &= m - 1) {
    const int s = __builtin_ctz(m);
    if (!used(u, s)) continue;                           // emptied by an earlier merge
    const int cs = close_set(T, t[fKey][s][ln]);
    if (cs == 0) continue;
    for (uint32_t m2 = above(u, s); m2; m2 &= m2 - 1) {
      const int s2 = __builtin_ctz(m2);
      if (close_set(T, t[fKey][s2][ln]) != cs) continue;
      const bool s_from = t[fVal][s][ln] < t[fVal][s2][ln];
      const int from = s_from ? s : s2, to = s_from ? s2 : s;
      t[fVal][to][ln] += t[fVal][from][ln];
      t[fScore][to][ln] += t[fScore][from][ln];
      t[fRel][to][ln] += t[fRel][from][ln];
      u &= ~(1u << from);
      break;
    }
  }
}

// RemoveUnreliableLanguages (compact_lang_det_impl.cc:997-1101) on the sorted
// tote (Find is then a linear scan: the first slot with the key).  As there, a
// merge moves the new byte count into the score field and leaves value alone.
__device__ __forceinline__ void remove_unreliable(const DevTables& T, Tote& t, int ln, uint32_t& u) {
  const int unk = (int)T.unknown_lang;
  for (uint32_t m = u; m; m &= m - 1) {
    const int s = __builtin_ctz(m);
    if (!used(u, s)) continue;                           // emptied by an earlier merge
    const int lang = t[fKey][s][ln], bytes = t[fVal][s][ln];
    if (bytes == 0) continue;
    const int rp = t[fRel][s][ln] / bytes;
    if (rp >= 41) continue;
    int alt = unk;
    if ((uint32_t)lang <= T.hawaiian && (uint32_t)lang < T.n_closest) alt = gld(T.closest + lang);
    if (alt == unk) continue;
    int as = -1;
    for (uint32_t m2 = u; m2 && as < 0; m2 &= m2 - 1)
      if (t[fKey][__builtin_ctz(m2)][ln] == alt) as = __builtin_ctz(m2);
    if (as < 0) continue;
    const int bytes2 = t[fVal][as][ln];
    if (bytes2 == 0) continue;
    const int rp2 = t[fRel][as][ln] / bytes2;
    int to = as, from = s;
    if (rp2 < rp || (rp2 == rp && lang < alt)) { to = s; from = as; }
    int np = rp > rp2 ? rp : rp2;
    if (np < 41) np = 41;
    const int nbytes = bytes + bytes2;
    u &= ~(1u << from);
    t[fScore][to][ln] = nbytes; t[fRel][to][ln] = np * nbytes;
  }
  for (uint32_t m = u; m; m &= m - 1) {
    const int s = __builtin_ctz(m), bytes = t[fVal][s][ln];
    if (bytes == 0) continue;
    if (t[fRel][s][ln] / bytes >= 41) continue;
    u &= ~(1u << s);
  }
}

// ExtractLangEtc (compact_lang_det_impl.cc:1276-1384) with GetNormalizedScore (:1269-1273)
__device__ __forceinline__ Extract extract(const DevTables& T, Tote& t, int ln, uint32_t u, int total) {
  const int unk = (int)T.unknown_lang;
  Extract x;
  int bc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    x.lang3[i] = unk; x.pct3[i] = 0; x.rp3[i] = 0; x.ns3[i] = 0.0;
    bc[i] = 0;
    const int k = used(u, i) ? t[fKey][i][ln] : unk;
    if (k != unk) {
      x.lang3[i] = k;
      bc[i] = t[fVal][i][ln];
      x.rp3[i] = t[fRel][i][ln] / (bc[i] ? bc[i] : 1);
      x.ns3[i] = bc[i] > 0 ? (double)((int32_t)((uint32_t)t[fScore][i][ln] << 10) / bc[i]) : 0.0;
    }
  }
  const int t12 = bc[0] + bc[1], t123 = t12 + bc[2];
  const int tot = total < t123 ? t123 : total;
  const int div = tot > 1 ? tot : 1;
  int q0 = (bc[0] * 100) / div, q1 = (t12 * 100) / div, q2 = (t123 * 100) / div;
  q2 -= q1;
  q1 -= q0;
  if (q1 < q2) { ++q1; --q2; }
  if (q0 < q1) { ++q0; --q1; }
  x.pct3[0] = q0; x.pct3[1] = q1; x.pct3[2] = q2;
  x.text_bytes = tot;
  // (slot 0's reliability percent is rp3[0], and 0 when the slot holds no language)
  x.reliable = x.lang3[0] != unk && x.rp3[0] >= 41;
  if (100 - (q0 + q1 + q2) > 20) x.reliable = false;
  return x;
}

}  // namespace wtail

// One lane per document of a batch k_wave<.., true, true> has been over.  A
// document whose first pass is not good enough (possible only past 256 text
// bytes) joins the re-queue list, as finish_document's `final = false` does in
// the wave.  One wavefront per workgroup: its 64 DocTotes are the block's LDS.
__global__ __launch_bounds__(64) void k_wtail(DevTables T, int n, const uint4* __restrict__ recs,
                                             cld_result* __restrict__ out, uint32_t* __restrict__ requeue_list,
                                             uint32_t* __restrict__ counters, uint32_t cflags) {
  __shared__ wtail::Tote tote;
  using namespace wtail;
  const int ln = (int)threadIdx.x, i = (int)blockIdx.x * 64 + ln;
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(recs + (size_t)(i < n ? i : 0) * (kTailSlotBytes / 16));
  const uint4 hd = i < n ? gld4(rec) : make_uint4(kTailNone, 0u, 0u, 0u);
  bool requeue = false;
  if (hd.x != kTailNone) {
    const int cnt = min((int)hd.x, kTailRecs), total = (int)hd.y;
    uint32_t u = 0;                                      // the slots in use
    uint4 nxt = cnt > 0 ? gld4(rec + 4) : make_uint4(0u, 0u, 0u, 0u);
    for (int r = 1; r <= cnt; ++r) {
      const uint4 c = nxt;
      if (r < cnt) nxt = gld4(rec + 4 * (r + 1));        // (the next record's load overlaps this one's arithmetic)
      if (c.x == kTailSpan) {
        add(tote, ln, u, (int)(uint16_t)c.y, (int)c.z, (int)c.z, 100);
        continue;
      }
      // SetChunkSummary (scoreonescriptspan.cc:60-96): language, close set and
      // expected score of both keys from the per-GPU key table (lng::keytab_eval)
      const uint64_t* kt = T.keytab + 256 * (c.w >> 16);
      const uint64_t i1 = gld(kt + (c.x & 0xFF)), i2 = gld(kt + ((c.x >> 8) & 0xFF));
      const int cs1 = (int)(c.y & 0xFFFF), cs2 = (int)(c.y >> 16);
      const int len = (int)(c.z >> 16) - (int)(c.z & 0xFFFF);
      int actual = 0;
      if (len > 0) actual = (int)((uint32_t)cs1 << 10) / len;
      const int expected = (int16_t)(uint16_t)(i1 >> 32);
      const uint16_t bytes = (uint16_t)len, grams = (uint16_t)(c.w & 0xFFFF);
      int rd = (uint8_t)reliability_delta(cs1, cs2, grams);
      const int c1 = (int)((i1 >> 16) & 0xFFFF);
      if (c1 != 0 && c1 == (int)((i2 >> 16) & 0xFFFF)) rd = 100;
      const int rsc = (uint8_t)reliability_expected(actual, expected);
      add(tote, ln, u, (int)(i1 & 0xFFFF), bytes, cs1, rd < rsc ? rd : rsc);
    }
    // the document level (compact_lang_det_impl.cc:1997-2065)
    const bool best_effort = (cflags & kCLDFlagBestEffort) != 0;
    refine_close_pairs(T, tote, ln, u);
    sort3(tote, ln, u);
    Extract x = extract(T, tote, ln, u, total);
    const bool good = total <= 256 || (x.reliable && x.pct3[0] >= 70) || (x.reliable && x.pct3[0] + x.pct3[1] >= 93);
    if (good) {
      if (!best_effort) remove_unreliable(T, tote, ln, u);
      sort3(tote, ln, u);
      x = extract(T, tote, ln, u, total);
      bool rel;
      const int summary = calc_summary_lang(T, total, x, rel, best_effort);
      write_result(&out[i], x, summary, rel);
    }
    requeue = !good;
  }
  wave_append(requeue, &counters[kCtrRequeue], requeue_list, (uint32_t)i, nullptr);
}

}  // namespace cld
