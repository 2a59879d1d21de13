// k_denoise.hip -- the feature table denoised into ZOTUs (itsx_denoise_table): the UNOISE rule on what itsx_trimmed_table left on the
// device (the representatives' text, totals, lengths and CSR cells, in table order = descending total).
//
// The rule (include/itsx_hip.h has it in full): features in table order; centroid t takes q iff 1 <= d(q, t) <= D and
// (double)a_q <= max_skew[d - 1] * (double)a_t, d the Levenshtein distance of the two texts; q joins the taker with the smallest d,
// then the smallest t; an untaken q with a_q >= minsize is the next centroid, any other is unassigned.
//
// Schedule.  Every max_skew < 1, so a_q <= max_skew[0] * a_t is necessary for any taking.  A level starts at feature f0 and runs
// while a_f > max_skew[0] * a_f0: no feature of a level can take another one of it, so a level's outcome depends on the centroids of
// the earlier levels alone and all its (feature, centroid) pairs are independent: one launch per level, no speculation.
//
// The distance kernel.  One wave (one block) owns a query feature.  It builds the query's match table in LDS once -- per 4-bit
// symbol code one bit per query position, 64 positions a word, by 16 ballots per word -- and walks the centroids 64 at a time: every
// lane works out its centroid's cut-off dmax (the largest d the skews allow) and drops the pair when dmax == 0 or the lengths differ
// by more than dmax; the pairs that stay are queued in LDS until 64 are there, so that the distance loop runs with full lanes.  Then
// each lane runs the banded bit-vector recurrence of k_dn_band.h over its own target: per target symbol two 64-bit LDS loads and a
// funnel shift for the band's match bits, about twenty 64-bit operations for the column, O(L) per pair with all state in registers.
// A pair whose score has passed its cut-off is dead; the loop ends when no lane is alive.  The result is min over (d << 32 | t):
// exact and independent of any order.  Centroids stand in table order, so dmax never rises along them, and the walk stops at the
// first chunk in which no lane has dmax >= 1.
// A query whose columns do not fit one table (m + 31 > DN_CH; the packer allows 65 535 bases) takes the same loop with the table
// rebuilt per window of DN_CH columns: slower, never refused.
#include <hip/hip_runtime.h>
#include "engine.h"
#include "k_api.h"
#include "k_dn_band.h"

namespace itsx {

constexpr int DN_CH = 2048;                 // target columns one match table serves
constexpr int DN_NW = DN_CH / 64 + 3;       // its words per symbol: 64 positions of lead (the band starts up to 31 rows above the column), the
                                            // columns, 63 rows below the last one, and the funnel's second word; odd, so the rows spread over the banks
constexpr unsigned long long DN_NO_TAKER = ~0ull;

// ---- level bounds from feat_total (a chain of bisections: one thread; D == 0: one level, nothing is ever taken)
__global__ void k_dn_levels(DnArgs a)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int32_t nl = 0, f0 = 0;
  while (f0 < a.F) {
    a.lv[nl++] = f0;
    if (a.D == 0) break;
    const double thr = a.max_skew[0] * (double)a.feat_total[f0];
    int32_t lo = f0 + 1, hi = a.F;                              // the first f past f0 with a_f <= thr (totals descend)
    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if ((double)a.feat_total[mid] <= thr) hi = mid; else lo = mid + 1; }
    f0 = lo;
  }
  a.lv[nl] = a.F; *a.nlev = nl; a.ncent[0] = 0;
}

// the query's match table for the columns J0 + 1 .. jmax: bit P of a symbol's row is query position J0 - 64 + P (0-based)
__device__ __forceinline__ void dn_build(uint64_t *tab, const uint8_t *__restrict__ q, int m, int J0, int jmax, int lane)
{
  const int base = J0 - 64;
  int wfill = ((jmax + 62 - base) >> 6) + 2;
  if (wfill > DN_NW) wfill = DN_NW;
  for (int W = 0; W < wfill; W++) {
    const int p = base + 64 * W + lane;
    const uint32_t code = (p >= 0 && p < m) ? dn_code(q[p]) : 16u;
    uint64_t mine = 0;
#pragma unroll 1
    for (uint32_t c = 0; c < 16; c++) { const uint64_t b = __ballot(code == c); if (lane == (int)c) mine = b; }
    if (lane < 16) tab[lane * DN_NW + W] = mine;
  }
}

__device__ __forceinline__ unsigned long long dn_wave_min(unsigned long long v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = ((unsigned long long)(uint32_t)__shfl_xor((int)(v >> 32), o, 64) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ int dn_wave_max(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
  return v;
}

__global__ void __launch_bounds__(64) k_dn_distance(DnArgs a, int32_t level, int32_t f0, int32_t f1)
{
  __shared__ uint64_t tab[16 * DN_NW];
  __shared__ int32_t cand_t[128], cand_k[128];
  __shared__ double skew[32];
  const int lane = threadIdx.x;
  if (lane < 32) skew[lane] = a.max_skew[lane];
  __syncthreads();
  const uint8_t *__restrict__ text = reinterpret_cast<const uint8_t *>(a.text);
  const int32_t C = a.D > 0 ? a.ncent[level] : 0;
  if (blockIdx.x == 0 && lane == 0) a.flag[f1 - f0] = 0;       // (closes the scan of the level's new centroids)
  unsigned long long n_pairs = 0, n_skew = 0, n_len = 0, n_cols = 0;
  for (int32_t q = f0 + (int32_t)blockIdx.x; q < f1; q += (int32_t)gridDim.x) {
    const int m = a.feat_len[q];
    const int32_t aq = a.feat_total[q];
    const uint8_t *__restrict__ qtext = text + a.seq_off[q];
    const bool single = m + DN_MAX_DIFFS <= DN_CH;
    bool built = false;
    unsigned long long best = DN_NO_TAKER;
    int qn = 0;
    int32_t c0 = 0;
    while (c0 < C || qn > 0) {
      // ---- the candidate filter: fill the queue to 64 pairs, or with what is left
      while (qn < 64 && c0 < C) {
        const int32_t c = c0 + lane;
        int32_t t = 0; int k = 0; bool ok = false;
        if (c < C) {
          t = a.cent[c];
          k = dn_dmax(aq, a.feat_total[t], skew, a.D);
          if (k == 0) n_skew++;
          else {
            const int dl = a.feat_len[t] - m;
            ok = (dl < 0 ? -dl : dl) <= k;
            if (!ok) n_len++;
          }
        }
        const unsigned long long okm = __ballot(ok);
        if (ok) { const int at = qn + __popcll(okm & ((1ull << lane) - 1ull)); cand_t[at] = t; cand_k[at] = k; }
        qn += __popcll(okm);
        const bool any_skew = __ballot(c < C && k > 0) != 0ull;
        c0 += 64;
        if (!any_skew) {                                        // dmax never rises along the centroids: the rest is out by the skew
          if (lane == 0 && c0 < C) n_skew += (unsigned long long)(C - c0);
          c0 = C;
        }
      }
      __syncthreads();
      const int take = qn < 64 ? qn : 64;
      if (take > 0) {
        const bool have = lane < take;
        const int32_t t = have ? cand_t[lane] : 0;
        const int k = have ? cand_k[lane] : 0;
        const int n = have ? a.feat_len[t] : 0;
        const int64_t toff = have ? a.seq_off[t] : 0;
        const int nmax = dn_wave_max(n);
        DnBand s;
        dn_band_init(s, k, m, n);
        bool alive = have;
        uint32_t cur = 0;
        for (int J0 = 0; J0 < nmax; J0 += DN_CH) {
          const int jend = J0 + DN_CH < nmax ? J0 + DN_CH : nmax;
          if (!single || !built) {
            __syncthreads();
            dn_build(tab, qtext, m, J0, single ? m + DN_MAX_DIFFS : jend, lane);
            built = true;
            __syncthreads();
          }
          const int base = J0 - 64;
          for (int j = J0 + 1; j <= jend; j++) {
            if (alive) {
              const int64_t pos = toff + j - 1;
              if (j == 1 || (pos & 3) == 0) cur = a.text[pos >> 2];
              const uint32_t code = dn_code((cur >> (8 * (int)(pos & 3))) & 255u);
              dn_band_step(s, dn_band_eq(tab + code * DN_NW, (j - k - 1) - base));
              alive = j < n && s.score <= k;
              n_cols++;
            }
            if (__ballot(alive) == 0ull) break;
          }
          if (__ballot(alive) == 0ull) break;
        }
        unsigned long long mine = DN_NO_TAKER;
        if (have && s.score >= 1 && s.score <= k) mine = ((unsigned long long)(uint32_t)s.score << 32) | (unsigned long long)(uint32_t)t;
        mine = dn_wave_min(mine);
        best = mine < best ? mine : best;
        if (lane == 0) n_pairs += (unsigned long long)take;
        // ---- what the queue holds past the 64 moves to its front
        const int rest = qn - take;
        int32_t mt = 0, mk = 0;
        if (lane < rest) { mt = cand_t[64 + lane]; mk = cand_k[64 + lane]; }
        __syncthreads();
        if (lane < rest) { cand_t[lane] = mt; cand_k[lane] = mk; }
        qn = rest;
      }
      __syncthreads();
    }
    if (lane == 0) {
      const int32_t i = q - f0;
      if (best != DN_NO_TAKER) {
        a.zotu_of[q] = a.zotu_of[(int32_t)(uint32_t)best]; a.dist_of[q] = (int32_t)(best >> 32); a.flag[i] = 0;
      } else if (aq >= a.minsize) {
        a.dist_of[q] = 0; a.flag[i] = 1;                        // (its ZOTU: k_dn_append, after the scan)
      } else {
        a.zotu_of[q] = DN_NONE; a.dist_of[q] = -1; a.flag[i] = 0;
        atomicAdd(&a.counters[DN_C_DROPPED], (unsigned long long)aq);
      }
    }
  }
  // the call's counts (sums of integers: any order gives the same)
  unsigned long long sk = n_skew, ln = n_len, co = n_cols;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sk += ((unsigned long long)(uint32_t)__shfl_xor((int)(sk >> 32), o, 64) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)sk, o, 64);
    ln += ((unsigned long long)(uint32_t)__shfl_xor((int)(ln >> 32), o, 64) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)ln, o, 64);
    co += ((unsigned long long)(uint32_t)__shfl_xor((int)(co >> 32), o, 64) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)co, o, 64);
  }
  if (lane == 0) {
    if (n_pairs) atomicAdd(&a.counters[DN_C_PAIRS], n_pairs);
    if (sk) atomicAdd(&a.counters[DN_C_SKIP_SKEW], sk);
    if (ln) atomicAdd(&a.counters[DN_C_SKIP_LEN], ln);
    if (co) atomicAdd(&a.counters[DN_C_COLUMNS], co);
  }
}

// the level's new centroids behind the others, in table order; their ZOTU is their place
__global__ void __launch_bounds__(256) k_dn_append(DnArgs a, int32_t level, int32_t f0, int32_t f1)
{
  const int32_t nl = f1 - f0, before = a.ncent[level];
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= nl; i += gridDim.x * blockDim.x) {
    if (i == nl) { a.ncent[level + 1] = before + a.pos[nl]; continue; }
    if (!a.flag[i]) continue;
    const int32_t z = before + a.pos[i];
    a.cent[z] = f0 + i; a.zotu_of[f0 + i] = z;
  }
}

// ---- the collapse, as the feature table makes its runs: keys of the assigned features' cells, a radix sort (the caller), heads, a scan
__global__ void __launch_bounds__(256) k_dn_keys(DnArgs a)
{
  for (int32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < a.F; f += gridDim.x * blockDim.x) {
    const int32_t z = a.zotu_of[f];
    for (int32_t e = a.row_off[f]; e < a.row_off[f + 1]; e++) {
      a.keys[e] = z < 0 ? ~0ull : ((unsigned long long)(uint32_t)z << a.sbits) | (unsigned long long)(uint32_t)a.entry_sample[e];
      a.vals[e] = a.entry_count[e];
    }
  }
}
// head [E + 1]: cell i starts a (zotu, sample) run (element E: 0, so that its scan is the number of runs); the sorted counts get a closing 0
// so that their scan has the total behind the last cell
__global__ void __launch_bounds__(256) k_dn_heads(DnArgs a)
{
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= a.E; i += gridDim.x * blockDim.x) {
    int h = 0;
    if (i < a.E) { const unsigned long long k = a.keys_sorted[i]; h = k != ~0ull && (i == 0 || k != a.keys_sorted[i - 1]); }
    else a.vals_sorted[i] = 0;
    a.head[i] = h;
  }
}
// run e starts at cell run_start[e]; the cell behind the last assigned one closes the last run (Ez = hpos[E] runs)
__global__ void __launch_bounds__(256) k_dn_runs(DnArgs a)
{
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.E; i += gridDim.x * blockDim.x) {
    const unsigned long long k = a.keys_sorted[i];
    if (k == ~0ull) continue;
    if (a.head[i]) a.run_start[a.hpos[i]] = i;
    if (i + 1 == a.E || a.keys_sorted[i + 1] == ~0ull) a.run_start[a.hpos[a.E]] = i + 1;
  }
}
// a run's cell: its sample and the sum of its counts, as the difference of the counts' running sum (csum: exclusive scan of the sorted
// counts; a table's reads fit 31 bits) -- no thread walks a run; the first run of a ZOTU starts its row
__global__ void __launch_bounds__(256) k_dn_rows(DnArgs a)
{
  const int32_t Ez = a.hpos[a.E];
  for (int32_t e = blockIdx.x * blockDim.x + threadIdx.x; e <= Ez; e += gridDim.x * blockDim.x) {
    if (e == Ez) { a.z_row_off[a.Z] = Ez; continue; }
    const int32_t i = a.run_start[e];
    const unsigned long long k = a.keys_sorted[i];
    a.z_entry_sample[e] = (int32_t)(k & ((1ull << a.sbits) - 1ull));
    a.z_entry_count[e] = a.csum[a.run_start[e + 1]] - a.csum[i];
    if (i == 0 || (a.keys_sorted[i - 1] >> a.sbits) != (k >> a.sbits)) a.z_row_off[(int32_t)(k >> a.sbits)] = e;
  }
}
__global__ void __launch_bounds__(256) k_dn_totals(DnArgs a)
{
  for (int32_t z = blockIdx.x * blockDim.x + threadIdx.x; z < a.Z; z += gridDim.x * blockDim.x) {
    int32_t sum = 0;
    for (int32_t e = a.z_row_off[z]; e < a.z_row_off[z + 1]; e++) sum += a.z_entry_count[e];
    a.z_total[z] = sum;
  }
}

// ---- host launchers ----
static inline int dn_grid(int64_t n, int cap = 8192)
{
  int64_t g = (n + 255) / 256;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}
void launch_dn_levels(const DnArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_dn_levels, dim3(1), dim3(64), 0, st, a); }
void launch_dn_distance(const DnArgs &a, int32_t level, int32_t f0, int32_t f1, hipStream_t st)
{
  const int32_t nl = f1 - f0;
  hipLaunchKernelGGL(k_dn_distance, dim3(nl < 1 ? 1 : (nl > (1 << 20) ? (1 << 20) : nl)), dim3(64), 0, st, a, level, f0, f1);
}
void launch_dn_append(const DnArgs &a, int32_t level, int32_t f0, int32_t f1, hipStream_t st)
{
  hipLaunchKernelGGL(k_dn_append, dim3(dn_grid((int64_t)(f1 - f0) + 1)), dim3(256), 0, st, a, level, f0, f1);
}
void launch_dn_keys(const DnArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_dn_keys, dim3(dn_grid(a.F)), dim3(256), 0, st, a); }
void launch_dn_heads(const DnArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_dn_heads, dim3(dn_grid((int64_t)a.E + 1)), dim3(256), 0, st, a); }
void launch_dn_runs(const DnArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_dn_runs, dim3(dn_grid(a.E)), dim3(256), 0, st, a); }
void launch_dn_rows(const DnArgs &a, hipStream_t st)
{
  hipLaunchKernelGGL(k_dn_rows, dim3(dn_grid((int64_t)a.E + 1)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_dn_totals, dim3(dn_grid(a.Z)), dim3(256), 0, st, a);
}

}  // namespace itsx
