// k_ftable.hip -- the feature table of a batch's trimmed regions (itsx_trimmed_table): distinct trimmed sequences by samples.
//
// What `vsearch --derep_fulllength --sizeout --relabel_sha1` makes of the trimmed FASTQ files of all samples (QIIME 2's
// dereplicate-sequences), from what the context holds after the search: the packed reads, their exception lists, the per-read
// coordinates and every read's sample.  The reference has no call site for it (its last step is the trimmed FASTQ).
//
// A read is counted iff the trimmed-FASTQ writer would write it and its slice [start, min(stop, len)) holds at least min_len bases.
// Two counted reads are one feature iff their slices are equal symbol for symbol, forward strand only.  The key of a slice is a run
// of 32-bit words: its 2-bit residues re-packed from bit 2 * start (the last word's unused fields zero), the exceptions inside it
// rebased to the slice (N and A are both 0 in the 2-bit plane, so the exceptions are part of the key), and its length (a prefix of
// another sequence is another feature).  Grouping is the dereplication's: an open-addressing table keyed on XXH64 of the key words that
// holds the smallest read index, then an exact word-by-word verification against the slot's holder, so that a 64-bit collision never
// merges two sequences: a read whose holder is another sequence probes on to the next slot of its hash in the next round.
// Integer work bound by HBM latency: one lane per read, one load per key word.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "engine.h"
#include "k_api.h"
#include "k_xxh64.h"
#include "iupac.h"

namespace itsx {

// the counting rule: the slice's length, 0 for a read that is not counted; off = its first base
__device__ __forceinline__ int ft_slice(const FtArgs &a, int64_t r, int &off)
{
  const int s = a.start[r], e = a.stop[r], L = a.rd.len[r];
  off = s;
  if (s < 0 || e < 0 || s >= e) return 0;
  const int b = e < L ? e : L;
  return b - s >= a.min_len ? b - s : 0;              // (min_len >= 1: a start past the end is not counted either)
}

// first exception of the sorted list exc[0, n) at or past position p
__device__ __forceinline__ int ft_exc_lower(const uint32_t *__restrict__ exc, int n, int p)
{
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int)(exc[mid] >> 4) < p) lo = mid + 1; else hi = mid; }
  return lo;
}

// Key words of one slice.  RegKey (k_derep.hip) loads two source words per output word and rescans the exception list per exception
// word; here the source word an output word ends in is carried to the next one (one load per output word when the words are asked for
// in rising order, as XXH64 and the verification do; any other order is served too, by a reload), and the exceptions inside the slice
// are a contiguous run of the read's sorted list, found by two bisections -- a read of 4 096 N costs its lane 4 096 loads, not 16 M.
struct SliceKey {
  const uint32_t *w; const uint32_t *exc; int nw_read, off, Ld, nwd, nex_in;
  mutable int ca; mutable uint32_t lo, up;            // source words ca and ca + 1 (ca = -2: none yet)
  __device__ __forceinline__ uint32_t word(int j) const
  {
    const int start = off + 16 * j;
    const int a = start >> 4, s = (start & 15) * 2;
    if (a != ca) {
      lo = (a == ca + 1) ? up : w[a];
      up = (a + 1 < nw_read) ? w[a + 1] : 0u;
      ca = a;
    }
    uint32_t W = s ? ((lo >> s) | (up << (32 - s))) : lo;
    const int cnt = Ld - 16 * j;
    if (cnt < 16) W &= (1u << (2 * cnt)) - 1u;
    return W;
  }
  __device__ __forceinline__ uint32_t operator()(int j) const
  {
    if (j < nwd) return word(j);
    j -= nwd;
    if (j < nex_in) { const uint32_t e = exc[j]; return ((uint32_t)((int)(e >> 4) - off) << 4) | (e & 15u); }
    return (uint32_t)Ld;
  }
  __device__ __forceinline__ int nwords() const { return nwd + nex_in + 1; }
};
__device__ __forceinline__ SliceKey make_slicekey(const ReadsDev &rd, int64_t read, int off, int Ld)
{
  SliceKey k;
  const int64_t wo = rd.woff[read], eo = rd.excoff[read];
  const int nexc = (int)(rd.excoff[read + 1] - eo);
  k.w = rd.words + wo; k.nw_read = (int)(rd.woff[read + 1] - wo);
  k.off = off; k.Ld = Ld; k.nwd = (Ld + 15) >> 4;
  k.exc = rd.exc + eo; k.nex_in = 0;
  if (nexc > 0) {
    const int e0 = ft_exc_lower(k.exc, nexc, off);
    k.nex_in = ft_exc_lower(k.exc + e0, nexc - e0, off + Ld);
    k.exc += e0;
  }
  k.ca = -2; k.lo = 0u; k.up = 0u;
  return k;
}

__global__ void __launch_bounds__(256) k_ft_coords(const int32_t *__restrict__ start, const int32_t *__restrict__ stop, int32_t stride, int64_t n,
                                                   int32_t *__restrict__ ostart, int32_t *__restrict__ ostop)
{
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    ostart[r] = start[r * stride]; ostop[r] = stop[r * stride];
  }
}

// 1. Key and insert.  Round 0: every counted read hashes its slice and enters the table.  Trimmed amplicon regions are massive
// duplicates, so -- as k_region_keys does -- the lanes of a wave that hold one hash send their lowest lane (the smallest read: r ascends
// with the lane), and that lane reads the slot before it issues an atomic.  Round k > 0 (after a resolve that left reads pending, which
// takes two different sequences under one 64-bit hash): only the pending reads enter again, and they pass the first k slots of their
// hash -- the ones whose holders they were compared with in rounds 0 .. k - 1 -- before they claim or join one.
__global__ void __launch_bounds__(256) k_ft_insert(FtArgs a, int round)
{
  const int lane = threadIdx.x & 63;
  const int64_t n = a.rd.n;
  // (whole waves walk the loop together: the block and the stride are multiples of 64)
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g - lane < n; g += (int64_t)gridDim.x * blockDim.x) {
    uint64_t key = 0;                                           // 0: no read to insert here
    if (g < n) {
      if (round == 0) {
        int off;
        const int Ld = ft_slice(a, g, off);
        if (Ld == 0) { a.slot_of[g] = FT_NONE; a.feature_read[g] = -1; }
        else {
          const SliceKey sk = make_slicekey(a.rd, g, off, Ld);
          key = xxh64_words(sk, sk.nwords(), 0x9E3779B97F4A7C15ULL);
          if (key == 0) key = 1;
          a.hash[g] = key;
        }
      } else if (a.feature_read[g] == FT_PENDING) key = a.hash[g];
    }
    unsigned long long todo = __ballot(key != 0);
    if (round == 0 && todo && lane == __builtin_ctzll(todo)) atomicAdd(&a.counters[0], (unsigned long long)__popcll(todo));
    int leader = lane;                                          // the lowest lane of every distinct hash leads it
    while (todo) {
      const int l0 = __builtin_ctzll(todo);
      const uint64_t k0 = ((uint64_t)(uint32_t)__shfl((int)(key >> 32), l0, 64) << 32) | (uint64_t)(uint32_t)__shfl((int)key, l0, 64);
      const unsigned long long same = __ballot(key == k0) & todo;
      if (key == k0) leader = l0;
      todo &= ~same;
    }
    uint32_t myslot = 0;
    if (key != 0 && leader == lane) {
      uint64_t slot = (key * 0x9E3779B97F4A7C15ULL >> 20) & a.mask;
      int skip = round;
      for (;;) {
        unsigned long long cur = __hip_atomic_load(&a.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) { cur = atomicCAS(&a.keys[slot], 0ull, (unsigned long long)key); if (cur == 0ull) { cur = key; skip = 0; } }
        if (cur == key) { if (skip == 0) break; skip--; }
        slot = (slot + 1) & a.mask;
      }
      if (__hip_atomic_load(&a.vals[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (int32_t)g) atomicMin(&a.vals[slot], (int32_t)g);
      myslot = (uint32_t)slot;
    }
    myslot = (uint32_t)__shfl((int)myslot, leader, 64);
    if (key != 0) a.slot_of[g] = myslot;
  }
}

// 2. Resolve.  feature_read[r] = the holder of r's slot once r's key words are verified to be the holder's, one by one: the same
// length, the same number of exceptions inside, the same words.  Another sequence under the same hash: r stays pending and the next
// round's insert probes on.  (Round 0 looks at every counted read, a later round at the pending ones.)
__global__ void __launch_bounds__(256) k_ft_resolve(FtArgs a, int round)
{
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.rd.n; r += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t slot = a.slot_of[r];
    if (slot == FT_NONE) continue;
    if (round > 0 && a.feature_read[r] != FT_PENDING) continue;
    const int32_t s = a.vals[slot];
    bool same = s == (int32_t)r;
    if (!same) {
      int offr, offs;
      const int Lr = ft_slice(a, r, offr), Ls = ft_slice(a, s, offs);
      same = Lr == Ls;
      if (same) {
        const SliceKey kr = make_slicekey(a.rd, r, offr, Lr), ks = make_slicekey(a.rd, s, offs, Ls);
        same = kr.nex_in == ks.nex_in;
        for (int j = 0; same && j < kr.nwd + kr.nex_in; j++) same = kr(j) == ks(j);
      }
    }
    if (same) a.feature_read[r] = s;
    else { a.feature_read[r] = FT_PENDING; atomicAdd(&a.counters[1], 1ull); }
  }
}

// 3. Count and order.  (holder, sample) pairs of the counted reads, sorted; their runs are the table's entries, the runs of equal
// holders its features (in holder order = rising first read), and one more sort on (~total << 32 | first_read) is the table's order.
__global__ void __launch_bounds__(256) k_ft_pairs(FtArgs a)
{
  const int64_t n = a.rd.n;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const int32_t h = a.feature_read[r];
    a.pair_keys[r] = h < 0 ? (unsigned long long)n << a.sbits
                           : ((unsigned long long)(uint32_t)h << a.sbits) | (unsigned long long)(uint32_t)(a.sample ? a.sample[r] : 0);
  }
}
// ehead / fhead [nc + 1]: position i starts an entry / a feature (element nc: 0, so that its scan is the number of runs)
__global__ void __launch_bounds__(256) k_ft_heads(FtArgs a)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= a.nc; i += (int64_t)gridDim.x * blockDim.x) {
    int eh = 0, fh = 0;
    if (i < a.nc) {
      const unsigned long long k = a.pair_sorted[i], p = i ? a.pair_sorted[i - 1] : ~k;
      eh = k != p; fh = (k >> a.sbits) != (p >> a.sbits) || i == 0;
      if (i == 0) eh = 1;
    }
    a.ehead[i] = eh; a.fhead[i] = fh;
  }
}
__global__ void __launch_bounds__(256) k_ft_runs(FtArgs a)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= a.nc; i += (int64_t)gridDim.x * blockDim.x) {
    if (i == a.nc) { a.ent_start[a.E] = (int32_t)a.nc; a.f_ent0[a.F] = a.E; a.f_pos0[a.F] = (int32_t)a.nc; continue; }
    if (!a.ehead[i]) continue;
    const unsigned long long k = a.pair_sorted[i];
    const int32_t e = a.epos[i], fh = a.fhead[i], f = a.fpos[i] + fh - 1;
    a.ent_start[e] = (int32_t)i; a.ent_sample[e] = (int32_t)(k & ((1ull << a.sbits) - 1ull)); a.ent_feat[e] = f;
    if (fh) {
      const int32_t holder = (int32_t)(k >> a.sbits);
      a.f_ent0[f] = e; a.f_pos0[f] = (int32_t)i; a.f_first[f] = holder; a.hold_f[holder] = f;
    }
  }
}
__global__ void __launch_bounds__(256) k_ft_order_keys(FtArgs a)
{
  for (int32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < a.F; f += gridDim.x * blockDim.x) {
    const uint32_t total = (uint32_t)(a.f_pos0[f + 1] - a.f_pos0[f]);
    a.okeys[f] = ((unsigned long long)(~total) << 32) | (unsigned long long)(uint32_t)a.f_first[f];
    a.ovals[f] = f;
  }
}
// the features in table order (element F of nent: 0, so that its scan is row_off)
__global__ void __launch_bounds__(256) k_ft_ranked(FtArgs a)
{
  for (int32_t g = blockIdx.x * blockDim.x + threadIdx.x; g <= a.F; g += gridDim.x * blockDim.x) {
    if (g == a.F) { a.nent[g] = 0; continue; }
    const unsigned long long k = a.okeys_sorted[g];
    const int32_t f = a.ovals_sorted[g], first = (int32_t)(uint32_t)k;
    int off;
    a.rank_of[f] = g;
    a.feat_total[g] = (int32_t)~(uint32_t)(k >> 32); a.feat_first[g] = first; a.feat_len[g] = ft_slice(a, first, off);
    a.nent[g] = a.f_ent0[f + 1] - a.f_ent0[f];
  }
}
// the entries behind their features (samples ascend inside a feature: the pairs were sorted), and every read's feature
__global__ void __launch_bounds__(256) k_ft_entries(FtArgs a)
{
  const int64_t n = a.rd.n, stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t e = t; e < a.E; e += stride) {
    const int32_t f = a.ent_feat[e];
    const int32_t o = a.row_off[a.rank_of[f]] + ((int32_t)e - a.f_ent0[f]);
    a.entry_sample[o] = a.ent_sample[e]; a.entry_count[o] = a.ent_start[e + 1] - a.ent_start[e];
  }
  for (int64_t r = t; r < n; r += stride) {
    const int32_t h = a.feature_read[r];
    a.feature_of_read[r] = h < 0 ? -1 : a.rank_of[a.hold_f[h]];
  }
}

// 4. Text.  The representatives' slices as ASCII, one after the other (feature g at seq_off[g]): a lane makes 16 consecutive bytes of
// the output and stores them at once, so a wave writes one contiguous KiB.  Bases are unpacked from wherever the slice starts in its
// read; the exceptions' symbols come from iupac.h.  A chunk that spans several short features walks them.
__global__ void __launch_bounds__(256) k_ft_text(FtArgs a)
{
  const int64_t nchunks = (a.text_bytes + 15) >> 4;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunks; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = c << 4;
    int32_t g = 0;                                              // the feature of byte o: seq_off[g] <= o < seq_off[g + 1]
    { int32_t hi = a.F; while (hi - g > 1) { const int32_t mid = g + ((hi - g) >> 1); if (a.seq_off[mid] <= o) g = mid; else hi = mid; } }
    int64_t next = 0, wo = 0; int p = 0, wi = -1, xpos = -1, ne = 0; uint32_t cur = 0, xcode = 0; const uint32_t *ex = nullptr;
    auto enter = [&](int64_t ob) {                              // byte ob is in feature g: its source position, word and next exception
      const int64_t base = a.seq_off[g]; next = a.seq_off[g + 1];
      const int32_t r = a.feat_first[g];
      p = a.start[r] + (int)(ob - base);
      wo = a.rd.woff[r]; wi = -1;
      const int64_t eo = a.rd.excoff[r];
      const int nexc = (int)(a.rd.excoff[r + 1] - eo);
      xpos = -1; ne = 0;
      if (nexc > 0) {
        const int e0 = ft_exc_lower(a.rd.exc + eo, nexc, p);
        ex = a.rd.exc + eo + e0; ne = nexc - e0;
        if (ne > 0) { xpos = (int)(ex[0] >> 4); xcode = ex[0] & 15u; }
      }
    };
    enter(o);
    uint32_t out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int64_t ob = o + k;
      if (ob < a.text_bytes) {                                  // (the bytes past the text's end stay 0: the buffer is padded)
        if (ob >= next) { g++; enter(ob); }                     // (every feature holds at least one base)
        if ((p >> 4) != wi) { wi = p >> 4; cur = a.rd.words[wo + wi]; }
        uint32_t ch = (0x54474341u >> (8 * ((cur >> (2 * (p & 15))) & 3u))) & 255u;      // "ACGT"
        if (p == xpos) {
          ch = iupac_symbol(xcode);
          ex++; ne--;
          xpos = ne > 0 ? (int)(ex[0] >> 4) : -1; if (ne > 0) xcode = ex[0] & 15u;
        }
        out[k >> 2] |= ch << (8 * (k & 3));
        p++;
      }
    }
    reinterpret_cast<uint4 *>(a.text)[c] = make_uint4(out[0], out[1], out[2], out[3]);
  }
}

// ---- host launchers ----
static inline int ft_grid(int64_t n, int cap = 8192)
{
  int64_t g = (n + 255) / 256;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}
void launch_ft_coords(const int32_t *start, const int32_t *stop, int32_t stride, int64_t n, int32_t *ostart, int32_t *ostop, hipStream_t st)
{
  hipLaunchKernelGGL(k_ft_coords, dim3(ft_grid(n)), dim3(256), 0, st, start, stop, stride, n, ostart, ostop);
}
void launch_ft_insert(const FtArgs &a, int round, hipStream_t st) { hipLaunchKernelGGL(k_ft_insert, dim3(ft_grid(a.rd.n)), dim3(256), 0, st, a, round); }
void launch_ft_resolve(const FtArgs &a, int round, hipStream_t st) { hipLaunchKernelGGL(k_ft_resolve, dim3(ft_grid(a.rd.n)), dim3(256), 0, st, a, round); }
void launch_ft_pairs(const FtArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_ft_pairs, dim3(ft_grid(a.rd.n)), dim3(256), 0, st, a); }
void launch_ft_heads(const FtArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_ft_heads, dim3(ft_grid(a.nc + 1)), dim3(256), 0, st, a); }
void launch_ft_runs(const FtArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_ft_runs, dim3(ft_grid(a.nc + 1)), dim3(256), 0, st, a); }
void launch_ft_order_keys(const FtArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_ft_order_keys, dim3(ft_grid(a.F)), dim3(256), 0, st, a); }
void launch_ft_ranked(const FtArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_ft_ranked, dim3(ft_grid((int64_t)a.F + 1)), dim3(256), 0, st, a); }
void launch_ft_entries(const FtArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_ft_entries, dim3(ft_grid(a.rd.n)), dim3(256), 0, st, a); }
void launch_ft_text(const FtArgs &a, hipStream_t st)
{
  if (a.text_bytes > 0) hipLaunchKernelGGL(k_ft_text, dim3(ft_grid((a.text_bytes + 15) >> 4)), dim3(256), 0, st, a);
}

size_t ft_sort_bytes(int64_t n)
{
  size_t b1 = 0, b2 = 0;
  (void)rocprim::radix_sort_keys(nullptr, b1, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (size_t)n, 0, 64, (hipStream_t)0);
  (void)rocprim::radix_sort_pairs(nullptr, b2, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr,
                                  (size_t)n, 0, 64, (hipStream_t)0);
  return (b1 > b2 ? b1 : b2) + 256;
}
int ft_sort_keys(void *tmp, size_t bytes, const unsigned long long *kin, unsigned long long *kout, int64_t n, int end_bit, hipStream_t st)
{
  if (n <= 0) return 0;
  return (int)rocprim::radix_sort_keys(tmp, bytes, kin, kout, (size_t)n, 0, (unsigned)end_bit, st);
}
int ft_sort_pairs(void *tmp, size_t bytes, const unsigned long long *kin, unsigned long long *kout, const int32_t *vin, int32_t *vout, int64_t n, hipStream_t st)
{
  if (n <= 0) return 0;
  return (int)rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0, 64, st);
}

}  // namespace itsx
