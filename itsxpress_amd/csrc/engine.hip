// engine.hip -- host orchestration and the C ABI (include/itsx_hip.h) of the gfx950 engine.
//
// The path it drives (reference: itsxpress/SeqSample.py:93-225 + 368-562, main.py:176-231):
//   reads (packed, resident in HBM) -> derep (k_derep) -> uniques ordered by length ->
//   MSV for every (unique, profile) (k_msv) -> survivor list grouped by profile ->
//   bias filter + Forward -> Backward + posterior decoding + regions -> envelope re-scoring
//   (k_float) -> scores, per-profile reported counts (domZ) -> domain thresholds ->
//   ItsPosition argmax -> per-read (start, stop, tlen).
// Everything numeric runs on the device; the host parses text, packs reads, sizes buffers,
// builds per-length constant tables with libm (as hmmsearch does on its host), and sorts rows
// for the file-compatible writers.  There is no CPU fallback for any stage.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <numeric>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string_view>
#include <thread>
#include <unordered_map>
#include "detmath.h"
#include "engine.h"
#include "k_api.h"
#include "deflate_codes.h"
#include "inflate_codes.h"
#include "fastq_rec.h"
#include "twriter_dev.h"
#include "cluster_multi.h"
#include "fastq_io.h"
#include "iupac.h"
#include "writers.h"

namespace itsx {
void launch_region_offsets(int64_t npairs, const PairRec *pairs, const int32_t *pref, const int64_t *seg_pair_start,
                           const int64_t *seg_region_start, int64_t *pair_region0, hipStream_t st);
void launch_finalize(itsx_domain *dom, int64_t n, const int64_t *domz, double domE, const int32_t *usample, int P, hipStream_t st);
void launch_positions(const itsx_domain *dom, int64_t n, const int8_t *side, unsigned long long *bl, unsigned long long *br,
                      int32_t *in_ddict, hipStream_t st);
void launch_position_coords(const itsx_domain *dom, int64_t n, const int8_t *side, const unsigned long long *bl, const unsigned long long *br,
                            int32_t *cl, int32_t *cr, hipStream_t st);
void launch_position_flags(const itsx_domain *dom, int64_t n, const int8_t *side, const unsigned long long *bl, const unsigned long long *br,
                           int32_t *uflag, hipStream_t st);
void launch_count_flags(const int32_t *uflag, int32_t U, const int32_t *uniq_of, int64_t n, unsigned long long *c, hipStream_t st);
void launch_compact_best(const itsx_domain *dom, int64_t n, const int8_t *cls, int ncls, double lnp_certain, unsigned long long *bestc, hipStream_t st);
void launch_compact_mark(const itsx_domain *dom, int64_t n, const int8_t *cls, int ncls, double lnp_certain, const unsigned long long *bestc, int32_t *keep, hipStream_t st);
void launch_compact_scatter(const itsx_domain *dom, int64_t n, const int32_t *keep, const int32_t *pos, itsx_domain *out, hipStream_t st);

// ---- a few tiny kernels that only the orchestration needs --------------------------------
__global__ void k_wave_rows_pairs(const WaveDesc *w, int nw, const PairRec *pairs, int32_t *rows)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nw) return;
  // (lengths ascend inside a segment -- piecewise, with prefix sharing: by (batch, depth) run -- so the longest need not be the last)
  int mx = 0;
  for (int k = 0; k < w[i].count; k++) mx = max(mx, pairs[w[i].first + k].L);
  rows[i] = mx + 1;
}
// The wave list of a whole chunk's pairs, made where it is used: wave i covers 64 consecutive pairs of one profile's segment, the
// profiles in launch order (`order`, waves before them in `woff`).  A million-read shard has 1.3 M waves: built on the host they were
// 43 MB up, 5 MB of row counts down and 43 MB up again -- 20 ms in which the GPU did nothing.  Also sums the waves' lane-rows.
__global__ void k_waves_build(int nw, int P, const int32_t *__restrict__ order, const int64_t *__restrict__ woff, const int64_t *__restrict__ seg_start,
                              const int32_t *__restrict__ total, const PairRec *__restrict__ pairs, WaveDesc *__restrict__ w, unsigned long long *__restrict__ lane_rows)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long mine = 0;
  if (i < nw) {
    int lo = 0, hi = P;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (woff[mid] <= (int64_t)i) lo = mid; else hi = mid; }
    const int p = order[lo];
    const int64_t k = ((int64_t)i - woff[lo]) * 64;
    WaveDesc d;
    d.prof = p; d.first = seg_start[p] + k; d.count = (int32_t)min((int64_t)64, (int64_t)total[p] - k); d.slab = 0;
    // (called on length-ordered segments today -- the unshared schedule -- but a share-ordered list must not under-size a wave silently:
    // the longest of the wave's pairs, not the last)
    int mx = 0;
    for (int q = 0; q < d.count; q++) { const int L = pairs[d.first + q].L; mx = L > mx ? L : mx; mine += (unsigned long long)L; }
    d.rows = mx + 1;
    d.pad = 0;
    w[i] = d;
  }
  for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(lane_rows, mine);
}
// merged read j out of the merge kernel's output (pair i's bases sit at foff[i] + roff[i]) into a gap-free text: one wave per read
__global__ void __launch_bounds__(256) k_gather_reads(const uint8_t *__restrict__ src, const int64_t *__restrict__ srcoff, const int64_t *__restrict__ dstoff, int64_t m,
                                                      uint8_t *__restrict__ dst)
{
  const int lane = threadIdx.x & 63;
  for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < m; j += (int64_t)gridDim.x * 4) {
    const int64_t so = srcoff[j], d0 = dstoff[j], len = dstoff[j + 1] - d0;
    for (int64_t k = lane; k < len; k += 64) dst[d0 + k] = src[so + k];
  }
}
__global__ void k_wave_rows_regions(const WaveDesc *w, int nw, const RegionRec *rg, int32_t *rows)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nw) return;
  int mx = 0;
  for (int k = 0; k < w[i].count; k++) { const RegionRec r = rg[w[i].first + k]; mx = max(mx, r.jenv - r.ienv + 1); }
  rows[i] = mx + 1;
}
__global__ void k_pair_counters(const PairOut *po, int64_t n, unsigned long long *c)
{
  unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const PairOut o = po[i];
    a0 += o.pass_bias; a1 += o.pass_fwd; a2 += o.pass_fwd ? o.nregions : 0; a3 += (o.flags & 2) ? 1 : 0; a4 += o.pass_fwd ? ((o.flags >> 8) & 0xff) : 0;
  }
  for (int d = 32; d >= 1; d >>= 1) { a0 += __shfl_down(a0, d, 64); a1 += __shfl_down(a1, d, 64); a2 += __shfl_down(a2, d, 64); a3 += __shfl_down(a3, d, 64); a4 += __shfl_down(a4, d, 64); }
  if ((threadIdx.x & 63) == 0) { atomicAdd(&c[0], a0); atomicAdd(&c[1], a1); atomicAdd(&c[2], a2); atomicAdd(&c[3], a3); atomicAdd(&c[4], a4); }
}
__global__ void k_gather_i32(const int32_t *src, const int64_t *idx, int n, int32_t *out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = src[idx[i]];
}
// slots of the envelope memoisation's table (k_derep.hip: k_region_keys) for n regions: a power of two, never more than half full
static uint64_t region_table_size(int64_t n)
{
  uint64_t tsize = 1024;
  while (tsize < (uint64_t)n * 2 + 16) tsize <<= 1;
  return tsize;
}

// out[i] = src[idx[i] / 64]: the selection's chunk scan (k_lazy.hip) at the start of each profile segment
__global__ void k_gather_chunk_i32(const int32_t *src, const int64_t *idx, int n, int32_t *out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = src[idx[i] >> 6];
}
__global__ void k_rep_coords(int32_t U, const unsigned long long *bl, const unsigned long long *br, const int32_t *cl, const int32_t *cr,
                             const int32_t *seed_read, const int32_t *len, int32_t *start, int32_t *stop, int32_t *tlen)
{
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const unsigned long long l = bl[u], r = br[u];
  start[u] = l ? cl[u] : -1;                      // left.to_pos  (itsxpress/SeqSample.py:480)
  stop[u] = r ? cr[u] - 1 : -1;                   // right.from_pos - 1  (:484)
  tlen[u] = (l || r) ? len[seed_read[u]] : -1;
}
__global__ void k_read_coords(int64_t n, const int32_t *uniq_of, const int32_t *us, const int32_t *ue, const int32_t *ut, const int32_t *uind,
                              int32_t *start, int32_t *stop, int32_t *tlen, int32_t *ind)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int u = uniq_of[r];
  if (u < 0) { start[r] = stop[r] = tlen[r] = -1; ind[r] = 0; return; }
  start[r] = us[u]; stop[r] = ue[u]; tlen[r] = ut[u]; ind[r] = uind[u];
}
__global__ void k_pack_coords4(int64_t n, const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int32_t *out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { out[i * 4] = a[i]; out[i * 4 + 1] = b[i]; out[i * 4 + 2] = c[i]; out[i * 4 + 3] = d[i]; }
}
// per unique: the orientation-free 128-bit key (two XXH64 seeds over the packed read, length folded in; the smaller of
// forward / reverse complement), the global index of its first occurrence, and whether the forward strand is the canonical one
__global__ void k_unique_keys128(int32_t U, const int32_t *seed_read, const int32_t *len, const uint64_t *f0, const uint64_t *r0, const uint64_t *f1,
                                 const uint64_t *r1, int64_t base, int64_t *out)
{
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int32_t r = seed_read[u];
  const uint64_t lm = (uint64_t)len[r] * 0x9E3779B97F4A7C15ULL;
  const uint64_t kf0 = f0[r] ^ lm, kr0 = r0[r] ^ lm, kf1 = f1[r] ^ lm, kr1 = r1[r] ^ lm;
  const bool fwd_le = (kf0 < kr0) || (kf0 == kr0 && kf1 <= kr1);
  out[(int64_t)u * 4 + 0] = (int64_t)(fwd_le ? kf0 : kr0);
  out[(int64_t)u * 4 + 1] = (int64_t)(fwd_le ? kf1 : kr1);
  out[(int64_t)u * 4 + 2] = base + r;
  out[(int64_t)u * 4 + 3] = fwd_le ? 1 : 0;
}
__global__ void k_widen_i32(int64_t n, const int32_t *in, int64_t *out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}
}  // namespace itsx

using namespace itsx;

static std::string g_create_error;

// device buffer that only ever grows: hipMalloc/hipFree of multi-GB buffers costs far more than the
// kernels that use them, so every work buffer is kept in the context between calls
// hipFree waits for the DEVICE to go idle.  With several contexts at work on one GPU (a streaming run: two chunks searched, a third
// being loaded, a fourth finalized) a buffer that grows in one context stalled its thread until every other context's kernels had
// finished -- 435 frees, 4.4 s of such waits in a 7.6-s pipeline.  Device memory that a context gives up is therefore kept on a
// list and returned in one go: when a context is destroyed, or when the list holds more than ITSX_DEFER_FREE_GB (16; 0 = free at
// once, as before).  Nothing is reused from the list, so a kernel still reading an old buffer reads valid memory.
static std::mutex g_grave_mu;
static std::vector<void *> g_grave;
static size_t g_grave_bytes = 0;
static void grave_flush()
{
  std::vector<void *> v;
  { std::lock_guard<std::mutex> g(g_grave_mu); v.swap(g_grave); g_grave_bytes = 0; }
  for (void *q : v) (void)hipFree(q);
}
static void defer_free(void *q, size_t bytes)
{
  static const size_t budget = (size_t)(sw_get("ITSX_DEFER_FREE_GB") ? std::max(0.0, atof(sw_get("ITSX_DEFER_FREE_GB"))) : 16.0) << 30;
  if (budget == 0) { (void)hipFree(q); return; }
  bool flush = false;
  { std::lock_guard<std::mutex> g(g_grave_mu); g_grave.push_back(q); g_grave_bytes += bytes; flush = g_grave_bytes > budget; }
  if (flush) grave_flush();
}

// The DP slab (pass A's saved states, then the rounds' rows) is the one buffer of tens of GB, and FRESH device memory costs 20-40 ms per GB
// (it is cleared): a streamed file's chunk contexts each brought their own (round 6: 9 x ~1 s).  A context that is done with its slab
// (itsx_release_scratch: its stream is idle) puts it here, and the next context's slab request takes a block of at least its size from
// here before it asks the driver.  Blocks leave the pool when the last context is destroyed.
struct PoolBlock { void *p; size_t bytes; int device; };
static std::mutex g_pool_mu;
static std::vector<PoolBlock> g_pool;
static int g_live_contexts = 0;
static void *pool_take(size_t bytes, int device, size_t *got)
{
  std::lock_guard<std::mutex> g(g_pool_mu);
  int best = -1;
  for (size_t i = 0; i < g_pool.size(); i++)
    if (g_pool[i].device == device && g_pool[i].bytes >= bytes && (best < 0 || g_pool[i].bytes < g_pool[(size_t)best].bytes)) best = (int)i;
  if (best < 0) return nullptr;
  void *q = g_pool[(size_t)best].p; *got = g_pool[(size_t)best].bytes;
  g_pool.erase(g_pool.begin() + best);
  return q;
}
static void pool_put(void *q, size_t bytes, int device)
{
  std::lock_guard<std::mutex> g(g_pool_mu);
  g_pool.push_back(PoolBlock{q, bytes, device});
}
static void pool_flush()
{
  std::vector<PoolBlock> v;
  { std::lock_guard<std::mutex> g(g_pool_mu); v.swap(g_pool); }
  for (auto &b : v) (void)hipFree(b.p);
}

// The labels of a read set: one blob + offsets instead of one std::string per record (10-20 M allocations per 10 M-read run, and
// as many moves when the parser's pieces are joined).  The part of std::vector<std::string>'s interface the engine uses.
struct NameList {
  std::vector<char> blob; std::vector<int64_t> off{0};
  size_t size() const { return off.size() - 1; }
  bool empty() const { return off.size() <= 1; }
  void clear() { blob.clear(); off.assign(1, 0); }
  void swap(NameList &o) { blob.swap(o.blob); off.swap(o.off); }
  const char *ptr(size_t i) const { return blob.data() + off[i]; }
  size_t len(size_t i) const { return (size_t)(off[i + 1] - off[i]); }
  void emplace_back(const char *b, const char *e) { blob.insert(blob.end(), b, e); off.push_back((int64_t)blob.size()); }
  std::string operator[](size_t i) const { return std::string(ptr(i), len(i)); }
  int cmp(size_t a, size_t b) const          // strcmp's order (labels hold no NUL)
  {
    const size_t la = len(a), lb = len(b), m = la < lb ? la : lb;
    const int c = m ? memcmp(ptr(a), ptr(b), m) : 0;
    return c ? c : (la < lb ? -1 : la > lb ? 1 : 0);
  }
  void assign(const char *names, const int64_t *name_offsets, int64_t n)      // names[name_offsets[i] .. name_offsets[i + 1])
  {
    const int64_t o0 = name_offsets[0];
    blob.assign(names + o0, names + name_offsets[n]);
    off.resize((size_t)n + 1);
    for (int64_t i = 0; i <= n; i++) off[(size_t)i] = name_offsets[i] - o0;
  }
  NameList slice(size_t lo, size_t hi) const
  {
    NameList r;
    r.blob.assign(blob.begin() + off[lo], blob.begin() + off[hi]);
    r.off.resize(hi - lo + 1);
    for (size_t i = lo; i <= hi; i++) r.off[i - lo] = off[i] - off[lo];
    return r;
  }
};

template <class T> struct DBuf {
  T *p = nullptr; size_t n = 0, cap = 0;
  int pool_device = -1;       // >= 0: a request that must allocate looks in the slab pool first (the DP slab only)
  // exact: no growth headroom (the slabs: their size is a budget, not a data-dependent count)
  hipError_t alloc(size_t count, bool exact = false)
  {
    n = count;
    if (count <= cap && p) return hipSuccess;
    static const bool trace = sw_get("ITSX_TRACE_ALLOC") != nullptr;
    if (p) {
      const auto f0 = std::chrono::steady_clock::now();
      defer_free(p, cap * sizeof(T));
      if (trace) fprintf(stderr, "[itsx] free %.3f GB: %.1f ms\n", cap * sizeof(T) / 1073741824.0, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f0).count());
    }
    p = nullptr; cap = 0;
    if (!count) return hipSuccess;
    if (pool_device >= 0) {
      size_t got = 0;
      if (void *q = pool_take(count * sizeof(T), pool_device, &got)) { p = (T *)q; cap = got / sizeof(T); return hipSuccess; }
    }
    const size_t want = exact ? count : count + count / 8 + 64;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
    if (trace) fprintf(stderr, "[itsx] hipMalloc %.3f GB: %.1f ms\n", want * sizeof(T) / 1073741824.0, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (e != hipSuccess) {               // no room for the growth headroom: the exact size, and the failed attempt's sticky error cleared
      (void)hipGetLastError();
      grave_flush();                     // (what was given up but not returned yet)
      e = hipMalloc((void **)&p, count * sizeof(T));
      if (e != hipSuccess) { p = nullptr; return e; }
      cap = count; return e;
    }
    cap = want;
    return hipSuccess;
  }
  void release() { if (p) defer_free(p, cap * sizeof(T)); p = nullptr; n = 0; cap = 0; }
  ~DBuf() { release(); }
};

struct itsx_ctx {
  int device = 0;
  hipStream_t st = nullptr, st2 = nullptr;   // st2: the bias filter of the next batch beside the decoder of this one
  // st_hi: a stream of the highest priority that the LOAD stage's entry points swap in for `st` (LoadPriority below).  Several contexts
  // share a GPU in a streaming run: a chunk's packing / hashing / grouping kernels are milliseconds of work that otherwise wait in line
  // behind the 20-ms launches of the chunks being searched (round 5: a chunk resident 0.9 s after its text was there, 0.3 s of it a
  // profile upload's synchronisation, 0.26 s a dereplication that takes 0.06 on an idle device)
  hipStream_t st_hi = nullptr;
  hipStream_t st3 = nullptr; hipEvent_t ev_s3a = nullptr, ev_s3b = nullptr;   // st3: every other batch of a shared MSV filter (their launch tails overlap)
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  // the MSV filter of chunk c + 1 runs on st2 beside the domain stage of chunk c (latency-bound kernels that leave the vector
  // ALUs idle): ev_msv0/1 bracket it; msv_pre_u0 = the chunk it was launched for (-1: none)
  hipEvent_t ev_msv0 = nullptr, ev_msv1 = nullptr, ev_c = nullptr;
  int64_t msv_pre_u0 = -1, next_u0 = -1; int32_t next_U = 0;
  mutable std::string err;
  void set_error(const std::string &m) const { err = m; }
  itsx_stats stats{};

  // ---- profiles
  std::vector<HostProfile> profs;
  int P = 0, G = 0;
  DBuf<DevProfile> d_prof;
  DBuf<uint32_t> d_etab;
  DBuf<int32_t> d_pbias, d_ptec, d_ptbm;
  DBuf<float> d_rtab, d_entab;             // k_bwd_bound's table; the folded emission odds by node (round 6: two-sided sharing)
  DBuf<ChainRec> sh_chain, sh_bchain;      // the chains' records by processing position (Forward / Backward)
  DBuf<float> d_flogsum; DBuf<LogTab> d_logtab; DBuf<float> d_btab; bool bound_fold = false;   // (the bound kernel's table, and whether it is the folded one)
  std::vector<char> generic_q;          // per profile: needs the runtime-Q kernels

  // ---- reads
  int64_t N = 0;
  itsx_io::Text h_bases;                 // original text (rep.fa keeps the input's case); not zero-filled when it grows
  const char *bases_view = "";           // = h_bases.data(), or the caller's buffer after itsx_set_reads_view
  const uint8_t *dev_bases = nullptr;    // after itsx_set_reads_device: the caller's device buffer (bases_view is fetched on demand)
  DBuf<uint8_t> d_merged_text;           // after a merge-and-load: the gathered text dev_bases points at, kept until the host has fetched it or the next read set
  static constexpr int NSTAGE = 3;       // pinned / device staging of the hand-over (pack_and_upload)
  void *stage_pin[NSTAGE] = {nullptr, nullptr, nullptr}; DBuf<uint8_t> stage_dev[NSTAGE]; hipEvent_t stage_ev[NSTAGE] = {nullptr, nullptr, nullptr}; size_t stage_cap = 0;
  DBuf<int64_t> w_pk_off; DBuf<int8_t> w_pk_lut; DBuf<int32_t> w_pk_excnt, w_pk_exstart, w_pk_tmp; DBuf<long long> w_pk_bad;
  std::vector<int64_t> h_off;
  NameList h_names;
  std::vector<int64_t> h_woff;           // word offset of each read (the words themselves and the exceptions live on the device only)
  std::vector<int32_t> h_len;
  DBuf<uint32_t> d_words, d_exc;
  DBuf<int64_t> d_woff, d_excoff;
  DBuf<int32_t> d_len;
  ReadsDev rd{};
  int Lmax = 0;
  // per-sample batching: S samples share the context; reads group only within their sample and
  // hmmsearch's domZ is kept per (sample, profile)
  int32_t S = 1, sel_sample = -1;
  std::vector<int32_t> h_sample, h_usample;          // per read / per unique; empty when S == 1
  DBuf<int32_t> d_sample, d_usample;
  const int32_t *dev_sample() const { return S > 1 ? d_sample.p : nullptr; }
  const int32_t *dev_usample() const { return S > 1 ? d_usample.p : nullptr; }
  int32_t usample(int64_t u) const { return S > 1 ? h_usample[(size_t)u] : 0; }
  // sample sharing (itsx_set_sample_sharing; k_derep.hip: k_class_*, k_expand_*): a full-rows search of S > 1 samples scores one holder
  // per score class (the uniques of all samples whose representatives are one string in one orientation) and copies its rows to the
  // other members.  sc: the last search's figures (all zero when the mode did not apply); sc_*: the classes on the device, rebuilt
  // by every search that shares (class_of [U], holder [C], the members as a CSR list: off [C + 1], members [U] in rising index)
  bool share_samples = false;
  // the same for the compact and lazy rows modes (itsx_set_sample_sharing_lazy): the chunk loops walk the holders, the members'
  // reported targets are counted from each chunk's scratch rows before compaction (sc_count_members, set while the holders are
  // walked: domain_pipeline), the kept rows are copied afterwards.  shared_lazy: the last search was such a one, so itsx_lazy_complete
  // walks h_sorted_searched again and expands the segments past sc_segs_done
  bool share_samples_lazy = false, sc_count_members = false, shared_lazy = false; size_t sc_segs_done = 0;
  bool active_narrowed = false;          // the CALLER chose the active uniques (itsx_set_active_uniques): the mode leaves them alone
  struct SampleSharing { int64_t n_classes = 0, n_shared = 0, n_expanded = 0; float ms_classes = 0, ms_expand = 0; } sc;
  // the list the last search walked when it was the holders' (PairRec::useq indexes it: append_traces), and whether the members'
  // pair traces have been made from their holders' yet (fetch_traces)
  bool searched_holders = false, trace_members_done = false; std::vector<int32_t> h_sorted_searched;
  DBuf<int32_t> sc_class_of, sc_holder, sc_off, sc_members, sc_members_in, sc_holder_of, sc_is_holder, sc_rank, sc_scan, sc_cnt, sc_pos;
  DBuf<unsigned long long> sc_keys, sc_keys_in; DBuf<uint8_t> sc_sort;
  double slab_gb = 0.0;                  // HBM budget for per-batch DP slabs

  // ---- what the context holds: one ladder, every level standing on the ones below it.  ST_GROUPED: a dereplication or a clustering is
  // in place; ST_SEARCHED: the rows of a search (or of itsx_debug_set_domains); ST_FINAL: itsx_search_finalize has decided them.
  // The stage rises through StageTxn::commit (below the struct) and falls through fall_to alone.
  enum Stage { ST_NONE, ST_READS, ST_GROUPED, ST_SEARCHED, ST_FINAL };
  Stage stage{ST_NONE};
  bool grouped() const { return stage >= ST_GROUPED; }
  bool searched() const { return stage >= ST_SEARCHED; }
  bool finalized() const { return stage >= ST_FINAL; }
  // Down to s at most, and whatever is attached to a level above s goes -- also when the stage is there already: a rebuild that failed
  // half way may have attached something.  What stays: the buffers themselves; thr_memo (it belongs to the profiles: install_profiles);
  // prev_* (search_active reads the last search's chunking at its next call); have_orient_db (the database is not the read set's);
  // the samples of the reads (h_sample, S: a new read set makes itself one sample, orient_apply_strands compacts them)
  void fall_to(Stage s)
  {
    if (s < ST_FINAL) { drop_alignments(); h_dom.clear(); }
    if (s < ST_SEARCHED) {
      h_trace.clear(); trace_sorted = trace_members_done = searched_holders = shared_lazy = false; sc = SampleSharing{};
      topup.valid = topup.list_live = false; injected = domz_on_device = domz_exchanged = false; lazy_pending = 0; lazy_pending_prof.clear();
    }
    if (s < ST_GROUPED) { clustered = false; drop_cigars(); order_cache_ok = false; h_usample.clear(); active_narrowed = false; }
    if (s < ST_READS) { rec.drop(); prec.drop(); ft.have = false; dn.have = false; }
    if (stage > s) stage = s;
  }

  // ---- derep
  std::vector<int32_t> order_cache; bool order_cache_ok = false;      // cluster_order() of the current dereplication (uc.txt and rep.fa both ask)
  int derep_strand_both = 1;             // how the last itsx_derep / itsx_cluster matched (the cross-shard keys follow it)
  int32_t U = 0;
  int32_t U_active = 0;                  // uniques this context scores (all of them unless itsx_set_active_uniques narrowed it)
  DBuf<int32_t> d_rep_of, d_uniq_of, d_seed_read, d_abund, d_sorted_uniq, d_ulen;
  DBuf<int8_t> d_strand;
  std::vector<int32_t> h_rep_of, h_uniq_of, h_seed_read, h_abund, h_sorted_uniq;
  std::vector<int8_t> h_strand;
  DBuf<uint32_t> d_orient_db; bool have_orient_db = false;   // f4: the orientation database's 12-mer bitmap
  DBuf<uint32_t> w_orient_tab; DBuf<int32_t> w_orient_list;  // f4: the long reads' word sets (k_orient_long: empty between calls) and their work list
  std::vector<int32_t> h_orient_longs;                        // (the work list on the host)
  bool clustered = false;                // last grouping came from itsx_cluster at id < 1 (uc rows carry identities)
  std::vector<double> h_pct;             // per read: identity of its H row, -1 for centroids / dropped reads
  std::vector<int32_t> h_order;          // kept reads in processing (label) order
  // itsx_align_clusters: the run-length alignment of every member with its centroid (uc column 8), read r's text at
  // h_cg_text[h_cg_off[r], h_cg_off[r + 1]) (empty: a centroid or a dropped read); whatever changes the clustering drops them
  bool have_cigar = false; std::vector<int64_t> h_cg_off; std::string h_cg_text;
  void drop_cigars() { have_cigar = false; std::vector<int64_t>().swap(h_cg_off); std::string().swap(h_cg_text); }
  bool cigars_live() const { return have_cigar && grouped() && clustered; }

  // ---- search
  bool injected = false;                 // the row table came from itsx_debug_set_domains, not from a search: nothing can be evaluated again
  double T = 10.0;
  int64_t npairs_padded = 0;
  DBuf<PairRec> d_pairs;
  DBuf<PairOut> d_pout;
  DBuf<RegionRec> d_regions;
  DBuf<RegionOut> d_rout;
  DBuf<int64_t> d_pair_region0;
  DBuf<int32_t> d_upos;                  // region -> index of its (shared) result
  DBuf<RegionRec> d_ulist;               // distinct envelopes, grouped by profile
  std::vector<std::unique_ptr<DBuf<itsx_domain>>> dom_bufs;   // one segment per chunk of uniques
  std::vector<int64_t> dom_n;            // padded rows in each segment
  int64_t pair_budget = 0; int32_t trace_u0 = 0; int n_chunks = 0; bool keep_trace = false, trace_sorted = false;
  DBuf<int16_t> d_vtab; DBuf<VitOut> d_vit; bool have_vit = false; double F2 = 1e-6;     // Viterbi filter (F2 < F1 only)
  DBuf<int32_t> d_domz32;
  DBuf<int64_t> d_domz64; bool domz_on_device = false;     // itsx_domz_device: the caller reduces the counters where they are
  // ITSX_COMPACT_ROWS=1: a chunk's domain rows live in w_domscratch (reused by every chunk) and only the rows that can still
  // win the argmax move to dom_bufs[chunk] (k_compact_*): 80 B x ~2 rows per representative instead of x ~130
  bool compact_rows = false; double compact_zmax = 1e9, compact_dome_min = 1e-2, compact_lnp = 0; int compact_ncls = 0;
  DBuf<itsx_domain> w_domscratch; DBuf<int8_t> w_cls; DBuf<unsigned long long> w_bestc; DBuf<int32_t> w_keep, w_keeppos, w_keeptmp;
  int64_t rows_before_compaction = 0;
  // rows mode (itsx_set_rows_mode / ITSX_ROWS): 0 every domain row stays resident (domtbl.txt), 1 compact, 2 lazy (k_lazy.hip)
  int rows_mode = -1;                    // -1: from the environment at every search
  bool lazy = false;                     // this search runs the lazy domain stage
  bool domz_exchanged = false;           // the caller moved domZ between search and finalize (a multi-rank driver): finalize never re-runs on its own
  int64_t lazy_pending = 0;              // undecided rows that could change a result, after the last lazy finalize
  double sF1 = 1e-6, sF3 = 1e-6;         // the last search's thresholds (finalize may have to repeat it in full)
  std::vector<int64_t> domz_ub;          // [S][P] pairs past the MSV filter: an upper bound of hmmsearch's domZ
  std::vector<int64_t> domz_loc, domz_ub_loc;   // this context's own counters (domz / domz_ub hold what finalize uses: the same, or the ranks' sums)
  bool completing = false;               // itsx_lazy_complete: every pair of the profiles in plist goes through the domain pipeline
  std::vector<int32_t> h_plist; DBuf<int32_t> d_plist;
  int64_t s_Uc = 0; int s_Lcap = 0;       // the last search's chunk size and length cap (the completion walks the same chunks)
  DBuf<float> l_fb; DBuf<uint32_t> l_b10, l_thr; DBuf<uint8_t> l_done; DBuf<unsigned long long> l_smask; DBuf<int32_t> l_scnt, l_spos, l_scan, l_has; DBuf<unsigned long long> l_gtop, l_sure;
  DBuf<PairRec> l_pairs; DBuf<int64_t> l_seg, l_zub; DBuf<int32_t> l_pflag; DBuf<uint8_t> l_uflag; bool partial_coords = false; bool kept_rows = false; std::vector<int32_t> lazy_pending_prof;
  std::vector<uint16_t> thr_memo; std::vector<char> thr_memo_have; double thr_memo_F1 = -1.0; int thr_memo_Ppad = 0;   // MSV thresholds by length, kept between searches
  DBuf<int32_t> w_coords4; DBuf<int64_t> w_keys128; DBuf<uint64_t> w_hf1, w_hr1;
  std::vector<int32_t> h_sorted_active;  // the length-sorted list the HMM stages walk (= h_sorted_uniq unless itsx_set_active_uniques narrowed it)
  DBuf<LenTables> d_lt;
  std::vector<int64_t> domz;
  std::vector<itsx_domain> h_dom;        // valid rows, domtblout order
  // itsx_align_domains: the alignments of the reported rows of the current finalize, ordered by (profile, representative, domain) for
  // the lookup of itsx_get_alignments / itsx_write_domtbl; whatever changes the rows or their dom_reported drops them (drop_alignments)
  struct AliRow { int32_t prof, dom_idx; int64_t rep; itsx_alignment a; };
  bool have_ali = false; std::vector<AliRow> h_ali;
  void drop_alignments() { have_ali = false; std::vector<AliRow>().swap(h_ali); }
  bool alignments_live() const { return have_ali && finalized(); }
  DBuf<PairRec> w_al_pairs; DBuf<RegionRec> w_al_regions; DBuf<RegionOut> w_al_rout; DBuf<int32_t> w_al_rep; DBuf<WaveDesc> w_al_waves; DBuf<itsx_alignment> w_al_out;
  std::vector<itsx_pairtrace> h_trace;

  // ---- persistent work buffers (see DBuf)
  DBuf<uint64_t> w_hf, w_hr; DBuf<unsigned long long> w_keys; DBuf<int32_t> w_vals, w_is_seed, w_seed_rank, w_scan_tmp, w_hist, w_cursor, w_tmp2;
  DBuf<uint32_t> w_slot_of; DBuf<unsigned int> w_ncoll;
  DBuf<uint16_t> w_thr, w_res; DBuf<int32_t> w_tjb, w_cnt, w_total, w_rows, w_rcnt, w_rpref, w_scan2, w_b, w_rrows;
  DBuf<int64_t> w_seg_start, w_idx, w_rseg, w_dz, w_counters, w_useg;
  DBuf<int32_t> w_rrep, w_ruq, w_rurank;
  DBuf<WaveDesc> w_waves, w_rw; DBuf<RegionRec> w_raw; DBuf<float> w_slab, w_eslab;
  DBuf<int32_t> w_mrcnt, w_mroff, w_mrlen, w_mrloff, w_mrrows, w_mrulist, w_mrulist2, w_mru; DBuf<int64_t> w_mrrowoff; DBuf<MrRec> w_mr; DBuf<MrOut> w_mrout; DBuf<int64_t> w_n2off; DBuf<float> w_n2sc, w_mrslab;
  DBuf<uint8_t> w_mrscratch; DBuf<WaveDesc> w_mrwaves;
  // regions past a pair's MAXDOM slots (k_decode appends; ordered by (pair, k) afterwards) and the ensemble stage's overflow path
  DBuf<RegionRec> w_pool, w_pool_sorted; DBuf<int32_t> w_pool_k; DBuf<unsigned long long> w_pool_n, w_pool_key; int64_t pool_cap = 0;
  DBuf<int32_t> w_mrsel; DBuf<int64_t> w_mrselrow; DBuf<MrBig> w_mrbig; DBuf<uint8_t> w_mrarena; DBuf<int32_t> w_mrenv; DBuf<WaveDesc> w_mrbigwaves;
  DBuf<int32_t> w_cl, w_cr;
  DBuf<int8_t> w_side; DBuf<unsigned long long> w_bl, w_br; DBuf<int32_t> w_uind, w_us, w_ue, w_ut, w_rs, w_re, w_rt, w_ri, w_uflag;

  // ---- prefix sharing (k_share.hip), rebuilt by every itsx_search: the prefix tree of the active uniques by sorted position s (sh_*_s)
  // and by processing position k = (batch, depth, s) (sh_dev); a batch is a range of s whose saved row states fit the slot budget
  struct ShareBatch { int32_t k0, k1; int64_t node0, nnodes; int32_t nsplit; int64_t gnode0, gnnodes; };   // nsplit > 1: the profiles in that many ranges, one after the other; g*: the batch's saved Backward states
  bool share_on = false; int share_B = 32, share_logB = 5, share_maxd = 0;
  DBuf<unsigned long long> sh_tab, sh_mask_s, sh_mask, sh_counters, msv_xb; DBuf<uint8_t> sh_depth_s, sh_depth;
  DBuf<int32_t> sh_src, sh_parent_s, sh_parent, sh_nn_s, sh_nn, sh_node0_s, sh_node0, sh_order, sh_ulen, sh_uorder, sh_inv, sh_flag, sh_pos, sh_bstart, sh_cursor, sh_segk, sh_scan, sh_cuts;
  std::vector<ShareBatch> sh_batches; std::vector<int32_t> sh_segk_h;            // [batch][SHARE_SEGS]
  DBuf<uint4> sh_mgslots; size_t sh_mgslots_half = 0;        // the MSV filter's saved Backward states (two-sided sharing)
  DBuf<uint4> sh_mslots; size_t sh_mslots_half = 0, sh_fslots_half = 0; DBuf<uint32_t> sh_pass, sh_need; DBuf<int32_t> sh_real, sh_segflat, sh_segdepth, sh_wc, sh_woff; DBuf<int64_t> sh_bnd;
  DBuf<uint16_t> sh_res_chk; DBuf<float> sh_fb_chk;
  ShareDev sh_dev{};
  // two-sided sharing (round 6): the suffix tree by s (sh_r*_s), the joins, the Backward chains by backward position kb (sh_bdev), their
  // batches' first positions (sh_bsegk_h), the slots of the saved Backward states behind the Forward ones in the DP slab
  std::string switches_at_search;
  // the top-up round of itsx_search_finalize (round 6): the last search's pair list, while it is still in the buffers (one chunk, one sample)
  struct TopUp { bool valid = false, list_live = false /* d_pairs, l_fb, l_b10 and l_done still hold the list (itsx_debug_lazy_pairs) */; int64_t NP = 0; std::vector<int64_t> seg_start; std::vector<int32_t> total; int32_t u0 = 0, Uc = 0; } topup;
  DBuf<unsigned long long> l_zneed, l_zsplit, l_tcnt; DBuf<int32_t> l_slot, l_pslot; DBuf<uint32_t> l_cut;
  // the count-only top-up round: each pair of its list's index in the search's list, the deferred pairs' bits and their number; the two
  // counters of the last search (itsx_topup_counters)
  DBuf<int32_t> l_src; DBuf<unsigned long long> l_dmask, l_defn, l_tcnt2;
  int64_t n_topup_deferred = 0, n_topup_ensemble = 0, topup_deferred_live = 0 /* deferred by the last count-only round and not evaluated since */;
  std::vector<int64_t> topup_defp;                                   // [P] deferred pairs per profile
  std::vector<int32_t> topup_profs, topup_partial;                   // the profiles of the last top-up round; those of them that took their `need` pairs instead of all (ITSX_LAZY_TOPUP_ALL=2)
  std::vector<unsigned long long> h_zneed;
  bool prev_lazy = false; int prev_P = 0; int64_t prev_U = 0, prev_Uc = 0;      // the last search's chunking (itsx_search)
  std::vector<int32_t> h_merge_index;      // per pair of the last merge-and-load: its merged read, -1 = not merged
  bool merge_join = false;                 // itsx_set_merge_join: pairs rejected for want of an overlap (reason 1, 3, 5) are joined and kept
  std::vector<int8_t> h_merge_join;        // per pair of the last merge call (itsx_merge_pairs_files included): 1 = its read is a joined one (all 0 with the setting off)
  int64_t pack_exc_hint = 0;               // non-ACGT symbols the next pack_and_upload is known to meet (a joined read's eight N); taken once
  // ---- the records of the read set (itsx_keep_records; consumer: itsx_write_trimmed_samples): what a FASTQ record needs beyond the
  // packed words -- ASCII bases as in the input, qualities, whole title lines -- one owned copy, dropped with the read set
  bool keep_records = false;
  struct Records {
    bool have = false;
    DBuf<uint8_t> seq, qual, titles;       // bases / qualities of read r at off[r]; its title line ('@' included, no newline) at toff[r]
    const uint8_t *seq_p = nullptr;        // the bases plane: seq.p, or after a merge d_merged_text.p (that text IS the plane)
    DBuf<int64_t> off, toff;               // [N + 1]
    NameList h_titles;                     // the titles on the host (itsx_orient_apply compacts them)
    void drop() { have = false; seq_p = nullptr; seq.release(); qual.release(); titles.release(); off.release(); toff.release(); h_titles.clear(); }
  } rec;
  // ---- the ORIGINAL pair records of a merge-and-load (itsx_keep_pair_records; consumer: itsx_write_trimmed_paired_samples): R1's and
  // R2's bases and qualities as the merge kernel read them (taken over from merge_core, not uploaded again), their whole title lines,
  // and per pair the read whose coordinates it is sliced with.  Pairs are sample-contiguous (pstart).  Dropped with the read set.
  bool keep_pair_records = false;
  struct PairRecords {
    bool have = false; int64_t n = 0;
    DBuf<uint8_t> s1, q1, t1, s2, q2, t2;  // bases / qualities of pair p's R1 at o1[p], its title line at to1[p]; R2 alike
    DBuf<int64_t> o1, to1, o2, to2;        // [n + 1]
    DBuf<int32_t> pair_read;               // [n] the read NAMED by R1's identifier among the sample's merged reads (the first of equal labels), -1: none
    std::vector<int64_t> pstart;           // [S + 1] sample s's pairs
    void drop()
    {
      have = false; n = 0; pstart.clear(); pair_read.release();
      s1.release(); q1.release(); t1.release(); s2.release(); q2.release(); t2.release(); o1.release(); to1.release(); o2.release(); to2.release();
    }
  } prec;
  DBuf<TrimRec> w_trec2; DBuf<int32_t> w_ttlen;          // itsx_write_trimmed_paired_samples (beside the buffers below)
  DBuf<TrimRec> w_trec; DBuf<int64_t> w_tcnt, w_ttot, w_tblk, w_tfirst, w_tbounds; DBuf<int32_t> w_tstart, w_tstop; DBuf<uint32_t> w_tout;   // itsx_write_trimmed_samples
  // ---- the feature table of the trimmed regions (itsx_trimmed_table; k_ftable.hip): the last call's table in its order, kept until the next
  // call or the next read set (the sequences were cut from this read set's words); the rest is that call's scratch
  struct FeatureTable {
    bool have = false; int64_t n = 0, nc = 0; int32_t F = 0, E = 0, S = 1; int64_t text_bytes = 0;   // (S: the samples its cells were counted over)
    DBuf<int32_t> feat_len, feat_total, feat_first, row_off, entry_sample, entry_count, feature_of_read; DBuf<uint32_t> text; std::vector<int64_t> h_seq_off;
    DBuf<int32_t> start, stop, vals, feature_read, ehead, epos, fhead, fpos, ent_start, ent_sample, ent_feat, f_ent0, f_pos0, f_first, hold_f, ovals, ovals2,
        rank_of, nent, scan;
    DBuf<unsigned long long> keys, counters, pair_keys, pair_sorted, okeys, okeys2; DBuf<uint64_t> hash; DBuf<uint32_t> slot_of; DBuf<int64_t> seq_off; DBuf<uint8_t> sort_tmp;
  } ft;
  // ---- the table above denoised into ZOTUs (itsx_denoise_table; k_denoise.hip): the last call's result, beside the table it was made of --
  // whatever drops ft drops it, and so does the next itsx_trimmed_table or itsx_denoise_table; the rest is that call's scratch
  struct Denoised {
    bool have = false; int32_t F = 0, Z = 0, E = 0; int64_t dropped = 0, pairs = 0, skip_skew = 0, skip_len = 0, columns = 0; int32_t levels = 0;
    DBuf<int32_t> cent, zotu_of, dist_of, z_row_off, z_total, z_entry_sample, z_entry_count;
    DBuf<int32_t> lv, nlev, ncent, flag, pos, vals, vals2, head, hpos, csum, run_start, scan; DBuf<double> skew;
    DBuf<unsigned long long> keys, keys2, counters; DBuf<uint8_t> sort_tmp;
  } dn;
  DBuf<DeflateBlock> w_dblk; DBuf<uint32_t> w_dtok, w_dtext; DBuf<uint8_t> w_dslots, w_dpacked; DBuf<int32_t> w_dsizes; DBuf<int64_t> w_ddst;   // deflate_ranges
  // a streamed writer's device path (twdev_*, for itsx_twriter_set_device): a unit's raw text, its line index and the plan's scratch
  // (records, output text and deflate scratch are the batch writers' buffers above); tw_mu serialises the writers that share the context
  DBuf<uint8_t> tw_raw; DBuf<int32_t> tw_ls, tw_le; DBuf<int64_t> tw_lblk, tw_qsrc, tw_info;
  DBuf<int8_t> tw_strand; DBuf<uint8_t> tw_comp; bool tw_comp_set = false;      // a unit's strands (itsx_twriter_strands) and iupac.h's complement table
  std::mutex tw_mu; bool tw_failed = false; float tw_ms_deflate = 0;
  // the device inflate (inflate_file): the uploaded file, the candidate scan's tiles and list, the members and their statuses, and the
  // text of the last successful call (inf_len bytes; -1: none).  inf_mu serialises the loader threads that share the context.
  DBuf<uint8_t> inf_gz, inf_text; DBuf<int64_t> inf_counts, inf_base, inf_list, inf_where; DBuf<InflateMember> inf_mem; DBuf<int32_t> inf_status;
  int64_t inf_len = -1, n_inf_device = 0, n_inf_declined = 0; bool device_inflate = false; std::mutex inf_mu;
  // the device parse (parse_text_device): a text uploaded for it, the line index and the plan's scratch, the last text's offsets, and
  // the planes -- of the last successful itsx_parse_device (ps_n records; -1: none), or of a load under way, whose bases plane then
  // becomes d_merged_text (the read set's text on the device, as after a merge).  ps_mu serialises the callers that share the context.
  DBuf<uint8_t> ps_text, ps_seq, ps_qual, ps_titles; DBuf<int64_t> ps_lblk, ps_nl, ps_blk, ps_off, ps_toff, ps_info;
  int64_t ps_n = -1, ps_nb = 0, ps_nt = 0, n_parse_device = 0, n_parse_declined = 0; bool ps_qual_kept = false, device_parse = false; std::mutex ps_mu;
  // a PAIR of texts needs the plane set once per side (itsx_parse_pairs_device, merge_pairs_load_device): a side's planes are moved into
  // ps_seq / ps_qual / ps_titles while its texts are parsed and back here afterwards.  off / toff: the offsets of the last successful
  // itsx_parse_pairs_device (pp_n pairs; -1: none); pp_info: k_fastq_pairs' two words
  struct PairSide { DBuf<uint8_t> seq, qual, titles; DBuf<int64_t> off, toff; int64_t nb = 0, nt = 0; } pp[2];
  int64_t pp_n = -1; DBuf<unsigned long long> pp_info;
  bool two_on = false; int share_maxrd = 0; int32_t Ub = 0; size_t sh_gslots_off = 0;
  DBuf<uint8_t> sh_rdepth_s, sh_rdepth; DBuf<unsigned long long> sh_rmask_s, sh_rmask, sh_keys, sh_keys2;
  DBuf<int32_t> sh_rparent_s, sh_rparent, sh_jlev_s, sh_jown_s, sh_endrow_s, sh_rsteps_s, sh_rnn_s, sh_rnode0_s, sh_endrow, sh_jlev, sh_jsrc, sh_jownb;
  DBuf<int32_t> sh_border_s, sh_invb, sh_bsegk, sh_rnn, sh_rnode0, sh_border, sh_bulen, sh_rsrc, sh_bsteps, sh_vals;
  DBuf<uint8_t> sh_sorttmp;
  std::vector<int32_t> sh_bsegk_h;
  BShareDev sh_bdev{};
  DBuf<uint32_t> sh_needb; DBuf<uint16_t> sh_resb; DBuf<int32_t> sh_cntb, sh_totalb, sh_realb, sh_bsegflat, sh_bsegdepth, sh_bwc, sh_bwoff; DBuf<int64_t> sh_bbnd, sh_bseg_start;
  DBuf<PairRec> sh_bpairs; DBuf<WaveDesc> sh_bwaves;
};

// An entry point that rebuilds a level of the ladder: the context falls below that level at once and rises to it through commit(), the last
// statement of the success path.  Every early return leaves it below (at `failed`, where that is lower than where the work starts: itsx_lazy_complete).
struct StageTxn {
  itsx_ctx *c; itsx_ctx::Stage failed; bool done = false;
  StageTxn(itsx_ctx *ctx, itsx_ctx::Stage below, itsx_ctx::Stage failed_) : c(ctx), failed(failed_) { c->fall_to(below); }
  StageTxn(itsx_ctx *ctx, itsx_ctx::Stage below) : StageTxn(ctx, below, below) {}
  StageTxn(const StageTxn &) = delete;
  void commit(itsx_ctx::Stage s) { c->stage = s; done = true; }
  ~StageTxn() { if (!done) c->fall_to(failed); }
};

#define CTXCHK(c)                                   \
  if (!(c)) return ITSX_E_ARG;
#define SET_ERR(ctx, code, msg) do { (ctx)->set_error(msg); return (code); } while (0)
#undef HIPCHK
#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e__ = (expr);                                                              \
    if (e__ != hipSuccess) { ctx->set_error(std::string(#expr) + ": " + hipGetErrorString(e__)); return ITSX_E_DEVICE; } \
  } while (0)

template <class T> static hipError_t upload(DBuf<T> &d, const std::vector<T> &h, hipStream_t st, size_t min_elems = 1)
{
  hipError_t e = d.alloc(std::max(h.size(), min_elems));
  if (e != hipSuccess) return e;
  if (h.empty()) return hipSuccess;
  return hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
}

// kernel timers that do not stall the stream: event pairs are recorded around launches and read back once,
// after the whole stage has been enqueued
struct LazyTimers {
  struct Rec { hipEvent_t a, b; float *acc; };
  std::vector<Rec> recs; hipStream_t st;
  explicit LazyTimers(hipStream_t s) : st(s) {}
  size_t begin(float *acc) { Rec r; (void)hipEventCreate(&r.a); (void)hipEventCreate(&r.b); r.acc = acc; (void)hipEventRecord(r.a, st); recs.push_back(r); return recs.size() - 1; }
  void end(size_t i) { (void)hipEventRecord(recs[i].b, st); }
  void collect()
  {
    for (auto &r : recs) { (void)hipEventSynchronize(r.b); float ms = 0; (void)hipEventElapsedTime(&ms, r.a, r.b); *r.acc += ms; (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    recs.clear();
  }
  ~LazyTimers() { collect(); }
};

struct StageTimer {
  hipEvent_t a = nullptr, b = nullptr; hipStream_t st;
  explicit StageTimer(hipStream_t s) : st(s) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, st); }
  float stop() { (void)hipEventRecord(b, st); (void)hipEventSynchronize(b); float ms = 0; (void)hipEventElapsedTime(&ms, a, b); return ms; }
  ~StageTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

using itsx_io::on_threads;

extern "C" {

int itsx_abi_version(void) { return ITSX_ABI_VERSION; }

const char *itsx_last_error(const itsx_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// the load stage's work on the high-priority stream: swapped in for the call, waited for and swapped back at its end (everything after
// the call -- the search on `st` -- sees the load stage's results complete)
struct LoadPriority {
  itsx_ctx *c; bool on;
  explicit LoadPriority(itsx_ctx *ctx) : c(ctx), on(ctx && ctx->st_hi != nullptr) { if (on) std::swap(c->st, c->st_hi); }
  ~LoadPriority() { if (on) { (void)hipStreamSynchronize(c->st); std::swap(c->st, c->st_hi); } }
  LoadPriority(const LoadPriority &) = delete;
  LoadPriority &operator=(const LoadPriority &) = delete;
};

itsx_ctx *itsx_create(int device_id, int flags)
{
  (void)flags;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) { g_create_error = "no HIP device is visible (the engine has no CPU fallback)"; return nullptr; }
  if (device_id < 0 || device_id >= ndev) { g_create_error = "device ordinal out of range"; return nullptr; }
  e = hipSetDevice(device_id);
  if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return nullptr; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return nullptr; }
  if (std::string(prop.gcnArchName).compare(0, 6, "gfx950") != 0) {
    g_create_error = std::string("device is ") + prop.gcnArchName + "; this engine ships gfx950 code only";
    return nullptr;
  }
  itsx_ctx *ctx = new itsx_ctx();
  ctx->device = device_id;
  ctx->w_slab.pool_device = device_id;
  if (hipStreamCreate(&ctx->st) != hipSuccess) { g_create_error = "hipStreamCreate failed"; delete ctx; return nullptr; }
  if (!(sw_get("ITSX_LOAD_PRIORITY") && atoi(sw_get("ITSX_LOAD_PRIORITY")) == 0)) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || greatest == least ||
        hipStreamCreateWithPriority(&ctx->st_hi, hipStreamDefault, greatest) != hipSuccess) { (void)hipGetLastError(); ctx->st_hi = nullptr; }
  }
  // p7_FLogsum's table, built with libm exactly as hmmsearch builds it at start-up
  std::vector<float> tbl(16000);
  for (int i = 0; i < 16000; i++) tbl[i] = (float)log(1. + exp((double)-i / 1000.f));
  if (upload(ctx->d_flogsum, tbl, ctx->st) != hipSuccess) { g_create_error = "device allocation failed"; delete ctx; return nullptr; }
  std::vector<LogTab> lt(LOGTAB_N);
  build_logtab(lt.data());
  if (upload(ctx->d_logtab, lt, ctx->st) != hipSuccess) { g_create_error = "device allocation failed"; delete ctx; return nullptr; }
  (void)hipStreamSynchronize(ctx->st);
  { std::lock_guard<std::mutex> g(g_pool_mu); g_live_contexts++; }      // (only a context that itsx_destroy will see is counted)
  return ctx;
}

void itsx_destroy(itsx_ctx *ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->st);
  if (ctx->st3) { (void)hipStreamSynchronize(ctx->st3); (void)hipStreamDestroy(ctx->st3); (void)hipEventDestroy(ctx->ev_s3a); (void)hipEventDestroy(ctx->ev_s3b); }
  if (ctx->st2) { (void)hipStreamSynchronize(ctx->st2); (void)hipStreamDestroy(ctx->st2); (void)hipEventDestroy(ctx->ev_a); (void)hipEventDestroy(ctx->ev_b);
                  if (ctx->ev_msv0) { (void)hipEventDestroy(ctx->ev_msv0); (void)hipEventDestroy(ctx->ev_msv1); (void)hipEventDestroy(ctx->ev_c); } }
  (void)hipStreamDestroy(ctx->st);
  if (ctx->st_hi) { (void)hipStreamSynchronize(ctx->st_hi); (void)hipStreamDestroy(ctx->st_hi); }
  for (int k = 0; k < itsx_ctx::NSTAGE; k++) { if (ctx->stage_pin[k]) (void)hipHostFree(ctx->stage_pin[k]); if (ctx->stage_ev[k]) (void)hipEventDestroy(ctx->stage_ev[k]); }
  delete ctx;
  grave_flush();                         // this context's buffers, and whatever the others have given up meanwhile
  bool last = false;
  { std::lock_guard<std::mutex> g(g_pool_mu); last = --g_live_contexts <= 0; }
  if (last) pool_flush();
}

// A context that will not search again soon (a streamed file's chunk after its search; results, row lists and everything a finalize or
// a completion needs stay) hands its DP slab to the next context on the device.  Safe: its streams are drained first.
int itsx_release_scratch(itsx_ctx *ctx)
{
  CTXCHK(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->st));
  if (ctx->st2) HIPCHK(hipStreamSynchronize(ctx->st2));
  if (ctx->st3) HIPCHK(hipStreamSynchronize(ctx->st3));
  if (ctx->w_slab.p) { pool_put(ctx->w_slab.p, ctx->w_slab.cap * sizeof(float), ctx->device); ctx->w_slab.p = nullptr; ctx->w_slab.n = ctx->w_slab.cap = 0; }
  return ITSX_OK;
}

// ------------------------------------------------------------------------------ profiles
static int install_profiles(itsx_ctx *ctx, std::vector<HostProfile> &pv, int *n_profiles)
{
  for (auto &p : pv) {
    if (p.M > MMAX || p.Q > QMAX) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "model '" + p.name + "' has more than 46 nodes; the device kernels hold at most 46");
    if (p.base_b + p.bias_b >= 255) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "model '" + p.name + "': MSV bias too large");
  }
  ctx->thr_memo.clear(); ctx->thr_memo_have.clear(); ctx->thr_memo_F1 = -1.0;      // (the MSV thresholds kept between searches belong to the old profiles)
  ctx->fall_to(itsx_ctx::ST_GROUPED);                    // ... and so do a search's rows, from here on whether the new ones arrive or not
  HIPCHK(hipSetDevice(ctx->device));
  LoadPriority load_priority(ctx);
  ctx->profs = std::move(pv);
  const int P = (int)ctx->profs.size();
  ctx->P = P; ctx->G = (P + 63) / 64;
  const int Ppad = ctx->G * 64;
  std::vector<DevProfile> dp(std::max(P, 1));
  ctx->generic_q.assign(P, 0);
  std::vector<uint32_t> etab((size_t)std::max(P, 1) * 16 * MSV_TW, 0);
  std::vector<int32_t> pb(std::max(Ppad, 64), 0), pt(std::max(Ppad, 64), 0), pm(std::max(Ppad, 64), 0);
  for (size_t i = 0; i < etab.size(); i++) etab[i] = 0xFF01FF01u;   // (0 - 255) as int16, twice: cells past M never rise above 0
  for (int i = 0; i < P; i++) {
    const HostProfile &h = ctx->profs[i];
    DevProfile &d = dp[i];
    memset(&d, 0, sizeof(d));
    for (int q = 0; q < h.Q; q++) {
      for (int t = 0; t < 7; t++) for (int z = 0; z < 4; z++) d.tf[(q * 8 + t) * 4 + z] = h.tfv[((size_t)q * 7 + t) * 4 + z];
      for (int z = 0; z < 4; z++) d.tf[(q * 8 + 7) * 4 + z] = h.tfv[((size_t)7 * h.Q + q) * 4 + z];
    }
    for (int k = 1; k <= 4 * h.Q; k++)            // the same transitions by node (slot k = z Q + q + 1 of the striped vectors)
      for (int t = 0; t < 8; t++) d.tfn[k * 8 + t] = d.tf[(((k - 1) % h.Q) * 8 + t) * 4 + (k - 1) / h.Q];
    for (int q = 0; q < h.Q; q++) {
      const int order[3] = {6, 5, 0};      // II MI BM of this group
      for (int k = 0; k < 3; k++) for (int z = 0; z < 4; z++) d.tb[(q * 6 + k) * 4 + z] = d.tf[(q * 8 + order[k]) * 4 + z];
      for (int k = 0; k < 3; k++)          // MM IM DM of the next group; group Q-1 wraps to group 0 shifted left by one lane
        for (int z = 0; z < 4; z++) {
          float v;
          if (q + 1 < h.Q) v = d.tf[((q + 1) * 8 + 1 + k) * 4 + z];
          else v = (z < 3) ? d.tf[(0 * 8 + 1 + k) * 4 + z + 1] : 0.0f;
          d.tb[(q * 6 + 3 + k) * 4 + z] = v;
        }
    }
    for (int x = 0; x < NCODE; x++)
      for (int q = 0; q < h.Q; q++) for (int z = 0; z < 4; z++) d.rf[(x * QMAX + q) * 4 + z] = h.rfv[((size_t)x * h.Q + q) * 4 + z];
    for (int x = 0; x < NCODE; x++) { d.feo[x * 2] = h.feo[x][0]; d.feo[x * 2 + 1] = h.feo[x][1]; }
    d.ft10 = h.ft10; d.ft11 = h.ft11; d.fpi0 = h.fpi0; d.fpi1 = h.fpi1;
    for (int k = 0; k < 6; k++) d.ev[k] = h.evparam[k];
    d.M = h.M; d.Q = h.Q;
    ctx->generic_q[i] = (h.Q != QMAX);
    for (int x = 0; x < NCODE; x++)
      for (int r = 0; r < MSV_REGS; r++) {
        uint32_t packed = 0;
        for (int half = 0; half < 2; half++) {
          const int k = half * MSV_REGS + r + 1;          // striped: register r = cells r and r + 23 (k_msv.hip)
          const int cost = (k <= h.M) ? h.rbv[(size_t)x * (h.M + 1) + k] : 255;
          const int16_t e = (int16_t)(h.bias_b - cost);
          packed |= (uint32_t)(uint16_t)e << (16 * half);
        }
        etab[((size_t)i * 16 + x) * MSV_TW + r] = packed;
      }
    pb[i] = h.bias_b; pt[i] = h.tec_b; pm[i] = h.tbm_b;
  }
  {   // Viterbi-filter word tables: per profile [8][47] transitions, [16][47] emissions
    std::vector<int16_t> vt((size_t)std::max(P, 1) * VIT_TAB, (int16_t)-32768);
    for (int i = 0; i < P; i++) {
      const HostProfile &h = ctx->profs[i];
      int16_t *t = vt.data() + (size_t)i * VIT_TAB;
      for (int k8 = 0; k8 < 8; k8++) for (int k = 0; k <= h.M; k++) t[k8 * (MMAX + 1) + k] = h.tww[(size_t)k8 * (h.M + 1) + k];
      for (int x = 0; x < NCODE; x++) for (int k = 0; k <= h.M; k++) t[(8 + x) * (MMAX + 1) + k] = h.rww[(size_t)x * (h.M + 1) + k];
    }
    HIPCHK(upload(ctx->d_vtab, vt, ctx->st));
  }
  {   // the bound kernel's transitions by pair of nodes (k_lazy.hip: k_fwd_bound), one 16-float record per step of its row loop
    // FOLD (k_lazy.hip): with H_k = 1 + t(D_k -> D_k+1) H_k+1 (what one unit of D_k adds to the row's E through itself and the deletes
    // after it), g_k = 1 + t(M_k -> D_k+1) H_k+1, s_1 = 1, s_k+1 = t(M_k -> D_k+1) / g_k, a_k = s_k t(D_k -> D_k+1) / s_k+1 the kernel
    // keeps M~_k = M_k g_k and D^_k = D_k / s_k:  D^_k+1 = D^_k a_k + M~_k,  E = sum of M~_k;  M -> M / I transitions divided by g_k, the D -> M
    // ones multiplied by s_k, the emission odds multiplied by g_k (in the kernel, from the table's last 48 floats); the insert cells likewise
    // divided by r_k = t(M_k -> I_k) / g_k (I^_k' = I^_k t(I_k -> I_k) + M~_k; the I -> M transitions multiplied by r_k).  Needs
    // t(M_k -> D_k+1) > 0 wherever the delete path goes on (every node hmmbuild writes; after the last node both are 0 and a_k = 0 ends the
    // chain); one profile without that and the whole set runs the plain recurrences (ITSX_BOUND_FOLD=0 does too).
    const int KK = 2 * BOUND_PAIRS;
    std::vector<std::vector<double>> G((size_t)P), SC((size_t)P), AA((size_t)P), RI((size_t)P);
    bool fold = !(sw_get("ITSX_BOUND_FOLD") && atoi(sw_get("ITSX_BOUND_FOLD")) == 0);
    for (int i = 0; i < P && fold; i++) {
      const DevProfile &d = dp[i];
      const int K = 4 * ctx->profs[i].Q;
      auto tn = [&](int k, int t) { return (k >= 1 && k <= K) ? (double)d.tfn[k * 8 + t] : 0.0; };
      std::vector<double> H((size_t)KK + 3, 1.0), &g = G[(size_t)i], &sc = SC[(size_t)i], &aa = AA[(size_t)i], &ri = RI[(size_t)i];
      g.assign((size_t)KK + 2, 1.0); sc.assign((size_t)KK + 3, 1.0); aa.assign((size_t)KK + 2, 0.0); ri.assign((size_t)KK + 2, 1.0);
      for (int k = KK; k >= 1; k--) H[(size_t)k] = 1.0 + tn(k, 7) * H[(size_t)k + 1];
      for (int k = 1; k <= KK; k++) g[(size_t)k] = 1.0 + tn(k, 4) * H[(size_t)k + 1];
      for (int k = 1; k <= KK; k++) {
        const double md = tn(k, 4), dd = tn(k, 7);
        if (md > 0.0) { sc[(size_t)k + 1] = md / g[(size_t)k]; aa[(size_t)k] = sc[(size_t)k] * dd / sc[(size_t)k + 1]; }
        else if (dd > 0.0 && k > 1) fold = false;          // a delete path that goes on past a node no match cell feeds: not foldable
        else { sc[(size_t)k + 1] = 1.0; aa[(size_t)k] = 0.0; }
        // (rescaling lets a row's cells reach ~1e21 -- 1e29 under ITSX_BOUND_RESCALE_EXP=28 -- before they are scaled back: the scaled cells
        // must stay far below FLT_MAX, 3.4e38)
        if (!(sc[(size_t)k + 1] > 1e-6 && sc[(size_t)k + 1] < 1e6 && aa[(size_t)k] < 1e6)) fold = false;
        // the insert cells by r_k = t(M_k -> I_k) / g_k: I^_k' = I^_k t(I_k -> I_k) + M~_k.  A node without M -> I must not use its insert cell at all
        const double mi = tn(k, 5);
        if (mi > 0.0) ri[(size_t)k] = mi / g[(size_t)k];
        else if (tn(k, 6) > 0.0 || tn(k + 1, 2) > 0.0) fold = false;
        else ri[(size_t)k] = 1.0;
        if (!(ri[(size_t)k] > 1e-6)) fold = false;
      }
    }
    ctx->bound_fold = fold;
    std::vector<float> bt((size_t)std::max(P, 1) * BOUND_TAB, 0.0f);
    for (int i = 0; i < P; i++) {
      const DevProfile &d = dp[i];
      const int K = 4 * ctx->profs[i].Q;                                      // slots of the striped layout (transitions beyond them: 0)
      auto tn = [&](int k, int t) { return (k >= 1 && k <= K) ? d.tfn[k * 8 + t] : 0.0f; };
      auto gk = [&](int k) { return fold && k >= 1 && k <= KK ? G[(size_t)i][(size_t)k] : 1.0; };
      auto sk = [&](int k) { return fold && k >= 1 && k <= KK + 1 ? SC[(size_t)i][(size_t)k] : 1.0; };
      auto rk = [&](int k) { return fold && k >= 1 && k <= KK ? RI[(size_t)i][(size_t)k] : 1.0; };
      // record j = what step j of the row loop reads: the chain of pair j (bm dd dd, md) and what pair j - 1's new cells leave for the next
      // row (mm im dm ii, mi)
      for (int j = 0; j <= BOUND_PAIRS; j++) {
        float *o = bt.data() + (size_t)i * BOUND_TAB + (size_t)j * 16;
        if (j > 0) {
          const int k1 = 2 * (j - 1) + 1, k2 = 2 * (j - 1) + 2;
          o[0] = (float)(tn(k1 + 1, 1) / gk(k1)); o[1] = (float)(tn(k2 + 1, 1) / gk(k2));      // M_k -> M_k+1 (tf stores it at the target node)
          o[2] = (float)(tn(k1 + 1, 2) * rk(k1)); o[3] = (float)(tn(k2 + 1, 2) * rk(k2));      // I_k -> M_k+1
          o[4] = (float)(tn(k1 + 1, 3) * sk(k1)); o[5] = (float)(tn(k2 + 1, 3) * sk(k2));      // D_k -> M_k+1
          o[6] = tn(k1, 6); o[7] = tn(k2, 6);                                                    // I_k -> I_k
          o[12] = (float)(tn(k1, 5) / gk(k1)); o[13] = (float)(tn(k2, 5) / gk(k2));            // M_k -> I_k (FOLD: not read)
        }
        if (j < BOUND_PAIRS) {
          const int k1 = 2 * j + 1, k2 = 2 * j + 2;
          o[8] = tn(k1, 0); o[9] = tn(k2, 0);              // B -> M_k
          if (fold) { o[10] = k1 > 1 ? (float)AA[(size_t)i][(size_t)k1 - 1] : 0.0f; o[11] = (float)AA[(size_t)i][(size_t)k1]; }
          else { o[10] = tn(k1 - 1, 7); o[11] = tn(k1, 7); }   // D_k1-1 -> D_k1 (0 before node 1), D_k1 -> D_k2
          o[14] = tn(k1, 4); o[15] = tn(k2, 4);            // M_k -> D_k+1 (FOLD: not read)
        }
      }
      float *gq = bt.data() + (size_t)i * BOUND_TAB + (size_t)(BOUND_PAIRS + 1) * 16;
      for (int k0 = 0; k0 < KK; k0++) gq[k0] = (float)gk(k0 + 1);
    }
    HIPCHK(upload(ctx->d_btab, bt, ctx->st));
    // k_bwd_bound (round 6) walks the same recurrences transposed: per pair of nodes (k1, k2) the folded M_k -> M_k+1, I_k -> M_k+1,
    // D_k -> M_k+1, I_k -> I_k, B -> M_k and D_k -> D_k+1 constants of the table above, by SOURCE node
    std::vector<float> rt((size_t)std::max(P, 1) * BOUND_RTAB, 0.0f);
    for (int i = 0; i < P && fold; i++) {
      const float *b = bt.data() + (size_t)i * BOUND_TAB;
      // record j = what the kernel's step j reads: bm of pair j (its w goes into the row's B) and mm im dm ii dd of pair j - 1 (whose cells'
      // adjoints are formed from the carried W and G in the same step: k_lazy.hip); record BOUND_PAIRS holds the last pair's alone
      for (int j = 0; j <= BOUND_PAIRS; j++) {
        float *o = rt.data() + (size_t)i * BOUND_RTAB + (size_t)j * 12;
        if (j < BOUND_PAIRS) { o[6] = b[(size_t)j * 16 + 8]; o[7] = b[(size_t)j * 16 + 9]; }      // B -> M_k1, B -> M_k2
        if (j >= 1) {
          const int jj = j - 1;
          for (int q = 0; q < 6; q++) o[q] = b[(size_t)(jj + 1) * 16 + q];                         // mm im dm of the pair's nodes
          o[8] = b[(size_t)(jj + 1) * 16 + 6]; o[9] = b[(size_t)(jj + 1) * 16 + 7];                // I_k -> I_k
          o[10] = b[(size_t)jj * 16 + 11];                                                         // D_k1 -> D_k2
          o[11] = (jj + 1 < BOUND_PAIRS) ? b[(size_t)(jj + 1) * 16 + 10] : 0.0f;                   // D_k2 -> D_k2+1 (none after the last node)
        }
      }
    }
    HIPCHK(upload(ctx->d_rtab, rt, ctx->st));
    // the folded emission odds by node, [code][k - 1]: what both kernels keep in LDS
    std::vector<float> et((size_t)std::max(P, 1) * NCODE * KK, 0.0f);
    for (int i = 0; i < P && fold; i++) {
      const DevProfile &d = dp[i];
      const int Q = ctx->profs[i].Q;
      const float *gq = bt.data() + (size_t)i * BOUND_TAB + (size_t)(BOUND_PAIRS + 1) * 16;
      for (int x = 0; x < NCODE; x++)
        for (int k0 = 0; k0 < KK; k0++) {
          const float e = (k0 < 4 * Q) ? d.rf[(x * QMAX + (k0 % Q)) * 4 + k0 / Q] : 0.0f;
          et[((size_t)i * NCODE + x) * KK + k0] = e * gq[k0];
        }
    }
    HIPCHK(upload(ctx->d_entab, et, ctx->st));
  }
  HIPCHK(upload(ctx->d_prof, dp, ctx->st));
  HIPCHK(upload(ctx->d_etab, etab, ctx->st));
  HIPCHK(upload(ctx->d_pbias, pb, ctx->st));
  HIPCHK(upload(ctx->d_ptec, pt, ctx->st));
  HIPCHK(upload(ctx->d_ptbm, pm, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  ctx->stats.n_profiles = P;
  if (n_profiles) *n_profiles = P;
  return ITSX_OK;
}

int itsx_load_profiles_mem(itsx_ctx *ctx, const char *text, int64_t len, int *n_profiles)
{
  CTXCHK(ctx && text && len >= 0);
  std::vector<HostProfile> pv;
  const std::string e = parse_hmm_text(text, len, pv);
  if (!e.empty()) SET_ERR(ctx, ITSX_E_FORMAT, e);
  return install_profiles(ctx, pv, n_profiles);
}

// whole file, decompressed by its magic bytes (fastq_io.h); read files stay in the text cache for the writers
// ctx: a context that opted in (itsx_set_device_inflate, ITSX_DEVICE_INFLATE=1) tries a gzip file on the device first (inflate_file,
// below); a file the device declines goes the host's way exactly as without it
static bool inflate_for_loader(itsx_ctx *ctx, const itsx_io::Text &raw, itsx_io::Text &out);
static bool device_inflate_on(const itsx_ctx *ctx);
// ctx: a context that opted in (itsx_set_device_parse, ITSX_DEVICE_PARSE=1) parses on the device (load_parsed_device, below: paths, or
// one text in memory); PARSE_FALLBACK = a text was declined or could not be read, and the caller goes the host's way from the start
constexpr int PARSE_FALLBACK = 1;
static bool device_parse_on(const itsx_ctx *ctx);
static int load_parsed_device(itsx_ctx *ctx, const char *const *paths, int32_t n_paths, const char *text, int64_t nbytes, int64_t *n_reads_per_file, bool batch);
// the same for the paired merge loaders (S samples from files, or one sample's two texts in memory); PARSE_FALLBACK also where R1 and R2
// of a sample differ in their record counts, a quality lies outside 33..126 or a pair is longer than the merge kernel takes
static int merge_pairs_load_device(itsx_ctx *ctx, const char *const *r1_paths, const char *const *r2_paths, const char *const *seq_out_paths, int32_t S,
                                   const char *text1, int64_t nb1, const char *text2, int64_t nb2, int maxdiffs, double maxee, int allow_stagger,
                                   int64_t *n_pairs_per_sample, int64_t *n_merged_per_sample, bool batch);
static std::shared_ptr<const itsx_io::Text> slurp(const char *path, bool cacheable, std::string &err, itsx_ctx *ctx = nullptr)
{
  if (ctx && device_inflate_on(ctx)) {
    const itsx_io::InflateFirst first = [ctx](const itsx_io::Text &raw, itsx_io::Text &out) { return inflate_for_loader(ctx, raw, out); };
    return itsx_io::read_text(path, err, cacheable, &first);
  }
  return itsx_io::read_text(path, err, cacheable);
}

int itsx_load_profiles_file(itsx_ctx *ctx, const char *hmm_path, int *n_profiles)
{
  CTXCHK(ctx && hmm_path);
  std::string err;
  const auto tp = slurp(hmm_path, false, err);
  if (!tp) SET_ERR(ctx, ITSX_E_IO, err);
  return itsx_load_profiles_mem(ctx, tp->data(), (int64_t)tp->size(), n_profiles);
}

int itsx_profile_name(const itsx_ctx *ctx, int i, char *buf, int buflen)
{
  CTXCHK(ctx && buf && buflen > 0 && i >= 0 && i < ctx->P);
  snprintf(buf, (size_t)buflen, "%s", ctx->profs[i].name.c_str());
  return ITSX_OK;
}

int itsx_profile_tables(const itsx_ctx *ctx, int i, uint8_t *rbv, float *rfv, float *tfv, int32_t *params6)
{
  CTXCHK(ctx && i >= 0 && i < ctx->P);
  const HostProfile &h = ctx->profs[i];
  if (rbv) memcpy(rbv, h.rbv.data(), h.rbv.size());
  if (rfv) memcpy(rfv, h.rfv.data(), h.rfv.size() * sizeof(float));
  if (tfv) memcpy(tfv, h.tfv.data(), h.tfv.size() * sizeof(float));
  if (params6) { params6[0] = h.M; params6[1] = h.Q; params6[2] = h.base_b; params6[3] = h.bias_b; params6[4] = h.tbm_b; params6[5] = h.tec_b; }
  return ITSX_OK;
}

// ------------------------------------------------------------------------------ reads
static int8_t g_code[256];
static bool g_code_init = false;
static void init_codes()
{
  if (g_code_init) return;
  memset(g_code, -1, sizeof(g_code));
  const char *sym = "ACGT-RYMKSWHBVDN";
  for (int i = 0; i < 16; i++) { g_code[(unsigned char)sym[i]] = (int8_t)i; g_code[(unsigned char)(sym[i] | 0x20)] = (int8_t)i; }
  g_code[(unsigned char)'-'] = -1;
  g_code[(unsigned char)'U'] = g_code[(unsigned char)'u'] = 3;
  g_code[(unsigned char)'X'] = g_code[(unsigned char)'x'] = 15;
  g_code_init = true;
}

// Hand-over of the reads: the ASCII bases travel in chunks of whole reads through three pinned staging buffers (a pool of
// host threads copies chunk c+1 into its buffer while chunk c is on the bus and chunk c-1 is being packed), and are packed on
// the device chunk by chunk (k_util.hip).  A pageable hipMemcpy of the whole text moved 4.4 GB (10 M merged reads) at ~5 GB/s.
// the three pinned / device staging buffers, at least `bytes` each
static int stage_reserve(itsx_ctx *ctx, int64_t bytes)
{
  if ((int64_t)ctx->stage_cap >= bytes) return ITSX_OK;
  for (int k = 0; k < itsx_ctx::NSTAGE; k++) {
    if (ctx->stage_pin[k]) { (void)hipHostFree(ctx->stage_pin[k]); ctx->stage_pin[k] = nullptr; }
    HIPCHK(hipHostMalloc(&ctx->stage_pin[k], (size_t)bytes, hipHostMallocDefault));
    HIPCHK(ctx->stage_dev[k].alloc((size_t)bytes + 16, true));
    if (!ctx->stage_ev[k]) HIPCHK(hipEventCreateWithFlags(&ctx->stage_ev[k], hipEventDisableTiming));
  }
  ctx->stage_cap = (size_t)bytes;
  return ITSX_OK;
}

static int pack_and_upload(itsx_ctx *ctx, const char *view = nullptr, const uint8_t *dev_raw = nullptr)
{
  init_codes();
  StageTxn txn(ctx, itsx_ctx::ST_NONE);                  // a new read set (whoever keeps records installs them after this), or none
  const auto tp0 = std::chrono::steady_clock::now();
  const int64_t n = ctx->N;
  ctx->dev_bases = dev_raw;
  if (ctx->d_merged_text.p && dev_raw != ctx->d_merged_text.p) ctx->d_merged_text.release();      // the last merge's text: this read set is another
  ctx->bases_view = dev_raw ? nullptr : (view ? view : ctx->h_bases.data());
  const char *bases = ctx->bases_view;
  ctx->h_len.resize((size_t)n); ctx->h_woff.resize((size_t)n + 1);
  ctx->h_woff[0] = 0;
  int Lmax = 0;
  {   // lengths, word offsets (a running sum: per thread over its share of the reads, then shifted by the shares before it), longest read
    const int T = n >= (1 << 20) ? std::max(1, std::min(8, itsx_io::io_threads())) : 1;
    std::vector<int64_t> wsum((size_t)T + 1, 0); std::vector<int> lmx((size_t)T, 0), bad((size_t)T, 0);
    on_threads(T, [&](int t) {
      const int64_t lo = n * t / T, hi = n * (t + 1) / T;
      int64_t w = 0; int mx = 0, b = 0;
      for (int64_t r = lo; r < hi; r++) {
        const int64_t L = ctx->h_off[r + 1] - ctx->h_off[r];
        if (L < 0) b |= 1;
        if (L > 65535) b |= 2;
        ctx->h_len[r] = (int32_t)L;
        mx = std::max(mx, (int)std::min<int64_t>(L, 1 << 30));
        w += std::max<int64_t>(1, (L + 15) / 16);
        ctx->h_woff[r + 1] = w;
      }
      wsum[(size_t)t + 1] = w; lmx[(size_t)t] = mx; bad[(size_t)t] = b;
    });
    int b = 0;
    for (int t = 0; t < T; t++) { wsum[(size_t)t + 1] += wsum[(size_t)t]; Lmax = std::max(Lmax, lmx[(size_t)t]); b |= bad[(size_t)t]; }
    if (b & 1) SET_ERR(ctx, ITSX_E_ARG, "read offsets must be non-decreasing");
    if (b & 2) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "reads longer than 65535 bases are not supported");
    if (T > 1)
      on_threads(T, [&](int t) {
        if (t == 0) return;
        const int64_t lo = n * t / T, hi = n * (t + 1) / T, add = wsum[(size_t)t];
        for (int64_t r = lo; r < hi; r++) ctx->h_woff[r + 1] += add;
      });
  }
  ctx->Lmax = Lmax;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const int64_t nb = n > 0 ? ctx->h_off[n] : 0;
  int64_t CH = 64ll << 20;
  if (const char *e = sw_get("ITSX_PACK_CHUNK")) CH = std::max<int64_t>(70000, atoll(e));       // bytes; a read has at most 65535
  CH = std::min<int64_t>(CH, std::max<int64_t>(nb, 70000));
  constexpr int K = itsx_ctx::NSTAGE;
  if (!dev_raw) { const int src = stage_reserve(ctx, CH); if (src != ITSX_OK) return src; }
  DBuf<int64_t> &d_off = ctx->w_pk_off; DBuf<int8_t> &d_lut = ctx->w_pk_lut; DBuf<int32_t> &d_excnt = ctx->w_pk_excnt, &d_exstart = ctx->w_pk_exstart, &d_tmp = ctx->w_pk_tmp;
  DBuf<long long> &d_bad = ctx->w_pk_bad;
  HIPCHK(d_off.alloc((size_t)n + 1)); HIPCHK(d_lut.alloc(256)); HIPCHK(d_excnt.alloc((size_t)n + 2)); HIPCHK(d_exstart.alloc((size_t)n + 2));
  HIPCHK(d_tmp.alloc((size_t)scan_tmp_elems(n + 2))); HIPCHK(d_bad.alloc(4));
  HIPCHK(ctx->d_words.alloc((size_t)ctx->h_woff[n] + 1)); HIPCHK(ctx->d_woff.alloc((size_t)n + 1)); HIPCHK(ctx->d_excoff.alloc((size_t)n + 1)); HIPCHK(ctx->d_len.alloc((size_t)n + 1));
  HIPCHK(hipMemcpyAsync(d_off.p, ctx->h_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ctx->d_woff.p, ctx->h_woff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
  if (n) HIPCHK(hipMemcpyAsync(ctx->d_len.p, ctx->h_len.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_lut.p, g_code, 256, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_excnt.p, 0, ((size_t)n + 2) * 4, st));
  // the exception list is sized by a guess; a read set with more non-ACGT symbols than that repeats the exception pass
  int64_t ecap = std::max<int64_t>((int64_t)ctx->d_exc.cap, nb / 256 + 4096 + ctx->pack_exc_hint);
  ctx->pack_exc_hint = 0;
  if (const char *e = sw_get("ITSX_PACK_ECAP")) ecap = std::max<int64_t>(1, atoll(e));
  HIPCHK(ctx->d_exc.alloc((size_t)ecap));
  int copy_threads = std::max(1, std::min(8, itsx_io::io_threads()));
  long long hb[4] = {0, 0, 0, 0};                        // exceptions so far, list overflow, first illegal read, -
  for (int pass = 0; pass < 2; pass++) {                 // pass 1 only when the exception list was too small
    const long long init[4] = {0, 0, 0x7f7f7f7f7f7f7f7fll, 0};
    HIPCHK(hipMemcpyAsync(d_bad.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    int64_t r0 = 0; int c = 0;
    if (dev_raw && n > 0) {                              // the text is in device memory already: one chunk, no staging
      if (pass == 0) launch_pack(dev_raw, 0, d_off.p, ctx->d_woff.p, 0, n, d_lut.p, ctx->d_words.p, d_excnt.p, d_bad.p + 2, st);
      launch_exclusive_scan(d_excnt.p, d_exstart.p, n + 1, d_tmp.p, st);
      launch_pack_exc(dev_raw, 0, d_off.p, 0, n, d_lut.p, d_excnt.p, d_exstart.p, d_bad.p, ecap, ctx->d_excoff.p, ctx->d_exc.p, st);
      r0 = n;
    }
    while (r0 < n) {
      // reads [r0, r1): as many whole reads as fit the staging buffer
      const int64_t b0 = ctx->h_off[r0];
      int64_t r1 = (int64_t)(std::upper_bound(ctx->h_off.begin() + r0, ctx->h_off.begin() + n + 1, b0 + CH) - ctx->h_off.begin()) - 1;
      r1 = std::min<int64_t>(n, std::max<int64_t>(r1, r0 + 1));
      const int64_t bytes = ctx->h_off[r1] - b0;
      const int k = c % K;
      if (c >= K) HIPCHK(hipEventSynchronize(ctx->stage_ev[k]));
      if (bytes > 0) {
        char *dst = (char *)ctx->stage_pin[k];
        const int T = bytes >= (4 << 20) ? copy_threads : 1;
        on_threads(T, [&](int t) { const int64_t lo = bytes * t / T, hi = bytes * (t + 1) / T; memcpy(dst + lo, bases + b0 + lo, (size_t)(hi - lo)); });
        HIPCHK(hipMemcpyAsync(ctx->stage_dev[k].p, dst, (size_t)bytes, hipMemcpyHostToDevice, st));
      }
      if (pass == 0) launch_pack(ctx->stage_dev[k].p, b0, d_off.p, ctx->d_woff.p, r0, r1, d_lut.p, ctx->d_words.p, d_excnt.p, d_bad.p + 2, st);
      launch_exclusive_scan(d_excnt.p + r0, d_exstart.p + r0, r1 - r0 + 1, d_tmp.p, st);
      launch_pack_exc(ctx->stage_dev[k].p, b0, d_off.p, r0, r1, d_lut.p, d_excnt.p, d_exstart.p, d_bad.p, ecap, ctx->d_excoff.p, ctx->d_exc.p, st);
      HIPCHK(hipEventRecord(ctx->stage_ev[k], st));
      r0 = r1; c++;
    }
    if (n == 0) HIPCHK(hipMemsetAsync(ctx->d_excoff.p, 0, 8, st));
    HIPCHK(hipMemcpyAsync(hb, d_bad.p, sizeof(hb), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (hb[2] >= 0 && hb[2] < n) SET_ERR(ctx, ITSX_E_FORMAT, "read " + std::to_string(hb[2]) + " contains a symbol outside the IUPAC DNA alphabet");
    if (!hb[1]) break;
    if (pass == 1) SET_ERR(ctx, ITSX_E_DEVICE, "exception list overflow after resizing");
    ecap = hb[0] + 1;
    HIPCHK(ctx->d_exc.alloc((size_t)ecap));
  }
  ctx->rd.words = ctx->d_words.p; ctx->rd.woff = ctx->d_woff.p; ctx->rd.len = ctx->d_len.p;
  ctx->rd.excoff = ctx->d_excoff.p; ctx->rd.exc = ctx->d_exc.p; ctx->rd.n = n;
  ctx->stats.n_reads = n;
  ctx->S = 1; ctx->sel_sample = -1; ctx->h_sample.clear();      // a new read set is one sample until told otherwise
  ctx->stats.ms_pack = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count();
  txn.commit(itsx_ctx::ST_READS);
  return ITSX_OK;
}

// the caller's offsets, rebased to 0 (10 M reads: 80 MB -- copied and shifted in one pass by a few threads)
static int64_t take_offsets(itsx_ctx *ctx, const int64_t *offsets, int64_t n)
{
  const int64_t base0 = offsets[0];
  ctx->h_off.resize((size_t)n + 1);
  int64_t *dst = ctx->h_off.data();
  const int T = n >= (1 << 20) ? std::max(1, std::min(8, itsx_io::io_threads())) : 1;
  on_threads(T, [&](int t) { for (int64_t r = (n + 1) * t / T, hi = (n + 1) * (t + 1) / T; r < hi; r++) dst[r] = offsets[r] - base0; });
  return base0;
}
static int set_reads_impl(itsx_ctx *ctx, const char *bases, const int64_t *offsets, int64_t n, const char *names, const int64_t *name_offsets, bool borrow)
{
  CTXCHK(ctx && offsets && n >= 0 && (bases || offsets[n] == offsets[0]));
  if (n >= (1ll << 31) - 64) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "more than 2^31 reads in one context");
  ctx->N = n;
  const int64_t base0 = take_offsets(ctx, offsets, n);
  const char *view = nullptr;
  if (borrow) { itsx_io::Text().swap(ctx->h_bases); view = bases ? bases + base0 : ""; }
  else if (bases) ctx->h_bases.assign(bases + base0, (size_t)(offsets[n] - base0));
  else ctx->h_bases.clear();
  ctx->h_names.clear();
  if (names && name_offsets) {
    ctx->h_names.assign(names, name_offsets, n);
  }
  return pack_and_upload(ctx, view);
}
int itsx_set_reads(itsx_ctx *ctx, const char *bases, const int64_t *offsets, int64_t n, const char *names, const int64_t *name_offsets)
{ return set_reads_impl(ctx, bases, offsets, n, names, name_offsets, false); }
int itsx_set_reads_view(itsx_ctx *ctx, const char *bases, const int64_t *offsets, int64_t n, const char *names, const int64_t *name_offsets)
{ return set_reads_impl(ctx, bases, offsets, n, names, name_offsets, true); }
// the text already lives in device memory (the output of a device-side parser or of the merge kernel): packed where it is
int itsx_set_reads_device(itsx_ctx *ctx, const void *d_bases, const int64_t *offsets, int64_t n, const char *names, const int64_t *name_offsets)
{
  CTXCHK(ctx && offsets && n >= 0 && (d_bases || offsets[n] == offsets[0]));
  if (n >= (1ll << 31) - 64) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "more than 2^31 reads in one context");
  ctx->N = n;
  const int64_t base0 = take_offsets(ctx, offsets, n);
  itsx_io::Text().swap(ctx->h_bases);
  ctx->h_names.clear();
  if (names && name_offsets) {
    ctx->h_names.assign(names, name_offsets, n);
  }
  static const uint8_t none = 0;
  return pack_and_upload(ctx, nullptr, d_bases ? (const uint8_t *)d_bases + base0 : &none);
}

// ---- FASTA / FASTQ text -> records (labels up to the first blank, as vsearch labels them).  Large texts are cut at record
// starts and parsed by the I/O pool; the pieces are joined in order, so the result is the serial parser's.
struct FastxPart {
  itsx_io::Text seq, qual; std::vector<int64_t> off{0}; NameList ids;
  NameList titles;                       // whole title lines, only where a caller collects them (parse_fastq_side)
  bool lower = false;                    // upper-casing changed a base: the text no longer holds the input's bytes
  int rc = ITSX_OK; std::string err;
};

static void parse_fastx_range(const char *s, const char *end, bool want_qual, bool upper, FastxPart &out)
{
  auto next_line = [&](const char *&b, const char *&e) -> bool {
    if (s >= end) return false;
    b = s; const char *nl = (const char *)memchr(s, '\n', (size_t)(end - s));
    e = nl ? nl : end; s = nl ? nl + 1 : end;
    if (e > b && e[-1] == '\r') e--;
    return true;
  };
  auto put_seq = [&](const char *b, const char *e) {
    const size_t o = out.seq.size();
    out.seq.append(b, e);
    if (upper) { char *q = out.seq.data(); for (size_t i = o; i < out.seq.size(); i++) { const char u = (char)toupper((unsigned char)q[i]); if (u != q[i]) { q[i] = u; out.lower = true; } } }
  };
  // (a FASTQ record is about half sequence: room for it up front instead of a dozen doublings with their copies)
  if (end > s && (size_t)(end - s) > ((size_t)1 << 20)) { out.seq.reserve(out.seq.size() + (size_t)(end - s) / 2 + 4096); if (want_qual) out.qual.reserve(out.qual.size() + (size_t)(end - s) / 2 + 4096); out.ids.blob.reserve(out.ids.blob.size() + (size_t)(end - s) / 8); }
  const char *b, *e;
  bool pending = false;                  // a header line already read into b,e
  while (pending || next_line(b, e)) {
    pending = false;
    if (b == e) continue;
    if (*b == '@') {                     // FASTQ record: 4 lines
      const char *ne = b + 1; while (ne < e && *ne != ' ' && *ne != '\t') ne++;
      out.ids.emplace_back(b + 1, ne);
      const char *sb, *se, *pb, *pe, *qb, *qe;
      if (!next_line(sb, se) || !next_line(pb, pe) || !next_line(qb, qe) || pb == pe || *pb != '+' || (qe - qb) != (se - sb)) {
        out.rc = ITSX_E_FORMAT; out.err = "malformed FASTQ record"; return;
      }
      put_seq(sb, se);
      if (want_qual) out.qual.append(qb, qe);
      out.off.push_back((int64_t)out.seq.size());
    } else if (*b == '>') {              // FASTA record: header + sequence lines
      const char *ne = b + 1; while (ne < e && *ne != ' ' && *ne != '\t') ne++;
      out.ids.emplace_back(b + 1, ne);
      while (next_line(b, e)) {
        if (b < e && *b == '>') { pending = true; break; }
        put_seq(b, e);
      }
      if (want_qual) { const size_t q0 = out.qual.size(); out.qual.resize(out.seq.size()); if (out.qual.size() > q0) memset(out.qual.data() + q0, 'I', out.qual.size() - q0); }
      out.off.push_back((int64_t)out.seq.size());
    } else { out.rc = ITSX_E_FORMAT; out.err = "input is neither FASTA nor FASTQ"; return; }
  }
}

static int parse_fastx(const itsx_io::Text &text, bool want_qual, bool upper, FastxPart &out, std::string &err)
{
  const size_t n = text.size();
  int T = itsx_io::io_threads();
  if (const char *e = sw_get("ITSX_PARSE_MIN_MB")) { if (n < (size_t)atol(e) << 20) T = 1; }
  else if (n < ((size_t)16 << 20)) T = 1;
  size_t first = 0;
  while (first < n && (text[first] == '\n' || text[first] == '\r')) first++;
  if (first < n && text[first] != '@' && text[first] != '>') T = 1;          // the serial parser reports it
  std::vector<size_t> cut(1, 0);
  if (T > 1) {
    const bool fastq = text[first] == '@';
    for (int k = 1; k < T; k++) { const size_t from = n / (size_t)T * (size_t)k, c = fastq ? itsx_io::fastq_record_start(text.data(), n, from) : itsx_io::fasta_record_start(text.data(), n, from); if (c > cut.back() && c < n) cut.push_back(c); }
  }
  cut.push_back(n);
  const size_t np = cut.size() - 1;
  if (np == 1) {
    parse_fastx_range(text.data(), text.data() + n, want_qual, upper, out);
    if (out.rc != ITSX_OK) err = out.err + (out.rc == ITSX_E_FORMAT && out.err[0] == 'm' ? " near read " + std::to_string(out.ids.size()) : "");
    return out.rc;
  }
  std::vector<FastxPart> parts(np);
  on_threads((int)np, [&](int k) { parse_fastx_range(text.data() + cut[(size_t)k], text.data() + cut[(size_t)k + 1], want_qual, upper, parts[(size_t)k]); });
  size_t nrec = 0, nseq = 0;
  for (size_t k = 0; k < np; k++) {
    if (parts[k].rc != ITSX_OK) { err = parts[k].err + " near read " + std::to_string(nrec + parts[k].ids.size()); return parts[k].rc; }
    nrec += parts[k].ids.size(); nseq += parts[k].seq.size();
    out.lower = out.lower || parts[k].lower;
  }
  const size_t rec0 = out.ids.size(), seq0 = out.seq.size(), nam0 = out.ids.blob.size();
  size_t nnam = 0;
  for (size_t k = 0; k < np; k++) nnam += parts[k].ids.blob.size();
  out.ids.off.resize(rec0 + nrec + 1); out.ids.blob.resize(nam0 + nnam); out.off.resize(rec0 + nrec + 1);
  if (!out.seq.resize(seq0 + nseq) || (want_qual && !out.qual.resize(seq0 + nseq))) { err = "out of memory parsing the reads"; return ITSX_E_NOMEM; }
  std::vector<size_t> rbase(np), sbase(np), nbase(np);
  { size_t r = rec0, q = seq0, m = nam0; for (size_t k = 0; k < np; k++) { rbase[k] = r; sbase[k] = q; nbase[k] = m; r += parts[k].ids.size(); q += parts[k].seq.size(); m += parts[k].ids.blob.size(); } }
  on_threads((int)np, [&](int k) {
    FastxPart &p = parts[(size_t)k];
    if (p.seq.size()) memcpy(out.seq.data() + sbase[(size_t)k], p.seq.data(), p.seq.size());
    if (want_qual && p.qual.size()) memcpy(out.qual.data() + sbase[(size_t)k], p.qual.data(), p.qual.size());
    if (p.ids.blob.size()) memcpy(out.ids.blob.data() + nbase[(size_t)k], p.ids.blob.data(), p.ids.blob.size());
    for (size_t i = 0; i < p.ids.size(); i++) {
      out.ids.off[rbase[(size_t)k] + i + 1] = (int64_t)nbase[(size_t)k] + p.ids.off[i + 1];
      out.off[rbase[(size_t)k] + i + 1] = (int64_t)sbase[(size_t)k] + p.off[i + 1];
    }
  });
  return ITSX_OK;
}

// appended to the context's host-side read set
// qual (may be null): the records' qualities are appended to it as the bases are to the read set's text
static int parse_fastx_append(itsx_ctx *ctx, const itsx_io::Text &text, itsx_io::Text *qual = nullptr)
{
  FastxPart part;
  part.seq.swap(ctx->h_bases); part.off.swap(ctx->h_off); part.ids.swap(ctx->h_names);
  if (qual) part.qual.swap(*qual);
  if (part.off.empty()) part.off.assign(1, 0);
  std::string err;
  const int rc = parse_fastx(text, qual != nullptr, false, part, err);
  ctx->h_bases.swap(part.seq); ctx->h_off.swap(part.off); ctx->h_names.swap(part.ids);
  if (qual) part.qual.swap(*qual);
  if (rc != ITSX_OK) SET_ERR(ctx, rc, err);
  return ITSX_OK;
}

int itsx_load_reads_file(itsx_ctx *ctx, const char *path, int64_t *n_reads)
{
  CTXCHK(ctx && path);
  if (device_parse_on(ctx)) { const int drc = load_parsed_device(ctx, &path, 1, nullptr, 0, n_reads, false); if (drc != PARSE_FALLBACK) return drc; }
  std::string rerr;
  static const bool trace = sw_get("ITSX_TRACE_ALLOC") != nullptr;
  const auto tt0 = std::chrono::steady_clock::now();
  const auto tp = slurp(path, true, rerr, ctx);
  if (!tp) SET_ERR(ctx, ITSX_E_IO, rerr);
  const auto tt1 = std::chrono::steady_clock::now();
  ctx->h_bases.clear(); ctx->h_off.assign(1, 0); ctx->h_names.clear();
  { const int prc = parse_fastx_append(ctx, *tp); if (prc != ITSX_OK) return prc; }
  ctx->N = (int64_t)ctx->h_names.size();
  if (n_reads) *n_reads = ctx->N;
  const auto tt2 = std::chrono::steady_clock::now();
  const int rc = pack_and_upload(ctx);
  if (trace) {
    const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[itsx] load %s: read+inflate %.0f ms, parse %.0f ms, upload+pack %.0f ms\n", path, ms(tt0, tt1), ms(tt1, tt2), ms(tt2, std::chrono::steady_clock::now()));
  }
  return rc;
}

int itsx_load_reads_text(itsx_ctx *ctx, const char *text, int64_t nbytes, int64_t *n_reads)
{
  CTXCHK(ctx && (text || nbytes == 0) && nbytes >= 0);
  LoadPriority load_priority(ctx);
  if (device_parse_on(ctx)) { const int drc = load_parsed_device(ctx, nullptr, 0, text ? text : "", nbytes, n_reads, false); if (drc != PARSE_FALLBACK) return drc; }
  itsx_io::Text view;
  view.borrow(text ? text : "", (size_t)nbytes);
  ctx->h_bases.clear(); ctx->h_off.assign(1, 0); ctx->h_names.clear();
  { const int prc = parse_fastx_append(ctx, view); if (prc != ITSX_OK) return prc; }
  ctx->N = (int64_t)ctx->h_names.size();
  if (n_reads) *n_reads = ctx->N;
  return pack_and_upload(ctx);
}

// One shard of a file's reads: records [n shard / n_shards, n (shard + 1) / n_shards) in file order (input order is kept inside a
// shard: first-occurrence representatives depend on it).  Every worker of a multi-GPU run parses the file itself (the decompressed
// text is cached per process) and keeps its own slice.
int itsx_load_reads_file_shard(itsx_ctx *ctx, const char *path, int32_t shard, int32_t n_shards, int64_t *n_total, int64_t *first, int64_t *n_reads)
{
  CTXCHK(ctx && path);
  if (n_shards < 1 || shard < 0 || shard >= n_shards) SET_ERR(ctx, ITSX_E_ARG, "itsx_load_reads_file_shard: shard out of range");
  std::string rerr;
  const auto tp = slurp(path, true, rerr);
  if (!tp) SET_ERR(ctx, ITSX_E_IO, rerr);
  ctx->h_bases.clear(); ctx->h_off.assign(1, 0); ctx->h_names.clear();
  { const int prc = parse_fastx_append(ctx, *tp); if (prc != ITSX_OK) return prc; }
  const int64_t tot = (int64_t)ctx->h_names.size();
  const int64_t lo = tot * shard / n_shards, hi = tot * (shard + 1) / n_shards;
  if (lo > 0 || hi < tot) {
    const int64_t b0 = ctx->h_off[(size_t)lo], b1 = ctx->h_off[(size_t)hi];
    itsx_io::Text bases;
    bases.assign(ctx->h_bases.data() + b0, (size_t)(b1 - b0));
    std::vector<int64_t> off((size_t)(hi - lo) + 1);
    for (int64_t r = lo; r <= hi; r++) off[(size_t)(r - lo)] = ctx->h_off[(size_t)r] - b0;
    NameList names = ctx->h_names.slice((size_t)lo, (size_t)hi);
    ctx->h_bases.swap(bases); ctx->h_off.swap(off); ctx->h_names.swap(names);
  }
  ctx->N = hi - lo;
  if (n_total) *n_total = tot;
  if (first) *first = lo;
  if (n_reads) *n_reads = ctx->N;
  return pack_and_upload(ctx);
}

// ---- per-sample batching (q2_itsxpress.py:273-333 runs the whole path once per sample)
int itsx_set_samples(itsx_ctx *ctx, const int32_t *sample_of_read, int32_t n_samples)
{
  CTXCHK(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  StageTxn txn(ctx, itsx_ctx::ST_READS);                 // the reads stay, what was grouped by the old samples goes
  ctx->sel_sample = -1;
  if (!sample_of_read || n_samples <= 1) { ctx->S = 1; ctx->h_sample.clear(); txn.commit(itsx_ctx::ST_READS); return ITSX_OK; }
  if ((int64_t)n_samples * std::max(ctx->P, 1) > (1ll << 28)) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "too many samples x profiles for one batch");
  for (int64_t r = 0; r < ctx->N; r++)
    if (sample_of_read[r] < 0 || sample_of_read[r] >= n_samples) SET_ERR(ctx, ITSX_E_ARG, "sample index of read " + std::to_string(r) + " is out of range");
  ctx->h_sample.assign(sample_of_read, sample_of_read + ctx->N);
  ctx->S = n_samples;
  HIPCHK(upload(ctx->d_sample, ctx->h_sample, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  txn.commit(itsx_ctx::ST_READS);
  return ITSX_OK;
}
int itsx_num_samples(const itsx_ctx *ctx) { return ctx ? ctx->S : ITSX_E_ARG; }
// test hook: every read's sample as the kernels see it (d_sample) and as the writers see it (h_sample)
int itsx_debug_read_samples(itsx_ctx *ctx, int32_t *device_ids, int32_t *host_ids)
{
  CTXCHK(ctx);
  const size_t n = (size_t)ctx->N;
  if (ctx->S <= 1) {
    if (device_ids) std::fill(device_ids, device_ids + n, 0);
    if (host_ids) std::fill(host_ids, host_ids + n, 0);
    return ITSX_OK;
  }
  if (ctx->h_sample.size() != n || ctx->d_sample.n < n) SET_ERR(ctx, ITSX_E_ARG, "the batch's sample vectors do not cover its reads");
  HIPCHK(hipSetDevice(ctx->device));
  if (device_ids && n) { HIPCHK(hipMemcpyAsync(device_ids, ctx->d_sample.p, n * 4, hipMemcpyDeviceToHost, ctx->st)); HIPCHK(hipStreamSynchronize(ctx->st)); }
  if (host_ids && n) memcpy(host_ids, ctx->h_sample.data(), n * 4);
  return ITSX_OK;
}
// test hook: the length-ordered unique list as it lies on the device (d_sorted_uniq, its first U_active entries)
int itsx_debug_sorted_uniques(itsx_ctx *ctx, int32_t *out)
{
  CTXCHK(ctx && ctx->grouped() && (out || ctx->U_active == 0));
  const size_t m = (size_t)ctx->U_active;
  if (ctx->d_sorted_uniq.n < m) SET_ERR(ctx, ITSX_E_ARG, "the length-ordered list does not cover the active uniques");
  HIPCHK(hipSetDevice(ctx->device));
  if (m) { HIPCHK(hipMemcpyAsync(out, ctx->d_sorted_uniq.p, m * 4, hipMemcpyDeviceToHost, ctx->st)); HIPCHK(hipStreamSynchronize(ctx->st)); }
  return (int)m;
}
int itsx_select_sample(itsx_ctx *ctx, int32_t sample)
{
  CTXCHK(ctx);
  if (sample < -1 || sample >= ctx->S) SET_ERR(ctx, ITSX_E_ARG, "sample index out of range");
  ctx->sel_sample = sample;
  ctx->order_cache_ok = false;
  return ITSX_OK;
}
// the title lines of a FASTQ text the parser has accepted ('@' to the end of the line, CR dropped), appended to `titles`
static void fastq_titles(const itsx_io::Text &text, NameList &titles)
{
  const char *s = text.data(), *end = s + text.size();
  auto line = [&](const char *&b, const char *&e) -> bool {
    if (s >= end) return false;
    b = s; const char *nl = (const char *)memchr(s, '\n', (size_t)(end - s));
    e = nl ? nl : end; s = nl ? nl + 1 : end;
    if (e > b && e[-1] == '\r') e--;
    return true;
  };
  const char *b, *e, *x, *y;
  while (line(b, e)) {
    if (b == e) continue;
    titles.emplace_back(b, e);
    if (!line(x, y) || !line(x, y) || !line(x, y)) break;
  }
}

// the records of the read set the context has just been given, from host planes (bases: the read set's own text and offsets)
static int install_records(itsx_ctx *ctx, const itsx_io::Text &qual, NameList &titles)
{
  itsx_ctx::Records &r = ctx->rec;
  const size_t n = (size_t)ctx->N, nb = n ? (size_t)ctx->h_off[n] : 0;
  if (qual.size() != nb || titles.size() != n) SET_ERR(ctx, ITSX_E_FORMAT, "the records kept for the read set do not match its reads");
  hipStream_t st = ctx->st;
  HIPCHK(r.seq.alloc(nb + 64)); HIPCHK(r.qual.alloc(nb + 64)); HIPCHK(r.titles.alloc(titles.blob.size() + 64));
  HIPCHK(r.off.alloc(n + 1)); HIPCHK(r.toff.alloc(n + 1));
  if (nb) { HIPCHK(hipMemcpyAsync(r.seq.p, ctx->bases_view, nb, hipMemcpyHostToDevice, st)); HIPCHK(hipMemcpyAsync(r.qual.p, qual.data(), nb, hipMemcpyHostToDevice, st)); }
  if (!titles.blob.empty()) HIPCHK(hipMemcpyAsync(r.titles.p, titles.blob.data(), titles.blob.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(r.off.p, ctx->h_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(r.toff.p, titles.off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  r.h_titles.swap(titles);
  r.seq_p = r.seq.p; r.have = true;
  return ITSX_OK;
}

int itsx_keep_records(itsx_ctx *ctx, int on)
{
  CTXCHK(ctx);
  ctx->keep_records = on != 0;
  return ITSX_OK;
}

int itsx_keep_pair_records(itsx_ctx *ctx, int on)
{
  CTXCHK(ctx);
  ctx->keep_pair_records = on != 0;
  return ITSX_OK;
}

int itsx_set_merge_join(itsx_ctx *ctx, int on)
{
  CTXCHK(ctx);
  ctx->merge_join = on != 0;
  return ITSX_OK;
}

int itsx_load_reads_files(itsx_ctx *ctx, const char *const *paths, int32_t n_paths, int64_t *n_reads_per_file)
{
  CTXCHK(ctx && paths && n_paths >= 1);
  if (device_parse_on(ctx)) { const int drc = load_parsed_device(ctx, paths, n_paths, nullptr, 0, n_reads_per_file, true); if (drc != PARSE_FALLBACK) return drc; }
  ctx->h_bases.clear(); ctx->h_off.assign(1, 0); ctx->h_names.clear();
  std::vector<int32_t> smp;
  const bool records = ctx->keep_records;
  itsx_io::Text qual; NameList titles;
  for (int32_t f = 0; f < n_paths; f++) {
    CTXCHK(paths[f]);
    std::string rerr;
    const auto tp = slurp(paths[f], true, rerr, ctx);
    if (!tp) SET_ERR(ctx, ITSX_E_IO, rerr);
    const size_t before = ctx->h_names.size();
    if (records) {
      size_t first = 0;
      while (first < tp->size() && ((*tp)[first] == '\n' || (*tp)[first] == '\r')) first++;
      if (first < tp->size() && (*tp)[first] == '>') SET_ERR(ctx, ITSX_E_FORMAT, std::string("records are kept (itsx_keep_records) and this file is FASTA, which has no qualities: ") + paths[f]);
    }
    { const int prc = parse_fastx_append(ctx, *tp, records ? &qual : nullptr); if (prc != ITSX_OK) { ctx->set_error(ctx->err + " (" + paths[f] + ")"); return prc; } }
    if (records) {
      fastq_titles(*tp, titles);
      if (titles.size() != ctx->h_names.size()) SET_ERR(ctx, ITSX_E_FORMAT, std::string("records are kept (itsx_keep_records) and this file is not FASTQ throughout: ") + paths[f]);
    }
    if (n_reads_per_file) n_reads_per_file[f] = (int64_t)(ctx->h_names.size() - before);
    smp.resize(ctx->h_names.size(), f);
  }
  ctx->N = (int64_t)ctx->h_names.size();
  if (ctx->N >= (1ll << 31) - 64) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "more than 2^31 reads in one context");
  int rc = pack_and_upload(ctx);
  if (rc != ITSX_OK) return rc;
  rc = itsx_set_samples(ctx, smp.data(), n_paths);
  if (rc != ITSX_OK || !records) return rc;
  return install_records(ctx, qual, titles);
}

// ------------------------------------------------------------------------------ derep
// uniques = seeds in input order, then ordered by length for the HMM stages (shared by derep and cluster)
static int build_unique_lists(itsx_ctx *ctx)
{
  const int64_t n = ctx->N;
  DBuf<int32_t> &is_seed = ctx->w_is_seed, &seed_rank = ctx->w_seed_rank, &scan_tmp = ctx->w_scan_tmp;
  int32_t U = 0;
  if (n > 0) {
    launch_exclusive_scan(is_seed.p, seed_rank.p, n + 1, scan_tmp.p, ctx->st);   // element n = total (is_seed[n] unused but allocated)
    HIPCHK(hipMemcpyAsync(&U, seed_rank.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
  }
  ctx->U = U; ctx->U_active = U;
  HIPCHK(ctx->d_seed_read.alloc((size_t)U + 1)); HIPCHK(ctx->d_abund.alloc((size_t)U + 1)); HIPCHK(ctx->d_sorted_uniq.alloc((size_t)U + 1));
  HIPCHK(ctx->d_ulen.alloc((size_t)U + 1));
  HIPCHK(hipMemsetAsync(ctx->d_abund.p, 0, ((size_t)U + 1) * sizeof(int32_t), ctx->st));
  if (n > 0) launch_uniques(n, ctx->d_rep_of.p, seed_rank.p, ctx->d_uniq_of.p, ctx->d_seed_read.p, ctx->d_abund.p, ctx->st);
  // order the uniques by length (counting sort) for the HMM stages
  if (U > 0) {
    const int32_t lcap = 65536;
    DBuf<int32_t> &hist = ctx->w_hist, &cursor = ctx->w_cursor, &tmp2 = ctx->w_tmp2;
    HIPCHK(hist.alloc(lcap)); HIPCHK(cursor.alloc(lcap)); HIPCHK(tmp2.alloc((size_t)scan_tmp_elems(lcap)));
    HIPCHK(hipMemsetAsync(hist.p, 0, lcap * sizeof(int32_t), ctx->st));
    launch_len_hist(U, ctx->d_seed_read.p, ctx->rd.len, hist.p, lcap, ctx->st, ctx->Lmax + 1);
    launch_exclusive_scan(hist.p, cursor.p, lcap, tmp2.p, ctx->st);
    launch_len_scatter(U, ctx->d_seed_read.p, ctx->rd.len, cursor.p, lcap, ctx->d_sorted_uniq.p, ctx->st, ctx->Lmax + 1);
    launch_fill_ulen(U, ctx->d_sorted_uniq.p, ctx->d_seed_read.p, ctx->rd.len, ctx->d_ulen.p, ctx->st);
    HIPCHK(hipStreamSynchronize(ctx->st));
  }
  return ITSX_OK;
}
static int mirror_derep(itsx_ctx *ctx)
{
  const int64_t n = ctx->N; const int32_t U = ctx->U;
  // host mirrors (writers, getters)
  ctx->h_rep_of.resize((size_t)n); ctx->h_strand.resize((size_t)n); ctx->h_uniq_of.resize((size_t)n);
  ctx->h_seed_read.resize((size_t)U); ctx->h_abund.resize((size_t)U); ctx->h_sorted_uniq.resize((size_t)U);
  if (n > 0) {
    HIPCHK(hipMemcpy(ctx->h_rep_of.data(), ctx->d_rep_of.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ctx->h_strand.data(), ctx->d_strand.p, (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ctx->h_uniq_of.data(), ctx->d_uniq_of.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  if (U > 0) {
    HIPCHK(hipMemcpy(ctx->h_seed_read.data(), ctx->d_seed_read.p, (size_t)U * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ctx->h_abund.data(), ctx->d_abund.p, (size_t)U * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ctx->h_sorted_uniq.data(), ctx->d_sorted_uniq.p, (size_t)U * 4, hipMemcpyDeviceToHost));
  }
  ctx->h_sorted_active = ctx->h_sorted_uniq;
  if (ctx->S > 1) {
    ctx->h_usample.resize((size_t)U);
    for (int32_t u = 0; u < U; u++) ctx->h_usample[(size_t)u] = ctx->h_sample[(size_t)ctx->h_seed_read[(size_t)u]];
    HIPCHK(upload(ctx->d_usample, ctx->h_usample, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
  }
  return ITSX_OK;
}

int itsx_derep(itsx_ctx *ctx, int strand_both, int minseqlength, int64_t *n_unique)
{
  CTXCHK(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  LoadPriority load_priority(ctx);
  StageTxn txn(ctx, itsx_ctx::ST_READS);
  const int64_t n = ctx->N;
  StageTimer tm(ctx->st);
  DBuf<uint64_t> &hf = ctx->w_hf, &hr = ctx->w_hr; DBuf<unsigned long long> &keys = ctx->w_keys;
  DBuf<int32_t> &vals = ctx->w_vals, &is_seed = ctx->w_is_seed, &seed_rank = ctx->w_seed_rank, &scan_tmp = ctx->w_scan_tmp;
  DBuf<uint32_t> &slot_of = ctx->w_slot_of; DBuf<unsigned int> &ncoll = ctx->w_ncoll;
  HIPCHK(hf.alloc((size_t)n + 1)); HIPCHK(hr.alloc((size_t)n + 1));
  uint64_t tsize = 1024; while (tsize < (uint64_t)n * 2 + 16) tsize <<= 1;
  HIPCHK(keys.alloc(tsize)); HIPCHK(vals.alloc(tsize)); HIPCHK(slot_of.alloc((size_t)n + 1)); HIPCHK(ncoll.alloc(1));
  HIPCHK(is_seed.alloc((size_t)n + 1)); HIPCHK(seed_rank.alloc((size_t)n + 1)); HIPCHK(scan_tmp.alloc((size_t)scan_tmp_elems(n + 1)));
  HIPCHK(hipMemsetAsync(is_seed.p, 0, ((size_t)n + 1) * sizeof(int32_t), ctx->st));
  HIPCHK(ctx->d_rep_of.alloc((size_t)n + 1)); HIPCHK(ctx->d_strand.alloc((size_t)n + 1)); HIPCHK(ctx->d_uniq_of.alloc((size_t)n + 1));
  unsigned int hcoll = 0;
  uint64_t seed = 0;
  ctx->stats.hash_reseeds = 0;
  for (int attempt = 0; attempt < 4; attempt++) {
    HIPCHK(hipMemsetAsync(keys.p, 0, tsize * sizeof(unsigned long long), ctx->st));
    HIPCHK(hipMemsetAsync(vals.p, 0x7f, tsize * sizeof(int32_t), ctx->st));
    HIPCHK(hipMemsetAsync(ncoll.p, 0, sizeof(unsigned int), ctx->st));
    if (n > 0) {
      launch_hash_reads(ctx->rd, seed, strand_both, hf.p, hr.p, ctx->st, ctx->dev_sample());
      launch_table_insert(n, ctx->rd.len, minseqlength, hf.p, hr.p, keys.p, vals.p, tsize - 1, slot_of.p, ctx->st);
      launch_table_resolve(ctx->rd, hf.p, vals.p, slot_of.p, ctx->d_rep_of.p, ctx->d_strand.p, is_seed.p, ncoll.p, ctx->st, ctx->dev_sample());
    }
    HIPCHK(hipMemcpyAsync(&hcoll, ncoll.p, sizeof(hcoll), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (hcoll == 0) break;
    seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
    ctx->stats.hash_reseeds++;
  }
  if (hcoll != 0) SET_ERR(ctx, ITSX_E_COLLISION, "64-bit key collisions survived 4 reseeds");
  { const int rc_ = build_unique_lists(ctx); if (rc_ != ITSX_OK) return rc_; }
  ctx->stats.ms_derep = tm.stop();
  HIPCHK(hipGetLastError());
  { const int rc_ = mirror_derep(ctx); if (rc_ != ITSX_OK) return rc_; }
  const int32_t U = ctx->U;
  int64_t dropped = 0;
  for (int64_t r = 0; r < n; r++) dropped += ctx->h_rep_of[r] < 0;
  ctx->stats.n_unique = U; ctx->stats.n_dropped_short = dropped;
  ctx->derep_strand_both = strand_both != 0;
  if (n_unique) *n_unique = U;
  txn.commit(itsx_ctx::ST_GROUPED);
  return ITSX_OK;
}

// vsearch's DUST soft mask (mask.cc dust() / wo()) on the host, for the orientation database (the reads are masked on the device by
// k_dust, same procedure): windows of 64 advancing by 32, 3-mer repeat score 10 * sum / j, masked above 20
static bool qmask_dust() { const char *e = sw_get("ITSX_QMASK"); return !(e && strcmp(e, "none") == 0); }
static void dust_host(const uint8_t *codes, int64_t L, std::vector<uint8_t> &masked)
{
  masked.assign((size_t)L, 0);
  for (int64_t i = 0; i < L; i += 32) {
    const int len = (L > i + 64) ? 64 : (int)(L - i);
    const int l1 = len - 7;
    int bestv = 0, besti = 0, bestj = 0;
    if (l1 >= 0) {
      int words[64], counts[64], word = 0;
      for (int j = 0; j < len; j++) { const int c = codes[i + j]; word = (word << 2) | (c < 4 ? c : 0); words[j] = word & 63; }
      for (int a = 0; a < l1; a++) {
        memset(counts, 0, sizeof(counts));
        int sum = 0;
        for (int j = 2; j < len - a; j++) {
          const int w = words[a + j], c = counts[w];
          if (c) { sum += c; const int v = 10 * sum / j; if (v > bestv) { bestv = v; besti = a; bestj = j; } }
          counts[w]++;
        }
      }
    }
    if (bestv > 20) {
      const int b = besti + bestj;
      for (int64_t j = besti + i; j <= b + i; j++) masked[(size_t)j] = 1;
      if (b < 32) i += 32 - b;
    }
  }
}

// a2: greedy centroid clustering (k_cluster.hip explains the speculative windows).  batched: every sample of the batch is
// clustered as a run of that sample alone, the samples' windows advancing side by side as the segments of shared windows.
// shards (itsx_cluster_multi): the mode-1 centroid stream is spread over the leader and helper contexts (cluster_multi.hip).
static int cluster_run(itsx_ctx *ctx, double id, int strand_both, int64_t *n_unique, bool batched, ClusterShards *shards = nullptr)
{
  HIPCHK(hipSetDevice(ctx->device));
  StageTxn txn(ctx, itsx_ctx::ST_READS);
  const int64_t n = ctx->N;
  const int minlen = 32;
  const int32_t S = batched ? ctx->S : 1;
  StageTimer tm(ctx->st);
  // processing order: abundance (all 1) descending, then label, then input position -- inside each sample, the samples one
  // after another; sample s owns processing positions and centroid columns [sstart[s], sstart[s + 1])
  std::vector<int32_t> ord; ord.reserve((size_t)n);
  std::vector<int32_t> sstart((size_t)S + 1, 0);
  int Lmax = 1;
  for (int64_t r = 0; r < n; r++)                          // vsearch defaults: --minseqlength 32, --maxseqlength 50000
    if (ctx->h_len[r] >= minlen && ctx->h_len[r] <= 50000) {
      ord.push_back((int32_t)r); Lmax = std::max(Lmax, (int)ctx->h_len[r]);
      sstart[batched ? (size_t)ctx->h_sample[(size_t)r] + 1 : 1]++;
    }
  for (int32_t s = 0; s < S; s++) sstart[(size_t)s + 1] += sstart[(size_t)s];
  std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
    if (batched && ctx->h_sample[(size_t)a] != ctx->h_sample[(size_t)b]) return ctx->h_sample[(size_t)a] < ctx->h_sample[(size_t)b];
    const int c = ctx->h_names.empty() ? 0 : ctx->h_names.cmp((size_t)a, (size_t)b);
    return c < 0 || (c == 0 && a < b);
  });
  const int32_t nk = (int32_t)ord.size();
  int Bmax = 4096;                                          // k_cl_resolve keeps the window's flags in LDS
  if (const char *e = sw_get("ITSX_CL_WINDOW")) Bmax = std::min(4096, std::max(1, atoi(e)));
  // DP rows per lane of the alignment wave: 64 lanes x S rows hold the whole query when Lmax + 1 <= 64 S; the lanes past the
  // query's end idle, so S is the smallest that fits (2x250-merged reads of <= 480 bases: S = 8, not 10: 78 % instead of 62 % busy)
  int rows_per_lane = (Lmax + 1 <= 320) ? 5 : (Lmax + 1 <= 512) ? 8 : 10;
  if (const char *e = sw_get("ITSX_CL_ROWS")) rows_per_lane = atoi(e) <= 5 ? 5 : atoi(e) <= 8 ? 8 : 10;
  const bool multipass = Lmax + 1 > 64 * rows_per_lane;
  const int32_t scratch_pitch = Lmax + 1;
  if (multipass) while (Bmax > 16 && 2LL * Bmax * 32 * scratch_pitch * 16 > (4LL << 30)) Bmax /= 2;
  const int32_t kcap = std::max(8, ((Lmax - 7 + 7) / 8) * 8);

  DBuf<int32_t> d_order, cent_len, cent_pos, cent_read, res_col, knk, state, rejects, acc_col, is_new, new_rank, scan_tmp, xlist, xn, hard, dbg;
  DBuf<int32_t> sel, selm, sel_short, wn, wcol, newq, rm, wout, work, xwork, work_n, replay, skipm, canon, ctab_val, need, awork, spairs;
  DBuf<int32_t> cw_n, wsum, wscan, qi_cnt, qi_cur, qi_off, ncand, ntop, ovf, qi_hid, qi_nheavy, cent_q, segtab, qpos, qseg, newcol;
  DBuf<uint32_t> qi_bm;
  DBuf<int64_t> cw_off;
  DBuf<uint16_t> klist, cw_poolA, cw_poolB, qi_ent, cntx; DBuf<uint32_t> tq, minm;
  DBuf<unsigned long long> ctab_key, n_skipped, pre_stats, cand, tkey;
  DBuf<int8_t> res_strand; DBuf<double> res_id, acc_id, d_pct, selpid, wpid, xpid;
  DBuf<unsigned long long> prev, bound, selkey, wkey, xkey, scratch, n_align;
  DBuf<uint16_t> *cw_pool = &cw_poolA, *cw_other = &cw_poolB;
  HIPCHK(upload(d_order, ord, ctx->st));
  const size_t ccap = (size_t)nk + 2048;
  HIPCHK(cent_len.alloc(ccap)); HIPCHK(cent_pos.alloc(ccap)); HIPCHK(cent_read.alloc(ccap));
  HIPCHK(cw_n.alloc(ccap)); HIPCHK(cw_off.alloc(ccap + 1)); HIPCHK(cent_q.alloc(ccap));
  HIPCHK(res_col.alloc((size_t)nk + 1)); HIPCHK(res_strand.alloc((size_t)nk + 1)); HIPCHK(res_id.alloc((size_t)nk + 1));
  const size_t nqs = 2 * (size_t)Bmax;
  HIPCHK(klist.alloc(nqs * kcap)); HIPCHK(knk.alloc(nqs)); HIPCHK(state.alloc(nqs)); HIPCHK(rejects.alloc(nqs));
  HIPCHK(acc_col.alloc(nqs)); HIPCHK(prev.alloc(nqs)); HIPCHK(bound.alloc(nqs)); HIPCHK(acc_id.alloc(nqs));
  HIPCHK(sel.alloc(nqs * 32)); HIPCHK(selm.alloc(nqs)); HIPCHK(sel_short.alloc(nqs)); HIPCHK(selkey.alloc(nqs * 32)); HIPCHK(selpid.alloc(nqs * 32));
  HIPCHK(wn.alloc(nqs)); HIPCHK(wcol.alloc(nqs * 32)); HIPCHK(wkey.alloc(nqs * 32)); HIPCHK(wpid.alloc(nqs * 32));
  HIPCHK(xlist.alloc(nqs * 32)); HIPCHK(xn.alloc(nqs)); HIPCHK(hard.alloc(nqs)); HIPCHK(xkey.alloc(nqs * 32)); HIPCHK(xpid.alloc(nqs * 32));
  HIPCHK(is_new.alloc((size_t)Bmax + 1)); HIPCHK(new_rank.alloc((size_t)Bmax + 1)); HIPCHK(newq.alloc((size_t)Bmax + 1)); HIPCHK(rm.alloc((size_t)Bmax + 1));
  HIPCHK(wsum.alloc((size_t)Bmax + 1)); HIPCHK(wscan.alloc((size_t)Bmax + 1));
  HIPCHK(segtab.alloc(5 * ((size_t)Bmax + 1))); HIPCHK(qpos.alloc((size_t)Bmax)); HIPCHK(qseg.alloc((size_t)Bmax)); HIPCHK(newcol.alloc((size_t)Bmax));
  HIPCHK(wout.alloc(3 * (size_t)Bmax + 1)); HIPCHK(dbg.alloc(4)); HIPCHK(work.alloc(nqs * 32)); HIPCHK(xwork.alloc(nqs * 32)); HIPCHK(work_n.alloc(8)); HIPCHK(awork.alloc(2 * nqs * 32)); HIPCHK(spairs.alloc(4 * nqs * 32)); HIPCHK(replay.alloc((size_t)Bmax + 1)); HIPCHK(skipm.alloc((size_t)Bmax + 1)); HIPCHK(canon.alloc((size_t)Bmax + 1)); HIPCHK(need.alloc(2 * nqs * 32)); HIPCHK(n_skipped.alloc(1)); HIPCHK(pre_stats.alloc(16)); HIPCHK(hipMemsetAsync(pre_stats.p, 0, 16 * sizeof(unsigned long long), ctx->st));
  HIPCHK(hipMemsetAsync(n_skipped.p, 0, sizeof(unsigned long long), ctx->st)); HIPCHK(ctab_key.alloc(16384)); HIPCHK(ctab_val.alloc(16384));
  HIPCHK(ctx->w_hf.alloc((size_t)n + 1)); HIPCHK(ctx->w_hr.alloc((size_t)n + 1));
  // identical reads of a window share one search (a batch: identical reads of one sample -- the hash carries the sample)
  if (n > 0) launch_hash_reads(ctx->rd, 0, 0, ctx->w_hf.p, ctx->w_hr.p, ctx->st, batched ? ctx->dev_sample() : nullptr);
  // vsearch's default --qmask dust / --dbmask dust: the DUST soft mask of every read (queries and centroids alike), once
  DBuf<uint32_t> dmask;
  const bool use_dust = qmask_dust();
  if (use_dust && n > 0) { HIPCHK(dmask.alloc((size_t)ctx->h_woff[n] + 1)); launch_dust(ctx->rd, dmask.p, ctx->st); }
  HIPCHK(scan_tmp.alloc((size_t)scan_tmp_elems(65537 + Bmax + 1))); HIPCHK(n_align.alloc(1));
  HIPCHK(scratch.alloc(multipass ? nqs * 32 * (size_t)scratch_pitch * 2 : 2));
  HIPCHK(hipMemsetAsync(n_align.p, 0, sizeof(unsigned long long), ctx->st));
  // the window's query index, the strands' thresholds and candidate lists, the counts against the window's own centroids
  HIPCHK(qi_cnt.alloc(65537)); HIPCHK(qi_cur.alloc(65536)); HIPCHK(qi_off.alloc(65537));
  HIPCHK(qi_ent.alloc(nqs * (size_t)kcap + 65536 * 8 + 64));
  int32_t hcap = 16384;                                     // strand bitmaps of conserved words (1 KB each); ITSX_CL_HEAVY=0: every word keeps its list
  if (const char *e = sw_get("ITSX_CL_HEAVY")) hcap = std::max(0, std::min(65536, atoi(e)));
  HIPCHK(qi_hid.alloc(65536)); HIPCHK(qi_nheavy.alloc(1)); HIPCHK(qi_bm.alloc((size_t)std::max(hcap, 1) * (CL_QS_MAX / 32)));
  HIPCHK(tq.alloc(CL_QS_MAX + 8)); HIPCHK(minm.alloc(CL_QS_MAX + 8)); HIPCHK(tkey.alloc(nqs)); HIPCHK(ncand.alloc(nqs)); HIPCHK(ntop.alloc(nqs)); HIPCHK(ovf.alloc(1));
  int32_t cand_cap = 4096;                                  // per strand; grows (and the window is searched again) when a list overflows
  if (const char *e = sw_get("ITSX_CL_CCAP")) cand_cap = std::max(32, atoi(e));
  HIPCHK(cand.alloc(nqs * (size_t)cand_cap));
  HIPCHK(cntx.alloc(nqs * (size_t)Bmax));
  int64_t pool_cap = 1LL << 26;                             // words of all centroids; doubles (with a copy) when a window could overrun it
  if (const char *e = sw_get("ITSX_CL_CAPACITY")) pool_cap = std::max<int64_t>(2048, atoll(e));
  pool_cap = std::max<int64_t>(pool_cap, (int64_t)Bmax * kcap);
  HIPCHK(cw_pool->alloc((size_t)pool_cap, true));
  int64_t pool_used = 0;
  struct ShardGuard { ClusterShards *s; ~ShardGuard() { if (s) s->sync(); } } shard_guard{shards};   // (no helper copy outlives the buffers above)

  ClusterArgs a{};
  a.rd = ctx->rd; a.order = d_order.p; a.strand_both = strand_both ? 1 : 0; a.dmask = (use_dust && n > 0) ? dmask.p : nullptr;
  a.cent_len = cent_len.p; a.cent_pos = cent_pos.p; a.cent_read = cent_read.p;
  a.klist = klist.p; a.kcap = kcap; a.nk = knk.p;
  a.cw_off = cw_off.p; a.cw_n = cw_n.p; a.wsum = wsum.p; a.wscan = wscan.p;
  a.cent_q = cent_q.p; a.qpos = qpos.p; a.qseg = qseg.p; a.newcol = newcol.p;
  a.qi_cnt = qi_cnt.p; a.qi_cur = qi_cur.p; a.qi_off = qi_off.p; a.qi_ent = qi_ent.p;
  a.qi_hid = qi_hid.p; a.qi_nheavy = qi_nheavy.p; a.qi_bm = qi_bm.p; a.hcap = hcap;
  a.heavy_min = CL_HEAVY;                                    // ITSX_CL_HEAVY_MIN: strands that must hold a word before it gets a bitmap (tuning; results do not depend on it)
  if (const char *e = sw_get("ITSX_CL_HEAVY_MIN")) a.heavy_min = std::max(8, atoi(e));
  a.tq = tq.p; a.minm = minm.p; a.tkey = tkey.p; a.ncand = ncand.p; a.ntop = ntop.p; a.ovf = ovf.p; a.cntx = cntx.p;
  a.state = state.p; a.rejects = rejects.p; a.acc_col = acc_col.p; a.prev = prev.p; a.bound = bound.p; a.acc_id = acc_id.p;
  a.sel = sel.p; a.selm = selm.p; a.sel_short = sel_short.p; a.selkey = selkey.p; a.selpid = selpid.p;
  a.wn = wn.p; a.wcol = wcol.p; a.wkey = wkey.p; a.wpid = wpid.p;
  a.res_col = res_col.p; a.res_strand = res_strand.p; a.res_id = res_id.p;
  a.is_new = is_new.p; a.new_rank = new_rank.p; a.newq = newq.p; a.rm = rm.p;
  a.xlist = xlist.p; a.xn = xn.p; a.hard = hard.p; a.xkey = xkey.p; a.xpid = xpid.p; a.wout = wout.p; a.dbg = dbg.p; a.work = work.p; a.xwork = xwork.p; a.work_n = work_n.p; a.awork = awork.p; a.spairs = spairs.p; a.replay = replay.p; a.skipm = skipm.p; a.canon = canon.p; a.need = sw_get("ITSX_CL_NOPRECHECK") ? nullptr : need.p; a.need_pitch = (int32_t)(nqs * 32); a.n_skipped = n_skipped.p; a.pre_stats = pre_stats.p;
  a.use_score = sw_get("ITSX_CL_NOSCORE") ? 0 : 1;
  a.pre_k = std::min(16, (int)((double)Lmax * (1.0 - id) / id) + 1); a.ctab_key = ctab_key.p; a.ctab_val = ctab_val.p; a.rhash = ctx->w_hf.p;
  a.scratch = scratch.p; a.scratch_pitch = scratch_pitch;
  a.thr = 100.0 * id; a.n_align = n_align.p;
  if (shards) {
    ClusterArgs ai = a; ai.ccap = cand_cap;
    if (shards->init(ai, (int32_t)nqs, nk, pool_cap) != hipSuccess) SET_ERR(ctx, ITSX_E_DEVICE, "clustering shards: " + shards->error());
  }

  // per sample: queries done f, centroid columns C, adaptive segment size B (start 256, double after an uncut segment,
  // max(64, 2 cut) after a cut).  A window takes a segment of every unfinished sample in sample order until it holds Bmax queries.
  std::vector<int32_t> sf((size_t)S, 0), sC((size_t)S, 0), sB((size_t)S, std::min(Bmax, 256));
  std::vector<int32_t> tab, wsmp, wo;                        // the window's segment table (5 rows of G + 1), its samples, the outcome
  int32_t first = 0, ncent = 0;
  int64_t windows = 0, cuts = 0, regrown = 0, stream_launches = 0;
  const bool debug = sw_get("ITSX_CL_DEBUG") != nullptr;
  for (;;) {
    while (first < S && sf[(size_t)first] >= sstart[(size_t)first + 1] - sstart[(size_t)first]) first++;
    if (first >= S) break;
    int nq = 0, Ctot = 0;
    wsmp.clear();
    std::vector<int32_t> q0, cb, base, cs, pos0;
    for (int32_t s = first; s < S && nq < Bmax; s++) {
      const int32_t rem = sstart[(size_t)s + 1] - sstart[(size_t)s] - sf[(size_t)s];
      if (rem <= 0) continue;
      const int32_t take = std::min(std::min(sB[(size_t)s], rem), Bmax - nq);
      wsmp.push_back(s); q0.push_back(nq); cb.push_back(Ctot); base.push_back(sstart[(size_t)s]); cs.push_back(sC[(size_t)s]);
      pos0.push_back(sstart[(size_t)s] + sf[(size_t)s]);
      nq += take; Ctot += sC[(size_t)s];
    }
    const int32_t G = (int32_t)wsmp.size();
    q0.push_back(nq); cb.push_back(Ctot); base.push_back(0); cs.push_back(0); pos0.push_back(0);
    tab.clear();
    for (const std::vector<int32_t> *v : {&q0, &cb, &base, &cs, &pos0}) tab.insert(tab.end(), v->begin(), v->end());
    HIPCHK(hipMemcpyAsync(segtab.p, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->st));
    a.G = G; a.seg = G > 1 ? 1 : 0;
    a.sg_q0 = segtab.p; a.sg_cb = segtab.p + (G + 1); a.sg_base = segtab.p + 2 * (G + 1); a.sg_C = segtab.p + 3 * (G + 1); a.sg_pos0 = segtab.p + 4 * (G + 1);
    if (pool_used + (int64_t)nq * kcap > pool_cap) {          // the window's would-be centroids could overrun the word pool: grow it
      int64_t ncap = pool_cap;
      while (pool_used + (int64_t)nq * kcap > ncap) ncap *= 2;
      HIPCHK(cw_other->alloc((size_t)ncap, true));
      HIPCHK(hipMemcpyAsync(cw_other->p, cw_pool->p, (size_t)pool_used * sizeof(uint16_t), hipMemcpyDeviceToDevice, ctx->st));
      HIPCHK(hipStreamSynchronize(ctx->st));
      std::swap(cw_pool, cw_other); cw_other->release();
      pool_cap = ncap;
    }
    a.nq = nq; a.pool0 = pool_used; a.cw_pool = cw_pool->p; a.cand = cand.p; a.ccap = cand_cap; a.xpitch = nq;
    launch_cl_segs(a, ctx->st);
    launch_cl_kmers(a, ctx->st);
    // every centroid streams past the window's query index; a strand keeps the candidates that can still be among its 32 best
    launch_cl_qindex(a, scan_tmp.p, ctx->st);
    if (shards) {                                              // each shard streams its own columns; their lists meet on the leader
      if (shards->stream(a, stream_launches) != hipSuccess) SET_ERR(ctx, ITSX_E_DEVICE, "clustering shards: " + shards->error());
    } else
    for (int c0 = 0, step = 2048; c0 < Ctot; step = std::min(step * 2, 1 << 20)) {
      const int c1 = std::min(Ctot, c0 + step);
      launch_cl_stream(a, c0, c1, 1, ctx->st);
      stream_launches++;
      if (c1 < Ctot) launch_cl_topk(a, 0, ctx->st);              // cut the lists back to their 32 best, raise the thresholds
      c0 = c1;
    }
    launch_cl_topk(a, 1, ctx->st);
    {   // a candidate list that overflowed is known HERE: the window is searched again before its walk, its validation and their
        // counters have run (they ran first and were counted twice until round 3: advisor)
      int32_t early = 0;
      HIPCHK(hipMemcpyAsync(&early, ovf.p, sizeof(early), hipMemcpyDeviceToHost, ctx->st));
      HIPCHK(hipStreamSynchronize(ctx->st));
      if (early) {
        if ((int64_t)cand_cap >= (int64_t)Ctot) SET_ERR(ctx, ITSX_E_DEVICE, "clustering candidate lists overflow although they hold every centroid");
        cand_cap *= 4;
        HIPCHK(cand.alloc(nqs * (size_t)cand_cap));
        regrown++;
        continue;
      }
    }
    launch_cl_init(a, ctx->st);
    if (Ctot > 0) launch_cl_walk(a, rows_per_lane, ctx->st);
    launch_cl_outcome(a, ctx->st);
    launch_exclusive_scan(is_new.p, new_rank.p, nq + 1, scan_tmp.p, ctx->st);
    launch_cl_wsum(a, ctx->st);
    launch_exclusive_scan(wsum.p, wscan.p, nq + 1, scan_tmp.p, ctx->st);
    launch_cl_columns(a, 0, ctx->st);
    HIPCHK(hipMemsetAsync(cntx.p, 0, (size_t)2 * nq * nq * sizeof(uint16_t), ctx->st));
    launch_cl_stream(a, 0, nq, 2, ctx->st);                   // the window's speculative centroids against their segments' strands
    launch_cl_validate(a, rows_per_lane, ctx->st);
    launch_cl_columns(a, 1, ctx->st);                         // roll back the speculative centroids that did not survive
    if (shards && shards->fetch_columns(a, cs[0]) != hipSuccess) SET_ERR(ctx, ITSX_E_DEVICE, "clustering shards: " + shards->error());
    int32_t overflow = 0;
    wo.assign(3 * (size_t)G + 1, 0);
    HIPCHK(hipMemcpyAsync(wo.data(), wout.p, wo.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(&overflow, ovf.p, sizeof(overflow), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());                              // a kernel that failed to launch must not pass silently
    if (overflow) {
      // a strand met more candidates at (or above) its threshold than its list holds -- long runs of equal counts: nothing of
      // this window is kept, the lists grow and the window is searched again (the centroid set has not changed yet)
      if ((int64_t)cand_cap >= (int64_t)Ctot) SET_ERR(ctx, ITSX_E_DEVICE, "clustering candidate lists overflow although they hold every centroid");
      cand_cap *= 4;
      HIPCHK(cand.alloc(nqs * (size_t)cand_cap));
      regrown++;
      continue;
    }
    if (debug) {
      int32_t d[4] = {0, 0, 0, 0};
      (void)hipMemcpy(d, dbg.p, sizeof(d), hipMemcpyDeviceToHost);
      std::vector<int32_t> hs(2 * (size_t)nq), hw(2 * (size_t)nq), hc(2 * (size_t)nq);
      (void)hipMemcpy(hs.data(), state.p, hs.size() * 4, hipMemcpyDeviceToHost);
      (void)hipMemcpy(hw.data(), wn.p, hw.size() * 4, hipMemcpyDeviceToHost);
      (void)hipMemcpy(hc.data(), ncand.p, hc.size() * 4, hipMemcpyDeviceToHost);
      long sc[4] = {0, 0, 0, 0}, sw[4] = {0, 0, 0, 0}, acc1 = 0, ncs = 0, ncm = 0;
      for (size_t q = 0; q < hs.size(); q++) { sc[hs[q] & 3]++; sw[hs[q] & 3] += hw[q]; acc1 += hs[q] == 1 && hw[q] == 1; ncs += hc[q]; ncm = std::max<long>(ncm, hc[q]); }
      fprintf(stderr, "[cluster] G=%d f=%d nq=%d C=%d cut=%d cols=%d new=%d | hard=%d budget=%d joined_new=%d xaligns=%d | accept %ld (first try %ld, walk %ld) rej32 %ld exhausted %ld (walk %ld) | appended %ld (max %ld per strand)\n",
              G, sf[(size_t)wsmp[0]], nq, Ctot, wo[0] - q0[0], wo[G], wo[2 * G], d[0], d[1], d[2], d[3], sc[1], acc1, sw[1], sc[2], sc[3], sw[3], ncs, ncm);
    }
    bool any_cut = false;
    for (int32_t g = 0; g < G; g++) {
      const size_t s = (size_t)wsmp[(size_t)g];
      const int32_t sq = q0[(size_t)g + 1] - q0[(size_t)g], cut = wo[(size_t)g] - q0[(size_t)g];
      if (cut < 1 || cut > sq) SET_ERR(ctx, ITSX_E_DEVICE, "clustering window validation returned an impossible cut");
      sC[s] += wo[(size_t)G + g]; ncent += wo[2 * (size_t)G + g]; sf[s] += cut; any_cut |= cut < sq;
      sB[s] = cut == sq ? std::min(Bmax, std::max(sB[s], sq) * 2) : std::min(Bmax, std::max(64, 2 * cut));
    }
    windows++; cuts += any_cut;
    pool_used += wo[3 * (size_t)G];                           // (the words of the last segment's rolled-back tail are taken again)
    if (shards && shards->adopt(a, cs[0], wo[(size_t)G]) != hipSuccess) SET_ERR(ctx, ITSX_E_DEVICE, "clustering shards: " + shards->error());
  }
  if (debug && shards) fprintf(stderr, "%s", shards->debug_line(windows).c_str());
  if (debug) fprintf(stderr, "[cluster] %lld windows, %lld stream launches, %lld regrown candidate lists, word pool %.1f MB\n", (long long)windows, (long long)stream_launches, (long long)regrown, pool_used * 2.0 / 1e6);

  HIPCHK(ctx->d_rep_of.alloc((size_t)n + 1)); HIPCHK(ctx->d_strand.alloc((size_t)n + 1)); HIPCHK(ctx->d_uniq_of.alloc((size_t)n + 1));
  HIPCHK(ctx->w_is_seed.alloc((size_t)n + 1)); HIPCHK(ctx->w_seed_rank.alloc((size_t)n + 1)); HIPCHK(ctx->w_scan_tmp.alloc((size_t)scan_tmp_elems(n + 1)));
  HIPCHK(d_pct.alloc((size_t)n + 1));
  HIPCHK(hipMemsetAsync(ctx->w_is_seed.p, 0, ((size_t)n + 1) * sizeof(int32_t), ctx->st));
  HIPCHK(hipMemsetAsync(ctx->d_rep_of.p, 0xff, ((size_t)n + 1) * sizeof(int32_t), ctx->st));
  HIPCHK(hipMemsetAsync(ctx->d_strand.p, 1, (size_t)n + 1, ctx->st));
  HIPCHK(hipMemsetAsync(d_pct.p, 0, ((size_t)n + 1) * sizeof(double), ctx->st));
  launch_cl_finalize(nk, d_order.p, res_col.p, res_strand.p, res_id.p, cent_read.p, ctx->d_rep_of.p, ctx->d_strand.p, d_pct.p, ctx->w_is_seed.p, ctx->st);
  { const int rc_ = build_unique_lists(ctx); if (rc_ != ITSX_OK) return rc_; }
  unsigned long long naln = 0, nskip = 0;
  HIPCHK(hipMemcpy(&naln, n_align.p, sizeof(naln), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&nskip, n_skipped.p, sizeof(nskip), hipMemcpyDeviceToHost));
  if (debug) {
    unsigned long long ps[16] = {0};
    (void)hipMemcpy(ps, pre_stats.p, sizeof(ps), hipMemcpyDeviceToHost);
    if (ps[12]) fprintf(stderr, "[cluster] stream phases (clock ticks per centroid and workgroup): pieces %.0f, list additions %.0f, scan %.0f, bitmaps %.0f (of which loads + adders %.0f); pieces per centroid %.0f\n",
                        (double)ps[8] / ps[12], (double)ps[9] / ps[12], (double)ps[10] / ps[12], (double)(ps[11] + ps[14]) / ps[12], (double)ps[14] / ps[12], (double)ps[13] / ps[12]);
    fprintf(stderr, "[cluster] certificate: not applicable %llu, bound too weak %llu (score pass: proven reject %llu, path exists %llu), path exists %llu, proven reject %llu; full alignments %llu\n", ps[0], ps[1], ps[4], ps[5], ps[2], ps[3], naln);
  }
  ctx->stats.ms_cluster = tm.stop();
  { const int rc_ = mirror_derep(ctx); if (rc_ != ITSX_OK) return rc_; }
  ctx->h_pct.assign((size_t)n, -1.0);
  if (n > 0) HIPCHK(hipMemcpy(ctx->h_pct.data(), d_pct.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t r = 0; r < n; r++) if (ctx->h_rep_of[r] < 0 || ctx->h_rep_of[r] == r) ctx->h_pct[r] = -1.0;
  ctx->h_order = ord;
  ctx->stats.n_unique = ctx->U; ctx->stats.n_dropped_short = n - nk;
  ctx->stats.cl_windows = windows; ctx->stats.cl_cuts = cuts; ctx->stats.cl_alignments = (int64_t)naln; ctx->stats.cl_certified = (int64_t)nskip;
  if (ctx->U != ncent) SET_ERR(ctx, ITSX_E_DEVICE, "clustering bookkeeping mismatch (centroids " + std::to_string(ncent) + " vs uniques " + std::to_string(ctx->U) + ")");
  if (n_unique) *n_unique = ctx->U;
  ctx->clustered = true;
  txn.commit(itsx_ctx::ST_GROUPED);
  return ITSX_OK;
}
int itsx_cluster(itsx_ctx *ctx, double id, int strand_both, int64_t *n_unique)
{
  CTXCHK(ctx);
  if (!(id > 0.0 && id <= 1.0)) SET_ERR(ctx, ITSX_E_ARG, "cluster id must be in (0, 1]");
  if (id == 1.0) return itsx_derep(ctx, strand_both, 32, n_unique);      // main.py:534-537 never clusters at 1.0
  if (ctx->S > 1) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "greedy clustering (id < 1) is sequential per sample: run it one sample per call, not on a sample batch");
  return cluster_run(ctx, id, strand_both, n_unique, false);
}
int itsx_cluster_multi(itsx_ctx *ctx, itsx_ctx *const *helpers, int32_t n_helpers, double id, int strand_both, int64_t *n_unique)
{
  CTXCHK(ctx);
  if (n_helpers < 0 || (n_helpers > 0 && !helpers)) SET_ERR(ctx, ITSX_E_ARG, "itsx_cluster_multi: helpers is NULL or n_helpers is negative");
  std::vector<ClusterShards::Helper> hs;
  for (int32_t h = 0; h < n_helpers; h++) {
    if (!helpers[h]) SET_ERR(ctx, ITSX_E_ARG, "itsx_cluster_multi: helper " + std::to_string(h) + " is NULL");
    if (helpers[h] == ctx) SET_ERR(ctx, ITSX_E_ARG, "itsx_cluster_multi: a helper is the leader context itself");
    for (int32_t g = 0; g < h; g++)
      if (helpers[g] == helpers[h]) SET_ERR(ctx, ITSX_E_ARG, "itsx_cluster_multi: helper " + std::to_string(h) + " appears twice");
    hs.push_back(ClusterShards::Helper{helpers[h]->device, helpers[h]->st});
  }
  if (n_helpers == 0) return itsx_cluster(ctx, id, strand_both, n_unique);
  if (!(id > 0.0 && id <= 1.0)) SET_ERR(ctx, ITSX_E_ARG, "cluster id must be in (0, 1]");
  if (id == 1.0) return itsx_derep(ctx, strand_both, 32, n_unique);      // as itsx_cluster
  if (ctx->S > 1) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "greedy clustering (id < 1) is sequential per sample: run it one sample per call, not on a sample batch");
  ClusterShards shards(ctx->device, ctx->st, hs);
  return cluster_run(ctx, id, strand_both, n_unique, false, &shards);
}
int itsx_cluster_samples(itsx_ctx *ctx, double id, int strand_both, int64_t *n_unique)
{
  CTXCHK(ctx);
  if (!(id > 0.0 && id <= 1.0)) SET_ERR(ctx, ITSX_E_ARG, "cluster id must be in (0, 1]");
  if (id == 1.0) return itsx_derep(ctx, strand_both, 32, n_unique);      // as itsx_cluster: a batched derep keeps every sample apart
  if (ctx->S <= 1) return itsx_cluster(ctx, id, strand_both, n_unique);
  return cluster_run(ctx, id, strand_both, n_unique, true);
}

int itsx_get_cluster(const itsx_ctx *ctx, double *pct_id, int64_t *order, int64_t *n_order)
{
  CTXCHK(ctx && ctx->grouped() && ctx->clustered);
  if (pct_id) for (int64_t r = 0; r < ctx->N; r++) pct_id[r] = ctx->h_pct[r];
  if (order) for (size_t i = 0; i < ctx->h_order.size(); i++) order[i] = ctx->h_order[i];
  if (n_order) *n_order = (int64_t)ctx->h_order.size();
  return ITSX_OK;
}

// uc column 8 (k_cigar.hip): every member of the current clustering aligned with its centroid once more, this time with the path.
// The pairs go in batches under a byte budget (ITSX_CIGAR_MB: the direction bits of a pair are about (Lq + 1)(Lt + 1) / 2 bytes);
// a pair larger than the budget is a batch of its own, in an allocation of its own size.
int itsx_align_clusters(itsx_ctx *ctx, int64_t *n_aligned, float *ms_kernels)
{
  CTXCHK(ctx);
  if (!ctx->grouped() || !ctx->clustered) SET_ERR(ctx, ITSX_E_ARG, "itsx_align_clusters comes after a clustering at id < 1 (itsx_cluster, itsx_cluster_multi, itsx_cluster_samples); exact dereplication has nothing to align");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->drop_cigars();
  const int64_t n = ctx->N;
  hipStream_t st = ctx->st;
  std::vector<int32_t> hq, ht; std::vector<int8_t> hs;
  int Lmax = 1;
  for (int64_t r = 0; r < n; r++) {
    const int32_t rep = ctx->h_rep_of[(size_t)r];
    if (rep < 0 || rep == r) continue;
    hq.push_back((int32_t)r); ht.push_back(rep); hs.push_back(ctx->h_strand[(size_t)r]);
    Lmax = std::max(Lmax, std::max((int)ctx->h_len[(size_t)r], (int)ctx->h_len[(size_t)rep]));
  }
  const size_t M = hq.size();
  float ms = 0.0f;
  std::vector<std::string> text(M);
  if (M > 0) {
    // rows per lane as the clustering chooses them (cluster_run): the smallest variant that holds the longest read in one pass
    int rows_per_lane = (Lmax + 1 <= 320) ? 5 : (Lmax + 1 <= 512) ? 8 : 10;
    if (const char *e = sw_get("ITSX_CL_ROWS")) rows_per_lane = atoi(e) <= 5 ? 5 : atoi(e) <= 8 ? 8 : 10;
    double budget_mb = 2048.0;
    if (const char *e = sw_get("ITSX_CIGAR_MB")) budget_mb = std::max(0.0, atof(e));
    const size_t budget = (size_t)(budget_mb * 1048576.0);
    DBuf<int32_t> d_q, d_t, d_eq, d_tlen; DBuf<int8_t> d_s; DBuf<int64_t> d_doff, d_soff, d_toff;
    DBuf<uint8_t> d_dir, d_text; DBuf<long long> d_scr, d_res; DBuf<double> d_pid;
    HIPCHK(upload(d_q, hq, st)); HIPCHK(upload(d_t, ht, st)); HIPCHK(upload(d_s, hs, st));
    HIPCHK(d_eq.alloc(M)); HIPCHK(d_res.alloc(M)); HIPCHK(d_pid.alloc(M));
    CigarArgs a{};
    a.rd = ctx->rd; a.q_read = d_q.p; a.t_read = d_t.p; a.strand = d_s.p; a.res = d_res.p; a.pid = d_pid.p;
    std::vector<int32_t> eq(M);
    launch_cg_equal(a, (int32_t)M, d_eq.p, st);
    HIPCHK(hipMemcpyAsync(eq.data(), d_eq.p, M * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // the pairs that need the dynamic program, in member order, with their places in their batch
    std::vector<int32_t> pq, pt, pm; std::vector<int8_t> ps; std::vector<int64_t> doff, soff;
    struct Batch { size_t p0, np, dir_bytes, scr_elems; };
    std::vector<Batch> batches;
    for (size_t m = 0; m < M; m++) {
      if (eq[m]) { text[m] = "="; continue; }
      size_t db = 0, sb = 0;
      cg_pair_bytes(ctx->h_len[(size_t)hq[m]], ctx->h_len[(size_t)ht[m]], rows_per_lane, &db, &sb);
      db = (db + 255) & ~(size_t)255;
      if (batches.empty() || (batches.back().np > 0 && batches.back().dir_bytes + batches.back().scr_elems * 8 + db + sb > budget)) batches.push_back(Batch{pq.size(), 0, 0, 0});
      Batch &b = batches.back();
      doff.push_back((int64_t)b.dir_bytes); soff.push_back((int64_t)b.scr_elems);
      b.np++; b.dir_bytes += db; b.scr_elems += sb / 8;
      pq.push_back(hq[m]); pt.push_back(ht[m]); ps.push_back(hs[m]); pm.push_back((int32_t)m);
    }
    const size_t NP = pq.size();
    if (NP > 0) {
      size_t max_dir = 0, max_scr = 0, max_np = 0;
      for (const Batch &b : batches) { max_dir = std::max(max_dir, b.dir_bytes); max_scr = std::max(max_scr, b.scr_elems); max_np = std::max(max_np, b.np); }
      HIPCHK(upload(d_q, pq, st)); HIPCHK(upload(d_t, pt, st)); HIPCHK(upload(d_s, ps, st)); HIPCHK(upload(d_doff, doff, st)); HIPCHK(upload(d_soff, soff, st));
      if (d_dir.alloc(max_dir + 256, true) != hipSuccess || d_scr.alloc(max_scr + 2, true) != hipSuccess) {
        (void)hipGetLastError();
        SET_ERR(ctx, ITSX_E_NOMEM, "itsx_align_clusters: no device memory for " + std::to_string((max_dir + max_scr * 8) >> 20) + " MB of direction bits (lower ITSX_CIGAR_MB; a pair larger than the budget needs its own size)");
      }
      HIPCHK(d_tlen.alloc(max_np)); HIPCHK(d_toff.alloc(max_np + 1));
      a.q_read = d_q.p; a.t_read = d_t.p; a.strand = d_s.p; a.dir_off = d_doff.p; a.scr_off = d_soff.p;
      a.dir = d_dir.p; a.scratch = d_scr.p; a.tlen = d_tlen.p; a.toff = d_toff.p;
      std::vector<int32_t> tlen; std::vector<int64_t> toff; std::vector<char> plane;
      for (const Batch &b : batches) {
        StageTimer t1(st);
        launch_cg_forward(a, (int32_t)b.p0, (int32_t)b.np, rows_per_lane, Lmax, st);
        launch_cg_traceback(a, (int32_t)b.p0, (int32_t)b.np, rows_per_lane, 0, st);
        ms += t1.stop();
        HIPCHK(hipGetLastError());
        tlen.resize(b.np); toff.assign(b.np + 1, 0);
        HIPCHK(hipMemcpy(tlen.data(), d_tlen.p, b.np * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < b.np; k++) {
          if (tlen[k] <= 0) SET_ERR(ctx, ITSX_E_DEVICE, "itsx_align_clusters: the direction bits of read " + std::to_string(pq[b.p0 + k]) + " do not lead back to the first cell");
          toff[k + 1] = toff[k] + tlen[k];
        }
        HIPCHK(d_text.alloc((size_t)toff[b.np] + 1));
        a.text = reinterpret_cast<char *>(d_text.p);
        HIPCHK(hipMemcpyAsync(d_toff.p, toff.data(), (b.np + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        StageTimer t2(st);
        launch_cg_traceback(a, (int32_t)b.p0, (int32_t)b.np, rows_per_lane, 1, st);
        ms += t2.stop();
        HIPCHK(hipGetLastError());
        plane.resize((size_t)toff[b.np]);
        HIPCHK(hipMemcpy(plane.data(), d_text.p, plane.size(), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < b.np; k++) text[(size_t)pm[b.p0 + k]].assign(plane.data() + toff[k], (size_t)tlen[k]);
      }
      // the sweep's last cell is the one the clustering accepted the member with: the same identity, bit for bit
      std::vector<double> pid(NP);
      HIPCHK(hipMemcpy(pid.data(), d_pid.p, NP * sizeof(double), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < NP; k++)
        if (memcmp(&pid[k], &ctx->h_pct[(size_t)pq[k]], sizeof(double)) != 0)
          SET_ERR(ctx, ITSX_E_DEVICE, "itsx_align_clusters: read " + std::to_string(pq[k]) + " aligns at identity " + std::to_string(pid[k]) + ", the clustering accepted it at " + std::to_string(ctx->h_pct[(size_t)pq[k]]));
    }
  }
  ctx->h_cg_off.assign((size_t)n + 1, 0);
  { size_t m = 0, tot = 0; for (int64_t r = 0; r < n; r++) { ctx->h_cg_off[(size_t)r] = (int64_t)tot; if (m < M && hq[m] == r) tot += text[m++].size(); } ctx->h_cg_off[(size_t)n] = (int64_t)tot; ctx->h_cg_text.reserve(tot); }
  for (size_t m = 0; m < M; m++) ctx->h_cg_text += text[m];
  ctx->have_cigar = true;
  if (n_aligned) *n_aligned = (int64_t)M;
  if (ms_kernels) *ms_kernels = ms;
  return ITSX_OK;
}
int itsx_get_cluster_cigars(const itsx_ctx *ctx, int64_t *offs, char *text)
{
  CTXCHK(ctx && offs);
  if (!ctx->cigars_live()) SET_ERR(ctx, ITSX_E_ARG, "itsx_get_cluster_cigars: no alignments for the current clustering (itsx_align_clusters comes after itsx_cluster* at id < 1)");
  memcpy(offs, ctx->h_cg_off.data(), ((size_t)ctx->N + 1) * sizeof(int64_t));
  if (text && !ctx->h_cg_text.empty()) memcpy(text, ctx->h_cg_text.data(), ctx->h_cg_text.size());
  return ITSX_OK;
}

int itsx_get_derep(const itsx_ctx *ctx, int64_t *rep_of, int8_t *strand, int64_t *uniq_of)
{
  CTXCHK(ctx && ctx->grouped());
  for (int64_t r = 0; r < ctx->N; r++) {
    if (rep_of) rep_of[r] = ctx->h_rep_of[r];
    if (strand) strand[r] = ctx->h_strand[r];
    if (uniq_of) uniq_of[r] = ctx->h_uniq_of[r];
  }
  return ITSX_OK;
}
int itsx_get_uniques(const itsx_ctx *ctx, int64_t *seed_read, int64_t *abundance)
{
  CTXCHK(ctx && ctx->grouped());
  for (int32_t u = 0; u < ctx->U; u++) { if (seed_read) seed_read[u] = ctx->h_seed_read[u]; if (abundance) abundance[u] = ctx->h_abund[u]; }
  return ITSX_OK;
}


// ---- multi-GPU exact dereplication (SURVEY 8e option 2): keys out, active set in
int itsx_unique_keys(itsx_ctx *ctx, uint64_t seed, uint64_t *fwd, uint64_t *rc)
{
  CTXCHK(ctx && ctx->grouped() && fwd && rc);
  if (ctx->S > 1) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "cross-rank dereplication of a sample batch is not supported: shard whole samples across ranks");
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->N;
  if (n == 0 || ctx->U == 0) return ITSX_OK;
  HIPCHK(ctx->w_hf.alloc((size_t)n + 1)); HIPCHK(ctx->w_hr.alloc((size_t)n + 1));
  launch_hash_reads(ctx->rd, seed, 1, ctx->w_hf.p, ctx->w_hr.p, ctx->st);
  std::vector<uint64_t> hf((size_t)n), hr((size_t)n);
  HIPCHK(hipMemcpyAsync(hf.data(), ctx->w_hf.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->st));
  HIPCHK(hipMemcpyAsync(hr.data(), ctx->w_hr.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  // trailing A's are zero bits in the packed words: the length is folded in so that a read and its A-extended copy differ
  for (int32_t u = 0; u < ctx->U; u++) {
    const size_t r = (size_t)ctx->h_seed_read[u];
    const uint64_t lm = (uint64_t)ctx->h_len[r] * 0x9E3779B97F4A7C15ULL;
    fwd[u] = hf[r] ^ lm; rc[u] = hr[r] ^ lm;
  }
  return ITSX_OK;
}

// the length-ordered list the HMM stages walk: `keep` (length-ordered already), or every unique again (keep == nullptr)
static int set_walked_uniques(itsx_ctx *ctx, const std::vector<int32_t> *keep)
{
  const std::vector<int32_t> &lst = keep ? *keep : ctx->h_sorted_uniq;
  ctx->U_active = (int32_t)lst.size();
  ctx->h_sorted_active = lst;
  if (!lst.empty()) {
    HIPCHK(hipMemcpyAsync(ctx->d_sorted_uniq.p, lst.data(), lst.size() * 4, hipMemcpyHostToDevice, ctx->st));
    launch_fill_ulen(ctx->U_active, ctx->d_sorted_uniq.p, ctx->d_seed_read.p, ctx->rd.len, ctx->d_ulen.p, ctx->st);
    HIPCHK(hipStreamSynchronize(ctx->st));
  }
  return ITSX_OK;
}

int itsx_set_active_uniques(itsx_ctx *ctx, const uint8_t *active)
{
  CTXCHK(ctx && ctx->grouped() && (active || ctx->U == 0));
  HIPCHK(hipSetDevice(ctx->device));
  StageTxn txn(ctx, itsx_ctx::ST_GROUPED);               // a search of other uniques is not this choice's
  std::vector<int32_t> keep; keep.reserve((size_t)ctx->U);
  for (int32_t s = 0; s < ctx->U; s++) { const int32_t u = ctx->h_sorted_uniq[(size_t)s]; if (active[u]) keep.push_back(u); }   // stays length-sorted
  { const int rc = set_walked_uniques(ctx, &keep); if (rc != ITSX_OK) return rc; }      // the traces and the searched-target count follow the active list
  ctx->active_narrowed = true;           // (sample sharing leaves a caller's choice alone)
  txn.commit(itsx_ctx::ST_GROUPED);
  return ITSX_OK;
}

// ------------------------------------------------------------------------------ search
static float msv_score_from_byte(int xj, int tjb)
{
  float sc = ((float)(xj - tjb) - 190.0f);
  sc /= (float)(3.0 / 0.69314718055994529);
  sc -= 3.0f;
  return sc;
}

static int search_chunk(itsx_ctx *ctx, int ci, int32_t u0, int32_t U, int Lcap, double T, double F1, double F3);
static int append_traces(itsx_ctx *ctx);

// Prefix sharing (k_share.hip) for the search that is about to run: the prefix tree of the active uniques (per length and per chunk of
// ctx->s_Uc uniques), the batches whose saved row states fit the slot budget, the processing order (batch, depth, length) and the tree
// in that order.  ctx->share_on = false when it is switched off (ITSX_SHARE=0), cannot apply, or would share less than ITSX_SHARE_MIN
// (default 0.10) of the rows: the search then runs today's schedule.
static int build_share(itsx_ctx *ctx)
{
  hipStream_t st = ctx->st;
  itsx_stats &S = ctx->stats;
  ctx->share_on = false; ctx->sh_batches.clear(); ctx->sh_segk_h.clear();
  S.share_B = 0; S.share_batches = 0; S.share_nodes = S.share_chains = 0; S.ms_share_build = 0; S.share_frac = 0;
  ctx->two_on = false; ctx->Ub = 0; ctx->share_maxrd = 0; ctx->sh_bsegk_h.clear();
  S.two_sided = 0; S.n_joined = 0; S.bwd_chains = 0; S.gamma_nodes = 0; S.bwd_rows = 0; S.join_maxdiff = 0; S.ms_bwd_bound = 0; S.n_bwd_launches = 0; S.two_fwd_rows = S.two_bwd_rows = S.two_rows_full = 0;
  const int32_t U = ctx->U_active, Uc = (int32_t)std::min<int64_t>(ctx->s_Uc, 0x7fffffff), P = ctx->P;
  if (const char *e = sw_get("ITSX_SHARE")) if (atoi(e) == 0) return ITSX_OK;
  // (the A/B switch of the bound pass uses the classic wave list)
  if (sw_get("ITSX_LAZY_EXACT_BOUND")) return ITSX_OK;
  if (U < 2 || U >= (1 << 26) || P <= 0) return ITSX_OK;
  int B = 32;
  if (const char *e = sw_get("ITSX_SHARE_B")) B = atoi(e);
  int logB = 0; while ((1 << logB) < B) logB++;
  if (B < 16 || B > 1024 || (1 << logB) != B) SET_ERR(ctx, ITSX_E_ARG, "ITSX_SHARE_B must be a power of two between 16 and 1024");
  StageTimer tm(st);
  TrieArgs a{};
  a.rd = ctx->rd; a.sorted_uniq = ctx->d_sorted_uniq.p; a.seed_read = ctx->d_seed_read.p; a.U = U; a.Uc = std::max(1, Uc); a.B = B;
  HIPCHK(ctx->sh_counters.alloc(16));
  HIPCHK(hipMemsetAsync(ctx->sh_counters.p, 0, 16 * sizeof(unsigned long long), st));
  a.counters = ctx->sh_counters.p;
  launch_trie_keycount(a, st);
  if (ctx->lazy && ctx->bound_fold) { TrieArgs r0 = a; r0.rev = 1; launch_trie_keycount(r0, st); }      // (the suffix tree uses the same table after the prefix tree)
  unsigned long long hc0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(hc0, ctx->sh_counters.p, sizeof(hc0), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const unsigned long long nkeys = std::max(hc0[4], hc0[6]);
  if (nkeys == 0) return ITSX_OK;
  uint64_t slots = 1024; while (slots < 2 * nkeys) slots <<= 1;
  HIPCHK(ctx->sh_tab.alloc((size_t)slots, true));
  HIPCHK(hipMemsetAsync(ctx->sh_tab.p, 0xFF, (size_t)slots * sizeof(unsigned long long), st));
  HIPCHK(ctx->sh_depth_s.alloc((size_t)U + 1)); HIPCHK(ctx->sh_parent_s.alloc((size_t)U + 1)); HIPCHK(ctx->sh_mask_s.alloc((size_t)U + 1));
  HIPCHK(ctx->sh_nn_s.alloc((size_t)U + 2)); HIPCHK(ctx->sh_node0_s.alloc((size_t)U + 2)); HIPCHK(ctx->sh_scan.alloc((size_t)scan_tmp_elems((int64_t)U + 2)));
  HIPCHK(hipMemsetAsync(ctx->sh_mask_s.p, 0, ((size_t)U + 1) * sizeof(unsigned long long), st));
  a.tab = ctx->sh_tab.p; a.tmask = slots - 1; a.depth = ctx->sh_depth_s.p; a.parent = ctx->sh_parent_s.p; a.mask = ctx->sh_mask_s.p; a.nn = ctx->sh_nn_s.p;
  launch_trie_insert(a, st); launch_trie_resolve(a, st); launch_trie_link(a, st); launch_trie_count(a, st);
  launch_exclusive_scan(ctx->sh_nn_s.p, ctx->sh_node0_s.p, (int64_t)U + 1, ctx->sh_scan.p, st);
  // ---- two-sided sharing (round 6; lazy searches with the folded bound kernel): the SUFFIX tree in the same table, the joins, the
  // chains' extents (k_share.hip: k_join_*)
  bool two = ctx->lazy && ctx->bound_fold && !(sw_get("ITSX_SHARE_TWO") && atoi(sw_get("ITSX_SHARE_TWO")) == 0);
  TrieArgs ar = a;
  JoinArgs ja{};
  if (two) {
    HIPCHK(ctx->sh_rdepth_s.alloc((size_t)U + 1)); HIPCHK(ctx->sh_rparent_s.alloc((size_t)U + 1)); HIPCHK(ctx->sh_rmask_s.alloc((size_t)U + 1));
    HIPCHK(ctx->sh_jlev_s.alloc((size_t)U + 1)); HIPCHK(ctx->sh_jown_s.alloc((size_t)U + 1)); HIPCHK(ctx->sh_endrow_s.alloc((size_t)U + 1));
    HIPCHK(ctx->sh_rsteps_s.alloc((size_t)U + 1)); HIPCHK(ctx->sh_rnn_s.alloc((size_t)U + 2)); HIPCHK(ctx->sh_rnode0_s.alloc((size_t)U + 2));
    HIPCHK(hipMemsetAsync(ctx->sh_tab.p, 0xFF, (size_t)slots * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(ctx->sh_rmask_s.p, 0, ((size_t)U + 1) * sizeof(unsigned long long), st));
    ar.rev = 1; ar.depth = ctx->sh_rdepth_s.p; ar.parent = ctx->sh_rparent_s.p; ar.mask = ctx->sh_rmask_s.p; ar.nn = ctx->sh_rnn_s.p;
    launch_trie_insert(ar, st); launch_trie_resolve(ar, st); launch_trie_link(ar, st);
    ja.t = ar; ja.fdepth = ctx->sh_depth_s.p; ja.fmask = ctx->sh_mask_s.p; ja.rmask = ctx->sh_rmask_s.p; ja.jlev = ctx->sh_jlev_s.p; ja.jown = ctx->sh_jown_s.p;
    ja.endrow = ctx->sh_endrow_s.p; ja.rsteps = ctx->sh_rsteps_s.p; ja.counters = ctx->sh_counters.p;
    launch_join_resolve(ja, st);
    for (int r = 63; r >= 1; r--) launch_join_up(ja, r, st);
    launch_join_ends(ja, st);
    launch_popc64(ctx->sh_rmask_s.p, ctx->sh_rnn_s.p, (int64_t)U + 1, U, st);
    launch_exclusive_scan(ctx->sh_rnn_s.p, ctx->sh_rnode0_s.p, (int64_t)U + 1, ctx->sh_scan.p, st);
  }
  // where a batch may start: a new length or a new chunk
  const int32_t ncap = 65536 + U / std::max(1, Uc) + 8;
  HIPCHK(ctx->sh_cuts.alloc((size_t)ncap * 3));
  launch_share_cuts(ctx->d_ulen.p, ctx->sh_node0_s.p, two ? ctx->sh_rnode0_s.p : nullptr, U, a.Uc, ncap, ctx->sh_cuts.p, ctx->sh_counters.p + 5, st);
  int32_t NN = 0, NG = 0;
  unsigned long long hc[16];
  HIPCHK(hipMemcpyAsync(hc, ctx->sh_counters.p, sizeof(hc), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&NN, ctx->sh_node0_s.p + U, sizeof(NN), hipMemcpyDeviceToHost, st));
  if (two) HIPCHK(hipMemcpyAsync(&NG, ctx->sh_rnode0_s.p + U, sizeof(NG), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int maxd = (int)hc[0];
  const double frac = hc[2] ? (double)hc[1] / (double)hc[2] : 0.0;
  S.share_frac = (float)frac;
  double min_frac = 0.10;
  if (const char *e = sw_get("ITSX_SHARE_MIN")) min_frac = atof(e);
  const int64_t ncuts = (int64_t)hc[5];
  if (frac < min_frac || maxd <= 0 || NN <= 0 || ncuts > ncap) { S.ms_share_build = tm.stop(); return ITSX_OK; }
  if (two && (hc[10] == 0 || NG <= 0)) two = false;            // nobody joins: the one-sided schedule
  const int maxrd = two ? (int)hc[13] : 0;
  std::vector<int32_t> cuts((size_t)ncuts * 3);
  HIPCHK(hipMemcpyAsync(cuts.data(), ctx->sh_cuts.p, cuts.size() * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  struct Cut { int32_t s, n, g; };
  std::vector<Cut> cv((size_t)ncuts);
  for (int64_t i = 0; i < ncuts; i++) cv[(size_t)i] = {cuts[(size_t)3 * i], cuts[(size_t)3 * i + 1], two ? cuts[(size_t)3 * i + 2] : 0};
  std::sort(cv.begin(), cv.end(), [](const Cut &x, const Cut &y) { return x.s < y.s; });
  cv.push_back({U, NN, two ? NG : 0});
  // ---- batches: consecutive groups of one chunk while their saved states (for every profile, at the Forward pass's size) fit the budget
  // (a lazy search: the Forward pass's states, up to 48 GB (in the DP slab's memory: below) and a third of what is free; otherwise only the MSV filter shares, its
  // states are a fifth the size, and the full table's rows and slabs want the memory: up to 8 GB and an eighth of what is free)
  const bool fwd_too = ctx->lazy;
  double gb = fwd_too ? (two ? 76.0 : 48.0) : 8.0;
  {
    size_t fr = 0, tot = 0;
    const double held = (double)ctx->w_slab.cap * sizeof(float) + (double)ctx->sh_mslots.cap * sizeof(uint4);
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) gb = std::min(gb, std::max(0.25, ((double)fr + held) / (double)(1ull << 30) / (fwd_too ? 3.0 : 8.0)));
  }
  if (const char *e = sw_get("ITSX_SHARE_GB")) gb = std::max(0.0001, atof(e));
  // Two batches of the MSV filter always run side by side, each on its own half of its (small) buffer.  The Forward pass does so only
  // with ITSX_SHARE_FWD_STREAMS=2: measured, its launches' tails are too short for that to gain anything (2.029 vs 2.024 s per 10 M
  // reads), and overlapping launches make a kernel trace's durations (each stretched by the other) disagree with the wall time
  // ... except in a SMALL search (under 2 M representatives: a GPU's share of a sharded job), where a (batch, depth) launch is a few
  // milliseconds and its tail a tenth of that: 1.25 M reads 244 -> 232 ms, the step 496 -> 476 (ITSX_SHARE_FWD_STREAMS=1 / 2 force one way)
  // (not under an explicit slot budget: two batches side by side need twice the slots)
  const bool two_fwd = sw_get("ITSX_SHARE_FWD_STREAMS") ? atoi(sw_get("ITSX_SHARE_FWD_STREAMS")) >= 2 : (U < 2000000 && !sw_get("ITSX_SHARE_GB"));
  const double state_b = fwd_too ? (two_fwd ? 2.0 : 1.0) * (double)FWD_STATE_Q * sizeof(float4) : 2.0 * (double)MSV_STATE_Q * sizeof(uint4);
  // ... and no more than a job of this size needs: a quarter of all its states at a time still gives every (batch, depth) launch
  // thousands of waves, and device memory is not free to get (20-40 ms per GB in a fresh context: a streamed file's chunks each bring
  // their own -- round 5's first streamed run spent 5 s in hipMalloc for slots its 1.3 M-read chunks filled to a tenth)
  // (a quarter and a twentieth: the groups a batch is made of do not fill four exact quarters, and a fifth batch with the 2 % that are left
  // over is thirty launches of a few thousand waves -- 39 ms of pass A and 20 ms of the filter at 10 M reads for 15 ms' worth of rows)
  // (ITSX_SHARE_DIV: the divisor, for A/B -- 2.8 gives three batches where 3.8 gives four; the cap above holds either way.  A divisor
  // that is asked for is obeyed in a small search too, which otherwise gets 1 GB and one batch)
  double share_div = 3.8, share_floor = 1.0;
  if (const char *e = sw_get("ITSX_SHARE_DIV")) { share_div = std::min(16.0, std::max(1.0, atof(e))); share_floor = 0.0001; }
  if (!sw_get("ITSX_SHARE_GB")) gb = std::min(gb, std::max(share_floor, (double)((int64_t)NN + NG) * state_b * (double)P / (double)(1ull << 30) / share_div));
  // (in steps of half a GB: a budget that follows the free memory byte by byte made every search of a warm context ask for a slab a few
  // KB larger than the one it held -- 20 GB freed and allocated again per search)
  if (gb > 1.0) gb = floor(gb * 2.0) / 2.0;
  const int64_t nodes_max = std::max<int64_t>(1, (int64_t)(gb * (double)(1ull << 30) / (state_b * (double)P)));
  std::vector<int32_t> bstart; std::vector<itsx_ctx::ShareBatch> &bt = ctx->sh_batches;
  {
    size_t i = 0;
    while (i + 1 < cv.size()) {
      size_t j = i + 1;                       // the batch takes groups i .. j - 1
      while (j + 1 < cv.size() && cv[j].s % a.Uc != 0 && ((int64_t)cv[j + 1].n - cv[i].n) + ((int64_t)cv[j + 1].g - cv[i].g) <= nodes_max) j++;
      itsx_ctx::ShareBatch b{};
      b.k0 = cv[i].s; b.k1 = cv[j].s; b.node0 = cv[i].n; b.nnodes = (int64_t)cv[j].n - cv[i].n; b.gnode0 = cv[i].g; b.gnnodes = (int64_t)cv[j].g - cv[i].g;
      b.nsplit = (int32_t)std::min<int64_t>(P, (b.nnodes + b.gnnodes + nodes_max - 1) / nodes_max); if (b.nsplit < 1) b.nsplit = 1;
      bstart.push_back(b.k0); bt.push_back(b);
      i = j;
    }
    bstart.push_back(U);
  }
  const int nb = (int)bt.size();
  if (nb >= (1 << 24)) { bt.clear(); S.ms_share_build = tm.stop(); return ITSX_OK; }
  // a batch that one group overfills takes its profiles in nsplit ranges; if even one profile's states do not fit, nothing is shared
  for (auto &b : bt) if ((double)(b.nnodes + b.gnnodes) * state_b * (double)((P + b.nsplit - 1) / b.nsplit) > 1.5 * gb * (double)(1ull << 30)) { bt.clear(); S.ms_share_build = tm.stop(); return ITSX_OK; }
  // ---- the processing order: stable by (batch, depth, last row) (k_order.hip)
  HIPCHK(upload(ctx->sh_bstart, bstart, st)); HIPCHK(ctx->sh_segk.alloc((size_t)nb * SHARE_SEGS));
  HIPCHK(ctx->sh_uorder.alloc((size_t)U + 1)); HIPCHK(ctx->sh_inv.alloc((size_t)U + 1));
  HIPCHK(ctx->sh_keys.alloc((size_t)U + 1)); HIPCHK(ctx->sh_keys2.alloc((size_t)U + 1)); HIPCHK(ctx->sh_vals.alloc((size_t)U + 1));
  const size_t sort_bytes = order_sort_bytes(U);
  HIPCHK(ctx->sh_sorttmp.alloc(sort_bytes));
  launch_order_keys(ctx->sh_depth_s.p, two ? ctx->sh_endrow_s.p : ctx->d_ulen.p, nullptr, U, ctx->sh_bstart.p, nb, ctx->sh_keys.p, ctx->sh_vals.p, st);
  if (order_sort(ctx->sh_sorttmp.p, sort_bytes, ctx->sh_keys.p, ctx->sh_keys2.p, ctx->sh_vals.p, ctx->sh_uorder.p, U, st) != 0) SET_ERR(ctx, ITSX_E_DEVICE, "prefix sharing: the order's radix sort failed");
  HIPCHK(hipMemsetAsync(ctx->sh_counters.p + 15, 0, sizeof(unsigned long long), st));
  launch_order_segk(ctx->sh_keys2.p, U, nb, ctx->sh_segk.p, ctx->sh_inv.p, ctx->sh_uorder.p, U, ctx->sh_counters.p + 15, st);
  ctx->sh_segk_h.assign((size_t)nb * SHARE_SEGS, 0);
  HIPCHK(hipMemcpyAsync(ctx->sh_segk_h.data(), ctx->sh_segk.p, (size_t)nb * SHARE_SEGS * 4, hipMemcpyDeviceToHost, st));
  // ---- the tree by processing position
  HIPCHK(ctx->sh_depth.alloc((size_t)U + 1)); HIPCHK(ctx->sh_parent.alloc((size_t)U + 1)); HIPCHK(ctx->sh_mask.alloc((size_t)U + 1));
  HIPCHK(ctx->sh_nn.alloc((size_t)U + 2)); HIPCHK(ctx->sh_node0.alloc((size_t)U + 2)); HIPCHK(ctx->sh_order.alloc((size_t)U + 1)); HIPCHK(ctx->sh_ulen.alloc((size_t)U + 1));
  HIPCHK(ctx->sh_endrow.alloc((size_t)U + 1)); HIPCHK(ctx->sh_jlev.alloc((size_t)U + 1)); HIPCHK(ctx->sh_jsrc.alloc((size_t)U + 1)); HIPCHK(ctx->sh_jownb.alloc((size_t)U + 1));
  ShareDev &o = ctx->sh_dev;
  HIPCHK(ctx->sh_src.alloc((size_t)U + 1));
  o.src = ctx->sh_src.p;
  o.depth = ctx->sh_depth.p; o.parent = ctx->sh_parent.p; o.mask = ctx->sh_mask.p; o.nn = ctx->sh_nn.p; o.node0 = ctx->sh_node0.p; o.order = ctx->sh_order.p; o.ulen = ctx->sh_ulen.p;
  o.endrow = ctx->sh_endrow.p; o.jlev = ctx->sh_jlev.p; o.jsrc = ctx->sh_jsrc.p;
  launch_share_permute(a, ctx->d_ulen.p, ctx->sh_uorder.p, ctx->sh_inv.p, two ? ctx->sh_endrow_s.p : nullptr, two ? ctx->sh_jlev_s.p : nullptr, o, st);
  launch_exclusive_scan(ctx->sh_nn.p, ctx->sh_node0.p, (int64_t)U + 1, ctx->sh_scan.p, st);
  launch_share_src(o, U, a.Uc, st);
  int32_t Ub = 0;
  if (two) {
    // ---- the Backward chains: the uniques that save a state for somebody, by (batch, blocks from the end they start at, rows they walk)
    HIPCHK(ctx->sh_border_s.alloc((size_t)U + 1)); HIPCHK(ctx->sh_invb.alloc((size_t)U + 1)); HIPCHK(ctx->sh_bsegk.alloc((size_t)nb * SHARE_SEGS));
    launch_order_keys(ctx->sh_rdepth_s.p, ctx->sh_rsteps_s.p, ctx->sh_rsteps_s.p, U, ctx->sh_bstart.p, nb, ctx->sh_keys.p, ctx->sh_vals.p, st);
    if (order_sort(ctx->sh_sorttmp.p, sort_bytes, ctx->sh_keys.p, ctx->sh_keys2.p, ctx->sh_vals.p, ctx->sh_border_s.p, U, st) != 0) SET_ERR(ctx, ITSX_E_DEVICE, "two-sided sharing: the order's radix sort failed");
    HIPCHK(hipMemsetAsync(ctx->sh_counters.p + 15, 0, sizeof(unsigned long long), st));
    launch_order_segk(ctx->sh_keys2.p, U, nb, ctx->sh_bsegk.p, ctx->sh_invb.p, ctx->sh_border_s.p, U, ctx->sh_counters.p + 15, st);
    unsigned long long nv = 0;
    ctx->sh_bsegk_h.assign((size_t)nb * SHARE_SEGS, 0);
    HIPCHK(hipMemcpyAsync(ctx->sh_bsegk_h.data(), ctx->sh_bsegk.p, (size_t)nb * SHARE_SEGS * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&nv, ctx->sh_counters.p + 15, sizeof(nv), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    Ub = (int32_t)nv;
    HIPCHK(ctx->sh_rdepth.alloc((size_t)Ub + 1)); HIPCHK(ctx->sh_rparent.alloc((size_t)Ub + 1)); HIPCHK(ctx->sh_rmask.alloc((size_t)Ub + 1));
    HIPCHK(ctx->sh_rnn.alloc((size_t)Ub + 2)); HIPCHK(ctx->sh_rnode0.alloc((size_t)Ub + 2)); HIPCHK(ctx->sh_border.alloc((size_t)Ub + 1)); HIPCHK(ctx->sh_bulen.alloc((size_t)Ub + 1));
    HIPCHK(ctx->sh_rsrc.alloc((size_t)Ub + 1)); HIPCHK(ctx->sh_bsteps.alloc((size_t)Ub + 1));
    BShareDev &ob = ctx->sh_bdev;
    ob.depth = ctx->sh_rdepth.p; ob.parent = ctx->sh_rparent.p; ob.mask = ctx->sh_rmask.p; ob.nn = ctx->sh_rnn.p; ob.node0 = ctx->sh_rnode0.p; ob.order = ctx->sh_border.p;
    ob.ulen = ctx->sh_bulen.p; ob.src = ctx->sh_rsrc.p; ob.steps = ctx->sh_bsteps.p;
    launch_bshare_permute(ar, Ub, ctx->d_ulen.p, ctx->sh_border_s.p, ctx->sh_invb.p, ctx->sh_rmask_s.p, ctx->sh_rsteps_s.p, ob, st);
    launch_exclusive_scan(ctx->sh_rnn.p, ctx->sh_rnode0.p, (int64_t)Ub + 1, ctx->sh_scan.p, st);
    launch_bshare_src(ob, Ub, st);
    launch_join_src(U, B, ctx->sh_uorder.p, ctx->sh_jown_s.p, ctx->sh_invb.p, ob, o, ctx->sh_jownb.p, st);
    HIPCHK(ctx->sh_chain.alloc((size_t)U + 1)); HIPCHK(ctx->sh_bchain.alloc((size_t)Ub + 1));
    launch_chain_recs(U, ctx->rd, o.order, ctx->d_seed_read.p, o.src, o.node0, o.mask, o.endrow, o.jlev, o.jsrc, ctx->sh_chain.p, st);
    launch_chain_recs(Ub, ctx->rd, ob.order, ctx->d_seed_read.p, ob.src, ob.node0, ob.mask, ob.steps, nullptr, nullptr, ctx->sh_bchain.p, st);
  }
  HIPCHK(hipStreamSynchronize(st));
  // ---- slots of the saved states: the largest batch's, for the MSV filter and for the Forward pass
  int64_t need_slots = 0, need_gslots = 0;
  for (auto &b : bt) {
    const int64_t pr = (int64_t)((P + b.nsplit - 1) / b.nsplit);
    need_slots = std::max<int64_t>(need_slots, b.nnodes * pr); need_gslots = std::max<int64_t>(need_gslots, b.gnnodes * pr);
  }
  // (no room for them: the search runs unshared)
  ctx->sh_mslots_half = (size_t)need_slots * MSV_STATE_Q;      // two batches of the MSV filter run side by side (search_chunk)
  // The Forward pass's states live in the DP slab (ctx->w_slab): pass A is over before the rounds' Forward / Backward kernels write their
  // rows there, so the two never need the memory at the same time -- 24-48 GB that round 5's first version held twice (and that cost the
  // stages behind it their batch sizes).  Two-sided: a batch's Backward states follow its Forward states.
  const size_t half = ((size_t)need_slots + (size_t)(two ? need_gslots : 0)) * FWD_STATE_Q;
  ctx->sh_gslots_off = (size_t)need_slots * FWD_STATE_Q;
  ctx->sh_fslots_half = (fwd_too && two_fwd && nb > 1) ? half : 0;       // (one batch: nothing to run beside it)
  ctx->sh_mgslots_half = (size_t)need_gslots * MSV_STATE_Q;
  if (ctx->sh_mslots.alloc(2 * (size_t)need_slots * MSV_STATE_Q + 1) != hipSuccess || (two && ctx->sh_mgslots.alloc(2 * (size_t)need_gslots * MSV_STATE_Q + 1) != hipSuccess) ||
      (fwd_too && ctx->w_slab.alloc(((4 * (half * (ctx->sh_fslots_half ? 2 : 1) + 1) + ((size_t)64 << 20) - 1) >> 26) << 26, true) != hipSuccess)) {
    (void)hipGetLastError();
    ctx->sh_mslots.release(); bt.clear();
    S.ms_share_build = tm.stop();
    return ITSX_OK;
  }
  ctx->share_on = true; ctx->share_B = B; ctx->share_logB = logB; ctx->share_maxd = maxd;
  ctx->two_on = two; ctx->Ub = Ub; ctx->share_maxrd = maxrd;
  S.share_B = B; S.share_batches = nb; S.share_nodes = NN; S.share_chains = (int64_t)hc[3];
  S.msv_rows_full = (int64_t)hc[2] * P; S.msv_rows = (int64_t)(hc[2] - hc[1]) * P;
  if (two && !(sw_get("ITSX_MSV_TWO") && atoi(sw_get("ITSX_MSV_TWO")) == 0)) S.msv_rows = (int64_t)(hc[11] + hc[12]) * P;
  if (two) { S.two_sided = 1; S.n_joined = (int64_t)hc[10]; S.bwd_chains = (int64_t)hc[14]; S.gamma_nodes = NG; S.two_fwd_rows = (int64_t)hc[11]; S.two_bwd_rows = (int64_t)hc[12]; S.two_rows_full = (int64_t)hc[2]; }
  S.ms_share_build = tm.stop();
  return ITSX_OK;
}

// the active uniques, chunk by chunk (s_Uc uniques at a time), through search_chunk
static int run_chunks(itsx_ctx *ctx, double T, double F1, double F3)
{
  const int64_t U = ctx->U_active, Uc = std::max<int64_t>(1, ctx->s_Uc);
  int ci = 0;
  if (ctx->st2) HIPCHK(hipStreamSynchronize(ctx->st2));      // a search that failed half-way may have left an MSV launch behind
  ctx->msv_pre_u0 = -1;
  msv_diag_begin();
  // diagnostic (ITSX_TEST_HOOKS=1 ITSX_PASSA_DBG=64): how often a floored row of the shared MSV kernel takes the "xB rose" branch
  const bool count_xb = sw_get("ITSX_PASSA_DBG") && (atoi(sw_get("ITSX_PASSA_DBG")) & 64);      // (a hook: nullptr unless ITSX_TEST_HOOKS=1)
  if (count_xb) { HIPCHK(ctx->msv_xb.alloc(8)); HIPCHK(hipMemsetAsync(ctx->msv_xb.p, 0, 8 * sizeof(unsigned long long), ctx->st)); HIPCHK(hipStreamSynchronize(ctx->st)); }
  else ctx->msv_xb.release();
  for (int64_t u0 = 0; u0 < U; u0 += Uc, ci++) {
    ctx->next_u0 = (u0 + Uc < U) ? u0 + Uc : -1;
    ctx->next_U = (int32_t)std::min<int64_t>(Uc, U - (u0 + Uc));
    const int rc = search_chunk(ctx, ci, (int32_t)u0, (int32_t)std::min<int64_t>(Uc, U - u0), ctx->s_Lcap, T, F1, F3);
    if (rc != ITSX_OK) return rc;
  }
  if (count_xb) {
    unsigned long long n[5] = {0, 0, 0, 0, 0};
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(n, ctx->msv_xb.p, sizeof(n), hipMemcpyDeviceToHost));
    fprintf(stderr, "[itsx] msv floored wave-rows %llu, with the xB branch %llu (%.4f)\n", n[0], n[1], n[0] ? (double)n[1] / (double)n[0] : 0.0);
    // (a wave counts once per launch: once per range when a batch takes its profiles in ranges)
    int nsplit = 0;
    for (const auto &b : ctx->sh_batches) nsplit = std::max(nsplit, (int)b.nsplit);
    fprintf(stderr, "[itsx] msv shared waves: whole read %llu, window %llu, 16 words at a time %llu; profile ranges of a batch: at most %d\n", n[2], n[3], n[4], nsplit);
  }
  ctx->n_chunks = ci;
  return ITSX_OK;
}

// What a compact / lazy search assumes and keeps per (representative, class): the assumptions (ITSX_COMPACT_ZMAX, ITSX_COMPACT_DOME_MIN),
// the profiles' classes and the cleared best-certain-row table.  Called by itsx_search and by itsx_debug_set_domains.
static int compact_setup(itsx_ctx *ctx)
{
  hipStream_t st = ctx->st;
  const int P = ctx->P;
  ctx->compact_zmax = 1e9; ctx->compact_dome_min = 1e-2;          // hmmsearch's --domE is 10 unless given; 1e9 reported targets per profile is a lot of data
  if (const char *e = sw_get("ITSX_COMPACT_ZMAX")) ctx->compact_zmax = std::max(1.0, atof(e));
  if (const char *e = sw_get("ITSX_COMPACT_DOME_MIN")) ctx->compact_dome_min = std::max(1e-300, atof(e));
  ctx->compact_lnp = log(ctx->compact_dome_min / ctx->compact_zmax) - 1e-6;       // certain: exp(lnP) * Zmax <= domE_min, with room for exp's last bit
  // classes = the distinct 2-character NAME prefixes (what create_runtime_hmm and ItsPosition select by: 1_ 2_ 3_ 4_)
  std::vector<int8_t> cls((size_t)P, 0); std::vector<std::string> seen;
  for (int p = 0; p < P; p++) {
    const std::string pre = ctx->profs[p].name.substr(0, 2);
    size_t k = 0; while (k < seen.size() && seen[k] != pre) k++;
    if (k == seen.size()) seen.push_back(pre);
    if (k > 126) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "ITSX_COMPACT_ROWS: more than 127 distinct 2-character profile name prefixes");
    cls[p] = (int8_t)k;
  }
  ctx->compact_ncls = (int)seen.size();
  HIPCHK(upload(ctx->w_cls, cls, st));
  HIPCHK(ctx->w_bestc.alloc((size_t)ctx->U * ctx->compact_ncls + 1));
  HIPCHK(hipMemsetAsync(ctx->w_bestc.p, 0, ((size_t)ctx->U * ctx->compact_ncls + 1) * sizeof(unsigned long long), st));
  return ITSX_OK;
}

// The compaction of one segment of domain rows (a search's chunk, or a segment handed to itsx_debug_set_domains): of the NR rows at d_rows
// keep what can still win once domZ is known (k_compact_*), in row order, in dom_bufs[di]; the best certain rows accumulate in w_bestc
static int compact_segment(itsx_ctx *ctx, const itsx_domain *d_rows, int64_t NR, size_t di)
{
  hipStream_t st = ctx->st;
  launch_compact_best(d_rows, NR, ctx->w_cls.p, ctx->compact_ncls, ctx->compact_lnp, ctx->w_bestc.p, st);
  HIPCHK(ctx->w_keep.alloc((size_t)NR + 1)); HIPCHK(ctx->w_keeppos.alloc((size_t)NR + 1)); HIPCHK(ctx->w_keeptmp.alloc((size_t)scan_tmp_elems(NR + 1)));
  launch_compact_mark(d_rows, NR, ctx->w_cls.p, ctx->compact_ncls, ctx->compact_lnp, ctx->w_bestc.p, ctx->w_keep.p, st);
  launch_exclusive_scan(ctx->w_keep.p, ctx->w_keeppos.p, NR + 1, ctx->w_keeptmp.p, st);
  int32_t kept = 0;
  HIPCHK(hipMemcpyAsync(&kept, ctx->w_keeppos.p + NR, sizeof(kept), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  DBuf<itsx_domain> &small = *ctx->dom_bufs[di];
  HIPCHK(small.alloc((size_t)std::max<int32_t>(kept, 1), true));
  launch_compact_scatter(d_rows, NR, ctx->w_keep.p, ctx->w_keeppos.p, small.p, st);
  ctx->rows_before_compaction += NR;
  ctx->dom_n[di] = kept;
  return ITSX_OK;
}

// rows mode of the search that is about to run: what the caller selected (itsx_set_rows_mode), else the environment
// (ITSX_ROWS=full|compact|lazy; ITSX_COMPACT_ROWS=1)
static int search_rows_mode(const itsx_ctx *ctx)
{
  int mode = ctx->rows_mode;
  if (mode < 0) {
    mode = ITSX_ROWS_FULL;
    if (sw_get("ITSX_COMPACT_ROWS") && atoi(sw_get("ITSX_COMPACT_ROWS")) != 0) mode = ITSX_ROWS_COMPACT;
    if (const char *e = sw_get("ITSX_ROWS")) mode = !strcmp(e, "lazy") ? ITSX_ROWS_LAZY : !strcmp(e, "compact") ? ITSX_ROWS_COMPACT : ITSX_ROWS_FULL;
  }
  if (mode == ITSX_ROWS_LAZY && sw_get("ITSX_KEEP_TRACE")) mode = ITSX_ROWS_COMPACT;      // pair traces describe the full pipeline
  return mode;
}

// What the MSV filter needs of the host before it runs over the context's active uniques (search_active, orient_profiles): the
// per-length constants (d_lt), the null-length table (w_tjb) and the pass thresholds at F1 (w_thr: a row per length that occurs),
// uploaded and waited for.  *cells_active: the residues of the active representatives.
static int filter_tables(itsx_ctx *ctx, double F1, int64_t *cells_active_out)
{
  hipStream_t st = ctx->st;
  const int P = ctx->P, Ppad = ctx->G * 64;
  // ---- per-length constants (host libm, as hmmsearch computes them per target)
  const int Lcap = ctx->Lmax + 1;
  std::vector<LenTables> lt((size_t)Lcap);
  std::vector<int32_t> tjb((size_t)Lcap, 0);
  std::vector<char> present((size_t)Lcap, 0);
  int64_t cells_active = 0;                                 // residues of the active representatives (the filter's cell count)
  {   // two gathers per representative from arrays the size of the read set: a few threads (10 M reads: 25 ms on one, the GPU idle)
    const int32_t Ua = ctx->U, Uact = ctx->U_active;
    const int Th = Ua >= (1 << 19) ? std::max(1, std::min(8, itsx_io::io_threads())) : 1;
    std::vector<std::vector<char>> pres((size_t)Th); std::vector<int64_t> csum((size_t)Th, 0);
    on_threads(Th, [&](int t) {
      std::vector<char> &pr = pres[(size_t)t]; pr.assign((size_t)Lcap, 0);
      int64_t c = 0;
      for (int64_t u = (int64_t)Ua * t / Th, hi = (int64_t)Ua * (t + 1) / Th; u < hi; u++) {
        const int32_t L = ctx->h_len[ctx->h_seed_read[(size_t)u]];
        pr[(size_t)L] = 1;
        if (Uact == Ua) c += L;
      }
      csum[(size_t)t] = c;
    });
    for (int t = 0; t < Th; t++) { cells_active += csum[(size_t)t]; for (int L = 0; L < Lcap; L++) present[(size_t)L] |= pres[(size_t)t][(size_t)L]; }
    if (Uact != Ua) for (int32_t u : ctx->h_sorted_active) cells_active += ctx->h_len[ctx->h_seed_read[(size_t)u]];      // a narrowed list: its own residues
  }
  for (int L = 0; L < Lcap; L++) {
    LenTables &t = lt[L]; memset(&t, 0, sizeof(t));
    if (L == 0) continue;
    const float p1 = (float)L / (float)(L + 1);
    t.p1 = p1;
    t.nullsc = (float)((double)(float)L * log((double)p1) + log(1. - (double)p1));
    t.bias_a = (float)L * logf(p1);
    t.bias_b = logf((float)(1. - (double)p1));
    t.lognn3 = log((double)((float)L / (float)(L + 3)));
    t.tjb = host_tjb_b(L);
    tjb[L] = t.tjb;
    {   // lazy domain stage (k_lazy.hip): bits <= (fwdsc - nullsc) / ln 2 + C(L); + 0.02 bits for float rounding, rounded up to float
      const double n = (double)L;
      const double c = 1.0 + (2.0 * log(2.0 * (n + 3.0) / (3.0 * (n + 2.0))) + n * log((n + 3.0) / (n + 2.0))) / 0.69314718055994529;
      // the margin covers the rounding of both float sums (the bound kernel's and HMMER's own: sums of positive products, relative
      // error <= ~3 (n + M) 2^-24 each): 0.02 bits up to ~38 000 residues, growing with n beyond (0.034 bits at 65 535)
      const double margin = std::max(0.02, 6.0 * (n + (double)MMAX) * 5.9604644775390625e-8 / 0.69314718055994529);
      t.lazy_c = nextafterf((float)(c + margin), 1e30f);
    }
    { const float w = roundf((float)(500.0 / 0.69314718055994529) * logf((2.0f + 1.0f) / ((float)L + 2.0f + 1.0f)));
      t.vmove = (w >= 32767.0f) ? 32767 : (w <= -32768.0f) ? -32768 : (int)w; }
  }
  // MSV pass threshold on the final xJ byte, per (length, profile): P(score) <= F1
  // (a row depends on the length, the profiles and F1 only: rows made by an earlier search of this context are kept -- 200 k
  // evaluations of the Gumbel tail, 13 ms per search of the bench's 280 lengths x 88 profiles, while the GPU waited)
  if (ctx->thr_memo_F1 != F1 || ctx->thr_memo_Ppad != Ppad) { ctx->thr_memo.clear(); ctx->thr_memo_have.clear(); ctx->thr_memo_F1 = F1; ctx->thr_memo_Ppad = Ppad; }
  if (ctx->thr_memo_have.size() < (size_t)Lcap) { ctx->thr_memo_have.resize((size_t)Lcap, 0); ctx->thr_memo.resize((size_t)Lcap * Ppad, 257); }
  std::vector<uint16_t> thr((size_t)Lcap * Ppad, 257);
  for (int L = 1; L < Lcap; L++) {
    if (!present[L]) continue;
    if (ctx->thr_memo_have[(size_t)L]) { memcpy(&thr[(size_t)L * Ppad], &ctx->thr_memo[(size_t)L * Ppad], (size_t)Ppad * sizeof(uint16_t)); continue; }
    ctx->thr_memo_have[(size_t)L] = 2;                 // (filled below)
    for (int p = 0; p < P; p++) {
      const HostProfile &h = ctx->profs[p];
      auto passes = [&](int xj) {
        const float usc = msv_score_from_byte(xj, lt[L].tjb);
        const double Pv = gumbel_surv((double)(usc - lt[L].nullsc) / 0.69314718055994529, (double)h.evparam[0], (double)h.evparam[1]);
        return !(Pv > F1);
      };
      int lo = 0, hi = 255;             // smallest xj in [0,254] that passes; 256 if none
      if (!passes(254)) { thr[(size_t)L * Ppad + p] = 256; continue; }
      while (lo < hi) { const int mid = (lo + hi) / 2; if (passes(mid)) hi = mid; else lo = mid + 1; }
      thr[(size_t)L * Ppad + p] = (uint16_t)lo;
    }
  }
  for (int L = 1; L < Lcap; L++)
    if (ctx->thr_memo_have[(size_t)L] == 2) { memcpy(&ctx->thr_memo[(size_t)L * Ppad], &thr[(size_t)L * Ppad], (size_t)Ppad * sizeof(uint16_t)); ctx->thr_memo_have[(size_t)L] = 1; }
  DBuf<uint16_t> &d_thr = ctx->w_thr; DBuf<int32_t> &d_tjb = ctx->w_tjb;
  HIPCHK(upload(ctx->d_lt, lt, st)); HIPCHK(upload(d_thr, thr, st)); HIPCHK(upload(d_tjb, tjb, st));

  HIPCHK(hipStreamSynchronize(st));
  if (cells_active_out) *cells_active_out = cells_active;
  return ITSX_OK;
}

// the search over the context's active uniques (itsx_search below: all of them, the caller's choice, or the holders of the score classes)
static int search_active(itsx_ctx *ctx, double T, double F1, double F2, double F3)
{
  CTXCHK(ctx);
  if (!ctx->grouped()) SET_ERR(ctx, ITSX_E_ARG, "itsx_search called before itsx_derep / itsx_cluster");
  if (ctx->P <= 0) SET_ERR(ctx, ITSX_E_ARG, "no profiles loaded");
  ctx->F2 = F2; ctx->have_vit = F2 < F1;              // hmmsearch enters the Viterbi filter only for P > F2: never when F1 <= F2
  ctx->switches_at_search = sw_report();              // what the environment asked of this search (itsx_switches)
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const int P = ctx->P, G = ctx->G, Ppad = G * 64, U = ctx->U_active;
  ctx->T = T;
  ctx->domz.assign((size_t)P * ctx->S, 0);
  itsx_stats &S = ctx->stats;
  S.n_pairs = (int64_t)U * P; S.n_past_msv = S.n_past_bias = S.n_past_fwd = S.n_regions = S.n_multidomain = S.n_domains = S.n_domain_overflow = 0;
  S.ms_msv = S.ms_filters = S.ms_domains = S.ms_msv_kernel = S.ms_fwd_kernel = S.ms_bwd_kernel = S.ms_env_kernel = S.ms_bias_kernel = S.ms_decode_kernel = 0; S.n_batches = 0; S.ms_ensemble = 0; S.n_mr_clustered = S.n_mr_distinct = S.n_mr_failed = S.n_mr_envelopes = 0; S.n_slab_shrinks = 0; S.n_mr_overflow = 0; S.ms_vit_kernel = 0; for (int k = 0; k < 8; k++) S.n_mr_fail_kind[k] = 0; S.n_rows_resident = 0; S.msv_cells = 0; S.msv_launches = 0; S.fwd_rows = 0; S.env_rows = 0; S.n_env_unique = 0;
  ctx->npairs_padded = 0; ctx->dom_n.clear(); ctx->trace_u0 = 0; ctx->n_chunks = 0;
  const int mode = search_rows_mode(ctx);
  ctx->compact_rows = mode != ITSX_ROWS_FULL;
  ctx->lazy = mode == ITSX_ROWS_LAZY;
  ctx->sF1 = F1; ctx->sF3 = F3;
  ctx->domz_ub.assign((size_t)P * ctx->S, 0);
  if (ctx->compact_rows)                    // a full table of an earlier search (80 B x ~130 per representative) goes back to the device
    for (auto &b : ctx->dom_bufs) if (b && b->cap * sizeof(itsx_domain) > ((size_t)256 << 20)) b->release();
  S.lazy = ctx->lazy; S.n_lazy_evaluated = S.n_lazy_round1 = S.n_lazy_pending = S.n_lazy_reruns = 0; S.n_lazy_completed = S.n_lazy_completed_profiles = S.n_lazy_pending_profiles = 0; S.ms_lazy_complete = 0; S.lazy_bound_maxdiff = 0; S.ms_bound_kernel = S.ms_lazy_select = 0; S.bound_rows = 0; S.n_bound_launches = 0; S.n_lazy_topup = 0; S.ms_lazy_topup = 0; S.ms_lazy_topup_stages = 0; ctx->n_topup_deferred = ctx->n_topup_ensemble = 0;
  if (ctx->compact_rows && U > 0) { const int rc = compact_setup(ctx); if (rc != ITSX_OK) return rc; }
  if (U == 0) return ITSX_OK;

  const int Lcap = ctx->Lmax + 1;
  int64_t cells_active = 0;                                 // residues of the active representatives (the filter's cell count, below)
  { const int rc = filter_tables(ctx, F1, &cells_active); if (rc != ITSX_OK) return rc; }
  HIPCHK(ctx->d_domz32.alloc((size_t)P * ctx->S));
  HIPCHK(hipMemsetAsync(ctx->d_domz32.p, 0, (size_t)P * ctx->S * 4, st));
  {
    const int64_t cells = cells_active;
    int64_t msum = 0; for (auto &h : ctx->profs) msum += h.M;
    S.msv_cells = cells * msum;
    S.msv_rows = S.msv_rows_full = cells * P; S.bound_rows_full = 0; S.n_share_helpers = 0; S.share_mismatch = 0;
  }
  // ---- the unique reads are searched in chunks so that every work list of a chunk fits a fixed share of HBM
  // (about 400 B per potential (unique, profile) pair); one chunk covers the 1 M-read bench
  if (ctx->pair_budget <= 0) {
    size_t fr = 0, tot = 0;
    double gb = 32.0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) gb = std::max(1.0, (double)fr / (double)(1ull << 30) / 4.0);
    ctx->pair_budget = (int64_t)(gb * (double)(1ull << 30) / 400.0);
  }
  // (the lazy stage keeps ~40 B per pair -- the record, its Forward score, its bound, the selection scan -- and the 400 B only for
  // the pairs it evaluates: chunks can be several times larger)
  int64_t lazy_budget = ctx->pair_budget * 5;
  if (ctx->lazy) {
    // ... but never more than the device can hold NOW: a context that ran the full pipeline before keeps its slabs and work lists
    // (buffers only grow).  ~64 B per pair, a third of what is free plus what the lazy lists hold already.
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
      const double held = (double)ctx->d_pairs.cap * sizeof(PairRec) + (double)ctx->l_fb.cap * 4 + (double)ctx->l_b10.cap * 4 + (double)ctx->l_smask.cap * 8 +
                          (double)ctx->l_scnt.cap * 4 + (double)ctx->l_spos.cap * 4 + (double)ctx->l_done.cap + (double)ctx->w_res.cap * 2;
      lazy_budget = std::min<int64_t>(lazy_budget, (int64_t)(((double)fr + held) / 3.0 / 64.0));
      lazy_budget = std::max<int64_t>(lazy_budget, (int64_t)1 << 20);
    }
  }
  int64_t Uc = std::max<int64_t>(1, (ctx->lazy ? lazy_budget : ctx->pair_budget) / std::max(P, 1));
  Uc = std::min<int64_t>(Uc, ((1ll << 31) - 4096) / std::max(Ppad, 1));
  // (a context that has searched a job of this size already holds the buffers for it -- they only grow --: what is FREE now says nothing
  // about whether the chunk fits, and a second, tiny chunk costs a round of every launch and the top-up round its list)
  if (ctx->lazy && ctx->prev_lazy && ctx->prev_P == P && (int64_t)U <= ctx->prev_U && ctx->prev_Uc > Uc) Uc = ctx->prev_Uc;
  if (const char *e = sw_get("ITSX_CHUNK_UNIQUES")) Uc = std::max<int64_t>(1, atoll(e));
  ctx->keep_trace = sw_get("ITSX_KEEP_TRACE") != nullptr;
  ctx->s_Uc = Uc; ctx->s_Lcap = Lcap;
  ctx->prev_lazy = ctx->lazy; ctx->prev_P = P; ctx->prev_U = U; ctx->prev_Uc = Uc;
  ctx->domz_ub_loc.assign((size_t)P * ctx->S, 0);
  { const int rc = build_share(ctx); if (rc != ITSX_OK) return rc; }
  { const int rc = run_chunks(ctx, T, F1, F3); if (rc != ITSX_OK) return rc; }
  std::vector<int32_t> dz32((size_t)P * ctx->S, 0);
  HIPCHK(hipMemcpyAsync(dz32.data(), ctx->d_domz32.p, dz32.size() * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  ctx->domz_loc.assign(dz32.begin(), dz32.end());
  ctx->domz = ctx->domz_loc; ctx->domz_ub = ctx->domz_ub_loc;
  S.n_rows_resident = 0;
  for (int64_t r : ctx->dom_n) S.n_rows_resident += r;
  // Nothing is capped: a pair's regions beyond its slots go to an overflow list, an ensemble beyond the fast kernel's bookkeeping to the
  // overflow path (k_ensemble.hip).  What remains is what makes hmmsearch itself throw: a region whose Forward matrix cannot be sampled
  // (p7_StochasticTrace's "probabilities were not normalised"): reported, not papered over.
  if (S.n_mr_failed > 0)
    SET_ERR(ctx, ITSX_E_UNSUPPORTED, std::to_string(S.n_mr_failed) + " multidomain region(s) with a Forward matrix that cannot be sampled (hmmsearch's stochastic traceback throws on them)");
  return ITSX_OK;
}

// ---- sample sharing (itsx_set_sample_sharing): one holder per score class goes through the HMM stages
static bool sample_sharing_wanted(const itsx_ctx *ctx)
{
  if (ctx->share_samples) return true;
  const char *e = sw_get("ITSX_SHARE_SAMPLES");
  return e && atoi(e) == 1;
}
static bool sample_sharing_lazy_wanted(const itsx_ctx *ctx)
{
  if (ctx->share_samples_lazy) return true;
  const char *e = sw_get("ITSX_SHARE_SAMPLES_LAZY");
  return e && atoi(e) == 1;
}
// the score classes of the current dereplication (k_derep.hip: k_class_*), on the device; holders [C] on the host
static int build_sample_classes(itsx_ctx *ctx, std::vector<int32_t> &holders)
{
  hipStream_t st = ctx->st;
  const int32_t U = ctx->U;
  StageTimer tm(st);
  uint64_t tsize = 1024; while (tsize < (uint64_t)U * 2 + 16) tsize <<= 1;
  DBuf<unsigned long long> &keys = ctx->w_keys; DBuf<int32_t> &vals = ctx->w_vals; DBuf<uint32_t> &slot_of = ctx->w_slot_of; DBuf<unsigned int> &ncoll = ctx->w_ncoll;
  HIPCHK(keys.alloc(tsize)); HIPCHK(vals.alloc(tsize)); HIPCHK(slot_of.alloc((size_t)U + 1)); HIPCHK(ncoll.alloc(1));
  HIPCHK(ctx->sc_holder_of.alloc((size_t)U + 1)); HIPCHK(ctx->sc_is_holder.alloc((size_t)U + 2)); HIPCHK(ctx->sc_rank.alloc((size_t)U + 2));
  HIPCHK(ctx->sc_scan.alloc((size_t)scan_tmp_elems((int64_t)U + 1)));
  HIPCHK(ctx->sc_class_of.alloc((size_t)U + 1)); HIPCHK(ctx->sc_members.alloc((size_t)U + 1)); HIPCHK(ctx->sc_members_in.alloc((size_t)U + 1));
  HIPCHK(ctx->sc_keys.alloc((size_t)U + 1)); HIPCHK(ctx->sc_keys_in.alloc((size_t)U + 1));
  unsigned int hcoll = 0;
  uint64_t seed = 0x5343ull;
  for (int attempt = 0; attempt < 4; attempt++) {
    HIPCHK(hipMemsetAsync(keys.p, 0, tsize * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(vals.p, 0x7f, tsize * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(ncoll.p, 0, sizeof(unsigned int), st));
    launch_class_insert(ctx->rd, ctx->d_seed_read.p, U, seed, keys.p, vals.p, tsize - 1, slot_of.p, st);
    launch_class_resolve(ctx->rd, ctx->d_seed_read.p, U, vals.p, slot_of.p, ctx->sc_holder_of.p, ctx->sc_is_holder.p, ncoll.p, st);
    HIPCHK(hipMemcpyAsync(&hcoll, ncoll.p, sizeof(hcoll), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (hcoll == 0) break;
    seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
  }
  if (hcoll != 0) SET_ERR(ctx, ITSX_E_COLLISION, "score classes: 64-bit key collisions survived 4 reseeds");
  int32_t C = 0;
  launch_exclusive_scan(ctx->sc_is_holder.p, ctx->sc_rank.p, (int64_t)U + 1, ctx->sc_scan.p, st);      // element U = the number of classes
  HIPCHK(hipMemcpyAsync(&C, ctx->sc_rank.p + U, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (C <= 0 || C > U) SET_ERR(ctx, ITSX_E_DEVICE, "score classes: bookkeeping mismatch (" + std::to_string(C) + " classes of " + std::to_string(U) + " uniques)");
  HIPCHK(ctx->sc_holder.alloc((size_t)C + 1)); HIPCHK(ctx->sc_off.alloc((size_t)C + 2));
  launch_class_number(U, ctx->sc_holder_of.p, ctx->sc_rank.p, ctx->sc_class_of.p, ctx->sc_holder.p, ctx->sc_keys_in.p, ctx->sc_members_in.p, st);
  const size_t sort_bytes = order_sort_bytes(U);
  HIPCHK(ctx->sc_sort.alloc(sort_bytes));
  if (order_sort(ctx->sc_sort.p, sort_bytes, ctx->sc_keys_in.p, ctx->sc_keys.p, ctx->sc_members_in.p, ctx->sc_members.p, U, st) != 0)
    SET_ERR(ctx, ITSX_E_DEVICE, "score classes: the member sort failed");
  launch_class_offsets(ctx->sc_keys.p, U, C, ctx->sc_off.p, st);
  holders.resize((size_t)C);
  HIPCHK(hipMemcpyAsync(holders.data(), ctx->sc_holder.p, (size_t)C * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  ctx->sc.n_classes = C; ctx->sc.n_shared = (int64_t)U - C;
  ctx->sc.ms_classes = tm.stop();
  return ITSX_OK;
}
// every non-holder member gets its holder's rows (k_expand_*), one more segment per segment of the search, and its reported targets
// are counted into its own sample's domZ; then the host's counters follow the device's.
// count == false (a lazy / compact sharing search: the segments hold the KEPT rows, and the members were counted chunk by chunk from
// the scratch rows, count_member_targets): the rows of the segments from seg0 on are copied, nothing is counted, and the figures add
// to those of the search (itsx_lazy_complete comes here for the segments it added).
static int expand_shared_rows(itsx_ctx *ctx, size_t seg0 = 0, bool count = true)
{
  hipStream_t st = ctx->st;
  StageTimer tm(st);
  const size_t nseg = ctx->dom_n.size();
  int64_t expanded = 0;
  for (size_t c = seg0; c < nseg; c++) {
    const int64_t NR = ctx->dom_n[c];
    if (NR <= 0) continue;
    HIPCHK(ctx->sc_cnt.alloc((size_t)NR + 1)); HIPCHK(ctx->sc_pos.alloc((size_t)NR + 1)); HIPCHK(ctx->sc_scan.alloc((size_t)scan_tmp_elems(NR + 1)));
    DBuf<int64_t> &d_c = ctx->w_counters;
    HIPCHK(d_c.alloc(8));
    HIPCHK(hipMemsetAsync(d_c.p, 0, sizeof(int64_t), st));
    launch_expand_count(ctx->dom_bufs[c]->p, NR, ctx->sc_class_of.p, ctx->sc_off.p, ctx->sc_cnt.p, (unsigned long long *)d_c.p, st);
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_c.p, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total <= 0) continue;
    if (total >= 2147483000ll)                // (the 32-bit scan below; rows of 80 bytes: such a table would not be resident either)
      SET_ERR(ctx, ITSX_E_UNSUPPORTED, "sample sharing: " + std::to_string(total) + " rows to copy from one chunk of the search, more than 2^31 (lower ITSX_CHUNK_UNIQUES or search without sharing)");
    launch_exclusive_scan(ctx->sc_cnt.p, ctx->sc_pos.p, NR + 1, ctx->sc_scan.p, st);
    const size_t di = ctx->dom_n.size();
    ctx->dom_n.push_back(0);
    while (ctx->dom_bufs.size() <= di) ctx->dom_bufs.emplace_back(new DBuf<itsx_domain>());
    HIPCHK(ctx->dom_bufs[di]->alloc((size_t)total));
    launch_expand_rows(ctx->dom_bufs[c]->p, NR, ctx->sc_pos.p, total, ctx->sc_class_of.p, ctx->sc_off.p, ctx->sc_members.p, ctx->dev_usample(), ctx->P,
                       ctx->dom_bufs[di]->p, count ? ctx->d_domz32.p : nullptr, st);
    ctx->dom_n[di] = total;
    expanded += total;
  }
  if (count) {
    std::vector<int32_t> dz32((size_t)ctx->P * ctx->S, 0);
    HIPCHK(hipMemcpyAsync(dz32.data(), ctx->d_domz32.p, dz32.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    ctx->domz_loc.assign(dz32.begin(), dz32.end());
    ctx->domz = ctx->domz_loc;
    ctx->sc.n_expanded = 0; ctx->sc.ms_expand = 0;
  } else {
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
  }
  ctx->sc_segs_done = ctx->dom_n.size();
  ctx->stats.n_rows_resident += expanded;
  ctx->sc.n_expanded += expanded;
  ctx->sc.ms_expand += tm.stop();
  return ITSX_OK;
}
// A lazy / compact sharing search, after k_score and before the compaction of the chunk's NR scratch rows at d_rows: every row that
// k_score counted for its holder's sample (dom_idx == 0, seq_reported) adds one to the counter of every other member's sample
// (k_derep.hip: k_member_*).  Exact: the members of a class lie in different samples, and a member's own search would have scored the
// same residues.
static int count_member_targets(itsx_ctx *ctx, const itsx_domain *d_rows, int64_t NR)
{
  if (NR <= 0) return ITSX_OK;
  hipStream_t st = ctx->st;
  StageTimer tm(st);
  HIPCHK(ctx->sc_cnt.alloc((size_t)NR + 1)); HIPCHK(ctx->sc_pos.alloc((size_t)NR + 1)); HIPCHK(ctx->sc_scan.alloc((size_t)scan_tmp_elems(NR + 1)));
  DBuf<int64_t> &d_c = ctx->w_counters;
  HIPCHK(d_c.alloc(8));
  HIPCHK(hipMemsetAsync(d_c.p, 0, sizeof(int64_t), st));
  launch_member_count(d_rows, NR, ctx->sc_class_of.p, ctx->sc_off.p, ctx->sc_cnt.p, (unsigned long long *)d_c.p, st);
  int64_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, d_c.p, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (total >= 2147483000ll)                  // (the 32-bit scan below)
    SET_ERR(ctx, ITSX_E_UNSUPPORTED, "sample sharing: " + std::to_string(total) + " member counts from one chunk of the search, more than 2^31 (lower ITSX_CHUNK_UNIQUES or search without sharing)");
  if (total > 0) {
    launch_exclusive_scan(ctx->sc_cnt.p, ctx->sc_pos.p, NR + 1, ctx->sc_scan.p, st);
    launch_member_add(d_rows, NR, ctx->sc_pos.p, total, ctx->sc_class_of.p, ctx->sc_off.p, ctx->sc_members.p, ctx->dev_usample(), ctx->P, ctx->d_domz32.p, st);
  }
  ctx->sc.ms_expand += tm.stop();
  return ITSX_OK;
}

// the search in the mode that applies: of all active uniques, or of the holders of the score classes and the rows' expansion to the members
static int search_in_mode(itsx_ctx *ctx, double T, double F1, double F2, double F3)
{
  ctx->sc_count_members = false; ctx->sc_segs_done = 0;
  // The mode applies to a search of S > 1 samples whose active set is the engine's own.  Each rows mode has its setting: the full mode
  // itsx_set_sample_sharing (the rows are copied and counted from afterwards), the lazy and compact modes -- they keep their domZ
  // bounds and their verdicts per (sample, profile), and their segments hold only the rows that can still win --
  // itsx_set_sample_sharing_lazy.  That is bookkeeping, not an obstacle: rounds 1 and 2 of lazy_rounds do not depend on the sample
  // (the bound comes from pass A's score, round 2's threshold is the group's best certain row, reported for every domZ <= 1e9); the
  // lower counter gets one count per member of an evaluated, reported pair's class (count_member_targets); the upper counter adds the
  // holders past the filter to every sample (search_chunk); the top-up round runs at S == 1 only; and a kept row depends on the sample
  // through `rep` alone until k_finalize_lazy.
  const bool full = search_rows_mode(ctx) == ITSX_ROWS_FULL;
  if (!(full ? sample_sharing_wanted(ctx) : sample_sharing_lazy_wanted(ctx)) || !ctx->grouped() || ctx->P <= 0 || ctx->S <= 1 || ctx->U <= 0 || ctx->active_narrowed)
    return search_active(ctx, T, F1, F2, F3);
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<int32_t> holders, keep;
  { const int rc = build_sample_classes(ctx, holders); if (rc != ITSX_OK) return rc; }
  const int32_t U = ctx->U, C = (int32_t)holders.size();
  if (C == U) return search_active(ctx, T, F1, F2, F3);              // nothing in common: every unique is its own holder
  {
    std::vector<char> is_holder((size_t)U, 0);
    for (int32_t h : holders) is_holder[(size_t)h] = 1;
    keep.reserve((size_t)C);
    for (int32_t s = 0; s < U; s++) { const int32_t u = ctx->h_sorted_uniq[(size_t)s]; if (is_holder[(size_t)u]) keep.push_back(u); }      // stays length-sorted
  }
  { const int rc = set_walked_uniques(ctx, &keep); if (rc != ITSX_OK) return rc; }
  ctx->h_sorted_searched.swap(keep); ctx->searched_holders = true;      // (kept past the restore below: the pair traces are fetched later)
  ctx->sc_count_members = !full;
  int rc = search_active(ctx, T, F1, F2, F3);
  ctx->sc_count_members = false;
  { const int rc2 = set_walked_uniques(ctx, nullptr); if (rc == ITSX_OK) rc = rc2; }      // (every exit leaves the context walking all its uniques again)
  if (rc == ITSX_OK) rc = expand_shared_rows(ctx, 0, full);
  if (rc == ITSX_OK) ctx->shared_lazy = !full;
  return rc;
}

int itsx_search(itsx_ctx *ctx, double T, double F1, double F2, double F3)
{
  CTXCHK(ctx);
  StageTxn txn(ctx, itsx_ctx::ST_GROUPED);               // the last search's rows, traces, counters' exchange, sharing figures and top-up list go
  const int rc = search_in_mode(ctx, T, F1, F2, F3);
  if (rc == ITSX_OK) txn.commit(itsx_ctx::ST_SEARCHED);
  return rc;
}

int itsx_set_sample_sharing(itsx_ctx *ctx, int on)
{
  CTXCHK(ctx);
  ctx->share_samples = on != 0;
  return ITSX_OK;
}
int itsx_set_sample_sharing_lazy(itsx_ctx *ctx, int on)
{
  CTXCHK(ctx);
  ctx->share_samples_lazy = on != 0;
  return ITSX_OK;
}
int itsx_sample_sharing_info(const itsx_ctx *ctx, int64_t *n_classes, int64_t *n_uniques_shared, int64_t *n_rows_expanded)
{
  CTXCHK(ctx && ctx->searched());
  if (n_classes) *n_classes = ctx->sc.n_classes;
  if (n_uniques_shared) *n_uniques_shared = ctx->sc.n_shared;
  if (n_rows_expanded) *n_rows_expanded = ctx->sc.n_expanded;
  return ITSX_OK;
}
int itsx_sample_sharing_times(const itsx_ctx *ctx, float *ms_classes, float *ms_expand)
{
  CTXCHK(ctx && ctx->searched());
  if (ms_classes) *ms_classes = ctx->sc.ms_classes;
  if (ms_expand) *ms_expand = ctx->sc.ms_expand;
  return ITSX_OK;
}
int itsx_debug_sample_classes(itsx_ctx *ctx, int32_t *class_of, int64_t n)
{
  CTXCHK(ctx && ctx->searched() && (class_of || n == 0));
  if (ctx->sc.n_classes <= 0) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_sample_classes: the last search built no score classes (itsx_sample_sharing_info reports 0)");
  if (n != (int64_t)ctx->U) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_sample_classes: n is not the number of uniques");
  HIPCHK(hipSetDevice(ctx->device));
  if (n) { HIPCHK(hipMemcpyAsync(class_of, ctx->sc_class_of.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->st)); HIPCHK(hipStreamSynchronize(ctx->st)); }
  return ITSX_OK;
}

// a work list of (representative, profile) pairs grouped by profile: 64-aligned segments, ascending length inside a segment
struct PairList {
  PairRec *pairs = nullptr; PairOut *pout = nullptr;
  int64_t NP = 0;
  std::vector<int64_t> seg_start;        // [P + 1]
  std::vector<int32_t> total;            // [P] pairs of each profile
  const int64_t *d_seg_start = nullptr;  // seg_start on the device
};

// wave descriptors of a pair list (fast Q == 12 waves first, then the runtime-Q ones) and each wave's longest target + 1
static int build_waves(itsx_ctx *ctx, const PairList &pl, std::vector<WaveDesc> &waves, std::vector<char> &wgeneric, std::vector<int32_t> &rows)
{
  hipStream_t st = ctx->st;
  const int P = ctx->P;
  waves.clear(); wgeneric.clear();
  for (int pass = 0; pass < 2; pass++)           // fast (Q == 12) waves first, then runtime-Q waves
    for (int p = 0; p < P; p++) {
      if ((int)ctx->generic_q[p] != pass) continue;
      for (int64_t k = 0; k < pl.total[(size_t)p]; k += 64) {
        WaveDesc w{}; w.prof = p; w.first = pl.seg_start[(size_t)p] + k; w.count = (int32_t)std::min<int64_t>(64, pl.total[(size_t)p] - k);
        waves.push_back(w); wgeneric.push_back((char)pass);
      }
    }
  const int NW = (int)waves.size();
  DBuf<WaveDesc> &d_waves = ctx->w_waves; DBuf<int32_t> &d_rows = ctx->w_rows;
  HIPCHK(upload(d_waves, waves, st)); HIPCHK(d_rows.alloc((size_t)std::max(NW, 1)));
  rows.assign((size_t)NW, 0);
  if (NW == 0) return ITSX_OK;
  hipLaunchKernelGGL(k_wave_rows_pairs, dim3((NW + 255) / 256), dim3(256), 0, st, d_waves.p, NW, pl.pairs, d_rows.p);
  HIPCHK(hipMemcpyAsync(rows.data(), d_rows.p, (size_t)NW * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return ITSX_OK;
}

// every stage after the survivor list, for the pairs of `pl`: bias filter + Forward, Backward + decoding + regions, the ensemble
// stage, envelope re-scoring, scores and domZ counts, domain rows (compacted when the context keeps only what can still win).
// count_only (the top-up round alone; pl is then select_compact's list with its source indices in l_src, l_dmask is zeroed and l_defn[0]
// counts): the call is there for the domZ counters, not for rows.  A pair with a multidomain region is deferred (k_topup_defer: no
// envelopes, no score, no count, unevaluated again) and the ensemble stage does not run; every other pair is scored and counted as
// always, and no row is written, compacted or merged -- a pair that is unevaluated after round 2 ranks below its group's best certain
// row (k_lazy_mark), so no row of it can win or tie ItsPosition's argmax.
static int domain_pipeline(itsx_ctx *ctx, const PairList &pl, const int32_t *d_sorted, double T, double F1, double F3, const std::function<int()> *next_msv, bool count_only = false)
{
  hipStream_t st = ctx->st;
  const int P = ctx->P;
  itsx_stats &S = ctx->stats;
  const int64_t NP = pl.NP;
  const size_t di = ctx->dom_n.size();           // this call's segment of domain rows
  ctx->dom_n.push_back(0);
  while (ctx->dom_bufs.size() <= di) ctx->dom_bufs.emplace_back(new DBuf<itsx_domain>());
  DBuf<itsx_domain> &d_dom = ctx->compact_rows ? ctx->w_domscratch : *ctx->dom_bufs[di];
  if (NP == 0) return ITSX_OK;
  StageTimer tm_list(st);
  std::vector<WaveDesc> waves; std::vector<char> wgeneric; std::vector<int32_t> rows;
  { const int rc = build_waves(ctx, pl, waves, wgeneric, rows); if (rc != ITSX_OK) return rc; }
  const int NW = (int)waves.size();
  DBuf<WaveDesc> &d_waves = ctx->w_waves;
  S.ms_msv += tm_list.stop();

  // ---- batches of waves sized to the slab budget
  if (ctx->slab_gb <= 0.0) {            // the default is decided once per context: a quarter of the free HBM, at most 64 GB
    ctx->slab_gb = 16.0;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) ctx->slab_gb = std::min(64.0, std::max(1.0, (double)fr / (double)(1ull << 30) / 4.0));
  }
  double slab_gb = ctx->slab_gb;
  if (const char *e = sw_get("ITSX_SLAB_GB")) slab_gb = std::max(0.25, atof(e));     // read at every call
  {   // never more than a quarter of what the device has left right now (plus what the context's slab already holds): the stages
      // after the DP kernels need room too.  A budget above that is cut here; one the allocator still refuses is halved below.
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
      const double room = ((double)fr / 4.0 + (double)ctx->w_slab.cap * 4.0) / (double)(1ull << 30);
      if (slab_gb > room) { slab_gb = std::max(0.0625, room); S.n_slab_shrinks++; }
    }
  }
  const int64_t row_bytes = 12 * 64 * 4;                   // XF fields of k_float.hip's parser slab
  int64_t budget_rows = (int64_t)(slab_gb * (1 << 30)) / row_bytes;
  // A job that fits a few batches does not need the whole budget: eight batches already keep the launch tails small, and
  // device memory is not free to get (20-40 ms per GB in a fresh process: a 64-GB slab costs more than the search of a
  // 100 k-read sample).  Memory the context holds already is used in full.
  static const bool adapt = !(sw_get("ITSX_SLAB_ADAPT") && atoi(sw_get("ITSX_SLAB_ADAPT")) == 0);
  if (adapt && !sw_get("ITSX_SLAB_GB")) {
    int64_t total_rows = 0;
    for (int w = 0; w < NW; w++) total_rows += rows[(size_t)w];
    const int64_t floor_rows = ((int64_t)4 << 30) / row_bytes, have_rows = (int64_t)(ctx->w_slab.cap / (12 * 64));
    // (memory the context holds is kept as it is while it is at least half of that: growing a buffer is a free and an allocation, and
    // on this driver both are paid at ~30 GB/s -- freed memory is wiped, fresh memory cleared: scripts/alloc_probe.hip)
    const int64_t want_rows = std::max(total_rows / 8 + 1, floor_rows);
    budget_rows = std::min(budget_rows, 2 * have_rows >= want_rows ? have_rows : want_rows);
  }
  DBuf<RegionRec> &d_raw = ctx->w_raw;
  HIPCHK(d_raw.alloc((size_t)NP * MAXDOM));
  // regions past a pair's MAXDOM slots: hmmsearch keeps them all (a concatemer, a CCS read with tandem copies), so they go to an
  // overflow list that k_decode appends to; should even that list run full it is enlarged and the pipeline call repeated (pool_retry)
  if (ctx->pool_cap <= 0) ctx->pool_cap = 1 << 16;
  RegionPoolView pv{nullptr, nullptr, 0};
 pool_retry:
  HIPCHK(ctx->w_pool.alloc((size_t)ctx->pool_cap)); HIPCHK(ctx->w_pool_k.alloc((size_t)ctx->pool_cap)); HIPCHK(ctx->w_pool_n.alloc(2));
  HIPCHK(hipMemsetAsync(ctx->w_pool_n.p, 0, 2 * sizeof(unsigned long long), st));
  const itsx_stats stats_before = S;
  {
    StageTimer tm(st);
    // ---- batches of waves that fit the slab
    struct Batch { int w0, w1; int64_t r; };
    std::vector<Batch> batches;
    DBuf<float> &d_slab = ctx->w_slab;
    for (;;) {
      batches.clear();
      int64_t rmax = 0;
      for (int w0 = 0; w0 < NW;) {
        int w1 = w0; int64_t r = 0;
        while (w1 < NW && wgeneric[w1] == wgeneric[w0] && (w1 == w0 || r + rows[w1] <= budget_rows)) { waves[w1].slab = r; waves[w1].rows = rows[w1]; r += rows[w1]; w1++; }
        batches.push_back(Batch{w0, w1, r});
        rmax = std::max(rmax, r);
        w0 = w1;
      }
      // several batches: take the whole budget, so that the next job (whose fullest batch may be a few waves larger) fits too
      const int64_t slab_rows = batches.size() > 1 ? std::max(rmax, budget_rows) : rmax;
      if ((size_t)slab_rows * 12 * 64 <= d_slab.cap) break;
      if (d_slab.alloc((size_t)slab_rows * 12 * 64, true) == hipSuccess) break;
      // the budget asked for more memory than the device has left (ITSX_SLAB_GB above the free HBM, another tenant):
      // halve it and batch again -- more, smaller launches -- rather than fail the search
      (void)hipGetLastError();
      if (budget_rows <= ((int64_t)64 << 20) / row_bytes) SET_ERR(ctx, ITSX_E_NOMEM, "not even 64 MB of device memory are left for the DP slab");
      budget_rows = std::max<int64_t>(budget_rows / 2, ((int64_t)64 << 20) / row_bytes);
      ctx->slab_gb = std::min(ctx->slab_gb, (double)(budget_rows * row_bytes) / (double)(1 << 30));
      S.n_slab_shrinks++;
    }
    HIPCHK(hipMemcpyAsync(d_waves.p, waves.data(), (size_t)NW * sizeof(WaveDesc), hipMemcpyHostToDevice, st));
    FloatArgs a{};
    a.rd = ctx->rd; a.sorted_uniq = d_sorted; a.seed_read = ctx->d_seed_read.p; a.prof = ctx->d_prof.p; a.lt = ctx->d_lt.p;
    a.flogsum = ctx->d_flogsum.p; a.logtab = ctx->d_logtab.p; a.pairs = pl.pairs; a.pout = pl.pout; a.waves = d_waves.p; a.slab = d_slab.p;
    a.regions = d_raw.p; a.F1 = F1; a.F3 = F3;
    a.pool.rec = ctx->w_pool.p; a.pool.k = ctx->w_pool_k.p; a.pool.n = ctx->w_pool_n.p; a.pool.cap = ctx->pool_cap;
    VitArgs va{};
    if (ctx->have_vit) {
      HIPCHK(ctx->d_vit.alloc((size_t)NP));
      va.rd = ctx->rd; va.sorted_uniq = d_sorted; va.seed_read = ctx->d_seed_read.p; va.prof = ctx->d_prof.p; va.lt = ctx->d_lt.p;
      va.pairs = pl.pairs; va.pout = pl.pout; va.waves = d_waves.p; va.vtab = ctx->d_vtab.p; va.vit = ctx->d_vit.p; va.F2 = ctx->F2;
      va.eloop = (int32_t)roundf((float)(500.0 / 0.69314718055994529) * logf(0.5f));
      a.vit = ctx->d_vit.p;
    }
    // The bias-composition filter of a batch (its own full-occupancy kernel, VALU-bound, ~48 registers) runs on a second
    // stream beside the decoder of the batch before it (latency-bound, ~50 registers): the two share the SIMDs, which
    // the 256-register DP kernels never do with anything.
    static const bool overlap = !(sw_get("ITSX_BIAS_OVERLAP") && atoi(sw_get("ITSX_BIAS_OVERLAP")) == 0);
    if (overlap && !ctx->st2) {
      int least = 0, greatest = 0;
      (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
      if (sw_get("ITSX_ST2_PRIO") && atoi(sw_get("ITSX_ST2_PRIO")) == 0) least = 0;
      HIPCHK(hipStreamCreateWithPriority(&ctx->st2, hipStreamNonBlocking, least));     // what runs there fills gaps, it does not take turns
      HIPCHK(hipEventCreateWithFlags(&ctx->ev_a, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&ctx->ev_b, hipEventDisableTiming));
    }
    LazyTimers lazy(st), lazy2(overlap ? ctx->st2 : st);
    auto bias_batch = [&](const Batch &bt, hipStream_t s, LazyTimers &lz) {
      // contiguous runs of pairs (the waves of one pass skip the profiles of the other pass)
      int w = bt.w0;
      while (w < bt.w1) {
        int e = w + 1;
        while (e < bt.w1 && waves[(size_t)e].first == waves[(size_t)e - 1].first + 64) e++;
        FloatArgs ab = a;
        ab.pairs = pl.pairs + waves[(size_t)w].first; ab.pout = pl.pout + waves[(size_t)w].first;
        const size_t t = lz.begin(&S.ms_bias_kernel); launch_bias(ab, (int64_t)(e - w) * 64, s); lz.end(t);
        w = e;
      }
    };
    if (!batches.empty()) bias_batch(batches[0], st, lazy);
    for (size_t bi = 0; bi < batches.size(); bi++) {
      const Batch &bt = batches[bi];
      const int w0 = bt.w0, w1 = bt.w1;
      a.slab_plane = bt.r * 6 * 64;
      const bool more = bi + 1 < batches.size();
      if (ctx->have_vit) { const size_t t = lazy.begin(&S.ms_vit_kernel); launch_vit(va, w1 - w0, w0, st); lazy.end(t); }
      { const size_t t = lazy.begin(&S.ms_fwd_kernel); launch_filters_fwd(a, w1 - w0, w0, wgeneric[w0], st); lazy.end(t); }
      { const size_t t = lazy.begin(&S.ms_bwd_kernel); launch_bwd_decode(a, w1 - w0, w0, wgeneric[w0], st); lazy.end(t); }
      if (more && overlap) {
        HIPCHK(hipEventRecord(ctx->ev_a, st)); HIPCHK(hipStreamWaitEvent(ctx->st2, ctx->ev_a, 0));
        bias_batch(batches[bi + 1], ctx->st2, lazy2);
        HIPCHK(hipEventRecord(ctx->ev_b, ctx->st2));
      }
      { const size_t t = lazy.begin(&S.ms_decode_kernel); launch_decode(a, w1 - w0, w0, st); lazy.end(t); }
      if (more && overlap) HIPCHK(hipStreamWaitEvent(st, ctx->ev_b, 0));
      else if (more) bias_batch(batches[bi + 1], st, lazy);
      for (int w = w0; w < w1; w++) S.fwd_rows += (int64_t)(rows[w] - 1) * waves[w].count;
      S.n_batches++;
    }
    lazy2.collect();
    lazy.collect();
    S.ms_filters += tm.stop();
  }
  {   // the overflow list: ordered by (pair, region number) so that the kernels below find region k >= MAXDOM of a pair by bisection
    unsigned long long pn = 0;
    HIPCHK(hipMemcpyAsync(&pn, ctx->w_pool_n.p, sizeof(pn), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if ((int64_t)pn > ctx->pool_cap) {               // (never seen; a sample made of concatemers would do it)
      while (ctx->pool_cap < (int64_t)pn) ctx->pool_cap *= 2;
      const float keep_ms = S.ms_filters;
      S = stats_before; S.ms_filters = keep_ms; S.n_slab_shrinks++;
      goto pool_retry;
    }
    if (pn > 0) {
      std::vector<RegionRec> hr((size_t)pn); std::vector<int32_t> hk((size_t)pn);
      HIPCHK(hipMemcpyAsync(hr.data(), ctx->w_pool.p, (size_t)pn * sizeof(RegionRec), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hk.data(), ctx->w_pool_k.p, (size_t)pn * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      std::vector<size_t> ord((size_t)pn);
      std::iota(ord.begin(), ord.end(), (size_t)0);
      auto key = [&](size_t i) { return ((unsigned long long)(uint32_t)hr[i].pair << 24) | (unsigned long long)(uint32_t)hk[i]; };
      std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return key(x) < key(y); });
      std::vector<RegionRec> sr((size_t)pn); std::vector<unsigned long long> sk((size_t)pn);
      for (size_t i = 0; i < (size_t)pn; i++) { sr[i] = hr[ord[i]]; sk[i] = key(ord[i]); }
      HIPCHK(upload(ctx->w_pool_sorted, sr, st)); HIPCHK(upload(ctx->w_pool_key, sk, st));
      HIPCHK(hipStreamSynchronize(st));
      pv.rec = ctx->w_pool_sorted.p; pv.key = ctx->w_pool_key.p; pv.n = (int64_t)pn;
    }
  }
  // ---- the next chunk's MSV filter, on the second stream: the kernels of the domain stage below wait on memory most of the
  // time (tracebacks, envelope slabs, hashing), the MSV kernel is pure VALU work at 75 registers -- the two share the SIMDs
  if (next_msv) { const int rc = (*next_msv)(); if (rc != ITSX_OK) return rc; }
  StageTimer tm_dom(st);
  // ---- multidomain regions: resolved into envelopes by stochastic traceback clustering (k_ensemble.hip)
  int64_t NMR = 0;
  const bool ensemble = !(sw_get("ITSX_NO_ENSEMBLE") && atoi(sw_get("ITSX_NO_ENSEMBLE")) != 0);
  if (ensemble && count_only) {
    HIPCHK(ctx->w_mrcnt.alloc((size_t)NP + 2));
    launch_mr_count(pl.pout, d_raw.p, pv, NP, ctx->w_mrcnt.p, st);
    launch_topup_defer(pl.pout, ctx->w_mrcnt.p, ctx->l_src.p, NP, ctx->l_done.p, ctx->l_dmask.p, ctx->l_defn.p, st);
  } else if (ensemble) {
    DBuf<int32_t> &mrcnt = ctx->w_mrcnt, &mroff = ctx->w_mroff, &stmp = ctx->w_scan2;
    HIPCHK(mrcnt.alloc((size_t)NP + 2)); HIPCHK(mroff.alloc((size_t)NP + 2)); HIPCHK(stmp.alloc((size_t)scan_tmp_elems(NP + 2)));
    launch_mr_count(pl.pout, d_raw.p, pv, NP, mrcnt.p, st);
    launch_exclusive_scan(mrcnt.p, mroff.p, NP + 1, stmp.p, st);
    int32_t tot = 0;
    HIPCHK(hipMemcpyAsync(&tot, mroff.p + NP, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    NMR = tot;
    if (NMR > 0) {
      StageTimer tm_e(st);
      static_assert(sizeof(MrRec) == sizeof(RegionRec), "MrRec is handed to the region memoisation kernels as a RegionRec");
      HIPCHK(ctx->w_mr.alloc((size_t)NMR));
      launch_mr_fill(pl.pout, d_raw.p, pv, NP, mroff.p, ctx->w_mr.p, st);
      // ---- memoisation: distinct (profile, target length, residues) regions
      DBuf<unsigned long long> &rkeys = ctx->w_keys; DBuf<int32_t> &rvals = ctx->w_vals; DBuf<uint32_t> &rslot = ctx->w_slot_of;
      DBuf<int32_t> &rrep = ctx->w_rrep, &ruq = ctx->w_ruq, &rurank = ctx->w_rurank, &rscan = ctx->w_scan_tmp;
      const uint64_t tsize = region_table_size(NMR);
      HIPCHK(rkeys.alloc(tsize)); HIPCHK(rvals.alloc(tsize)); HIPCHK(rslot.alloc((size_t)NMR + 1));
      HIPCHK(rrep.alloc((size_t)NMR + 1)); HIPCHK(ruq.alloc((size_t)NMR + 1)); HIPCHK(rurank.alloc((size_t)NMR + 1)); HIPCHK(rscan.alloc((size_t)scan_tmp_elems(NMR + 1)));
      HIPCHK(hipMemsetAsync(rkeys.p, 0, tsize * sizeof(unsigned long long), st));
      HIPCHK(hipMemsetAsync(rvals.p, 0x7f, tsize * sizeof(int32_t), st));
      HIPCHK(hipMemsetAsync(ruq.p, 0, ((size_t)NMR + 1) * sizeof(int32_t), st));
      const RegionRec *mr_as_regions = (const RegionRec *)ctx->w_mr.p;
      launch_region_keys(ctx->rd, mr_as_regions, NMR, pl.pairs, d_sorted, ctx->d_seed_read.p, rkeys.p, rvals.p, tsize - 1, rslot.p, st);
      launch_region_resolve(ctx->rd, mr_as_regions, NMR, pl.pairs, d_sorted, ctx->d_seed_read.p, rvals.p, rslot.p, rrep.p, ruq.p, st);
      launch_exclusive_scan(ruq.p, rurank.p, NMR + 1, rscan.p, st);
      int32_t NU = 0;
      HIPCHK(hipMemcpyAsync(&NU, rurank.p + NMR, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      DBuf<int32_t> &ulist0 = ctx->w_mrulist, &ulist = ctx->w_mrulist2, &ulen = ctx->w_mrlen, &newpos = ctx->w_mrloff, &mru = ctx->w_mru;
      HIPCHK(ulist0.alloc((size_t)NU + 1)); HIPCHK(ulist.alloc((size_t)NU + 1)); HIPCHK(ulen.alloc((size_t)NU + 2)); HIPCHK(newpos.alloc((size_t)NU + 2)); HIPCHK(mru.alloc((size_t)NMR + 1));
      launch_mr_ulist(NMR, ctx->w_mr.p, rrep.p, ruq.p, rurank.p, ulist0.p, ulen.p, mru.p, st);
      // the distinct regions are walked in order of length: the lanes of a wave then have paths and residue loops of like length
      std::vector<int32_t> hlen((size_t)NU), ord((size_t)NU), hpos((size_t)NU);
      HIPCHK(hipMemcpyAsync(hlen.data(), ulen.p, (size_t)NU * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      std::iota(ord.begin(), ord.end(), 0);
      std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return hlen[(size_t)x] < hlen[(size_t)y]; });
      std::vector<int64_t> hn2((size_t)NU + 1, 0), hrow((size_t)NU + 1, 0);
      for (int32_t x = 0; x < NU; x++) {
        const int32_t o = ord[(size_t)x];
        hpos[(size_t)o] = x;
        hn2[(size_t)x + 1] = hn2[(size_t)x] + hlen[(size_t)o];
        hrow[(size_t)x + 1] = hrow[(size_t)x] + hlen[(size_t)o] + 1;
      }
      HIPCHK(hipMemcpyAsync(newpos.p, hpos.data(), (size_t)NU * 4, hipMemcpyHostToDevice, st));
      launch_mr_reorder(NU, NMR, newpos.p, ulist0.p, ulist.p, mru.p, st);
      HIPCHK(upload(ctx->w_n2off, hn2, st)); HIPCHK(upload(ctx->w_mrrowoff, hrow, st));
      HIPCHK(ctx->w_mrout.alloc((size_t)NU)); HIPCHK(ctx->w_n2sc.alloc((size_t)hn2[(size_t)NU] + 1));
      // waves over the regions in ascending length.  The longest regions decide when a batch ends (200 sequential paths each, and a
      // wave walks its lanes' paths in phases, so it takes as long as its slowest lane in EVERY phase): they get waves of
      // MR_LANES_LONG lanes, and the kernels take the waves from the back (longest first).
      static const int lanes_long = sw_get("ITSX_MR_LONG_LANES") ? std::max(1, std::min(MR_LANES, atoi(sw_get("ITSX_MR_LONG_LANES")))) : MR_LANES_LONG;
      static const double frac_long = sw_get("ITSX_MR_LONG_FRAC") ? atof(sw_get("ITSX_MR_LONG_FRAC")) : MR_LONG_FRAC;
      const int64_t n_long = std::min<int64_t>(NU, (int64_t)(frac_long * (double)NU));
      // A lazy search sends few regions here (10 M reads: 1 000 - 8 000 distinct ones per round, against 600 000 of a full table): in waves of
      // 64 they are 16 - 120 waves on a chip of 1 024 SIMDs, each walking 200 x ~125 dependent steps for its lanes' 200 x ~60.  The kernel holds
      // four waves per SIMD: as few lanes per wave as keep every wave resident at once (ITSX_MR_WAVES, 4 096; never under two lanes) --
      // less of the phase divergence, the same latency per step (10 M reads: 215 -> 168 ms per step; a full table's waves stay at 64 lanes)
      const int64_t waves_target = sw_get("ITSX_MR_WAVES") ? atoll(sw_get("ITSX_MR_WAVES")) : 4096;       // (read at every search: the tests walk every layout)
      const int lanes_norm = waves_target <= 0 ? MR_LANES : (int)std::max<int64_t>(2, std::min<int64_t>(MR_LANES, (NU + waves_target - 1) / waves_target));
      std::vector<WaveDesc> mw;
      std::vector<int64_t> wfirst;
      for (int64_t x = 0; x < NU;) {
        const int lanes = x >= NU - n_long ? std::min(lanes_long, lanes_norm) : (int)std::min<int64_t>(lanes_norm, NU - n_long - x);
        WaveDesc d{};
        d.prof = -1; d.first = x; d.count = (int32_t)std::min<int64_t>(lanes, (int64_t)NU - x);
        d.rows = hlen[(size_t)ord[(size_t)(d.first + d.count - 1)]] + 1;                  // ascending length: the last lane's
        wfirst.push_back(x);
        mw.push_back(d);
        x += d.count;
      }
      const int NMW = (int)mw.size();
      wfirst.push_back(NU);
      HIPCHK(upload(ctx->w_mrwaves, mw, st));
      const int64_t mrow_bytes = (int64_t)MRV * 16;
      const int64_t mbudget = std::max<int64_t>(1, (int64_t)(std::min(slab_gb, 16.0) * (1 << 30)) / mrow_bytes);
      const int64_t wave_cap = std::max<int64_t>(1, ((int64_t)6 << 30) / ((int64_t)MR_SCRATCH * MR_LANES));      // 6 GB of bookkeeping blocks per batch
      int w0 = 0;
      int64_t mr_wave_cap = wave_cap;
      while (w0 < NMW) {
        int w1 = w0;
        const int64_t row0 = hrow[(size_t)wfirst[(size_t)w0]];
        auto rows_to = [&](int w) { return hrow[(size_t)wfirst[(size_t)std::min(w, NMW)]] - row0; };
        while (w1 < NMW && w1 - w0 < std::min(wave_cap, mr_wave_cap) && (w1 == w0 || rows_to(w1 + 1) <= mbudget)) w1++;
        const int64_t r = rows_to(w1);
        if (((size_t)r * MRV * 4 > ctx->w_mrslab.cap && ctx->w_mrslab.alloc((size_t)r * MRV * 4) != hipSuccess) ||
            ctx->w_mrscratch.alloc((size_t)(wfirst[(size_t)w1] - wfirst[(size_t)w0]) * MR_SCRATCH) != hipSuccess) {
          (void)hipGetLastError();
          if (w1 - w0 <= 1) SET_ERR(ctx, ITSX_E_NOMEM, "no device memory left for the matrices of one wave of multidomain regions");
          mr_wave_cap = std::max<int64_t>(1, (int64_t)(w1 - w0) / 2);     // half as many regions at a time
          S.n_slab_shrinks++;
          continue;
        }
        MrArgs ma{};
        ma.rd = ctx->rd; ma.sorted_uniq = d_sorted; ma.seed_read = ctx->d_seed_read.p; ma.prof = ctx->d_prof.p; ma.pairs = pl.pairs;
        ma.mr = ctx->w_mr.p; ma.ulist = ulist.p; ma.u0 = wfirst[(size_t)w0]; ma.waves = ctx->w_mrwaves.p; ma.slab = (float4 *)ctx->w_mrslab.p;
        ma.rowoff = ctx->w_mrrowoff.p; ma.rowoff0 = row0;
        ma.n2off = ctx->w_n2off.p; ma.n2sc = ctx->w_n2sc.p; ma.out = ctx->w_mrout.p; ma.scratch = ctx->w_mrscratch.p;
        static const bool mrdbg = sw_get("ITSX_MR_DEBUG") != nullptr;
        if (mrdbg) { HIPCHK(ctx->w_counters.alloc(8)); HIPCHK(hipMemsetAsync(ctx->w_counters.p, 0, 64, st)); ma.dbg = (unsigned long long *)ctx->w_counters.p; }
        // a small batch (a shard of a million reads, a chunk of a streaming run) cannot hide a path's chain of dependent matrix reads
        // behind other waves: its regions are walked one per wave with the matrix in LDS (k_ensemble.hip: k_mr_trace<., true>)
        const int64_t one_max = sw_get("ITSX_MR_ONE_MAX") ? atoll(sw_get("ITSX_MR_ONE_MAX")) : 2048;      // (10 M reads: 6 400 and 21 500 regions in the two rounds took 252 and 531 ms this way, 212 in waves of 64)
        const int64_t nreg = wfirst[(size_t)w1] - wfirst[(size_t)w0];
        const bool one = nreg <= one_max;
        if (one) ma.lds_bytes = (int32_t)std::min<int64_t>(40 << 10, (int64_t)mw[(size_t)w1 - 1].rows * MRV * 16);
        launch_mr_ensemble(ma, w1 - w0, w0, st, one ? wfirst[(size_t)w0] : 0, one ? nreg : 0);
        if (mrdbg) {
          unsigned long long d[5];
          HIPCHK(hipMemcpyAsync(d, ctx->w_counters.p, 40, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
          fprintf(stderr, "[itsx] ensemble batch: %d waves, %lld matrix rows; per wave (100 MHz ticks): walk %.0f, close %.0f (samples %.0f), cluster %.0f\n", w1 - w0, (long long)r,
                  (double)d[0] / std::max<double>(1.0, (double)d[3]), (double)d[1] / std::max<double>(1.0, (double)d[3]), (double)d[4] / std::max<double>(1.0, (double)d[3]),
                  (double)d[2] / std::max<double>(1.0, (double)d[3]));
        }
        w0 = w1;
      }
      // ---- the overflow path: regions whose ensemble did not fit the fast kernel's fixed bookkeeping (more than 8 domains in a
      // sampled path, more than 512 distinct tuples, more than 4 envelopes) run again with per-region arrays sized by their length
      {
        HIPCHK(ctx->w_mrsel.alloc((size_t)NU + 1)); HIPCHK(ctx->w_pool_n.alloc(2));
        HIPCHK(hipMemsetAsync(ctx->w_pool_n.p + 1, 0, sizeof(unsigned long long), st));
        launch_mr_overflowed(ctx->w_mrout.p, NU, ctx->w_mrsel.p, ctx->w_pool_n.p + 1, st);
        unsigned long long nov = 0;
        HIPCHK(hipMemcpyAsync(&nov, ctx->w_pool_n.p + 1, sizeof(nov), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (nov > 0) {
          std::vector<int32_t> sel((size_t)nov);
          HIPCHK(hipMemcpyAsync(sel.data(), ctx->w_mrsel.p, (size_t)nov * 4, hipMemcpyDeviceToHost, st));
          HIPCHK(hipStreamSynchronize(st));
          std::sort(sel.begin(), sel.end());              // ascending position = ascending length (the fast pass's order)
          S.n_mr_overflow += (int64_t)nov;
          int64_t envtot = 0;                             // the envelope lists of all of them: 2 x 4 (Lr + 1) ints each, kept until the chunk is scored
          std::vector<int64_t> envoff(sel.size());
          for (size_t x = 0; x < sel.size(); x++) { envoff[x] = envtot; envtot += 8 * ((int64_t)hlen[(size_t)ord[(size_t)sel[x]]] + 1); }
          HIPCHK(ctx->w_mrenv.alloc((size_t)envtot + 8));
          size_t x0 = 0;
          while (x0 < sel.size()) {                       // batches of regions whose blocks fit 8 GB together (one region at least)
            std::vector<MrBig> big; std::vector<int64_t> srow; std::vector<WaveDesc> bw;
            int64_t arena = 0, rows = 0; size_t x1 = x0;
            while (x1 < sel.size()) {
              const int Lr = hlen[(size_t)ord[(size_t)sel[x1]]];
              MrBig g{}; g.capD = Lr + 1; g.capT = 200 * g.capD;
              uint32_t hs = 1024; while (hs < 2u * (uint32_t)g.capT) hs <<= 1;
              g.hmask = hs - 1;
              auto al = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
              const int64_t capSig = 4 * (int64_t)g.capD;
              const int64_t bytes = al(8ll * g.capT) + 6 * al(4ll * g.capT) + al(4ll * hs) + al(4ll * g.capD) + al(16ll * g.capD) + 3 * al(4 * capSig) +
                                    al(g.capT) + al(2ll * g.capD) + al(capSig) + al(2 * MR_EPC) + 64;
              g.envoff = envoff[x1];
              if (x1 > x0 && arena + bytes > ((int64_t)8 << 30)) break;
              g.off = arena; arena += bytes;
              big.push_back(g); srow.push_back(rows); rows += Lr + 1;
              x1++;
            }
            for (size_t x = x0; x < x1; x += MR_LANES_LONG) {      // few lanes per wave: these are the long, slow regions
              WaveDesc d{}; d.prof = -1; d.first = (int64_t)(x - x0); d.count = (int32_t)std::min<size_t>(MR_LANES_LONG, x1 - x);
              d.rows = hlen[(size_t)ord[(size_t)sel[x + d.count - 1]]] + 1;
              bw.push_back(d);
            }
            std::vector<int32_t> selb(sel.begin() + x0, sel.begin() + x1);
            HIPCHK(upload(ctx->w_mrsel, selb, st)); HIPCHK(upload(ctx->w_mrselrow, srow, st)); HIPCHK(upload(ctx->w_mrbig, big, st)); HIPCHK(upload(ctx->w_mrbigwaves, bw, st));
            if ((size_t)rows * MRV * 4 > ctx->w_mrslab.cap) HIPCHK(ctx->w_mrslab.alloc((size_t)rows * MRV * 4));
            HIPCHK(ctx->w_mrarena.alloc((size_t)arena));
            MrArgs mb{};
            mb.rd = ctx->rd; mb.sorted_uniq = d_sorted; mb.seed_read = ctx->d_seed_read.p; mb.prof = ctx->d_prof.p; mb.pairs = pl.pairs;
            mb.mr = ctx->w_mr.p; mb.ulist = ulist.p; mb.u0 = 0; mb.waves = ctx->w_mrbigwaves.p; mb.slab = (float4 *)ctx->w_mrslab.p;
            mb.rowoff = ctx->w_mrrowoff.p; mb.rowoff0 = 0; mb.n2off = ctx->w_n2off.p; mb.n2sc = ctx->w_n2sc.p; mb.out = ctx->w_mrout.p;
            mb.scratch = nullptr; mb.sel = ctx->w_mrsel.p; mb.sel_rowoff = ctx->w_mrselrow.p; mb.big = ctx->w_mrbig.p; mb.arena = ctx->w_mrarena.p; mb.envpool = ctx->w_mrenv.p;
            launch_mr_ensemble_big(mb, (int)bw.size(), st);
            x0 = x1;
          }
        }
      }
      S.ms_ensemble += tm_e.stop();
      HIPCHK(hipGetLastError());
      S.n_mr_clustered += NMR; S.n_mr_distinct += NU;
    }
  }
  // ---- compact regions into a profile-grouped list
  DBuf<int32_t> &d_rcnt = ctx->w_rcnt, &d_rpref = ctx->w_rpref, &d_scan_tmp = ctx->w_scan2;
  HIPCHK(d_rcnt.alloc((size_t)NP + 1)); HIPCHK(d_rpref.alloc((size_t)NP + 1)); HIPCHK(d_scan_tmp.alloc((size_t)scan_tmp_elems(NP + 1)));
  HIPCHK(hipMemsetAsync(d_rcnt.p, 0, ((size_t)NP + 1) * 4, st));
  RegionListArgs rl{};
  rl.pout = pl.pout; rl.raw = d_raw.p; rl.pv = pv; rl.npairs = NP;
  if (NMR > 0) { rl.mr_off = ctx->w_mroff.p; rl.mr_u = ctx->w_mru.p; rl.mrout = ctx->w_mrout.p; rl.envpool = ctx->w_mrenv.p; }
  {
    DBuf<int64_t> &d_c = ctx->w_counters;
    HIPCHK(d_c.alloc(16));
    HIPCHK(hipMemsetAsync(d_c.p, 0, 16 * sizeof(int64_t), st));
    launch_region_list_count(rl, d_rcnt.p, (unsigned long long *)d_c.p, st);
    int64_t hc[10] = {0};
    HIPCHK(hipMemcpyAsync(hc, d_c.p, sizeof(hc), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    S.n_mr_failed += hc[0]; S.n_mr_envelopes += hc[1];
    for (int k = 0; k < 8; k++) S.n_mr_fail_kind[k] += hc[2 + k];
  }
  launch_exclusive_scan(d_rcnt.p, d_rpref.p, NP + 1, d_scan_tmp.p, st);
  std::vector<int32_t> bound((size_t)P + 1);
  {
    DBuf<int64_t> &d_idx = ctx->w_idx; DBuf<int32_t> &d_b = ctx->w_b;
    HIPCHK(upload(d_idx, pl.seg_start, st)); HIPCHK(d_b.alloc((size_t)P + 1));
    hipLaunchKernelGGL(k_gather_i32, dim3((P + 1 + 255) / 256), dim3(256), 0, st, d_rpref.p, d_idx.p, P + 1, d_b.p);
    HIPCHK(hipMemcpyAsync(bound.data(), d_b.p, ((size_t)P + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  std::vector<int64_t> rseg((size_t)P + 1, 0);
  std::vector<int32_t> rtotal((size_t)P);
  for (int p = 0; p < P; p++) { rtotal[p] = bound[p + 1] - bound[p]; rseg[p + 1] = rseg[p] + ((int64_t)rtotal[p] + 63) / 64 * 64; S.n_domains += rtotal[p]; }
  const int64_t NR = rseg[P];
  ctx->dom_n[di] = count_only ? 0 : NR;                    // (count_only: this call leaves no segment of rows)
  HIPCHK(ctx->d_pair_region0.alloc((size_t)NP));
  HIPCHK(ctx->d_regions.alloc((size_t)std::max<int64_t>(NR, 1)));
  if (!count_only) {
    HIPCHK(d_dom.alloc((size_t)std::max<int64_t>(NR, 1)));
    HIPCHK(hipMemsetAsync(d_dom.p, 0xFF, (size_t)std::max<int64_t>(NR, 1) * sizeof(itsx_domain), st));
  }
  if (NR > 0) {
    DBuf<int64_t> &d_rseg = ctx->w_rseg;
    HIPCHK(upload(d_rseg, rseg, st));
    launch_region_offsets(NP, pl.pairs, d_rpref.p, pl.d_seg_start, d_rseg.p, ctx->d_pair_region0.p, st);
    HIPCHK(hipMemsetAsync(ctx->d_regions.p, 0xFF, (size_t)NR * sizeof(RegionRec), st));     // padding slots: pair = -1
    launch_region_list_fill(rl, ctx->d_pair_region0.p, ctx->d_regions.p, st);
    // ---- envelope memoisation: only distinct (profile, L, residues) envelopes are re-scored
    DBuf<unsigned long long> &rkeys = ctx->w_keys; DBuf<int32_t> &rvals = ctx->w_vals; DBuf<uint32_t> &rslot = ctx->w_slot_of;
    DBuf<int32_t> &rrep = ctx->w_rrep, &ruq = ctx->w_ruq, &rurank = ctx->w_rurank, &rscan = ctx->w_scan_tmp;
    const uint64_t tsize = region_table_size(NR);
    HIPCHK(rkeys.alloc(tsize)); HIPCHK(rvals.alloc(tsize)); HIPCHK(rslot.alloc((size_t)NR + 1));
    HIPCHK(rrep.alloc((size_t)NR + 1)); HIPCHK(ruq.alloc((size_t)NR + 1)); HIPCHK(rurank.alloc((size_t)NR + 1));
    HIPCHK(rscan.alloc((size_t)scan_tmp_elems(NR + 1))); HIPCHK(ctx->d_upos.alloc((size_t)NR + 1));
    HIPCHK(hipMemsetAsync(rkeys.p, 0, tsize * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(rvals.p, 0x7f, tsize * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(ruq.p, 0, ((size_t)NR + 1) * sizeof(int32_t), st));
    launch_region_keys(ctx->rd, ctx->d_regions.p, NR, pl.pairs, d_sorted, ctx->d_seed_read.p, rkeys.p, rvals.p, tsize - 1, rslot.p, st);
    launch_region_resolve(ctx->rd, ctx->d_regions.p, NR, pl.pairs, d_sorted, ctx->d_seed_read.p, rvals.p, rslot.p, rrep.p, ruq.p, st);
    launch_exclusive_scan(ruq.p, rurank.p, NR + 1, rscan.p, st);
    std::vector<int32_t> ub((size_t)P + 1);
    {
      DBuf<int64_t> &d_idx = ctx->w_idx; DBuf<int32_t> &d_b = ctx->w_b;
      HIPCHK(upload(d_idx, rseg, st)); HIPCHK(d_b.alloc((size_t)P + 1));
      hipLaunchKernelGGL(k_gather_i32, dim3((P + 1 + 255) / 256), dim3(256), 0, st, rurank.p, d_idx.p, P + 1, d_b.p);
      HIPCHK(hipMemcpyAsync(ub.data(), d_b.p, ((size_t)P + 1) * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    std::vector<int64_t> useg((size_t)P + 1, 0);
    std::vector<int32_t> utotal((size_t)P);
    for (int p = 0; p < P; p++) { utotal[p] = ub[p + 1] - ub[p]; useg[p + 1] = useg[p] + ((int64_t)utotal[p] + 63) / 64 * 64; S.n_env_unique += utotal[p]; }
    const int64_t NU = useg[P];
    DBuf<int64_t> &d_useg = ctx->w_useg;
    HIPCHK(upload(d_useg, useg, st));
    HIPCHK(ctx->d_ulist.alloc((size_t)std::max<int64_t>(NU, 1))); HIPCHK(ctx->d_rout.alloc((size_t)std::max<int64_t>(NU, 1)));
    HIPCHK(hipMemsetAsync(ctx->d_rout.p, 0, (size_t)std::max<int64_t>(NU, 1) * sizeof(RegionOut), st));
    launch_region_upos(NR, ctx->d_regions.p, pl.pairs, ruq.p, rurank.p, d_rseg.p, d_useg.p, ctx->d_upos.p, ctx->d_ulist.p, st);
    launch_region_upos_follow(NR, rrep.p, ruq.p, ctx->d_upos.p, st);
    std::vector<WaveDesc> rw; std::vector<char> rgen;
    for (int pass = 0; pass < 2; pass++)
      for (int p = 0; p < P; p++) {
        if ((int)ctx->generic_q[p] != pass) continue;
        for (int64_t k = 0; k < utotal[p]; k += 64) {
          WaveDesc w{}; w.prof = p; w.first = useg[p] + k; w.count = (int32_t)std::min<int64_t>(64, utotal[p] - k);
          rw.push_back(w); rgen.push_back((char)pass);
        }
      }
    const int NRW = (int)rw.size();
    DBuf<WaveDesc> &d_rw = ctx->w_rw; DBuf<int32_t> &d_rrows = ctx->w_rrows;
    HIPCHK(upload(d_rw, rw, st)); HIPCHK(d_rrows.alloc((size_t)NRW));
    hipLaunchKernelGGL(k_wave_rows_regions, dim3((NRW + 255) / 256), dim3(256), 0, st, d_rw.p, NRW, ctx->d_ulist.p, d_rrows.p);
    std::vector<int32_t> rrows((size_t)NRW);
    HIPCHK(hipMemcpyAsync(rrows.data(), d_rrows.p, (size_t)NRW * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t erow_bytes = 104 * 64 * 4;
    int64_t ebudget = (int64_t)(slab_gb * (1 << 30)) / erow_bytes;
    LazyTimers elazy(st);
    DBuf<float> &d_eslab = ctx->w_eslab; int64_t ealloc = (int64_t)(d_eslab.cap / (104 * 64));
    if (adapt && !sw_get("ITSX_SLAB_GB")) {                  // as for the parser slab: four batches are enough here
      int64_t total_rows = 0;
      for (int w = 0; w < NRW; w++) total_rows += rrows[(size_t)w];
      ebudget = std::min(ebudget, std::max(std::max(total_rows / 4 + 1, ((int64_t)2 << 30) / erow_bytes), ealloc));
    }
    int w0 = 0;
    while (w0 < NRW) {
      int w1 = w0; int64_t r = 0;
      while (w1 < NRW && rgen[w1] == rgen[w0] && (w1 == w0 || r + rrows[w1] <= ebudget)) { rw[w1].slab = r; rw[w1].rows = rrows[w1]; r += rrows[w1]; w1++; }
      if (r > ealloc) {
        if (d_eslab.alloc((size_t)r * 104 * 64) != hipSuccess) {      // as for the parser slab: a budget the device cannot supply is halved
          (void)hipGetLastError();
          ealloc = 0;
          if (w1 - w0 <= 1) SET_ERR(ctx, ITSX_E_NOMEM, "no device memory left for the envelope slab of a single wave");
          ebudget = std::max<int64_t>(r / 2, rrows[(size_t)w0]);
          S.n_slab_shrinks++;
          continue;
        }
        ealloc = r;
      }
      HIPCHK(hipMemcpyAsync(d_rw.p + w0, rw.data() + w0, (size_t)(w1 - w0) * sizeof(WaveDesc), hipMemcpyHostToDevice, st));
      EnvArgs a{};
      a.rd = ctx->rd; a.sorted_uniq = d_sorted; a.seed_read = ctx->d_seed_read.p; a.prof = ctx->d_prof.p; a.lt = ctx->d_lt.p;
      a.pairs = pl.pairs; a.regions = ctx->d_ulist.p; a.rout = ctx->d_rout.p; a.waves = d_rw.p; a.slab = d_eslab.p;
      { const size_t t = elazy.begin(&S.ms_env_kernel); launch_envelopes(a, w1 - w0, w0, rgen[w0], st); elazy.end(t); }
      for (int w = w0; w < w1; w++) S.env_rows += (int64_t)(rrows[w] - 1) * rw[w].count;
      w0 = w1;
    }
    ScoreArgs sa{};
    sa.rd = ctx->rd; sa.sorted_uniq = d_sorted; sa.seed_read = ctx->d_seed_read.p; sa.prof = ctx->d_prof.p; sa.lt = ctx->d_lt.p;
    sa.flogsum = ctx->d_flogsum.p; sa.pairs = pl.pairs; sa.pout = pl.pout; sa.regions = ctx->d_regions.p; sa.rout = ctx->d_rout.p;
    sa.pair_region0 = ctx->d_pair_region0.p; sa.upos = ctx->d_upos.p; sa.dom = count_only ? nullptr : d_dom.p; sa.npairs = NP; sa.T = T;
    if (NMR > 0) { sa.mr = ctx->w_mr.p; sa.mr_u = ctx->w_mru.p; sa.mrout = ctx->w_mrout.p; sa.n2off = ctx->w_n2off.p; sa.n2sc = ctx->w_n2sc.p; sa.mr_off = ctx->w_mroff.p; }
    sa.domz = ctx->d_domz32.p; sa.usample = ctx->dev_usample(); sa.P = ctx->P;
    launch_score(sa, st);
    if (ctx->sc_count_members && !count_only) { const int rc = count_member_targets(ctx, d_dom.p, NR); if (rc != ITSX_OK) return rc; }
    if (ctx->compact_rows && !count_only) {
      // keep what can still win once domZ is known, in row order; the chunk's full rows are scratch
      { const int rc = compact_segment(ctx, d_dom.p, NR, di); if (rc != ITSX_OK) return rc; }
    }
  }
  S.ms_domains += tm_dom.stop();
  // filter counters
  {
    DBuf<int64_t> &d_c = ctx->w_counters;
    HIPCHK(d_c.alloc(8));
    HIPCHK(hipMemsetAsync(d_c.p, 0, 8 * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_pair_counters, dim3((unsigned)std::min<int64_t>(4096, (NP + 255) / 256)), dim3(256), 0, st, pl.pout, NP, (unsigned long long *)d_c.p);
    int64_t hc[8];
    HIPCHK(hipMemcpyAsync(hc, d_c.p, sizeof(hc), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    S.n_past_bias += hc[0]; S.n_past_fwd += hc[1]; S.n_regions += hc[2]; S.n_domain_overflow += hc[3]; S.n_multidomain += hc[4];
  }
  HIPCHK(hipGetLastError());                                // a kernel of this chunk that failed to launch must not pass silently
  return ITSX_OK;
}


namespace itsx {
__global__ void k_dbg_group_count(const PairRec *__restrict__ pairs, int64_t NP, const unsigned long long *__restrict__ smask, const int8_t *__restrict__ cls, int ncls, unsigned long long *__restrict__ cnt)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NP || !((smask[i >> 6] >> (i & 63)) & 1ull)) return;
  const PairRec pr = pairs[i];
  if (pr.prof < 0) return;
  atomicAdd(&cnt[(size_t)pr.useq * ncls + cls[pr.prof]], 1ull);
}
__global__ void k_dbg_group_hist(const unsigned long long *__restrict__ cnt, int64_t ng, unsigned long long *__restrict__ hist)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ng) return;
  const unsigned long long c = cnt[i];
  const int b = c <= 4 ? (int)c : c <= 8 ? 5 : c <= 16 ? 6 : 7;
  atomicAdd(&hist[b], 1ull);
  if (c > 1) atomicAdd(&hist[8], c - 1);
  if (c > 2) atomicAdd(&hist[9], c - 2);
}
}  // namespace itsx

// The pairs that a marking kernel (k_lazy_mark, k_topup_mark) set a bit for, as a list of their own in l_pairs / d_pout: the chunk counts
// are scanned, the profiles' totals read at their segments' first chunks, and the set bits scattered.  Each profile keeps its segment,
// padded to 64 with 0xFF records, and its pairs their order.  nsel = pairs selected; sub.NP == 0: none (nothing was allocated).
// want_src: l_src[k] = the index in `pairs` of the new list's pair k (padding records: not written).
static int select_compact(itsx_ctx *ctx, const PairRec *pairs, int64_t NP, int P, const std::vector<int64_t> &seg_start, const int64_t *d_seg_start, PairList &sub, int64_t &nsel, bool want_src = false)
{
  hipStream_t st = ctx->st;
  const int64_t nch = (NP + 63) >> 6;
  launch_exclusive_scan(ctx->l_scnt.p, ctx->l_spos.p, nch + 1, ctx->l_scan.p, st);
  std::vector<int32_t> bound((size_t)P + 1);
  {
    DBuf<int64_t> &d_idx = ctx->w_idx; DBuf<int32_t> &d_b = ctx->w_b;
    HIPCHK(upload(d_idx, seg_start, st)); HIPCHK(d_b.alloc((size_t)P + 1));
    hipLaunchKernelGGL(k_gather_chunk_i32, dim3((P + 1 + 255) / 256), dim3(256), 0, st, ctx->l_spos.p, d_idx.p, P + 1, d_b.p);
    HIPCHK(hipMemcpyAsync(bound.data(), d_b.p, ((size_t)P + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  sub.seg_start.assign((size_t)P + 1, 0); sub.total.assign((size_t)P, 0);
  for (int p = 0; p < P; p++) { sub.total[(size_t)p] = bound[(size_t)p + 1] - bound[(size_t)p]; sub.seg_start[(size_t)p + 1] = sub.seg_start[(size_t)p] + ((int64_t)sub.total[(size_t)p] + 63) / 64 * 64; }
  sub.NP = sub.seg_start[(size_t)P];
  nsel = (int64_t)bound[(size_t)P] - bound[0];
  if (sub.NP == 0) return ITSX_OK;
  HIPCHK(ctx->l_pairs.alloc((size_t)sub.NP)); HIPCHK(ctx->d_pout.alloc((size_t)sub.NP));
  HIPCHK(hipMemsetAsync(ctx->l_pairs.p, 0xFF, (size_t)sub.NP * sizeof(PairRec), st));
  HIPCHK(hipMemsetAsync(ctx->d_pout.p, 0, (size_t)sub.NP * sizeof(PairOut), st));
  HIPCHK(upload(ctx->l_seg, sub.seg_start, st));
  if (want_src) HIPCHK(ctx->l_src.alloc((size_t)sub.NP));
  launch_lazy_scatter(pairs, NP, ctx->l_smask.p, ctx->l_spos.p, d_seg_start, ctx->l_seg.p, ctx->l_pairs.p, st, want_src ? ctx->l_src.p : nullptr);
  sub.pairs = ctx->l_pairs.p; sub.pout = ctx->d_pout.p; sub.d_seg_start = ctx->l_seg.p;
  return ITSX_OK;
}
// the selection's chunk buffers for a list of NP pairs (NP a multiple of 64: every segment is padded)
static int select_alloc(itsx_ctx *ctx, int64_t NP)
{
  if (NP & 63) SET_ERR(ctx, ITSX_E_DEVICE, "lazy stage: the pair list is not padded to whole chunks of 64");
  const int64_t nch = NP >> 6;                                  // one mask word and one count each (k_lazy.hip)
  HIPCHK(ctx->l_smask.alloc((size_t)nch + 1)); HIPCHK(ctx->l_scnt.alloc((size_t)nch + 2)); HIPCHK(ctx->l_spos.alloc((size_t)nch + 2));
  HIPCHK(ctx->l_scan.alloc((size_t)scan_tmp_elems(nch + 2)));
  return ITSX_OK;
}

// The lazy domain stage (k_lazy.hip): Forward scores for every pair of the chunk, then two rounds of the domain pipeline over
// the pairs that can still win ItsPosition's argmax.
static int lazy_rounds(itsx_ctx *ctx, const PairList &pl, const int32_t *d_sorted, int32_t u0, int32_t Uc, double T, double F1, double F3, const std::function<int()> *next_msv)
{
  hipStream_t st = ctx->st;
  const int P = ctx->P, ncls = ctx->compact_ncls;
  itsx_stats &S = ctx->stats;
  const int64_t NP = pl.NP;
  // ---- pass A: the Forward score of every pair (nothing else is kept)
  HIPCHK(ctx->l_fb.alloc((size_t)NP + 1)); HIPCHK(ctx->l_b10.alloc((size_t)NP + 1)); HIPCHK(ctx->l_done.alloc((size_t)NP + 1));
  { const int rc = select_alloc(ctx, NP); if (rc != ITSX_OK) return rc; }
  HIPCHK(ctx->l_gtop.alloc((size_t)Uc * ncls + 1));
  HIPCHK(hipMemsetAsync(ctx->l_done.p, 0, (size_t)NP + 1, st));
  HIPCHK(hipMemsetAsync(ctx->l_gtop.p, 0, ((size_t)Uc * ncls + 1) * sizeof(unsigned long long), st));
  if (ctx->share_on) {
    // prefix sharing (k_share.hip): the pairs of a profile ascend by processing position = (batch, depth, length); one launch takes the
    // chains of one (batch, depth) for every profile, the depths of a batch in ascending order -- a chain starts from the state that a
    // chain of a lower depth saved for the same profile
    const int maxd = ctx->share_maxd, DS = maxd + 1;
    const bool two = ctx->two_on;
    std::vector<int32_t> segflat, segdepth, segbatch;
    for (size_t bi = 0; bi < ctx->sh_batches.size(); bi++) {
      const auto &b = ctx->sh_batches[bi];
      if (b.k0 < u0 || b.k0 >= u0 + Uc) continue;
      for (int d = 0; d < DS; d++) { segflat.push_back(ctx->sh_segk_h[bi * SHARE_SEGS + d] - u0); segdepth.push_back(d); segbatch.push_back((int32_t)bi); }
    }
    const int nseg = (int)segdepth.size();
    segflat.push_back(Uc);
    if ((int64_t)nseg * P + 1 >= (1ll << 31)) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "prefix sharing: too many (batch, depth, profile) segments in one chunk");
    HIPCHK(upload(ctx->sh_segflat, segflat, st)); HIPCHK(upload(ctx->sh_segdepth, segdepth, st, 1)); HIPCHK(upload(ctx->w_rcnt, pl.total, st));
    HIPCHK(ctx->sh_bnd.alloc((size_t)(nseg + 1) * P)); HIPCHK(ctx->sh_wc.alloc((size_t)nseg * P + 2)); HIPCHK(ctx->sh_woff.alloc((size_t)nseg * P + 2));
    HIPCHK(ctx->sh_scan.alloc((size_t)scan_tmp_elems((int64_t)nseg * P + 2)));
    launch_share_bounds(pl.pairs, pl.d_seg_start, ctx->w_rcnt.p, ctx->sh_segflat.p, nseg, P, ctx->sh_bnd.p, st);
    launch_share_wcount(ctx->sh_bnd.p, nseg, P, ctx->sh_wc.p, st);
    launch_exclusive_scan(ctx->sh_wc.p, ctx->sh_woff.p, (int64_t)nseg * P + 1, ctx->sh_scan.p, st);
    std::vector<int32_t> woff((size_t)nseg * P + 1);
    HIPCHK(hipMemcpyAsync(woff.data(), ctx->sh_woff.p, woff.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int NW = woff.back();
    HIPCHK(ctx->w_waves.alloc((size_t)std::max(NW, 1))); HIPCHK(ctx->w_counters.alloc(512));
    HIPCHK(hipMemsetAsync(ctx->w_counters.p, 0, 512 * sizeof(int64_t), st));
    // the wave list from the segment bounds alone, the row counters by chain (k_share.hip).  Who reads a wave's last row from its descriptor
    // -- the launch dump, and the check hooks' kernels on the one-sided schedule's own list -- gets the list that looks at every pair
    // (its sums go to the spare counters: ITSX_SHARE_CHECK=1 runs it in any case and counts a sum that differs from the chains' as a mismatch)
    const bool dump = sw_get("ITSX_PASSA_DUMP") != nullptr;
    const bool share_check = sw_get("ITSX_SHARE_CHECK") && atoi(sw_get("ITSX_SHARE_CHECK")) != 0;
    const bool want_check = sw_get("ITSX_LAZY_CHECK_BOUND") || share_check;
    const bool need_rows = dump || (want_check && !two);
    const int Wn = (P + 31) / 32;
    launch_share_rows(Uc, Wn, ctx->sh_need.p, ctx->sh_ulen.p + u0, two ? ctx->sh_endrow.p + u0 : nullptr, ctx->sh_segflat.p, nseg, ctx->sh_segdepth.p, ctx->share_B, 0,
                      (unsigned long long *)ctx->w_counters.p, st);
    if (need_rows || share_check)
      launch_share_waves(NW, nseg, P, ctx->sh_woff.p, ctx->sh_bnd.p, ctx->sh_segdepth.p, ctx->share_B, pl.pairs, two ? ctx->sh_endrow.p + u0 : nullptr, 0, ctx->w_waves.p,
                         (unsigned long long *)ctx->w_counters.p + 256, st);
    if (!need_rows) launch_share_wavelist(NW, nseg, P, ctx->sh_woff.p, ctx->sh_bnd.p, ctx->w_waves.p, st);
    // the shared pass stores a pair's bound and its group's best beside its score (k_fwd_bound: ShareLaunch::b10): no pass over the list
    // for them afterwards; the padding records' b10 = 0 is written here
    launch_pad_b10(P, pl.d_seg_start, ctx->w_rcnt.p, ctx->l_b10.p, st);
    std::vector<int64_t> lr((size_t)512, 0);
    FloatArgs a{};
    a.rd = ctx->rd; a.sorted_uniq = d_sorted; a.seed_read = ctx->d_seed_read.p; a.prof = ctx->d_prof.p; a.lt = ctx->d_lt.p;
    a.pairs = pl.pairs; a.waves = ctx->w_waves.p; a.F1 = F1; a.F3 = F3;
    // ---- two-sided sharing (round 6): the Backward chains' work list.  A chain runs for a profile when a pair past the filter joins one of
    // its states, or a chain below it in the suffix tree runs (k_join_need / k_need_up_b); the list is made like the Forward pass's own
    const int maxrd = ctx->share_maxrd, DSB = maxrd + 1;
    int32_t cb0 = 0, Ubc = 0; int NWB = 0;
    std::vector<int32_t> bwoff;
    FloatArgs ab = a;
    if (two) {
      int32_t cb1 = 0; bool any = false;
      std::vector<int32_t> bsegflat, bsegdepth;
      for (size_t bi = 0; bi < ctx->sh_batches.size(); bi++) {
        const auto &b = ctx->sh_batches[bi];
        if (b.k0 < u0 || b.k0 >= u0 + Uc) continue;
        const int32_t lo = ctx->sh_bsegk_h[bi * SHARE_SEGS], hi = ctx->sh_bsegk_h[bi * SHARE_SEGS + SHARE_SEGS - 1];
        if (!any) { cb0 = lo; any = true; }
        cb1 = hi;
      }
      Ubc = any ? cb1 - cb0 : 0;
      for (size_t bi = 0; bi < ctx->sh_batches.size(); bi++) {
        const auto &b = ctx->sh_batches[bi];
        if (b.k0 < u0 || b.k0 >= u0 + Uc) continue;
        for (int d = 0; d < DSB; d++) { bsegflat.push_back(ctx->sh_bsegk_h[bi * SHARE_SEGS + d] - cb0); bsegdepth.push_back(d); }
      }
      const int nbseg = (int)bsegdepth.size();
      bsegflat.push_back(Ubc);
      bwoff.assign((size_t)nbseg * P + 1, 0);
      if (Ubc > 0) {
        const int W = (P + 31) / 32;
        HIPCHK(ctx->sh_needb.alloc((size_t)Ubc * W + 1));
        HIPCHK(hipMemsetAsync(ctx->sh_needb.p, 0, ((size_t)Ubc * W + 1) * 4, st));
        launch_join_need(ctx->sh_jlev.p + u0, ctx->sh_jownb.p + u0, Uc, W, cb0, ctx->sh_pass.p, ctx->sh_needb.p, st);
        for (int r = maxrd; r >= 1; r--) launch_need_up_b(r, ctx->sh_rdepth.p + cb0, ctx->sh_rparent.p + cb0, cb0, Ubc, W, ctx->sh_needb.p, st);
        HIPCHK(ctx->sh_resb.alloc((size_t)P * Ubc + 1));
        launch_need_res(ctx->sh_needb.p, Ubc, P, W, ctx->sh_resb.p, st);
        const int nchb = (Ubc + CHUNK - 1) / CHUNK;
        HIPCHK(ctx->sh_cntb.alloc((size_t)P * nchb)); HIPCHK(ctx->sh_totalb.alloc((size_t)P)); HIPCHK(ctx->sh_realb.alloc((size_t)P));
        launch_pair_count(ctx->sh_resb.p, P, Ubc, nchb, ctx->sh_cntb.p, st);
        launch_chunk_scan(ctx->sh_cntb.p, P, nchb, ctx->sh_totalb.p, ctx->sh_realb.p, st);
        std::vector<int32_t> totalb((size_t)P);
        HIPCHK(hipMemcpyAsync(totalb.data(), ctx->sh_totalb.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::vector<int64_t> bseg((size_t)P + 1, 0);
        for (int p = 0; p < P; p++) bseg[(size_t)p + 1] = bseg[(size_t)p] + ((int64_t)totalb[(size_t)p] + 63) / 64 * 64;
        const int64_t NPB = bseg[(size_t)P];
        if (NPB >= (1ll << 31) || (int64_t)nbseg * P + 1 >= (1ll << 31)) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "two-sided sharing: too many Backward chains in one chunk");
        if (NPB > 0) {
          HIPCHK(upload(ctx->sh_bseg_start, bseg, st));
          HIPCHK(ctx->sh_bpairs.alloc((size_t)NPB));
          launch_pair_fill(ctx->sh_resb.p, P, Ubc, nchb, ctx->sh_cntb.p, ctx->sh_bseg_start.p, ctx->sh_totalb.p, ctx->sh_bulen.p + cb0, ctx->sh_bpairs.p, st);
          HIPCHK(upload(ctx->sh_bsegflat, bsegflat, st)); HIPCHK(upload(ctx->sh_bsegdepth, bsegdepth, st, 1));
          HIPCHK(ctx->sh_bbnd.alloc((size_t)(nbseg + 1) * P)); HIPCHK(ctx->sh_bwc.alloc((size_t)nbseg * P + 2)); HIPCHK(ctx->sh_bwoff.alloc((size_t)nbseg * P + 2));
          HIPCHK(ctx->sh_scan.alloc((size_t)scan_tmp_elems((int64_t)nbseg * P + 2)));
          launch_share_bounds(ctx->sh_bpairs.p, ctx->sh_bseg_start.p, ctx->sh_totalb.p, ctx->sh_bsegflat.p, nbseg, P, ctx->sh_bbnd.p, st);
          launch_share_wcount(ctx->sh_bbnd.p, nbseg, P, ctx->sh_bwc.p, st);
          launch_exclusive_scan(ctx->sh_bwc.p, ctx->sh_bwoff.p, (int64_t)nbseg * P + 1, ctx->sh_scan.p, st);
          HIPCHK(hipMemcpyAsync(bwoff.data(), ctx->sh_bwoff.p, bwoff.size() * 4, hipMemcpyDeviceToHost, st));
          HIPCHK(hipStreamSynchronize(st));
          NWB = bwoff.back();
          HIPCHK(ctx->sh_bwaves.alloc((size_t)std::max(NWB, 1)));
          launch_share_rows(Ubc, W, ctx->sh_needb.p, nullptr, ctx->sh_bsteps.p + cb0, nullptr, 0, nullptr, 0, 1, (unsigned long long *)ctx->w_counters.p + 128, st);
          if (dump || share_check)
            launch_share_waves(NWB, nbseg, P, ctx->sh_bwoff.p, ctx->sh_bbnd.p, ctx->sh_bsegdepth.p, ctx->share_B, ctx->sh_bpairs.p, ctx->sh_bsteps.p + cb0, 1, ctx->sh_bwaves.p,
                               (unsigned long long *)ctx->w_counters.p + 384, st);
          if (!dump) launch_share_wavelist(NWB, nbseg, P, ctx->sh_bwoff.p, ctx->sh_bbnd.p, ctx->sh_bwaves.p, st);
          ab.sorted_uniq = ctx->sh_border.p + cb0; ab.pairs = ctx->sh_bpairs.p; ab.waves = ctx->sh_bwaves.p;
        }
      }
    }
    HIPCHK(hipMemcpyAsync(lr.data(), ctx->w_counters.p, 512 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    // diagnostic (scripts/passa_launches.py): every launch's waves and wave-rows, in launch order, to set against a kernel trace
    std::vector<WaveDesc> dumpf, dumpb;
    if (dump) {
      dumpf.resize((size_t)std::max(NW, 1)); dumpb.resize((size_t)std::max(NWB, 1));
      HIPCHK(hipMemcpyAsync(dumpf.data(), ctx->w_waves.p, (size_t)NW * sizeof(WaveDesc), hipMemcpyDeviceToHost, st));
      if (NWB > 0) HIPCHK(hipMemcpyAsync(dumpb.data(), ctx->sh_bwaves.p, (size_t)NWB * sizeof(WaveDesc), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    auto dump_launch = [&](const char *what, int batch, int d, int w0, int w1, const std::vector<WaveDesc> &wv, int row0) {
      int64_t rows = 0, mx = 0, lanes = 0;
      for (int w = w0; w < w1; w++) { const int64_t r = wv[(size_t)w].rows - 1 - row0; rows += r; mx = std::max(mx, r); lanes += wv[(size_t)w].count; }
      fprintf(stderr, "[passa] %s batch %d depth %d waves %d wave_rows %lld max_rows %lld lanes %lld\n", what, batch, d, w1 - w0, (long long)rows, (long long)mx, (long long)lanes);
    };
    StageTimer tm(st);
    LazyTimers tb(st);                                      // the Backward chains' share of the pass (batches on the main stream)
    // (batches are independent: every other one on a second stream with its own half of the slot buffer, so that a launch's tail --
    // the next depth waits for its last waves -- is filled by the other batch's waves)
    hipStream_t alt = st;
    if (ctx->sh_fslots_half > 0 && nseg > DS) {
      if (!ctx->st3) {
        if (hipStreamCreateWithFlags(&ctx->st3, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ctx->st3 = nullptr; }
        else { (void)hipEventCreateWithFlags(&ctx->ev_s3a, hipEventDisableTiming); (void)hipEventCreateWithFlags(&ctx->ev_s3b, hipEventDisableTiming); }
      }
      if (ctx->st3) { alt = ctx->st3; HIPCHK(hipEventRecord(ctx->ev_s3a, st)); HIPCHK(hipStreamWaitEvent(alt, ctx->ev_s3a, 0)); }
    }
    for (int t0 = 0; t0 < nseg; t0 += DS) {                 // one batch: its profile ranges one after the other, depths ascending
      const auto &b = ctx->sh_batches[(size_t)segbatch[(size_t)t0]];
      const bool on_alt = alt != st && ((t0 / DS) & 1);
      hipStream_t bs = on_alt ? alt : st;
      float4 *fsl = (float4 *)ctx->w_slab.p + (on_alt ? ctx->sh_fslots_half : 0);
      float4 *gsl = fsl + ctx->sh_gslots_off;
      const int tb0 = (t0 / DS) * DSB;
      for (int r = 0; r < b.nsplit; r++) {
        const int pa = (int)((int64_t)P * r / b.nsplit), pb = (int)((int64_t)P * (r + 1) / b.nsplit);
        if (pb <= pa) continue;
        // the batch's Backward chains first, the deepest suffixes last (a chain starts from the state a shorter suffix's chain saved):
        // every state a Forward chain of this batch joins is there before the first of them runs
        const size_t tbi = (two && NWB > 0 && bs == st) ? tb.begin(&S.ms_bwd_bound) : (size_t)-1;
        if (two && NWB > 0)
          for (int d = 0; d < DSB; d++) {
            const int t = tb0 + d;
            const int w0 = bwoff[(size_t)t * P + pa], w1 = bwoff[(size_t)t * P + pb];
            if (w1 <= w0) continue;
            ShareLaunch sl{};
            sl.src = ctx->sh_rsrc.p + cb0; sl.mask = ctx->sh_rmask.p + cb0; sl.node0 = ctx->sh_rnode0.p + cb0; sl.endrow = ctx->sh_bsteps.p + cb0;
            sl.slots = gsl; sl.node_base = b.gnode0; sl.p0 = pa; sl.Pb = pb - pa; sl.depth = d; sl.logB = ctx->share_logB;
            sl.chain = ctx->sh_bchain.p + cb0; sl.entab = ctx->d_entab.p;
            if (sw_get("ITSX_TEST_HOOKS") && sw_get("ITSX_PASSA_DBG")) sl.dbg = atoi(sw_get("ITSX_PASSA_DBG"));
            if (dump) dump_launch("bwd", t0 / DS, d, w0, w1, dumpb, 0);
            for (int w = w0; w < w1; w += 1 << 20) { launch_bwd_bound_share(ab, ctx->d_btab.p, ctx->d_rtab.p, std::min(1 << 20, w1 - w), w, sl, bs); S.n_bwd_launches++; }
          }
        if (tbi != (size_t)-1) tb.end(tbi);
        for (int d = 0; d < DS; d++) {
          const int t = t0 + d;
          const int w0 = woff[(size_t)t * P + pa], w1 = woff[(size_t)t * P + pb];
          if (w1 <= w0) continue;
          ShareLaunch sl{};
          sl.src = ctx->sh_src.p + u0; sl.mask = ctx->sh_mask.p + u0; sl.node0 = ctx->sh_node0.p + u0;
          sl.slots = fsl; sl.node_base = b.node0; sl.p0 = pa; sl.Pb = pb - pa; sl.depth = d; sl.logB = ctx->share_logB;
          sl.b10 = ctx->l_b10.p; sl.done = ctx->l_done.p; sl.gtop = ctx->l_gtop.p; sl.cls = ctx->w_cls.p; sl.ncls = ncls;
          if (two) {
            sl.endrow = ctx->sh_endrow.p + u0; sl.jlev = ctx->sh_jlev.p + u0; sl.jsrc = ctx->sh_jsrc.p + u0; sl.gslots = gsl; sl.gnode_base = b.gnode0;
            if (!sw_get("ITSX_NO_CHAINREC")) { sl.chain = ctx->sh_chain.p + u0; sl.entab = ctx->d_entab.p; }
            if (sw_get("ITSX_TEST_HOOKS") && sw_get("ITSX_PASSA_DBG")) sl.dbg = atoi(sw_get("ITSX_PASSA_DBG"));
          }
          if (dump) dump_launch("fwd", t0 / DS, d, w0, w1, dumpf, d << ctx->share_logB);
          for (int w = w0; w < w1; w += 1 << 20) { launch_fwd_bound_share(a, ctx->d_btab.p, ctx->bound_fold, ctx->l_fb.p, std::min(1 << 20, w1 - w), w, sl, bs); S.n_bound_launches++; }
        }
      }
    }
    if (alt != st) { HIPCHK(hipEventRecord(ctx->ev_s3b, alt)); HIPCHK(hipStreamWaitEvent(st, ctx->ev_s3b, 0)); }
    const float ms = tm.stop();
    tb.collect();
    S.ms_bound_kernel += ms; S.ms_filters += ms;
    int64_t by_pair[3] = {0, 0, 0}, by_chain[3] = {0, 0, 0};
    for (int q = 0; q < 64; q++) {
      by_chain[0] += lr[(size_t)2 * q]; by_chain[1] += lr[(size_t)2 * q + 1]; by_chain[2] += lr[(size_t)128 + 2 * q];
      by_pair[0] += lr[(size_t)256 + 2 * q]; by_pair[1] += lr[(size_t)256 + 2 * q + 1]; by_pair[2] += lr[(size_t)384 + 2 * q];
    }
    S.bound_rows += by_chain[0]; S.bound_rows_full += by_chain[1]; S.bwd_rows += by_chain[2];
    if (share_check)                                        // test hook: the three sums pair by pair (k_share_waves) against the chains' (k_share_rows)
      for (int q = 0; q < 3; q++) S.share_mismatch += by_pair[q] != by_chain[q];
    // the check hooks below run every pair from row 1: their waves reach the pairs' last rows
    if (two && want_check)
      launch_share_waves(NW, nseg, P, ctx->sh_woff.p, ctx->sh_bnd.p, ctx->sh_segdepth.p, ctx->share_B, pl.pairs, nullptr, 0, ctx->w_waves.p, (unsigned long long *)ctx->w_counters.p + 256, st);
    if (sw_get("ITSX_LAZY_CHECK_BOUND")) {       // test hook: the shared chains' scores against HMMER's own arithmetic from row 1
      DBuf<float> ref;
      HIPCHK(ref.alloc((size_t)NP + 1));
      for (int t = 0; t < nseg; t++)
        for (int p = 0; p < P; p++) {
          const int w0 = woff[(size_t)t * P + p], w1 = woff[(size_t)t * P + p + 1];
          if (w1 > w0) launch_fwd_bound(a, ref.p, w1 - w0, w0, (int)ctx->generic_q[(size_t)p], st);
        }
      std::vector<float> h0((size_t)NP), h1((size_t)NP); std::vector<PairRec> hp((size_t)NP);
      HIPCHK(hipMemcpyAsync(h0.data(), ref.p, (size_t)NP * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(h1.data(), ctx->l_fb.p, (size_t)NP * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hp.data(), pl.pairs, (size_t)NP * sizeof(PairRec), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      float mx = S.lazy_bound_maxdiff;
      for (int64_t i = 0; i < NP; i++) {
        if (hp[(size_t)i].prof < 0 || hp[(size_t)i].xj < 0) continue;          // (a pair that ran for its row states only has no score)
        const float x = h0[(size_t)i], y = h1[(size_t)i];
        if (x != x || y != y) { if ((x != x) != (y != y)) mx = 1e30f; continue; }
        mx = std::max(mx, fabsf(x - y));
      }
      S.lazy_bound_maxdiff = mx;
    }
    if (sw_get("ITSX_SHARE_CHECK") && atoi(sw_get("ITSX_SHARE_CHECK")) != 0) {
      // test hook: every pair again from row 1 (the same wave list serves: a wave needs its profile, its pairs and its longest target).  A
      // chain that ran on its own to L has the unshared score bit for bit; a JOINED pair's score is the same sum over paths in another
      // order of operations: it must agree within 2e-3 nats (join_maxdiff reports the largest difference)
      HIPCHK(ctx->sh_fb_chk.alloc((size_t)NP + 1));
      for (int w0 = 0; w0 < NW; w0 += 1 << 20) launch_fwd_bound_seq(a, ctx->d_btab.p, ctx->bound_fold, ctx->sh_fb_chk.p, std::min(1 << 20, NW - w0), w0, st);
      HIPCHK(hipMemsetAsync(ctx->sh_counters.p + 8, 0, 2 * sizeof(unsigned long long), st));
      launch_diff_scores(ctx->l_fb.p, ctx->sh_fb_chk.p, pl.pairs, NP, two ? ctx->sh_jlev.p + u0 : nullptr, ctx->sh_counters.p + 8, st);
      unsigned long long nd[2] = {0, 0};
      HIPCHK(hipMemcpyAsync(nd, ctx->sh_counters.p + 8, sizeof(nd), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      S.share_mismatch += (int64_t)nd[0];
      S.join_maxdiff = std::max(S.join_maxdiff, __builtin_bit_cast(float, (uint32_t)nd[1]));
    }
  } else {
    // the waves over every pair, fast (Q == 12) profiles first, then runtime-Q ones: built on the device (k_waves_build)
    std::vector<int32_t> order; std::vector<int64_t> woff(1, 0);
    int64_t nfast64 = 0;
    for (int pass = 0; pass < 2; pass++)
      for (int p = 0; p < P; p++) {
        if ((int)ctx->generic_q[p] != pass) continue;
        order.push_back(p);
        woff.push_back(woff.back() + ((int64_t)pl.total[(size_t)p] + 63) / 64);
        if (pass == 0) nfast64 = woff.back();
      }
    if (woff.back() >= (1ll << 31)) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "more than 2^31 waves of pairs in one chunk");
    const int NW = (int)woff.back(), nfast = (int)nfast64;
    DBuf<int32_t> &d_order = ctx->w_b; DBuf<int64_t> &d_woff = ctx->w_idx; DBuf<int32_t> &d_tot = ctx->w_rcnt;
    HIPCHK(upload(d_order, order, st)); HIPCHK(upload(d_woff, woff, st)); HIPCHK(upload(d_tot, pl.total, st));
    HIPCHK(ctx->w_waves.alloc((size_t)std::max(NW, 1))); HIPCHK(ctx->w_counters.alloc(16));
    HIPCHK(hipMemsetAsync(ctx->w_counters.p, 0, 16 * sizeof(int64_t), st));
    if (NW > 0) hipLaunchKernelGGL(k_waves_build, dim3((NW + 255) / 256), dim3(256), 0, st, NW, (int)order.size(), d_order.p, d_woff.p, pl.d_seg_start, d_tot.p,
                                   pl.pairs, ctx->w_waves.p, (unsigned long long *)ctx->w_counters.p);
    int64_t lane_rows = 0;
    HIPCHK(hipMemcpyAsync(&lane_rows, ctx->w_counters.p, sizeof(lane_rows), hipMemcpyDeviceToHost, st));
    FloatArgs a{};
    a.rd = ctx->rd; a.sorted_uniq = d_sorted; a.seed_read = ctx->d_seed_read.p; a.prof = ctx->d_prof.p; a.lt = ctx->d_lt.p;
    a.pairs = pl.pairs; a.waves = ctx->w_waves.p; a.F1 = F1; a.F3 = F3;
    StageTimer tm(st);
    // launches of at most 2^20 waves: the timers of bench.py's roofline block want more than one sample
    static const bool exact_bound = sw_get("ITSX_LAZY_EXACT_BOUND") && atoi(sw_get("ITSX_LAZY_EXACT_BOUND")) != 0;     // A/B: HMMER's own Forward as the bound pass
    if (!exact_bound) {
      for (int w0 = 0; w0 < NW; w0 += 1 << 20) { launch_fwd_bound_seq(a, ctx->d_btab.p, ctx->bound_fold, ctx->l_fb.p, std::min(1 << 20, NW - w0), w0, st); S.n_bound_launches++; }
    } else {
      for (int w0 = 0; w0 < nfast; w0 += 1 << 20) { launch_fwd_bound(a, ctx->l_fb.p, std::min(1 << 20, nfast - w0), w0, 0, st); S.n_bound_launches++; }
      if (NW > nfast) { launch_fwd_bound(a, ctx->l_fb.p, NW - nfast, nfast, 1, st); S.n_bound_launches++; }
    }
    const float ms = tm.stop();
    S.ms_bound_kernel += ms; S.ms_filters += ms;
    if (sw_get("ITSX_LAZY_CHECK_BOUND") && !exact_bound) {      // test hook: the fast kernel's scores against HMMER's own arithmetic
      DBuf<float> ref;
      HIPCHK(ref.alloc((size_t)NP + 1));
      for (int w0 = 0; w0 < nfast; w0 += 1 << 20) launch_fwd_bound(a, ref.p, std::min(1 << 20, nfast - w0), w0, 0, st);
      if (NW > nfast) launch_fwd_bound(a, ref.p, NW - nfast, nfast, 1, st);
      std::vector<float> h0((size_t)NP), h1((size_t)NP); std::vector<PairRec> hp((size_t)NP);
      HIPCHK(hipMemcpyAsync(h0.data(), ref.p, (size_t)NP * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(h1.data(), ctx->l_fb.p, (size_t)NP * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hp.data(), pl.pairs, (size_t)NP * sizeof(PairRec), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      float mx = S.lazy_bound_maxdiff;
      for (int64_t i = 0; i < NP; i++) {
        if (hp[(size_t)i].prof < 0) continue;
        const float x = h0[(size_t)i], y = h1[(size_t)i];
        if (x != x || y != y) { if ((x != x) != (y != y)) mx = 1e30f; continue; }
        mx = std::max(mx, fabsf(x - y));
      }
      S.lazy_bound_maxdiff = mx;
    }
    S.bound_rows += lane_rows; S.bound_rows_full += lane_rows;     // (its copy was waited for with the kernel's timer)
  }
  StageTimer tm_sel(st);
  LazyArgs la{};
  la.pairs = pl.pairs; la.NP = NP; la.fb = ctx->l_fb.p; la.lt = ctx->d_lt.p; la.cls = ctx->w_cls.p; la.ncls = ncls; la.sorted_uniq = d_sorted;
  la.b10 = ctx->l_b10.p; la.gtop = ctx->l_gtop.p; la.bestc = ctx->w_bestc.p; la.done = ctx->l_done.p; la.smask = ctx->l_smask.p; la.scnt = ctx->l_scnt.p; la.ngroups = (int64_t)Uc * ncls;
  HIPCHK(ctx->l_thr.alloc((size_t)Uc * ncls + 1));
  la.thr = ctx->l_thr.p; la.nthr = (int64_t)Uc * ncls; la.nbest = (int64_t)ctx->w_bestc.n;
  if (!ctx->share_on) launch_lazy_bound(la, st);          // (the shared pass A has stored b10, done and gtop itself)
  float ms_sel = tm_sel.stop();
  for (int round = 0; round < 2; round++) {
    StageTimer tm_r(st);
    launch_lazy_mark(la, round, st);
    if (round == 1 && sw_get("ITSX_LAZY_HIST")) {      // experiment: how many candidates a group sends into round 2
      const int64_t ng = (int64_t)Uc * ncls;
      HIPCHK(hipMemsetAsync(ctx->l_gtop.p, 0, (size_t)ng * 8, st));
      hipLaunchKernelGGL(k_dbg_group_count, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, st, pl.pairs, NP, ctx->l_smask.p, ctx->w_cls.p, ncls, ctx->l_gtop.p);
      DBuf<unsigned long long> hist; HIPCHK(hist.alloc(16)); HIPCHK(hipMemsetAsync(hist.p, 0, 16 * 8, st));
      hipLaunchKernelGGL(k_dbg_group_hist, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, st, ctx->l_gtop.p, ng, hist.p);
      unsigned long long h[16];
      HIPCHK(hipMemcpyAsync(h, hist.p, sizeof(h), hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
      fprintf(stderr, "[itsx] round 2 candidates per group: 0:%llu 1:%llu 2:%llu 3:%llu 4:%llu 5-8:%llu 9-16:%llu 17+:%llu; pairs beyond a group's first %llu, beyond its second %llu\n",
              h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9]);
    }
    PairList sub; int64_t nsel = 0;
    { const int rc = select_compact(ctx, pl.pairs, NP, P, pl.seg_start, pl.d_seg_start, sub, nsel); if (rc != ITSX_OK) return rc; }
    const bool last = round == 1;
    if (sub.NP == 0) {
      ms_sel += tm_r.stop();
      if (last && next_msv) { const int rc = (*next_msv)(); if (rc != ITSX_OK) return rc; }
      continue;
    }
    ms_sel += tm_r.stop();
    S.n_lazy_evaluated += nsel;
    if (round == 0) S.n_lazy_round1 += nsel;
    { const int rc = domain_pipeline(ctx, sub, d_sorted, T, F1, F3, last ? next_msv : nullptr); if (rc != ITSX_OK) return rc; }
  }
  S.ms_lazy_select += ms_sel; S.ms_filters += ms_sel;
  // (the list, the bounds and the done flags stay where they are: the top-up round of itsx_search_finalize reads them when this was the
  // search's only chunk)
  ctx->topup.valid = !ctx->completing; ctx->topup.list_live = !ctx->completing; ctx->topup.NP = NP; ctx->topup.seg_start = pl.seg_start; ctx->topup.total = pl.total; ctx->topup.u0 = u0; ctx->topup.Uc = Uc;
  return ITSX_OK;
}

// The MSV filter's arguments for the cU sequences seed_read[sorted[0 .. cU)] of `rd`, every profile, unshared, with the tables
// filter_tables left on the device (search_chunk's msv_for, orient_profiles).
// blocks of 256 sequences x PB profiles: a few thousand blocks at least, and up to 32 profiles per block so that a
// large job re-reads its sequences' packed words (from L2) 32 times less often than it has profiles
// test hook ITSX_MSV_PB: the profiles a block takes its sequences through, whatever the job's size (a small job gets 1)
static int msv_pb_forced() { return sw_get("ITSX_MSV_PB") ? std::max(1, std::min(32, atoi(sw_get("ITSX_MSV_PB")))) : 0; }
static int msv_pb(int64_t cU, int np)
{
  const int64_t tiles = (cU + 255) / 256;
  const int pb_forced = msv_pb_forced();
  return pb_forced ? pb_forced : (int)std::max<int64_t>(1, std::min<int64_t>(32, tiles * np / 4096));
}
static MsvArgs msv_args(const itsx_ctx *ctx, const ReadsDev &rd, const int32_t *sorted, const int32_t *seed_read, int32_t cU, int Lcap, uint16_t *res)
{
  MsvArgs a{};
  a.rd = rd; a.sorted_uniq = sorted; a.seed_read = seed_read; a.U = cU; a.G = ctx->G;
  a.etab = ctx->d_etab.p; a.pbias = ctx->d_pbias.p; a.ptec = ctx->d_ptec.p; a.ptbm = ctx->d_ptbm.p;
  a.thr = ctx->w_thr.p; a.tjb = ctx->w_tjb.p; a.Lcap = Lcap; a.res = res;
  a.P = ctx->P;
  a.PB = msv_pb(cU, ctx->P);
  return a;
}

// one chunk [u0, u0+U) of the length-sorted unique list through every stage up to per-sequence reporting
static int search_chunk(itsx_ctx *ctx, int ci, int32_t u0, int32_t U, int Lcap, double T, double F1, double F3)
{
  (void)ci;
  hipStream_t st = ctx->st;
  const int P = ctx->P, G = ctx->G, Ppad = G * 64;
  itsx_stats &S = ctx->stats;
  // PairRec::useq is relative to the chunk; with prefix sharing it is the PROCESSING position: (batch, depth, length) order
  const bool sh = ctx->share_on;
  const int32_t *d_sorted = (sh ? ctx->sh_order.p : ctx->d_sorted_uniq.p) + u0;
  const int32_t *d_ulen = (sh ? ctx->sh_ulen.p : ctx->d_ulen.p) + u0;
  ctx->trace_u0 = u0;
  // ---- MSV for every (unique, profile)
  DBuf<uint16_t> &d_res = ctx->w_res;
  HIPCHK(d_res.alloc((size_t)Ppad * std::max<int64_t>(U, ctx->next_u0 >= 0 ? ctx->next_U : 0)));
  auto msv_for = [&](int64_t cu0, int32_t cU, hipStream_t s, int lds_pad = 0, uint16_t *res_out = nullptr, bool shared = true) {
    MsvArgs a = msv_args(ctx, ctx->rd, (sh ? ctx->sh_order.p : ctx->d_sorted_uniq.p) + cu0, ctx->d_seed_read.p, cU, Lcap, res_out ? res_out : d_res.p);
    if (ctx->completing) {           // only the listed profiles are filtered; every other row of res must read "not passed"
      a.plist = ctx->d_plist.p; a.nlist = (int32_t)ctx->h_plist.size();
      (void)hipMemsetAsync(a.res, 0, (size_t)Ppad * (size_t)cU * sizeof(uint16_t), s);
    }
    const int np = a.plist ? a.nlist : P;
    const int pb_forced = msv_pb_forced();
    a.PB = msv_pb(cU, np);
    // (the completion filters a handful of profiles: its launches would be a hundred tiny ones per chunk -- it runs unshared, on the same
    // processing order)
    if (!sh || !shared || ctx->completing) { launch_msv(a, s, lds_pad); return; }
    // prefix sharing: batch by batch (the saved states of one batch fit the slot buffer), depth by depth (a chain starts from a state
    // that a chain of a lower depth saved: launches of one stream run in order).  Batches are independent of each other: every other
    // one runs on a second stream with a slot buffer of its own, so that the tail of one launch -- the next depth waits for its last
    // blocks -- is filled by the other batch's blocks (and blocks may take their sequences through more profiles: fewer re-reads)
    static const bool two = !(sw_get("ITSX_SHARE_MSV_STREAMS") && atoi(sw_get("ITSX_SHARE_MSV_STREAMS")) < 2);
    int nbatch_here = 0;
    for (const auto &b : ctx->sh_batches) nbatch_here += (b.k0 >= cu0 && b.k0 < cu0 + cU);
    hipStream_t alt = s;
    if (two && nbatch_here > 1) {
      if (!ctx->st3) {
        if (hipStreamCreateWithFlags(&ctx->st3, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ctx->st3 = nullptr; }
        else { (void)hipEventCreateWithFlags(&ctx->ev_s3a, hipEventDisableTiming); (void)hipEventCreateWithFlags(&ctx->ev_s3b, hipEventDisableTiming); }
      }
      if (ctx->st3) { alt = ctx->st3; (void)hipEventRecord(ctx->ev_s3a, s); (void)hipStreamWaitEvent(alt, ctx->ev_s3a, 0); }
    }
    // two-sided sharing (round 6): the filter is max-plus arithmetic on integers, so a chain that stops where its suffix is shared and
    // takes the rest from the saved Backward state (k_msv_bwd) gets the unshared kernel's xJ exactly (ITSX_SHARE_CHECK counts cells)
    static const bool msv_two = !(sw_get("ITSX_MSV_TWO") && atoi(sw_get("ITSX_MSV_TWO")) == 0);
    const bool bi2 = ctx->two_on && msv_two;
    int32_t cb0 = 0;
    if (bi2) { bool any = false; for (const auto &b : ctx->sh_batches) if (b.k0 >= cu0 && b.k0 < cu0 + cU && !any) { cb0 = ctx->sh_bsegk_h[(size_t)(&b - ctx->sh_batches.data()) * SHARE_SEGS]; any = true; } }
    int seen = 0;
    for (const auto &b : ctx->sh_batches) {
      if (b.k0 < cu0 || b.k0 >= cu0 + cU) continue;
      const size_t bi = (size_t)(&b - ctx->sh_batches.data());
      const bool on_alt = alt != s && (seen++ & 1);
      hipStream_t bs = on_alt ? alt : s;
      uint4 *slots = ctx->sh_mslots.p + (on_alt ? ctx->sh_mslots_half : 0);
      uint4 *gslots = bi2 ? ctx->sh_mgslots.p + (on_alt ? ctx->sh_mgslots_half : 0) : nullptr;
      for (int r = 0; r < b.nsplit; r++) {
        const int pa = (int)((int64_t)np * r / b.nsplit), pb = (int)((int64_t)np * (r + 1) / b.nsplit);
        if (pb <= pa) continue;
        if (bi2)
          for (int d = 0; d <= ctx->share_maxrd; d++) {       // the batch's Backward chains, shortest suffixes first
            const int32_t k0 = ctx->sh_bsegk_h[bi * SHARE_SEGS + d], k1 = ctx->sh_bsegk_h[bi * SHARE_SEGS + d + 1];
            if (k1 <= k0) continue;
            MsvArgs c = a;
            c.sorted_uniq = ctx->sh_border.p + cb0; c.U = 0; c.res = nullptr;
            c.k0 = (int32_t)(k0 - cb0); c.k1 = (int32_t)(k1 - cb0); c.pfirst = pa; c.plast = pb; c.share = 2;
            if (sw_get("ITSX_TEST_HOOKS") && sw_get("ITSX_PASSA_DBG")) c.sl.dbg = atoi(sw_get("ITSX_PASSA_DBG"));
            c.sl.src = ctx->sh_rsrc.p + cb0; c.sl.mask = ctx->sh_rmask.p + cb0; c.sl.node0 = ctx->sh_rnode0.p + cb0; c.sl.endrow = ctx->sh_bsteps.p + cb0;
            c.sl.slots = gslots; c.sl.node_base = b.gnode0; c.sl.p0 = pa; c.sl.Pb = pb - pa; c.sl.depth = d; c.sl.logB = ctx->share_logB;
            const int64_t t2 = ((int64_t)(k1 - k0) + 255) / 256;
            c.PB = (int)std::max<int64_t>(1, std::min<int64_t>(32, t2 * (pb - pa) / (alt != s ? 4096 : 16384)));
            if (pb_forced) c.PB = pb_forced;
            launch_msv(c, bs, lds_pad);
          }
        for (int d = 0; d <= ctx->share_maxd; d++) {
          const int32_t k0 = ctx->sh_segk_h[bi * SHARE_SEGS + d], k1 = ctx->sh_segk_h[bi * SHARE_SEGS + d + 1];
          if (k1 <= k0) continue;
          MsvArgs c = a;
          c.k0 = (int32_t)(k0 - cu0); c.k1 = (int32_t)(k1 - cu0); c.pfirst = pa; c.plast = pb; c.share = 1;
          c.xb_cnt = ctx->msv_xb.p;                  // (nullptr unless the search counts xB branches: run_chunks)
          c.sl.src = ctx->sh_src.p + cu0; c.sl.mask = ctx->sh_mask.p + cu0; c.sl.node0 = ctx->sh_node0.p + cu0;
          c.sl.slots = slots; c.sl.node_base = b.node0; c.sl.p0 = pa; c.sl.Pb = pb - pa; c.sl.depth = d; c.sl.logB = ctx->share_logB;
          if (bi2) { c.sl.endrow = ctx->sh_endrow.p + cu0; c.sl.jlev = ctx->sh_jlev.p + cu0; c.sl.jsrc = ctx->sh_jsrc.p + cu0; c.sl.gslots = gslots; c.sl.gnode_base = b.gnode0; }
          // (a launch ends when its last blocks end, and the next depth waits for it: many short blocks -- rounds of the ~1 000-1 500 a
          // chip holds -- rather than a few long ones that take their sequences through 32 profiles; with the other batch's launches
          // beside it a block may be four times as long)
          const int64_t t2 = ((int64_t)(k1 - k0) + 255) / 256;
          c.PB = (int)std::max<int64_t>(1, std::min<int64_t>(32, t2 * (pb - pa) / (alt != s ? 4096 : 16384)));
          if (pb_forced) c.PB = pb_forced;
          launch_msv(c, bs, lds_pad);
        }
      }
    }
    if (alt != s) { (void)hipEventRecord(ctx->ev_s3b, alt); (void)hipStreamWaitEvent(s, ctx->ev_s3b, 0); }
  };
  if (ctx->msv_pre_u0 == (int64_t)u0) {
    // launched on st2 while the chunk before this one was in its domain stage
    HIPCHK(hipStreamWaitEvent(st, ctx->ev_msv1, 0));
    HIPCHK(hipEventSynchronize(ctx->ev_msv1));
    float ms = 0; (void)hipEventElapsedTime(&ms, ctx->ev_msv0, ctx->ev_msv1);
    S.ms_msv_kernel += ms;                       // its stretched wall time beside other kernels: not extra step time
    S.msv_launches += 1;
    ctx->msv_pre_u0 = -1;
  } else {
    StageTimer tm(st);
    msv_for(u0, U, st);
    const float ms = tm.stop();
    S.ms_msv_kernel += ms; S.ms_msv += ms;
    S.msv_launches += 1;
  }
  StageTimer tm_list(st);
  // ---- survivor list grouped by profile (64-aligned segments, ascending length)
  const int nchunks = (U + CHUNK - 1) / CHUNK;
  DBuf<int32_t> &d_cnt = ctx->w_cnt, &d_total = ctx->w_total;
  HIPCHK(d_cnt.alloc((size_t)P * nchunks)); HIPCHK(d_total.alloc((size_t)P));
  const bool lazy_now = ctx->lazy && !ctx->completing;
  if (sh && sw_get("ITSX_SHARE_CHECK") && atoi(sw_get("ITSX_SHARE_CHECK")) != 0) {
    // test hook: the same chunk through the unshared kernel; every cell of the result must be the same
    HIPCHK(ctx->sh_res_chk.alloc((size_t)Ppad * (size_t)U));
    msv_for(u0, U, st, 0, ctx->sh_res_chk.p, false);
    HIPCHK(hipMemsetAsync(ctx->sh_counters.p + 8, 0, sizeof(unsigned long long), st));
    launch_diff_u16(d_res.p, ctx->sh_res_chk.p, (int64_t)P * U, ctx->sh_counters.p + 8, st);
    unsigned long long nd = 0;
    HIPCHK(hipMemcpyAsync(&nd, ctx->sh_counters.p + 8, sizeof(nd), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    S.share_mismatch += (int64_t)nd;
  }
  if (sh && lazy_now) {
    // pass A runs a pair that failed the filter when a chain below it passed: it needs the row states (PairRec::xj = -1)
    const int W = (P + 31) / 32;
    HIPCHK(ctx->sh_pass.alloc((size_t)U * W + 1)); HIPCHK(ctx->sh_need.alloc((size_t)U * W + 1));
    launch_need_bits(d_res.p, U, P, W, ctx->sh_pass.p, ctx->sh_need.p, st);
    for (int d = ctx->share_maxd; d >= 1; d--) launch_need_up(d, ctx->sh_depth.p + u0, ctx->sh_parent.p + u0, U, W, ctx->sh_need.p, st);
    HIPCHK(hipMemsetAsync(ctx->sh_counters.p + 9, 0, sizeof(unsigned long long), st));
    launch_need_mark(d_res.p, U, P, W, ctx->sh_pass.p, ctx->sh_need.p, ctx->sh_counters.p + 9, st);
  }
  HIPCHK(ctx->sh_real.alloc((size_t)P));
  launch_pair_count(d_res.p, P, U, nchunks, d_cnt.p, st);
  launch_chunk_scan(d_cnt.p, P, nchunks, d_total.p, ctx->sh_real.p, st);
  std::vector<int32_t> total((size_t)P), real((size_t)P);       // pairs on the list / pairs past the filter (the same without sharing)
  HIPCHK(hipMemcpyAsync(total.data(), d_total.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(real.data(), ctx->sh_real.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<int64_t> seg_start((size_t)P + 1, 0);
  for (int p = 0; p < P; p++) { seg_start[p + 1] = seg_start[p] + ((int64_t)total[p] + 63) / 64 * 64; if (ctx->completing) S.n_lazy_completed += real[p]; else S.n_past_msv += real[p]; S.n_share_helpers += total[p] - real[p]; }
  const int64_t NP = seg_start[P];
  ctx->npairs_padded = ctx->lazy ? 0 : NP;
  if (NP == 0) { S.ms_msv += tm_list.stop(); ctx->dom_n.push_back(0); while (ctx->dom_bufs.size() < ctx->dom_n.size()) ctx->dom_bufs.emplace_back(new DBuf<itsx_domain>()); return ITSX_OK; }
  if (NP >= (1ll << 31)) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "more than 2^31 surviving (representative, profile) pairs");
  DBuf<int64_t> &d_seg_start = ctx->w_seg_start;
  HIPCHK(upload(d_seg_start, seg_start, st));
  ctx->topup.list_live = false;
  HIPCHK(ctx->d_pairs.alloc((size_t)NP));                    // (k_pair_fill writes all of it, the segments' padding included)
  if (!lazy_now) {                                 // (the lazy stage keeps a PairOut only for the pairs it evaluates)
    HIPCHK(ctx->d_pout.alloc((size_t)NP));
    HIPCHK(hipMemsetAsync(ctx->d_pout.p, 0, (size_t)NP * sizeof(PairOut), st));
  }
  launch_pair_fill(d_res.p, P, U, nchunks, d_cnt.p, d_seg_start.p, d_total.p, d_ulen, ctx->d_pairs.p, st);
  S.ms_msv += tm_list.stop();
  const int64_t zub_scale = sw_get("ITSX_LAZY_ZUB_SCALE") ? std::max<int64_t>(1, atoll(sw_get("ITSX_LAZY_ZUB_SCALE"))) : 1;   // test hook: looser bounds, more undecided rows
  if (!ctx->completing)
    // an upper bound of hmmsearch's domZ: every reported target is a pair past the MSV filter.  Sample-blind: every sample gets the
    // chunk's count.  In a sharing search (itsx_set_sample_sharing_lazy) real[p] counts the HOLDERS past the filter, and stays a bound
    // for every sample: a sample holds at most one member of a class, so the classes past the filter for p are at least any one
    // sample's uniques past it
    for (int p = 0; p < P; p++)
      for (int32_t sm = 0; sm < ctx->S; sm++) ctx->domz_ub_loc[(size_t)sm * P + p] += (int64_t)real[p] * zub_scale;
  PairList pl;
  pl.pairs = ctx->d_pairs.p; pl.pout = lazy_now ? nullptr : ctx->d_pout.p; pl.NP = NP; pl.seg_start = seg_start; pl.total = total; pl.d_seg_start = d_seg_start.p;
  // the next chunk's MSV filter on the second stream (its result buffer is free: this chunk's survivor list is built)
  const std::function<int()> next_msv = [&]() -> int {
    const bool msv_overlap = !(sw_get("ITSX_MSV_OVERLAP") && atoi(sw_get("ITSX_MSV_OVERLAP")) == 0);     // (read at every search: bench.py times one step without the overlap)
    if (msv_overlap && ctx->next_u0 >= 0 && ctx->st2 && !ctx->keep_trace) {
      if (!ctx->ev_msv0) {
        HIPCHK(hipEventCreate(&ctx->ev_msv0)); HIPCHK(hipEventCreate(&ctx->ev_msv1));
        HIPCHK(hipEventCreateWithFlags(&ctx->ev_c, hipEventDisableTiming));
      }
      HIPCHK(hipEventRecord(ctx->ev_c, st)); HIPCHK(hipStreamWaitEvent(ctx->st2, ctx->ev_c, 0));
      HIPCHK(hipEventRecord(ctx->ev_msv0, ctx->st2));
      msv_for(ctx->next_u0, ctx->next_U, ctx->st2, sw_get("ITSX_MSV_PAD") ? atoi(sw_get("ITSX_MSV_PAD")) : 40000);
      HIPCHK(hipEventRecord(ctx->ev_msv1, ctx->st2));
      ctx->msv_pre_u0 = ctx->next_u0;
    }
    return ITSX_OK;
  };
  if (lazy_now) return lazy_rounds(ctx, pl, d_sorted, u0, U, T, F1, F3, &next_msv);
  { const int rc = domain_pipeline(ctx, pl, d_sorted, T, F1, F3, &next_msv); if (rc != ITSX_OK) return rc; }
  if (ctx->keep_trace) { const int rc = append_traces(ctx); if (rc != ITSX_OK) return rc; }
  return ITSX_OK;
}

int itsx_set_rows_mode(itsx_ctx *ctx, int mode)
{
  CTXCHK(ctx);
  if (mode < -1 || mode > ITSX_ROWS_LAZY) SET_ERR(ctx, ITSX_E_ARG, "itsx_set_rows_mode: mode must be -1 (environment), 0 (full), 1 (compact) or 2 (lazy)");
  ctx->rows_mode = mode;
  return ITSX_OK;
}
int64_t itsx_lazy_pending(const itsx_ctx *ctx) { return ctx ? ctx->lazy_pending : -1; }
int itsx_lazy_pending_profiles(const itsx_ctx *ctx, int32_t *flags)
{
  CTXCHK(ctx && flags && ctx->searched());
  for (int p = 0; p < ctx->P; p++) flags[p] = (ctx->lazy && (size_t)p < ctx->lazy_pending_prof.size()) ? (ctx->lazy_pending_prof[(size_t)p] != 0) : 0;
  return ITSX_OK;
}
int itsx_topup_counters(const itsx_ctx *ctx, int64_t *counters)
{
  CTXCHK(ctx && counters);
  counters[0] = ctx->n_topup_deferred; counters[1] = ctx->n_topup_ensemble;
  return ITSX_OK;
}
int itsx_set_partial_coords(itsx_ctx *ctx, int on) { CTXCHK(ctx); ctx->partial_coords = on != 0; return ITSX_OK; }
int itsx_set_kept_rows(itsx_ctx *ctx, int on) { CTXCHK(ctx); if (ctx->kept_rows != (on != 0)) { ctx->h_dom.clear(); ctx->drop_alignments(); } ctx->kept_rows = on != 0; return ITSX_OK; }
// flags[n_unique]: 1 where an undecided row could still change the representative's coordinates (the rows itsx_lazy_pending counts)
int itsx_lazy_pending_uniques(itsx_ctx *ctx, uint8_t *flags)
{
  CTXCHK(ctx && flags && ctx->searched());
  if (ctx->U <= 0) return ITSX_OK;
  if (!ctx->lazy || !ctx->finalized() || ctx->l_uflag.n < (size_t)ctx->U) { memset(flags, 0, (size_t)ctx->U); return ITSX_OK; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(flags, ctx->l_uflag.p, (size_t)ctx->U, hipMemcpyDeviceToHost, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  return ITSX_OK;
}
// Exact counters for the flagged profiles: EVERY pair of theirs past the MSV filter goes through the domain pipeline (the ones the
// lazy rounds evaluated already come again -- their rows are duplicates with the same rank key, which changes no argmax), so that the
// reported targets of these profiles are counted, not bounded.  Afterwards this context's lower and upper counters of the flagged
// profiles are equal; a multi-rank driver exchanges the counters again before it finalizes.
int itsx_lazy_complete(itsx_ctx *ctx, const int32_t *flags)
{
  CTXCHK(ctx && flags && ctx->searched());
  if (!ctx->lazy) SET_ERR(ctx, ITSX_E_ARG, "itsx_lazy_complete: the last search was not a lazy one");
  if (ctx->injected) SET_ERR(ctx, ITSX_E_ARG, "itsx_lazy_complete: the row table was handed in (itsx_debug_set_domains): there are no pairs to evaluate");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const int P = ctx->P;
  ctx->h_plist.clear();
  for (int p = 0; p < P; p++) if (flags[p]) ctx->h_plist.push_back(p);
  if (ctx->h_plist.empty() || ctx->U_active == 0) return ITSX_OK;
  // the rows are added to, so they are to be finalized again; a completion that fails half way leaves no search to finalize
  StageTxn txn(ctx, itsx_ctx::ST_SEARCHED, itsx_ctx::ST_GROUPED);
  StageTimer tm(st);
  HIPCHK(upload(ctx->d_plist, ctx->h_plist, st));
  // the flagged profiles are counted afresh (k_score adds one per reported target)
  std::vector<int32_t> dz32((size_t)P * ctx->S, 0);
  HIPCHK(hipMemcpyAsync(dz32.data(), ctx->d_domz32.p, dz32.size() * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int32_t sm = 0; sm < ctx->S; sm++) for (int p : ctx->h_plist) dz32[(size_t)sm * P + p] = 0;
  HIPCHK(hipMemcpyAsync(ctx->d_domz32.p, dz32.data(), dz32.size() * 4, hipMemcpyHostToDevice, st));
  // after a sharing search (itsx_set_sample_sharing_lazy) the holders are walked again -- the prefix tree, the chunks and the classes
  // are that search's --, the members are counted as there, and the kept rows of the segments added here are copied to the members
  const bool shared = ctx->shared_lazy;
  if (shared) {
    const int rcw = set_walked_uniques(ctx, &ctx->h_sorted_searched);
    if (rcw != ITSX_OK) { (void)set_walked_uniques(ctx, nullptr); return rcw; }
    ctx->sc_count_members = true;
  }
  ctx->completing = true;
  int rc = run_chunks(ctx, ctx->T, ctx->sF1, ctx->sF3);
  ctx->completing = false;
  if (shared) {
    ctx->sc_count_members = false;
    { const int rc2 = set_walked_uniques(ctx, nullptr); if (rc == ITSX_OK) rc = rc2; }      // (every exit leaves the context walking all its uniques again)
    if (rc == ITSX_OK) rc = expand_shared_rows(ctx, ctx->sc_segs_done, false);
  }
  if (rc != ITSX_OK) return rc;
  HIPCHK(hipMemcpyAsync(dz32.data(), ctx->d_domz32.p, dz32.size() * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int32_t sm = 0; sm < ctx->S; sm++)
    for (int p : ctx->h_plist) {
      const size_t z = (size_t)sm * P + p;
      ctx->domz_loc[z] = ctx->domz_ub_loc[z] = dz32[z];
      if (!ctx->domz_exchanged) ctx->domz[z] = ctx->domz_ub[z] = dz32[z];
    }
  ctx->stats.n_lazy_completed_profiles += (int64_t)ctx->h_plist.size();
  ctx->stats.n_rows_resident = 0;
  for (int64_t r : ctx->dom_n) ctx->stats.n_rows_resident += r;
  ctx->stats.ms_lazy_complete += tm.stop();
  txn.commit(itsx_ctx::ST_SEARCHED);
  return ITSX_OK;
}

// After a lazy search the counters are BOUNDS on hmmsearch's domZ: [S][P] reported targets among the evaluated pairs (below),
// then [S][P] pairs past the MSV filter (above).  itsx_get_domz / itsx_set_domz move the lower half only when the search was
// not lazy; after a lazy search they move both halves (2 x S x P values), like itsx_domz_device.
int itsx_get_domz(const itsx_ctx *ctx, int64_t *domZ)
{
  CTXCHK(ctx && domZ && ctx->searched());
  // this context's OWN counters (what a multi-rank driver sums), whatever itsx_set_domz / an in-place reduction put in their place
  for (size_t p = 0; p < ctx->domz_loc.size(); p++) domZ[p] = ctx->domz_loc[p];
  if (ctx->lazy) for (size_t p = 0; p < ctx->domz_ub_loc.size(); p++) domZ[ctx->domz_loc.size() + p] = ctx->domz_ub_loc[p];
  return ITSX_OK;
}
int itsx_set_domz(itsx_ctx *ctx, const int64_t *domZ)
{
  CTXCHK(ctx && domZ && ctx->searched());
  for (size_t p = 0; p < ctx->domz.size(); p++) ctx->domz[p] = domZ[p];
  if (ctx->lazy) for (size_t p = 0; p < ctx->domz_ub.size(); p++) ctx->domz_ub[p] = domZ[ctx->domz.size() + p];
  ctx->domz_on_device = false; ctx->domz_exchanged = true;
  ctx->drop_alignments();
  return ITSX_OK;
}
int64_t itsx_domz_count(const itsx_ctx *ctx) { return ctx ? (int64_t)ctx->domz.size() * (ctx->lazy ? 2 : 1) : -1; }

// ---- device-resident exchange (multi-GPU): the caller reduces / gathers these buffers where they are (RCCL), nothing bounces
// through host arrays.  Pointers stay valid until the next call that recomputes the same quantity.
int itsx_domz_device(itsx_ctx *ctx, int64_t **d_domz, int64_t *n)
{
  CTXCHK(ctx && d_domz && ctx->searched());
  HIPCHK(hipSetDevice(ctx->device));
  const size_t m = ctx->domz.size(), mm = m * (ctx->lazy ? 2 : 1);
  HIPCHK(ctx->d_domz64.alloc(std::max<size_t>(mm, 1)));
  // (this context's OWN counters: after an exchange ctx->domz holds the ranks' sums, and a second exchange -- after
  // itsx_lazy_complete -- must not add them up again)
  if (m) HIPCHK(hipMemcpyAsync(ctx->d_domz64.p, ctx->domz_loc.data(), m * 8, hipMemcpyHostToDevice, ctx->st));
  if (m && ctx->lazy) HIPCHK(hipMemcpyAsync(ctx->d_domz64.p + m, ctx->domz_ub_loc.data(), m * 8, hipMemcpyHostToDevice, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  ctx->domz_on_device = true; ctx->domz_exchanged = true;
  *d_domz = ctx->d_domz64.p;
  if (n) *n = (int64_t)mm;
  return ITSX_OK;
}

// Test hook: a hand-made domain table in place of a search's results.  rows[n_rows] in n_segs segments of seg_rows[s] rows each (a
// segment = what one chunk of a search leaves; empty ones are allowed); rows with dom_idx < 0 are padding and stay as given, every
// other row names a representative of the finished dereplication and a loaded profile.  mode = ITSX_ROWS_FULL: the segments stay as
// they are; ITSX_ROWS_COMPACT: each goes through compact_segment, as a chunk does; ITSX_ROWS_LAZY: they are the rows a lazy search
// kept.  The counters ([S][P], twice that for lazy) are zero: the caller gives them with itsx_set_domz, then itsx_search_finalize.
int itsx_debug_set_domains(itsx_ctx *ctx, const itsx_domain *rows, int64_t n_rows, const int64_t *seg_rows, int32_t n_segs, int mode)
{
  CTXCHK(ctx);
  if (!ctx->grouped()) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_set_domains called before itsx_derep / itsx_cluster");
  if (ctx->P <= 0) SET_ERR(ctx, ITSX_E_ARG, "no profiles loaded");
  if (mode < ITSX_ROWS_FULL || mode > ITSX_ROWS_LAZY) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_set_domains: mode must be 0 (full), 1 (compact) or 2 (lazy)");
  if (n_rows < 0 || n_segs < 0 || (n_rows > 0 && !rows) || (n_segs > 0 && !seg_rows)) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_set_domains: missing arrays");
  int64_t sum = 0;
  for (int32_t s = 0; s < n_segs; s++) {
    if (seg_rows[s] < 0 || seg_rows[s] > (int64_t)INT32_MAX - 4096) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_set_domains: segment " + std::to_string(s) + " has a row count outside [0, 2^31 - 4096]");
    sum += seg_rows[s];
  }
  if (sum != n_rows) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_set_domains: the segments hold " + std::to_string(sum) + " rows, " + std::to_string(n_rows) + " were given");
  for (int64_t i = 0; i < n_rows; i++) {
    const itsx_domain &d = rows[i];
    if (d.dom_idx < 0) continue;
    if (d.rep < 0 || d.rep >= ctx->U) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_set_domains: row " + std::to_string(i) + " names representative " + std::to_string(d.rep) + " of " + std::to_string(ctx->U));
    if (d.prof < 0 || d.prof >= ctx->P) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_set_domains: row " + std::to_string(i) + " names profile " + std::to_string(d.prof) + " of " + std::to_string(ctx->P));
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const size_t m = (size_t)ctx->P * ctx->S;
  StageTxn txn(ctx, itsx_ctx::ST_GROUPED);
  ctx->switches_at_search = sw_report();
  ctx->injected = true;
  ctx->domz.assign(m, 0); ctx->domz_ub.assign(m, 0); ctx->domz_loc.assign(m, 0); ctx->domz_ub_loc.assign(m, 0);
  ctx->npairs_padded = 0; ctx->dom_n.clear(); ctx->n_chunks = n_segs;
  ctx->compact_rows = mode != ITSX_ROWS_FULL; ctx->lazy = mode == ITSX_ROWS_LAZY;
  itsx_stats &S = ctx->stats;
  S.lazy = ctx->lazy; S.n_domains = 0; S.n_lazy_pending = S.n_lazy_reruns = S.n_lazy_topup = S.n_lazy_completed = S.n_lazy_completed_profiles = S.n_lazy_pending_profiles = 0; ctx->n_topup_deferred = ctx->n_topup_ensemble = 0;
  for (int64_t i = 0; i < n_rows; i++) S.n_domains += rows[i].dom_idx >= 0;
  HIPCHK(ctx->d_domz32.alloc(std::max<size_t>(m, 1)));
  HIPCHK(hipMemsetAsync(ctx->d_domz32.p, 0, std::max<size_t>(m, 1) * 4, st));
  if (ctx->compact_rows) { const int rc = compact_setup(ctx); if (rc != ITSX_OK) return rc; }
  int64_t o = 0;
  for (int32_t s = 0; s < n_segs; s++) {
    const size_t di = ctx->dom_n.size();
    const int64_t NR = seg_rows[s];
    ctx->dom_n.push_back(0);
    while (ctx->dom_bufs.size() <= di) ctx->dom_bufs.emplace_back(new DBuf<itsx_domain>());
    if (NR > 0) {
      DBuf<itsx_domain> &d_dom = mode == ITSX_ROWS_COMPACT ? ctx->w_domscratch : *ctx->dom_bufs[di];
      HIPCHK(d_dom.alloc((size_t)NR));
      HIPCHK(hipMemcpyAsync(d_dom.p, rows + o, (size_t)NR * sizeof(itsx_domain), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
      ctx->dom_n[di] = NR;
      if (mode == ITSX_ROWS_COMPACT) { const int rc = compact_segment(ctx, d_dom.p, NR, di); if (rc != ITSX_OK) return rc; }
    }
    o += NR;
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  S.n_rows_resident = 0;
  for (int64_t r : ctx->dom_n) S.n_rows_resident += r;
  txn.commit(itsx_ctx::ST_SEARCHED);
  return ITSX_OK;
}

// Test hook: the rows the context holds as they lie in its segments (segment after segment, padding rows included, dom_reported as the
// last finalize left it -- 2 = undecided after a lazy one): the count; the rows too when cap holds them all.  Negative on error.
int64_t itsx_debug_get_rows(itsx_ctx *ctx, itsx_domain *rows, int64_t cap)
{
  if (!ctx || !ctx->searched()) return ITSX_E_ARG;
  int64_t n = 0;
  for (int64_t r : ctx->dom_n) n += std::max<int64_t>(r, 0);
  if (!rows || cap < n) return n;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->st));
  int64_t o = 0;
  for (size_t c = 0; c < ctx->dom_n.size(); c++) {
    if (ctx->dom_n[c] <= 0) continue;
    HIPCHK(hipMemcpy(rows + o, ctx->dom_bufs[c]->p, (size_t)ctx->dom_n[c] * sizeof(itsx_domain), hipMemcpyDeviceToHost));
    o += ctx->dom_n[c];
  }
  return n;
}

// thresholds of a lazy search: rows both bounds decide alike are final; ctx->lazy_pending = undecided rows that could matter
static int finalize_lazy(itsx_ctx *ctx, double domE)
{
  hipStream_t st = ctx->st;
  const size_t m = ctx->domz.size();
  DBuf<int64_t> &d_dz = ctx->domz_on_device ? ctx->d_domz64 : ctx->w_dz;
  if (ctx->domz_on_device) {             // reduced in place by the caller: lower bounds, then upper bounds
    if (m) { HIPCHK(hipMemcpyAsync(ctx->domz.data(), d_dz.p, m * 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipMemcpyAsync(ctx->domz_ub.data(), d_dz.p + m, m * 8, hipMemcpyDeviceToHost, st)); }
  } else {
    std::vector<int64_t> both(ctx->domz); both.insert(both.end(), ctx->domz_ub.begin(), ctx->domz_ub.end());
    HIPCHK(upload(d_dz, both, st, 2));
  }
  const int32_t U = ctx->U; const int ncls = std::max(ctx->compact_ncls, 1);
  HIPCHK(ctx->l_sure.alloc((size_t)U * ncls + 1)); HIPCHK(ctx->l_has.alloc((size_t)U + 1)); HIPCHK(ctx->w_counters.alloc(16));
  HIPCHK(hipMemsetAsync(ctx->l_sure.p, 0, ((size_t)U * ncls + 1) * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(ctx->l_has.p, 0, ((size_t)U + 1) * sizeof(int32_t), st));
  HIPCHK(hipMemsetAsync(ctx->w_counters.p, 0, 16 * sizeof(int64_t), st));
  HIPCHK(ctx->l_pflag.alloc((size_t)std::max(ctx->P, 1)));
  HIPCHK(hipMemsetAsync(ctx->l_pflag.p, 0, (size_t)std::max(ctx->P, 1) * 4, st));
  HIPCHK(ctx->l_uflag.alloc((size_t)U + 1));
  HIPCHK(hipMemsetAsync(ctx->l_uflag.p, 0, (size_t)U + 1, st));
  {   // per profile: what would settle its undecided rows from below / from above (lazy_topup); the split between the two lies 60 % of the way up
    const size_t Pn = (size_t)std::max(ctx->P, 1);
    std::vector<unsigned long long> init(2 * Pn), split(Pn, 0);
    for (size_t p = 0; p < Pn; p++) {
      init[2 * p] = 0; init[2 * p + 1] = ~0ull;
      if (p < ctx->domz.size() && ctx->S == 1) {
        double lo = (double)ctx->domz[p], hi = (double)std::max(ctx->domz_ub[p], ctx->domz[p]);
        // (no more targets than the profile has pairs on the last search's list, whatever the upper bound says: a multi-rank sum, a test's inflated bound)
        if (ctx->topup.valid && ctx->n_chunks == 1 && p < ctx->topup.total.size()) hi = std::min(hi, std::max(lo, (double)ctx->topup.total[p]));
        split[p] = (unsigned long long)(lo + 0.6 * (hi - lo));
      }
    }
    HIPCHK(upload(ctx->l_zneed, init, st)); HIPCHK(upload(ctx->l_zsplit, split, st));
  }
  for (size_t c = 0; c < ctx->dom_n.size(); c++)
    if (ctx->dom_n[c] > 0) launch_finalize_lazy(ctx->dom_bufs[c]->p, ctx->dom_n[c], d_dz.p, d_dz.p + m, domE, ctx->dev_usample(), ctx->P, st);
  for (size_t c = 0; c < ctx->dom_n.size(); c++)
    if (ctx->dom_n[c] > 0) launch_lazy_sure(ctx->dom_bufs[c]->p, ctx->dom_n[c], ctx->w_cls.p, ncls, ctx->l_sure.p, ctx->l_has.p, st);
  for (size_t c = 0; c < ctx->dom_n.size(); c++)
    if (ctx->dom_n[c] > 0) launch_lazy_pending(ctx->dom_bufs[c]->p, ctx->dom_n[c], ctx->w_cls.p, ncls, ctx->l_sure.p, ctx->l_has.p, (unsigned long long *)ctx->w_counters.p, ctx->l_pflag.p, ctx->l_uflag.p, ctx->S == 1 ? ctx->l_zneed.p : nullptr, ctx->l_zsplit.p, domE, st);
  int64_t pend = 0;
  ctx->h_zneed.assign((size_t)std::max(ctx->P, 1) * 2, 0);
  HIPCHK(hipMemcpyAsync(ctx->h_zneed.data(), ctx->l_zneed.p, (size_t)std::max(ctx->P, 1) * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&pend, ctx->w_counters.p, sizeof(pend), hipMemcpyDeviceToHost, st));
  ctx->lazy_pending_prof.assign((size_t)std::max(ctx->P, 1), 0);
  HIPCHK(hipMemcpyAsync(ctx->lazy_pending_prof.data(), ctx->l_pflag.p, (size_t)std::max(ctx->P, 1) * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  { int np = 0; for (int32_t f : ctx->lazy_pending_prof) np += f != 0; ctx->stats.n_lazy_pending_profiles = np; }
  if (sw_get("ITSX_LAZY_FORCE_PENDING")) pend += atoll(sw_get("ITSX_LAZY_FORCE_PENDING"));      // test hook: exercises the full re-run
  ctx->lazy_pending = pend; ctx->stats.n_lazy_pending = pend;
  return ITSX_OK;
}

// The bounds after a sub-round of the top-up (its profiles: ctx->topup_profs): reported among the evaluated pairs below, those + the pairs
// still not evaluated above (a pair the count-only round deferred is one of the latter until it is evaluated)
static int topup_bounds(itsx_ctx *ctx, bool with_deferred)
{
  hipStream_t st = ctx->st;
  const auto &tu = ctx->topup;
  const std::vector<int32_t> &prof_of = ctx->topup_profs;
  const int ns = (int)prof_of.size(), P = ctx->P;
  std::vector<int32_t> dz32((size_t)P * ctx->S, 0);
  HIPCHK(hipMemcpyAsync(dz32.data(), ctx->d_domz32.p, dz32.size() * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(upload(ctx->w_idx, tu.seg_start, st)); HIPCHK(upload(ctx->w_rcnt, tu.total, st)); HIPCHK(upload(ctx->l_pslot, prof_of, st));      // (the pipeline used the buffers)
  HIPCHK(ctx->l_tcnt.alloc((size_t)std::max(ns, 1)));
  HIPCHK(hipMemsetAsync(ctx->l_tcnt.p, 0, (size_t)std::max(ns, 1) * sizeof(unsigned long long), st));
  launch_topup_count(ctx->l_done.p, ctx->w_idx.p, ctx->w_rcnt.p, ctx->l_pslot.p, ns, ctx->l_tcnt.p, st);
  std::vector<unsigned long long> ndone((size_t)ns, 0), ndef((size_t)ns, 0);
  if (ns > 0) HIPCHK(hipMemcpyAsync(ndone.data(), ctx->l_tcnt.p, (size_t)ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  if (with_deferred && ns > 0) {                          // the profiles' deferred pairs: what a second sub-round could still add to / take off their bounds
    HIPCHK(ctx->l_tcnt2.alloc((size_t)ns));
    HIPCHK(hipMemsetAsync(ctx->l_tcnt2.p, 0, (size_t)ns * sizeof(unsigned long long), st));
    launch_topup_count_mask(ctx->l_dmask.p, ctx->w_idx.p, ctx->w_rcnt.p, ctx->l_pslot.p, ns, ctx->l_tcnt2.p, st);
    HIPCHK(hipMemcpyAsync(ndef.data(), ctx->l_tcnt2.p, (size_t)ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  ctx->topup_defp.assign((size_t)P, 0);
  for (int k = 0; k < ns; k++) ctx->topup_defp[(size_t)prof_of[(size_t)k]] = (int64_t)ndef[(size_t)k];
  for (size_t z = 0; z < dz32.size(); z++) { ctx->domz_loc[z] = dz32[z]; ctx->domz[z] = dz32[z]; }
  for (int k = 0; k < ns; k++) {
    const int p = prof_of[(size_t)k];
    const int64_t left = (int64_t)tu.total[(size_t)p] - (int64_t)ndone[(size_t)k];       // (helper pairs, xj < 0, are marked done by k_lazy_bound)
    const int64_t hi = (int64_t)dz32[(size_t)p] + std::max<int64_t>(0, left);
    if (hi < ctx->domz_ub[(size_t)p]) { ctx->domz_ub[(size_t)p] = hi; ctx->domz_ub_loc[(size_t)p] = hi; }
    if (sw_get("ITSX_LAZY_HIST")) fprintf(stderr, "[itsx] top-up: profile %d now %d .. %lld\n", p, dz32[(size_t)p], (long long)ctx->domz_ub[(size_t)p]);
  }
  return ITSX_OK;
}

// The top-up round (round 6).  A row is undecided when domE / P-value lies between the bounds on its profile's domZ -- the reported
// targets among the EVALUATED pairs below, the pairs past the MSV filter above.  On amplicon data nearly every pair past the filter is a
// reported target, so the truth is almost always "domZ is far larger, the row is not reported", and proving it does not take the exact
// count (itsx_lazy_complete: every pair of the profile through the whole pipeline, 13.7 M pairs for 4 rows at 10 M reads): it takes
// enough MORE reported targets for the lower bound to pass domE / P-value.  So the profile's unevaluated pairs are ordered by their
// bound (one radix sort), as many of the best as the rows need (+ 2 %) go through the domain pipeline -- count-only, see below -- and the
// thresholds are applied again; what is still undecided then (a row that IS reported, or one whose count lies in the top third of the
// profile's pairs) is counted in full as before.  The upper bound is tightened on the way: reported among the evaluated + pairs not evaluated.  Exact for the same reason the bounds are: a lower bound that passes domE / P-value decides the row whatever the
// exact count is.  Only for a search of one chunk and one sample whose lists are still in the buffers; everything else goes straight on.
// rest (only after a count-only call that took a nearly-needed profile's `need` pairs instead of all of them, ITSX_LAZY_TOPUP_ALL=2): the
// remaining unevaluated pairs of those profiles whose rows are still undecided, count-only again.
static int lazy_topup(itsx_ctx *ctx, double domE, bool *ran, bool rest = false)
{
  (void)domE;
  *ran = false;
  if (!rest) { ctx->topup_deferred_live = 0; ctx->topup_partial.clear(); }
  const auto &tu = ctx->topup;
  if (sw_get("ITSX_LAZY_HIST")) fprintf(stderr, "[itsx] top-up: valid %d chunks %d samples %d pairs %lld\n", (int)tu.valid, ctx->n_chunks, ctx->S, (long long)tu.NP);
  if (!tu.valid || ctx->n_chunks != 1 || ctx->S != 1 || tu.NP <= 0) return ITSX_OK;
  if (sw_get("ITSX_LAZY_TOPUP") && atoi(sw_get("ITSX_LAZY_TOPUP")) == 0) return ITSX_OK;      // (read at every call)
  hipStream_t st = ctx->st;
  const int P = ctx->P;
  itsx_stats &S = ctx->stats;
  // the profiles with undecided rows
  std::vector<int32_t> slot((size_t)P, -1), prof_of;
  for (int p = 0; p < P; p++) {
    if (!ctx->lazy_pending_prof[(size_t)p]) continue;
    if (ctx->h_zneed[(size_t)2 * p] == 0 && ctx->h_zneed[(size_t)2 * p + 1] == ~0ull) continue;
    if (rest && std::find(ctx->topup_partial.begin(), ctx->topup_partial.end(), p) == ctx->topup_partial.end()) continue;
    slot[(size_t)p] = (int32_t)prof_of.size(); prof_of.push_back(p);
  }
  const int ns = (int)prof_of.size();
  if (ns == 0) return ITSX_OK;
  StageTimer tm(st);
  const int64_t NP = tu.NP;
  HIPCHK(upload(ctx->l_slot, slot, st)); HIPCHK(upload(ctx->l_pslot, prof_of, st));
  HIPCHK(upload(ctx->w_idx, tu.seg_start, st)); HIPCHK(upload(ctx->w_rcnt, tu.total, st));
  // the unevaluated pairs of those profiles, compact (a few per cent of the list), then ordered by (profile, bound descending)
  const int64_t nch = (NP + 63) >> 6;                           // (the chunk buffers are lazy_rounds' own: the same list)
  launch_topup_keys(ctx->d_pairs.p, NP, ctx->l_done.p, ctx->l_b10.p, ctx->l_slot.p, ctx->l_smask.p, ctx->l_scnt.p, nullptr, nullptr, nullptr, st);
  launch_exclusive_scan(ctx->l_scnt.p, ctx->l_spos.p, nch + 1, ctx->l_scan.p, st);
  int32_t M32 = 0;
  HIPCHK(hipMemcpyAsync(&M32, ctx->l_spos.p + nch, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t M = M32;
  if (M <= 0) return ITSX_OK;
  HIPCHK(ctx->sh_keys.alloc((size_t)M + 1)); HIPCHK(ctx->sh_keys2.alloc((size_t)M + 1)); HIPCHK(ctx->sh_vals.alloc((size_t)M + 1)); HIPCHK(ctx->sh_uorder.alloc((size_t)M + 1));
  const size_t sort_bytes = order_sort_bytes(M);
  HIPCHK(ctx->sh_sorttmp.alloc(sort_bytes));
  launch_topup_keys(ctx->d_pairs.p, NP, ctx->l_done.p, ctx->l_b10.p, ctx->l_slot.p, ctx->l_smask.p, ctx->l_scnt.p, ctx->l_spos.p, ctx->sh_keys.p, ctx->sh_vals.p, st);
  if (order_sort(ctx->sh_sorttmp.p, sort_bytes, ctx->sh_keys.p, ctx->sh_keys2.p, ctx->sh_vals.p, ctx->sh_uorder.p, M, st) != 0) SET_ERR(ctx, ITSX_E_DEVICE, "top-up round: the radix sort failed");
  HIPCHK(hipStreamSynchronize(st));
  auto lower = [&](unsigned long long key, int64_t &pos) -> int {       // binary search over device memory: ~24 eight-byte copies per probe
    int64_t lo = 0, hi = M;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1; unsigned long long v = 0;
      HIPCHK(hipMemcpy(&v, ctx->sh_keys2.p + mid, 8, hipMemcpyDeviceToHost));
      if (v < key) lo = mid + 1; else hi = mid;
    }
    pos = lo; return ITSX_OK;
  };
  std::vector<uint32_t> cut((size_t)2 * ns, 0);
  bool any = false;
  for (int k = 0; k < ns; k++) {
    const int p = prof_of[(size_t)k];
    int64_t a = 0, b = 0;
    { const int rc = lower((unsigned long long)k << 32, a); if (rc != ITSX_OK) return rc; }
    { const int rc = lower((unsigned long long)(k + 1) << 32, b); if (rc != ITSX_OK) return rc; }
    const int64_t have = b - a;                          // its unevaluated pairs, best bound first in [a, b)
    if (have <= 0) continue;
    const int64_t lo = ctx->domz[(size_t)p], hi = lo + have;       // (the tight upper bound: every unevaluated pair reported)
    int64_t from_top = 0, from_bottom = 0;
    const unsigned long long zl = ctx->h_zneed[(size_t)2 * p], zh = ctx->h_zneed[(size_t)2 * p + 1];
    // rows settled from BELOW: the lower bound must reach zl -- that many more reported targets, taken from the best pairs (+ 2 %: a few are not)
    if (zl > 0 && (int64_t)zl > lo) { const int64_t need = (int64_t)zl - lo; from_top = need + need / 50 + 64; }
    // rows settled from ABOVE: the upper bound must fall to zh -- that many pairs shown unreported, looked for among the weakest (+ 25 %: some are reported)
    // (only with ITSX_LAZY_TOPUP=2: on amplicon data nearly every pair past the filter IS a reported target -- at 10 M reads 387 k of a profile's
    // 394 k weakest pairs were --, so the upper bound hardly moves and such a row goes to the full count anyway)
    const bool both = sw_get("ITSX_LAZY_TOPUP") && atoi(sw_get("ITSX_LAZY_TOPUP")) == 2;
    if (both && zh != ~0ull && hi > (int64_t)zh) { const int64_t need = hi - (int64_t)zh; from_bottom = need + need / 4 + 64; }
    if (sw_get("ITSX_LAZY_HIST")) fprintf(stderr, "[itsx] top-up: profile %d bounds %lld .. %lld (%lld unevaluated), rows need >= %llu / <= %llu: best %lld, weakest %lld\n", p, (long long)lo, (long long)hi,
                                          (long long)have, zl, zh == ~0ull ? 0ull : zh, (long long)from_top, (long long)from_bottom);
    // A profile whose rows need most of its pairs anyway gets ALL of its unevaluated pairs in this round: its bounds meet afterwards (every
    // pair evaluated once, the count exact), and what itsx_lazy_complete would do for it -- the filter again on the profile, every pair of
    // it through the pipeline again, the evaluated ones a second time, in an invocation of its own with its own ensemble batch -- is not
    // needed (10 M reads: top-up 89 + full count 165 ms -> one round of 2xx ms).  ITSX_LAZY_TOPUP_ALL=0: left to the full count as before.
    // ITSX_LAZY_TOPUP_ALL=2 (count-only rounds; read at every call): a round that only counts is cheap enough to come twice, so a row
    // that the lower bound settles takes its `need` best pairs like every other profile's, and the profile's remaining pairs follow in a
    // count-only sub-round of their own only if the row is still undecided then (`rest`).
    static const bool topup_all = !(sw_get("ITSX_LAZY_TOPUP_ALL") && atoi(sw_get("ITSX_LAZY_TOPUP_ALL")) == 0);
    const bool by_need = sw_get("ITSX_LAZY_TOPUP_ALL") && atoi(sw_get("ITSX_LAZY_TOPUP_ALL")) == 2 && !(sw_get("ITSX_TOPUP_COUNT_ONLY") && atoi(sw_get("ITSX_TOPUP_COUNT_ONLY")) == 0);
    const bool above = zh != ~0ull && hi > (int64_t)zh;      // a row that only the upper bound settles: its count lies in the top third of the profile's pairs
    // (by need, such a row is asked from below as well: zh is the SMALLEST Z* past the split, so the lower bound reaching it settles that row at
    // least; the rows with a larger one, if there are any, are what the rest sub-round is for)
    if (by_need && !rest && above && from_bottom == 0 && (int64_t)zh > lo) { const int64_t need = (int64_t)zh - lo; from_top = std::max(from_top, need + need / 50 + 64); }
    const bool partial = by_need && !rest && from_bottom == 0 && from_top > 0 && from_top < have;
    if (rest || (!partial && ((above && !both) || from_top + from_bottom > have - have / 3))) {
      if (!topup_all && !rest) continue;
      cut[(size_t)2 * k] = 1u; cut[(size_t)2 * k + 1] = 0u;      // (every bound is at least 1: k_lazy_bound)
      any = true;
      continue;
    }
    if (partial && (above || from_top > have - have / 3)) ctx->topup_partial.push_back(p);
    unsigned long long v = 0;
    if (from_top > 0) {
      HIPCHK(hipMemcpy(&v, ctx->sh_keys2.p + a + from_top - 1, 8, hipMemcpyDeviceToHost));
      cut[(size_t)2 * k] = std::max<uint32_t>(1u, 0xFFFFFFFFu - (uint32_t)(v & 0xFFFFFFFFull));
    }
    if (from_bottom > 0) {
      HIPCHK(hipMemcpy(&v, ctx->sh_keys2.p + b - from_bottom, 8, hipMemcpyDeviceToHost));
      cut[(size_t)2 * k + 1] = std::max<uint32_t>(1u, 0xFFFFFFFFu - (uint32_t)(v & 0xFFFFFFFFull));
      if (cut[(size_t)2 * k] > 0 && cut[(size_t)2 * k + 1] >= cut[(size_t)2 * k]) { cut[(size_t)2 * k] = cut[(size_t)2 * k + 1] = 0; continue; }   // (the two ends meet: the full count)
    }
    any = any || from_top > 0 || from_bottom > 0;
  }
  if (!any) return ITSX_OK;
  HIPCHK(upload(ctx->l_cut, cut, st));
  launch_topup_mark(ctx->d_pairs.p, NP, ctx->l_done.p, ctx->l_b10.p, ctx->l_slot.p, ctx->l_cut.p, ctx->l_smask.p, ctx->l_scnt.p, st);
  // The round wants ONE number per profile -- how many of these pairs are reported targets -- and no row of theirs can win or tie (they are
  // unevaluated after round 2: below their group's best certain row).  So the pipeline runs count-only (ITSX_TOPUP_COUNT_ONLY=0: as a third
  // lazy round, rows and ensemble stage included): pairs with a multidomain region are deferred, the ensemble stage is not launched.
  const bool count_only = !(sw_get("ITSX_TOPUP_COUNT_ONLY") && atoi(sw_get("ITSX_TOPUP_COUNT_ONLY")) == 0);      // (read at every call)
  PairList sub; int64_t nsel = 0;
  { const int rc = select_compact(ctx, ctx->d_pairs.p, NP, P, tu.seg_start, ctx->w_seg_start.p, sub, nsel, count_only); if (rc != ITSX_OK) return rc; }
  if (sub.NP == 0) return ITSX_OK;
  if (count_only) {
    HIPCHK(ctx->l_dmask.alloc((size_t)nch + 1)); HIPCHK(ctx->l_defn.alloc(2));
    if (!rest) HIPCHK(hipMemsetAsync(ctx->l_dmask.p, 0, ((size_t)nch + 1) * sizeof(unsigned long long), st));      // (rest: the first call's bits stay)
    HIPCHK(hipMemsetAsync(ctx->l_defn.p, 0, 2 * sizeof(unsigned long long), st));      // (counts the pairs whose bit is new)
  }
  const int32_t *d_sorted = (ctx->share_on ? ctx->sh_order.p : ctx->d_sorted_uniq.p) + tu.u0;
  ctx->trace_u0 = tu.u0;
  { StageTimer tp(st); const int rc = domain_pipeline(ctx, sub, d_sorted, ctx->T, ctx->sF1, ctx->sF3, nullptr, count_only); if (rc != ITSX_OK) return rc; S.ms_lazy_topup_stages += tp.stop(); }
  unsigned long long ndef = 0;
  if (count_only) HIPCHK(hipMemcpyAsync(&ndef, ctx->l_defn.p, sizeof(ndef), hipMemcpyDeviceToHost, st));      // (topup_bounds waits for the stream)
  if (!rest) ctx->topup_profs = prof_of;                  // (rest: a subset of them)
  { const int rc = topup_bounds(ctx, count_only); if (rc != ITSX_OK) return rc; }
  // (a deferred pair counts when and if it is evaluated; a rest call selects the first call's deferred pairs of its profiles again -- they
  // are unevaluated -- and defers them again: new bits are the ones it counts)
  if (rest && count_only) {
    unsigned long long again = 0;
    HIPCHK(hipMemcpy(&again, ctx->l_defn.p + 1, sizeof(again), hipMemcpyDeviceToHost));
    nsel -= (int64_t)again;
  }
  nsel -= (int64_t)ndef;
  if (rest) { ctx->n_topup_deferred += (int64_t)ndef; ctx->topup_deferred_live += (int64_t)ndef; }
  else { ctx->n_topup_deferred = (int64_t)ndef; ctx->topup_deferred_live = (int64_t)ndef; }
  S.n_lazy_evaluated += nsel; S.n_lazy_topup += nsel;
  S.n_rows_resident = 0;
  for (int64_t r : ctx->dom_n) S.n_rows_resident += r;
  S.ms_lazy_topup += tm.stop();
  *ran = true;
  return ITSX_OK;
}

// The top-up round's second sub-round: the pairs the count-only round deferred (their bits are in l_dmask), and only they, through the
// ordinary pipeline -- ensemble stage, rows and all.  Taken when a row of the round's profiles is still undecided without them.
static int lazy_topup_deferred(itsx_ctx *ctx)
{
  const auto &tu = ctx->topup;
  hipStream_t st = ctx->st;
  itsx_stats &S = ctx->stats;
  StageTimer tm(st);
  ctx->topup_deferred_live = 0;
  launch_topup_deferred_select(ctx->l_dmask.p, tu.NP, ctx->l_smask.p, ctx->l_scnt.p, ctx->l_done.p, st);
  PairList sub; int64_t nsel = 0;
  { const int rc = select_compact(ctx, ctx->d_pairs.p, tu.NP, ctx->P, tu.seg_start, ctx->w_seg_start.p, sub, nsel); if (rc != ITSX_OK) return rc; }
  if (sub.NP == 0) return ITSX_OK;
  const int32_t *d_sorted = (ctx->share_on ? ctx->sh_order.p : ctx->d_sorted_uniq.p) + tu.u0;
  ctx->trace_u0 = tu.u0;
  { StageTimer tp(st); const int rc = domain_pipeline(ctx, sub, d_sorted, ctx->T, ctx->sF1, ctx->sF3, nullptr); if (rc != ITSX_OK) return rc; S.ms_lazy_topup_stages += tp.stop(); }
  { const int rc = topup_bounds(ctx, false); if (rc != ITSX_OK) return rc; }
  S.n_lazy_evaluated += nsel; S.n_lazy_topup += nsel;
  ctx->n_topup_ensemble = 1;
  S.n_rows_resident = 0;
  for (int64_t r : ctx->dom_n) S.n_rows_resident += r;
  S.ms_lazy_topup += tm.stop();
  return ITSX_OK;
}

int itsx_search_finalize(itsx_ctx *ctx, double domE)
{
  CTXCHK(ctx && ctx->searched());
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->injected && ctx->lazy && !ctx->domz_exchanged)
    SET_ERR(ctx, ITSX_E_ARG, "itsx_search_finalize: a lazy row table that was handed in (itsx_debug_set_domains) has no counters of its own: give both bounds with itsx_set_domz first");
  StageTxn txn(ctx, itsx_ctx::ST_SEARCHED);              // the last finalize's verdicts, row table and alignments go
  StageTimer tm(ctx->st);
  auto check_compaction = [&](const std::vector<int64_t> &z) -> int {       // the rows were thinned out under two assumptions: check them against what finalize was given
    int64_t zmax = 0;
    for (int64_t v : z) zmax = std::max(zmax, v);
    if ((double)zmax > ctx->compact_zmax || domE < ctx->compact_dome_min)
      SET_ERR(ctx, ITSX_E_UNSUPPORTED, "compacted domain rows: only the rows that are reported for every domZ <= " + std::to_string(ctx->compact_zmax) +
              " and every domE >= " + std::to_string(ctx->compact_dome_min) + " were kept, but finalize got domZ up to " + std::to_string(zmax) + " and domE " + std::to_string(domE) +
              " (raise ITSX_COMPACT_ZMAX / lower ITSX_COMPACT_DOME_MIN and search again)");
    return ITSX_OK;
  };
  if (ctx->lazy) {
    { const int rc = finalize_lazy(ctx, domE); if (rc != ITSX_OK) return rc; }
    { const int rc = check_compaction(ctx->domz_ub); if (rc != ITSX_OK) return rc; }
    if (ctx->lazy_pending > 0 && !ctx->domz_exchanged && !sw_get("ITSX_LAZY_NO_RERUN")) {
      // Rows whose reporting depends on the exact domZ could change a result.  This context is on its own (nobody exchanged
      // counters): the profiles of those rows are counted exactly (itsx_lazy_complete) and the thresholds applied again; a
      // multi-rank driver does the same across ranks (itsxpress_amd/dist.py: exchange_and_finalize).
      const int64_t pend = ctx->lazy_pending;
      {   // first the cheap way: enough more of the profiles' best pairs for the lower bounds to decide the rows (lazy_topup)
        bool ran = false;
        { const int rc = lazy_topup(ctx, domE, &ran); if (rc != ITSX_OK) return rc; }
        if (ran) {
          { const int rc = finalize_lazy(ctx, domE); if (rc != ITSX_OK) return rc; }
          ctx->stats.n_lazy_pending = pend;
          // the count-only round deferred pairs and a row of its profiles is still undecided: those pairs, through the ensemble stage
          // (test hook ITSX_TOPUP_FORCE_SECOND: as if the first sub-round had not settled its rows)
          // (ITSX_LAZY_TOPUP_ALL=2: first the remaining pairs of a profile that took only what its row needed and is still undecided)
          bool more = false;
          if (ctx->lazy_pending > 0) for (int32_t p : ctx->topup_partial) more = more || ctx->lazy_pending_prof[(size_t)p] != 0;
          if (more) {
            bool ran2 = false;
            { const int rc = lazy_topup(ctx, domE, &ran2, true); if (rc != ITSX_OK) return rc; }
            if (ran2) { const int rc = finalize_lazy(ctx, domE); if (rc != ITSX_OK) return rc; ctx->stats.n_lazy_pending = pend; }
          }
          bool second = sw_get("ITSX_TOPUP_FORCE_SECOND") && atoi(sw_get("ITSX_TOPUP_FORCE_SECOND")) != 0;
          // (a profile's deferred pairs are worth their ensemble invocation when they could settle every row of it that is still undecided --
          // all of them reported targets for the rows that wait for the lower bound, none of them for the rows that wait for the upper one;
          // a profile they cannot settle is counted in full below, deferred pairs included, whatever this sub-round would have found)
          if (ctx->lazy_pending > 0 && ctx->S == 1)
            for (int32_t p : ctx->topup_profs) {
              const int64_t nd = (size_t)p < ctx->topup_defp.size() ? ctx->topup_defp[(size_t)p] : 0;
              if (!ctx->lazy_pending_prof[(size_t)p] || nd <= 0) continue;
              const unsigned long long zl = ctx->h_zneed[(size_t)2 * p], zh = ctx->h_zneed[(size_t)2 * p + 1];
              if (zl == 0 && zh == ~0ull) continue;
              const int64_t lo = ctx->domz[(size_t)p], hi = std::max(ctx->domz_ub[(size_t)p], lo);
              const bool below = zl == 0 || (int64_t)zl <= lo || (int64_t)zl - lo + 1 <= nd;
              const bool above = zh == ~0ull || hi <= (int64_t)zh || hi - (int64_t)zh + 1 <= nd;
              second = second || (below && above);
            }
          if (second && ctx->topup_deferred_live > 0) {
            { const int rc = lazy_topup_deferred(ctx); if (rc != ITSX_OK) return rc; }
            { const int rc = finalize_lazy(ctx, domE); if (rc != ITSX_OK) return rc; }
            ctx->stats.n_lazy_pending = pend;
          }
          if (ctx->lazy_pending == 0) {
            ctx->stats.ms_finalize = tm.stop();
            txn.commit(itsx_ctx::ST_FINAL);
            return ITSX_OK;
          }
        }
      }
      if (!sw_get("ITSX_LAZY_NO_COMPLETE")) {
        std::vector<int32_t> flags(ctx->lazy_pending_prof);
        flags.resize((size_t)std::max(ctx->P, 1), 0);
        { const int rc = itsx_lazy_complete(ctx, flags.data()); if (rc != ITSX_OK) return rc; }
        { const int rc = finalize_lazy(ctx, domE); if (rc != ITSX_OK) return rc; }
        ctx->stats.n_lazy_pending = pend;
      }
      if (ctx->lazy_pending == 0) {
        ctx->stats.ms_finalize = tm.stop();
        txn.commit(itsx_ctx::ST_FINAL);
        return ITSX_OK;
      }
      // (cannot happen after a completion -- every row of a counted profile is decided --; kept as the safety net: everything in full)
      const int keep = ctx->rows_mode;
      int64_t pend_profiles = 0; for (int32_t f : ctx->lazy_pending_prof) pend_profiles += f != 0;      // (the search forgets them)
      ctx->rows_mode = ITSX_ROWS_COMPACT;
      const int rc = itsx_search(ctx, ctx->T, ctx->sF1, ctx->F2, ctx->sF3);
      ctx->rows_mode = keep;
      if (rc != ITSX_OK) return rc;
      ctx->stats.n_lazy_reruns = 1; ctx->stats.n_lazy_pending = pend; ctx->stats.n_lazy_pending_profiles = pend_profiles;
    } else {
      ctx->stats.ms_finalize = tm.stop();
      txn.commit(itsx_ctx::ST_FINAL);
      return ITSX_OK;
    }
  }
  {
    DBuf<int64_t> &d_dz = ctx->domz_on_device ? ctx->d_domz64 : ctx->w_dz;
    if (ctx->domz_on_device) {             // reduced in place by the caller (RCCL): the host copy follows the device
      if (!ctx->domz.empty()) HIPCHK(hipMemcpyAsync(ctx->domz.data(), d_dz.p, ctx->domz.size() * 8, hipMemcpyDeviceToHost, ctx->st));
    } else HIPCHK(upload(d_dz, ctx->domz, ctx->st));
    for (size_t c = 0; c < ctx->dom_n.size(); c++)
      if (ctx->dom_n[c] > 0) launch_finalize(ctx->dom_bufs[c]->p, ctx->dom_n[c], d_dz.p, domE, ctx->dev_usample(), ctx->P, ctx->st);
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (ctx->compact_rows) { const int rc = check_compaction(ctx->domz); if (rc != ITSX_OK) return rc; }
  }
  ctx->stats.ms_finalize = tm.stop();
  txn.commit(itsx_ctx::ST_FINAL);
  return ITSX_OK;
}

static int fetch_domains(const itsx_ctx *cctx)
{
  itsx_ctx *ctx = const_cast<itsx_ctx *>(cctx);
  if (ctx->compact_rows && !ctx->kept_rows) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "the domain rows of this search were compacted (ITSX_COMPACT_ROWS=1): only coordinates are available, not the row table / domtbl.txt (itsx_set_kept_rows(ctx, 1) serves the rows that were kept)");
  if (ctx->compact_rows && !ctx->finalized()) SET_ERR(ctx, ITSX_E_ARG, "the kept rows of a compact / lazy search are served after itsx_search_finalize");
  if (ctx->lazy && ctx->lazy_pending > 0) SET_ERR(ctx, ITSX_E_ARG, "the kept rows of a lazy search are served once no row is undecided (itsx_lazy_pending)");
  if (!ctx->h_dom.empty()) return ITSX_OK;
  // domtblout order: profile, then target, then domain.  The device rows are grouped by profile already (not contiguously
  // across chunks), so: counting sort by profile, then every profile's rows are ordered on their own by a pool of threads.
  const int P = std::max(ctx->P, 1);
  std::vector<itsx_domain> all;
  std::vector<int64_t> start((size_t)P + 1, 0);
  for (size_t c = 0; c < ctx->dom_n.size(); c++) {
    if (ctx->dom_n[c] <= 0) continue;
    const size_t o = all.size();
    all.resize(o + (size_t)ctx->dom_n[c]);
    HIPCHK(hipMemcpy(all.data() + o, ctx->dom_bufs[c]->p, (size_t)ctx->dom_n[c] * sizeof(itsx_domain), hipMemcpyDeviceToHost));
  }
  for (const auto &d : all) if (d.dom_idx >= 0 && d.prof >= 0 && d.prof < P) start[(size_t)d.prof + 1]++;
  for (int p = 0; p < P; p++) start[(size_t)p + 1] += start[(size_t)p];
  ctx->h_dom.resize((size_t)start[(size_t)P]);
  {
    std::vector<int64_t> cur(start.begin(), start.end() - 1);
    for (const auto &d : all) if (d.dom_idx >= 0 && d.prof >= 0 && d.prof < P) ctx->h_dom[(size_t)cur[(size_t)d.prof]++] = d;
  }
  std::vector<itsx_domain>().swap(all);
  std::atomic<int> next{0};
  on_threads(std::min(itsx_io::io_threads(), P), [&](int) {
    for (int p = next.fetch_add(1); p < P; p = next.fetch_add(1))
      std::sort(ctx->h_dom.begin() + start[(size_t)p], ctx->h_dom.begin() + start[(size_t)p + 1], [](const itsx_domain &a, const itsx_domain &b) {
        if (a.rep != b.rep) return a.rep < b.rep;
        return a.dom_idx < b.dom_idx;
      });
  });
  if (ctx->compact_rows) {
    // kept rows (itsx_set_kept_rows): a pair the lazy stage evaluated twice -- a top-up or completion round after round 1 / 2 -- left
    // its rows twice, bit for bit the same; the table names every (profile, target, domain) once.  A row that is still undecided
    // (dom_reported == 2: reported under the lower bound on domZ only) is one that cannot win -- it ranks below its group's best sure
    // row, or it would have been settled (k_lazy_pending) -- and is left out like every other row that cannot
    // ... and of the decided rows the table lists the WINNERS: per target and 2-character prefix the reported row with the largest rank
    // key, the one ItsPosition.parse ends up with.  (What else is resident -- a round-1 row that a round-2 row outranked, a row that
    // was best until a later batch -- depends on the order the batches ran in; the winners do not.)
    std::vector<int8_t> cls((size_t)P, 0); std::vector<std::string> seen;
    for (int p = 0; p < ctx->P; p++) {
      const std::string pre = ctx->profs[(size_t)p].name.substr(0, 2);
      size_t k = 0; while (k < seen.size() && seen[k] != pre) k++;
      if (k == seen.size()) seen.push_back(pre);
      cls[(size_t)p] = (int8_t)k;
    }
    const size_t ncls = std::max<size_t>(seen.size(), 1);
    std::vector<unsigned long long> best((size_t)std::max(ctx->U, 1) * ncls, 0ull);
    for (const auto &d : ctx->h_dom)
      if (d.dom_reported == 1) { unsigned long long &b = best[(size_t)d.rep * ncls + (size_t)cls[(size_t)d.prof]]; b = std::max(b, rank_key(d)); }
    size_t w = 0;
    for (size_t r = 0; r < ctx->h_dom.size(); r++) {
      const itsx_domain &d = ctx->h_dom[r];
      if (d.dom_reported != 1 || rank_key(d) != best[(size_t)d.rep * ncls + (size_t)cls[(size_t)d.prof]]) continue;
      if (w > 0 && ctx->h_dom[w - 1].prof == d.prof && ctx->h_dom[w - 1].rep == d.rep && ctx->h_dom[w - 1].dom_idx == d.dom_idx) continue;
      if (w != r) ctx->h_dom[w] = d;
      w++;
    }
    ctx->h_dom.resize(w);
  }
  return ITSX_OK;
}

int64_t itsx_num_domains(const itsx_ctx *ctx)
{
  if (!ctx || !ctx->searched()) return -1;
  if (fetch_domains(ctx) != ITSX_OK) return -1;
  return (int64_t)ctx->h_dom.size();
}
int itsx_get_domains(const itsx_ctx *ctx, itsx_domain *rows)
{
  CTXCHK(ctx && rows && ctx->searched());
  const int rc = fetch_domains(ctx);
  if (rc != ITSX_OK) return rc;
  if (!ctx->h_dom.empty()) memcpy(rows, ctx->h_dom.data(), ctx->h_dom.size() * sizeof(itsx_domain));
  return ITSX_OK;
}

// ---- the optimal-accuracy alignments of the reported rows (opt-in: nothing of the search is touched)
// out[k] = the alignment of ctx->h_dom[k], looked up by (profile, representative, domain); all zero where there is none
static void alignments_of_rows(const itsx_ctx *ctx, itsx_alignment *out)
{
  const auto &A = ctx->h_ali;
  for (size_t k = 0; k < ctx->h_dom.size(); k++) {
    const itsx_domain &d = ctx->h_dom[k];
    itsx_alignment a{};
    if (d.dom_reported == 1) {
      size_t lo = 0, hi = A.size();
      while (lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        const itsx_ctx::AliRow &r = A[mid];
        const bool less = r.prof != d.prof ? r.prof < d.prof : r.rep != d.rep ? r.rep < d.rep : r.dom_idx < d.dom_idx;
        if (less) lo = mid + 1; else hi = mid;
      }
      if (lo < A.size() && A[lo].prof == d.prof && A[lo].rep == d.rep && A[lo].dom_idx == d.dom_idx) a = A[lo].a;
    }
    out[k] = a;
  }
}

int itsx_align_domains(itsx_ctx *ctx, int64_t *n_aligned, float *ms_kernels)
{
  CTXCHK(ctx);
  if (!ctx->finalized()) SET_ERR(ctx, ITSX_E_ARG, "itsx_align_domains is called after itsx_search_finalize");
  { const int rc = fetch_domains(ctx); if (rc != ITSX_OK) return rc; }       // (refuses where the row table is refused)
  HIPCHK(hipSetDevice(ctx->device));
  ctx->drop_alignments();
  hipStream_t st = ctx->st;
  const int P = ctx->P;
  // the work list: every resident row with dom_reported == 1, grouped by profile (the unrolled kernels' profiles first), ascending
  // envelope length.  A row carries all the stage needs; it is checked against the read set before anything indexes with it.
  std::vector<int32_t> rlen;
  if ((int64_t)ctx->h_len.size() == ctx->N) rlen = ctx->h_len;
  else { rlen.resize((size_t)ctx->N); if (ctx->N > 0) HIPCHK(hipMemcpy(rlen.data(), ctx->d_len.p, (size_t)ctx->N * 4, hipMemcpyDeviceToHost)); }
  std::vector<itsx_ctx::AliRow> items;
  std::vector<int32_t> iL, iLd;
  {
    std::vector<itsx_domain> seg;
    for (size_t c = 0; c < ctx->dom_n.size(); c++) {
      if (ctx->dom_n[c] <= 0) continue;
      seg.resize((size_t)ctx->dom_n[c]);
      HIPCHK(hipMemcpy(seg.data(), ctx->dom_bufs[c]->p, seg.size() * sizeof(itsx_domain), hipMemcpyDeviceToHost));
      for (size_t r = 0; r < seg.size(); r++) {
        const itsx_domain &d = seg[r];
        if (d.dom_idx < 0 || d.dom_reported != 1) continue;
        const bool ok = d.prof >= 0 && d.prof < P && d.rep >= 0 && d.rep < ctx->U && d.ienv >= 1 && d.jenv >= d.ienv && d.jenv <= d.tlen &&
                        ctx->h_seed_read[(size_t)d.rep] >= 0 && ctx->h_seed_read[(size_t)d.rep] < ctx->N && d.tlen == rlen[(size_t)ctx->h_seed_read[(size_t)d.rep]];
        if (!ok) SET_ERR(ctx, ITSX_E_ARG, "itsx_align_domains: row " + std::to_string(r) + " of segment " + std::to_string(c) + " does not name an envelope of a loaded read (profile " +
                         std::to_string(d.prof) + ", representative " + std::to_string(d.rep) + ", envelope " + std::to_string(d.ienv) + ".." + std::to_string(d.jenv) + " of " + std::to_string(d.tlen) + ")");
        itsx_ctx::AliRow it{}; it.prof = d.prof; it.dom_idx = d.dom_idx; it.rep = d.rep;
        it.a.ali_from = d.ienv; it.a.ali_to = d.jenv; it.a.hmm_from = d.tlen;             // (carried to the device lists below)
        items.push_back(it);
      }
    }
  }
  const int64_t NI = (int64_t)items.size();
  float ms = 0.0f;
  if (NI > 0) {
    std::sort(items.begin(), items.end(), [&](const itsx_ctx::AliRow &x, const itsx_ctx::AliRow &y) {
      const int gx = ctx->generic_q[(size_t)x.prof], gy = ctx->generic_q[(size_t)y.prof];
      if (gx != gy) return gx < gy;
      if (x.prof != y.prof) return x.prof < y.prof;
      const int lx = x.a.ali_to - x.a.ali_from, ly = y.a.ali_to - y.a.ali_from;
      if (lx != ly) return lx < ly;
      if (x.rep != y.rep) return x.rep < y.rep;
      return x.dom_idx < y.dom_idx;
    });
    std::vector<PairRec> pairs((size_t)NI); std::vector<RegionRec> regions((size_t)NI); std::vector<int32_t> reps((size_t)NI);
    for (int64_t k = 0; k < NI; k++) {
      const itsx_ctx::AliRow &it = items[(size_t)k];
      pairs[(size_t)k] = PairRec{(int32_t)k, it.prof, 0, it.a.hmm_from};
      regions[(size_t)k] = RegionRec{(int32_t)k, it.a.ali_from, it.a.ali_to, 0};
      reps[(size_t)k] = (int32_t)it.rep;
    }
    std::vector<WaveDesc> waves; std::vector<char> wgen;
    for (int64_t k = 0; k < NI;) {
      int64_t e = k + 1;
      while (e < NI && e - k < 64 && items[(size_t)e].prof == items[(size_t)k].prof) e++;
      WaveDesc w{}; w.prof = items[(size_t)k].prof; w.first = k; w.count = (int32_t)(e - k);
      w.rows = regions[(size_t)e - 1].jenv - regions[(size_t)e - 1].ienv + 2;              // the wave's longest envelope + 1
      waves.push_back(w); wgen.push_back(ctx->generic_q[(size_t)w.prof]);
      k = e;
    }
    const int NW = (int)waves.size();
    HIPCHK(upload(ctx->w_al_pairs, pairs, st)); HIPCHK(upload(ctx->w_al_regions, regions, st)); HIPCHK(upload(ctx->w_al_rep, reps, st));
    HIPCHK(ctx->w_al_rout.alloc((size_t)NI)); HIPCHK(ctx->w_al_out.alloc((size_t)NI)); HIPCHK(ctx->w_al_waves.alloc((size_t)NW));
    HIPCHK(hipMemsetAsync(ctx->w_al_rout.p, 0, (size_t)NI * sizeof(RegionOut), st));
    HIPCHK(hipMemsetAsync(ctx->w_al_out.p, 0, (size_t)NI * sizeof(itsx_alignment), st));
    // the slab is sized from the envelopes of a batch of waves, under a budget: as many batches as it takes, one wave at the least
    const int64_t row_floats = 104 * 64;
    double mb = 4096.0;
    if (const char *e = sw_get("ITSX_ALIGN_SLAB_MB")) { const double v = atof(e); if (v > 0.0) mb = v; }
    const int64_t budget = std::max<int64_t>((int64_t)(mb * 1048576.0) / (row_floats * 4), 1);
    DBuf<float> &d_eslab = ctx->w_eslab;
    LazyTimers lt(st);
    int w0 = 0;
    while (w0 < NW) {
      int w1 = w0; int64_t r = 0;
      while (w1 < NW && wgen[(size_t)w1] == wgen[(size_t)w0] && (w1 == w0 || r + waves[(size_t)w1].rows <= budget)) { waves[(size_t)w1].slab = r; r += waves[(size_t)w1].rows; w1++; }
      if ((int64_t)(d_eslab.cap / (size_t)row_floats) < r && d_eslab.alloc((size_t)(r * row_floats)) != hipSuccess) {
        (void)hipGetLastError();
        SET_ERR(ctx, ITSX_E_NOMEM, "itsx_align_domains: no device memory for a slab of " + std::to_string(r) + " rows (lower ITSX_ALIGN_SLAB_MB)");
      }
      HIPCHK(hipMemcpyAsync(ctx->w_al_waves.p + w0, waves.data() + w0, (size_t)(w1 - w0) * sizeof(WaveDesc), hipMemcpyHostToDevice, st));
      EnvArgs a{};
      a.rd = ctx->rd; a.sorted_uniq = ctx->w_al_rep.p; a.seed_read = ctx->d_seed_read.p; a.prof = ctx->d_prof.p; a.lt = ctx->d_lt.p;
      a.pairs = ctx->w_al_pairs.p; a.regions = ctx->w_al_regions.p; a.rout = ctx->w_al_rout.p; a.waves = ctx->w_al_waves.p; a.slab = d_eslab.p;
      { const size_t t = lt.begin(&ms); launch_align(a, ctx->w_al_out.p, w1 - w0, w0, wgen[(size_t)w0], st); lt.end(t); }
      HIPCHK(hipStreamSynchronize(st));            // (the next batch's wave list and slab are the same buffers)
      w0 = w1;
    }
    lt.collect();
    std::vector<itsx_alignment> res((size_t)NI);
    HIPCHK(hipMemcpy(res.data(), ctx->w_al_out.p, (size_t)NI * sizeof(itsx_alignment), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < NI; k++) {
      itsx_ctx::AliRow &it = items[(size_t)k];
      const itsx_alignment &o = res[(size_t)k];
      const bool sane = o.aligned == 1 && o.hmm_from >= 1 && o.hmm_from <= o.hmm_to && o.hmm_to <= ctx->profs[(size_t)it.prof].M &&
                        o.ali_from >= it.a.ali_from && o.ali_from <= o.ali_to && o.ali_to <= it.a.ali_to && std::isfinite(o.oasc);
      if (!sane) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "itsx_align_domains: the posteriors of an envelope are unusable: profile " + ctx->profs[(size_t)it.prof].name + ", representative " +
                         std::to_string(it.rep) + ", domain " + std::to_string(it.dom_idx) + ", envelope " + std::to_string(it.a.ali_from) + ".." + std::to_string(it.a.ali_to));
      it.a = o;
    }
    std::sort(items.begin(), items.end(), [](const itsx_ctx::AliRow &x, const itsx_ctx::AliRow &y) {
      if (x.prof != y.prof) return x.prof < y.prof;
      if (x.rep != y.rep) return x.rep < y.rep;
      return x.dom_idx < y.dom_idx;
    });
  }
  ctx->h_ali.swap(items);
  ctx->have_ali = true;
  if (n_aligned) *n_aligned = NI;
  if (ms_kernels) *ms_kernels = ms;
  return ITSX_OK;
}

int itsx_get_alignments(const itsx_ctx *ctx, itsx_alignment *out)
{
  CTXCHK(ctx && out);
  if (!ctx->alignments_live()) SET_ERR(ctx, ITSX_E_ARG, "itsx_get_alignments: no alignments for the current finalize (itsx_align_domains comes after itsx_search_finalize)");
  { const int rc = fetch_domains(ctx); if (rc != ITSX_OK) return rc; }
  alignments_of_rows(ctx, out);
  return ITSX_OK;
}

// copy the current chunk's pair records into the host trace list
static int append_traces(itsx_ctx *ctx)
{
  const int64_t NP = ctx->npairs_padded;
  if (NP == 0) return ITSX_OK;
  std::vector<PairRec> pr((size_t)NP); std::vector<PairOut> po((size_t)NP); std::vector<VitOut> vo;
  HIPCHK(hipMemcpy(pr.data(), ctx->d_pairs.p, (size_t)NP * sizeof(PairRec), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(po.data(), ctx->d_pout.p, (size_t)NP * sizeof(PairOut), hipMemcpyDeviceToHost));
  if (ctx->have_vit) { vo.resize((size_t)NP); HIPCHK(hipMemcpy(vo.data(), ctx->d_vit.p, (size_t)NP * sizeof(VitOut), hipMemcpyDeviceToHost)); }
  // PairRec::useq is a position in the list the search walked: with prefix sharing the processing order (k_share.hip), else by length
  // (a sample-sharing search walked the holders only, and the context walks all its uniques again by the time a one-chunk search's
  // traces are fetched: the list and the length are the SEARCHED ones)
  const std::vector<int32_t> &searched = ctx->searched_holders ? ctx->h_sorted_searched : ctx->h_sorted_active;
  std::vector<int32_t> order;
  if (ctx->share_on) {
    order.resize(searched.size());
    if (!order.empty()) HIPCHK(hipMemcpy(order.data(), ctx->sh_order.p, order.size() * 4, hipMemcpyDeviceToHost));
  }
  const int32_t *walked = ctx->share_on ? order.data() : searched.data();
  for (int64_t i = 0; i < NP; i++) {
    if (pr[i].prof < 0 || pr[i].xj < 0) continue;          // (padding; a pair that ran only for a chain below it)
    itsx_pairtrace t{};
    t.rep = walked[(size_t)ctx->trace_u0 + pr[i].useq]; t.prof = pr[i].prof; t.msv_xj = pr[i].xj; t.pass_msv = 1;
    t.pass_bias = po[i].pass_bias; t.pass_fwd = po[i].pass_fwd; t.msv_sc = po[i].msv_sc; t.filtersc = po[i].filtersc;
    t.fwdsc = po[i].fwdsc; t.bcksc = po[i].bcksc; t.nullsc = po[i].nullsc; t.nregions = po[i].nregions; t.ndom = po[i].ndom;
    const bool ran = ctx->have_vit && po[i].pass_bias && vo[(size_t)i].ran;
    t.ran_vit = ran; t.vitsc = ran ? vo[(size_t)i].vitsc : 0.0f; t.pass_vit = po[i].pass_bias && (!ran || vo[(size_t)i].pass);
    ctx->h_trace.push_back(t);
  }
  return ITSX_OK;
}
// traces are fetched lazily when the search ran as one chunk; multi-chunk runs keep them only with ITSX_KEEP_TRACE=1
static int fetch_traces(const itsx_ctx *cctx)
{
  itsx_ctx *ctx = const_cast<itsx_ctx *>(cctx);
  if (ctx->h_trace.empty() && !ctx->keep_trace) {
    if (ctx->n_chunks > 1) SET_ERR(ctx, ITSX_E_ARG, "pair traces of a multi-chunk search are kept only when ITSX_KEEP_TRACE=1");
    const int rc = append_traces(ctx);
    if (rc != ITSX_OK) return rc;
  }
  if (ctx->searched_holders && !ctx->trace_members_done) {
    // sample sharing: the pairs of a holder are the pairs of every member of its class (same residues, same filters, same scores):
    // each member gets its holder's traces with `rep` rewritten, so the table is the one a search without the mode leaves
    const size_t C = (size_t)ctx->sc.n_classes, U = (size_t)ctx->U;
    std::vector<int32_t> cls(U), off(C + 1), mem(U);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpy(cls.data(), ctx->sc_class_of.p, U * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(off.data(), ctx->sc_off.p, (C + 1) * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mem.data(), ctx->sc_members.p, U * 4, hipMemcpyDeviceToHost));
    const size_t n0 = ctx->h_trace.size();
    for (size_t i = 0; i < n0; i++) {
      const size_t c = (size_t)cls[(size_t)ctx->h_trace[i].rep];
      for (int32_t k = off[c] + 1; k < off[c + 1]; k++) { itsx_pairtrace t = ctx->h_trace[i]; t.rep = mem[(size_t)k]; ctx->h_trace.push_back(t); }
    }
    ctx->trace_members_done = true; ctx->trace_sorted = false;
  }
  if (!ctx->trace_sorted) {
    std::sort(ctx->h_trace.begin(), ctx->h_trace.end(), [](const itsx_pairtrace &a, const itsx_pairtrace &b) {
      if (a.prof != b.prof) return a.prof < b.prof;
      return a.rep < b.rep;
    });
    ctx->trace_sorted = true;
  }
  return ITSX_OK;
}
int64_t itsx_num_pairtraces(const itsx_ctx *ctx)
{
  if (!ctx || !ctx->searched()) return -1;
  if (fetch_traces(ctx) != ITSX_OK) return -1;
  return (int64_t)ctx->h_trace.size();
}
int itsx_get_pairtraces(const itsx_ctx *ctx, itsx_pairtrace *rows, int64_t row_size)
{
  if (ctx && row_size != (int64_t)sizeof(itsx_pairtrace)) SET_ERR(ctx, ITSX_E_ARG, "itsx_get_pairtraces: the caller's rows have " + std::to_string(row_size) + " bytes, this library's " + std::to_string(sizeof(itsx_pairtrace)));
  CTXCHK(ctx && rows && ctx->searched());
  const int rc = fetch_traces(ctx);
  if (rc != ITSX_OK) return rc;
  if (!ctx->h_trace.empty()) memcpy(rows, ctx->h_trace.data(), ctx->h_trace.size() * sizeof(itsx_pairtrace));
  return ITSX_OK;
}



// ------------------------------------------------------------------------------ f4: read orientation
int itsx_orient_load_db(itsx_ctx *ctx, const char *fasta_path, int64_t *n_sequences)
{
  CTXCHK(ctx && fasta_path);
  HIPCHK(hipSetDevice(ctx->device));
  init_codes();
  std::string rerr;
  const auto tp = slurp(fasta_path, false, rerr);
  if (!tp) SET_ERR(ctx, ITSX_E_IO, rerr);
  const itsx_io::Text &text = *tp;
  std::vector<uint32_t> bits(1u << 19, 0u);                 // 4^12 bits
  int64_t nseq = 0;
  const bool use_dust = qmask_dust();                        // vsearch --dbmask dust (its default): masked words are not indexed
  std::vector<uint8_t> seq, msk;
  auto add_seq = [&]() {
    if (seq.empty()) return;
    if (use_dust) dust_host(seq.data(), (int64_t)seq.size(), msk);
    uint32_t w = 0; int good = 0;
    for (size_t i = 0; i < seq.size(); i++) {
      const int code = seq[i];
      if (code <= 3 && !(use_dust && msk[i])) { w = (w >> 2) | ((uint32_t)code << 22); good++; } else { w = 0; good = 0; }
      if (good >= 12) bits[w >> 5] |= 1u << (w & 31);
    }
    seq.clear();
  };
  bool header = false;
  for (size_t i = 0; i < text.size(); i++) {
    const char c = text[i];
    // a record starts at a '>' that begins a line: one inside a header is the header's, one inside a sequence line breaks words as N does
    if (c == '>' && !header && (i == 0 || text[i - 1] == '\n')) { add_seq(); header = true; nseq++; continue; }
    if (c == '\n') { header = false; continue; }
    if (header || c == '\r') continue;
    const int code = g_code[(unsigned char)c];
    seq.push_back((uint8_t)((code >= 0 && code <= 15) ? code : 15));
  }
  add_seq();
  if (nseq == 0) SET_ERR(ctx, ITSX_E_FORMAT, std::string("no FASTA records in ") + fasta_path);
  HIPCHK(upload(ctx->d_orient_db, bits, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  ctx->have_orient_db = true;
  if (n_sequences) *n_sequences = nseq;
  return ITSX_OK;
}

// strand and both counts of every read of the context, left in device memory (enqueued on ctx->st).  Reads of at most 12 011 bases are
// k_orient's; it leaves the longer ones at 0 / 0, and those -- a work list of their indices -- go through k_orient_long (k_orient.hip),
// whose word sets live in w_orient_tab: zeroed when the buffer is new, left empty by the kernel
static int orient_enqueue(itsx_ctx *ctx, DBuf<int8_t> &d_s, DBuf<int32_t> &d_f, DBuf<int32_t> &d_r, DBuf<uint32_t> &dmask)
{
  const int64_t n = ctx->N;
  HIPCHK(d_s.alloc((size_t)n)); HIPCHK(d_f.alloc((size_t)n)); HIPCHK(d_r.alloc((size_t)n));
  const bool use_dust = qmask_dust();                        // vsearch --qmask dust (its default)
  if (use_dust) { HIPCHK(dmask.alloc((size_t)ctx->h_woff[n] + 1)); launch_dust(ctx->rd, dmask.p, ctx->st); }
  launch_orient(ctx->rd, ctx->d_orient_db.p, use_dust ? dmask.p : nullptr, d_s.p, d_f.p, d_r.p, ctx->st);
  if (ctx->Lmax - 11 > 12000) {
    std::vector<int32_t> &longs = ctx->h_orient_longs;      // (the context's: alive until the copy that upload() enqueues has run)
    longs.clear();
    for (int64_t r = 0; r < n; r++) if (ctx->h_len[(size_t)r] - 11 > 12000) longs.push_back((int32_t)r);
    HIPCHK(upload(ctx->w_orient_list, longs, ctx->st));
    const size_t tw = (size_t)orient_long_table_words((int64_t)longs.size());
    const bool fresh = !ctx->w_orient_tab.p || ctx->w_orient_tab.cap < tw;
    HIPCHK(ctx->w_orient_tab.alloc(tw));
    if (fresh) HIPCHK(hipMemsetAsync(ctx->w_orient_tab.p, 0, ctx->w_orient_tab.cap * sizeof(uint32_t), ctx->st));
    launch_orient_long(ctx->rd, ctx->w_orient_list.p, (int64_t)longs.size(), ctx->d_orient_db.p, use_dust ? dmask.p : nullptr, ctx->w_orient_tab.p,
                       d_s.p, d_f.p, d_r.p, ctx->st);
  }
  HIPCHK(hipGetLastError());
  return ITSX_OK;
}

// ... and fetched: strand (and the counts, where wanted) on the host when this returns.  The long reads' word sets are empty between
// calls only if k_orient_long ran to its end: after any failure they are given up, and the next call starts from a zeroed buffer
static int orient_device(itsx_ctx *ctx, int8_t *strand, int32_t *count_fwd, int32_t *count_rev, DBuf<int8_t> &d_s)
{
  const int64_t n = ctx->N;
  DBuf<int32_t> d_f, d_r; DBuf<uint32_t> dmask;
  const int rc = [&]() -> int {
    { const int rc1 = orient_enqueue(ctx, d_s, d_f, d_r, dmask); if (rc1 != ITSX_OK) return rc1; }
    HIPCHK(hipMemcpyAsync(strand, d_s.p, (size_t)n, hipMemcpyDeviceToHost, ctx->st));
    if (count_fwd) HIPCHK(hipMemcpyAsync(count_fwd, d_f.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->st));
    if (count_rev) HIPCHK(hipMemcpyAsync(count_rev, d_r.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    return ITSX_OK;
  }();
  if (rc != ITSX_OK) ctx->w_orient_tab.release();
  return rc;
}

int itsx_orient(itsx_ctx *ctx, int8_t *strand, int32_t *count_fwd, int32_t *count_rev)
{
  CTXCHK(ctx && strand);
  if (!ctx->have_orient_db) SET_ERR(ctx, ITSX_E_ARG, "itsx_orient called before itsx_orient_load_db");
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->N;
  if (n == 0) return ITSX_OK;
  DBuf<int8_t> d_s;
  return orient_device(ctx, strand, count_fwd, count_rev, d_s);
}

extern "C++" { template <class T> static void dbuf_swap(DBuf<T> &a, DBuf<T> &b) { std::swap(a.p, b.p); std::swap(a.n, b.n); std::swap(a.cap, b.cap); } }
static int host_bases(const itsx_ctx *cctx);

// The context's reads oriented and replaced, where they are, by the reads vsearch --orient --fastqout keeps: the state
// itsx_load_reads_files leaves after loading the samples' oriented.fq files.  The device side is a plan (what each kept read's words and
// exceptions are and where they go) and a scatter into fresh buffers (k_orient.hip); the host needs the strand vector alone and compacts
// its labels, offsets and text -- the reverse reads' text reverse-complemented with the table the oriented FASTQ writer uses -- while
// those kernels run.  Everything is built beside the read set and swapped in at the end: whatever fails, the context keeps what it had.
static int orient_apply_strands(itsx_ctx *ctx, const std::vector<int8_t> &hs, DBuf<int8_t> &d_s, int64_t *n_kept_per_sample);
int itsx_orient_apply(itsx_ctx *ctx, int8_t *strand, int32_t *count_fwd, int32_t *count_rev, int64_t *n_kept_per_sample)
{
  CTXCHK(ctx);
  if (!ctx->have_orient_db) SET_ERR(ctx, ITSX_E_ARG, "itsx_orient_apply called before itsx_orient_load_db");
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->N;
  if (!ctx->bases_view) { const int rc = host_bases(ctx); if (rc != ITSX_OK) return rc; }      // reads handed over in device memory: their text comes back first
  std::vector<int8_t> hs((size_t)n + 1, 0);
  DBuf<int8_t> d_s;
  if (n > 0) { const int rc = orient_device(ctx, hs.data(), count_fwd, count_rev, d_s); if (rc != ITSX_OK) return rc; }
  { const int rc = orient_apply_strands(ctx, hs, d_s, n_kept_per_sample); if (rc != ITSX_OK) return rc; }
  if (strand && n > 0) memcpy(strand, hs.data(), (size_t)n);
  return ITSX_OK;
}
// ... given the strands (hs on the host, d_s on the device: +1 kept, -1 kept reverse-complemented, 0 dropped; the host's text present):
// itsx_orient_apply's, and itsx_orient_profiles_apply's, which drops nothing
static int orient_apply_strands(itsx_ctx *ctx, const std::vector<int8_t> &hs, DBuf<int8_t> &d_s, int64_t *n_kept_per_sample)
{
  const int64_t n = ctx->N;
  const int32_t S = ctx->S;
  hipStream_t st = ctx->st;
  // ---- what the host knows from the strands: the kept reads, their offsets, their words
  int64_t m = 0;
  for (int64_t r = 0; r < n; r++) m += hs[(size_t)r] != 0;
  std::vector<int64_t> off((size_t)m + 1, 0), woff((size_t)m + 1, 0); std::vector<int32_t> len((size_t)m), smp, from((size_t)m);
  std::vector<int64_t> scnt((size_t)S, 0);
  if (S > 1) smp.resize((size_t)m);
  int Lmax = 0;
  {
    int64_t j = 0;
    for (int64_t r = 0; r < n; r++) {
      if (!hs[(size_t)r]) continue;
      const int32_t L = ctx->h_len[(size_t)r];
      from[(size_t)j] = (int32_t)r; len[(size_t)j] = L; Lmax = std::max(Lmax, (int)L);
      off[(size_t)j + 1] = off[(size_t)j] + L;
      woff[(size_t)j + 1] = woff[(size_t)j] + (ctx->h_woff[(size_t)r + 1] - ctx->h_woff[(size_t)r]);
      if (S > 1) { smp[(size_t)j] = ctx->h_sample[(size_t)r]; scnt[(size_t)smp[(size_t)j]]++; }
      j++;
    }
    if (S == 1) scnt[0] = m;
  }
  // ---- the device side, enqueued: plan and scatter into fresh buffers
  DBuf<uint32_t> n_words, n_exc; DBuf<int64_t> n_woff, n_excoff, d_blk, d_tot, d_scnt; DBuf<int32_t> n_len, n_sample, d_src;
  HIPCHK(n_words.alloc((size_t)woff[(size_t)m] + 1)); HIPCHK(n_exc.alloc(std::max<size_t>(ctx->d_exc.n, 1)));
  HIPCHK(n_woff.alloc((size_t)m + 1)); HIPCHK(n_excoff.alloc((size_t)m + 1)); HIPCHK(n_len.alloc((size_t)m + 1));
  if (S > 1) HIPCHK(n_sample.alloc((size_t)m + 1));
  int64_t tot[3] = {0, 0, 0};
  std::vector<int64_t> dcnt((size_t)S, 0);
  if (n > 0) {
    const int64_t nb = orient_apply_blocks(n);
    HIPCHK(d_blk.alloc((size_t)nb * 3)); HIPCHK(d_tot.alloc(3)); HIPCHK(d_src.alloc((size_t)m + 1));
    OrientApplyArgs a{};
    a.rd = ctx->rd; a.strand = d_s.p; a.blk = d_blk.p; a.total = d_tot.p; a.src = d_src.p;
    a.woff = n_woff.p; a.excoff = n_excoff.p; a.len = n_len.p; a.words = n_words.p; a.exc = n_exc.p;
    if (S > 1) {
      HIPCHK(d_scnt.alloc((size_t)S)); HIPCHK(hipMemsetAsync(d_scnt.p, 0, (size_t)S * 8, st));
      a.sample = ctx->d_sample.p; a.osample = n_sample.p; a.sample_count = d_scnt.p;
    }
    launch_orient_apply_plan(a, st);
    launch_orient_apply_scatter(a, m, st);
    HIPCHK(hipGetLastError());
  } else { HIPCHK(hipMemsetAsync(n_woff.p, 0, 8, st)); HIPCHK(hipMemsetAsync(n_excoff.p, 0, 8, st)); }
  // ---- the records of the kept reads (itsx_keep_records), beside the old ones like everything else: what itsx_write_oriented_fastq writes
  const bool records = ctx->rec.have;
  DBuf<uint8_t> r_seq, r_qual, r_titles, d_comp; DBuf<int64_t> r_off, r_toff; NameList r_names;
  if (records) {
    HIPCHK(r_seq.alloc((size_t)off[(size_t)m] + 64)); HIPCHK(r_qual.alloc((size_t)off[(size_t)m] + 64)); HIPCHK(r_off.alloc((size_t)m + 1)); HIPCHK(r_toff.alloc((size_t)m + 1));
    HIPCHK(d_comp.alloc(256));
    HIPCHK(hipMemcpyAsync(d_comp.p, itsx::iupac_complement(), 256, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r_off.p, off.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, st));
    if (m > 0) launch_trim_orient(ctx->rec.seq_p, ctx->rec.qual.p, ctx->rec.off.p, d_src.p, d_s.p, d_comp.p, r_off.p, m, r_seq.p, r_qual.p, st);
    const NameList &ot = ctx->rec.h_titles;
    r_names.off.resize((size_t)m + 1);
    int64_t nbytes = 0;
    for (int64_t j = 0; j < m; j++) { r_names.off[(size_t)j] = nbytes; nbytes += (int64_t)ot.len((size_t)from[(size_t)j]); }
    r_names.off[(size_t)m] = nbytes;
    r_names.blob.resize((size_t)nbytes);
    for (int64_t j = 0; j < m; j++) { const size_t r = (size_t)from[(size_t)j]; if (ot.len(r)) memcpy(r_names.blob.data() + r_names.off[(size_t)j], ot.ptr(r), ot.len(r)); }
    HIPCHK(r_titles.alloc((size_t)nbytes + 64));
    if (nbytes) HIPCHK(hipMemcpyAsync(r_titles.p, r_names.blob.data(), (size_t)nbytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r_toff.p, r_names.off.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipGetLastError());
  }
  // ---- the host side meanwhile: labels and text of the kept reads
  NameList names;
  if (!ctx->h_names.empty()) {
    names.off.resize((size_t)m + 1);
    int64_t nbytes = 0;
    for (int64_t j = 0; j < m; j++) { names.off[(size_t)j] = nbytes; nbytes += (int64_t)ctx->h_names.len((size_t)from[(size_t)j]); }
    names.off[(size_t)m] = nbytes;
    names.blob.resize((size_t)nbytes);
    for (int64_t j = 0; j < m; j++) { const size_t r = (size_t)from[(size_t)j]; if (ctx->h_names.len(r)) memcpy(names.blob.data() + names.off[(size_t)j], ctx->h_names.ptr(r), ctx->h_names.len(r)); }
  }
  itsx_io::Text text;
  if (!text.resize((size_t)off[(size_t)m])) SET_ERR(ctx, ITSX_E_NOMEM, "out of memory orienting the reads' text");
  {
    const char *comp = itsx::iupac_complement();
    const char *srcb = ctx->bases_view;
    char *dst = text.data();
    const int T = off[(size_t)m] >= (4 << 20) ? std::max(1, std::min(8, itsx_io::io_threads())) : 1;
    on_threads(T, [&](int t) {
      for (int64_t j = m * t / T, hi = m * (t + 1) / T; j < hi; j++) {
        const size_t r = (size_t)from[(size_t)j];
        const char *sb = srcb + ctx->h_off[r];
        char *db = dst + off[(size_t)j];
        const int64_t L = len[(size_t)j];
        if (hs[r] > 0) memcpy(db, sb, (size_t)L);
        else for (int64_t k = 0; k < L; k++) db[k] = comp[(unsigned char)sb[L - 1 - k]];
      }
    });
  }
  // ---- the device's own count of what it kept, and the swap
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(tot, d_tot.p, sizeof(tot), hipMemcpyDeviceToHost, st));
    if (S > 1) HIPCHK(hipMemcpyAsync(dcnt.data(), d_scnt.p, (size_t)S * 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  if (n > 0 && (tot[0] != m || tot[1] != woff[(size_t)m] || (S > 1 && dcnt != scnt)))
    SET_ERR(ctx, ITSX_E_DEVICE, "the oriented reads counted on the device and on the host differ");
  dbuf_swap(ctx->d_words, n_words); dbuf_swap(ctx->d_exc, n_exc); dbuf_swap(ctx->d_woff, n_woff); dbuf_swap(ctx->d_excoff, n_excoff); dbuf_swap(ctx->d_len, n_len);
  if (S > 1) dbuf_swap(ctx->d_sample, n_sample);
  ctx->rd.words = ctx->d_words.p; ctx->rd.woff = ctx->d_woff.p; ctx->rd.len = ctx->d_len.p;
  ctx->rd.excoff = ctx->d_excoff.p; ctx->rd.exc = ctx->d_exc.p; ctx->rd.n = m;
  ctx->N = m; ctx->Lmax = Lmax;
  ctx->h_off.swap(off); ctx->h_woff.swap(woff); ctx->h_len.swap(len); ctx->h_names.swap(names);
  if (S > 1) ctx->h_sample.swap(smp);
  ctx->h_bases.swap(text); ctx->bases_view = ctx->h_bases.data();
  ctx->prec.drop();                                      // the pairs' map named the reads that were
  ctx->ft.have = false; ctx->dn.have = false;
  if (records) {
    itsx_ctx::Records &rr = ctx->rec;
    dbuf_swap(rr.seq, r_seq); dbuf_swap(rr.qual, r_qual); dbuf_swap(rr.titles, r_titles); dbuf_swap(rr.off, r_off); dbuf_swap(rr.toff, r_toff);
    rr.h_titles.swap(r_names); rr.seq_p = rr.seq.p;
  }
  ctx->dev_bases = nullptr; ctx->d_merged_text.release();      // the text of the read set that was: this one's is on the host
  ctx->fall_to(itsx_ctx::ST_READS);      // (no StageTxn: the read set is replaced after the last step that can fail, and a failure keeps what stood on the old one)
  ctx->sel_sample = -1;
  ctx->stats.n_reads = m;
  if (n_kept_per_sample) for (int32_t s = 0; s < S; s++) n_kept_per_sample[s] = scnt[(size_t)s];
  return ITSX_OK;
}

// ------------------------------------------------------------------------------ f4: orientation by the profiles (k_orient_prof.hip)
// n_fwd / n_rev of a text: the profiles whose MSV filter passes at F1 on it / on its reverse complement -- the search's own filter
// (filter_tables' thresholds, launch_msv unshared, a res cell != 0).  Strand +1 / -1 by the larger count, 0 when they are equal.
// The read set is dereplicated here (strand both, minseqlength 1, per sample) and only the uniques' seeds are scanned, chunk by chunk
// of the length-sorted list: the chunk's reverse complements are written into a scratch read set by the apply kernels of k_orient.hip
// (source list = the chunk's seeds, every strand -1) and go through the filter with the same threshold rows -- a text and its reverse
// complement have one length.  The reads take their seed's verdict, negated and swapped where they are its reverse complement.
// apply: the reads of strand -1 are reverse-complemented where they are (orient_apply_strands with 0 as +1: nothing is dropped).
// Whatever happens the context holds no dereplication afterwards, and on an error the read set it had.
static int orient_profiles(itsx_ctx *ctx, double F1, int8_t *strand, int32_t *count_fwd, int32_t *count_rev, float *ms_kernels, bool apply)
{
  CTXCHK(ctx);
  const char *who = apply ? "itsx_orient_profiles_apply" : "itsx_orient_profiles";
  if (ms_kernels) *ms_kernels = 0;
  if (ctx->P <= 0) SET_ERR(ctx, ITSX_E_ARG, std::string(who) + " called before the profiles are loaded");
  if (!ctx->rd.woff) SET_ERR(ctx, ITSX_E_ARG, std::string(who) + " called before a read set is loaded");
  HIPCHK(hipSetDevice(ctx->device));
  if (apply && !ctx->bases_view) { const int rc = host_bases(ctx); if (rc != ITSX_OK) return rc; }
  StageTxn own(ctx, itsx_ctx::ST_READS);                     // never committed: the dereplication is this call's own, and goes with it
  { const int rc = itsx_derep(ctx, 1, 1, nullptr); if (rc != ITSX_OK) return rc; }
  hipStream_t st = ctx->st;
  const int64_t n = ctx->N;
  const int32_t U = ctx->U;
  const int P = ctx->P, Ppad = ctx->G * 64, Lcap = ctx->Lmax + 1;
  float ms = 0;
  DBuf<int32_t> ucf, ucr; DBuf<int8_t> ustr;
  HIPCHK(ucf.alloc((size_t)U + 1)); HIPCHK(ucr.alloc((size_t)U + 1)); HIPCHK(ustr.alloc((size_t)U + 1));
  if (U > 0) {
    { const int rc = filter_tables(ctx, F1, nullptr); if (rc != ITSX_OK) return rc; }
    // a chunk holds two result tables, its reverse complements and their lists: a quarter of what is free
    const size_t per_unique = (size_t)Ppad * 4 + (size_t)((ctx->Lmax + 15) / 16) * 4 + 64;
    int64_t Uc = ((1ll << 31) - 4096) / std::max(Ppad, 1);
    { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) Uc = std::min<int64_t>(Uc, (int64_t)(fr / 4 / per_unique)); }
    if (const char *e = sw_get("ITSX_CHUNK_UNIQUES")) Uc = atoll(e);
    Uc = std::max<int64_t>(1, std::min<int64_t>(Uc, U));
    std::vector<int64_t> hexc((size_t)n + 1, 0);             // (the exceptions' offsets live on the device only)
    HIPCHK(hipMemcpyAsync(hexc.data(), ctx->d_excoff.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    DBuf<int8_t> d_neg; DBuf<int32_t> d_iota, s_src, s_len; DBuf<int64_t> s_woff, s_excoff; DBuf<uint32_t> s_words, s_exc; DBuf<uint16_t> res_f, res_r;
    HIPCHK(d_neg.alloc((size_t)n + 1)); HIPCHK(hipMemsetAsync(d_neg.p, 0xff, (size_t)n + 1, st));
    HIPCHK(d_iota.alloc((size_t)Uc)); launch_op_iota(d_iota.p, (int32_t)Uc, st);
    HIPCHK(res_f.alloc((size_t)Ppad * (size_t)Uc)); HIPCHK(res_r.alloc((size_t)Ppad * (size_t)Uc));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int32_t> src, len; std::vector<int64_t> woff, excoff;
    for (int64_t u0 = 0; u0 < U; u0 += Uc) {
      const int32_t cU = (int32_t)std::min<int64_t>(Uc, U - u0);
      src.assign((size_t)cU, 0); len.assign((size_t)cU, 0); woff.assign((size_t)cU + 1, 0); excoff.assign((size_t)cU + 1, 0);
      for (int32_t j = 0; j < cU; j++) {
        const size_t r = (size_t)ctx->h_seed_read[(size_t)ctx->h_sorted_uniq[(size_t)(u0 + j)]];
        src[(size_t)j] = (int32_t)r; len[(size_t)j] = ctx->h_len[r];
        woff[(size_t)j + 1] = woff[(size_t)j] + (ctx->h_woff[r + 1] - ctx->h_woff[r]);
        excoff[(size_t)j + 1] = excoff[(size_t)j] + (hexc[r + 1] - hexc[r]);
      }
      HIPCHK(s_words.alloc((size_t)woff[(size_t)cU] + 1)); HIPCHK(s_exc.alloc((size_t)excoff[(size_t)cU] + 1));
      HIPCHK(upload(s_src, src, st)); HIPCHK(upload(s_len, len, st)); HIPCHK(upload(s_woff, woff, st)); HIPCHK(upload(s_excoff, excoff, st));
      StageTimer tm(st);
      OrientApplyArgs a{};
      a.rd = ctx->rd; a.strand = d_neg.p; a.src = s_src.p; a.woff = s_woff.p; a.excoff = s_excoff.p; a.len = s_len.p; a.words = s_words.p; a.exc = s_exc.p;
      launch_orient_apply_scatter(a, cU, st);
      ReadsDev srd{};
      srd.words = s_words.p; srd.woff = s_woff.p; srd.len = s_len.p; srd.excoff = s_excoff.p; srd.exc = s_exc.p; srd.n = cU;
      launch_msv(msv_args(ctx, ctx->rd, ctx->d_sorted_uniq.p + u0, ctx->d_seed_read.p, cU, Lcap, res_f.p), st);
      launch_msv(msv_args(ctx, srd, d_iota.p, d_iota.p, cU, Lcap, res_r.p), st);
      launch_op_verdict(res_f.p, res_r.p, cU, P, ctx->d_sorted_uniq.p + u0, ucf.p, ucr.p, ustr.p, st);
      ms += tm.stop();                                        // (waited for: the host's lists may change for the next chunk)
      HIPCHK(hipGetLastError());
    }
  }
  std::vector<int8_t> hs((size_t)n + 1, 0);
  DBuf<int8_t> d_s, d_keep; DBuf<int32_t> d_f, d_r;
  HIPCHK(d_s.alloc((size_t)n + 1)); HIPCHK(d_f.alloc((size_t)n + 1)); HIPCHK(d_r.alloc((size_t)n + 1));
  if (apply) HIPCHK(d_keep.alloc((size_t)n + 1));
  if (n > 0) {
    StageTimer tm(st);
    launch_op_compose(n, ctx->d_uniq_of.p, ctx->d_strand.p, ucf.p, ucr.p, ustr.p, d_s.p, d_f.p, d_r.p, apply ? d_keep.p : nullptr, st);
    ms += tm.stop();
    HIPCHK(hipMemcpyAsync(hs.data(), d_s.p, (size_t)n, hipMemcpyDeviceToHost, st));
    if (count_fwd) HIPCHK(hipMemcpyAsync(count_fwd, d_f.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (count_rev) HIPCHK(hipMemcpyAsync(count_rev, d_r.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
  }
  if (apply) {
    std::vector<int8_t> hk((size_t)n + 1, 1);
    for (int64_t r = 0; r < n; r++) if (hs[(size_t)r] < 0) hk[(size_t)r] = -1;
    const int rc = orient_apply_strands(ctx, hk, d_keep, nullptr);
    if (rc != ITSX_OK) return rc;
  }
  if (strand && n > 0) memcpy(strand, hs.data(), (size_t)n);
  if (ms_kernels) *ms_kernels = ms;
  return ITSX_OK;
}
int itsx_orient_profiles(itsx_ctx *ctx, double F1, int8_t *strand, int32_t *count_fwd, int32_t *count_rev, float *ms_kernels)
{
  return orient_profiles(ctx, F1, strand, count_fwd, count_rev, ms_kernels, false);
}
int itsx_orient_profiles_apply(itsx_ctx *ctx, double F1, int8_t *strand, int32_t *count_fwd, int32_t *count_rev, float *ms_kernels)
{
  return orient_profiles(ctx, F1, strand, count_fwd, count_rev, ms_kernels, true);
}

// ------------------------------------------------------------------------------ f2: paired-end merge (k_merge.hip)
extern "C++" {
namespace {
struct MergeTables {
  std::vector<double> q2p, match, mism; std::vector<uint8_t> qsame, qdiff;
  MergeTables() : q2p(128, 0.0), match(128 * 128, 0.0), mism(128 * 128, 0.0), qsame(128 * 128, 0), qdiff(128 * 128, 0)
  {
    // quality-aware scores and merged qualities of vsearch --fastq_mergepairs (Edgar & Flyvbjerg 2015), host libm.  Worked out in
    // long double and rounded once, as the oracle does: in double a log-odds next to 0 carries the rounding of 1 - px - py whole
    // (up to 27 ulp of the entry at Q2) and pow(10, -x/10) the rounding of x/10
    auto q_to_p = [](int c) -> long double { const int x = c - 33; return x < 2 ? 0.75L : powl(10.0L, -(long double)x / 10.0L); };
    auto qual_of = [](long double p) { long double q = rintl(-10.0L * log10l(p)); if (q > 41.0L) q = 41.0L; if (q < 0.0L) q = 0.0L; return (uint8_t)(33 + (int)q); };
    for (int x = 33; x < 127; x++) {
      const long double px = q_to_p(x);
      q2p[x] = (double)px;
      for (int y = 33; y < 127; y++) {
        const long double py = q_to_p(y);
        qsame[x * 128 + y] = qual_of(px * py / 3.0L / (1.0L - px - py + 4.0L * px * py / 3.0L));
        qdiff[x * 128 + y] = qual_of(px * (1.0L - py / 3.0L) / (px + py - 4.0L * px * py / 3.0L));
        match[x * 128 + y] = (double)log2l((1.0L - px - py + px * py * 4.0L / 3.0L) / 0.25L);
        mism[x * 128 + y] = (double)log2l(((px + py) / 3.0L - px * py * 4.0L / 9.0L) / 0.25L);
        // beside an error of 3/4 both probabilities are exactly 1/4: log-odds 0, which the rounded expressions miss
        if (x < 35 || y < 35) match[x * 128 + y] = mism[x * 128 + y] = 0.0;
      }
    }
  }
};
const MergeTables &merge_tables() { static MergeTables t; return t; }
}  // namespace
}  // extern "C++"

int itsx_merge_tables(double *q2p, double *match, double *mism, uint8_t *qsame, uint8_t *qdiff)
{
  const MergeTables &t = merge_tables();
  if (q2p) memcpy(q2p, t.q2p.data(), 128 * sizeof(double));
  if (match) memcpy(match, t.match.data(), 128 * 128 * sizeof(double));
  if (mism) memcpy(mism, t.mism.data(), 128 * 128 * sizeof(double));
  if (qsame) memcpy(qsame, t.qsame.data(), 128 * 128);
  if (qdiff) memcpy(qdiff, t.qdiff.data(), 128 * 128);
  return ITSX_OK;
}

// what the merge kernel read and wrote, kept in device memory for the compaction that follows it (merge_load_core)
struct MergeKeep {
  DBuf<uint8_t> os, oq; DBuf<int64_t> fo, ro; DBuf<int32_t> len, reason; bool want_oq = false;      // oq: the merged qualities, only where records are kept
  DBuf<uint8_t> fs, fq, rs, rq; bool want_pairs = false;       // the kernel's inputs, only where the pair records are kept
};
// The device step of a merge: bases, qualities and offsets of both sides lie in device memory (fb / rb bytes a side, max_total = the
// longest pair, at least 2); the kernel runs and the results are copied back.  keep (may be null): the merged bases stay in device
// memory (pair i's at foff[i] + roff[i]) with the pairs' lengths and reasons, taken over by *keep (the inputs stay the caller's); the
// bases are copied back only if out_seq is given -- the merge-and-load calls pack them where they are.  join: the kernel that joins
// runs (k_merge.hip: JOIN); the output planes are fb + rb + 8 n bytes, pair i's slot starts at foff[i] + roff[i] + 8 i, and joined
// (may be null) takes the pairs' marks.
static int merge_device(itsx_ctx *ctx, const uint8_t *d_fs, const uint8_t *d_fq, const int64_t *d_fo, const uint8_t *d_rs, const uint8_t *d_rq, const int64_t *d_ro,
                        int64_t n, int64_t fb, int64_t rb, int64_t max_total, int maxdiffs, double maxee, int allow_stagger,
                        char *out_seq, char *out_qual, int32_t *out_len, int32_t *reason, double *score, int32_t *shift, MergeKeep *keep,
                        bool join = false, int8_t *joined = nullptr)
{
  const MergeTables &t = merge_tables();
  DBuf<uint8_t> d_os, d_oq, d_qs, d_qd; DBuf<int32_t> d_len, d_reason, d_shift; DBuf<double> d_q2p, d_m, d_x, d_score; DBuf<int8_t> d_joined;
  const int64_t ob = fb + rb + (join ? 8 * n : 0);       // the bytes of an output plane
  HIPCHK(d_os.alloc((size_t)ob + 1)); HIPCHK(d_oq.alloc((size_t)ob + 1));
  if (join) HIPCHK(d_joined.alloc((size_t)n));
  HIPCHK(d_len.alloc((size_t)n)); HIPCHK(d_reason.alloc((size_t)n)); HIPCHK(d_shift.alloc((size_t)n)); HIPCHK(d_score.alloc((size_t)n));
  HIPCHK(upload(d_q2p, t.q2p, ctx->st)); HIPCHK(upload(d_m, t.match, ctx->st)); HIPCHK(upload(d_x, t.mism, ctx->st));
  HIPCHK(upload(d_qs, t.qsame, ctx->st)); HIPCHK(upload(d_qd, t.qdiff, ctx->st));
  MergeArgs a{};
  a.fseq = d_fs; a.fqual = d_fq; a.rseq = d_rs; a.rqual = d_rq; a.foff = d_fo; a.roff = d_ro; a.n = n; a.max_total = (int32_t)max_total;
  a.maxdiffs = maxdiffs; a.allow_stagger = allow_stagger ? 1 : 0; a.maxee = maxee;
  a.q2p = d_q2p.p; a.match = d_m.p; a.mism = d_x.p; a.qsame = d_qs.p; a.qdiff = d_qd.p;
  a.out_seq = d_os.p; a.out_qual = d_oq.p; a.out_len = d_len.p; a.reason = d_reason.p; a.shift = d_shift.p; a.score = d_score.p;
  a.join = join ? 1 : 0; a.joined = d_joined.p;
  StageTimer tm(ctx->st);
  launch_merge(a, ctx->st);
  ctx->stats.ms_merge = tm.stop();
  HIPCHK(hipGetLastError());
  if (out_seq) HIPCHK(hipMemcpyAsync(out_seq, d_os.p, (size_t)ob, hipMemcpyDeviceToHost, ctx->st));
  if (out_qual) HIPCHK(hipMemcpyAsync(out_qual, d_oq.p, (size_t)ob, hipMemcpyDeviceToHost, ctx->st));
  if (join && joined) HIPCHK(hipMemcpyAsync(joined, d_joined.p, (size_t)n, hipMemcpyDeviceToHost, ctx->st));
  HIPCHK(hipMemcpyAsync(out_len, d_len.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->st)); HIPCHK(hipMemcpyAsync(reason, d_reason.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->st));
  if (score) HIPCHK(hipMemcpyAsync(score, d_score.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->st));
  if (shift) HIPCHK(hipMemcpyAsync(shift, d_shift.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  if (keep) { dbuf_swap(keep->os, d_os); if (keep->want_oq) dbuf_swap(keep->oq, d_oq); dbuf_swap(keep->len, d_len); dbuf_swap(keep->reason, d_reason); }
  return ITSX_OK;
}
// The upload step: host planes are checked (offsets, the 12 000-base limit, the quality range) and go up, then merge_device runs on
// them.  keep (may be null) also takes over the pairs' offsets and, where the pair records are kept, the uploaded planes.
static int merge_core(itsx_ctx *ctx, const char *fseq, const char *fqual, const int64_t *foff, const char *rseq, const char *rqual,
                      const int64_t *roff, int64_t n, int maxdiffs, double maxee, int allow_stagger,
                      char *out_seq, char *out_qual, int32_t *out_len, int32_t *reason, double *score, int32_t *shift, MergeKeep *keep,
                      bool join = false, int8_t *joined = nullptr)
{
  CTXCHK(ctx && foff && roff && n >= 0 && out_len && reason && (n == 0 || (fseq && fqual && rseq && rqual && (keep || (out_seq && out_qual)))));
  HIPCHK(hipSetDevice(ctx->device));
  if (n == 0) return ITSX_OK;
  const int64_t fb = foff[n], rb = roff[n];
  int64_t max_total = 2;
  for (int64_t i = 0; i < n; i++) {
    const int64_t fl = foff[i + 1] - foff[i], rl = roff[i + 1] - roff[i];
    if (fl < 0 || rl < 0) SET_ERR(ctx, ITSX_E_ARG, "offsets must be non-decreasing");
    max_total = std::max(max_total, fl + rl);
  }
  if (max_total > 12000) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "read pairs longer than 12000 bases in total are not supported by the merge kernel");
  {   // every quality byte is looked at once (a gigabyte per million pairs: a pool of threads, not one)
    std::atomic<int> badf{0}, badr{0};
    const int T = (fb + rb) >= ((int64_t)8 << 20) ? std::max(1, std::min(itsx_io::io_threads(), 16)) : 1;
    on_threads(T, [&](int t) {
      int bf = 0, br = 0;
      for (int64_t i = fb * t / T, e = fb * (t + 1) / T; i < e; i++) bf |= ((unsigned char)fqual[i] < 33) | ((unsigned char)fqual[i] > 126);
      for (int64_t i = rb * t / T, e = rb * (t + 1) / T; i < e; i++) br |= ((unsigned char)rqual[i] < 33) | ((unsigned char)rqual[i] > 126);
      if (bf) badf = 1;
      if (br) badr = 1;
    });
    if (badf) SET_ERR(ctx, ITSX_E_FORMAT, "forward quality outside ASCII 33..126 (--fastq_qmax 93)");
    if (badr) SET_ERR(ctx, ITSX_E_FORMAT, "reverse quality outside ASCII 33..126 (--fastq_qmax 93)");
  }
  DBuf<uint8_t> d_fs, d_fq, d_rs, d_rq; DBuf<int64_t> d_fo, d_ro;
  // (kept planes are read by k_trim_copy, whose trim_load4 reads two aligned dwords: 8 bytes past the end must be readable)
  const size_t pad = keep && keep->want_pairs ? 64 : 1;
  HIPCHK(d_fs.alloc((size_t)fb + pad)); HIPCHK(d_fq.alloc((size_t)fb + pad)); HIPCHK(d_rs.alloc((size_t)rb + pad)); HIPCHK(d_rq.alloc((size_t)rb + pad));
  HIPCHK(d_fo.alloc((size_t)n + 1)); HIPCHK(d_ro.alloc((size_t)n + 1));
  HIPCHK(hipMemcpyAsync(d_fs.p, fseq, (size_t)fb, hipMemcpyHostToDevice, ctx->st)); HIPCHK(hipMemcpyAsync(d_fq.p, fqual, (size_t)fb, hipMemcpyHostToDevice, ctx->st));
  HIPCHK(hipMemcpyAsync(d_rs.p, rseq, (size_t)rb, hipMemcpyHostToDevice, ctx->st)); HIPCHK(hipMemcpyAsync(d_rq.p, rqual, (size_t)rb, hipMemcpyHostToDevice, ctx->st));
  HIPCHK(hipMemcpyAsync(d_fo.p, foff, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, ctx->st)); HIPCHK(hipMemcpyAsync(d_ro.p, roff, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, ctx->st));
  const int rc = merge_device(ctx, d_fs.p, d_fq.p, d_fo.p, d_rs.p, d_rq.p, d_ro.p, n, fb, rb, max_total, maxdiffs, maxee, allow_stagger,
                              out_seq, out_qual, out_len, reason, score, shift, keep, join, joined);
  if (rc != ITSX_OK) return rc;
  if (keep) { dbuf_swap(keep->fo, d_fo); dbuf_swap(keep->ro, d_ro); }
  if (keep && keep->want_pairs) { dbuf_swap(keep->fs, d_fs); dbuf_swap(keep->fq, d_fq); dbuf_swap(keep->rs, d_rs); dbuf_swap(keep->rq, d_rq); }
  return ITSX_OK;
}
int itsx_merge_buffers(itsx_ctx *ctx, const char *fseq, const char *fqual, const int64_t *foff, const char *rseq, const char *rqual,
                       const int64_t *roff, int64_t n, int maxdiffs, double maxee, int allow_stagger,
                       char *out_seq, char *out_qual, int32_t *out_len, int32_t *reason, double *score, int32_t *shift)
{
  CTXCHK(ctx && (n == 0 || (out_seq && out_qual)));
  return merge_core(ctx, fseq, fqual, foff, rseq, rqual, roff, n, maxdiffs, maxee, allow_stagger, out_seq, out_qual, out_len, reason, score, shift, nullptr);
}

// the same with the join always on (the context's setting is not consulted): output planes of foff[n] + roff[n] + 8 n bytes, pair i's
// slot at foff[i] + roff[i] + 8 i, joined[i] = 1 where the read there is R1 + NNNNNNNN + revcomp(R2)
int itsx_merge_buffers_join(itsx_ctx *ctx, const char *fseq, const char *fqual, const int64_t *foff, const char *rseq, const char *rqual,
                            const int64_t *roff, int64_t n, int maxdiffs, double maxee, int allow_stagger,
                            char *out_seq, char *out_qual, int32_t *out_len, int32_t *reason, double *score, int32_t *shift, int8_t *joined)
{
  CTXCHK(ctx && (n == 0 || (out_seq && out_qual && joined)));
  return merge_core(ctx, fseq, fqual, foff, rseq, rqual, roff, n, maxdiffs, maxee, allow_stagger, out_seq, out_qual, out_len, reason, score, shift, nullptr, true, joined);
}

// FASTQ in, FASTQ out: R1/R2 (plain or gzip) -> merged reads, labels = forward read's identifier up to the first blank
int itsx_merge_pairs_files(itsx_ctx *ctx, const char *r1_path, const char *r2_path, const char *out_path, int maxdiffs, double maxee,
                           int allow_stagger, int64_t *n_pairs, int64_t *n_merged)
{
  CTXCHK(ctx && r1_path && r2_path && out_path);
  typedef FastxPart Side;
  auto parse = [ctx](const char *path, Side &sd, std::string &perr) -> int {   // no shared state: the two files are read side by side
    const auto tp = slurp(path, true, perr, ctx);
    if (!tp) return ITSX_E_IO;
    if (!tp->empty() && (*tp)[0] != '@') { perr = std::string("malformed FASTQ record 1 in ") + path; return ITSX_E_FORMAT; }
    const int prc = parse_fastx(*tp, true, true, sd, perr);
    if (prc != ITSX_OK) perr += std::string(" in ") + path;
    return prc;
  };
  Side f, r;
  std::string ferr, rerr2;
  int rc2 = ITSX_OK;
  static const bool trace = sw_get("ITSX_TRACE_ALLOC") != nullptr;
  const auto tm0 = std::chrono::steady_clock::now();
  std::thread other([&] { rc2 = parse(r2_path, r, rerr2); });
  int rc = parse(r1_path, f, ferr);
  other.join();
  const auto tm1 = std::chrono::steady_clock::now();
  if (rc != ITSX_OK) { ctx->set_error(ferr); return rc; }
  if (rc2 != ITSX_OK) { ctx->set_error(rerr2); return rc2; }
  if (f.ids.size() != r.ids.size()) SET_ERR(ctx, ITSX_E_FORMAT, "R1 and R2 hold different numbers of records");
  const int64_t n = (int64_t)f.ids.size();
  const bool join = ctx->merge_join;                     // (itsx_set_merge_join: joined records go to seq.fq in pair order, 8 bytes more per slot)
  std::string oseq((size_t)(f.seq.size() + r.seq.size()) + (join ? (size_t)n * 8 : 0) + 1, '\0'), oqual = oseq;
  std::vector<int32_t> olen((size_t)n + 1), reason((size_t)n + 1);
  rc = merge_core(ctx, f.seq.data(), f.qual.data(), f.off.data(), r.seq.data(), r.qual.data(), r.off.data(), n, maxdiffs, maxee, allow_stagger,
                  &oseq[0], &oqual[0], olen.data(), reason.data(), nullptr, nullptr, nullptr, join, nullptr);
  if (rc != ITSX_OK) return rc;
  ctx->h_merge_join.assign((size_t)n, 0);                // itsx_merge_join_info: the marks of this call's pairs
  if (join) for (int64_t i = 0; i < n; i++) ctx->h_merge_join[(size_t)i] = olen[i] > 0 && reason[i] != 0;
  const auto tm2 = std::chrono::steady_clock::now();
  // seq.fq is read back by the loader and by the paired trimmer: written through the block writer, which also leaves
  // its text in the reader's cache
  itsx_io::BlockWriter bw;
  std::string werr, buf;
  if (!bw.open(out_path, itsx_io::PLAIN, werr, true)) SET_ERR(ctx, ITSX_E_IO, werr);
  int64_t merged = 0;
  for (int64_t i = 0; i < n; i++) {
    if (join ? olen[i] <= 0 : reason[i] != 0) continue;
    const size_t o = (size_t)(f.off[i] + r.off[i]) + (join ? (size_t)i * 8 : 0);
    buf += '@'; buf.append(f.ids.ptr((size_t)i), f.ids.len((size_t)i)); buf += '\n';
    buf.append(oseq.data() + o, (size_t)olen[i]); buf += "\n+\n";
    buf.append(oqual.data() + o, (size_t)olen[i]); buf += '\n';
    if (buf.size() >= (1u << 20)) { bw.put(buf); buf.clear(); }
    if (reason[i] == 0) merged++;                        // (joined records are not counted here: itsx_merge_join_info has them)
  }
  bw.put(buf);
  if (!bw.close(werr)) SET_ERR(ctx, ITSX_E_IO, werr);
  if (trace) {
    const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[itsx] merge files: read+inflate+parse %.0f ms, upload+kernel+download %.0f ms, write %.0f ms\n", ms(tm0, tm1), ms(tm1, tm2), ms(tm2, std::chrono::steady_clock::now()));
  }
  if (n_pairs) *n_pairs = n;
  if (n_merged) *n_merged = merged;
  return ITSX_OK;
}

// one side of a paired sample: a file (text == nullptr) or a record-aligned piece of its text already in memory.  No shared state: the
// sides of one sample, and the samples of a batch, are parsed side by side
// titles: the records' whole title lines are collected too (sd.titles; the pair records of itsx_keep_pair_records)
static int parse_fastq_side(const char *path, const char *text, int64_t nb, FastxPart &sd, std::string &perr, bool titles = false, itsx_ctx *ctx = nullptr)
{
  std::shared_ptr<const itsx_io::Text> tp;
  itsx_io::Text view;
  const itsx_io::Text *t = &view;
  if (text) view.borrow(text, (size_t)nb);
  else { tp = slurp(path, true, perr, ctx); if (!tp) return ITSX_E_IO; t = tp.get(); }
  if (!t->empty() && (*t)[0] != '@') { perr = std::string("malformed FASTQ record 1 in ") + path; return ITSX_E_FORMAT; }
  const int prc = parse_fastx(*t, true, true, sd, perr);
  if (prc != ITSX_OK) { perr += std::string(" in ") + path; return prc; }
  if (titles) {
    fastq_titles(*t, sd.titles);
    if (sd.titles.size() != sd.ids.size()) { perr = std::string("pair records are kept (itsx_keep_pair_records) and this file is not FASTQ throughout: ") + path; return ITSX_E_FORMAT; }
  }
  return prc;
}

// The pairs of one sample or of a batch of samples -> merged reads as the context's read set.  f / r: the forward and the reverse reads of
// ALL pairs (offsets over the whole batch); pairs [pstart[s], pstart[s + 1]) are sample s's and their labels are ids[s]'s.  One merge
// kernel for all of them; what it left on the device is compacted there (k_merge.hip: k_merge_compact), gathered into a gap-free text and
// packed.  The host walks the pairs once, for the labels, while the gather runs.  seq_out_paths (may be null, entries may be null): the
// sample's merged records as itsx_merge_pairs_files writes them -- the only case in which merged bases and qualities come back.
// dev (may be null; the device parse's loader, merge_pairs_load_device): the planes already lie in device memory, upper-cased and checked
// (k_fastq.hip: k_fastq_pairs); of f and r only `off` is filled, and the title planes and their offsets are dev's.
struct MergeDev {
  DBuf<uint8_t> *fs, *fq, *rs, *rq, *t1, *t2; DBuf<int64_t> *fo, *ro;      // taken over where they are kept, left alone otherwise
  const std::vector<int64_t> *to1, *to2;                                  // [n + 1] the title lines' offsets
  int64_t max_total;
};
static int merge_load_core(itsx_ctx *ctx, const FastxPart &f, const FastxPart &r, const std::vector<const NameList *> &ids, const std::vector<int64_t> &pstart,
                           const char *const *seq_out_paths, int maxdiffs, double maxee, int allow_stagger, double parse_ms, int64_t *n_merged_per_sample,
                           bool records = false, bool pair_records = false, MergeDev *dev = nullptr)
{
  const int32_t S = (int32_t)pstart.size() - 1;
  const int64_t n = pstart[(size_t)S];
  if (S > 1 && (int64_t)S * std::max(ctx->P, 1) > (1ll << 28)) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "too many samples x profiles for one batch");
  static const bool trace = sw_get("ITSX_TRACE_ALLOC") != nullptr;
  const auto tm1 = std::chrono::steady_clock::now();
  bool want_text = false;
  if (seq_out_paths) for (int32_t s = 0; s < S; s++) want_text = want_text || seq_out_paths[s] != nullptr;
  std::vector<int32_t> olen((size_t)n + 1), reason((size_t)n + 1);
  std::string oseq, oqual;
  // itsx_set_merge_join: the reads are the merged AND the joined pairs (out_len > 0), and a pair's slot lies 8 bytes further per pair before it
  const bool join = ctx->merge_join;
  const auto kept = [&](int64_t p) { return join ? olen[(size_t)p] > 0 : reason[(size_t)p] == 0; };
  const auto slot = [&](int64_t p) { return (size_t)(f.off[(size_t)p] + r.off[(size_t)p]) + (join ? (size_t)p * 8 : 0); };
  if (want_text) { oseq.assign((dev ? (size_t)(f.off[(size_t)n] + r.off[(size_t)n]) : (size_t)(f.seq.size() + r.seq.size())) + (join ? (size_t)n * 8 : 0) + 1, '\0'); oqual = oseq; }
  MergeKeep k;
  k.want_oq = records; k.want_pairs = pair_records;
  int rc = ITSX_OK;
  if (!dev) rc = merge_core(ctx, f.seq.data(), f.qual.data(), f.off.data(), r.seq.data(), r.qual.data(), r.off.data(), n, maxdiffs, maxee, allow_stagger,
                            want_text ? &oseq[0] : nullptr, want_text ? &oqual[0] : nullptr, olen.data(), reason.data(), nullptr, nullptr, &k, join, nullptr);
  else if (n > 0) {
    rc = merge_device(ctx, dev->fs->p, dev->fq->p, dev->fo->p, dev->rs->p, dev->rq->p, dev->ro->p, n, f.off[(size_t)n], r.off[(size_t)n], std::max<int64_t>(dev->max_total, 2),
                      maxdiffs, maxee, allow_stagger, want_text ? &oseq[0] : nullptr, want_text ? &oqual[0] : nullptr, olen.data(), reason.data(), nullptr, nullptr, &k, join, nullptr);
    if (rc == ITSX_OK) {                                 // as merge_core leaves *keep
      dbuf_swap(k.fo, *dev->fo); dbuf_swap(k.ro, *dev->ro);
      if (pair_records) { dbuf_swap(k.fs, *dev->fs); dbuf_swap(k.fq, *dev->fq); dbuf_swap(k.rs, *dev->rs); dbuf_swap(k.rq, *dev->rq); }
    }
  }
  if (rc != ITSX_OK) return rc;
  const auto tm2 = std::chrono::steady_clock::now();
  hipStream_t st = ctx->st;
  DBuf<int64_t> d_src, d_dst, d_blk, d_tot, d_scnt, d_pstart; DBuf<int32_t> d_pidx; DBuf<uint8_t> d_cmp;
  int64_t tot[2] = {0, 0};                               // merged reads, the bytes of their text
  std::vector<int64_t> scnt((size_t)S, 0);               // merged reads per sample
  if (n > 0) {
    const int64_t nb = merge_compact_blocks(n);
    HIPCHK(d_src.alloc((size_t)n + 1)); HIPCHK(d_dst.alloc((size_t)n + 1)); HIPCHK(d_pidx.alloc((size_t)n)); HIPCHK(d_blk.alloc((size_t)nb * 2)); HIPCHK(d_tot.alloc(2));
    MergeCompactArgs a{};
    a.reason = k.reason.p; a.out_len = k.len.p; a.foff = k.fo.p; a.roff = k.ro.p; a.n = n; a.n_samples = S; a.join = join ? 1 : 0;
    a.blk_cnt = d_blk.p; a.blk_len = d_blk.p + nb; a.pair_index = d_pidx.p; a.srcoff = d_src.p; a.dstoff = d_dst.p;
    if (S > 1) {
      HIPCHK(upload(d_pstart, pstart, st)); HIPCHK(d_scnt.alloc((size_t)S)); HIPCHK(ctx->d_sample.alloc((size_t)n + 1));
      HIPCHK(hipMemsetAsync(d_scnt.p, 0, (size_t)S * 8, st));
      a.pair_start = d_pstart.p; a.sample = ctx->d_sample.p; a.sample_count = d_scnt.p;
    }
    launch_merge_compact(a, d_tot.p, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tot, d_tot.p, sizeof(tot), hipMemcpyDeviceToHost, st));
    if (S > 1) HIPCHK(hipMemcpyAsync(scnt.data(), d_scnt.p, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  const int64_t m = tot[0];
  if (m >= (1ll << 31) - 64) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "more than 2^31 reads in one context");
  if (S == 1) scnt[0] = m;
  ctx->h_off.assign((size_t)m + 1, 0);
  ctx->h_merge_index.assign((size_t)n, -1);              // per pair: its merged read (itsx_merge_pair_index)
  ctx->h_merge_join.assign((size_t)n, 0);                // per pair: its read is a joined one (itsx_merge_join_info)
  std::vector<int64_t> sjoin((size_t)S, 0);              // joined reads per sample
  if (join) for (int32_t s = 0; s < S; s++)
    for (int64_t p = pstart[(size_t)s]; p < pstart[(size_t)s + 1]; p++)
      if (olen[(size_t)p] > 0 && reason[(size_t)p] != 0) { ctx->h_merge_join[(size_t)p] = 1; sjoin[(size_t)s]++; }
  HIPCHK(d_cmp.alloc((size_t)tot[1] + 64));
  if (m > 0) {
    hipLaunchKernelGGL(k_gather_reads, dim3((unsigned)std::min<int64_t>((m + 3) / 4, 65535)), dim3(256), 0, st, k.os.p, d_src.p, d_dst.p, m, d_cmp.p);
  }
  // records: the merged qualities through the same compaction, into a plane beside the text
  DBuf<uint8_t> r_qual;
  if (records) {
    HIPCHK(r_qual.alloc((size_t)tot[1] + 64));
    if (m > 0) hipLaunchKernelGGL(k_gather_reads, dim3((unsigned)std::min<int64_t>((m + 3) / 4, 65535)), dim3(256), 0, st, k.oq.p, d_src.p, d_dst.p, m, r_qual.p);
  }
  // the gather has only been enqueued: the labels need `reason` alone.  (The copies back go into pageable memory and would hold the host
  // until the stream reaches them, so they are issued after the loop.)
  ctx->h_names.clear();
  for (int32_t s = 0; s < S; s++) {
    const NameList &nl = *ids[(size_t)s];
    const int64_t p0 = pstart[(size_t)s], cnt = pstart[(size_t)s + 1] - p0;
    for (int64_t i = 0; i < cnt; i++)
      if (kept(p0 + i)) ctx->h_names.emplace_back(nl.ptr((size_t)i), nl.ptr((size_t)i) + nl.len((size_t)i));
  }
  if (m > 0) HIPCHK(hipMemcpyAsync(ctx->h_off.data(), d_dst.p, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost, st));
  if (n > 0) HIPCHK(hipMemcpyAsync(ctx->h_merge_index.data(), d_pidx.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  if ((int64_t)ctx->h_names.size() != m) SET_ERR(ctx, ITSX_E_DEVICE, "the merged pairs counted on the device and on the host differ");
  ctx->N = m;
  itsx_io::Text().swap(ctx->h_bases);
  static const uint8_t none = 0;
  // rep.fa and the seeds' sequences fetch the text from dev_bases later (host_bases): the context owns it from here on
  ctx->d_merged_text.release();
  dbuf_swap(ctx->d_merged_text, d_cmp);
  // every joined read brings eight N: the exception list is sized for them at once (its guess is one symbol in 256 bases, and a read set
  // past it packs its exceptions twice)
  for (int32_t s = 0; s < S; s++) ctx->pack_exc_hint += 8 * sjoin[(size_t)s];
  rc = pack_and_upload(ctx, nullptr, m > 0 ? ctx->d_merged_text.p : &none);
  if (rc != ITSX_OK) return rc;
  if (records) {                                         // bases = the gathered text, titles = '@' + label (what itsx_merge_pairs_files writes)
    itsx_ctx::Records &rr = ctx->rec;
    NameList &t = rr.h_titles;
    t.off.resize((size_t)m + 1); t.blob.resize(ctx->h_names.blob.size() + (size_t)m);
    for (int64_t j = 0; j < m; j++) {
      t.off[(size_t)j] = ctx->h_names.off[(size_t)j] + j;
      t.blob[(size_t)t.off[(size_t)j]] = '@';
      if (ctx->h_names.len((size_t)j)) memcpy(t.blob.data() + t.off[(size_t)j] + 1, ctx->h_names.ptr((size_t)j), ctx->h_names.len((size_t)j));
    }
    t.off[(size_t)m] = (int64_t)t.blob.size();
    HIPCHK(rr.titles.alloc(t.blob.size() + 64)); HIPCHK(rr.toff.alloc((size_t)m + 1)); HIPCHK(rr.off.alloc((size_t)m + 1));
    if (!t.blob.empty()) HIPCHK(hipMemcpyAsync(rr.titles.p, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(rr.toff.p, t.off.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(rr.off.p, ctx->h_off.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    dbuf_swap(rr.qual, r_qual);
    rr.seq_p = ctx->d_merged_text.p; rr.have = true;
  }
  if (pair_records) {
    // the ORIGINAL pairs beside the merged reads: the planes the merge kernel read, the title lines, and per pair the read its R1
    // identifier NAMES among its sample's merged reads -- Dedup looks record1.id up in the sample's dictionary, so a pair that did not
    // merge but carries a merged pair's identifier is sliced with that read's coordinates, and of equal labels the first wins
    // (trim_host.cpp: NameIndex).  h_merge_index is not that map.
    itsx_ctx::PairRecords &pr = ctx->prec;
    if (!dev && ((int64_t)f.titles.size() != n || (int64_t)r.titles.size() != n)) SET_ERR(ctx, ITSX_E_FORMAT, "the title lines kept for the pairs do not match the pairs");
    std::vector<int32_t> pread((size_t)n, -1);
    {
      std::vector<int64_t> rfirst((size_t)S + 1, 0);
      for (int32_t s = 0; s < S; s++) rfirst[(size_t)s + 1] = rfirst[(size_t)s] + scnt[(size_t)s];
      const int T = std::max(1, std::min<int>({itsx_io::io_threads(), 16, (int)S}));
      on_threads(T, [&](int t) {
        std::unordered_map<std::string_view, int32_t> named;
        for (int32_t s = t; s < S; s += T) {
          const NameList &nl = *ids[(size_t)s];
          const int64_t p0 = pstart[(size_t)s], cnt = pstart[(size_t)s + 1] - p0;
          named.clear(); named.reserve((size_t)scnt[(size_t)s] * 2);
          int64_t j = rfirst[(size_t)s];
          for (int64_t i = 0; i < cnt; i++)
            if (kept(p0 + i)) named.emplace(std::string_view(nl.ptr((size_t)i), nl.len((size_t)i)), (int32_t)j++);      // (emplace keeps the first)
          for (int64_t i = 0; i < cnt; i++) {
            const auto it = named.find(std::string_view(nl.ptr((size_t)i), nl.len((size_t)i)));
            if (it != named.end()) pread[(size_t)(p0 + i)] = it->second;
          }
        }
      });
    }
    if (n == 0) {                                        // merge_core had nothing to upload
      HIPCHK(k.fs.alloc(64)); HIPCHK(k.fq.alloc(64)); HIPCHK(k.rs.alloc(64)); HIPCHK(k.rq.alloc(64)); HIPCHK(k.fo.alloc(1)); HIPCHK(k.ro.alloc(1));
      HIPCHK(hipMemsetAsync(k.fo.p, 0, 8, st)); HIPCHK(hipMemsetAsync(k.ro.p, 0, 8, st));
    }
    if (dev && n > 0) { dbuf_swap(pr.t1, *dev->t1); dbuf_swap(pr.t2, *dev->t2); }      // the parser's title planes, where the gather left them
    else {
      const size_t nt1 = dev ? 0 : f.titles.blob.size(), nt2 = dev ? 0 : r.titles.blob.size();
      HIPCHK(pr.t1.alloc(nt1 + 64)); HIPCHK(pr.t2.alloc(nt2 + 64));
      if (nt1) HIPCHK(hipMemcpyAsync(pr.t1.p, f.titles.blob.data(), nt1, hipMemcpyHostToDevice, st));
      if (nt2) HIPCHK(hipMemcpyAsync(pr.t2.p, r.titles.blob.data(), nt2, hipMemcpyHostToDevice, st));
    }
    HIPCHK(pr.to1.alloc((size_t)n + 1)); HIPCHK(pr.to2.alloc((size_t)n + 1)); HIPCHK(pr.pair_read.alloc((size_t)n + 1));
    HIPCHK(hipMemcpyAsync(pr.to1.p, dev ? dev->to1->data() : f.titles.off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pr.to2.p, dev ? dev->to2->data() : r.titles.off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    if (n > 0) HIPCHK(hipMemcpyAsync(pr.pair_read.p, pread.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    dbuf_swap(pr.s1, k.fs); dbuf_swap(pr.q1, k.fq); dbuf_swap(pr.s2, k.rs); dbuf_swap(pr.q2, k.rq); dbuf_swap(pr.o1, k.fo); dbuf_swap(pr.o2, k.ro);
    pr.pstart = pstart; pr.n = n; pr.have = true;
  }
  if (S > 1) {                                           // the state itsx_load_reads_files + itsx_set_samples leave (d_sample is filled already)
    ctx->h_sample.resize((size_t)m);
    int64_t at = 0;
    for (int32_t s = 0; s < S; s++) { std::fill(ctx->h_sample.begin() + at, ctx->h_sample.begin() + at + scnt[(size_t)s], s); at += scnt[(size_t)s]; }
    if (at != m) SET_ERR(ctx, ITSX_E_DEVICE, "the merged pairs counted per sample do not add up");
    ctx->S = S;
  }
  const auto tm3 = std::chrono::steady_clock::now();
  if (want_text) {
    // seq.fq is read back by the reference's Dedup and by the single-file trimmer: written through the block writer, which also leaves
    // its text in the reader's cache.  One file per sample, several at a time
    std::vector<int32_t> todo;
    for (int32_t s = 0; s < S; s++) if (seq_out_paths[s]) todo.push_back(s);
    const int T = std::max(1, std::min<int>({itsx_io::io_threads(), 16, (int)todo.size()}));
    std::vector<std::string> werrs((size_t)T);
    std::atomic<size_t> next{0};
    on_threads(T, [&](int t) {
      itsx_io::IoThreadCap share(16 / T);                // the block writers' own pools: 16 threads in all
      for (;;) {
        const size_t q = next.fetch_add(1);
        if (q >= todo.size()) break;
        const int32_t s = todo[q];
        const NameList &nl = *ids[(size_t)s];
        itsx_io::BlockWriter bw;
        std::string werr, buf;
        if (!bw.open(seq_out_paths[s], itsx_io::PLAIN, werr, true)) { werrs[(size_t)t] = werr; continue; }
        for (int64_t p = pstart[(size_t)s], i = 0; p < pstart[(size_t)s + 1]; p++, i++) {
          if (!kept(p)) continue;
          const size_t o = slot(p);
          buf += '@'; buf.append(nl.ptr((size_t)i), nl.len((size_t)i)); buf += '\n';
          buf.append(oseq.data() + o, (size_t)olen[(size_t)p]); buf += "\n+\n";
          buf.append(oqual.data() + o, (size_t)olen[(size_t)p]); buf += '\n';
          if (buf.size() >= (1u << 20)) { bw.put(buf); buf.clear(); }
        }
        bw.put(buf);
        if (!bw.close(werr)) werrs[(size_t)t] = werr;
      }
    });
    for (const std::string &e : werrs) if (!e.empty()) SET_ERR(ctx, ITSX_E_IO, e);
  }
  if (trace) {
    const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[itsx] merge + load (%d sample%s): read+inflate+parse %.0f ms, upload+kernel %.0f ms, compact+gather+pack %.0f ms, write %.0f ms\n",
            (int)S, S == 1 ? "" : "s", parse_ms, ms(tm1, tm2), ms(tm2, tm3), ms(tm3, std::chrono::steady_clock::now()));
  }
  if (n_merged_per_sample) for (int32_t s = 0; s < S; s++) n_merged_per_sample[s] = scnt[(size_t)s] - sjoin[(size_t)s];      // merged pairs only
  return ITSX_OK;
}

// R1/R2 -> merged reads as THIS CONTEXT'S READ SET (arrays mode: nothing written, nothing parsed again).  The reference writes the merged
// reads to tempdir/seq.fq and vsearch reads them back (SeqSample.py:266-365, 93-131); here the merge kernel's output is gathered into
// a gap-free text on the device and packed where it is -- the merged bases never visit the host, the merged qualities are not needed at
// all (the paired writer slices the ORIGINAL R1 / R2 records with the merged reads' coordinates).  Labels = R1 identifiers of the merged
// pairs, in input order, as itsx_merge_pairs_files writes them.
// the two sides of a paired sample from files (text1 == nullptr) or from record-aligned pieces of their text already in memory (a
// streaming driver's slices: itsx_merge_pairs_load_text)
static int merge_pairs_load_impl(itsx_ctx *ctx, const char *r1_path, const char *r2_path, const char *text1, int64_t nb1, const char *text2, int64_t nb2,
                                 int maxdiffs, double maxee, int allow_stagger, int64_t *n_pairs, int64_t *n_merged)
{
  if (device_parse_on(ctx)) {
    const int drc = merge_pairs_load_device(ctx, &r1_path, &r2_path, nullptr, 1, text1, nb1, text2, nb2, maxdiffs, maxee, allow_stagger, n_pairs, n_merged, false);
    if (drc != PARSE_FALLBACK) return drc;
  }
  FastxPart f, r;
  std::string ferr, rerr2;
  int rc2 = ITSX_OK;
  const auto tm0 = std::chrono::steady_clock::now();
  const bool pair_records = ctx->keep_pair_records && !text1;      // (a streamed piece keeps none, as with itsx_keep_records)
  std::thread other([&] { rc2 = parse_fastq_side(r2_path, text2, nb2, r, rerr2, pair_records, ctx); });
  int rc = parse_fastq_side(r1_path, text1, nb1, f, ferr, pair_records, ctx);
  other.join();
  if (rc != ITSX_OK) { ctx->set_error(ferr); return rc; }
  if (rc2 != ITSX_OK) { ctx->set_error(rerr2); return rc2; }
  if (f.ids.size() != r.ids.size()) SET_ERR(ctx, ITSX_E_FORMAT, "R1 and R2 hold different numbers of records");
  const int64_t n = (int64_t)f.ids.size();
  int64_t m = 0;
  rc = merge_load_core(ctx, f, r, {&f.ids}, {0, n}, nullptr, maxdiffs, maxee, allow_stagger,
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tm0).count(), &m, ctx->keep_records && !text1,
                       pair_records && !f.lower && !r.lower);      // (lower-case bases: see merge_pairs_load_files_impl)
  if (rc != ITSX_OK) return rc;
  if (n_pairs) *n_pairs = n;
  if (n_merged) *n_merged = m;
  return ITSX_OK;
}
int itsx_merge_pairs_load(itsx_ctx *ctx, const char *r1_path, const char *r2_path, int maxdiffs, double maxee, int allow_stagger, int64_t *n_pairs, int64_t *n_merged)
{
  CTXCHK(ctx && r1_path && r2_path);
  return merge_pairs_load_impl(ctx, r1_path, r2_path, nullptr, 0, nullptr, 0, maxdiffs, maxee, allow_stagger, n_pairs, n_merged);
}
// Round 6 (a streamed paired sample, itsxpress_amd/stream.py): the same, from record-aligned pieces of R1's and R2's text that hold the
// same number of records (itsx_stream_next / itsx_stream_next_records)
int itsx_merge_pairs_load_text(itsx_ctx *ctx, const char *text1, int64_t nbytes1, const char *text2, int64_t nbytes2, int maxdiffs, double maxee, int allow_stagger,
                               int64_t *n_pairs, int64_t *n_merged)
{
  CTXCHK(ctx && text1 && text2 && nbytes1 >= 0 && nbytes2 >= 0);
  return merge_pairs_load_impl(ctx, "(R1 slice)", "(R2 slice)", text1, nbytes1, text2, nbytes2, maxdiffs, maxee, allow_stagger, n_pairs, n_merged);
}
// f4 batching: the read pairs of EVERY sample of a batch through one merge (the QIIME 2 plugin merges once per manifest row,
// q2_itsxpress.py:72-80 -> SeqSample.py:266-365).  All files are read and parsed side by side on the I/O pool, all pairs go through one
// merge_load_core, and the context ends up as itsx_load_reads_files leaves it: S = n_samples, reads in sample order and then pair order.
static int merge_pairs_load_files_impl(itsx_ctx *ctx, const char *const *r1_paths, const char *const *r2_paths, const char *const *seq_out_paths,
                                       int32_t S, int maxdiffs, double maxee, int allow_stagger, int64_t *n_pairs_per_sample, int64_t *n_merged_per_sample)
{
  if (device_parse_on(ctx)) {
    const int drc = merge_pairs_load_device(ctx, r1_paths, r2_paths, seq_out_paths, S, nullptr, 0, nullptr, 0, maxdiffs, maxee, allow_stagger, n_pairs_per_sample, n_merged_per_sample, true);
    if (drc != PARSE_FALLBACK) return drc;
  }
  const auto tm0 = std::chrono::steady_clock::now();
  std::vector<FastxPart> fs((size_t)S), rs((size_t)S);
  const bool pair_records = ctx->keep_pair_records;
  std::vector<std::string> errs((size_t)S * 2);
  std::vector<int> rcs((size_t)S * 2, ITSX_OK);
  const int T = std::max(1, std::min<int>({itsx_io::io_threads(), 16, (int)std::min<int64_t>((int64_t)S * 2, 16)}));
  {
    std::atomic<int64_t> next{0};
    on_threads(T, [&](int) {
      // at most 16 threads in all: a worker's reader, inflater and parser size their pools by io_threads(), so each gets the worker's
      // share of the budget (16 workers: everything a worker calls runs on the worker itself)
      itsx_io::IoThreadCap share(16 / T);
      for (;;) {
        const int64_t q = next.fetch_add(1);
        if (q >= (int64_t)S * 2) break;
        const size_t s = (size_t)(q >> 1);
        rcs[(size_t)q] = (q & 1) ? parse_fastq_side(r2_paths[s], nullptr, 0, rs[s], errs[(size_t)q], pair_records, ctx) : parse_fastq_side(r1_paths[s], nullptr, 0, fs[s], errs[(size_t)q], pair_records, ctx);
      }
    });
  }
  for (size_t q = 0; q < (size_t)S * 2; q++) if (rcs[q] != ITSX_OK) { ctx->set_error(errs[q]); return rcs[q]; }
  std::vector<int64_t> pstart((size_t)S + 1, 0);
  std::vector<const NameList *> ids((size_t)S);
  for (size_t s = 0; s < (size_t)S; s++) {
    if (fs[s].ids.size() != rs[s].ids.size())
      SET_ERR(ctx, ITSX_E_FORMAT, std::string("R1 and R2 hold different numbers of records: ") + r1_paths[s] + " (" + std::to_string(fs[s].ids.size()) + ") and " +
              r2_paths[s] + " (" + std::to_string(rs[s].ids.size()) + ")");
    pstart[s + 1] = pstart[s] + (int64_t)fs[s].ids.size();
    ids[s] = &fs[s].ids;
    if (n_pairs_per_sample) n_pairs_per_sample[s] = (int64_t)fs[s].ids.size();
  }
  const int64_t n = pstart[(size_t)S];
  // The pair records' bases are the merge's own upload, which is upper case.  Where that changed a base, slices of them would not be the
  // input's bytes, which the host writer and the reference copy: such a batch keeps no pair records and its trimmed pairs come from the
  // host writer.
  bool lower = false;
  for (size_t s = 0; s < (size_t)S; s++) lower = lower || fs[s].lower || rs[s].lower;
  // the samples' reads side by side in one text per direction (one sample: its own)
  FastxPart F, R;
  bool oom = false;
  auto join = [&](std::vector<FastxPart> &parts, FastxPart &out) {
    std::vector<int64_t> sb((size_t)S + 1, 0);
    for (size_t s = 0; s < (size_t)S; s++) sb[s + 1] = sb[s] + (int64_t)parts[s].seq.size();
    if (!out.seq.resize((size_t)sb[(size_t)S]) || !out.qual.resize((size_t)sb[(size_t)S])) { oom = true; return; }
    out.off.assign((size_t)n + 1, 0);
    const int TJ = std::max(1, std::min(T, (int)S));
    on_threads(TJ, [&](int t) {
      for (size_t s = (size_t)t; s < (size_t)S; s += (size_t)TJ) {
        FastxPart &p = parts[s];
        if (p.seq.size()) { memcpy(out.seq.data() + sb[s], p.seq.data(), p.seq.size()); memcpy(out.qual.data() + sb[s], p.qual.data(), p.seq.size()); }
        for (size_t i = 0; i < p.ids.size(); i++) out.off[(size_t)pstart[s] + i + 1] = sb[s] + p.off[i + 1];
        itsx_io::Text().swap(p.seq); itsx_io::Text().swap(p.qual);
      }
    });
    if (pair_records) for (size_t s = 0; s < (size_t)S; s++) {      // the title lines, in the same order
      NameList &t = parts[s].titles;
      const int64_t b0 = (int64_t)out.titles.blob.size();
      out.titles.blob.insert(out.titles.blob.end(), t.blob.begin(), t.blob.end());
      for (size_t i = 0; i < t.size(); i++) out.titles.off.push_back(b0 + t.off[i + 1]);
      NameList().swap(t);
    }
  };
  if (S > 1) { join(fs, F); if (!oom) join(rs, R); }
  if (oom) SET_ERR(ctx, ITSX_E_NOMEM, "out of memory joining the samples' reads");
  return merge_load_core(ctx, S > 1 ? F : fs[0], S > 1 ? R : rs[0], ids, pstart, seq_out_paths, maxdiffs, maxee, allow_stagger,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tm0).count(), n_merged_per_sample, ctx->keep_records, pair_records && !lower);
}
int itsx_merge_pairs_load_files(itsx_ctx *ctx, const char *const *r1_paths, const char *const *r2_paths, const char *const *seq_out_paths,
                                int32_t n_samples, int maxdiffs, double maxee, int allow_stagger, int64_t *n_pairs_per_sample, int64_t *n_merged_per_sample)
{
  CTXCHK(ctx && r1_paths && r2_paths && n_samples >= 1);
  for (int32_t s = 0; s < n_samples; s++) CTXCHK(r1_paths[s] && r2_paths[s]);
  const int rc = merge_pairs_load_files_impl(ctx, r1_paths, r2_paths, seq_out_paths, n_samples, maxdiffs, maxee, allow_stagger, n_pairs_per_sample, n_merged_per_sample);
  if (rc != ITSX_OK) {                                   // whatever failed, the context is left empty (no reads, one sample) and usable
    const std::string why = ctx->err;
    const int64_t zero = 0;
    (void)itsx_set_reads(ctx, nullptr, &zero, 0, nullptr, nullptr);
    ctx->h_merge_index.clear(); ctx->h_merge_join.clear();
    ctx->set_error(why);
  }
  return rc;
}
// per pair of the last itsx_merge_pairs_load / _load_text / _load_files (there: the pairs of all samples, in sample order): the index of its
// merged read in the context's read set, -1 = not merged
int itsx_merge_pair_index(const itsx_ctx *ctx, int32_t *index, int64_t n_pairs)
{
  CTXCHK(ctx && index);
  if ((size_t)n_pairs != ctx->h_merge_index.size()) SET_ERR(ctx, ITSX_E_ARG, "itsx_merge_pair_index: the last merge held " + std::to_string(ctx->h_merge_index.size()) + " pairs");
  memcpy(index, ctx->h_merge_index.data(), (size_t)n_pairs * sizeof(int32_t));
  return ITSX_OK;
}

// per pair of the context's last merge call (a merge-and-load: the pairs itsx_merge_pair_index speaks of; itsx_merge_pairs_files: that
// call's pairs): 1 = the pair was joined (itsx_set_merge_join), and how many were
int itsx_merge_join_info(const itsx_ctx *ctx, int8_t *joined, int64_t n_pairs, int64_t *n_joined)
{
  CTXCHK(ctx);
  if ((size_t)n_pairs != ctx->h_merge_join.size()) SET_ERR(ctx, ITSX_E_ARG, "itsx_merge_join_info: the last merge held " + std::to_string(ctx->h_merge_join.size()) + " pairs");
  if (joined && n_pairs > 0) memcpy(joined, ctx->h_merge_join.data(), (size_t)n_pairs);
  if (n_joined) { int64_t c = 0; for (const int8_t j : ctx->h_merge_join) c += j; *n_joined = c; }
  return ITSX_OK;
}

// ------------------------------------------------------------------------------ coordinates
static int coords_common(itsx_ctx *ctx, const char *lp, const char *rp, bool per_read, int32_t *start, int32_t *stop, int32_t *tlen, int32_t *ind)
{
  CTXCHK(ctx && lp && rp);
  const bool to_host = start && stop && tlen && ind;        // all four, or none (the results stay on the device)
  if (!to_host && (start || stop || tlen || ind)) return ITSX_E_ARG;
  if (!ctx->finalized()) SET_ERR(ctx, ITSX_E_ARG, "coordinates requested before itsx_search_finalize");
  if (ctx->lazy && ctx->lazy_pending > 0 && !ctx->partial_coords)
    SET_ERR(ctx, ITSX_E_ARG, std::to_string(ctx->lazy_pending) + " domain row(s) of the lazy search depend on the exact domZ and could change a result: "
            "search again with itsx_set_rows_mode(ctx, 1) (itsx_lazy_pending reports this after itsx_search_finalize)");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const int32_t U = ctx->U; const int64_t n = ctx->N;
  std::vector<int8_t> side((size_t)std::max(ctx->P, 1), 0);
  const size_t ll = strlen(lp), rl = strlen(rp);
  if (ctx->compact_rows && (ll > 2 || rl > 2)) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "ITSX_COMPACT_ROWS keeps the best rows per 2-character profile prefix: a longer prefix cannot be served");
  for (int p = 0; p < ctx->P; p++) {
    const std::string &nm = ctx->profs[p].name;
    if (nm.compare(0, ll, lp) == 0) side[p] = 1;
    else if (nm.compare(0, rl, rp) == 0) side[p] = 2;
  }
  DBuf<int8_t> &d_side = ctx->w_side; DBuf<unsigned long long> &bl = ctx->w_bl, &br = ctx->w_br; DBuf<int32_t> &uind = ctx->w_uind, &us = ctx->w_us, &ue = ctx->w_ue, &ut = ctx->w_ut;
  HIPCHK(upload(d_side, side, st));
  HIPCHK(bl.alloc((size_t)U + 1)); HIPCHK(br.alloc((size_t)U + 1)); HIPCHK(uind.alloc((size_t)U + 1));
  HIPCHK(us.alloc((size_t)U + 1)); HIPCHK(ue.alloc((size_t)U + 1)); HIPCHK(ut.alloc((size_t)U + 1));
  HIPCHK(hipMemsetAsync(bl.p, 0, ((size_t)U + 1) * 8, st)); HIPCHK(hipMemsetAsync(br.p, 0, ((size_t)U + 1) * 8, st));
  HIPCHK(hipMemsetAsync(uind.p, 0, ((size_t)U + 1) * 4, st));
  HIPCHK(ctx->w_cl.alloc((size_t)U + 1)); HIPCHK(ctx->w_cr.alloc((size_t)U + 1));
  for (size_t c = 0; c < ctx->dom_n.size(); c++)
    if (ctx->dom_n[c] > 0) launch_positions(ctx->dom_bufs[c]->p, ctx->dom_n[c], d_side.p, bl.p, br.p, uind.p, st);
  for (size_t c = 0; c < ctx->dom_n.size(); c++)          // the winners' coordinates (exactly one row carries each winning key)
    if (ctx->dom_n[c] > 0) launch_position_coords(ctx->dom_bufs[c]->p, ctx->dom_n[c], d_side.p, bl.p, br.p, ctx->w_cl.p, ctx->w_cr.p, st);
  if (U > 0) hipLaunchKernelGGL(k_rep_coords, dim3((U + 255) / 256), dim3(256), 0, st, U, bl.p, br.p, ctx->w_cl.p, ctx->w_cr.p, ctx->d_seed_read.p, ctx->rd.len, us.p, ue.p, ut.p);
  {   // parity-risk counters (itsx_stats): winners out of clustered regions, pairs at the region cap
    DBuf<int32_t> &uflag = ctx->w_uflag; DBuf<int64_t> &d_c = ctx->w_counters;
    HIPCHK(uflag.alloc((size_t)U + 1)); HIPCHK(d_c.alloc(8));
    HIPCHK(hipMemsetAsync(uflag.p, 0, ((size_t)U + 1) * 4, st)); HIPCHK(hipMemsetAsync(d_c.p, 0, 8 * sizeof(int64_t), st));
    for (size_t c = 0; c < ctx->dom_n.size(); c++)
      if (ctx->dom_n[c] > 0) launch_position_flags(ctx->dom_bufs[c]->p, ctx->dom_n[c], d_side.p, bl.p, br.p, uflag.p, st);
    launch_count_flags(uflag.p, U, ctx->d_uniq_of.p, n, (unsigned long long *)d_c.p, st);
    int64_t hc[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(hc, d_c.p, sizeof(hc), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ctx->stats.n_uniq_multi_winner = hc[0]; ctx->stats.n_reads_multi_winner = hc[1]; ctx->stats.n_uniq_region_cap = hc[2]; ctx->stats.n_reads_region_cap = hc[3];
  }
  if (!per_read) {
    if (U > 0 && to_host) {
      HIPCHK(hipMemcpyAsync(start, us.p, (size_t)U * 4, hipMemcpyDeviceToHost, st)); HIPCHK(hipMemcpyAsync(stop, ue.p, (size_t)U * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(tlen, ut.p, (size_t)U * 4, hipMemcpyDeviceToHost, st)); HIPCHK(hipMemcpyAsync(ind, uind.p, (size_t)U * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return ITSX_OK;
  }
  DBuf<int32_t> &rs = ctx->w_rs, &re = ctx->w_re, &rt = ctx->w_rt, &ri = ctx->w_ri;
  HIPCHK(rs.alloc((size_t)n + 1)); HIPCHK(re.alloc((size_t)n + 1)); HIPCHK(rt.alloc((size_t)n + 1)); HIPCHK(ri.alloc((size_t)n + 1));
  if (n > 0) {
    hipLaunchKernelGGL(k_read_coords, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, ctx->d_uniq_of.p, us.p, ue.p, ut.p, uind.p, rs.p, re.p, rt.p, ri.p);
    if (to_host) {
    HIPCHK(hipMemcpyAsync(start, rs.p, (size_t)n * 4, hipMemcpyDeviceToHost, st)); HIPCHK(hipMemcpyAsync(stop, re.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(tlen, rt.p, (size_t)n * 4, hipMemcpyDeviceToHost, st)); HIPCHK(hipMemcpyAsync(ind, ri.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  return ITSX_OK;
}
int itsx_trim_coords(itsx_ctx *ctx, const char *lp, const char *rp, int32_t *start, int32_t *stop, int32_t *tlen, int32_t *ind)
{ return coords_common(ctx, lp, rp, true, start, stop, tlen, ind); }
// the same results left on the device as [n][4] int32 rows (start, stop, tlen, in_ddict): per read / per representative
static int coords_device(itsx_ctx *ctx, const char *lp, const char *rp, bool per_read, int32_t **d_rows, int64_t *n_rows)
{
  CTXCHK(ctx && d_rows);
  const int rc = coords_common(ctx, lp, rp, per_read, nullptr, nullptr, nullptr, nullptr);
  if (rc != ITSX_OK) return rc;
  const int64_t n = per_read ? ctx->N : ctx->U;
  HIPCHK(ctx->w_coords4.alloc((size_t)n * 4 + 4));
  if (n > 0) {
    if (per_read) hipLaunchKernelGGL(k_pack_coords4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->st, n, ctx->w_rs.p, ctx->w_re.p, ctx->w_rt.p, ctx->w_ri.p, ctx->w_coords4.p);
    else hipLaunchKernelGGL(k_pack_coords4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->st, n, ctx->w_us.p, ctx->w_ue.p, ctx->w_ut.p, ctx->w_uind.p, ctx->w_coords4.p);
  }
  HIPCHK(hipStreamSynchronize(ctx->st));
  HIPCHK(hipGetLastError());
  *d_rows = ctx->w_coords4.p;
  if (n_rows) *n_rows = n;
  return ITSX_OK;
}
int itsx_trim_coords_device(itsx_ctx *ctx, const char *lp, const char *rp, int32_t **d_rows, int64_t *n_rows) { return coords_device(ctx, lp, rp, true, d_rows, n_rows); }
int itsx_rep_coords_device(itsx_ctx *ctx, const char *lp, const char *rp, int32_t **d_rows, int64_t *n_rows) { return coords_device(ctx, lp, rp, false, d_rows, n_rows); }
// ITSX_DEVICE_DEFLATE=1: the batch writers' gzip output (compression 1) takes the device path (compression 3); read at every call
static bool device_deflate_switch() { const char *e = sw_get("ITSX_DEVICE_DEFLATE"); return e && atoi(e) == 1; }
// nbytes of device memory to the host: pieces through the pinned staging buffers, copied on while the next piece is on the bus
static int fetch_staged(itsx_ctx *ctx, const uint8_t *dsrc, int64_t total, char *dst)
{
  hipStream_t st = ctx->st;
  if (total > 0) {
    const int64_t CH = std::min<int64_t>(64ll << 20, std::max<int64_t>(total, 70000));
    { const int rc = stage_reserve(ctx, CH); if (rc != ITSX_OK) return rc; }
    const int64_t piece = (int64_t)ctx->stage_cap;
    const int64_t np = (total + piece - 1) / piece;
    constexpr int K = itsx_ctx::NSTAGE;
    auto drain = [&](int64_t c) -> int {       // piece c has been enqueued: wait for it and copy it on
      HIPCHK(hipEventSynchronize(ctx->stage_ev[c % K]));
      const int64_t o = c * piece, b = std::min(piece, total - o);
      memcpy(dst + o, ctx->stage_pin[c % K], (size_t)b);
      return ITSX_OK;
    };
    for (int64_t c = 0; c < np; c++) {
      if (c >= K) { const int rc = drain(c - K); if (rc != ITSX_OK) return rc; }
      const int64_t o = c * piece, b = std::min(piece, total - o);
      HIPCHK(hipMemcpyAsync(ctx->stage_pin[c % K], dsrc + o, (size_t)b, hipMemcpyDeviceToHost, st));
      HIPCHK(hipEventRecord(ctx->stage_ev[c % K], st));
    }
    for (int64_t c = std::max<int64_t>(0, np - K); c < np; c++) { const int rc = drain(c); if (rc != ITSX_OK) return rc; }
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return ITSX_OK;
}
// ------------------------------------------------------------------------------ gzip members made on the device (k_deflate.hip)
// Ranges [lo, hi) of a device text (readable 8 bytes past the last range), each cut into blocks of at most DEFLATE_BLOCK_BYTES; every
// block becomes one gzip member (an empty range: one empty member), and range r's members end up one after another in
// z[zb[r], zb[r + 1]).  The blocks go through the device in waves of at most DEFLATE_WAVE, so the scratch (worst-case slots, the
// packed members, the token slots of the resident workgroups) is a fixed budget of about 0.4 GB whatever the text's size; only
// compressed bytes come back, through the pinned staging buffers.  stats.ms_deflate: the wave kernels' time, by device events.
constexpr int32_t DEFLATE_WAVE = 2048;
static int64_t deflate_bound(int64_t nbytes, int64_t n_ranges)
{ return nbytes + (nbytes / DEFLATE_BLOCK_BYTES + n_ranges) * (int64_t)(DEFLATE_SLOT_BYTES - DEFLATE_BLOCK_BYTES); }
static int deflate_ranges(itsx_ctx *ctx, const uint8_t *dtext, const std::vector<std::pair<int64_t, int64_t>> &ranges, std::vector<char> &z,
                          std::vector<int64_t> &zb)
{
  hipStream_t st = ctx->st;
  std::vector<DeflateBlock> blocks; std::vector<int32_t> owner;
  for (size_t r = 0; r < ranges.size(); r++) {
    int64_t o = ranges[r].first;
    do {
      const int64_t b = std::min<int64_t>(DEFLATE_BLOCK_BYTES, ranges[r].second - o);
      blocks.push_back(DeflateBlock{o, (int32_t)b, 0}); owner.push_back((int32_t)r);
      o += b;
    } while (o < ranges[r].second);
  }
  zb.assign(ranges.size() + 1, 0); z.clear();
  ctx->stats.ms_deflate = 0;
  if (blocks.empty()) return ITSX_OK;
  int ncu = 256;
  { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, ctx->device) == hipSuccess && pr.multiProcessorCount > 0) ncu = pr.multiProcessorCount; }
  const int32_t wave = (int32_t)std::min<size_t>(blocks.size(), (size_t)DEFLATE_WAVE);
  const int grid = std::min<int>(wave, ncu);                                 // one workgroup's LDS is most of a CU's
  HIPCHK(ctx->w_dblk.alloc((size_t)wave)); HIPCHK(ctx->w_dsizes.alloc((size_t)wave)); HIPCHK(ctx->w_ddst.alloc((size_t)wave));
  HIPCHK(ctx->w_dtok.alloc((size_t)grid * DEFLATE_TOKEN_SLOT));
  HIPCHK(ctx->w_dslots.alloc((size_t)wave * DEFLATE_SLOT_BYTES)); HIPCHK(ctx->w_dpacked.alloc((size_t)wave * DEFLATE_SLOT_BYTES));
  std::vector<int32_t> sizes((size_t)wave); std::vector<int64_t> dst((size_t)wave);
  std::vector<int64_t> rsize(ranges.size(), 0);
  for (size_t b0 = 0; b0 < blocks.size(); b0 += (size_t)wave) {
    const int32_t nb = (int32_t)std::min<size_t>((size_t)wave, blocks.size() - b0);
    HIPCHK(hipMemcpyAsync(ctx->w_dblk.p, blocks.data() + b0, (size_t)nb * sizeof(DeflateBlock), hipMemcpyHostToDevice, st));
    DeflateArgs da{};
    da.text = dtext; da.blk = ctx->w_dblk.p; da.nblk = nb; da.tokens = ctx->w_dtok.p; da.slots = ctx->w_dslots.p; da.sizes = ctx->w_dsizes.p;
    {
      StageTimer tm(st);
      launch_deflate(da, grid, st);
      ctx->stats.ms_deflate += tm.stop();
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sizes.data(), ctx->w_dsizes.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t packed = 0;
    for (int32_t k = 0; k < nb; k++) {
      if (sizes[(size_t)k] < 20 || sizes[(size_t)k] > DEFLATE_SLOT_BYTES - 2) SET_ERR(ctx, ITSX_E_DEVICE, "the device deflate left a member of " + std::to_string(sizes[(size_t)k]) + " bytes");
      dst[(size_t)k] = packed; packed += sizes[(size_t)k]; rsize[(size_t)owner[b0 + (size_t)k]] += sizes[(size_t)k];
    }
    HIPCHK(hipMemcpyAsync(ctx->w_ddst.p, dst.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
    launch_deflate_pack(ctx->w_dslots.p, ctx->w_dsizes.p, ctx->w_ddst.p, nb, ctx->w_dpacked.p, st);
    HIPCHK(hipGetLastError());
    const size_t at = z.size();
    try { z.resize(at + (size_t)packed); } catch (const std::bad_alloc &) { SET_ERR(ctx, ITSX_E_NOMEM, "out of memory for the batch's compressed text"); }
    { const int rc = fetch_staged(ctx, ctx->w_dpacked.p, packed, z.data() + at); if (rc != ITSX_OK) return rc; }
  }
  for (size_t r = 0; r < ranges.size(); r++) zb[r + 1] = zb[r] + rsize[r];
  return ITSX_OK;
}
// the second half of the batch writers: the text k_trim_copy left in w_tout (total bytes; sample s's file is bytes [bo[s], bo[s + 1]))
// comes back through the pinned staging buffers in pieces, and each sample's range goes through a BlockWriter of its own, several samples
// at a time (a null path: that sample is skipped).  A file that could not be written whole is removed; the other samples' files stay.
// compression 3: the text stays where it is, its samples' ranges are deflated on the device (deflate_ranges) and the files are plain
// writes of the gzip members that come back.
static int trim_text_to_files(itsx_ctx *ctx, int64_t total, const int64_t *bo, const char *const *out_paths, int compression)
{
  const int32_t S = ctx->S;
  std::vector<int32_t> todo;
  for (int32_t s = 0; s < S; s++) if (out_paths[s]) todo.push_back(s);
  if (compression == 3) {
    std::vector<std::pair<int64_t, int64_t>> ranges;
    for (int32_t s : todo) ranges.emplace_back(bo[s], bo[s + 1]);
    std::vector<char> z; std::vector<int64_t> zb;
    { const int rc = deflate_ranges(ctx, reinterpret_cast<const uint8_t *>(ctx->w_tout.p), ranges, z, zb); if (rc != ITSX_OK) return rc; }
    const int T = std::max(1, std::min<int>({itsx_io::io_threads(), 16, (int)todo.size()}));
    std::vector<std::string> werrs((size_t)T);
    std::atomic<size_t> next{0};
    on_threads(T, [&](int t) {
      for (;;) {
        const size_t q = next.fetch_add(1);
        if (q >= todo.size()) break;
        const char *path = out_paths[todo[q]];
        const size_t nz = (size_t)(zb[q + 1] - zb[q]);
        FILE *fp = fopen(path, "wb");
        if (!fp) { werrs[(size_t)t] = std::string("cannot open ") + path + " for writing"; continue; }
        const bool short_write = fwrite(z.data() + zb[q], 1, nz, fp) != nz;
        if (fclose(fp) != 0 || short_write) { werrs[(size_t)t] = std::string("could not write ") + path; (void)remove(path); }      // never a short file
      }
    });
    for (const std::string &e : werrs) if (!e.empty()) SET_ERR(ctx, ITSX_E_IO, e);
    return ITSX_OK;
  }
  // ---- the text to the host
  itsx_io::Text text;
  if (!text.resize((size_t)total)) SET_ERR(ctx, ITSX_E_NOMEM, "out of memory for the batch's trimmed text");
  { const int rc = fetch_staged(ctx, reinterpret_cast<const uint8_t *>(ctx->w_tout.p), total, text.data()); if (rc != ITSX_OK) return rc; }
  // ---- one file per sample, several at a time (16 threads in all, the block writers' own pools included)
  const int T = std::max(1, std::min<int>({itsx_io::io_threads(), 16, (int)todo.size()}));
  std::vector<std::string> werrs((size_t)T);
  std::atomic<size_t> next{0};
  on_threads(T, [&](int t) {
    itsx_io::IoThreadCap share(16 / T);
    for (;;) {
      const size_t q = next.fetch_add(1);
      if (q >= todo.size()) break;
      const int32_t s = todo[q];
      itsx_io::BlockWriter bw;
      std::string werr;
      if (!bw.open(out_paths[s], compression, werr)) { werrs[(size_t)t] = werr; continue; }
      for (int64_t o = bo[s]; o < bo[s + 1]; o += (1 << 20)) bw.put(text.data() + o, (size_t)std::min<int64_t>(1 << 20, bo[s + 1] - o));
      if (!bw.close(werr)) { werrs[(size_t)t] = werr; (void)remove(out_paths[s]); }      // never a short file
    }
  });
  for (const std::string &e : werrs) if (!e.empty()) SET_ERR(ctx, ITSX_E_IO, e);
  return ITSX_OK;
}
// Where a trimming call takes its coordinates from: the finalized search by two profile prefixes, or the caller's arrays over the reads
// (tlen among them where the caller has one: with_tlen) -- exactly one of the two, checked in the caller's name.  As device pointers: the
// rows of coords_device (stride 4), or the arrays in w_tstart / w_tstop / w_ttlen (stride 1; upload = false: the caller places them itself)
struct CoordSource { const int32_t *start = nullptr, *stop = nullptr, *tlen = nullptr; int32_t stride = 1; bool by_prefix = false; };
static int coord_source(itsx_ctx *ctx, const std::string &who, const char *lp, const char *rp, const int32_t *start, const int32_t *stop, const int32_t *tlen,
                        bool with_tlen, bool upload, CoordSource &out)
{
  const bool by_prefix = lp || rp, by_arrays = start || stop || tlen;
  if (by_prefix == by_arrays || (by_prefix && !(lp && rp)) || (by_arrays && !(start && stop && (tlen || !with_tlen))))
    SET_ERR(ctx, ITSX_E_ARG, who + ": give either left_prefix and right_prefix or " + (with_tlen ? "start, stop and tlen" : "start and stop"));
  if (by_prefix && !ctx->finalized()) SET_ERR(ctx, ITSX_E_ARG, who + ": prefixes given before itsx_search_finalize");
  HIPCHK(hipSetDevice(ctx->device));
  out.by_prefix = by_prefix;
  if (by_prefix) {
    int32_t *rows = nullptr; int64_t nrows = 0;
    const int rc = coords_device(ctx, lp, rp, true, &rows, &nrows);
    if (rc != ITSX_OK) return rc;
    out.start = rows; out.stop = rows + 1; out.tlen = rows + 2; out.stride = 4;
  } else if (upload) {
    const size_t n = (size_t)ctx->N;
    const int32_t *src[3] = {start, stop, tlen}; DBuf<int32_t> *dst[3] = {&ctx->w_tstart, &ctx->w_tstop, &ctx->w_ttlen}; const int32_t **res[3] = {&out.start, &out.stop, &out.tlen};
    for (int k = 0; k < (with_tlen ? 3 : 2); k++) {
      HIPCHK(dst[k]->alloc(n + 1));
      if (n > 0) HIPCHK(hipMemcpyAsync(dst[k]->p, src[k], n * 4, hipMemcpyHostToDevice, ctx->st));
      *res[k] = dst[k]->p;
    }
  }
  return ITSX_OK;
}
// ------------------------------------------------------------------------------ f1 for a batch (k_trim.hip)
// The trimmed FASTQ of every sample from the records the context keeps: one plan (lengths, 64-bit scan) and one copy kernel make the
// text of the whole batch in device memory; it comes back through the pinned staging buffers in pieces, and each sample's byte range
// goes through a BlockWriter of its own, several samples at a time.  A file that could not be written whole is removed.
int itsx_write_trimmed_samples(itsx_ctx *ctx, const char *const *out_paths, int32_t n_samples, int compression, int trim_ccs,
                               const char *left_prefix, const char *right_prefix, const int32_t *start, const int32_t *stop,
                               int64_t *n_written_per_sample, int64_t *total_len_per_sample)
{
  CTXCHK(ctx && out_paths);
  if (!ctx->rec.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_write_trimmed_samples: the read set keeps no records; call itsx_keep_records(ctx, 1) before the reads are loaded, merged or oriented");
  if (n_samples != ctx->S) SET_ERR(ctx, ITSX_E_ARG, "itsx_write_trimmed_samples: " + std::to_string(n_samples) + " output paths for " + std::to_string(ctx->S) + " sample(s)");
  if (compression < 0 || compression > 3) SET_ERR(ctx, ITSX_E_ARG, "compression must be 0 (plain), 1 (gzip), 2 (zstd) or 3 (gzip, deflated on the device)");
  if (compression == 1 && device_deflate_switch()) compression = 3;
  CoordSource cs;
  { const int rc = coord_source(ctx, "itsx_write_trimmed_samples", left_prefix, right_prefix, start, stop, nullptr, false, true, cs); if (rc != ITSX_OK) return rc; }
  if (compression != 3) { itsx_io::PieceCompressor probe(compression); if (!probe.ok()) SET_ERR(ctx, ITSX_E_IO, "zstd output requested but libzstd.so.1 could not be loaded"); }
  hipStream_t st = ctx->st;
  const int64_t n = ctx->N; const int32_t S = ctx->S;
  TrimPlanArgs pa{};
  pa.start = cs.start; pa.stop = cs.stop; pa.stride = cs.stride;
  // samples are contiguous in the read set: sample s is reads [first[s], first[s + 1])
  std::vector<int64_t> first((size_t)S + 1, 0), bounds((size_t)(S + 1) * 3, 0);
  if (S > 1) { for (int64_t r = 0; r < n; r++) first[(size_t)ctx->h_sample[(size_t)r] + 1]++; for (int32_t s = 0; s < S; s++) first[(size_t)s + 1] += first[(size_t)s]; }
  else first[1] = n;
  HIPCHK(upload(ctx->w_tfirst, first, st));
  HIPCHK(ctx->w_trec.alloc((size_t)n + 1)); HIPCHK(ctx->w_tcnt.alloc((size_t)n + 1)); HIPCHK(ctx->w_ttot.alloc((size_t)n + 1));
  HIPCHK(ctx->w_tblk.alloc((size_t)trim_plan_blocks(n) * 3 + 3)); HIPCHK(ctx->w_tbounds.alloc(bounds.size()));
  pa.off = ctx->rec.off.p; pa.toff = ctx->rec.toff.p; pa.n = n; pa.ccs = trim_ccs ? 1 : 0;
  pa.blk = ctx->w_tblk.p; pa.rec = ctx->w_trec.p; pa.cnt = ctx->w_tcnt.p; pa.tot = ctx->w_ttot.p;
  launch_trim_plan(pa, ctx->w_tfirst.p, S, ctx->w_tbounds.p, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(bounds.data(), ctx->w_tbounds.p, bounds.size() * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t *bo = bounds.data(), *bc = bo + (S + 1), *bt = bc + (S + 1);
  const int64_t total = bo[S];
  HIPCHK(ctx->w_tout.alloc((size_t)(trim_copy_bytes(total) / 4) + 16));
  TrimCopyArgs ca{};
  ca.rec = ctx->w_trec.p; ca.n = n; ca.seq = ctx->rec.seq_p; ca.qual = ctx->rec.qual.p; ca.titles = ctx->rec.titles.p;
  ca.total = total; ca.ccs = pa.ccs; ca.out = ctx->w_tout.p;
  launch_trim_copy(ca, st);
  HIPCHK(hipGetLastError());
  { const int rc = trim_text_to_files(ctx, total, bo, out_paths, compression); if (rc != ITSX_OK) return rc; }
  for (int32_t s = 0; s < S; s++) {
    if (n_written_per_sample) n_written_per_sample[s] = bc[s + 1] - bc[s];
    if (total_len_per_sample) total_len_per_sample[s] = bt[s + 1] - bt[s];
  }
  return ITSX_OK;
}
// ------------------------------------------------------------------------------ the feature table of the trimmed regions (k_ftable.hip)
// Distinct trimmed sequences by samples, from the packed reads, the coordinates and the samples the context holds: what a user makes of
// the trimmed FASTQ files with `vsearch --derep_fulllength --sizeout`.  The table stays in the context (ctx->ft) for the getters below.
int itsx_trimmed_table(itsx_ctx *ctx, const char *left_prefix, const char *right_prefix, const int32_t *start, const int32_t *stop, int32_t min_len,
                       int64_t *n_features, int64_t *n_entries, int64_t *n_counted, float *ms_kernels)
{
  CTXCHK(ctx);
  if (min_len < 1) SET_ERR(ctx, ITSX_E_ARG, "itsx_trimmed_table: min_len must be at least 1, not " + std::to_string(min_len));
  if (!ctx->rd.woff || ctx->N <= 0) SET_ERR(ctx, ITSX_E_ARG, "itsx_trimmed_table called before a read set is loaded");
  hipStream_t st = ctx->st;
  itsx_ctx::FeatureTable &t = ctx->ft;
  t.have = false; ctx->dn.have = false;
  CoordSource cs;                                          // (the arrays go straight into the table's own buffers, below)
  { const int rc = coord_source(ctx, "itsx_trimmed_table", left_prefix, right_prefix, start, stop, nullptr, false, false, cs); if (rc != ITSX_OK) return rc; }
  const int64_t n = ctx->N;
  HIPCHK(t.start.alloc((size_t)n)); HIPCHK(t.stop.alloc((size_t)n));
  StageTimer tm(st);
  if (cs.by_prefix) launch_ft_coords(cs.start, cs.stop, cs.stride, n, t.start.p, t.stop.p, st);
  else { HIPCHK(hipMemcpyAsync(t.start.p, start, (size_t)n * 4, hipMemcpyHostToDevice, st)); HIPCHK(hipMemcpyAsync(t.stop.p, stop, (size_t)n * 4, hipMemcpyHostToDevice, st)); }
  // ---- 1 + 2: the table (a power of two, at least 2 n slots: never more than half full), and the exact verification
  uint64_t tsize = 1024; while (tsize < 2 * (uint64_t)n) tsize <<= 1;
  HIPCHK(t.keys.alloc((size_t)tsize)); HIPCHK(t.vals.alloc((size_t)tsize)); HIPCHK(t.hash.alloc((size_t)n)); HIPCHK(t.slot_of.alloc((size_t)n));
  HIPCHK(t.feature_read.alloc((size_t)n)); HIPCHK(t.counters.alloc(2)); HIPCHK(t.feature_of_read.alloc((size_t)n));
  HIPCHK(hipMemsetAsync(t.keys.p, 0, (size_t)tsize * 8, st)); HIPCHK(hipMemsetAsync(t.vals.p, 0x7f, (size_t)tsize * 4, st));
  HIPCHK(hipMemsetAsync(t.counters.p, 0, 16, st));
  FtArgs a{};
  a.rd = ctx->rd; a.start = t.start.p; a.stop = t.stop.p; a.min_len = min_len; a.sample = ctx->dev_sample();
  a.keys = t.keys.p; a.vals = t.vals.p; a.mask = tsize - 1; a.hash = t.hash.p; a.slot_of = t.slot_of.p; a.feature_read = t.feature_read.p; a.counters = t.counters.p;
  unsigned long long hc[2] = {0, 0};
  for (int round = 0;; round++) {                       // one round, unless two different sequences share a 64-bit hash
    launch_ft_insert(a, round, st);
    launch_ft_resolve(a, round, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hc, t.counters.p, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (hc[1] == 0) break;
    if (round >= 64) SET_ERR(ctx, ITSX_E_COLLISION, "itsx_trimmed_table: sequences still share a hash after 64 rounds of probing");
    HIPCHK(hipMemsetAsync(t.counters.p + 1, 0, 8, st));
  }
  const int64_t nc = (int64_t)hc[0];
  // ---- 3: (holder, sample) pairs, sorted; their runs; the features' order
  int sbits = 0; while (((int64_t)1 << sbits) < (int64_t)ctx->S) sbits++;
  int nbits = 1; while (((int64_t)1 << nbits) <= n) nbits++;
  const size_t sort_bytes = ft_sort_bytes(n);
  HIPCHK(t.sort_tmp.alloc(sort_bytes)); HIPCHK(t.pair_keys.alloc((size_t)n)); HIPCHK(t.pair_sorted.alloc((size_t)n));
  HIPCHK(t.ehead.alloc((size_t)nc + 1)); HIPCHK(t.epos.alloc((size_t)nc + 1)); HIPCHK(t.fhead.alloc((size_t)nc + 1)); HIPCHK(t.fpos.alloc((size_t)nc + 1));
  HIPCHK(t.scan.alloc((size_t)scan_tmp_elems(n + 1)));
  a.pair_keys = t.pair_keys.p; a.pair_sorted = t.pair_sorted.p; a.sbits = sbits; a.nc = nc;
  a.ehead = t.ehead.p; a.epos = t.epos.p; a.fhead = t.fhead.p; a.fpos = t.fpos.p;
  launch_ft_pairs(a, st);
  if (ft_sort_keys(t.sort_tmp.p, sort_bytes, t.pair_keys.p, t.pair_sorted.p, n, sbits + nbits, st) != 0) SET_ERR(ctx, ITSX_E_DEVICE, "itsx_trimmed_table: the pair sort failed");
  launch_ft_heads(a, st);
  launch_exclusive_scan(t.ehead.p, t.epos.p, nc + 1, t.scan.p, st);
  launch_exclusive_scan(t.fhead.p, t.fpos.p, nc + 1, t.scan.p, st);
  HIPCHK(hipGetLastError());
  int32_t EF[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&EF[0], t.epos.p + nc, 4, hipMemcpyDeviceToHost, st)); HIPCHK(hipMemcpyAsync(&EF[1], t.fpos.p + nc, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int32_t E = EF[0], F = EF[1];
  HIPCHK(t.ent_start.alloc((size_t)E + 1)); HIPCHK(t.ent_sample.alloc((size_t)E + 1)); HIPCHK(t.ent_feat.alloc((size_t)E + 1));
  HIPCHK(t.f_ent0.alloc((size_t)F + 1)); HIPCHK(t.f_pos0.alloc((size_t)F + 1)); HIPCHK(t.f_first.alloc((size_t)F + 1)); HIPCHK(t.hold_f.alloc((size_t)n));
  HIPCHK(t.okeys.alloc((size_t)F + 1)); HIPCHK(t.okeys2.alloc((size_t)F + 1)); HIPCHK(t.ovals.alloc((size_t)F + 1)); HIPCHK(t.ovals2.alloc((size_t)F + 1));
  HIPCHK(t.rank_of.alloc((size_t)F + 1)); HIPCHK(t.feat_len.alloc((size_t)F + 1)); HIPCHK(t.feat_total.alloc((size_t)F + 1)); HIPCHK(t.feat_first.alloc((size_t)F + 1));
  HIPCHK(t.nent.alloc((size_t)F + 1)); HIPCHK(t.row_off.alloc((size_t)F + 1)); HIPCHK(t.entry_sample.alloc((size_t)E + 1)); HIPCHK(t.entry_count.alloc((size_t)E + 1));
  a.ent_start = t.ent_start.p; a.ent_sample = t.ent_sample.p; a.ent_feat = t.ent_feat.p; a.f_ent0 = t.f_ent0.p; a.f_pos0 = t.f_pos0.p; a.f_first = t.f_first.p;
  a.hold_f = t.hold_f.p; a.E = E; a.F = F; a.okeys = t.okeys.p; a.okeys_sorted = t.okeys2.p; a.ovals = t.ovals.p; a.ovals_sorted = t.ovals2.p;
  a.rank_of = t.rank_of.p; a.feat_len = t.feat_len.p; a.feat_total = t.feat_total.p; a.feat_first = t.feat_first.p; a.nent = t.nent.p; a.row_off = t.row_off.p;
  a.entry_sample = t.entry_sample.p; a.entry_count = t.entry_count.p; a.feature_of_read = t.feature_of_read.p;
  launch_ft_runs(a, st);
  launch_ft_order_keys(a, st);
  if (ft_sort_pairs(t.sort_tmp.p, sort_bytes, t.okeys.p, t.okeys2.p, t.ovals.p, t.ovals2.p, F, st) != 0) SET_ERR(ctx, ITSX_E_DEVICE, "itsx_trimmed_table: the feature sort failed");
  launch_ft_ranked(a, st);
  launch_exclusive_scan(t.nent.p, t.row_off.p, (int64_t)F + 1, t.scan.p, st);
  launch_ft_entries(a, st);
  HIPCHK(hipGetLastError());
  // ---- 4: the representatives' sequences (their offsets are a 64-bit running sum of F lengths: made here, on the host)
  std::vector<int32_t> flen((size_t)F);
  if (F > 0) HIPCHK(hipMemcpyAsync(flen.data(), t.feat_len.p, (size_t)F * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  t.h_seq_off.assign((size_t)F + 1, 0);
  for (int32_t g = 0; g < F; g++) t.h_seq_off[(size_t)g + 1] = t.h_seq_off[(size_t)g] + flen[(size_t)g];
  t.text_bytes = t.h_seq_off[(size_t)F];
  HIPCHK(upload(t.seq_off, t.h_seq_off, st));
  HIPCHK(t.text.alloc((size_t)((t.text_bytes + 15) / 16) * 4 + 4));
  a.seq_off = t.seq_off.p; a.text = t.text.p; a.text_bytes = t.text_bytes;
  launch_ft_text(a, st);
  HIPCHK(hipGetLastError());
  const float ms = tm.stop();
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  t.have = true; t.n = n; t.nc = nc; t.F = F; t.E = E; t.S = ctx->S;
  if (n_features) *n_features = F;
  if (n_entries) *n_entries = E;
  if (n_counted) *n_counted = nc;
  if (ms_kernels) *ms_kernels = ms;
  return ITSX_OK;
}
int itsx_trimmed_table_get(itsx_ctx *ctx, int32_t *feat_len, int32_t *feat_total, int32_t *feat_first_read, int64_t *row_off, int32_t *entry_sample, int32_t *entry_count)
{
  CTXCHK(ctx);
  itsx_ctx::FeatureTable &t = ctx->ft;
  if (!t.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_trimmed_table_get: no table (call itsx_trimmed_table; a new read set drops it)");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const size_t F = (size_t)t.F, E = (size_t)t.E;
  std::vector<int32_t> ro(F + 1, 0);
  if (F && feat_len) HIPCHK(hipMemcpyAsync(feat_len, t.feat_len.p, F * 4, hipMemcpyDeviceToHost, st));
  if (F && feat_total) HIPCHK(hipMemcpyAsync(feat_total, t.feat_total.p, F * 4, hipMemcpyDeviceToHost, st));
  if (F && feat_first_read) HIPCHK(hipMemcpyAsync(feat_first_read, t.feat_first.p, F * 4, hipMemcpyDeviceToHost, st));
  if (F && row_off) HIPCHK(hipMemcpyAsync(ro.data(), t.row_off.p, (F + 1) * 4, hipMemcpyDeviceToHost, st));
  if (E && entry_sample) HIPCHK(hipMemcpyAsync(entry_sample, t.entry_sample.p, E * 4, hipMemcpyDeviceToHost, st));
  if (E && entry_count) HIPCHK(hipMemcpyAsync(entry_count, t.entry_count.p, E * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (row_off) for (size_t g = 0; g <= F; g++) row_off[g] = ro[g];
  return ITSX_OK;
}
int itsx_trimmed_table_size(itsx_ctx *ctx, int64_t *n_features, int64_t *n_entries, int64_t *n_counted)
{
  CTXCHK(ctx);
  itsx_ctx::FeatureTable &t = ctx->ft;
  if (!t.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_trimmed_table_size: no table (call itsx_trimmed_table; a new read set drops it)");
  if (n_features) *n_features = t.F;
  if (n_entries) *n_entries = t.E;
  if (n_counted) *n_counted = t.nc;
  return ITSX_OK;
}
int itsx_trimmed_table_reads(itsx_ctx *ctx, int32_t *feature_of_read)
{
  CTXCHK(ctx && feature_of_read);
  itsx_ctx::FeatureTable &t = ctx->ft;
  if (!t.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_trimmed_table_reads: no table (call itsx_trimmed_table; a new read set drops it)");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(feature_of_read, t.feature_of_read.p, (size_t)t.n * 4, hipMemcpyDeviceToHost, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  return ITSX_OK;
}
int itsx_trimmed_table_seqs(itsx_ctx *ctx, char *bases, int64_t *offsets)
{
  CTXCHK(ctx);
  itsx_ctx::FeatureTable &t = ctx->ft;
  if (!t.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_trimmed_table_seqs: no table (call itsx_trimmed_table; a new read set drops it)");
  if (offsets) memcpy(offsets, t.h_seq_off.data(), t.h_seq_off.size() * sizeof(int64_t));
  if (!bases) return ITSX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  return fetch_staged(ctx, reinterpret_cast<const uint8_t *>(t.text.p), t.text_bytes, bases);
}
// ------------------------------------------------------------------------------ the feature table denoised into ZOTUs (k_denoise.hip)
// The UNOISE rule (include/itsx_hip.h) on the table the last itsx_trimmed_table left in ctx->ft, level by level: per level the distance
// kernel, a scan of the new centroids and their append -- no host round trip between the levels -- then the collapse of the cells.
int itsx_denoise_table(itsx_ctx *ctx, const double *max_skew, int32_t n_diffs, int32_t minsize, int64_t *n_zotus, int64_t *n_entries,
                       int64_t *n_dropped_reads, int64_t *n_pairs, float *ms_kernels)
{
  CTXCHK(ctx);
  itsx_ctx::FeatureTable &t = ctx->ft;
  itsx_ctx::Denoised &d = ctx->dn;
  d.have = false;
  if (!t.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_denoise_table: no table (call itsx_trimmed_table; a new read set drops it)");
  if (n_diffs < 0 || n_diffs > DN_MAX_DIFFS) SET_ERR(ctx, ITSX_E_ARG, "itsx_denoise_table: n_diffs must be 0 .. 31, not " + std::to_string(n_diffs));
  if (n_diffs > 0 && !max_skew) SET_ERR(ctx, ITSX_E_ARG, "itsx_denoise_table: n_diffs > 0 without max_skew");
  if (minsize < 1) SET_ERR(ctx, ITSX_E_ARG, "itsx_denoise_table: minsize must be at least 1, not " + std::to_string(minsize));
  std::vector<double> skew(32, 0.0);
  for (int32_t i = 0; i < n_diffs; i++) {
    if (!(max_skew[i] > 0.0 && max_skew[i] < 1.0)) SET_ERR(ctx, ITSX_E_ARG, "itsx_denoise_table: max_skew[" + std::to_string(i) + "] is not inside (0, 1)");
    if (i > 0 && max_skew[i] > max_skew[i - 1]) SET_ERR(ctx, ITSX_E_ARG, "itsx_denoise_table: max_skew[" + std::to_string(i) + "] is above the entry before it");
    skew[(size_t)i] = max_skew[i];
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const int32_t F = t.F, E = t.E;
  int sbits = 0; while (((int64_t)1 << sbits) < (int64_t)t.S) sbits++;
  HIPCHK(upload(d.skew, skew, st));
  HIPCHK(d.lv.alloc((size_t)F + 1)); HIPCHK(d.nlev.alloc(1)); HIPCHK(d.ncent.alloc((size_t)F + 2)); HIPCHK(d.cent.alloc((size_t)F + 1));
  HIPCHK(d.zotu_of.alloc((size_t)F + 1)); HIPCHK(d.dist_of.alloc((size_t)F + 1)); HIPCHK(d.flag.alloc((size_t)F + 1)); HIPCHK(d.pos.alloc((size_t)F + 1));
  HIPCHK(d.counters.alloc(DN_COUNTERS)); HIPCHK(d.scan.alloc((size_t)scan_tmp_elems(std::max<int64_t>(F, E) + 1)));
  HIPCHK(d.keys.alloc((size_t)E + 1)); HIPCHK(d.keys2.alloc((size_t)E + 1)); HIPCHK(d.vals.alloc((size_t)E + 1)); HIPCHK(d.vals2.alloc((size_t)E + 1));
  HIPCHK(d.head.alloc((size_t)E + 1)); HIPCHK(d.hpos.alloc((size_t)E + 1)); HIPCHK(d.csum.alloc((size_t)E + 1)); HIPCHK(d.run_start.alloc((size_t)E + 1));
  HIPCHK(d.z_row_off.alloc((size_t)F + 1)); HIPCHK(d.z_total.alloc((size_t)F + 1)); HIPCHK(d.z_entry_sample.alloc((size_t)E + 1)); HIPCHK(d.z_entry_count.alloc((size_t)E + 1));
  const size_t sort_bytes = ft_sort_bytes(std::max<int64_t>(E, 1));
  HIPCHK(d.sort_tmp.alloc(sort_bytes));
  StageTimer tm(st);
  HIPCHK(hipMemsetAsync(d.counters.p, 0, DN_COUNTERS * 8, st));
  DnArgs a{};
  a.F = F; a.feat_total = t.feat_total.p; a.feat_len = t.feat_len.p; a.seq_off = t.seq_off.p; a.text = t.text.p;
  a.row_off = t.row_off.p; a.entry_sample = t.entry_sample.p; a.entry_count = t.entry_count.p; a.E = E; a.sbits = sbits;
  a.max_skew = d.skew.p; a.D = n_diffs; a.minsize = minsize;
  a.lv = d.lv.p; a.nlev = d.nlev.p; a.cent = d.cent.p; a.ncent = d.ncent.p; a.zotu_of = d.zotu_of.p; a.dist_of = d.dist_of.p;
  a.flag = d.flag.p; a.pos = d.pos.p; a.counters = d.counters.p;
  a.keys = d.keys.p; a.keys_sorted = d.keys2.p; a.vals = d.vals.p; a.vals_sorted = d.vals2.p; a.head = d.head.p; a.hpos = d.hpos.p; a.csum = d.csum.p; a.run_start = d.run_start.p;
  a.z_row_off = d.z_row_off.p; a.z_total = d.z_total.p; a.z_entry_sample = d.z_entry_sample.p; a.z_entry_count = d.z_entry_count.p;
  // ---- the levels (their number is at most F; with UNOISE's skews about one per factor 8 of abundance)
  launch_dn_levels(a, st);
  HIPCHK(hipGetLastError());
  int32_t nlev = 0;
  HIPCHK(hipMemcpyAsync(&nlev, d.nlev.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<int32_t> lv((size_t)nlev + 1, 0);
  HIPCHK(hipMemcpyAsync(lv.data(), d.lv.p, ((size_t)nlev + 1) * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int32_t l = 0; l < nlev; l++) {
    const int32_t f0 = lv[(size_t)l], f1 = lv[(size_t)l + 1];
    launch_dn_distance(a, l, f0, f1, st);
    launch_exclusive_scan(d.flag.p, d.pos.p, (int64_t)(f1 - f0) + 1, d.scan.p, st);
    launch_dn_append(a, l, f0, f1, st);
  }
  HIPCHK(hipGetLastError());
  int32_t Z = 0;
  HIPCHK(hipMemcpyAsync(&Z, d.ncent.p + nlev, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // ---- the collapse: a ZOTU's row is the sample-wise sum of its members' rows
  a.Z = Z;
  launch_dn_keys(a, st);
  if (ft_sort_pairs(d.sort_tmp.p, sort_bytes, d.keys.p, d.keys2.p, d.vals.p, d.vals2.p, E, st) != 0) SET_ERR(ctx, ITSX_E_DEVICE, "itsx_denoise_table: the cell sort failed");
  launch_dn_heads(a, st);
  launch_exclusive_scan(d.head.p, d.hpos.p, (int64_t)E + 1, d.scan.p, st);
  launch_exclusive_scan(d.vals2.p, d.csum.p, (int64_t)E + 1, d.scan.p, st);
  launch_dn_runs(a, st);
  launch_dn_rows(a, st);
  HIPCHK(hipGetLastError());
  int32_t Ez = 0; unsigned long long hc[DN_COUNTERS] = {0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(&Ez, d.hpos.p + E, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hc, d.counters.p, DN_COUNTERS * 8, hipMemcpyDeviceToHost, st));
  const float ms = tm.stop();
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  d.F = F; d.Z = Z; d.E = Ez; d.levels = nlev;
  d.pairs = (int64_t)hc[DN_C_PAIRS]; d.skip_skew = (int64_t)hc[DN_C_SKIP_SKEW]; d.skip_len = (int64_t)hc[DN_C_SKIP_LEN]; d.dropped = (int64_t)hc[DN_C_DROPPED]; d.columns = (int64_t)hc[DN_C_COLUMNS];
  d.have = true;
  if (n_zotus) *n_zotus = Z;
  if (n_entries) *n_entries = Ez;
  if (n_dropped_reads) *n_dropped_reads = d.dropped;
  if (n_pairs) *n_pairs = d.pairs;
  if (ms_kernels) *ms_kernels = ms;
  return ITSX_OK;
}
int itsx_denoise_table_get(itsx_ctx *ctx, int32_t *zotu_feature, int32_t *zotu_total, int64_t *row_off, int32_t *entry_sample, int32_t *entry_count)
{
  CTXCHK(ctx);
  itsx_ctx::Denoised &d = ctx->dn;
  if (!d.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_denoise_table_get: no denoised table (call itsx_denoise_table; a new table or read set drops it)");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const size_t Z = (size_t)d.Z, E = (size_t)d.E;
  std::vector<int32_t> ro(Z + 1, 0);
  if (Z && zotu_feature) HIPCHK(hipMemcpyAsync(zotu_feature, d.cent.p, Z * 4, hipMemcpyDeviceToHost, st));
  if (Z && zotu_total) HIPCHK(hipMemcpyAsync(zotu_total, d.z_total.p, Z * 4, hipMemcpyDeviceToHost, st));
  if (Z && row_off) HIPCHK(hipMemcpyAsync(ro.data(), d.z_row_off.p, (Z + 1) * 4, hipMemcpyDeviceToHost, st));
  if (E && entry_sample) HIPCHK(hipMemcpyAsync(entry_sample, d.z_entry_sample.p, E * 4, hipMemcpyDeviceToHost, st));
  if (E && entry_count) HIPCHK(hipMemcpyAsync(entry_count, d.z_entry_count.p, E * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (row_off) for (size_t z = 0; z <= Z; z++) row_off[z] = ro[z];
  return ITSX_OK;
}
int itsx_denoise_table_features(itsx_ctx *ctx, int32_t *zotu_of_feature, int32_t *dist_of_feature)
{
  CTXCHK(ctx);
  itsx_ctx::Denoised &d = ctx->dn;
  if (!d.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_denoise_table_features: no denoised table (call itsx_denoise_table; a new table or read set drops it)");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const size_t F = (size_t)d.F;
  if (F && zotu_of_feature) HIPCHK(hipMemcpyAsync(zotu_of_feature, d.zotu_of.p, F * 4, hipMemcpyDeviceToHost, st));
  if (F && dist_of_feature) HIPCHK(hipMemcpyAsync(dist_of_feature, d.dist_of.p, F * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return ITSX_OK;
}
int itsx_denoise_table_info(itsx_ctx *ctx, int64_t *n_levels, int64_t *n_skipped_skew, int64_t *n_skipped_length, int64_t *n_columns)
{
  CTXCHK(ctx);
  itsx_ctx::Denoised &d = ctx->dn;
  if (!d.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_denoise_table_info: no denoised table (call itsx_denoise_table; a new table or read set drops it)");
  if (n_levels) *n_levels = d.levels;
  if (n_skipped_skew) *n_skipped_skew = d.skip_skew;
  if (n_skipped_length) *n_skipped_length = d.skip_len;
  if (n_columns) *n_columns = d.columns;
  return ITSX_OK;
}
// f1 for a batch of PAIRED samples: Dedup.create_paired_trimmed_seqs (SeqSample.py:564-790) of every sample in one call, from the pair
// records the context keeps (itsx_keep_pair_records).  One plan for both sides; then per side the copy kernel with that side's planes and
// the text's way back to the files, R1's first.
int itsx_write_trimmed_paired_samples(itsx_ctx *ctx, const char *const *out1_paths, const char *const *out2_paths, int32_t n_samples, int compression,
                                      int trim_ccs, const char *left_prefix, const char *right_prefix, const int32_t *start, const int32_t *stop,
                                      const int32_t *tlen, int64_t *n_written_per_sample)
{
  CTXCHK(ctx && out1_paths && out2_paths);
  const itsx_ctx::PairRecords &pr = ctx->prec;
  // (SampleBatch.write_paired_trimmed falls back to the host writer when this message names itsx_keep_pair_records: keep the name in it)
  if (!pr.have) SET_ERR(ctx, ITSX_E_ARG, "itsx_write_trimmed_paired_samples: the read set keeps no pair records; call itsx_keep_pair_records(ctx, 1) before the pairs are merged (pairs with lower-case bases keep none)");
  if (n_samples != ctx->S || (size_t)n_samples + 1 != pr.pstart.size())
    SET_ERR(ctx, ITSX_E_ARG, "itsx_write_trimmed_paired_samples: " + std::to_string(n_samples) + " pairs of output paths for " + std::to_string(ctx->S) + " sample(s)");
  for (int32_t s = 0; s < n_samples; s++)
    if ((out1_paths[s] == nullptr) != (out2_paths[s] == nullptr)) SET_ERR(ctx, ITSX_E_ARG, "itsx_write_trimmed_paired_samples: sample " + std::to_string(s) + " has one output path of its two");
  if (compression < 0 || compression > 3) SET_ERR(ctx, ITSX_E_ARG, "compression must be 0 (plain), 1 (gzip), 2 (zstd) or 3 (gzip, deflated on the device)");
  if (compression == 1 && device_deflate_switch()) compression = 3;
  CoordSource cs;
  { const int rc = coord_source(ctx, "itsx_write_trimmed_paired_samples", left_prefix, right_prefix, start, stop, tlen, true, true, cs); if (rc != ITSX_OK) return rc; }
  if (compression != 3) { itsx_io::PieceCompressor probe(compression); if (!probe.ok()) SET_ERR(ctx, ITSX_E_IO, "zstd output requested but libzstd.so.1 could not be loaded"); }
  hipStream_t st = ctx->st;
  const int64_t nr = ctx->N, n = pr.n; const int32_t S = ctx->S;
  TrimPairPlanArgs pa{};
  pa.start = cs.start; pa.stop = cs.stop; pa.tlen = cs.tlen; pa.stride = cs.stride;
  std::vector<int64_t> bounds((size_t)(S + 1) * 3, 0);
  HIPCHK(upload(ctx->w_tfirst, pr.pstart, st));          // sample s is pairs [pstart[s], pstart[s + 1])
  HIPCHK(ctx->w_trec.alloc((size_t)n + 1)); HIPCHK(ctx->w_trec2.alloc((size_t)n + 1)); HIPCHK(ctx->w_tcnt.alloc((size_t)n + 1));
  HIPCHK(ctx->w_tblk.alloc((size_t)trim_plan_blocks(n) * 3 + 3)); HIPCHK(ctx->w_tbounds.alloc(bounds.size()));
  pa.pair_read = pr.pair_read.p; pa.n_reads = nr; pa.off1 = pr.o1.p; pa.toff1 = pr.to1.p; pa.off2 = pr.o2.p; pa.toff2 = pr.to2.p;
  pa.n = n; pa.ccs = trim_ccs ? 1 : 0;
  pa.blk = ctx->w_tblk.p; pa.rec1 = ctx->w_trec.p; pa.rec2 = ctx->w_trec2.p; pa.cnt = ctx->w_tcnt.p;
  {
    StageTimer tm(st);
    launch_trim_pair_plan(pa, ctx->w_tfirst.p, S, ctx->w_tbounds.p, st);
    ctx->stats.ms_trim_plan = tm.stop();
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(bounds.data(), ctx->w_tbounds.p, bounds.size() * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t *bc = bounds.data() + 2 * (S + 1);
  HIPCHK(ctx->w_tout.alloc((size_t)(trim_copy_bytes(std::max(bounds[(size_t)S], bounds[(size_t)(S + 1) + (size_t)S])) / 4) + 16));
  ctx->stats.ms_trim_copy = 0;
  for (int side = 0; side < 2; side++) {
    const int64_t *bo = bounds.data() + (size_t)side * (size_t)(S + 1);
    TrimCopyArgs ca{};
    ca.rec = side ? ctx->w_trec2.p : ctx->w_trec.p; ca.n = n;
    ca.seq = side ? pr.s2.p : pr.s1.p; ca.qual = side ? pr.q2.p : pr.q1.p; ca.titles = side ? pr.t2.p : pr.t1.p;
    ca.total = bo[S]; ca.ccs = pa.ccs; ca.out = ctx->w_tout.p;
    {
      StageTimer tm(st);
      launch_trim_copy(ca, st);
      ctx->stats.ms_trim_copy += tm.stop();
    }
    HIPCHK(hipGetLastError());
    const int rc = trim_text_to_files(ctx, ca.total, bo, side ? out2_paths : out1_paths, compression);
    if (rc != ITSX_OK) {                                   // R1's files come first: a failed call leaves no half of a pair of files behind
      for (int32_t s = 0; s < S; s++) if (out1_paths[s]) { (void)remove(out1_paths[s]); (void)remove(out2_paths[s]); }
      return rc;
    }
  }
  if (n_written_per_sample) for (int32_t s = 0; s < S; s++) n_written_per_sample[s] = bc[s + 1] - bc[s];
  return ITSX_OK;
}
// ---- the device deflate by itself
int64_t itsx_deflate_block_bytes(void) { return DEFLATE_BLOCK_BYTES; }
int64_t itsx_deflate_bound(int64_t nbytes, int32_t n_ranges) { return deflate_bound(std::max<int64_t>(nbytes, 0), std::max<int32_t>(n_ranges, 0)); }
int itsx_deflate_device(itsx_ctx *ctx, const char *text, int64_t nbytes, const int64_t *bounds, int32_t n_ranges, char *out, int64_t out_cap,
                        int64_t *out_bounds)
{
  CTXCHK(ctx && bounds && out_bounds && n_ranges >= 0 && nbytes >= 0 && (text || nbytes == 0) && (out || out_cap == 0));
  if (n_ranges > 0 && (bounds[0] != 0 || bounds[n_ranges] != nbytes)) SET_ERR(ctx, ITSX_E_ARG, "itsx_deflate_device: bounds must run from 0 to nbytes");
  for (int32_t r = 0; r < n_ranges; r++) if (bounds[r] > bounds[r + 1]) SET_ERR(ctx, ITSX_E_ARG, "itsx_deflate_device: bounds must not decrease");
  if (out_cap < itsx_deflate_bound(nbytes, n_ranges)) SET_ERR(ctx, ITSX_E_ARG, "itsx_deflate_device: out_cap is below itsx_deflate_bound(nbytes, n_ranges)");
  HIPCHK(hipSetDevice(ctx->device));
  out_bounds[0] = 0;
  if (n_ranges == 0) return ITSX_OK;
  HIPCHK(ctx->w_dtext.alloc((size_t)(nbytes / 4) + 16));
  if (nbytes > 0) HIPCHK(hipMemcpyAsync(ctx->w_dtext.p, text, (size_t)nbytes, hipMemcpyHostToDevice, ctx->st));
  std::vector<std::pair<int64_t, int64_t>> ranges;
  for (int32_t r = 0; r < n_ranges; r++) ranges.emplace_back(bounds[r], bounds[r + 1]);
  std::vector<char> z; std::vector<int64_t> zb;
  { const int rc = deflate_ranges(ctx, reinterpret_cast<const uint8_t *>(ctx->w_dtext.p), ranges, z, zb); if (rc != ITSX_OK) return rc; }
  if ((int64_t)z.size() > out_cap) SET_ERR(ctx, ITSX_E_DEVICE, "the device deflate went past its bound");
  if (!z.empty()) memcpy(out, z.data(), z.size());
  for (int32_t r = 0; r <= n_ranges; r++) out_bounds[r] = zb[(size_t)r];
  return ITSX_OK;
}
// ---- a streamed writer's device path (twriter_dev.h; the writer object itself is trim_host.cpp's)
}  // extern "C"
// nbytes of host memory to the device through the pinned staging buffers, in pieces: a piece is copied into its buffer while the one
// before it is on the bus (a pageable copy of a text moves at ~5 GB/s, the staged one at ~35)
static int put_staged(itsx_ctx *ctx, const char *src, int64_t total, uint8_t *ddst)
{
  if (total <= 0) return ITSX_OK;
  { const int rc = stage_reserve(ctx, 4 << 20); if (rc != ITSX_OK) return rc; }
  const int64_t piece = std::min<int64_t>((int64_t)ctx->stage_cap, 4 << 20);
  constexpr int K = itsx_ctx::NSTAGE;
  for (int64_t c = 0, o = 0; o < total; c++, o += piece) {
    const int64_t b = std::min(piece, total - o);
    HIPCHK(hipEventSynchronize(ctx->stage_ev[c % K]));      // what this buffer held last is on the device (an event never recorded: no wait)
    memcpy(ctx->stage_pin[c % K], src + o, (size_t)b);
    HIPCHK(hipMemcpyAsync(ddst + o, ctx->stage_pin[c % K], (size_t)b, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipEventRecord(ctx->stage_ev[c % K], ctx->st));
  }
  return ITSX_OK;
}
// ------------------------------------------------------------------------------ gzip members inflated on the device (k_inflate.hip)
// A gzip file made of independent members (this project's writers', bgzip's, any cat a.gz b.gz): the bytes go up through the pinned
// staging buffers, k_inflate_find lists the positions that pass the strict member-start test, the list IS the plan -- member i spans
// [c_i, c_i+1), its ISIZE is its span's last 4 bytes (read from the caller's copy: four bytes a member, no walk), the text offsets are
// the 64-bit scan of the ISIZEs -- and k_inflate decodes one member per wave, longest spans first.  Every member verifies its own
// length, CRC-32 and ISIZE; one refusal declines the whole file (ITSX_E_UNSUPPORTED, the reason and the member named), as do a file
// whose byte 0 is no member start, a member longer than ITSX_INFLATE_MEMBER_KB (it would be one wave's serial work), more text than
// deflate can expand to, and a text that cannot be allocated.  A decline leaves no text behind.  stats.ms_inflate: the kernels' time.
static bool device_inflate_on(const itsx_ctx *ctx) { const char *e = sw_get("ITSX_DEVICE_INFLATE"); return ctx->device_inflate || (e && atoi(e) == 1); }
static int64_t inflate_member_cap()
{
  const char *e = sw_get("ITSX_INFLATE_MEMBER_KB");
  const long long kb = e ? atoll(e) : 8192;                  // twice the host writer's 4 MiB block of text: its members always pass
  return (int64_t)std::min<long long>(std::max<long long>(kb, 1), 2097151) * 1024;      // (a stored run's offset is 32 bits)
}
static int inflate_file(itsx_ctx *ctx, const char *gz, int64_t nbytes, int64_t *text_len, int64_t *n_members)
{
  using namespace itsx_ic;
  hipStream_t st = ctx->st;
  ctx->inf_len = -1; ctx->stats.ms_inflate = 0; ctx->stats.n_inflate_members = 0;
  auto decline = [&](int32_t why, int64_t member, const std::string &more = std::string()) {
    ctx->n_inf_declined++;
    ctx->set_error(std::string("the device inflate declined the file: ") + ic_reason_name(why) + (member >= 0 ? " (member " + std::to_string(member) + ")" : std::string()) + more);
    return (int)ITSX_E_UNSUPPORTED;
  };
  const uint8_t *g = reinterpret_cast<const uint8_t *>(gz);
  if (nbytes < 2 || g[0] != 0x1f || g[1] != 0x8b) return decline(IC_E_NOT_GZIP, -1);
  if (nbytes < IC_MIN_MEMBER) return decline(IC_E_INPUT, 0);
  // byte 0 is no member start: the reason its header gives (these few bytes are read here, nothing is walked), else just that
  auto first_reason = [&]() { int32_t why = IC_OK; (void)ic_header(g, nbytes, &why); return why ? why : (int32_t)IC_E_FIRST; };
  // device memory that cannot be had is a decline like any other ("no memory"), whichever buffer it is
  auto room = [&](hipError_t e) { if (e != hipSuccess) { (void)hipGetLastError(); } return e == hipSuccess; };
  // ---- up, and the member starts
  if (!room(ctx->inf_gz.alloc((size_t)nbytes + 16))) return decline(IC_E_NOMEM, -1, ": the file's " + std::to_string(nbytes) + " bytes");
  { const int rc = put_staged(ctx, gz, nbytes, ctx->inf_gz.p); if (rc != ITSX_OK) return rc; }
  const int64_t ntiles = (nbytes + INFLATE_FIND_TILE - 1) / INFLATE_FIND_TILE;
  if (!room(ctx->inf_counts.alloc((size_t)ntiles)) || !room(ctx->inf_base.alloc((size_t)ntiles + 1))) return decline(IC_E_NOMEM, -1, ": the member search");
  int64_t M = 0;
  {
    StageTimer tm(st);
    launch_inflate_find(ctx->inf_gz.p, nbytes, ctx->inf_counts.p, nullptr, nullptr, st);
    launch_inflate_scan(ctx->inf_counts.p, ntiles, ctx->inf_base.p, ctx->inf_base.p + ntiles, st);
    ctx->stats.ms_inflate += tm.stop();
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&M, ctx->inf_base.p + ntiles, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (M <= 0) return decline(first_reason(), -1);
  if (M > 0x7fffffff) return decline(IC_E_NOMEM, -1, ": more than 2^31 members");
  if (!room(ctx->inf_list.alloc((size_t)M))) return decline(IC_E_NOMEM, -1, ": the list of " + std::to_string(M) + " members");
  {
    StageTimer tm(st);
    launch_inflate_find(ctx->inf_gz.p, nbytes, ctx->inf_counts.p, ctx->inf_base.p, ctx->inf_list.p, st);
    ctx->stats.ms_inflate += tm.stop();
  }
  HIPCHK(hipGetLastError());
  std::vector<int64_t> start((size_t)M + 1);
  HIPCHK(hipMemcpyAsync(start.data(), ctx->inf_list.p, (size_t)M * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  start[(size_t)M] = nbytes;
  if (start[0] != 0) return decline(first_reason(), -1);
  // ---- the plan
  const int64_t cap = inflate_member_cap();
  std::vector<InflateMember> mem((size_t)M);
  int64_t total = 0;
  for (int64_t i = 0; i < M; i++) {
    const int64_t c = start[(size_t)i], ce = start[(size_t)i + 1];
    if (c < 0 || ce <= c || ce > nbytes) SET_ERR(ctx, ITSX_E_DEVICE, "the device inflate's member list is not increasing");
    if (ce - c < IC_MIN_MEMBER) return decline(IC_E_INPUT, i);
    if (ce - c > cap) return decline(IC_E_MEMBER_LONG, i, ": " + std::to_string(ce - c) + " compressed bytes, the cap (ITSX_INFLATE_MEMBER_KB) is " + std::to_string(cap));
    const uint8_t *q = g + ce - 4;
    const uint32_t isize = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    mem[(size_t)i] = InflateMember{c, ce, total, isize, (int32_t)i};
    total += isize;
    if (total > 1032 * nbytes + 64 * M) return decline(IC_E_EXPANSION, i);
  }
  if (!room(ctx->inf_text.alloc((size_t)total + 16))) return decline(IC_E_NOMEM, -1, ": the text's " + std::to_string(total) + " bytes");
  std::stable_sort(mem.begin(), mem.end(), [](const InflateMember &x, const InflateMember &y) { return x.c_end - x.c > y.c_end - y.c; });
  if (!room(ctx->inf_mem.alloc((size_t)M)) || !room(ctx->inf_status.alloc((size_t)M)) || !room(ctx->inf_where.alloc((size_t)M))) return decline(IC_E_NOMEM, -1, ": the plan of " + std::to_string(M) + " members");
  HIPCHK(hipMemcpyAsync(ctx->inf_mem.p, mem.data(), (size_t)M * sizeof(InflateMember), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(ctx->inf_status.p, 0xff, (size_t)M * 4, st));        // a member no workgroup reached is not a verified one
  int ncu = 256;
  { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, ctx->device) == hipSuccess && pr.multiProcessorCount > 0) ncu = pr.multiProcessorCount; }
  InflateArgs ia{};
  ia.gz = ctx->inf_gz.p; ia.mem = ctx->inf_mem.p; ia.nmem = (int32_t)M; ia.text = ctx->inf_text.p; ia.status = ctx->inf_status.p; ia.where = ctx->inf_where.p;
  int64_t grid = std::min<int64_t>(M, (int64_t)ncu * 4);                               // four workgroups' LDS fit a CU
  if (const char *e = sw_get("ITSX_INFLATE_GRID")) grid = std::max<int64_t>(1, std::min<int64_t>(grid, atoll(e)));
  {
    StageTimer tm(st);
    launch_inflate(ia, (int)grid, st);
    ctx->stats.ms_inflate += tm.stop();
  }
  HIPCHK(hipGetLastError());
  std::vector<int32_t> status((size_t)M);
  HIPCHK(hipMemcpyAsync(status.data(), ctx->inf_status.p, (size_t)M * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < M; i++) if (status[(size_t)i] != 0) return decline(status[(size_t)i], i);
  ctx->inf_len = total; ctx->n_inf_device++; ctx->stats.n_inflate_members = (int32_t)M;
  if (text_len) *text_len = total;
  if (n_members) *n_members = M;
  return ITSX_OK;
}
// read_text's "try this inflater first" for a context that opted in: false = the host path continues exactly as without it
static bool inflate_for_loader(itsx_ctx *ctx, const itsx_io::Text &raw, itsx_io::Text &out)
{
  std::lock_guard<std::mutex> g(ctx->inf_mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return false;
  int64_t n = 0;
  if (inflate_file(ctx, raw.data(), (int64_t)raw.size(), &n, nullptr) != ITSX_OK) return false;
  if (!out.resize((size_t)n)) return false;
  return fetch_staged(ctx, ctx->inf_text.p, n, out.data()) == ITSX_OK;
}
extern "C" {
int itsx_inflate_device(itsx_ctx *ctx, const char *gz, int64_t nbytes, int64_t *text_len, int64_t *n_members)
{
  CTXCHK(ctx && gz && nbytes >= 0);
  std::lock_guard<std::mutex> g(ctx->inf_mu);
  HIPCHK(hipSetDevice(ctx->device));
  return inflate_file(ctx, gz, nbytes, text_len, n_members);
}
int itsx_inflate_fetch(itsx_ctx *ctx, char *out, int64_t out_cap)
{
  CTXCHK(ctx);
  std::lock_guard<std::mutex> g(ctx->inf_mu);
  if (ctx->inf_len < 0) SET_ERR(ctx, ITSX_E_ARG, "itsx_inflate_fetch: no text (the last itsx_inflate_device did not succeed, or there was none)");
  if (out_cap < ctx->inf_len || (!out && ctx->inf_len > 0)) SET_ERR(ctx, ITSX_E_ARG, "itsx_inflate_fetch: out_cap is below the text's " + std::to_string(ctx->inf_len) + " bytes");
  HIPCHK(hipSetDevice(ctx->device));
  return fetch_staged(ctx, ctx->inf_text.p, ctx->inf_len, out);
}
int itsx_set_device_inflate(itsx_ctx *ctx, int on)
{
  CTXCHK(ctx);
  ctx->device_inflate = on != 0;
  return ITSX_OK;
}
int itsx_debug_inflate_where(itsx_ctx *ctx, int64_t *where, int64_t n)
{
  CTXCHK(ctx && where && n >= 0);
  std::lock_guard<std::mutex> g(ctx->inf_mu);
  if (ctx->inf_len < 0 || n != (int64_t)ctx->stats.n_inflate_members) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_inflate_where: n is not the member count of a successful itsx_inflate_device");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(where, ctx->inf_where.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  return ITSX_OK;
}
int64_t itsx_debug_inflate_candidates(const char *gz, int64_t nbytes, int64_t *positions, int64_t cap)
{
  if (!gz || nbytes < 0 || cap < 0 || (!positions && cap > 0)) return ITSX_E_ARG;
  int64_t n = 0;
  for (int64_t at = 0; at < nbytes; at++)
    if (itsx_ic::ic_candidate(reinterpret_cast<const uint8_t *>(gz), nbytes, at)) { if (n < cap) positions[n] = at; n++; }
  return n;
}
int itsx_debug_inflate_host(const char *gz, int64_t nbytes, char *out, int64_t out_cap, int64_t *text_len, int64_t *n_members, int32_t *reason)
{
  if (!gz || nbytes < 0 || out_cap < 0 || (!out && out_cap > 0) || !text_len || !n_members || !reason) return ITSX_E_ARG;
  std::unique_ptr<itsx_ic::IcHostScratch> w(new (std::nothrow) itsx_ic::IcHostScratch);
  if (!w) return ITSX_E_NOMEM;
  *reason = itsx_ic::ic_inflate_file_host(reinterpret_cast<const uint8_t *>(gz), nbytes, reinterpret_cast<uint8_t *>(out), out_cap, text_len, n_members, *w);
  return *reason ? ITSX_E_UNSUPPORTED : ITSX_OK;
}
}  // extern "C"
// ------------------------------------------------------------------------------ FASTQ text parsed on the device (k_fastq.hip)
// A text that lies in device memory (the device inflate's, or one uploaded once through the staging buffers): k_fastq.hip counts and
// indexes its lines, checks every record by fastq_rec.h's rule and measures it, and gathers bases, qualities (where they are kept) and
// title lines into the context's planes behind what earlier texts of the same call left there.  Two small reads come back in between
// (the line count; the verdict and the totals), nothing of the text.  A text the rule does not accept is DECLINED (ITSX_E_UNSUPPORTED,
// the reason and the record named), as is one whose index or planes cannot be allocated.  stats.ms_parse: the kernels' time.
static bool device_parse_on(const itsx_ctx *ctx) { const char *e = sw_get("ITSX_DEVICE_PARSE"); return ctx->device_parse || (e && atoi(e) == 1); }
struct ParsedText { int64_t n = 0, nb = 0, nt = 0; };      // records, bases, title bytes
// room for `need` bytes (and the padding every plane has) in a plane whose first `used` bytes are kept
static hipError_t plane_room(DBuf<uint8_t> &d, int64_t used, int64_t need, hipStream_t st)
{
  if (d.p && (size_t)need + 64 <= d.cap) { d.n = (size_t)need + 64; return hipSuccess; }
  DBuf<uint8_t> nd;
  hipError_t e = hipErrorOutOfMemory;
  if (used > 0) e = nd.alloc(std::max((size_t)need + 64, 2 * d.cap), true);      // a batch's planes grow file by file: doubled
  if (e != hipSuccess) { (void)hipGetLastError(); e = nd.alloc((size_t)need + 64, true); }
  if (e != hipSuccess) return e;
  if (used > 0) e = hipMemcpyAsync(nd.p, d.p, (size_t)used, hipMemcpyDeviceToDevice, st);
  dbuf_swap(d, nd);
  return e;
}
static int parse_text_device(itsx_ctx *ctx, const uint8_t *dtext, int64_t nbytes, bool keep_qual, int64_t gb, int64_t gt, ParsedText &out)
{
  using namespace itsx_fq;
  hipStream_t st = ctx->st;
  out = ParsedText();
  auto decline = [&](int32_t why, int64_t rec, const std::string &more = std::string()) {
    ctx->n_parse_declined++;
    ctx->set_error(std::string("the device parse declined the text: ") + fq_reason_name(why) + (rec >= 0 ? " (record " + std::to_string(rec) + ")" : std::string()) + more);
    return (int)ITSX_E_UNSUPPORTED;
  };
  auto room = [&](hipError_t e) { if (e != hipSuccess) { (void)hipGetLastError(); } return e == hipSuccess; };
  if (nbytes == 0) { ctx->n_parse_device++; return ITSX_OK; }                  // no bytes: no lines, no records
  FastqArgs a{};
  a.text = dtext; a.nbytes = nbytes;
  if (!room(ctx->ps_lblk.alloc((size_t)fastq_index_blocks(nbytes) + 1)) || !room(ctx->ps_info.alloc(FASTQ_INFO))) return decline(FQ_E_NOMEM, -1, ": the line count");
  a.lblk = ctx->ps_lblk.p; a.info = ctx->ps_info.p;
  int64_t info[FASTQ_INFO] = {0, 0, 0, 0, 0, 0, 0, 0};
  {
    StageTimer tm(st);
    launch_fastq_count(a, st);
    ctx->stats.ms_parse += tm.stop();
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(info, ctx->ps_info.p, 2 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t lines = info[0], nnl = info[1];
  if (lines <= 0 || lines % 4 != 0 || nnl < lines - 1 || nnl > lines) return decline(FQ_E_LINES, -1, ": " + std::to_string(lines) + " lines");
  const int64_t n = lines / 4;
  if (n >= (1ll << 31) - 64) return decline(FQ_E_NOMEM, -1, ": more than 2^31 records");
  if (!room(ctx->ps_nl.alloc((size_t)lines + 1)) || !room(ctx->ps_blk.alloc((size_t)(2 * fastq_plan_blocks(n) + 2))) || !room(ctx->ps_off.alloc((size_t)n + 1)) ||
      !room(ctx->ps_toff.alloc((size_t)n + 1))) return decline(FQ_E_NOMEM, -1, ": the index of " + std::to_string(lines) + " lines");
  a.nl = ctx->ps_nl.p; a.nlines = lines; a.nnl = nnl; a.n = n; a.blk = ctx->ps_blk.p; a.off = ctx->ps_off.p; a.toff = ctx->ps_toff.p;
  {
    StageTimer tm(st);
    launch_fastq_index(a, st);
    launch_fastq_plan(a, st);
    ctx->stats.ms_parse += tm.stop();
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(info, ctx->ps_info.p, sizeof(info), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const unsigned long long verdict = (unsigned long long)info[4];
  if (verdict != FQ_VERDICT_NONE) return decline((int32_t)(verdict & 7), (int64_t)(verdict >> 3));
  const int64_t nb = info[2], nt = info[3];
  if (nb < 0 || nt < n || nb > nbytes || nt > nbytes) SET_ERR(ctx, ITSX_E_DEVICE, "the device parse's totals do not fit its text");
  if (!room(plane_room(ctx->ps_seq, gb, gb + nb, st)) || (keep_qual && !room(plane_room(ctx->ps_qual, gb, gb + nb, st))) || !room(plane_room(ctx->ps_titles, gt, gt + nt, st)))
    return decline(FQ_E_NOMEM, -1, ": the planes of " + std::to_string(gb + nb) + " bases");
  {
    StageTimer tm(st);
    launch_fastq_gather(dtext, a.nl, a.off, n, 1, ctx->ps_seq.p, gb, nb, st);
    if (keep_qual) launch_fastq_gather(dtext, a.nl, a.off, n, 3, ctx->ps_qual.p, gb, nb, st);
    launch_fastq_gather(dtext, a.nl, a.toff, n, 0, ctx->ps_titles.p, gt, nt, st);
    ctx->stats.ms_parse += tm.stop();
  }
  HIPCHK(hipGetLastError());
  out.n = n; out.nb = nb; out.nt = nt;
  ctx->n_parse_device++;
  return ITSX_OK;
}
// a host text to ps_text (padded as the kernels want it); false: no device memory for it
static int parse_upload(itsx_ctx *ctx, const char *text, int64_t nbytes, bool &fits)
{
  fits = true;
  if (nbytes <= 0) return ITSX_OK;
  if (ctx->ps_text.alloc((size_t)nbytes + 16) != hipSuccess) { (void)hipGetLastError(); fits = false; return ITSX_OK; }
  return put_staged(ctx, text, nbytes, ctx->ps_text.p);
}
// The whole-file loaders' device path: every text (the files of `paths`, or the one text in memory) is parsed on the device into the
// same planes with running bases; offsets and title lines come back, identifiers are cut from the titles, and the bases plane becomes
// the read set's device text (d_merged_text: packed where it lies, fetched by host_bases when rep.fa wants it, released by the next
// read set), with records kept also their bases plane, installed without a host copy.  PARSE_FALLBACK: nothing of the context's read
// set has been touched, and the caller takes the host path from its start -- a declined text, or a file that could not be read (the
// host path says why).
static int load_parsed_device(itsx_ctx *ctx, const char *const *paths, int32_t n_paths, const char *text, int64_t nbytes, int64_t *n_reads_per_file, bool batch)
{
  std::lock_guard<std::mutex> g(ctx->ps_mu);
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const bool records = batch && ctx->keep_records;
  const int32_t ntexts = paths ? n_paths : 1;
  ctx->ps_n = -1; ctx->stats.ms_parse = 0;
  std::vector<int64_t> off(1, 0); NameList titles; std::vector<int32_t> smp;
  std::vector<int64_t> counts((size_t)ntexts, 0);
  int64_t gb = 0, gt = 0;
  for (int32_t f = 0; f < ntexts; f++) {
    const uint8_t *dtext = nullptr; int64_t len = 0;
    std::shared_ptr<const itsx_io::Text> tp;
    bool kept = false;
    if (paths) {
      if (!paths[f]) return PARSE_FALLBACK;
      std::string rerr;
      if (device_inflate_on(ctx)) {
        // the device inflate's text stays where it is: nothing of it comes back, nothing of it is cached
        const itsx_io::InflateFirst first = [ctx](const itsx_io::Text &raw, itsx_io::Text &) {
          std::lock_guard<std::mutex> gi(ctx->inf_mu);
          if (hipSetDevice(ctx->device) != hipSuccess) return false;
          return inflate_file(ctx, raw.data(), (int64_t)raw.size(), nullptr, nullptr) == ITSX_OK;
        };
        tp = itsx_io::read_text(paths[f], rerr, true, &first, &kept);
      } else tp = itsx_io::read_text(paths[f], rerr, true);
      if (!tp) return PARSE_FALLBACK;
    }
    if (kept) { dtext = ctx->inf_text.p; len = ctx->inf_len; }
    else {
      const char *h = paths ? tp->data() : text;
      len = paths ? (int64_t)tp->size() : nbytes;
      bool fits = true;
      { const int rc = parse_upload(ctx, h, len, fits); if (rc != ITSX_OK) return rc; }
      if (!fits) return PARSE_FALLBACK;
      dtext = ctx->ps_text.p;
    }
    ParsedText pt;
    const int rc = parse_text_device(ctx, dtext, len, records, gb, gt, pt);
    if (rc == ITSX_E_UNSUPPORTED) return PARSE_FALLBACK;
    if (rc != ITSX_OK) return rc;
    if (pt.n > 0) {                              // this text's offsets and title lines: all that comes back
      const size_t r0 = off.size() - 1;
      off.resize(r0 + (size_t)pt.n + 1); titles.off.resize(r0 + (size_t)pt.n + 1); titles.blob.resize((size_t)(gt + pt.nt));
      HIPCHK(hipMemcpyAsync(off.data() + r0 + 1, ctx->ps_off.p + 1, (size_t)pt.n * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(titles.off.data() + r0 + 1, ctx->ps_toff.p + 1, (size_t)pt.n * 8, hipMemcpyDeviceToHost, st));
      { const int frc = fetch_staged(ctx, ctx->ps_titles.p + gt, pt.nt, titles.blob.data() + gt); if (frc != ITSX_OK) return frc; }
      if (gb || gt) for (size_t r = r0 + 1; r < off.size(); r++) { off[r] += gb; titles.off[r] += gt; }
    }
    gb += pt.nb; gt += pt.nt;
    counts[(size_t)f] = pt.n;
    if (batch) smp.resize(off.size() - 1, f);
  }
  HIPCHK(hipStreamSynchronize(st));
  const int64_t N = (int64_t)off.size() - 1;
  if (N >= (1ll << 31) - 64) return PARSE_FALLBACK;
  NameList names;                                // the identifier: the title after its '@' up to the first blank or tab
  names.off.reserve((size_t)N + 1); names.blob.reserve(titles.blob.size());
  for (int64_t r = 0; r < N; r++) {
    const char *b = titles.ptr((size_t)r) + 1, *e = titles.ptr((size_t)r) + titles.len((size_t)r), *ne = b;
    while (ne < e && *ne != ' ' && *ne != '\t') ne++;
    names.emplace_back(b, ne);
  }
  // ---- the read set
  if (n_reads_per_file) for (int32_t f = 0; f < ntexts; f++) n_reads_per_file[f] = counts[(size_t)f];
  itsx_io::Text().swap(ctx->h_bases);
  ctx->h_off.swap(off); ctx->h_names.swap(names); ctx->N = N;
  ctx->d_merged_text.release();
  dbuf_swap(ctx->d_merged_text, ctx->ps_seq);
  if (!ctx->d_merged_text.p) HIPCHK(ctx->d_merged_text.alloc(64));
  int rc = pack_and_upload(ctx, nullptr, ctx->d_merged_text.p);
  if (rc != ITSX_OK || !batch) return rc;
  rc = itsx_set_samples(ctx, smp.data(), n_paths);
  if (rc != ITSX_OK || !records) return rc;
  itsx_ctx::Records &rr = ctx->rec;              // the planes as the gather left them: no host copy of bases or qualities exists
  dbuf_swap(rr.qual, ctx->ps_qual); dbuf_swap(rr.titles, ctx->ps_titles);
  if (!rr.qual.p) HIPCHK(rr.qual.alloc(64));
  if (!rr.titles.p) HIPCHK(rr.titles.alloc(64));
  HIPCHK(rr.off.alloc((size_t)N + 1)); HIPCHK(rr.toff.alloc((size_t)N + 1));
  HIPCHK(hipMemcpyAsync(rr.off.p, ctx->h_off.data(), ((size_t)N + 1) * 8, hipMemcpyHostToDevice, ctx->st));
  HIPCHK(hipMemcpyAsync(rr.toff.p, titles.off.data(), ((size_t)N + 1) * 8, hipMemcpyHostToDevice, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  rr.h_titles.swap(titles);
  rr.seq_p = ctx->d_merged_text.p; rr.have = true;
  return ITSX_OK;
}
// ---- a PAIR of texts: the plane set once per side
// a side's planes into the parser's slots (and, for the raw entry, the parser's offsets out of them) and back
static void pair_side_swap(itsx_ctx *ctx, int side)
{
  itsx_ctx::PairSide &p = ctx->pp[side];
  dbuf_swap(ctx->ps_seq, p.seq); dbuf_swap(ctx->ps_qual, p.qual); dbuf_swap(ctx->ps_titles, p.titles);
}
struct PairSideScope {      // the side's planes are the parser's for the scope's life
  itsx_ctx *ctx; int side;
  PairSideScope(itsx_ctx *c, int s) : ctx(c), side(s) { pair_side_swap(ctx, side); }
  ~PairSideScope() { pair_side_swap(ctx, side); }
};
// the pass over both sides' finished planes (k_fastq.hip: k_fastq_pairs): flags and the longest pair come back
static int pairs_pass_device(itsx_ctx *ctx, const int64_t *d_off1, const int64_t *d_off2, int64_t n, int64_t nb1, int64_t nb2, int32_t &flags, int64_t &max_total)
{
  flags = 0; max_total = 0;
  if (n <= 0) return ITSX_OK;
  hipStream_t st = ctx->st;
  HIPCHK(ctx->pp_info.alloc(2));
  FastqPairArgs a{};
  a.seq[0] = ctx->pp[0].seq.p; a.qual[0] = ctx->pp[0].qual.p; a.total[0] = nb1; a.off[0] = d_off1;
  a.seq[1] = ctx->pp[1].seq.p; a.qual[1] = ctx->pp[1].qual.p; a.total[1] = nb2; a.off[1] = d_off2;
  a.n = n; a.info = ctx->pp_info.p;
  {
    StageTimer tm(st);
    launch_fastq_pairs(a, st);
    ctx->stats.ms_parse += tm.stop();
  }
  HIPCHK(hipGetLastError());
  unsigned long long info[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(info, ctx->pp_info.p, sizeof(info), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  flags = (int32_t)info[0]; max_total = (int64_t)info[1];
  return ITSX_OK;
}
// The paired merge loaders' device path.  All R1 texts of the call are parsed into one plane set and all R2 texts into the other, with
// running bases as load_parsed_device's batch has them; a file the device inflate accepted is parsed where it lies, any other text goes
// up once.  What comes back: the parser's two small reads per text, the offsets (8 bytes a record and plane, rebased per sample here and
// sent up again as the merge kernel's), R1's title lines (the identifiers are cut from them) and the counts.  Bases and qualities never
// do: k_fastq_pairs upper-cases and checks them where they lie, and merge_load_core runs the merge kernel on them and keeps them as the
// pair records.  PARSE_FALLBACK: nothing of the context's read set, records or pair records has been touched.
static int merge_pairs_load_device(itsx_ctx *ctx, const char *const *r1_paths, const char *const *r2_paths, const char *const *seq_out_paths, int32_t S,
                                   const char *text1, int64_t nb1, const char *text2, int64_t nb2, int maxdiffs, double maxee, int allow_stagger,
                                   int64_t *n_pairs_per_sample, int64_t *n_merged_per_sample, bool batch)
{
  const auto tm0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> g(ctx->ps_mu);
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  ctx->ps_n = -1; ctx->pp_n = -1; ctx->stats.ms_parse = 0;
  FastxPart f, r;                                // of these only `off` is filled: the pairs' offsets over the whole call
  std::vector<int64_t> toff[2] = {std::vector<int64_t>(1, 0), std::vector<int64_t>(1, 0)};
  std::vector<NameList> names((size_t)S);        // R1's identifiers per sample: the title after its '@' up to the first blank or tab
  std::vector<int64_t> counts[2] = {std::vector<int64_t>((size_t)S, 0), std::vector<int64_t>((size_t)S, 0)};
  for (int side = 0; side < 2; side++) {
    PairSideScope planes(ctx, side);
    std::vector<int64_t> &off = side ? r.off : f.off;
    int64_t gb = 0, gt = 0;
    for (int32_t s = 0; s < S; s++) {
      const char *path = text1 ? nullptr : (side ? r2_paths[s] : r1_paths[s]);
      const uint8_t *dtext = nullptr; int64_t len = 0;
      std::shared_ptr<const itsx_io::Text> tp;
      bool kept = false;
      if (path) {
        std::string rerr;
        if (device_inflate_on(ctx)) {
          // the device inflate's text stays where it is: nothing of it comes back, nothing of it is cached
          const itsx_io::InflateFirst first = [ctx](const itsx_io::Text &raw, itsx_io::Text &) {
            std::lock_guard<std::mutex> gi(ctx->inf_mu);
            if (hipSetDevice(ctx->device) != hipSuccess) return false;
            return inflate_file(ctx, raw.data(), (int64_t)raw.size(), nullptr, nullptr) == ITSX_OK;
          };
          tp = itsx_io::read_text(path, rerr, true, &first, &kept);
        } else tp = itsx_io::read_text(path, rerr, true);
        if (!tp) return PARSE_FALLBACK;
      }
      if (kept) { dtext = ctx->inf_text.p; len = ctx->inf_len; }
      else {
        const char *h = path ? tp->data() : (side ? text2 : text1);
        len = path ? (int64_t)tp->size() : (side ? nb2 : nb1);
        bool fits = true;
        { const int rc = parse_upload(ctx, h, len, fits); if (rc != ITSX_OK) return rc; }
        if (!fits) return PARSE_FALLBACK;
        dtext = ctx->ps_text.p;
      }
      ParsedText pt;
      const int rc = parse_text_device(ctx, dtext, len, true, gb, gt, pt);
      if (rc == ITSX_E_UNSUPPORTED) return PARSE_FALLBACK;
      if (rc != ITSX_OK) return rc;
      if (pt.n > 0) {
        const size_t r0 = off.size() - 1;
        off.resize(r0 + (size_t)pt.n + 1); toff[side].resize(r0 + (size_t)pt.n + 1);
        HIPCHK(hipMemcpyAsync(off.data() + r0 + 1, ctx->ps_off.p + 1, (size_t)pt.n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(toff[side].data() + r0 + 1, ctx->ps_toff.p + 1, (size_t)pt.n * 8, hipMemcpyDeviceToHost, st));
        std::vector<char> tl;
        if (side == 0) { tl.resize((size_t)pt.nt); const int frc = fetch_staged(ctx, ctx->ps_titles.p + gt, pt.nt, tl.data()); if (frc != ITSX_OK) return frc; }
        HIPCHK(hipStreamSynchronize(st));
        if (side == 0) {
          NameList &nm = names[(size_t)s];
          nm.off.reserve((size_t)pt.n + 1); nm.blob.reserve((size_t)pt.nt);
          for (size_t q = r0; q + 1 < off.size(); q++) {      // (the offsets are still this text's own; its first title starts at 0)
            const char *b = tl.data() + (q > r0 ? toff[0][q] : 0) + 1, *e = tl.data() + toff[0][q + 1], *ne = b;
            while (ne < e && *ne != ' ' && *ne != '\t') ne++;
            nm.emplace_back(b, ne);
          }
        }
        if (gb || gt) for (size_t q = r0 + 1; q < off.size(); q++) { off[q] += gb; toff[side][q] += gt; }
      }
      gb += pt.nb; gt += pt.nt;
      counts[side][(size_t)s] = pt.n;
    }
    ctx->pp[side].nb = gb; ctx->pp[side].nt = gt;
  }
  std::vector<int64_t> pstart((size_t)S + 1, 0);
  for (int32_t s = 0; s < S; s++) {
    if (counts[0][(size_t)s] != counts[1][(size_t)s]) return PARSE_FALLBACK;      // the host path names the files and the counts
    pstart[(size_t)s + 1] = pstart[(size_t)s] + counts[0][(size_t)s];
  }
  const int64_t n = pstart[(size_t)S];
  if (n >= (1ll << 31) - 64) return PARSE_FALLBACK;
  DBuf<int64_t> d_fo, d_ro;
  int32_t flags = 0; int64_t max_total = 0;
  if (n > 0) {
    if (d_fo.alloc((size_t)n + 1) != hipSuccess || d_ro.alloc((size_t)n + 1) != hipSuccess) { (void)hipGetLastError(); return PARSE_FALLBACK; }
    HIPCHK(hipMemcpyAsync(d_fo.p, f.off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_ro.p, r.off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    const int rc = pairs_pass_device(ctx, d_fo.p, d_ro.p, n, f.off[(size_t)n], r.off[(size_t)n], flags, max_total);
    if (rc != ITSX_OK) return rc;
  }
  if ((flags & (itsx_fq::FQ_PAIR_QUAL1 | itsx_fq::FQ_PAIR_QUAL2)) || max_total > 12000) return PARSE_FALLBACK;      // the host path's errors, in its words
  // ---- from here on the context's read set is replaced, as on the host path
  const bool lower = (flags & (itsx_fq::FQ_PAIR_LOWER1 | itsx_fq::FQ_PAIR_LOWER2)) != 0;
  const bool records = ctx->keep_records && !text1, pair_records = ctx->keep_pair_records && !text1 && !lower;
  std::vector<const NameList *> ids((size_t)S);
  for (int32_t s = 0; s < S; s++) { ids[(size_t)s] = &names[(size_t)s]; if (batch && n_pairs_per_sample) n_pairs_per_sample[s] = counts[0][(size_t)s]; }
  itsx_ctx::PairSide &p1 = ctx->pp[0], &p2 = ctx->pp[1];
  MergeDev dev{&p1.seq, &p1.qual, &p2.seq, &p2.qual, &p1.titles, &p2.titles, &d_fo, &d_ro, &toff[0], &toff[1], max_total};
  std::vector<int64_t> merged((size_t)S, 0);
  const int rc = merge_load_core(ctx, f, r, ids, pstart, seq_out_paths, maxdiffs, maxee, allow_stagger,
                                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tm0).count(), merged.data(), records, pair_records, &dev);
  if (rc != ITSX_OK) return rc;
  if (batch) { if (n_merged_per_sample) for (int32_t s = 0; s < S; s++) n_merged_per_sample[s] = merged[(size_t)s]; }
  else { if (n_pairs_per_sample) *n_pairs_per_sample = n; if (n_merged_per_sample) *n_merged_per_sample = merged[0]; }
  return ITSX_OK;
}
extern "C" {
int itsx_set_device_parse(itsx_ctx *ctx, int on)
{
  CTXCHK(ctx);
  ctx->device_parse = on != 0;
  return ITSX_OK;
}
int itsx_parse_device(itsx_ctx *ctx, const char *text, int64_t nbytes, int keep_qual, int64_t *n_records)
{
  CTXCHK(ctx && nbytes >= 0 && (text || nbytes == 0) && n_records);
  std::lock_guard<std::mutex> g(ctx->ps_mu);
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ps_n = -1; ctx->stats.ms_parse = 0;
  bool fits = true;
  { const int rc = parse_upload(ctx, text, nbytes, fits); if (rc != ITSX_OK) return rc; }
  if (!fits) {
    ctx->n_parse_declined++;
    SET_ERR(ctx, ITSX_E_UNSUPPORTED, std::string("the device parse declined the text: ") + itsx_fq::fq_reason_name(itsx_fq::FQ_E_NOMEM) + ": the text's " + std::to_string(nbytes) + " bytes");
  }
  ParsedText pt;
  const int rc = parse_text_device(ctx, ctx->ps_text.p, nbytes, keep_qual != 0, 0, 0, pt);
  if (rc != ITSX_OK) return rc;
  HIPCHK(hipStreamSynchronize(ctx->st));
  HIPCHK(hipGetLastError());
  ctx->ps_n = pt.n; ctx->ps_nb = pt.nb; ctx->ps_nt = pt.nt; ctx->ps_qual_kept = keep_qual != 0;
  *n_records = pt.n;
  return ITSX_OK;
}
int itsx_parse_fetch(itsx_ctx *ctx, int32_t plane, int64_t lo, int64_t hi, void *out)
{
  CTXCHK(ctx);
  std::lock_guard<std::mutex> g(ctx->ps_mu);
  if (ctx->ps_n < 0) SET_ERR(ctx, ITSX_E_ARG, "itsx_parse_fetch: no parse to fetch from (the last itsx_parse_device did not succeed, or there was none)");
  if (plane < ITSX_PARSE_OFF || plane > ITSX_PARSE_TITLES || (plane == ITSX_PARSE_QUAL && !ctx->ps_qual_kept)) SET_ERR(ctx, ITSX_E_ARG, "itsx_parse_fetch: no such plane");
  const bool offs = plane == ITSX_PARSE_OFF || plane == ITSX_PARSE_TOFF;
  const int64_t size = offs ? ctx->ps_n + 1 : plane == ITSX_PARSE_TITLES ? ctx->ps_nt : ctx->ps_nb;
  if (lo < 0 || hi < lo || hi > size || (!out && hi > lo)) SET_ERR(ctx, ITSX_E_ARG, "itsx_parse_fetch: the range is not inside the plane's " + std::to_string(size) + (offs ? " entries" : " bytes"));
  if (hi == lo) return ITSX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (offs) {
    if (ctx->ps_n == 0) { *reinterpret_cast<int64_t *>(out) = 0; return ITSX_OK; }      // a text of no bytes: off = toff = {0}
    const int64_t *src = plane == ITSX_PARSE_OFF ? ctx->ps_off.p : ctx->ps_toff.p;
    return fetch_staged(ctx, reinterpret_cast<const uint8_t *>(src + lo), (hi - lo) * 8, reinterpret_cast<char *>(out));
  }
  const uint8_t *src = plane == ITSX_PARSE_SEQ ? ctx->ps_seq.p : plane == ITSX_PARSE_QUAL ? ctx->ps_qual.p : ctx->ps_titles.p;
  return fetch_staged(ctx, src + lo, hi - lo, reinterpret_cast<char *>(out));
}
int itsx_parse_pairs_device(itsx_ctx *ctx, const char *text1, int64_t nbytes1, const char *text2, int64_t nbytes2, int64_t *n_pairs, int32_t *flags, int64_t *max_total)
{
  CTXCHK(ctx && nbytes1 >= 0 && nbytes2 >= 0 && (text1 || nbytes1 == 0) && (text2 || nbytes2 == 0) && n_pairs && flags && max_total);
  std::lock_guard<std::mutex> g(ctx->ps_mu);
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ps_n = -1; ctx->pp_n = -1; ctx->stats.ms_parse = 0;
  int64_t n[2] = {0, 0};
  for (int side = 0; side < 2; side++) {
    const char *text = side ? text2 : text1; const int64_t nbytes = side ? nbytes2 : nbytes1;
    bool fits = true;
    { const int rc = parse_upload(ctx, text, nbytes, fits); if (rc != ITSX_OK) return rc; }
    if (!fits) {
      ctx->n_parse_declined++;
      SET_ERR(ctx, ITSX_E_UNSUPPORTED, std::string("the device parse declined the text: ") + itsx_fq::fq_reason_name(itsx_fq::FQ_E_NOMEM) + ": the text's " + std::to_string(nbytes) + " bytes");
    }
    ParsedText pt;
    {
      PairSideScope planes(ctx, side);
      const int rc = parse_text_device(ctx, ctx->ps_text.p, nbytes, true, 0, 0, pt);
      if (rc != ITSX_OK) return rc;
    }
    itsx_ctx::PairSide &p = ctx->pp[side];
    dbuf_swap(p.off, ctx->ps_off); dbuf_swap(p.toff, ctx->ps_toff);      // (the next text's parse makes its own)
    p.nb = pt.nb; p.nt = pt.nt; n[side] = pt.n;
  }
  if (n[0] != n[1])
    SET_ERR(ctx, ITSX_E_UNSUPPORTED, std::string("the device parse declined the pair: ") + itsx_fq::fq_reason_name(itsx_fq::FQ_E_PAIRS) + " (" + std::to_string(n[0]) + " and " + std::to_string(n[1]) + ")");
  { const int rc = pairs_pass_device(ctx, ctx->pp[0].off.p, ctx->pp[1].off.p, n[0], ctx->pp[0].nb, ctx->pp[1].nb, *flags, *max_total); if (rc != ITSX_OK) return rc; }
  HIPCHK(hipStreamSynchronize(ctx->st));
  HIPCHK(hipGetLastError());
  ctx->pp_n = n[0];
  *n_pairs = n[0];
  return ITSX_OK;
}
int itsx_parse_pairs_fetch(itsx_ctx *ctx, int32_t side, int32_t plane, int64_t lo, int64_t hi, void *out)
{
  CTXCHK(ctx);
  std::lock_guard<std::mutex> g(ctx->ps_mu);
  if (ctx->pp_n < 0) SET_ERR(ctx, ITSX_E_ARG, "itsx_parse_pairs_fetch: no parse to fetch from (the last itsx_parse_pairs_device did not succeed, or there was none)");
  if (side < 0 || side > 1) SET_ERR(ctx, ITSX_E_ARG, "itsx_parse_pairs_fetch: no such side");
  if (plane < ITSX_PARSE_OFF || plane > ITSX_PARSE_TITLES) SET_ERR(ctx, ITSX_E_ARG, "itsx_parse_pairs_fetch: no such plane");
  const itsx_ctx::PairSide &p = ctx->pp[side];
  const bool offs = plane == ITSX_PARSE_OFF || plane == ITSX_PARSE_TOFF;
  const int64_t size = offs ? ctx->pp_n + 1 : plane == ITSX_PARSE_TITLES ? p.nt : p.nb;
  if (lo < 0 || hi < lo || hi > size || (!out && hi > lo)) SET_ERR(ctx, ITSX_E_ARG, "itsx_parse_pairs_fetch: the range is not inside the plane's " + std::to_string(size) + (offs ? " entries" : " bytes"));
  if (hi == lo) return ITSX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (offs) {
    if (ctx->pp_n == 0) { *reinterpret_cast<int64_t *>(out) = 0; return ITSX_OK; }      // texts of no bytes: off = toff = {0}
    const int64_t *src = plane == ITSX_PARSE_OFF ? p.off.p : p.toff.p;
    return fetch_staged(ctx, reinterpret_cast<const uint8_t *>(src + lo), (hi - lo) * 8, reinterpret_cast<char *>(out));
  }
  const uint8_t *src = plane == ITSX_PARSE_SEQ ? p.seq.p : plane == ITSX_PARSE_QUAL ? p.qual.p : p.titles.p;
  return fetch_staged(ctx, src + lo, hi - lo, reinterpret_cast<char *>(out));
}
int itsx_debug_parse_pairs_host(const char *text1, int64_t nbytes1, const char *text2, int64_t nbytes2, int64_t *off1, int64_t *toff1, char *seq1, char *qual1, char *titles1,
                                int64_t *off2, int64_t *toff2, char *seq2, char *qual2, char *titles2, int64_t cap_records, int64_t cap_bases, int64_t cap_titles,
                                int64_t *n_pairs, int64_t *sizes, int32_t *flags, int64_t *max_total, int32_t *reason, int32_t *bad_side, int64_t *bad_record)
{
  if (nbytes1 < 0 || nbytes2 < 0 || (!text1 && nbytes1 > 0) || (!text2 && nbytes2 > 0) || !off1 || !toff1 || !off2 || !toff2 || cap_records < 0 || cap_bases < 0 || cap_titles < 0 ||
      ((!seq1 || !qual1 || !seq2 || !qual2) && cap_bases > 0) || ((!titles1 || !titles2) && cap_titles > 0) || !n_pairs || !sizes || !flags || !max_total || !reason || !bad_side || !bad_record)
    return ITSX_E_ARG;
  auto u = [](char *p) { return reinterpret_cast<uint8_t *>(p); };
  const itsx_fq::FqSideBufs b1{off1, toff1, u(seq1), u(qual1), u(titles1)}, b2{off2, toff2, u(seq2), u(qual2), u(titles2)};
  *reason = itsx_fq::fq_parse_pairs_host(reinterpret_cast<const uint8_t *>(text1), nbytes1, reinterpret_cast<const uint8_t *>(text2), nbytes2, b1, b2, cap_records, cap_bases, cap_titles,
                                         n_pairs, sizes, flags, max_total, bad_side, bad_record);
  return *reason == itsx_fq::FQ_OK ? ITSX_OK : *reason == itsx_fq::FQ_E_CAP ? ITSX_E_ARG : ITSX_E_UNSUPPORTED;
}
int itsx_debug_pair_pass_host(char *seq, const char *qual, int64_t nbytes, int32_t *flags)
{
  if (nbytes < 0 || ((!seq || !qual) && nbytes > 0) || !flags) return ITSX_E_ARG;
  *flags = itsx_fq::fq_pair_side_host(reinterpret_cast<uint8_t *>(seq), reinterpret_cast<const uint8_t *>(qual), nbytes);
  return ITSX_OK;
}
int itsx_debug_parse_host(const char *text, int64_t nbytes, int64_t *off, int64_t *toff, int64_t cap_records, char *seq, char *qual, int64_t cap_bases,
                          char *titles, int64_t cap_titles, int64_t *n_records, int64_t *n_bases, int64_t *n_title_bytes, int32_t *reason, int64_t *bad_record)
{
  if (nbytes < 0 || (!text && nbytes > 0) || !off || !toff || cap_records < 0 || cap_bases < 0 || cap_titles < 0 || (!seq && cap_bases > 0) || (!titles && cap_titles > 0) ||
      !n_records || !n_bases || !n_title_bytes || !reason || !bad_record) return ITSX_E_ARG;
  *reason = itsx_fq::fq_parse_host(reinterpret_cast<const uint8_t *>(text), nbytes, off, toff, cap_records, reinterpret_cast<uint8_t *>(seq), reinterpret_cast<uint8_t *>(qual), cap_bases,
                                   reinterpret_cast<uint8_t *>(titles), cap_titles, n_records, n_bases, n_title_bytes, bad_record);
  return *reason == itsx_fq::FQ_OK ? ITSX_OK : *reason == itsx_fq::FQ_E_CAP ? ITSX_E_ARG : ITSX_E_UNSUPPORTED;
}
}  // extern "C"
// the scratch deflate_ranges takes for a text of nbytes in one range, held before the first unit arrives
static int deflate_reserve(itsx_ctx *ctx, int64_t nbytes)
{
  int ncu = 256;
  { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, ctx->device) == hipSuccess && pr.multiProcessorCount > 0) ncu = pr.multiProcessorCount; }
  const size_t wave = (size_t)std::min<int64_t>(DEFLATE_WAVE, nbytes / DEFLATE_BLOCK_BYTES + 1);
  HIPCHK(ctx->w_dblk.alloc(wave)); HIPCHK(ctx->w_dsizes.alloc(wave)); HIPCHK(ctx->w_ddst.alloc(wave));
  HIPCHK(ctx->w_dtok.alloc((size_t)std::min<size_t>(wave, (size_t)ncu) * DEFLATE_TOKEN_SLOT));
  HIPCHK(ctx->w_dslots.alloc(wave * DEFLATE_SLOT_BYTES)); HIPCHK(ctx->w_dpacked.alloc(wave * DEFLATE_SLOT_BYTES));
  return ITSX_OK;
}
static int tw_alloc_unit(itsx_ctx *ctx, int64_t nbytes, int64_t count)
{
  HIPCHK(ctx->tw_raw.alloc((size_t)((nbytes + 15) / 16 * 16 + 16)));
  HIPCHK(ctx->tw_ls.alloc((size_t)(4 * count + 1))); HIPCHK(ctx->tw_le.alloc((size_t)(4 * count + 1)));
  HIPCHK(ctx->tw_lblk.alloc((size_t)trim_index_blocks(nbytes) + 1)); HIPCHK(ctx->tw_info.alloc(TRIM_UNIT_INFO));
  HIPCHK(ctx->w_tstart.alloc((size_t)count + 1)); HIPCHK(ctx->w_tstop.alloc((size_t)count + 1));
  HIPCHK(ctx->w_trec.alloc((size_t)count + 1)); HIPCHK(ctx->tw_qsrc.alloc((size_t)count + 1));
  HIPCHK(ctx->w_tblk.alloc((size_t)trim_plan_blocks(count) * 3 + 3));
  HIPCHK(ctx->tw_strand.alloc((size_t)count + 1)); HIPCHK(ctx->tw_comp.alloc(256));
  return ITSX_OK;
}
// one text in w_tout -> its gzip members
static int tw_deflate(itsx_ctx *ctx, int64_t total, std::string &comp)
{
  std::vector<std::pair<int64_t, int64_t>> ranges(1, std::make_pair((int64_t)0, total));
  std::vector<char> z; std::vector<int64_t> zb;
  const int rc = deflate_ranges(ctx, reinterpret_cast<const uint8_t *>(ctx->w_tout.p), ranges, z, zb);
  ctx->tw_ms_deflate += ctx->stats.ms_deflate; ctx->stats.ms_deflate = ctx->tw_ms_deflate;      // (a lent context reports the sum over its writers' units)
  if (rc != ITSX_OK) return rc;
  comp.assign(z.data(), z.size());
  return ITSX_OK;
}
static int tw_unit(itsx_ctx *ctx, const itsx::TwUnit &u, bool &fits, std::string &comp, int64_t &nw, int64_t &tot, const char *&step)
{
  step = "hipSetDevice";
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  const int64_t nbytes = (int64_t)u.nbytes, n = u.count;
  step = "allocating the unit's buffers";
  { const int rc = tw_alloc_unit(ctx, nbytes, n); if (rc != ITSX_OK) return rc; }
  step = "uploading the unit's text and coordinates";
  { const int rc = put_staged(ctx, u.text, nbytes, ctx->tw_raw.p); if (rc != ITSX_OK) return rc; }
  { const int rc = put_staged(ctx, reinterpret_cast<const char *>(u.start), n * 4, reinterpret_cast<uint8_t *>(ctx->w_tstart.p)); if (rc != ITSX_OK) return rc; }
  { const int rc = put_staged(ctx, reinterpret_cast<const char *>(u.stop), n * 4, reinterpret_cast<uint8_t *>(ctx->w_tstop.p)); if (rc != ITSX_OK) return rc; }
  const bool flips = u.strand != nullptr && u.mode == 0;
  if (flips) {
    { const int rc = put_staged(ctx, reinterpret_cast<const char *>(u.strand), n, reinterpret_cast<uint8_t *>(ctx->tw_strand.p)); if (rc != ITSX_OK) return rc; }
    if (!ctx->tw_comp_set) {
      const int rc = put_staged(ctx, itsx::iupac_complement(), 256, ctx->tw_comp.p);
      if (rc != ITSX_OK) return rc;
      ctx->tw_comp_set = true;
    }
  }
  step = "the unit's line index and plan";
  TrimUnitArgs ua{};
  ua.text = ctx->tw_raw.p; ua.nbytes = nbytes; ua.count = n; ua.ls = ctx->tw_ls.p; ua.le = ctx->tw_le.p;
  ua.start = ctx->w_tstart.p; ua.stop = ctx->w_tstop.p; ua.mode = u.mode; ua.ccs = u.ccs ? 1 : 0;
  ua.strand = flips ? ctx->tw_strand.p : nullptr;
  ua.lblk = ctx->tw_lblk.p; ua.blk = ctx->w_tblk.p; ua.rec = ctx->w_trec.p; ua.qsrc = ctx->tw_qsrc.p; ua.info = ctx->tw_info.p;
  launch_trim_unit(ua, st);
  HIPCHK(hipGetLastError());
  int64_t info[TRIM_UNIT_INFO];
  HIPCHK(hipMemcpyAsync(info, ctx->tw_info.p, sizeof(info), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  fits = info[0] == 4 * n && info[1] == 0;
  if (!fits) return ITSX_OK;
  ctx->stats.n_tw_units_device++;
  const int64_t total = info[2];
  nw = info[3]; tot = info[4];
  comp.clear();
  if (total <= 0) return ITSX_OK;
  step = "copying the unit's records";
  HIPCHK(ctx->w_tout.alloc((size_t)(trim_copy_bytes(total) / 4) + 16));
  TrimCopyArgs ca{};
  ca.rec = ctx->w_trec.p; ca.n = n; ca.seq = ca.qual = ca.titles = ctx->tw_raw.p; ca.qsrc = ctx->tw_qsrc.p;
  ca.total = total; ca.ccs = ua.ccs; ca.out = ctx->w_tout.p;
  ca.comp = flips ? ctx->tw_comp.p : nullptr;
  launch_trim_copy(ca, st);
  HIPCHK(hipGetLastError());
  step = "deflating the unit's output";
  return tw_deflate(ctx, total, comp);
}
static int tw_text(itsx_ctx *ctx, const char *text, size_t nbytes, std::string &comp, const char *&step)
{
  step = "hipSetDevice";
  HIPCHK(hipSetDevice(ctx->device));
  ctx->stats.n_tw_units_host++;
  step = "uploading the unit's output";
  HIPCHK(ctx->w_tout.alloc((size_t)(trim_copy_bytes((int64_t)nbytes) / 4) + 16));
  { const int rc = put_staged(ctx, text, (int64_t)nbytes, reinterpret_cast<uint8_t *>(ctx->w_tout.p)); if (rc != ITSX_OK) return rc; }
  step = "deflating the unit's output";
  return tw_deflate(ctx, (int64_t)nbytes, comp);
}
namespace itsx {
template <class F> static int tw_call(itsx_ctx *ctx, std::string &err, F &&f)
{
  std::lock_guard<std::mutex> lk(ctx->tw_mu);
  if (ctx->tw_failed) { err = "device writer: an earlier step on this context failed (" + ctx->err + ")"; return ITSX_E_DEVICE; }
  const char *step = "";
  const int rc = f(step);
  if (rc != ITSX_OK) {
    if (rc == ITSX_E_DEVICE) ctx->tw_failed = true;
    err = std::string("device writer: ") + step + ": " + ctx->err;
  }
  return rc;
}
int twdev_reserve(itsx_ctx *ctx, size_t unit_bytes, std::string &err)
{
  return tw_call(ctx, err, [&](const char *&step) -> int {
    step = "allocating the device buffers";
    HIPCHK(hipSetDevice(ctx->device));
    // a unit ends at the first record start past its size, reads are a few hundred bytes, a record of 4 lines is at least 7 bytes
    const int64_t nbytes = (int64_t)std::min<size_t>(unit_bytes + unit_bytes / 8 + 65536, ((size_t)1 << 31) - 1);
    // records of 32 bytes of text or more (a read of 10 bases); the output of a unit is its text at most, plus --trim-ccs's 68 bytes per record
    const int64_t nrec = nbytes / 32 + 1, nout = nbytes + 68 * nrec;
    { const int rc = tw_alloc_unit(ctx, nbytes, nrec); if (rc != ITSX_OK) return rc; }
    HIPCHK(ctx->w_tout.alloc((size_t)(trim_copy_bytes(nout) / 4) + 16));
    { const int rc = stage_reserve(ctx, std::min<int64_t>(64ll << 20, std::max<int64_t>(nout, 4 << 20))); if (rc != ITSX_OK) return rc; }      // (what fetch_staged asks for at most)
    return deflate_reserve(ctx, nout);
  });
}
int twdev_unit(itsx_ctx *ctx, const TwUnit &u, bool &fits, std::string &comp, int64_t &nw, int64_t &tot, std::string &err)
{
  fits = false; nw = tot = 0;
  return tw_call(ctx, err, [&](const char *&step) -> int { return tw_unit(ctx, u, fits, comp, nw, tot, step); });
}
int twdev_text(itsx_ctx *ctx, const char *text, size_t nbytes, std::string &comp, std::string &err)
{
  return tw_call(ctx, err, [&](const char *&step) -> int { return tw_text(ctx, text, nbytes, comp, step); });
}
}  // namespace itsx
extern "C" {
int itsx_debug_huffman_lengths(const uint32_t *freq, int32_t n, int32_t maxbits, uint8_t *lengths)
{
  if (!freq || !lengths || n < 1 || n > itsx_dc::MAX_SYMS || maxbits < 1 || maxbits > 15 || (maxbits < 9 && n > (1 << maxbits))) return ITSX_E_ARG;
  uint64_t sum = 0;
  for (int32_t i = 0; i < n; i++) sum += freq[i];
  if (sum >> 32) return ITSX_E_ARG;
  uint32_t work[itsx_dc::WORK_WORDS];
  itsx_dc::dc_huffman_lengths(freq, n, maxbits, lengths, work);
  return ITSX_OK;
}
int itsx_derep_device(itsx_ctx *ctx, const int32_t **d_rep_of, const int32_t **d_uniq_of, const int8_t **d_strand, const int32_t **d_seed_read)
{
  CTXCHK(ctx && ctx->grouped());
  if (d_rep_of) *d_rep_of = ctx->d_rep_of.p;
  if (d_uniq_of) *d_uniq_of = ctx->d_uniq_of.p;
  if (d_strand) *d_strand = ctx->d_strand.p;
  if (d_seed_read) *d_seed_read = ctx->d_seed_read.p;
  return ITSX_OK;
}
int itsx_unique_keys128_device(itsx_ctx *ctx, uint64_t seed_a, uint64_t seed_b, int64_t gidx_base, int64_t **d_tuples, int64_t *n_unique)
{
  CTXCHK(ctx && ctx->grouped() && d_tuples);
  if (ctx->S > 1) SET_ERR(ctx, ITSX_E_UNSUPPORTED, "cross-rank dereplication of a sample batch is not supported: shard whole samples across ranks");
  HIPCHK(hipSetDevice(ctx->device));
  LoadPriority load_priority(ctx);
  const int64_t n = ctx->N; const int32_t U = ctx->U;
  HIPCHK(ctx->w_keys128.alloc((size_t)U * 4 + 4));
  if (n > 0 && U > 0) {
    HIPCHK(ctx->w_hf.alloc((size_t)n + 1)); HIPCHK(ctx->w_hr.alloc((size_t)n + 1)); HIPCHK(ctx->w_hf1.alloc((size_t)n + 1)); HIPCHK(ctx->w_hr1.alloc((size_t)n + 1));
    // (a plus-strand-only dereplication keeps a sequence and its reverse complement apart across shards too: the key is the forward
    // strand's then -- k_hash_reads returns it for both strands -- and every flag says "forward")
    launch_hash_reads(ctx->rd, seed_a, ctx->derep_strand_both, ctx->w_hf.p, ctx->w_hr.p, ctx->st);
    launch_hash_reads(ctx->rd, seed_b, ctx->derep_strand_both, ctx->w_hf1.p, ctx->w_hr1.p, ctx->st);
    hipLaunchKernelGGL(k_unique_keys128, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, ctx->st, U, ctx->d_seed_read.p, ctx->rd.len, ctx->w_hf.p, ctx->w_hr.p,
                       ctx->w_hf1.p, ctx->w_hr1.p, gidx_base, ctx->w_keys128.p);
  }
  HIPCHK(hipStreamSynchronize(ctx->st));
  HIPCHK(hipGetLastError());
  *d_tuples = ctx->w_keys128.p;
  if (n_unique) *n_unique = U;
  return ITSX_OK;
}
int itsx_rep_coords(itsx_ctx *ctx, const char *lp, const char *rp, int32_t *start, int32_t *stop, int32_t *tlen, int32_t *ind)
{ return coords_common(ctx, lp, rp, false, start, stop, tlen, ind); }
// the same tuples in host memory (a driver without a collective library: itsxpress_amd/multi.py moves them through pipes)
int itsx_unique_keys128(itsx_ctx *ctx, uint64_t seed_a, uint64_t seed_b, int64_t gidx_base, int64_t *tuples)
{
  CTXCHK(ctx && (tuples || ctx->U == 0));
  int64_t *d = nullptr; int64_t nu = 0;
  const int rc = itsx_unique_keys128_device(ctx, seed_a, seed_b, gidx_base, &d, &nu);
  if (rc != ITSX_OK) return rc;
  if (nu > 0) HIPCHK(hipMemcpy(tuples, d, (size_t)nu * 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
  return ITSX_OK;
}
// E-value parameters and length of profile i: {MSV mu, lambda, Viterbi mu, lambda, Forward tau, lambda} (the array writers' columns)
int itsx_profile_params(const itsx_ctx *ctx, int i, int32_t *M, float *evparam6)
{
  CTXCHK(ctx && i >= 0 && i < ctx->P);
  if (M) *M = ctx->profs[(size_t)i].M;
  if (evparam6) for (int k = 0; k < 6; k++) evparam6[k] = ctx->profs[(size_t)i].evparam[k];
  return ITSX_OK;
}
// reads handed over in device memory: the text comes back once (rep.fa, the seeds' sequences)
static int host_bases(const itsx_ctx *cctx)
{
  itsx_ctx *ctx = const_cast<itsx_ctx *>(cctx);
  if (ctx->bases_view) return ITSX_OK;
  HIPCHK(hipSetDevice(ctx->device));
  ctx->h_bases.resize((size_t)ctx->h_off[(size_t)ctx->N]);
  if (!ctx->h_bases.empty()) HIPCHK(hipMemcpy(&ctx->h_bases[0], ctx->dev_bases, ctx->h_bases.size(), hipMemcpyDeviceToHost));
  ctx->bases_view = ctx->h_bases.data();
  // the host has it now -- unless it is the bases plane of the read set's records
  if (ctx->d_merged_text.p && ctx->dev_bases == ctx->d_merged_text.p && !(ctx->rec.have && ctx->rec.seq_p == ctx->d_merged_text.p)) { ctx->d_merged_text.release(); ctx->dev_bases = nullptr; }
  return ITSX_OK;
}
// sequences of the unique representatives in input order of the seeds (what rep.fa holds), concatenated; offsets[n_unique + 1];
// bases == NULL fills the offsets only
int itsx_get_unique_seqs(itsx_ctx *ctx, char *bases, int64_t cap, int64_t *offsets)
{
  CTXCHK(ctx && offsets && ctx->grouped());
  { const int rc = host_bases(ctx); if (rc != ITSX_OK) return rc; }
  int64_t o = 0;
  for (int32_t u = 0; u < ctx->U; u++) {
    const int64_t s = ctx->h_seed_read[(size_t)u], L = ctx->h_len[(size_t)s];
    offsets[u] = o;
    if (bases) { if (o + L > cap) SET_ERR(ctx, ITSX_E_ARG, "sequence buffer too small"); memcpy(bases + o, ctx->bases_view + ctx->h_off[(size_t)s], (size_t)L); }
    o += L;
  }
  offsets[ctx->U] = o;
  return ITSX_OK;
}

// ------------------------------------------------------------------------------ writers
// the files themselves are formatted by writers_host.cpp (writers.h), which the array writers of a multi-GPU run share: these
// adapters check the state, hand over the context's arrays and map a failure to the context's error

static itsx::Labels read_labels(const itsx_ctx *ctx)
{
  return ctx->h_names.empty() ? itsx::Labels{} : itsx::Labels{ctx->h_names.blob.data(), ctx->h_names.off.data()};
}
static itsx::Clusters clusters(const itsx_ctx *ctx)
{
  itsx::Clusters c;
  c.n = ctx->N; c.U = ctx->U;
  c.uniq_of = ctx->h_uniq_of.data(); c.seed_read = ctx->h_seed_read.data(); c.abund = ctx->h_abund.data();
  c.len = ctx->h_len.data(); c.strand = ctx->h_strand.data(); c.labels = read_labels(ctx);
  if (ctx->clustered) { c.order = ctx->h_order.data(); c.n_order = (int64_t)ctx->h_order.size(); c.pct = ctx->h_pct.data(); }
  if (ctx->cigars_live()) { c.cigar_off = ctx->h_cg_off.data(); c.cigar_text = ctx->h_cg_text.data(); }
  if (ctx->S > 1) { c.sample = ctx->h_sample.data(); c.usample = ctx->h_usample.data(); c.sel = ctx->sel_sample; }   // writers restricted to one sample of a batch
  return c;
}
// clusters in vsearch's output order, kept for the current dereplication (uc.txt and rep.fa both ask)
static const std::vector<int32_t> &cluster_order(const itsx_ctx *cctx, const itsx::Clusters &c)
{
  itsx_ctx *ctx = const_cast<itsx_ctx *>(cctx);
  if (!ctx->order_cache_ok) { itsx::cluster_order(c, ctx->order_cache); ctx->order_cache_ok = true; }
  return ctx->order_cache;
}

int itsx_write_uc(const itsx_ctx *ctx, const char *path)
{
  CTXCHK(ctx && path && ctx->grouped());
  const itsx::Clusters c = clusters(ctx);
  std::string err;
  const int rc = itsx::write_uc(path, c, cluster_order(ctx, c), err);
  if (rc != ITSX_OK) SET_ERR(ctx, rc, err);
  return ITSX_OK;
}

int itsx_write_rep_fasta(const itsx_ctx *ctx, const char *path)
{
  CTXCHK(ctx && path && ctx->grouped());
  { const int rc = host_bases(ctx); if (rc != ITSX_OK) return rc; }
  const itsx::Clusters c = clusters(ctx);
  std::string err;
  const int rc = itsx::write_rep_fasta(path, c, cluster_order(ctx, c), itsx::Seqs{ctx->bases_view, ctx->h_off.data(), false}, err);
  if (rc != ITSX_OK) SET_ERR(ctx, rc, err);
  return ITSX_OK;
}

int itsx_write_domtbl(const itsx_ctx *ctx, const char *path)
{
  CTXCHK(ctx && path && ctx->finalized());
  { const int rc = fetch_domains(ctx); if (rc != ITSX_OK) return rc; }
  std::vector<int64_t> Zs((size_t)ctx->S, 0);          // hmmsearch's Z: targets searched, per sample
  // (a context narrowed by itsx_set_active_uniques searched only its active targets: the E-value columns of a sharded run are
  // this shard's own, the reported / not-reported decisions are global through the all-reduced domZ)
  if (ctx->S == 1) Zs[0] = ctx->U_active; else for (int32_t u = 0; u < ctx->U; u++) Zs[(size_t)ctx->usample(u)]++;
  std::string pnames;
  std::vector<int64_t> poffs(1, 0);
  std::vector<int32_t> M;
  std::vector<float> tau, lambda;
  for (const HostProfile &h : ctx->profs) {
    pnames += h.name; poffs.push_back((int64_t)pnames.size());
    M.push_back(h.M); tau.push_back(h.evparam[4]); lambda.push_back(h.evparam[5]);
  }
  itsx::DomTable t;
  t.rows = ctx->h_dom.data(); t.n = ctx->h_dom.size(); t.P = ctx->P;
  t.prof_names = itsx::Labels{pnames.data(), poffs.data()}; t.M = M.data(); t.tau = tau.data(); t.lambda = lambda.data();
  t.Z = Zs.data(); t.domz = ctx->domz.data();
  if (ctx->S > 1) { t.usample = ctx->h_usample.data(); t.sel = ctx->sel_sample; }
  t.seed_read = ctx->h_seed_read.data(); t.targets = read_labels(ctx);
  std::vector<itsx_alignment> ali;
  if (ctx->alignments_live()) { ali.resize(ctx->h_dom.size()); alignments_of_rows(ctx, ali.data()); t.ali = ali.data(); }
  std::string err;
  const int rc = itsx::write_domtbl(path, t, err);
  if (rc != ITSX_OK) SET_ERR(ctx, rc, err);
  return ITSX_OK;
}

// labels of the loaded reads (identifier up to the first blank), concatenated; offsets[n+1].  names == NULL: offsets only
// (offsets[n] = bytes needed).  Reads handed over without names are labelled r%09d, as the writers label them.
int itsx_get_read_names(const itsx_ctx *ctx, char *names, int64_t cap, int64_t *offsets)
{
  CTXCHK(ctx && offsets);
  if (!ctx->h_names.empty() && (int64_t)ctx->h_names.size() == ctx->N) {      // the labels as they are kept: one copy
    const int64_t tot = ctx->h_names.off[(size_t)ctx->N];
    if (names) { if (tot > cap) SET_ERR(ctx, ITSX_E_ARG, "name buffer too small"); if (tot) memcpy(names, ctx->h_names.blob.data(), (size_t)tot); }
    memcpy(offsets, ctx->h_names.off.data(), ((size_t)ctx->N + 1) * sizeof(int64_t));
    return ITSX_OK;
  }
  int64_t o = 0;
  for (int64_t r = 0; r < ctx->N; r++) {
    offsets[r] = o;
    const std::string nm = read_labels(ctx)(r);
    if (names) { if (o + (int64_t)nm.size() > cap) SET_ERR(ctx, ITSX_E_ARG, "name buffer too small"); memcpy(names + o, nm.data(), nm.size()); }
    o += (int64_t)nm.size();
  }
  offsets[ctx->N] = o;
  return ITSX_OK;
}

// the library's environment switches (csrc/switches.cpp) that are set: of the last search of ctx (snapshot taken when it started), or, with
// ctx == NULL, of the environment right now.  "NAME=value\n" lines; returns the length needed (incl. the terminator)
int64_t itsx_switches(const itsx_ctx *ctx, char *buf, int64_t cap)
{
  const std::string s = ctx ? ctx->switches_at_search : sw_report();
  if (buf && cap > 0) { const size_t n = std::min<size_t>(s.size(), (size_t)cap - 1); memcpy(buf, s.data(), n); buf[n] = 0; }
  return (int64_t)s.size() + 1;
}

// the registry itself: "NAME\tclass\tmeaning\n" lines (class: tuning | mode | diagnostic | hook)
int64_t itsx_switch_registry(char *buf, int64_t cap)
{
  static const char *kinds[] = {"tuning", "mode", "diagnostic", "hook"};
  int n = 0; const Switch *r = sw_registry(&n);
  std::string s;
  for (int i = 0; i < n; i++) { s += r[i].name; s += "\t"; s += kinds[r[i].kind]; s += "\t"; s += r[i].what; s += "\n"; }
  if (buf && cap > 0) { const size_t m = std::min<size_t>(s.size(), (size_t)cap - 1); memcpy(buf, s.data(), m); buf[m] = 0; }
  return (int64_t)s.size() + 1;
}

int itsx_get_stats(const itsx_ctx *ctx, itsx_stats *out, int64_t out_size)
{
  CTXCHK(ctx && out);
  if (out_size != (int64_t)sizeof(itsx_stats)) SET_ERR(ctx, ITSX_E_ARG, "itsx_get_stats: the caller's itsx_stats has " + std::to_string(out_size) + " bytes, this library's " + std::to_string(sizeof(itsx_stats)) + " (header and library from different sources)");
  *out = ctx->stats;
  out->n_inflate_device = ctx->n_inf_device; out->n_inflate_declined = ctx->n_inf_declined;
  out->n_parse_device = ctx->n_parse_device; out->n_parse_declined = ctx->n_parse_declined;
  return ITSX_OK;
}

// ------------------------------------------------------------------------------ test hooks
int itsx_debug_read_hashes(itsx_ctx *ctx, uint64_t *fwd, uint64_t *rc)
{
  CTXCHK(ctx && fwd && rc);
  HIPCHK(hipSetDevice(ctx->device));
  DBuf<uint64_t> hf, hr;
  HIPCHK(hf.alloc((size_t)ctx->N + 1)); HIPCHK(hr.alloc((size_t)ctx->N + 1));
  if (ctx->N > 0) {
    launch_hash_reads(ctx->rd, 0, 1, hf.p, hr.p, ctx->st);
    HIPCHK(hipMemcpyAsync(fwd, hf.p, (size_t)ctx->N * 8, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(rc, hr.p, (size_t)ctx->N * 8, hipMemcpyDeviceToHost, ctx->st));
  }
  HIPCHK(hipStreamSynchronize(ctx->st));
  return ITSX_OK;
}

int itsx_debug_packed_read(const itsx_ctx *ctx, int64_t i, uint32_t *words, int32_t *nwords, uint32_t *exc, int32_t *nexc)
{
  CTXCHK(ctx && i >= 0 && i < ctx->N && nwords && nexc);
  HIPCHK(hipSetDevice(ctx->device));
  int64_t eo[2] = {0, 0};
  HIPCHK(hipMemcpy(eo, ctx->d_excoff.p + i, sizeof(eo), hipMemcpyDeviceToHost));
  const int32_t nw = (int32_t)(ctx->h_woff[i + 1] - ctx->h_woff[i]), ne = (int32_t)(eo[1] - eo[0]);
  if (words) HIPCHK(hipMemcpy(words, ctx->d_words.p + ctx->h_woff[i], (size_t)nw * 4, hipMemcpyDeviceToHost));
  if (exc && ne) HIPCHK(hipMemcpy(exc, ctx->d_exc.p + eo[0], (size_t)ne * 4, hipMemcpyDeviceToHost));
  *nwords = nw; *nexc = ne;
  return ITSX_OK;
}

// streams `gbytes` GB in slab pattern `pattern` (k_util.hip: launch_calib) `iters` times; returns the bytes one launch touches
int itsx_debug_calibrate(itsx_ctx *ctx, int pattern, double gbytes, int iters, int64_t *bytes_per_launch, double *ms_per_launch)
{
  CTXCHK(ctx && pattern >= 0 && pattern <= 3 && gbytes > 0 && iters >= 1);
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t nwaves = 256 * 32;                          // 8 waves per SIMD, as k_decode runs
  const int64_t row_floats = pattern == 3 ? 4 * 64 : 6 * 64;
  const int64_t R = std::max<int64_t>(1, (int64_t)(gbytes * 1e9) / (nwaves * row_floats * 4));
  DBuf<float> slab, out;
  HIPCHK(slab.alloc((size_t)(nwaves * R * row_floats), true)); HIPCHK(out.alloc((size_t)nwaves * 64));
  HIPCHK(hipMemsetAsync(slab.p, 0, (size_t)(nwaves * R * row_floats) * 4, ctx->st));
  StageTimer tm(ctx->st);
  for (int i = 0; i < iters; i++) launch_calib(pattern, slab.p, nwaves, R, out.p, ctx->st);
  const float ms = tm.stop();
  HIPCHK(hipGetLastError());
  const int64_t touched = pattern == 1 ? 5 * 64 * 4 : row_floats * 4;
  if (bytes_per_launch) *bytes_per_launch = nwaves * R * touched;
  if (ms_per_launch) *ms_per_launch = ms / iters;
  return ITSX_OK;
}

// VALU issue rates (profiles/round5_valu_issue.md): one instruction class, no dependence between consecutive instructions,
// waves_per_simd waves on every SIMD of the chip.  cycles_per_instr = median over waves of s_memtime ticks per instruction as ONE wave
// sees them (divide by waves_per_simd for the SIMD's issue interval); ms = the launch.
int itsx_debug_issue(itsx_ctx *ctx, int op, int waves_per_simd, int iters, double *cycles_per_instr, double *ms)
{
  CTXCHK(ctx && op >= 0 && op <= 12 && waves_per_simd >= 1 && waves_per_simd <= 8 && (waves_per_simd <= 4 || waves_per_simd % 2 == 0) && iters >= 1);
  HIPCHK(hipSetDevice(ctx->device));
  int ncu = 256;
  { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, ctx->device) == hipSuccess) ncu = pr.multiProcessorCount; }
  const int nw = ncu * 4 * waves_per_simd;
  DBuf<unsigned long long> ticks; DBuf<float> sink;
  HIPCHK(ticks.alloc((size_t)nw)); HIPCHK(sink.alloc(1024));          // (the scalar probes read 1.1 KB of it)
  HIPCHK(hipMemsetAsync(sink.p, 0, 1024 * sizeof(float), ctx->st));
  launch_issue(op, waves_per_simd, 16, ncu, ticks.p, sink.p, ctx->st);          // warm-up (clocks, code)
  StageTimer tm(ctx->st);
  launch_issue(op, waves_per_simd, iters, ncu, ticks.p, sink.p, ctx->st);
  const float t = tm.stop();
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> h((size_t)nw);
  HIPCHK(hipMemcpy(h.data(), ticks.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::sort(h.begin(), h.end());
  if (cycles_per_instr) *cycles_per_instr = (double)h[h.size() / 2] / (64.0 * (double)iters);
  if (ms) *ms = t;
  return ITSX_OK;
}

int itsx_debug_detmath(itsx_ctx *ctx, const double *x, int64_t n, double *out_log, double *out_exp)
{
  CTXCHK(ctx && x && out_log && out_exp && n >= 0);
  HIPCHK(hipSetDevice(ctx->device));
  DBuf<double> dx, dl, de;
  HIPCHK(dx.alloc((size_t)n + 1)); HIPCHK(dl.alloc((size_t)n + 1)); HIPCHK(de.alloc((size_t)n + 1));
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)n * 8, hipMemcpyHostToDevice, ctx->st));
    launch_detmath(dx.p, n, dl.p, de.p, ctx->st);
    HIPCHK(hipMemcpyAsync(out_log, dl.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(out_exp, de.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->st));
  }
  HIPCHK(hipStreamSynchronize(ctx->st));
  return ITSX_OK;
}

int itsx_debug_dust(itsx_ctx *ctx, uint8_t *masked)
{
  CTXCHK(ctx && masked);
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->N;
  if (n == 0) return ITSX_OK;
  DBuf<uint32_t> dm;
  HIPCHK(dm.alloc((size_t)ctx->h_woff[n] + 1));
  launch_dust(ctx->rd, dm.p, ctx->st);
  std::vector<uint32_t> h((size_t)ctx->h_woff[n] + 1);
  HIPCHK(hipMemcpyAsync(h.data(), dm.p, h.size() * 4, hipMemcpyDeviceToHost, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  HIPCHK(hipGetLastError());
  int64_t o = 0;
  for (int64_t r = 0; r < n; r++)
    for (int p = 0; p < ctx->h_len[r]; p++) masked[o++] = (uint8_t)((h[(size_t)ctx->h_woff[r] + (p >> 5)] >> (p & 31)) & 1u);
  return ITSX_OK;
}

int itsx_debug_logf(itsx_ctx *ctx, const float *x, int64_t n, float *out)
{
  CTXCHK(ctx && x && out && n >= 0);
  HIPCHK(hipSetDevice(ctx->device));
  DBuf<float> dx, dy;
  HIPCHK(dx.alloc((size_t)n + 1)); HIPCHK(dy.alloc((size_t)n + 1));
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice, ctx->st));
    launch_logf_fast(dx.p, n, ctx->d_logtab.p, dy.p, ctx->st);
    HIPCHK(hipMemcpyAsync(out, dy.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->st));
  }
  HIPCHK(hipStreamSynchronize(ctx->st));
  return ITSX_OK;
}

int itsx_debug_scan(itsx_ctx *ctx, const int32_t *in, int64_t n, int32_t *out, int in_place)
{
  CTXCHK(ctx && n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || (in && out)));
  HIPCHK(hipSetDevice(ctx->device));
  if (n == 0) return ITSX_OK;
  DBuf<int32_t> din, dout, tmp;
  HIPCHK(din.alloc((size_t)n)); HIPCHK(dout.alloc((size_t)n)); HIPCHK(tmp.alloc((size_t)scan_tmp_elems(n)));
  HIPCHK(hipMemcpyAsync(din.p, in, (size_t)n * 4, hipMemcpyHostToDevice, ctx->st));
  int32_t *res = in_place ? din.p : dout.p;
  launch_exclusive_scan(din.p, res, n, tmp.p, ctx->st);
  HIPCHK(hipMemcpyAsync(out, res, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  HIPCHK(hipGetLastError());
  return ITSX_OK;
}

int itsx_debug_select(itsx_ctx *ctx, int mode, const int32_t *pairs, int64_t NP, const int64_t *seg_start, int32_t P, uint8_t *done, const uint32_t *b10,
                      const int8_t *cls, int32_t ncls, const unsigned long long *group, int64_t n_group, const int32_t *sorted_uniq, int64_t n_sorted,
                      const int32_t *slot_of_prof, const uint32_t *cutoff, int32_t n_slots, int64_t *out_seg, int32_t *out_pairs, int64_t out_cap,
                      unsigned long long *out_keys, int32_t *out_vals, int64_t *out_n)
{
  CTXCHK(ctx && mode >= 0 && mode <= 3 && pairs && NP > 0 && NP < ((int64_t)1 << 31) && seg_start && P > 0 && done && b10 && out_n && out_cap >= 0);
  CTXCHK(mode > 1 || (cls && ncls > 0 && group && n_group > 0 && (mode == 0 || (sorted_uniq && n_sorted > 0))));
  CTXCHK(mode <= 1 || (slot_of_prof && n_slots > 0 && (mode == 3 || cutoff)));
  CTXCHK(mode <= 2 ? (out_seg && out_pairs) : (out_keys && out_vals));
  // every index a kernel follows is checked here: the lists are a test's own
  const PairRec *hp = (const PairRec *)pairs;
  if (seg_start[0] != 0 || seg_start[P] != NP) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_select: the segments do not cover the list");
  for (int p = 0; p < P; p++) {
    if (seg_start[p + 1] < seg_start[p] || (seg_start[p + 1] & 63)) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_select: segment " + std::to_string(p) + " is not a whole number of chunks of 64");
    if (mode >= 2 && (slot_of_prof[p] < -1 || slot_of_prof[p] >= n_slots)) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_select: slot of profile " + std::to_string(p));
    if (mode <= 1 && (cls[p] < 0 || cls[p] >= ncls)) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_select: class of profile " + std::to_string(p));
    for (int64_t i = seg_start[p]; i < seg_start[p + 1]; i++) {
      const PairRec &r = hp[i];
      if (r.prof < 0) continue;
      bool ok = r.prof == p && r.useq >= 0;
      if (ok && mode == 0) ok = (int64_t)r.useq * ncls + cls[p] < n_group;
      if (ok && mode == 1) ok = r.useq < n_sorted && sorted_uniq[r.useq] >= 0 && (int64_t)sorted_uniq[r.useq] * ncls + cls[p] < n_group;
      if (!ok) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_select: pair " + std::to_string(i) + " points outside the tables");
    }
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  DBuf<PairRec> dp; DBuf<uint8_t> dd; DBuf<uint32_t> db, dcut, dthr; DBuf<int8_t> dcls; DBuf<unsigned long long> dg; DBuf<int32_t> dsu, dslot; DBuf<int64_t> dseg;
  HIPCHK(dp.alloc((size_t)NP)); HIPCHK(dd.alloc((size_t)NP)); HIPCHK(db.alloc((size_t)NP)); HIPCHK(dseg.alloc((size_t)P + 1));
  HIPCHK(hipMemcpyAsync(dp.p, pairs, (size_t)NP * sizeof(PairRec), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dd.p, done, (size_t)NP, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(db.p, b10, (size_t)NP * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dseg.p, seg_start, ((size_t)P + 1) * 8, hipMemcpyHostToDevice, st));
  if (mode <= 1) {
    HIPCHK(dcls.alloc((size_t)P)); HIPCHK(dg.alloc((size_t)n_group));
    HIPCHK(hipMemcpyAsync(dcls.p, cls, (size_t)P, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dg.p, group, (size_t)n_group * 8, hipMemcpyHostToDevice, st));
    if (mode == 1) { HIPCHK(dsu.alloc((size_t)n_sorted)); HIPCHK(hipMemcpyAsync(dsu.p, sorted_uniq, (size_t)n_sorted * 4, hipMemcpyHostToDevice, st)); }
  } else {
    HIPCHK(dslot.alloc((size_t)P)); HIPCHK(dcut.alloc((size_t)2 * n_slots));
    HIPCHK(hipMemcpyAsync(dslot.p, slot_of_prof, (size_t)P * 4, hipMemcpyHostToDevice, st));
    if (cutoff) HIPCHK(hipMemcpyAsync(dcut.p, cutoff, (size_t)2 * n_slots * 4, hipMemcpyHostToDevice, st));
  }
  { const int rc = select_alloc(ctx, NP); if (rc != ITSX_OK) return rc; }
  if (mode == 3) {
    const int64_t nch = NP >> 6;
    launch_topup_keys(dp.p, NP, dd.p, db.p, dslot.p, ctx->l_smask.p, ctx->l_scnt.p, nullptr, nullptr, nullptr, st);
    launch_exclusive_scan(ctx->l_scnt.p, ctx->l_spos.p, nch + 1, ctx->l_scan.p, st);
    int32_t M = 0;
    HIPCHK(hipMemcpyAsync(&M, ctx->l_spos.p + nch, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *out_n = M;
    if (M > 0 && M <= out_cap) {
      DBuf<unsigned long long> dk; DBuf<int32_t> dv;
      HIPCHK(dk.alloc((size_t)M)); HIPCHK(dv.alloc((size_t)M));
      launch_topup_keys(dp.p, NP, dd.p, db.p, dslot.p, ctx->l_smask.p, ctx->l_scnt.p, ctx->l_spos.p, dk.p, dv.p, st);
      HIPCHK(hipMemcpyAsync(out_keys, dk.p, (size_t)M * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out_vals, dv.p, (size_t)M * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipGetLastError());
    return ITSX_OK;
  }
  if (mode <= 1) {
    LazyArgs la{};
    la.pairs = dp.p; la.NP = NP; la.cls = dcls.p; la.ncls = ncls; la.sorted_uniq = dsu.p; la.b10 = db.p;
    la.gtop = mode == 0 ? dg.p : nullptr; la.ngroups = mode == 0 ? n_group : 0; la.bestc = mode == 1 ? dg.p : nullptr; la.done = dd.p;
    if (mode == 1) { HIPCHK(dthr.alloc((size_t)n_sorted * ncls + 1)); la.thr = dthr.p; la.nthr = (int64_t)n_sorted * ncls; la.nbest = n_group; } la.smask = ctx->l_smask.p; la.scnt = ctx->l_scnt.p;
    launch_lazy_mark(la, mode, st);
  } else launch_topup_mark(dp.p, NP, dd.p, db.p, dslot.p, dcut.p, ctx->l_smask.p, ctx->l_scnt.p, st);
  PairList sub; int64_t nsel = 0;
  const std::vector<int64_t> hseg(seg_start, seg_start + P + 1);
  { const int rc = select_compact(ctx, dp.p, NP, P, hseg, dseg.p, sub, nsel); if (rc != ITSX_OK) return rc; }
  for (int p = 0; p <= P; p++) out_seg[p] = sub.seg_start[(size_t)p];
  *out_n = sub.NP;
  HIPCHK(hipMemcpyAsync(done, dd.p, (size_t)NP, hipMemcpyDeviceToHost, st));
  if (sub.NP > 0 && sub.NP <= out_cap) HIPCHK(hipMemcpyAsync(out_pairs, sub.pairs, (size_t)sub.NP * sizeof(PairRec), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return ITSX_OK;
}

int64_t itsx_debug_lazy_pairs(itsx_ctx *ctx, itsx_lazy_pair *out, int64_t cap, int32_t *tenths_bias)
{
  if (!ctx) return ITSX_E_ARG;
  if (tenths_bias) *tenths_bias = LAZY_TENTHS_BIAS;
  const auto &tu = ctx->topup;
  // the buffers lazy_rounds left (what the top-up round reads): only a lazy search of one chunk still has its whole list in them
  if (!ctx->searched() || !ctx->lazy || ctx->injected || !tu.list_live || ctx->n_chunks != 1 || ctx->S != 1 || tu.NP <= 0)
    SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_lazy_pairs: the pair list of a lazy search of one chunk and one sample is not in the buffers");
  const int64_t NP = tu.NP;
  if (!out || cap < NP) return NP;
  if (ctx->d_pairs.n < (size_t)NP || ctx->l_fb.n < (size_t)NP || ctx->l_b10.n < (size_t)NP || ctx->l_done.n < (size_t)NP || ctx->s_Lcap <= 0 || ctx->d_lt.n < (size_t)ctx->s_Lcap)
    SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_lazy_pairs: the lazy stage's buffers are smaller than its list");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  std::vector<PairRec> hp((size_t)NP); std::vector<float> fb((size_t)NP); std::vector<uint32_t> b10((size_t)NP); std::vector<uint8_t> done((size_t)NP);
  std::vector<int32_t> sorted((size_t)std::max(tu.Uc, 1)); std::vector<LenTables> lt((size_t)ctx->s_Lcap);
  const int32_t *d_sorted = (ctx->share_on ? ctx->sh_order.p : ctx->d_sorted_uniq.p) + tu.u0;
  HIPCHK(hipMemcpyAsync(hp.data(), ctx->d_pairs.p, (size_t)NP * sizeof(PairRec), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(fb.data(), ctx->l_fb.p, (size_t)NP * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(b10.data(), ctx->l_b10.p, (size_t)NP * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(done.data(), ctx->l_done.p, (size_t)NP, hipMemcpyDeviceToHost, st));
  if (tu.Uc > 0) HIPCHK(hipMemcpyAsync(sorted.data(), d_sorted, (size_t)tu.Uc * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(lt.data(), ctx->d_lt.p, (size_t)ctx->s_Lcap * sizeof(LenTables), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < NP; i++) {
    const PairRec &r = hp[(size_t)i];
    itsx_lazy_pair &o = out[i];
    memset(&o, 0, sizeof(o));
    o.rep = (r.prof >= 0 && r.useq >= 0 && r.useq < tu.Uc) ? (int64_t)sorted[(size_t)r.useq] : -1;
    o.prof = r.prof; o.L = r.L; o.xj = r.xj; o.fb = fb[(size_t)i]; o.b10 = b10[(size_t)i]; o.done = done[(size_t)i];
    if (r.prof >= 0 && r.L > 0 && r.L < ctx->s_Lcap) { o.nullsc = lt[(size_t)r.L].nullsc; o.lazy_c = lt[(size_t)r.L].lazy_c; }
  }
  return NP;
}

int itsx_debug_region_keys(itsx_ctx *ctx, const int32_t *regions, int64_t n_regions, const int32_t *pairs, int64_t n_pairs, int32_t *rep_region, int32_t *is_uniq)
{
  CTXCHK(ctx && regions && n_regions > 0 && n_regions < ((int64_t)1 << 30) && pairs && n_pairs > 0 && rep_region && is_uniq);
  if (ctx->N <= 0) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_region_keys: no reads are loaded");
  const RegionRec *hr = (const RegionRec *)regions; const PairRec *hp = (const PairRec *)pairs;
  for (int64_t g = 0; g < n_regions; g++) {
    if (hr[g].pair < 0) continue;
    bool ok = hr[g].pair < n_pairs;
    if (ok) { const PairRec &r = hp[hr[g].pair]; ok = r.useq >= 0 && r.useq < ctx->N && hr[g].ienv >= 1 && hr[g].jenv >= hr[g].ienv && hr[g].jenv <= ctx->h_len[(size_t)r.useq]; }
    if (!ok) SET_ERR(ctx, ITSX_E_ARG, "itsx_debug_region_keys: region " + std::to_string(g) + " points outside its read");
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->st;
  std::vector<int32_t> ident((size_t)ctx->N);
  std::iota(ident.begin(), ident.end(), 0);
  DBuf<RegionRec> dr; DBuf<PairRec> dp; DBuf<int32_t> did, dvals, drep, duq; DBuf<unsigned long long> dkeys; DBuf<uint32_t> dslot;
  const uint64_t tsize = region_table_size(n_regions);
  HIPCHK(dr.alloc((size_t)n_regions)); HIPCHK(dp.alloc((size_t)n_pairs)); HIPCHK(upload(did, ident, st));
  HIPCHK(dkeys.alloc(tsize)); HIPCHK(dvals.alloc(tsize)); HIPCHK(dslot.alloc((size_t)n_regions)); HIPCHK(drep.alloc((size_t)n_regions)); HIPCHK(duq.alloc((size_t)n_regions));
  HIPCHK(hipMemcpyAsync(dr.p, regions, (size_t)n_regions * sizeof(RegionRec), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dp.p, pairs, (size_t)n_pairs * sizeof(PairRec), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(dkeys.p, 0, tsize * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(dvals.p, 0x7f, tsize * sizeof(int32_t), st));
  launch_region_keys(ctx->rd, dr.p, n_regions, dp.p, did.p, did.p, dkeys.p, dvals.p, tsize - 1, dslot.p, st);
  launch_region_resolve(ctx->rd, dr.p, n_regions, dp.p, did.p, did.p, dvals.p, dslot.p, drep.p, duq.p, st);
  HIPCHK(hipMemcpyAsync(rep_region, drep.p, (size_t)n_regions * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(is_uniq, duq.p, (size_t)n_regions * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return ITSX_OK;
}

}  // extern "C"
