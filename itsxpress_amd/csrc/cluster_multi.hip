// cluster_multi.hip -- the centroid stream of greedy clustering spread over several contexts (itsx_cluster_multi, cluster_multi.h).
//
// Why the answer is the one-context answer, bit for bit:
//  * a strand's candidate list is the 32 best rank keys cand_key(count, length, position) over every existing centroid; the
//    position is unique, so the keys are totally ordered, and the 32 best of all centroids are the 32 best of the union of every
//    shard's own 32 best;
//  * a shard streams its columns with the unchanged k_cl_stream (mode 1) and cuts its lists with k_cl_topk(..., 0) between chunks.
//    Its thresholds come from its own lists, so they only drop keys that cannot be among the shard's own 32 best.  The scan compares
//    the high half of the key with a strict '>', which is exact only because a later column that ties on count and length loses on
//    position: a shard's columns therefore stay in increasing position order (they are adopted in column order);
//  * the count of (strand, centroid) needs only the centroid's words and the window's query index, which every shard builds from the
//    window's word lists (klist / nk / canon, copied from the leader).
// Everything after the candidate lists -- walk, alignments, validation, resolve, cuts -- stays on the leader, unchanged.
//
// Ownership: column c belongs to shard c % shards (round robin keeps the shards' word counts close on any read order).  Rolled-back
// columns (cw_n == 0) are never adopted.  Shard 0 lives on the leader and shares its query index, thresholds and lists.
#include <algorithm>
#include <cstdio>
#include "cluster_multi.h"

namespace itsx {

// ------------------------------------------------------------------ kernels
// The helpers' <= 32 keys per strand join shard 0's list on the leader: keys [H][CL_QS_MAX][32], counts [H][CL_QS_MAX + 1] (the
// last entry: the helper's overflow flag).  One wave per strand; k_cl_topk(..., 1) then cuts the union to its 32 best.
__global__ __launch_bounds__(256) void k_cl_merge_keys(ClusterArgs a, const unsigned long long *keys, const int32_t *cnt, int32_t H)
{
  const int lane = threadIdx.x & 63;
  const int qs = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qs >= 2 * a.nq) return;
  if (qs == 0 && lane == 0)
    for (int h = 0; h < H; h++) if (cnt[(size_t)h * (CL_QS_MAX + 1) + CL_QS_MAX]) a.ovf[0] = 1;
  int base = __shfl(lane == 0 ? a.ncand[qs] : 0, 0);
  unsigned long long *out = a.cand + (size_t)qs * a.ccap;
  for (int h = 0; h < H; h++) {
    int m = cnt[(size_t)h * (CL_QS_MAX + 1) + qs];
    m = m < 32 ? m : 32;
    if (lane < m && base + lane < a.ccap) out[base + lane] = keys[((size_t)h * CL_QS_MAX + qs) * 32 + lane];
    base += m;
  }
  if (lane == 0) a.ncand[qs] = base;                          // (more than ccap: k_cl_topk raises the overflow flag)
}

// One adopted column: its metadata and where its words are (src: in the window's word range; dst: in the shard's pool).
struct AdoptRec { int64_t src, dst; int32_t n, len, pos, pad; };
// A shard keeps the window's columns it owns: metadata appended at column col0 + j, words compacted into the shard's pool.  One wave
// per column.
__global__ __launch_bounds__(256) void k_cl_adopt(const AdoptRec *rec, int32_t nrec, int32_t col0, const uint16_t *src, uint16_t *pool,
                                                 int32_t *cent_len, int32_t *cent_pos, int32_t *cw_n, int64_t *cw_off)
{
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= nrec) return;
  const AdoptRec r = rec[j];
  for (int i = lane; i < r.n; i += 64) pool[r.dst + i] = src[r.src + i];
  if (lane == 0) { cent_len[col0 + j] = r.len; cent_pos[col0 + j] = r.pos; cw_n[col0 + j] = r.n; cw_off[col0 + j] = r.dst; }
}

// ------------------------------------------------------------------ host side
template <class T> struct Dev {
  T *p = nullptr; size_t cap = 0;
  Dev() = default;
  Dev(const Dev &) = delete;
  Dev &operator=(const Dev &) = delete;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n)                                 // (on the current device; the old contents are dropped)
  {
    if (n <= cap && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    hipError_t e = hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) cap = std::max<size_t>(n, 1); else p = nullptr;
    return e;
  }
  hipError_t grow(size_t n, size_t keep, hipStream_t st)     // the first `keep` elements survive; doubles at least
  {
    if (n <= cap && p) return hipSuccess;
    const size_t ncap = std::max(n, 2 * cap);
    T *q = nullptr;
    hipError_t e = hipMalloc((void **)&q, ncap * sizeof(T));
    if (e != hipSuccess) return e;
    if (keep) e = hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipFree(q); return e; }
    if (p) (void)hipFree(p);
    p = q; cap = ncap;
    return hipSuccess;
  }
};
template <class T> struct Pinned {
  T *p = nullptr; size_t cap = 0;
  Pinned() = default;
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  ~Pinned() { if (p) (void)hipHostFree(p); }
  hipError_t alloc(size_t n)
  {
    if (n <= cap && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    hipError_t e = hipHostMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) cap = std::max<size_t>(n, 1); else p = nullptr;
    return e;
  }
};

struct Shard {
  int dev = 0; hipStream_t st = nullptr;
  // the shard's columns (increasing position) and their words
  Dev<int32_t> cent_len, cent_pos, cw_n; Dev<int64_t> cw_off; Dev<uint16_t> pool;
  int32_t ncol = 0; int64_t pool_used = 0;
  Dev<int32_t> segtab;                                       // sg_base[0] = 0: k_cl_stream (seg == 0) reads column t
  Dev<AdoptRec> rec; Pinned<AdoptRec> h_rec;
  // helpers only: the window's word lists, query index, thresholds and candidate lists, and the copy of the words to adopt
  Dev<uint16_t> klist, qi_ent, wstage; Dev<int32_t> knk, canon, qi_cnt, qi_cur, qi_off, qi_hid, qi_nheavy, ncand, ntop, ovf, scan_tmp;
  Dev<uint32_t> qi_bm, tq, minm; Dev<unsigned long long> tkey, cand, keys32, pre_stats;
  int32_t ccap = 0;
  int64_t adopted_words = 0;
};

struct ShardSet {
  explicit ShardSet(size_t n) : sh(n) {}
  int ldev = 0; hipStream_t lst = nullptr;
  std::vector<Shard> sh;                                     // [0] on the leader
  Dev<unsigned long long> stage_keys; Dev<int32_t> stage_n;  // the helpers' keys and counts, on the leader
  Pinned<int32_t> h_len, h_pos, h_n; Pinned<int64_t> h_off;  // the window's new columns (fetch_columns)
  int32_t nqs_max = 0, kcap = 0;
  int64_t bytes = 0;                                         // copied between contexts (and to the shards' tables)
};

#define SCHK(expr)                                                                                  \
  do {                                                                                              \
    hipError_t e__ = (expr);                                                                        \
    if (e__ != hipSuccess) { err_ = std::string(#expr) + ": " + hipGetErrorString(e__); (void)hipSetDevice(s.ldev); return e__; } \
  } while (0)

ClusterShards::ClusterShards(int leader_device, hipStream_t leader_st, const std::vector<Helper> &helpers) : s_(new ShardSet(helpers.size() + 1))
{
  ShardSet &s = *s_;
  s.ldev = leader_device; s.lst = leader_st;
  s.sh[0].dev = leader_device; s.sh[0].st = leader_st;
  for (size_t h = 0; h < helpers.size(); h++) { s.sh[h + 1].dev = helpers[h].device; s.sh[h + 1].st = helpers[h].st; }
}
ClusterShards::~ClusterShards()
{
  sync();
  (void)hipStreamSynchronize(s_->lst);                       // (shard 0's adoption runs on the leader's stream)
}
int ClusterShards::shards() const { return (int)s_->sh.size(); }
void ClusterShards::sync()
{
  ShardSet &s = *s_;
  for (size_t i = 1; i < s.sh.size(); i++) { (void)hipSetDevice(s.sh[i].dev); (void)hipStreamSynchronize(s.sh[i].st); }
  (void)hipSetDevice(s.ldev);
}

hipError_t ClusterShards::init(const ClusterArgs &a, int32_t nqs, int64_t n_kept, int64_t pool_cap)
{
  ShardSet &s = *s_;
  const int nsh = (int)s.sh.size(), H = nsh - 1;
  s.nqs_max = nqs; s.kcap = a.kcap;
  const int32_t nq_max = nqs / 2;
  // peer access where the devices differ (hipMemcpyPeerAsync works without it, through the host)
  for (int i = 1; i < nsh; i++) {
    const int d = s.sh[i].dev;
    if (d == s.ldev) continue;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, d, s.ldev) == hipSuccess && can) { (void)hipSetDevice(d); (void)hipDeviceEnablePeerAccess(s.ldev, 0); }
    if (hipDeviceCanAccessPeer(&can, s.ldev, d) == hipSuccess && can) { (void)hipSetDevice(s.ldev); (void)hipDeviceEnablePeerAccess(d, 0); }
    (void)hipGetLastError();                                 // (already enabled is not an error here)
  }
  SCHK(hipSetDevice(s.ldev));
  SCHK(s.stage_keys.alloc((size_t)std::max(H, 1) * CL_QS_MAX * 32)); SCHK(s.stage_n.alloc((size_t)std::max(H, 1) * (CL_QS_MAX + 1)));
  SCHK(s.h_len.alloc((size_t)nq_max)); SCHK(s.h_pos.alloc((size_t)nq_max)); SCHK(s.h_n.alloc((size_t)nq_max)); SCHK(s.h_off.alloc((size_t)nq_max));
  for (int i = 0; i < nsh; i++) {
    Shard &x = s.sh[(size_t)i];
    SCHK(hipSetDevice(x.dev));
    const size_t cols = (size_t)(n_kept / nsh) + 2048;
    SCHK(x.cent_len.alloc(cols)); SCHK(x.cent_pos.alloc(cols)); SCHK(x.cw_n.alloc(cols)); SCHK(x.cw_off.alloc(cols));
    SCHK(x.pool.alloc((size_t)std::max<int64_t>(pool_cap / nsh, 1 << 20)));
    SCHK(x.segtab.alloc(10));
    SCHK(hipMemsetAsync(x.segtab.p, 0, 10 * sizeof(int32_t), x.st));
    SCHK(x.rec.alloc((size_t)nq_max)); SCHK(x.h_rec.alloc((size_t)nq_max));
    if (i == 0) continue;
    SCHK(x.klist.alloc((size_t)nqs * a.kcap)); SCHK(x.knk.alloc((size_t)nqs)); SCHK(x.canon.alloc((size_t)nq_max + 1));
    SCHK(x.qi_cnt.alloc(65537)); SCHK(x.qi_cur.alloc(65536)); SCHK(x.qi_off.alloc(65537));
    SCHK(x.qi_ent.alloc((size_t)nqs * a.kcap + 65536 * 8 + 64));
    SCHK(x.qi_hid.alloc(65536)); SCHK(x.qi_nheavy.alloc(1)); SCHK(x.qi_bm.alloc((size_t)std::max(a.hcap, 1) * (CL_QS_MAX / 32)));
    SCHK(x.tq.alloc(CL_QS_MAX + 8)); SCHK(x.minm.alloc(CL_QS_MAX + 8)); SCHK(x.tkey.alloc((size_t)nqs)); SCHK(x.ncand.alloc((size_t)nqs));
    SCHK(x.ntop.alloc((size_t)nqs)); SCHK(x.ovf.alloc(1)); SCHK(x.keys32.alloc((size_t)nqs * 32));
    SCHK(x.scan_tmp.alloc((size_t)scan_tmp_elems(65537))); SCHK(x.pre_stats.alloc(16));
    SCHK(hipMemsetAsync(x.pre_stats.p, 0, 16 * sizeof(unsigned long long), x.st));
    SCHK(x.cand.alloc((size_t)nqs * a.ccap)); x.ccap = a.ccap;
    SCHK(x.wstage.alloc((size_t)nq_max * a.kcap));
  }
  for (int i = 1; i < nsh; i++) { SCHK(hipSetDevice(s.sh[(size_t)i].dev)); SCHK(hipStreamSynchronize(s.sh[(size_t)i].st)); }
  SCHK(hipSetDevice(s.ldev));
  return hipSuccess;
}

// mode-1 stream of a shard's columns [0, ncol) in the doubling chunks of cluster_run, the lists cut back between chunks and at the end
static void stream_columns(const ClusterArgs &b, int32_t ncol, hipStream_t st, int64_t &launches)
{
  for (int c0 = 0, step = 2048; c0 < ncol; step = std::min(step * 2, 1 << 20)) {
    const int c1 = std::min(ncol, c0 + step);
    launch_cl_stream(b, c0, c1, 1, st);
    launches++;
    launch_cl_topk(b, 0, st);
    c0 = c1;
  }
}

hipError_t ClusterShards::stream(const ClusterArgs &a, int64_t &launches)
{
  ShardSet &s = *s_;
  const int nsh = (int)s.sh.size();
  const size_t nqs = 2 * (size_t)a.nq;
  // the window's word lists (k_cl_kmers) and the leader's query index are on the device
  SCHK(hipStreamSynchronize(s.lst));
  int active = 0;
  for (int i = 1; i < nsh; i++) {
    Shard &x = s.sh[(size_t)i];
    if (x.ncol == 0 || a.nq == 0) continue;                  // (no columns yet: nothing to add)
    SCHK(hipSetDevice(x.dev));
    if (x.ccap != a.ccap) { SCHK(x.cand.alloc((size_t)s.nqs_max * a.ccap)); x.ccap = a.ccap; }   // the lists grew after an overflow
    ClusterArgs b{};
    b.nq = a.nq; b.strand_both = a.strand_both; b.G = 1; b.seg = 0;
    b.sg_q0 = b.sg_cb = b.sg_base = b.sg_C = b.sg_pos0 = x.segtab.p;
    b.cent_len = x.cent_len.p; b.cent_pos = x.cent_pos.p; b.cw_pool = x.pool.p; b.cw_off = x.cw_off.p; b.cw_n = x.cw_n.p;
    b.klist = x.klist.p; b.kcap = a.kcap; b.nk = x.knk.p; b.canon = x.canon.p;
    b.qi_cnt = x.qi_cnt.p; b.qi_cur = x.qi_cur.p; b.qi_off = x.qi_off.p; b.qi_ent = x.qi_ent.p;
    b.qi_hid = x.qi_hid.p; b.qi_nheavy = x.qi_nheavy.p; b.qi_bm = x.qi_bm.p; b.hcap = a.hcap; b.heavy_min = a.heavy_min;
    b.tq = x.tq.p; b.minm = x.minm.p; b.tkey = x.tkey.p; b.ncand = x.ncand.p; b.ntop = x.ntop.p; b.ovf = x.ovf.p;
    b.cand = x.cand.p; b.ccap = x.ccap; b.pre_stats = x.pre_stats.p;
    SCHK(hipMemcpyPeerAsync(x.klist.p, x.dev, a.klist, s.ldev, nqs * a.kcap * sizeof(uint16_t), x.st));
    SCHK(hipMemcpyPeerAsync(x.knk.p, x.dev, a.nk, s.ldev, nqs * sizeof(int32_t), x.st));
    SCHK(hipMemcpyPeerAsync(x.canon.p, x.dev, a.canon, s.ldev, (size_t)a.nq * sizeof(int32_t), x.st));
    launch_cl_qindex(b, x.scan_tmp.p, x.st);
    stream_columns(b, x.ncol, x.st, launches);
    // the lists are cut to <= 32 keys at row starts of pitch ccap: gathered into rows of 32, then sent to the leader
    SCHK(hipMemcpy2DAsync(x.keys32.p, 32 * sizeof(unsigned long long), x.cand.p, (size_t)x.ccap * sizeof(unsigned long long),
                          32 * sizeof(unsigned long long), nqs, hipMemcpyDeviceToDevice, x.st));
    SCHK(hipMemcpyPeerAsync(s.stage_keys.p + (size_t)active * CL_QS_MAX * 32, s.ldev, x.keys32.p, x.dev, nqs * 32 * sizeof(unsigned long long), x.st));
    SCHK(hipMemcpyPeerAsync(s.stage_n.p + (size_t)active * (CL_QS_MAX + 1), s.ldev, x.ncand.p, x.dev, nqs * sizeof(int32_t), x.st));
    SCHK(hipMemcpyPeerAsync(s.stage_n.p + (size_t)active * (CL_QS_MAX + 1) + CL_QS_MAX, s.ldev, x.ovf.p, x.dev, sizeof(int32_t), x.st));
    s.bytes += (int64_t)(nqs * a.kcap * 2 + nqs * 4 + (size_t)a.nq * 4 + nqs * 32 * 8 + nqs * 4 + 4);
    active++;
  }
  SCHK(hipSetDevice(s.ldev));
  // shard 0: the leader's query index, thresholds and lists, its own columns
  {
    Shard &x = s.sh[0];
    ClusterArgs b = a;
    b.cent_len = x.cent_len.p; b.cent_pos = x.cent_pos.p; b.cw_pool = x.pool.p; b.cw_off = x.cw_off.p; b.cw_n = x.cw_n.p;
    b.sg_base = x.segtab.p;
    stream_columns(b, x.ncol, s.lst, launches);
  }
  for (int i = 1; i < nsh; i++) {
    Shard &x = s.sh[(size_t)i];
    if (x.ncol == 0 || a.nq == 0) continue;
    SCHK(hipSetDevice(x.dev));
    SCHK(hipStreamSynchronize(x.st));
  }
  SCHK(hipSetDevice(s.ldev));
  if (active > 0) hipLaunchKernelGGL(k_cl_merge_keys, dim3((unsigned)((nqs + 3) / 4)), dim3(256), 0, s.lst, a, s.stage_keys.p, s.stage_n.p, active);
  return hipGetLastError();
}

hipError_t ClusterShards::fetch_columns(const ClusterArgs &a, int32_t c0)
{
  ShardSet &s = *s_;
  if (a.nq == 0) return hipSuccess;
  const size_t n = (size_t)a.nq;
  SCHK(hipMemcpyAsync(s.h_len.p, a.cent_len + c0, n * sizeof(int32_t), hipMemcpyDeviceToHost, s.lst));
  SCHK(hipMemcpyAsync(s.h_pos.p, a.cent_pos + c0, n * sizeof(int32_t), hipMemcpyDeviceToHost, s.lst));
  SCHK(hipMemcpyAsync(s.h_n.p, a.cw_n + c0, n * sizeof(int32_t), hipMemcpyDeviceToHost, s.lst));
  SCHK(hipMemcpyAsync(s.h_off.p, a.cw_off + c0, n * sizeof(int64_t), hipMemcpyDeviceToHost, s.lst));
  return hipSuccess;
}

hipError_t ClusterShards::adopt(const ClusterArgs &a, int32_t c0, int32_t consumed)
{
  ShardSet &s = *s_;
  const int nsh = (int)s.sh.size();
  for (int i = 0; i < nsh; i++) {
    Shard &x = s.sh[(size_t)i];
    // the columns this shard owns, in column (= position) order; their words keep their order in the window's range
    int32_t k = 0; int64_t words = 0, lo = INT64_MAX, hi = 0;
    for (int32_t j = (i - c0 % nsh + nsh) % nsh; j < consumed; j += nsh) {
      const int32_t n = s.h_n.p[j];
      if (n == 0) continue;                                   // rolled back
      AdoptRec &r = x.h_rec.p[k++];
      r.src = s.h_off.p[j]; r.dst = x.pool_used + words; r.n = n; r.len = s.h_len.p[j]; r.pos = s.h_pos.p[j]; r.pad = 0;
      lo = std::min(lo, r.src); hi = std::max(hi, r.src + n);
      words += n;
    }
    if (k == 0) continue;
    for (int32_t j = 0; j < k; j++) x.h_rec.p[j].src -= lo;
    SCHK(hipSetDevice(x.dev));
    SCHK(x.cent_len.grow((size_t)x.ncol + k, (size_t)x.ncol, x.st)); SCHK(x.cent_pos.grow((size_t)x.ncol + k, (size_t)x.ncol, x.st));
    SCHK(x.cw_n.grow((size_t)x.ncol + k, (size_t)x.ncol, x.st)); SCHK(x.cw_off.grow((size_t)x.ncol + k, (size_t)x.ncol, x.st));
    SCHK(x.pool.grow((size_t)(x.pool_used + words), (size_t)x.pool_used, x.st));
    SCHK(hipMemcpyAsync(x.rec.p, x.h_rec.p, (size_t)k * sizeof(AdoptRec), hipMemcpyHostToDevice, x.st));
    const uint16_t *src = a.cw_pool + lo;                     // shard 0: straight from the leader's pool
    if (i > 0) {
      SCHK(x.wstage.grow((size_t)(hi - lo), 0, x.st));
      SCHK(hipMemcpyPeerAsync(x.wstage.p, x.dev, a.cw_pool + lo, s.ldev, (size_t)(hi - lo) * sizeof(uint16_t), x.st));
      src = x.wstage.p;
      s.bytes += (hi - lo) * 2 + (int64_t)k * (int64_t)sizeof(AdoptRec);
    }
    hipLaunchKernelGGL(k_cl_adopt, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, x.st, x.rec.p, k, x.ncol, src, x.pool.p,
                       x.cent_len.p, x.cent_pos.p, x.cw_n.p, x.cw_off.p);
    SCHK(hipGetLastError());
    x.ncol += k; x.pool_used += words; x.adopted_words += words;
  }
  // the tables (host memory) are written again by the next window; the helpers read the leader's pool, which may move
  for (int i = 0; i < nsh; i++) { SCHK(hipSetDevice(s.sh[(size_t)i].dev)); SCHK(hipStreamSynchronize(s.sh[(size_t)i].st)); }
  SCHK(hipSetDevice(s.ldev));
  return hipSuccess;
}

std::string ClusterShards::debug_line(int64_t windows) const
{
  const ShardSet &s = *s_;
  std::string cols;
  for (const Shard &x : s.sh) cols += (cols.empty() ? "" : " ") + std::to_string(x.ncol);
  char buf[256];
  snprintf(buf, sizeof(buf), "[cluster] %d shards, columns per shard %s, %.2f MB copied per window\n", (int)s.sh.size(), cols.c_str(),
           windows > 0 ? (double)s.bytes / (double)windows / 1e6 : 0.0);
  return buf;
}

}  // namespace itsx
