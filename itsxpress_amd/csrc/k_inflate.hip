// k_inflate.hip -- gzip files made of independent members, inflated on the device (itsx_inflate_device; the loaders' opt-in path).
// k_inflate_find flags the positions of the uploaded bytes that pass the strict member-start test (inflate_codes.h: ic_candidate) and
// compacts them in order into a 64-bit list: a count per tile, k_inflate_scan over the tiles, and the same kernel again to write.
// k_inflate: one wave (a 64-thread workgroup) per member, grid-strided over the members in the order the host gives (longest spans
// first).  Per member:
//   * lane 0 runs inflate_codes.h's decoder (ic_begin / ic_next / ic_finish, the code the host routine runs) and queues up to 64
//     tokens in LDS; a token has passed every check when it is queued (inside the member's text, distance inside what THIS member has
//     produced -- the ring still holds the previous member's bytes, the produced count is what bounds a distance);
//   * the wave executes the queue in order: the literals up to the next match are stored by their own lanes, a match or a stored run
//     is copied by as many lanes as it has bytes (distance < length: byte j comes from src + j % distance).  Every back-reference is
//     read from the 32 KiB ring in LDS: global memory is write-only, so nothing depends on when a store becomes visible;
//   * after every batch the ring's new bytes leave for the text as aligned dwords (the ring is indexed in the text's own alignment),
//     the few bytes before the first and after the last whole dword as bytes, and CRC-32 is folded over what leaves: lane L takes the
//     remainder of its dword times x^(32 (63 - L)), the wave XORs them, and the running register moves on by the round's bytes.
// Invariants: no load lies outside [c, c_end) of the member's span (the decoder's, see inflate_codes.h; a stored run's source was
// checked against c_end when its block began), and no store outside [o, o + isize): a queued token ends at or before isize, and the
// flush moves bytes [flushed, pos) with pos <= isize.  Every turn of every loop consumes at least one input bit or stops.
#include "k_api.h"
#include "k_scan.h"
#include "inflate_codes.h"

#include <algorithm>

namespace itsx {

using namespace itsx_ic;

constexpr int IF_BLOCK = 256, IF_ITEMS = 16;
constexpr int IF_TILE = INFLATE_FIND_TILE;
static_assert(IF_TILE == IF_BLOCK * IF_ITEMS, "a tile is one block's positions");

// list null: counts[tile] = candidates of the tile; else their positions to list[base[tile] ...], in order.  gz is 16-byte aligned.
__global__ __launch_bounds__(IF_BLOCK) void k_inflate_find(const uint8_t *__restrict__ gz, int64_t n, int64_t *__restrict__ counts,
                                                           const int64_t *__restrict__ base, int64_t *__restrict__ list)
{
  const int64_t ntiles = (n + IF_TILE - 1) / IF_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t p0 = tile * IF_TILE + (int64_t)threadIdx.x * IF_ITEMS;
    uint32_t flags = 0;
    if (p0 + IF_ITEMS <= n) {
      const uint4 w = *reinterpret_cast<const uint4 *>(gz + p0);
      const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int k = 0; k < IF_ITEMS; k++)
        if (((ws[k >> 2] >> (8 * (k & 3))) & 255u) == 0x1fu && ic_candidate(gz, n, p0 + k)) flags |= 1u << k;
    } else {
      for (int k = 0; k < IF_ITEMS; k++) if (p0 + k < n && gz[p0 + k] == 0x1f && ic_candidate(gz, n, p0 + k)) flags |= 1u << k;
    }
    const int64_t v[1] = {(int64_t)__popc(flags)};
    int64_t ex[1], tot[1];
    block_scan64<1, IF_BLOCK>(v, ex, tot);
    if (!list) { if (threadIdx.x == 0) counts[tile] = tot[0]; }
    else {
      int64_t at = base[tile] + ex[0];
      for (int k = 0; k < IF_ITEMS; k++) if (flags & (1u << k)) list[at++] = p0 + k;
    }
  }
}

// base[t] = candidates before tile t, *total = all of them (one block)
__global__ __launch_bounds__(IF_BLOCK) void k_inflate_scan(const int64_t *__restrict__ counts, int64_t ntiles, int64_t *__restrict__ base,
                                                           int64_t *__restrict__ total)
{
  int64_t carry = 0;
  for (int64_t t0 = 0; t0 < ntiles; t0 += IF_BLOCK) {
    const int64_t i = t0 + threadIdx.x;
    const int64_t v[1] = {i < ntiles ? counts[i] : 0};
    int64_t ex[1], tot[1];
    block_scan64<1, IF_BLOCK>(v, ex, tot);
    if (i < ntiles) base[i] = carry + ex[0];
    carry += tot[0];
  }
  if (threadIdx.x == 0) *total = carry;
}

constexpr int IN_Q = 64;                        // tokens of a batch: a wave's worth
constexpr uint32_t IN_MASK = IC_WINDOW - 1;
struct InflateShared {
  uint32_t ring[IC_WINDOW / 4];
  IcDecoder dec;
  uint32_t crctab[256];
  uint32_t xw[65];                              // xw[k] = x^(32 k) mod P, as the CRC register keeps polynomials
  IcToken q[IN_Q];
  int32_t nq, why, done;
};
static_assert(sizeof(InflateShared) <= 40 * 1024, "four workgroups fit a CU's 160 KiB of LDS");
static_assert(IN_Q * 258 + 4 <= IC_WINDOW, "a batch's bytes and the unflushed tail never reach back over the window");

__global__ __launch_bounds__(64) void k_inflate(InflateArgs a)
{
  __shared__ InflateShared sh;
  const int lane = threadIdx.x;
  uint8_t *ringb = reinterpret_cast<uint8_t *>(sh.ring);
  for (int i = lane; i < 256; i += 64) sh.crctab[i] = itsx_dc::dc_crc_table_entry((uint32_t)i);
  if (lane == 0) {
    uint32_t xp[itsx_dc::CRC_POWERS];
    itsx_dc::dc_crc_powers(xp);                 // xp[2] = x^32
    sh.xw[0] = 0x80000000u;
    for (int k = 1; k <= 64; k++) sh.xw[k] = itsx_dc::dc_gf2_mulmod(sh.xw[k - 1], xp[2]);
  }
  __syncthreads();
  const uint32_t xlane = sh.xw[63 - lane];
  int32_t seq = 0;                                // members this workgroup has decoded before
  for (int m = blockIdx.x; m < a.nmem; m += gridDim.x, seq++) {
    const InflateMember mb = a.mem[m];
    const uint8_t *c = a.gz + mb.c;
    uint8_t *o = a.text + mb.o;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(o) & 3u);      // ring index of text byte q: (q + mis) & IN_MASK
    uint32_t *o4 = reinterpret_cast<uint32_t *>(o - mis);                       // dword w of this view holds text bytes 4 w - mis ...
    if (lane == 0) { sh.why = ic_begin(sh.dec, c, a.gz + mb.c_end, mb.isize); sh.done = 0; sh.nq = 0; }
    __syncthreads();
    int32_t why = sh.why;
    bool done = false;
    uint32_t pos = 0, flushed = 0, crc = 0xffffffffu;                           // the same in every lane
    while (!why && !done) {
      if (lane == 0) {
        IcHot h = sh.dec.h;                      // the bit reader and the counts in registers for the batch
        int nq = 0, e = 0;
        int32_t r = IC_OK;
        while (nq < IN_Q) {
          IcToken t;
          r = ic_next(sh.dec, h, t);
          if (r) break;
          if (ic_tok_kind(t) == IC_TOK_END) { e = 1; break; }
          sh.q[nq++] = t;
        }
        sh.dec.h = h;
        sh.nq = nq; sh.why = r; sh.done = e;
      }
      __syncthreads();
      why = sh.why; done = sh.done != 0;
      const int nq = sh.nq;
      if (why) break;
      // ---- where each token's bytes go
      IcToken t;
      t.kind_len = 0; t.val = 0;
      if (lane < nq) t = sh.q[lane];
      const uint32_t len = lane < nq ? ic_tok_len(t) : 0u;
      const int kind = ic_tok_kind(t);
      uint32_t inc = len;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(inc, d, 64); if (lane >= d) inc += u; }
      const uint32_t at = pos + inc - len;
      const uint32_t total = __shfl(inc, 63, 64);
      // ---- in order: the literals up to the next match by their own lanes, then the match by all
      unsigned long long copies = __ballot(lane < nq && kind != IC_TOK_LIT);
      int prev = -1;
      for (;;) {
        const int k = copies ? __ffsll((long long)copies) - 1 : nq;
        if (lane < nq && kind == IC_TOK_LIT && lane > prev && lane < k) ringb[(at + mis) & IN_MASK] = (uint8_t)t.val;
        __syncthreads();
        if (k >= nq) break;
        copies &= copies - 1;
        const uint32_t lk = __shfl(len, k, 64), ak = __shfl(at, k, 64), vk = __shfl(t.val, k, 64);
        const int kk = __shfl(kind, k, 64);
        if (kk == IC_TOK_STORED) {
          for (uint32_t j = (uint32_t)lane; j < lk; j += 64) ringb[(ak + j + mis) & IN_MASK] = c[vk + j];
        } else {
          // 64 bytes a turn, every lane's load before any lane's store: with a distance in (32768 - 258, 32768) a byte's source slot
          // is the destination slot of a HIGHER byte of the same match (the ring is exactly one window), so no store of a turn may
          // come before a load of that turn; the stores of earlier turns only touch lower bytes' slots
          for (uint32_t j0 = 0; j0 < lk; j0 += 64) {
            const uint32_t j = j0 + (uint32_t)lane;
            const bool on = j < lk;
            const uint32_t src = ak - vk + (vk < lk ? j % vk : j);
            const uint8_t x = on ? ringb[(src + mis) & IN_MASK] : (uint8_t)0;
            __syncthreads();
            if (on) ringb[(ak + j + mis) & IN_MASK] = x;
          }
        }
        __syncthreads();
        prev = k;
      }
      pos += total;
      // ---- the new bytes leave: bytes up to the first whole dword (once), whole dwords, and at the member's end the rest
      while (flushed < pos && ((flushed + mis) & 3u)) {
        const uint8_t x = ringb[(flushed + mis) & IN_MASK];
        if (lane == 0) o[flushed] = x;
        crc = sh.crctab[(crc ^ x) & 255u] ^ (crc >> 8);
        flushed++;
      }
      const uint32_t nd = (pos - flushed) >> 2;
      const uint32_t w0 = (flushed + mis) >> 2;
      for (uint32_t r0 = 0; r0 < nd; r0 += 64) {
        const uint32_t k = nd - r0 < 64u ? nd - r0 : 64u;
        const int i = lane - (64 - (int)k);                                    // the round's dwords sit in the last k lanes
        uint32_t part = 0;
        if (i >= 0) {
          const uint32_t w = w0 + r0 + (uint32_t)i;
          const uint32_t v = sh.ring[w & (IC_WINDOW / 4 - 1)];
          o4[w] = v;
          uint32_t p = v;
#pragma unroll
          for (int b = 0; b < 4; b++) p = sh.crctab[p & 255u] ^ (p >> 8);
          part = itsx_dc::dc_gf2_mulmod(xlane, p);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part ^= __shfl_xor(part, d, 64);
        crc = itsx_dc::dc_gf2_mulmod(sh.xw[k], crc) ^ part;
      }
      flushed += 4 * nd;
      if (done) {
        while (flushed < pos) {
          const uint8_t x = ringb[(flushed + mis) & IN_MASK];
          if (lane == 0) o[flushed] = x;
          crc = sh.crctab[(crc ^ x) & 255u] ^ (crc >> 8);
          flushed++;
        }
      }
    }
    __syncthreads();
    if (lane == 0) {
      a.status[mb.id] = why ? why : ic_finish(sh.dec, sh.dec.h, ~crc);
      a.where[mb.id] = ((int64_t)blockIdx.x << 32) | (int64_t)seq;
    }
    __syncthreads();
  }
}

void launch_inflate_find(const uint8_t *gz, int64_t n, int64_t *counts, const int64_t *base, int64_t *list, hipStream_t st)
{
  if (n <= 0) return;
  const int64_t ntiles = (n + IF_TILE - 1) / IF_TILE;
  hipLaunchKernelGGL(k_inflate_find, dim3((unsigned)std::min<int64_t>(ntiles, 65536)), dim3(IF_BLOCK), 0, st, gz, n, counts, base, list);
}

void launch_inflate_scan(const int64_t *counts, int64_t ntiles, int64_t *base, int64_t *total, hipStream_t st)
{
  hipLaunchKernelGGL(k_inflate_scan, dim3(1), dim3(IF_BLOCK), 0, st, counts, ntiles, base, total);
}

void launch_inflate(const InflateArgs &a, int grid, hipStream_t st)
{
  if (a.nmem <= 0) return;
  hipLaunchKernelGGL(k_inflate, dim3((unsigned)std::max(1, std::min(grid, a.nmem))), dim3(64), 0, st, a);
}

}  // namespace itsx
