// k_scan.h -- exclusive prefix of NV 64-bit values over the threads of a block, shared by the compactions (k_merge.hip: the merged
// pairs; k_orient.hip: the oriented reads).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace itsx {

// ex[k] = the sum of v[k] over the threads before this one (thread order), tot[k] = the block's sum: a wave64 shuffle scan, one LDS
// partial per wave, nothing assumed across waves but the barrier.  May be called again: the partials are free when it returns.
template <int NV, int BLOCK>
__device__ __forceinline__ void block_scan64(const int64_t (&v)[NV], int64_t (&ex)[NV], int64_t (&tot)[NV])
{
  static_assert(BLOCK % 64 == 0, "whole waves");
  __shared__ int64_t part[NV][BLOCK / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int64_t inc[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) inc[k] = v[k];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int64_t u = __shfl_up(inc[k], d, 64);
      if (lane >= d) inc[k] += u;
    }
  }
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < NV; k++) part[k][wid] = inc[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; k++) {
    int64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) {
      const int64_t p = part[k][w];
      if (w < wid) before += p;
      all += p;
    }
    ex[k] = before + inc[k] - v[k];
    tot[k] = all;
  }
  __syncthreads();
}

}  // namespace itsx
