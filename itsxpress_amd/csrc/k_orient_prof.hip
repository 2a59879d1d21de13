// k_orient_prof.hip -- f4, orientation by the profiles (itsx_orient_profiles): what turns the MSV filter's verdicts on a chunk of
// unique texts and on their reverse complements into a strand per unique, and the uniques' strands into the reads'.  The scans
// themselves are k_msv's, unshared; the reverse complements are k_orient.hip's (k_oa_words, k_oa_exc) into a scratch read set.
#include <algorithm>
#include "engine.h"
#include "k_api.h"

namespace itsx {

// 0, 1, 2, ...: the scratch read set is its own unique list and its own seed list
__global__ __launch_bounds__(256) void k_op_iota(int32_t *__restrict__ v, int32_t n)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = i;
}

// The verdict of the chunk's sorted position k: n_fwd / n_rev = the non-zero cells of its column in the forward / the reverse scan's
// res[Ppad][cU] over the P real profiles (the padding rows are never read), the strand by majority, 0 on a tie.  A thread per position:
// a wave's loads of one profile's row are 64 consecutive halfwords; four rows in flight per buffer.
__global__ __launch_bounds__(256) void k_op_verdict(const uint16_t *__restrict__ res_f, const uint16_t *__restrict__ res_r, int32_t cU, int32_t P,
                                                    const int32_t *__restrict__ sorted, int32_t *__restrict__ ucf, int32_t *__restrict__ ucr,
                                                    int8_t *__restrict__ ustrand)
{
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cU) return;
  int f = 0, r = 0, p = 0;
  for (; p + 4 <= P; p += 4) {
    uint16_t a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { a[i] = res_f[(size_t)(p + i) * cU + k]; b[i] = res_r[(size_t)(p + i) * cU + k]; }
#pragma unroll
    for (int i = 0; i < 4; i++) { f += a[i] != 0; r += b[i] != 0; }
  }
  for (; p < P; p++) { f += res_f[(size_t)p * cU + k] != 0; r += res_r[(size_t)p * cU + k] != 0; }
  const int32_t u = sorted[k];
  ucf[u] = f; ucr[u] = r;
  ustrand[u] = (int8_t)(f > r ? 1 : r > f ? -1 : 0);
}

// The reads from their uniques: a read that is its seed's reverse complement (rstrand < 0) gets the seed's strand negated and its
// counts swapped, a read the dereplication dropped 0 / 0 / 0.  keep (may be null): the strand the apply step takes, 0 as +1.
__global__ __launch_bounds__(256) void k_op_compose(int64_t n, const int32_t *__restrict__ uniq_of, const int8_t *__restrict__ rstrand,
                                                    const int32_t *__restrict__ ucf, const int32_t *__restrict__ ucr, const int8_t *__restrict__ ustrand,
                                                    int8_t *__restrict__ strand, int32_t *__restrict__ cf, int32_t *__restrict__ cr, int8_t *__restrict__ keep)
{
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int32_t u = uniq_of[r];
  int s = 0, f = 0, v = 0;
  if (u >= 0) {
    const bool flip = rstrand[r] < 0;
    s = flip ? -ustrand[u] : ustrand[u];
    f = flip ? ucr[u] : ucf[u];
    v = flip ? ucf[u] : ucr[u];
  }
  strand[r] = (int8_t)s; cf[r] = f; cr[r] = v;
  if (keep) keep[r] = (int8_t)(s < 0 ? -1 : 1);
}

void launch_op_iota(int32_t *v, int32_t n, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_op_iota, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, v, n);
}
void launch_op_verdict(const uint16_t *res_f, const uint16_t *res_r, int32_t cU, int32_t P, const int32_t *sorted, int32_t *ucf, int32_t *ucr,
                       int8_t *ustrand, hipStream_t st)
{
  if (cU > 0) hipLaunchKernelGGL(k_op_verdict, dim3((unsigned)((cU + 255) / 256)), dim3(256), 0, st, res_f, res_r, cU, P, sorted, ucf, ucr, ustrand);
}
void launch_op_compose(int64_t n, const int32_t *uniq_of, const int8_t *rstrand, const int32_t *ucf, const int32_t *ucr, const int8_t *ustrand,
                       int8_t *strand, int32_t *cf, int32_t *cr, int8_t *keep, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_op_compose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, uniq_of, rstrand, ucf, ucr, ustrand, strand, cf, cr, keep);
}

}  // namespace itsx
