// k_lines.h -- the newlines among 16 aligned bytes of a text, shared by the line indexes (k_trim.hip: a unit of a streamed writer;
// k_fastq.hip: a whole file's text).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace itsx {

// bit b of the result: byte p0 + b is a newline (p0: a multiple of 16; the text is readable to the end of its last 16-byte group).
// Bytes at or past nbytes never count.
__device__ __forceinline__ uint32_t trim_newlines16(const uint8_t *__restrict__ text, int64_t nbytes, int64_t p0)
{
  if (p0 >= nbytes) return 0;
  const uint4 v = *reinterpret_cast<const uint4 *>(text + p0);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
#pragma unroll
    for (int b = 0; b < 4; b++) if (((w[k] >> (8 * b)) & 255u) == (uint32_t)'\n') m |= 1u << (4 * k + b);
  }
  const int64_t left = nbytes - p0;
  if (left < 16) m &= (1u << (int)left) - 1u;
  return m;
}

}  // namespace itsx
