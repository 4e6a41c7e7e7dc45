// metric_common.h - what the quality-metric headers share (frechet.h, lpips.h, identity.h, inception.h): the fp64 sum over a
// block's 256 threads, the pointer test of the launchers and the grid of a one-lane-per-element kernel.  Helpers only, no
// kernels.  DESIGN.md section 4.30.
#pragma once
#include <cstdint>

#include "hf_common.h"

namespace {

// Sum of v over the 256 threads of a block through red[256] (LDS): red[t] = v, barrier, then for h = 128, 64, .. 1 thread
// t < h adds red[t + h] to red[t], a barrier after every step.  The tree's shape is fixed, so the total's bits depend on the
// 256 values alone.  Every thread of the block must call it; every thread gets the total (it stands in red[0] after the last
// barrier).  The helper does NOT wait before it writes red: a caller that sums again through the same red puts a
// __syncthreads() between the two calls, or a thread's store could overtake another thread's read of red[0].
__device__ __forceinline__ double hf_block_sum_f64(double v, double *red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  return red[0];
}

// p is not NULL and a multiple of a (a power of two; 1: no requirement, as for uint8 data)
inline bool hf_aligned(const void *p, unsigned a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

// Grid of a kernel with one lane per output element, 256 lanes per block: false when `total` elements need more blocks than
// a grid's x dimension holds.
inline bool hf_lane_blocks(long long total, unsigned &blocks) {
  const long long b = (total + 255) / 256;
  blocks = (unsigned)b;
  return b <= 0x7fffffffLL;
}

}  // namespace
