// codec_common.h - the device pieces the image codecs share (png.h, jpeg.h and, through jpeg.h, jpeg_decode.h): a 16-byte
// vector, a bit packer for either bit order, a workgroup scan, the copy of a workspace slot to its place in a file and the
// sum of the items before a workgroup's own.  Helpers only, no kernels.  DESIGN.md section 4.24.
#pragma once
#include <cstdint>

#include "hf_common.h"

namespace {

struct alignas(16) CodecVec16 {
  uint32_t x, y, z, w;
};

// Bits appended at a bit offset of a zeroed word array, LSB first (deflate: stream bit p is bit p % 32 of word p / 32) or
// MSB first (JPEG: bit 31 - p % 32).  Threads write disjoint bit fields of one array: a word shared with a neighbour is
// completed by atomic add, which on zeroed words is an OR.
template <bool MSB_FIRST>
struct CodecBits {
  uint32_t *w;
  uint64_t acc;
  int n, pos;
  __device__ __forceinline__ void init(uint32_t *words, uint32_t bit_offset) {
    w = words;
    pos = (int)(bit_offset >> 5);
    n = (int)(bit_offset & 31u);
    acc = 0;
  }
  __device__ __forceinline__ void put(uint32_t v, int nb) {  // nb <= 32, v < 2^nb; MSB first: 0 < nb
    acc |= (uint64_t)v << (MSB_FIRST ? 64 - n - nb : n);
    n += nb;
    if (n >= 32) {
      atomicAdd(&w[pos++], (uint32_t)(MSB_FIRST ? acc >> 32 : acc));
      acc = MSB_FIRST ? acc << 32 : acc >> 32;
      n -= 32;
    }
  }
  __device__ __forceinline__ void flush() {
    if (n > 0) atomicAdd(&w[pos], (uint32_t)(MSB_FIRST ? acc >> 32 : acc));
    n = 0;
    acc = 0;
  }
};

// ALL threads (contains barriers): inclusive sum of v over the workgroup of THREADS threads in thread order; buf holds
// 2 * THREADS words.  The leading barrier frees the readers of an earlier scan in the same buffer; the barriers behind it
// publish what the caller wrote to LDS before the call.
template <int THREADS>
__device__ __forceinline__ uint32_t codec_scan(uint32_t *buf, int tid, uint32_t v, uint32_t &total) {
  uint32_t *src = buf, *dst = buf + THREADS;
  __syncthreads();
  src[tid] = v;
  __syncthreads();
  for (int d = 1; d < THREADS; d <<= 1) {
    dst[tid] = src[tid] + (tid >= d ? src[tid - d] : 0u);
    __syncthreads();
    uint32_t *t = src;
    src = dst;
    dst = t;
  }
  total = src[THREADS - 1];
  return src[tid];
}

// ALL threads (contains one barrier): sum[0] (LDS) becomes the sum of item(s) over s in [0, mine).  The value is complete
// only behind the CALLER's next barrier: the assemble kernels place one, jpegd_marker_place uses those of the scan it runs.
template <int THREADS, class Item>
__device__ __forceinline__ void codec_sum_before(uint32_t *sum, int mine, int tid, Item &&item) {
  if (tid == 0) sum[0] = 0;
  __syncthreads();
  uint32_t part = 0;
  for (int s = tid; s < mine; s += THREADS) part += item(s);
  if (part) atomicAdd(&sum[0], part);
}

// n bytes of a workspace slot to their place in a file, by the whole workgroup: head bytes up to the destination's dword
// alignment, dword stores built from the shifted pair of source words, tail bytes.  src is dword-aligned and must be
// READABLE UP TO THE WORD BEHIND ITS LAST BYTE (the pair's second word); every slot is sized with at least 16 bytes behind
// its longest content for this.
template <int THREADS>
__device__ __forceinline__ void codec_copy_slot(uint8_t *dst, const uint8_t *src, uint32_t n, int tid) {
  const uint32_t *srcw = reinterpret_cast<const uint32_t *>(src);
  uint32_t head = (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
  if (head > n) head = n;
  const uint32_t nw = (n - head) >> 2;
  if ((uint32_t)tid < head) dst[tid] = src[tid];
  uint32_t *dstw = reinterpret_cast<uint32_t *>(dst + head);
  const uint32_t sh = (head & 3u) * 8u;
  for (uint32_t j = (uint32_t)tid; j < nw; j += THREADS) {
    const uint32_t wi = (head + 4u * j) >> 2;
    const uint32_t w0 = srcw[wi];
    dstw[j] = sh ? (w0 >> sh) | (srcw[wi + 1] << (32u - sh)) : w0;
  }
  const uint32_t done = head + 4u * nw;
  if ((uint32_t)tid < n - done) dst[done + tid] = src[done + tid];
}

}  // namespace
