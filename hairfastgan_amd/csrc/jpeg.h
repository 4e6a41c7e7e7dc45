// jpeg.h - a baseline JPEG encoder on the device: uint8 images [B,H,W,C] (C = 1 grey, 3 RGB; what hf_image_to_bytes_f32's
// interleaved layout and hf_paste_quad_u8 produce) become complete JFIF files in caller-allocated slots, byte for byte the
// file libjpeg(-turbo) writes for the same quality and subsampling with one restart interval per MCU row (Pillow:
// Image.save(format="JPEG", quality=, subsampling=, restart_marker_rows=1)).  Included by encoder_ops.hip.  DESIGN.md 4.22.
//
//   hf_jpeg_bound / hf_jpeg_workspace_bytes / hf_jpeg_chunk_mcus   host-only shape arithmetic
//   hf_jpeg_encode_u8                                              three launches, no allocation, no synchronisation
//
// File: SOI, APP0 (JFIF 1.01, unit 0, density 1x1), DQT (one segment per table), SOF0, DHT (DC0, AC0, DC1, AC1: the Annex K
// tables), DRI (the MCUs of one MCU row), SOS, the restart intervals with RSTm (m = interval index mod 8) between them, EOI.
// A restart interval starts on a byte boundary with the DC predictors at zero, so MCU rows are encoded by independent
// workgroups and concatenated byte-wise.
//
// jpeg_blocks (MCU tiles x MCU rows x images, 256 threads): the tile's pixels to LDS as component planes - RGB -> YCbCr in
//   16-bit fixed point, columns clamped to the image (right-edge replication at full resolution), chroma box-downsampled with
//   libjpeg's alternating bias - then the chroma rows below the component's last downsampled row are copies of THAT row (for
//   4:2:0 this is not the same as clamping the full-resolution rows: an even height ends on a row pair); one thread per 8x8
//   block: level shift, jfdctint's two passes in int32 registers, quantisation (|c| + (8q >> 1)) / (8q) with the sign
//   restored, int16 in zig-zag order to the workspace in scan order.  Luma blocks outside the component's own block extent
//   (right and bottom edge of 4:2:2 / 4:2:0) are libjpeg's dummy blocks: AC zero, DC that of the block before them in the MCU.
// jpeg_entropy (MCU rows x images): one restart interval, walked in chunks of hf_jpeg_chunk_mcus MCUs (one block per thread):
//   bit count of each block, a workgroup scan for the bit offsets, the codes written MSB first into zeroed LDS words by
//   atomic add of disjoint fields; the whole bytes of the chunk are byte-stuffed (FF -> FF 00) to the interval's workspace
//   slot at offsets from a second scan over the FF counts; the bits of a last partial byte are carried into the next chunk;
//   the last chunk is padded with 1-bits.  The interval's length goes to a meta word.
// jpeg_assemble (MCU rows x images): exclusive sum of the interval lengths, the bytes to their place in the file (dword
//   stores on the destination's alignment), RSTm or EOI behind them, the header (built on the host, passed by value) by the
//   first workgroup, sizes[b] by the last.
// Every loop is bounded by the shape; the bytes of image b depend on that image, the shape, the quality and the subsampling
// only.
// The 16-byte vector, the bit packer (JpegBits is its MSB-first form), the workgroup scan, the sum of the lengths before an
// interval and the copy of a slot to the file are codec_common.h's, shared with png.h.  What encoder and decoder share is
// stated here and used by jpeg_decode.h: the odd part of the DCT (jpeg_dct_odd), the MCU geometry (jpeg_mcus), the block of
// an MCU -> component and place (jpeg_block_component, jpeg_luma_block_at), a coefficient of a stored block (jpeg_coef).
#pragma once
#include <cstdint>

#include "codec_common.h"
#include "hf_common.h"

namespace {

constexpr int kJpegThreads = 256;
// most bits of one coded block, from the code tables: a DC code of at most 11 bits (the chroma table; luma 9) and 11 value
// bits, 63 AC coefficients of at most 16 code bits and 10 value bits each (a ZRL or EOB symbol stands for coefficients that
// cost nothing themselves, and is no longer than 16 bits)
constexpr int kJpegBlockBits = 11 + 11 + 63 * (16 + 10);
constexpr int kJpegHeaderMax = 640;

struct JpegQuant {
  uint16_t q8[2][64];  // 8 * the quantisation step, zig-zag order: luma, chroma
};
struct JpegCodes {
  uint32_t dc[2][12];   // length << 16 | code of a DC size
  uint32_t ac[2][256];  // the same of run << 4 | size
};
struct JpegHeader {
  uint8_t b[kJpegHeaderMax];
  int n;
};

// ITU-T T.81 Annex K: the quantisation tables in zig-zag order, and the Huffman tables as (codes per length, symbols)
const unsigned char kJpegQuantBase[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18,  17,  16,  19,  24, 40, 26,  24,  22,  22,  24,  49,
     35, 37, 29, 40, 58, 51, 61, 60, 57, 51, 56,  55,  64,  72,  92, 78, 64,  68,  87,  69,  55,  56,
     80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
const unsigned char kJpegDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const unsigned char kJpegAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const unsigned char kJpegAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
     0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
     0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
     0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
     0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
     0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4,
     0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}};

// natural index (8 * row + column) of each zig-zag position (T.81 figure A.6)
static __device__ const unsigned char kJpegNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The odd part that jfdctint.c and jidctint.c share: the rotations of libjpeg's z1..z5 network (CONST_BITS 13) over four
// values, in place.  The forward pass hands in (t4, t5, t6, t7) and gets the unscaled (d7, d5, d3, d1), the inverse pass hands
// in (d7, d5, d3, d1) and gets (t0, t1, t2, t3).
__device__ __forceinline__ void jpeg_dct_odd(int &a, int &b, int &c, int &d) {
  int z1 = a + d, z2 = b + c, z3 = a + c, z4 = b + d;
  const int z5 = (z3 + z4) * 9633;
  a *= 2446;
  b *= 16819;
  c *= 25172;
  d *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a += z1 + z3;
  b += z2 + z4;
  c += z2 + z3;
  d += z1 + z4;
}

// One pass of jfdctint.c over eight values: FIRST is the row pass (results scaled up by 2^PASS1_BITS), the other the column
// pass (that scaling removed again; the output stays scaled by 8).  CONST_BITS 13, PASS1_BITS 2.
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int &d0, int &d1, int &d2, int &d3, int &d4, int &d5, int &d6, int &d7) {
  constexpr int kShift = FIRST ? 13 - 2 : 13 + 2;
  constexpr int kRound = 1 << (kShift - 1);
  int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d0 = (t10 + t11) * 4;
    d4 = (t10 - t11) * 4;
  } else {
    d0 = (t10 + t11 + 2) >> 2;
    d4 = (t10 - t11 + 2) >> 2;
  }
  const int z1 = (t12 + t13) * 4433;
  d2 = (z1 + t13 * 6270 + kRound) >> kShift;
  d6 = (z1 - t12 * 15137 + kRound) >> kShift;
  jpeg_dct_odd(t4, t5, t6, t7);
  d7 = (t4 + kRound) >> kShift;
  d5 = (t5 + kRound) >> kShift;
  d3 = (t6 + kRound) >> kShift;
  d1 = (t7 + kRound) >> kShift;
}

// Block k of an MCU in scan order - nl = hs * vs luma blocks row by row, then Cb, Cr: its component, and for a luma block
// its place (by, bx) among the MCU's luma blocks.
__device__ __forceinline__ int jpeg_block_component(int k, int nl) { return k < nl ? 0 : k - nl + 1; }

__device__ __forceinline__ void jpeg_luma_block_at(int k, int hs, int &by, int &bx) {  // k < nl
  by = k / hs;
  bx = k - by * hs;
}

// coefficient j (0..7) of the eight int16 a 16-byte vector of a block holds
__device__ __forceinline__ int jpeg_coef(const CodecVec16 &q, int j) {
  const uint32_t wv[4] = {q.x, q.y, q.z, q.w};
  return (int)(int16_t)((wv[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
}

// whether block k of an MCU is a dummy block of image h x w
__device__ __forceinline__ bool jpeg_is_dummy(int k, int hs, int vs, int mcu, int row, int h, int w) {
  if (k >= hs * vs) return false;
  int by, bx;
  jpeg_luma_block_at(k, hs, by, bx);
  return (mcu * hs + bx) * 8 >= w || (row * vs + by) * 8 >= h;
}

// ---------------------------------------------------------------------------------------------------------------------
// Quantised coefficients of a tile of MCUs.  Dynamic LDS: Y [8 vs][tile 8 hs] | Cb [8][tile 8] | Cr [8][tile 8] | DCs [256].
__global__ __launch_bounds__(kJpegThreads) void jpeg_blocks(int16_t *__restrict__ coefs, const uint8_t *__restrict__ in, int h, int w,
                                                            int nc, int hs, int vs, int nb, int mcus, int tile, JpegQuant Q) {
  HF_DYN_LDS;
  const int tid = (int)threadIdx.x;
  const int row = (int)blockIdx.y, rows = (int)gridDim.y, img = (int)blockIdx.z;
  const int m0 = (int)blockIdx.x * tile;
  const int nm = (mcus - m0) < tile ? (mcus - m0) : tile;
  const int yw = tile * 8 * hs, cw = tile * 8;
  uint8_t *Y = hf_dyn_lds;
  uint8_t *Cb = Y + 8 * vs * yw;
  uint8_t *Cr = Cb + 8 * cw;
  int *dcs = reinterpret_cast<int *>(nc == 3 ? Cr + 8 * cw : Cb);
  const uint8_t *g = in + (long long)img * h * w * nc;

  // ---- 1. the planes: one item per sample of the coarsest component (hs x vs pixels) ----
  const int ncx = nm * 8;
  for (int it = tid; it < 8 * ncx; it += kJpegThreads) {
    const int cy = it / ncx, cx = it - cy * ncx;
    const int gcx = m0 * 8 + cx;
    int sb = 0, sr = 0;
    for (int j = 0; j < vs; ++j) {
      int y = (row * 8 + cy) * vs + j;
      y = y < h ? y : h - 1;
      for (int i = 0; i < hs; ++i) {
        int x = gcx * hs + i;
        x = x < w ? x : w - 1;
        const uint8_t *p = g + ((long long)y * w + x) * nc;
        uint8_t *yd = Y + (cy * vs + j) * yw + cx * hs + i;
        if (nc == 1) {
          *yd = p[0];
        } else {
          const int r = p[0], gg = p[1], b = p[2];
          *yd = (uint8_t)((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16);
          sb += (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
          sr += (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
        }
      }
    }
    if (nc == 3) {
      if (hs * vs == 4) {  // h2v2: bias 1, 2, 1, 2 along the output row
        sb = (sb + 1 + (gcx & 1)) >> 2;
        sr = (sr + 1 + (gcx & 1)) >> 2;
      } else if (hs == 2) {  // h2v1: bias 0, 1, 0, 1
        sb = (sb + (gcx & 1)) >> 1;
        sr = (sr + (gcx & 1)) >> 1;
      }
      Cb[cy * cw + cx] = (uint8_t)sb;
      Cr[cy * cw + cx] = (uint8_t)sr;
    }
  }
  __syncthreads();
  // ---- 2. chroma rows below the last downsampled row of the image: copies of that row ----
  const int last = (h + vs - 1) / vs - 1 - row * 8;  // the last chroma row of the image inside this MCU row, if < 7
  if (nc == 3 && last < 7) {
    for (int it = tid; it < (7 - last) * ncx; it += kJpegThreads) {
      const int cy = last + 1 + it / ncx, cx = it % ncx;
      Cb[cy * cw + cx] = Cb[last * cw + cx];
      Cr[cy * cw + cx] = Cr[last * cw + cx];
    }
  }
  __syncthreads();

  // ---- 3. one block per thread ----
  const bool active = tid < nm * nb;
  const int mcu = tid / nb, k = tid - mcu * nb;
  const int nl = hs * vs;
  uint32_t pk[32];
  bool dummy = false;
  if (active) {
    const uint8_t *src;
    int pitch;
    if (k < nl) {
      int by, bx;
      jpeg_luma_block_at(k, hs, by, bx);
      src = Y + by * 8 * yw + (mcu * hs + bx) * 8;
      pitch = yw;
    } else {
      src = (k == nl ? Cb : Cr) + mcu * 8;
      pitch = cw;
    }
    const int tq = k < nl ? 0 : 1;
    dummy = jpeg_is_dummy(k, hs, vs, m0 + mcu, row, h, w);
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t lo = *reinterpret_cast<const uint32_t *>(src + r * pitch), hi = *reinterpret_cast<const uint32_t *>(src + r * pitch + 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        d[r * 8 + c] = (int)((lo >> (8 * c)) & 255u) - 128;
        d[r * 8 + 4 + c] = (int)((hi >> (8 * c)) & 255u) - 128;
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
      jpeg_fdct8<true>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
#pragma unroll
    for (int c = 0; c < 8; ++c)
      jpeg_fdct8<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
#pragma unroll
    for (int z = 0; z < 64; ++z) {
      const int c = d[kJpegNatural[z]];
      const uint32_t q8 = Q.q8[tq][z];
      const uint32_t a = (uint32_t)(c < 0 ? -c : c);
      const uint32_t m = (a + (q8 >> 1)) / q8;
      const uint32_t v = (uint32_t)(c < 0 ? -(int)m : (int)m) & 0xFFFFu;
      if (z & 1) pk[z >> 1] |= v << 16;
      else pk[z >> 1] = v;
    }
    dcs[tid] = (int)(int16_t)(pk[0] & 0xFFFFu);
  }
  __syncthreads();
  if (!active) return;
  if (dummy) {  // AC zero, the DC of the block before it in the MCU (block 0 is never a dummy)
    int dc = 0;
    for (int j = k - 1; j >= 0; --j)
      if (!jpeg_is_dummy(j, hs, vs, m0 + mcu, row, h, w)) {
        dc = dcs[tid - k + j];
        break;
      }
#pragma unroll
    for (int i = 0; i < 32; ++i) pk[i] = 0;
    pk[0] = (uint32_t)dc & 0xFFFFu;
  }
  const long long blk = ((long long)img * rows + row) * ((long long)mcus * nb) + (long long)(m0 + mcu) * nb + k;
  CodecVec16 *dst = reinterpret_cast<CodecVec16 *>(coefs + blk * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) dst[i] = CodecVec16{pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]};
}

using JpegBits = CodecBits<true>;  // the entropy-coded segment packs bits MSB first

// The code of one block (64 int16 in zig-zag order, 16-byte aligned) with DC predictor `pred`: put(bits, count) for the DC
// symbol, every AC (run, size) symbol with its value bits, ZRL for runs above 15, EOB unless coefficient 63 is non-zero.
template <class Put>
__device__ __forceinline__ void jpeg_block_code(const int16_t *blk, int pred, const uint32_t *dct, const uint32_t *act, Put &&put) {
  const CodecVec16 *v = reinterpret_cast<const CodecVec16 *>(blk);
  int run = 0;
  for (int gI = 0; gI < 8; ++gI) {
    const CodecVec16 q = v[gI];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = jpeg_coef(q, j);
      if (gI == 0 && j == 0) {
        const int diff = c - pred;
        const uint32_t a = (uint32_t)(diff < 0 ? -diff : diff);
        int s = a ? 32 - __builtin_clz(a) : 0;
        s = s > 11 ? 11 : s;
        const uint32_t e = dct[s];
        const uint32_t vb = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u);
        put((e & 0xFFFFu) << s | vb, (int)(e >> 16) + s);
        continue;
      }
      if (c == 0) {
        ++run;
        continue;
      }
      for (int r = 0; r < 3 && run > 15; ++r) {  // at most 62 zeros precede a coefficient
        put(act[0xF0] & 0xFFFFu, (int)(act[0xF0] >> 16));
        run -= 16;
      }
      const uint32_t a = (uint32_t)(c < 0 ? -c : c);
      const int s = 32 - __builtin_clz(a);
      const uint32_t e = act[(run << 4 | s) & 255];
      const uint32_t vb = (uint32_t)(c < 0 ? c - 1 : c) & ((1u << s) - 1u);
      put((e & 0xFFFFu) << s | vb, (int)(e >> 16) + s);
      run = 0;
    }
  }
  if (run) put(act[0] & 0xFFFFu, (int)(act[0] >> 16));
}

__device__ __forceinline__ uint32_t jpeg_stream_byte(const uint32_t *words, uint32_t p) { return (words[p >> 2] >> (24u - 8u * (p & 3u))) & 255u; }

// jpeg_entropy's dynamic LDS in words: bit buffer [nwords] | code tables | scan | carry.  The bit buffer takes the bits of a
// chunk of `blocks` blocks, a carried byte, the padding, and is rounded to whole 16 bytes.
constexpr int kJpegTabWords = 32 + 2 * 256;  // DC codes [2][12] padded to 32, AC codes [2][256]
constexpr int jpeg_entropy_words(int blocks) { return ((blocks * kJpegBlockBits + 8 + 31) / 32 + 1 + 3) / 4 * 4; }
constexpr int jpeg_entropy_lds_words(int nwords) { return nwords + kJpegTabWords + 2 * kJpegThreads + 4; }

// One restart interval (MCU row) -> its byte-stuffed entropy-coded bytes in its workspace slot, the length in meta.
__global__ __launch_bounds__(kJpegThreads) void jpeg_entropy(uint8_t *__restrict__ slots, uint32_t *__restrict__ meta,
                                                             const int16_t *__restrict__ coefs, int hs, int vs, int nb, int mcus,
                                                             int tile, long long slot_bytes, int nwords, JpegCodes C) {
  HF_DYN_LDS;
  uint32_t *words = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  uint32_t *tab = words + nwords;
  uint32_t *scan = tab + kJpegTabWords;
  uint32_t *carry = scan + 2 * kJpegThreads;  // partial byte, its bit count, bytes written so far
  const int tid = (int)threadIdx.x;
  const int row = (int)blockIdx.x, rows = (int)gridDim.x, img = (int)blockIdx.y;
  const long long row_blocks = (long long)mcus * nb;
  const int16_t *rc = coefs + ((long long)img * rows + row) * row_blocks * 64;
  uint8_t *slot = slots + ((long long)img * rows + row) * slot_bytes;
  for (int i = tid; i < 24; i += kJpegThreads) tab[i] = C.dc[i / 12][i % 12];
  for (int i = tid; i < 512; i += kJpegThreads) tab[32 + i] = C.ac[i >> 8][i & 255];
  if (tid < 4) carry[tid] = 0;
  const int nl = hs * vs;
  const int chunk = tile * nb;  // blocks per chunk, at most kJpegThreads
  const int nchunks = (mcus + tile - 1) / tile;
  const int k = tid % nb;
  const uint32_t *dct = tab + (k < nl ? 0 : 12), *act = tab + 32 + (k < nl ? 0 : 256);

  for (int ch = 0; ch < nchunks; ++ch) {
    __syncthreads();  // the tables and the carry of the chunk before are written, its bytes are read
    const uint32_t cbyte = carry[0], cbits = carry[1], out_off = carry[2];
    const long long blk = (long long)ch * chunk + tid;
    const bool active = tid < chunk && blk < row_blocks;
    int pred = 0;
    if (active && blk >= nb) {  // not the first MCU of the interval: the DC of the component's block before this one
      const long long pb = k == 0 ? blk - nb + nl - 1 : (k < nl ? blk - 1 : blk - nb);
      pred = rc[pb * 64];
    } else if (active && k > 0 && k < nl) {
      pred = rc[(blk - 1) * 64];
    }
    uint32_t bits = 0;
    if (active) jpeg_block_code(rc + blk * 64, pred, dct, act, [&](uint32_t, int n) { bits += (uint32_t)n; });
    uint32_t total;
    const uint32_t incl = codec_scan<kJpegThreads>(scan, tid, bits, total);
    const int nzero = (int)((cbits + total + 8u) >> 5) + 1;  // the words this chunk's bits and padding reach, at most nwords
    for (int i = tid; i < nzero && i < nwords; i += kJpegThreads) words[i] = 0;
    __syncthreads();
    if (tid == 0) atomicAdd(&words[0], cbyte << 24);
    if (active) {
      JpegBits bw;
      bw.init(words, cbits + incl - bits);
      jpeg_block_code(rc + blk * 64, pred, dct, act, [&](uint32_t v, int n) { bw.put(v, n); });
      bw.flush();
    }
    const uint32_t T = cbits + total;
    const bool lastc = ch == nchunks - 1;
    uint32_t nbytes = T >> 3;
    const uint32_t rem = T & 7u;
    if (lastc && rem) {  // padding with 1-bits to a byte boundary
      if (tid == 0) atomicAdd(&words[T >> 5], ((1u << (8u - rem)) - 1u) << (32u - (T & 31u) - (8u - rem)));
      nbytes += 1;
    }
    __syncthreads();
    const uint32_t q = (nbytes + kJpegThreads - 1) / kJpegThreads;
    const uint32_t a = (uint32_t)tid * q < nbytes ? (uint32_t)tid * q : nbytes;
    const uint32_t b = a + q < nbytes ? a + q : nbytes;
    uint32_t ff = 0;
    for (uint32_t p = a; p < b; ++p) ff += jpeg_stream_byte(words, p) == 255u ? 1u : 0u;
    uint32_t nff;
    const uint32_t ffi = codec_scan<kJpegThreads>(scan, tid, ff, nff);
    uint8_t *dst = slot + out_off + a + (ffi - ff);
    for (uint32_t p = a; p < b; ++p) {
      const uint32_t v = jpeg_stream_byte(words, p);
      *dst++ = (uint8_t)v;
      if (v == 255u) *dst++ = 0;
    }
    if (tid == 0) {
      carry[0] = (lastc || !rem) ? 0u : jpeg_stream_byte(words, nbytes);
      carry[1] = lastc ? 0u : rem;
      carry[2] = out_off + nbytes + nff;
    }
  }
  __syncthreads();
  if (tid == 0) meta[(long long)img * rows + row] = carry[2];
}

// The interval's bytes to their place in the file, the marker behind them; the header; sizes.  Dynamic LDS: sum [4].
__global__ __launch_bounds__(kJpegThreads) void jpeg_assemble(uint8_t *__restrict__ out, long long out_stride, long long *__restrict__ sizes,
                                                              const uint8_t *__restrict__ slots, const uint32_t *__restrict__ meta,
                                                              long long slot_bytes, JpegHeader H) {
  HF_DYN_LDS;
  uint32_t *sum = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  const int tid = (int)threadIdx.x;
  const int row = (int)blockIdx.x, rows = (int)gridDim.x, img = (int)blockIdx.y;
  const uint32_t *mimg = meta + (long long)img * rows;
  codec_sum_before<kJpegThreads>(sum, row, tid, [&](int s) { return mimg[s] + 2u; });  // an interval and the marker behind it
  __syncthreads();
  const uint32_t off = (uint32_t)H.n + sum[0];
  const uint32_t n = mimg[row];
  const uint8_t *src = slots + ((long long)img * rows + row) * slot_bytes;
  uint8_t *o = out + (long long)img * out_stride;
  uint8_t *dst = o + off;
  codec_copy_slot<kJpegThreads>(dst, src, n, tid);
  if (tid == 0) {
    dst[n] = 0xFF;
    if (row + 1 < rows) {
      dst[n + 1] = (uint8_t)(0xD0 + (row & 7));  // RSTm
    } else {
      dst[n + 1] = 0xD9;  // EOI
      sizes[img] = (long long)off + n + 2;
    }
  }
  if (row == 0)
    for (int i = tid; i < H.n; i += kJpegThreads) o[i] = H.b[i];
}

// The MCU geometry that encoder and decoder derive from a frame: nl luma blocks and nb blocks per MCU, MCUs per MCU row, MCU rows
struct JpegMcus {
  int nc, hs, vs, nl, nb, mcus, rows;
};

// false: a dimension outside 1..65535, components other than 1 / 3, luma sampling other than 1x1 or, with three components,
// 2x1 and 2x2 (the chroma components are 1x1)
inline bool jpeg_mcus(int h, int w, int components, int hs, int vs, JpegMcus &m) {
  if (h <= 0 || w <= 0 || h > 65535 || w > 65535 || (components != 1 && components != 3)) return false;
  if (!((hs == 1 && vs == 1) || (components == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
  m.nc = components, m.hs = hs, m.vs = vs;
  m.nl = hs * vs;
  m.nb = m.nl + (components == 3 ? 2 : 0);
  m.mcus = (w + 8 * hs - 1) / (8 * hs);
  m.rows = (h + 8 * vs - 1) / (8 * vs);
  return true;
}

struct JpegShape : JpegMcus {
  int tile, header;
  long long row_blocks, slot, bound;
};

// false: a shape the encoder does not take (what jpeg_mcus refuses, subsampling outside 0..2, a file of 2 GiB or more)
inline bool jpeg_shape(int h, int w, int channels, int subsampling, JpegShape &s) {
  if (subsampling < 0 || subsampling > 2) return false;
  const int hs = (channels == 3 && subsampling > 0) ? 2 : 1, vs = (channels == 3 && subsampling == 2) ? 2 : 1;
  if (!jpeg_mcus(h, w, channels, hs, vs, s)) return false;
  s.tile = kJpegThreads / s.nb;
  s.row_blocks = (long long)s.mcus * s.nb;
  // SOI 2, APP0 18, DQT 69 each, SOF0 10 + 3 nc, DHT 33 + 183 per table pair, DRI 6, SOS 8 + 2 nc
  s.header = 2 + 18 + 69 * (channels == 3 ? 2 : 1) + 10 + 3 * channels + 216 * (channels == 3 ? 2 : 1) + 6 + 8 + 2 * channels;
  const long long interval = 2 * ((s.row_blocks * kJpegBlockBits + 7) / 8);  // padded to a byte; stuffing at most doubles
  s.slot = (interval + 15) / 16 * 16 + 16;
  s.bound = s.header + (long long)s.rows * interval + 2ll * (s.rows - 1) + 2;  // RSTm between the intervals, EOI
  return s.bound < (1ll << 31);
}

inline long long jpeg_meta_bytes(int batch, const JpegShape &s) { return ((long long)batch * s.rows * 4 + 15) / 16 * 16; }

inline void jpeg_put_segment(JpegHeader &H, int marker, int body) {
  H.b[H.n++] = 0xFF;
  H.b[H.n++] = (uint8_t)marker;
  H.b[H.n++] = (uint8_t)((body + 2) >> 8);
  H.b[H.n++] = (uint8_t)(body + 2);
}

// libjpeg's jpeg_set_quality(quality, force_baseline): the tables, the Huffman codes and the header of the file
inline void jpeg_tables(int h, int w, int quality, const JpegShape &s, JpegQuant &Q, JpegCodes &C, JpegHeader &H) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  uint8_t qt[2][64];
  for (int t = 0; t < 2; ++t)
    for (int z = 0; z < 64; ++z) {
      int v = (kJpegQuantBase[t][z] * scale + 50) / 100;
      v = v < 1 ? 1 : (v > 255 ? 255 : v);
      qt[t][z] = (uint8_t)v;
      Q.q8[t][z] = (uint16_t)(8 * v);
    }
  for (int t = 0; t < 2; ++t) {  // T.81 annex C: codes of one length count up, a longer length appends a zero
    for (int i = 0; i < 256; ++i) C.ac[t][i] = 0;
    uint32_t code = 0;
    int idx = 0;
    for (int len = 1; len <= 16; ++len, code <<= 1)
      for (int i = 0; i < kJpegDcBits[t][len - 1]; ++i) C.dc[t][idx++] = (uint32_t)len << 16 | code++;  // the DC symbols are 0..11 in order
    code = 0;
    idx = 0;
    for (int len = 1; len <= 16; ++len, code <<= 1)
      for (int i = 0; i < kJpegAcBits[t][len - 1]; ++i) C.ac[t][kJpegAcVals[t][idx++]] = (uint32_t)len << 16 | code++;
  }
  const int ntab = s.nc == 3 ? 2 : 1;
  H.n = 0;
  H.b[H.n++] = 0xFF;
  H.b[H.n++] = 0xD8;
  jpeg_put_segment(H, 0xE0, 14);
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (int i = 0; i < 14; ++i) H.b[H.n++] = jfif[i];
  for (int t = 0; t < ntab; ++t) {
    jpeg_put_segment(H, 0xDB, 65);
    H.b[H.n++] = (uint8_t)t;
    for (int z = 0; z < 64; ++z) H.b[H.n++] = qt[t][z];
  }
  jpeg_put_segment(H, 0xC0, 6 + 3 * s.nc);
  H.b[H.n++] = 8;
  H.b[H.n++] = (uint8_t)(h >> 8);
  H.b[H.n++] = (uint8_t)h;
  H.b[H.n++] = (uint8_t)(w >> 8);
  H.b[H.n++] = (uint8_t)w;
  H.b[H.n++] = (uint8_t)s.nc;
  for (int c = 0; c < s.nc; ++c) {
    H.b[H.n++] = (uint8_t)(c + 1);
    H.b[H.n++] = c == 0 ? (uint8_t)(s.hs << 4 | s.vs) : 0x11;
    H.b[H.n++] = c == 0 ? 0 : 1;
  }
  for (int t = 0; t < ntab; ++t) {
    jpeg_put_segment(H, 0xC4, 1 + 16 + 12);
    H.b[H.n++] = (uint8_t)t;
    for (int i = 0; i < 16; ++i) H.b[H.n++] = kJpegDcBits[t][i];
    for (int i = 0; i < 12; ++i) H.b[H.n++] = (uint8_t)i;
    jpeg_put_segment(H, 0xC4, 1 + 16 + 162);
    H.b[H.n++] = (uint8_t)(0x10 | t);
    for (int i = 0; i < 16; ++i) H.b[H.n++] = kJpegAcBits[t][i];
    for (int i = 0; i < 162; ++i) H.b[H.n++] = kJpegAcVals[t][i];
  }
  jpeg_put_segment(H, 0xDD, 2);
  H.b[H.n++] = (uint8_t)(s.mcus >> 8);
  H.b[H.n++] = (uint8_t)s.mcus;
  jpeg_put_segment(H, 0xDA, 4 + 2 * s.nc);
  H.b[H.n++] = (uint8_t)s.nc;
  for (int c = 0; c < s.nc; ++c) {
    H.b[H.n++] = (uint8_t)(c + 1);
    H.b[H.n++] = c == 0 ? 0x00 : 0x11;
  }
  H.b[H.n++] = 0;
  H.b[H.n++] = 63;
  H.b[H.n++] = 0;
}

}  // namespace

extern "C" long long hf_jpeg_bound(int h, int w, int channels, int subsampling) {
  JpegShape s;
  return jpeg_shape(h, w, channels, subsampling, s) ? s.bound : 0;
}

extern "C" int hf_jpeg_chunk_mcus(int channels, int subsampling) {
  JpegShape s;
  return jpeg_shape(8, 8, channels, subsampling, s) ? s.tile : 0;
}

extern "C" long long hf_jpeg_workspace_bytes(int batch, int h, int w, int channels, int subsampling) {
  JpegShape s;
  if (batch <= 0 || !jpeg_shape(h, w, channels, subsampling, s)) return 0;
  return jpeg_meta_bytes(batch, s) + (long long)batch * s.rows * (s.row_blocks * 128 + s.slot);
}

extern "C" int hf_jpeg_encode_u8(unsigned char *out, long long out_stride, long long *sizes, const unsigned char *in, int batch,
                                 int h, int w, int channels, int quality, int subsampling, void *workspace,
                                 long long workspace_bytes, void *stream) {
  JpegShape s;
  if (!out || !sizes || !in || !workspace || batch <= 0 || batch > 65535 || quality < 1 || quality > 100) return HF_E_INVALID;
  if (!jpeg_shape(h, w, channels, subsampling, s) || out_stride < s.bound) return HF_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || (reinterpret_cast<uintptr_t>(sizes) & 7u) != 0) return HF_E_INVALID;
  if (workspace_bytes < hf_jpeg_workspace_bytes(batch, h, w, channels, subsampling)) return HF_E_WORKSPACE;
  JpegQuant Q;
  JpegCodes C;
  JpegHeader H;
  jpeg_tables(h, w, quality, s, Q, C, H);
  if (H.n != s.header) return HF_E_INVALID;  // the bound counts the header bytes: both statements must agree
  uint32_t *meta = static_cast<uint32_t *>(workspace);
  int16_t *coefs = reinterpret_cast<int16_t *>(static_cast<uint8_t *>(workspace) + jpeg_meta_bytes(batch, s));
  uint8_t *slots = reinterpret_cast<uint8_t *>(coefs) + (long long)batch * s.rows * s.row_blocks * 128;
  const int tiles = (s.mcus + s.tile - 1) / s.tile;
  const size_t lds_blocks = (size_t)s.tile * 64 * s.nb + kJpegThreads * 4;
  const int nwords = jpeg_entropy_words(s.tile * s.nb);
  const size_t lds_entropy = (size_t)jpeg_entropy_lds_words(nwords) * 4;
  static_assert(jpeg_entropy_lds_words(jpeg_entropy_words(kJpegThreads)) * 4 <= 65536,
                "a chunk's LDS stays inside the 64 KiB a kernel gets without opting in");
  static_assert(sizeof(JpegCodes) + sizeof(JpegHeader) + sizeof(JpegQuant) < 4096, "tables passed by value: the kernel argument limit");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_blocks, dim3(tiles, s.rows, batch), dim3(kJpegThreads), lds_blocks, st, coefs, in, h, w, s.nc, s.hs, s.vs, s.nb,
                     s.mcus, s.tile, Q);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  hipLaunchKernelGGL(jpeg_entropy, dim3(s.rows, batch), dim3(kJpegThreads), lds_entropy, st, slots, meta, coefs, s.hs, s.vs, s.nb, s.mcus,
                     s.tile, s.slot, nwords, C);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  hipLaunchKernelGGL(jpeg_assemble, dim3(s.rows, batch), dim3(kJpegThreads), 16, st, out, out_stride, sizes, slots, meta, s.slot, H);
  return hf_launch_status();
}
