// paste.h - the inverse of the face alignment: the aligned swap result warped back onto the original photograph and
// composited through a feathered mask (hairfastgan_amd.face_align.paste_back; no counterpart in the reference - the
// contract is a chain of Pillow operations, restated in tests/paste_ref.py).  Included by encoder_ops.hip.
//
//   hf_paste_quad_u8    Image.transform(roi, QUAD, BILINEAR) of the result AND of its mask, then Image.composite onto the
//                       photograph's region of interest: one launch, in place
//   hf_multiply_u8      ImageChops.multiply of two byte planes (the feather with a caller's mask)
//
// Layout: planar uint8, as in align.h.  Arithmetic:
// * the source position of a ROI pixel is align.h's quad_source (double, no contraction), evaluated ONCE per pixel; the
//   mask and the colour planes have the same n x n size, so the one position, its neighbour indices and its two fractions
//   serve all four bilinear_at calls (each: three lerps in double, truncated - Pillow's bilinear_filter8);
// * a position outside the n x n source is mask 0 (Pillow leaves such pixels of the transformed mask 0); mask 0 leaves the
//   photograph's bytes as they are, so neither colour samples nor the blend run there;
// * composite: t = a m + b (255 - m) + 128, byte = ((t >> 8) + t) >> 8 (Pillow's MULDIV255 blend; a = warped result, b = photograph);
// * multiply: byte = a b / 255 rounded down, the rule of the Pillow version DESIGN.md section 4.19 names.
#pragma once
#include <cstdint>

#include "align.h"
#include "hf_common.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ uint8_t paste_blend8(int a, int b, int m) {
  const int t = a * m + b * (255 - m) + 128;
  return (uint8_t)(((t >> 8) + t) >> 8);
}

// photo [planes][H][W] (in place), src [planes][n][n], mask [n][n]; the ROI is rw pixels wide with its corner at (x0, y0);
// q maps ROI pixel centres to source positions.  total = ROI pixels.
__global__ __launch_bounds__(256) void paste_quad(uint8_t *__restrict__ photo, const uint8_t *__restrict__ src,
                                                  const uint8_t *__restrict__ mask, QuadCoef q, int planes, int H, int W, int n,
                                                  int x0, int y0, int rw, long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long hw = (long long)H * W, nn = (long long)n * n;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int y = (int)(i / rw), x = (int)(i - (long long)y * rw);
    double xin, yin;
    if (!quad_source(q, n, n, x, y, xin, yin)) continue;
    const int m = bilinear_at(mask, n, n, xin, yin);
    if (m == 0) continue;
    uint8_t *p = photo + (long long)(y0 + y) * W + (x0 + x);
    for (int c = 0; c < planes; ++c) p[c * hw] = paste_blend8(bilinear_at(src + c * nn, n, n, xin, yin), p[c * hw], m);
  }
}

__global__ __launch_bounds__(256) void multiply_u8(uint8_t *__restrict__ out, const uint8_t *__restrict__ a,
                                                   const uint8_t *__restrict__ b, long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
    out[i] = (uint8_t)((unsigned)a[i] * (unsigned)b[i] / 255u);
}

}  // namespace

extern "C" int hf_paste_quad_u8(unsigned char *photo, const unsigned char *src, const unsigned char *mask, const double *coef8,
                                int planes, int h, int w, int n, int x0, int y0, int x1, int y1, void *stream) {
  if (!photo || !src || !mask || !coef8 || !align_dims_ok(planes, h, w) || !align_dims_ok(planes, n, n)) return HF_E_INVALID;
  if (x0 < 0 || y0 < 0 || x1 > w || y1 > h || x0 >= x1 || y0 >= y1) return HF_E_INVALID;  // the ROI lies inside the photograph
  QuadCoef q;
  for (int k = 0; k < 8; ++k) q.a[k] = coef8[k];
  const long long total = (long long)(x1 - x0) * (y1 - y0);
  hipLaunchKernelGGL(paste_quad, dim3(align_grid(total)), dim3(256), 0, (hipStream_t)stream, photo, src, mask, q, planes, h, w, n,
                     x0, y0, x1 - x0, total);
  return hf_launch_status();
}

extern "C" int hf_multiply_u8(unsigned char *out, const unsigned char *a, const unsigned char *b, long long n, void *stream) {
  if (!out || !a || !b || n <= 0) return HF_E_INVALID;
  hipLaunchKernelGGL(multiply_u8, dim3(align_grid(n)), dim3(256), 0, (hipStream_t)stream, out, a, b, n);
  return hf_launch_status();
}
