// inception.h - what stands around the convolutions of the FID Inception-v3 (torch-fidelity's FeatureExtractorInceptionV3,
// the network behind torchmetrics' FrechetInceptionDistance; scripts/fid_metric.py's plain FID column).  Included by
// encoder_ops.hip; the convolutions are csrc/conv_rect.h.
//
//   hf_pool3x3_f32               3x3 max pool or average pool that does not count padding, (stride 1, pad 1) or
//                                (stride 2, pad 0, floor), between channel slices of NCHW tensors
//   hf_resize_bilinear_tf1_f32   TF1-style bilinear resize (align_corners = False, no half-pixel offset) of uint8 or fp32
//                                images to fp32, with an optional affine of the result
//
// Plain vector stores, no atomics; every output element has ONE owner and every sum a fixed order.
// metric_common.h: hf_aligned, hf_lane_blocks (both launchers).
#pragma once
#include <cmath>
#include <cstdint>

#include "metric_common.h"

namespace {

// one lane per output element.  The window's real pixels are visited in row-major order; the average adds them in fp32 in
// that order, starting from the first, and divides by their count (count_include_pad = False); the maximum ignores padding.
__global__ __launch_bounds__(256) void pool3x3(float *__restrict__ out, const float *__restrict__ x, int avg, int c, int h, int w,
                                               int stride, int pad, int oh, int ow, int xc0, int xct, int oc0, int oct,
                                               long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int ox = (int)(e % ow);
  long long r = e / ow;
  const int oy = (int)(r % oh);
  r /= oh;
  const int ch = (int)(r % c);
  const long long n = r / c;
  const float *src = x + (n * xct + xc0 + ch) * (long long)h * w;
  float acc = 0.0f;
  int count = 0;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * stride - pad + ky;
    if (iy < 0 || iy >= h) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * stride - pad + kx;
      if (ix < 0 || ix >= w) continue;
      const float v = src[(long long)iy * w + ix];
      acc = avg ? acc + v : (count == 0 ? v : fmaxf(acc, v));
      ++count;
    }
  }
  out[((n * oct + oc0 + ch) * oh + oy) * (long long)ow + ox] = avg ? acc / (float)count : acc;
}

// one lane per output element, all in fp32 and every operation rounded on its own (no contraction): per axis
// scale = in / out, src = o * scale, i0 = floor(src), i1 = min(i0 + 1, in - 1), t = src - i0; the horizontal lerp
// a + (b - a) * tx of the two rows first, then the vertical one; then, with an affine, v * mul + add.
template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_tf1(float *__restrict__ out, const T *__restrict__ x, int h, int w, int oh,
                                                           int ow, int affine, float mul, float add, long long total) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int ox = (int)(e % ow);
  const long long r = e / ow;
  const int oy = (int)(r % oh);
  const long long plane = r / oh;
  const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;
  const float fy = (float)oy * sy, fx = (float)ox * sx;
  int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
  y0 = y0 > h - 1 ? h - 1 : y0;
  x0 = x0 > w - 1 ? w - 1 : x0;
  const int y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1, x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1;
  const float ty = fy - (float)y0, tx = fx - (float)x0;
  const T *src = x + plane * (long long)h * w;
  const float a = (float)src[(long long)y0 * w + x0], b = (float)src[(long long)y0 * w + x1];
  const float c = (float)src[(long long)y1 * w + x0], d = (float)src[(long long)y1 * w + x1];
  const float top = a + (b - a) * tx;
  const float bot = c + (d - c) * tx;
  float v = top + (bot - top) * ty;
  if (affine) v = v * mul + add;
  out[e] = v;
}

}  // namespace

extern "C" int hf_pool3x3_f32(float *out, const float *x, int mode, int n, int c, int h, int w, int stride, int xc0, int x_ctotal,
                              int oc0, int o_ctotal, void *stream) {
  if (!hf_aligned(out, 4) || !hf_aligned(x, 4) || (mode != 0 && mode != 1) || n <= 0 || c <= 0 || h <= 0 || w <= 0 ||
      (stride != 1 && stride != 2) || (stride == 2 && (h < 3 || w < 3)) || xc0 < 0 || oc0 < 0 || (long long)xc0 + c > x_ctotal ||
      (long long)oc0 + c > o_ctotal || (long long)h * w > 0x7fffffffLL)
    return HF_E_INVALID;
  const int pad = stride == 1 ? 1 : 0;
  const int oh = stride == 1 ? h : (h - 3) / 2 + 1, ow = stride == 1 ? w : (w - 3) / 2 + 1;
  const long long total = (long long)n * c * oh * ow;
  unsigned blocks;
  if (!hf_lane_blocks(total, blocks)) return HF_E_INVALID;
  hipLaunchKernelGGL(pool3x3, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, x, mode, c, h, w, stride, pad, oh, ow,
                     xc0, x_ctotal, oc0, o_ctotal, total);
  return hf_launch_status();
}

extern "C" int hf_resize_bilinear_tf1_f32(float *out, const void *x, int is_u8, int n, int c, int h, int w, int oh, int ow, int affine,
                                          float mul, float add, void *stream) {
  if (!hf_aligned(out, 4) || !hf_aligned(x, is_u8 ? 1 : 4) || n <= 0 || c <= 0 || h <= 0 || w <= 0 || oh <= 0 ||
      ow <= 0 || h > (1 << 23) || w > (1 << 23) || oh > (1 << 23) || ow > (1 << 23) || (long long)h * w > 0x7fffffffLL)
    return HF_E_INVALID;
  const long long total = (long long)n * c * oh * ow;
  unsigned blocks;
  if (!hf_lane_blocks(total, blocks)) return HF_E_INVALID;
  if (is_u8)
    hipLaunchKernelGGL(resize_bilinear_tf1<unsigned char>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out,
                       static_cast<const unsigned char *>(x), h, w, oh, ow, affine ? 1 : 0, mul, add, total);
  else
    hipLaunchKernelGGL(resize_bilinear_tf1<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out,
                       static_cast<const float *>(x), h, w, oh, ow, affine ? 1 : 0, mul, add, total);
  return hf_launch_status();
}
