// export.h - the image side of --save_all (utils/save_utils.py:12-30: ToPILImage and mask_to_rgb on the CPU in the
// reference): float images and label maps become the bytes a PNG holds before they leave the device.  Included by
// encoder_ops.hip.
//
//   hf_image_to_bytes_f32     planar fp32 [B,3,H,W] -> uint8 [B,H,W,3] (interleaved) or [B,3,H,W], two rounding rules
//   hf_labels_to_rgb_i64      int64 labels -> uint8 RGB through a palette (models/CtrlHair/util/mask_color_util.py:46-63)
//
// Arithmetic of hf_image_to_bytes_f32 - every step one float32 rounding, in this order, byte-equal to the torch composition:
// * range:  t = (x - lo) / (hi - lo).  (lo, hi) = (-1, 1) is the reference's (x + 1) / 2 (x - (-1) IS x + 1, the division by
//   2 a true division); (0, 1) is t = x: no subtraction and no division are executed.
// * round_half = 0 (save_gen_image: ToPILImage of ((x + 1) / 2).clamp(0, 1)):   byte = trunc(clamp(t, 0, 1) * 255)
// * round_half = 1 (torchvision save_image: mul(255).add_(0.5).clamp_(0, 255)): byte = trunc(clamp(t * 255 + 0.5, 0, 255))
// No contraction: the multiplication by 255 and the addition of 0.5 are two roundings - one fused multiply-add changes which
// byte a value next to k / 255 truncates to (contract(off) below, and the two steps are separate statements).
// NaN gives 0 (fmaxf(NaN, 0) = 0); +-inf clamp like large finite values.
//
// Data movement: one thread converts 4 consecutive pixels of a row - three 16-byte loads (one per plane) and one 12-byte
// store (interleaved) or three 4-byte stores (planar) - in a grid-stride loop over B*H*W/4.  Rows with W % 4 != 0, an input
// base that is not 16-byte aligned or an output base that is not 4-byte aligned take the scalar kernel: one pixel per
// thread, same arithmetic.
#pragma once
#include <cmath>
#include <cstdint>

#include "hf_common.h"

#pragma clang fp contract(off)

namespace {

struct ExportRule {
  float lo, span;  // t = (x - lo) / span
  int unit;        // (lo, hi) = (0, 1): t = x
  int round_half;
};

struct alignas(4) ExportBytes12 {
  uint32_t a, b, c;
};

__device__ __forceinline__ uint32_t export_byte(float x, const ExportRule &r) {
  float t = x;
  if (!r.unit) {
    const float d = x - r.lo;
    t = d / r.span;
  }
  float v;
  if (r.round_half) {
    const float scaled = t * 255.0f;
    const float half = scaled + 0.5f;
    v = fminf(fmaxf(half, 0.0f), 255.0f);
  } else {
    const float c = fminf(fmaxf(t, 0.0f), 1.0f);
    v = c * 255.0f;
  }
  return (uint32_t)(int)v;
}

// groups = B * hw / 4; hw % 4 == 0, in 16-byte aligned, out 4-byte aligned (checked by the launcher)
__global__ __launch_bounds__(256) void image_to_bytes_vec(uint8_t *__restrict__ out, const float *__restrict__ in, long long hw,
                                                          long long groups, ExportRule rule, int interleaved) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long per_image = hw / 4;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    const long long b = g / per_image;
    const long long p = (g - b * per_image) * 4;
    const float *src = in + b * 3 * hw + p;
    const float4 r = *reinterpret_cast<const float4 *>(src);
    const float4 gr = *reinterpret_cast<const float4 *>(src + hw);
    const float4 bl = *reinterpret_cast<const float4 *>(src + 2 * hw);
    const uint32_t r0 = export_byte(r.x, rule), r1 = export_byte(r.y, rule), r2 = export_byte(r.z, rule), r3 = export_byte(r.w, rule);
    const uint32_t g0 = export_byte(gr.x, rule), g1 = export_byte(gr.y, rule), g2 = export_byte(gr.z, rule), g3 = export_byte(gr.w, rule);
    const uint32_t b0 = export_byte(bl.x, rule), b1 = export_byte(bl.y, rule), b2 = export_byte(bl.z, rule), b3 = export_byte(bl.w, rule);
    if (interleaved) {
      ExportBytes12 o;
      o.a = r0 | g0 << 8 | b0 << 16 | r1 << 24;
      o.b = g1 | b1 << 8 | r2 << 16 | g2 << 24;
      o.c = b2 | r3 << 8 | g3 << 16 | b3 << 24;
      *reinterpret_cast<ExportBytes12 *>(out + (b * hw + p) * 3) = o;
    } else {
      uint8_t *dst = out + b * 3 * hw + p;
      *reinterpret_cast<uint32_t *>(dst) = r0 | r1 << 8 | r2 << 16 | r3 << 24;
      *reinterpret_cast<uint32_t *>(dst + hw) = g0 | g1 << 8 | g2 << 16 | g3 << 24;
      *reinterpret_cast<uint32_t *>(dst + 2 * hw) = b0 | b1 << 8 | b2 << 16 | b3 << 24;
    }
  }
}

// one pixel per thread, any width and alignment; pixels = B * hw
__global__ __launch_bounds__(256) void image_to_bytes_scalar(uint8_t *__restrict__ out, const float *__restrict__ in, long long hw,
                                                             long long pixels, ExportRule rule, int interleaved) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
    const long long b = i / hw;
    const long long p = i - b * hw;
    const float *src = in + b * 3 * hw + p;
    for (int c = 0; c < 3; ++c) {
      const uint8_t v = (uint8_t)export_byte(src[c * hw], rule);
      if (interleaved) out[i * 3 + c] = v;
      else out[(b * 3 + c) * hw + p] = v;
    }
  }
}

// mask_to_rgb(pred, 0): palette[label] for 0 <= label < n_colors, then white where label == unknown_label; black otherwise
// (what the reference's zero-initialised array keeps: negative labels, labels past the table, values above 2^31)
__global__ __launch_bounds__(256) void labels_to_rgb(uint8_t *__restrict__ out, const long long *__restrict__ labels,
                                                     long long n, const uint8_t *__restrict__ palette, int n_colors,
                                                     int unknown_label) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const long long l = labels[i];
    uint8_t r = 0, g = 0, b = 0;
    if (l >= 0 && l < (long long)n_colors) {
      const uint8_t *c = palette + 3 * l;
      r = c[0];
      g = c[1];
      b = c[2];
    }
    if (l == (long long)unknown_label) r = g = b = 255;
    uint8_t *o = out + 3 * i;
    o[0] = r;
    o[1] = g;
    o[2] = b;
  }
}

inline int export_grid(long long n) {
  long long g = (n + 255) / 256;
  return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int hf_image_to_bytes_f32(unsigned char *out, const float *in, int batch, int h, int w, float lo, float hi,
                                     int round_half, int interleaved, void *stream) {
  if (!out || !in || batch <= 0 || h <= 0 || w <= 0 || !(hi > lo)) return HF_E_INVALID;
  ExportRule rule;
  rule.lo = lo;
  rule.span = hi - lo;
  rule.unit = (lo == 0.0f && hi == 1.0f) ? 1 : 0;
  rule.round_half = round_half ? 1 : 0;
  const long long hw = (long long)h * w;
  const long long pixels = (long long)batch * hw;
  const bool vec = w % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(image_to_bytes_vec, dim3(export_grid(pixels / 4)), dim3(256), 0, (hipStream_t)stream, out, in, hw, pixels / 4,
                       rule, interleaved ? 1 : 0);
  else
    hipLaunchKernelGGL(image_to_bytes_scalar, dim3(export_grid(pixels)), dim3(256), 0, (hipStream_t)stream, out, in, hw, pixels, rule,
                       interleaved ? 1 : 0);
  return hf_launch_status();
}

extern "C" int hf_labels_to_rgb_i64(unsigned char *out, const long long *labels, long long n_pixels, const unsigned char *palette,
                                    int n_colors, int unknown_label, void *stream) {
  if (!out || !labels || !palette || n_pixels <= 0 || n_colors <= 0) return HF_E_INVALID;
  hipLaunchKernelGGL(labels_to_rgb, dim3(export_grid(n_pixels)), dim3(256), 0, (hipStream_t)stream, out, labels, n_pixels, palette,
                     n_colors, unknown_label);
  return hf_launch_status();
}
