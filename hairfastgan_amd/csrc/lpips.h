// lpips.h - the reconstruction metrics LPIPS and L2 / PSNR (losses/pp_losses.py:375-529,
// models/encoder4editing/scripts/calc_losses_on_images.py): included by encoder_ops.hip.
//
//   hf_conv2d_direct_f32   first layer of the AlexNet / VGG16 towers: a k x k conv of an input with at most 4 channels, with
//                          the z-score as an input affine, in exact fp32 FMA
//   hf_maxpool2d_f32       MaxPool2d(k, stride) without padding, floor mode
//   hf_lpips_layer_f64     one LPIPS layer: unit-normalise two feature maps along C, weighted squared difference, spatial mean
//   hf_sq_err_sum_f64      per image sum (a - b)^2 of uint8 or fp32 images (L2, PSNR)
//
// Plain vector stores, no floating-point atomics; every output element has ONE owner and every sum a fixed order: results do
// not depend on timing, and a sample's bits depend neither on the batch size nor on its place in the batch (the grid's
// partition of a sample follows from the sample's shape alone).
// metric_common.h: hf_block_sum_f64 (sq_err_partial, metric_finish), hf_aligned.
#pragma once
#include <cmath>
#include <cstdint>

#include "metric_common.h"

namespace {

constexpr int kDcCout = 16;       // direct conv: output channels of a block (one accumulator each per thread)
constexpr int kDcMaxK = 11;       // largest filter
constexpr int kDcMaxCin = 4;
constexpr int kActNone = 0, kActLrelu = 1;  // the `act` codes of hf_conv2d_f32
constexpr int kLpPixels = 64;     // LPIPS layer: pixels of a block (one wave per channel group)
constexpr int kLpGroups = 4;      // channel groups: thread (g, p) owns channels g, g + 4, ...
constexpr int kSqPerThread = 16;  // squared error: elements per thread from which a second block is started
constexpr int kSqMaxBlocks = 1024;

// grid (ceil(oh ow / 256), ceil(cout / 16), n), 256 threads, LDS [K][16] fp32 (K = cin k k): the block's filters, transposed
// so that a thread reads the 16 weights of one (ci, ky, kx) as four 16-byte broadcasts.  A thread owns one output pixel of
// 16 channels; products are added by fmaf in ascending (ci, ky, kx), taps in the padding are skipped (they would add zero).
__global__ __launch_bounds__(256) void conv_direct(float *__restrict__ out, const float *__restrict__ x, const float *__restrict__ wgt,
                                                   const float *__restrict__ in_scale, const float *__restrict__ in_shift,
                                                   const float *__restrict__ bias, int act, float alpha, int cin, int cout, int h,
                                                   int w, int k, int stride, int pad, int oh, int ow) {
  HF_DYN_LDS;
  float *ws = reinterpret_cast<float *>(hf_dyn_lds);
  const int tid = threadIdx.x, kk = cin * k * k;
  const int co0 = blockIdx.y * kDcCout, n = blockIdx.z;
  for (int e = tid; e < kk * kDcCout; e += 256) {
    const int t = e / kDcCout, c = e - t * kDcCout;
    ws[e] = co0 + c < cout ? wgt[(long long)(co0 + c) * kk + t] : 0.0f;
  }
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p >= oh * ow) return;
  const int oy = p / ow, ox = p - oy * ow;
  const int iy0 = oy * stride - pad, ix0 = ox * stride - pad;
  float acc[kDcCout];
#pragma unroll
  for (int c = 0; c < kDcCout; ++c) acc[c] = 0.0f;
  for (int ci = 0; ci < cin; ++ci) {
    const float *plane = x + ((long long)n * cin + ci) * h * w;
    const float sc = in_scale ? in_scale[ci] : 1.0f, sh = in_shift ? in_shift[ci] : 0.0f;
    const bool affine = in_scale || in_shift;
    for (int ky = 0; ky < k; ++ky) {
      const int iy = iy0 + ky;
      if (iy < 0 || iy >= h) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int ix = ix0 + kx;
        if (ix < 0 || ix >= w) continue;
        float v = plane[(long long)iy * w + ix];
        if (affine) v = fmaf(sc, v, sh);
        const float4 *wv = reinterpret_cast<const float4 *>(ws + ((ci * k + ky) * k + kx) * kDcCout);
#pragma unroll
        for (int q = 0; q < kDcCout / 4; ++q) {
          const float4 f = wv[q];
          acc[4 * q + 0] = fmaf(f.x, v, acc[4 * q + 0]);
          acc[4 * q + 1] = fmaf(f.y, v, acc[4 * q + 1]);
          acc[4 * q + 2] = fmaf(f.z, v, acc[4 * q + 2]);
          acc[4 * q + 3] = fmaf(f.w, v, acc[4 * q + 3]);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kDcCout; ++c) {
    if (co0 + c < cout) {
      float v = acc[c];
      if (bias) v += bias[co0 + c];
      if (act == kActLrelu) v = v > 0.0f ? v : v * alpha;
      out[(((long long)n * cout + co0 + c) * oh + oy) * ow + ox] = v;
    }
  }
}

// one thread per output element; the window lies inside the plane (no padding, floor mode).  The first value of the window
// stays unless a later one is greater (or NaN): torch's rule, so that ties between -0 and +0 fall the same way.
__global__ __launch_bounds__(256) void maxpool2d(float *__restrict__ out, const float *__restrict__ x, long long planes, int h, int w,
                                                 int k, int stride, int oh, int ow) {
  const long long total = planes * oh * ow, step = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const int ox = (int)(e % ow);
    const long long r = e / ow;
    const int oy = (int)(r % oh);
    const float *src = x + ((r / oh) * h + (long long)oy * stride) * w + (long long)ox * stride;
    float m = src[0];
    for (int ky = 0; ky < k; ++ky)
      for (int kx = 0; kx < k; ++kx) {
        const float v = src[(long long)ky * w + kx];
        if (v > m || v != v) m = v;
      }
    out[e] = m;
  }
}

// grid (ceil(hw / 64), n), 256 threads = 4 channel groups (one wave each) x 64 pixels, LDS 2 x [4][64] fp32 + [64] fp64.
// Pass 1: thread (g, p) adds fx_c^2 and fy_c^2 over its channels c = g, g + 4, ... in ascending c; the four partial sums of
// a pixel are combined as (s0 + s1) + (s2 + s3).  Pass 2 reads the same values again (from L2: a block's 64 pixels x C x 2
// maps), forms d = fx_c / (|fx| + eps) - fy_c / (|fy| + eps) itself and adds lin_w[c] d^2 the same way.  All of that is fp32;
// the 64 pixel values are then added in fp64 by a tree of fixed shape into part[n][block].
__global__ __launch_bounds__(256) void lpips_layer(double *__restrict__ part, const float *__restrict__ fx, const float *__restrict__ fy,
                                                   const float *__restrict__ lin_w, int c, int hw) {
#pragma clang fp contract(off)
  HF_DYN_LDS;
  float *sa = reinterpret_cast<float *>(hf_dyn_lds);          // [4][64]
  float *sb = sa + kLpGroups * kLpPixels;                     // [4][64]
  double *red = reinterpret_cast<double *>(sb + kLpGroups * kLpPixels);  // [64]
  const int tid = threadIdx.x, g = tid >> 6, lane = tid & 63;
  const int p = blockIdx.x * kLpPixels + lane, n = blockIdx.y;
  const bool live = p < hw;
  const float *px = fx + (long long)n * c * hw + p, *py = fy + (long long)n * c * hw + p;
  float sx = 0.0f, sy = 0.0f;
  if (live)
    for (int ch = g; ch < c; ch += kLpGroups) {
      const float a = px[(long long)ch * hw], b = py[(long long)ch * hw];
      sx = fmaf(a, a, sx);
      sy = fmaf(b, b, sy);
    }
  sa[tid] = sx;
  sb[tid] = sy;
  __syncthreads();
  const float nx = sqrtf((sa[lane] + sa[64 + lane]) + (sa[128 + lane] + sa[192 + lane])) + 1e-10f;
  const float ny = sqrtf((sb[lane] + sb[64 + lane]) + (sb[128 + lane] + sb[192 + lane])) + 1e-10f;
  __syncthreads();
  float acc = 0.0f;
  if (live)
    for (int ch = g; ch < c; ch += kLpGroups) {
      const float d = px[(long long)ch * hw] / nx - py[(long long)ch * hw] / ny;
      acc = fmaf(lin_w[ch], d * d, acc);
    }
  sa[tid] = acc;
  __syncthreads();
  if (tid < kLpPixels) red[tid] = (double)((sa[tid] + sa[64 + tid]) + (sa[128 + tid] + sa[192 + tid]));
  __syncthreads();
  for (int s = kLpPixels / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) part[(long long)n * gridDim.x + blockIdx.x] = red[0];
}

// grid (blocks, n), 256 threads, LDS [256] fp64: thread t of block b adds the elements (b 256 + t) + j (blocks 256),
// j = 0, 1, ... of its image; a tree of fixed shape adds the 256 threads into part[n][b].  The difference of two bytes or of
// two fp32 values is exact in fp64; byte sums are exact integers (below 2^53), so their order does not matter at all.
template <typename T>
__global__ __launch_bounds__(256) void sq_err_partial(double *__restrict__ part, const T *__restrict__ a, const T *__restrict__ b,
                                                      long long per_image) {
#pragma clang fp contract(off)
  HF_DYN_LDS;
  double *red = reinterpret_cast<double *>(hf_dyn_lds);
  const int tid = threadIdx.x, n = blockIdx.y;
  const T *pa = a + (long long)n * per_image, *pb = b + (long long)n * per_image;
  const long long step = (long long)gridDim.x * 256;
  double s = 0.0;
  for (long long e = (long long)blockIdx.x * 256 + tid; e < per_image; e += step) {
    const double d = (double)pa[e] - (double)pb[e];
    s += d * d;
  }
  const double total = hf_block_sum_f64(s, red);
  if (tid == 0) part[(long long)n * gridDim.x + blockIdx.x] = total;
}

// grid (n), 256 threads, LDS [256] fp64: thread t adds part[n][t], part[n][t + 256], ... in that order, a tree of fixed shape
// adds the threads; out[n] = (or +=) total * scale.
__global__ __launch_bounds__(256) void metric_finish(double *__restrict__ out, const double *__restrict__ part, int blocks, double scale,
                                                     int accumulate) {
#pragma clang fp contract(off)
  HF_DYN_LDS;
  double *red = reinterpret_cast<double *>(hf_dyn_lds);
  const int tid = threadIdx.x, n = blockIdx.x;
  double s = 0.0;
  for (int e = tid; e < blocks; e += 256) s += part[(long long)n * blocks + e];
  const double total = hf_block_sum_f64(s, red);
  if (tid == 0) {
    const double v = total * scale;
    out[n] = accumulate ? out[n] + v : v;
  }
}

inline int sq_err_blocks(long long per_image) {
  const long long b = (per_image + 256LL * kSqPerThread - 1) / (256LL * kSqPerThread);
  return (int)(b < 1 ? 1 : (b > kSqMaxBlocks ? kSqMaxBlocks : b));
}

}  // namespace

extern "C" int hf_conv2d_direct_f32(float *out, const float *x, const float *weight, const float *in_scale, const float *in_shift,
                                    const float *bias, int act, float alpha, int n, int cin, int cout, int h, int w, int k, int stride,
                                    int pad, void *stream) {
  if (!hf_aligned(out, 4) || !hf_aligned(x, 4) || !hf_aligned(weight, 4) || n <= 0 || n > 65535 || cin <= 0 ||
      cin > kDcMaxCin || cout <= 0 || cout > 65535 * kDcCout || k <= 0 || k > kDcMaxK || stride < 1 || stride > 4 || pad < 0 ||
      pad >= k || h <= 0 || w <= 0 || h + 2 * pad < k || w + 2 * pad < k || (act != kActNone && act != kActLrelu))
    return HF_E_INVALID;
  const int oh = (h + 2 * pad - k) / stride + 1, ow = (w + 2 * pad - k) / stride + 1;
  if ((long long)oh * ow > 0x7fffffffLL - 256 || (long long)h * w > 0x7fffffffLL) return HF_E_INVALID;
  const dim3 grid(hf_cdiv((long long)oh * ow, 256), hf_cdiv(cout, kDcCout), n);
  hipLaunchKernelGGL(conv_direct, grid, dim3(256), (size_t)cin * k * k * kDcCout * sizeof(float), (hipStream_t)stream, out, x, weight,
                     in_scale, in_shift, bias, act, alpha, cin, cout, h, w, k, stride, pad, oh, ow);
  return hf_launch_status();
}

extern "C" int hf_maxpool2d_f32(float *out, const float *x, long long planes, int h, int w, int k, int stride, void *stream) {
  if (!hf_aligned(out, 4) || !hf_aligned(x, 4) || planes <= 0 || (k != 2 && k != 3) || stride < 1 || stride > k || h < k ||
      w < k)
    return HF_E_INVALID;
  const int oh = (h - k) / stride + 1, ow = (w - k) / stride + 1;
  const long long blocks = (planes * oh * ow + 255) / 256;
  hipLaunchKernelGGL(maxpool2d, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, (hipStream_t)stream, out, x, planes,
                     h, w, k, stride, oh, ow);
  return hf_launch_status();
}

extern "C" long long hf_lpips_layer_work_doubles(int n, int h, int w) {
  return n <= 0 || h <= 0 || w <= 0 ? 0 : (long long)n * hf_cdiv((long long)h * w, kLpPixels);
}

extern "C" int hf_lpips_layer_f64(double *dist, const float *fx, const float *fy, const float *lin_w, double *work, int n, int c,
                                  int h, int w, int accumulate, void *stream) {
  if (!hf_aligned(dist, 8) || !hf_aligned(fx, 4) || !hf_aligned(fy, 4) || !hf_aligned(lin_w, 4) || !hf_aligned(work, 8) ||
      n <= 0 || n > 65535 || c <= 0 || h <= 0 || w <= 0 || (long long)h * w > 0x7fffffffLL - kLpPixels)
    return HF_E_INVALID;
  const int hw = h * w, blocks = hf_cdiv(hw, kLpPixels);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lpips_layer, dim3(blocks, n), dim3(256),
                     (size_t)2 * kLpGroups * kLpPixels * sizeof(float) + kLpPixels * sizeof(double), st, work, fx, fy, lin_w, c, hw);
  hipLaunchKernelGGL(metric_finish, dim3(n), dim3(256), 256 * sizeof(double), st, dist, (const double *)work, blocks, 1.0 / (double)hw,
                     accumulate);
  return hf_launch_status();
}

extern "C" long long hf_sq_err_sum_work_doubles(int n, long long per_image) {
  return n <= 0 || per_image <= 0 ? 0 : (long long)n * sq_err_blocks(per_image);
}

extern "C" int hf_sq_err_sum_f64(double *out, const void *a, const void *b, double *work, int n, long long per_image, int is_u8,
                                 void *stream) {
  const unsigned align = is_u8 ? 1 : 4;
  if (!hf_aligned(out, 8) || !hf_aligned(a, align) || !hf_aligned(b, align) || !hf_aligned(work, 8) || n <= 0 || n > 65535 ||
      per_image <= 0)
    return HF_E_INVALID;
  const int blocks = sq_err_blocks(per_image);
  const hipStream_t st = (hipStream_t)stream;
  if (is_u8)
    hipLaunchKernelGGL(sq_err_partial<unsigned char>, dim3(blocks, n), dim3(256), 256 * sizeof(double), st, work,
                       static_cast<const unsigned char *>(a), static_cast<const unsigned char *>(b), per_image);
  else
    hipLaunchKernelGGL(sq_err_partial<float>, dim3(blocks, n), dim3(256), 256 * sizeof(double), st, work, static_cast<const float *>(a),
                       static_cast<const float *>(b), per_image);
  hipLaunchKernelGGL(metric_finish, dim3(n), dim3(256), 256 * sizeof(double), st, out, (const double *)work, blocks, 1.0, 0);
  return hf_launch_status();
}
