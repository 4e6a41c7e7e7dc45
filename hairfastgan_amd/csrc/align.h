// align.h - FFHQ face alignment from 68 landmarks, the image work of utils/shape_predictor.py:145-185 (PIL and scipy on
// the CPU in the reference): included by encoder_ops.hip.
//
//   hf_resize_lanczos_u8      PIL Image.resize(size, LANCZOS) on 8-bit planes: two separable integer passes
//   hf_quad_bilinear_u8       PIL Image.transform(size, QUAD, quad, BILINEAR)
//   hf_quad_lanczos4_u8       the two above fused for transform_size = 4 * output_size (the real path, 4096^2 -> 1024^2)
//   hf_align_pad_blur_f32     np.pad(reflect) + scipy.ndimage.gaussian_filter + the blur fade   (:170-176)
//   hf_align_pad_finish_u8    the median fade, rint, clip, byte                                   (:177-178)
//   hf_u8_to_unit_f32         ToTensor: float(byte) / 255 (a true division)
//
// Layout: every image is PLANAR uint8 [channels][h][w] - the [3,H,W] tensors `swap` takes and returns, so nothing is
// transposed on the way in or out; a plane is an independent single-band image for every step here.
//
// Arithmetic (restated from Pillow's Resample.c / Geometry.c and scipy's ni_filters.c; pinned by tests/align_ref.py):
// * resize: the coefficient tables come from the host (double -> 22-bit fixed point, face_align.lanczos_coeffs); the
//   device computes acc = 2^21 + sum pixel * k in int32 and stores clamp(acc >> 22, 0, 255); the horizontal pass is rounded
//   to bytes before the vertical pass reads it.  A pass whose size does not change is skipped, as in Pillow.
// * transform: per output pixel (x + 0.5, y + 0.5): xin = a0 + a1 x + a2 y + a3 x y (a0..a7 from the host, as Pillow's
//   Image.__transformer derives them), 0 if (xin, yin) is outside [0, w) x [0, h); else subtract 0.5, floor, neighbour
//   indices clamped to the edge, three lerps v1 + (v2 - v1) d in DOUBLE, truncated to the byte.  No contraction: an fma
//   in the coordinate polynomial or a lerp changes which byte a near-integer value truncates to.
// * fused: a workgroup owns a 32 x 32 output tile of one plane.  It evaluates the (4*32 + 24)^2 window of the transform
//   grid as truncated bytes into LDS (Pillow's rounding point: the 4096^2 image is 8-bit), runs the horizontal integer
//   pass into LDS and the vertical pass from there.  LDS: 152^2 + 152*32 = 27968 bytes - five workgroups per CU of the
//   160 KiB; a 64 x 64 tile (96 KiB) would leave one.  Same bytes as the two kernels chained.
// * pad: the Gaussian is separable, axis 0 (rows) first; weights in double from the host, the line extended by scipy's
//   'reflect' (edge sample repeated) over the np.pad 'reflect' extension (edge not repeated) of the source bytes; the sum
//   runs in double in ni_filters.c's symmetric order - centre, then the pairs (in[l-j] + in[l+j]) * w[j] from the outermost
//   inwards - and the result of EACH axis is rounded to float32.  The fades are float32, one rounding per operation.
#pragma once
#include <cmath>
#include <cstdint>

#include "hf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kAlignPrecisionBits = 32 - 8 - 2;  // Pillow's PRECISION_BITS
constexpr int kFusedTile = 32;                   // output tile of the fused kernel
constexpr int kFusedRatio = 4;                   // transform_size / output_size it is instantiated for
constexpr int kFusedHalo = 12;                   // Lanczos support (3) * ratio
constexpr int kFusedWin = kFusedRatio * kFusedTile + 2 * kFusedHalo;
constexpr int kPadTile = 64;                     // pixels along the filtered axis per workgroup
constexpr int kPadLanesV = 64, kPadLanesH = 16;  // columns (vertical pass) / rows (horizontal pass) per workgroup
constexpr int kPadMaxRadius = 448;               // LDS: (64 + 2*448) * 64 bytes = 60 KiB, 16 * (64 + 896) floats the same; sigma <= 112
                                                 // (the reference's sigma is 0.02 * qsize with qsize < 4 * output_size after the shrink: 82)

struct QuadCoef {
  double a[8];
};

__device__ __forceinline__ uint8_t align_clip8(int acc) {
  const int v = acc >> kAlignPrecisionBits;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// taps of output `o`: [first, first + n) of an axis of `in_size` samples, n <= ksize (a wrong table cannot index outside)
__device__ __forceinline__ void align_taps(const int *__restrict__ bounds, int o, int in_size, int ksize, int &first, int &n) {
  first = bounds[2 * o];
  n = bounds[2 * o + 1];
  first = first < 0 ? 0 : (first > in_size ? in_size : first);
  n = n < 0 ? 0 : n;
  n = n > ksize ? ksize : n;
  n = n > in_size - first ? in_size - first : n;
}

// in [planes][h][w_in] -> out [planes][h][w_out]
__global__ __launch_bounds__(256) void resize_lanczos_h(uint8_t *__restrict__ out, const uint8_t *__restrict__ in,
                                                        const int *__restrict__ bounds, const int *__restrict__ kk, int ksize,
                                                        int h, int w_in, int w_out, long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int xo = (int)(i % w_out);
    const long long row = i / w_out;
    int first, n;
    align_taps(bounds, xo, w_in, ksize, first, n);
    const uint8_t *p = in + row * w_in + first;
    const int *k = kk + (long long)xo * ksize;
    int acc = 1 << (kAlignPrecisionBits - 1);
    for (int j = 0; j < n; ++j) acc += (int)p[j] * k[j];
    out[i] = align_clip8(acc);
  }
}

// in [planes][h_in][w] -> out [planes][h_out][w]
__global__ __launch_bounds__(256) void resize_lanczos_v(uint8_t *__restrict__ out, const uint8_t *__restrict__ in,
                                                        const int *__restrict__ bounds, const int *__restrict__ kk, int ksize,
                                                        int h_in, int h_out, int w, long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int x = (int)(i % w);
    const long long r = i / w;
    const int yo = (int)(r % h_out);
    const long long plane = r / h_out;
    int first, n;
    align_taps(bounds, yo, h_in, ksize, first, n);
    const uint8_t *p = in + (plane * h_in + first) * w + x;
    const int *k = kk + (long long)yo * ksize;
    int acc = 1 << (kAlignPrecisionBits - 1);
    for (int j = 0; j < n; ++j) acc += (int)p[(long long)j * w] * k[j];
    out[i] = align_clip8(acc);
  }
}

// Pillow's quad_transform at output pixel (x, y): the source position in an h x w image; false outside it
__device__ __forceinline__ bool quad_source(const QuadCoef &q, int h, int w, int x, int y, double &xin, double &yin) {
  const double xs = x + 0.5, ys = y + 0.5;
  xin = q.a[0] + q.a[1] * xs + q.a[2] * ys + q.a[3] * xs * ys;
  yin = q.a[4] + q.a[5] * xs + q.a[6] * ys + q.a[7] * xs * ys;
  return !(!(xin >= 0.0) || xin >= (double)w || !(yin >= 0.0) || yin >= (double)h);  // (NaN: outside)
}

// Pillow's bilinear_filter8 of one h x w plane at a position quad_source accepted
__device__ __forceinline__ uint8_t bilinear_at(const uint8_t *__restrict__ plane, int h, int w, double xin, double yin) {
  xin -= 0.5;
  yin -= 0.5;
  const int xi = xin >= 0.0 ? (int)xin : (int)floor(xin);
  const int yi = yin >= 0.0 ? (int)yin : (int)floor(yin);
  const double dx = xin - xi, dy = yin - yi;
  const int x0 = xi < 0 ? 0 : (xi >= w ? w - 1 : xi);
  const int x1 = xi + 1 < 0 ? 0 : (xi + 1 >= w ? w - 1 : xi + 1);
  const int y0 = yi < 0 ? 0 : (yi >= h ? h - 1 : yi);
  const int y1 = yi + 1 < 0 ? 0 : (yi + 1 >= h ? h - 1 : yi + 1);
  const uint8_t *r0 = plane + (long long)y0 * w, *r1 = plane + (long long)y1 * w;
  const double p00 = r0[x0], p01 = r0[x1], p10 = r1[x0], p11 = r1[x1];
  const double v1 = p00 + (p01 - p00) * dx;
  const double v2 = p10 + (p11 - p10) * dx;
  const double v = v1 + (v2 - v1) * dy;
  return (uint8_t)(int)v;
}

// the two above: Pillow's transform(QUAD, BILINEAR) at output pixel (x, y) of one h x w plane, 0 outside it
__device__ __forceinline__ uint8_t quad_bilinear_sample(const uint8_t *__restrict__ plane, int h, int w, const QuadCoef &q, int x,
                                                        int y) {
  double xin, yin;
  return quad_source(q, h, w, x, y, xin, yin) ? bilinear_at(plane, h, w, xin, yin) : 0;
}

// src [planes][h][w] -> out [planes][oh][ow]
__global__ __launch_bounds__(256) void quad_bilinear(uint8_t *__restrict__ out, const uint8_t *__restrict__ src, QuadCoef q, int h,
                                                     int w, int oh, int ow, long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long ohw = (long long)oh * ow;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long plane = i / ohw;
    const int p = (int)(i - plane * ohw);
    const int y = p / ow;
    out[i] = quad_bilinear_sample(src + plane * h * w, h, w, q, p - y * ow, y);
  }
}

// grid (out/32, out/32 rounded up, planes), 256 threads; the transform grid is (4*osize)^2, bounds / kk are the tables of the
// 4*osize -> osize Lanczos pass (both axes: the image is square)
__global__ __launch_bounds__(256) void quad_lanczos4(uint8_t *__restrict__ out, const uint8_t *__restrict__ src, QuadCoef q, int h,
                                                     int w, int osize, const int *__restrict__ bounds,
                                                     const int *__restrict__ kk, int ksize) {
  HF_DYN_LDS;
  uint8_t *win = hf_dyn_lds;                        // [kFusedWin][kFusedWin] transform-grid bytes
  uint8_t *mid = hf_dyn_lds + kFusedWin * kFusedWin;  // [kFusedWin][kFusedTile] after the horizontal pass
  const int tsize = kFusedRatio * osize;
  const int ox0 = blockIdx.x * kFusedTile, oy0 = blockIdx.y * kFusedTile;
  const int gx0 = kFusedRatio * ox0 - kFusedHalo, gy0 = kFusedRatio * oy0 - kFusedHalo;
  const uint8_t *plane = src + (long long)blockIdx.z * h * w;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kFusedWin * kFusedWin; idx += 256) {
    const int r = idx / kFusedWin, c = idx - r * kFusedWin;
    const int gy = gy0 + r, gx = gx0 + c;
    win[idx] = (gy >= 0 && gy < tsize && gx >= 0 && gx < tsize) ? quad_bilinear_sample(plane, h, w, q, gx, gy) : 0;
  }
  __syncthreads();
  for (int idx = tid; idx < kFusedWin * kFusedTile; idx += 256) {
    const int r = idx / kFusedTile, c = idx - r * kFusedTile;
    const int xo = ox0 + c;
    uint8_t v = 0;
    if (xo < osize) {
      int first, n;
      align_taps(bounds, xo, tsize, ksize, first, n);
      const int *k = kk + (long long)xo * ksize;
      int lo = first - gx0;  // window column of the first tap; taps outside the window (a foreign table) are dropped
      int j0 = lo < 0 ? -lo : 0;
      int j1 = n > kFusedWin - lo ? kFusedWin - lo : n;
      int acc = 1 << (kAlignPrecisionBits - 1);
      for (int j = j0; j < j1; ++j) acc += (int)win[r * kFusedWin + lo + j] * k[j];
      v = align_clip8(acc);
    }
    mid[idx] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < kFusedTile * kFusedTile; idx += 256) {
    const int r = idx / kFusedTile, c = idx - r * kFusedTile;
    const int yo = oy0 + r, xo = ox0 + c;
    if (yo >= osize || xo >= osize) continue;
    int first, n;
    align_taps(bounds, yo, tsize, ksize, first, n);
    const int *k = kk + (long long)yo * ksize;
    int lo = first - gy0;
    int j0 = lo < 0 ? -lo : 0;
    int j1 = n > kFusedWin - lo ? kFusedWin - lo : n;
    int acc = 1 << (kAlignPrecisionBits - 1);
    for (int j = j0; j < j1; ++j) acc += (int)mid[(lo + j) * kFusedTile + c] * k[j];
    out[((long long)blockIdx.z * osize + yo) * osize + xo] = align_clip8(acc);
  }
}

// scipy 'reflect' (d c b a | a b c d | d c b a) of index i on an axis of n samples, for -n <= i < 2n
__device__ __forceinline__ int align_reflect_edge(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

// np.pad 'reflect' (d c b | a b c d | c b a): padded index i -> source index on an axis of n samples, any pad width
__device__ __forceinline__ int align_reflect_pad(int i, int pad_before, int n) {
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  int j = (i - pad_before) % period;
  if (j < 0) j += period;
  return j < n ? j : period - j;
}

// Axis 0 of the Gaussian on the reflect-padded image.  src u8 [planes][h0][w0] -> tmp fp32 [planes][H][W], H = pad_t + h0 +
// pad_b, W = pad_l + w0 + pad_r.  grid (ceil(W/64), ceil(H/64), planes), 256 threads; LDS: (64 + 2r) x 64 bytes - a column strip
// of the padded image (bytes: exact), both reflections applied while loading.  wts: the 2r+1 normalised weights.
__global__ __launch_bounds__(256) void align_blur_v(float *__restrict__ tmp, const uint8_t *__restrict__ src,
                                                    const double *__restrict__ wts, int radius, int h0, int w0, int pad_l, int pad_t,
                                                    int H, int W) {
  HF_DYN_LDS;
  uint8_t *strip = hf_dyn_lds;
  const int rows = kPadTile + 2 * radius;
  const int X0 = blockIdx.x * kPadLanesV, Y0 = blockIdx.y * kPadTile;
  const uint8_t *plane = src + (long long)blockIdx.z * h0 * w0;
  for (int idx = threadIdx.x; idx < rows * kPadLanesV; idx += 256) {
    const int r = idx / kPadLanesV, c = idx - r * kPadLanesV;
    const int X = X0 + c, Y = Y0 - radius + r;
    uint8_t v = 0;
    if (X < W && Y >= -H && Y < 2 * H) {
      const int sy = align_reflect_pad(align_reflect_edge(Y, H), pad_t, h0);
      const int sx = align_reflect_pad(X, pad_l, w0);
      v = plane[(long long)sy * w0 + sx];
    }
    strip[idx] = v;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < kPadTile * kPadLanesV; idx += 256) {
    const int r = idx / kPadLanesV, c = idx - r * kPadLanesV;
    const int X = X0 + c, Y = Y0 + r;
    if (X >= W || Y >= H) continue;
    const uint8_t *l = strip + (r + radius) * kPadLanesV + c;
    double acc = (double)l[0] * wts[radius];
    for (int j = radius; j >= 1; --j) acc += ((double)l[-j * kPadLanesV] + (double)l[j * kPadLanesV]) * wts[radius - j];
    tmp[((long long)blockIdx.z * H + Y) * W + X] = (float)acc;
  }
}

// Axis 1 of the Gaussian and the blur fade: img = pad(src); img += (gauss - img) * clip(mask * 3 + 1, 0, 1) with
// mask = max(mx[x], my[y]) (the two ramps 1 - min(x / pad_l, (W-1-x) / pad_r), 1 - min(y / pad_t, (H-1-y) / pad_b) in float32
// from the host).  grid (ceil(W/64), ceil(H/16), planes); LDS: 16 x (64 + 2r) floats.
__global__ __launch_bounds__(256) void align_blur_h_fade(float *__restrict__ out, const float *__restrict__ tmp,
                                                         const uint8_t *__restrict__ src, const double *__restrict__ wts,
                                                         const float *__restrict__ mx, const float *__restrict__ my, int radius,
                                                         int h0, int w0, int pad_l, int pad_t, int H, int W) {
  HF_DYN_LDS;
  float *strip = reinterpret_cast<float *>(hf_dyn_lds);
  const int cols = kPadTile + 2 * radius;
  const int X0 = blockIdx.x * kPadTile, Y0 = blockIdx.y * kPadLanesH;
  const float *tp = tmp + (long long)blockIdx.z * H * W;
  for (int idx = threadIdx.x; idx < kPadLanesH * cols; idx += 256) {
    const int r = idx / cols, c = idx - r * cols;
    const int X = X0 - radius + c, Y = Y0 + r;
    strip[idx] = (Y < H && X >= -W && X < 2 * W) ? tp[(long long)Y * W + align_reflect_edge(X, W)] : 0.0f;
  }
  __syncthreads();
  const uint8_t *plane = src + (long long)blockIdx.z * h0 * w0;
  for (int idx = threadIdx.x; idx < kPadLanesH * kPadTile; idx += 256) {
    const int r = idx / kPadTile, c = idx - r * kPadTile;
    const int X = X0 + c, Y = Y0 + r;
    if (X >= W || Y >= H) continue;
    const float *l = strip + r * cols + c + radius;
    double acc = (double)l[0] * wts[radius];
    for (int j = radius; j >= 1; --j) acc += ((double)l[-j] + (double)l[j]) * wts[radius - j];
    const float gauss = (float)acc;
    const float img = (float)plane[(long long)align_reflect_pad(Y, pad_t, h0) * w0 + align_reflect_pad(X, pad_l, w0)];
    const float mask = fmaxf(mx[X], my[Y]);
    const float m3 = mask * 3.0f;
    const float a = fminf(fmaxf(m3 + 1.0f, 0.0f), 1.0f);
    const float d = gauss - img;
    const float t = d * a;
    out[((long long)blockIdx.z * H + Y) * W + X] = img + t;
  }
}

// img += (median[plane] - img) * clip(mask, 0, 1); pre (optional) = that float32; out = uint8(clip(rint(img), 0, 255))
__global__ __launch_bounds__(256) void align_pad_finish(uint8_t *__restrict__ out, float *__restrict__ pre,
                                                        const float *__restrict__ img, const float *__restrict__ median,
                                                        const float *__restrict__ mx, const float *__restrict__ my, int H, int W,
                                                        long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long hw = (long long)H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long plane = i / hw;
    const int p = (int)(i - plane * hw);
    const int y = p / W, x = p - y * W;
    const float a = fminf(fmaxf(fmaxf(mx[x], my[y]), 0.0f), 1.0f);
    const float v = img[i];
    const float d = median[plane] - v;
    const float t = d * a;
    const float r = v + t;
    if (pre) pre[i] = r;
    out[i] = (uint8_t)(int)fminf(fmaxf(rintf(r), 0.0f), 255.0f);
  }
}

__global__ __launch_bounds__(256) void u8_to_unit(float *__restrict__ out, const uint8_t *__restrict__ in, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (float)in[i] / 255.0f;
}

inline int align_grid(long long n) {
  long long g = (n + 255) / 256;
  return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

inline bool align_dims_ok(int planes, long long a, long long b) {  // a plane is indexed with int, the whole with long long
  return planes > 0 && planes <= 65535 && a > 0 && b > 0 && a * b <= 0x7fffffffLL;
}

}  // namespace

extern "C" int hf_resize_lanczos_u8(unsigned char *out, unsigned char *mid, const unsigned char *in, int planes, int h_in, int w_in,
                                    int h_out, int w_out, const int *bounds_x, const int *kk_x, int ksize_x, const int *bounds_y,
                                    const int *kk_y, int ksize_y, void *stream) {
  if (!out || !in || !align_dims_ok(planes, h_in, w_in) || !align_dims_ok(planes, h_out, w_out) || !align_dims_ok(planes, h_in, w_out))
    return HF_E_INVALID;
  const bool do_x = w_out != w_in, do_y = h_out != h_in;
  if (!do_x && !do_y) return HF_E_INVALID;  // nothing to resample: the caller copies
  if ((do_x && (!bounds_x || !kk_x || ksize_x <= 0)) || (do_y && (!bounds_y || !kk_y || ksize_y <= 0))) return HF_E_INVALID;
  if (do_x && do_y && (!mid || mid == out || mid == in)) return HF_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned char *vin = in;
  if (do_x) {
    unsigned char *hout = do_y ? mid : out;
    const long long total = (long long)planes * h_in * w_out;
    hipLaunchKernelGGL(resize_lanczos_h, dim3(align_grid(total)), dim3(256), 0, st, hout, in, bounds_x, kk_x, ksize_x, h_in, w_in,
                       w_out, total);
    if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
    vin = hout;
  }
  if (do_y) {
    const long long total = (long long)planes * h_out * w_out;
    hipLaunchKernelGGL(resize_lanczos_v, dim3(align_grid(total)), dim3(256), 0, st, out, vin, bounds_y, kk_y, ksize_y, h_in, h_out,
                       w_out, total);
  }
  return hf_launch_status();
}

extern "C" int hf_quad_bilinear_u8(unsigned char *out, const unsigned char *src, const double *coef8, int planes, int h, int w,
                                   int oh, int ow, void *stream) {
  if (!out || !src || !coef8 || !align_dims_ok(planes, h, w) || !align_dims_ok(planes, oh, ow)) return HF_E_INVALID;
  QuadCoef q;
  for (int k = 0; k < 8; ++k) q.a[k] = coef8[k];
  const long long total = (long long)planes * oh * ow;
  hipLaunchKernelGGL(quad_bilinear, dim3(align_grid(total)), dim3(256), 0, (hipStream_t)stream, out, src, q, h, w, oh, ow, total);
  return hf_launch_status();
}

extern "C" int hf_quad_lanczos4_u8(unsigned char *out, const unsigned char *src, const double *coef8, int planes, int h, int w,
                                   int osize, const int *bounds, const int *kk, int ksize, void *stream) {
  if (!out || !src || !coef8 || !bounds || !kk || ksize <= 0 || !align_dims_ok(planes, h, w) || osize <= 0 ||
      osize > 0x7fffffff / kFusedRatio / kFusedRatio / osize)
    return HF_E_INVALID;
  QuadCoef q;
  for (int k = 0; k < 8; ++k) q.a[k] = coef8[k];
  const int tiles = hf_cdiv(osize, kFusedTile);
  if (tiles > 65535) return HF_E_INVALID;
  hipLaunchKernelGGL(quad_lanczos4, dim3(tiles, tiles, planes), dim3(256), (size_t)kFusedWin * (kFusedWin + kFusedTile),
                     (hipStream_t)stream, out, src, q, h, w, osize, bounds, kk, ksize);
  return hf_launch_status();
}

extern "C" int hf_quad_lanczos4_ratio(void) { return kFusedRatio; }

extern "C" int hf_align_pad_blur_f32(float *out, float *tmp, const unsigned char *src, const double *weights, int radius,
                                     const float *mask_x, const float *mask_y, int planes, int h, int w, int pad_left, int pad_top,
                                     int pad_right, int pad_bottom, void *stream) {
  if (!out || !tmp || out == tmp || !src || !weights || !mask_x || !mask_y || !align_dims_ok(planes, h, w) || pad_left < 0 ||
      pad_top < 0 || pad_right < 0 || pad_bottom < 0 || radius < 0 || radius > kPadMaxRadius)
    return HF_E_INVALID;
  const long long H = (long long)pad_top + h + pad_bottom, W = (long long)pad_left + w + pad_right;
  if (!align_dims_ok(planes, H, W) || radius >= H || radius >= W) return HF_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  const int gy_v = hf_cdiv(H, kPadTile), gy_h = hf_cdiv(H, kPadLanesH);
  if (gy_v > 65535 || gy_h > 65535) return HF_E_INVALID;
  hipLaunchKernelGGL(align_blur_v, dim3(hf_cdiv(W, kPadLanesV), gy_v, planes), dim3(256),
                     (size_t)(kPadTile + 2 * radius) * kPadLanesV, st, tmp, src, weights, radius, h, w, pad_left, pad_top, (int)H,
                     (int)W);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  hipLaunchKernelGGL(align_blur_h_fade, dim3(hf_cdiv(W, kPadTile), gy_h, planes), dim3(256),
                     (size_t)kPadLanesH * (kPadTile + 2 * radius) * sizeof(float), st, out, tmp, src, weights, mask_x, mask_y, radius,
                     h, w, pad_left, pad_top, (int)H, (int)W);
  return hf_launch_status();
}

extern "C" int hf_align_pad_finish_u8(unsigned char *out, float *pre, const float *img, const float *median, const float *mask_x,
                                      const float *mask_y, int planes, int h, int w, void *stream) {
  if (!out || !img || !median || !mask_x || !mask_y || !align_dims_ok(planes, h, w)) return HF_E_INVALID;
  const long long total = (long long)planes * h * w;
  hipLaunchKernelGGL(align_pad_finish, dim3(align_grid(total)), dim3(256), 0, (hipStream_t)stream, out, pre, img, median, mask_x,
                     mask_y, h, w, total);
  return hf_launch_status();
}

extern "C" int hf_u8_to_unit_f32(float *out, const unsigned char *in, long long n, void *stream) {
  if (!out || !in || n <= 0) return HF_E_INVALID;
  hipLaunchKernelGGL(u8_to_unit, dim3(align_grid(n)), dim3(256), 0, (hipStream_t)stream, out, in, n);
  return hf_launch_status();
}
