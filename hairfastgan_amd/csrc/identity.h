// identity.h - identity similarity (ArcFace IR-SE50: losses/pp_losses.py:267-296 `IDLoss`,
// models/encoder4editing/criteria/id_loss.py): what stands around the network's body.  Included by encoder_ops.hip.
//
//   hf_crop_avgpool_f32        AdaptiveAvgPool2d of a window of the image, read in place (the face crop and `face_pool`)
//   hf_l2_normalize_rows_f32   x / |x|_2 per row (`l2_norm`, pp_losses.py:50-53)
//   hf_row_similarity_f64      dot products of unit rows: the N pairs or the whole [N,M] matrix, summed in fp64
//
// Plain vector stores, no atomics; every output element has ONE owner and every sum a fixed order: an image's, a row's or an
// entry's bits depend on its own data alone, never on how many others the launch holds.
// metric_common.h: hf_block_sum_f64 (l2_normalize_rows), hf_aligned, hf_lane_blocks (hf_crop_avgpool_f32).
#pragma once
#include <cmath>
#include <cstdint>

#include "metric_common.h"

namespace {

constexpr int kSimWaves = 4;  // similarity: entries of a block (one wave each)

// one lane per output element.  Bin (i, j) covers the rows y0 + floor(i ch / oh) .. y0 + ceil((i + 1) ch / oh) - 1 of the
// image and the columns likewise (torch's adaptive windows, laid over the crop); its pixels are added in fp32 in row-major
// order (rows ascending, columns ascending inside a row), starting from the first pixel, and the sum is divided by the
// count.  With an affine the result is fmaf(scale[c], mean, shift[c]) (a missing scale is 1, a missing shift 0).
__global__ __launch_bounds__(256) void crop_avgpool(float *__restrict__ out, const float *__restrict__ x, const float *__restrict__ scale,
                                                    const float *__restrict__ shift, int c, int h, int w, int y0, int x0, int ch,
                                                    int cw, int oh, int ow, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e % ow);
  const long long r = e / ow;
  const int i = (int)(r % oh);
  const long long plane = r / oh;
  const int ya = y0 + (int)(((long long)i * ch) / oh), yb = y0 + (int)((((long long)i + 1) * ch + oh - 1) / oh);
  const int xa = x0 + (int)(((long long)j * cw) / ow), xb = x0 + (int)((((long long)j + 1) * cw + ow - 1) / ow);
  const float *src = x + plane * h * w;
  float acc = 0.0f;
  for (int yy = ya; yy < yb; ++yy)
    for (int xx = xa; xx < xb; ++xx) acc += src[(long long)yy * w + xx];
  float v = acc / (float)((yb - ya) * (xb - xa));
  if (scale || shift) {
    const int cc = (int)(plane % c);
    v = fmaf(scale ? scale[cc] : 1.0f, v, shift ? shift[cc] : 0.0f);
  }
  out[e] = v;
}

// grid (rows), 256 threads, LDS [256] fp64: thread t adds the squares of x[t], x[t + 256], ... in that order in fp64 (the
// square of an fp32 value is exact there), a tree of fixed shape adds the threads; norm = fp32(sqrt(total)), and every
// element is divided by it in fp32 (torch.div, not a multiplication by the reciprocal).
__global__ __launch_bounds__(256) void l2_normalize_rows(float *__restrict__ out, float *__restrict__ norms, const float *__restrict__ x,
                                                         int d) {
  HF_DYN_LDS;
  double *red = reinterpret_cast<double *>(hf_dyn_lds);
  const int tid = threadIdx.x;
  const float *xr = x + (long long)blockIdx.x * d;
  double s = 0.0;
  for (int k = tid; k < d; k += 256) {
    const double v = (double)xr[k];
    s += v * v;
  }
  const float norm = (float)sqrt(hf_block_sum_f64(s, red));
  for (int k = tid; k < d; k += 256) out[(long long)blockIdx.x * d + k] = xr[k] / norm;
  if (norms && tid == 0) norms[blockIdx.x] = norm;
}

// grid (ceil(entries / 4)), 256 threads = 4 entries x 64 lanes, LDS [256] fp64.  Entry e is (i, j) = (e, e) (paired) or
// (e / m, e % m) (matrix); lane l adds a[i][k] b[j][k] for k = l, l + 64, ... in that order in fp64 (the product of two
// fp32 values is exact there, so fusing the multiply into the add changes nothing), a tree of fixed shape adds the lanes.
__global__ __launch_bounds__(256) void row_similarity(double *__restrict__ out, const float *__restrict__ a, const float *__restrict__ b,
                                                      long long entries, int m, int d, int paired) {
  HF_DYN_LDS;
  double *red = reinterpret_cast<double *>(hf_dyn_lds);
  const int tid = threadIdx.x, lane = tid & 63;
  const long long e = (long long)blockIdx.x * kSimWaves + (tid >> 6);
  double s = 0.0;
  if (e < entries) {
    const long long i = paired ? e : e / m, j = paired ? e : e % m;
    const float *ar = a + i * d, *br = b + j * d;
    for (int k = lane; k < d; k += 64) s += (double)ar[k] * (double)br[k];
  }
  red[tid] = s;
  __syncthreads();
  for (int hlf = 32; hlf >= 1; hlf >>= 1) {
    if (lane < hlf) red[tid] += red[tid + hlf];
    __syncthreads();
  }
  if (lane == 0 && e < entries) out[e] = red[tid];
}

}  // namespace

extern "C" int hf_crop_avgpool_f32(float *out, const float *x, const float *scale, const float *shift, int n, int c, int h, int w,
                                   int y0, int x0, int ch, int cw, int oh, int ow, void *stream) {
  if (!hf_aligned(out, 4) || !hf_aligned(x, 4) || n <= 0 || c <= 0 || h <= 0 || w <= 0 || ch <= 0 || cw <= 0 || oh <= 0 || ow <= 0 ||
      y0 < 0 || x0 < 0 || (long long)y0 + ch > h || (long long)x0 + cw > w || (long long)h * w > 0x7fffffffLL)
    return HF_E_INVALID;
  const long long total = (long long)n * c * oh * ow;
  unsigned blocks;
  if (!hf_lane_blocks(total, blocks)) return HF_E_INVALID;
  hipLaunchKernelGGL(crop_avgpool, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, x, scale, shift, c, h, w, y0, x0, ch,
                     cw, oh, ow, total);
  return hf_launch_status();
}

extern "C" int hf_l2_normalize_rows_f32(float *out, float *norms, const float *x, int rows, int d, void *stream) {
  if (!hf_aligned(out, 4) || !hf_aligned(x, 4) || (norms && !hf_aligned(norms, 4)) || rows <= 0 || d <= 0) return HF_E_INVALID;
  hipLaunchKernelGGL(l2_normalize_rows, dim3(rows), dim3(256), 256 * sizeof(double), (hipStream_t)stream, out, norms, x, d);
  return hf_launch_status();
}

extern "C" int hf_row_similarity_f64(double *out, const float *a, const float *b, int n, int m, int d, int paired, void *stream) {
  if (!hf_aligned(out, 8) || !hf_aligned(a, 4) || !hf_aligned(b, 4) || n <= 0 || m <= 0 || d <= 0 || (paired && n != m))
    return HF_E_INVALID;
  const long long entries = paired ? n : (long long)n * m, blocks = (entries + kSimWaves - 1) / kSimWaves;
  if (blocks > 0x7fffffffLL) return HF_E_INVALID;
  hipLaunchKernelGGL(row_similarity, dim3((unsigned)blocks), dim3(256), 256 * sizeof(double), (hipStream_t)stream, out, a, b, entries, m,
                     d, paired ? 1 : 0);
  return hf_launch_status();
}
