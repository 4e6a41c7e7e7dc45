// ssim.h - structural similarity (SSIM, MS-SSIM: losses/lpips/__init__.py:52-53 `dssim`, losses/lpips/networks_basic.py:167
// `DSSIM`, there scikit-image on the host): included by encoder_ops.hip after lpips.h (metric_finish).
//
//   hf_ssim_planes_f64     the window moments of two images, the SSIM formula and its sums in ONE launch, all in fp64; on
//                          request the map, the contrast-structure sums, a weighted sum and the next 2x2-mean pyramid level
//
// Why fp64: the variances are E[x^2] - E[x]^2, a difference of large numbers next to C2 = (0.03 R)^2; in fp32 the image mean of
// S is off by up to 1.6e-6 and flat regions by more.
// Plain vector stores, no atomics; every output element has ONE owner and every sum a fixed order: a plane's bits depend on
// the plane's shape and content alone, not on the number of planes or its place among them.
// metric_common.h: hf_block_sum_f64, hf_aligned.  lpips.h: metric_finish.
#pragma once
#include <cstdint>

#include "metric_common.h"

namespace {

constexpr int kSsTileW = 32;   // output pixels of a block: 32 columns (one per lane of a half wave) ...
constexpr int kSsTileH = 16;   // ... x 16 rows: lane (tx, g) owns rows 2 g and 2 g + 1 of column tx
constexpr int kSsRowPitch = kSsTileW + 1;  // doubles between two rows of a moment plane (33: see the horizontal pass)
constexpr int kSsRun = 4;      // horizontal pass: consecutive columns of one row that a lane produces
constexpr int kSsMinWin = 3, kSsMaxWin = 11;
constexpr int kSsU8 = 0, kSsF32 = 1, kSsF64 = 2;  // the `dtype` codes of hf_ssim_planes_f64

inline size_t ssim_elem_size(int dtype) { return dtype == kSsU8 ? 1 : (dtype == kSsF32 ? 4 : 8); }
// elements of one staged input tile, rounded up to 16 so that the second tile starts 16-byte aligned for every type
__host__ __device__ inline int ssim_tile_elems(int win) { return ((kSsTileH + win - 1) * (kSsTileW + win - 1) + 15) & ~15; }
inline size_t ssim_lds_bytes(int dtype, int win) {
  return (size_t)(256 + 5 * (kSsTileH + win - 1) * kSsRowPitch) * sizeof(double) + 2 * (size_t)ssim_tile_elems(win) * ssim_elem_size(dtype);
}

// grid (tiles_x tiles_y, planes), 256 threads.  A block owns the output tile [ty0, ty0 + 16) x [tx0, tx0 + 32) of one plane.
// LDS: red [256] fp64 | five moment planes [rows_in][33] fp64 | the x and the y tile [rows_in][cols_in] in their OWN type T
// (rows_in = 16 + WIN - 1, cols_in = 32 + WIN - 1; outside the plane: 0).  The taps live in registers (WIN is a template
// argument, every tap loop is unrolled).
//   1. the input tiles are read once from memory (bounds-checked) into LDS
//   2. next level (on request): the block owns the input rows [ty0, ty0 + 16) - the last tile row all rows up to h - and the
//      columns likewise; both tile sizes are even, so no 2x2 cell straddles two blocks, and every owned pixel lies in the
//      staged tile.  mean = (((a00 + a01) + a10) + a11) * 0.25.
//   3. horizontal pass: element (r, c) of the moment planes = sum_b w[b] z[r][c + b], b ascending, for z = x, y, xx, yy, xy.
//      A lane produces 4 consecutive columns of a row from the WIN + 3 inputs under them: every input is read, converted and
//      multiplied (x x, y y, x y) once and feeds up to 4 sums.  Lane t: row 4 (t >> 5) + ((t >> 2) & 3), columns
//      4 ((t & 3) + 4 ((t >> 4) & 1)) ..: the 16 lanes of a store group cover 4 column runs of 4 rows, and with a row pitch of
//      33 doubles their 16 stores fall on 16 different bank pairs; the vertical pass reads 32 consecutive doubles of a row.
//   4. vertical pass in registers: lane (tx, g) reads rows 2 g .. 2 g + WIN of column tx ONCE and feeds both its pixels,
//      each sum in ascending a; then the formula (the expression order is the contract of include/hairfast_hip.h)
//   5. two block sums through hf_block_sum_f64 into part[0][plane][block] and part[1][plane][block]
// Every sum starts from 0.0 and adds products in ascending tap order wherever the pixel lies in its tile.
template <typename T, int WIN>
__global__ __launch_bounds__(256) void ssim_planes(double *__restrict__ part, double *__restrict__ map, double *__restrict__ next_x,
                                                   double *__restrict__ next_y, const T *__restrict__ x, const T *__restrict__ y,
                                                   const float *__restrict__ mask, const double *__restrict__ taps_g, int channels,
                                                   int h, int w, int tiles_x, double c1, double c2, double cn) {
#pragma clang fp contract(off)
  HF_DYN_LDS;
  constexpr int rows_in = kSsTileH + WIN - 1, cols_in = kSsTileW + WIN - 1;
  constexpr int msize = rows_in * kSsRowPitch;  // one moment plane
  double *red = reinterpret_cast<double *>(hf_dyn_lds);
  double *mom = red + 256;
  T *xs = reinterpret_cast<T *>(mom + 5 * msize);
  T *ys = xs + ssim_tile_elems(WIN);
  const int tid = threadIdx.x, plane = blockIdx.y;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int ty0 = tile_y * kSsTileH, tx0 = tile_x * kSsTileW;
  const int oh = h - WIN + 1, ow = w - WIN + 1;
  const long long in_off = (long long)plane * h * w;
  const T *px = x + in_off, *py = y + in_off;
  double taps[WIN];
#pragma unroll
  for (int k = 0; k < WIN; ++k) taps[k] = taps_g[k];

  for (int e = tid; e < rows_in * cols_in; e += 256) {
    const int r = e / cols_in, c = e - r * cols_in;
    const int gy = ty0 + r, gx = tx0 + c;
    const bool in = gy < h && gx < w;
    const long long at = (long long)gy * w + gx;
    xs[e] = in ? px[at] : T(0);
    ys[e] = in ? py[at] : T(0);
  }
  __syncthreads();

  if (next_x) {
    const int nh = h >> 1, nw = w >> 1;
    const bool last_y = ty0 + kSsTileH >= oh, last_x = tx0 + kSsTileW >= ow;
    const int cy0 = ty0 >> 1, cx0 = tx0 >> 1;
    const int cy1 = last_y ? nh : (ty0 + kSsTileH) >> 1, cx1 = last_x ? nw : (tx0 + kSsTileW) >> 1;
    const int ch = cy1 - cy0, cw = cx1 - cx0;  // at most (16 + WIN - 1) / 2 x (32 + WIN - 1) / 2 cells, all inside the staged tile
    const long long out_off = (long long)plane * nh * nw;
    for (int e = tid; e < ch * cw; e += 256) {
      const int r = e / cw, c = e - r * cw;
      const int at = 2 * r * cols_in + 2 * c;
      const long long o = out_off + (long long)(cy0 + r) * nw + cx0 + c;
      next_x[o] = ((((double)xs[at] + (double)xs[at + 1]) + (double)xs[at + cols_in]) + (double)xs[at + cols_in + 1]) * 0.25;
      next_y[o] = ((((double)ys[at] + (double)ys[at + 1]) + (double)ys[at + cols_in]) + (double)ys[at + cols_in + 1]) * 0.25;
    }
  }

  {
    const int r = 4 * (tid >> 5) + ((tid >> 2) & 3), c0 = kSsRun * ((tid & 3) + 4 * ((tid >> 4) & 1));
    if (r < rows_in) {  // rows_in <= 26 of the 32 rows the 256 lanes span
      const T *rx = xs + r * cols_in + c0, *ry = ys + r * cols_in + c0;
      double acc[kSsRun][5];
#pragma unroll
      for (int o = 0; o < kSsRun; ++o)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
#pragma unroll
      for (int j = 0; j < WIN + kSsRun - 1; ++j) {  // input j is tap j - o of output o
        const double a = (double)rx[j], v = (double)ry[j];
        const double aa = a * a, vv = v * v, av = a * v;
#pragma unroll
        for (int o = 0; o < kSsRun; ++o) {
          if (j - o >= 0 && j - o < WIN) {
            const double wb = taps[j - o];
            acc[o][0] += wb * a;
            acc[o][1] += wb * v;
            acc[o][2] += wb * aa;
            acc[o][3] += wb * vv;
            acc[o][4] += wb * av;
          }
        }
      }
      double *dst = mom + r * kSsRowPitch + c0;
#pragma unroll
      for (int o = 0; o < kSsRun; ++o)
#pragma unroll
        for (int m = 0; m < 5; ++m) dst[m * msize + o] = acc[o][m];
    }
  }
  __syncthreads();

  const int tx = tid & (kSsTileW - 1), g = tid >> 5;
  double acc[2][5];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[i][m] = 0.0;
#pragma unroll
  for (int r = 0; r <= WIN; ++r) {  // rows 2 g .. 2 g + WIN of the moment planes: row r is tap r of pixel 0 and tap r - 1 of pixel 1
    const double *src = mom + (2 * g + r) * kSsRowPitch + tx;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      const double v = src[m * msize];
      if (r < WIN) acc[0][m] += taps[r < WIN ? r : 0] * v;
      if (r >= 1) acc[1][m] += taps[r >= 1 ? r - 1 : 0] * v;
    }
  }
  const int ox = tx0 + tx;
  double sum_s = 0.0, sum_aux = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int oy = ty0 + 2 * g + i;
    if (oy >= oh || ox >= ow) continue;
    const double ux = acc[i][0], uy = acc[i][1], uxx = acc[i][2], uyy = acc[i][3], uxy = acc[i][4];
    const double vx = cn * (uxx - ux * ux), vy = cn * (uyy - uy * uy), vxy = cn * (uxy - ux * uy);
    const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2;
    const double b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
    const double cs = a2 / b2, s = (a1 * a2) / (b1 * b2);
    if (map) map[((long long)plane * oh + oy) * ow + ox] = s;
    if (mask) {
      const double m = (double)mask[((long long)(plane / channels) * oh + oy) * ow + ox];
      sum_s += m * s;
      sum_aux += m;
    } else {
      sum_s += s;
      sum_aux += cs;
    }
  }
  const long long slot = (long long)plane * gridDim.x + blockIdx.x, half = (long long)gridDim.y * gridDim.x;
  const double total_s = hf_block_sum_f64(sum_s, red);
  __syncthreads();
  const double total_aux = hf_block_sum_f64(sum_aux, red);
  if (tid == 0) {
    part[slot] = total_s;
    part[half + slot] = total_aux;
  }
}

inline bool ssim_shape_ok(int planes, int h, int w, int win) {
  return planes > 0 && planes <= 65535 && win >= kSsMinWin && win <= kSsMaxWin && (win & 1) && h >= win && w >= win &&
         (long long)h * w <= 0x7fffffffLL;  // so the tiles of a plane fit a grid's x dimension as well
}

struct SsimLaunch {
  hipStream_t st;
  int dtype, planes, tiles, channels, h, w, tiles_x;
  double *work, *map, *next_x, *next_y;
  const void *x, *y;
  const float *mask;
  const double *taps;
  double c1, c2, cn;
};

template <typename T, int WIN>
void ssim_launch_win(const SsimLaunch &a) {
  hipLaunchKernelGGL((ssim_planes<T, WIN>), dim3(a.tiles, a.planes), dim3(256), ssim_lds_bytes(a.dtype, WIN), a.st, a.work, a.map, a.next_x,
                     a.next_y, static_cast<const T *>(a.x), static_cast<const T *>(a.y), a.mask, a.taps, a.channels, a.h, a.w, a.tiles_x,
                     a.c1, a.c2, a.cn);
}

template <typename T>
void ssim_launch(const SsimLaunch &a, int win) {
  switch (win) {
    case 3: return ssim_launch_win<T, 3>(a);
    case 5: return ssim_launch_win<T, 5>(a);
    case 7: return ssim_launch_win<T, 7>(a);
    case 9: return ssim_launch_win<T, 9>(a);
    default: return ssim_launch_win<T, 11>(a);
  }
}

}  // namespace

extern "C" long long hf_ssim_work_doubles(int planes, int h, int w, int win) {
  if (!ssim_shape_ok(planes, h, w, win)) return 0;
  return 2LL * planes * hf_cdiv(h - win + 1, kSsTileH) * hf_cdiv(w - win + 1, kSsTileW);
}

extern "C" int hf_ssim_tile(int axis) { return axis == 0 ? kSsTileH : kSsTileW; }

extern "C" int hf_ssim_planes_f64(double *sum_s, double *sum_aux, double *map, double *next_x, double *next_y, const void *x,
                                  const void *y, const float *mask, const double *taps, double *work, int dtype, int planes,
                                  int channels, int h, int w, int win, double c1, double c2, double cn, void *stream) {
  if (dtype != kSsU8 && dtype != kSsF32 && dtype != kSsF64) return HF_E_INVALID;
  const unsigned align = (unsigned)ssim_elem_size(dtype);
  if (!hf_aligned(sum_s, 8) || !hf_aligned(x, align) || !hf_aligned(y, align) || !hf_aligned(taps, 8) || !hf_aligned(work, 8) ||
      (sum_aux && !hf_aligned(sum_aux, 8)) || (map && !hf_aligned(map, 8)) || (next_x && !hf_aligned(next_x, 8)) ||
      (next_y && !hf_aligned(next_y, 8)) || (mask && !hf_aligned(mask, 4)) || !ssim_shape_ok(planes, h, w, win))
    return HF_E_INVALID;
  if ((next_x == nullptr) != (next_y == nullptr) || (next_x && (h < 2 || w < 2))) return HF_E_INVALID;
  if (mask && (channels <= 0 || planes % channels != 0)) return HF_E_INVALID;
  const int tiles_x = hf_cdiv(w - win + 1, kSsTileW), tiles = tiles_x * hf_cdiv(h - win + 1, kSsTileH);
  const hipStream_t st = (hipStream_t)stream;
  const SsimLaunch args{st, dtype, planes, tiles, mask ? channels : 1, h, w, tiles_x, work, map, next_x, next_y, x, y, mask, taps, c1, c2, cn};
  if (dtype == kSsU8)
    ssim_launch<unsigned char>(args, win);
  else if (dtype == kSsF32)
    ssim_launch<float>(args, win);
  else
    ssim_launch<double>(args, win);
  hipLaunchKernelGGL(metric_finish, dim3(planes), dim3(256), 256 * sizeof(double), st, sum_s, (const double *)work, tiles, 1.0, 0);
  if (sum_aux)
    hipLaunchKernelGGL(metric_finish, dim3(planes), dim3(256), 256 * sizeof(double), st, sum_aux,
                       (const double *)(work + (long long)planes * tiles), tiles, 1.0, 0);
  return hf_launch_status();
}
