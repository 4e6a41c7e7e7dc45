// poisson.h - Poisson image blending of utils/image_utils.py:58-94 (the reference writes three PNGs and runs
// `fpie -s face -t final -m mask -n maxn -g max`): included by encoder_ops.hip.
//
//   hf_quantize_u8_f32      torchvision save_image's byte: uint8(trunc(clamp(fl(fl(x*255) + 0.5), 0, 255)))
//   hf_poisson_setup_u8     u8 source / target / mask -> right-hand side B and start value X_0 of the Jacobi solve
//   hf_poisson_jacobi_f32   1..T synchronous Jacobi sweeps in ONE launch (temporal blocking in LDS)
//   hf_poisson_finish_u8    X -> u8 result (target outside the solved region)
//
// The equation system (fpie's "max" gradient mode; restated, fpie's source is not pinned): Omega = pixels whose mask
// byte is >= 128, minus the outermost row and column of the image.  For p in Omega
//   B(p) = sum_{q in (L,R,U,D)} mix(s_p - s_q, t_p - t_q) + sum_{q in N(p) \ Omega} t_q,   mix(a,b) = |a| < |b| ? b : a
// (integers: exact in fp32), X_0 = t on Omega and 0 elsewhere, and every sweep
//   X_{k+1}(p) = ((((B + X_k(up)) + X_k(down)) + X_k(left)) + X_k(right)) / 4    (fp32, this order; X = 0 off Omega).
// Temporal blocking: a workgroup owns a 64 x 64 output tile of one (image, channel) plane, loads it with a halo of T
// pixels into two LDS buffers and runs up to T sweeps there (one barrier per sweep).  A sweep is the same expression
// at every point of the region except its outermost ring, which keeps its loaded value; a wrong value spreads one
// pixel per sweep from that ring, so after n <= T sweeps the tile - T pixels inside the ring - holds exactly the
// values T single-sweep launches would give.
#pragma once
#include <cstdint>

#include "hf_common.h"

namespace {

constexpr int kPoissonTile = 64;
constexpr int kPoissonThreads = 256;

__global__ __launch_bounds__(256) void quantize_u8(uint8_t *__restrict__ out, const float *__restrict__ x, long long n) {
  // save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8) - two roundings, never one fused multiply-add
#pragma clang fp contract(off)
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float scaled = x[i] * 255.0f;
    const float v = scaled + 0.5f;
    out[i] = (uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);
  }
}

__device__ __forceinline__ bool poisson_in_omega(const uint8_t *__restrict__ mask, int y, int x, int h, int w) {
  return y >= 1 && y <= h - 2 && x >= 1 && x <= w - 2 && mask[(long long)y * w + x] >= 128;
}

// one thread per (image, channel, pixel); mask [images][h][w], s / t / b / x0 [images][channels][h][w]
__global__ __launch_bounds__(256) void poisson_setup(float *__restrict__ b, float *__restrict__ x0, const uint8_t *__restrict__ src,
                                                     const uint8_t *__restrict__ tgt, const uint8_t *__restrict__ mask, int channels,
                                                     int h, int w, long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long hw = (long long)h * w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long plane = i / hw;
    const int p = (int)(i - plane * hw);
    const int y = p / w, x = p - y * w;
    const uint8_t *m = mask + (plane / channels) * hw;
    if (!poisson_in_omega(m, y, x, h, w)) {
      b[i] = 0.0f;
      x0[i] = 0.0f;
      continue;
    }
    const uint8_t *s = src + plane * hw, *t = tgt + plane * hw;
    const int sp = s[p], tp = t[p];
    const int nb[4] = {p - 1, p + 1, p - w, p + w};  // Omega excludes the border: all four are inside the image
    const int ny[4] = {y, y, y - 1, y + 1}, nx[4] = {x - 1, x + 1, x, x};
    int acc = 0;
    for (int k = 0; k < 4; ++k) {
      const int gs = sp - s[nb[k]], gt = tp - t[nb[k]];
      acc += (gs < 0 ? -gs : gs) < (gt < 0 ? -gt : gt) ? gt : gs;  // tie: the source gradient
      if (!poisson_in_omega(m, ny[k], nx[k], h, w)) acc += t[nb[k]];
    }
    b[i] = (float)acc;
    x0[i] = (float)tp;
  }
}

// grid (tiles_x, tiles_y, images * channels), 256 threads; LDS: two (64 + 2T)^2 fp32 buffers.  Each thread owns the
// region points tid + 256 k; their B and "is updated" flag stay in registers for the whole launch.
template <int T>
__global__ __launch_bounds__(256) void poisson_jacobi(float *__restrict__ x_out, const float *__restrict__ x_in,
                                                      const float *__restrict__ b, const uint8_t *__restrict__ mask, int channels,
                                                      int h, int w, int sweeps) {
  constexpr int R = kPoissonTile + 2 * T, RR = R * R;
  constexpr int NP = (RR + kPoissonThreads - 1) / kPoissonThreads;
  static_assert(NP <= 64, "update flags are one 64-bit word");
  HF_DYN_LDS;
  float *buf0 = reinterpret_cast<float *>(hf_dyn_lds);
  float *buf1 = buf0 + RR;
  const int plane = blockIdx.z;
  const long long hw = (long long)h * w;
  const float *xin = x_in + plane * hw, *bp = b + plane * hw;
  const uint8_t *m = mask + (long long)(plane / channels) * hw;
  const int y0 = blockIdx.y * kPoissonTile - T, x0 = blockIdx.x * kPoissonTile - T;
  const int tid = threadIdx.x;
  float bv[NP];
  unsigned long long upd = 0;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int idx = tid + k * kPoissonThreads;
    bv[k] = 0.0f;
    if (idx < RR) {
      const int r = idx / R, c = idx - r * R;
      const int gy = y0 + r, gx = x0 + c;
      const bool om = gy >= 0 && gy < h && gx >= 0 && gx < w && poisson_in_omega(m, gy, gx, h, w);
      const float xv = om ? xin[(long long)gy * w + gx] : 0.0f;
      buf0[idx] = xv;
      buf1[idx] = xv;  // the ring and the points off Omega are never written again: both buffers hold them
      if (om) bv[k] = bp[(long long)gy * w + gx];
      if (om && r >= 1 && r <= R - 2 && c >= 1 && c <= R - 2) upd |= 1ull << k;
    }
  }
  __syncthreads();
  for (int s = 0; s < sweeps; ++s) {
    const float *cur = (s & 1) ? buf1 : buf0;
    float *nxt = (s & 1) ? buf0 : buf1;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      if (upd >> k & 1ull) {
        const int idx = tid + k * kPoissonThreads;
        nxt[idx] = ((((bv[k] + cur[idx - R]) + cur[idx + R]) + cur[idx - 1]) + cur[idx + 1]) * 0.25f;
      }
    }
    __syncthreads();
  }
  const float *fin = (sweeps & 1) ? buf1 : buf0;
  float *xo = x_out + plane * hw;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int idx = tid + k * kPoissonThreads;
    if (idx < RR) {
      const int r = idx / R, c = idx - r * R;
      const int gy = y0 + r, gx = x0 + c;
      if (r >= T && r < T + kPoissonTile && c >= T && c < T + kPoissonTile && gy < h && gx < w) xo[(long long)gy * w + gx] = fin[idx];
    }
  }
}

__global__ __launch_bounds__(256) void poisson_finish(uint8_t *__restrict__ out, const float *__restrict__ x,
                                                      const uint8_t *__restrict__ tgt, const uint8_t *__restrict__ mask, int channels,
                                                      int h, int w, long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long hw = (long long)h * w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long plane = i / hw;
    const int p = (int)(i - plane * hw);
    const int y = p / w;
    out[i] = poisson_in_omega(mask + (plane / channels) * hw, y, p - y * w, h, w)
                 ? (uint8_t)(int)fminf(fmaxf(x[i], 0.0f), 255.0f)
                 : tgt[i];
  }
}

inline int poisson_grid(long long n) {
  long long g = (n + 255) / 256;
  return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

template <int T>
int poisson_jacobi_launch(float *x_out, const float *x_in, const float *b, const uint8_t *mask, int images, int channels, int h,
                          int w, int sweeps, hipStream_t st) {
  constexpr int R = kPoissonTile + 2 * T;
  const dim3 grid((w + kPoissonTile - 1) / kPoissonTile, (h + kPoissonTile - 1) / kPoissonTile, images * channels);
  hipLaunchKernelGGL(poisson_jacobi<T>, grid, dim3(kPoissonThreads), (size_t)2 * R * R * sizeof(float), st, x_out, x_in, b, mask,
                     channels, h, w, sweeps);
  return hf_launch_status();
}

}  // namespace

extern "C" int hf_quantize_u8_f32(unsigned char *out, const float *x, long long n, void *stream) {
  if (!out || !x || n <= 0) return HF_E_INVALID;
  hipLaunchKernelGGL(quantize_u8, dim3(poisson_grid(n)), dim3(256), 0, (hipStream_t)stream, out, x, n);
  return hf_launch_status();
}

extern "C" int hf_poisson_setup_u8(float *b, float *x0, const unsigned char *src, const unsigned char *tgt, const unsigned char *mask,
                                   int images, int channels, int h, int w, void *stream) {
  if (!b || !x0 || !src || !tgt || !mask || images <= 0 || channels <= 0 || h <= 0 || w <= 0) return HF_E_INVALID;
  const long long total = (long long)images * channels * h * w;
  hipLaunchKernelGGL(poisson_setup, dim3(poisson_grid(total)), dim3(256), 0, (hipStream_t)stream, b, x0, src, tgt, mask, channels, h,
                     w, total);
  return hf_launch_status();
}

extern "C" int hf_poisson_jacobi_f32(float *x_out, const float *x_in, const float *b, const unsigned char *mask, int images,
                                     int channels, int h, int w, int sweeps, int tblock, void *stream) {
  if (!x_out || !x_in || !b || !mask || x_out == x_in || images <= 0 || channels <= 0 || h <= 0 || w <= 0 ||
      (long long)images * channels > 65535 || sweeps < 1 || sweeps > tblock)
    return HF_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  switch (tblock) {
    case 1: return poisson_jacobi_launch<1>(x_out, x_in, b, mask, images, channels, h, w, sweeps, st);
    case 2: return poisson_jacobi_launch<2>(x_out, x_in, b, mask, images, channels, h, w, sweeps, st);
    case 4: return poisson_jacobi_launch<4>(x_out, x_in, b, mask, images, channels, h, w, sweeps, st);
    case 8: return poisson_jacobi_launch<8>(x_out, x_in, b, mask, images, channels, h, w, sweeps, st);
    case 16: return poisson_jacobi_launch<16>(x_out, x_in, b, mask, images, channels, h, w, sweeps, st);
    default: return HF_E_INVALID;
  }
}

extern "C" int hf_poisson_finish_u8(unsigned char *out, const float *x, const unsigned char *tgt, const unsigned char *mask,
                                    int images, int channels, int h, int w, void *stream) {
  if (!out || !x || !tgt || !mask || images <= 0 || channels <= 0 || h <= 0 || w <= 0) return HF_E_INVALID;
  const long long total = (long long)images * channels * h * w;
  hipLaunchKernelGGL(poisson_finish, dim3(poisson_grid(total)), dim3(256), 0, (hipStream_t)stream, out, x, tgt, mask, channels, h, w,
                     total);
  return hf_launch_status();
}
