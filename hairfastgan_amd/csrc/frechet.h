// frechet.h - the Frechet distance between two Gaussians fitted to feature sets (FID / FID-CLIP: scripts/fid_metric.py:25-50,
// utils/train.py:90-161, which leave it to torchmetrics and a host eigensolver): included by encoder_ops.hip.
//
//   hf_frechet_accumulate_f64      sum += sum_n f[n], cov_sum += sum_n f[n] f[n]^T of an fp32 (or fp16) feature batch
//   hf_frechet_stats_f64           mu = sum / n, cov = (cov_sum - n mu mu^T) / (n - 1)
//   hf_sym_eig_jacobi_f64          eigenvalues (and vectors) of a symmetric matrix: cyclic two-sided Jacobi
//   hf_frechet_congruence_f64      M = B S2 B^T with B = diag(sqrt(max(w, 0))) V^T, i.e. S1^(1/2) S2 S1^(1/2) in S1's eigenbasis
//   hf_frechet_finish_f64          |mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum_i sqrt(max(ev_i, 0))
//
// All arithmetic is fp64 on the vector ALU; every output element has ONE owner thread that adds in a fixed order, and
// the reductions go through LDS trees of a fixed shape: results do not depend on the grid or on timing.
//
// The distance takes the symmetric route: the spectrum of S1 S2 is that of S1^(1/2) S2 S1^(1/2), a symmetric positive
// semi-definite matrix, so two symmetric eigenproblems (the first with vectors) replace the reference's eigvals of the
// non-symmetric product.
//
// Jacobi scheme.  The d indices (plus one phantom index when d is odd) play a round-robin tournament: m = d rounded up to
// even, m - 1 rounds per sweep, m / 2 disjoint pairs (p, q) per round; a pair with the phantom index is a bye.  All
// rotations of one round commute in the sense that A' = J^T A J with J the product of the round's rotations, and the
// 2 x 2 block of A' at (row pair i, column pair j) needs only the block of A at the same place and the two rotations, which
// follow from A's diagonal blocks i and j.  So a round is ONE launch A_in -> A_out over ping-pong buffers: a thread
// recomputes both rotations from A_in and writes R_i^T B R_j; nothing is read that the same launch writes, no block
// waits on another and nothing spins on memory.  Only the blocks i <= j are computed and stored together with their mirror
// images: A stays exactly symmetric.  The same thread grid rotates the columns of V (V' = V J).
// A rotation is skipped when |a_pq| <= eps sqrt(|a_pp a_qq|).  After every sweep one block reduces the off-diagonal
// norm, the Frobenius norm and the number of pairs still above that threshold to three device doubles, which the host reads
// (one 24-byte copy per sweep) to stop: converged when no pair is above the threshold - the next sweep would be the
// identity - or when off <= eps |A|_F.  The absolute test alone cannot be met in general: the skip rule may leave d^2
// elements of the size of its threshold behind.
// metric_common.h: hf_block_sum_f64 (jacobi_norms, frechet_finish: three sums through one red, a barrier between them),
// hf_aligned.
#pragma once
#include <cmath>
#include <cstdint>

#include "metric_common.h"

namespace {

constexpr int kFrTile = 64;     // accumulate: output tile of a block, 4 x 4 outputs per thread
constexpr int kFrChunk = 16;    // samples staged in LDS at a time
constexpr int kFrGemm = 32;     // congruence: output tile of a block, 2 x 2 outputs per thread
constexpr int kFrGemmK = 16;
constexpr int kFrPairCols = 4;  // Jacobi: column pairs per thread below kFrWidePairs pairs, one from there on
constexpr int kFrWidePairs = 128;
constexpr double kFrEps = 2.220446049250313e-16;

__device__ __forceinline__ float frechet_f32(float v) { return v; }
__device__ __forceinline__ float frechet_f32(_Float16 v) { return (float)v; }  // exact

// grid (ceil(d/64), ceil(d/64)), 256 threads, LDS 2 x [16][64] fp32.  Thread (ty, tx) owns cov_sum rows i0 + 4 ty .. + 3,
// columns j0 + 4 tx .. + 3: it starts from the value in memory and adds the samples in ascending n (the product of two
// fp32 values is exact in fp64: the fused multiply-add rounds once, like numpy's multiply-then-add).  The blocks of
// the first tile row own sum[j0 .. j0 + 63] the same way.
template <typename T>
__global__ __launch_bounds__(256) void frechet_accumulate(double *__restrict__ sum, double *__restrict__ cov_sum,
                                                          const T *__restrict__ feats, int n, int d) {
  HF_DYN_LDS;
  float *fi = reinterpret_cast<float *>(hf_dyn_lds);
  float *fj = fi + kFrChunk * kFrTile;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * kFrTile, j0 = blockIdx.x * kFrTile;
  const bool owns_sum = blockIdx.y == 0 && tid < kFrTile && j0 + tid < d;
  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + 4 * ty + r, j = j0 + 4 * tx + c;
      acc[r][c] = (i < d && j < d) ? cov_sum[(long long)i * d + j] : 0.0;
    }
  double s = owns_sum ? sum[j0 + tid] : 0.0;
  for (int n0 = 0; n0 < n; n0 += kFrChunk) {
    const int cn = n - n0 < kFrChunk ? n - n0 : kFrChunk;
    for (int e = tid; e < kFrChunk * kFrTile; e += 256) {
      const int k = e >> 6, c = e & 63;
      const T *row = feats + (long long)(n0 + k) * d;
      fi[e] = (k < cn && i0 + c < d) ? frechet_f32(row[i0 + c]) : 0.0f;
      fj[e] = (k < cn && j0 + c < d) ? frechet_f32(row[j0 + c]) : 0.0f;
    }
    __syncthreads();
    for (int k = 0; k < cn; ++k) {
      const float4 a = *reinterpret_cast<const float4 *>(fi + k * kFrTile + 4 * ty);
      const float4 b = *reinterpret_cast<const float4 *>(fj + k * kFrTile + 4 * tx);
      const double av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] += av[r] * bv[c];
      if (owns_sum) s += (double)fj[k * kFrTile + tid];
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + 4 * ty + r, j = j0 + 4 * tx + c;
      if (i < d && j < d) cov_sum[(long long)i * d + j] = acc[r][c];
    }
  if (owns_sum) sum[j0 + tid] = s;
}

// one thread per element of cov; row 0's threads write mu as well
__global__ __launch_bounds__(256) void frechet_stats(double *__restrict__ mu, double *__restrict__ cov, const double *__restrict__ sum,
                                                     const double *__restrict__ cov_sum, double n, int d) {
#pragma clang fp contract(off)
  const long long total = (long long)d * d, stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int i = (int)(e / d), j = (int)(e - (long long)i * d);
    const double mi = sum[i] / n, mj = sum[j] / n;
    const double outer = n * (mi * mj);  // (mi * mj) first: the same bits at (i, j) and (j, i)
    cov[e] = (cov_sum[e] - outer) / (n - 1.0);
    if (i == 0) mu[j] = mj;
  }
}

// ---- Jacobi -------------------------------------------------------------------------------------------------------
// pair k (0 <= k < m / 2) of round r (0 <= r < m - 1) of the round-robin tournament of m players (m even): player m - 1
// stays, the others rotate.  Returned with p < q; q >= d marks a bye (d odd: the phantom player m - 1 = d).
__device__ __forceinline__ void jacobi_pair(int k, int round, int m, int &p, int &q) {
  const int ring = m - 1;
  int a, b;
  if (k == 0) {
    a = round;
    b = m - 1;
  } else {
    a = (round + k) % ring;
    b = (round + ring - k) % ring;
  }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// the rotation J = [[c, s], [-s, c]] that annihilates a_pq; t = s / c.  Identity for a bye and under the skip rule.
__device__ __forceinline__ bool jacobi_rotation(const double *__restrict__ A, int d, int p, int q, double &c, double &s, double &t) {
  c = 1.0;
  s = 0.0;
  t = 0.0;
  if (q >= d) return false;
  const double app = A[(long long)p * d + p], aqq = A[(long long)q * d + q], apq = A[(long long)p * d + q];
  if (fabs(apq) <= kFrEps * sqrt(fabs(app * aqq))) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // theta^2 = inf: t = 0, a_pq is dropped
  c = 1.0 / sqrt(t * t + 1.0);
  s = t * c;
  return true;
}

// one round: work item (i, jc) = row pair i, column pairs cols * jc .. + cols - 1.  A thread's column pairs are a chain of
// dependent loads (the rotation's three elements, then the block), and a round is bound by that latency: from
// kFrWidePairs pairs on cols = 1 (at d = 512: 65536 threads, every CU busy); below, a round is a few thousand threads
// either way and cols = kFrPairCols keeps their number down.  The result does not depend on cols.
__global__ __launch_bounds__(256) void jacobi_round(double *__restrict__ a_out, const double *__restrict__ a_in,
                                                    double *__restrict__ v_out, const double *__restrict__ v_in, int d, int m,
                                                    int round, int cols) {
  const int np = m / 2, njc = (np + cols - 1) / cols;
  const int item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= np * njc) return;
  const int i = item / njc, jc = item - i * njc;
  int pi, qi;
  jacobi_pair(i, round, m, pi, qi);
  double ci, si, ti;
  const bool rot_i = jacobi_rotation(a_in, d, pi, qi, ci, si, ti);
  const bool has_qi = qi < d;
  const long long rp = (long long)pi * d, rq = (long long)qi * d;
  for (int j = jc * cols; j < np && j < (jc + 1) * cols; ++j) {
    int pj, qj;
    jacobi_pair(j, round, m, pj, qj);
    const bool has_qj = qj < d;
    if (j == i) {  // the diagonal block: a_pq -> 0
      const double app = a_in[rp + pi];
      if (!has_qi) {
        a_out[rp + pi] = app;
      } else {
        const double aqq = a_in[rq + qi], apq = a_in[rp + qi];
        a_out[rp + pi] = rot_i ? app - ti * apq : app;
        a_out[rq + qi] = rot_i ? aqq + ti * apq : aqq;
        a_out[rp + qi] = rot_i ? 0.0 : apq;
        a_out[rq + pi] = rot_i ? 0.0 : apq;
      }
    }
    double cj = ci, sj = si, tj;
    if (j != i) jacobi_rotation(a_in, d, pj, qj, cj, sj, tj);
    if (j > i) {  // B' = R_i^T B R_j, stored with its mirror image
      const double bpp = a_in[rp + pj], bpq = has_qj ? a_in[rp + qj] : 0.0;
      const double bqp = has_qi ? a_in[rq + pj] : 0.0, bqq = (has_qi && has_qj) ? a_in[rq + qj] : 0.0;
      const double lpp = ci * bpp - si * bqp, lpq = ci * bpq - si * bqq;  // rows
      const double lqp = si * bpp + ci * bqp, lqq = si * bpq + ci * bqq;
      const double opp = cj * lpp - sj * lpq, opq = sj * lpp + cj * lpq;  // columns
      const double oqp = cj * lqp - sj * lqq, oqq = sj * lqp + cj * lqq;
      a_out[rp + pj] = opp;
      a_out[(long long)pj * d + pi] = opp;
      if (has_qj) {
        a_out[rp + qj] = opq;
        a_out[(long long)qj * d + pi] = opq;
      }
      if (has_qi) {
        a_out[rq + pj] = oqp;
        a_out[(long long)pj * d + qi] = oqp;
      }
      if (has_qi && has_qj) {
        a_out[rq + qj] = oqq;
        a_out[(long long)qj * d + qi] = oqq;
      }
    }
    if (v_in) {  // V' = V J on the rows pi, qi (any partition of the rows would do) and the columns pj, qj
      const double vpp = v_in[rp + pj], vpq = has_qj ? v_in[rp + qj] : 0.0;
      v_out[rp + pj] = cj * vpp - sj * vpq;
      if (has_qj) v_out[rp + qj] = sj * vpp + cj * vpq;
      if (has_qi) {
        const double vqp = v_in[rq + pj], vqq = has_qj ? v_in[rq + qj] : 0.0;
        v_out[rq + pj] = cj * vqp - sj * vqq;
        if (has_qj) v_out[rq + qj] = sj * vqp + cj * vqq;
      }
    }
  }
}

// one block: scal[0] = off-diagonal Frobenius norm, scal[1] = Frobenius norm, scal[2] = pairs above the skip threshold
__global__ __launch_bounds__(256) void jacobi_norms(double *__restrict__ scal, const double *__restrict__ a, int d) {
  HF_DYN_LDS;
  double *red = reinterpret_cast<double *>(hf_dyn_lds);
  double off = 0.0, diag = 0.0, above = 0.0;
  const long long total = (long long)d * d;
  for (long long e = threadIdx.x; e < total; e += 256) {
    const int r = (int)(e / d), c = (int)(e - (long long)r * d);
    if (r > c) continue;
    const double v = a[e];
    if (r == c) {
      diag += v * v;
    } else {
      off += v * v;
      if (fabs(v) > kFrEps * sqrt(fabs(a[(long long)r * d + r] * a[(long long)c * d + c]))) above += 1.0;
    }
  }
  __syncthreads();  // as before every sum: red[0] of the one before may still be read
  off = hf_block_sum_f64(off, red);
  __syncthreads();
  diag = hf_block_sum_f64(diag, red);
  __syncthreads();
  above = hf_block_sum_f64(above, red);
  if (threadIdx.x == 0) {
    scal[0] = sqrt(2.0 * off);
    scal[1] = sqrt(2.0 * off + diag);
    scal[2] = above;
  }
}

// a0 = A, v0 = I
__global__ __launch_bounds__(256) void jacobi_init(double *__restrict__ a0, double *__restrict__ v0, const double *__restrict__ a, int d) {
  const long long total = (long long)d * d, stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    a0[e] = a[e];
    if (v0) v0[e] = (e / d == e % d) ? 1.0 : 0.0;
  }
}

// w = diag(A_final), V = V_final
__global__ __launch_bounds__(256) void jacobi_extract(double *__restrict__ w, double *__restrict__ v, const double *__restrict__ a,
                                                      const double *__restrict__ v_fin, int d) {
  const long long total = (long long)d * d, stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    if (e < d) w[e] = a[e * d + e];
    if (v) v[e] = v_fin[e];
  }
}

// ---- congruence ---------------------------------------------------------------------------------------------------
// C[i][j] = rs_i cs_j sum_k X(i, k) Y[k][j], X(i, k) = XT ? X[k][i] : X[i][k]; rs / cs = sqrt(max(w, 0)) or 1 (NULL).
// grid (ceil(d/32), ceil(d/32)), 256 threads, 2 x 2 outputs per thread, k ascending.
template <bool XT>
__global__ __launch_bounds__(256) void frechet_gemm(double *__restrict__ c_out, const double *__restrict__ x, const double *__restrict__ y,
                                                    const double *__restrict__ w_rows, const double *__restrict__ w_cols, int d) {
  HF_DYN_LDS;
  double *xs = reinterpret_cast<double *>(hf_dyn_lds);  // [k][i]
  double *ys = xs + kFrGemmK * kFrGemm;                 // [k][j]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * kFrGemm, j0 = blockIdx.x * kFrGemm;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int k0 = 0; k0 < d; k0 += kFrGemmK) {
    for (int e = tid; e < kFrGemmK * kFrGemm; e += 256) {
      const int kx = XT ? e >> 5 : e & 15, ix = XT ? e & 31 : e >> 4;
      const bool okx = k0 + kx < d && i0 + ix < d;
      xs[kx * kFrGemm + ix] = okx ? (XT ? x[(long long)(k0 + kx) * d + i0 + ix] : x[(long long)(i0 + ix) * d + k0 + kx]) : 0.0;
      const int ky = e >> 5, jy = e & 31;
      ys[e] = (k0 + ky < d && j0 + jy < d) ? y[(long long)(k0 + ky) * d + j0 + jy] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kFrGemmK; ++k) {
      const double a0 = xs[k * kFrGemm + 2 * ty], a1 = xs[k * kFrGemm + 2 * ty + 1];
      const double b0 = ys[k * kFrGemm + 2 * tx], b1 = ys[k * kFrGemm + 2 * tx + 1];
      acc[0][0] += a0 * b0;
      acc[0][1] += a0 * b1;
      acc[1][0] += a1 * b0;
      acc[1][1] += a1 * b1;
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int i = i0 + 2 * ty + r, j = j0 + 2 * tx + c;
      if (i < d && j < d) {
        double v = acc[r][c];
        if (w_rows) v *= sqrt(fmax(w_rows[i], 0.0));
        if (w_cols) v *= sqrt(fmax(w_cols[j], 0.0));
        c_out[(long long)i * d + j] = v;
      }
    }
}

__global__ __launch_bounds__(256) void frechet_symmetrise(double *__restrict__ out, const double *__restrict__ x, int d) {
  const long long total = (long long)d * d, stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long i = e / d, j = e - i * d;
    out[e] = 0.5 * (x[e] + x[j * d + i]);
  }
}

// one block
__global__ __launch_bounds__(256) void frechet_finish(double *__restrict__ out, const double *__restrict__ mu1, const double *__restrict__ mu2,
                                                      const double *__restrict__ s1, const double *__restrict__ s2,
                                                      const double *__restrict__ ev, int d) {
  HF_DYN_LDS;
  double *red = reinterpret_cast<double *>(hf_dyn_lds);
  double dist = 0.0, trace = 0.0, roots = 0.0;
  for (int i = threadIdx.x; i < d; i += 256) {
    const double dm = mu1[i] - mu2[i];
    dist += dm * dm;
    trace += s1[(long long)i * d + i] + s2[(long long)i * d + i];
    roots += sqrt(fmax(ev[i], 0.0));
  }
  __syncthreads();  // as before every sum: red[0] of the one before may still be read
  dist = hf_block_sum_f64(dist, red);
  __syncthreads();
  trace = hf_block_sum_f64(trace, red);
  __syncthreads();
  roots = hf_block_sum_f64(roots, red);
  if (threadIdx.x == 0) out[0] = dist + trace - 2.0 * roots;
}

inline int frechet_grid(long long n) {
  const long long g = (n + 255) / 256;
  return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

// the three doubles of jacobi_norms on the host: the one synchronisation of a sweep
inline int jacobi_read_norms(double *host, const double *dev, hipStream_t st) {
#if defined(__HIP__)
  if (hipMemcpyAsync(host, dev, 3 * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return HF_E_LAUNCH;
#else  // the CPU interpreter build: one address space, launches run to completion
  (void)st;
  for (int k = 0; k < 3; ++k) host[k] = dev[k];
#endif
  return HF_OK;
}

template <typename T>
int frechet_accumulate_launch(double *sum, double *cov_sum, const T *feats, int n, int d, void *stream) {
  if (!hf_aligned(sum, 8) || !hf_aligned(cov_sum, 8) || !hf_aligned(feats, sizeof(T)) || n <= 0 || d <= 0 ||
      d > 65535 * kFrTile)
    return HF_E_INVALID;
  const int tiles = hf_cdiv(d, kFrTile);
  hipLaunchKernelGGL(frechet_accumulate<T>, dim3(tiles, tiles), dim3(256), (size_t)2 * kFrChunk * kFrTile * sizeof(float),
                     (hipStream_t)stream, sum, cov_sum, feats, n, d);
  return hf_launch_status();
}

}  // namespace

extern "C" int hf_frechet_accumulate_f64(double *sum, double *cov_sum, const float *feats, int n, int d, void *stream) {
  return frechet_accumulate_launch<float>(sum, cov_sum, feats, n, d, stream);
}

extern "C" int hf_frechet_accumulate_f16_f64(double *sum, double *cov_sum, const void *feats, int n, int d, void *stream) {
  return frechet_accumulate_launch<_Float16>(sum, cov_sum, static_cast<const _Float16 *>(feats), n, d, stream);
}

extern "C" int hf_frechet_stats_f64(double *mu, double *cov, const double *sum, const double *cov_sum, long long n, int d, void *stream) {
  if (!hf_aligned(mu, 8) || !hf_aligned(cov, 8) || !hf_aligned(sum, 8) || !hf_aligned(cov_sum, 8) || n < 2 || d <= 0)
    return HF_E_INVALID;
  hipLaunchKernelGGL(frechet_stats, dim3(frechet_grid((long long)d * d)), dim3(256), 0, (hipStream_t)stream, mu, cov, sum, cov_sum,
                     (double)n, d);
  return hf_launch_status();
}

extern "C" long long hf_sym_eig_jacobi_work_doubles(int d, int want_vectors) {
  return d <= 0 ? 0 : (long long)(want_vectors ? 4 : 2) * d * d + 4;
}

extern "C" int hf_sym_eig_jacobi_f64(double *w, double *v, const double *a, double *work, int d, int max_sweeps, int *sweeps,
                                     double *off_norm, void *stream) {
  if (!hf_aligned(w, 8) || (v && !hf_aligned(v, 8)) || !hf_aligned(a, 8) || !hf_aligned(work, 8) || d <= 0 ||
      d > 16384 || max_sweeps < 1 || !sweeps || !off_norm)
    return HF_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  const long long dd = (long long)d * d;
  double *ab[2] = {work, work + dd};
  double *vb[2] = {v ? work + 2 * dd : nullptr, v ? work + 3 * dd : nullptr};
  double *scal = work + (v ? 4 : 2) * dd;
  const int m = (d + 1) & ~1, rounds = m - 1, np = m / 2;
  const int cols = np >= kFrWidePairs ? 1 : kFrPairCols;
  const int items = np * ((np + cols - 1) / cols);
  const dim3 flat(frechet_grid(dd));
  hipLaunchKernelGGL(jacobi_init, flat, dim3(256), 0, st, ab[0], vb[0], a, d);
  int cur = 0, done = 0, status = HF_OK;
  bool converged = false;
  double host[3] = {0.0, 0.0, 0.0};
  for (;;) {
    hipLaunchKernelGGL(jacobi_norms, dim3(1), dim3(256), 256 * sizeof(double), st, scal, ab[cur], d);
    if ((status = hf_launch_status()) != HF_OK || (status = jacobi_read_norms(host, scal, st)) != HF_OK) return status;
    converged = host[2] == 0.0 || host[0] <= kFrEps * host[1];
    if (converged || done == max_sweeps) break;
    for (int r = 0; r < rounds; ++r) {
      hipLaunchKernelGGL(jacobi_round, dim3(hf_cdiv(items, 256)), dim3(256), 0, st, ab[cur ^ 1], ab[cur], vb[cur ^ 1], vb[cur], d, m, r, cols);
      cur ^= 1;
    }
    ++done;
  }
  hipLaunchKernelGGL(jacobi_extract, flat, dim3(256), 0, st, w, v, ab[cur], vb[cur], d);
  *sweeps = converged ? done : -1;
  *off_norm = host[0];
  return hf_launch_status();
}

extern "C" int hf_frechet_congruence_f64(double *m_out, const double *w, const double *v, const double *s2, double *work, int d,
                                         void *stream) {
  if (!hf_aligned(m_out, 8) || !hf_aligned(w, 8) || !hf_aligned(v, 8) || !hf_aligned(s2, 8) ||
      !hf_aligned(work, 8) || d <= 0 || d > 65535 * kFrGemm)
    return HF_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  double *t = work, *u = work + (long long)d * d;
  const int tiles = hf_cdiv(d, kFrGemm);
  const size_t lds = (size_t)2 * kFrGemmK * kFrGemm * sizeof(double);
  hipLaunchKernelGGL(frechet_gemm<true>, dim3(tiles, tiles), dim3(256), lds, st, t, v, s2, w, (const double *)nullptr, d);   // T = B S2
  hipLaunchKernelGGL(frechet_gemm<false>, dim3(tiles, tiles), dim3(256), lds, st, u, t, v, (const double *)nullptr, w, d);  // U = T B^T
  hipLaunchKernelGGL(frechet_symmetrise, dim3(frechet_grid((long long)d * d)), dim3(256), 0, st, m_out, u, d);
  return hf_launch_status();
}

extern "C" int hf_frechet_finish_f64(double *out, const double *mu1, const double *mu2, const double *s1, const double *s2,
                                     const double *ev, int d, void *stream) {
  if (!hf_aligned(out, 8) || !hf_aligned(mu1, 8) || !hf_aligned(mu2, 8) || !hf_aligned(s1, 8) ||
      !hf_aligned(s2, 8) || !hf_aligned(ev, 8) || d <= 0)
    return HF_E_INVALID;
  hipLaunchKernelGGL(frechet_finish, dim3(1), dim3(256), 256 * sizeof(double), (hipStream_t)stream, out, mu1, mu2, s1, s2, ev, d);
  return hf_launch_status();
}
