// conv_rect.h - convolution over an arbitrary rectangle of taps between channel slices of NCHW tensors: the layers of the FID
// Inception-v3 (torch-fidelity's FeatureExtractorInceptionV3: 1x1, 1x3, 3x1, 1x7, 7x1, 5x5 and 3x3 taps, stride 1 and 2, valid
// and padded, output widths that are no multiple of 64, branch results concatenated along channels).  Included by gemm_h.hip.
//
//   y[n, oc0+co, oy, ox] = act( out_scale[co] * sum_{ky,kx,ci} W[co,ci,ky,kx] * x[n, xc0+ci, oy*s-pt+ky, ox*s-pl+kx] + bias[co] )
//
// zero outside the plane.  Input and output are channel slices (xc0 of x_ctotal, oc0 of o_ctotal): the branches of a block
// write the concatenated tensor directly, and several consumers read slices of one merged 1x1 result.
//
// conv_rect_h (nterms 3 / 1): gemm1x1_h's structure with a tap loop around it.  One block = 64 output channels x 128 FLAT
// output pixels (n, oy, ox) -> n*oh*ow + oy*ow + ox, so a tile runs across image boundaries and batch 128 of 8^2 planes fills
// tiles; 4 waves = 2 (channels) x 2 (pixels), each 1 x 2 MFMA tiles (v_mfma_f32_32x32x16_f16).  K loop over
// (tap, 32-channel stage), taps in (ky, kx) order outside, channels inside, double-buffered in LDS: weights by LDS-DMA from
// [tap][cinp/16][2][coutp][8 halves] hi (+ lo) (cinp = cin rounded up to 32, coutp = cout to 64, the padding zero;
// pre-scaled by 2^k, un-scaled in the epilogue), activations through registers with a per-(pixel, tap) validity mask
// (channels >= cin read as zero), saturating split, one 16-byte LDS write per part.  K is never split and its order is
// fixed: an output's bits depend on its own image alone, whatever the batch and wherever the image stands in it.
//
// conv_rect_f32 (nterms 0): the readable restatement - one lane per output, fmaf in ascending (ky, kx, ci).
#pragma once

namespace {

struct RectParams {
  float *out;
  const float *x, *wf, *d, *bias;
  int batch, cin, cout, h, w, kh, kw, stride, pt, pl, oh, ow, xc0, xct, oc0, oct, relu;
  int cinp, coutp;
  long long total;  // flat output pixels: batch * oh * ow
};

// __launch_bounds__(256, 2): the LEAST occupancy the register allocator has to leave room for (gemm1x1_h's bound); the kernel
// needs 92 (f16x3) / 84 (f16) VGPRs, so what limits a CU is LDS: 48 KiB of stage buffers with f16x3 operands - three blocks per
// CU - and 24 KiB with f16 operands.
template <int NTERMS>
__global__ __launch_bounds__(256, 2) void conv_rect_h(const RectParams P, const _Float16 *__restrict__ wth,
                                                      const _Float16 *__restrict__ wtl) {
  using L = GemmLayout<NTERMS, 2, 2>;
  constexpr int PG = 2, NW = 4, NT = 256, CT = L::CT, PT = L::PT;
  constexpr int NPART = L::NPART, W_UNITS = L::W_UNITS, X_UNITS = L::X_UNITS, BUF_UNITS = L::BUF_UNITS;
  constexpr int OFF_WL = L::OFF_WL, OFF_XH = L::OFF_XH, OFF_XL = L::OFF_XL;
  constexpr int XE = X_UNITS / NT;                // staging items per thread and stage: kblocks kb0 and kb0 + 2 of ONE pixel
  constexpr int N_WPIECE = NPART * W_UNITS / 64;  // 1 KiB DMA pieces per stage
  constexpr int ND = N_WPIECE / NW;
  static_assert(CT == 64 && PT == 128 && XE == 2 && NT % PT == 0 && N_WPIECE % NW == 0, "the tile this kernel is written for");

  HF_DYN_LDS;
  half8 *lds = reinterpret_cast<half8 *>(hf_dyn_lds);  // [2][BUF_UNITS]
  const int taps = P.kh * P.kw, cst = P.cinp / KS;
  const long long wn = (long long)taps * P.cinp * P.coutp;
  const float w_unscale = *reinterpret_cast<const float *>(wth + wn);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wave_co = (wave >> 1) * 32, wave_pg = (wave & 1) * PG;
  const int co0 = (int)blockIdx.y * CT;
  const long long p0 = (long long)blockIdx.x * PT;
  const int oplane = P.oh * P.ow;
  const long long iplane = (long long)P.h * P.w;

  // the thread's pixel (stage invariant): its two items are the 8-channel blocks kb0 and kb0 + 2 of it
  const int px = tid % PT, kb0 = tid / PT;
  const long long p = p0 + px;
  const bool p_ok = p < P.total;
  int iy0 = 0, ix0 = 0;
  long long e_base = 0;  // element of (n, xc0, iy0, ix0); may lie outside the plane (masked per tap)
  if (p_ok) {
    const long long n = p / oplane;
    const int rem = (int)(p - n * oplane);
    const int oy = rem / P.ow, ox = rem - oy * P.ow;
    iy0 = oy * P.stride - P.pt;
    ix0 = ox * P.stride - P.pl;
    e_base = (n * P.xct + P.xc0) * iplane + (long long)iy0 * P.w + ix0;
  }

  const int nstages = taps * cst;
  const unsigned lds_addr0 = hf_lds_addr(lds);
  auto dma_w = [&](int stage, int bufsel) {
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const int pc = wave + j * NW;  // piece: (part, 16-channel chunk of the stage, kgroup)
      const int part = pc / (W_UNITS / 64), row = pc % (W_UNITS / 64);
      const _Float16 *src = (part ? wtl : wth) + ((long long)(stage * (KS / KH) * 2 + row) * P.coutp + co0) * 8;
      hf_glds16_raw_s(src, (unsigned)lane * 16u, lds_addr0 + (unsigned)(bufsel * BUF_UNITS + part * W_UNITS + row * 64) * 16u);
    }
  };
  float xr[XE][8];
  auto load_x = [&](int stage) {
    const int tap = stage / cst, cs = stage - tap * cst;
    const int ky = tap / P.kw, kx = tap - ky * P.kw;
    const bool inside = p_ok && (unsigned)(iy0 + ky) < (unsigned)P.h && (unsigned)(ix0 + kx) < (unsigned)P.w;
    const float *src = P.x + (inside ? e_base + (long long)ky * P.w + kx : 0);
#pragma unroll
    for (int e = 0; e < XE; ++e) {
      const int c0 = cs * KS + (kb0 + 2 * e) * 8;
#pragma unroll
      for (int k = 0; k < 8; ++k) xr[e][k] = (inside && c0 + k < P.cin) ? src[(long long)(c0 + k) * iplane] : 0.0f;
    }
  };
  auto convert_x = [&](half8 *buf) {
    bool ovf = false;
#pragma unroll
    for (int e = 0; e < XE; ++e) {
      const int i = tid + e * NT;  // = (kb0 + 2 e) * PT + px
      half8 hi, lo;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        _Float16 hv, lv;
        hf_split_f16(xr[e][k], hv, lv, ovf);
        hi[k] = hv;
        lo[k] = lv;
      }
      buf[OFF_XH + i] = hi;
      if (NTERMS == 3) buf[OFF_XL + i] = lo;
    }
    hf_note_overflow(ovf);
  };

  f32x16 acc[PG];
#pragma unroll
  for (int g = 0; g < PG; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = 0.0f;

  dma_w(0, 0);
  load_x(0);
  convert_x(lds);
  hf_barrier_keep_young<0>();
  for (int s = 0; s < nstages; ++s) {
    const int cb = s & 1;
    half8 *buf = lds + cb * BUF_UNITS, *nbuf = lds + (cb ^ 1) * BUF_UNITS;
    const bool more = s + 1 < nstages;
    if (more) {
      dma_w(s + 1, cb ^ 1);
      load_x(s + 1);
    }
#pragma unroll
    for (int cs = 0; cs < KS / KH; ++cs) {
      const half8 ah = buf[(cs * 2 + lh) * CT + wave_co + li];
      half8 al;
      if (NTERMS == 3) al = buf[OFF_WL + (cs * 2 + lh) * CT + wave_co + li];
#pragma unroll
      for (int g = 0; g < PG; ++g) {
        const int u = (cs * 2 + lh) * PT + (wave_pg + g) * 32 + li;
        const half8 bh = buf[OFF_XH + u];
        HF_MFMA_F16X3(NTERMS, 1, 1, &acc[g], &ah, &al, &bh, &buf[OFF_XL + u]);
      }
    }
    if (more) convert_x(nbuf);
    hf_barrier_keep_young<0>();
  }

  // epilogue: the pre-scale comes out (exact, a power of two), then one fma and the activation; only true channels are stored
  const long long ostride = (long long)oplane;
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    const long long q = p0 + (wave_pg + g) * 32 + li;
    if (q >= P.total) continue;
    const long long n = q / oplane;
    const long long rem = q - n * oplane;
    float *ob = P.out + (n * P.oct + P.oc0) * ostride + rem;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wave_co + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (co >= P.cout) continue;
      float v = fmaf(acc[g][r] * w_unscale, P.d ? P.d[co] : 1.0f, P.bias ? P.bias[co] : 0.0f);
      if (P.relu) v = v > 0.0f ? v : 0.0f;
      ob[(long long)co * ostride] = v;
    }
  }
}

// one lane per output element (n, co, oy, ox); weights in torch's layout [cout][cin][kh][kw]
__global__ __launch_bounds__(256) void conv_rect_f32(const RectParams P) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= P.total * P.cout) return;
  const int ox = (int)(e % P.ow);
  long long r = e / P.ow;
  const int oy = (int)(r % P.oh);
  r /= P.oh;
  const int co = (int)(r % P.cout);
  const long long n = r / P.cout;
  const long long iplane = (long long)P.h * P.w;
  const int taps = P.kh * P.kw;
  const float *xb = P.x + (n * P.xct + P.xc0) * iplane;
  const float *wb = P.wf + (long long)co * P.cin * taps;
  float acc = 0.0f;
  for (int ky = 0; ky < P.kh; ++ky) {
    const int iy = oy * P.stride - P.pt + ky;
    if (iy < 0 || iy >= P.h) continue;
    for (int kx = 0; kx < P.kw; ++kx) {
      const int ix = ox * P.stride - P.pl + kx;
      if (ix < 0 || ix >= P.w) continue;
      const float *xs = xb + (long long)iy * P.w + ix, *ws = wb + ky * P.kw + kx;
      for (int ci = 0; ci < P.cin; ++ci) acc = fmaf(ws[(long long)ci * taps], xs[(long long)ci * iplane], acc);
    }
  }
  float v = fmaf(acc, P.d ? P.d[co] : 1.0f, P.bias ? P.bias[co] : 0.0f);
  if (P.relu) v = v > 0.0f ? v : 0.0f;
  P.out[((n * P.oct + P.oc0 + co) * P.oh + oy) * (long long)P.ow + ox] = v;
}

}  // namespace

extern "C" int hf_conv2d_rect_f16_f32(float *out, const float *x, const float *weight, const void *wt_hi, const void *wt_lo,
                                      int nterms, const float *out_scale, const float *bias, int act, int batch, int cin, int cout,
                                      int h, int w, int kh, int kw, int stride, int pad_top, int pad_left, int out_h, int out_w,
                                      int xc0, int x_ctotal, int oc0, int o_ctotal, void *stream) {
  if (!out || !x || batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || kh < 1 || kh > 7 || kw < 1 || kw > 7 ||
      (stride != 1 && stride != 2) || pad_top < 0 || pad_top >= kh || pad_left < 0 || pad_left >= kw || out_h <= 0 || out_w <= 0 ||
      (act != 0 && act != 1) || xc0 < 0 || oc0 < 0 || (long long)xc0 + cin > x_ctotal || (long long)oc0 + cout > o_ctotal ||
      (nterms != 0 && nterms != 1 && nterms != 3) || (nterms == 0 && !weight) || (nterms != 0 && !wt_hi) || (nterms == 3 && !wt_lo))
    return HF_E_INVALID;
  // the last output's first tap lies inside the plane or its padding: an output plane larger than the input gives is refused
  if ((long long)(out_h - 1) * stride - pad_top >= h || (long long)(out_w - 1) * stride - pad_left >= w) return HF_E_INVALID;
  RectParams P{};
  P.out = out; P.x = x; P.wf = weight; P.d = out_scale; P.bias = bias;
  P.batch = batch; P.cin = cin; P.cout = cout; P.h = h; P.w = w; P.kh = kh; P.kw = kw; P.stride = stride;
  P.pt = pad_top; P.pl = pad_left; P.oh = out_h; P.ow = out_w; P.xc0 = xc0; P.xct = x_ctotal; P.oc0 = oc0; P.oct = o_ctotal;
  P.relu = act;
  P.cinp = (cin + KS - 1) / KS * KS;
  P.coutp = (cout + 63) / 64 * 64;
  P.total = (long long)batch * out_h * out_w;
  if ((long long)out_h * out_w > 0x7fffffffLL || (long long)h * w > 0x7fffffffLL) return HF_E_INVALID;
  if (nterms == 0) {
    const long long blocks = (P.total * cout + 255) / 256;
    if (blocks > 0x7fffffffLL) return HF_E_INVALID;
    hipLaunchKernelGGL(conv_rect_f32, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
    return hf_launch_status();
  }
  const long long tiles = (P.total + 127) / 128;
  if (tiles > 0x7fffffffLL || P.coutp / 64 > 65535) return HF_E_INVALID;
  const dim3 grid((unsigned)tiles, (unsigned)(P.coutp / 64));
  const _Float16 *hi = static_cast<const _Float16 *>(wt_hi), *lo = static_cast<const _Float16 *>(wt_lo);
  const size_t lds3 = GemmLayout<3, 2, 2>::lds_bytes, lds1 = GemmLayout<1, 2, 2>::lds_bytes;
  if (nterms == 3)
    hipLaunchKernelGGL((conv_rect_h<3>), grid, dim3(256), lds3, (hipStream_t)stream, P, hi, lo);
  else
    hipLaunchKernelGGL((conv_rect_h<1>), grid, dim3(256), lds1, (hipStream_t)stream, P, hi, lo);
  return hf_launch_status();
}
