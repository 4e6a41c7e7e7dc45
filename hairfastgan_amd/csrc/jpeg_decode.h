// jpeg_decode.h - a baseline JPEG decoder on the device, the counterpart of jpeg.h: the entropy-coded scans of a group of
// files of one geometry (bytes in device memory, the tables of each file's header beside them) become uint8 images
// [B,H,W,1|3] and, optionally, float images [B,1|3,H,W] = byte / 255 - the pixels libjpeg-turbo (Pillow's
// Image.open(f).convert("RGB")) returns, byte for byte.  Included by encoder_ops.hip.  DESIGN.md 4.23.
//
//   hf_jpeg_decode_workspace_bytes   host-only shape arithmetic
//   hf_jpeg_decode_u8                four launches (six with restart markers), no allocation, no synchronisation
//
// The host parses the marker segments from SOI to SOS and never looks at the scan.  Per file it hands over kJdTableBytes:
// three quantisation tables (by component, natural order, uint16) and six Huffman tables (DC then AC, by component) as the
// DHT segment states them: 16 counts and up to 256 symbols.
//
// jpegd_clear         zeroes the coefficients (the entropy pass writes the non-zero ones only) and the status words, sets
//                     every interval boundary to the end of the scan.
// jpegd_marker_count / jpegd_marker_place (only with a restart interval): the markers of the scan in 16 KiB chunks - a
//                     count per chunk, then each chunk sums the counts before it and writes the positions of its markers;
//                     marker j must be RST(j mod 8), the one behind the last interval ends the scan.
// jpegd_entropy       (intervals x images, 256 threads) one restart interval - the whole scan without DRI - in windows:
//                     the window's raw bytes are unstuffed (FF 00 -> FF, a marker cuts the data) into LDS behind the bytes
//                     carried over from the window before; the window is cut into subsequences of sub_bytes bytes, one lane
//                     each.  Pass 0 decodes every subsequence from the guess "a block starts here" and records the state
//                     (bit position, block of the MCU, zig-zag index) in which it leaves the subsequence and the blocks it
//                     completed; later passes re-enter a subsequence whose predecessor's exit state changed, until none
//                     changes (lane 0 enters from the true state, so at most as many passes as subsequences).  A scan over
//                     the block counts, and a last pass writes DC differences and AC coefficients (int16, zig-zag order,
//                     scan order).  The last 8 bytes of a window are not entered but carried, so a symbol never needs
//                     bytes the window does not hold.  At the end the DC differences of the interval are summed per
//                     component (a workgroup scan over MCUs).
// jpegd_blocks        one thread per 8x8 block: dequantisation, jidctint.c's two passes in int32 registers, + 128 saturated
//                     to a byte (what libjpeg-turbo's SIMD IDCT stores), to the component's plane.
// jpegd_pixels        one thread per pixel: libjpeg's fancy chroma upsampling (h2v1 / h2v2 triangle filters over the
//                     component's downsampled extent, plain replication where that is 1 or 2 samples wide), jdcolor.c's
//                     fixed-point YCbCr -> RGB, the pixel and, if asked for, its float planes.
//
// Safety: nothing read from the scan becomes an index, a count or an address unchecked.  Scan reads are bounded by the scan's
// length (itself clamped to the buffer), table indices are masked, a coefficient is written only for a block index below the
// interval's block count and a zig-zag index below 64, every loop is bounded by the shape or the scan length.  A code that is
// not in the table, a block of more than 64 coefficients, a DC size above 11, a wrong or missing marker and a scan that ends
// early set status[2 b] (the largest code wins); status[2 b + 1] is the largest number of synchronisation passes of a window.
// From jpeg.h: kJpegNatural, jpeg_dct_odd, jpeg_mcus, jpeg_block_component / jpeg_luma_block_at, jpeg_coef; through it from
// codec_common.h: CodecVec16, codec_scan (every scan below), codec_sum_before (jpegd_marker_place).
#pragma once
#include <cstdint>

#include "hf_common.h"
#include "jpeg.h"

namespace {

constexpr int kJdThreads = kJpegThreads;
constexpr int kJdTableBytes = 2048;  // 3 x 64 uint16, 6 x (16 + 256) bytes, padded
constexpr int kJdHuffOffset = 384;
constexpr int kJdSubMin = 4, kJdSubMax = 64, kJdSubDefault = 16;
constexpr int kJdChunk = 16384;      // bytes of the scan per workgroup of the marker kernels
constexpr uint32_t kJdDead = 0xFFFFFFFFu;
enum { JD_OK = 0, JD_TRUNCATED = 1, JD_MARKER = 2, JD_COEFS = 3, JD_CODE = 4, JD_DC = 5 };

struct JdGeom : JpegMcus {
  int ri, n_int;  // ri: MCUs per interval (all of them without DRI)
  long long total_mcus, total_blocks, yw, yh, cw, ch;
  long long coef_bytes, plane_bytes, bounds_bytes, counts_bytes;
  int nchunks;
};

// the scan of file b inside the buffer: offsets are clamped, so a wrong table of offsets reads wrong bytes, never outside
__device__ __forceinline__ void jd_scan_range(const long long *offsets, int b, long long scans_bytes, long long &start, uint32_t &len) {
  long long s = offsets[b], e = offsets[b + 1];
  s = s < 0 ? 0 : (s > scans_bytes ? scans_bytes : s);
  e = e < s ? s : (e > scans_bytes ? scans_bytes : e);
  start = s;
  len = (uint32_t)((e - s) > 0x7fffffffLL ? 0x7fffffffLL : (e - s));
}

__global__ __launch_bounds__(kJdThreads) void jpegd_clear(CodecVec16 *__restrict__ coefs, long long n16, int *__restrict__ status,
                                                          uint32_t *__restrict__ bounds, const long long *__restrict__ offsets,
                                                          long long scans_bytes, int batch, int n_int) {
  const long long stride = (long long)gridDim.x * kJdThreads;
  const long long t0 = (long long)blockIdx.x * kJdThreads + threadIdx.x;
  for (long long i = t0; i < n16; i += stride) coefs[i] = CodecVec16{0u, 0u, 0u, 0u};
  for (long long i = t0; i < 2ll * batch; i += stride) status[i] = 0;
  for (long long i = t0; i < (long long)batch * n_int; i += stride) {
    long long s;
    uint32_t len;
    jd_scan_range(offsets, (int)(i / n_int), scans_bytes, s, len);
    bounds[i] = len;
  }
}

// whether a marker stands at byte p of the scan: FF followed by neither 00 (a stuffed FF) nor FF (a fill byte)
__device__ __forceinline__ bool jd_marker_at(const uint8_t *g, uint32_t p, uint32_t len) {
  return g[p] == 0xFFu && p + 1u < len && g[p + 1u] != 0u && g[p + 1u] != 0xFFu;
}

__global__ __launch_bounds__(kJdThreads) void jpegd_marker_count(uint32_t *__restrict__ counts, const uint8_t *__restrict__ scans,
                                                                 const long long *__restrict__ offsets, long long scans_bytes) {
  HF_DYN_LDS;
  uint32_t *sum = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  const int tid = (int)threadIdx.x, c = (int)blockIdx.x, b = (int)blockIdx.y;
  long long start;
  uint32_t len;
  jd_scan_range(offsets, b, scans_bytes, start, len);
  const uint8_t *g = scans + start;
  if (tid == 0) sum[0] = 0;
  __syncthreads();
  const uint64_t a = (uint64_t)c * kJdChunk + (uint64_t)tid * (kJdChunk / kJdThreads);
  uint32_t n = 0;
  for (int i = 0; i < kJdChunk / kJdThreads; ++i)
    if (a + i < len && jd_marker_at(g, (uint32_t)(a + i), len)) ++n;
  if (n) atomicAdd(&sum[0], n);
  __syncthreads();
  if (tid == 0) counts[(long long)b * gridDim.x + c] = sum[0];
}

// Dynamic LDS: sum [4] | scan [2 * threads]
__global__ __launch_bounds__(kJdThreads) void jpegd_marker_place(uint32_t *__restrict__ bounds, int *__restrict__ status,
                                                                 const uint32_t *__restrict__ counts, const uint8_t *__restrict__ scans,
                                                                 const long long *__restrict__ offsets, long long scans_bytes, int n_int) {
  HF_DYN_LDS;
  uint32_t *sum = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  uint32_t *scan = sum + 4;
  const int tid = (int)threadIdx.x, c = (int)blockIdx.x, b = (int)blockIdx.y;
  long long start;
  uint32_t len;
  jd_scan_range(offsets, b, scans_bytes, start, len);
  const uint8_t *g = scans + start;
  codec_sum_before<kJdThreads>(sum, c, tid, [&](int i) { return counts[(long long)b * gridDim.x + i]; });
  const uint64_t a = (uint64_t)c * kJdChunk + (uint64_t)tid * (kJdChunk / kJdThreads);
  uint32_t n = 0;
  for (int i = 0; i < kJdChunk / kJdThreads; ++i)
    if (a + i < len && jd_marker_at(g, (uint32_t)(a + i), len)) ++n;
  uint32_t total;
  const uint32_t incl = codec_scan<kJdThreads>(scan, tid, n, total);  // its barriers also publish sum[0]: codec_sum_before leaves that to its caller
  uint64_t j = (uint64_t)sum[0] + incl - n;
  if (n == 0) return;
  for (int i = 0; i < kJdChunk / kJdThreads; ++i) {
    if (!(a + i < len && jd_marker_at(g, (uint32_t)(a + i), len))) continue;
    if (j < (uint64_t)n_int) {
      bounds[(long long)b * n_int + (long long)j] = (uint32_t)(a + i);
      if (j + 1 < (uint64_t)n_int && g[a + i + 1] != (uint8_t)(0xD0u + (uint32_t)(j & 7u))) atomicMax(reinterpret_cast<unsigned int *>(status + 2 * b), (unsigned int)JD_MARKER);
    }
    ++j;
  }
}

// the Huffman tables of a file in LDS
struct JdTabs {
  const uint16_t *look;   // [6][256] length << 8 | symbol of the codes of at most 8 bits, 0 for longer ones
  const int *maxcode;     // [6][17] the largest code of each length, -1 if there is none
  const int *valoff;      // [6][17] index of the length's first symbol minus its first code
  const uint8_t *vals;    // [6][256]
};

// the 32 bits at bit position pos of the unstuffed bytes (5 bytes are read: the buffer is zero behind its end)
__device__ __forceinline__ uint32_t jd_peek(const uint8_t *buf, uint32_t pos) {
  const uint32_t i = pos >> 3;
  const uint64_t v = (uint64_t)buf[i] << 32 | (uint64_t)buf[i + 1] << 24 | (uint64_t)buf[i + 2] << 16 | (uint64_t)buf[i + 3] << 8 | (uint64_t)buf[i + 4];
  return (uint32_t)((v << (pos & 7u)) >> 8);
}

// One subsequence: symbols are decoded while the position lies before end_bits.  pos / kz (block of the MCU << 8 | zig-zag
// index, kJdDead after an error) are the entry state and become the exit state; returns the blocks completed.  WRITE: the
// coefficients go to `coefs` (the interval's blocks), blocks from index blk on; nothing is decoded from block `expected` on,
// an error below it goes to *status, and the position behind block expected - 1 goes to *endpos.
template <bool WRITE>
__device__ __forceinline__ uint32_t jd_decode_sub(const uint8_t *buf, uint32_t &pos, uint32_t &kz, uint32_t end_bits, const JdTabs &T, int nb,
                                                  int nl, int16_t *coefs, long long blk, long long expected, int *status,
                                                  uint32_t *endpos) {
  uint32_t done = 0;
  if (kz == kJdDead) return 0;
  int k = (int)(kz >> 8), z = (int)(kz & 255u);
  int err = 0;
  while (pos < end_bits) {
    if (WRITE && blk >= expected) break;
    const int comp = k < nl ? 0 : k - nl + 1;  // jpeg_block_component written out: called here, the compiler schedules
    const int t = (z == 0 ? 0 : 3) + comp;     // jpegd_entropy differently; so its machine code stays what it was
    const uint32_t v = jd_peek(buf, pos);
    uint32_t e = T.look[t * 256 + (v >> 24)];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (e == 0) {
      len = 0;
      for (int l = 9; l <= 16; ++l) {
        const int c = (int)(v >> (32 - l));
        if (c <= T.maxcode[t * 17 + l]) {
          sym = T.vals[t * 256 + ((T.valoff[t * 17 + l] + c) & 255)];
          len = l;
          break;
        }
      }
      if (len == 0) {
        err = JD_CODE;
        break;
      }
    }
    const int s = sym & 15, r = sym >> 4;
    bool complete = false;
    if (z == 0) {
      if (sym > 11) {
        err = JD_DC;
        break;
      }
      if (WRITE && sym) {
        const int bits = (int)((v << len) >> (32 - sym));
        coefs[blk * 64] = (int16_t)((bits >> (sym - 1)) ? bits : bits - (1 << sym) + 1);
      }
      pos += (uint32_t)(len + sym);
      z = 1;
    } else if (s == 0) {
      pos += (uint32_t)len;
      if (r == 15) {
        z += 16;
        if (z > 64) {
          err = JD_COEFS;
          break;
        }
        complete = z == 64;
      } else {
        complete = true;
      }
    } else {
      z += r;
      if (z > 63) {
        err = JD_COEFS;
        break;
      }
      if (WRITE) {
        const int bits = (int)((v << len) >> (32 - s));
        coefs[blk * 64 + z] = (int16_t)((bits >> (s - 1)) ? bits : bits - (1 << s) + 1);
      }
      pos += (uint32_t)(len + s);
      ++z;
      complete = z == 64;
    }
    if (complete) {
      ++done;
      z = 0;
      k = k + 1 == nb ? 0 : k + 1;
      if (WRITE) {
        ++blk;
        if (blk == expected) *endpos = pos;
      }
    }
  }
  if (err) {
    if (WRITE && blk < expected) atomicMax(reinterpret_cast<unsigned int *>(status), (unsigned int)err);
    kz = kJdDead;
  } else {
    kz = (uint32_t)k << 8 | (uint32_t)z;
  }
  return done;
}

// raw bytes [a, b) of an interval of `ilen` bytes: the bytes that remain after unstuffing, up to the first marker (FF not
// followed by 00; an FF that ends the interval counts as one).  PUT: they are stored to dst.  -> their number; cut: the
// position of that marker.
template <bool PUT>
__device__ __forceinline__ uint32_t jd_unstuff(const uint8_t *g, uint32_t a, uint32_t b, uint32_t ilen, uint8_t *dst, uint32_t &cut) {
  uint32_t kept = 0;
  uint32_t prev = a > 0 ? g[a - 1] : 0u;
  for (uint32_t p = a; p < b; ++p) {
    const uint32_t v = g[p];
    const bool stuffed = v == 0u && prev == 0xFFu;  // the 00 of FF 00: dropped (a 00 behind it follows a 00: data)
    prev = v;
    if (stuffed) continue;
    if (v == 0xFFu && (p + 1u >= ilen || g[p + 1u] != 0u)) {
      cut = p;
      break;
    }
    if (PUT) dst[kept] = (uint8_t)v;
    ++kept;
  }
  return kept;
}

// Dynamic LDS: bytes [threads * sub + 32] | look [6 * 256] u16 | maxcode [6 * 17] | valoff [6 * 17] | vals [6 * 256] |
//              entry pos, entry kz, exit pos, exit kz, exit blocks [5 * threads] | scan [2 * threads] | misc [16]
constexpr int kJdLaneArrays = 5, kJdMiscWords = 16;
constexpr size_t jd_entropy_lds(int sub) {
  return (size_t)kJdThreads * sub + 32 + 6 * 256 * 2 + 2 * 6 * 17 * 4 + 6 * 256 + (kJdLaneArrays + 2) * kJdThreads * 4 + kJdMiscWords * 4;
}
static_assert(jd_entropy_lds(kJdSubMax) <= 65536, "the entropy kernel's LDS stays inside the 64 KiB a kernel gets without opting in");

__global__ __launch_bounds__(kJdThreads) void jpegd_entropy(int16_t *__restrict__ coefs, int *__restrict__ status,
                                                            const uint8_t *__restrict__ scans, const long long *__restrict__ offsets,
                                                            long long scans_bytes, const uint8_t *__restrict__ tables,
                                                            const uint32_t *__restrict__ bounds, int n_int, int ri, long long total_mcus,
                                                            int nb, int nl, int nc, int sub) {
  HF_DYN_LDS;
  const int tid = (int)threadIdx.x, iv = (int)blockIdx.x, img = (int)blockIdx.y;
  const int cap = kJdThreads * sub;
  uint8_t *buf = hf_dyn_lds;
  uint16_t *look = reinterpret_cast<uint16_t *>(buf + cap + 32);
  int *maxcode = reinterpret_cast<int *>(look + 6 * 256);
  int *valoff = maxcode + 6 * 17;
  uint8_t *vals = reinterpret_cast<uint8_t *>(valoff + 6 * 17);
  uint32_t *ent_pos = reinterpret_cast<uint32_t *>(vals + 6 * 256);
  uint32_t *ent_kz = ent_pos + kJdThreads, *ex_pos = ent_kz + kJdThreads, *ex_kz = ex_pos + kJdThreads, *ex_n = ex_kz + kJdThreads;
  uint32_t *scan = ent_pos + kJdLaneArrays * kJdThreads;
  uint32_t *misc = scan + 2 * kJdThreads;  // 0, 1: changed flags; 2: inverted cut; 3: end position of the last block
  const uint8_t *tab = tables + (long long)img * kJdTableBytes + kJdHuffOffset;
  int *st = status + 2 * img;

  // ---- the tables ----
  for (int i = tid; i < 6 * 256; i += kJdThreads) vals[i] = tab[(i >> 8) * 272 + 16 + (i & 255)];
  if (tid < 6) {
    int code = 0, p = 0;
    maxcode[tid * 17] = -1;
    valoff[tid * 17] = 0;
    for (int l = 1; l <= 16; ++l) {
      const int n = tab[tid * 272 + l - 1];
      valoff[tid * 17 + l] = p - code;
      maxcode[tid * 17 + l] = n ? code + n - 1 : -1;
      code = (code + n) << 1;
      p += n;
    }
  }
  if (tid < 4) misc[tid] = 0;
  __syncthreads();
  for (int i = tid; i < 6 * 256; i += kJdThreads) {
    const int t = i >> 8, p = i & 255;
    uint32_t e = 0;
    for (int l = 1; l <= 8; ++l) {
      const int c = p >> (8 - l);
      if (c <= maxcode[t * 17 + l]) {
        e = (uint32_t)l << 8 | vals[t * 256 + ((valoff[t * 17 + l] + c) & 255)];
        break;
      }
    }
    look[i] = (uint16_t)e;
  }
  const JdTabs T{look, maxcode, valoff, vals};

  // ---- the interval ----
  long long start;
  uint32_t len;
  jd_scan_range(offsets, img, scans_bytes, start, len);
  const uint32_t *bd = bounds + (long long)img * n_int;
  uint32_t i0 = iv == 0 ? 0u : bd[iv - 1] + 2u, i1 = bd[iv];
  i1 = i1 > len ? len : i1;
  i0 = i0 > i1 ? i1 : i0;
  const uint8_t *g = scans + start + i0;
  const uint32_t ilen = i1 - i0;
  const long long mcu0 = (long long)iv * ri;
  const long long imcus = (total_mcus - mcu0) < ri ? (total_mcus - mcu0) : ri;
  const long long expected = imcus * nb;
  int16_t *ic = coefs + ((long long)img * total_mcus + mcu0) * nb * 64;
  const bool last_iv = iv == n_int - 1;
  bool unterminated = false;  // the scan's last interval ends with the bytes, not with a marker

  const uint32_t chunk = (uint32_t)cap - 16u, sbits = (uint32_t)sub * 8u;
  uint32_t rawpos = 0, carry_n = 0, pos0 = 0, kz0 = 0;
  long long done = 0;
  uint32_t max_passes = 0;
  bool final_seen = false;
  const uint32_t max_windows = ilen / chunk + 2u;
  for (uint32_t win = 0; win < max_windows && !final_seen; ++win) {
    __syncthreads();  // the tables are built; the window before is read
    if (done >= expected || kz0 == kJdDead) break;
    // ---- 1. unstuff the window's raw bytes behind the carried ones ----
    const uint32_t cend = rawpos + chunk < ilen ? rawpos + chunk : ilen;
    uint32_t a = rawpos + (uint32_t)tid * (uint32_t)sub, b = a + (uint32_t)sub;
    a = a > cend ? cend : a;
    b = b > cend ? cend : b;
    uint32_t mycut = 0xFFFFFFFFu;
    uint32_t kept = jd_unstuff<false>(g, a, b, ilen, nullptr, mycut);
    if (mycut != 0xFFFFFFFFu) atomicMax(&misc[2], 0xFFFFFFFFu - mycut);
    __syncthreads();
    const uint32_t cut = 0xFFFFFFFFu - misc[2];  // 0xFFFFFFFF: none
    if (a > cut) kept = 0;
    uint32_t total_kept;
    const uint32_t incl = codec_scan<kJdThreads>(scan, tid, kept, total_kept);
    if (kept) {
      uint32_t dummy;
      jd_unstuff<true>(g, a, b, ilen, buf + carry_n + incl - kept, dummy);
    }
    const uint32_t n_total = carry_n + total_kept;
    if (tid < 16) buf[n_total + tid] = 0;
    const bool final = cut != 0xFFFFFFFFu || cend >= ilen;
    if (final && last_iv && i1 >= len && (cut == 0xFFFFFFFFu || cut + 1u >= ilen)) unterminated = true;
    final_seen = final;
    const uint32_t limit = final ? n_total * 8u : (n_total > 8u ? (n_total - 8u) * 8u : 0u);
    const uint32_t nsub = (limit + sbits - 1u) / sbits;  // at most kJdThreads: n_total <= 16 + chunk
    __syncthreads();
    if (tid < 3) misc[tid] = 0;
    // ---- 2. pass 0: every subsequence from the guess "a block starts here", the first from the true state ----
    const bool lane = (uint32_t)tid < nsub && nsub <= (uint32_t)kJdThreads;
    const uint32_t my_end = ((uint32_t)tid + 1u) * sbits < limit ? ((uint32_t)tid + 1u) * sbits : limit;
    if (lane) {
      uint32_t p = tid == 0 ? pos0 : (uint32_t)tid * sbits, kz = tid == 0 ? kz0 : 0u;
      ent_pos[tid] = p;
      ent_kz[tid] = kz;
      ex_n[tid] = jd_decode_sub<false>(buf, p, kz, my_end, T, nb, nl, nullptr, 0, 0, nullptr, nullptr);
      ex_pos[tid] = p;
      ex_kz[tid] = kz;
    } else {
      ex_n[tid] = 0;
    }
    // ---- 3. synchronisation passes ----
    uint32_t passes = 0;
    for (uint32_t it = 0; it < nsub; ++it) {
      __syncthreads();
      if (it > 0 && misc[(it - 1u) & 1u] == 0u) break;
      uint32_t pp = 0, pk = 0;
      if (lane && tid > 0) {
        pp = ex_pos[tid - 1];
        pk = ex_kz[tid - 1];
      }
      __syncthreads();
      if (tid == 0) misc[(it + 1u) & 1u] = 0;
      if (lane && tid > 0 && (pp != ent_pos[tid] || pk != ent_kz[tid])) {
        ent_pos[tid] = pp;
        ent_kz[tid] = pk;
        ex_n[tid] = jd_decode_sub<false>(buf, pp, pk, my_end, T, nb, nl, nullptr, 0, 0, nullptr, nullptr);
        ex_pos[tid] = pp;
        ex_kz[tid] = pk;
        misc[it & 1u] = 1u;
      }
      ++passes;
    }
    max_passes = passes > max_passes ? passes : max_passes;
    // ---- 4. block indices, then the coefficients ----
    uint32_t nblocks;
    const uint32_t bincl = codec_scan<kJdThreads>(scan, tid, lane ? ex_n[tid] : 0u, nblocks);
    if (lane) {
      uint32_t p = ent_pos[tid], kz = ent_kz[tid];
      jd_decode_sub<true>(buf, p, kz, my_end, T, nb, nl, ic, done + (long long)(bincl - ex_n[tid]), expected, st, &misc[3]);
    }
    __syncthreads();
    if (nsub > 0 && nsub <= (uint32_t)kJdThreads) {
      pos0 = ex_pos[nsub - 1];
      kz0 = ex_kz[nsub - 1];
    }
    const bool finished = done < expected && done + (long long)nblocks >= expected;
    done += nblocks;
    if (finished && final && misc[3] > n_total * 8u && tid == 0) atomicMax(reinterpret_cast<unsigned int *>(st), (unsigned int)JD_TRUNCATED);
    if (final) break;
    // ---- 5. carry the bytes from the exit position on ----
    const uint32_t cstart = pos0 >> 3;
    uint32_t ncarry = n_total > cstart ? n_total - cstart : 0u;  // at most 8: the exit position lies behind the limit
    ncarry = ncarry > 16u ? 16u : ncarry;                        // (a dead state ends the loop at the next window)
    const uint8_t keep = (uint32_t)tid < ncarry ? buf[cstart + tid] : (uint8_t)0;
    __syncthreads();
    if ((uint32_t)tid < ncarry) buf[tid] = keep;
    carry_n = ncarry;
    pos0 &= 7u;
    rawpos = cend;
  }
  __syncthreads();
  if (tid == 0) {
    if (done < expected) atomicMax(reinterpret_cast<unsigned int *>(st), (unsigned int)JD_TRUNCATED);
    if (unterminated) atomicMax(reinterpret_cast<unsigned int *>(st), (unsigned int)JD_TRUNCATED);
    atomicMax(reinterpret_cast<unsigned int *>(st + 1), max_passes);
  }

  // ---- the DC values: sums of the differences per component over the interval, one MCU per thread and round ----
  uint32_t run[3] = {0u, 0u, 0u};
  for (long long m0 = 0; m0 < imcus; m0 += kJdThreads) {
    const long long m = m0 + tid;
    const bool active = m < imcus;
    int16_t *mc = ic + m * nb * 64;
    uint32_t sum[3] = {0u, 0u, 0u};
    if (active) {
      for (int k = 0; k < nl; ++k) sum[0] += (uint32_t)(int)mc[k * 64];
      for (int c = 1; c < nc; ++c) sum[c] = (uint32_t)(int)mc[(nl + c - 1) * 64];
    }
    for (int c = 0; c < nc; ++c) {
      uint32_t total;
      const uint32_t inc = codec_scan<kJdThreads>(scan, tid, sum[c], total);
      uint32_t v = run[c] + inc - sum[c];
      run[c] += total;
      if (!active) continue;
      if (c == 0) {
        for (int k = 0; k < nl; ++k) {
          v += (uint32_t)(int)mc[k * 64];
          mc[k * 64] = (int16_t)v;
        }
      } else {
        mc[(nl + c - 1) * 64] = (int16_t)(v + sum[c]);
      }
    }
  }
}

// jidctint.c: one pass over eight values; SHIFT 11 for the column pass (the results stay scaled by 2^PASS1_BITS), 18 for
// the row pass
template <int SHIFT>
__device__ __forceinline__ void jd_idct8(int &d0, int &d1, int &d2, int &d3, int &d4, int &d5, int &d6, int &d7) {
  constexpr int kRound = 1 << (SHIFT - 1);
  const int z1 = (d2 + d6) * 4433;
  const int tmp2 = z1 - d6 * 15137, tmp3 = z1 + d2 * 6270;
  const int tmp0 = (d0 + d4) * 8192, tmp1 = (d0 - d4) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  int t0 = d7, t1 = d5, t2 = d3, t3 = d1;
  jpeg_dct_odd(t0, t1, t2, t3);
  d0 = (tmp10 + t3 + kRound) >> SHIFT;
  d7 = (tmp10 - t3 + kRound) >> SHIFT;
  d1 = (tmp11 + t2 + kRound) >> SHIFT;
  d6 = (tmp11 - t2 + kRound) >> SHIFT;
  d2 = (tmp12 + t1 + kRound) >> SHIFT;
  d5 = (tmp12 - t1 + kRound) >> SHIFT;
  d3 = (tmp13 + t0 + kRound) >> SHIFT;
  d4 = (tmp13 - t0 + kRound) >> SHIFT;
}

// Dynamic LDS: quantisation tables [3][64] uint16
__global__ __launch_bounds__(kJdThreads) void jpegd_blocks(uint8_t *__restrict__ planes, const int16_t *__restrict__ coefs,
                                                           const uint8_t *__restrict__ tables, long long total_blocks, int nb, int nl, int hs,
                                                           int mcus_x, long long yw, long long ysize, long long cw, long long csize,
                                                           long long image_planes) {
  HF_DYN_LDS;
  uint16_t *q = reinterpret_cast<uint16_t *>(hf_dyn_lds);
  const int tid = (int)threadIdx.x, img = (int)blockIdx.y;
  if (tid < 192) q[tid] = reinterpret_cast<const uint16_t *>(tables + (long long)img * kJdTableBytes)[tid];
  __syncthreads();
  const long long blk = (long long)blockIdx.x * kJdThreads + tid;
  if (blk >= total_blocks) return;
  const long long mcu = blk / nb;
  const int k = (int)(blk - mcu * nb);
  const long long my = mcu / mcus_x, mx = mcu - my * mcus_x;
  const int comp = jpeg_block_component(k, nl);
  uint8_t *dst = planes + (long long)img * image_planes;
  long long pitch;
  if (k < nl) {
    int by, bx;
    jpeg_luma_block_at(k, hs, by, bx);
    pitch = yw;
    dst += ((my * (nl / hs) + by) * 8) * yw + (mx * hs + bx) * 8;
  } else {
    pitch = cw;
    dst += ysize + (long long)(comp - 1) * csize + (my * 8) * cw + mx * 8;
  }
  const CodecVec16 *src = reinterpret_cast<const CodecVec16 *>(coefs + ((long long)img * total_blocks + blk) * 64);
  const uint16_t *qc = q + comp * 64;
  int d[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const CodecVec16 v = src[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int n = kJpegNatural[i * 8 + j];
      d[n] = jpeg_coef(v, j) * (int)qc[n];
    }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) jd_idct8<11>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    jd_idct8<18>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      int v = d[r * 8 + c] + 128;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      w[c >> 2] |= (uint32_t)v << (8 * (c & 3));
    }
    uint32_t *o = reinterpret_cast<uint32_t *>(dst + r * pitch);
    o[0] = w[0];
    o[1] = w[1];
  }
}

// one chroma sample at full resolution: jdsample.c's fancy upsampling of plane C (pitch cw) for pixel (x, y)
__device__ __forceinline__ int jd_chroma(const uint8_t *C, long long cw, int x, int y, int hs, int vs, int dw, int dh) {
  if (hs == 1) return C[(long long)y * cw + x];
  const int i = x >> 1;
  if (vs == 1) {
    const uint8_t *row = C + (long long)y * cw;
    const int s = row[i];
    if (dw <= 2) return s;
    if (x & 1) return i == dw - 1 ? s : (3 * s + row[i + 1] + 2) >> 2;
    return i == 0 ? s : (3 * s + row[i - 1] + 1) >> 2;
  }
  const int r = y >> 1;
  const uint8_t *row = C + (long long)r * cw;
  if (dw <= 2) return row[i];
  const int rn = (y & 1) ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
  const uint8_t *near = C + (long long)rn * cw;
  const int c = 3 * row[i] + near[i];
  const int j = (x & 1) ? i + 1 : i - 1;
  const int bias = (x & 1) ? 7 : 8;
  if (j < 0 || j >= dw) return (4 * c + bias) >> 4;
  return (3 * c + 3 * row[j] + near[j] + bias) >> 4;
}

__device__ __forceinline__ int jd_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(kJdThreads) void jpegd_pixels(uint8_t *__restrict__ out, float *__restrict__ outf, const uint8_t *__restrict__ planes,
                                                           int h, int w, int nc, int hs, int vs, int oc, long long yw, long long ysize,
                                                           long long cw, long long csize, long long image_planes) {
  const long long idx = (long long)blockIdx.x * kJdThreads + threadIdx.x;
  const long long npix = (long long)h * w;
  if (idx >= npix) return;
  const int img = (int)blockIdx.y;
  const int y = (int)(idx / w), x = (int)(idx - (long long)y * w);
  const uint8_t *P = planes + (long long)img * image_planes;
  const int Y = P[(long long)y * yw + x];
  int rgb[3] = {Y, Y, Y};
  if (nc == 3) {
    const int dw = (w + hs - 1) / hs, dh = (h + vs - 1) / vs;
    const int cb = jd_chroma(P + ysize, cw, x, y, hs, vs, dw, dh) - 128;
    const int cr = jd_chroma(P + ysize + csize, cw, x, y, hs, vs, dw, dh) - 128;
    rgb[0] = jd_clamp255(Y + ((91881 * cr + 32768) >> 16));
    rgb[1] = jd_clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = jd_clamp255(Y + ((116130 * cb + 32768) >> 16));
  }
  if (out)
    for (int c = 0; c < oc; ++c) out[((long long)img * npix + idx) * oc + c] = (uint8_t)rgb[c];
  if (outf)
    for (int c = 0; c < oc; ++c) outf[((long long)img * oc + c) * npix + idx] = (float)rgb[c] / 255.0f;  // a true division
}

// false: a geometry the decoder does not take
inline bool jd_geometry(int batch, int h, int w, int components, int hs, int vs, int restart_interval, long long max_scan_bytes, JdGeom &g) {
  if (batch <= 0 || batch > 65535 || restart_interval < 0 || restart_interval > 65535) return false;
  if (max_scan_bytes < 0 || max_scan_bytes > 0x7fffffffLL) return false;
  if (!jpeg_mcus(h, w, components, hs, vs, g)) return false;
  g.total_mcus = (long long)g.mcus * g.rows;
  g.total_blocks = g.total_mcus * g.nb;
  const long long per = restart_interval ? restart_interval : g.total_mcus;
  const long long n_int = (g.total_mcus + per - 1) / per;
  if (per > 0x7fffffffLL || n_int > 0x7fffffffLL) return false;
  g.ri = (int)per, g.n_int = (int)n_int;
  g.yw = (long long)g.mcus * hs * 8, g.yh = (long long)g.rows * vs * 8;
  g.cw = (long long)g.mcus * 8, g.ch = (long long)g.rows * 8;
  g.coef_bytes = (long long)batch * g.total_blocks * 128;
  g.plane_bytes = (g.yw * g.yh + (components == 3 ? 2 * g.cw * g.ch : 0) + 15) / 16 * 16;
  g.bounds_bytes = ((long long)batch * g.n_int * 4 + 15) / 16 * 16;
  g.nchunks = (int)((max_scan_bytes + kJdChunk - 1) / kJdChunk);
  g.nchunks = g.nchunks < 1 ? 1 : g.nchunks;
  g.counts_bytes = restart_interval ? ((long long)batch * g.nchunks * 4 + 15) / 16 * 16 : 0;
  return g.coef_bytes + (long long)batch * g.plane_bytes < (1ll << 40);
}

}  // namespace

extern "C" long long hf_jpeg_decode_workspace_bytes(int batch, int h, int w, int components, int hs, int vs, int restart_interval,
                                                    long long max_scan_bytes) {
  JdGeom g;
  if (!jd_geometry(batch, h, w, components, hs, vs, restart_interval, max_scan_bytes, g)) return 0;
  return g.coef_bytes + (long long)batch * g.plane_bytes + g.bounds_bytes + g.counts_bytes;
}

extern "C" int hf_jpeg_decode_u8(unsigned char *out, float *out_f32, int *status, const unsigned char *scans, long long scans_bytes,
                                 const long long *scan_offsets, long long max_scan_bytes, const unsigned char *tables, int batch, int h,
                                 int w, int components, int hs, int vs, int restart_interval, int out_channels, int sub_bytes,
                                 void *workspace, long long workspace_bytes, void *stream) {
  JdGeom g;
  if ((!out && !out_f32) || !status || !scans || !scan_offsets || !tables || !workspace || scans_bytes <= 0) return HF_E_INVALID;
  if (!jd_geometry(batch, h, w, components, hs, vs, restart_interval, max_scan_bytes, g)) return HF_E_INVALID;
  if (!(out_channels == 3 || (out_channels == 1 && components == 1))) return HF_E_INVALID;
  const int sub = sub_bytes == 0 ? kJdSubDefault : sub_bytes;
  if (sub < kJdSubMin || sub > kJdSubMax) return HF_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || (reinterpret_cast<uintptr_t>(scan_offsets) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(tables) & 1u) != 0 || (reinterpret_cast<uintptr_t>(status) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(out_f32) & 3u) != 0)
    return HF_E_INVALID;
  if (workspace_bytes < hf_jpeg_decode_workspace_bytes(batch, h, w, components, hs, vs, restart_interval, max_scan_bytes)) return HF_E_WORKSPACE;
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  int16_t *coefs = reinterpret_cast<int16_t *>(ws);
  uint8_t *planes = ws + g.coef_bytes;
  uint32_t *bounds = reinterpret_cast<uint32_t *>(planes + (long long)batch * g.plane_bytes);
  uint32_t *counts = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(bounds) + g.bounds_bytes);
  hipStream_t st = (hipStream_t)stream;
  const long long n16 = g.coef_bytes / 16;
  const long long clear_items = n16 > (long long)batch * g.n_int ? n16 : (long long)batch * g.n_int;
  long long cg = (clear_items + kJdThreads - 1) / kJdThreads;
  cg = cg > 16384 ? 16384 : (cg < 1 ? 1 : cg);
  hipLaunchKernelGGL(jpegd_clear, dim3((unsigned)cg), dim3(kJdThreads), 0, st, reinterpret_cast<CodecVec16 *>(coefs), n16, status, bounds,
                     scan_offsets, scans_bytes, batch, g.n_int);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  if (restart_interval) {
    hipLaunchKernelGGL(jpegd_marker_count, dim3(g.nchunks, batch), dim3(kJdThreads), 16, st, counts, scans, scan_offsets, scans_bytes);
    if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
    hipLaunchKernelGGL(jpegd_marker_place, dim3(g.nchunks, batch), dim3(kJdThreads), 16 + 2 * kJdThreads * 4, st, bounds, status, counts,
                       scans, scan_offsets, scans_bytes, g.n_int);
    if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  }
  hipLaunchKernelGGL(jpegd_entropy, dim3(g.n_int, batch), dim3(kJdThreads), jd_entropy_lds(sub), st, coefs, status, scans, scan_offsets,
                     scans_bytes, tables, bounds, g.n_int, g.ri, g.total_mcus, g.nb, g.nl, g.nc, sub);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  const long long ysize = g.yw * g.yh, csize = g.cw * g.ch;
  hipLaunchKernelGGL(jpegd_blocks, dim3((unsigned)((g.total_blocks + kJdThreads - 1) / kJdThreads), batch), dim3(kJdThreads), 384, st, planes,
                     coefs, tables, g.total_blocks, g.nb, g.nl, g.hs, g.mcus, g.yw, ysize, g.cw, csize, g.plane_bytes);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  const long long npix = (long long)h * w;
  hipLaunchKernelGGL(jpegd_pixels, dim3((unsigned)((npix + kJdThreads - 1) / kJdThreads), batch), dim3(kJdThreads), 0, st, out, out_f32, planes,
                     h, w, g.nc, g.hs, g.vs, out_channels, g.yw, ysize, g.cw, csize, g.plane_bytes);
  return hf_launch_status();
}
