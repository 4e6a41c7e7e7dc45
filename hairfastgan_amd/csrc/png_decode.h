// png_decode.h - a PNG decoder on the device, the counterpart of png.h: the zlib streams (the concatenated IDAT payloads) of a
// group of files of one geometry become uint8 images [B,H,W,1|2|3|4] and, optionally, float images [B,C,H,W] = byte / 255 -
// the pixels Pillow's Image.open(f).convert("RGB") returns (or the file's own samples), byte for byte.  Bit depth 8, no
// interlace, colour types 0, 2, 3, 4 and 6.  Included by encoder_ops.hip.  DESIGN.md 4.25.
//
//   hf_png_decode_workspace_bytes   host-only shape arithmetic
//   hf_png_decode_u8                eight launches, no allocation, no synchronisation
//
// pngd_count / pngd_place   the candidate segment starts of each stream in 16 KiB chunks: the positions behind every
//                     00 00 FF FF (an empty stored block, what ends a segment of png.h and a Z_FULL_FLUSH), in stream order,
//                     at most kPdMaxCand of them; candidate 0 is byte 2, behind the zlib header, which is checked here.
// pngd_inflate<false> (candidates x files, one wave) decodes from its candidate as if a block began there at bit 0 and writes
//                     NOTHING but its record: it stops where a block ends byte-aligned on a later candidate, or behind the
//                     final block, or at the first error, or when its output passes the image's total; the record holds the
//                     end, the output count, the error, the candidate it ended on and whether a match reached before its
//                     own first byte.  Symbols do not depend on the bytes they produce, so counting needs no output.
// pngd_chain          (files) walks the records from candidate 0: a candidate is valid iff a valid one ended on it.  A
//                     decoder that ends a block byte-aligned at c is in the state a decoder starting at c assumes, so the
//                     chain is the sequential decode.  Output offsets are the sums of the counts before.  If a valid segment
//                     holds a match that reaches before its start, the file takes the serial route: candidate 0 alone,
//                     decoding to the final block.
// pngd_inflate<true>  the valid segments decode again (the tokens of the first pass are not kept: a segment's tokens are as
//                     many as its bytes, the second decode reads only the compressed bytes) and write at their offsets.
//                     Lane 0 decodes symbols into a token buffer in LDS (token_cap tokens), then the wave stores the
//                     literals in parallel and copies the matches in order, each by all lanes (byte k of a match comes from
//                     position k mod distance of its source, so a match longer than its distance needs no second pass).  The
//                     window is the output buffer itself.  A stored block is copied by the wave from the stream.
// pngd_adler          Adler-32 partial sums (sum, weighted sum) of 4 KiB chunks of the inflated bytes.
// pngd_unfilter       (files, one wave) combines the partial sums by png_finish's rule and compares with the stream's trailer;
//                     then undoes the row filters in place as a skewed wavefront: lane j takes row r0 + j one pixel behind
//                     lane j - 1, `a` is the lane's last pixel, `b` the last pixel of the lane above (a DPP wave shift), `c`
//                     the `b` of the step before; one instruction stream for the five types.  Lane 0 of a band reads the row
//                     above, the last of the band before, from memory.
// pngd_pixels         one thread per pixel: grey -> RGB, alpha dropped, the palette, the float planes.
//
// Safety: nothing read from a stream becomes an index, a count or an address unchecked.  Stream offsets are clamped to the
// buffer, every stream read is bounded by the stream's length, every output write by the segment's count and by
// H * (W * channels + 1), table indices are masked or bounded by construction of a checked code, a distance beyond the bytes
// produced is an error, every loop consumes at least one bit per turn or is bounded by a count.  The first pass writes only
// its record.  status[2 b] is the largest error code of file b, status[2 b + 1] the number of segments decoded independently.
// From png.h: kAdlerMod, kPngClOrder, png_paeth, png_length_extra_bits; from jpeg_decode.h: jd_scan_range; from
// codec_common.h: codec_scan, codec_sum_before.
#pragma once
#include <cstdint>

#include "hf_common.h"
#include "jpeg_decode.h"
#include "png.h"

namespace {

constexpr int kPdThreads = 256;      // the byte-parallel kernels
constexpr int kPdWave = 64;          // inflate and unfilter: one wave
constexpr int kPdChunk = 16384;      // bytes of a stream per workgroup of the candidate search
constexpr int kPdMaxCand = 2048;     // candidates per file
constexpr int kPdAdlerChunk = 4096;  // bytes per workgroup of pngd_adler: 16 per thread
constexpr int kPdTokMin = 2, kPdTokMax = 2048, kPdTokDefault = 1024;
constexpr int kPdRecWords = 8;       // end, count, error, flags, next, offset, valid
constexpr int kPdInfoWords = 4;      // candidates, trailer position
enum { PD_OK = 0, PD_TRUNCATED = 1, PD_BTYPE = 2, PD_STORED = 3, PD_LENGTHS = 4, PD_REPEAT = 5, PD_COUNTS = 6, PD_CODE = 7,
       PD_LENSYM = 8, PD_DISTSYM = 9, PD_DIST = 10, PD_MANY = 11, PD_FEW = 12, PD_FILTER = 13, PD_ADLER = 14, PD_ZLIB = 15 };
enum { PDR_END = 0, PDR_COUNT = 1, PDR_ERR = 2, PDR_FLAGS = 3, PDR_NEXT = 4, PDR_OFFSET = 5, PDR_VALID = 6 };
enum { PDS_ERR = 0, PDS_BTYPE, PDS_NLEN, PDS_NDIST, PDS_STOP, PDS_NLIT, PDS_NMATCH, PDS_DONE, PDS_SRC, PDS_SLEN, PDS_OUT, PDS_WORDS = 16 };

struct PdGeom {
  int bpp, nchunks, nadler;
  long long rb, total, raw_stride;
  long long raw_bytes, cand_bytes, rec_bytes, info_bytes, count_bytes, adler_bytes;
};

// whether 00 00 FF FF stands at byte p of the stream (behind the zlib header)
__device__ __forceinline__ bool pd_pattern_at(const uint8_t *g, uint64_t p, uint32_t len) {
  return p >= 2u && p + 3u < len && g[p] == 0u && g[p + 1] == 0u && g[p + 2] == 0xFFu && g[p + 3] == 0xFFu;
}

// Dynamic LDS: sum [4].  Block (0, b) also checks the zlib header and initialises status and info.
__global__ __launch_bounds__(kPdThreads) void pngd_count(uint32_t *__restrict__ counts, int *__restrict__ status, uint32_t *__restrict__ info,
                                                         const uint8_t *__restrict__ streams, const long long *__restrict__ offsets,
                                                         long long streams_bytes) {
  HF_DYN_LDS;
  uint32_t *sum = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  const int tid = (int)threadIdx.x, c = (int)blockIdx.x, b = (int)blockIdx.y;
  long long start;
  uint32_t len;
  jd_scan_range(offsets, b, streams_bytes, start, len);
  const uint8_t *g = streams + start;
  if (tid == 0) sum[0] = 0;
  __syncthreads();
  const uint64_t a = (uint64_t)c * kPdChunk + (uint64_t)tid * (kPdChunk / kPdThreads);
  uint32_t n = 0;
  for (int i = 0; i < kPdChunk / kPdThreads; ++i)
    if (pd_pattern_at(g, a + i, len)) ++n;
  if (n) atomicAdd(&sum[0], n);
  __syncthreads();
  if (tid != 0) return;
  counts[(long long)b * gridDim.x + c] = sum[0];
  if (c != 0) return;
  int err = PD_OK;
  if (len < 2u) {
    err = PD_TRUNCATED;
  } else {
    const uint32_t cmf = g[0], flg = g[1];  // CM 8, a window of at most 32 KiB, the check bits, no preset dictionary
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8 | flg) % 31u) != 0u || (flg & 0x20u)) err = PD_ZLIB;
  }
  status[2 * b] = err;
  status[2 * b + 1] = 0;
  for (int i = 0; i < kPdInfoWords; ++i) info[(long long)b * kPdInfoWords + i] = 0;
}

// Dynamic LDS: sum [4] | scan [2 * threads]
__global__ __launch_bounds__(kPdThreads) void pngd_place(uint32_t *__restrict__ cands, uint32_t *__restrict__ info, const uint32_t *__restrict__ counts,
                                                         const uint8_t *__restrict__ streams, const long long *__restrict__ offsets,
                                                         long long streams_bytes, int max_cand) {
  HF_DYN_LDS;
  uint32_t *sum = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  uint32_t *scan = sum + 4;
  const int tid = (int)threadIdx.x, c = (int)blockIdx.x, b = (int)blockIdx.y;
  long long start;
  uint32_t len;
  jd_scan_range(offsets, b, streams_bytes, start, len);
  const uint8_t *g = streams + start;
  codec_sum_before<kPdThreads>(sum, c, tid, [&](int i) { return counts[(long long)b * gridDim.x + i]; });
  const uint64_t a = (uint64_t)c * kPdChunk + (uint64_t)tid * (kPdChunk / kPdThreads);
  uint32_t n = 0;
  for (int i = 0; i < kPdChunk / kPdThreads; ++i)
    if (pd_pattern_at(g, a + i, len)) ++n;
  uint32_t total;
  const uint32_t incl = codec_scan<kPdThreads>(scan, tid, n, total);  // its barriers also publish sum[0]
  uint64_t j = 1ull + sum[0] + incl - n;                              // candidate 0 is the stream's start
  uint32_t *cd = cands + (long long)b * kPdMaxCand;
  if (tid == 0 && c == 0) cd[0] = 2u;
  if (tid == 0 && c == (int)gridDim.x - 1) {
    const uint64_t all = 1ull + sum[0] + total;
    info[(long long)b * kPdInfoWords] = (uint32_t)(all > (uint64_t)max_cand ? (uint64_t)max_cand : all);
  }
  if (n == 0) return;
  for (int i = 0; i < kPdChunk / kPdThreads; ++i) {
    if (!pd_pattern_at(g, a + i, len)) continue;
    if (j < (uint64_t)max_cand) cd[j] = (uint32_t)(a + i + 4u);
    ++j;
  }
}

// the tables of the inflate kernel in LDS; code 0: literal / length, code 1: distance (the code-length code borrows code 0)
struct PdShared {
  uint32_t cnt[2][16], first[2][16], offs[2][16], fill[16];
  uint32_t state[PDS_WORDS];
  uint16_t sorted[2][288];  // symbols by (length, symbol)
  uint16_t table[2][1024];  // by the next 10 bits of the stream: length << 12 | symbol, 0: a longer code or none
  uint8_t lens[320];
};
static_assert(sizeof(PdShared) % 16 == 0, "the token arrays behind the tables stay aligned");
constexpr size_t pd_inflate_lds(int cap) { return sizeof(PdShared) + (size_t)cap * 13 + 16; }
static_assert(pd_inflate_lds(kPdTokMax) <= 65536, "the inflate kernel's LDS stays inside the 64 KiB a kernel gets without opting in");

// The stream's bits, LSB first.  The next four bytes are loaded one refill ahead (`ahead`); measured, this does not shorten
// the decode loop.  Behind the stream's end the bytes read as zeros; `trunc` is set once a bit behind the
// end has been consumed.
struct PdBits {
  const uint8_t *g;
  uint32_t len, pos;  // pos: the bytes merged into acc (it may pass len: zeros)
  uint32_t ahead;     // the bytes [pos, pos + 4)
  uint64_t acc;
  int n;
  bool trunc;
  __device__ __forceinline__ uint32_t word_at(uint32_t p) const {
    if (p < len && len - p >= 4u) return (uint32_t)g[p] | (uint32_t)g[p + 1] << 8 | (uint32_t)g[p + 2] << 16 | (uint32_t)g[p + 3] << 24;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4u; ++k)
      if (p < len && k < len - p) v |= (uint32_t)g[p + k] << (8u * k);
    return v;
  }
  __device__ __forceinline__ void init(const uint8_t *stream, uint32_t length, uint32_t at) {
    g = stream, len = length, pos = at > length ? length : at, acc = 0, n = 0, trunc = false;
    ahead = word_at(pos);
  }
  __device__ __forceinline__ void refill() {  // afterwards more than 32 bits
    if (n > 32) return;
    acc |= (uint64_t)ahead << n;
    n += 32;
    pos += 4u;
    ahead = word_at(pos);
  }
  __device__ __forceinline__ long long left() const { return (long long)len * 8 - ((long long)pos * 8 - n); }  // true bits not consumed
  __device__ __forceinline__ void drop(int k) {  // k <= n
    acc >>= k;
    n -= k;
    if (left() < 0) trunc = true;
  }
  __device__ __forceinline__ uint32_t take(int k) {  // k <= 16
    refill();
    const uint32_t v = (uint32_t)acc & ((1u << k) - 1u);
    drop(k);
    return trunc ? 0u : v;
  }
  __device__ __forceinline__ uint32_t byte_pos() const {  // of the next bit, at most len
    const long long p = (long long)pos - (n >> 3);
    return p > (long long)len ? len : (uint32_t)p;
  }
};

// lane 0: counts, first codes and the sorted symbols of the code lengths lens[0, nsym) (each below 16) -> an error code.
// strict: the code-length code, which must be complete; the others may be one code of one bit, or empty.
__device__ __forceinline__ int pd_code_prepare(PdShared &S, int t, const uint8_t *lens, int nsym, bool strict) {
  for (int l = 0; l < 16; ++l) S.cnt[t][l] = 0;
  for (int i = 0; i < nsym; ++i) S.cnt[t][lens[i] & 15] += 1;
  S.cnt[t][0] = 0;
  int left = 1, maxl = 0;
  for (int l = 1; l < 16; ++l) {
    left = (left << 1) - (int)S.cnt[t][l];
    if (left < 0) return PD_LENGTHS;  // over-subscribed
    if (S.cnt[t][l]) maxl = l;
  }
  if (left > 0 && (strict || maxl > 1)) return PD_LENGTHS;  // incomplete with more than one code
  uint32_t code = 0, off = 0;
  S.first[t][0] = 0, S.offs[t][0] = 0;
  for (int l = 1; l < 16; ++l) {
    code = (code + S.cnt[t][l - 1]) << 1;
    S.first[t][l] = code;
    S.offs[t][l] = off;
    S.fill[l] = off;
    off += S.cnt[t][l];
  }
  for (int i = 0; i < nsym; ++i) {
    const int l = lens[i] & 15;
    if (l) S.sorted[t][S.fill[l]++] = (uint16_t)i;  // below nsym <= 288: the counts sum to the used symbols
  }
  return PD_OK;
}

// the symbol whose code the `width` bits of rev begin with (MSB first), lengths lo..hi -> its length, 0 if there is none
__device__ __forceinline__ int pd_canonical(const PdShared &S, int t, uint32_t rev, int width, int lo, int hi, uint32_t &sym) {
  for (int l = lo; l <= hi; ++l) {
    const uint32_t d = (rev >> (width - l)) - S.first[t][l];  // wraps below the first code: no match
    if (d < S.cnt[t][l]) {
      const uint32_t at = S.offs[t][l] + d;
      sym = S.sorted[t][at < 288u ? at : 287u];
      return l;
    }
  }
  return 0;
}

// ALL lanes (contains barriers): the 10-bit table of code t
__device__ __forceinline__ void pd_code_table(PdShared &S, int t, int lane) {
  __syncthreads();
  for (int idx = lane; idx < 1024; idx += kPdWave) {
    uint32_t sym = 0;
    const int l = pd_canonical(S, t, __builtin_bitreverse32((uint32_t)idx) >> 22, 10, 1, 10, sym);
    S.table[t][idx] = (uint16_t)(l ? (uint32_t)l << 12 | sym : 0u);
  }
  __syncthreads();
}

__device__ __forceinline__ int pd_decode(const PdShared &S, int t, uint32_t bits, uint32_t &sym) {
  const uint32_t e = S.table[t][bits & 1023u];
  if (e) {
    sym = e & 0xFFFu;
    return (int)(e >> 12);
  }
  return pd_canonical(S, t, __builtin_bitreverse32(bits) >> 17, 15, 11, 15, sym);
}

// lane 0: the header of a dynamic block -> S.lens, S.state[PDS_NLEN / PDS_NDIST]; an error code
__device__ __forceinline__ int pd_dynamic_header(PdShared &S, PdBits &br) {
  const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncl = (int)br.take(4) + 4;
  if (br.trunc) return PD_TRUNCATED;
  if (nlen > 286 || ndist > 30) return PD_COUNTS;
  uint8_t clc[19];
  for (int i = 0; i < 19; ++i) clc[i] = 0;
  for (int i = 0; i < ncl; ++i) clc[kPngClOrder[i]] = (uint8_t)br.take(3);
  if (br.trunc) return PD_TRUNCATED;
  const int e = pd_code_prepare(S, 0, clc, 19, true);
  if (e) return e;
  const int total = nlen + ndist;
  int i = 0;
  while (i < total) {  // i grows by at least 1 per turn
    br.refill();
    uint32_t sym = 0;
    const int l = pd_canonical(S, 0, __builtin_bitreverse32((uint32_t)br.acc) >> 25, 7, 1, 7, sym);
    if (l == 0) return br.left() < 7 ? PD_TRUNCATED : PD_CODE;
    br.drop(l);
    if (br.trunc) return PD_TRUNCATED;
    if (sym < 16u) {
      S.lens[i++] = (uint8_t)sym;
      continue;
    }
    uint32_t prev = 0;
    int rep;
    if (sym == 16u) {
      if (i == 0) return PD_REPEAT;
      prev = S.lens[i - 1];
      rep = 3 + (int)br.take(2);
    } else if (sym == 17u) {
      rep = 3 + (int)br.take(3);
    } else {
      rep = 11 + (int)br.take(7);
    }
    if (br.trunc) return PD_TRUNCATED;
    if (i + rep > total) return PD_LENGTHS;
    for (int k = 0; k < rep; ++k) S.lens[i++] = (uint8_t)prev;
  }
  if (S.lens[256] == 0) return PD_LENGTHS;  // no end-of-block code
  S.state[PDS_NLEN] = (uint32_t)nlen;
  S.state[PDS_NDIST] = (uint32_t)ndist;
  return PD_OK;
}

// lane 0: the index above `c` of the candidate at byte p, 0 if there is none
__device__ __forceinline__ uint32_t pd_find_candidate(const uint32_t *cd, uint32_t ncand, uint32_t c, uint32_t p) {
  uint32_t lo = c + 1u, hi = ncand;
  while (lo < hi) {  // the interval halves
    const uint32_t mid = (lo + hi) >> 1;
    if (cd[mid] < p) lo = mid + 1u;
    else hi = mid;
  }
  return lo < ncand && cd[lo] == p ? lo : 0u;
}

// One candidate of one file.  WRITE false: the record only.  WRITE true: the valid segments (record word PDR_VALID 1: to the
// candidate it ended on; 2: the serial route, the whole stream) write their bytes.
// Dynamic LDS: PdShared | literal positions [cap] | match positions [cap] | match length << 16 | distance - 1 [cap] |
//              literal bytes [cap]
template <bool WRITE>
__global__ __launch_bounds__(kPdWave) void pngd_inflate(uint8_t *__restrict__ raw, long long raw_stride, uint32_t *__restrict__ recs,
                                                        uint32_t *__restrict__ info, int *__restrict__ status, const uint32_t *__restrict__ cands,
                                                        const uint8_t *__restrict__ streams, const long long *__restrict__ offsets,
                                                        long long streams_bytes, long long total, int cap) {
  HF_DYN_LDS;
  PdShared &S = *reinterpret_cast<PdShared *>(hf_dyn_lds);
  uint32_t *lit_pos = reinterpret_cast<uint32_t *>(hf_dyn_lds + sizeof(PdShared));
  uint32_t *m_pos = lit_pos + cap, *m_ld = m_pos + cap;
  uint8_t *lit_val = reinterpret_cast<uint8_t *>(m_ld + cap);
  const int lane = (int)threadIdx.x, b = (int)blockIdx.y;
  const uint32_t c = blockIdx.x;
  uint32_t ncand = info[(long long)b * kPdInfoWords];
  ncand = ncand > (uint32_t)kPdMaxCand ? (uint32_t)kPdMaxCand : ncand;
  if (c >= ncand) return;
  uint32_t *R = recs + ((long long)b * kPdMaxCand + c) * kPdRecWords;
  const uint32_t *cd = cands + (long long)b * kPdMaxCand;
  bool serial = false;
  uint32_t limit = (uint32_t)total;  // most bytes this decode may produce
  uint8_t *o = raw + (long long)b * raw_stride;
  if (WRITE) {
    const uint32_t valid = R[PDR_VALID];
    if (valid == 0u) return;
    serial = valid == 2u;
    if (!serial) {
      const uint32_t off = R[PDR_OFFSET], cnt = R[PDR_COUNT];
      if ((long long)off + cnt > total) return;  // the chain summed the counts to the total
      o += off;
      limit = cnt;
    }
  }
  long long start;
  uint32_t len;
  jd_scan_range(offsets, b, streams_bytes, start, len);
  const uint8_t *g = streams + start;
  PdBits br;
  br.init(g, len, serial ? 2u : cd[c]);
  uint32_t nout = 0, flags = 0, next = 0;
  if (lane < PDS_WORDS) S.state[lane] = 0;
  __syncthreads();

  const uint64_t max_blocks = (uint64_t)len * 8u / 3u + 2u;  // a block is at least 3 bits
  for (uint64_t blk = 0; blk < max_blocks; ++blk) {
    // ---- the block's header, by lane 0 ----
    if (lane == 0) {
      int err = PD_OK;
      const uint32_t final = br.take(1), btype = br.take(2);
      if (br.trunc) err = PD_TRUNCATED;
      else if (btype == 3u) err = PD_BTYPE;
      else if (btype == 0u) {
        br.drop(br.n & 7);
        const uint32_t n = br.take(16), nn = br.take(16);
        const uint32_t src = br.byte_pos();
        if (br.trunc) err = PD_TRUNCATED;
        else if ((n ^ nn) != 0xFFFFu) err = PD_STORED;
        else if (src + n > len) err = PD_TRUNCATED;
        else if (n > limit - nout) err = PD_MANY;
        S.state[PDS_SRC] = src;
        S.state[PDS_SLEN] = n;
      } else if (btype == 1u) {
        for (int i = 0; i < 288; ++i) S.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 32; ++i) S.lens[288 + i] = 5;
        S.state[PDS_NLEN] = 288;
        S.state[PDS_NDIST] = 32;
      } else {
        err = pd_dynamic_header(S, br);
      }
      if (!err && btype != 0u) {
        const int nl = (int)S.state[PDS_NLEN];
        err = pd_code_prepare(S, 0, S.lens, nl, false);
        if (!err) err = pd_code_prepare(S, 1, S.lens + nl, (int)S.state[PDS_NDIST], false);
      }
      S.state[PDS_ERR] = (uint32_t)err;
      S.state[PDS_BTYPE] = btype;
      S.state[PDS_STOP] = final;
      S.state[PDS_OUT] = nout;
    }
    __syncthreads();
    const uint32_t herr = S.state[PDS_ERR], btype = S.state[PDS_BTYPE];
    const uint32_t final = S.state[PDS_STOP];
    __syncthreads();
    if (herr) break;
    if (btype == 0u) {
      // ---- a stored block: the wave copies ----
      const uint32_t n = S.state[PDS_SLEN], src = S.state[PDS_SRC], at = S.state[PDS_OUT];
      if (WRITE)
        for (uint32_t k = (uint32_t)lane; k < n; k += kPdWave) o[at + k] = g[src + k];  // at + n <= limit, src + n <= len
      if (lane == 0) {
        nout += n;
        br.init(g, len, src + n);
      }
    } else {
      pd_code_table(S, 0, lane);
      pd_code_table(S, 1, lane);
      // ---- the symbols: lane 0 decodes up to `cap` tokens, the wave writes them ----
      const uint64_t max_rounds = WRITE ? (uint64_t)len * 8u / (uint32_t)cap + 2u : 1u;  // a token is at least one bit
      uint32_t serr = 0, done = 0;
      for (uint64_t round = 0; round < max_rounds; ++round) {
        if (lane == 0) {
          int err = PD_OK;
          uint32_t nl = 0, nm = 0, eob = 0;
          while (!WRITE || nl + nm < (uint32_t)cap) {  // a turn consumes at least one bit, or ends the loop
            br.refill();
            uint32_t sym = 0;
            const int l = pd_decode(S, 0, (uint32_t)br.acc, sym);
            if (l == 0) {
              err = br.left() >= 15 ? PD_CODE : PD_TRUNCATED;
              break;
            }
            br.drop(l);
            if (br.trunc) {
              err = PD_TRUNCATED;
              break;
            }
            if (sym < 256u) {
              if (nout >= limit) {
                err = PD_MANY;
                break;
              }
              if (WRITE) {
                lit_pos[nl] = nout;
                lit_val[nl] = (uint8_t)sym;
              }
              ++nl;
              ++nout;
              continue;
            }
            if (sym == 256u) {
              eob = 1;
              break;
            }
            if (sym >= 286u) {
              err = PD_LENSYM;
              break;
            }
            const int idx = (int)sym - 257, eb = png_length_extra_bits(idx);
            const uint32_t mlen = (idx < 8 ? 3u + (uint32_t)idx : idx == 28 ? 258u : 3u + ((4u + ((uint32_t)idx & 3u)) << eb)) + br.take(eb);
            br.refill();
            uint32_t dsym = 0;
            const int dl = pd_decode(S, 1, (uint32_t)br.acc, dsym);
            if (br.trunc || dl == 0) {
              err = (!br.trunc && br.left() >= 15) ? PD_CODE : PD_TRUNCATED;
              break;
            }
            br.drop(dl);
            if (dsym >= 30u) {
              err = PD_DISTSYM;
              break;
            }
            const int deb = dsym < 4u ? 0 : (int)(dsym >> 1) - 1;
            const uint32_t dist = (dsym < 4u ? 1u + dsym : 1u + ((2u + (dsym & 1u)) << deb)) + br.take(deb);
            if (br.trunc) {
              err = PD_TRUNCATED;
              break;
            }
            if (dist > nout) {
              if (WRITE) {
                err = PD_DIST;
                break;
              }
              flags |= 1u;  // reaches before this decode's first byte: for the chain to judge
            }
            if (mlen > limit - nout) {
              err = PD_MANY;
              break;
            }
            if (WRITE) {
              m_pos[nm] = nout;
              m_ld[nm] = mlen << 16 | (dist - 1u);
            }
            ++nm;
            nout += mlen;
          }
          S.state[PDS_ERR] = (uint32_t)err;
          S.state[PDS_NLIT] = nl;
          S.state[PDS_NMATCH] = nm;
          S.state[PDS_DONE] = eob;
        }
        __syncthreads();
        serr = S.state[PDS_ERR];
        const uint32_t nl = S.state[PDS_NLIT], nm = S.state[PDS_NMATCH];
        done = S.state[PDS_DONE];
        if (WRITE) {
          for (uint32_t i = (uint32_t)lane; i < nl; i += kPdWave) o[lit_pos[i]] = lit_val[i];  // positions below limit
          for (uint32_t i = 0; i < nm; ++i) {
            __syncthreads();  // the bytes before this match are written
            const uint32_t at = m_pos[i], mlen = m_ld[i] >> 16, dist = (m_ld[i] & 0xFFFFu) + 1u;  // dist <= at, at + mlen <= limit
            for (uint32_t k = (uint32_t)lane; k < mlen; k += kPdWave) o[at + k] = o[at - dist + k % dist];
          }
        }
        __syncthreads();
        if (serr || done) break;
      }
      if (serr) break;
      if (done == 0u) {  // the rounds ran out: cannot happen within the stream's bits
        if (lane == 0) S.state[PDS_ERR] = PD_TRUNCATED;
        break;
      }
    }
    // ---- the block's end ----
    if (lane == 0) {
      uint32_t stop = final;
      if (final) {
        flags |= 2u;
        br.drop(br.n & 7);
      } else if (!serial && (br.n & 7) == 0) {
        next = pd_find_candidate(cd, ncand, c, br.byte_pos());
        stop = next != 0u;
      }
      S.state[PDS_STOP] = stop;
    }
    __syncthreads();
    const uint32_t stop = S.state[PDS_STOP];
    __syncthreads();
    if (stop) break;
  }
  __syncthreads();
  if (lane != 0) return;
  uint32_t err = S.state[PDS_ERR];
  if (!err && !(flags & 2u) && next == 0u) err = PD_TRUNCATED;  // neither a final block nor a candidate ended it
  if (!WRITE) {
    R[PDR_END] = br.byte_pos();
    R[PDR_COUNT] = nout;
    R[PDR_ERR] = err;
    R[PDR_FLAGS] = flags;
    R[PDR_NEXT] = next;
    return;
  }
  if (!err && nout != limit) err = nout < limit ? PD_FEW : PD_MANY;
  if (err) atomicMax(reinterpret_cast<unsigned int *>(status + 2 * b), (unsigned int)err);
  if (serial) info[(long long)b * kPdInfoWords + 1] = br.byte_pos();
}

// Dynamic LDS: next [kPdMaxCand] | count [kPdMaxCand] | error | flags << 8 [kPdMaxCand]
__global__ __launch_bounds__(kPdThreads) void pngd_chain(uint32_t *__restrict__ recs, uint32_t *__restrict__ info, int *__restrict__ status,
                                                         long long total) {
  HF_DYN_LDS;
  uint32_t *nxt = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  uint32_t *cnt = nxt + kPdMaxCand, *meta = cnt + kPdMaxCand;
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  uint32_t ncand = info[(long long)b * kPdInfoWords];
  ncand = ncand > (uint32_t)kPdMaxCand ? (uint32_t)kPdMaxCand : ncand;
  uint32_t *R = recs + (long long)b * kPdMaxCand * kPdRecWords;
  for (uint32_t i = (uint32_t)tid; i < ncand; i += kPdThreads) {
    nxt[i] = R[i * kPdRecWords + PDR_NEXT];
    cnt[i] = R[i * kPdRecWords + PDR_COUNT];
    meta[i] = (R[i * kPdRecWords + PDR_ERR] & 255u) | R[i * kPdRecWords + PDR_FLAGS] << 8;
    R[i * kPdRecWords + PDR_VALID] = 0;
  }
  __syncthreads();
  if (tid != 0 || ncand == 0u || status[2 * b] != 0) return;
  uint32_t s = 0, steps = 0, nseg = 0, err = 0, back = 0, last = 0;
  unsigned long long sum = 0;
  bool ended = false;
  for (uint32_t it = 0; it < ncand; ++it) {  // s grows per turn
    const uint32_t m = meta[s];
    back |= (m >> 8) & 1u;
    if (m & 255u) {
      err = m & 255u;
      break;
    }
    sum += cnt[s];
    ++steps;
    nseg += cnt[s] ? 1u : 0u;  // a segment without bytes (the final empty block of png.h's files) is not counted
    last = s;
    if ((m >> 8) & 2u) {
      ended = true;
      break;
    }
    const uint32_t n = nxt[s];
    if (n <= s || n >= ncand) break;
    s = n;
  }
  if (back) {  // the serial route decides, errors included
    R[PDR_VALID] = 2u;
    status[2 * b + 1] = 1;
    return;
  }
  if (!err && !ended) err = PD_TRUNCATED;
  if (!err && sum != (unsigned long long)total) err = sum < (unsigned long long)total ? PD_FEW : PD_MANY;
  status[2 * b + 1] = (int)nseg;
  if (err) {
    status[2 * b] = (int)err;
    return;
  }
  uint32_t off = 0;
  s = 0;
  for (uint32_t it = 0; it < steps; ++it) {
    R[s * kPdRecWords + PDR_OFFSET] = off;
    R[s * kPdRecWords + PDR_VALID] = cnt[s] ? 1u : 0u;
    off += cnt[s];
    s = nxt[s];
  }
  info[(long long)b * kPdInfoWords + 1] = R[last * kPdRecWords + PDR_END];
}

// Dynamic LDS: sums [4]
__global__ __launch_bounds__(kPdThreads) void pngd_adler(uint32_t *__restrict__ parts, const uint8_t *__restrict__ raw, long long raw_stride,
                                                         long long total) {
  HF_DYN_LDS;
  uint32_t *sum = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  const int tid = (int)threadIdx.x, c = (int)blockIdx.x, b = (int)blockIdx.y;
  const uint8_t *f = raw + (long long)b * raw_stride;
  if (tid < 2) sum[tid] = 0;
  __syncthreads();
  long long cend = ((long long)c + 1) * kPdAdlerChunk;
  cend = cend > total ? total : cend;
  long long a0 = (long long)c * kPdAdlerChunk + (long long)tid * (kPdAdlerChunk / kPdThreads);
  a0 = a0 > cend ? cend : a0;
  long long b0 = a0 + kPdAdlerChunk / kPdThreads;
  b0 = b0 > cend ? cend : b0;
  uint32_t sa = 0, sb = 0;
  for (long long p = a0; p < b0; ++p) {
    const uint32_t v = f[p];
    sa += v;
    sb += v * (uint32_t)(b0 - p);
  }
  atomicAdd(&sum[0], sa);                                           // at most 255 * 4096
  atomicAdd(&sum[1], (sb + sa * (uint32_t)(cend - b0)) % kAdlerMod);  // below 255 * 16 * 4096
  __syncthreads();
  if (tid == 0) {
    uint32_t *p = parts + ((long long)b * gridDim.x + c) * 2;
    p[0] = sum[0] % kAdlerMod;
    p[1] = sum[1] % kAdlerMod;
  }
}

// Dynamic LDS: sums [4]
__global__ __launch_bounds__(kPdWave) void pngd_unfilter(uint8_t *__restrict__ raw, long long raw_stride, int *__restrict__ status,
                                                         const uint32_t *__restrict__ info, const uint32_t *__restrict__ parts, int nadler,
                                                         const uint8_t *__restrict__ streams, const long long *__restrict__ offsets,
                                                         long long streams_bytes, int h, int w, int bpp, long long total) {
  HF_DYN_LDS;
  uint32_t *sum = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  const int lane = (int)threadIdx.x, b = (int)blockIdx.x;
  const bool inflated = status[2 * b] == 0;  // else the bytes are not the file's: their filter types are not judged
  // ---- Adler-32: A = 1 + sum(a_s), B = N + sum(b_s + a_s * bytes_after_s) mod 65521 (png_finish's rule) ----
  if (lane < 2) sum[lane] = 0;
  __syncthreads();
  {
    unsigned long long sa = 0, sb = 0;
    for (int s = lane; s < nadler; s += kPdWave) {
      const uint32_t *p = parts + ((long long)b * nadler + s) * 2;
      long long endf = ((long long)s + 1) * kPdAdlerChunk;
      endf = endf > total ? total : endf;
      sa += p[0];
      sb = (sb + p[1] + (unsigned long long)p[0] * ((unsigned long long)(total - endf) % kAdlerMod)) % kAdlerMod;
    }
    atomicAdd(&sum[0], (uint32_t)(sa % kAdlerMod));
    atomicAdd(&sum[1], (uint32_t)sb);
  }
  __syncthreads();
  if (lane == 0 && inflated) {
    const uint32_t adl_a = (1u + sum[0] % kAdlerMod) % kAdlerMod;
    const uint32_t adl_b = (uint32_t)(((unsigned long long)total % kAdlerMod + sum[1] % kAdlerMod) % kAdlerMod);
    long long start;
    uint32_t len;
    jd_scan_range(offsets, b, streams_bytes, start, len);
    const uint8_t *g = streams + start;
    const uint32_t tp = info[(long long)b * kPdInfoWords + 1];
    int err = PD_OK;
    if (tp > len || len - tp < 4u) err = PD_TRUNCATED;
    else if (((uint32_t)g[tp] << 24 | (uint32_t)g[tp + 1] << 16 | (uint32_t)g[tp + 2] << 8 | (uint32_t)g[tp + 3]) != (adl_b << 16 | adl_a)) err = PD_ADLER;
    if (err) atomicMax(reinterpret_cast<unsigned int *>(status + 2 * b), (unsigned int)err);
  }
  // ---- the filters, in place: bands of 64 rows, lane j one pixel behind lane j - 1 ----
  uint8_t *f = raw + (long long)b * raw_stride;
  const long long stride = (long long)w * bpp + 1;
  for (int r0 = 0; r0 < h; r0 += kPdWave) {
    const int r = r0 + lane;
    const bool active = r < h;
    uint8_t *cur = f + (long long)(active ? r : 0) * stride + 1;
    const uint8_t *above = f + (long long)(r0 > 0 ? r0 - 1 : 0) * stride + 1;  // lane 0's row above: the band before
    uint32_t ft = active ? cur[-1] : 0u;
    if (ft > 4u) {
      if (inflated) atomicMax(reinterpret_cast<unsigned int *>(status + 2 * b), (unsigned int)PD_FILTER);
      ft = 0;
    }
    uint32_t last[4] = {0u, 0u, 0u, 0u}, cprev[4] = {0u, 0u, 0u, 0u};  // a (the lane's last pixel) and c (the b before)
    for (int t = 0; t < w + kPdWave - 1; ++t) {
      const int x = t - lane;
      const bool on = active && x >= 0 && x < w;
      uint32_t bv[4];
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) bv[ch] = ch < bpp ? (uint32_t)hf_lane_up((float)last[ch]) : 0u;  // every lane: a wave shift
      if (lane == 0) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) bv[ch] = (on && r0 > 0 && ch < bpp) ? above[(long long)x * bpp + ch] : 0u;
      }
      if (on) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
          if (ch >= bpp) break;
          uint8_t *px = cur + (long long)x * bpp + ch;
          const uint32_t a = last[ch], bb = bv[ch], cc = cprev[ch];
          uint32_t pred = 0;
          if (ft == 1u) pred = a;
          else if (ft == 2u) pred = bb;
          else if (ft == 3u) pred = (a + bb) >> 1;
          else if (ft == 4u) pred = png_paeth((int)a, (int)bb, (int)cc);
          const uint32_t v = (*px + pred) & 255u;
          *px = (uint8_t)v;
          last[ch] = v;
          cprev[ch] = bb;
        }
      }
    }
    __syncthreads();  // the band's last row is written before the next band's lane 0 reads it
  }
}

__global__ __launch_bounds__(kPdThreads) void pngd_pixels(uint8_t *__restrict__ out, float *__restrict__ outf, const uint8_t *__restrict__ raw,
                                                          long long raw_stride, const uint8_t *__restrict__ palettes, int h, int w,
                                                          int color_type, int bpp, int oc) {
  const long long idx = (long long)blockIdx.x * kPdThreads + threadIdx.x;
  const long long npix = (long long)h * w;
  if (idx >= npix) return;
  const int img = (int)blockIdx.y;
  const long long y = idx / w, x = idx - y * w;
  const uint8_t *p = raw + (long long)img * raw_stride + y * ((long long)w * bpp + 1) + 1 + x * bpp;
  uint32_t v[4] = {0u, 0u, 0u, 0u};
  if (color_type == 3) {
    const uint8_t *pal = palettes + ((long long)img * 256 + p[0]) * 3;
    v[0] = pal[0], v[1] = pal[1], v[2] = pal[2];
  } else if (color_type == 2 || color_type == 6) {
    v[0] = p[0], v[1] = p[1], v[2] = p[2];
    if (color_type == 6) v[3] = p[3];
  } else if (oc == 3) {  // grey, with or without alpha, as RGB
    v[0] = v[1] = v[2] = p[0];
  } else {
    v[0] = p[0];
    if (color_type == 4) v[1] = p[1];
  }
  if (out)
    for (int c = 0; c < oc; ++c) out[((long long)img * npix + idx) * oc + c] = (uint8_t)v[c];
  if (outf)
    for (int c = 0; c < oc; ++c) outf[((long long)img * oc + c) * npix + idx] = (float)v[c] / 255.0f;  // a true division
}

inline int pd_channels(int color_type) { return color_type == 0 ? 1 : color_type == 2 ? 3 : color_type == 3 ? 1 : color_type == 4 ? 2 : color_type == 6 ? 4 : 0; }

// false: a geometry the decoder does not take
inline bool pd_geometry(int batch, int h, int w, int color_type, long long max_stream_bytes, PdGeom &g) {
  g.bpp = pd_channels(color_type);
  if (batch <= 0 || batch > 65535 || h <= 0 || w <= 0 || g.bpp == 0) return false;
  if (max_stream_bytes < 0 || max_stream_bytes > 0x7fffffffLL) return false;
  g.rb = (long long)w * g.bpp;
  g.total = (long long)h * (g.rb + 1);
  if (g.total > 0x7fffffffLL || (long long)h * w > 0x7fffffffLL) return false;
  g.raw_stride = (g.total + 15) / 16 * 16;
  g.nchunks = (int)((max_stream_bytes + kPdChunk - 1) / kPdChunk);
  g.nchunks = g.nchunks < 1 ? 1 : g.nchunks;
  g.nadler = (int)((g.total + kPdAdlerChunk - 1) / kPdAdlerChunk);
  g.raw_bytes = (long long)batch * g.raw_stride;
  g.cand_bytes = (long long)batch * kPdMaxCand * 4;
  g.rec_bytes = (long long)batch * kPdMaxCand * kPdRecWords * 4;
  g.info_bytes = ((long long)batch * kPdInfoWords * 4 + 15) / 16 * 16;
  g.count_bytes = ((long long)batch * g.nchunks * 4 + 15) / 16 * 16;
  g.adler_bytes = ((long long)batch * g.nadler * 8 + 15) / 16 * 16;
  return g.raw_bytes < (1ll << 40);
}

}  // namespace

extern "C" long long hf_png_decode_workspace_bytes(int batch, int h, int w, int color_type, long long max_stream_bytes) {
  PdGeom g;
  if (!pd_geometry(batch, h, w, color_type, max_stream_bytes, g)) return 0;
  return g.raw_bytes + g.cand_bytes + g.rec_bytes + g.info_bytes + g.count_bytes + g.adler_bytes;
}

extern "C" int hf_png_decode_u8(unsigned char *out, float *out_f32, int *status, const unsigned char *streams, long long streams_bytes,
                                const long long *stream_offsets, long long max_stream_bytes, const unsigned char *palettes, int batch,
                                int h, int w, int color_type, int out_channels, int token_cap, void *workspace, long long workspace_bytes,
                                void *stream) {
  PdGeom g;
  if ((!out && !out_f32) || !status || !streams || !stream_offsets || !workspace || streams_bytes <= 0) return HF_E_INVALID;
  if (!pd_geometry(batch, h, w, color_type, max_stream_bytes, g)) return HF_E_INVALID;
  if (color_type == 3 && !palettes) return HF_E_INVALID;
  const int own = color_type == 3 ? 3 : g.bpp;  // the file's samples, a palette expanded
  if (!(out_channels == 3 || out_channels == own)) return HF_E_INVALID;
  const int cap = token_cap == 0 ? kPdTokDefault : token_cap;
  if (cap < kPdTokMin || cap > kPdTokMax) return HF_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || (reinterpret_cast<uintptr_t>(stream_offsets) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(status) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out_f32) & 3u) != 0)
    return HF_E_INVALID;
  if (workspace_bytes < hf_png_decode_workspace_bytes(batch, h, w, color_type, max_stream_bytes)) return HF_E_WORKSPACE;
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  uint8_t *raw = ws;
  uint32_t *cands = reinterpret_cast<uint32_t *>(ws + g.raw_bytes);
  uint32_t *recs = reinterpret_cast<uint32_t *>(ws + g.raw_bytes + g.cand_bytes);
  uint32_t *info = reinterpret_cast<uint32_t *>(ws + g.raw_bytes + g.cand_bytes + g.rec_bytes);
  uint32_t *counts = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(info) + g.info_bytes);
  uint32_t *parts = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(counts) + g.count_bytes);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pngd_count, dim3(g.nchunks, batch), dim3(kPdThreads), 16, st, counts, status, info, streams, stream_offsets, streams_bytes);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  long long ngrid = 1 + max_stream_bytes / 4;  // a stream holds no more candidates (the pattern is four bytes and cannot
  ngrid = ngrid > kPdMaxCand ? kPdMaxCand : ngrid;  // overlap itself); later ones are ignored, which costs parallelism only
  hipLaunchKernelGGL(pngd_place, dim3(g.nchunks, batch), dim3(kPdThreads), 16 + 2 * kPdThreads * 4, st, cands, info, counts, streams,
                     stream_offsets, streams_bytes, (int)ngrid);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  const size_t lds = pd_inflate_lds(cap);
  hipLaunchKernelGGL(pngd_inflate<false>, dim3((unsigned)ngrid, batch), dim3(kPdWave), lds, st, raw, g.raw_stride, recs, info, status, cands, streams,
                     stream_offsets, streams_bytes, g.total, cap);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  hipLaunchKernelGGL(pngd_chain, dim3(batch), dim3(kPdThreads), 3 * kPdMaxCand * 4, st, recs, info, status, g.total);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  hipLaunchKernelGGL(pngd_inflate<true>, dim3((unsigned)ngrid, batch), dim3(kPdWave), lds, st, raw, g.raw_stride, recs, info, status, cands, streams,
                     stream_offsets, streams_bytes, g.total, cap);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  hipLaunchKernelGGL(pngd_adler, dim3(g.nadler, batch), dim3(kPdThreads), 16, st, parts, raw, g.raw_stride, g.total);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  hipLaunchKernelGGL(pngd_unfilter, dim3(batch), dim3(kPdWave), 16, st, raw, g.raw_stride, status, info, parts, g.nadler, streams,
                     stream_offsets, streams_bytes, h, w, g.bpp, g.total);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  const long long npix = (long long)h * w;
  hipLaunchKernelGGL(pngd_pixels, dim3((unsigned)((npix + kPdThreads - 1) / kPdThreads), batch), dim3(kPdThreads), 0, st, out, out_f32, raw,
                     g.raw_stride, palettes, h, w, color_type, g.bpp, out_channels);
  return hf_launch_status();
}
