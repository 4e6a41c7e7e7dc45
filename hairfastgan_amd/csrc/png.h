// png.h - a PNG encoder on the device: uint8 images [B,H,W,C] (C = 1 grey, 3 RGB; what hf_image_to_bytes_f32's interleaved
// layout and hf_labels_to_rgb_i64 produce) become complete PNG files in caller-allocated slots, so that saving a result
// moves only the compressed bytes to the host and runs no zlib there.  Included by encoder_ops.hip.  DESIGN.md section 4.21.
//
//   hf_png_bound / hf_png_segment_rows / hf_png_workspace_bytes   host-only shape arithmetic
//   hf_png_encode_u8                                              three launches, no allocation, no synchronisation
//
// File: signature, IHDR (bit depth 8, colour type 0 / 2, no interlace), ONE IDAT, IEND.  The zlib stream is 78 01, deflate
// data, Adler-32 of the filtered scanlines.  The image is cut into segments of R rows (hf_png_segment_rows: as many rows,
// up to 16, as keep a segment's filtered bytes within kPngSegBytes of LDS); a segment is one deflate block that refers to
// nothing before it and ends on a byte boundary (an empty stored block), so segments concatenate byte-wise and are encoded
// by independent workgroups.  A final empty stored block (BFINAL) closes the stream.
//
// png_segment (grid: segments x images, 256 threads, everything in LDS):
//   1. the segment's rows into LDS (16-byte loads once the address is aligned), 2. the row filters (adaptive: the type with
//   the smallest sum of |signed residual|, lowest type on ties; the row above a segment's first row is read from the input),
//   3. Adler partial sums, 4. tokens: literals and matches of distance 1 (a run of L repeats of the byte before it is cut
//   into matches of 258 from its start; a rest of 1 or 2 stays literal) - each thread walks a fixed slice of the segment and
//   owns the tokens that START in it, the run a slice begins in is found through per-slice first / last break tables, so
//   the token sequence is a function of the bytes alone, 5. histogram, 6. code lengths: parallel rank sort by (count,
//   symbol), one thread runs the two-queue Huffman merge, depths (hops to the root) and counts per length are parallel
//   again, depths above 15 (7 for the code-length alphabet) are clamped and one thread repairs the Kraft sum one unit per
//   step (a code of the longest length moves under a shorter leaf: fewer steps than symbols) - always a complete code,
//   7. either the dynamic block (header by one thread, the body by all: bit offsets from a scan of per-slice bit counts,
//   bits OR-ed into zeroed LDS words by atomic add) or, when that is not smaller, one stored block, 8. the block to the
//   segment's workspace slot as 16-byte stores.
// png_assemble (segments x images): exclusive sum of the segment sizes before this one, the bytes to their place in the file
//   (dword stores on the destination's alignment), CRC-32 of the segment from 256 slice CRCs combined by
//   crc(A|B) = crc(A) * x^(8|B|) mod P  xor  crc(B).
// png_finish (images): the same combine over segments plus the chunk type, zlib header and trailer; Adler-32 from the
//   segments' (sum, weighted sum) pairs: A = 1 + sum(a_s), B = N + sum(b_s + a_s * bytes_after_s) mod 65521; header, chunk
//   lengths, checksums, IEND and sizes[b].
// Every loop is bounded by the shape (the Kraft repair by the symbol count); passes that depend on each other are separate
// launches; the bytes of image b depend on that image, the shape and the filter mode only.
// The 16-byte vector, the bit packer (PngBits is its LSB-first form), the sum of the sizes before a segment and the copy of
// a slot to the file are codec_common.h's, shared with jpeg.h.
#pragma once
#include <cstdint>

#include "codec_common.h"
#include "hf_common.h"

namespace {

constexpr int kPngThreads = 256;
constexpr int kPngSegBytes = 24640;  // most filtered bytes (rows * (w * c + 1)) of a segment: 8 rows of 1024 RGB pixels
constexpr int kPngMaxRows = 16;
constexpr int kPngCandidates = 5;    // filter types the adaptive mode compares: None, Sub, Up, Average, Paeth
constexpr int kPngHeadBytes = 43;    // signature 8, IHDR 25, IDAT length and type 8, zlib header 2
constexpr int kPngTailBytes = 25;    // final block 5, Adler 4, IDAT CRC 4, IEND 12
constexpr int kPngMetaWords = 8;     // per segment: size, adler a, adler b, crc, offset
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kAdlerMod = 65521u;

// order in which the code-length code's lengths are sent (RFC 1951 3.2.7)
static __device__ const unsigned char kPngClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct PngTables {
  uint32_t hist[288];   // literal / length counts
  uint32_t ssym[288];   // used symbols by ascending (count, symbol)
  uint32_t node[576];   // Huffman nodes: weight, then depth
  uint32_t par[576];
  uint32_t len[292];    // code lengths: literal / length symbols, then the two distance codes
  uint32_t code[288];   // bit-reversed codes
  uint32_t seq[292];    // the run-length coded length sequence: symbol | extra << 8
  uint32_t clhist[20], cllen[20], clcode[20];
  uint32_t cnt[16], nxt[16];
  int brk_last[kPngThreads], brk_first[kPngThreads];
  uint32_t tbits[kPngThreads];
  uint32_t cost[kPngMaxRows * 5];
  uint32_t ftype[kPngMaxRows];
  uint32_t n_used, n_cl, nlit, ncl, nseq, hdr_bits, body_bits, stored, adl_a, adl_b, pad0, pad1;
};

__device__ __forceinline__ uint32_t png_abs_res(uint32_t r) {  // |residual as a signed byte|
  r &= 255u;
  return r < 128u ? r : 256u - r;
}

__device__ __forceinline__ uint32_t png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

__device__ __forceinline__ uint32_t png_filter(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t pred = 0;
  if (type == 1) pred = a;
  else if (type == 2) pred = b;
  else if (type == 3) pred = (a + b) >> 1;
  else if (type == 4) pred = png_paeth((int)a, (int)b, (int)c);
  return (x - pred) & 255u;
}

using PngBits = CodecBits<false>;  // deflate packs bits LSB first

// match length 3..258 -> length code index (symbol 257 + index), number and value of the extra bits
__device__ __forceinline__ void png_length_code(int m, int &idx, int &eb, uint32_t &ev) {
  const int l = m - 3;
  if (m == 258) {
    idx = 28; eb = 0; ev = 0;
  } else if (l < 8) {
    idx = l; eb = 0; ev = 0;
  } else {
    const int lg = 31 - __builtin_clz((unsigned)l);
    eb = lg - 2;
    idx = 4 * eb + 4 + ((l >> eb) & 3);
    ev = (uint32_t)l & ((1u << eb) - 1u);
  }
}

__device__ __forceinline__ int png_length_extra_bits(int idx) { return (idx < 8 || idx == 28) ? 0 : (idx >> 2) - 1; }

__device__ __forceinline__ bool png_is_break(const uint8_t *f, int p) { return p == 0 || f[p] != f[p - 1]; }

// The tokens that start in [a, b) of the segment's filtered bytes f[0, S): lit(byte) / match(length), in order.
template <class Lit, class Match>
__device__ __forceinline__ void png_tokens(const uint8_t *f, const PngTables &T, int S, int a, int b, int t, Lit &&lit, Match &&match) {
  if (a >= b) return;
  int s = 0;  // the last break at or before p
  if (!png_is_break(f, a)) {
    for (int tt = t - 1; tt >= 0; --tt)
      if (T.brk_last[tt] >= 0) {
        s = T.brk_last[tt];
        break;
      }
  }
  int e = 0;
  bool e_known = false;
  int p = a;
  while (p < b) {  // p grows by at least 1 per turn
    if (png_is_break(f, p)) {
      s = p;
      e_known = false;
      lit((uint32_t)f[p]);
      ++p;
      continue;
    }
    if (!e_known) {  // the first break after p, or S
      e = S;
      bool found = false;
      for (int q = p + 1; q < b; ++q)
        if (f[q] != f[q - 1]) {
          e = q;
          found = true;
          break;
        }
      if (!found)
        for (int tt = t + 1; tt < kPngThreads; ++tt)
          if (T.brk_first[tt] >= 0) {
            e = T.brk_first[tt];
            break;
          }
      e_known = true;
    }
    const int L = e - s - 1, k = p - s - 1;  // p is repeat k of L repeats of f[s]
    const int rem = L % 258;
    const int lit_from = rem < 3 ? L - rem : L;  // a rest of 1 or 2 repeats stays literal
    if (k >= lit_from) {
      lit((uint32_t)f[p]);
      ++p;
      continue;
    }
    const int r = k % 258;
    const int k0 = k - r;
    const int mlen = (lit_from - k0) < 258 ? (lit_from - k0) : 258;
    if (r == 0) match(mlen);  // r != 0: inside a match that started in an earlier slice
    p = s + 1 + k0 + mlen;
  }
}

// used symbols of freq[0, nsym) by ascending (count, symbol); *n_used (zeroed by the caller) counts them
__device__ __forceinline__ void png_rank_sort(const uint32_t *freq, int nsym, uint32_t *ssym, uint32_t *n_used, int tid) {
  for (int sym = tid; sym < nsym; sym += kPngThreads) {
    const uint32_t fq = freq[sym];
    if (!fq) continue;
    int rank = 0;
    for (int j = 0; j < nsym; ++j) {
      const uint32_t g = freq[j];
      rank += (g != 0 && (g < fq || (g == fq && j < sym))) ? 1 : 0;
    }
    ssym[rank] = (uint32_t)sym;
    atomicAdd(n_used, 1u);
  }
}

// ALL threads (contains barriers): lengths of a complete prefix code of at most maxbits for the n sorted symbols
// T.ssym[0, n).  One thread merges (the two-queue form: leaves in sorted order, merged nodes in the order they were made,
// both queue heads held in registers) and repairs the Kraft sum; depths, counts per length and the hand-out are parallel.
__device__ __forceinline__ void png_code_lengths(PngTables &T, const uint32_t *freq, int n, int nsym, int maxbits, uint32_t *lens,
                                                 int tid) {
  for (int i = tid; i < nsym; i += kPngThreads) lens[i] = 0;
  if (tid < 16) T.cnt[tid] = 0;
  for (int i = tid; i < n; i += kPngThreads) T.node[i] = freq[T.ssym[i]];
  __syncthreads();
  if (n < 2) {  // n is the same for every thread.  One symbol: two codes of one bit, a complete code
    if (tid == 0 && n == 1) {
      lens[T.ssym[0]] = 1;
      lens[T.ssym[0] == 0 ? 1 : 0] = 1;
    }
    __syncthreads();
    return;
  }
  const int root = 2 * n - 2;
  if (tid == 0) {
    const uint32_t none = 0xFFFFFFFFu;  // an empty queue; weights are at most kPngSegBytes
    uint32_t lw = T.node[0], iw = none;
    int leaf = 0, inner = n;
    for (int next = n; next <= root; ++next) {
      uint32_t wsum = 0;
      for (int k = 0; k < 2; ++k) {
        if (lw <= iw) {  // a leaf on ties: the shallower tree
          wsum += lw;
          T.par[leaf] = (uint32_t)next;
          ++leaf;
          lw = leaf < n ? T.node[leaf] : none;
        } else {
          wsum += iw;
          T.par[inner] = (uint32_t)next;
          ++inner;
          iw = inner < next ? T.node[inner] : none;
        }
      }
      T.node[next] = wsum;
      if (inner == next) iw = wsum;  // the queue of merged nodes was empty: the new node is its head
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += kPngThreads) {  // depth of leaf i: hops to the root, fewer than n
    int d = 0, j = i;
    for (int hop = 0; hop < n && j != root; ++hop) {
      j = (int)T.par[j];
      ++d;
    }
    atomicAdd(&T.cnt[d < maxbits ? d : maxbits], 1u);  // depths above the limit are clamped to it ...
  }
  __syncthreads();
  if (tid == 0) {  // ... and the Kraft sum repaired: each step lowers it by one unit of 2^-maxbits, fewer than n steps
    uint32_t total = 0;
    for (int l = 1; l <= maxbits; ++l) total += T.cnt[l] << (maxbits - l);
    const uint32_t full = 1u << maxbits;
    for (int it = 0; it < n && total > full; ++it) {
      T.cnt[maxbits] -= 1;  // a code of the longest length moves under ...
      for (int l = maxbits - 1; l >= 1; --l)
        if (T.cnt[l]) {  // ... the deepest shorter leaf, which becomes two leaves one level down
          T.cnt[l] -= 1;
          T.cnt[l + 1] += 2;
          break;
        }
      total -= 1;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < n; idx += kPngThreads) {  // along the sorted order: the rarest symbols the longest codes
    uint32_t acc = 0, len = 1;
    for (int l = maxbits; l >= 1; --l) {
      acc += T.cnt[l];
      if ((uint32_t)idx < acc) {
        len = (uint32_t)l;
        break;
      }
    }
    lens[T.ssym[idx]] = len;
  }
  __syncthreads();
}

// ALL threads (contains barriers): canonical codes (RFC 1951 3.2.2), stored bit-reversed - Huffman codes enter the stream
// MSB first.  A symbol's code is the first code of its length plus the number of earlier symbols of that length.
__device__ __forceinline__ void png_assign_codes(PngTables &T, const uint32_t *lens, int nsym, uint32_t *codes, int tid) {
  if (tid < 16) T.cnt[tid] = 0;
  __syncthreads();
  for (int i = tid; i < nsym; i += kPngThreads)
    if (lens[i]) atomicAdd(&T.cnt[lens[i]], 1u);
  __syncthreads();
  if (tid == 0) {
    uint32_t c = 0;
    T.nxt[0] = 0;
    for (int l = 1; l < 16; ++l) {
      c = (c + T.cnt[l - 1]) << 1;
      T.nxt[l] = c;
    }
  }
  __syncthreads();
  for (int i = tid; i < nsym; i += kPngThreads) {
    const uint32_t l = lens[i];
    uint32_t v = 0;
    if (l) {
      v = T.nxt[l];
      for (int j = 0; j < i; ++j) v += lens[j] == l ? 1u : 0u;
      v = __builtin_bitreverse32(v) >> (32 - l);
    }
    codes[i] = v;
  }
  __syncthreads();
}

// ONE thread: T.len[0, total) run-length coded with the symbols 16 / 17 / 18 into T.seq, counts into T.clhist
__device__ __forceinline__ void png_length_sequence(PngTables &T, int total) {
  for (int i = 0; i < 20; ++i) T.clhist[i] = 0;
  int nseq = 0;
  int i = 0;
  while (i < total) {  // i grows by at least 1 per turn
    const uint32_t v = T.len[i];
    int run = 1;
    while (i + run < total && T.len[i + run] == v) ++run;
    uint32_t sym, extra = 0;
    int used;
    if (v == 0 && run >= 11) {
      used = run < 138 ? run : 138;
      sym = 18;
      extra = (uint32_t)(used - 11);
    } else if (v == 0 && run >= 3) {
      used = run;
      sym = 17;
      extra = (uint32_t)(used - 3);
    } else if (v != 0 && run >= 4) {  // the length itself, then "repeat the previous 3..6 times"
      T.seq[nseq++] = v;
      T.clhist[v] += 1;
      used = (run - 1) < 6 ? (run - 1) : 6;
      sym = 16;
      extra = (uint32_t)(used - 3);
      used += 1;
    } else {
      used = 1;
      sym = v;
    }
    T.seq[nseq++] = sym | extra << 8;
    T.clhist[sym] += 1;
    i += used;
  }
  T.nseq = (uint32_t)nseq;
}

__device__ __forceinline__ uint32_t png_crc_mul(uint32_t a, uint32_t b) {  // a * b mod P, reflected bit order (bit 31 = x^0)
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

__device__ __forceinline__ uint32_t png_crc_xpow8(uint32_t nbytes) {  // x^(8 * nbytes) mod P
  uint32_t result = 0x80000000u, base = 0x00800000u;            // 1, x^8
  for (int i = 0; i < 32; ++i) {
    if (!(nbytes >> i)) break;
    if ((nbytes >> i) & 1u) result = png_crc_mul(result, base);
    base = png_crc_mul(base, base);
  }
  return result;
}

__device__ __forceinline__ int png_put_be32(uint8_t *stage, int n, uint32_t v) {  // -> the position behind the value
  for (int i = 0; i < 4; ++i) stage[n + i] = (uint8_t)(v >> (24 - 8 * i));
  return n + 4;
}

__device__ __forceinline__ uint32_t png_crc_byte(uint32_t c, uint32_t byte) {  // table-free, for the few header bytes
  c ^= byte;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}

// ---------------------------------------------------------------------------------------------------------------------
// One segment -> one deflate block in its workspace slot.  Dynamic LDS: filtered bytes | block words | PngTables.
__global__ __launch_bounds__(kPngThreads) void png_segment(uint8_t *__restrict__ slots, uint32_t *__restrict__ meta,
                                                           const uint8_t *__restrict__ in, int h, int rb, int bpp, int R,
                                                           int filter, int slot_bytes, int lds_filt, int lds_obuf) {
  HF_DYN_LDS;
  uint8_t *f = hf_dyn_lds;
  uint8_t *obuf = hf_dyn_lds + lds_filt;
  uint32_t *obw = reinterpret_cast<uint32_t *>(obuf);
  PngTables &T = *reinterpret_cast<PngTables *>(hf_dyn_lds + lds_filt + lds_obuf);
  const int tid = (int)threadIdx.x;
  const int seg = (int)blockIdx.x, nseg = (int)gridDim.x, img = (int)blockIdx.y;
  const int y0 = seg * R;
  const int rows = (h - y0) < R ? (h - y0) : R;
  const int stride = rb + 1;
  const int S = rows * stride;
  const uint8_t *g = in + ((long long)img * h + y0) * rb;
  const int nraw = rows * rb;

  // ---- 0. tables, raw rows into LDS (at the global address's offset inside 16 bytes, so that vectors stay aligned) ----
  for (int i = tid; i < 288; i += kPngThreads) T.hist[i] = 0;
  if (tid < kPngMaxRows * 5) T.cost[tid] = 0;
  if (tid == 0) {
    T.n_used = 0;
    T.n_cl = 0;
    T.body_bits = 0;
    T.adl_a = 0;
    T.adl_b = 0;
  }
  const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 15u);
  uint8_t *raw = obuf + mis;
  {
    int head = (16 - mis) & 15;
    if (head > nraw) head = nraw;
    const int nvec = (nraw - head) >> 4;
    if (tid < head) raw[tid] = g[tid];
    for (int j = tid; j < nvec; j += kPngThreads)
      *reinterpret_cast<CodecVec16 *>(raw + head + 16 * j) = *reinterpret_cast<const CodecVec16 *>(g + head + 16 * j);
    const int done = head + 16 * nvec;
    if (tid < nraw - done) raw[done + tid] = g[done + tid];
  }
  __syncthreads();

  const bool have_up = y0 > 0;  // the row above the segment: from the input
  // ---- 1. filter types ----
  if (filter == 3) {
    const int wave = tid >> 6, lane = tid & 63;
    for (int y = wave; y < rows; y += kPngThreads / 64) {
      uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
      const uint8_t *cur = raw + y * rb;
      for (int i = lane; i < rb; i += 64) {
        const uint32_t x = cur[i];
        const uint32_t a = i >= bpp ? cur[i - bpp] : 0u;
        uint32_t b = 0, c = 0;
        if (y > 0) {
          b = cur[i - rb];
          c = i >= bpp ? cur[i - rb - bpp] : 0u;
        } else if (have_up) {
          b = g[i - rb];
          c = i >= bpp ? g[i - rb - bpp] : 0u;
        }
        c0 += png_abs_res(x);
        c1 += png_abs_res(x - a);
        c2 += png_abs_res(x - b);
        if (kPngCandidates > 3) {
          c3 += png_abs_res(x - ((a + b) >> 1));
          c4 += png_abs_res(x - png_paeth((int)a, (int)b, (int)c));
        }
      }
      atomicAdd(&T.cost[y * 5 + 0], c0);
      atomicAdd(&T.cost[y * 5 + 1], c1);
      atomicAdd(&T.cost[y * 5 + 2], c2);
      if (kPngCandidates > 3) {
        atomicAdd(&T.cost[y * 5 + 3], c3);
        atomicAdd(&T.cost[y * 5 + 4], c4);
      }
    }
    __syncthreads();
    if (tid < rows) {
      uint32_t best = 0, bc = T.cost[tid * 5];
      for (int k = 1; k < kPngCandidates; ++k) {
        const uint32_t ck = T.cost[tid * 5 + k];
        if (ck < bc) {  // lowest type on ties
          bc = ck;
          best = (uint32_t)k;
        }
      }
      T.ftype[tid] = best;
    }
  } else if (tid < rows) {
    T.ftype[tid] = (uint32_t)filter;
  }
  __syncthreads();

  // ---- 2. filtered bytes ----
  for (int y = 0; y < rows; ++y) {
    const uint32_t ft = T.ftype[y];
    const uint8_t *cur = raw + y * rb;
    uint8_t *dst = f + y * stride;
    if (tid == 0) dst[0] = (uint8_t)ft;
    for (int i = tid; i < rb; i += kPngThreads) {
      const uint32_t x = cur[i];
      const uint32_t a = i >= bpp ? cur[i - bpp] : 0u;
      uint32_t b = 0, c = 0;
      if (y > 0) {
        b = cur[i - rb];
        c = i >= bpp ? cur[i - rb - bpp] : 0u;
      } else if (have_up) {
        b = g[i - rb];
        c = i >= bpp ? g[i - rb - bpp] : 0u;
      }
      dst[1 + i] = (uint8_t)png_filter(ft, x, a, b, c);
    }
  }
  __syncthreads();

  // ---- 3. slices: Adler partial sums and break tables ----
  const int q = (S + kPngThreads - 1) / kPngThreads;
  const int a0 = tid * q < S ? tid * q : S;
  const int b0 = a0 + q < S ? a0 + q : S;
  {
    uint32_t sa = 0, sb = 0;
    int last = -1, first = -1;
    for (int p = a0; p < b0; ++p) {
      const uint32_t v = f[p];
      sa += v;
      sb += v * (uint32_t)(b0 - p);
      if (png_is_break(f, p)) {
        if (first < 0) first = p;
        last = p;
      }
    }
    T.brk_first[tid] = first;
    T.brk_last[tid] = last;
    atomicAdd(&T.adl_a, sa % kAdlerMod);
    atomicAdd(&T.adl_b, (sb + sa * (uint32_t)(S - b0)) % kAdlerMod);
  }
  __syncthreads();

  // ---- 4. histogram ----
  png_tokens(
      f, T, S, a0, b0, tid, [&](uint32_t v) { atomicAdd(&T.hist[v], 1u); },
      [&](int m) {
        int idx, eb;
        uint32_t ev;
        png_length_code(m, idx, eb, ev);
        atomicAdd(&T.hist[257 + idx], 1u);
      });
  if (tid == 0) atomicAdd(&T.hist[256], 1u);  // end of block
  __syncthreads();

  // ---- 5. code lengths ----
  png_rank_sort(T.hist, 286, T.ssym, &T.n_used, tid);
  __syncthreads();
  png_code_lengths(T, T.hist, (int)T.n_used, 288, 15, T.len, tid);
  if (tid == 0) {
    int nlit = 257;
    for (int i = 257; i < 286; ++i)
      if (T.len[i]) nlit = i + 1;
    T.nlit = (uint32_t)nlit;
    T.len[nlit] = 1;  // two distance codes of one bit (distance 1 is code 0): a complete code whether or not matches occur
    T.len[nlit + 1] = 1;
    png_length_sequence(T, nlit + 2);
    T.len[nlit] = 0;
    T.len[nlit + 1] = 0;
  }
  __syncthreads();
  png_rank_sort(T.clhist, 19, T.ssym, &T.n_cl, tid);
  __syncthreads();
  png_code_lengths(T, T.clhist, (int)T.n_cl, 19, 7, T.cllen, tid);
  png_assign_codes(T, T.cllen, 19, T.clcode, tid);
  png_assign_codes(T, T.len, 288, T.code, tid);
  for (int i = tid; i < 286; i += kPngThreads) {  // bits of the block's body: the tokens and the end-of-block code
    uint32_t bits = T.len[i];
    if (i > 256) bits += (uint32_t)png_length_extra_bits(i - 257) + 1u;  // extra bits and the distance code
    if (T.hist[i]) atomicAdd(&T.body_bits, T.hist[i] * bits);
  }
  __syncthreads();
  if (tid == 0) {
    int ncl = 4;
    for (int i = 4; i < 19; ++i)
      if (T.cllen[kPngClOrder[i]]) ncl = i + 1;
    T.ncl = (uint32_t)ncl;
    uint32_t hdr = 3 + 5 + 5 + 4 + 3 * (uint32_t)ncl;
    for (int i = 0; i < 19; ++i) hdr += T.clhist[i] * (T.cllen[i] + (i == 16 ? 2u : i == 17 ? 3u : i == 18 ? 7u : 0u));
    T.hdr_bits = hdr;
    const uint32_t dyn_bytes = ((hdr + T.body_bits + 3u + 7u) >> 3) + 4u;
    T.stored = dyn_bytes >= (uint32_t)S + 5u ? 1u : 0u;
  }
  __syncthreads();

  // ---- 6. the block ----
  uint32_t nbytes;
  if (T.stored) {
    nbytes = (uint32_t)S + 5u;
    if (tid == 0) {
      obuf[0] = 0;  // BFINAL 0, BTYPE 00, padding
      obuf[1] = (uint8_t)(S & 255);
      obuf[2] = (uint8_t)(S >> 8);
      obuf[3] = (uint8_t)(~S & 255);
      obuf[4] = (uint8_t)((~S >> 8) & 255);
    }
    for (int i = tid; i < S; i += kPngThreads) obuf[5 + i] = f[i];
  } else {
    const uint32_t hdr = T.hdr_bits, body = T.body_bits - T.len[256];  // the tokens' bits
    nbytes = ((hdr + T.body_bits + 3u + 7u) >> 3) + 4u;
    const int nwords = (int)((nbytes + 3u) >> 2) + 1;
    for (int i = tid; i < nwords; i += kPngThreads) obw[i] = 0;
    uint32_t mybits = 0;
    png_tokens(
        f, T, S, a0, b0, tid, [&](uint32_t v) { mybits += T.len[v]; },
        [&](int m) {
          int idx, eb;
          uint32_t ev;
          png_length_code(m, idx, eb, ev);
          mybits += T.len[257 + idx] + (uint32_t)eb + 1u;
        });
    T.tbits[tid] = mybits;
    __syncthreads();
    uint32_t off = hdr;
    for (int tt = 0; tt < tid; ++tt) off += T.tbits[tt];
    PngBits bw;
    bw.init(obw, off);
    png_tokens(
        f, T, S, a0, b0, tid, [&](uint32_t v) { bw.put(T.code[v], (int)T.len[v]); },
        [&](int m) {
          int idx, eb;
          uint32_t ev;
          png_length_code(m, idx, eb, ev);
          const uint32_t l = T.len[257 + idx];
          bw.put(T.code[257 + idx] | ev << l, (int)l + eb + 1);  // the distance code (0, one bit) rides on top
        });
    bw.flush();
    if (tid == 0) {
      PngBits hw;
      hw.init(obw, 0);
      hw.put(0u, 1);  // BFINAL
      hw.put(2u, 2);  // dynamic Huffman
      hw.put(T.nlit - 257u, 5);
      hw.put(1u, 5);  // two distance codes
      hw.put(T.ncl - 4u, 4);
      for (uint32_t i = 0; i < T.ncl; ++i) hw.put(T.cllen[kPngClOrder[i]], 3);
      for (uint32_t i = 0; i < T.nseq; ++i) {
        const uint32_t sym = T.seq[i] & 255u, extra = T.seq[i] >> 8;
        hw.put(T.clcode[sym], (int)T.cllen[sym]);
        if (sym == 16) hw.put(extra, 2);
        else if (sym == 17) hw.put(extra, 3);
        else if (sym == 18) hw.put(extra, 7);
      }
      hw.flush();
      PngBits ew;  // end of block, then an empty stored block: three zero bits, padding to a byte, LEN 0000, NLEN FFFF
      const uint32_t end = hdr + body;
      ew.init(obw, end);
      ew.put(T.code[256], (int)T.len[256]);
      ew.put(0u, 3);
      const uint32_t at = end + T.len[256] + 3u;
      ew.put(0u, (int)((8u - (at & 7u)) & 7u));
      ew.put(0xFFFF0000u, 32);
      ew.flush();
    }
  }
  __syncthreads();

  // ---- 7. to the slot ----
  uint8_t *slot = slots + ((long long)img * nseg + seg) * slot_bytes;
  const int nvec = (int)((nbytes + 15u) >> 4);
  for (int j = tid; j < nvec; j += kPngThreads)
    reinterpret_cast<CodecVec16 *>(slot)[j] = reinterpret_cast<const CodecVec16 *>(obuf)[j];
  if (tid == 0) {
    uint32_t *m = meta + ((long long)img * nseg + seg) * kPngMetaWords;
    m[0] = nbytes;
    m[1] = T.adl_a % kAdlerMod;
    m[2] = T.adl_b % kAdlerMod;
  }
}

// dynamic LDS of png_assemble and png_finish in words: the kernels carve at these offsets, the launches pass the totals
constexpr int kPngAsmRed = 256, kPngAsmSum = kPngAsmRed + kPngThreads, kPngAsmLdsWords = kPngAsmSum + 4;
constexpr int kPngFinSum = kPngThreads, kPngFinStage = kPngFinSum + 4, kPngFinStageBytes = 64;
constexpr int kPngFinLdsBytes = kPngFinStage * 4 + kPngFinStageBytes;
static_assert(kPngHeadBytes <= kPngFinStageBytes && kPngTailBytes <= kPngFinStageBytes, "png_finish stages the head and the tail");

// The segment's bytes to their place in the file, and their CRC.  Dynamic LDS: crc table [256], slice CRCs [256], sum [4].
__global__ __launch_bounds__(kPngThreads) void png_assemble(uint8_t *__restrict__ out, long long out_stride,
                                                            const uint8_t *__restrict__ slots, uint32_t *__restrict__ meta,
                                                            int slot_bytes) {
  HF_DYN_LDS;
  uint32_t *tab = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  uint32_t *red = tab + kPngAsmRed;
  uint32_t *sum = tab + kPngAsmSum;
  const int tid = (int)threadIdx.x;
  const int seg = (int)blockIdx.x, nseg = (int)gridDim.x, img = (int)blockIdx.y;
  uint32_t *mimg = meta + (long long)img * nseg * kPngMetaWords;
  {
    uint32_t c = (uint32_t)tid;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    tab[tid] = c;
  }
  codec_sum_before<kPngThreads>(sum, seg, tid, [&](int s) { return mimg[s * kPngMetaWords]; });
  __syncthreads();
  const uint32_t off = sum[0];
  const uint32_t n = mimg[seg * kPngMetaWords];
  const uint8_t *src = slots + ((long long)img * nseg + seg) * slot_bytes;
  codec_copy_slot<kPngThreads>(out + (long long)img * out_stride + kPngHeadBytes + off, src, n, tid);

  // CRC: slices of whole source words
  const uint32_t words = (n + 3u) >> 2;
  const uint32_t wq = (words + kPngThreads - 1) / kPngThreads;
  uint32_t a = (uint32_t)tid * wq * 4u, b = a + wq * 4u;
  if (a > n) a = n;
  if (b > n) b = n;
  uint32_t c = 0xFFFFFFFFu;
  for (uint32_t p = a; p < b; ++p) c = tab[(c ^ src[p]) & 255u] ^ (c >> 8);
  c ^= 0xFFFFFFFFu;  // an empty slice: 0
  red[tid] = c ? png_crc_mul(c, png_crc_xpow8(n - b)) : 0u;
  __syncthreads();
  if (tid == 0) {
    uint32_t x = 0;
    for (int t = 0; t < kPngThreads; ++t) x ^= red[t];
    mimg[seg * kPngMetaWords + 3] = x;
    mimg[seg * kPngMetaWords + 4] = off;
  }
}

// Header, chunk lengths, checksums and IEND of one image; sizes[img].  Dynamic LDS: slice CRCs [256], sums [4], bytes [64].
__global__ __launch_bounds__(kPngThreads) void png_finish(uint8_t *__restrict__ out, long long out_stride,
                                                          long long *__restrict__ sizes, const uint32_t *__restrict__ meta,
                                                          int nseg, int h, int w, int channels, int R) {
  HF_DYN_LDS;
  uint32_t *red = reinterpret_cast<uint32_t *>(hf_dyn_lds);
  uint32_t *sum = red + kPngFinSum;
  uint8_t *stage = reinterpret_cast<uint8_t *>(red + kPngFinStage);
  const int tid = (int)threadIdx.x, img = (int)blockIdx.x;
  const uint32_t *mimg = meta + (long long)img * nseg * kPngMetaWords;
  if (tid < 4) sum[tid] = 0;
  __syncthreads();
  const uint32_t *mlast = mimg + (long long)(nseg - 1) * kPngMetaWords;
  const uint32_t total = mlast[4] + mlast[0];
  const unsigned long long stride = (unsigned long long)w * channels + 1ull;
  const unsigned long long nfilt = (unsigned long long)h * stride;
  uint32_t x = 0;
  unsigned long long sa = 0, sb = 0;
  for (int s = tid; s < nseg; s += kPngThreads) {
    const uint32_t *m = mimg + (long long)s * kPngMetaWords;
    x ^= png_crc_mul(m[3], png_crc_xpow8(total - (m[4] + m[0]) + 9u));
    unsigned long long endf = (unsigned long long)(s + 1) * R * stride;
    if (endf > nfilt) endf = nfilt;
    sa += m[1];
    sb = (sb + m[2] + (unsigned long long)m[1] * ((nfilt - endf) % kAdlerMod)) % kAdlerMod;
  }
  red[tid] = x;
  atomicAdd(&sum[0], (uint32_t)(sa % kAdlerMod));
  atomicAdd(&sum[1], (uint32_t)sb);
  __syncthreads();
  if (tid != 0) return;
  uint8_t *o = out + (long long)img * out_stride;
  const uint32_t adl_a = (1u + sum[0] % kAdlerMod) % kAdlerMod;
  const uint32_t adl_b = (uint32_t)((nfilt % kAdlerMod + sum[1] % kAdlerMod) % kAdlerMod);
  const uint32_t adler = adl_b << 16 | adl_a;
  // signature, IHDR, IDAT length and type, zlib header
  const uint32_t idat_len = total + 11u;
  int n = 0;
  n = png_put_be32(stage, n, 0x89504E47u);  // the signature
  n = png_put_be32(stage, n, 0x0D0A1A0Au);
  n = png_put_be32(stage, n, 13u);
  n = png_put_be32(stage, n, 0x49484452u);  // IHDR
  n = png_put_be32(stage, n, (uint32_t)w);
  n = png_put_be32(stage, n, (uint32_t)h);
  stage[n++] = 8; stage[n++] = channels == 3 ? 2 : 0; stage[n++] = 0; stage[n++] = 0; stage[n++] = 0;
  uint32_t c = 0xFFFFFFFFu;
  for (int i = 12; i < 29; ++i) c = png_crc_byte(c, stage[i]);
  n = png_put_be32(stage, n, c ^ 0xFFFFFFFFu);
  n = png_put_be32(stage, n, idat_len);
  n = png_put_be32(stage, n, 0x49444154u);  // IDAT
  stage[n++] = 0x78; stage[n++] = 0x01;  // n == kPngHeadBytes: nine 32-bit values, five IHDR bytes, the zlib header
  for (int i = 0; i < kPngHeadBytes; ++i) o[i] = stage[i];
  uint32_t chead = 0xFFFFFFFFu;
  for (int i = 37; i < kPngHeadBytes; ++i) chead = png_crc_byte(chead, stage[i]);
  chead ^= 0xFFFFFFFFu;
  // final empty stored block, Adler-32
  n = 0;
  stage[n++] = 1; stage[n++] = 0; stage[n++] = 0; stage[n++] = 0xFF; stage[n++] = 0xFF;
  n = png_put_be32(stage, n, adler);
  uint32_t ctail = 0xFFFFFFFFu;
  for (int i = 0; i < 9; ++i) ctail = png_crc_byte(ctail, stage[i]);
  ctail ^= 0xFFFFFFFFu;
  uint32_t crc = png_crc_mul(chead, png_crc_xpow8(total + 9u)) ^ ctail;
  for (int t = 0; t < kPngThreads; ++t) crc ^= red[t];
  n = png_put_be32(stage, n, crc);
  n = png_put_be32(stage, n, 0u);
  n = png_put_be32(stage, n, 0x49454E44u);  // IEND
  n = png_put_be32(stage, n, 0xAE426082u);  // and its CRC; n == kPngTailBytes: the stored block's five bytes, five values
  uint8_t *tail = o + kPngHeadBytes + total;
  for (int i = 0; i < kPngTailBytes; ++i) tail[i] = stage[i];
  sizes[img] = (long long)kPngHeadBytes + total + kPngTailBytes;
}

struct PngShape {
  int rb, R, nseg, S;
  long long slot, bound;
};

// false: a shape the encoder does not take (a filtered row longer than kPngSegBytes, a file of 2 GiB or more)
inline bool png_shape(int h, int w, int channels, PngShape &s) {
  if (h <= 0 || w <= 0 || (channels != 1 && channels != 3)) return false;
  const long long rb = (long long)w * channels;
  if (rb + 1 > kPngSegBytes) return false;
  s.rb = (int)rb;
  int R = kPngSegBytes / (s.rb + 1);
  if (R > kPngMaxRows) R = kPngMaxRows;
  if (R > h) R = h;
  s.R = R;
  s.nseg = (h + R - 1) / R;
  s.S = R * (s.rb + 1);
  s.slot = (((long long)s.S + 5 + 15) / 16) * 16 + 32;
  s.bound = (long long)h * (rb + 1) + 5ll * s.nseg + kPngHeadBytes + kPngTailBytes;
  return s.bound < (1ll << 31);
}

}  // namespace

extern "C" long long hf_png_bound(int h, int w, int channels) {
  PngShape s;
  return png_shape(h, w, channels, s) ? s.bound : 0;
}

extern "C" int hf_png_segment_rows(int h, int w, int channels) {
  PngShape s;
  return png_shape(h, w, channels, s) ? s.R : 0;
}

extern "C" long long hf_png_workspace_bytes(int batch, int h, int w, int channels) {
  PngShape s;
  if (batch <= 0 || !png_shape(h, w, channels, s)) return 0;
  return (long long)batch * s.nseg * (kPngMetaWords * 4 + s.slot);
}

extern "C" int hf_png_encode_u8(unsigned char *out, long long out_stride, long long *sizes, const unsigned char *in, int batch,
                                int h, int w, int channels, int filter, void *workspace, long long workspace_bytes,
                                void *stream) {
  PngShape s;
  if (!out || !sizes || !in || !workspace || batch <= 0 || batch > 65535 || filter < 0 || filter > 3) return HF_E_INVALID;
  if (!png_shape(h, w, channels, s) || out_stride < s.bound) return HF_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || (reinterpret_cast<uintptr_t>(sizes) & 7u) != 0) return HF_E_INVALID;
  if (workspace_bytes < hf_png_workspace_bytes(batch, h, w, channels)) return HF_E_WORKSPACE;
  uint32_t *meta = static_cast<uint32_t *>(workspace);
  uint8_t *slots = static_cast<uint8_t *>(workspace) + (long long)batch * s.nseg * kPngMetaWords * 4;
  const int lds_filt = (s.S + 15) / 16 * 16;
  const int lds_obuf = (s.S + 5 + 15) / 16 * 16 + 48;
  const size_t lds = (size_t)lds_filt + lds_obuf + sizeof(PngTables);
  static_assert((kPngSegBytes + 15) / 16 * 16 + (kPngSegBytes + 5 + 15) / 16 * 16 + 48 + sizeof(PngTables) <= 65536,
                "a segment's LDS stays inside the 64 KiB a kernel gets without opting in");
  static_assert(sizeof(PngTables) % 16 == 0, "16-byte carve offsets");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(png_segment, dim3(s.nseg, batch), dim3(kPngThreads), lds, st, slots, meta, in, h, s.rb, channels, s.R, filter,
                     (int)s.slot, lds_filt, lds_obuf);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  hipLaunchKernelGGL(png_assemble, dim3(s.nseg, batch), dim3(kPngThreads), kPngAsmLdsWords * 4, st, out, out_stride, slots, meta,
                     (int)s.slot);
  if (hf_launch_status() != HF_OK) return HF_E_LAUNCH;
  hipLaunchKernelGGL(png_finish, dim3(batch), dim3(kPngThreads), kPngFinLdsBytes, st, out, out_stride, sizes, meta, s.nseg, h, w,
                     channels, s.R);
  return hf_launch_status();
}
