// Baseline JPEG entropy decoding, shared by the device kernel (jpeg.hip) and the host (tests build it with a plain C++ compiler):
// the byte reader, the Huffman lookup tables and the decoder of one 8x8 block.  Nothing here depends on HIP.
//
// Safety contract (any bytes, any tables):
//   * the reader loads inside [lo, hi) of the buffer only and returns zero bits past the end of its segment or behind a marker;
//   * a coefficient index never exceeds 63, a table index never leaves its table;
//   * JpegBits::starved() says whether bits were consumed that the segment did not hold.
#pragma once
#include <stdint.h>

#include "../../include/syncfusion_amd.h"

#if defined(__HIPCC__)
#define SF_JPEG_HD __host__ __device__ inline
#else
#define SF_JPEG_HD inline
#endif

// On the device every lane of the wave runs the decoder on the same values.  SF_JPEG_UNI marks what comes back from memory as
// wave-uniform (the first lane's value), so the bit buffer, the positions and every branch on them live in scalar registers; on the
// host it is the value itself.
#if defined(__HIP_DEVICE_COMPILE__)
#define SF_JPEG_UNI(x) __builtin_amdgcn_readfirstlane((int)(x))
#else
#define SF_JPEG_UNI(x) ((int)(x))
#endif

namespace sf {

SF_JPEG_HD uint64_t jpeg_uni64(uint64_t x) {
  return ((uint64_t)(uint32_t)SF_JPEG_UNI((uint32_t)(x >> 32)) << 32) | (uint64_t)(uint32_t)SF_JPEG_UNI((uint32_t)x);
}

// zigzag position -> natural (row-major) position
#define SF_JPEG_NATURAL_ORDER                                                                                                      \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

constexpr int JPEG_LOOK_BITS = 9;

// One Huffman table: codes of up to 9 bits resolve in `look` ((length << 8) | symbol, 0: no such code), longer ones through the canonical
// maxcode / value-offset pair of their length.
struct JpegHuff {
  uint16_t look[1 << JPEG_LOOK_BITS];
  int32_t maxcode[17];   // [l]: the largest code of length l, -1 when there is none
  int32_t valoff[17];    // [l]: index of the first value of length l minus its code
  int32_t nvalues;
  uint8_t values[256];
};

// counts[16] / values[] as a DHT segment holds them.  Returns false for counts that are no prefix code (the table is still safe to use).
SF_JPEG_HD bool jpeg_build_huff(const uint8_t *counts, const uint8_t *values, JpegHuff *t) {
  for (int i = 0; i < (1 << JPEG_LOOK_BITS); ++i) t->look[i] = 0;
  int total = 0;
  for (int l = 0; l < 16; ++l) total += counts[l];
  bool ok = total <= 256;
  if (total > 256) total = 256;
  t->nvalues = total;
  for (int i = 0; i < 256; ++i) t->values[i] = i < total ? values[i] : 0;
  int code = 0, k = 0;
  t->maxcode[0] = -1;
  t->valoff[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    t->valoff[l] = k - code;
    int n = counts[l - 1];
    if (k + n > total) n = total - k;
    if (code + n > (1 << l)) {   // more codes than the length holds
      ok = false;
      n = (1 << l) - code;
      if (n < 0) n = 0;
    }
    for (int i = 0; i < n; ++i, ++code, ++k) {
      if (l <= JPEG_LOOK_BITS) {
        const int first = code << (JPEG_LOOK_BITS - l), span = 1 << (JPEG_LOOK_BITS - l);
        for (int j = 0; j < span; ++j) t->look[first + j] = (uint16_t)((l << 8) | t->values[k]);
      }
    }
    t->maxcode[l] = n > 0 ? code - 1 : -1;
    code <<= 1;
  }
  return ok;
}

// MSB-first bit reader over bytes [pos, end) of one segment, with the FF 00 stuffing removed.  It stops at any other FF xx pair.
struct JpegBits {
  const uint8_t *base;
  int64_t lo, hi;        // the buffer: no load outside base[lo .. hi)
  int64_t pos, end;      // the segment; pos: the next byte to take
  uint64_t buf;          // the low `nbits` bits are unread, oldest on top
  int nbits;
  int fake;              // zero bits appended behind the end (or a marker) that are still unread or were read
  bool stopped;          // a marker or the end was met
  uint64_t cache;        // the next `cache_left` bytes from pos on, lowest byte first
  int cache_left;

  SF_JPEG_HD void open(const uint8_t *b, int64_t lo_, int64_t hi_, int64_t begin, int64_t end_) {
    base = b;
    lo = lo_;
    hi = hi_;
    pos = begin < lo_ ? lo_ : begin;
    end = end_ > hi_ ? hi_ : end_;
    buf = 0;
    nbits = 0;
    fake = 0;
    stopped = false;
    cache = 0;
    cache_left = 0;
  }
  // the bytes from pos on (lo <= pos < hi): the rest of the aligned 8-byte word around pos where that word lies inside the buffer, one
  // byte at the buffer's ragged ends
  SF_JPEG_HD void reload() {
    const int off = (int)(reinterpret_cast<uintptr_t>(base + pos) & 7);
    const int64_t w = pos - off;
    if (w >= lo && w + 8 <= hi) {
      cache = jpeg_uni64(*reinterpret_cast<const uint64_t *>(base + w)) >> (8 * off);   // little endian
      cache_left = 8 - off;
    } else {
      cache = (uint64_t)SF_JPEG_UNI(base[pos]);
      cache_left = 1;
    }
  }
  // the next byte of the segment, -1 behind its end
  SF_JPEG_HD int take() {
    if (pos >= end) return -1;
    if (cache_left == 0) reload();
    const int b = (int)(cache & 0xFF);
    cache >>= 8;
    --cache_left;
    ++pos;
    return b;
  }
  SF_JPEG_HD int peek_byte() {
    if (pos >= end) return -1;
    if (cache_left == 0) reload();
    return (int)(cache & 0xFF);
  }
  SF_JPEG_HD void fill() {
    while (nbits <= 56) {
      int b = 0;
      if (!stopped) {
        b = take();
        if (b == 0xFF) {
          if (peek_byte() == 0) {
            (void)take();   // stuffing
          } else {          // a marker (or FF as the last byte): the segment's bits end in front of it
            --pos;
            cache_left = 0;
            b = -1;
          }
        }
        if (b < 0) {
          stopped = true;
          b = 0;
        }
      }
      if (stopped) fake += 8;
      buf = (buf << 8) | (uint64_t)b;
      nbits += 8;
    }
  }
  // at least 32 unread bits: one symbol (<= 16 bits) and its value bits (<= 15)
  SF_JPEG_HD void ensure() {
    if (nbits < 32) fill();
  }
  // n <= 16 <= nbits
  SF_JPEG_HD int peek(int n) const { return (int)((buf >> (nbits - n)) & ((1u << n) - 1u)); }
  SF_JPEG_HD void skip(int n) { nbits -= n; }
  SF_JPEG_HD int get(int n) {
    const int v = peek(n);
    nbits -= n;
    return v;
  }
  SF_JPEG_HD bool starved() const { return nbits < fake; }
  // whole bytes of the segment that no bit was taken from (behind the padding of the last byte read)
  SF_JPEG_HD int64_t bytes_left() const {
    const int real = nbits - fake;   // unread real bits in the buffer
    return (end - pos) + (real > 0 ? real / 8 : 0);
  }
};

// the next symbol, or -1 when no code matches
SF_JPEG_HD int jpeg_decode_symbol(JpegBits &r, const JpegHuff &t) {
  r.ensure();
  const int e = SF_JPEG_UNI(t.look[r.peek(JPEG_LOOK_BITS)]);
  if (e) {
    r.skip(e >> 8);
    return e & 0xFF;
  }
  const int c16 = r.peek(16);
  for (int l = JPEG_LOOK_BITS + 1; l <= 16; ++l) {
    const int c = c16 >> (16 - l);
    if (c <= SF_JPEG_UNI(t.maxcode[l])) {
      const int idx = c + SF_JPEG_UNI(t.valoff[l]);
      if (idx < 0 || idx >= SF_JPEG_UNI(t.nvalues)) return -1;
      r.skip(l);
      return SF_JPEG_UNI(t.values[idx]);
    }
  }
  return -1;
}

SF_JPEG_HD int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One block: `block` holds 64 zeros on entry and the coefficients in natural order on return; *pred is the component's DC predictor;
// `natural`: the 64 entries of SF_JPEG_NATURAL_ORDER (the kernel keeps them in LDS).
// Returns 0 or the SF_JPEG_ST_* code of the first problem (the block may then be partly written).
SF_JPEG_HD int jpeg_decode_block(JpegBits &r, const JpegHuff &dc, const JpegHuff &ac, const uint8_t *natural, int *pred, int16_t *block) {
  int s = jpeg_decode_symbol(r, dc);
  if (s < 0 || s > 15) return SF_JPEG_ST_BAD_CODE;
  if (s) *pred = (int)((unsigned)*pred + (unsigned)jpeg_extend(r.get(s), s));   // wraps (a crafted stream can run it past int range)
  block[0] = (int16_t)(uint16_t)(unsigned)*pred;
  for (int k = 1; k < 64;) {
    const int rs = jpeg_decode_symbol(r, ac);
    if (rs < 0) return SF_JPEG_ST_BAD_CODE;
    const int run = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (run != 15) break;   // end of block
      k += 16;
      continue;
    }
    k += run;
    if (k > 63) return SF_JPEG_ST_INDEX_OVERFLOW;
    block[SF_JPEG_UNI(natural[k]) & 63] = (int16_t)jpeg_extend(r.get(s), s);
    ++k;
  }
  return r.starved() ? SF_JPEG_ST_OUT_OF_BITS : 0;
}

// ---- geometry of a descriptor (the fields the parser filled) -----------------------------------------------------------------------------
SF_JPEG_HD int jpeg_blocks_w(const sf_jpeg_desc &d, int c) { return d.mcus_x * d.h[c]; }
SF_JPEG_HD int jpeg_blocks_h(const sf_jpeg_desc &d, int c) { return d.mcus_y * d.v[c]; }
SF_JPEG_HD int64_t jpeg_comp_blocks(const sf_jpeg_desc &d, int c) { return (int64_t)jpeg_blocks_w(d, c) * jpeg_blocks_h(d, c); }
SF_JPEG_HD int64_t jpeg_image_blocks(const sf_jpeg_desc &d) {
  int64_t n = 0;
  for (int c = 0; c < d.ncomp; ++c) n += jpeg_comp_blocks(d, c);
  return n;
}

}  // namespace sf
