// JPEG marker parser behind sf_jpeg_parse: plain C++ (no HIP), every read bounds-checked against the file's own byte range.
// One call per file fills its sf_jpeg_desc; jpeg_fill_segments() then writes the file's entries of the segment table.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "jpeg_decode.h"

namespace sf {

namespace jpeg_detail {

struct Cursor {
  const uint8_t *p;
  int64_t pos, end;
  bool have(int64_t n) const { return n >= 0 && end - pos >= n; }
  int u8() { return p[pos++]; }
  int u16() {
    const int v = (p[pos] << 8) | p[pos + 1];
    pos += 2;
    return v;
  }
};

inline int verdict(sf_jpeg_desc *d, int status, const char *fmt, int a = 0, int b = 0) {
  if (d->status == SF_JPEG_MALFORMED) return d->status;                             // the first defect stays
  if (d->status == SF_JPEG_UNSUPPORTED && status == SF_JPEG_UNSUPPORTED) return d->status;   // and the first reason
  d->status = status;
  snprintf(d->reason, sizeof(d->reason), fmt, a, b);
  return status;
}

}  // namespace jpeg_detail

// Parses file bytes[begin .. end).  Returns desc->status.  Geometry fields are complete whenever a frame header was read.
inline int jpeg_parse_one(const uint8_t *bytes, int64_t begin, int64_t end, sf_jpeg_desc *d) {
  using namespace jpeg_detail;
  const uint8_t natural[64] = SF_JPEG_NATURAL_ORDER;
  memset(d, 0, sizeof(*d));
  for (int i = 0; i < 4; ++i) d->quant_precision[i] = -1;
  Cursor c{bytes, begin, end};
  if (!c.have(2) || c.u8() != 0xFF || c.u8() != 0xD8) return verdict(d, SF_JPEG_MALFORMED, "no SOI marker");
  bool have_frame = false, have_scan = false, jfif = false;
  int adobe_transform = -1, comp_id[3] = {0, 0, 0};
  while (!have_scan) {
    // the next marker: FF, any number of FF fill bytes, a code
    if (!c.have(2)) return verdict(d, SF_JPEG_MALFORMED, "truncated before the scan");
    if (c.u8() != 0xFF) return verdict(d, SF_JPEG_MALFORMED, "marker expected");
    int m = c.u8();
    while (m == 0xFF) {
      if (!c.have(1)) return verdict(d, SF_JPEG_MALFORMED, "truncated before the scan");
      m = c.u8();
    }
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // TEM, stray RSTn: no length
    if (m == 0xD9) return verdict(d, SF_JPEG_MALFORMED, "EOI before any scan");
    if (m == 0xD8 || m == 0x00) return verdict(d, SF_JPEG_MALFORMED, "unexpected marker FF%02X", m);
    if (!c.have(2)) return verdict(d, SF_JPEG_MALFORMED, "truncated marker FF%02X", m);
    const int len = c.u16();
    if (len < 2 || !c.have(len - 2)) return verdict(d, SF_JPEG_MALFORMED, "marker FF%02X: length %d outside the file", m, len);
    Cursor s{bytes, c.pos, c.pos + len - 2};   // this segment's payload
    c.pos += len - 2;
    if (m == 0xDB) {   // DQT
      while (s.have(1)) {
        const int pq = s.u8(), prec = pq >> 4, id = pq & 15;
        if (prec > 1 || id > 3) return verdict(d, SF_JPEG_MALFORMED, "DQT: precision %d / table %d", prec, id);
        if (!s.have(prec ? 128 : 64)) return verdict(d, SF_JPEG_MALFORMED, "DQT: table %d truncated", id);
        for (int k = 0; k < 64; ++k) d->quant[id][natural[k]] = (uint16_t)(prec ? s.u16() : s.u8());
        d->quant_precision[id] = prec;
      }
    } else if (m == 0xC4) {   // DHT
      while (s.have(1)) {
        const int tc = s.u8(), cls = tc >> 4, id = tc & 15;
        if (cls > 1 || id > 3) return verdict(d, SF_JPEG_MALFORMED, "DHT: class %d / table %d", cls, id);
        if (!s.have(16)) return verdict(d, SF_JPEG_MALFORMED, "DHT: truncated");
        uint8_t counts[16];
        int total = 0, code = 0;
        bool prefix = true;
        for (int l = 0; l < 16; ++l) {
          counts[l] = (uint8_t)s.u8();
          total += counts[l];
          code += counts[l];
          if (code > (1 << (l + 1))) prefix = false;
          code <<= 1;
        }
        if (total > 256 || !prefix || !s.have(total)) return verdict(d, SF_JPEG_MALFORMED, "DHT: table %d is no prefix code or is truncated", id);
        if (id > 1) {   // (kept out of the descriptor: it holds two tables per class)
          verdict(d, SF_JPEG_UNSUPPORTED, "Huffman table id %d (above 1)", id);
          s.pos += total;
          continue;
        }
        const int slot = cls * 2 + id;
        memcpy(d->huff_counts[slot], counts, 16);
        memset(d->huff_values[slot], 0, 256);
        for (int k = 0; k < total; ++k) d->huff_values[slot][k] = (uint8_t)s.u8();
        if (cls == 0)
          for (int k = 0; k < total; ++k)
            if (d->huff_values[slot][k] > 15) return verdict(d, SF_JPEG_MALFORMED, "DHT: DC table %d holds category %d", id, d->huff_values[slot][k]);
        d->huff_present |= 1 << slot;
      }
    } else if (m == 0xDD) {   // DRI
      if (!s.have(2)) return verdict(d, SF_JPEG_MALFORMED, "DRI: truncated");
      d->restart_interval = s.u16();
    } else if (m == 0xE0) {   // APP0
      if (s.have(5) && memcmp(bytes + s.pos, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {   // APP14
      if (s.have(12) && memcmp(bytes + s.pos, "Adobe", 5) == 0) adobe_transform = bytes[s.pos + 11];
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {   // SOFn
      if (have_frame) return verdict(d, SF_JPEG_MALFORMED, "two frame headers");
      if (!s.have(6)) return verdict(d, SF_JPEG_MALFORMED, "SOF: truncated");
      const int prec = s.u8();
      d->height = s.u16();
      d->width = s.u16();
      const int nc = s.u8();
      d->ncomp = nc;
      have_frame = true;
      if (d->width < 1 || d->height < 1 || nc < 1 || !s.have(3 * (int64_t)nc)) return verdict(d, SF_JPEG_MALFORMED, "SOF: %d x %d, bad size or truncated", d->width, d->height);
      if (m == 0xC2) verdict(d, SF_JPEG_UNSUPPORTED, "progressive frame (SOF2)");
      else if (m >= 0xC9) verdict(d, SF_JPEG_UNSUPPORTED, "arithmetic-coded frame (SOF%d)", m - 0xC0);
      else if (m != 0xC0 && m != 0xC1) verdict(d, SF_JPEG_UNSUPPORTED, "SOF%d frame (lossless / hierarchical)", m - 0xC0);
      if (prec != 8) verdict(d, SF_JPEG_UNSUPPORTED, "%d-bit samples", prec);
      if (nc != 1 && nc != 3) {
        verdict(d, SF_JPEG_UNSUPPORTED, "%d components", nc);   // (no per-component field is filled)
        continue;
      }
      for (int i = 0; i < nc; ++i) {
        comp_id[i] = s.u8();
        const int hv = s.u8();
        d->h[i] = hv >> 4;
        d->v[i] = hv & 15;
        d->tq[i] = s.u8();
        if (d->h[i] < 1 || d->h[i] > 4 || d->v[i] < 1 || d->v[i] > 4 || d->tq[i] > 3) return verdict(d, SF_JPEG_MALFORMED, "SOF: component %d: bad sampling or table", i);
      }
      if (nc == 1) d->h[0] = d->v[0] = 1;   // a one-component scan is never interleaved: its MCU is one block
      else if (!(d->h[1] == 1 && d->v[1] == 1 && d->h[2] == 1 && d->v[2] == 1 && ((d->h[0] == 1 && d->v[0] == 1) || (d->h[0] == 2 && d->v[0] <= 2))))
        verdict(d, SF_JPEG_UNSUPPORTED, "sampling %dx%d luma with other than 1x1 / 2x1 / 2x2 over 1x1 chroma", d->h[0], d->v[0]);
      if (nc == 3 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') verdict(d, SF_JPEG_UNSUPPORTED, "component ids R G B (not YCbCr)");
      const int hmax = d->h[0], vmax = d->v[0];   // (supported layouts: luma carries the maxima)
      d->mcus_x = (d->width + 8 * hmax - 1) / (8 * hmax);
      d->mcus_y = (d->height + 8 * vmax - 1) / (8 * vmax);
    } else if (m == 0xDA) {   // SOS
      if (!have_frame) return verdict(d, SF_JPEG_MALFORMED, "scan before the frame header");
      if (!s.have(1)) return verdict(d, SF_JPEG_MALFORMED, "SOS: truncated");
      const int ns = s.u8();
      if (ns < 1 || ns > 4 || !s.have(2 * (int64_t)ns + 3)) return verdict(d, SF_JPEG_MALFORMED, "SOS: %d components or truncated", ns);
      have_scan = true;
      d->data_begin = c.pos;
      if (d->ncomp != 1 && d->ncomp != 3) break;
      if (ns != d->ncomp) {
        verdict(d, SF_JPEG_UNSUPPORTED, "several scans (%d of %d components in the first)", ns, d->ncomp);
        break;
      }
      for (int i = 0; i < ns; ++i) {
        const int id = s.u8(), t = s.u8();
        if (id != comp_id[i]) verdict(d, SF_JPEG_UNSUPPORTED, "scan components out of frame order");
        d->td[i] = t >> 4;
        d->ta[i] = t & 15;
        if (d->td[i] > 3 || d->ta[i] > 3) return verdict(d, SF_JPEG_MALFORMED, "SOS: table selector above 3");
        if (d->td[i] > 1 || d->ta[i] > 1) verdict(d, SF_JPEG_UNSUPPORTED, "Huffman table id above 1");
      }
      const int ss = s.u8(), se = s.u8(), ahal = s.u8();
      if (d->status == SF_JPEG_OK && (ss != 0 || se != 63 || ahal != 0)) verdict(d, SF_JPEG_UNSUPPORTED, "spectral selection / successive approximation in a sequential frame");
    }
    // every other marker (APPn, COM, DNL, ...) is skipped by its length
  }
  if (adobe_transform >= 0 && adobe_transform != 1 && d->ncomp == 3) verdict(d, SF_JPEG_UNSUPPORTED, "Adobe marker with transform %d", adobe_transform);
  (void)jfif;
  // the end of the entropy-coded data: the first marker that is neither stuffing nor RSTn
  int64_t q = d->data_begin;
  d->data_end = end;
  bool eoi = false;
  while (q < end) {
    const void *f = memchr(bytes + q, 0xFF, (size_t)(end - q));
    if (!f) break;
    q = static_cast<const uint8_t *>(f) - bytes;
    if (q + 1 >= end) break;   // FF as the last byte: data to the end, the decoder stops there
    const int m = bytes[q + 1];
    if (m == 0x00 || (m >= 0xD0 && m <= 0xD7)) {
      q += 2;
      continue;
    }
    if (m == 0xFF) {   // a fill byte: the pair that counts starts at the next FF (the decoder stops at the fill byte and flags the rest)
      q += 1;
      continue;
    }
    d->data_end = q;
    eoi = m == 0xD9;
    break;
  }
  if (d->status == SF_JPEG_OK && d->data_end < end && !eoi) verdict(d, SF_JPEG_UNSUPPORTED, "several scans (marker FF%02X behind the first)", bytes[d->data_end + 1]);
  if (d->status != SF_JPEG_OK) return d->status;
  // tables the scan selects must exist
  for (int i = 0; i < d->ncomp; ++i) {
    if (d->quant_precision[d->tq[i]] < 0) return verdict(d, SF_JPEG_MALFORMED, "component %d: quantisation table %d missing", i, d->tq[i]);
    if (!(d->huff_present & (1 << d->td[i]))) return verdict(d, SF_JPEG_MALFORMED, "component %d: DC table %d missing", i, d->td[i]);
    if (!(d->huff_present & (4 << d->ta[i]))) return verdict(d, SF_JPEG_MALFORMED, "component %d: AC table %d missing", i, d->ta[i]);
  }
  if ((int64_t)d->mcus_x * d->mcus_y > (int64_t)1 << 30) return verdict(d, SF_JPEG_UNSUPPORTED, "frame of more than 2^30 MCUs");
  const int64_t mcus = (int64_t)d->mcus_x * d->mcus_y;
  d->seg_count = d->restart_interval > 0 ? (int32_t)((mcus + d->restart_interval - 1) / d->restart_interval) : 1;
  return d->status;
}

// The d->seg_count entries of file `image` (status SF_JPEG_OK): RSTn markers by a byte scan of [data_begin, data_end).
inline void jpeg_fill_segments(const uint8_t *bytes, const sf_jpeg_desc *d, int image, sf_jpeg_segment *out) {
  const int64_t mcus = (int64_t)d->mcus_x * d->mcus_y;
  const int64_t ri = d->restart_interval > 0 ? d->restart_interval : mcus;
  int64_t q = d->data_begin;
  for (int s = 0; s < d->seg_count; ++s) {
    sf_jpeg_segment &g = out[s];
    g.image = image;
    g.first_mcu = (int32_t)(s * ri);
    g.mcu_count = (int32_t)((mcus - s * ri) < ri ? (mcus - s * ri) : ri);
    g.reserved = 0;
    g.byte_begin = q;
    g.byte_end = d->data_end;
    if (s + 1 == d->seg_count) break;   // the last one runs to the end of the data, whatever markers it holds
    int64_t k = q;
    while (k < d->data_end) {   // the next RSTn
      const void *f = memchr(bytes + k, 0xFF, (size_t)(d->data_end - k));
      if (!f) {
        k = d->data_end;
        break;
      }
      k = static_cast<const uint8_t *>(f) - bytes;
      if (k + 1 < d->data_end && bytes[k + 1] >= 0xD0 && bytes[k + 1] <= 0xD7) break;
      k += (k + 1 < d->data_end && bytes[k + 1] == 0x00) ? 2 : 1;
    }
    if (k >= d->data_end) {   // fewer markers than the header promises: the remaining segments are empty (the decoder flags them)
      g.byte_end = d->data_end;
      q = d->data_end;
    } else {
      g.byte_end = k;
      q = k + 2;
    }
  }
}

// One segment on the host, block after block as the entropy kernel walks it (the same reader and block decoder): coefficients
// into `coef` (the file's blocks, zeroed by the caller).  Returns 0 or the SF_JPEG_ST_* code of the first problem.
inline int jpeg_decode_segment_host(const uint8_t *bytes, int64_t n_bytes, const sf_jpeg_desc &d, const sf_jpeg_segment &g, int16_t *coef) {
  const int64_t mcus = (int64_t)d.mcus_x * d.mcus_y, image_blocks = jpeg_image_blocks(d);
  if (g.first_mcu < 0 || g.mcu_count < 0 || (int64_t)g.first_mcu + g.mcu_count > mcus || g.byte_begin < 0 || g.byte_begin > g.byte_end || g.byte_end > n_bytes)
    return SF_JPEG_ST_BAD_SEGMENT;
  const uint8_t natural[64] = SF_JPEG_NATURAL_ORDER;
  JpegHuff tabs[4];
  for (int t = 0; t < 4; ++t) jpeg_build_huff(d.huff_counts[t], d.huff_values[t], &tabs[t]);
  JpegBits r;
  r.open(bytes, 0, n_bytes, g.byte_begin, g.byte_end);
  int pred[3] = {0, 0, 0};
  for (int m = g.first_mcu; m < g.first_mcu + g.mcu_count; ++m) {
    const int my = m / d.mcus_x, mx = m - my * d.mcus_x;
    int64_t comp_base = 0;
    for (int c = 0; c < d.ncomp; ++c) {
      const int ch = d.h[c], cv = d.v[c], bw = d.mcus_x * ch;
      for (int v = 0; v < cv; ++v)
        for (int h = 0; h < ch; ++h) {
          int16_t block[64] = {0};
          const int e = jpeg_decode_block(r, tabs[d.td[c]], tabs[2 + d.ta[c]], natural, &pred[c], block);
          if (e) return e;
          const int64_t slot = comp_base + (int64_t)(my * cv + v) * bw + mx * ch + h;
          if (slot < image_blocks) memcpy(coef + slot * 64, block, sizeof(block));
        }
      comp_base += (int64_t)bw * d.mcus_y * cv;
    }
  }
  return r.bytes_left() > 0 ? SF_JPEG_ST_TRAILING_BYTES : 0;
}

// bytes of workspace areas one file takes (0 unless SF_JPEG_OK)
inline int64_t jpeg_coef_elems(const sf_jpeg_desc &d) { return d.status == SF_JPEG_OK ? jpeg_image_blocks(d) * 64 : 0; }
inline int64_t jpeg_plane_bytes(const sf_jpeg_desc &d) { return jpeg_coef_elems(d); }

}  // namespace sf
