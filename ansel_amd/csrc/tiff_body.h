// tiff_body.h -- the body of the TIFF encoder (tiff.hip) that is written once and compiled twice, as png_deflate.h is
// for PNG: the strips' payload bytes (the predictors), the geometry and its refusals, and the file's head.  The
// kernels call the payload functions from their threads; tests/native/tiff_host.cpp runs them on the host and deflates
// every strip with the host build of png_deflate.h, so the CPU suite checks the file against libtiff and the device
// file equals the host build's.
//
// The file: little-endian classic TIFF (BigTIFF is not written: every offset is 32 bits, and a file whose bound does
// not fit is refused).  `II*\0`, the IFD at offset 8, then the out-of-line values in tag order, then the strips; every
// out-of-line value and every strip starts on an even offset (one zero byte of padding where needed), and the file
// ends with the last strip's last byte.  StripOffsets and StripByteCounts are LONG; with deflate their slots are left
// empty here and filled on the device.
#pragma once
#include <stdint.h>

#include "ansel_hip.h"
#include "png_deflate.h"

// ---------------------------------------------------------------------------------------------------------------------
// payload

// sample i (0 .. w * layers - 1) of row y of RGBA samples of type T: channel i % layers of pixel i / layers, with
// predictor 2 its difference modulo 2^bits from the same channel of the pixel to the left
template <class T>
PD_FN T tf_sample(const T *in, int w, int layers, int predictor, int y, uint32_t i)
{
  const uint32_t px = i / (uint32_t)layers, c = i - px * (uint32_t)layers;
  const T *p = in + ((size_t)y * w + px) * 4 + c;
  return (predictor == 2 && px > 0) ? (T)(p[0] - p[-4]) : p[0];
}

// predictor 3: byte j (0 .. 4 n - 1, n = w * layers samples) of a row whose sample i has the bits bits(i): the
// samples' big-endian bytes regrouped into four planes, the most significant first, then every byte j >= layers
// replaced by its difference modulo 256 from byte j - layers
template <class Bits>
PD_FN uint32_t tf_fp_byte(uint32_t n, int layers, uint32_t j, Bits bits)
{
  const uint32_t b = j / n, i = j - b * n;
  const uint32_t cur = (bits(i) >> (24 - 8 * b)) & 255;
  if(j < (uint32_t)layers) return cur;
  const uint32_t jp = j - (uint32_t)layers, bp = jp / n, ip = jp - bp * n;
  return (cur - ((bits(ip) >> (24 - 8 * bp)) & 255)) & 255;
}

// the bits of sample i of row y of RGBA f32
PD_FN uint32_t tf_float_bits(const uint32_t *in, int w, int layers, int y, uint32_t i)
{
  const uint32_t px = i / (uint32_t)layers, c = i - px * (uint32_t)layers;
  return in[((size_t)y * w + px) * 4 + c];
}

PD_FN uint64_t tf_align2(uint64_t v) { return (v + 1) & ~(uint64_t)1; }

// the most a strip of n payload bytes takes as a zlib stream: header, stored blocks with the worst padding, Adler-32
PD_FN uint64_t tf_zmax(uint64_t n) { return 2 + (42 * ((n + PD_SEG - 1) / PD_SEG) + 7) / 8 + n + 4; }

// ---------------------------------------------------------------------------------------------------------------------
// geometry and head (host)

#include <vector>

struct tf_geom_t
{
  uint32_t row_bytes;
  uint32_t rps;         // the RowsPerStrip tag (may exceed the frame's rows)
  uint32_t nstrips;
  uint64_t strip_bytes; // payload of every strip but the last
  uint64_t last_bytes;  // payload of the last strip
  uint64_t sps;         // segments of a full strip
  uint64_t nseg;        // segments of all strips
  uint32_t head_bytes;  // IFD and out-of-line values
  uint32_t data_start;  // the first strip's offset (even)
  uint32_t pos_offsets, pos_counts; // where the StripOffsets / StripByteCounts values stand
  uint64_t bound;       // 8 + the file at most (the file exactly without compression)
};

// libtiff's TIFFDefaultStripSize(tif, 0): about 8 KB of rows, at least one
inline uint32_t tf_default_rows(uint64_t row_bytes) { return row_bytes >= 8192 ? 1 : (uint32_t)(8192 / row_bytes); }

// why the settings are refused, or nullptr
inline const char *tf_refusal(int width, int height, const dt_hip_tiff_data_t *d)
{
  if(!d) return "no dt_hip_tiff_data_t";
  if(width < 1 || height < 1) return "width or height below 1";
  if(d->bpp != 8 && d->bpp != 16 && d->bpp != 32) return "bpp is not 8, 16 or 32";
  if(d->layers != 3 && d->layers != 1) return "layers is not 3 or 1";
  if(d->compression != DT_HIP_TIFF_NONE && d->compression != DT_HIP_TIFF_DEFLATE) return "compression is not 1 (none) or 8 (deflate)";
  if(d->predictor < 1 || d->predictor > 3) return "predictor is not 1, 2 or 3";
  if(d->predictor == 2 && d->bpp == 32) return "predictor 2 (horizontal) belongs to 8 and 16 bits";
  if(d->predictor == 3 && d->bpp != 32) return "predictor 3 (floating point) belongs to 32 bits";
  if(d->predictor != 1 && d->compression != DT_HIP_TIFF_DEFLATE) return "a predictor other than 1 needs deflate";
  if(d->compression_level < 0 || d->compression_level > 9) return "compression level outside 0..9";
  if(d->rows_per_strip < 0) return "rows_per_strip is negative";
  if(d->dpi < 0) return "dpi is negative";
  if(d->icc_bytes && !d->icc) return "icc_bytes without an icc pointer";
  if(d->icc && d->icc_bytes > 0xffffffffull) return "the ICC profile does not fit a classic TIFF";
  return nullptr;
}

inline void tf_le(std::vector<uint8_t> &o, uint64_t v, int n)
{
  for(int k = 0; k < n; k++) o.push_back((uint8_t)(v >> (8 * k)));
}

// the sizes and, when head is given, the file's first head_bytes bytes (rounded up to data_start with a zero);
// without compression the strips' offsets and byte counts are in it.  Returns why not, or nullptr
inline const char *tf_geometry(int width, int height, const dt_hip_tiff_data_t *d, tf_geom_t *g, std::vector<uint8_t> *head)
{
  if(const char *why = tf_refusal(width, height, d)) return why;
  const uint64_t too_big = 0xffffffffull;
  const uint64_t rb = (uint64_t)width * d->layers * (d->bpp / 8);
  if(rb > too_big) return "the file does not fit 32-bit offsets (classic TIFF only)";
  const uint32_t rps = d->rows_per_strip ? (uint32_t)d->rows_per_strip : tf_default_rows(rb);
  const uint32_t rows = rps < (uint32_t)height ? rps : (uint32_t)height; // rows of a full strip
  const uint32_t nstrips = (uint32_t)(((uint64_t)height + rows - 1) / rows);
  if((unsigned __int128)rb * height > too_big) return "the file does not fit 32-bit offsets (classic TIFF only)";
  const bool deflate = d->compression == DT_HIP_TIFF_DEFLATE;
  const uint64_t icc_bytes = d->icc ? d->icc_bytes : 0;
  g->row_bytes = (uint32_t)rb;
  g->rps = rps;
  g->nstrips = nstrips;
  g->strip_bytes = rb * rows;
  g->last_bytes = rb * ((uint64_t)height - (uint64_t)(nstrips - 1) * rows);
  g->sps = (g->strip_bytes + PD_SEG - 1) / PD_SEG;
  g->nseg = (uint64_t)(nstrips - 1) * g->sps + (g->last_bytes + PD_SEG - 1) / PD_SEG;
  if(g->nseg > 0x7fffffff) return "more strips than a launch has workgroups";

  // the IFD's entries: tag, type (3 SHORT, 4 LONG, 5 RATIONAL, 7 UNDEFINED), count, value bytes
  struct entry_t
  {
    uint32_t tag, type, count;
    std::vector<uint8_t> v;
  };
  std::vector<entry_t> e;
  auto shorts = [&](uint32_t tag, uint32_t count, uint32_t value) {
    entry_t x = { tag, 3, count, {} };
    for(uint32_t k = 0; k < count; k++) tf_le(x.v, value, 2);
    e.push_back(x);
  };
  auto longs = [&](uint32_t tag, uint64_t count, uint32_t value) { // an array of `count` slots: filled later
    entry_t x = { tag, 4, (uint32_t)count, {} };
    if(head || count == 1)
      for(uint64_t k = 0; k < count; k++) tf_le(x.v, value, 4);
    e.push_back(x);
  };
  const uint64_t array_bytes = 4 * (uint64_t)nstrips; // sizes only: the vectors stay empty without `head`
  longs(256, 1, (uint32_t)width);
  longs(257, 1, (uint32_t)height);
  shorts(258, (uint32_t)d->layers, (uint32_t)d->bpp);
  shorts(259, 1, (uint32_t)d->compression);
  shorts(262, 1, d->layers == 3 ? 2 : 1);
  longs(273, nstrips, 0);
  shorts(274, 1, 1);
  shorts(277, 1, (uint32_t)d->layers);
  longs(278, 1, rps);
  longs(279, nstrips, 0);
  if(d->dpi > 0)
    for(uint32_t tag = 282; tag <= 283; tag++)
    {
      entry_t x = { tag, 5, 1, {} };
      tf_le(x.v, (uint32_t)d->dpi, 4);
      tf_le(x.v, 1, 4);
      e.push_back(x);
    }
  shorts(284, 1, 1);
  if(d->dpi > 0) shorts(296, 1, 2);
  if(d->predictor != 1) shorts(317, 1, (uint32_t)d->predictor);
  shorts(339, (uint32_t)d->layers, d->bpp == 32 ? 3 : 1);
  if(icc_bytes)
  {
    entry_t x = { 34675, 7, (uint32_t)icc_bytes, {} };
    if(head) x.v.assign((const uint8_t *)d->icc, (const uint8_t *)d->icc + icc_bytes);
    e.push_back(x);
  }
  auto bytes_of = [&](const entry_t &x) -> uint64_t {
    return (x.tag == 273 || x.tag == 279) ? array_bytes : x.tag == 34675 ? icc_bytes : x.v.size();
  };
  // positions: the IFD, then every value of more than 4 bytes on the next even offset
  uint64_t at = 8 + 2 + 12 * (uint64_t)e.size() + 4;
  std::vector<uint64_t> where(e.size());
  for(size_t k = 0; k < e.size(); k++)
  {
    if(bytes_of(e[k]) <= 4)
    {
      where[k] = 8 + 2 + 12 * k + 8;
      continue;
    }
    at = tf_align2(at);
    where[k] = at;
    at += bytes_of(e[k]);
  }
  const uint64_t data_start = tf_align2(at);
  const uint64_t data = deflate ? (uint64_t)(nstrips - 1) * tf_align2(tf_zmax(g->strip_bytes)) + tf_zmax(g->last_bytes)
                                : (uint64_t)(nstrips - 1) * tf_align2(g->strip_bytes) + g->last_bytes;
  if((unsigned __int128)data_start + data > too_big) return "the file does not fit 32-bit offsets (classic TIFF only)";
  g->head_bytes = (uint32_t)at;
  g->data_start = (uint32_t)data_start;
  g->bound = 8 + data_start + data;
  for(size_t k = 0; k < e.size(); k++)
  {
    if(e[k].tag == 273) g->pos_offsets = (uint32_t)where[k];
    if(e[k].tag == 279) g->pos_counts = (uint32_t)where[k];
  }
  if(!head) return nullptr;
  std::vector<uint8_t> &o = *head;
  o.assign((size_t)data_start, 0);
  const uint8_t magic[8] = { 'I', 'I', 42, 0, 8, 0, 0, 0 };
  for(int k = 0; k < 8; k++) o[k] = magic[k];
  o[8] = (uint8_t)e.size();
  o[9] = (uint8_t)(e.size() >> 8);
  for(size_t k = 0; k < e.size(); k++)
  {
    uint8_t *p = o.data() + 10 + 12 * k;
    const uint32_t f[3] = { e[k].tag, e[k].type, e[k].count };
    p[0] = (uint8_t)f[0], p[1] = (uint8_t)(f[0] >> 8), p[2] = (uint8_t)f[1], p[3] = 0;
    for(int b = 0; b < 4; b++) p[4 + b] = (uint8_t)(f[2] >> (8 * b));
    if(e[k].v.size() <= 4)
      for(size_t b = 0; b < e[k].v.size(); b++) p[8 + b] = e[k].v[b];
    else
    {
      for(int b = 0; b < 4; b++) p[8 + b] = (uint8_t)(where[k] >> (8 * b));
      for(size_t b = 0; b < e[k].v.size(); b++) o[(size_t)where[k] + b] = e[k].v[b];
    }
  }
  if(!deflate)
    for(uint32_t s = 0; s < nstrips; s++)
    {
      const uint64_t off = data_start + (uint64_t)s * tf_align2(g->strip_bytes);
      const uint64_t cnt = s + 1 == nstrips ? g->last_bytes : g->strip_bytes;
      for(int b = 0; b < 4; b++)
      {
        o[(size_t)g->pos_offsets + 4 * s + b] = (uint8_t)(off >> (8 * b));
        o[(size_t)g->pos_counts + 4 * s + b] = (uint8_t)(cnt >> (8 * b));
      }
    }
  return nullptr;
}
