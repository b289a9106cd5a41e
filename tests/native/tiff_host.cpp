// tests/native/tiff_host.cpp -- TEST INFRASTRUCTURE: the TIFF encoder's body (ansel_amd/csrc/tiff_body.h and
// png_deflate.h, run by the kernels of tiff.hip on gfx950) compiled for the host and run one step after the other: the
// same payload bytes, geometry and head, and every strip deflated on its own by the host build of the deflate
// (png_host.cpp's zlib_stream(), which sees nothing but the strip it is given).  tests/test_tiff_host.py checks its file
// against libtiff and zlib; tests/test_gpu_tiff.py checks that the device's file equals it byte for byte.
//
//   g++ -O2 -std=c++17 -fPIC -shared -I ansel_amd/csrc -I include tests/native/tiff_host.cpp -o libtiff_host.so
//
// With -DTIFF_HOST_MAIN it is a program of its own (for -fsanitize=address,undefined): it encodes a corpus of small
// frames in every format and checks the layout of each file.
#include "png_host.cpp" // the host deflate of one stream: zlib_stream()

#include "tiff_body.h"

namespace
{

std::vector<uint8_t> g_tiff;

// the payload of all rows, one after the other (the strips are runs of whole rows)
std::vector<uint8_t> payload(const void *in, int w, int h, const dt_hip_tiff_data_t *d, const tf_geom_t &g)
{
  std::vector<uint8_t> p((size_t)g.row_bytes * h);
  const uint32_t n = (uint32_t)w * d->layers;
  for(int y = 0; y < h; y++)
  {
    uint8_t *o = p.data() + (size_t)y * g.row_bytes;
    if(d->predictor == 3)
    {
      for(uint32_t j = 0; j < 4 * n; j++)
        o[j] = (uint8_t)tf_fp_byte(n, d->layers, j, [&](uint32_t i) { return tf_float_bits((const uint32_t *)in, w, d->layers, y, i); });
      continue;
    }
    for(uint32_t i = 0; i < n; i++)
    {
      if(d->bpp == 8) o[i] = tf_sample<uint8_t>((const uint8_t *)in, w, d->layers, d->predictor, y, i);
      if(d->bpp == 16)
      {
        const uint16_t v = tf_sample<uint16_t>((const uint16_t *)in, w, d->layers, d->predictor, y, i);
        memcpy(o + 2 * i, &v, 2);
      }
      if(d->bpp == 32)
      {
        const uint32_t v = tf_sample<uint32_t>((const uint32_t *)in, w, d->layers, d->predictor, y, i);
        memcpy(o + 4 * i, &v, 4);
      }
    }
  }
  return p;
}

void le32(std::vector<uint8_t> &o, size_t at, uint64_t v)
{
  for(int b = 0; b < 4; b++) o[at + b] = (uint8_t)(v >> (8 * b));
}

uint64_t get32(const std::vector<uint8_t> &o, size_t at)
{
  return (uint64_t)o[at] | ((uint64_t)o[at + 1] << 8) | ((uint64_t)o[at + 2] << 16) | ((uint64_t)o[at + 3] << 24);
}

bool encode(const void *in, int w, int h, const dt_hip_tiff_data_t *d, std::vector<uint8_t> &o)
{
  tf_geom_t g;
  if(tf_geometry(w, h, d, &g, &o)) return false;
  const std::vector<uint8_t> p = payload(in, w, h, d, g);
  for(uint32_t s = 0; s < g.nstrips; s++)
  {
    const uint8_t *b = p.data() + (size_t)s * g.strip_bytes;
    const size_t n = (size_t)(s + 1 == g.nstrips ? g.last_bytes : g.strip_bytes);
    if(o.size() & 1) o.push_back(0);
    if(d->compression == DT_HIP_TIFF_NONE)
    {
      if(get32(o, g.pos_offsets + 4 * s) != o.size() || get32(o, g.pos_counts + 4 * s) != n) return false;
      o.insert(o.end(), b, b + n);
      continue;
    }
    const std::vector<uint8_t> z = zlib_stream(std::vector<uint8_t>(b, b + n), d->compression_level);
    if(z.empty() || z.size() > tf_zmax(n)) return false;
    le32(o, g.pos_offsets + 4 * s, o.size());
    le32(o, g.pos_counts + 4 * s, z.size());
    o.insert(o.end(), z.begin(), z.end());
  }
  return 8 + o.size() <= g.bound;
}

} // namespace

// the strips' payload, h * row bytes; returns the byte count (0: refused)
extern "C" size_t tiff_host_payload(const void *in, int w, int h, const dt_hip_tiff_data_t *d, uint8_t *out)
{
  tf_geom_t g;
  if(tf_geometry(w, h, d, &g, nullptr)) return 0;
  const std::vector<uint8_t> p = payload(in, w, h, d, g);
  if(out) memcpy(out, p.data(), p.size());
  return p.size();
}

// the whole file; returns its length (0: refused, or the host build disagrees with itself), tiff_host_copy() fetches it
extern "C" size_t tiff_host_encode(const void *in, int w, int h, const dt_hip_tiff_data_t *d)
{
  std::vector<uint8_t> o;
  if(!encode(in, w, h, d, o)) return 0;
  g_tiff = o;
  return o.size();
}

extern "C" void tiff_host_copy(uint8_t *out) { memcpy(out, g_tiff.data(), g_tiff.size()); }

// 8 + the most the file takes (0: refused), computed as dt_hip_tiff_bound() does
extern "C" size_t tiff_host_bound(int w, int h, const dt_hip_tiff_data_t *d)
{
  tf_geom_t g;
  return tf_geometry(w, h, d, &g, nullptr) ? 0 : (size_t)g.bound;
}

#ifdef TIFF_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

// every format over small frames (strips of one and of several segments, one sample wide, odd strips, ICC and dpi):
// each file must encode, lie inside its bound and have ascending, even, non-overlapping strips that end at L
int main()
{
  const int sizes[][3] = { { 1, 1, 5 }, { 1, 5, 5 }, { 2, 1, 5 }, { 37, 13, 5 }, { 37, 13, 100 }, { 37, 13, 1 }, { 3, 130, 1 },
                           { 10923, 3, 1 }, { 2000, 16, 7 }, { 300, 40, 0 } };
  std::vector<uint8_t> icc(2001, 0x5a);
  int files = 0;
  for(const auto &sz : sizes)
    for(int bpp : { 8, 16, 32 })
      for(int layers : { 3, 1 })
        for(int variant = 0; variant < 7; variant++)
        {
          const int w = sz[0], h = sz[1];
          dt_hip_tiff_data_t d = {};
          d.bpp = bpp;
          d.layers = layers;
          d.compression = variant == 0 ? DT_HIP_TIFF_NONE : DT_HIP_TIFF_DEFLATE;
          d.predictor = (variant == 0 || (variant & 1)) ? 1 : (bpp == 32 ? 3 : 2);
          d.compression_level = variant < 3 ? 0 : variant < 5 ? 1 : 6;
          d.rows_per_strip = sz[2];
          d.dpi = variant == 2 ? 300 : 0;
          if(variant >= 5)
          {
            d.icc = icc.data();
            d.icc_bytes = variant == 5 ? 1 : icc.size();
          }
          std::vector<uint8_t> in((size_t)w * h * 4 * (bpp / 8));
          srand(w * 31 + h + variant);
          for(size_t i = 0; i < in.size(); i++) in[i] = (variant & 2) ? (uint8_t)(rand() >> 7) : (uint8_t)(i / 64);
          std::vector<uint8_t> o;
          tf_geom_t g;
          if(!encode(in.data(), w, h, &d, o) || tf_geometry(w, h, &d, &g, nullptr))
          {
            fprintf(stderr, "%d x %d bpp %d layers %d variant %d: not encoded\n", w, h, bpp, layers, variant);
            return 1;
          }
          uint64_t at = g.data_start;
          for(uint32_t s = 0; s < g.nstrips; s++)
          {
            const uint64_t off = get32(o, g.pos_offsets + 4 * s), cnt = get32(o, g.pos_counts + 4 * s);
            if(off != at || (off & 1) || !cnt)
            {
              fprintf(stderr, "%d x %d bpp %d layers %d variant %d: strip %u at %llu, expected %llu\n", w, h, bpp, layers,
                      variant, s, (unsigned long long)off, (unsigned long long)at);
              return 1;
            }
            at = off + cnt + (s + 1 < g.nstrips ? (cnt & 1) : 0);
          }
          if(at != o.size()) return 1;
          files++;
        }
  printf("tiff_host: %d files encoded, every layout consistent\n", files);
  return 0;
}
#endif
