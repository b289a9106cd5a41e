// tests/native/png_host.cpp -- TEST INFRASTRUCTURE: the PNG encoder's body (ansel_amd/csrc/png_deflate.h, run by the
// kernels of png.hip on gfx950) compiled for the host and run one step after the other: the same filter choice,
// matches, parse, tables, blocks, checksums and chunks.  tests/test_png_host.py checks its file against libpng and
// zlib; tests/test_gpu_png.py checks that the device's file equals it byte for byte.
//
//   g++ -O2 -std=c++17 -fPIC -shared -I ansel_amd/csrc tests/native/png_host.cpp -o libpng_host.so
#include <string.h>

#include <algorithm>
#include <vector>

#include "png_deflate.h"

namespace
{

std::vector<uint8_t> filtered(const void *in, int w, int h, int depth)
{
  const uint64_t rb = (uint64_t)w * (depth == 8 ? 3 : 6);
  std::vector<uint8_t> fs((size_t)(h * (rb + 1)));
  std::vector<uint32_t> row[5];
  for(int f = 0; f < 5; f++) row[f].resize(rb);
  for(int y = 0; y < h; y++)
  {
    uint64_t sum[5] = { 0, 0, 0, 0, 0 };
    for(uint64_t j = 0; j < rb; j++)
    {
      uint32_t r[5];
      pf_byte(in, w, depth, y, (uint32_t)j, r);
      for(int f = 0; f < 5; f++)
      {
        row[f][j] = r[f];
        sum[f] += pf_cost(r[f]);
      }
    }
    const int best = pf_choose(sum);
    uint8_t *o = fs.data() + y * (rb + 1);
    o[0] = (uint8_t)best;
    for(uint64_t j = 0; j < rb; j++) o[1 + j] = (uint8_t)row[best][j];
  }
  return fs;
}

struct bitwriter_t
{
  std::vector<uint8_t> b;
  uint64_t pos = 0;
  void put(uint32_t v, int n)
  {
    for(int k = 0; k < n; k++, pos++)
    {
      if((pos >> 3) >= b.size()) b.push_back(0);
      b[pos >> 3] |= ((v >> k) & 1) << (pos & 7);
    }
  }
  void align() { pos = (pos + 7) & ~(uint64_t)7; b.resize(pos >> 3); }
};

std::vector<uint8_t> zlib_stream(const std::vector<uint8_t> &fs, int level)
{
  const uint64_t N = fs.size();
  const uint64_t nseg = (N + PD_SEG - 1) / PD_SEG;
  const uint8_t *s = fs.data();
  bitwriter_t bw;
  const uint16_t zh = pd_zlib_header(level);
  bw.put(zh >> 8, 8);
  bw.put(zh & 255, 8);
  std::vector<int32_t> head(PD_NTAB << PD_TBITS);
  std::vector<uint32_t> lenv(PD_SEG), distv(PD_SEG);
  std::vector<uint8_t> tok(PD_SEG), mat(PD_SEG);
  static pd_tab_work_t tw;
  for(uint64_t k = 0; k < nseg; k++)
  {
    const uint64_t s0 = k * PD_SEG, s1 = std::min<uint64_t>(N, s0 + PD_SEG), n = s1 - s0;
    std::fill(tok.begin(), tok.end(), 0);
    std::fill(mat.begin(), mat.end(), 0);
    uint32_t freq[PD_NLIT + PD_NDIST] = { 0 };
    if(level > 0)
    {
      const uint64_t ws = s0 > PD_WIN ? s0 - PD_WIN : 0;
      std::fill(head.begin(), head.end(), -1);
      std::fill(lenv.begin(), lenv.end(), 0);
      for(uint64_t c = ws; c < s1; c += PD_STEP)
      {
        const uint64_t e = std::min<uint64_t>(c + PD_STEP, s1);
        for(uint64_t p = std::max(c, s0); p < e; p++)
          lenv[p - s0] = pd_best(s, N, p, ws, (uint32_t)std::min<uint64_t>(PD_MAXLEN, s1 - p),
                                 [&](uint32_t slot) { return head[slot]; }, &distv[p - s0]);
        for(uint64_t p = c; p < e; p++)
          for(int t = 0; t < PD_NTAB && pd_keyed(p, N, t); t++)
          {
            int32_t &hd = head[pd_slot(s, p, t)];
            hd = std::max(hd, (int32_t)(p - ws));
          }
      }
      for(uint64_t i = 0; i < n;)
      {
        const uint32_t l = lenv[i], ln = i + 1 < n ? lenv[i + 1] : 0;
        tok[i] = 1;
        if(pd_take(l, ln, level))
        {
          mat[i] = 1;
          i += l;
        }
        else
          i++;
      }
      for(uint64_t i = 0; i < n; i++)
        if(tok[i])
        {
          uint32_t ne, ex;
          if(mat[i])
          {
            freq[pd_len_sym(lenv[i], &ne, &ex)]++;
            freq[PD_NLIT + pd_dist_sym(distv[i], &ne, &ex)]++;
          }
          else
            freq[s[s0 + i]]++;
        }
      freq[256]++;
    }
    pd_seg_t seg;
    pd_tables(&tw, freq, (uint32_t)n, level, 0, 1, [](uint64_t v) { return v; }, []() {}, &seg);
    const bool last = k + 1 == nseg;
    const uint64_t start = bw.pos;
    if(seg.type == PD_STORED)
    {
      bw.put(last ? 1 : 0, 3);
      bw.align();
      bw.put((uint32_t)n & 0xffff, 16);
      bw.put(~(uint32_t)n & 0xffff, 16);
      for(uint64_t i = 0; i < n; i++) bw.put(s[s0 + i], 8);
      if(bw.pos != pd_seg_end(seg, start)) return {};
      continue;
    }
    uint16_t code[PD_NLIT + PD_NDIST], cl_code[PD_NCL];
    pd_codes(seg.len, PD_NLIT, code, seg.type == PD_FIXED);
    pd_codes(seg.len + PD_NLIT, PD_NDIST, code + PD_NLIT);
    pd_codes(seg.cl_len, PD_NCL, cl_code);
    pd_block_header(seg, last, cl_code, [&](uint32_t v, int nb) { bw.put(v, nb); });
    for(uint64_t i = 0; i < n; i++)
    {
      if(!tok[i]) continue;
      if(!mat[i])
      {
        bw.put(code[s[s0 + i]], seg.len[s[s0 + i]]);
        continue;
      }
      uint32_t ne, ex;
      const uint32_t ls = pd_len_sym(lenv[i], &ne, &ex);
      bw.put(code[ls], seg.len[ls]);
      bw.put(ex, (int)ne);
      const uint32_t ds = pd_dist_sym(distv[i], &ne, &ex);
      bw.put(code[PD_NLIT + ds], seg.len[PD_NLIT + ds]);
      bw.put(ex, (int)ne);
    }
    bw.put(code[256], seg.len[256]);
    if(bw.pos != pd_seg_end(seg, start)) return {}; // the counted bits and the written ones must agree
  }
  bw.align();
  uint32_t a = 1, b = 0;
  for(uint64_t j = 0; j < N; j++)
  {
    a = (a + s[j]) % PD_ADLER_MOD;
    b = (b + a) % PD_ADLER_MOD;
  }
  bw.put(b >> 8, 8);
  bw.put(b & 255, 8);
  bw.put(a >> 8, 8);
  bw.put(a & 255, 8);
  return bw.b;
}

std::vector<uint8_t> g_out;

} // namespace

// the filtered stream (h * (1 + w * bpp) bytes) of RGBA u8 (depth 8) or RGBA u16 (depth 16) pixels
extern "C" void png_host_filtered(const void *in, int w, int h, int depth, uint8_t *out)
{
  const std::vector<uint8_t> fs = filtered(in, w, h, depth);
  memcpy(out, fs.data(), fs.size());
}

// the whole file; returns its length (0: the counted and written bits disagree), png_host_copy() fetches it
extern "C" size_t png_host_encode(const void *in, int w, int h, int depth, int level, const uint8_t *icc,
                                  size_t icc_bytes, int dpi)
{
  const std::vector<uint8_t> z = zlib_stream(filtered(in, w, h, depth), level);
  if(z.empty()) return 0;
  std::vector<uint8_t> o = pd_file_head(w, h, depth, icc, icc_bytes, dpi);
  for(size_t i = 0; i < z.size(); i += PD_IDAT)
    pd_chunk(o, "IDAT", z.data() + i, std::min<size_t>(PD_IDAT, z.size() - i));
  pd_chunk(o, "IEND", nullptr, 0);
  g_out = o;
  return o.size();
}

extern "C" void png_host_copy(uint8_t *out) { memcpy(out, g_out.data(), g_out.size()); }
