// tests/native/png_host.cpp -- TEST INFRASTRUCTURE: the PNG encoder's body (ansel_amd/csrc/png_deflate.h, run by the
// kernels of png.hip on gfx950) compiled for the host and run one step after the other: the same filter choice,
// matches, parse, tables, blocks, checksums and chunks.  tests/test_png_host.py checks its file against libpng and
// zlib; tests/test_gpu_png.py checks that the device's file equals it byte for byte.
//
//   g++ -O2 -std=c++17 -fPIC -shared -I ansel_amd/csrc tests/native/png_host.cpp -o libpng_host.so
#include <string.h>

#include <algorithm>
#include <string>
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

// what the last encode did, as JSON (png_host_stats()): the tests' proof that a frame reached a branch
std::string g_stats;

void js(std::string &o, const char *key, uint64_t v) { o += "\"" + std::string(key) + "\":" + std::to_string(v) + ","; }

template <class T>
void js_list(std::string &o, const char *key, const T *v, int n)
{
  o += "\"" + std::string(key) + "\":[";
  for(int i = 0; i < n; i++) o += std::to_string((unsigned)v[i]) + (i + 1 < n ? "," : "");
  o += "],";
}

std::vector<uint8_t> zlib_stream(const std::vector<uint8_t> &fs, int level)
{
  g_stats = "{\"blocks\":[";
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
    uint64_t refused = ~0ull;
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
        for(uint64_t p = std::max(c, s0); p < e; p++) // stats: the nearest 3-byte match refused as too far
          for(int t = 0; t < PD_NTAB && pd_keyed(p, N, t); t++)
          {
            const int32_t q = head[pd_slot(s, p, t)];
            if(q < 0) continue;
            const uint64_t d = p - ws - (uint64_t)q;
            uint32_t l = 0;
            while(l < 4 && l < s1 - p && s[ws + q + l] == s[p + l]) l++;
            if(l == 3 && d > PD_TOO_FAR && d <= PD_WIN) refused = std::min(refused, d);
          }
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
    int longest[3] = { 0, 0, 0 };
    pd_tables(&tw, freq, (uint32_t)n, level, 0, 1, [](uint64_t v) { return v; }, []() {}, &seg, longest);
    const bool last = k + 1 == nseg;
    const uint64_t start = bw.pos;
    {
      std::string &o = g_stats;
      o += k ? ",{" : "{";
      js(o, "type", seg.type);
      js(o, "nbytes", n);
      js(o, "phase", start & 7);
      js(o, "bits", seg.bits);
      uint32_t nm = 0, lmin = ~0u, lmax = 0, dmin = ~0u, dmax = 0, far3 = 0, used = 0;
      for(uint64_t i = 0; i < n; i++)
        if(mat[i])
        {
          nm++;
          lmin = std::min(lmin, lenv[i]);
          lmax = std::max(lmax, lenv[i]);
          dmin = std::min(dmin, distv[i]);
          dmax = std::max(dmax, distv[i]);
          if(lenv[i] == 3) far3 = std::max(far3, distv[i]);
        }
      for(int i = 0; i < PD_NDIST; i++) used += freq[PD_NLIT + i] != 0;
      js(o, "matches", nm);
      js(o, "len_min", nm ? lmin : 0);
      js(o, "len_max", lmax);
      js(o, "dist_min", nm ? dmin : 0);
      js(o, "dist_max", dmax);
      js(o, "far3_taken", far3);
      js(o, "far3_refused", refused == ~0ull ? 0 : refused);
      js(o, "dist_used", used);
      if(level > 0)
      {
        js_list(o, "longest", longest, 3);
        js(o, "nlit", seg.nlit);
        js(o, "ndist", seg.ndist);
        js(o, "ncl", seg.ncl);
      }
      if(seg.type == PD_DYNAMIC)
      {
        js_list(o, "len", seg.len, PD_NLIT + PD_NDIST);
        js_list(o, "cl_len", seg.cl_len, PD_NCL);
        std::vector<uint32_t> r;
        pd_rle(seg.len, (int)seg.nlit, (int)seg.ndist, [&](int sym, uint32_t extra, int) {
          r.push_back((uint32_t)sym);
          r.push_back(extra);
        });
        js_list(o, "rle", r.data(), (int)r.size());
      }
      o += "\"last\":" + std::to_string(last ? 1 : 0) + "}";
    }
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
  const uint64_t zlen = bw.b.size(), nidat = (zlen + PD_IDAT - 1) / PD_IDAT;
  g_stats += "],";
  js(g_stats, "N", N);
  js(g_stats, "zlen", zlen);
  js(g_stats, "nidat", nidat);
  g_stats += "\"last_idat\":" + std::to_string(zlen - (nidat - 1) * PD_IDAT) + "}";
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

// what the last png_host_encode() did, as JSON: per block its type, bytes, the bit phase it started at, its matches'
// shortest / longest length and distance, the farthest 3-byte match taken and the nearest one refused, the distance
// codes used, the longest unadjusted code length of the three alphabets, and of a dynamic block HLIT / HDIST / HCLEN's
// counts, the code lengths and what pd_rle() coded (symbol, extra, ...); then N, zlen, the IDAT count and the last
// chunk's bytes.  Returns the length; out may be null
extern "C" size_t png_host_stats(char *out)
{
  if(out) memcpy(out, g_stats.data(), g_stats.size());
  return g_stats.size();
}

// pd_rle() alone: len is PD_NLIT + PD_NDIST code lengths; out takes (symbol, extra) pairs; returns their count
extern "C" size_t png_host_rle(const uint8_t *len, int nlit, int ndist, uint32_t *out)
{
  size_t k = 0;
  pd_rle(len, nlit, ndist, [&](int sym, uint32_t extra, int) {
    out[2 * k] = (uint32_t)sym;
    out[2 * k + 1] = extra;
    k++;
  });
  return k;
}

// pd_tables() with one lane on nseg histograms of PD_NLIT + PD_NDIST counts (a stream of nbytes bytes: every segment
// PD_SEG but the last): the twin of dt_hip_test_png_tables() in png.hip; longest (may be null) takes three words per
// segment
extern "C" size_t png_host_sizeof_seg(void) { return sizeof(pd_seg_t); }

extern "C" void png_host_tables(const uint32_t *freq, uint64_t nbytes, int nseg, int level, void *segs_out, int *longest)
{
  static pd_tab_work_t tw;
  for(int k = 0; k < nseg; k++)
  {
    pd_seg_t seg;
    memset(&seg, 0, sizeof(seg));
    const uint64_t s0 = (uint64_t)k * PD_SEG;
    pd_tables(&tw, freq + (size_t)k * (PD_NLIT + PD_NDIST), (uint32_t)(std::min(nbytes, s0 + PD_SEG) - s0), level, 0, 1, [](uint64_t v) { return v; }, []() {},
              &seg, longest ? longest + 3 * k : nullptr);
    memcpy((char *)segs_out + (size_t)k * sizeof(seg), &seg, sizeof(seg));
  }
}
