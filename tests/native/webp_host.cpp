// tests/native/webp_host.cpp -- TEST INFRASTRUCTURE: the WebP encoder's body (ansel_amd/csrc/webp_body.h, run by the
// kernels of webp.hip on gfx950) compiled for the host and run one step after the other: the same predictor choice,
// matches, parse, tables, headers and tokens.  tests/test_webp_host.py has libwebp's decoder (Pillow) judge its file;
// tests/test_gpu_webp.py checks that the device's file equals it byte for byte.
//
//   g++ -O2 -std=c++17 -fPIC -shared -I ansel_amd/csrc -I include tests/native/webp_host.cpp -o libwebp_host.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DWEBP_HOST_MAIN -I ansel_amd/csrc -I include \
//       tests/native/webp_host.cpp -o webp_host && ./webp_host      (a program of its own: a small corpus, each
//       file's layout checked)
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "webp_body.h"

namespace
{

std::vector<uint8_t> g_out;
std::string g_stats;

void js(std::string &o, const char *key, uint64_t v) { o += "\"" + std::string(key) + "\":" + std::to_string(v) + ","; }

template <class T>
void js_list(std::string &o, const char *key, const T *v, int n)
{
  o += "\"" + std::string(key) + "\":[";
  for(int i = 0; i < n; i++) o += std::to_string((unsigned long long)v[i]) + (i + 1 < n ? "," : "");
  o += "],";
}

// the file; empty: refused, or the counted and the written bits disagree
std::vector<uint8_t> encode(const uint8_t *in, int w, int h, const dt_hip_webp_data_t *d)
{
  wp_geom_t g;
  char why[256];
  if(!wp_geometry(w, h, d, &g, why, sizeof(why))) return {};
  wp_head_t hd;
  if(!wp_file_head(w, h, g, (const uint8_t *)d->icc, d->icc ? (size_t)d->icc_bytes : 0, &hd)) return {};
  const uint64_t N = g.N;
  const int level = d->level;
  // the transforms
  std::vector<uint8_t> modes((size_t)g.bx * g.by);
  std::vector<uint32_t> res(N);
  uint64_t mode_count[WP_NMODES] = { 0 };
  for(uint32_t by = 0; by < g.by; by++)
    for(uint32_t bx = 0; bx < g.bx; bx++)
    {
      const int x0 = (int)(bx << g.pb), y0 = (int)(by << g.pb);
      const int x1 = std::min(w, x0 + (1 << g.pb)), y1 = std::min(h, y0 + (1 << g.pb));
      uint32_t cost[WP_NMODES] = { 0 };
      for(int y = y0; y < y1; y++)
        for(int x = x0; x < x1; x++) wp_costs(in, w, x, y, cost);
      const int m = wp_choose(cost);
      modes[(size_t)by * g.bx + bx] = (uint8_t)m;
      mode_count[m]++;
      for(int y = y0; y < y1; y++)
        for(int x = x0; x < x1; x++) res[(size_t)y * w + x] = wp_residual(in, w, x, y, m);
    }
  // matches and the parse, segment by segment
  const uint32_t *s = res.data();
  std::vector<uint8_t> tok(N, 1), mat(N, 0);
  std::vector<uint32_t> m(N, 0);
  uint64_t nmatch = 0, len_min = ~0ull, len_max = 0, dist_min = ~0ull, dist_max = 0, lazy = 0, two_near = 0;
  uint64_t d_one = 0, d_row = 0, d_far = 0;
  if(level > 0)
  {
    std::vector<int32_t> head(WP_NTAB << WP_TBITS);
    std::vector<uint32_t> lenv(WP_SEG), distv(WP_SEG);
    for(uint64_t k = 0; k < g.nseg; k++)
    {
      const uint64_t s0 = k * WP_SEG, s1 = std::min<uint64_t>(N, s0 + WP_SEG), n = s1 - s0;
      const uint64_t ws = s0 > WP_WIN ? s0 - WP_WIN : 0;
      std::fill(head.begin(), head.end(), -1);
      for(uint64_t c = ws; c < s1; c += WP_STEP)
      {
        const uint64_t e = std::min<uint64_t>(c + WP_STEP, s1);
        for(uint64_t p = std::max(c, s0); p < e; p++)
          lenv[p - s0] = wp_best(s, N, p, ws, (uint32_t)std::min<uint64_t>(WP_MAXLEN, s1 - p), (uint32_t)w,
                                 [&](uint32_t slot) { return head[slot]; }, &distv[p - s0]);
        for(uint64_t p = c; p < e; p++)
          for(int t = 0; t < WP_NTAB && wp_keyed(p, N, t); t++)
          {
            int32_t &hd2 = head[wp_slot(s, p, t)];
            hd2 = std::max(hd2, (int32_t)(p - ws));
          }
      }
      for(uint64_t i = 0; i < n;)
      {
        const uint32_t l = lenv[i], ln = i + 1 < n ? lenv[i + 1] : 0;
        if(wp_take(l, ln, level))
        {
          mat[s0 + i] = 1;
          m[s0 + i] = (l << 16) | (distv[i] - 1);
          nmatch++;
          len_min = std::min<uint64_t>(len_min, l);
          len_max = std::max<uint64_t>(len_max, l);
          dist_min = std::min<uint64_t>(dist_min, distv[i]);
          dist_max = std::max<uint64_t>(dist_max, distv[i]);
          if(l == 2) two_near++;
          if(distv[i] == 1) d_one++;
          else if(distv[i] == (uint32_t)w) d_row++;
          else d_far++;
          for(uint32_t j = 1; j < l; j++) tok[s0 + i + j] = 0;
          i += l;
        }
        else
        {
          if(l >= 2) lazy++;
          i++;
        }
      }
    }
  }
  // the groups
  const uint32_t ntiles = g.tx * g.ty;
  std::vector<wp_group_t> groups(ntiles);
  std::vector<wp_tab_work_t> work(1);
  wp_tab_work_t &tw = work[0];
  uint64_t kinds[4] = { 0 }, rle_used[WP_NCL] = { 0 }, rep_first = 0, cl_max = 0;
  int longest_all[10] = { 0 }, len_used_max = 0;
  {
    std::vector<uint32_t> freq((size_t)ntiles * WP_NSYM, 0);
    for(uint64_t p = 0; p < N; p++)
      if(tok[p])
      {
        uint32_t *f = freq.data() + (size_t)wp_tile((uint32_t)p, (uint32_t)w, g.eb, g.tx) * WP_NSYM;
        wp_count(s[p], mat[p] != 0, m[p], [&](uint32_t i) { f[i]++; });
      }
    for(uint32_t t = 0; t < ntiles; t++)
    {
      int longest[10];
      wp_tables(&tw, freq.data() + (size_t)t * WP_NSYM, 0, 1, [](uint64_t v) { return v; }, []() {}, &groups[t], longest);
      for(int a = 0; a < 5; a++)
      {
        const wp_code_t &c = groups[t].c[a];
        kinds[c.kind]++;
        longest_all[a] = std::max(longest_all[a], longest[a]);
        longest_all[5 + a] = std::max(longest_all[5 + a], longest[5 + a]);
        if(c.kind < WP_NORMAL) continue;
        bool nonzero_seen = false;
        wp_rle([&](int i) { return wp_header_len(&groups[t], a, i); }, wp_alpha_size(a), [&](int sym, uint32_t, int) {
          rle_used[sym]++;
          if(sym == 16 && !nonzero_seen) rep_first++;
          if(sym >= 1 && sym <= 15) nonzero_seen = true;
        });
        for(int i = 0; i < WP_NCL; i++) cl_max = std::max<uint64_t>(cl_max, c.cl_len[i]);
        for(int i = 0; i < wp_alpha_size(a); i++) len_used_max = std::max<int>(len_used_max, groups[t].len[wp_alpha_off(a) + i]);
      }
    }
  }
  // the stream
  wp_bits_t o;
  o.b = hd.a;
  o.pos = hd.a_bits;
  for(size_t i = 0; i < modes.size(); i++) o.put(wp_rev(modes[i], 4), 4);
  for(uint64_t i = 0; i < hd.b_bits; i++) o.put((hd.b[i >> 3] >> (i & 7)) & 1, 1);
  for(uint32_t t = 0; t < ntiles; t++)
  {
    const uint64_t start = o.pos;
    for(int a = 0; a < 5; a++) wp_code_header(&groups[t], a, [&](uint32_t v, int nb) { o.put(v, nb); });
    if(o.pos - start != groups[t].hdr_bits) return {};
  }
  uint64_t token_bits = 0;
  for(uint64_t p = 0; p < N; p++)
    if(tok[p])
    {
      const wp_group_t *gr = &groups[wp_tile((uint32_t)p, (uint32_t)w, g.eb, g.tx)];
      wp_token(gr, s[p], mat[p] != 0, m[p], [&](uint32_t c, int l, uint32_t e, int ne) {
        o.put(c, l);
        o.put(e, ne);
        token_bits += (uint64_t)(l + ne);
      });
    }
  std::vector<uint8_t> f = o.b;
  f.resize((size_t)((o.pos + 7) / 8), 0);
  const uint64_t payload = f.size() - hd.payload_at;
  if(payload & 1) f.push_back(0);
  for(int k = 0; k < 4; k++)
  {
    f[hd.vp8l_size_at + k] = (uint8_t)(payload >> (8 * k));
    f[4 + k] = (uint8_t)((f.size() - 8) >> (8 * k));
  }
  std::string &st = g_stats;
  st = "{";
  js_list(st, "modes", mode_count, WP_NMODES);
  js_list(st, "kinds", kinds, 4);
  js_list(st, "rle", rle_used, WP_NCL);
  js_list(st, "longest", longest_all, 5);
  js_list(st, "cl_longest", longest_all + 5, 5);
  js(st, "rep_first", rep_first);
  js(st, "cl_max", cl_max);
  js(st, "len_used_max", (uint64_t)len_used_max);
  js(st, "matches", nmatch);
  js(st, "len_min", nmatch ? len_min : 0);
  js(st, "len_max", len_max);
  js(st, "dist_min", nmatch ? dist_min : 0);
  js(st, "dist_max", dist_max);
  js(st, "dist_one", d_one);
  js(st, "dist_row", d_row);
  js(st, "dist_other", d_far);
  js(st, "lazy", lazy);
  js(st, "two_near", two_near);
  js(st, "tiles", ntiles);
  js(st, "tx", g.tx);
  js(st, "ty", g.ty);
  js(st, "blocks", (uint64_t)g.bx * g.by);
  js(st, "pb", (uint64_t)g.pb);
  js(st, "eb", (uint64_t)g.eb);
  js(st, "nseg", g.nseg);
  js(st, "token_bits", token_bits);
  js(st, "payload", payload);
  st += "\"bytes\":" + std::to_string(f.size()) + "}";
  return f;
}

} // namespace

// the whole file; returns its length (0: refused, or the counted and written bits disagree); webp_host_copy() fetches it
extern "C" size_t webp_host_encode(const void *in, int w, int h, const dt_hip_webp_data_t *d)
{
  g_out = encode((const uint8_t *)in, w, h, d);
  return g_out.size();
}

extern "C" void webp_host_copy(uint8_t *out) { memcpy(out, g_out.data(), g_out.size()); }

// the twin of dt_hip_webp_bound()
extern "C" size_t webp_host_bound(int w, int h, const dt_hip_webp_data_t *d)
{
  wp_geom_t g;
  char why[256];
  return wp_geometry(w, h, d, &g, why, sizeof(why)) ? (size_t)g.bound : 0;
}

// what the last webp_host_encode() did, as JSON: the blocks per predictor mode, the codes per kind (WP_SIMPLE1 ...),
// the code length symbols the headers used, the longest unlimited code length per alphabet, the repeats (16) written
// before any non-zero length, the matches' shortest / longest length and distance and how many went left, up or
// elsewhere, the matches the lazy step passed over, the matches of 2 pixels, the geometry.  Returns the length; out may be null
extern "C" size_t webp_host_stats(char *out)
{
  if(out) memcpy(out, g_stats.data(), g_stats.size());
  return g_stats.size();
}

// wp_rle() alone on n code lengths: out takes (symbol, extra) pairs; returns their count
extern "C" size_t webp_host_rle(const uint8_t *len, int n, uint32_t *out)
{
  size_t k = 0;
  wp_rle([&](int i) { return (int)len[i]; }, n, [&](int sym, uint32_t extra, int) {
    out[2 * k] = (uint32_t)sym;
    out[2 * k + 1] = extra;
    k++;
  });
  return k;
}

#ifdef WEBP_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

namespace
{

uint32_t le32(const std::vector<uint8_t> &f, size_t at) { return f[at] | (f[at + 1] << 8) | (f[at + 2] << 16) | ((uint32_t)f[at + 3] << 24); }

// RIFF size, chunk order and sizes, even lengths, the VP8L signature and dimensions
bool layout_ok(const std::vector<uint8_t> &f, int w, int h, size_t icc)
{
  if(f.size() < 20 + 5 || (f.size() & 1) || memcmp(f.data(), "RIFF", 4) || memcmp(f.data() + 8, "WEBP", 4)) return false;
  if(le32(f, 4) != f.size() - 8) return false;
  size_t at = 12;
  std::string order;
  while(at + 8 <= f.size())
  {
    const uint32_t n = le32(f, at + 4);
    order += std::string((const char *)f.data() + at, 4);
    if(!memcmp(f.data() + at, "VP8L", 4))
    {
      const uint8_t *p = f.data() + at + 8;
      const uint32_t bits = le32(f, at + 9);
      if(p[0] != 0x2f || (int)(bits & 0x3fff) + 1 != w || (int)((bits >> 14) & 0x3fff) + 1 != h || (bits >> 28)) return false;
    }
    if(!memcmp(f.data() + at, "ICCP", 4) && n != icc) return false;
    at += 8 + n + (n & 1);
  }
  return at == f.size() && order == (icc ? "VP8XICCPVP8L" : "VP8L");
}

} // namespace

int main()
{
  const int sizes[][2] = { { 1, 1 }, { 1, 7 }, { 7, 1 }, { 2, 2 }, { 3, 5 }, { 4, 4 }, { 5, 3 }, { 9, 7 }, { 17, 33 }, { 40, 30 },
                           { 16383, 1 }, { 1, 16383 } };
  int files = 0;
  uint32_t seed = 12345;
  auto rnd = [&]() { return seed = seed * 1664525u + 1013904223u; };
  for(const auto &sz : sizes)
    for(int content = 0; content < 5; content++)
      for(int level : { 0, 1, 6 })
        for(int bits : { 0, 2, 3 })
        {
          const int w = sz[0], h = sz[1];
          if((w > 1000 || h > 1000) && (content != 4 || level != 6 || bits != 0)) continue; // the long frames once
          std::vector<uint8_t> img((size_t)w * h * 4);
          for(int y = 0; y < h; y++)
            for(int x = 0; x < w; x++)
            {
              uint8_t *p = &img[((size_t)y * w + x) * 4];
              for(int c = 0; c < 4; c++)
                p[c] = content == 0   ? 77
                       : content == 1 ? (uint8_t)(rnd() >> 24)
                       : content == 2 ? (uint8_t)(x * 3 + c * 40)
                       : content == 3 ? (uint8_t)((x / 3 + y) % 2 ? 200 : 13)
                                      : (uint8_t)((x % 7) * 30 + (rnd() >> 30));
            }
          std::vector<uint8_t> icc(content == 1 ? 3 : 0, 0x42);
          dt_hip_webp_data_t d;
          memset(&d, 0, sizeof(d));
          d.lossless = 1;
          d.level = level;
          d.predictor_bits = bits;
          d.entropy_bits = bits;
          d.icc = icc.empty() ? nullptr : icc.data();
          d.icc_bytes = icc.size();
          const std::vector<uint8_t> f = encode(img.data(), w, h, &d);
          if(f.empty() || !layout_ok(f, w, h, icc.size()) || 8 + f.size() > webp_host_bound(w, h, &d))
          {
            fprintf(stderr, "webp_host: %d x %d content %d level %d bits %d failed (%zu bytes)\n", w, h, content, level, bits, f.size());
            return 1;
          }
          files++;
        }
  printf("webp_host: %d files\n", files);
  return 0;
}
#endif
