// webp_body.h -- the body of the lossless WebP (VP8L) encoder (webp.hip), written once and compiled twice: the device
// kernels call these functions from their threads, and tests/native/webp_host.cpp runs the same functions one after the
// other on the host, so the CPU suite judges the file with libwebp's decoder and the device file equals the host
// build's.
//
// The stream: SUBTRACT_GREEN, then PREDICTOR (one of the 14 modes per block of 2^predictor_bits squared pixels, chosen
// by libpng's cost: the sum of |signed residual byte|, the lowest mode on a tie), then the residual pixels as 32-bit
// ARGB words in scan order, cut into segments of WP_SEG pixels.  A segment's matches: WP_NTAB hash tables of the most
// recent position of a key of 1, 2, 3 pixels, filled in steps of WP_STEP positions (all lookups of a step before its
// entries, the largest position wins), started WP_WIN pixels before the segment; the pixel to the left and the pixel
// above are candidates of their own.  A match stays inside its segment.  The parse is greedy at levels 1-3, lazy (a
// match is passed over while the next position's is longer) at 4-9; level 0 writes literals.  Every tile of
// 2^entropy_bits squared pixels has its own five prefix codes (jh_build(), 15 bits; the code length code 7 bits), a
// token takes the codes of the tile of its first pixel.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "png_deflate.h"

#define WP_FN PD_FN

#define WP_SEG 8192     // pixels per segment
#define WP_WIN 8192     // the hash tables start this many pixels before the segment: their distances are 1..WP_WIN
#define WP_STEP 256     // positions per step of the hash tables
#define WP_NTAB 3       // hash tables
#define WP_TBITS 12     // entries per table: 1 << WP_TBITS
#define WP_KEY(t) (1 + (t)) // pixels keyed by table t
#define WP_MAXLEN 4096  // the longest backward reference
#define WP_NEAR 512     // a match of 2 pixels further back than this is not taken
#define WP_MAXDIM 16383 // libwebp's limit of width and height
#define WP_MAXTILES 65536 // the entropy image's index has 16 bits
#define WP_MAXICC (16u << 20) // the profile travels with the host-built head through the runtime's pinned staging

#define WP_NGREEN 280 // 256 literals + 24 length prefixes (no colour cache)
#define WP_NDIST 40
#define WP_NSYM (WP_NGREEN + 3 * 256 + WP_NDIST)
#define WP_NCL 19
#define WP_NMODES 14
// per prefix code at most: simple bit, count, 19 lengths, max_symbol, then <= 14 bits per symbol
#define WP_CODE_MAX_BITS(n) (1 + 4 + 3 * WP_NCL + 1 + 14 * (uint64_t)(n))
#define WP_GROUP_MAX_BITS (5 * WP_CODE_MAX_BITS(0) + 14 * (uint64_t)WP_NSYM)
#define WP_PIXEL_MAX_BITS 45 // three literals of 15 bits (alpha costs nothing); a reference: 58 bits for >= 2 pixels

enum
{
  WP_GREEN = 0,
  WP_RED = 1,
  WP_BLUE = 2,
  WP_ALPHA = 3,
  WP_DIST = 4
};

// how a prefix code is written
enum
{
  WP_SIMPLE1 = 0, // one symbol < 256: zero bits per occurrence
  WP_SIMPLE2 = 1, // two symbols < 256: one bit each
  WP_NORMAL = 2,  // code lengths
  WP_NORMAL1 = 3  // one symbol >= 256: written as one code length of 1, read as a zero-bit code
};

WP_FN int wp_alpha_size(int a) { return a == WP_GREEN ? WP_NGREEN : a == WP_DIST ? WP_NDIST : 256; }
WP_FN int wp_alpha_off(int a) { return a == WP_GREEN ? 0 : WP_NGREEN + 256 * (a - 1); }

// ---------------------------------------------------------------------------------------------------------------------
// transforms

// pixel (x, y) as ARGB behind SUBTRACT_GREEN; alpha is coded as 255
WP_FN uint32_t wp_px(const uint8_t *in, int w, int x, int y)
{
  const uint8_t *p = in + ((size_t)y * w + x) * 4;
  const uint32_t r = p[0], g = p[1], b = p[2];
  return 0xff000000u | (((r - g) & 255) << 16) | (g << 8) | ((b - g) & 255);
}

WP_FN uint32_t wp_avg(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
WP_FN int wp_byte(uint32_t v, int c) { return (int)((v >> (8 * c)) & 255); }
WP_FN uint32_t wp_clip(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// a - b per byte
WP_FN uint32_t wp_sub(uint32_t a, uint32_t b)
{
  const uint32_t ag = 0x00ff00ffu + (a & 0xff00ff00u) - (b & 0xff00ff00u);
  const uint32_t rb = 0xff00ff00u + (a & 0x00ff00ffu) - (b & 0x00ff00ffu);
  return (ag & 0xff00ff00u) | (rb & 0x00ff00ffu);
}

// the prediction of mode 0..13 from the left, top, top-left and top-right pixels
WP_FN uint32_t wp_predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR)
{
  switch(mode)
  {
    case 0: return 0xff000000u;
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return wp_avg(wp_avg(L, TR), T);
    case 6: return wp_avg(L, TL);
    case 7: return wp_avg(L, T);
    case 8: return wp_avg(TL, T);
    case 9: return wp_avg(T, TR);
    case 10: return wp_avg(wp_avg(L, TL), wp_avg(T, TR));
    case 11:
    {
      // p = L + T - TL: |p - L| = |T - TL|, |p - T| = |L - TL|
      int sl = 0, st = 0;
      for(int c = 0; c < 4; c++)
      {
        const int dl = wp_byte(T, c) - wp_byte(TL, c), dt = wp_byte(L, c) - wp_byte(TL, c);
        sl += dl < 0 ? -dl : dl;
        st += dt < 0 ? -dt : dt;
      }
      return sl < st ? L : T;
    }
    case 12:
    {
      uint32_t r = 0;
      for(int c = 0; c < 4; c++) r |= wp_clip(wp_byte(L, c) + wp_byte(T, c) - wp_byte(TL, c)) << (8 * c);
      return r;
    }
    default:
    {
      uint32_t r = 0;
      for(int c = 0; c < 4; c++)
      {
        const int a = (wp_byte(L, c) + wp_byte(T, c)) >> 1;
        r |= wp_clip(a + (a - wp_byte(TL, c)) / 2) << (8 * c);
      }
      return r;
    }
  }
}

// is the prediction of (x, y) fixed by the frame's edge (*pred then holds it), or the block's mode (the neighbours)?
WP_FN bool wp_neighbours(const uint8_t *in, int w, int x, int y, uint32_t *pred, uint32_t *L, uint32_t *T, uint32_t *TL,
                         uint32_t *TR)
{
  if(y == 0)
  {
    *pred = x == 0 ? 0xff000000u : wp_px(in, w, x - 1, 0);
    return false;
  }
  if(x == 0)
  {
    *pred = wp_px(in, w, 0, y - 1);
    return false;
  }
  *L = wp_px(in, w, x - 1, y);
  *T = wp_px(in, w, x, y - 1);
  *TL = wp_px(in, w, x - 1, y - 1);
  *TR = x + 1 < w ? wp_px(in, w, x + 1, y - 1) : wp_px(in, w, 0, y); // the pixel behind T in memory
  return true;
}

// the cost of a residual pixel: libpng's |signed byte|, summed over its bytes
WP_FN uint32_t wp_cost(uint32_t r)
{
  return pf_cost(r & 255) + pf_cost((r >> 8) & 255) + pf_cost((r >> 16) & 255) + pf_cost(r >> 24);
}

// cost[m] += the cost of pixel (x, y) under mode m
WP_FN void wp_costs(const uint8_t *in, int w, int x, int y, uint32_t cost[WP_NMODES])
{
  uint32_t pred = 0, L = 0, T = 0, TL = 0, TR = 0;
  const uint32_t v = wp_px(in, w, x, y);
  if(!wp_neighbours(in, w, x, y, &pred, &L, &T, &TL, &TR))
  {
    const uint32_t c = wp_cost(wp_sub(v, pred));
    for(int m = 0; m < WP_NMODES; m++) cost[m] += c;
    return;
  }
  for(int m = 0; m < WP_NMODES; m++) cost[m] += wp_cost(wp_sub(v, wp_predict(m, L, T, TL, TR)));
}

// the residual of pixel (x, y) under mode
WP_FN uint32_t wp_residual(const uint8_t *in, int w, int x, int y, int mode)
{
  uint32_t pred = 0, L = 0, T = 0, TL = 0, TR = 0;
  if(wp_neighbours(in, w, x, y, &pred, &L, &T, &TL, &TR)) pred = wp_predict(mode, L, T, TL, TR);
  return wp_sub(wp_px(in, w, x, y), pred);
}

// the lowest mode of the smallest cost
WP_FN int wp_choose(const uint32_t cost[WP_NMODES])
{
  int best = 0;
  for(int m = 1; m < WP_NMODES; m++)
    if(cost[m] < cost[best]) best = m;
  return best;
}

// ---------------------------------------------------------------------------------------------------------------------
// matching and parsing

// the slot of position p in hash table t, keyed by the WP_KEY(t) pixels at p
WP_FN uint32_t wp_slot(const uint32_t *s, uint64_t p, int t)
{
  uint32_t v = s[p] * 2654435761u;
  for(int k = 1; k < WP_KEY(t); k++) v = (v ^ s[p + k]) * 2246822519u;
  v ^= v >> 15;
  return ((uint32_t)t << WP_TBITS) | ((v * 2654435761u) >> (32 - WP_TBITS));
}

WP_FN bool wp_keyed(uint64_t p, uint64_t N, int t) { return p + WP_KEY(t) <= N; }

// the match of position p against the earlier position q, at most maxlen pixels; 0 when not taken.  The reference may
// overlap what it writes
WP_FN uint32_t wp_match(const uint32_t *s, uint64_t p, uint64_t q, uint32_t maxlen)
{
  uint32_t l = 0;
  while(l < maxlen && s[q + l] == s[p + l]) l++;
  if(l < 2 || (l == 2 && p - q > WP_NEAR)) return 0;
  return l;
}

// the match of position p: the pixel to the left, the pixel above (distance w), the tables' candidates (positions
// window_start + head(slot), head() < 0: none), in that order; the longest, the nearer on a tie, and a candidate that
// reaches maxlen ends the search; *dist its distance; 0 when none
template <class Head>
WP_FN uint32_t wp_best(const uint32_t *s, uint64_t N, uint64_t p, uint64_t window_start, uint32_t maxlen, uint32_t w,
                       Head head, uint32_t *dist)
{
  uint32_t bl = 0, bd = 0, tried[2 + WP_NTAB];
  int nt = 0;
  for(int k = 0; k < 2 + WP_NTAB; k++)
  {
    uint32_t d;
    if(k == 0)
      d = 1;
    else if(k == 1)
      d = w;
    else
    {
      if(!wp_keyed(p, N, k - 2)) break;
      const int32_t q = head(wp_slot(s, p, k - 2));
      if(q < 0) continue;
      d = (uint32_t)(p - window_start - (uint64_t)q);
      if(d > WP_WIN) continue;
    }
    if(d > p) continue;
    bool seen = false;
    for(int i = 0; i < nt; i++) seen = seen || tried[i] == d;
    if(seen) continue;
    tried[nt++] = d;
    const uint32_t l = wp_match(s, p, p - d, maxlen);
    if(l > bl || (l && l == bl && d < bd))
    {
      bl = l;
      bd = d;
    }
    if(bl == maxlen) break; // nothing is longer: flat residuals cost one comparison of maxlen pixels, not five
  }
  *dist = bd;
  return bl;
}

// the parse's rule at one position: take the match of length l here, given the next position's length ln?  Lazy
// (levels 4-9): not while the next position's match is longer, so a rising run of lengths becomes literals (PNG's rule)
WP_FN bool wp_take(uint32_t l, uint32_t ln, int level) { return l >= 2 && !(level >= 4 && ln > l); }

// the prefix symbol of a length or distance code v >= 1, its extra bits and their value (deflate's distance symbols)
WP_FN uint32_t wp_prefix(uint32_t v, uint32_t *nextra, uint32_t *extra) { return pd_dist_sym(v, nextra, extra); }

// the tile of position p (row-major pixel index) of a frame w wide, tiles of 2^eb squared pixels, tx tiles a row
WP_FN uint32_t wp_tile(uint32_t p, uint32_t w, int eb, uint32_t tx)
{
  const uint32_t y = p / w, x = p - y * w;
  return (y >> eb) * tx + (x >> eb);
}

// ---------------------------------------------------------------------------------------------------------------------
// prefix codes

struct wp_code_t
{
  uint8_t kind; // WP_SIMPLE1 ...
  uint8_t ncl;  // code length code lengths written
  uint16_t sym0, sym1;
  uint8_t cl_len[WP_NCL];
};

// the five codes of one tile (or of a sub-image)
struct wp_group_t
{
  uint32_t hdr_bits;      // the five codes as written
  wp_code_t c[5];
  uint8_t len[WP_NSYM];   // bits per occurrence (0 for the only symbol of an alphabet)
  uint16_t code[WP_NSYM]; // canonical, bit-reversed for LSB-first output
};

WP_FN int wp_cl_order(int i)
{
  const uint8_t o[WP_NCL] = { 17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15 };
  return o[i];
}

// the run-length coding of n code lengths at(i): emit(symbol, extra, nbits).  16 repeats the last non-zero length,
// which starts as 8
template <class At, class F>
WP_FN void wp_rle(At at, int n, F emit)
{
  int i = 0, prev = 8;
  while(i < n)
  {
    const int v = at(i);
    int r = 1;
    while(i + r < n && at(i + r) == v) r++;
    i += r;
    if(v == 0)
    {
      while(r >= 11)
      {
        const int k = r < 138 ? r : 138;
        emit(18, (uint32_t)(k - 11), 7);
        r -= k;
      }
      if(r >= 3)
      {
        emit(17, (uint32_t)(r - 3), 3);
        r = 0;
      }
    }
    else
    {
      if(v != prev)
      {
        emit(v, 0u, 0);
        r--;
        prev = v;
      }
      while(r >= 3)
      {
        const int k = r < 6 ? r : 6;
        emit(16, (uint32_t)(k - 3), 2);
        r -= k;
      }
    }
    while(r-- > 0) emit(v, 0u, 0);
  }
}

// the code length of symbol i of alphabet a as the header writes it
WP_FN int wp_header_len(const wp_group_t *g, int a, int i)
{
  const wp_code_t &c = g->c[a];
  if(c.kind == WP_NORMAL1) return i == c.sym0 ? 1 : 0;
  return g->len[wp_alpha_off(a) + i];
}

// prefix code a of the group: put(value, nbits), LSB first
template <class Put>
WP_FN void wp_code_header(const wp_group_t *g, int a, Put put)
{
  const wp_code_t &c = g->c[a];
  if(c.kind == WP_SIMPLE1 || c.kind == WP_SIMPLE2)
  {
    put(1u, 1);
    put(c.kind == WP_SIMPLE2 ? 1u : 0u, 1);
    put(c.sym0 < 2 ? 0u : 1u, 1);
    put(c.sym0, c.sym0 < 2 ? 1 : 8);
    if(c.kind == WP_SIMPLE2) put(c.sym1, 8);
    return;
  }
  uint16_t cl_code[WP_NCL];
  pd_codes(c.cl_len, WP_NCL, cl_code);
  put(0u, 1);
  put((uint32_t)c.ncl - 4, 4);
  for(int i = 0; i < c.ncl; i++) put(c.cl_len[wp_cl_order(i)], 3);
  put(0u, 1); // max_symbol: the whole alphabet
  wp_rle([&](int i) { return wp_header_len(g, a, i); }, wp_alpha_size(a), [&](int sym, uint32_t extra, int nb) {
    put(cl_code[sym], c.cl_len[sym]);
    if(nb) put(extra, nb);
  });
}

// the work area of wp_tables()
struct wp_tab_work_t
{
  jh_work_t w;
  uint32_t clfreq[WP_NCL];
  uint8_t bits[16];
  uint16_t vals[JH_MAX_SYM];
  int32_t nz, s0, s1;
};

// the code lengths of one alphabet with at least two counted symbols (pd_lengths() keeps the number of codes of a
// length in a byte; 256 equally frequent symbols take 256 codes of 8 bits, so the counts are read from the work area)
template <class WaveMin, class Sync>
WP_FN void wp_lengths(wp_tab_work_t *tw, const uint32_t *freq, int n, int limit, int lane, int nlanes, WaveMin wave_min,
                      Sync sync, uint8_t *len_out, int *longest = nullptr)
{
  jh_work_t *w = &tw->w;
  if(lane == 0)
  {
    int nz = 0;
    for(int i = 0; i < n; i++) nz += freq[i] != 0;
    for(int i = 0; i < n; i++)
    {
      int64_t f = freq[i];
      if(!f && nz < 2)
      {
        f = 1;
        nz++;
      }
      w->freq[i] = f;
    }
  }
  sync();
  jh_build(w, n, limit, false, lane, nlanes, wave_min, sync, tw->bits, tw->vals);
  if(lane == 0)
  {
    for(int i = 0; i < n; i++) len_out[i] = 0;
    int p = 0;
    for(int l = 1; l <= limit; l++)
      for(int k = 0; k < w->bits[l]; k++) len_out[tw->vals[p++]] = (uint8_t)l;
    if(longest)
    {
      *longest = 0;
      for(int i = 0; i < n; i++)
        if(w->codesize[i] > *longest) *longest = w->codesize[i];
    }
  }
  sync();
}

// the five codes of one group from its WP_NSYM symbol counts (green, red, blue, alpha, distance); lane / nlanes /
// wave_min / sync as jh_build().  An alphabet without a count is coded as its symbol 0 alone; one used symbol costs no
// bits.  longest (tests; the kernels pass none): ten words, the longest code length before the limit of the five codes
// (15 bits), then of their code length codes (7 bits)
template <class WaveMin, class Sync>
WP_FN void wp_tables(wp_tab_work_t *tw, const uint32_t *freq, int lane, int nlanes, WaveMin wave_min, Sync sync,
                     wp_group_t *g, int *longest = nullptr)
{
  if(lane == 0) g->hdr_bits = 0;
  for(int a = 0; a < 5; a++)
  {
    const int n = wp_alpha_size(a), off = wp_alpha_off(a);
    if(lane == 0)
    {
      int nz = 0, s0 = 0, s1 = 0;
      for(int i = 0; i < n; i++)
        if(freq[off + i])
        {
          if(nz == 0) s0 = i;
          if(nz == 1) s1 = i;
          nz++;
        }
      tw->nz = nz;
      tw->s0 = s0;
      tw->s1 = s1;
      if(longest) longest[a] = longest[5 + a] = 0;
    }
    sync();
    const int nz = tw->nz, s0 = tw->s0, s1 = tw->s1;
    wp_code_t *c = &g->c[a];
    int kind;
    if(nz <= 1)
      kind = s0 < 256 ? WP_SIMPLE1 : WP_NORMAL1;
    else if(nz == 2 && s1 < 256)
      kind = WP_SIMPLE2;
    else
      kind = WP_NORMAL;
    if(kind == WP_NORMAL)
      wp_lengths(tw, freq + off, n, 15, lane, nlanes, wave_min, sync, g->len + off,
                 longest ? longest + a : nullptr);
    else if(lane == 0)
    {
      for(int i = 0; i < n; i++) g->len[off + i] = 0;
      if(kind == WP_SIMPLE2) g->len[off + s0] = g->len[off + s1] = 1;
    }
    if(lane == 0)
    {
      c->kind = (uint8_t)kind;
      c->sym0 = (uint16_t)s0;
      c->sym1 = (uint16_t)s1;
      c->ncl = 0;
      for(int i = 0; i < WP_NCL; i++)
      {
        c->cl_len[i] = 0;
        tw->clfreq[i] = 0;
      }
      for(int i = 0; i < n; i++) g->code[off + i] = 0;
      pd_codes(g->len + off, n, g->code + off);
      if(kind >= WP_NORMAL) wp_rle([&](int i) { return wp_header_len(g, a, i); }, n, [&](int s, uint32_t, int) { tw->clfreq[s]++; });
    }
    sync();
    if(kind >= WP_NORMAL)
    {
      wp_lengths(tw, tw->clfreq, WP_NCL, 7, lane, nlanes, wave_min, sync, c->cl_len, longest ? longest + 5 + a : nullptr);
      if(lane == 0)
      {
        int ncl = WP_NCL;
        while(ncl > 4 && c->cl_len[wp_cl_order(ncl - 1)] == 0) ncl--;
        c->ncl = (uint8_t)ncl;
      }
    }
    if(lane == 0)
    {
      uint32_t b = 0;
      wp_code_header(g, a, [&](uint32_t, int nb) { b += (uint32_t)nb; });
      g->hdr_bits += b;
    }
    sync();
  }
}

// the bits of the token at position p of the residual stream s (m: its match, len << 16 | dist - 1, when is_match):
// f(code, length, extra, extra bits) per symbol written
template <class F>
WP_FN void wp_token(const wp_group_t *g, uint32_t px, bool is_match, uint32_t m, F f)
{
  if(!is_match)
  {
    const uint32_t gr = (px >> 8) & 255, r = WP_NGREEN + ((px >> 16) & 255), b = WP_NGREEN + 256 + (px & 255),
                   al = WP_NGREEN + 512 + (px >> 24);
    f(g->code[gr], g->len[gr], 0u, 0);
    f(g->code[r], g->len[r], 0u, 0);
    f(g->code[b], g->len[b], 0u, 0);
    f(g->code[al], g->len[al], 0u, 0);
    return;
  }
  uint32_t ne, ex;
  const uint32_t ls = 256 + wp_prefix(m >> 16, &ne, &ex);
  f(g->code[ls], g->len[ls], ex, (int)ne);
  const uint32_t ds = WP_NGREEN + 768 + wp_prefix((m & 0xffff) + 1 + 120, &ne, &ex);
  f(g->code[ds], g->len[ds], ex, (int)ne);
}

// the symbols of that token into the group's WP_NSYM counts: add(index)
template <class Add>
WP_FN void wp_count(uint32_t px, bool is_match, uint32_t m, Add add)
{
  if(!is_match)
  {
    add((px >> 8) & 255);
    add(WP_NGREEN + ((px >> 16) & 255));
    add(WP_NGREEN + 256 + (px & 255));
    add(WP_NGREEN + 512 + (px >> 24));
    return;
  }
  uint32_t ne, ex;
  add(256 + wp_prefix(m >> 16, &ne, &ex));
  add(WP_NGREEN + 768 + wp_prefix((m & 0xffff) + 1 + 120, &ne, &ex));
}

WP_FN uint32_t wp_rev(uint32_t v, int n)
{
  uint32_t r = 0;
  for(int k = 0; k < n; k++) r |= ((v >> k) & 1) << (n - 1 - k);
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// geometry, bound and the host-built parts of the file

#include <string.h>

#include <vector>

#include "ansel_hip.h"

struct wp_geom_t
{
  int pb, eb;           // predictor_bits, entropy_bits as used
  uint32_t bx, by;      // predictor blocks
  uint32_t tx, ty;      // tiles (groups)
  uint64_t N, nseg;     // pixels, segments
  uint64_t container;   // bytes in front of the VP8L payload
  uint64_t bound;       // 8 + the file at most
};

// the frame's sizes; false (why: the reason) for refused settings
inline bool wp_geometry(int width, int height, const dt_hip_webp_data_t *d, wp_geom_t *g, char *why, size_t nwhy)
{
  if(!d)
  {
    snprintf(why, nwhy, "no dt_hip_webp_data_t");
    return false;
  }
  if(d->lossless != 1)
  {
    snprintf(why, nwhy, "lossless %d: only lossless WebP (VP8L) is written", (int)d->lossless);
    return false;
  }
  if(width < 1 || height < 1 || width > WP_MAXDIM || height > WP_MAXDIM)
  {
    snprintf(why, nwhy, "%d x %d is outside 1..%d", width, height, WP_MAXDIM);
    return false;
  }
  if(d->level < 0 || d->level > 9)
  {
    snprintf(why, nwhy, "level %d is outside 0..9", (int)d->level);
    return false;
  }
  if(d->predictor_bits != 0 && (d->predictor_bits < 2 || d->predictor_bits > 9))
  {
    snprintf(why, nwhy, "predictor_bits %d is neither 0 nor in 2..9", (int)d->predictor_bits);
    return false;
  }
  if(d->entropy_bits != 0 && (d->entropy_bits < 2 || d->entropy_bits > 9))
  {
    snprintf(why, nwhy, "entropy_bits %d is neither 0 nor in 2..9", (int)d->entropy_bits);
    return false;
  }
  if(d->icc_bytes && !d->icc)
  {
    snprintf(why, nwhy, "icc_bytes %llu without an icc pointer", (unsigned long long)d->icc_bytes);
    return false;
  }
  if(d->icc && d->icc_bytes > WP_MAXICC)
  {
    snprintf(why, nwhy, "an ICC profile of %llu bytes is more than the %u this encoder takes", (unsigned long long)d->icc_bytes,
             (unsigned)WP_MAXICC);
    return false;
  }
  const uint32_t w = (uint32_t)width, h = (uint32_t)height;
  g->pb = d->predictor_bits ? d->predictor_bits : 5;
  g->bx = (w + (1u << g->pb) - 1) >> g->pb;
  g->by = (h + (1u << g->pb) - 1) >> g->pb;
  int eb = d->entropy_bits;
  if(!eb)
    for(eb = 6; eb < 9; eb++)
      if((uint64_t)((w + (1u << eb) - 1) >> eb) * ((h + (1u << eb) - 1) >> eb) <= 4096) break;
  g->eb = eb;
  g->tx = (w + (1u << eb) - 1) >> eb;
  g->ty = (h + (1u << eb) - 1) >> eb;
  const uint64_t ntiles = (uint64_t)g->tx * g->ty, nblocks = (uint64_t)g->bx * g->by;
  if(ntiles > WP_MAXTILES)
  {
    snprintf(why, nwhy, "entropy_bits %d gives %llu tiles, more than the %d the entropy image can index", eb,
             (unsigned long long)ntiles, WP_MAXTILES);
    return false;
  }
  g->N = (uint64_t)w * h;
  g->nseg = (g->N + WP_SEG - 1) / WP_SEG;
  const uint64_t icc = d->icc ? d->icc_bytes : 0;
  g->container = 12 + (icc ? 8 + 10 + 8 + icc + (icc & 1) : 0) + 8;
  const uint64_t bits = 128 + 2 * WP_GROUP_MAX_BITS + 4 * nblocks + 16 * ntiles + ntiles * WP_GROUP_MAX_BITS
                        + WP_PIXEL_MAX_BITS * g->N;
  g->bound = 8 + g->container + (bits + 7) / 8 + 2;
  return true;
}

// LSB-first bits into bytes
struct wp_bits_t
{
  std::vector<uint8_t> b;
  uint64_t pos = 0;
  void put(uint32_t v, int n)
  {
    for(int k = 0; k < n; k++, pos++)
    {
      if((pos >> 3) >= b.size()) b.push_back(0);
      b[pos >> 3] |= (uint8_t)(((v >> k) & 1) << (pos & 7));
    }
  }
};

// what the host knows of the file: `a` (a_bits bits from the file's first byte: the container, the VP8L header, the
// transforms up to the predictor image's codes), then 4 bits per predictor block (the device's), then `b` (b_bits bits:
// the end of the transforms, the main image's flags and the entropy image); the groups' codes start behind it
struct wp_head_t
{
  std::vector<uint8_t> a, b;
  uint64_t a_bits = 0, b_bits = 0;
  uint64_t vp8l_size_at = 0; // the byte offset of the VP8L chunk's size; the RIFF size is at 4
  uint64_t payload_at = 0;   // the payload's first byte
};

inline void wp_le32(std::vector<uint8_t> &o, uint32_t v)
{
  for(int k = 0; k < 4; k++) o.push_back((uint8_t)(v >> (8 * k)));
}

// the five codes of a sub-image whose green bytes take ngreen equally frequent values and whose red bytes nred
inline bool wp_fixed_group(int ngreen, int nred, int want_green, int want_red, wp_group_t *g)
{
  std::vector<wp_tab_work_t> tw(1); // the caller's own: several threads may encode at once
  std::vector<uint32_t> freq(WP_NSYM, 0);
  for(int i = 0; i < ngreen; i++) freq[i] = 1;
  for(int i = 0; i < nred; i++) freq[WP_NGREEN + i] = 1;
  wp_tables(tw.data(), freq.data(), 0, 1, [](uint64_t v) { return v; }, []() {}, g);
  for(int i = 0; i < ngreen; i++)
    if(g->len[i] != want_green) return false;
  for(int i = 0; i < nred; i++)
    if(g->len[WP_NGREEN + i] != want_red) return false;
  return true;
}

// false: the fixed codes did not come out as the device writes them (never)
inline bool wp_file_head(int width, int height, const wp_geom_t &g, const uint8_t *icc, size_t icc_bytes, wp_head_t *h)
{
  wp_bits_t o;
  std::vector<uint8_t> &c = o.b;
  c.insert(c.end(), { 'R', 'I', 'F', 'F', 0, 0, 0, 0, 'W', 'E', 'B', 'P' });
  if(icc && icc_bytes)
  {
    c.insert(c.end(), { 'V', 'P', '8', 'X' });
    wp_le32(c, 10);
    c.insert(c.end(), { 0x20, 0, 0, 0 });
    for(int k = 0; k < 3; k++) c.push_back((uint8_t)((uint32_t)(width - 1) >> (8 * k)));
    for(int k = 0; k < 3; k++) c.push_back((uint8_t)((uint32_t)(height - 1) >> (8 * k)));
    c.insert(c.end(), { 'I', 'C', 'C', 'P' });
    wp_le32(c, (uint32_t)icc_bytes);
    c.insert(c.end(), icc, icc + icc_bytes);
    if(icc_bytes & 1) c.push_back(0);
  }
  c.insert(c.end(), { 'V', 'P', '8', 'L' });
  h->vp8l_size_at = c.size();
  wp_le32(c, 0);
  h->payload_at = c.size();
  if(h->payload_at != g.container) return false;
  o.pos = 8 * (uint64_t)c.size();
  auto put = [&](uint32_t v, int n) { o.put(v, n); };
  put(0x2f, 8);
  put((uint32_t)width - 1, 14);
  put((uint32_t)height - 1, 14);
  put(0, 1); // alpha_is_used
  put(0, 3); // version
  put(1, 1);
  put(2, 2); // SUBTRACT_GREEN
  put(1, 1);
  put(0, 2); // PREDICTOR
  put((uint32_t)g.pb - 2, 3);
  // the predictor image: no colour cache; green 16 symbols of 4 bits (the modes 0..13 and two more, so that the code
  // is complete), the others one symbol
  wp_group_t fg;
  if(!wp_fixed_group(16, 0, 4, 0, &fg)) return false;
  put(0, 1);
  for(int a = 0; a < 5; a++) wp_code_header(&fg, a, put);
  h->a = o.b;
  h->a_bits = o.pos;
  wp_bits_t q;
  auto putb = [&](uint32_t v, int n) { q.put(v, n); };
  putb(0, 1); // no more transforms
  putb(0, 1); // no colour cache
  const uint32_t ntiles = g.tx * g.ty;
  putb(ntiles > 1 ? 1 : 0, 1);
  if(ntiles > 1)
  {
    // the entropy image: the tile's raster number in red << 8 | green, both bytes in 8 bits
    putb((uint32_t)g.eb - 2, 3);
    if(!wp_fixed_group(256, 256, 8, 8, &fg)) return false;
    putb(0, 1);
    for(int a = 0; a < 5; a++) wp_code_header(&fg, a, putb);
    for(uint32_t t = 0; t < ntiles; t++)
    {
      putb(wp_rev(t & 255, 8), 8);
      putb(wp_rev(t >> 8, 8), 8);
    }
  }
  h->b = q.b;
  h->b_bits = q.pos;
  return true;
}
