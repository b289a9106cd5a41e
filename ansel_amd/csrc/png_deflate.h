// png_deflate.h -- the body of the PNG encoder (png.hip), written once and compiled twice: the device kernels call
// these functions from their threads, and tests/native/png_host.cpp runs the same functions one after the other on
// the host, so the CPU suite checks the file against libpng and zlib and the device file equals the host build's.
//
// The filtered stream: libpng 1.6 png_write_find_filter() -- per row the sum of |signed byte| of None, Sub, Up,
// Average, Paeth in that order, a strict `<` replacing the best, bpp 3 (8 bits) or 6 (16 bits, big-endian samples),
// the first row against a zero row.
//
// The zlib stream: the filtered stream cut into segments of PD_SEG bytes, each one deflate block (only the last is
// BFINAL).  A segment's matches: a hash of the bytes at each position into a table of the most recent position with that hash,
// filled in steps of PD_STEP positions -- every position of a step looks the table up, then all of them enter it (the
// largest position wins, so the order of arrival does not matter).  The table starts with the PD_WIN bytes before the
// segment, so matches reach back into the previous segment; a match stays inside its own segment.  There are
// PD_NTAB such tables, keyed by 3, 4, ... bytes, and a position takes the longest of their candidates' matches.  The parse walks
// the segment: greedy at levels 1-3, one step of lazy evaluation at 4-9.  Each block is dynamic Huffman (codes limited
// to 15 / 7 bits by jh_build()), or fixed or stored when that is smaller.
#pragma once
#include <stdint.h>

#include "jpeg_huff.h"

#ifdef __HIPCC__
#define PD_FN __host__ __device__ __forceinline__
#else
#define PD_FN inline
#endif

#define PD_SEG 32768     // bytes of the filtered stream per segment (one deflate block)
#define PD_WIN 32768     // the window: distances 1..32768
#define PD_STEP 256      // positions per step of the hash table
#define PD_NTAB 4        // hash tables, each with the most recent position of its key
#define PD_TBITS 12      // entries per table: 1 << PD_TBITS
#define PD_KEY(t) (3 + (t)) // bytes keyed by table t: 3, 4, 5, 6
#define PD_MAXLEN 257    // the longest match kept (one byte per position holds len - 2)
#define PD_TOO_FAR 4096  // zlib's TOO_FAR: a 3-byte match further back than this is not taken
#define PD_NLIT 286
#define PD_NDIST 30
#define PD_NCL 19
#define PD_IDAT 65536    // data bytes per IDAT chunk (the last one shorter)
#define PD_STORED_MAX_BITS(n) (3 + 7 + 32 + 8 * (uint64_t)(n)) // a stored block of n bytes, worst padding

enum
{
  PD_STORED = 0,
  PD_FIXED = 1,
  PD_DYNAMIC = 2
};

// ---------------------------------------------------------------------------------------------------------------------
// filter

// byte j (0 .. w * bpp - 1) of row y of the raw PNG row: RGB of RGBA u8, or big-endian RGB of RGBA u16 (alpha dropped)
PD_FN uint32_t pf_raw(const void *in, int w, int depth, int y, uint32_t j)
{
  if(depth == 8)
  {
    const uint32_t px = j / 3, c = j - px * 3;
    return ((const uint8_t *)in)[((size_t)y * w + px) * 4 + c];
  }
  const uint32_t px = j / 6, k = j - px * 6;
  const uint32_t v = ((const uint16_t *)in)[((size_t)y * w + px) * 4 + (k >> 1)];
  return (k & 1) ? (v & 255) : (v >> 8);
}

// the filtered byte of filter f (0 None .. 4 Paeth) from x and its neighbours a (left), b (up), c (up-left)
PD_FN uint32_t pf_residual(int f, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
  switch(f)
  {
    case 0: return x;
    case 1: return (x - a) & 255;
    case 2: return (x - b) & 255;
    case 3: return (x - ((a + b) >> 1)) & 255;
    default:
    {
      const int p = (int)b - (int)c, pc0 = (int)a - (int)c;
      const int pa = p < 0 ? -p : p, pb = pc0 < 0 ? -pc0 : pc0, pcc = (p + pc0) < 0 ? -(p + pc0) : (p + pc0);
      const uint32_t pr = (pa <= pb && pa <= pcc) ? a : (pb <= pcc) ? b : c;
      return (x - pr) & 255;
    }
  }
}

// libpng's cost of one filtered byte: |v| as a signed byte
PD_FN uint32_t pf_cost(uint32_t v) { return v < 128 ? v : 256 - v; }

// the five residuals of byte j of row y (its row above: y - 1, or zeros for the first row)
PD_FN void pf_byte(const void *in, int w, int depth, int y, uint32_t j, uint32_t r[5])
{
  const uint32_t bpp = depth == 8 ? 3 : 6;
  const uint32_t x = pf_raw(in, w, depth, y, j);
  const uint32_t a = j >= bpp ? pf_raw(in, w, depth, y, j - bpp) : 0;
  const uint32_t b = y > 0 ? pf_raw(in, w, depth, y - 1, j) : 0;
  const uint32_t c = (y > 0 && j >= bpp) ? pf_raw(in, w, depth, y - 1, j - bpp) : 0;
  for(int f = 0; f < 5; f++) r[f] = pf_residual(f, x, a, b, c);
}

// the choice among the five sums: None first, a strict `<` to replace the best
PD_FN int pf_choose(const uint64_t sum[5])
{
  int best = 0;
  for(int f = 1; f < 5; f++)
    if(sum[f] < sum[best]) best = f;
  return best;
}

// ---------------------------------------------------------------------------------------------------------------------
// matching and parsing

// the slot of position p in hash table t: table t is keyed by the PD_KEY(t) bytes at p (PD_NTAB tables of
// 1 << PD_TBITS entries, one array)
PD_FN uint32_t pd_slot(const uint8_t *s, uint64_t p, int t)
{
  uint32_t v = ((uint32_t)s[p] << 16) | ((uint32_t)s[p + 1] << 8) | s[p + 2];
  v *= 2654435761u;
  for(int k = 3; k < PD_KEY(t); k++) v = (v ^ s[p + k]) * 2246822519u;
  return ((uint32_t)t << PD_TBITS) | (v >> (32 - PD_TBITS));
}

// can position p enter table t (its key lies inside the stream)?
PD_FN bool pd_keyed(uint64_t p, uint64_t N, int t) { return p + PD_KEY(t) <= N; }

// the match of position p against the earlier position q (q < p), at most maxlen bytes; 0 when not taken
PD_FN uint32_t pd_match(const uint8_t *s, uint64_t p, uint64_t q, uint32_t maxlen)
{
  const uint64_t dist = p - q;
  if(dist > PD_WIN) return 0;
  uint32_t l = 0;
  while(l < maxlen && s[q + l] == s[p + l]) l++;
  if(l < 3 || (l == 3 && dist > PD_TOO_FAR)) return 0;
  return l;
}

// the match of position p (earlier positions window_start + head(slot), head() < 0: none): the longest over the
// tables, the nearer on a tie; *dist its distance; 0 when none is taken
template <class Head>
PD_FN uint32_t pd_best(const uint8_t *s, uint64_t N, uint64_t p, uint64_t window_start, uint32_t maxlen, Head head,
                       uint32_t *dist)
{
  uint32_t bl = 0, bd = 0;
  for(int t = 0; t < PD_NTAB; t++)
  {
    if(!pd_keyed(p, N, t)) break;
    const int32_t q = head(pd_slot(s, p, t));
    if(q < 0) continue;
    const uint32_t d = (uint32_t)(p - window_start - (uint64_t)q);
    if(bl && d == bd) continue;
    const uint32_t l = pd_match(s, p, window_start + q, maxlen);
    if(l > bl || (l && l == bl && d < bd))
    {
      bl = l;
      bd = d;
    }
  }
  *dist = bd;
  return bl;
}

// the parse's rule at one position: take the match of length l (> 0) here, given the next position's length ln?
PD_FN bool pd_take(uint32_t l, uint32_t ln, int level) { return l >= 3 && !(level >= 4 && ln > l); }

// ---------------------------------------------------------------------------------------------------------------------
// symbols

// literal / length symbol of a match length 3..258, its extra bits and their value
PD_FN uint32_t pd_len_sym(uint32_t len, uint32_t *nextra, uint32_t *extra)
{
  const uint32_t l = len - 3;
  if(l < 8)
  {
    *nextra = 0;
    *extra = 0;
    return 257 + l;
  }
  if(l == 255)
  {
    *nextra = 0;
    *extra = 0;
    return 285;
  }
  uint32_t k = 31;
  while(!(l >> k)) k--;
  *nextra = k - 2;
  *extra = l & ((1u << (k - 2)) - 1);
  return 257 + 4 * (k - 1) + ((l >> (k - 2)) & 3);
}

// distance symbol of a distance 1..32768, its extra bits and their value
PD_FN uint32_t pd_dist_sym(uint32_t dist, uint32_t *nextra, uint32_t *extra)
{
  const uint32_t d = dist - 1;
  if(d < 4)
  {
    *nextra = 0;
    *extra = 0;
    return d;
  }
  uint32_t k = 31;
  while(!(d >> k)) k--;
  *nextra = k - 1;
  *extra = d & ((1u << (k - 1)) - 1);
  return 2 * k + ((d >> (k - 1)) & 1);
}

PD_FN uint32_t pd_lit_extra(int s) { return (s >= 265 && s < 285) ? (uint32_t)(s - 261) / 4 : 0; }
PD_FN uint32_t pd_dist_extra(int s) { return s >= 4 ? (uint32_t)s / 2 - 1 : 0; }
PD_FN uint32_t pd_fixed_lit_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// the order of the code length code lengths in the block header
PD_FN int pd_cl_order(int i)
{
  const uint8_t o[PD_NCL] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
  return o[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// one segment's block: tables, header, choice

// the per-segment record the tables build and the emission reads
struct pd_seg_t
{
  uint32_t type;   // PD_STORED / PD_FIXED / PD_DYNAMIC
  uint32_t nbytes; // bytes of the filtered stream in the segment
  uint64_t bits;   // fixed / dynamic: the block's bits, header included (stored: see pd_stored_end())
  uint32_t nlit, ndist, ncl;
  uint32_t adler_s, adler_t; // sum of the bytes, sum of (nbytes - j) * byte_j, both mod 65521
  uint8_t len[PD_NLIT + PD_NDIST]; // code lengths: literal / length, then distance
  uint8_t cl_len[PD_NCL];
};

// canonical codes (bit-reversed for LSB-first output) from code lengths; fixed_lit: the fixed literal / length code,
// whose symbols 286 and 287 (8 bits, never sent) take their place in the count
PD_FN void pd_codes(const uint8_t *len, int n, uint16_t *code, bool fixed_lit = false)
{
  uint32_t count[16] = { 0 }, next[16];
  for(int i = 0; i < n; i++) count[len[i]]++;
  count[0] = 0;
  if(fixed_lit) count[8] += 2;
  uint32_t c = 0;
  for(int l = 1; l < 16; l++)
  {
    c = (c + count[l - 1]) << 1;
    next[l] = c;
  }
  for(int i = 0; i < n; i++)
  {
    const int l = len[i];
    if(!l) continue;
    uint32_t v = next[l]++, r = 0;
    for(int k = 0; k < l; k++) r |= ((v >> k) & 1) << (l - 1 - k);
    code[i] = (uint16_t)r;
  }
}

// the run-length coding of the code lengths (literal / length then distance, one sequence): emit(symbol, extra, nbits)
template <class F>
PD_FN void pd_rle(const uint8_t *len, int nlit, int ndist, F emit)
{
  const int n = nlit + ndist;
  auto at = [&](int i) { return i < nlit ? len[i] : len[PD_NLIT + i - nlit]; };
  int i = 0;
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
      emit(v, 0u, 0);
      r--;
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

// the code lengths of one alphabet from its counts (at least two symbols get a code: zero counts are raised to 1 from
// symbol 0 up, so that every code is complete); lane / nlanes / wave_min / sync as jh_build().  longest (tests; the
// kernels pass none): the longest code length before the Annex K.3 adjustment
template <class WaveMin, class Sync>
PD_FN void pd_lengths(jh_work_t *w, const uint32_t *freq, int n, int limit, int lane, int nlanes, WaveMin wave_min,
                      Sync sync, uint8_t *bits, uint16_t *vals, uint8_t *len_out, int *longest = nullptr)
{
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
  const int nv = jh_build(w, n, limit, false, lane, nlanes, wave_min, sync, bits, vals);
  if(lane == 0)
  {
    for(int i = 0; i < n; i++) len_out[i] = 0;
    int p = 0;
    for(int l = 1; l <= limit; l++)
      for(int k = 0; k < bits[l - 1]; k++) len_out[vals[p++]] = (uint8_t)l;
    (void)nv;
    if(longest)
    {
      *longest = 0;
      for(int i = 0; i < n; i++)
        if(w->codesize[i] > *longest) *longest = w->codesize[i];
    }
  }
  sync();
}

// the work area of pd_tables()
struct pd_tab_work_t
{
  jh_work_t w;
  uint32_t clfreq[PD_NCL];
  uint8_t bits[16];
  uint16_t vals[JH_MAX_SYM];
};

// the block of one segment from its symbol counts (freq: PD_NLIT literal / length, then PD_NDIST distance counts; the
// stream's byte count nbytes; level 0: stored).  Fills every field of *seg but the Adler sums.  longest (tests; the
// kernels pass none): three words, the longest unadjusted code length of the literal / length, distance and code
// length alphabets (pd_lengths())
template <class WaveMin, class Sync>
PD_FN void pd_tables(pd_tab_work_t *tw, const uint32_t *freq, uint32_t nbytes, int level, int lane, int nlanes,
                     WaveMin wave_min, Sync sync, pd_seg_t *seg, int *longest = nullptr)
{
  if(level == 0)
  {
    if(lane == 0)
    {
      seg->type = PD_STORED;
      seg->nbytes = nbytes;
      seg->bits = 0;
      seg->nlit = seg->ndist = seg->ncl = 0;
    }
    return;
  }
  pd_lengths(&tw->w, freq, PD_NLIT, 15, lane, nlanes, wave_min, sync, tw->bits, tw->vals, seg->len,
             longest);
  pd_lengths(&tw->w, freq + PD_NLIT, PD_NDIST, 15, lane, nlanes, wave_min, sync, tw->bits, tw->vals,
             seg->len + PD_NLIT, longest ? longest + 1 : nullptr);
  uint32_t nlit = PD_NLIT, ndist = PD_NDIST;
  if(lane == 0)
  {
    while(nlit > 257 && seg->len[nlit - 1] == 0) nlit--;
    while(ndist > 1 && seg->len[PD_NLIT + ndist - 1] == 0) ndist--;
    for(int i = 0; i < PD_NCL; i++) tw->clfreq[i] = 0;
    pd_rle(seg->len, (int)nlit, (int)ndist, [&](int s, uint32_t, int) { tw->clfreq[s]++; });
  }
  sync();
  pd_lengths(&tw->w, tw->clfreq, PD_NCL, 7, lane, nlanes, wave_min, sync, tw->bits, tw->vals, seg->cl_len,
             longest ? longest + 2 : nullptr);
  if(lane == 0)
  {
    uint32_t ncl = PD_NCL;
    while(ncl > 4 && seg->cl_len[pd_cl_order(ncl - 1)] == 0) ncl--;
    uint64_t dyn = 3 + 5 + 5 + 4 + 3 * (uint64_t)ncl, fix = 3;
    for(int s = 0; s < PD_NCL; s++)
      dyn += (uint64_t)tw->clfreq[s] * (seg->cl_len[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
    for(int s = 0; s < PD_NLIT; s++)
    {
      dyn += (uint64_t)freq[s] * (seg->len[s] + pd_lit_extra(s));
      fix += (uint64_t)freq[s] * (pd_fixed_lit_len(s) + pd_lit_extra(s));
    }
    for(int s = 0; s < PD_NDIST; s++)
    {
      dyn += (uint64_t)freq[PD_NLIT + s] * (seg->len[PD_NLIT + s] + pd_dist_extra(s));
      fix += (uint64_t)freq[PD_NLIT + s] * (5 + pd_dist_extra(s));
    }
    const uint64_t sto = PD_STORED_MAX_BITS(nbytes);
    seg->nbytes = nbytes;
    seg->nlit = nlit;
    seg->ndist = ndist;
    seg->ncl = ncl;
    if(dyn <= fix && dyn <= sto)
    {
      seg->type = PD_DYNAMIC;
      seg->bits = dyn;
    }
    else if(fix <= sto)
    {
      seg->type = PD_FIXED;
      seg->bits = fix;
      for(int s = 0; s < PD_NLIT; s++) seg->len[s] = (uint8_t)pd_fixed_lit_len(s);
      for(int s = 0; s < PD_NDIST; s++) seg->len[PD_NLIT + s] = 5;
    }
    else
    {
      seg->type = PD_STORED;
      seg->bits = 0;
    }
  }
  sync();
}

// the bit offset behind a segment that starts at bit o
PD_FN uint64_t pd_seg_end(const pd_seg_t &s, uint64_t o)
{
  if(s.type != PD_STORED) return o + s.bits;
  return ((o + 3 + 7) & ~(uint64_t)7) + 32 + 8 * (uint64_t)s.nbytes;
}

// the block header of a fixed or dynamic segment: put(value, nbits), LSB first
template <class Put>
PD_FN void pd_block_header(const pd_seg_t &s, bool last, const uint16_t *cl_code, Put put)
{
  put((last ? 1u : 0u) | ((uint32_t)s.type << 1), 3);
  if(s.type != PD_DYNAMIC) return;
  put(s.nlit - 257, 5);
  put(s.ndist - 1, 5);
  put(s.ncl - 4, 4);
  for(uint32_t i = 0; i < s.ncl; i++) put(s.cl_len[pd_cl_order(i)], 3);
  pd_rle(s.len, (int)s.nlit, (int)s.ndist, [&](int sym, uint32_t extra, int nb) {
    put(cl_code[sym], s.cl_len[sym]);
    if(nb) put(extra, nb);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// checksums

#define PD_ADLER_MOD 65521u

// CRC-32 (reflected, polynomial 0xedb88320): zlib's multmodp / x2nmodp, so that crc(A B) = shift(crc(A), |B|) ^ crc(B)
PD_FN uint32_t pd_multmodp(uint32_t a, uint32_t b)
{
  uint32_t m = 1u << 31, p = 0;
  for(;;)
  {
    if(a & m)
    {
      p ^= b;
      if((a & (m - 1)) == 0) break;
    }
    m >>= 1;
    b = b & 1 ? (b >> 1) ^ 0xedb88320u : b >> 1;
  }
  return p;
}

// x^(8 n) mod p: the shift of a CRC by n zero bytes
PD_FN uint32_t pd_x8n(uint64_t n)
{
  uint32_t x2k = 1u << 30; // x^1
  for(int k = 0; k < 3; k++) x2k = pd_multmodp(x2k, x2k);
  uint32_t p = 1u << 31;
  while(n)
  {
    if(n & 1) p = pd_multmodp(x2k, p);
    x2k = pd_multmodp(x2k, x2k);
    n >>= 1;
  }
  return p;
}

PD_FN uint32_t pd_crc_byte(uint32_t c, uint32_t b)
{
  c ^= b;
  for(int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ 0xedb88320u : c >> 1;
  return c;
}

// the standard CRC-32 of n bytes
PD_FN uint32_t pd_crc(const uint8_t *p, uint64_t n)
{
  uint32_t c = 0xffffffffu;
  for(uint64_t i = 0; i < n; i++) c = pd_crc_byte(c, p[i]);
  return ~c;
}

// ---------------------------------------------------------------------------------------------------------------------
// framing (host)

#include <vector>

// zlib's header: CMF 0x78 (deflate, 32 KB window), FLEVEL by deflate.c's rule, FCHECK
inline uint16_t pd_zlib_header(int level)
{
  const uint32_t flags = level < 2 ? 0 : level < 6 ? 1 : level == 6 ? 2 : 3;
  uint32_t h = (0x78u << 8) | (flags << 6);
  h += 31 - h % 31;
  return (uint16_t)h;
}

inline void pd_be32(std::vector<uint8_t> &o, uint32_t v)
{
  for(int k = 3; k >= 0; k--) o.push_back((uint8_t)(v >> (8 * k)));
}

inline void pd_chunk(std::vector<uint8_t> &o, const char *type, const uint8_t *data, size_t n)
{
  pd_be32(o, (uint32_t)n);
  const size_t at = o.size();
  o.insert(o.end(), type, type + 4);
  o.insert(o.end(), data, data + n);
  pd_be32(o, pd_crc(o.data() + at, 4 + n));
}

// the iCCP payload's zlib stream: stored blocks of at most 65535 bytes
inline std::vector<uint8_t> pd_zlib_stored(const uint8_t *p, size_t n)
{
  std::vector<uint8_t> o = { 0x78, 0x01 };
  size_t i = 0;
  do
  {
    const size_t k = n - i < 65535 ? n - i : 65535;
    o.push_back(i + k == n ? 1 : 0);
    o.push_back((uint8_t)k);
    o.push_back((uint8_t)(k >> 8));
    o.push_back((uint8_t)~k);
    o.push_back((uint8_t)(~k >> 8));
    o.insert(o.end(), p + i, p + i + k);
    i += k;
  } while(i < n);
  uint32_t a = 1, b = 0;
  for(size_t j = 0; j < n; j++)
  {
    a = (a + p[j]) % PD_ADLER_MOD;
    b = (b + a) % PD_ADLER_MOD;
  }
  pd_be32(o, (b << 16) | a);
  return o;
}

// the pixels per metre of a pHYs chunk for dpi
inline uint32_t pd_ppm(int dpi) { return (uint32_t)((double)dpi / 0.0254 + 0.5); }

// the bytes in front of the first IDAT: signature, IHDR, iCCP (profile name "icc"), pHYs
inline std::vector<uint8_t> pd_file_head(int w, int h, int depth, const uint8_t *icc, size_t icc_bytes, int dpi)
{
  std::vector<uint8_t> o = { 0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a };
  std::vector<uint8_t> ihdr;
  pd_be32(ihdr, (uint32_t)w);
  pd_be32(ihdr, (uint32_t)h);
  ihdr.push_back((uint8_t)depth);
  ihdr.push_back(2); // RGB
  ihdr.push_back(0);
  ihdr.push_back(0);
  ihdr.push_back(0);
  pd_chunk(o, "IHDR", ihdr.data(), ihdr.size());
  if(icc && icc_bytes)
  {
    std::vector<uint8_t> p = { 'i', 'c', 'c', 0, 0 };
    const std::vector<uint8_t> z = pd_zlib_stored(icc, icc_bytes);
    p.insert(p.end(), z.begin(), z.end());
    pd_chunk(o, "iCCP", p.data(), p.size());
  }
  if(dpi > 0)
  {
    std::vector<uint8_t> p;
    pd_be32(p, pd_ppm(dpi));
    pd_be32(p, pd_ppm(dpi));
    p.push_back(1); // metre
    pd_chunk(o, "pHYs", p.data(), p.size());
  }
  return o;
}

// the iCCP chunk's size for a profile of n bytes (0: none)
inline uint64_t pd_iccp_bytes(uint64_t n) { return n ? 12 + 5 + 2 + 5 * ((n + 65534) / 65535) + n + 4 : 0; }
