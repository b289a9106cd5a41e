// jpeg_huff.h -- the Huffman table builder of the JPEG encoder (jpeg.hip), written once and compiled twice: on gfx950
// one wave of 64 lanes builds one table, and tests/native/jpeg_huff_host.cpp runs the same body with one lane on the
// host, so the CPU suite checks it against libjpeg's tables.
//
// jh_gen_optimal_table() is jchuff.c jpeg_gen_optimal_table() (T.81 Annex K.2): the reserved pseudo-symbol 256 with a
// count of 1, repeated merging of the two least frequent nodes -- "least" taken as libjpeg's upward scan with
// `freq[i] <= v` takes it: the largest index among equal counts, and counts above 10^9 never chosen --, code lengths
// limited to 16 by the Annex K.3 adjustment, and the values sorted by their unadjusted length, then value.  The two
// minimum searches of a merge are the only work over all 257 symbols; each lane scans its share and the wave
// reduces one key (count << 9 | 511 - symbol) with `wave_min`.  The bookkeeping of a merge is serial and runs on
// lane 0 between two `sync()`s.
//
// jh_build() is that body with the alphabet, the length limit and the reserved pseudo-symbol as arguments: the PNG
// encoder's deflate (png_deflate.h) builds its 286 / 30 / 19-symbol codes with it, limited to 15 / 15 / 7 bits and
// without the pseudo-symbol, so that each code is complete as inflate requires (the K.3 moves keep the Kraft sum).  The
// WebP encoder (webp_body.h) builds its 280 / 256 / 40 / 19-symbol codes with it too, and calls it on the host of a HIP
// translation unit for the fixed codes of its sub-images: under hipcc the functions are __host__ __device__.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define JH_FN __host__ __device__ __forceinline__
#else
#define JH_FN inline
#endif

#define JH_NSYM 257
#define JH_MAX_SYM 288 // the work arrays: JPEG's 256 symbols + 1, deflate's 286 literal / length symbols
#define JH_MAX_CLEN 32

struct jh_work_t
{
  int64_t freq[JH_MAX_SYM]; // caller fills the real symbols; the pseudo-symbol is set here
  int32_t codesize[JH_MAX_SYM];
  int32_t others[JH_MAX_SYM];
  int32_t bits[JH_MAX_CLEN + 1];
  int32_t start[JH_MAX_CLEN + 2];
};

// the lane-local part of one minimum search: the smallest key among this lane's eligible symbols (~0: none)
JH_FN uint64_t jh_local_min(const jh_work_t *w, int nsym, int lane, int nlanes, int skip)
{
  uint64_t k = ~0ull;
  for(int i = lane; i < nsym; i += nlanes)
  {
    const int64_t f = w->freq[i];
    if(f != 0 && f <= 1000000000LL && i != skip)
    {
      const uint64_t key = ((uint64_t)f << 9) | (uint64_t)(511 - i);
      if(key < k) k = key;
    }
  }
  return k;
}

// bits_out[0..limit-1]: the number of codes of length 1..limit; vals_out: the symbols in code order; returns their
// count.  nreal symbols 0..nreal-1 (freq filled by the caller); reserve: the pseudo-symbol nreal with a count of 1,
// whose code (the all-ones one) is dropped at the end.  All lanes of the group call it; only lane 0 writes bits_out /
// vals_out.
template <class V, class WaveMin, class Sync>
JH_FN int jh_build(jh_work_t *w, int nreal, int limit, bool reserve, int lane, int nlanes, WaveMin wave_min, Sync sync,
                   uint8_t *bits_out, V *vals_out)
{
  const int nsym = nreal + (reserve ? 1 : 0);
  for(int i = lane; i < nsym; i += nlanes)
  {
    w->codesize[i] = 0;
    w->others[i] = -1;
  }
  if(lane == 0 && reserve) w->freq[nreal] = 1;
  sync();
  for(;;)
  {
    const uint64_t k1 = wave_min(jh_local_min(w, nsym, lane, nlanes, -1));
    if(k1 == ~0ull) break;
    int c1 = 511 - (int)(k1 & 511);
    const uint64_t k2 = wave_min(jh_local_min(w, nsym, lane, nlanes, c1));
    if(k2 == ~0ull) break;
    int c2 = 511 - (int)(k2 & 511);
    sync();
    if(lane == 0)
    {
      w->freq[c1] += w->freq[c2];
      w->freq[c2] = 0;
      w->codesize[c1]++;
      while(w->others[c1] >= 0)
      {
        c1 = w->others[c1];
        w->codesize[c1]++;
      }
      w->others[c1] = c2;
      w->codesize[c2]++;
      while(w->others[c2] >= 0)
      {
        c2 = w->others[c2];
        w->codesize[c2]++;
      }
    }
    sync();
  }
  int nvals = 0;
  if(lane == 0)
  {
    for(int i = 0; i <= JH_MAX_CLEN; i++) w->bits[i] = 0;
    for(int i = 0; i < nsym; i++)
    {
      int cs = w->codesize[i];
      if(cs > JH_MAX_CLEN) cs = JH_MAX_CLEN; // libjpeg stops with an error here; counts below 2^31 cannot get there
      w->codesize[i] = cs;
      if(cs) w->bits[cs]++;
    }
    // the values' order: by unadjusted length, then value (the pseudo-symbol excluded)
    for(int i = 0; i <= JH_MAX_CLEN + 1; i++) w->start[i] = 0;
    for(int j = 0; j < nreal; j++)
      if(w->codesize[j]) w->start[w->codesize[j] + 1]++;
    for(int i = 1; i <= JH_MAX_CLEN + 1; i++) w->start[i] += w->start[i - 1];
    for(int j = 0; j < nreal; j++)
      if(w->codesize[j]) vals_out[w->start[w->codesize[j]]++] = (V)j;
    nvals = w->start[JH_MAX_CLEN];
    // Annex K.3: no code longer than `limit` bits
    for(int i = JH_MAX_CLEN; i > limit; i--)
    {
      while(w->bits[i] > 0)
      {
        int j = i - 2;
        while(w->bits[j] == 0) j--;
        w->bits[i] -= 2;
        w->bits[i - 1]++;
        w->bits[j + 1] += 2;
        w->bits[j]--;
      }
    }
    if(reserve)
    {
      int i = limit;
      while(w->bits[i] == 0) i--;
      w->bits[i]--; // the pseudo-symbol's code
    }
    for(int l = 1; l <= limit; l++) bits_out[l - 1] = (uint8_t)w->bits[l];
  }
  return nvals;
}

// JPEG: 256 symbols and the pseudo-symbol 256, codes of at most 16 bits
template <class WaveMin, class Sync>
JH_FN int jh_gen_optimal_table(jh_work_t *w, int lane, int nlanes, WaveMin wave_min, Sync sync, uint8_t *bits_out,
                               uint8_t *vals_out)
{
  return jh_build(w, 256, 16, true, lane, nlanes, wave_min, sync, bits_out, vals_out);
}

// jchuff.c jpeg_make_c_derived_tbl(): code and length per symbol (length 0: no code)
JH_FN void jh_derive(const uint8_t *bits, const uint8_t *vals, uint16_t *code, uint8_t *size)
{
  for(int s = 0; s < 256; s++) size[s] = 0;
  unsigned c = 0;
  int p = 0;
  for(int l = 1; l <= 16; l++)
  {
    for(int n = 0; n < bits[l - 1]; n++)
    {
      code[vals[p]] = (uint16_t)c;
      size[vals[p]] = (uint8_t)l;
      c++;
      p++;
    }
    c <<= 1;
  }
}
