// deflate_kernels.h -- the device side of png_deflate.h's deflate, shared by png.hip (one zlib stream: the filtered
// frame) and tiff.hip (one zlib stream per strip): a workgroup's work on ONE segment of ONE stream, the stream and the
// segment's bounds being arguments.  A stream is N bytes at `s`; its segment is [s0, s1) of it (s0 a multiple of
// PD_SEG), the hash tables start at most PD_WIN bytes before s0 and never in front of the stream, a match stays inside
// its segment, and the block is BFINAL when the caller says so.  The callers' kernels map blockIdx.x to (stream,
// segment) and hand in pointers that already point at the stream's / the segment's records.
#pragma once
#include "hip_common.h"
#include "png_deflate.h"

namespace ansel
{
namespace
{

constexpr int PT = 256;                     // threads per workgroup (the tables: 64)
constexpr int SEG_WORDS = PD_SEG / 64;      // 64-bit token masks per segment
constexpr int SEG_PER_THREAD = PD_SEG / PT; // positions per thread in the emission
constexpr int NSYM = PD_NLIT + PD_NDIST;

template <class T>
__device__ __forceinline__ T block_sum(T v)
{
  __shared__ T s[PT];
  s[threadIdx.x] = v;
  __syncthreads();
  for(int o = PT / 2; o > 0; o >>= 1)
  {
    if((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  const T r = s[0];
  __syncthreads();
  return r;
}

template <class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *total)
{
  __shared__ T s[PT];
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for(int o = 1; o < PT; o <<= 1)
  {
    const T a = t >= o ? s[t - o] : (T)0;
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  const T incl = s[t];
  *total = s[PT - 1];
  __syncthreads();
  return incl - v;
}

// one segment [s0, s1) of the stream s[0 .. N): the Adler-32 sums; at level > 0 the matches (m, indexed by the
// stream's positions: len << 16 | dist - 1, at the positions that have one), the parse (tokm: a token starts here,
// matm: that token is a match; both the segment's SEG_WORDS words) and the symbol counts (freq: the segment's NSYM)
__device__ __forceinline__ void dk_lz_segment(const uint8_t *__restrict__ s, const uint64_t N, const uint64_t s0,
                                              const uint64_t s1, const int level, uint32_t *__restrict__ m,
                                              uint64_t *__restrict__ tokm, uint64_t *__restrict__ matm,
                                              uint32_t *__restrict__ freq, pd_seg_t *__restrict__ seg)
{
  __shared__ int32_t head[PD_NTAB << PD_TBITS];
  __shared__ uint8_t lenv[PD_SEG];
  __shared__ uint64_t tk[SEG_WORDS], mt[SEG_WORDS];
  __shared__ uint32_t hist[NSYM];
  const int tid = threadIdx.x;
  const uint32_t n = (uint32_t)(s1 - s0);
  {
    uint64_t S = 0, T = 0;
    for(uint32_t j = tid; j < n; j += PT)
    {
      const uint32_t x = s[s0 + j];
      S += x;
      T += (uint64_t)(n - j) * x;
    }
    S = block_sum<uint64_t>(S);
    T = block_sum<uint64_t>(T);
    if(tid == 0)
    {
      seg->adler_s = (uint32_t)(S % PD_ADLER_MOD);
      seg->adler_t = (uint32_t)(T % PD_ADLER_MOD);
    }
  }
  if(level == 0) return;
  for(int i = tid; i < (PD_NTAB << PD_TBITS); i += PT) head[i] = -1;
  for(int i = tid; i < PD_SEG; i += PT) lenv[i] = 0;
  for(int i = tid; i < NSYM; i += PT) hist[i] = 0;
  __syncthreads();
  const uint64_t ws = s0 > PD_WIN ? s0 - PD_WIN : 0;
  for(uint64_t c = ws; c < s1; c += PD_STEP)
  {
    const uint64_t p = c + tid;
    if(p < s1 && p >= s0)
    {
      uint32_t dist;
      const uint32_t l = pd_best(s, N, p, ws, (uint32_t)min<uint64_t>(PD_MAXLEN, s1 - p),
                                 [&](uint32_t slot) { return head[slot]; }, &dist);
      if(l)
      {
        lenv[p - s0] = (uint8_t)(l - 2);
        m[p] = (l << 16) | (dist - 1);
      }
    }
    __syncthreads();
    if(p < s1)
      for(int t = 0; t < PD_NTAB && pd_keyed(p, N, t); t++) atomicMax(&head[pd_slot(s, p, t)], (int32_t)(p - ws));
    __syncthreads();
  }
  // the parse: wave 0, 64 positions' lengths per step in registers, the walk on the wave's uniform position
  if(tid < 64)
  {
    const int lane = tid;
    uint32_t q = 0;
    for(uint32_t base = 0; base < n; base += 64)
    {
      const int lv = base + lane < n ? lenv[base + lane] : 0;
      const int lv2 = base + 64 + lane < n ? lenv[base + 64 + lane] : 0;
      uint64_t tkm = 0, mtm = 0;
      while(q < base + 64 && q < n)
      {
        const int i = (int)(q - base);
        const int lr = __builtin_amdgcn_readlane(lv, i);
        const int lnr = i + 1 < 64 ? __builtin_amdgcn_readlane(lv, i + 1) : __builtin_amdgcn_readlane(lv2, 0);
        const uint32_t l = lr ? lr + 2 : 0, ln = (q + 1 < n && lnr) ? lnr + 2 : 0;
        tkm |= 1ull << i;
        if(pd_take(l, ln, level))
        {
          mtm |= 1ull << i;
          q += l;
        }
        else
          q++;
      }
      if(lane == 0)
      {
        tk[base / 64] = tkm;
        mt[base / 64] = mtm;
      }
    }
  }
  __syncthreads();
  for(uint32_t j = tid; j < n; j += PT)
  {
    if(!((tk[j >> 6] >> (j & 63)) & 1)) continue;
    if((mt[j >> 6] >> (j & 63)) & 1)
    {
      const uint32_t v = m[s0 + j];
      uint32_t ne, ex;
      atomicAdd(&hist[pd_len_sym(v >> 16, &ne, &ex)], 1u);
      atomicAdd(&hist[PD_NLIT + pd_dist_sym((v & 0xffff) + 1, &ne, &ex)], 1u);
    }
    else
      atomicAdd(&hist[s[s0 + j]], 1u);
  }
  __syncthreads();
  for(int i = tid; i < NSYM; i += PT) freq[i] = hist[i] + (i == 256 ? 1u : 0u);
  for(uint32_t i = tid; i < (n + 63) / 64; i += PT)
  {
    tokm[i] = tk[i];
    matm[i] = mt[i];
  }
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#pragma unroll
  for(int o = 32; o > 0; o >>= 1)
  {
    const uint64_t other = __shfl_xor(v, o, 64);
    v = other < v ? other : v;
  }
  return v;
}

// one wave: the code lengths and the block type of a segment of n bytes from its NSYM counts (pd_tables)
__device__ __forceinline__ void dk_tables_segment(const uint32_t *__restrict__ freq, const uint32_t n, const int level,
                                                  pd_seg_t *__restrict__ seg)
{
  __shared__ pd_tab_work_t tw;
  __shared__ uint32_t f[NSYM];
  if(level > 0)
    for(int i = threadIdx.x; i < NSYM; i += 64) f[i] = freq[i];
  __syncthreads();
  pd_tables(
      &tw, f, n, level, threadIdx.x, 64, [](uint64_t v) { return wave_min_u64(v); }, []() { __syncthreads(); }, seg);
}

__device__ __forceinline__ uint64_t align8(uint64_t v) { return (v + 7) & ~(uint64_t)7; }

__device__ __forceinline__ void or_byte(uint32_t *words, uint64_t i, uint32_t v)
{
  atomicOr(&words[i >> 2], (v & 255) << (8 * (i & 3)));
}

// nb (<= 25) bits at bit offset o, LSB first
__device__ __forceinline__ void or_bits(uint32_t *words, uint64_t o, uint32_t v, int nb)
{
  const uint64_t x = (uint64_t)v << (o & 31);
  atomicOr(&words[o >> 5], (uint32_t)x);
  if((o & 31) + nb > 32) atomicOr(&words[(o >> 5) + 1], (uint32_t)(x >> 32));
}

// LSB-first writer from bit `start`: the first and the last word it touches are ORed, the words between stored
struct writer_t
{
  uint32_t *words;
  uint64_t acc;
  int nacc;
  uint64_t wi;
  bool first;
  __device__ writer_t(uint32_t *w, uint64_t start) : words(w), acc(0), nacc((int)(start & 31)), wi(start >> 5), first(true) {}
  __device__ __forceinline__ void put(uint32_t v, int nb)
  {
    acc |= (uint64_t)v << nacc;
    nacc += nb;
    if(nacc >= 32)
    {
      if(first)
        atomicOr(&words[wi], (uint32_t)acc);
      else
        words[wi] = (uint32_t)acc;
      first = false;
      wi++;
      acc >>= 32;
      nacc -= 32;
    }
  }
  __device__ __forceinline__ void flush()
  {
    if(nacc > 0) atomicOr(&words[wi], (uint32_t)acc);
  }
};

// the block of one segment at bit offset o of the zeroed words: s the stream, s0 the segment's first position, m the
// stream's matches, tkw / mtw the segment's token masks, last: BFINAL
__device__ __forceinline__ void dk_emit_segment(const uint8_t *__restrict__ s, const uint64_t s0,
                                                const uint32_t *__restrict__ m, const uint64_t *__restrict__ tkw,
                                                const uint64_t *__restrict__ mtw, const pd_seg_t *__restrict__ seg,
                                                const uint64_t o, const bool last, uint32_t *__restrict__ words)
{
  __shared__ pd_seg_t sg;
  __shared__ uint16_t code[NSYM], cl_code[PD_NCL];
  const int tid = threadIdx.x;
  if(tid == 0)
  {
    sg = *seg;
    if(sg.type != PD_STORED)
    {
      pd_codes(sg.len, PD_NLIT, code, sg.type == PD_FIXED);
      pd_codes(sg.len + PD_NLIT, PD_NDIST, code + PD_NLIT);
      pd_codes(sg.cl_len, PD_NCL, cl_code);
    }
  }
  __syncthreads();
  const uint32_t n = sg.nbytes;
  if(sg.type == PD_STORED)
  {
    const uint64_t q = align8(o + 3) / 8;
    if(tid == 0)
    {
      or_bits(words, o, last ? 1u : 0u, 3);
      or_byte(words, q, n & 255);
      or_byte(words, q + 1, (n >> 8) & 255);
      or_byte(words, q + 2, ~n & 255);
      or_byte(words, q + 3, (~n >> 8) & 255);
    }
    for(uint32_t j = tid; j < n; j += PT) or_byte(words, q + 4 + j, s[s0 + j]);
    return;
  }
  const uint32_t j0 = min(n, (uint32_t)tid * SEG_PER_THREAD), j1 = min(n, j0 + SEG_PER_THREAD);
  // each token of the thread's range: f(code, its length, extra, extra bits) for its one or two symbols
  auto walk = [&](auto f) {
    for(uint32_t j = j0; j < j1; j++)
    {
      if(!((tkw[j >> 6] >> (j & 63)) & 1)) continue;
      if(!((mtw[j >> 6] >> (j & 63)) & 1))
      {
        const uint32_t b = s[s0 + j];
        f(code[b], sg.len[b], 0u, 0);
        continue;
      }
      const uint32_t v = m[s0 + j];
      uint32_t ne, ex;
      const uint32_t ls = pd_len_sym(v >> 16, &ne, &ex);
      f(code[ls], sg.len[ls], ex, (int)ne);
      const uint32_t ds = pd_dist_sym((v & 0xffff) + 1, &ne, &ex);
      f(code[PD_NLIT + ds], sg.len[PD_NLIT + ds], ex, (int)ne);
    }
  };
  uint64_t nbits = 0;
  walk([&](uint32_t, int l, uint32_t, int ne) { nbits += l + ne; });
  if(tid == 0) pd_block_header(sg, last, cl_code, [&](uint32_t, int nb) { nbits += nb; });
  if(tid == PT - 1) nbits += sg.len[256];
  uint64_t total;
  const uint64_t ex = block_exclusive_scan<uint64_t>(nbits, &total);
  writer_t wr(words, o + ex);
  if(tid == 0) pd_block_header(sg, last, cl_code, [&](uint32_t v, int nb) { wr.put(v, nb); });
  walk([&](uint32_t c, int l, uint32_t e, int ne) {
    wr.put(c, l);
    if(ne) wr.put(e, ne);
  });
  if(tid == PT - 1) wr.put(code[256], sg.len[256]);
  wr.flush();
}

} // namespace
} // namespace ansel
