// webp.hip -- lossless WebP (VP8L) encoding of the export_u8 frame on gfx950: a valid stream of our own that libwebp's
// decoder turns back into the input's RGB (webp_body.h holds the body).
//
// Stages, all on the device's stream, no host synchronisation:
//   webp_predict  one workgroup per predictor block: the 14 modes' costs, the choice, the block's residual pixels
//   webp_lz       one workgroup per segment of WP_SEG residual pixels: the matches (WP_NTAB hash tables in LDS, WP_STEP
//                 positions per step, atomicMax on insertion, the pixel to the left and the pixel above as candidates of
//                 their own) and the parse (wave 0 walks the match lengths of 64 positions at a time from registers)
//   webp_tables   one wave per tile: the tile's symbol counts (an LDS histogram, integer atomics) and its five codes
//                 (jh_build(), limits 15 / 7), the bits of their header
//   webp_count    one workgroup per segment: the bits of its tokens under their tiles' codes
//   webp_scan     one workgroup: every group header's and every segment's bit offset, L, whether it fits, the length word
//   webp_emit     the zeroed stream ORed together: the host-built head, the predictor image (4 bits a block), the
//                 groups' codes (one thread each), the tokens (one workgroup per segment: a workgroup scan, then each
//                 thread's tokens), the RIFF and VP8L sizes
//   webp_copy     the stream into the file
// Nothing is written to dev_out past its capacity: the length word (the first 8 bytes) is L or UINT64_MAX, and the file
// bytes are written only when they fit.
#include <algorithm>
#include <vector>

#include "deflate_kernels.h"
#include "hip_common.h"
#include "webp_body.h"

namespace ansel
{
namespace
{

constexpr int WSEG_WORDS = WP_SEG / 64;      // 64-bit token masks per segment
constexpr int WSEG_PER_THREAD = WP_SEG / PT; // positions per thread in the emission

struct wstate_t
{
  uint64_t bits;   // the stream's bits, from the file's first byte
  uint64_t length; // L, or UINT64_MAX
  uint64_t bytes;  // L when it fits, else 0: what webp_emit's kernels and webp_copy work on
};

// the frame's constants
struct wframe_t
{
  int w, h, pb, eb;
  uint32_t bx, by, tx, ty;
  uint64_t N, nseg;
};

__global__ __launch_bounds__(PT) void webp_predict(const uint8_t *__restrict__ in, const wframe_t f,
                                                   uint8_t *__restrict__ modes, uint32_t *__restrict__ res)
{
  __shared__ uint32_t tot[WP_NMODES];
  const uint32_t bxi = blockIdx.x % f.bx, byi = blockIdx.x / f.bx;
  const int x0 = (int)(bxi << f.pb), y0 = (int)(byi << f.pb);
  const int bw = min(f.w - x0, 1 << f.pb), bh = min(f.h - y0, 1 << f.pb);
  const int n = bw * bh;
  uint32_t cost[WP_NMODES];
#pragma unroll
  for(int m = 0; m < WP_NMODES; m++) cost[m] = 0;
  for(int i = threadIdx.x; i < n; i += PT) wp_costs(in, f.w, x0 + i % bw, y0 + i / bw, cost);
#pragma unroll
  for(int m = 0; m < WP_NMODES; m++)
  {
    const uint32_t s = block_sum<uint32_t>(cost[m]);
    if(threadIdx.x == 0) tot[m] = s;
  }
  __syncthreads();
  const int best = wp_choose(tot);
  if(threadIdx.x == 0) modes[blockIdx.x] = (uint8_t)best;
  for(int i = threadIdx.x; i < n; i += PT)
  {
    const int x = x0 + i % bw, y = y0 + i / bw;
    res[(size_t)y * f.w + x] = wp_residual(in, f.w, x, y, best);
  }
}

// per segment: the matches (m: len << 16 | dist - 1, at the positions that have one) and the parse (tokm: a token
// starts here, matm: that token is a match; the stream's positions, WSEG_WORDS words a segment)
__global__ __launch_bounds__(PT) void webp_lz(const uint32_t *__restrict__ s, const uint64_t N, const uint32_t width,
                                              const int level, uint32_t *__restrict__ m, uint64_t *__restrict__ tokm,
                                              uint64_t *__restrict__ matm)
{
  __shared__ int32_t head[WP_NTAB << WP_TBITS];
  __shared__ uint16_t lenv[WP_SEG];
  __shared__ uint64_t tk[WSEG_WORDS], mt[WSEG_WORDS];
  const int tid = threadIdx.x;
  const uint64_t s0 = (uint64_t)blockIdx.x * WP_SEG, s1 = min(N, s0 + WP_SEG);
  const uint32_t n = (uint32_t)(s1 - s0);
  const uint32_t nw = (n + 63) / 64;
  tokm += (uint64_t)blockIdx.x * WSEG_WORDS;
  matm += (uint64_t)blockIdx.x * WSEG_WORDS;
  if(level == 0)
  {
    for(uint32_t i = tid; i < nw; i += PT)
    {
      const uint32_t left = n - 64 * i;
      tokm[i] = left >= 64 ? ~0ull : (1ull << left) - 1;
      matm[i] = 0;
    }
    return;
  }
  for(int i = tid; i < (WP_NTAB << WP_TBITS); i += PT) head[i] = -1;
  for(int i = tid; i < WP_SEG; i += PT) lenv[i] = 0;
  __syncthreads();
  const uint64_t ws = s0 > WP_WIN ? s0 - WP_WIN : 0;
  for(uint64_t c = ws; c < s1; c += WP_STEP)
  {
    const uint64_t p = c + tid;
    if(p < s1 && p >= s0)
    {
      uint32_t dist;
      const uint32_t l = wp_best(s, N, p, ws, (uint32_t)min<uint64_t>(WP_MAXLEN, s1 - p), width,
                                 [&](uint32_t slot) { return head[slot]; }, &dist);
      if(l)
      {
        lenv[p - s0] = (uint16_t)l;
        m[p] = (l << 16) | (dist - 1);
      }
    }
    __syncthreads();
    if(p < s1)
      for(int t = 0; t < WP_NTAB && wp_keyed(p, N, t); t++) atomicMax(&head[wp_slot(s, p, t)], (int32_t)(p - ws));
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
        const uint32_t l = (uint32_t)__builtin_amdgcn_readlane(lv, i);
        const uint32_t lnr = (uint32_t)(i + 1 < 64 ? __builtin_amdgcn_readlane(lv, i + 1) : __builtin_amdgcn_readlane(lv2, 0));
        const uint32_t ln = q + 1 < n ? lnr : 0;
        tkm |= 1ull << i;
        if(wp_take(l, ln, level))
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
  for(uint32_t i = tid; i < nw; i += PT)
  {
    tokm[i] = tk[i];
    matm[i] = mt[i];
  }
}

// one wave per tile: the counts of the symbols of the tokens that start in the tile, and the tile's five codes
__global__ __launch_bounds__(64) void webp_tables(const uint32_t *__restrict__ s, const uint32_t *__restrict__ m,
                                                  const uint64_t *__restrict__ tokm, const uint64_t *__restrict__ matm,
                                                  const wframe_t f, wp_group_t *__restrict__ groups)
{
  __shared__ wp_tab_work_t tw;
  __shared__ uint32_t hist[WP_NSYM];
  const uint32_t txi = blockIdx.x % f.tx, tyi = blockIdx.x / f.tx;
  const int x0 = (int)(txi << f.eb), y0 = (int)(tyi << f.eb);
  const int bw = min(f.w - x0, 1 << f.eb), bh = min(f.h - y0, 1 << f.eb);
  for(int i = threadIdx.x; i < WP_NSYM; i += 64) hist[i] = 0;
  __syncthreads();
  for(int i = threadIdx.x; i < bw * bh; i += 64)
  {
    const uint64_t p = (uint64_t)(y0 + i / bw) * f.w + (x0 + i % bw);
    if(!((tokm[p >> 6] >> (p & 63)) & 1)) continue;
    const bool is_match = (matm[p >> 6] >> (p & 63)) & 1;
    wp_count(s[p], is_match, is_match ? m[p] : 0u, [&](uint32_t k) { atomicAdd(&hist[k], 1u); });
  }
  __syncthreads();
  wp_tables(
      &tw, hist, threadIdx.x, 64, [](uint64_t v) { return wave_min_u64(v); }, []() { __syncthreads(); },
      &groups[blockIdx.x]);
}

// the tokens that start at the thread's positions j0 .. j1 of segment k: f(code, its length, extra, extra bits)
template <class F>
__device__ __forceinline__ void walk_tokens(const uint32_t *__restrict__ s, const uint32_t *__restrict__ m,
                                            const uint64_t *__restrict__ tokm, const uint64_t *__restrict__ matm,
                                            const wframe_t &f, const wp_group_t *__restrict__ groups, const uint64_t s0,
                                            const uint32_t j0, const uint32_t j1, F fn)
{
  for(uint32_t j = j0; j < j1; j++)
  {
    const uint64_t p = s0 + j;
    if(!((tokm[p >> 6] >> (p & 63)) & 1)) continue;
    const bool is_match = (matm[p >> 6] >> (p & 63)) & 1;
    const wp_group_t *g = &groups[wp_tile((uint32_t)p, (uint32_t)f.w, f.eb, f.tx)];
    wp_token(g, s[p], is_match, is_match ? m[p] : 0u, fn);
  }
}

__global__ __launch_bounds__(PT) void webp_count(const uint32_t *__restrict__ s, const uint32_t *__restrict__ m,
                                                 const uint64_t *__restrict__ tokm, const uint64_t *__restrict__ matm,
                                                 const wframe_t f, const wp_group_t *__restrict__ groups,
                                                 uint64_t *__restrict__ segbits)
{
  const uint64_t s0 = (uint64_t)blockIdx.x * WP_SEG;
  const uint32_t n = (uint32_t)(min(f.N, s0 + WP_SEG) - s0);
  const uint32_t j0 = min(n, (uint32_t)threadIdx.x * WSEG_PER_THREAD), j1 = min(n, j0 + WSEG_PER_THREAD);
  uint64_t nbits = 0;
  walk_tokens(s, m, tokm, matm, f, groups, s0, j0, j1, [&](uint32_t, int l, uint32_t, int ne) { nbits += l + ne; });
  nbits = block_sum<uint64_t>(nbits);
  if(threadIdx.x == 0) segbits[blockIdx.x] = nbits;
}

// the exclusive scan of n lengths len(i) from `start` into off[]: each thread a run of them; returns the end
template <class Len>
__device__ __forceinline__ uint64_t scan_offsets(const uint64_t n, const uint64_t start, Len len, uint64_t *__restrict__ off)
{
  const int t = threadIdx.x;
  const uint64_t per = (n + PT - 1) / PT;
  const uint64_t k0 = min(n, t * per), k1 = min(n, k0 + per);
  uint64_t sum = 0;
  for(uint64_t k = k0; k < k1; k++) sum += len(k);
  uint64_t total;
  uint64_t o = start + block_exclusive_scan<uint64_t>(sum, &total);
  for(uint64_t k = k0; k < k1; k++)
  {
    off[k] = o;
    o += len(k);
  }
  return start + total;
}

// one workgroup: the groups' and the segments' bit offsets, L, whether it fits, the length word
__global__ __launch_bounds__(PT) void webp_scan(const wp_group_t *__restrict__ groups, const uint64_t ngroups,
                                                const uint64_t *__restrict__ segbits, const uint64_t nseg,
                                                const uint64_t groups_at, const uint64_t payload_at, const uint64_t capacity,
                                                const uint64_t stream_bytes, uint64_t *__restrict__ goff, uint64_t *__restrict__ soff,
                                                wstate_t *__restrict__ st, uint8_t *__restrict__ out)
{
  const uint64_t tokens_at = scan_offsets(ngroups, groups_at, [&](uint64_t k) { return (uint64_t)groups[k].hdr_bits; }, goff);
  const uint64_t end = scan_offsets(nseg, tokens_at, [&](uint64_t k) { return segbits[k]; }, soff);
  if(threadIdx.x == 0)
  {
    const uint64_t bytes = (end + 7) / 8;
    const uint64_t L = bytes + ((bytes - payload_at) & 1);
    // stream_bytes: the scratch the stream is built in, sized by the bound
    const bool fits = 8 + L <= capacity && L <= stream_bytes;
    st->bits = end;
    st->length = fits ? L : ~0ull;
    st->bytes = fits ? L : 0;
    for(int i = 0; i < 8; i++) out[i] = (uint8_t)(st->length >> (8 * i));
  }
}

__global__ __launch_bounds__(PT) void webp_zero(uint32_t *__restrict__ words, const wstate_t *__restrict__ st)
{
  const uint64_t n = (st->bytes + 3) / 4;
  for(uint64_t i = blockIdx.x * (uint64_t)PT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * PT) words[i] = 0;
}

// the host-built bytes a (from the file's first byte), the predictor image (4 bits a block from bit a_bits), the
// host-built bits b behind it, and the two chunk sizes
__global__ __launch_bounds__(PT) void webp_head(const uint8_t *__restrict__ a, const uint64_t a_bytes, const uint64_t a_bits,
                                                const uint8_t *__restrict__ modes, const uint64_t nblocks,
                                                const uint8_t *__restrict__ b, const uint64_t b_bytes,
                                                const uint64_t vp8l_size_at, const uint64_t payload_at,
                                                const wstate_t *__restrict__ st, uint32_t *__restrict__ words)
{
  const uint64_t L = st->bytes;
  if(!L) return;
  const uint64_t i0 = blockIdx.x * (uint64_t)PT + threadIdx.x, step = (uint64_t)gridDim.x * PT;
  for(uint64_t i = i0; i < a_bytes; i += step) or_byte(words, i, a[i]);
  for(uint64_t i = i0; i < nblocks; i += step) or_bits(words, a_bits + 4 * i, wp_rev(modes[i], 4), 4);
  const uint64_t b_at = a_bits + 4 * nblocks;
  for(uint64_t i = i0; i < b_bytes; i += step) or_bits(words, b_at + 8 * i, b[i], 8);
  if(i0 == 0)
  {
    const uint64_t payload = (st->bits + 7) / 8 - payload_at;
    for(int k = 0; k < 4; k++)
    {
      or_byte(words, 4 + k, (uint32_t)((L - 8) >> (8 * k)));
      or_byte(words, vp8l_size_at + k, (uint32_t)(payload >> (8 * k)));
    }
  }
}

// one thread per group: its five codes at its offset
__global__ __launch_bounds__(PT) void webp_groups(const wp_group_t *__restrict__ groups, const uint64_t ngroups,
                                                  const uint64_t *__restrict__ goff, const wstate_t *__restrict__ st,
                                                  uint32_t *__restrict__ words)
{
  const uint64_t k = blockIdx.x * (uint64_t)PT + threadIdx.x;
  if(!st->bytes || k >= ngroups) return;
  writer_t wr(words, goff[k]);
  for(int a = 0; a < 5; a++) wp_code_header(&groups[k], a, [&](uint32_t v, int nb) { wr.put(v, nb); });
  wr.flush();
}

__global__ __launch_bounds__(PT) void webp_tokens(const uint32_t *__restrict__ s, const uint32_t *__restrict__ m,
                                                  const uint64_t *__restrict__ tokm, const uint64_t *__restrict__ matm,
                                                  const wframe_t f, const wp_group_t *__restrict__ groups,
                                                  const uint64_t *__restrict__ soff, const wstate_t *__restrict__ st,
                                                  uint32_t *__restrict__ words)
{
  if(!st->bytes) return;
  const uint64_t s0 = (uint64_t)blockIdx.x * WP_SEG;
  const uint32_t n = (uint32_t)(min(f.N, s0 + WP_SEG) - s0);
  const uint32_t j0 = min(n, (uint32_t)threadIdx.x * WSEG_PER_THREAD), j1 = min(n, j0 + WSEG_PER_THREAD);
  uint64_t nbits = 0;
  walk_tokens(s, m, tokm, matm, f, groups, s0, j0, j1, [&](uint32_t, int l, uint32_t, int ne) { nbits += l + ne; });
  uint64_t total;
  const uint64_t ex = block_exclusive_scan<uint64_t>(nbits, &total);
  writer_t wr(words, soff[blockIdx.x] + ex);
  walk_tokens(s, m, tokm, matm, f, groups, s0, j0, j1, [&](uint32_t c, int l, uint32_t e, int ne) {
    wr.put(c, l);
    if(ne) wr.put(e, ne);
  });
  wr.flush();
}

// the stream into the file: whole words where dev_out allows it, the last bytes one by one
__global__ __launch_bounds__(PT) void webp_copy(const uint32_t *__restrict__ words, const wstate_t *__restrict__ st,
                                                uint8_t *__restrict__ out)
{
  const uint64_t L = st->bytes;
  const uint64_t i0 = blockIdx.x * (uint64_t)PT + threadIdx.x, step = (uint64_t)gridDim.x * PT;
  uint8_t *dst = out + 8;
  const uint64_t nw = ((uintptr_t)dst & 3) == 0 ? L / 4 : 0;
  for(uint64_t i = i0; i < nw; i += step) ((uint32_t *)dst)[i] = words[i];
  const uint8_t *src = (const uint8_t *)words;
  for(uint64_t i = 4 * nw + i0; i < L; i += step) dst[i] = src[i];
}

bool webp_geometry(int width, int height, const dt_hip_webp_data_t *d, const char *who, wp_geom_t *g)
{
  char why[256];
  if(wp_geometry(width, height, d, g, why, sizeof(why))) return true;
  set_last_error("%s: %s", who, why);
  return false;
}

} // namespace
} // namespace ansel

using namespace ansel;

extern "C" size_t dt_hip_webp_bound(int width, int height, const dt_hip_webp_data_t *d)
{
  wp_geom_t g;
  if(!webp_geometry(width, height, d, "dt_hip_webp_bound", &g)) return 0;
  return (size_t)g.bound;
}

extern "C" int dt_hip_export_webp(int devid, int width, int height, const dt_hip_webp_data_t *d, dt_hip_mem_t dev_in,
                                  dt_hip_mem_t dev_out)
{
  if(!valid_device(devid) || !dev_in || !dev_out) return DT_HIP_INVALID_ARG;
  wp_geom_t g;
  if(!webp_geometry(width, height, d, "export_webp", &g)) return DT_HIP_INVALID_ARG;
  if(d->capacity < 8)
  {
    set_last_error("export_webp: capacity %llu cannot hold the 8-byte length word", (unsigned long long)d->capacity);
    return DT_HIP_INVALID_ARG;
  }
  wp_head_t hd;
  if(!wp_file_head(width, height, g, (const uint8_t *)d->icc, d->icc ? (size_t)d->icc_bytes : 0, &hd))
  {
    set_last_error("export_webp: the fixed codes of the sub-images did not come out as fixed");
    return DT_HIP_DEFAULT_ERROR;
  }
  const int level = d->level;
  const uint64_t N = g.N, nseg = g.nseg, nblocks = (uint64_t)g.bx * g.by, ngroups = (uint64_t)g.tx * g.ty;
  const wframe_t f = { width, height, g.pb, g.eb, g.bx, g.by, g.tx, g.ty, N, nseg };
  const uint64_t nwords = (g.bound - 8) / 4 + 2;
  const uint64_t groups_at = hd.a_bits + 4 * nblocks + hd.b_bits;
  // the host-built bytes, a then b, in one upload
  std::vector<uint8_t> up(hd.a);
  up.insert(up.end(), hd.b.begin(), hd.b.end());
  // scratch from the runtime's pool, released behind the launches (the pool's reuse is stream-ordered)
  const dev_buf_t m_res = dev_buf_t::alloc(devid, (size_t)N * 4);
  const dev_buf_t m_m = dev_buf_t::alloc(devid, level ? (size_t)N * 4 : 4);
  const dev_buf_t m_tok = dev_buf_t::alloc(devid, (size_t)nseg * WSEG_WORDS * 8);
  const dev_buf_t m_mat = dev_buf_t::alloc(devid, (size_t)nseg * WSEG_WORDS * 8);
  const dev_buf_t m_modes = dev_buf_t::alloc(devid, (size_t)nblocks);
  const dev_buf_t m_groups = dev_buf_t::alloc(devid, (size_t)ngroups * sizeof(wp_group_t));
  const dev_buf_t m_segbits = dev_buf_t::alloc(devid, (size_t)nseg * 8);
  const dev_buf_t m_goff = dev_buf_t::alloc(devid, (size_t)ngroups * 8);
  const dev_buf_t m_soff = dev_buf_t::alloc(devid, (size_t)nseg * 8);
  const dev_buf_t m_words = dev_buf_t::alloc(devid, (size_t)nwords * 4);
  const dev_buf_t m_st = dev_buf_t::alloc(devid, sizeof(wstate_t));
  const dev_buf_t m_up = dev_buf_t::alloc(devid, up.size());
  if(!m_res || !m_m || !m_tok || !m_mat || !m_modes || !m_groups || !m_segbits || !m_goff || !m_soff || !m_words || !m_st || !m_up)
    return DT_HIP_DEFAULT_ERROR;
  hipStream_t s = stream_of(devid);
  const int err = upload_small(devid, m_up.ptr(), up.data(), up.size());
  if(err != DT_HIP_SUCCESS) return err;
  const uint32_t *res = m_res.as<const uint32_t>(), *mm = m_m.as<const uint32_t>();
  const uint64_t *tok = m_tok.as<const uint64_t>(), *mat = m_mat.as<const uint64_t>();
  wp_group_t *groups = m_groups.as<wp_group_t>();
  wstate_t *st = m_st.as<wstate_t>();
  uint32_t *words = m_words.as<uint32_t>();
  {
    launch_scope ls(devid, "webp_predict");
    webp_predict<<<(unsigned)nblocks, PT, 0, s>>>((const uint8_t *)dev_in, f, m_modes.as<uint8_t>(), m_res.as<uint32_t>());
  }
  {
    launch_scope ls(devid, "webp_lz");
    webp_lz<<<(unsigned)nseg, PT, 0, s>>>(res, N, (uint32_t)width, level, m_m.as<uint32_t>(), m_tok.as<uint64_t>(),
                                          m_mat.as<uint64_t>());
  }
  {
    launch_scope ls(devid, "webp_tables");
    webp_tables<<<(unsigned)ngroups, 64, 0, s>>>(res, mm, tok, mat, f, groups);
  }
  {
    launch_scope ls(devid, "webp_scan");
    webp_count<<<(unsigned)nseg, PT, 0, s>>>(res, mm, tok, mat, f, groups, m_segbits.as<uint64_t>());
    webp_scan<<<1, PT, 0, s>>>(groups, ngroups, m_segbits.as<const uint64_t>(), nseg, groups_at, hd.payload_at, d->capacity, g.bound - 8,
                               m_goff.as<uint64_t>(), m_soff.as<uint64_t>(), st, (uint8_t *)dev_out);
  }
  {
    launch_scope ls(devid, "webp_emit");
    webp_zero<<<stream_grid(nwords, PT), PT, 0, s>>>(words, st);
    webp_head<<<stream_grid(std::max<uint64_t>(up.size(), nblocks), PT), PT, 0, s>>>(
        m_up.as<const uint8_t>(), hd.a.size(), hd.a_bits, m_modes.as<const uint8_t>(), nblocks,
        m_up.as<const uint8_t>() + hd.a.size(), hd.b.size(), hd.vp8l_size_at, hd.payload_at, st, words);
    webp_groups<<<(unsigned)((ngroups + PT - 1) / PT), PT, 0, s>>>(groups, ngroups, m_goff.as<const uint64_t>(), st, words);
    webp_tokens<<<(unsigned)nseg, PT, 0, s>>>(res, mm, tok, mat, f, groups, m_soff.as<const uint64_t>(), st, words);
  }
  {
    launch_scope ls(devid, "webp_copy");
    webp_copy<<<stream_grid(nwords, PT), PT, 0, s>>>(words, st, (uint8_t *)dev_out);
  }
  return check_launch("export_webp");
}
