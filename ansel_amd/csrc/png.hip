// png.hip -- PNG encoding of the export_u8 / export_u16 frame on gfx950: the file that Ansel's
// src/imageio/format/png.c write_image() makes with libpng (RGB, 8 or 16 bits, no interlace), with libpng's filtered
// stream byte for byte and a deflate of our own (png_deflate.h holds the body).
//
// Stages, all on the device's stream, no host synchronisation:
//   png_filter   one workgroup per row: the five filters' sums (png_write_find_filter), the choice, the filtered row
// (png_lz, png_tables and png_emit are deflate_kernels.h's bodies on segment k of the one stream)
//   png_lz       one workgroup per segment of PD_SEG bytes: the Adler-32 partial sums; the matches (PD_NTAB hash
//                tables in LDS, PD_STEP positions per step, atomicMax on insertion); the parse (wave 0 walks the match lengths
//                of 64 positions at a time from registers); the symbol counts (an LDS histogram, integer atomics)
//   png_tables   one wave per segment: the code lengths (jh_build(), limits 15 / 7), the block type
//   png_scan     one workgroup: each segment's bit offset (a stored block's padding depends on where it starts: the
//                offsets compose functions o -> o + L and o -> align8(o + a) + c), the Adler-32, L and whether it fits
//   png_emit     one workgroup per segment: each thread's tokens' bits, a workgroup scan, integer OR on shared words
//   png_tail     the zlib header and the Adler-32
//   png_idat     one workgroup per IDAT chunk: the copy into the file and the chunk's CRC-32 (per-thread CRCs shifted
//                by the bytes behind them and XORed)
//   png_head     the host-built signature, IHDR, iCCP and pHYs; IEND
// Nothing is written to dev_out past its capacity: the length word (the first 8 bytes) is L or UINT64_MAX, and the file
// bytes are written only when they fit.
#include <algorithm>
#include <vector>

#include "deflate_kernels.h"
#include "hip_common.h"
#include "png_deflate.h"

namespace ansel
{
namespace
{

struct pstate_t
{
  uint64_t zbits;  // bit offset behind the last block (the zlib header included)
  uint64_t zlen;   // bytes of the zlib stream
  uint64_t nidat;  // IDAT chunks
  uint64_t length; // L, or UINT64_MAX
  uint32_t adler;
  uint32_t fits;
};

__device__ __forceinline__ uint32_t block_xor(uint32_t v)
{
  __shared__ uint32_t s[PT];
  s[threadIdx.x] = v;
  __syncthreads();
  for(int o = PT / 2; o > 0; o >>= 1)
  {
    if((int)threadIdx.x < o) s[threadIdx.x] ^= s[threadIdx.x + o];
    __syncthreads();
  }
  const uint32_t r = s[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(PT) void png_filter(const void *__restrict__ in, const int w, const int depth,
                                                 uint8_t *__restrict__ fs)
{
  const int y = blockIdx.x;
  const uint32_t rb = (uint32_t)w * (depth == 8 ? 3 : 6);
  uint64_t sum[5] = { 0, 0, 0, 0, 0 };
  for(uint32_t j = threadIdx.x; j < rb; j += PT)
  {
    uint32_t r[5];
    pf_byte(in, w, depth, y, j, r);
#pragma unroll
    for(int f = 0; f < 5; f++) sum[f] += pf_cost(r[f]);
  }
  uint64_t tot[5];
#pragma unroll
  for(int f = 0; f < 5; f++) tot[f] = block_sum<uint64_t>(sum[f]);
  const int best = pf_choose(tot);
  uint8_t *o = fs + (uint64_t)y * ((uint64_t)rb + 1);
  if(threadIdx.x == 0) o[0] = (uint8_t)best;
  for(uint32_t j = threadIdx.x; j < rb; j += PT)
  {
    uint32_t r[5];
    pf_byte(in, w, depth, y, j, r);
    o[1 + j] = (uint8_t)r[best];
  }
}

// per segment: Adler-32 sums; at level > 0 the matches (m: len << 16 | dist - 1, at the positions that have one), the
// parse (tokm: a token starts here, matm: that token is a match) and the symbol counts
__global__ __launch_bounds__(PT) void png_lz(const uint8_t *__restrict__ fs, const uint64_t N, const int level,
                                             uint32_t *__restrict__ m, uint64_t *__restrict__ tokm,
                                             uint64_t *__restrict__ matm, uint32_t *__restrict__ freq,
                                             pd_seg_t *__restrict__ segs)
{
  const uint64_t k = blockIdx.x;
  const uint64_t s0 = k * PD_SEG;
  dk_lz_segment(fs, N, s0, min(N, s0 + PD_SEG), level, m, tokm + k * SEG_WORDS, matm + k * SEG_WORDS, freq + k * NSYM,
                &segs[k]);
}

// one wave per segment: code lengths and the block type (pd_tables)
__global__ __launch_bounds__(64) void png_tables(const uint32_t *__restrict__ freq, const uint64_t N, const int level,
                                                 pd_seg_t *__restrict__ segs)
{
  const uint64_t k = blockIdx.x;
  const uint64_t s0 = k * PD_SEG;
  dk_tables_segment(freq + k * NSYM, (uint32_t)(min(N, s0 + PD_SEG) - s0), level, &segs[k]);
}

// the offset map of a run of segments: o -> o + c (align < 0) or o -> align8(o + a) + c
struct omap_t
{
  int64_t a; // -1: no alignment
  uint64_t c;
};

__device__ __forceinline__ omap_t omap_of(const pd_seg_t &s)
{
  if(s.type == PD_STORED) return { 3, 32 + 8 * (uint64_t)s.nbytes };
  return { -1, s.bits };
}

// f, then g
__device__ __forceinline__ omap_t omap_then(omap_t f, omap_t g)
{
  if(g.a < 0) return { f.a, f.c + g.c };
  if(f.a < 0) return { (int64_t)(g.a + f.c), g.c };
  return { f.a, align8(f.c + (uint64_t)g.a) + g.c };
}

__device__ __forceinline__ uint64_t omap_apply(omap_t f, uint64_t o)
{
  return f.a < 0 ? o + f.c : align8(o + (uint64_t)f.a) + f.c;
}

// one workgroup: the segments' bit offsets, the Adler-32, the zlib length, L, whether it fits, the length word
__global__ __launch_bounds__(PT) void png_scan(const pd_seg_t *__restrict__ segs, const uint64_t nseg, const uint64_t N,
                                               const uint32_t head_len, const uint64_t capacity,
                                               uint64_t *__restrict__ off, pstate_t *__restrict__ st,
                                               uint8_t *__restrict__ out)
{
  __shared__ omap_t maps[PT];
  __shared__ uint64_t starts[PT];
  __shared__ uint64_t total;
  const int t = threadIdx.x;
  const uint64_t per = (nseg + PT - 1) / PT;
  const uint64_t k0 = min(nseg, t * per), k1 = min(nseg, k0 + per);
  omap_t f = { -1, 0 };
  uint64_t A = 0, B = 0;
  for(uint64_t k = k0; k < k1; k++)
  {
    const pd_seg_t &s = segs[k];
    f = omap_then(f, omap_of(s));
    const uint64_t e = min(N, (k + 1) * PD_SEG);
    A += s.adler_s;
    B = (B + s.adler_t + ((N - e) % PD_ADLER_MOD) * s.adler_s) % PD_ADLER_MOD;
  }
  maps[t] = f;
  A = block_sum<uint64_t>(A % PD_ADLER_MOD);
  B = block_sum<uint64_t>(B);
  if(t == 0)
  {
    uint64_t o = 16; // the zlib header
    for(int i = 0; i < PT; i++)
    {
      starts[i] = o;
      o = omap_apply(maps[i], o);
    }
    total = o;
  }
  __syncthreads();
  uint64_t o = starts[t];
  for(uint64_t k = k0; k < k1; k++)
  {
    off[k] = o;
    o = pd_seg_end(segs[k], o);
  }
  if(t == 0)
  {
    const uint32_t a = (uint32_t)((1 + A) % PD_ADLER_MOD), b = (uint32_t)((N % PD_ADLER_MOD + B) % PD_ADLER_MOD);
    const uint64_t zlen = (total + 7) / 8 + 4;
    const uint64_t nidat = (zlen + PD_IDAT - 1) / PD_IDAT;
    const uint64_t L = head_len + zlen + 12 * nidat + 12;
    const bool fits = 8 + L <= capacity;
    st->zbits = total;
    st->zlen = zlen;
    st->nidat = nidat;
    st->adler = (b << 16) | a;
    st->fits = fits;
    st->length = fits ? L : ~0ull;
    for(int i = 0; i < 8; i++) out[i] = (uint8_t)(st->length >> (8 * i));
  }
}

__global__ __launch_bounds__(PT) void png_zero(uint32_t *__restrict__ words, const pstate_t *__restrict__ st)
{
  const uint64_t n = (st->zlen + 3) / 4;
  for(uint64_t i = blockIdx.x * (uint64_t)PT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * PT) words[i] = 0;
}

__global__ __launch_bounds__(PT) void png_emit(const uint8_t *__restrict__ fs, const uint32_t *__restrict__ m,
                                               const uint64_t *__restrict__ tokm, const uint64_t *__restrict__ matm,
                                               const pd_seg_t *__restrict__ segs, const uint64_t *__restrict__ off,
                                               const uint64_t nseg, uint32_t *__restrict__ words)
{
  const uint64_t k = blockIdx.x;
  dk_emit_segment(fs, k * PD_SEG, m, tokm + k * SEG_WORDS, matm + k * SEG_WORDS, &segs[k], off[k], k + 1 == nseg, words);
}

// the zlib header and the Adler-32 behind the last block
__global__ void png_tail(uint32_t *__restrict__ words, const uint32_t zheader, const pstate_t *__restrict__ st)
{
  if(threadIdx.x != 0) return;
  or_byte(words, 0, zheader >> 8);
  or_byte(words, 1, zheader & 255);
  const uint64_t a = (st->zbits + 7) / 8;
  for(int i = 0; i < 4; i++) or_byte(words, a + i, st->adler >> (24 - 8 * i));
}

constexpr int IDAT_PER_THREAD = PD_IDAT / PT;

// one workgroup per IDAT chunk: length, type, the data copied from the zlib stream, CRC-32
__global__ __launch_bounds__(PT) void png_idat(const uint8_t *__restrict__ z, const pstate_t *__restrict__ stp,
                                               const uint32_t head_len, const uint32_t crc_type,
                                               uint8_t *__restrict__ out)
{
  __shared__ uint32_t table[256];
  const pstate_t st = *stp;
  if(!st.fits) return;
  {
    uint32_t c = threadIdx.x;
    for(int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ 0xedb88320u : c >> 1;
    table[threadIdx.x] = c;
  }
  __syncthreads();
  for(uint64_t ci = blockIdx.x; ci < st.nidat; ci += gridDim.x)
  {
    const uint64_t d0 = ci * PD_IDAT;
    const uint32_t len = (uint32_t)min<uint64_t>(PD_IDAT, st.zlen - d0);
    uint8_t *dst = out + 8 + head_len + ci * (PD_IDAT + 12);
    const uint32_t p0 = min(len, (uint32_t)threadIdx.x * IDAT_PER_THREAD), p1 = min(len, p0 + IDAT_PER_THREAD);
    uint32_t c = 0xffffffffu;
    for(uint32_t j = p0; j < p1; j++)
    {
      const uint32_t b = z[d0 + j];
      dst[8 + j] = (uint8_t)b;
      c = table[(c ^ b) & 255] ^ (c >> 8);
    }
    c = ~c;
    const uint32_t mine = p1 > p0 ? pd_multmodp(pd_x8n(len - p1), c) : 0u;
    const uint32_t crc = block_xor(mine) ^ pd_multmodp(pd_x8n(len), crc_type);
    if(threadIdx.x == 0)
    {
      const uint8_t hdr[8] = { (uint8_t)(len >> 24), (uint8_t)(len >> 16), (uint8_t)(len >> 8), (uint8_t)len,
                               'I', 'D', 'A', 'T' };
      for(int i = 0; i < 8; i++) dst[i] = hdr[i];
      for(int i = 0; i < 4; i++) dst[8 + len + i] = (uint8_t)(crc >> (24 - 8 * i));
    }
  }
}

// the bytes in front of the first IDAT (host-built) and IEND
__global__ __launch_bounds__(PT) void png_head(const uint8_t *__restrict__ head, const uint32_t head_len,
                                               const pstate_t *__restrict__ stp, uint8_t *__restrict__ out)
{
  const pstate_t st = *stp;
  if(!st.fits) return;
  for(uint32_t i = threadIdx.x; i < head_len; i += PT) out[8 + i] = head[i];
  if(threadIdx.x == 0)
  {
    const uint8_t iend[12] = { 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82 };
    for(int i = 0; i < 12; i++) out[8 + st.length - 12 + i] = iend[i];
  }
}

// the frame's sizes; false (with the reason) for refused settings or a bound beyond size_t
struct pgeom_t
{
  uint64_t N;     // filtered stream bytes
  uint64_t nseg;
  uint64_t zmax;  // the zlib stream's bytes at most
  uint64_t head;  // bytes in front of the first IDAT
  uint64_t bound; // 8 + the file at most
};

bool png_geometry(int width, int height, const dt_hip_png_data_t *d, const char *who, pgeom_t *g)
{
  if(!d)
  {
    set_last_error("%s: no dt_hip_png_data_t", who);
    return false;
  }
  if(width < 1 || height < 1)
  {
    set_last_error("%s: %d x %d is not a frame", who, width, height);
    return false;
  }
  if(d->bit_depth != 8 && d->bit_depth != 16)
  {
    set_last_error("%s: bit depth %d is not 8 or 16", who, (int)d->bit_depth);
    return false;
  }
  if(d->compression_level < 0 || d->compression_level > 9)
  {
    set_last_error("%s: compression level %d is outside 0..9", who, (int)d->compression_level);
    return false;
  }
  if(d->dpi < 0)
  {
    set_last_error("%s: dpi %d is negative", who, (int)d->dpi);
    return false;
  }
  if(d->icc_bytes && !d->icc)
  {
    set_last_error("%s: icc_bytes %llu without an icc pointer", who, (unsigned long long)d->icc_bytes);
    return false;
  }
  if(d->icc && d->icc_bytes > (1ull << 30))
  {
    set_last_error("%s: an ICC profile of %llu bytes does not fit an iCCP chunk", who, (unsigned long long)d->icc_bytes);
    return false;
  }
  const unsigned __int128 rb = (unsigned __int128)width * (d->bit_depth / 8 * 3);
  const unsigned __int128 N = (unsigned __int128)height * (rb + 1);
  const unsigned __int128 nseg = (N + PD_SEG - 1) / PD_SEG;
  const unsigned __int128 zmax = (42 * nseg + 8 * N + 7) / 8 + 6;
  const unsigned __int128 head = 8 + 25 + pd_iccp_bytes(d->icc ? d->icc_bytes : 0) + (d->dpi > 0 ? 21 : 0);
  const unsigned __int128 bound = 8 + head + zmax + 12 * ((zmax + PD_IDAT - 1) / PD_IDAT) + 12;
  if(rb >= 0xffffffffu || nseg > 0x7fffffff || bound > (unsigned __int128)SIZE_MAX)
  {
    set_last_error("%s: the bound of a %d x %d frame at %d bits does not fit", who, width, height, (int)d->bit_depth);
    return false;
  }
  g->N = (uint64_t)N;
  g->nseg = (uint64_t)nseg;
  g->zmax = (uint64_t)zmax;
  g->head = (uint64_t)head;
  g->bound = (uint64_t)bound;
  return true;
}

} // namespace
} // namespace ansel

using namespace ansel;

extern "C" size_t dt_hip_png_bound(int width, int height, const dt_hip_png_data_t *d)
{
  pgeom_t g;
  if(!png_geometry(width, height, d, "dt_hip_png_bound", &g)) return 0;
  return (size_t)g.bound;
}

extern "C" int dt_hip_export_png(int devid, int width, int height, const dt_hip_png_data_t *d, dt_hip_mem_t dev_in,
                                 dt_hip_mem_t dev_out)
{
  if(!valid_device(devid) || !dev_in || !dev_out) return DT_HIP_INVALID_ARG;
  pgeom_t g;
  if(!png_geometry(width, height, d, "export_png", &g)) return DT_HIP_INVALID_ARG;
  if(d->capacity < 8)
  {
    set_last_error("export_png: capacity %llu cannot hold the 8-byte length word", (unsigned long long)d->capacity);
    return DT_HIP_INVALID_ARG;
  }
  const int level = d->compression_level;
  const std::vector<uint8_t> head = pd_file_head(width, height, d->bit_depth, (const uint8_t *)d->icc,
                                                 d->icc ? (size_t)d->icc_bytes : 0, d->dpi);
  const uint32_t crc_type = pd_crc((const uint8_t *)"IDAT", 4);
  const uint64_t N = g.N, nseg = g.nseg;
  const uint64_t nwords = g.zmax / 4 + 2;
  const uint64_t max_idat = (g.zmax + PD_IDAT - 1) / PD_IDAT;
  // scratch from the runtime's pool, released behind the launches (the pool's reuse is stream-ordered)
  const size_t sz_fs = (size_t)N, sz_m = level ? (size_t)N * 4 : 4, sz_tok = level ? (size_t)nseg * SEG_WORDS * 8 : 8;
  const size_t sz_freq = (size_t)nseg * NSYM * 4, sz_segs = (size_t)nseg * sizeof(pd_seg_t), sz_off = (size_t)nseg * 8;
  const size_t sz_words = (size_t)nwords * 4;
  const dev_buf_t m_fs = dev_buf_t::alloc(devid, sz_fs);
  const dev_buf_t m_m = dev_buf_t::alloc(devid, sz_m);
  const dev_buf_t m_tok = dev_buf_t::alloc(devid, sz_tok);
  const dev_buf_t m_mat = dev_buf_t::alloc(devid, sz_tok);
  const dev_buf_t m_freq = dev_buf_t::alloc(devid, sz_freq);
  const dev_buf_t m_segs = dev_buf_t::alloc(devid, sz_segs);
  const dev_buf_t m_off = dev_buf_t::alloc(devid, sz_off);
  const dev_buf_t m_words = dev_buf_t::alloc(devid, sz_words);
  const dev_buf_t m_st = dev_buf_t::alloc(devid, sizeof(pstate_t));
  const dev_buf_t m_head = dev_buf_t::alloc(devid, head.size());
  if(!m_fs || !m_m || !m_tok || !m_mat || !m_freq || !m_segs || !m_off || !m_words || !m_st || !m_head) return DT_HIP_DEFAULT_ERROR;
  hipStream_t s = stream_of(devid);
  const int err = upload_small(devid, m_head.ptr(), head.data(), head.size());
  if(err != DT_HIP_SUCCESS) return err;
  pd_seg_t *segs = m_segs.as<pd_seg_t>();
  pstate_t *st = m_st.as<pstate_t>();
  {
    launch_scope ls(devid, "png_filter");
    png_filter<<<height, PT, 0, s>>>(dev_in, width, d->bit_depth, m_fs.as<uint8_t>());
  }
  {
    launch_scope ls(devid, "png_lz");
    png_lz<<<(unsigned)nseg, PT, 0, s>>>(m_fs.as<const uint8_t>(), N, level, m_m.as<uint32_t>(), m_tok.as<uint64_t>(),
                                         m_mat.as<uint64_t>(), m_freq.as<uint32_t>(), segs);
  }
  {
    launch_scope ls(devid, "png_tables");
    png_tables<<<(unsigned)nseg, 64, 0, s>>>(m_freq.as<const uint32_t>(), N, level, segs);
  }
  {
    launch_scope ls(devid, "png_scan");
    png_scan<<<1, PT, 0, s>>>(segs, nseg, N, (uint32_t)head.size(), d->capacity, m_off.as<uint64_t>(), st,
                              (uint8_t *)dev_out);
  }
  {
    launch_scope ls(devid, "png_emit");
    png_zero<<<stream_grid(nwords, PT), PT, 0, s>>>(m_words.as<uint32_t>(), st);
    png_emit<<<(unsigned)nseg, PT, 0, s>>>(m_fs.as<const uint8_t>(), m_m.as<const uint32_t>(), m_tok.as<const uint64_t>(),
                                           m_mat.as<const uint64_t>(), segs, m_off.as<const uint64_t>(), nseg,
                                           m_words.as<uint32_t>());
    png_tail<<<1, 64, 0, s>>>(m_words.as<uint32_t>(), pd_zlib_header(level), st);
  }
  {
    launch_scope ls(devid, "png_idat");
    png_idat<<<(unsigned)std::min<uint64_t>(max_idat, 2048), PT, 0, s>>>(m_words.as<const uint8_t>(), st,
                                                                          (uint32_t)head.size(), crc_type,
                                                                          (uint8_t *)dev_out);
    png_head<<<1, PT, 0, s>>>(m_head.as<const uint8_t>(), (uint32_t)head.size(), st, (uint8_t *)dev_out);
  }
  return check_launch("export_png");
}

// tests only (not in include/ansel_hip.h): png_tables alone on caller-supplied histograms -- nseg x (PD_NLIT + PD_NDIST)
// host counts for a stream of nbytes bytes -- and the pd_seg_t records copied back to segs_out (the Adler sums are not
// set); at most 65536 histograms a call.  tests/native/png_host.cpp png_host_tables() is its twin with one lane.
extern "C" size_t dt_hip_test_png_sizeof_seg(void) { return sizeof(pd_seg_t); }

extern "C" int dt_hip_test_png_tables(int devid, const uint32_t *freq, uint64_t nbytes, int nseg, int level, void *segs_out)
{
  if(!valid_device(devid) || !freq || !segs_out || nseg < 1 || nseg > 65536 || level < 0 || level > 9) return DT_HIP_INVALID_ARG;
  if(nbytes <= (uint64_t)(nseg - 1) * PD_SEG || nbytes > (uint64_t)nseg * PD_SEG) return DT_HIP_INVALID_ARG;
  const size_t sz_freq = (size_t)nseg * NSYM * 4, sz_segs = (size_t)nseg * sizeof(pd_seg_t);
  const dev_buf_t m_freq = dev_buf_t::alloc(devid, sz_freq);
  const dev_buf_t m_segs = dev_buf_t::alloc(devid, sz_segs);
  int err = (m_freq && m_segs) ? DT_HIP_SUCCESS : DT_HIP_DEFAULT_ERROR;
  if(err == DT_HIP_SUCCESS) err = dt_hip_write_buffer_to_device(devid, freq, m_freq.ptr(), 0, sz_freq, 1);
  if(err == DT_HIP_SUCCESS)
  {
    hipStream_t s = stream_of(devid);
    if(hipMemsetAsync(m_segs.ptr(), 0, sz_segs, s) != hipSuccess) err = DT_HIP_DEFAULT_ERROR;
  }
  if(err == DT_HIP_SUCCESS)
  {
    {
      launch_scope ls(devid, "png_tables");
      png_tables<<<(unsigned)nseg, 64, 0, stream_of(devid)>>>(m_freq.as<const uint32_t>(), nbytes, level, m_segs.as<pd_seg_t>());
    }
    err = check_launch("test_png_tables");
  }
  if(err == DT_HIP_SUCCESS) err = dt_hip_read_buffer_from_device(devid, segs_out, m_segs.ptr(), 0, sz_segs, 1);
  return err;
}
