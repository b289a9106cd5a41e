// tiff.hip -- TIFF encoding of the export_u8 / export_u16 / float frame on gfx950: a little-endian classic TIFF in
// strips (BigTIFF is not written), the strips' payload libtiff's byte for byte, with DT_HIP_TIFF_DEFLATE every strip a
// zlib stream of its own from the deflate of png_deflate.h (tiff_body.h holds the format's body, deflate_kernels.h the
// deflate's device side).
//
// Stages, all on the device's stream, no host synchronisation:
//   tiff_rows     one thread per sample: alpha dropped (or sample 0 taken), predictor 2, the strips' payload
//   tiff_rows_fp  predictor 3: one workgroup per piece of a row, the piece's floats staged in LDS, four byte planes out
//   tiff_lz       one workgroup per segment of PD_SEG bytes of ONE strip (deflate_kernels.h dk_lz_segment(): the window
//                 and the hash tables never reach in front of the strip's first byte)
//   tiff_tables   one wave per segment
//   tiff_scan     one workgroup: every strip starts on a byte, so a strip's length needs no map composition -- a thread
//                 walks its strips' segments from bit 16 (the zlib header), then a workgroup scan of align2(length)
//                 gives StripOffsets, StripByteCounts, every segment's bit offset, the strips' Adler-32 and L
//   tiff_emit     one workgroup per segment, into a zeroed scratch image of the file
//   tiff_tail     per strip the zlib header and the Adler-32
//   tiff_copy     the scratch image (head, arrays, strips) into dev_out, when it fits
// Without compression every offset is host arithmetic: the head is uploaded and tiff_rows writes straight into dev_out.
// Nothing is written to dev_out past its capacity: the length word (the first 8 bytes) is L or UINT64_MAX, and the file
// bytes are written only when they fit.
#include <algorithm>
#include <vector>

#include "deflate_kernels.h"
#include "hip_common.h"
#include "tiff_body.h"

namespace ansel
{
namespace
{

constexpr int FP_PIECE = 2048; // samples of a row per workgroup of tiff_rows_fp

// the strips' payload layout in a kernel's destination
struct tstrips_t
{
  uint32_t row_bytes, rows, nstrips; // rows: of every strip but the last
  uint64_t strip_bytes, last_bytes;  // payload bytes
  uint64_t stride;                   // from one strip's first byte to the next one's
  uint64_t sps;                      // segments of a full strip
};

struct tstate_t
{
  uint64_t length; // L, or UINT64_MAX
  uint64_t file;   // L
  uint32_t fits;
};

__device__ __forceinline__ void store_sample(uint8_t *p, uint8_t v) { *p = v; }
__device__ __forceinline__ void store_sample(uint8_t *p, uint16_t v) { *(uint16_t *)p = v; }
// a strip starts on an even offset, not on a multiple of 4
__device__ __forceinline__ void store_sample(uint8_t *p, uint32_t v)
{
  ((uint16_t *)p)[0] = (uint16_t)v;
  ((uint16_t *)p)[1] = (uint16_t)(v >> 16);
}

// predictors 1 and 2: sample g of the frame (row-major, w * layers a row) into its strip; pad: the zero byte behind a
// strip of odd length (not behind the last)
template <class T>
__global__ __launch_bounds__(PT) void tiff_rows(const T *__restrict__ in, const int w, const int h, const int layers,
                                                const int predictor, const tstrips_t g, const bool pad,
                                                uint8_t *__restrict__ dst)
{
  const uint32_t n = (uint32_t)w * layers;
  const uint64_t total = (uint64_t)n * h;
  for(uint64_t q = blockIdx.x * (uint64_t)PT + threadIdx.x; q < total; q += (uint64_t)gridDim.x * PT)
  {
    const uint32_t y = (uint32_t)(q / n), i = (uint32_t)(q - (uint64_t)y * n);
    const uint32_t strip = y / g.rows, r = y - strip * g.rows;
    uint8_t *o = dst + strip * g.stride + (uint64_t)r * g.row_bytes;
    store_sample(o + (size_t)i * sizeof(T), tf_sample<T>(in, w, layers, predictor, (int)y, i));
    if(pad && i + 1 == n && r + 1 == g.rows && strip + 1 < g.nstrips && (g.strip_bytes & 1)) o[g.row_bytes] = 0;
  }
}

// predictor 3: workgroup (row, piece); the piece's samples and the `layers` in front of them from LDS, the few bytes
// that difference against the end of the previous plane from memory
__global__ __launch_bounds__(PT) void tiff_rows_fp(const uint32_t *__restrict__ in, const int w, const int layers,
                                                   const uint32_t pieces, const tstrips_t g, uint8_t *__restrict__ dst)
{
  __shared__ uint32_t bits[FP_PIECE + 4];
  const uint32_t n = (uint32_t)w * layers;
  const uint32_t y = blockIdx.x / pieces, piece = blockIdx.x - y * pieces;
  const uint32_t i0 = piece * FP_PIECE, i1 = min(n, i0 + FP_PIECE);
  const uint32_t lo = i0 >= (uint32_t)layers ? i0 - layers : 0;
  for(uint32_t i = lo + threadIdx.x; i < i1; i += PT) bits[i - lo] = tf_float_bits(in, w, layers, (int)y, i);
  __syncthreads();
  const uint32_t strip = y / g.rows, r = y - strip * g.rows;
  uint8_t *o = dst + strip * g.stride + (uint64_t)r * g.row_bytes;
  auto sample = [&](uint32_t i) { return (i >= lo && i < i1) ? bits[i - lo] : tf_float_bits(in, w, layers, (int)y, i); };
  for(uint32_t b = 0; b < 4; b++)
    for(uint32_t i = i0 + threadIdx.x; i < i1; i += PT) o[b * n + i] = (uint8_t)tf_fp_byte(n, layers, b * n + i, sample);
}

// segment k of all strips' segments: its strip, the strip's payload and length, the segment's bounds in it
struct tseg_t
{
  uint32_t strip;
  uint64_t base, N, s0, s1;
};

__device__ __forceinline__ tseg_t seg_of(const tstrips_t &g, uint64_t k)
{
  tseg_t s;
  s.strip = (uint32_t)(k / g.sps);
  s.base = s.strip * g.strip_bytes;
  s.N = s.strip + 1 == g.nstrips ? g.last_bytes : g.strip_bytes;
  s.s0 = (k - s.strip * g.sps) * PD_SEG;
  s.s1 = min(s.N, s.s0 + PD_SEG);
  return s;
}

__global__ __launch_bounds__(PT) void tiff_lz(const uint8_t *__restrict__ payload, const tstrips_t g, const int level,
                                              uint32_t *__restrict__ m, uint64_t *__restrict__ tokm,
                                              uint64_t *__restrict__ matm, uint32_t *__restrict__ freq,
                                              pd_seg_t *__restrict__ segs)
{
  const uint64_t k = blockIdx.x;
  const tseg_t s = seg_of(g, k);
  dk_lz_segment(payload + s.base, s.N, s.s0, s.s1, level, m + s.base, tokm + k * SEG_WORDS, matm + k * SEG_WORDS,
                freq + k * NSYM, &segs[k]);
}

__global__ __launch_bounds__(64) void tiff_tables(const uint32_t *__restrict__ freq, const tstrips_t g, const int level,
                                                  pd_seg_t *__restrict__ segs)
{
  const uint64_t k = blockIdx.x;
  const tseg_t s = seg_of(g, k);
  dk_tables_segment(freq + k * NSYM, (uint32_t)(s.s1 - s.s0), level, &segs[k]);
}

__device__ __forceinline__ void put_le32(uint8_t *p, uint32_t v)
{
  for(int b = 0; b < 4; b++) p[b] = (uint8_t)(v >> (8 * b));
}

__device__ __forceinline__ uint32_t get_le32(const uint8_t *p)
{
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// one workgroup: per strip the zlib stream's length and Adler-32, the strips' offsets (every one even), the segments'
// bit offsets in the file image, L and whether it fits, the length word
__global__ __launch_bounds__(PT) void tiff_scan(const pd_seg_t *__restrict__ segs, const tstrips_t g,
                                                const uint32_t data_start, const uint32_t pos_offsets,
                                                const uint32_t pos_counts, const uint64_t capacity,
                                                uint64_t *__restrict__ off, uint32_t *__restrict__ adler,
                                                uint8_t *__restrict__ image, tstate_t *__restrict__ st,
                                                uint8_t *__restrict__ out)
{
  const uint32_t t = threadIdx.x;
  const uint32_t per = (g.nstrips + PT - 1) / PT;
  const uint32_t q0 = min(g.nstrips, t * per), q1 = min(g.nstrips, q0 + per);
  uint64_t sum = 0;
  for(uint32_t q = q0; q < q1; q++)
  {
    const uint64_t N = q + 1 == g.nstrips ? g.last_bytes : g.strip_bytes;
    const uint64_t k0 = q * g.sps, k1 = k0 + (N + PD_SEG - 1) / PD_SEG;
    uint64_t o = 16, A = 0, B = 0, e = 0;
    for(uint64_t k = k0; k < k1; k++)
    {
      const pd_seg_t &s = segs[k];
      off[k] = o;
      o = pd_seg_end(s, o);
      e += s.nbytes;
      A += s.adler_s;
      B = (B + s.adler_t + ((N - e) % PD_ADLER_MOD) * s.adler_s) % PD_ADLER_MOD;
    }
    const uint32_t a = (uint32_t)((1 + A) % PD_ADLER_MOD), b = (uint32_t)((N % PD_ADLER_MOD + B) % PD_ADLER_MOD);
    adler[q] = (b << 16) | a;
    const uint64_t len = (o + 7) / 8 + 4;
    put_le32(image + pos_counts + 4 * (uint64_t)q, (uint32_t)len);
    sum += tf_align2(len);
  }
  uint64_t total;
  uint64_t at = data_start + block_exclusive_scan<uint64_t>(sum, &total);
  for(uint32_t q = q0; q < q1; q++)
  {
    const uint64_t N = q + 1 == g.nstrips ? g.last_bytes : g.strip_bytes;
    const uint64_t k0 = q * g.sps, k1 = k0 + (N + PD_SEG - 1) / PD_SEG;
    for(uint64_t k = k0; k < k1; k++) off[k] += 8 * at;
    put_le32(image + pos_offsets + 4 * (uint64_t)q, (uint32_t)at);
    const uint64_t len = get_le32(image + pos_counts + 4 * (uint64_t)q);
    if(q + 1 == g.nstrips)
    {
      const uint64_t L = at + len;
      const bool fits = 8 + L <= capacity;
      st->file = L;
      st->fits = fits;
      st->length = fits ? L : ~0ull;
      for(int i = 0; i < 8; i++) out[i] = (uint8_t)(st->length >> (8 * i));
    }
    at += tf_align2(len);
  }
}

// the strips' part of the file image, zeroed: whole words, and the two bytes in front of them where the first strip
// starts in the middle of a word (the bytes before belong to the head)
__global__ __launch_bounds__(PT) void tiff_zero(uint32_t *__restrict__ words, const uint32_t data_start,
                                                const tstate_t *__restrict__ st)
{
  const uint64_t w0 = ((uint64_t)data_start + 3) / 4, w1 = (st->file + 3) / 4;
  for(uint64_t i = w0 + blockIdx.x * (uint64_t)PT + threadIdx.x; i < w1; i += (uint64_t)gridDim.x * PT) words[i] = 0;
  if(blockIdx.x == 0 && threadIdx.x == 0)
    for(uint64_t i = data_start; i < 4 * w0; i++) ((uint8_t *)words)[i] = 0;
}

__global__ __launch_bounds__(PT) void tiff_emit(const uint8_t *__restrict__ payload, const tstrips_t g,
                                                const uint32_t *__restrict__ m, const uint64_t *__restrict__ tokm,
                                                const uint64_t *__restrict__ matm, const pd_seg_t *__restrict__ segs,
                                                const uint64_t *__restrict__ off, uint32_t *__restrict__ words)
{
  const uint64_t k = blockIdx.x;
  const tseg_t s = seg_of(g, k);
  dk_emit_segment(payload + s.base, s.s0, m + s.base, tokm + k * SEG_WORDS, matm + k * SEG_WORDS, &segs[k], off[k],
                  s.s1 == s.N, words);
}

// per strip the zlib header in front and the Adler-32 behind its blocks
__global__ __launch_bounds__(PT) void tiff_tail(uint32_t *__restrict__ words, const uint32_t nstrips,
                                                const uint32_t pos_offsets, const uint32_t pos_counts,
                                                const uint32_t zheader, const uint32_t *__restrict__ adler)
{
  const uint8_t *image = (const uint8_t *)words;
  for(uint32_t q = blockIdx.x * PT + threadIdx.x; q < nstrips; q += gridDim.x * PT)
  {
    const uint64_t at = get_le32(image + pos_offsets + 4 * (uint64_t)q), len = get_le32(image + pos_counts + 4 * (uint64_t)q);
    or_byte(words, at, zheader >> 8);
    or_byte(words, at + 1, zheader & 255);
    for(int i = 0; i < 4; i++) or_byte(words, at + len - 4 + i, adler[q] >> (24 - 8 * i));
  }
}

// n bytes (st given: the file, if it fits) to dst, in words where both sides are on a word
__global__ __launch_bounds__(PT) void tiff_copy(const uint8_t *__restrict__ src, const tstate_t *__restrict__ st,
                                                const uint64_t n_host, uint8_t *__restrict__ dst)
{
  const uint64_t n = st ? (st->fits ? st->file : 0) : n_host;
  const bool words = (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
  const uint64_t nw = words ? n / 4 : 0;
  for(uint64_t i = blockIdx.x * (uint64_t)PT + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * PT)
    ((uint32_t *)dst)[i] = ((const uint32_t *)src)[i];
  for(uint64_t i = 4 * nw + blockIdx.x * (uint64_t)PT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * PT) dst[i] = src[i];
}

__global__ void tiff_length_word(uint8_t *__restrict__ out, const uint64_t v)
{
  if(threadIdx.x < 8) out[threadIdx.x] = (uint8_t)(v >> (8 * threadIdx.x));
}

bool tiff_geometry(int width, int height, const dt_hip_tiff_data_t *d, const char *who, tf_geom_t *g, std::vector<uint8_t> *head)
{
  const char *why = tf_geometry(width, height, d, g, head);
  if(why) set_last_error("%s: %d x %d: %s", who, width, height, why);
  return !why;
}

void launch_rows(hipStream_t s, int width, int height, const dt_hip_tiff_data_t *d, const tstrips_t &ts, bool pad, const void *in,
                 uint8_t *dst)
{
  const uint32_t n = (uint32_t)width * d->layers;
  if(d->predictor == 3)
  {
    const uint32_t pieces = (n + FP_PIECE - 1) / FP_PIECE;
    tiff_rows_fp<<<pieces * (uint32_t)height, PT, 0, s>>>((const uint32_t *)in, width, d->layers, pieces, ts, dst);
    return;
  }
  const unsigned grid = stream_grid((size_t)n * height, PT);
  if(d->bpp == 8)
    tiff_rows<uint8_t><<<grid, PT, 0, s>>>((const uint8_t *)in, width, height, d->layers, d->predictor, ts, pad, dst);
  else if(d->bpp == 16)
    tiff_rows<uint16_t><<<grid, PT, 0, s>>>((const uint16_t *)in, width, height, d->layers, d->predictor, ts, pad, dst);
  else
    tiff_rows<uint32_t><<<grid, PT, 0, s>>>((const uint32_t *)in, width, height, d->layers, d->predictor, ts, pad, dst);
}

} // namespace
} // namespace ansel

using namespace ansel;

extern "C" size_t dt_hip_tiff_bound(int width, int height, const dt_hip_tiff_data_t *d)
{
  tf_geom_t g;
  if(!tiff_geometry(width, height, d, "dt_hip_tiff_bound", &g, nullptr)) return 0;
  return (size_t)g.bound;
}

extern "C" int dt_hip_export_tiff(int devid, int width, int height, const dt_hip_tiff_data_t *d, dt_hip_mem_t dev_in,
                                  dt_hip_mem_t dev_out)
{
  if(!valid_device(devid) || !dev_in || !dev_out) return DT_HIP_INVALID_ARG;
  tf_geom_t g;
  std::vector<uint8_t> head;
  if(!tiff_geometry(width, height, d, "export_tiff", &g, &head)) return DT_HIP_INVALID_ARG;
  if(d->capacity < 8)
  {
    set_last_error("export_tiff: capacity %llu cannot hold the 8-byte length word", (unsigned long long)d->capacity);
    return DT_HIP_INVALID_ARG;
  }
  hipStream_t s = stream_of(devid);
  uint8_t *out = (uint8_t *)dev_out;
  tstrips_t ts;
  ts.row_bytes = g.row_bytes;
  ts.rows = (uint32_t)(g.strip_bytes / g.row_bytes);
  ts.nstrips = g.nstrips;
  ts.strip_bytes = g.strip_bytes;
  ts.last_bytes = g.last_bytes;
  ts.sps = g.sps;
  if(d->compression == DT_HIP_TIFF_NONE)
  {
    // every position is known here: the head, then the rows straight into the file
    const uint64_t L = g.bound - 8;
    const bool fits = 8 + L <= d->capacity;
    ts.stride = tf_align2(g.strip_bytes);
    const dev_buf_t m_head = dev_buf_t::alloc(devid, head.size());
    if(!m_head) return DT_HIP_DEFAULT_ERROR;
    const int err = upload_small(devid, m_head.ptr(), head.data(), head.size());
    if(err != DT_HIP_SUCCESS) return err;
    launch_scope ls(devid, "tiff_rows");
    tiff_length_word<<<1, 64, 0, s>>>(out, fits ? L : ~0ull);
    if(fits)
    {
      tiff_copy<<<stream_grid(head.size() / 4 + 1, PT), PT, 0, s>>>(m_head.as<const uint8_t>(), nullptr, head.size(), out + 8);
      launch_rows(s, width, height, d, ts, true, dev_in, out + 8 + g.data_start);
    }
    return check_launch("export_tiff");
  }
  const int level = d->compression_level;
  const uint64_t N = (uint64_t)g.row_bytes * height, nseg = g.nseg;
  ts.stride = g.strip_bytes;
  const uint64_t nwords = (g.bound - 8) / 4 + 2;
  // scratch from the runtime's pool, released behind the launches (the pool's reuse is stream-ordered)
  const size_t sz_m = level ? (size_t)N * 4 : 4, sz_tok = level ? (size_t)nseg * SEG_WORDS * 8 : 8;
  const dev_buf_t m_pay = dev_buf_t::alloc(devid, (size_t)N);
  const dev_buf_t m_m = dev_buf_t::alloc(devid, sz_m);
  const dev_buf_t m_tok = dev_buf_t::alloc(devid, sz_tok);
  const dev_buf_t m_mat = dev_buf_t::alloc(devid, sz_tok);
  const dev_buf_t m_freq = dev_buf_t::alloc(devid, (size_t)nseg * NSYM * 4);
  const dev_buf_t m_segs = dev_buf_t::alloc(devid, (size_t)nseg * sizeof(pd_seg_t));
  const dev_buf_t m_off = dev_buf_t::alloc(devid, (size_t)nseg * 8);
  const dev_buf_t m_adler = dev_buf_t::alloc(devid, (size_t)g.nstrips * 4);
  const dev_buf_t m_words = dev_buf_t::alloc(devid, (size_t)nwords * 4);
  const dev_buf_t m_st = dev_buf_t::alloc(devid, sizeof(tstate_t));
  if(!m_pay || !m_m || !m_tok || !m_mat || !m_freq || !m_segs || !m_off || !m_adler || !m_words || !m_st) return DT_HIP_DEFAULT_ERROR;
  // the head is the first part of the file image; the device fills its two arrays
  const int err = upload_small(devid, m_words.ptr(), head.data(), head.size());
  if(err != DT_HIP_SUCCESS) return err;
  pd_seg_t *segs = m_segs.as<pd_seg_t>();
  tstate_t *st = m_st.as<tstate_t>();
  {
    launch_scope ls(devid, "tiff_rows");
    launch_rows(s, width, height, d, ts, false, dev_in, m_pay.as<uint8_t>());
  }
  {
    launch_scope ls(devid, "tiff_lz");
    tiff_lz<<<(unsigned)nseg, PT, 0, s>>>(m_pay.as<const uint8_t>(), ts, level, m_m.as<uint32_t>(), m_tok.as<uint64_t>(),
                                          m_mat.as<uint64_t>(), m_freq.as<uint32_t>(), segs);
  }
  {
    launch_scope ls(devid, "tiff_tables");
    tiff_tables<<<(unsigned)nseg, 64, 0, s>>>(m_freq.as<const uint32_t>(), ts, level, segs);
  }
  {
    launch_scope ls(devid, "tiff_scan");
    tiff_scan<<<1, PT, 0, s>>>(segs, ts, g.data_start, g.pos_offsets, g.pos_counts, d->capacity, m_off.as<uint64_t>(),
                               m_adler.as<uint32_t>(), m_words.as<uint8_t>(), st, out);
  }
  {
    launch_scope ls(devid, "tiff_emit");
    tiff_zero<<<stream_grid(nwords, PT), PT, 0, s>>>(m_words.as<uint32_t>(), g.data_start, st);
    tiff_emit<<<(unsigned)nseg, PT, 0, s>>>(m_pay.as<const uint8_t>(), ts, m_m.as<const uint32_t>(), m_tok.as<const uint64_t>(),
                                            m_mat.as<const uint64_t>(), segs, m_off.as<const uint64_t>(), m_words.as<uint32_t>());
    tiff_tail<<<stream_grid(g.nstrips, PT), PT, 0, s>>>(m_words.as<uint32_t>(), g.nstrips, g.pos_offsets, g.pos_counts,
                                                        pd_zlib_header(level), m_adler.as<const uint32_t>());
  }
  {
    launch_scope ls(devid, "tiff_copy");
    tiff_copy<<<stream_grid(nwords, PT), PT, 0, s>>>(m_words.as<const uint8_t>(), st, 0, out + 8);
  }
  return check_launch("export_tiff");
}
