// jpeg.hip -- baseline JPEG encoding of the export_u8 frame on gfx950: the libjpeg(-turbo) path that Ansel's
// src/imageio/format/jpeg.c write_image() runs on the host, byte for byte (tests/jpeg_ref.py restates it in numpy).
//
// Stages, all on the device's stream, no host synchronisation:
//   jpeg_fdct      one thread per 8x8 block in scan (MCU) order: RGB -> YCbCr (jccolor.c, SCALEBITS 16), the
//                  downsampling of jcsample.c (h2v1 bias 0,1 / h2v2 bias 1,2 by output column) over the edge
//                  expansion of jcprep.c (last column / row replicated), jpeg_fdct_islow (jfdctint.c), the quantizer
//                  of jcdctmgr.c (divide by 8 q, round half away from zero) and jccoefct.c's dummy blocks (AC zero,
//                  DC of the neighbouring block).  The int16 coefficients are stored in zigzag order (128 B / block):
//                  the three later passes read them instead of recomputing the transform.
//   jpeg_stats     (optimize_coding) the DC / AC symbol counts of jchuff.c: an LDS histogram per workgroup, then one
//                  integer atomic per bin -- order-free, so the counts and the tables are deterministic.
//   jpeg_tables    one wave per table: jpeg_gen_optimal_table() (jpeg_huff.h), or the Annex K tables of
//                  jpeg_set_defaults(); then the code / length of every symbol.
//   jpeg_lengths   each block's bit count and each workgroup's sum; jpeg_scan_partials scans the sums (one
//                  workgroup): a multi-kernel reduce-then-scan.
//   jpeg_emit      each block writes its bits at its offset; a word shared with a neighbouring block is combined
//                  with an integer OR.
//   jpeg_ff_count / jpeg_ff_scan / jpeg_compact
//                  byte stuffing (0xFF -> 0xFF 0x00) per 4 KB chunk: count, scan, compact into dev_out; the last byte
//                  padded with 1-bits.  jpeg_ff_scan also fixes the file length L and whether 8 + L fits the capacity.
//   jpeg_headers   the header bytes: SOI .. SOF0 (host-built, they depend on no pixel) then DHT x 4 and SOS from the
//                  tables, EOI at the end.
// Nothing is written to dev_out past its capacity: the length word (the first 8 bytes) is L or UINT64_MAX, and the
// file bytes are written only when they fit.
#include <algorithm>
#include <vector>

#include "hip_common.h"
#include "jpeg_huff.h"

namespace ansel
{
namespace
{

constexpr int JPEG_THREADS = 256; // blocks per workgroup in the per-block passes
constexpr int CHUNK = 4096;       // bytes per chunk of the stuffing pass: 256 threads x 16 bytes
constexpr int BLOCK_BITS = 1665;  // the most one block can emit: DC 16 + 11, 63 x (16 + 10)
constexpr int HDR_FIXED_MAX = 2 + 18 + 2 * 69 + 19; // SOI, APP0, DQT x 2, SOF0 (ICC chunks come on top)
constexpr int HDR_TAIL_MAX = 4 * (4 + 1 + 16 + 256) + 14; // DHT x 4, SOS

__constant__ uint8_t c_zigzag[64] = { 0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                      12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                      58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

// jcparam.c std_huff_tables (T.81 Annex K.3): DC0, AC0, DC1, AC1
__constant__ uint8_t c_std_bits[4][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 },
                                           { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d },
                                           { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 },
                                           { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 } };
__constant__ uint8_t c_std_dc_vals[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
__constant__ uint8_t c_std_ac0_vals[162] = {
  0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
  0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
  0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
  0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
  0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
  0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
  0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
  0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
  0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa
};
__constant__ uint8_t c_std_ac1_vals[162] = {
  0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
  0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
  0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
  0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
  0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
  0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
  0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
  0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
  0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa
};

// the frame's block layout (libjpeg's jinit_c_master_control / per_scan_setup for one interleaved scan)
struct geom_t
{
  int w, h;
  int hy, vy;        // Y sampling factors; Cb / Cr are 1 x 1
  int nb;            // blocks per MCU: hy * vy + 2
  int mcux, mcuy;
  int wib[3], hib[3]; // width / height in (real) blocks per component
  uint32_t nblocks;   // mcux * mcuy * nb
};

struct quant_t
{
  uint16_t div[2][64]; // 8 q, natural order
};

// Huffman tables after jpeg_tables
struct tables_t
{
  uint16_t code[4][256];
  uint8_t size[4][256];
  uint8_t bits[4][16];
  uint8_t vals[4][256];
  uint32_t nvals[4];
};

// the device-side bookkeeping of one call
struct state_t
{
  uint64_t total_bits;
  uint64_t nbytes;    // entropy-coded bytes before stuffing
  uint64_t nchunks;
  uint64_t length;    // L, or UINT64_MAX
  uint32_t hdr_len;
  uint32_t fits;
};

// block b of the scan: component, position in the component's (MCU-padded) block grid
struct block_t
{
  int c, bx, by;
};

__device__ __forceinline__ block_t block_of(const geom_t &g, uint32_t b)
{
  const uint32_t mcu = b / (uint32_t)g.nb;
  const int j = (int)(b - mcu * (uint32_t)g.nb);
  const int my = (int)(mcu / (uint32_t)g.mcux), mx = (int)(mcu - (uint32_t)my * (uint32_t)g.mcux);
  const int ny = g.hy * g.vy;
  block_t r;
  if(j < ny)
  {
    r.c = 0;
    r.by = my * g.vy + j / g.hy;
    r.bx = mx * g.hy + j % g.hy;
  }
  else
  {
    r.c = j - ny + 1;
    r.by = my;
    r.bx = mx;
  }
  return r;
}

// the block whose DC the previous DC of block b's component is (jchuff.c last_dc_val, in MCU order); -1: none (0)
__device__ __forceinline__ int64_t prev_block(const geom_t &g, uint32_t b)
{
  const uint32_t mcu = b / (uint32_t)g.nb;
  const int j = (int)(b - mcu * (uint32_t)g.nb);
  const int ny = g.hy * g.vy;
  const int j0 = j < ny ? 0 : j;
  const int nc = j < ny ? ny : 1;
  if(j > j0) return (int64_t)b - 1;
  if(mcu == 0) return -1;
  return (int64_t)(mcu - 1) * g.nb + j0 + nc - 1;
}

// jccolor.c: one of Y, Cb, Cr of an RGBA8 pixel (little-endian r g b a)
__device__ __forceinline__ int ycc(uint32_t px, int c)
{
  const int r = px & 255, gg = (px >> 8) & 255, b = (px >> 16) & 255;
  constexpr int ONE_HALF = 1 << 15, CBCR_OFFSET = 128 << 16;
  if(c == 0) return (19595 * r + 38470 * gg + 7471 * b + ONE_HALF) >> 16;
  if(c == 1) return (-11059 * r - 21709 * gg + 32768 * b + CBCR_OFFSET + ONE_HALF - 1) >> 16;
  return (32768 * r - 27439 * gg - 5329 * b + CBCR_OFFSET + ONE_HALF - 1) >> 16;
}

// the FDCT input sample (x, y) of component c: full resolution with the last column / row replicated, or
// downsampled (the component's x, y) from the replicated plane; rows past the last downsampled row replicate it
__device__ __forceinline__ int sample(const uint32_t *__restrict__ in, const geom_t &g, int c, int x, int y)
{
  const int W = g.w, H = g.h;
  if(c == 0 || (g.hy == 1 && g.vy == 1))
    return ycc(in[(size_t)min(y, H - 1) * W + min(x, W - 1)], c);
  const int xa = min(2 * x, W - 1), xb = min(2 * x + 1, W - 1);
  if(g.vy == 1)
  {
    const uint32_t *row = in + (size_t)min(y, H - 1) * W;
    return (ycc(row[xa], c) + ycc(row[xb], c) + (x & 1)) >> 1;
  }
  const int y2 = min(y, (H + 1) / 2 - 1);
  const uint32_t *ra = in + (size_t)min(2 * y2, H - 1) * W;
  const uint32_t *rb = in + (size_t)min(2 * y2 + 1, H - 1) * W;
  return (ycc(ra[xa], c) + ycc(ra[xb], c) + ycc(rb[xa], c) + ycc(rb[xb], c) + 1 + (x & 1)) >> 2;
}

// jfdctint.c jpeg_fdct_islow, one pass over 8 values with stride s (first: the row pass)
template <bool FIRST>
__device__ __forceinline__ void fdct_pass(int *d, int s)
{
  constexpr int CB = 13, PB = 2;
  constexpr int N = FIRST ? CB - PB : CB + PB;
  const int t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s];
  const int t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
  const int t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s];
  const int t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if(FIRST)
  {
    d[0] = (t10 + t11) * (1 << PB);
    d[4 * s] = (t10 - t11) * (1 << PB);
  }
  else
  {
    d[0] = (t10 + t11 + (1 << (PB - 1))) >> PB;
    d[4 * s] = (t10 - t11 + (1 << (PB - 1))) >> PB;
  }
  int z1 = (t12 + t13) * 4433;
  d[2 * s] = (z1 + t13 * 6270 + (1 << (N - 1))) >> N;
  d[6 * s] = (z1 - t12 * 15137 + (1 << (N - 1))) >> N;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * s] = (a4 + z1 + z3 + (1 << (N - 1))) >> N;
  d[5 * s] = (a5 + z2 + z4 + (1 << (N - 1))) >> N;
  d[3 * s] = (a6 + z2 + z3 + (1 << (N - 1))) >> N;
  d[s] = (a7 + z1 + z4 + (1 << (N - 1))) >> N;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_fdct(const uint32_t *__restrict__ in, const geom_t g, const quant_t q,
                                                          int16_t *__restrict__ coef)
{
  const uint32_t b = blockIdx.x * JPEG_THREADS + threadIdx.x;
  if(b >= g.nblocks) return;
  const block_t k = block_of(g, b);
  const int wib = g.wib[k.c], hib = g.hib[k.c];
  const int h = k.c == 0 ? g.hy : 1;
  // the block whose transform this one is (itself, or the real neighbour whose DC a dummy block copies)
  int sx = k.bx, sy = k.by;
  const bool dummy = k.bx >= wib || k.by >= hib;
  if(k.by >= hib)
  {
    sy = hib - 1;
    sx = min((k.bx / h) * h + h - 1, wib - 1);
  }
  else if(k.bx >= wib)
    sx = wib - 1;
  int d[64];
#pragma unroll
  for(int r = 0; r < 8; r++)
#pragma unroll
    for(int x = 0; x < 8; x++) d[r * 8 + x] = sample(in, g, k.c, sx * 8 + x, sy * 8 + r) - 128;
#pragma unroll
  for(int r = 0; r < 8; r++) fdct_pass<true>(d + r * 8, 1);
#pragma unroll
  for(int x = 0; x < 8; x++) fdct_pass<false>(d + x, 8);
  const uint16_t *div = q.div[k.c == 0 ? 0 : 1];
  int16_t out[64];
#pragma unroll
  for(int i = 0; i < 64; i++)
  {
    const int v = d[c_zigzag[i]];
    const unsigned dv = div[c_zigzag[i]];
    const int a = (int)(((unsigned)abs(v) + (dv >> 1)) / dv);
    out[i] = (int16_t)(v < 0 ? -a : a);
  }
  if(dummy)
  {
#pragma unroll
    for(int i = 1; i < 64; i++) out[i] = 0;
  }
  uint4 *dst = (uint4 *)(coef + (size_t)b * 64);
#pragma unroll
  for(int i = 0; i < 8; i++)
  {
    uint4 v;
    v.x = (uint16_t)out[i * 8 + 0] | ((uint32_t)(uint16_t)out[i * 8 + 1] << 16);
    v.y = (uint16_t)out[i * 8 + 2] | ((uint32_t)(uint16_t)out[i * 8 + 3] << 16);
    v.z = (uint16_t)out[i * 8 + 4] | ((uint32_t)(uint16_t)out[i * 8 + 5] << 16);
    v.w = (uint16_t)out[i * 8 + 6] | ((uint32_t)(uint16_t)out[i * 8 + 7] << 16);
    dst[i] = v;
  }
}

__device__ __forceinline__ int nbits_of(int v)
{
  const unsigned a = (unsigned)abs(v);
  return a ? 32 - __clz(a) : 0;
}

// jchuff.c encode_one_block / htest_one_block: emit(table 0 DC / 1 AC, symbol, extra bits, their count) in file order
template <class F>
__device__ __forceinline__ void walk_block(const int16_t *__restrict__ c, int last_dc, F emit)
{
  int v[64];
  const uint4 *src = (const uint4 *)c;
#pragma unroll
  for(int i = 0; i < 8; i++)
  {
    const uint4 u = src[i];
    const uint32_t w4[4] = { u.x, u.y, u.z, u.w };
#pragma unroll
    for(int j = 0; j < 4; j++)
    {
      v[i * 8 + 2 * j] = (int16_t)(w4[j] & 0xffff);
      v[i * 8 + 2 * j + 1] = (int16_t)(w4[j] >> 16);
    }
  }
  const int diff = v[0] - last_dc;
  int nb = nbits_of(diff);
  emit(0, nb, (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
  int r = 0;
#pragma unroll
  for(int k = 1; k < 64; k++)
  {
    const int a = v[k];
    if(a == 0)
    {
      r++;
      continue;
    }
    while(r > 15)
    {
      emit(1, 0xF0, 0u, 0);
      r -= 16;
    }
    nb = nbits_of(a);
    emit(1, (r << 4) + nb, (unsigned)(a < 0 ? a - 1 : a) & ((1u << nb) - 1), nb);
    r = 0;
  }
  if(r > 0) emit(1, 0, 0u, 0);
}

__device__ __forceinline__ int last_dc_of(const geom_t &g, const int16_t *__restrict__ coef, uint32_t b)
{
  const int64_t p = prev_block(g, b);
  return p < 0 ? 0 : coef[(size_t)p * 64];
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_stats(const int16_t *__restrict__ coef, const geom_t g,
                                                           uint32_t *__restrict__ freq)
{
  __shared__ uint32_t hist[4 * JH_NSYM];
  for(int i = threadIdx.x; i < 4 * JH_NSYM; i += JPEG_THREADS) hist[i] = 0;
  __syncthreads();
  const uint32_t b = blockIdx.x * JPEG_THREADS + threadIdx.x;
  if(b < g.nblocks)
  {
    const int t = block_of(g, b).c == 0 ? 0 : 2;
    walk_block(coef + (size_t)b * 64, last_dc_of(g, coef, b),
               [&](int ac, int sym, unsigned, int) { atomicAdd(&hist[(t + ac) * JH_NSYM + sym], 1u); });
  }
  __syncthreads();
  for(int i = threadIdx.x; i < 4 * JH_NSYM; i += JPEG_THREADS)
    if(hist[i]) atomicAdd(&freq[i], hist[i]);
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t k)
{
#pragma unroll
  for(int o = 32; o > 0; o >>= 1)
  {
    const uint64_t other = __shfl_xor(k, o, 64);
    k = other < k ? other : k;
  }
  return k;
}

// one wave per table (blockIdx.x = DC0, AC0, DC1, AC1)
__global__ __launch_bounds__(64) void jpeg_tables(const uint32_t *__restrict__ freq, const int optimize,
                                                  tables_t *__restrict__ tab)
{
  __shared__ jh_work_t w;
  __shared__ uint8_t bits[16], vals[256];
  __shared__ int nvals;
  const int t = blockIdx.x, lane = threadIdx.x;
  if(optimize)
  {
    for(int i = lane; i < 256; i += 64) w.freq[i] = freq[t * JH_NSYM + i];
    __syncthreads();
    const int n = jh_gen_optimal_table(
        &w, lane, 64, [](uint64_t k) { return wave_min_u64(k); }, []() { __syncthreads(); }, bits, vals);
    if(lane == 0) nvals = n;
  }
  else if(lane == 0)
  {
    const uint8_t *sv = (t & 1) ? (t == 1 ? c_std_ac0_vals : c_std_ac1_vals) : c_std_dc_vals;
    int n = 0;
    for(int l = 0; l < 16; l++)
    {
      bits[l] = c_std_bits[t][l];
      n += bits[l];
    }
    for(int i = 0; i < n; i++) vals[i] = sv[i];
    nvals = n;
  }
  __syncthreads();
  if(lane == 0)
  {
    jh_derive(bits, vals, tab->code[t], tab->size[t]);
    for(int l = 0; l < 16; l++) tab->bits[t][l] = bits[l];
    for(int i = 0; i < nvals; i++) tab->vals[t][i] = vals[i];
    tab->nvals[t] = (uint32_t)nvals;
  }
}

// inclusive scan of one value per thread over a 256-thread workgroup; returns the exclusive prefix, *total the sum
template <class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *total)
{
  __shared__ T s[JPEG_THREADS];
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for(int o = 1; o < JPEG_THREADS; o <<= 1)
  {
    const T a = t >= o ? s[t - o] : (T)0;
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  const T incl = s[t];
  *total = s[JPEG_THREADS - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_lengths(const int16_t *__restrict__ coef, const geom_t g,
                                                             const tables_t *__restrict__ tab, uint32_t *__restrict__ len,
                                                             uint64_t *__restrict__ partial)
{
  __shared__ uint8_t size[4][256];
  for(int i = threadIdx.x; i < 4 * 256; i += JPEG_THREADS) (&size[0][0])[i] = (&tab->size[0][0])[i];
  __syncthreads();
  const uint32_t b = blockIdx.x * JPEG_THREADS + threadIdx.x;
  uint32_t n = 0;
  if(b < g.nblocks)
  {
    const int t = block_of(g, b).c == 0 ? 0 : 2;
    walk_block(coef + (size_t)b * 64, last_dc_of(g, coef, b),
               [&](int ac, int sym, unsigned, int nb) { n += size[t + ac][sym] + nb; });
    len[b] = n;
  }
  uint32_t total;
  (void)block_exclusive_scan<uint32_t>(n, &total);
  if(threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the per-workgroup bit counts, and the total
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_scan_partials(uint64_t *__restrict__ partial, const uint32_t n,
                                                                   state_t *__restrict__ st)
{
  uint64_t carry = 0;
  for(uint32_t base = 0; base < n; base += JPEG_THREADS)
  {
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < n ? partial[i] : 0;
    uint64_t total;
    const uint64_t ex = block_exclusive_scan<uint64_t>(v, &total);
    if(i < n) partial[i] = carry + ex;
    carry += total;
  }
  if(threadIdx.x == 0)
  {
    st->total_bits = carry;
    st->nbytes = (carry + 7) / 8;
    st->nchunks = (st->nbytes + CHUNK - 1) / CHUNK;
  }
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_zero(uint32_t *__restrict__ words, const state_t *__restrict__ st)
{
  const uint64_t n = (st->total_bits + 31) / 32;
  for(uint64_t i = blockIdx.x * (uint64_t)JPEG_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * JPEG_THREADS)
    words[i] = 0;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_emit(const int16_t *__restrict__ coef, const geom_t g,
                                                          const tables_t *__restrict__ tab, const uint32_t *__restrict__ len,
                                                          const uint64_t *__restrict__ partial, uint32_t *__restrict__ words)
{
  __shared__ uint16_t code[4][256];
  __shared__ uint8_t size[4][256];
  for(int i = threadIdx.x; i < 4 * 256; i += JPEG_THREADS)
  {
    (&code[0][0])[i] = (&tab->code[0][0])[i];
    (&size[0][0])[i] = (&tab->size[0][0])[i];
  }
  const uint32_t b = blockIdx.x * JPEG_THREADS + threadIdx.x;
  const uint32_t n = b < g.nblocks ? len[b] : 0;
  uint32_t total;
  const uint32_t ex = block_exclusive_scan<uint32_t>(n, &total); // its barriers also cover the table loads
  if(b >= g.nblocks) return;
  const uint64_t start = partial[blockIdx.x] + ex;
  // acc holds nacc pending bits (the low ones); the first word starts at bit (start & 31) of word start >> 5
  uint64_t acc = 0;
  int nacc = (int)(start & 31);
  uint64_t wi = start >> 5;
  bool first = true;
  const int t = block_of(g, b).c == 0 ? 0 : 2;
  auto put = [&](int ac, int sym, unsigned extra, int nb) {
    const int tt = t + ac;
    const int l = size[tt][sym];
    acc = (acc << (l + nb)) | ((uint64_t)code[tt][sym] << nb) | extra;
    nacc += l + nb;
    if(nacc >= 32)
    {
      const uint32_t word = (uint32_t)(acc >> (nacc - 32));
      if(first)
        atomicOr(&words[wi], word);
      else
        words[wi] = word;
      first = false;
      wi++;
      nacc -= 32;
    }
  };
  walk_block(coef + (size_t)b * 64, last_dc_of(g, coef, b), put);
  if(nacc > 0) atomicOr(&words[wi], (uint32_t)(acc << (32 - nacc)));
}

__device__ __forceinline__ uint32_t entropy_byte(const uint32_t *__restrict__ words, const state_t &st, uint64_t i)
{
  uint32_t v = (words[i >> 2] >> (24 - 8 * (i & 3))) & 255;
  if(i == st.nbytes - 1 && (st.total_bits & 7)) v |= (1u << (8 - (st.total_bits & 7))) - 1; // pad with 1-bits
  return v;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_ff_count(const uint32_t *__restrict__ words,
                                                              const state_t *__restrict__ stp, uint32_t *__restrict__ cnt)
{
  const state_t st = *stp;
  for(uint64_t c = blockIdx.x; c < st.nchunks; c += gridDim.x)
  {
    const uint64_t i0 = c * CHUNK + threadIdx.x * 16;
    uint32_t n = 0;
    for(int j = 0; j < 16; j++)
      if(i0 + j < st.nbytes) n += entropy_byte(words, st, i0 + j) == 0xFF;
    uint32_t total;
    (void)block_exclusive_scan<uint32_t>(n, &total);
    if(threadIdx.x == 0) cnt[c] = total;
  }
}

// one workgroup: exclusive scan of the chunks' 0xFF counts, the header length, L and whether it fits; the length word
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_ff_scan(uint32_t *__restrict__ cnt, state_t *__restrict__ st,
                                                             const tables_t *__restrict__ tab, const uint32_t hdr_fixed,
                                                             const uint64_t capacity, uint8_t *__restrict__ out)
{
  const uint64_t n = st->nchunks;
  uint64_t carry = 0;
  for(uint64_t base = 0; base < n; base += JPEG_THREADS)
  {
    const uint64_t i = base + threadIdx.x;
    const uint32_t v = i < n ? cnt[i] : 0;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan<uint32_t>(v, &total);
    if(i < n) cnt[i] = (uint32_t)(carry + ex); // < 2^32: at most one stuffed byte per entropy byte of a chunk offset
    carry += total;
  }
  if(threadIdx.x == 0)
  {
    uint32_t hdr = hdr_fixed + 14; // SOS
    for(int t = 0; t < 4; t++) hdr += 5 + 16 + tab->nvals[t];
    const uint64_t L = hdr + st->nbytes + carry + 2;
    const bool fits = 8 + L <= capacity;
    st->hdr_len = hdr;
    st->fits = fits;
    st->length = fits ? L : ~0ull;
    const uint64_t word = st->length;
    for(int k = 0; k < 8; k++) out[k] = (uint8_t)(word >> (8 * k));
  }
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_compact(const uint32_t *__restrict__ words,
                                                             const state_t *__restrict__ stp,
                                                             const uint32_t *__restrict__ off, uint8_t *__restrict__ out)
{
  const state_t st = *stp;
  if(!st.fits) return;
  uint8_t *dst = out + 8 + st.hdr_len;
  for(uint64_t c = blockIdx.x; c < st.nchunks; c += gridDim.x)
  {
    const uint64_t i0 = c * CHUNK + threadIdx.x * 16;
    uint32_t v[16];
    uint32_t n = 0;
#pragma unroll
    for(int j = 0; j < 16; j++)
    {
      v[j] = i0 + j < st.nbytes ? entropy_byte(words, st, i0 + j) : 0x100;
      n += v[j] == 0xFF;
    }
    uint32_t total;
    uint64_t o = i0 + off[c] + block_exclusive_scan<uint32_t>(n, &total);
#pragma unroll
    for(int j = 0; j < 16; j++)
    {
      if(v[j] > 0xFF) break;
      dst[o++] = (uint8_t)v[j];
      if(v[j] == 0xFF) dst[o++] = 0;
    }
  }
}

// the header (host-built SOI .. SOF0, then DHT x 4 and SOS from the tables) and EOI, when the file fits
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_headers(const uint8_t *__restrict__ fixed, const uint32_t nfixed,
                                                             const tables_t *__restrict__ tab,
                                                             const state_t *__restrict__ stp, uint8_t *__restrict__ out)
{
  const state_t st = *stp;
  if(!st.fits) return;
  uint8_t *o = out + 8;
  for(uint32_t i = threadIdx.x; i < nfixed; i += JPEG_THREADS) o[i] = fixed[i];
  if(threadIdx.x == 0)
  {
    uint32_t p = nfixed;
    for(int t = 0; t < 4; t++)
    {
      const uint32_t nv = tab->nvals[t];
      const uint32_t l = 2 + 1 + 16 + nv;
      o[p++] = 0xFF;
      o[p++] = 0xC4;
      o[p++] = (uint8_t)(l >> 8);
      o[p++] = (uint8_t)l;
      o[p++] = (uint8_t)(((t & 1) << 4) | (t >> 1));
      for(int k = 0; k < 16; k++) o[p++] = tab->bits[t][k];
      for(uint32_t k = 0; k < nv; k++) o[p++] = tab->vals[t][k];
    }
    const uint8_t sos[14] = { 0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0 };
    for(int k = 0; k < 14; k++) o[p++] = sos[k];
    o[st.length - 2] = 0xFF;
    o[st.length - 1] = 0xD9;
  }
}

// jcparam.c jpeg_set_quality(q, force_baseline = TRUE) -> jpeg_add_quant_table(): natural order
const uint8_t std_quant[2][64] = {
  { 16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
    69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
    81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 },
  { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
    99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 }
};
const uint8_t zigzag[64] = { 0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
constexpr size_t ICC_CHUNK = 65519; // 65533 bytes of marker payload less "ICC_PROFILE\0", sequence number, count

void quant_tables(int quality, uint8_t qt[2][64])
{
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for(int t = 0; t < 2; t++)
    for(int i = 0; i < 64; i++)
    {
      long v = ((long)std_quant[t][i] * scale + 50) / 100;
      qt[t][i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

geom_t geometry(int w, int h, int subsampling)
{
  geom_t g;
  g.w = w;
  g.h = h;
  g.hy = subsampling == DT_HIP_JPEG_444 ? 1 : 2;
  g.vy = subsampling == DT_HIP_JPEG_420 ? 2 : 1;
  g.nb = g.hy * g.vy + 2;
  g.mcux = (w + 8 * g.hy - 1) / (8 * g.hy);
  g.mcuy = (h + 8 * g.vy - 1) / (8 * g.vy);
  g.wib[0] = (w + 7) / 8;
  g.hib[0] = (h + 7) / 8;
  g.wib[1] = g.wib[2] = g.mcux;
  g.hib[1] = g.hib[2] = g.mcuy;
  g.nblocks = (uint32_t)g.mcux * (uint32_t)g.mcuy * (uint32_t)g.nb;
  return g;
}

size_t icc_chunks(uint64_t icc_bytes) { return (size_t)((icc_bytes + ICC_CHUNK - 1) / ICC_CHUNK); }

void put_marker(std::vector<uint8_t> &o, uint8_t m, size_t payload)
{
  o.push_back(0xFF);
  o.push_back(m);
  o.push_back((uint8_t)((payload + 2) >> 8));
  o.push_back((uint8_t)(payload + 2));
}

// SOI, APP0 JFIF 1.01, APP2 ICC_PROFILE chunks, DQT x 2, SOF0 (jcmarker.c write_file_header / write_frame_header)
std::vector<uint8_t> fixed_header(int w, int h, const dt_hip_jpeg_data_t *d)
{
  std::vector<uint8_t> o = { 0xFF, 0xD8 };
  put_marker(o, 0xE0, 14);
  const uint8_t app0[14] = { 'J', 'F', 'I', 'F', 0, 1, 1, (uint8_t)d->density_unit, (uint8_t)(d->x_density >> 8),
                             (uint8_t)d->x_density, (uint8_t)(d->y_density >> 8), (uint8_t)d->y_density, 0, 0 };
  o.insert(o.end(), app0, app0 + 14);
  const size_t n = d->icc ? icc_chunks(d->icc_bytes) : 0;
  for(size_t i = 0; i < n; i++)
  {
    const size_t off = i * ICC_CHUNK, len = std::min<size_t>(ICC_CHUNK, d->icc_bytes - off);
    put_marker(o, 0xE2, 14 + len);
    const char tag[12] = "ICC_PROFILE";
    o.insert(o.end(), tag, tag + 12);
    o.push_back((uint8_t)(i + 1));
    o.push_back((uint8_t)n);
    const uint8_t *src = (const uint8_t *)d->icc + off;
    o.insert(o.end(), src, src + len);
  }
  uint8_t qt[2][64];
  quant_tables(d->quality, qt);
  for(int t = 0; t < 2; t++)
  {
    put_marker(o, 0xDB, 65);
    o.push_back((uint8_t)t);
    for(int k = 0; k < 64; k++) o.push_back(qt[t][zigzag[k]]);
  }
  const int hy = d->subsampling == DT_HIP_JPEG_444 ? 1 : 2, vy = d->subsampling == DT_HIP_JPEG_420 ? 2 : 1;
  put_marker(o, 0xC0, 15);
  const uint8_t sof[15] = { 8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, 3,
                            1, (uint8_t)(hy * 16 + vy), 0, 2, 0x11, 1, 3, 0x11, 1 };
  o.insert(o.end(), sof, sof + 15);
  return o;
}

bool valid_args(int width, int height, const dt_hip_jpeg_data_t *d, const char *who)
{
  if(!d)
  {
    set_last_error("%s: no dt_hip_jpeg_data_t", who);
    return false;
  }
  if(width < 1 || width > 65535 || height < 1 || height > 65535)
  {
    set_last_error("%s: %d x %d is outside 1..65535 (the frame header's 16-bit dimensions)", who, width, height);
    return false;
  }
  if(d->subsampling != DT_HIP_JPEG_444 && d->subsampling != DT_HIP_JPEG_422 && d->subsampling != DT_HIP_JPEG_420)
  {
    set_last_error("%s: subsampling %d is not DT_HIP_JPEG_444 / _422 / _420", who, (int)d->subsampling);
    return false;
  }
  if(d->quality < 1 || d->quality > 100)
  {
    set_last_error("%s: quality %d is outside 1..100", who, (int)d->quality);
    return false;
  }
  if(d->density_unit < 0 || d->density_unit > 2 || d->x_density < 0 || d->x_density > 65535 || d->y_density < 0
     || d->y_density > 65535)
  {
    set_last_error("%s: density unit %d / %d x %d does not fit the JFIF header", who, (int)d->density_unit,
                   (int)d->x_density, (int)d->y_density);
    return false;
  }
  if(d->icc_bytes && !d->icc)
  {
    set_last_error("%s: icc_bytes %llu without an icc pointer", who, (unsigned long long)d->icc_bytes);
    return false;
  }
  if(d->icc && icc_chunks(d->icc_bytes) > 255)
  {
    set_last_error("%s: an ICC profile of %llu bytes needs more than 255 APP2 chunks", who,
                   (unsigned long long)d->icc_bytes);
    return false;
  }
  return true;
}

} // namespace
} // namespace ansel

using namespace ansel;

extern "C" size_t dt_hip_jpeg_bound(int width, int height, const dt_hip_jpeg_data_t *d)
{
  if(!valid_args(width, height, d, "dt_hip_jpeg_bound")) return 0;
  const geom_t g = geometry(width, height, d->subsampling);
  const uint64_t entropy = ((uint64_t)g.nblocks * BLOCK_BITS + 7) / 8;
  const uint64_t icc = d->icc ? d->icc_bytes + icc_chunks(d->icc_bytes) * 18 : 0;
  return (size_t)(8 + HDR_FIXED_MAX + icc + HDR_TAIL_MAX + 2 * entropy + 2);
}

extern "C" int dt_hip_export_jpeg(int devid, int width, int height, const dt_hip_jpeg_data_t *d,
                                  dt_hip_mem_t dev_in_rgba8, dt_hip_mem_t dev_out)
{
  if(!valid_device(devid) || !dev_in_rgba8 || !dev_out) return DT_HIP_INVALID_ARG;
  if(!valid_args(width, height, d, "export_jpeg")) return DT_HIP_INVALID_ARG;
  if(d->capacity < 8)
  {
    set_last_error("export_jpeg: capacity %llu cannot hold the 8-byte length word", (unsigned long long)d->capacity);
    return DT_HIP_INVALID_ARG;
  }
  const geom_t g = geometry(width, height, d->subsampling);
  const std::vector<uint8_t> fixed = fixed_header(width, height, d);
  quant_t q;
  {
    uint8_t qt[2][64];
    quant_tables(d->quality, qt);
    for(int t = 0; t < 2; t++)
      for(int i = 0; i < 64; i++) q.div[t][i] = (uint16_t)(8 * qt[t][i]);
  }
  const uint32_t nwg = (g.nblocks + JPEG_THREADS - 1) / JPEG_THREADS;
  const uint64_t max_bits = (uint64_t)g.nblocks * BLOCK_BITS;
  const uint64_t max_chunks = (max_bits / 8 + 1 + CHUNK - 1) / CHUNK;
  // scratch from the runtime's pool, released behind the launches (the pool's reuse is stream-ordered)
  const size_t sz_coef = (size_t)g.nblocks * 128, sz_len = (size_t)g.nblocks * 4, sz_part = (size_t)nwg * 8;
  const size_t sz_words = (size_t)(max_bits / 32 + 2) * 4, sz_cnt = (size_t)max_chunks * 4 + 4;
  const size_t sz_small = sizeof(tables_t) + sizeof(state_t) + 4 * JH_NSYM * 4;
  const dev_buf_t m_coef = dev_buf_t::alloc(devid, sz_coef);
  const dev_buf_t m_len = dev_buf_t::alloc(devid, sz_len);
  const dev_buf_t m_part = dev_buf_t::alloc(devid, sz_part);
  const dev_buf_t m_words = dev_buf_t::alloc(devid, sz_words);
  const dev_buf_t m_cnt = dev_buf_t::alloc(devid, sz_cnt);
  const dev_buf_t m_small = dev_buf_t::alloc(devid, sz_small);
  const dev_buf_t m_fixed = dev_buf_t::alloc(devid, fixed.size());
  if(!m_coef || !m_len || !m_part || !m_words || !m_cnt || !m_small || !m_fixed) return DT_HIP_DEFAULT_ERROR;
  tables_t *tab = m_small.as<tables_t>();
  state_t *st = (state_t *)(m_small.as<uint8_t>() + sizeof(tables_t));
  uint32_t *freq = (uint32_t *)(m_small.as<uint8_t>() + sizeof(tables_t) + sizeof(state_t));
  hipStream_t s = stream_of(devid);
  const int err = upload_small(devid, m_fixed.ptr(), fixed.data(), fixed.size());
  if(err != DT_HIP_SUCCESS) return err;
  {
    launch_scope ls(devid, "jpeg_fdct");
    jpeg_fdct<<<nwg, JPEG_THREADS, 0, s>>>((const uint32_t *)dev_in_rgba8, g, q, m_coef.as<int16_t>());
  }
  if(d->optimize_coding)
  {
    launch_scope ls(devid, "jpeg_stats");
    (void)hipMemsetAsync(freq, 0, 4 * JH_NSYM * 4, s);
    jpeg_stats<<<nwg, JPEG_THREADS, 0, s>>>(m_coef.as<const int16_t>(), g, freq);
  }
  {
    launch_scope ls(devid, "jpeg_tables");
    jpeg_tables<<<4, 64, 0, s>>>(freq, d->optimize_coding ? 1 : 0, tab);
  }
  {
    launch_scope ls(devid, "jpeg_lengths");
    jpeg_lengths<<<nwg, JPEG_THREADS, 0, s>>>(m_coef.as<const int16_t>(), g, tab, m_len.as<uint32_t>(), m_part.as<uint64_t>());
    jpeg_scan_partials<<<1, JPEG_THREADS, 0, s>>>(m_part.as<uint64_t>(), nwg, st);
  }
  {
    launch_scope ls(devid, "jpeg_emit");
    jpeg_zero<<<stream_grid(max_bits / 32 + 1, JPEG_THREADS), JPEG_THREADS, 0, s>>>(m_words.as<uint32_t>(), st);
    jpeg_emit<<<nwg, JPEG_THREADS, 0, s>>>(m_coef.as<const int16_t>(), g, tab, m_len.as<const uint32_t>(),
                                           m_part.as<const uint64_t>(), m_words.as<uint32_t>());
  }
  {
    launch_scope ls(devid, "jpeg_stuff");
    const unsigned cg = (unsigned)std::min<uint64_t>(max_chunks, 2048);
    jpeg_ff_count<<<cg, JPEG_THREADS, 0, s>>>(m_words.as<const uint32_t>(), st, m_cnt.as<uint32_t>());
    jpeg_ff_scan<<<1, JPEG_THREADS, 0, s>>>(m_cnt.as<uint32_t>(), st, tab, (uint32_t)fixed.size(), d->capacity,
                                             (uint8_t *)dev_out);
    jpeg_compact<<<cg, JPEG_THREADS, 0, s>>>(m_words.as<const uint32_t>(), st, m_cnt.as<const uint32_t>(), (uint8_t *)dev_out);
    jpeg_headers<<<1, JPEG_THREADS, 0, s>>>(m_fixed.as<const uint8_t>(), (uint32_t)fixed.size(), tab, st,
                                             (uint8_t *)dev_out);
  }
  return check_launch("export_jpeg");
}
