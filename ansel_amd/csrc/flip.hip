// flip.hip -- orientation (the flip module) on gfx950.
//
// Reference: process() / process_cl() of src/iop/flip.c, whose pixel loop is dt_imageio_flip_buffers()
// (src/common/imageio.c).  The module permutes whole pixels; nothing is computed, so every output word is an input
// word (NaN payloads included).
//
// Orientation = the three bits of dt_image_orientation_t: FLIP_Y = 1, FLIP_X = 2, SWAP_XY = 4.  For an input of
// W x H pixels, input pixel (row j, column i) goes to
//
//   j' = FLIP_Y ? H-1-j : j,   i' = FLIP_X ? W-1-i : i,   out(row, col) = SWAP_XY ? (i', j') : (j', i')
//
// so the output is H x W pixels (width H) when SWAP_XY is set and W x H otherwise.  In numpy, with x[j, i]:
// y = x; FLIP_Y: y = y[::-1]; FLIP_X: y = y[:, ::-1]; SWAP_XY: y = y.T -- the table of the eight values is in
// include/ansel_hip.h and DESIGN.md section 2.
//
// Two kernels, both out of place:
//  * flip_copy   (SWAP_XY clear): one thread per output pixel reads the input pixel of the mirrored indices.  A wave
//    reads and writes 64 consecutive pixels (a mirrored row is read backwards: the same cache lines), so both sides
//    are coalesced 16-byte accesses.
//  * flip_swap   (SWAP_XY set): a 32 x 32-pixel tile goes through LDS.  Reads run along input rows, writes along output
//    rows, each a 512-byte run of float4 per 32 lanes.  The tile's rows are padded by one element: the transposed
//    read takes one tile row per lane, and with a pitch of 33 x 16 B lane r of a ds_read_b128 lane group lands on
//    16-byte slot (r + c) mod 16 of the 256-byte bank row; the lanes of each group {0-3,12-15,20-27},
//    {4-11,16-19,28-31} (and the same + 32) have distinct r mod 16, so the read is conflict-free.  The writes are rows
//    of the tile (8 contiguous lanes per ds_write_b128 group: 128 contiguous bytes), conflict-free with any pitch.
//    With 1-channel f32 (ds_*_b32, banks (a/4) mod 32) the pitch of 33 words puts lane r on bank (r + c) mod 32.
#include "hip_common.h"

#include <algorithm>

using namespace ansel;

namespace
{

constexpr int FLIP_Y = 1, FLIP_X = 2, SWAP_XY = 4;
constexpr int TILE = 32;         // tile edge, pixels
constexpr int TILE_THREADS = 256; // 8 tile rows per pass, 4 passes

template <typename T>
__global__ __launch_bounds__(256) void flip_copy(const T *__restrict__ in, T *__restrict__ out, const int w, const int h,
                                                 const int orientation)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= (size_t)w * h) return;
  const int r = (int)(k / (unsigned)w), c = (int)(k - (size_t)r * w); // output pixel = input geometry
  const int j = (orientation & FLIP_Y) ? h - 1 - r : r;
  const int i = (orientation & FLIP_X) ? w - 1 - c : c;
  out[k] = in[(size_t)j * w + i];
}

// grid: x over output column tiles (input rows), y over output row tiles (input columns); w, h: the INPUT size
template <typename T>
__global__ __launch_bounds__(TILE_THREADS) void flip_swap(const T *__restrict__ in, T *__restrict__ out, const int w,
                                                          const int h, const int orientation)
{
  __shared__ T tile[TILE][TILE + 1]; // tile[a][b]: output (R0 + b, C0 + a) = input (row j(C0 + a), column i(R0 + b))
  const int C0 = blockIdx.x * TILE, R0 = blockIdx.y * TILE;
  const int lane = threadIdx.x % TILE, row = threadIdx.x / TILE;
  // load: consecutive lanes take consecutive input columns (backwards under FLIP_X)
  const int b = lane, ro = R0 + b;
  if(ro < w)
  {
    const int i = (orientation & FLIP_X) ? w - 1 - ro : ro;
#pragma unroll
    for(int a = row; a < TILE; a += TILE_THREADS / TILE)
    {
      const int co = C0 + a;
      if(co < h)
      {
        const int j = (orientation & FLIP_Y) ? h - 1 - co : co;
        tile[a][b] = in[(size_t)j * w + i];
      }
    }
  }
  __syncthreads();
  // store: consecutive lanes take consecutive output columns; the output is w rows of h pixels
  const int a = lane, co = C0 + a;
  if(co < h)
  {
#pragma unroll
    for(int bb = row; bb < TILE; bb += TILE_THREADS / TILE)
    {
      const int r = R0 + bb;
      if(r < w) out[(size_t)r * h + co] = tile[a][bb];
    }
  }
}

template <typename T>
int flip_launch(int devid, const T *in, T *out, const int w, const int h, const int orientation)
{
  hipStream_t s = stream_of(devid);
  launch_scope ls(devid, "flip");
  if(orientation & SWAP_XY)
  {
    const dim3 grid((unsigned)((h + TILE - 1) / TILE), (unsigned)((w + TILE - 1) / TILE));
    flip_swap<T><<<grid, TILE_THREADS, 0, s>>>(in, out, w, h, orientation);
  }
  else
    flip_copy<T><<<pixel_grid((size_t)w * h), 256, 0, s>>>(in, out, w, h, orientation);
  return check_launch("flip");
}

bool valid_orientation(const dt_hip_flip_data_t *d, const char *who)
{
  if(!d) return false;
  if(d->orientation < 0 || d->orientation > 7)
  {
    set_last_error("%s: orientation %d is not one of 0..7 (resolve -1 to the image's orientation first)", who, (int)d->orientation);
    return false;
  }
  return true;
}

// the forward map of a region (frame-relative): input region -> output region of an iw x ih input
void roi_forward(const int o, const int iw, const int ih, const dt_hip_roi_t *in, dt_hip_roi_t *out)
{
  *out = *in;
  const int x = (o & FLIP_X) ? iw - in->x - in->width : in->x;
  const int y = (o & FLIP_Y) ? ih - in->y - in->height : in->y;
  if(o & SWAP_XY)
  {
    out->x = y;
    out->y = x;
    out->width = in->height;
    out->height = in->width;
  }
  else
  {
    out->x = x;
    out->y = y;
  }
}

// ... and its inverse
void roi_backward(const int o, const int iw, const int ih, const dt_hip_roi_t *out, dt_hip_roi_t *in)
{
  *in = *out;
  int x = out->x, y = out->y, wd = out->width, ht = out->height;
  if(o & SWAP_XY)
  {
    std::swap(x, y);
    std::swap(wd, ht);
  }
  in->width = wd;
  in->height = ht;
  in->x = (o & FLIP_X) ? iw - x - wd : x;
  in->y = (o & FLIP_Y) ? ih - y - ht : y;
}

} // namespace

extern "C" {

int dt_hip_iop_flip_process(int devid, const dt_hip_piece_t *piece, const dt_hip_flip_data_t *d, dt_hip_mem_t dev_in,
                            dt_hip_mem_t dev_out)
{
  if(!valid_device(devid) || !piece || !d || !dev_in || !dev_out) return DT_HIP_INVALID_ARG;
  if(!valid_orientation(d, "flip")) return DT_HIP_INVALID_ARG;
  if(piece->channels != 1 && piece->channels != 4)
  {
    set_last_error("flip: %u channels (1 or 4 floats per pixel)", piece->channels);
    return DT_HIP_INVALID_ARG;
  }
  const int o = d->orientation;
  const int w = piece->roi_in.width, h = piece->roi_in.height;
  const int ow = (o & SWAP_XY) ? h : w, oh = (o & SWAP_XY) ? w : h;
  if(piece->roi_out.width != ow || piece->roi_out.height != oh)
  {
    set_last_error("flip: orientation %d takes %d x %d to %d x %d, roi_out is %d x %d", o, w, h, ow, oh, piece->roi_out.width,
                   piece->roi_out.height);
    return DT_HIP_INVALID_ARG;
  }
  if(w <= 0 || h <= 0) return DT_HIP_SUCCESS;
  if(dev_in == dev_out)
  {
    set_last_error("flip: the permutation runs out of place (dev_in == dev_out)");
    return DT_HIP_INVALID_ARG;
  }
  if(piece->channels == 4) return flip_launch(devid, (const float4 *)dev_in, (float4 *)dev_out, w, h, o);
  return flip_launch(devid, (const float *)dev_in, (float *)dev_out, w, h, o);
}

int dt_hip_iop_flip_modify_roi_out(const dt_hip_flip_data_t *d, int iw, int ih, const dt_hip_roi_t *roi_in, dt_hip_roi_t *roi_out)
{
  if(!valid_orientation(d, "flip_modify_roi_out") || !roi_in || !roi_out || iw < 0 || ih < 0) return DT_HIP_INVALID_ARG;
  roi_forward(d->orientation, iw, ih, roi_in, roi_out);
  return DT_HIP_SUCCESS;
}

int dt_hip_iop_flip_modify_roi_in(const dt_hip_flip_data_t *d, int iw, int ih, const dt_hip_roi_t *roi_out, dt_hip_roi_t *roi_in)
{
  if(!valid_orientation(d, "flip_modify_roi_in") || !roi_in || !roi_out || iw < 0 || ih < 0) return DT_HIP_INVALID_ARG;
  roi_backward(d->orientation, iw, ih, roi_out, roi_in);
  return DT_HIP_SUCCESS;
}

// points: x, y pairs in pixel units with pixel (j, i) covering [i, i+1) x [j, j+1): x -> iw - x mirrors pixel centres
int dt_hip_iop_flip_distort_transform(const dt_hip_flip_data_t *d, int iw, int ih, float *points, size_t points_count)
{
  if(!valid_orientation(d, "flip_distort_transform") || (points_count && !points)) return DT_HIP_INVALID_ARG;
  const int o = d->orientation;
  for(size_t k = 0; k < 2 * points_count; k += 2)
  {
    const float x = (o & FLIP_X) ? (float)iw - points[k] : points[k];
    const float y = (o & FLIP_Y) ? (float)ih - points[k + 1] : points[k + 1];
    points[k] = (o & SWAP_XY) ? y : x;
    points[k + 1] = (o & SWAP_XY) ? x : y;
  }
  return DT_HIP_SUCCESS;
}

int dt_hip_iop_flip_distort_backtransform(const dt_hip_flip_data_t *d, int iw, int ih, float *points, size_t points_count)
{
  if(!valid_orientation(d, "flip_distort_backtransform") || (points_count && !points)) return DT_HIP_INVALID_ARG;
  const int o = d->orientation;
  for(size_t k = 0; k < 2 * points_count; k += 2)
  {
    const float x = (o & SWAP_XY) ? points[k + 1] : points[k];
    const float y = (o & SWAP_XY) ? points[k] : points[k + 1];
    points[k] = (o & FLIP_X) ? (float)iw - x : x;
    points[k + 1] = (o & FLIP_Y) ? (float)ih - y : y;
  }
  return DT_HIP_SUCCESS;
}

// one tile of dt_hip_plan_tiles_roi()'s grid: the good part of the output is the whole output tile (flip has no
// overlap and reads nothing around a pixel), the input is its preimage
int dt_hip_tile_rois_flip(const dt_hip_tile_plan_roi_t *pl, const dt_hip_roi_t *roi_in, const dt_hip_roi_t *roi_out,
                          const dt_hip_flip_data_t *d, int tx, int ty, dt_hip_roi_t *iroi_full, dt_hip_roi_t *oroi_full,
                          dt_hip_roi_t *oroi_good)
{
  if(!pl || !roi_in || !roi_out || tx < 0 || ty < 0 || tx >= pl->tiles_x || ty >= pl->tiles_y) return DT_HIP_INVALID_ARG;
  if(!valid_orientation(d, "dt_hip_tile_rois_flip")) return DT_HIP_INVALID_ARG;
  const int swap = d->orientation & SWAP_XY;
  if(roi_out->width != (swap ? roi_in->height : roi_in->width) || roi_out->height != (swap ? roi_in->width : roi_in->height))
  {
    set_last_error("dt_hip_tile_rois_flip: roi_out %d x %d is not roi_in %d x %d oriented by %d", roi_out->width, roi_out->height,
                   roi_in->width, roi_in->height, (int)d->orientation);
    return DT_HIP_INVALID_ARG;
  }
  const int x0 = tx * pl->tile_wd, y0 = ty * pl->tile_ht;
  const int wd = std::min(pl->tile_wd, roi_out->width - x0), ht = std::min(pl->tile_ht, roi_out->height - y0);
  if(wd <= 0 || ht <= 0) return DT_HIP_TILE_EMPTY;
  const dt_hip_roi_t og_rel = { x0, y0, wd, ht, roi_out->scale };
  dt_hip_roi_t ig_rel;
  roi_backward(d->orientation, roi_in->width, roi_in->height, &og_rel, &ig_rel);
  ig_rel.scale = roi_in->scale;
  dt_hip_roi_t og = og_rel, ig = ig_rel;
  og.x += roi_out->x;
  og.y += roi_out->y;
  ig.x += roi_in->x;
  ig.y += roi_in->y;
  if(iroi_full) *iroi_full = ig;
  if(oroi_full) *oroi_full = og;
  if(oroi_good) *oroi_good = og;
  return DT_HIP_SUCCESS;
}

} // extern "C"
