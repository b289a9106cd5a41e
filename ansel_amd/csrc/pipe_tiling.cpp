// pipe_tiling.cpp -- a host frame through one module tile by tile: default_process_tiling_cl(), src/develop/tiling.c:842-1390.
// The tile plans are pure functions of the frame, the module's requirements and the device's limits.
#include "pipe_internal.h"

#include <algorithm>

using namespace ansel;

namespace
{
unsigned gcd(unsigned a, unsigned b)
{
  while(b)
  {
    const unsigned t = b;
    b = a % b;
    a = t;
  }
  return a;
}
unsigned lcm(unsigned a, unsigned b) { return (a && b) ? a / gcd(a, b) * b : 0u; }

// One tile through the device: upload the tile of the host input that `host_in` points at, run the module with the tile's
// ROIs (n.piece), download the good rectangle (gx, gy, gw, gh) of the output tile to `host_out`.  The stream is idle on return
int run_tile(int devid, const node_t &n, const char *host_in, size_t ipitch, int in_bpp, char *host_out, size_t opitch, int out_bpp,
             int gx, int gy, int gw, int gh, bool zero_output, int tx, int ty)
{
  const dt_hip_roi_t &ri = n.piece.roi_in, &ro = n.piece.roi_out;
  hipStream_t st = stream_of(devid);
  dev_buf_t input(dt_hip_alloc_device(devid, ri.width, ri.height, in_bpp), true);
  dev_buf_t output(dt_hip_alloc_device(devid, ro.width, ro.height, out_bpp), true);
  if(!input || !output) return DT_HIP_SYSMEM_ALLOCATION;
  int err = dt_hip_write_host_to_device_rowpitch(devid, host_in, input.ptr(), ri.width, ri.height, in_bpp, ipitch, 1);
  if(err == DT_HIP_SUCCESS && zero_output && hipMemsetAsync(output.ptr(), 0, (size_t)ro.width * ro.height * out_bpp, st) != hipSuccess)
    err = DT_HIP_DEFAULT_ERROR;
  if(err == DT_HIP_SUCCESS) err = run_single(devid, n, input.ptr(), output.ptr());
  if(err != DT_HIP_SUCCESS) return err;
  const char *src = (const char *)output.ptr() + ((size_t)gy * ro.width + gx) * out_bpp;
  if(hipMemcpy2DAsync(host_out, opitch, src, (size_t)ro.width * out_bpp, (size_t)gw * out_bpp, gh, hipMemcpyDeviceToHost, st) != hipSuccess
     || hipStreamSynchronize(st) != hipSuccess)
  {
    set_last_error("tiling: download of tile (%d, %d) failed: %s", tx, ty, hipGetErrorString(hipGetLastError()));
    return DT_HIP_DEFAULT_ERROR;
  }
  input.release(); // in this order: the pool hands out what came back last first
  output.release();
  return DT_HIP_SUCCESS;
}
} // namespace

extern "C" {

// ---- default_process_tiling_cl() for roi_in == roi_out, src/develop/tiling.c:842-1067 ----------------------------
// the tile plan of _default_process_tiling_cl_ptp(), :868-979, as a pure function of the frame, the module's
// requirements and the device's limits
int dt_hip_plan_tiles_ptp(int roi_width, int roi_height, int in_bpp, int out_bpp, const dt_hip_tiling_t *tiling,
                          unsigned filters, size_t available_bytes, size_t memalloc_bytes, int max_width, int max_height,
                          dt_hip_tile_plan_t *plan)
{
  if(!tiling || !plan || roi_width <= 0 || roi_height <= 0 || in_bpp <= 0 || out_bpp <= 0) return DT_HIP_INVALID_ARG;
  const int max_bpp = in_bpp > out_bpp ? in_bpp : out_bpp;
  const float available = (float)available_bytes;
  const float factor = fmaxf(tiling->factor_cl, 1.0f);
  const float singlebuffer = fminf(fmaxf((available - tiling->overhead) / factor, 0.0f), (float)memalloc_bytes);
  const float maxbuf = fmaxf(tiling->maxbuf_cl, 1.0f);
  int width = roi_width < max_width ? roi_width : max_width;
  int height = roi_height < max_height ? roi_height : max_height;
  // shrink the tile when it exceeds the per-buffer budget, :879-899
  if((float)width * height * max_bpp * maxbuf > singlebuffer)
  {
    const float scale = singlebuffer / ((float)width * height * max_bpp * maxbuf);
    if(width < height && scale >= 0.333f)
      height = (int)floorf(height * scale);
    else if(height <= width && scale >= 0.333f)
      width = (int)floorf(width * scale);
    else
    {
      width = (int)floorf(width * sqrtf(scale));
      height = (int)floorf(height * sqrtf(scale));
    }
  }
  // squares when the overlap would eat the tile, :901-907
  if(3 * tiling->overlap > (unsigned)width || 3 * tiling->overlap > (unsigned)height)
    width = height = (int)floorf(sqrtf((float)width * height));
  // alignment, :917-933 (CL_ALIGNMENT, :54: 4 unless X-Trans)
  const unsigned xyalign = lcm(tiling->xalign, tiling->yalign);
  const unsigned walign = lcm(xyalign, filters != 9u ? 4u : 1u);
  const unsigned halign = xyalign;
  if(!xyalign || !walign) return DT_HIP_INVALID_ARG;
  if(width < roi_width) width = (width / walign) * walign;
  if(height < roi_height) height = (height / halign) * halign;
  // the rounded-footprint loop, :941-950 (linear allocations are not rounded: dt_hip_dev_roundup_* are identities)
  while((float)width * height * max_bpp * maxbuf > singlebuffer)
  {
    if(width <= (int)walign && height <= (int)halign) break;
    if(width < height && height > (int)halign)
      height -= halign;
    else if(width > (int)walign)
      width -= walign;
    else
      height -= halign;
  }
  // :961-962
  auto align_down = [](int n, int a) { return n - n % a; };
  if(width < roi_width) width = std::max((int)walign, align_down(width, (int)walign));
  if(height < roi_height) height = std::max((int)halign, align_down(height, (int)halign));
  const int overlap = tiling->overlap % xyalign != 0 ? (tiling->overlap / xyalign + 1) * xyalign : tiling->overlap;
  plan->width = width;
  plan->height = height;
  plan->overlap = overlap;
  plan->tile_wd = width - 2 * overlap > 0 ? width - 2 * overlap : 1;
  plan->tile_ht = height - 2 * overlap > 0 ? height - 2 * overlap : 1;
  plan->tiles_x = width < roi_width ? (int)ceilf(roi_width / (float)plan->tile_wd) : 1;
  plan->tiles_y = height < roi_height ? (int)ceilf(roi_height / (float)plan->tile_ht) : 1;
  if((long)plan->tiles_x * plan->tiles_y > 10000) // _maximum_number_tiles(), :110-113
  {
    set_last_error("tiling: %d x %d tiles is too many", plan->tiles_x, plan->tiles_y);
    return DT_HIP_DEFAULT_ERROR;
  }
  return DT_HIP_SUCCESS;
}

// the tile loop, :981-1054: upload a tile of the host input, run the module on it with the tile's ROIs, download the
// part of its output that is not overlap.  available_bytes = 0 asks the device.
int dt_hip_default_process_tiling_ptp(int devid, const char *op, const dt_hip_piece_t *piece, const void *data,
                                      size_t data_size, const dt_hip_tiling_t *tiling, const void *host_in, void *host_out,
                                      int in_bpp, int out_bpp, size_t available_bytes)
{
  if(!valid_device(devid) || !op || !piece || !tiling || !host_in || !host_out) return DT_HIP_INVALID_ARG;
  node_t n;
  const int made = make_node(n, "tiling", op, piece, data, data_size);
  if(made == DT_HIP_SUCCESS && n.op == OP_FLIP)
  {
    // a mirrored tile lands elsewhere in the output: flip is tiled by dt_hip_default_process_tiling_roi()
    set_last_error("tiling: 'flip' moves pixels between tiles; use dt_hip_default_process_tiling_roi()");
    return DT_HIP_INVALID_ARG;
  }
  if(made != DT_HIP_SUCCESS || (k_ops[n.op].flags & OPF_NO_PTP))
  {
    set_last_error("tiling: module '%s' cannot be tiled here", op);
    return DT_HIP_INVALID_ARG;
  }
  const dt_hip_roi_t &ri = piece->roi_in, &ro = piece->roi_out;
  if(ri.x != ro.x || ri.y != ro.y || ri.width != ro.width || ri.height != ro.height || ri.scale != ro.scale)
  {
    set_last_error("tiling: '%s' changes the geometry (roi_in != roi_out): only the point-to-point plan is implemented", op);
    return DT_HIP_INVALID_ARG;
  }
  int max_w = 0, max_h = 0;
  dt_hip_get_device_max_image_size(devid, &max_w, &max_h);
  dt_hip_tile_plan_t pl;
  int err = dt_hip_plan_tiles_ptp(ri.width, ri.height, in_bpp, out_bpp, tiling, piece->filters,
                                  available_bytes ? available_bytes : dt_hip_get_device_available(devid),
                                  dt_hip_get_device_memalloc(devid), max_w, max_h, &pl);
  if(err != DT_HIP_SUCCESS) return err;
  const size_t ipitch = (size_t)ri.width * in_bpp, opitch = (size_t)ro.width * out_bpp;
  for(int tx = 0; tx < pl.tiles_x; tx++)
    for(int ty = 0; ty < pl.tiles_y; ty++)
    {
      const int wd = tx * pl.tile_wd + pl.width > ri.width ? ri.width - tx * pl.tile_wd : pl.width;
      const int ht = ty * pl.tile_ht + pl.height > ri.height ? ri.height - ty * pl.tile_ht : pl.height;
      // end tiles that are all overlap carry nothing new, :990-991
      if((wd <= 2 * pl.overlap && tx > 0) || (ht <= 2 * pl.overlap && ty > 0)) continue;
      n.piece = *piece;
      n.piece.roi_in.x = ri.x + tx * pl.tile_wd;
      n.piece.roi_in.y = ri.y + ty * pl.tile_ht;
      n.piece.roi_in.width = n.piece.roi_out.width = wd;
      n.piece.roi_in.height = n.piece.roi_out.height = ht;
      n.piece.roi_out.x = ro.x + tx * pl.tile_wd;
      n.piece.roi_out.y = ro.y + ty * pl.tile_ht;
      // only the good part goes back, :1023-1040: not the overlap a tile shares with the one to its left / above it
      const int ox = tx > 0 ? pl.overlap : 0, oy = ty > 0 ? pl.overlap : 0;
      const size_t ioffs = (size_t)ty * pl.tile_ht * ipitch + (size_t)tx * pl.tile_wd * in_bpp;
      const size_t ooffs = ((size_t)ty * pl.tile_ht + oy) * opitch + ((size_t)tx * pl.tile_wd + ox) * out_bpp;
      // a module may leave part of its output to the caller (the alpha of the demosaic border ring): the tile buffer
      // comes from the pool, so give those bytes a value
      err = run_tile(devid, n, (const char *)host_in + ioffs, ipitch, in_bpp, (char *)host_out + ooffs, opitch, out_bpp, ox, oy,
                     wd - ox, ht - oy, true, tx, ty);
      if(err != DT_HIP_SUCCESS) return err;
    }
  return DT_HIP_SUCCESS;
}

// ---- default_process_tiling_cl() for roi_in != roi_out, src/develop/tiling.c:1076-1390 (_default_process_tiling_cl_roi)
// Two modules of the export path change the geometry: finalscale, whose modify_roi_in() (src/iop/finalscale.c:76-107,
// the full-resolution pipeline of an export) is restated here, and flip (flip.hip, dt_hip_tile_rois_flip()).
namespace
{
static int ra_align_up(const int n, const int a) { return n + a - (n % a); } // tiling.c:92-95: one more step even when aligned
static int ra_align_down(const int n, const int a) { return n - (n % a); }
static int ra_align_close(const int n, const int a)
{
  const int off = n % a;
  const int shift = (off > a / 2) ? a - off : -off;
  return n + shift;
}

// finalscale modify_roi_in(), finalscale.c:76-107
static void finalscale_modify_roi_in(const dt_hip_roi_t *roi_out, dt_hip_roi_t *roi_in)
{
  *roi_in = *roi_out;
  if(roi_in->scale > 1.f)
  {
    roi_in->x = (int)roundf((float)roi_in->x / roi_out->scale);
    roi_in->y = (int)roundf((float)roi_in->y / roi_out->scale);
    roi_in->width = (int)roundf(roi_out->width / roi_out->scale);
    roi_in->height = (int)roundf(roi_out->height / roi_out->scale);
    roi_in->scale = 1.0f;
  }
  else
  {
    roi_in->width = (int)roundf(roi_out->width / roi_out->scale);
    roi_in->height = (int)roundf(roi_out->height / roi_out->scale);
    roi_in->scale = 1.0f;
    const float resample_scale = roi_out->scale / roi_in->scale;
    roi_in->x = (int)roundf(roi_in->x / resample_scale);
    roi_in->y = (int)roundf(roi_in->y / resample_scale);
  }
}

// _fit_output_to_input_roi(), tiling.c:197-237, its iterative search.  The Nelder-Mead fallback (:170-190) is for
// modules that distort; finalscale's search converges in one or two steps, so its failure is reported, not papered over
static bool fit_output_to_input_roi(const dt_hip_roi_t *iroi, dt_hip_roi_t *oroi, const int delta, int iter)
{
  dt_hip_roi_t probe = *iroi;
  finalscale_modify_roi_in(oroi, &probe);
  while((abs(probe.x - iroi->x) > delta || abs(probe.y - iroi->y) > delta || abs(probe.width - iroi->width) > delta
         || abs(probe.height - iroi->height) > delta)
        && iter > 0)
  {
    oroi->x += (iroi->x - probe.x) * oroi->scale / iroi->scale;
    oroi->y += (iroi->y - probe.y) * oroi->scale / iroi->scale;
    oroi->width += (iroi->width - probe.width) * oroi->scale / iroi->scale;
    oroi->height += (iroi->height - probe.height) * oroi->scale / iroi->scale;
    finalscale_modify_roi_in(oroi, &probe);
    iter--;
  }
  return iter > 0;
}
} // namespace

// the tile grid of :1100-1220 as a pure function of the two regions, the module's requirements and the device's limits
int dt_hip_plan_tiles_roi(const dt_hip_roi_t *roi_in, const dt_hip_roi_t *roi_out, int in_bpp, int out_bpp,
                          const dt_hip_tiling_t *tiling, unsigned filters, size_t available_bytes, size_t memalloc_bytes,
                          int max_width, int max_height, dt_hip_tile_plan_roi_t *plan)
{
  if(!roi_in || !roi_out || !tiling || !plan || roi_in->width <= 0 || roi_in->height <= 0 || roi_out->width <= 0
     || roi_out->height <= 0 || in_bpp <= 0 || out_bpp <= 0)
    return DT_HIP_INVALID_ARG;
  const int max_bpp = std::max(in_bpp, out_bpp);
  const float fullscale = fmaxf((float)(roi_in->scale / roi_out->scale),
                                sqrtf(((float)roi_in->width * roi_in->height) / ((float)roi_out->width * roi_out->height)));
  const int delta = (int)ceilf(fullscale);
  const int inacc = 5 * delta; // RESERVE, :59
  const float available = (float)available_bytes;
  const float factor = fmaxf(tiling->factor_cl, 1.0f);
  const float singlebuffer = fminf(fmaxf((available - tiling->overhead) / factor, 0.0f), (float)memalloc_bytes);
  const float maxbuf = fmaxf(tiling->maxbuf_cl, 1.0f);
  int width = std::min(std::max(roi_in->width, roi_out->width), max_width);
  int height = std::min(std::max(roi_in->height, roi_out->height), max_height);
  unsigned xyalign = lcm(tiling->xalign, tiling->yalign);
  xyalign = lcm(xyalign, filters != 9u ? 4u : 1u); // CL_ALIGNMENT, :54
  if(!xyalign) return DT_HIP_INVALID_ARG;
  const int al = (int)xyalign;
  if((float)width * height * max_bpp * maxbuf > singlebuffer)
  {
    const float scale = singlebuffer / ((float)width * height * max_bpp * maxbuf);
    if(width < height && scale >= 0.333f)
      height = ra_align_down((int)floorf(height * scale), al);
    else if(height <= width && scale >= 0.333f)
      width = ra_align_down((int)floorf(width * scale), al);
    else
    {
      width = ra_align_down((int)floorf(width * sqrtf(scale)), al);
      height = ra_align_down((int)floorf(height * sqrtf(scale)), al);
    }
  }
  if(3 * tiling->overlap > (unsigned)width || 3 * tiling->overlap > (unsigned)height)
    width = height = ra_align_down((int)floorf(sqrtf((float)width * height)), al);
  const int overlap_in = ra_align_up((int)tiling->overlap, al);
  const int overlap_out = (int)ceilf((float)overlap_in / fullscale);
  // the rounded-footprint loop, :1170-1179 (linear allocations are not rounded: dt_hip_dev_roundup_* are identities)
  while((float)width * height * max_bpp * maxbuf > singlebuffer)
  {
    if(width <= al && height <= al) break;
    if(width < height && height > al)
      height -= al;
    else if(width > al)
      width -= al;
    else
      height -= al;
  }
  if(width < std::max(roi_in->width, roi_out->width)) width = std::max(al, ra_align_down(width, al));
  if(height < std::max(roi_in->height, roi_out->height)) height = std::max(al, ra_align_down(height, al));
  int tiles_x = 1, tiles_y = 1;
  if(roi_in->width > roi_out->width)
    tiles_x = width < roi_in->width ? (int)ceilf((float)roi_in->width / (float)std::max(width - 2 * overlap_in - inacc, 1)) : 1;
  else
    tiles_x = width < roi_out->width ? (int)ceilf((float)roi_out->width / (float)std::max(width - 2 * overlap_out, 1)) : 1;
  if(roi_in->height > roi_out->height)
    tiles_y = height < roi_in->height ? (int)ceilf((float)roi_in->height / (float)std::max(height - 2 * overlap_in - inacc, 1)) : 1;
  else
    tiles_y = height < roi_out->height ? (int)ceilf((float)roi_out->height / (float)std::max(height - 2 * overlap_out, 1)) : 1;
  if((long)tiles_x * tiles_y > 10000)
  {
    set_last_error("tiling: %d x %d tiles is too many", tiles_x, tiles_y);
    return DT_HIP_DEFAULT_ERROR;
  }
  plan->width = width;
  plan->height = height;
  plan->tiles_x = tiles_x;
  plan->tiles_y = tiles_y;
  plan->tile_wd = ra_align_up(roi_out->width % tiles_x == 0 ? roi_out->width / tiles_x : roi_out->width / tiles_x + 1, al);
  plan->tile_ht = ra_align_up(roi_out->height % tiles_y == 0 ? roi_out->height / tiles_y : roi_out->height / tiles_y + 1, al);
  plan->overlap_in = overlap_in;
  plan->overlap_out = overlap_out;
  plan->delta = delta;
  plan->xyalign = al;
  return DT_HIP_SUCCESS;
}

// the three regions of tile (tx, ty), :1228-1300: the good part of the output, the input it is computed from (with
// overlap, alignment and `delta` of slack) and the output region that input produces
int dt_hip_tile_rois_finalscale(const dt_hip_tile_plan_roi_t *pl, const dt_hip_roi_t *roi_in, const dt_hip_roi_t *roi_out, int tx,
                                int ty, dt_hip_roi_t *iroi_full_out, dt_hip_roi_t *oroi_full_out, dt_hip_roi_t *oroi_good_out)
{
  if(!pl || !roi_in || !roi_out || tx < 0 || ty < 0 || tx >= pl->tiles_x || ty >= pl->tiles_y) return DT_HIP_INVALID_ARG;
  const int tile_wd = pl->tile_wd, tile_ht = pl->tile_ht, al = pl->xyalign, delta = pl->delta, overlap_in = pl->overlap_in;
  const int wd = (tx + 1) * tile_wd > roi_out->width ? roi_out->width - tx * tile_wd : tile_wd;
  const int ht = (ty + 1) * tile_ht > roi_out->height ? roi_out->height - ty * tile_ht : tile_ht;
  if(wd <= 0 || ht <= 0) return DT_HIP_TILE_EMPTY; // align_up() of the tile step can leave nothing for the last tile
  dt_hip_roi_t iroi_good = { roi_in->x + tx * tile_wd, roi_in->y + ty * tile_ht, wd, ht, roi_in->scale };
  dt_hip_roi_t oroi_good = { roi_out->x + tx * tile_wd, roi_out->y + ty * tile_ht, wd, ht, roi_out->scale };
  finalscale_modify_roi_in(&oroi_good, &iroi_good);
  iroi_good.x = std::max(iroi_good.x, roi_in->x);
  iroi_good.y = std::max(iroi_good.y, roi_in->y);
  iroi_good.width = std::min(iroi_good.width, roi_in->width + roi_in->x - iroi_good.x);
  iroi_good.height = std::min(iroi_good.height, roi_in->height + roi_in->y - iroi_good.y);
  const int x_in = iroi_good.x, y_in = iroi_good.y, width_in = iroi_good.width, height_in = iroi_good.height;
  const int new_x_in = std::max(ra_align_close(x_in - overlap_in - delta, al), roi_in->x);
  const int new_y_in = std::max(ra_align_close(y_in - overlap_in - delta, al), roi_in->y);
  const int new_width_in = std::min(ra_align_up(width_in + overlap_in + delta + (x_in - new_x_in), al), roi_in->width + roi_in->x - new_x_in);
  const int new_height_in = std::min(ra_align_up(height_in + overlap_in + delta + (y_in - new_y_in), al), roi_in->height + roi_in->y - new_y_in);
  dt_hip_roi_t iroi_full = { new_x_in, new_y_in, new_width_in, new_height_in, iroi_good.scale };
  dt_hip_roi_t oroi_full = oroi_good;
  if(!fit_output_to_input_roi(&iroi_full, &oroi_full, delta, 10))
  {
    set_last_error("tiling: no output region matches the input of tile (%d, %d)", tx, ty);
    return DT_HIP_DEFAULT_ERROR;
  }
  oroi_full.x = std::min(oroi_full.x, oroi_good.x);
  oroi_full.y = std::min(oroi_full.y, oroi_good.y);
  oroi_full.width = std::max(oroi_full.width, oroi_good.x + oroi_good.width - oroi_full.x);
  oroi_full.height = std::max(oroi_full.height, oroi_good.y + oroi_good.height - oroi_full.y);
  oroi_full.x = std::max(oroi_full.x, roi_out->x);
  oroi_full.y = std::max(oroi_full.y, roi_out->y);
  oroi_full.width = std::min(oroi_full.width, roi_out->width + roi_out->x - oroi_full.x);
  oroi_full.height = std::min(oroi_full.height, roi_out->height + roi_out->y - oroi_full.y);
  finalscale_modify_roi_in(&oroi_full, &iroi_full);
  iroi_full.x = std::max(iroi_full.x, roi_in->x);
  iroi_full.y = std::max(iroi_full.y, roi_in->y);
  iroi_full.width = std::min(iroi_full.width, roi_in->width + roi_in->x - iroi_full.x);
  iroi_full.height = std::min(iroi_full.height, roi_in->height + roi_in->y - iroi_full.y);
  if(iroi_full_out) *iroi_full_out = iroi_full;
  if(oroi_full_out) *oroi_full_out = oroi_full;
  if(oroi_good_out) *oroi_good_out = oroi_good;
  return DT_HIP_SUCCESS;
}

// the loop of :1222-1370: host frame -> every tile's full input region through the device -> the good part of its
// output back into the host frame.  `op` is "finalscale" or "flip": the modules with a tile-region function
int dt_hip_default_process_tiling_roi(int devid, const char *op, const dt_hip_piece_t *piece, const void *data, size_t data_size,
                                      const dt_hip_tiling_t *tiling, const void *host_in, void *host_out, int in_bpp,
                                      int out_bpp, size_t available_bytes)
{
  if(!valid_device(devid) || !op || !piece || !tiling || !host_in || !host_out) return DT_HIP_INVALID_ARG;
  if(strcmp(op, "finalscale") && strcmp(op, "flip"))
  {
    set_last_error("tiling (roi_in != roi_out): '%s' has no modify_roi_in() here; finalscale and flip are the modules of the "
                   "path that change the geometry", op);
    return DT_HIP_INVALID_ARG;
  }
  node_t n;
  if(make_node(n, "tiling (roi_in != roi_out)", op, piece, data, data_size) != DT_HIP_SUCCESS) return DT_HIP_INVALID_ARG;
  const dt_hip_roi_t &ri = piece->roi_in, &ro = piece->roi_out;
  int max_w = 0, max_h = 0;
  dt_hip_get_device_max_image_size(devid, &max_w, &max_h);
  dt_hip_tile_plan_roi_t pl;
  int err = dt_hip_plan_tiles_roi(&ri, &ro, in_bpp, out_bpp, tiling, piece->filters,
                                  available_bytes ? available_bytes : dt_hip_get_device_available(devid),
                                  dt_hip_get_device_memalloc(devid), max_w, max_h, &pl);
  if(err != DT_HIP_SUCCESS) return err;
  const size_t ipitch = (size_t)ri.width * in_bpp, opitch = (size_t)ro.width * out_bpp;
  for(int tx = 0; tx < pl.tiles_x; tx++)
    for(int ty = 0; ty < pl.tiles_y; ty++)
    {
      dt_hip_roi_t iroi_full, oroi_full, oroi_good;
      err = n.op == OP_FLIP
              ? dt_hip_tile_rois_flip(&pl, &ri, &ro, n.as<dt_hip_flip_data_t>(), tx, ty, &iroi_full, &oroi_full, &oroi_good)
              : dt_hip_tile_rois_finalscale(&pl, &ri, &ro, tx, ty, &iroi_full, &oroi_full, &oroi_good);
      if(err == DT_HIP_TILE_EMPTY) continue;
      if(err != DT_HIP_SUCCESS) return err;
      const size_t ioffs = (size_t)(iroi_full.y - ri.y) * ipitch + (size_t)(iroi_full.x - ri.x) * in_bpp;
      const size_t ooffs = (size_t)(oroi_good.y - ro.y) * opitch + (size_t)(oroi_good.x - ro.x) * out_bpp;
      n.piece = *piece;
      n.piece.roi_in = iroi_full;
      n.piece.roi_out = oroi_full;
      err = run_tile(devid, n, (const char *)host_in + ioffs, ipitch, in_bpp, (char *)host_out + ooffs, opitch, out_bpp,
                     oroi_good.x - oroi_full.x, oroi_good.y - oroi_full.y, oroi_good.width, oroi_good.height, false, tx, ty);
      if(err != DT_HIP_SUCCESS) return err;
    }
  return DT_HIP_SUCCESS;
}

// default_tiling_callback(), src/develop/tiling.c:1423-1463, for the modules without a callback of their own
// (rawprepare, temperature, highlights, exposure, colorin, channelmixerrgb, filmicrgb, colorout, finalscale)
void dt_hip_default_tiling(const dt_hip_piece_t *piece, int before_demosaic, dt_hip_tiling_t *tiling)
{
  const float ioratio = ((float)piece->roi_out.width * (float)piece->roi_out.height)
                        / ((float)piece->roi_in.width * (float)piece->roi_in.height);
  tiling->factor = tiling->factor_cl = 1.0f + ioratio;
  tiling->maxbuf = tiling->maxbuf_cl = 1.0f;
  tiling->overhead = 0;
  tiling->overlap = 0;
  tiling->xalign = tiling->yalign = 1;
  if(before_demosaic && piece->filters) tiling->xalign = tiling->yalign = piece->filters == 9u ? 3 : 2;
}

} // extern "C"
