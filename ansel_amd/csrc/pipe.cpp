// pipe.cpp -- export-pipe executor on the dt_hip_* runtime: the device-resident part of
// dt_dev_pixelpipe_process_rec() (src/develop/pixelpipe_hb.c:881-1282) + pixelpipe_process_on_GPU()
// (src/develop/pixelpipe_gpu.c:191-744) for an export, where no module output is re-used.
//
// The reference walks the node list recursively from the last node, acquires a cacheline per module
// output and calls process_cl(); here the list is walked forward, outputs come from the runtime's
// pool and go back to it as soon as the consumer is enqueued (stream-ordered, so safe), and runs
// of pointwise modules are planned into fused launches (pipe_fused.hip).
//
// This file: the module table, the node list, its plan and the walk of a whole frame.  A stream of frames is
// pipe_batch.cpp, row bands are pipe_bands.cpp, host frames tile by tile are pipe_tiling.cpp.
#include "pipe_internal.h"

using namespace ansel;

namespace
{

// the table's launcher from a module's typed entry point: the row's data size and its launcher come from the one type
template <typename D> using process_fn = int (*)(int, const dt_hip_piece_t *, const D *, dt_hip_mem_t, dt_hip_mem_t);
template <typename D, process_fn<D> F> int run_module(int devid, const node_t &n, dt_hip_mem_t in, dt_hip_mem_t out)
{
  return F(devid, &n.piece, n.as<D>(), in, out);
}
template <typename D, int (*F)(const dt_hip_piece_t *, const D *)> int halo_of_module(const node_t &n) { return F(&n.piece, n.as<D>()); }
template <typename D, process_fn<D> F>
constexpr op_info_t module(op_t op, const char *name, int bpp_out, unsigned flags = 0, int (*halo_rows)(const node_t &) = nullptr)
{
  return { op, name, sizeof(D), bpp_out, nullptr, run_module<D, F>, flags, halo_rows };
}

// the nodes behind the pipe's last module: a frame in the file format's sample type ...
template <int (*F)(int, int, int, dt_hip_mem_t, dt_hip_mem_t)> int run_convert(int devid, const node_t &n, dt_hip_mem_t in, dt_hip_mem_t out)
{
  return F(devid, n.piece.roi_out.width, n.piece.roi_out.height, in, out);
}
int run_export_rows(int devid, const node_t &n, dt_hip_mem_t in, dt_hip_mem_t out)
{
  const dt_hip_export_rows_t *d = n.as<dt_hip_export_rows_t>();
  return dt_hip_export_pack_rows(devid, n.piece.roi_out.width, n.piece.roi_out.height, d->bpp, d->layers, in, out);
}
size_t export_rows_size(const node_t &n)
{
  const dt_hip_export_rows_t *d = n.as<dt_hip_export_rows_t>();
  return (size_t)n.piece.roi_out.width * n.piece.roi_out.height * (size_t)d->layers * (size_t)(d->bpp / 8);
}
// ... and the file itself: the encoder reads the ICC profile from the node's copy, not from the caller's pointer
template <typename D, int (*F)(int, int, int, const D *, dt_hip_mem_t, dt_hip_mem_t)>
int run_encoder(int devid, const node_t &n, dt_hip_mem_t in, dt_hip_mem_t out)
{
  D d = *n.as<D>();
  d.icc = n.icc.empty() ? nullptr : n.icc.data();
  d.icc_bytes = n.icc.size();
  return F(devid, n.piece.roi_out.width, n.piece.roi_out.height, &d, in, out);
}
template <typename D> size_t encoder_capacity(const node_t &n) { return (size_t)n.as<D>()->capacity; }
template <typename D> void keep_icc(node_t &n)
{
  const D *d = n.as<D>();
  if(d->icc && d->icc_bytes) n.icc.assign((const unsigned char *)d->icc, (const unsigned char *)d->icc + d->icc_bytes);
}
int run_nothing(int, const node_t &, dt_hip_mem_t, dt_hip_mem_t) { return DT_HIP_INVALID_ARG; }
// a file is not rows, and a flipped frame's rows are not its input's
int no_band_mode(const node_t &) { return -1; }
int flip_halo_rows(const node_t &n) { return n.as<dt_hip_flip_data_t>()->orientation == 0 ? 0 : -1; }

} // namespace

namespace ansel
{

// (host pass only: every translation unit is compiled as HIP, a constant table is emitted for the device as well, and these
// launchers have no device side)
#ifndef __HIP_DEVICE_COMPILE__
constexpr op_info_t k_ops[OP_UNKNOWN] = {
  module<dt_hip_rawprepare_data_t, dt_hip_iop_rawprepare_process>(OP_RAWPREPARE, "rawprepare", 4, OPF_CFA),
  module<dt_hip_temperature_data_t, dt_hip_iop_temperature_process>(OP_TEMPERATURE, "temperature", 0, OPF_CFA),
  module<dt_hip_highlights_data_t, dt_hip_iop_highlights_process>(OP_HIGHLIGHTS, "highlights", 0, OPF_CFA),
  module<dt_hip_demosaic_data_t, dt_hip_iop_demosaic_process>(OP_DEMOSAIC, "demosaic", 16),
  module<dt_hip_denoiseprofile_data_t, dt_hip_iop_denoiseprofile_process>(
    OP_DENOISEPROFILE, "denoiseprofile", 16, OPF_STENCIL, halo_of_module<dt_hip_denoiseprofile_data_t, denoiseprofile_halo_rows>),
  module<dt_hip_exposure_data_t, dt_hip_iop_exposure_process>(OP_EXPOSURE, "exposure", 0),
  module<dt_hip_conversion_t, dt_hip_iop_colorin_process>(OP_COLORIN, "colorin", 16),
  module<dt_hip_channelmixerrgb_data_t, dt_hip_iop_channelmixerrgb_process>(OP_CHANNELMIXERRGB, "channelmixerrgb", 16),
  module<dt_hip_filmicrgb_data_t, dt_hip_iop_filmicrgb_process>(OP_FILMICRGB, "filmicrgb", 16),
  module<dt_hip_conversion_t, dt_hip_iop_colorout_process>(OP_COLOROUT, "colorout", 16),
  module<dt_hip_diffuse_data_t, dt_hip_iop_diffuse_process>(OP_DIFFUSE, "diffuse", 16, OPF_STENCIL,
                                                            halo_of_module<dt_hip_diffuse_data_t, diffuse_halo_rows>),
  module<dt_hip_lab_data_t, dt_hip_transform_rgb_to_lab>(OP_RGB_TO_LAB, "rgb_to_lab", 16),
  module<dt_hip_nlmeans_data_t, dt_hip_iop_nlmeans_process>(OP_NLMEANS, "nlmeans", 16, OPF_STENCIL,
                                                            halo_of_module<dt_hip_nlmeans_data_t, nlmeans_halo_rows>),
  module<dt_hip_bilat_data_t, dt_hip_iop_bilat_process>(OP_BILAT, "bilat", 16),
  module<dt_hip_lab_data_t, dt_hip_transform_lab_to_rgb>(OP_LAB_TO_RGB, "lab_to_rgb", 16),
  module<dt_hip_finalscale_data_t, dt_hip_iop_finalscale_process>(OP_FINALSCALE, "finalscale", 16),
  module<dt_hip_finalscale_data_t, dt_hip_iop_initialscale_process>(OP_INITIALSCALE, "initialscale", 16),
  { OP_EXPORT_U16, "export_u16", 0, 8, nullptr, run_convert<dt_hip_export_convert_u16>, 0, nullptr },
  // in place in the output of the module in front of it (dt_hip_pipe_process()): no launch and no tile of its own
  { OP_BLEND, "blend", sizeof(dt_hip_blend_data_t), 16, nullptr, run_nothing, OPF_NO_PTP, nullptr },
  { OP_EXPORT_ROWS, "export_rows", sizeof(dt_hip_export_rows_t), 0, export_rows_size, run_export_rows, 0, nullptr },
  { OP_EXPORT_U8, "export_u8", 0, 4, nullptr, run_convert<dt_hip_export_convert_u8>, 0, nullptr },
  module<dt_hip_detailmask_data_t, dt_hip_iop_detailmask_process>(OP_DETAILMASK, "detailmask", 16),
  module<dt_hip_flip_data_t, dt_hip_iop_flip_process>(OP_FLIP, "flip", 0, OPF_NO_PTP, flip_halo_rows),
  { OP_EXPORT_JPEG, "export_jpeg", sizeof(dt_hip_jpeg_data_t), 0, encoder_capacity<dt_hip_jpeg_data_t>,
    run_encoder<dt_hip_jpeg_data_t, dt_hip_export_jpeg>, OPF_NO_PTP, no_band_mode },
  { OP_EXPORT_PNG, "export_png", sizeof(dt_hip_png_data_t), 0, encoder_capacity<dt_hip_png_data_t>,
    run_encoder<dt_hip_png_data_t, dt_hip_export_png>, OPF_NO_PTP, no_band_mode },
  { OP_EXPORT_TIFF, "export_tiff", sizeof(dt_hip_tiff_data_t), 0, encoder_capacity<dt_hip_tiff_data_t>,
    run_encoder<dt_hip_tiff_data_t, dt_hip_export_tiff>, OPF_NO_PTP, no_band_mode },
  { OP_EXPORT_WEBP, "export_webp", sizeof(dt_hip_webp_data_t), 0, encoder_capacity<dt_hip_webp_data_t>,
    run_encoder<dt_hip_webp_data_t, dt_hip_export_webp>, OPF_NO_PTP, no_band_mode },
};
constexpr bool table_follows_enum()
{
  for(int k = 0; k < (int)OP_UNKNOWN; k++)
    if(k_ops[k].op != (op_t)k || !k_ops[k].name || !k_ops[k].run) return false;
  return true;
}
static_assert(table_follows_enum(), "the module table needs one row per op_t, in the enum's order");
#endif

int make_node(node_t &n, const char *who, const char *name, const dt_hip_piece_t *piece, const void *data, size_t data_size)
{
  n.op = OP_UNKNOWN;
  for(int k = 0; k < (int)OP_UNKNOWN; k++)
    if(!strcmp(name, k_ops[k].name)) n.op = (op_t)k;
  if(n.op == OP_UNKNOWN)
  {
    set_last_error("%s: module '%s' has no device implementation", who, name);
    return DT_HIP_INVALID_ARG;
  }
  if(data_size != k_ops[n.op].data_size || (data_size && !data))
  {
    set_last_error("%s: '%s' expects %zu bytes of data, got %zu", who, name, k_ops[n.op].data_size, data_size);
    return DT_HIP_INVALID_ARG;
  }
  n.piece = *piece;
  if(data_size) n.data.assign((const unsigned char *)data, (const unsigned char *)data + data_size);
  if(n.op == OP_EXPORT_JPEG) keep_icc<dt_hip_jpeg_data_t>(n);
  if(n.op == OP_EXPORT_PNG) keep_icc<dt_hip_png_data_t>(n);
  if(n.op == OP_EXPORT_TIFF) keep_icc<dt_hip_tiff_data_t>(n);
  if(n.op == OP_EXPORT_WEBP) keep_icc<dt_hip_webp_data_t>(n);
  return DT_HIP_SUCCESS;
}

size_t out_bytes(const node_t &n)
{
  const op_info_t &o = k_ops[n.op];
  if(o.out_size) return o.out_size(n);
  return (size_t)n.piece.roi_out.width * n.piece.roi_out.height * (size_t)(o.bpp_out ? o.bpp_out : 4 * (int)n.piece.channels);
}

} // namespace ansel

// The launch groups of the node list, and the checks that depend on the node list alone.
//
// Which groups a "blend" group can follow (the walks hold the group's input for the blend then):
//   * a SINGLE group: a module in front of a blend is never fused (blended() below);
//   * never a RAW group: none of its three nodes may be blended;
//   * an RGB group only where it ends in "export_u16" / "export_rows", which the run takes without asking blended().  No
//     module is blended there, the pipe is invalid and nothing rejects it: the blend then gets the run's INPUT and the
//     converted samples, and the walk returns what dt_hip_develop_blend_process() makes of them.  A run that ends in a
//     stage or in the Lab glue stops in front of a blended node.
void dt_hip_pipe_t::plan()
{
  groups.clear();
  placement = plan_error_t();
  band_checked = false;
  planned = true;
  const int n = (int)nodes.size();
  // the encoder takes the 8-bit frame and makes a file: nothing can read its output
  for(int k = 0; k < n && placement.code == DT_HIP_SUCCESS; k++)
    if(nodes[k].op == OP_EXPORT_JPEG && (k + 1 != n || k == 0 || nodes[k - 1].op != OP_EXPORT_U8))
    {
      set_last_error("pipe: 'export_jpeg' must be the last node, directly behind 'export_u8' (it is node %d of %d%s%s)", k + 1, n,
                     k ? ", behind " : "", k ? k_ops[nodes[k - 1].op].name : "");
      placement.keep(DT_HIP_INVALID_ARG);
    }
  for(int k = 0; k < n && placement.code == DT_HIP_SUCCESS; k++)
    if(nodes[k].op == OP_EXPORT_WEBP && (k + 1 != n || k == 0 || nodes[k - 1].op != OP_EXPORT_U8))
    {
      set_last_error("pipe: 'export_webp' must be the last node, directly behind 'export_u8' (it is node %d of %d%s%s)", k + 1, n,
                     k ? ", behind " : "", k ? k_ops[nodes[k - 1].op].name : "");
      placement.keep(DT_HIP_INVALID_ARG);
    }
  for(int k = 0; k < n && placement.code == DT_HIP_SUCCESS; k++)
    if(nodes[k].op == OP_EXPORT_PNG)
    {
      const int depth = nodes[k].as<dt_hip_png_data_t>()->bit_depth;
      const op_t want = depth == 16 ? OP_EXPORT_U16 : OP_EXPORT_U8;
      if(k + 1 != n || k == 0 || nodes[k - 1].op != want)
      {
        set_last_error("pipe: 'export_png' at %d bits must be the last node, directly behind '%s' (it is node %d of %d%s%s)", depth,
                       k_ops[want].name, k + 1, n, k ? ", behind " : "", k ? k_ops[nodes[k - 1].op].name : "");
        placement.keep(DT_HIP_INVALID_ARG);
      }
    }
  for(int k = 0; k < n && placement.code == DT_HIP_SUCCESS; k++)
    if(nodes[k].op == OP_EXPORT_TIFF)
    {
      const int bpp = nodes[k].as<dt_hip_tiff_data_t>()->bpp;
      // 8 / 16 bits: the export conversion of that depth; 32 bits: any node that writes four floats a pixel
      const char *want = bpp == 8 ? "'export_u8'" : bpp == 16 ? "'export_u16'" : "a node that writes four floats a pixel";
      bool ok = k + 1 == n && k > 0;
      if(ok)
      {
        const node_t &p = nodes[k - 1];
        const bool floats = p.op != OP_EXPORT_U8 && p.op != OP_EXPORT_U16 && p.op != OP_EXPORT_ROWS && p.op < OP_EXPORT_JPEG
                            && (k_ops[p.op].bpp_out ? k_ops[p.op].bpp_out : 4 * (int)p.piece.channels) == 16;
        ok = bpp == 8 ? p.op == OP_EXPORT_U8 : bpp == 16 ? p.op == OP_EXPORT_U16 : floats;
      }
      if(!ok)
      {
        set_last_error("pipe: 'export_tiff' at %d bits must be the last node, directly behind %s (it is node %d of %d%s%s)", bpp,
                       want, k + 1, n, k ? ", behind " : "", k ? k_ops[nodes[k - 1].op].name : "");
        placement.keep(DT_HIP_INVALID_ARG);
      }
    }
  // flip passes its input format through: a consumer that reads another one would read past the flip's output
  for(int k = 0; k + 1 < n && placement.code == DT_HIP_SUCCESS; k++)
    if(nodes[k].op == OP_FLIP && nodes[k + 1].piece.channels != nodes[k].piece.channels)
    {
      set_last_error("pipe: the flip node has %u channels, the '%s' node behind it reads %u", nodes[k].piece.channels,
                     k_ops[nodes[k + 1].op].name, nodes[k + 1].piece.channels);
      placement.keep(DT_HIP_INVALID_ARG);
    }
  // a module followed by a "blend" node keeps both its input and its output as buffers: it is never fused
  auto blended = [&](const int k) { return k + 1 < n && nodes[k + 1].op == OP_BLEND; };
  int i = 0;
  while(i < n)
  {
    group_t g;
    g.kind = group_t::SINGLE;
    g.first = i;
    g.count = 1;
    if(fusion && nodes[i].op == OP_RAWPREPARE && !blended(i) && !blended(i + 1) && !blended(i + 2))
    {
      raw_group_t r;
      memset(&r, 0, sizeof(r));
      r.rawprepare_piece = nodes[i].piece;
      r.rawprepare = *nodes[i].as<dt_hip_rawprepare_data_t>();
      int j = i + 1;
      if(j < n && nodes[j].op == OP_TEMPERATURE)
      {
        r.has_temperature = true;
        r.temperature_piece = nodes[j].piece;
        r.temperature = *nodes[j].as<dt_hip_temperature_data_t>();
        j++;
      }
      if(j < n && nodes[j].op == OP_HIGHLIGHTS)
      {
        r.has_highlights = true;
        r.highlights_piece = nodes[j].piece;
        r.highlights = *nodes[j].as<dt_hip_highlights_data_t>();
        j++;
      }
      if(j - i > 1 && raw_group_supported(r))
      {
        g.kind = group_t::RAW;
        g.count = j - i;
        g.raw = r;
      }
    }
    else if(fusion && nodes[i].piece.channels == 4 && !blended(i)
            && ((nodes[i].op >= OP_EXPOSURE && nodes[i].op <= OP_COLOROUT)
                || (nodes[i].op == OP_LAB_TO_RGB && !nodes[i].as<dt_hip_lab_data_t>()->nonlinearlut && i + 1 < n
                    && nodes[i + 1].op >= OP_EXPOSURE && nodes[i + 1].op <= OP_COLOROUT)))
    {
      rgb_group_t r;
      memset(&r, 0, sizeof(r));
      r.width = nodes[i].piece.roi_out.width;
      r.height = nodes[i].piece.roi_out.height;
      // the fused kernel applies its stages in the reference's pipe order (exposure < colorin <
      // channelmixerrgb < filmicrgb < colorout, src/develop/iop_order.c); a run is fusable as long
      // as it walks that order
      int last_op = -1;
      int j = i;
      if(nodes[i].op == OP_LAB_TO_RGB)
      {
        // the Lab -> RGB glue behind a Lab module is the first stage of the run that follows it
        r.pre_lab = 1;
        r.lab_pre = *nodes[i].as<dt_hip_lab_data_t>();
        j++;
      }
      while(j < n && r.n_ops < 8)
      {
        const node_t &nd = nodes[j];
        if(nd.op < OP_EXPOSURE || nd.op > OP_COLOROUT || (int)nd.op <= last_op || blended(j)) break;
        if(nd.piece.roi_out.width != r.width || nd.piece.roi_out.height != r.height || nd.piece.channels != 4) break;
        if(nd.op == OP_FILMICRGB)
        {
          const int v = nd.as<dt_hip_filmicrgb_data_t>()->version;
          if(v < 3 || v > 9) break;
        }
        if(nd.op == OP_CHANNELMIXERRGB && nd.as<dt_hip_channelmixerrgb_data_t>()->adaptation > DT_HIP_ADAPTATION_RGB) break;
        last_op = (int)nd.op;
        switch(nd.op)
        {
          case OP_EXPOSURE: r.ops[r.n_ops++] = RGB_OP_EXPOSURE; r.exposure = *nd.as<dt_hip_exposure_data_t>(); break;
          case OP_COLORIN: r.ops[r.n_ops++] = RGB_OP_COLORIN; r.colorin = *nd.as<dt_hip_conversion_t>(); break;
          case OP_CHANNELMIXERRGB: r.ops[r.n_ops++] = RGB_OP_CHANNELMIXER; r.channelmixer = *nd.as<dt_hip_channelmixerrgb_data_t>(); break;
          case OP_FILMICRGB: r.ops[r.n_ops++] = RGB_OP_FILMIC; r.filmic = *nd.as<dt_hip_filmicrgb_data_t>(); break;
          default: r.ops[r.n_ops++] = RGB_OP_COLOROUT; r.colorout = *nd.as<dt_hip_conversion_t>(); break;
        }
        j++;
      }
      if(j < n && nodes[j].op == OP_EXPORT_U16 && nodes[j].piece.roi_out.width == r.width
         && nodes[j].piece.roi_out.height == r.height)
      {
        r.to_u16 = 1;
        j++;
        // ... and straight into the scanlines of the format writer
        if(j < n && nodes[j].op == OP_EXPORT_ROWS && nodes[j].as<dt_hip_export_rows_t>()->bpp == 16
           && nodes[j].as<dt_hip_export_rows_t>()->layers == 3 && nodes[j].piece.roi_out.width == r.width
           && nodes[j].piece.roi_out.height == r.height)
        {
          r.to_u16 = 2;
          j++;
        }
      }
      else if(r.n_ops > 0 && j < n && nodes[j].op == OP_RGB_TO_LAB && !blended(j) && nodes[j].piece.channels == 4
              && !nodes[j].as<dt_hip_lab_data_t>()->nonlinearlut
              && nodes[j].piece.roi_out.width == r.width && nodes[j].piece.roi_out.height == r.height)
      {
        // ... and the RGB -> Lab glue in front of a Lab module its last one
        r.post_lab = 1;
        r.lab_post = *nodes[j].as<dt_hip_lab_data_t>();
        j++;
      }
      if(j - i > 1 && r.n_ops > 0)
      {
        g.kind = group_t::RGB;
        g.count = j - i;
        g.rgb = r;
      }
    }
    groups.push_back(g);
    i += g.count;
  }
}

extern "C" {

dt_hip_pipe_t *dt_hip_pipe_new(int devid)
{
  if(!valid_device(devid)) return nullptr;
  dt_hip_pipe_t *p = new dt_hip_pipe_t;
  p->devid = devid;
  return p;
}

void dt_hip_pipe_free(dt_hip_pipe_t *pipe) { delete pipe; }

int dt_hip_pipe_add_node(dt_hip_pipe_t *pipe, const char *op, const dt_hip_piece_t *piece, const void *data,
                         size_t data_size)
{
  if(!pipe || !op || !piece) return DT_HIP_INVALID_ARG;
  node_t n;
  const int err = make_node(n, "dt_hip_pipe_add_node", op, piece, data, data_size);
  if(err != DT_HIP_SUCCESS) return err;
  if(n.op == OP_BLEND && (pipe->dropped_flip || (!pipe->nodes.empty() && pipe->nodes.back().op == OP_FLIP)))
  {
    set_last_error("dt_hip_pipe_add_node: flip has no blending (a 'blend' node cannot follow it)");
    return DT_HIP_INVALID_ARG;
  }
  pipe->dropped_flip = false;
  if(n.op == OP_FLIP)
  {
    const int orientation = n.as<dt_hip_flip_data_t>()->orientation;
    if(orientation < 0 || orientation > 7)
    {
      set_last_error("dt_hip_pipe_add_node: flip orientation %d is not one of 0..7 (resolve -1 to the image's orientation first)",
                     orientation);
      return DT_HIP_INVALID_ARG;
    }
    const bool swap = (orientation & 4) != 0;
    if(piece->roi_out.width != (swap ? piece->roi_in.height : piece->roi_in.width)
       || piece->roi_out.height != (swap ? piece->roi_in.width : piece->roi_in.height))
    {
      set_last_error("dt_hip_pipe_add_node: flip orientation %d: roi_out %d x %d is not roi_in %d x %d oriented", orientation,
                     piece->roi_out.width, piece->roi_out.height, piece->roi_in.width, piece->roi_in.height);
      return DT_HIP_INVALID_ARG;
    }
    if(orientation == 0)
    {
      // the identity: no node, so launches and words are those of the pipe without it
      pipe->dropped_flip = true;
      return DT_HIP_SUCCESS;
    }
  }
  pipe->nodes.push_back(std::move(n));
  pipe->planned = false;
  return DT_HIP_SUCCESS;
}

void dt_hip_pipe_set_fusion(dt_hip_pipe_t *pipe, int enabled)
{
  if(!pipe) return;
  pipe->fusion = enabled != 0;
  pipe->planned = false;
}

int dt_hip_pipe_num_groups(dt_hip_pipe_t *pipe)
{
  if(!pipe) return 0;
  if(!pipe->planned) pipe->plan();
  return (int)pipe->groups.size();
}

int dt_hip_pipe_process(dt_hip_pipe_t *pipe, dt_hip_mem_t dev_in, dt_hip_mem_t dev_out)
{
  if(!pipe || !dev_in || !dev_out) return DT_HIP_INVALID_ARG;
  if(pipe->nodes.empty()) return DT_HIP_SUCCESS;
  if(!pipe->planned) pipe->plan();
  if(pipe->placement.code != DT_HIP_SUCCESS) return pipe->placement.report();
  const int devid = pipe->devid;
  // Every buffer of the walk is a handle: whatever path leaves the walk, what it owns goes back to the pool.  On the paths
  // that succeed the releases are explicit (release(), or the assignment that replaces a buffer) and stand where the
  // pool's reuse wants them: behind the launch that reads the buffer, in front of the next group's allocation
  dev_buf_t cur = dev_buf_t::borrow(dev_in);
  dev_buf_t held; // the input of a module whose output is about to be blended
  // the lightness cells of the current buffer's pixels, written by the non-local-means kernels for the bilateral grid of the local
  // contrast module right behind them (round 6: bilat_zcells' pass over the frame -- 24 B/px -- folded into their epilogue)
  dev_buf_t cells;
  const size_t ng = pipe->groups.size();
  // A module and the group behind it in ONE launch: `launch(in, out)` runs the pair, or returns DT_HIP_INVALID_ARG when it
  // has no kernel for this combination -- as this step does when the pair may not fuse; the caller then runs the two groups
  // one after the other.  On success the pair's output is the current buffer and the caller skips the group behind.
  // A blend behind the pair wants the second group's input as a buffer, which a fused pair never writes: not fused
  // (plan(): behind "rgb_to_lab", or behind a run that ends in the export conversion)
  auto fused_pair = [&](const size_t gi, const bool may_fuse, const size_t pair_bytes, auto launch) -> int {
    if(!pipe->fusion || !may_fuse || pipe->is_blend_group(gi + 2)) return DT_HIP_INVALID_ARG;
    dev_buf_t fout = gi + 2 == ng ? dev_buf_t::borrow(dev_out) : dev_buf_t::alloc(devid, pair_bytes);
    if(!fout) return DT_HIP_INVALID_ARG;
    const int err = launch(cur.ptr(), fout.ptr());
    if(err == DT_HIP_SUCCESS) cur = std::move(fout); // releases the pair's input: stream-ordered
    return err;
  };
  for(size_t gi = 0; gi < ng; gi++)
  {
    const group_t &g = pipe->groups[gi];
    const node_t &nd = pipe->nodes[g.first];
    const node_t &last = pipe->nodes[g.first + g.count - 1];
    if(last.op == OP_BLEND)
    {
      // dt_develop_blend_process() after the module's process(), pixelpipe_cpu.c:137-228: in place in the output
      int err = DT_HIP_INVALID_ARG;
      if(held) err = dt_hip_develop_blend_process(devid, &last.piece, last.as<dt_hip_blend_data_t>(), held.ptr(), cur.ptr());
      else set_last_error("pipe: a blend node needs the module it blends in front of it");
      held.release();
      if(err != DT_HIP_SUCCESS) return err;
      continue;
    }
    if(g.kind == group_t::SINGLE && gi + 1 < ng)
    {
      const group_t &gn = pipe->groups[gi + 1];
      const node_t &tail = pipe->nodes[gn.first + gn.count - 1];
      int ferr = DT_HIP_INVALID_ARG;
      if(nd.op == OP_DENOISEPROFILE)
        // denoise (profiled) followed by a pointwise run: the run becomes the tail of the module's last kernel
        // (denoiseprofile.hip dn_finish_chain) when there is such a kernel for the combination
        ferr = fused_pair(gi, gn.kind == group_t::RGB, out_bytes(tail), [&](dt_hip_mem_t in, dt_hip_mem_t out) {
          return denoiseprofile_process_chain(devid, &nd.piece, nd.as<dt_hip_denoiseprofile_data_t>(), in, out, &gn.rgb);
        });
      else if(nd.op == OP_BILAT)
        // local contrast (bilateral grid) followed by a pointwise run: the module's slice -- pointwise, given the blurred grid -- becomes
        // the run's first stage (bilat.hip bilat_process_chain()): the module's output plane is never written
        ferr = fused_pair(gi, gn.kind == group_t::RGB, out_bytes(tail), [&](dt_hip_mem_t in, dt_hip_mem_t out) {
          const int err = bilat_process_chain(devid, &nd.piece, nd.as<dt_hip_bilat_data_t>(), in, out, &gn.rgb, cells.ptr());
          if(err == DT_HIP_SUCCESS) cells.release(); // stream-ordered
          return err;
        });
      else if(nd.op == OP_DIFFUSE)
        // diffuse or sharpen followed by the RGB -> Lab glue: the conversion is the tail of the module's last kernel
        ferr = fused_pair(gi, gn.kind == group_t::SINGLE && tail.op == OP_RGB_TO_LAB && !tail.as<dt_hip_lab_data_t>()->nonlinearlut,
                          out_bytes(tail), [&](dt_hip_mem_t in, dt_hip_mem_t out) {
                            return diffuse_process_post_lab(devid, &nd.piece, nd.as<dt_hip_diffuse_data_t>(), in, out, tail.as<dt_hip_lab_data_t>());
                          });
      if(ferr == DT_HIP_SUCCESS)
      {
        gi++;
        continue;
      }
      if(ferr != DT_HIP_INVALID_ARG) return ferr;
    }
    dev_buf_t out = pipe->is_final_group(gi) ? dev_buf_t::borrow(dev_out) : dev_buf_t::alloc(devid, out_bytes(last));
    if(!out) return DT_HIP_SYSMEM_ALLOCATION;
    if(out.owned() && g.kind == group_t::SINGLE && pipe->leaves_unwritten_alpha(g.first)
       && hipMemsetAsync(out.ptr(), 0, out_bytes(last), stream_of(devid)) != hipSuccess)
      return DT_HIP_DEFAULT_ERROR;
    int err;
    if(g.kind == group_t::RAW)
      err = raw_group_launch(devid, g.raw, cur.ptr(), out.ptr());
    else if(g.kind == group_t::RGB)
      err = rgb_group_launch(devid, g.rgb, cur.ptr(), out.ptr());
    else
    {
      err = DT_HIP_INVALID_ARG;
      // denoise (non-local means) with local contrast's bilateral grid right behind it: the cells of the grid's third axis leave the
      // non-local-means kernels with the pixels (no blend in between: the grid is splatted from the module's own output)
      if(pipe->fusion && nd.op == OP_NLMEANS && gi + 1 < ng && pipe->groups[gi + 1].kind == group_t::SINGLE
         && pipe->nodes[pipe->groups[gi + 1].first].op == OP_BILAT)
      {
        const node_t &bl = pipe->nodes[pipe->groups[gi + 1].first];
        float sigma_r = 0.0f;
        int size_z = 0;
        if(bilat_cell_params(&bl.piece, bl.as<dt_hip_bilat_data_t>(), &sigma_r, &size_z) == DT_HIP_SUCCESS
           && bl.piece.roi_in.width == nd.piece.roi_out.width && bl.piece.roi_in.height == nd.piece.roi_out.height)
        {
          cells = dev_buf_t::alloc(devid, (size_t)nd.piece.roi_out.width * nd.piece.roi_out.height * 2 * sizeof(float));
          if(cells)
          {
            err = nlmeans_process_cells(devid, &nd.piece, nd.as<dt_hip_nlmeans_data_t>(), cur.ptr(), out.ptr(), cells.ptr(), sigma_r, size_z);
            if(err != DT_HIP_SUCCESS) cells.release();
          }
        }
      }
      else if(nd.op == OP_BILAT && cells)
      {
        err = bilat_process_cells(devid, &nd.piece, nd.as<dt_hip_bilat_data_t>(), cur.ptr(), out.ptr(), cells.ptr());
        cells.release();
      }
      if(err == DT_HIP_INVALID_ARG && !cells) err = run_single(devid, nd, cur.ptr(), out.ptr());
    }
    if(err == DT_HIP_SUCCESS && pipe->is_blend_group(gi + 1)) held = std::move(cur);
    else cur.release(); // stream-ordered: re-used only by later launches
    if(err != DT_HIP_SUCCESS) return err;
    cur = std::move(out);
  }
  return DT_HIP_SUCCESS;
}

} // extern "C"
