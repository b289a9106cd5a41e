// pipe_internal.h -- what the translation units of the executor share: the module table, the node list with its plan,
// (pipe.cpp, pipe_batch.cpp, pipe_bands.cpp, pipe_tiling.cpp).
// Not part of the C-ABI (that is include/ansel_hip.h).
#pragma once
#include "hip_common.h"
#include "dev_buf.h"
#include "pipe_fused.h"

#include <string>
#include <utility>
#include <vector>

namespace ansel
{

// The index of k_ops[].  OP_EXPOSURE ... OP_COLOROUT are contiguous and in the reference's pipe order (exposure <
// colorin < channelmixerrgb < filmicrgb < colorout, src/develop/iop_order.c): dt_hip_pipe_t::plan() tests "a stage of
// the fused RGBA run" as a range of this enum and "the run walks the pipe order" by comparing its values
enum op_t
{
  OP_RAWPREPARE,
  OP_TEMPERATURE,
  OP_HIGHLIGHTS,
  OP_DEMOSAIC,
  OP_DENOISEPROFILE,
  OP_EXPOSURE,
  OP_COLORIN,
  OP_CHANNELMIXERRGB,
  OP_FILMICRGB,
  OP_COLOROUT,
  OP_DIFFUSE,
  OP_RGB_TO_LAB,
  OP_NLMEANS,
  OP_BILAT,
  OP_LAB_TO_RGB,
  OP_FINALSCALE,
  OP_INITIALSCALE,
  OP_EXPORT_U16,
  OP_BLEND,
  OP_EXPORT_ROWS,
  OP_EXPORT_U8,
  OP_DETAILMASK,
  OP_FLIP, // changes the geometry (SWAP_XY): never inside a fused group
  OP_EXPORT_JPEG, // the last node, behind export_u8: a file, not pixels
  OP_EXPORT_PNG,  // the last node, behind export_u8 (8 bits) or export_u16 (16 bits): a file
  OP_EXPORT_TIFF, // the last node, behind export_u8, export_u16 or (32 bits) a node that writes four floats a pixel: a file
  OP_EXPORT_WEBP, // the last node, behind export_u8: a file, not a frame
  OP_UNKNOWN
};
static_assert(OP_COLORIN == OP_EXPOSURE + 1 && OP_CHANNELMIXERRGB == OP_EXPOSURE + 2 && OP_FILMICRGB == OP_EXPOSURE + 3
                && OP_COLOROUT == OP_EXPOSURE + 4,
              "plan() relies on exposure ... colorout being contiguous and in the reference's pipe order");

struct node_t
{
  op_t op;
  dt_hip_piece_t piece;
  std::vector<unsigned char> data;
  std::vector<unsigned char> icc; // export_jpeg / export_png / export_tiff / export_webp: the node's copy of the ICC profile its data pointed to
  template <typename T> const T *as() const { return reinterpret_cast<const T *>(data.data()); }
};

enum
{
  OPF_CFA = 1,     // works on the mosaic: the first stage of a row band (dt_hip_pipe_band_begin())
  OPF_STENCIL = 2, // reads rows beyond its own: a row band stops in front of it for the neighbours' rows
  OPF_NO_PTP = 4   // dt_hip_default_process_tiling_ptp() cannot run it tile by tile
};

// One row per module: everything the executor, the band walk and the tile drivers know about it
struct op_info_t
{
  op_t op; // the row's own index (checked at compile time, pipe.cpp)
  const char *name;
  size_t data_size;
  int bpp_out;                         // bytes per pixel of the module output; 0: 4 bytes per channel, as the input
  size_t (*out_size)(const node_t &n); // the export nodes whose output size comes from their data (then bpp_out is not read)
  int (*run)(int devid, const node_t &n, dt_hip_mem_t in, dt_hip_mem_t out);
  unsigned flags; // OPF_*
  // rows of its input the module's own rows depend on beyond a band (-1: no row-band implementation, or the module passes
  // this frame through); nullptr: none
  int (*halo_rows)(const node_t &n);
};
extern const op_info_t k_ops[OP_UNKNOWN];

// (name, piece, data) -> node, with the node's own copy of what the data points to.  DT_HIP_INVALID_ARG with the last error
// set ("<who>: ...") for a name without a row in k_ops[] and for data of another size than the module's struct
int make_node(node_t &n, const char *who, const char *name, const dt_hip_piece_t *piece, const void *data, size_t data_size);
size_t out_bytes(const node_t &n);
static inline int run_single(int devid, const node_t &n, dt_hip_mem_t in, dt_hip_mem_t out) { return k_ops[n.op].run(devid, n, in, out); }
static inline int band_halo_rows(const node_t &n) { return k_ops[n.op].halo_rows ? k_ops[n.op].halo_rows(n) : 0; }

struct group_t
{
  enum kind_t { SINGLE, RAW, RGB } kind;
  int first, count; // node range
  raw_group_t raw;
  rgb_group_t rgb;
};

// what a check of the node list found: kept with the plan, reported by every call on that node list
struct plan_error_t
{
  int code = DT_HIP_SUCCESS;
  std::string text;
  // the text just given to set_last_error()
  int keep(const int c)
  {
    code = c;
    text = dt_hip_last_error();
    return c;
  }
  int report() const
  {
    if(code != DT_HIP_SUCCESS) set_last_error("%s", text.c_str());
    return code;
  }
};

} // namespace ansel

struct dt_hip_pipe_t
{
  int devid = 0;
  bool fusion = true;
  bool planned = false;
  bool dropped_flip = false; // the last node added was a flip of orientation 0 (not kept)
  std::vector<ansel::node_t> nodes;
  // what plan() makes of the node list
  std::vector<ansel::group_t> groups;
  ansel::plan_error_t placement; // a node in a place where dt_hip_pipe_process() cannot run it
  // a node without a row-band implementation: looked for by the first dt_hip_pipe_band_begin() on this plan (pipe_bands.cpp)
  bool band_checked = false;
  ansel::plan_error_t band_mode;

  void plan(); // pipe.cpp
  bool is_blend_group(const size_t k) const { return k < groups.size() && nodes[groups[k].first].op == ansel::OP_BLEND; }
  // the group's output is the pipe's: it is the last group, or only the blend of its module follows
  bool is_final_group(const size_t k) const { return k + 1 == groups.size() || (is_blend_group(k + 1) && k + 2 == groups.size()); }
  // The demosaics leave the fourth channel of their output to their caller, as the reference's do (RCD and PPG on the border
  // ring, AMaZE and the passthroughs on the whole frame), and so does the local laplacian.  Where no node behind node k writes
  // that channel whatever it finds (colorin, colorout, denoise (profiled)) or drops it (scanlines of three samples), the words
  // reach the pipe's output -- and in a buffer of the executor's own they would be what the pool held: true then, and the walk
  // clears the buffer before the module runs (a buffer of the caller's keeps what the caller put there).  The tests state the
  // same rule for their node lists: tests/pipe_cases.py, SETS_ALPHA and alpha_is_written() -- change the two together
  bool leaves_unwritten_alpha(const size_t k) const
  {
    const ansel::node_t &n = nodes[k];
    const bool leaves = n.op == ansel::OP_DEMOSAIC
                        || (n.op == ansel::OP_BILAT && n.as<dt_hip_bilat_data_t>()->mode == DT_HIP_BILAT_LOCAL_LAPLACIAN);
    if(!leaves) return false;
    for(size_t j = k + 1; j < nodes.size(); j++)
    {
      const ansel::op_t op = nodes[j].op;
      if(op == ansel::OP_COLORIN || op == ansel::OP_COLOROUT || op == ansel::OP_DENOISEPROFILE) return false;
      if(op == ansel::OP_EXPORT_ROWS && nodes[j].as<dt_hip_export_rows_t>()->layers == 3) return false;
    }
    return true;
  }
  // the pipe's output is a file -- a little-endian uint64 length word and that many bytes in a buffer of the encoder's bound -- and
  // not a frame: what a batch in file mode downloads (pipe_batch.cpp, dt_hip_batch_set_file_output())
  bool output_is_a_file() const
  {
    if(nodes.empty()) return false;
    const ansel::op_t op = nodes.back().op;
    return op == ansel::OP_EXPORT_JPEG || op == ansel::OP_EXPORT_PNG || op == ansel::OP_EXPORT_TIFF || op == ansel::OP_EXPORT_WEBP;
  }
  // the same for the pipe's output: the group that writes it leaves the fourth channel to whoever owns that buffer (the batch
  // owns its slots' and clears them once: pipe_batch.cpp)
  bool output_keeps_the_callers_alpha() const
  {
    for(size_t k = 0; k < groups.size(); k++)
      if(is_final_group(k)) return groups[k].kind == ansel::group_t::SINGLE && leaves_unwritten_alpha(groups[k].first);
    return false;
  }
};
