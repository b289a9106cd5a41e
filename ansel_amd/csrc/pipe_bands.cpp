// pipe_bands.cpp -- one frame as row bands (include/ansel_hip.h section 3b): the band plan, the resumable walk of one band
// on one device (dt_hip_pipe_band_*), and the gang that walks the bands of a frame over the devices of one process
// (dt_hip_pipe_process_bands()).
#include "pipe_internal.h"
#include "amaze_stream_body.h" // amz::stream_tile_ok(): which AMaZE tiles the on-chip kernel takes (band planning)

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace ansel;

namespace ansel
{
int dt_hip_iop_demosaic_process_band(int devid, const dt_hip_piece_t *piece, const dt_hip_demosaic_data_t *d,
                                     const rcd_band_t *band, dt_hip_mem_t dev_in, dt_hip_mem_t dev_out);
}

namespace
{
const int RCD_TV = 94, RCD_TS = 112, RCD_HALO = 9; // tile pitch, tile size, RCD_BORDER (rcd.c:70-76)
const int AMZ_TV = 128, AMZ_HALO = 16;              // AMaZE: rows a tile keeps, rows it reads beyond them (amaze.cc:181-350)

// What a band holds between the calls of its walk.  Deleting it gives everything back, wherever the walk stands
struct band_priv_t
{
  dev_buf_t journal;             // deferred highlights journal or empty
  dt_hip_mem_t hl_out = nullptr; // the rows the journal indexes (in `cur`)
  size_t next_group = 0;
  // dt_hip_pipe_band_finish() is resumable: where the walk stands
  bool walking = false;
  // the current module input: the allocation (after dt_hip_pipe_band_begin(): the output of the CFA stages, in the halo
  // layout when a demosaic follows) and, as its view, the band's own rows
  dev_buf_t cur;
  bool cur_is_halo_layout = false;
  int stage = 0; // inside a stencil group: 0 before the halo exchange, 1 after it, 2 after the sums, 3 done
  dev_buf_t out; // a stencil module's output while the walk stops inside the module; its view: the band's own rows
  dev_buf_t held; // the input of a module whose output is about to be blended; its view: the band's own rows
  dn_band_job_t *dn_job = nullptr;
  dev_buf_t relay; // local contrast: this band's copy of the frame's bilateral grid
  size_t relay_bytes = 0;
  ~band_priv_t()
  {
    if(dn_job) denoiseprofile_band_abort(dn_job);
  }
};

// the band's view of a node: same columns, rows [row0, row0 + rows) of the frame
void band_piece(dt_hip_piece_t &p, const dt_hip_band_t &b)
{
  p.roi_in.y += b.row0;
  p.roi_in.height = b.rows;
  p.roi_out.y += b.row0;
  p.roi_out.height = b.rows;
}
void band_rawprepare(dt_hip_piece_t &p, dt_hip_rawprepare_data_t &d, const dt_hip_band_t &b)
{
  // the band input starts at input row crop_y + row0: fold the crop into the CFA phase
  p.roi_out.y += d.y + b.row0;
  d.y = 0;
  p.roi_in.height = b.rows;
  p.roi_out.height = b.rows;
}
} // namespace

extern "C" {

int dt_hip_plan_bands(int width, int height, int demosaic_method, int n_bands, dt_hip_band_t *bands)
{
  if(width <= 0 || height <= 0 || n_bands <= 0 || !bands) return DT_HIP_INVALID_ARG;
  memset(bands, 0, sizeof(dt_hip_band_t) * (size_t)n_bands);
  if(demosaic_method == DT_HIP_DEMOSAIC_RCD)
  {
    if(width < 16 || height < 16) return DT_HIP_INVALID_ARG;
    const int num_vertical = 1 + (height - 2 * RCD_HALO - 1) / RCD_TV; // rcd.c:286
    if(num_vertical < n_bands)
    {
      set_last_error("dt_hip_plan_bands: %d rows give %d RCD tile rows, fewer than %d bands", height, num_vertical, n_bands);
      return DT_HIP_INVALID_ARG;
    }
    for(int k = 0; k < n_bands; k++)
    {
      const int tv0 = (int)((long)k * num_vertical / n_bands), tv1 = (int)((long)(k + 1) * num_vertical / n_bands);
      dt_hip_band_t &b = bands[k];
      b.tile_row0 = tv0;
      b.tile_row1 = tv1;
      b.row0 = tv0 ? tv0 * RCD_TV + RCD_HALO : 0;
      const int row1 = (tv1 < num_vertical) ? tv1 * RCD_TV + RCD_HALO : height;
      b.rows = row1 - b.row0;
      b.halo_top = b.row0 - tv0 * RCD_TV;
      const int need1 = (tv1 - 1) * RCD_TV + RCD_TS < height ? (tv1 - 1) * RCD_TV + RCD_TS : height;
      b.halo_bottom = need1 > row1 ? need1 - row1 : 0;
    }
    return DT_HIP_SUCCESS;
  }
  if(demosaic_method == DT_HIP_DEMOSAIC_AMAZE)
  {
    // AMaZE's own tiles (amaze.cc:181-350): 160 rows of the mosaic 16 above a tile row's 128 kept rows.  A band owns whole
    // tile rows, so it needs 16 mosaic rows of either neighbour; the rows a tile mirrors at the frame's bottom edge lie in
    // the last band's own rows and in what the band above it fetches of them (fewer than 16 rows are left there)
    if(width < 34 || height < 34) return DT_HIP_INVALID_ARG;
    const int tile_rows = (height + AMZ_TV - 1) / AMZ_TV;
    if(tile_rows < n_bands)
    {
      set_last_error("dt_hip_plan_bands: %d rows give %d AMaZE tile rows, fewer than %d bands", height, tile_rows, n_bands);
      return DT_HIP_INVALID_ARG;
    }
    // only the on-chip kernel walks a band (demosaic_amaze.hip): a frame that keeps tiles in the first kernel's body -- a
    // last tile column of odd width, a mirrored strip past its plane -- would be refused by the band's demosaic launch,
    // after the CFA stages and the halo copies of every band have run.  Say so here, where the caller can still take
    // the unsplit path
    for(int ty = 0; ty < tile_rows; ty++)
      for(int tx = 0; tx < (width + AMZ_HALO + AMZ_TV - 1) / AMZ_TV; tx++) // the launch's tile columns (demosaic_amaze.hip)
        if(!amz::stream_tile_ok(width, height, -AMZ_HALO + ty * AMZ_TV, -AMZ_HALO + tx * AMZ_TV))
        {
          set_last_error("dt_hip_plan_bands: the AMaZE tile at row %d, column %d of a %d x %d frame is not one the on-chip kernel takes "
                         "(odd width of the last tile column, or a mirrored strip past its plane): no band mode for this frame",
                         ty * AMZ_TV, tx * AMZ_TV, width, height);
          return DT_HIP_INVALID_ARG;
        }
    for(int k = 0; k < n_bands; k++)
    {
      const int tv0 = (int)((long)k * tile_rows / n_bands), tv1 = (int)((long)(k + 1) * tile_rows / n_bands);
      dt_hip_band_t &b = bands[k];
      b.tile_row0 = tv0;
      b.tile_row1 = tv1;
      b.row0 = tv0 * AMZ_TV;
      const int row1 = tv1 < tile_rows ? tv1 * AMZ_TV : height;
      b.rows = row1 - b.row0;
      b.halo_top = tv0 ? AMZ_HALO : 0;
      b.halo_bottom = height - row1 < AMZ_HALO ? height - row1 : AMZ_HALO;
    }
    return DT_HIP_SUCCESS;
  }
  if(demosaic_method != -1)
  {
    set_last_error("dt_hip_plan_bands: demosaic method %d has no band mode", demosaic_method);
    return DT_HIP_INVALID_ARG;
  }
  if(height / 2 < n_bands) return DT_HIP_INVALID_ARG;
  for(int k = 0; k < n_bands; k++)
  {
    const int r0 = (int)((long)k * (height / 2) / n_bands) * 2;
    const int r1 = (k + 1 == n_bands) ? height : (int)((long)(k + 1) * (height / 2) / n_bands) * 2;
    bands[k].row0 = r0;
    bands[k].rows = r1 - r0;
  }
  return DT_HIP_SUCCESS;
}

namespace
{
// The checks of dt_hip_pipe_band_begin() that depend on the node list alone: made once per plan
static void check_band_mode(dt_hip_pipe_t *pipe)
{
  pipe->band_checked = true;
  pipe->band_mode = plan_error_t();
  auto refuse = [&]() { pipe->band_mode.keep(DT_HIP_INVALID_ARG); };
  const int W = pipe->nodes[0].piece.roi_out.width, H = pipe->nodes[0].piece.roi_out.height;
  for(const node_t &n : pipe->nodes)
    if(n.op == OP_EXPORT_JPEG || n.op == OP_EXPORT_PNG || n.op == OP_EXPORT_TIFF || n.op == OP_EXPORT_WEBP)
    {
      // a file is not rows: the entropy-coded data (the zlib stream) of one band depends on every band before it
      set_last_error("band mode: '%s' encodes the whole frame and has no row-band implementation", k_ops[n.op].name);
      return refuse();
    }
  for(const node_t &n : pipe->nodes)
    if(n.op == OP_FLIP)
    {
      // row bands of a transposed frame are columns of its input; a mirrored one would take another band's rows
      set_last_error("band mode: 'flip' with orientation %d has no row-band implementation", (int)n.as<dt_hip_flip_data_t>()->orientation);
      return refuse();
    }
  for(const node_t &n : pipe->nodes)
    if(n.piece.roi_out.width != W || n.piece.roi_out.height != H)
    {
      set_last_error("band mode: every node must produce the same %d x %d geometry", W, H);
      return refuse();
    }
  for(const node_t &n : pipe->nodes)
  {
    if(n.op == OP_FINALSCALE || n.op == OP_INITIALSCALE)
    {
      // finalscale / initialscale change the geometry
      set_last_error("band mode: '%s' has no row-band implementation", k_ops[n.op].name);
      return refuse();
    }
    if(n.op == OP_BILAT && !bilat_band_supported(&n.piece, n.as<dt_hip_bilat_data_t>()))
    {
      // the bilateral grid is relayed from band to band; the local laplacian's pyramid is not
      set_last_error("band mode: local contrast runs on row bands in its bilateral-grid mode only");
      return refuse();
    }
    if(n.op == OP_DETAILMASK || (n.op == OP_BLEND && blend_refines_with_detail_mask(n.as<dt_hip_blend_data_t>())))
    {
      // the raw detail mask is one plane of the frame on one device; its 9 x 9 blur reads across band borders
      set_last_error("band mode: the detail mask (the \"detailmask\" stage, a blend's details threshold) has no row-band "
                     "implementation");
      return refuse();
    }
    if(n.op == OP_BLEND && n.as<dt_hip_blend_data_t>()->feathering_radius > 0.1f)
    {
      // the guided filter works on its own 512-pixel tile grid over the whole frame
      set_last_error("band mode: a blend with mask feathering has no row-band implementation");
      return refuse();
    }
    if(n.op == OP_BLEND && n.as<dt_hip_blend_data_t>()->blur_radius > 0.0f)
    {
      // uniform and parametric masks are pointwise; the mask blur is a recursive filter down whole columns
      set_last_error("band mode: a blend with a mask blur has no row-band implementation");
      return refuse();
    }
  }
}
} // namespace

int dt_hip_pipe_band_begin(dt_hip_pipe_t *pipe, const dt_hip_band_t *band, dt_hip_mem_t dev_in_band,
                           dt_hip_band_state_t *state)
{
  if(!pipe || !band || !dev_in_band || !state || band->rows <= 0) return DT_HIP_INVALID_ARG;
  memset(state, 0, sizeof(*state));
  if(pipe->nodes.empty()) return DT_HIP_INVALID_ARG;
  if(!pipe->planned) pipe->plan();
  if(!pipe->band_checked) check_band_mode(pipe);
  if(pipe->band_mode.code != DT_HIP_SUCCESS) return pipe->band_mode.report();
  const int devid = pipe->devid;
  const dt_hip_band_t &b = *band;
  const int W = pipe->nodes[0].piece.roi_out.width, H = pipe->nodes[0].piece.roi_out.height;
  if(b.row0 < 0 || b.row0 + b.rows > H) return DT_HIP_INVALID_ARG;
  const size_t ng = pipe->groups.size();
  // the CFA stage ends where the first non-CFA group starts
  size_t n_cfa = 0;
  while(n_cfa < ng && (k_ops[pipe->nodes[pipe->groups[n_cfa].first].op].flags & OPF_CFA)) n_cfa++;
  const bool has_demosaic = n_cfa < ng && pipe->nodes[pipe->groups[n_cfa].first].op == OP_DEMOSAIC;
  if(!has_demosaic && (b.halo_top || b.halo_bottom)) return DT_HIP_INVALID_ARG;
  band_priv_t *pv = new band_priv_t;
  const size_t row_bytes = (size_t)W * 4;
  const size_t halo_rows = (size_t)b.halo_top + b.rows + b.halo_bottom;

  int err = DT_HIP_SUCCESS;
  dev_buf_t cur = dev_buf_t::borrow(dev_in_band);
  for(size_t gi = 0; gi < n_cfa && err == DT_HIP_SUCCESS; gi++)
  {
    const group_t &g = pipe->groups[gi];
    const bool last_cfa = gi + 1 == n_cfa;
    dev_buf_t buf = dev_buf_t::alloc(devid, last_cfa ? halo_rows * row_bytes : (size_t)b.rows * row_bytes);
    if(!buf)
    {
      err = DT_HIP_SYSMEM_ALLOCATION;
      break;
    }
    dt_hip_mem_t out = last_cfa ? (dt_hip_mem_t)((char *)buf.base() + (size_t)b.halo_top * row_bytes) : buf.base();
    const node_t &first = pipe->nodes[g.first];
    if(g.kind == group_t::RAW)
    {
      raw_group_t r = g.raw;
      band_rawprepare(r.rawprepare_piece, r.rawprepare, b);
      if(r.has_temperature) band_piece(r.temperature_piece, b);
      if(r.has_highlights)
      {
        band_piece(r.highlights_piece, b);
        pv->journal = dev_buf_t::alloc(devid, DT_HIP_HIGHLIGHTS_JOURNAL_BYTES);
        pv->hl_out = out;
        if(!pv->journal) err = DT_HIP_SYSMEM_ALLOCATION;
      }
      if(err == DT_HIP_SUCCESS) err = raw_group_launch(devid, r, cur.ptr(), out, pv->journal.ptr());
    }
    else
    {
      dt_hip_piece_t p = first.piece;
      if(first.op == OP_RAWPREPARE)
      {
        dt_hip_rawprepare_data_t d = *first.as<dt_hip_rawprepare_data_t>();
        band_rawprepare(p, d, b);
        err = dt_hip_iop_rawprepare_process(devid, &p, &d, cur.ptr(), out);
      }
      else if(first.op == OP_TEMPERATURE)
      {
        band_piece(p, b);
        err = dt_hip_iop_temperature_process(devid, &p, first.as<dt_hip_temperature_data_t>(), cur.ptr(), out);
      }
      else
      {
        band_piece(p, b);
        pv->journal = dev_buf_t::alloc(devid, DT_HIP_HIGHLIGHTS_JOURNAL_BYTES);
        pv->hl_out = out;
        if(!pv->journal) err = DT_HIP_SYSMEM_ALLOCATION;
        else err = dt_hip_iop_highlights_process_deferred(devid, &p, first.as<dt_hip_highlights_data_t>(), cur.ptr(), out, pv->journal.ptr());
      }
    }
    cur = std::move(buf); // releases the stage's input: stream-ordered
  }
  if(err == DT_HIP_SUCCESS && n_cfa == 0 && has_demosaic)
  {
    // the pipe starts at demosaic: stage the band's mosaic rows into the halo layout
    dev_buf_t buf = dev_buf_t::alloc(devid, halo_rows * row_bytes);
    if(!buf) err = DT_HIP_SYSMEM_ALLOCATION;
    else
    {
      err = dt_hip_enqueue_copy_buffer_to_buffer(devid, cur.ptr(), buf.base(), 0, (size_t)b.halo_top * row_bytes, (size_t)b.rows * row_bytes);
      cur = std::move(buf);
    }
  }
  if(err != DT_HIP_SUCCESS)
  {
    delete pv;
    return err;
  }
  state->halo_buf = (has_demosaic && cur.owned()) ? cur.base() : nullptr;
  state->row_bytes = row_bytes;
  state->clipped_count = pv->journal.ptr();
  state->priv = pv;
  pv->cur = std::move(cur);
  pv->next_group = n_cfa;
  return DT_HIP_SUCCESS;
}

int dt_hip_pipe_band_resolve(dt_hip_pipe_t *pipe, const dt_hip_band_t *band, dt_hip_band_state_t *state)
{
  if(!pipe || !band || !state || !state->priv) return DT_HIP_INVALID_ARG;
  band_priv_t *pv = (band_priv_t *)state->priv;
  int err = DT_HIP_SUCCESS;
  if(pv->journal)
  {
    // must precede the halo exchange: the neighbours read these rows after the bypass decision
    err = dt_hip_iop_highlights_resolve(pipe->devid, pv->hl_out, pv->journal.ptr());
    pv->journal.release();
    state->clipped_count = nullptr;
  }
  return err;
}

// ---- one frame over the devices of ONE process (BASELINE.json config 4 from C) ----------------------------------
// The reference is a single C process (src/develop/pixelpipe_hb.c:1470): it cannot run one rank per GPU under a
// launcher, so the band walk of section 3b is also driven from inside the library -- one host thread per band (a
// module's launch code may block on ITS device, e.g. the patch table upload of the non-local means; with a thread
// per device the others keep enqueueing), the bands in lockstep at the exchange points, the collectives as peer
// copies over xGMI:
//   * the clipped count of the highlights bypass: 8 bytes per band through the host, summed in band order (integers);
//   * halo rows: each band PULLS the rows it needs from its neighbours' buffers (hipMemcpyPeerAsync on its own
//     stream), after every band has finished the step that produces them and before any band goes on;
//   * the profiled wavelets' table of partial sums: every entry is non-zero in exactly one band's table (the band
//     that owns the row), so the all-reduce is an all-gather of row segments -- one strided peer copy per
//     neighbour and band, exact by construction (x + 0 + ... + 0), no arithmetic at all.
// Bands may share a device (the single-GPU test of this path): a peer copy is then a device copy.
namespace
{
// What the bands of one walk share.  A band publishes POINTS: a hipEvent recorded on its stream behind the work the
// point stands for, and a counter the other bands' host threads watch.  Somebody who needs that work waits on the HOST
// only until the event has been recorded (the owner's thread got that far enqueueing), then makes ITS stream wait for
// the event: no stream is ever drained inside the walk, and a band only waits for the bands it reads from (its two
// neighbours at a halo stop).  Every band passes the same points in the same order (same node list).
struct band_gang_t
{
  int n = 0;
  std::mutex m;
  std::condition_variable cv;
  std::vector<int> posted;                    // points band k has published
  std::vector<std::vector<hipEvent_t>> events; // [band][point]
  std::vector<int> done;                      // the band's walk has ended (its posted count is final)
  bool failed = false;
  // the classic meeting, used once per frame for the 8-byte clipped count that travels through the host
  int waiting = 0;
  unsigned long generation = 0;
  // statistics of the last walk (dt_hip_pipe_bands_stats())
  std::atomic<unsigned long long> peer_bytes{ 0 }, peer_copies{ 0 }, host_wait_ns{ 0 };

  void meet()
  {
    std::unique_lock<std::mutex> lk(m);
    const unsigned long g = generation;
    if(++waiting == n)
    {
      waiting = 0;
      generation++;
      cv.notify_all();
    }
    else
      cv.wait(lk, [&] { return generation != g; });
  }
  // band k: "everything enqueued on `s` so far is point number posted[k]"
  bool publish(const int k, hipStream_t s)
  {
    hipEvent_t e = nullptr;
    if(hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess || hipEventRecord(e, s) != hipSuccess)
    {
      (void)hipGetLastError();
      if(e) (void)hipEventDestroy(e);
      fail();
      return false;
    }
    std::lock_guard<std::mutex> lk(m);
    events[k].push_back(e);
    posted[k]++;
    cv.notify_all();
    return true;
  }
  // make stream `s` wait for point `pt` of band j; false when the walk has failed or band j will never get there
  bool await(const int j, const int pt, hipStream_t s)
  {
    hipEvent_t e = nullptr;
    {
      const auto t0 = std::chrono::steady_clock::now();
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [&] { return failed || posted[j] > pt || done[j]; });
      host_wait_ns += (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
      if(failed || posted[j] <= pt) return false;
      e = events[j][pt];
    }
    if(hipStreamWaitEvent(s, e, 0) != hipSuccess)
    {
      (void)hipGetLastError();
      fail();
      return false;
    }
    return true;
  }
  void fail()
  {
    std::lock_guard<std::mutex> lk(m);
    failed = true;
    cv.notify_all();
  }
  void finished(const int k)
  {
    std::lock_guard<std::mutex> lk(m);
    done[k] = 1;
    cv.notify_all();
  }
  bool has_failed()
  {
    std::lock_guard<std::mutex> lk(m);
    return failed;
  }
};

dt_hip_band_stats_t g_band_stats = { 0, 0, 0, 0, 0, 0, 0 };
std::mutex g_band_stats_mutex;

static int copy_between(band_gang_t &gang, const int dst_devid, void *dst, const int src_devid, const void *src, const size_t bytes,
                 hipStream_t s)
{
  if(!bytes) return DT_HIP_SUCCESS;
  const int dd = hip_device_of(dst_devid), sd = hip_device_of(src_devid);
  if(dd == sd) ANSEL_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  else
  {
    ANSEL_HIP_CHECK(hipMemcpyPeerAsync(dst, dd, src, sd, bytes, s));
    gang.peer_bytes += bytes;
    gang.peer_copies++;
  }
  return DT_HIP_SUCCESS;
}
} // namespace

void dt_hip_pipe_bands_stats(dt_hip_band_stats_t *out)
{
  if(!out) return;
  std::lock_guard<std::mutex> lk(g_band_stats_mutex);
  *out = g_band_stats;
}

// Can the devices of a band walk reach each other?  Checks hipDeviceCanAccessPeer for every ordered pair, enables the
// access, and moves a small buffer device to device and back with a cross-device event in between -- the three things
// dt_hip_pipe_process_bands() relies on and a single-GPU box never executes.  0, or an error with the pair in the text.
int dt_hip_peer_selftest(const int *devids, int n)
{
  if(!devids || n < 1) return DT_HIP_INVALID_ARG;
  for(int i = 0; i < n; i++)
    if(!valid_device(devids[i])) return DT_HIP_INVALID_ARG;
  for(int i = 0; i < n; i++)
    for(int j = 0; j < n; j++)
    {
      const int di = hip_device_of(devids[i]), dj = hip_device_of(devids[j]);
      if(di == dj) continue;
      int can = 0;
      if(hipDeviceCanAccessPeer(&can, di, dj) != hipSuccess || !can)
      {
        (void)hipGetLastError();
        set_last_error("peer self-test: device %d cannot access device %d (hipDeviceCanAccessPeer): halo rows would travel "
                       "through the host", devids[i], devids[j]);
        return DT_HIP_DEFAULT_ERROR;
      }
      (void)stream_of(devids[i]); // makes device i current
      const hipError_t e = hipDeviceEnablePeerAccess(dj, 0);
      if(e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
      {
        (void)hipGetLastError();
        set_last_error("peer self-test: hipDeviceEnablePeerAccess(%d -> %d): %s", devids[i], devids[j], hipGetErrorString(e));
        return DT_HIP_DEFAULT_ERROR;
      }
      (void)hipGetLastError();
    }
  // every ORDERED pair (a, b): a's pattern travels to b behind an event of a's stream -- dt_hip_pipe_process_bands() pulls halo
  // rows from both neighbours, the bilateral grid from the last band to every band, the wavelets' sums from every band to every
  // band -- once as a linear peer copy and once as the strided hipMemcpy2DAsync(hipMemcpyDefault) the sums' all-gather uses
  const size_t N = 1 << 16;
  std::vector<unsigned> pattern(N), back(N);
  for(int pair = 0; pair < (n == 1 ? 1 : n * n); pair++)
  {
    const int ka = n == 1 ? 0 : pair / n, kb = n == 1 ? 0 : pair % n;
    if(n > 1 && ka == kb) continue;
    const int k = pair;
    const int a = devids[ka], b = devids[kb];
    for(size_t i = 0; i < N; i++) pattern[i] = (unsigned)(i * 2654435761u + (unsigned)k);
    const dev_buf_t da_buf = dev_buf_t::alloc(a, N * 4), db_buf = dev_buf_t::alloc(b, N * 4);
    unsigned *const da = da_buf.as<unsigned>(), *const db = db_buf.as<unsigned>();
    int err = (da && db) ? DT_HIP_SUCCESS : DT_HIP_SYSMEM_ALLOCATION;
    hipEvent_t ev = nullptr;
    if(err == DT_HIP_SUCCESS)
    {
      hipStream_t sa = stream_of(a);
      if(hipMemcpyAsync(da, pattern.data(), N * 4, hipMemcpyHostToDevice, sa) != hipSuccess
         || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, sa) != hipSuccess)
        err = DT_HIP_DEFAULT_ERROR;
      hipStream_t sb = stream_of(b);
      if(err == DT_HIP_SUCCESS
         && (hipStreamWaitEvent(sb, ev, 0) != hipSuccess
             || (hip_device_of(a) == hip_device_of(b) ? hipMemcpyAsync(db, da, N * 4, hipMemcpyDeviceToDevice, sb)
                                                      : hipMemcpyPeerAsync(db, hip_device_of(b), da, hip_device_of(a), N * 4, sb))
                    != hipSuccess
             || hipMemcpyAsync(back.data(), db, N * 4, hipMemcpyDeviceToHost, sb) != hipSuccess
             || hipStreamSynchronize(sb) != hipSuccess))
        err = DT_HIP_DEFAULT_ERROR;
      if(err == DT_HIP_SUCCESS && memcmp(back.data(), pattern.data(), N * 4) != 0) err = DT_HIP_DEFAULT_ERROR;
      // the strided form: 64 rows of 256 words out of rows of 1024, kind Default (the runtime routes between the two memories)
      if(err == DT_HIP_SUCCESS
         && (hipMemsetAsync(db, 0, N * 4, sb) != hipSuccess
             || hipMemcpy2DAsync(db + 128, 1024 * 4, da + 128, 1024 * 4, 256 * 4, 64, hipMemcpyDefault, sb) != hipSuccess
             || hipMemcpyAsync(back.data(), db, N * 4, hipMemcpyDeviceToHost, sb) != hipSuccess
             || hipStreamSynchronize(sb) != hipSuccess))
        err = DT_HIP_DEFAULT_ERROR;
      for(size_t i = 0; err == DT_HIP_SUCCESS && i < N; i++)
      {
        const size_t col = i % 1024;
        if(back[i] != ((col >= 128 && col < 384) ? pattern[i] : 0u)) err = DT_HIP_DEFAULT_ERROR;
      }
      (void)hipStreamSynchronize(sa);
    }
    if(ev) (void)hipEventDestroy(ev);
    if(err != DT_HIP_SUCCESS)
    {
      (void)hipGetLastError();
      set_last_error("peer self-test: the copy device %d -> device %d behind a cross-device event did not arrive intact", a, b);
      return err;
    }
  }
  return DT_HIP_SUCCESS;
}

int dt_hip_pipe_process_bands(dt_hip_pipe_t *const *pipes, int n, const dt_hip_band_t *bands, const dt_hip_mem_t *dev_in,
                              const dt_hip_mem_t *dev_out)
{
  if(!pipes || n < 1 || n > 64 || !bands || !dev_in || !dev_out) return DT_HIP_INVALID_ARG;
  for(int k = 0; k < n; k++)
    if(!pipes[k] || !dev_in[k] || !dev_out[k] || pipes[k]->nodes.empty() || !valid_device(pipes[k]->devid)) return DT_HIP_INVALID_ARG;
  const int W = pipes[0]->nodes[0].piece.roi_out.width, H = pipes[0]->nodes[0].piece.roi_out.height;
  for(int k = 0; k < n; k++)
  {
    bool same = pipes[k]->nodes.size() == pipes[0]->nodes.size() && pipes[k]->nodes[0].piece.roi_out.width == W
                && pipes[k]->nodes[0].piece.roi_out.height == H;
    for(size_t i = 0; same && i < pipes[k]->nodes.size(); i++) same = pipes[k]->nodes[i].op == pipes[0]->nodes[i].op;
    if(!same)
    {
      set_last_error("dt_hip_pipe_process_bands: pipe %d does not hold the node list of pipe 0", k);
      return DT_HIP_INVALID_ARG;
    }
    if(bands[k].row0 != (k ? bands[k - 1].row0 + bands[k - 1].rows : 0) || (k + 1 == n && bands[k].row0 + bands[k].rows != H))
    {
      set_last_error("dt_hip_pipe_process_bands: the bands do not tile the %d rows of the frame", H);
      return DT_HIP_INVALID_ARG;
    }
  }
  // the mosaic halo is pulled out of the neighbour's OWN rows: a band thinner than it cannot serve it
  for(int k = 0; k < n; k++)
    if((k > 0 && bands[k].halo_top > bands[k - 1].rows) || (k + 1 < n && bands[k].halo_bottom > bands[k + 1].rows))
    {
      set_last_error("dt_hip_pipe_process_bands: band %d owns fewer rows than the mosaic halo its neighbour needs: use fewer bands", k);
      return DT_HIP_INVALID_ARG;
    }
  band_gang_t gang;
  gang.n = n;
  gang.posted.assign(n, 0);
  gang.done.assign(n, 0);
  gang.events.resize(n);
  std::vector<int> rcs(n, DT_HIP_SUCCESS);
  std::vector<dt_hip_band_state_t> st(n);
  std::vector<unsigned long long> counts(n, 0ull);
  std::vector<std::string> errors(n);
  std::atomic<int> peer_missing{ 0 }, stops{ 0 };
  for(auto &x : st) memset(&x, 0, sizeof(x));

  auto worker = [&](const int k) {
    dt_hip_pipe_t *const pipe = pipes[k];
    const int devid = pipe->devid;
    const dt_hip_band_t &b = bands[k];
    hipStream_t s = stream_of(devid); // also makes the device current for this thread
    // direct loads / stores between the devices of the gang.  A pair without peer access still works (the runtime
    // stages the copies through the host) but not at xGMI speed: counted, reported by dt_hip_pipe_bands_stats()
    for(int j = 0; j < n; j++)
      if(hip_device_of(pipes[j]->devid) != hip_device_of(devid))
      {
        int can = 0;
        if(hipDeviceCanAccessPeer(&can, hip_device_of(devid), hip_device_of(pipes[j]->devid)) != hipSuccess || !can) peer_missing++;
        else
        {
          const hipError_t e = hipDeviceEnablePeerAccess(hip_device_of(pipes[j]->devid), 0);
          if(e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) peer_missing++;
        }
        (void)hipGetLastError();
      }
    bool walking = false; // the band state holds buffers that give_up() must free
    auto fail = [&](const int code, const char *what = nullptr) {
      rcs[k] = code;
      errors[k] = what ? what : dt_hip_last_error();
      gang.fail();
    };
    auto give_up = [&]() {
      // the failure is published (fail() before every give_up() that follows an error of this band) and the own stream drained
      // BEFORE the band's buffers go back to the pool: a healthy neighbour may have peer copies in flight that read them --
      // what they copy is discarded, but it must still be this band's memory -- and a fault stays attributed to this band
      (void)hipStreamSynchronize(s);
      if(walking) dt_hip_pipe_band_abort(pipe, &st[k]);
      walking = false;
      gang.finished(k);
    };
    auto await = [&](const int j, const int pt) -> bool {
      if(j == k) return true;
      if(!gang.await(j, pt, s))
      {
        if(rcs[k] >= 0) rcs[k] = DT_HIP_DEFAULT_ERROR, errors[k] = "another band failed";
        return false;
      }
      return true;
    };

    // 1. the CFA stages on the own rows
    int rc = dt_hip_pipe_band_begin(pipe, &b, dev_in[k], &st[k]);
    if(rc != DT_HIP_SUCCESS) fail(rc);
    else walking = true;
    if(rcs[k] >= 0 && st[k].clipped_count
       && (hipMemcpyAsync(&counts[k], st[k].clipped_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess
           || hipStreamSynchronize(s) != hipSuccess))
      fail(DT_HIP_DEFAULT_ERROR);
    gang.meet(); // the one meeting of the walk: eight bytes per band through the host (the CFA stages are short)
    if(gang.has_failed()) return give_up();
    // 2. the bypass of the highlight clipping is decided on the frame's count
    if(st[k].clipped_count)
    {
      unsigned long long total = 0;
      for(int j = 0; j < n; j++) total += counts[j];
      if(hipMemcpyAsync(st[k].clipped_count, &total, sizeof(total), hipMemcpyHostToDevice, s) != hipSuccess
         || hipStreamSynchronize(s) != hipSuccess) // `total` is a stack variable
        fail(DT_HIP_DEFAULT_ERROR);
    }
    if(rcs[k] >= 0 && (rc = dt_hip_pipe_band_resolve(pipe, &b, &st[k])) != DT_HIP_SUCCESS) fail(rc);
    if(rcs[k] < 0) return give_up();
    int pt = 0; // the next point this band publishes; the same number on every band at the same place of the walk
    // 3. mosaic rows the demosaic reads beyond the band: point 0 = "my CFA rows are final", point 1 = "I have pulled"
    if(st[k].halo_buf)
    {
      if(!gang.publish(k, s)) return fail(DT_HIP_DEFAULT_ERROR, "hipEventRecord"), give_up();
      char *const mine = (char *)st[k].halo_buf;
      const size_t rb = st[k].row_bytes;
      if(k > 0 && b.halo_top && st[k - 1].halo_buf)
      {
        if(!await(k - 1, pt)) return give_up();
        const dt_hip_band_t &ub = bands[k - 1];
        rc = copy_between(gang, devid, mine, pipes[k - 1]->devid,
                          (const char *)st[k - 1].halo_buf + (size_t)(ub.halo_top + ub.rows - b.halo_top) * rb,
                          (size_t)b.halo_top * rb, s);
        if(rc != DT_HIP_SUCCESS) return fail(rc), give_up();
      }
      if(k + 1 < n && b.halo_bottom && st[k + 1].halo_buf)
      {
        if(!await(k + 1, pt)) return give_up();
        const dt_hip_band_t &db = bands[k + 1];
        rc = copy_between(gang, devid, mine + (size_t)(b.halo_top + b.rows) * rb, pipes[k + 1]->devid,
                          (const char *)st[k + 1].halo_buf + (size_t)db.halo_top * rb, (size_t)b.halo_bottom * rb, s);
        if(rc != DT_HIP_SUCCESS) return fail(rc), give_up();
      }
      if(!gang.publish(k, s)) return fail(DT_HIP_DEFAULT_ERROR, "hipEventRecord"), give_up();
      // nobody frees or overwrites rows a neighbour is still pulling
      if((k > 0 && !await(k - 1, pt + 1)) || (k + 1 < n && !await(k + 1, pt + 1))) return give_up();
      pt += 2;
    }
    // 4. the walk, stopping where a stencil module needs its neighbours.  A stop is three points: "what the others
    //    read from me is written", "my turn of a relay is over", "I have pulled everything I need".
    for(;;)
    {
      rc = dt_hip_pipe_band_finish(pipe, &b, &st[k], dev_out[k]);
      if(rc < 0)
      {
        walking = false; // a finish() that failed has freed its state itself
        return fail(rc), give_up();
      }
      if(rc == DT_HIP_SUCCESS) break;
      stops++;
      if(!gang.publish(k, s)) return fail(DT_HIP_DEFAULT_ERROR, "hipEventRecord"), give_up();
      const bool everybody = st[k].relay_buf || (st[k].sum_buf && st[k].sum_planes > 0);
      if(st[k].relay_buf)
      {
        // local contrast: the bands splat their rows into the grid one after the other (the frame's pixel order), each
        // starting from the grid its predecessor left; the last band's grid is the frame's and goes to everybody
        if(k > 0)
        {
          if(!await(k - 1, pt + 1)) return give_up();
          if((rc = copy_between(gang, devid, st[k].relay_buf, pipes[k - 1]->devid, st[k - 1].relay_buf, st[k].relay_bytes, s)) != DT_HIP_SUCCESS)
            return fail(rc), give_up();
        }
        if((rc = dt_hip_pipe_band_relay(pipe, &b, &st[k])) != DT_HIP_SUCCESS) return fail(rc), give_up();
      }
      if(!gang.publish(k, s)) return fail(DT_HIP_DEFAULT_ERROR, "hipEventRecord"), give_up(); // point pt + 1
      if(st[k].relay_buf && k + 1 < n)
      {
        if(!await(n - 1, pt + 1)) return give_up();
        if((rc = copy_between(gang, devid, st[k].relay_buf, pipes[n - 1]->devid, st[n - 1].relay_buf, st[k].relay_bytes, s)) != DT_HIP_SUCCESS)
          return fail(rc), give_up();
      }
      if(st[k].sum_buf && st[k].sum_planes > 0)
      {
        const size_t plane = st[k].sum_count / (size_t)st[k].sum_planes, per_row = plane / (size_t)H;
        for(int j = 0; j < n; j++)
        {
          if(j == k) continue;
          if(!await(j, pt)) return give_up();
          const size_t off = (size_t)bands[j].row0 * per_row, len = (size_t)bands[j].rows * per_row;
          // kind Default: the runtime routes the strided copy between the two devices' memories (unified addressing)
          if(hipMemcpy2DAsync(st[k].sum_buf + off, plane * sizeof(double), st[j].sum_buf + off, plane * sizeof(double),
                              len * sizeof(double), (size_t)st[k].sum_planes, hipMemcpyDefault, s) != hipSuccess)
            return fail(DT_HIP_DEFAULT_ERROR), give_up();
          if(hip_device_of(pipes[j]->devid) != hip_device_of(devid))
          {
            gang.peer_bytes += len * sizeof(double) * (size_t)st[k].sum_planes;
            gang.peer_copies++;
          }
        }
      }
      if(st[k].halo_rows > 0 && st[k].halo_buf)
      {
        const int h = st[k].halo_rows;
        auto parts = [&](const int j, int &top, int &bottom) {
          top = std::min(h, bands[j].row0);
          bottom = std::min(h, H - bands[j].row0 - bands[j].rows);
        };
        int top, bottom;
        parts(k, top, bottom);
        char *const mine = (char *)st[k].halo_buf;
        const size_t rb = st[k].row_bytes;
        if((k > 0 && bands[k - 1].rows < top) || (k + 1 < n && bands[k + 1].rows < bottom))
          return fail(DT_HIP_INVALID_ARG, "dt_hip_pipe_process_bands: a band owns fewer rows than the halo its neighbour needs: use fewer bands"),
                 give_up();
        if(k > 0 && top)
        {
          int utop, ubot;
          parts(k - 1, utop, ubot);
          if(!await(k - 1, pt)) return give_up();
          rc = copy_between(gang, devid, mine, pipes[k - 1]->devid,
                            (const char *)st[k - 1].halo_buf + (size_t)(utop + bands[k - 1].rows - top) * rb, (size_t)top * rb, s);
          if(rc != DT_HIP_SUCCESS) return fail(rc), give_up();
        }
        if(k + 1 < n && bottom)
        {
          int dtop, dbot;
          parts(k + 1, dtop, dbot);
          if(!await(k + 1, pt)) return give_up();
          rc = copy_between(gang, devid, mine + (size_t)(top + b.rows) * rb, pipes[k + 1]->devid,
                            (const char *)st[k + 1].halo_buf + (size_t)dtop * rb, (size_t)bottom * rb, s);
          if(rc != DT_HIP_SUCCESS) return fail(rc), give_up();
        }
      }
      if(!gang.publish(k, s)) return fail(DT_HIP_DEFAULT_ERROR, "hipEventRecord"), give_up(); // point pt + 2
      // what the others pull from this band stays as it is until they have: the neighbours at a halo stop, everybody
      // where the table of sums or the grid travelled
      for(int j = 0; j < n; j++)
        if(j != k && (everybody || j == k - 1 || j == k + 1) && !await(j, pt + 2)) return give_up();
      pt += 3;
    }
    walking = false;
    if(hipStreamSynchronize(s) != hipSuccess)
    {
      (void)hipGetLastError();
      fail(DT_HIP_DEFAULT_ERROR, "the band's stream reported an error at the end of the walk");
    }
    gang.finished(k);
  };

  std::vector<std::thread> gangsters;
  gangsters.reserve(n);
  int started = 0;
  try
  {
    for(int k = 0; k < n; k++, started++) gangsters.emplace_back(worker, k);
  }
  catch(...)
  {
    // no thread for band `started`: the others must not wait for it at the meeting
    gang.fail();
    {
      std::lock_guard<std::mutex> lk(gang.m);
      gang.n = started;
      if(gang.waiting >= gang.n && gang.n > 0)
      {
        gang.waiting = 0;
        gang.generation++;
      }
      for(int k = started; k < n; k++) gang.done[k] = 1;
      gang.cv.notify_all();
    }
    for(int k = started; k < n; k++) rcs[k] = DT_HIP_DEFAULT_ERROR, errors[k] = "no host thread for this band";
  }
  for(auto &t : gangsters) t.join();
  for(auto &ev : gang.events)
    for(hipEvent_t e : ev) (void)hipEventDestroy(e);
  {
    std::lock_guard<std::mutex> lk(g_band_stats_mutex);
    g_band_stats.bands = n;
    int devs = 0;
    for(int k = 0; k < n; k++)
    {
      bool seen = false;
      for(int j = 0; j < k; j++) seen |= hip_device_of(pipes[j]->devid) == hip_device_of(pipes[k]->devid);
      devs += !seen;
    }
    g_band_stats.devices = devs;
    g_band_stats.exchange_stops = n ? stops.load() / n : 0;
    g_band_stats.peer_copies = gang.peer_copies.load();
    g_band_stats.peer_bytes = gang.peer_bytes.load();
    g_band_stats.host_wait_ns = gang.host_wait_ns.load();
    g_band_stats.pairs_without_peer_access = peer_missing.load();
  }
  for(int k = 0; k < n; k++)
    if(rcs[k] < 0 && errors[k] != "another band failed")
    {
      set_last_error("band %d of %d: %s", k, n, errors[k].c_str());
      return rcs[k];
    }
  for(int k = 0; k < n; k++)
    if(rcs[k] < 0)
    {
      set_last_error("band %d of %d: %s", k, n, errors[k].c_str());
      return rcs[k];
    }
  return DT_HIP_SUCCESS;
}

// Give up a band between dt_hip_pipe_band_begin() and the last dt_hip_pipe_band_finish(): frees what the state holds
void dt_hip_pipe_band_abort(dt_hip_pipe_t *pipe, dt_hip_band_state_t *state)
{
  if(!pipe || !state || !state->priv) return;
  delete(band_priv_t *)state->priv;
  memset(state, 0, sizeof(*state));
}

int dt_hip_band_halo_rows(const char *op, const dt_hip_piece_t *piece, const void *data, size_t data_size)
{
  if(!op || !piece) return -1;
  node_t n;
  if(make_node(n, "dt_hip_band_halo_rows", op, piece, data, data_size) != DT_HIP_SUCCESS) return -1;
  return band_halo_rows(n);
}

// The band's turn in a relay stop: its rows of the module input are accumulated on top of what relay_buf holds (the
// grid bands 0 .. k-1 left, copied in by the driver).
int dt_hip_pipe_band_relay(dt_hip_pipe_t *pipe, const dt_hip_band_t *band, dt_hip_band_state_t *state)
{
  if(!pipe || !band || !state || !state->priv) return DT_HIP_INVALID_ARG;
  band_priv_t *pv = (band_priv_t *)state->priv;
  if(!pv->walking || !pv->relay || pv->next_group >= pipe->groups.size())
  {
    set_last_error("dt_hip_pipe_band_relay: the band is not at a relay stop");
    return DT_HIP_INVALID_ARG;
  }
  const node_t &n = pipe->nodes[pipe->groups[pv->next_group].first];
  if(n.op != OP_BILAT || pv->stage != 1) return DT_HIP_INVALID_ARG;
  return bilat_band_splat(pipe->devid, &n.piece, n.as<dt_hip_bilat_data_t>(), pv->relay.ptr(), pv->cur.ptr(), band->row0, band->rows);
}

// Resumable: returns DT_HIP_BAND_EXCHANGE in front of a stencil module (fill the halo rows of state->halo_buf)
// and in the middle of the profiled wavelets (all-reduce state->sum_buf); the caller does what the state
// asks for and calls again with the same arguments.
int dt_hip_pipe_band_finish(dt_hip_pipe_t *pipe, const dt_hip_band_t *band, dt_hip_band_state_t *state,
                            dt_hip_mem_t dev_out_band)
{
  if(!pipe || !band || !state || !state->priv || !dev_out_band) return DT_HIP_INVALID_ARG;
  band_priv_t *pv = (band_priv_t *)state->priv;
  const int devid = pipe->devid;
  const dt_hip_band_t &b = *band;
  const size_t ng = pipe->groups.size();
  const int W = pipe->nodes[0].piece.roi_out.width, H = pipe->nodes[0].piece.roi_out.height;
  const size_t rgba_row = (size_t)W * 16;
  int err = DT_HIP_SUCCESS;
  state->halo_rows = 0;
  state->sum_buf = nullptr;
  state->sum_count = 0;
  state->sum_planes = 0;
  state->relay_buf = nullptr;
  state->relay_bytes = 0;
  if(!pv->walking)
  {
    if(pv->journal) err = dt_hip_pipe_band_resolve(pipe, band, state); // caller skipped the explicit step
    pv->walking = true;
    if(pv->next_group >= ng && err == DT_HIP_SUCCESS)
    {
      // CFA-only pipe: the result is the band buffer itself
      const node_t &last = pipe->nodes.back();
      err = dt_hip_enqueue_copy_buffer_to_buffer(devid, pv->cur.ptr(), dev_out_band, 0, 0,
                                                 (size_t)b.rows * last.piece.roi_out.width * 4);
    }
  }
  // the group's output: the caller's buffer, or `bytes` from the pool with the band's own rows `lead` bytes into them
  auto output_of = [&](const bool to_caller, const size_t bytes, const size_t lead) {
    return to_caller ? dev_buf_t::borrow(dev_out_band) : dev_buf_t::alloc(devid, bytes, lead);
  };
  // the current buffer stops being the module input: free it, or keep it for the blend that follows the module
  auto retire_cur = [&](const size_t gi) {
    if(pipe->is_blend_group(gi + 1)) pv->held = std::move(pv->cur);
    else pv->cur.release();
  };
  // rows a stencil group takes from the neighbours, clipped at the frame
  auto halo_of = [&](const size_t gi, int &top, int &bottom) {
    const int h = band_halo_rows(pipe->nodes[pipe->groups[gi].first]);
    top = h < b.row0 ? h : b.row0;
    bottom = h < H - (b.row0 + b.rows) ? h : H - (b.row0 + b.rows);
    return h;
  };
  while(pv->next_group < ng && err == DT_HIP_SUCCESS)
  {
    const size_t gi = pv->next_group;
    const group_t &g = pipe->groups[gi];
    const node_t &first = pipe->nodes[g.first];
    const node_t &last = pipe->nodes[g.first + g.count - 1];
    const bool final_group = pipe->is_final_group(gi);
    if(first.op == OP_BLEND)
    {
      // dt_develop_blend_process() after the module's process(), pixelpipe_cpu.c:137-228: in place in the output
      if(!pv->held)
      {
        set_last_error("pipe: a blend node needs the module it blends in front of it");
        err = DT_HIP_INVALID_ARG;
        break;
      }
      node_t n = first;
      band_piece(n.piece, b);
      dt_hip_blend_data_t bd = *n.as<dt_hip_blend_data_t>();
      // the host-rendered form mask is the FRAME's plane (every band's device holds it whole): the band reads its rows
      if(bd.form_mask) bd.form_mask = (dt_hip_mem_t)((float *)bd.form_mask + (size_t)b.row0 * first.piece.roi_out.width);
      err = dt_hip_develop_blend_process(devid, &n.piece, &bd, pv->held.ptr(), pv->cur.ptr());
      pv->held.release();
      pv->next_group++;
      continue;
    }
    if(g.kind == group_t::SINGLE && first.op == OP_BILAT)
    {
      // the bilateral grid: a relay stop (every band splats its rows in turn), then blur + slice of the own rows
      const dt_hip_bilat_data_t *d = first.as<dt_hip_bilat_data_t>();
      if(pv->stage == 0)
      {
        dt_hip_mem_t grid = nullptr;
        err = bilat_band_begin(devid, &first.piece, d, &grid, &pv->relay_bytes);
        pv->relay = dev_buf_t(grid, true);
        if(err != DT_HIP_SUCCESS) break;
        pv->stage = 1;
        state->relay_buf = pv->relay.ptr();
        state->relay_bytes = pv->relay_bytes;
        return DT_HIP_BAND_EXCHANGE;
      }
      dev_buf_t out = output_of(final_group, (size_t)b.rows * rgba_row, 0);
      if(!out)
      {
        err = DT_HIP_SYSMEM_ALLOCATION;
        break;
      }
      err = bilat_band_finish(devid, &first.piece, d, pv->relay.ptr(), pv->cur.ptr(), out.ptr(), b.row0, b.rows);
      pv->relay.release(); // stream-ordered
      if(err != DT_HIP_SUCCESS) break;
      retire_cur(gi);
      pv->cur = std::move(out);
      pv->stage = 0;
      pv->next_group++;
      continue;
    }
    if(g.kind == group_t::SINGLE && (k_ops[first.op].flags & OPF_STENCIL))
    {
      int top, bottom;
      const int h = halo_of(gi, top, bottom);
      const int buf_rows = top + b.rows + bottom;
      if(pv->stage == 0)
      {
        if(h < 0)
        {
          // the module does nothing on a frame this small (denoiseprofile.c:1325-1329): pass the rows through
          pv->stage = 3;
          continue;
        }
        if(!pv->cur_is_halo_layout)
        {
          // own rows into the middle of a [top][rows][bottom] buffer
          dev_buf_t hb = dev_buf_t::alloc(devid, (size_t)buf_rows * rgba_row, (size_t)top * rgba_row);
          if(!hb)
          {
            err = DT_HIP_SYSMEM_ALLOCATION;
            break;
          }
          err = dt_hip_enqueue_copy_buffer_to_buffer(devid, pv->cur.ptr(), hb.base(), 0, hb.offset(), (size_t)b.rows * rgba_row);
          pv->cur = std::move(hb);
          if(err != DT_HIP_SUCCESS) break;
        }
        pv->cur_is_halo_layout = false;
        pv->stage = 1;
        if(top || bottom)
        {
          state->halo_buf = pv->cur.base();
          state->row_bytes = rgba_row;
          state->halo_rows = h;
          return DT_HIP_BAND_EXCHANGE;
        }
      }
      if(pv->stage == 1)
      {
        // the module on the buffer.  diffuse and the wavelets run on it as on a frame of its own: every row whose
        // stencils stay inside the buffer or hit a real frame border is exact, and the halo covers the rest.
        // non-local means keeps the frame's chunk grid and stores own rows only.
        state->halo_buf = nullptr;
        band_view_t v;
        v.frame_h = H;
        v.buf_row0 = b.row0 - top;
        v.row0 = b.row0;
        v.row1 = b.row0 + b.rows;
        // only diffuse runs on the whole buffer and leaves its halo rows in the output
        const bool own_rows_out = first.op != OP_DIFFUSE;
        pv->out = output_of(own_rows_out && final_group, (size_t)(own_rows_out ? b.rows : buf_rows) * rgba_row,
                            own_rows_out ? 0 : (size_t)top * rgba_row);
        if(!pv->out)
        {
          err = DT_HIP_SYSMEM_ALLOCATION;
          break;
        }
        if(first.op == OP_NLMEANS)
          err = nlmeans_process_band(devid, &first.piece, first.as<dt_hip_nlmeans_data_t>(), &v, pv->cur.base(), pv->out.base());
        else if(first.op == OP_DIFFUSE)
        {
          dt_hip_piece_t p = first.piece;
          p.roi_in.height = p.roi_out.height = buf_rows;
          err = diffuse_process_rows(devid, &p, first.as<dt_hip_diffuse_data_t>(), v.buf_row0, pv->cur.base(), pv->out.base());
        }
        else
        {
          err = denoiseprofile_band_begin(devid, &first.piece, first.as<dt_hip_denoiseprofile_data_t>(), &v, buf_rows,
                                          pv->cur.base(), pv->out.base(), &pv->dn_job);
          if(err == DT_HIP_SUCCESS && pv->dn_job) pv->stage = 2; // wavelets: one decomposition per step below
        }
        if(err != DT_HIP_SUCCESS) break;
        if(pv->stage != 2) pv->stage = 3;
      }
      if(pv->stage == 2)
      {
        // the profiled wavelets: a decomposition, then the neighbours' rows of its coarse plane for the next one; after
        // the last, the frame-wide sums; then thresholds and synthesis
        int rc;
        do
        {
          dt_hip_mem_t hbuf = nullptr;
          int hrows = 0;
          double *sums = nullptr;
          size_t count = 0;
          rc = denoiseprofile_band_step(pv->dn_job, &hbuf, &hrows, &sums, &count);
          if(rc < 0)
          {
            pv->dn_job = nullptr; // freed by the failing step
            err = rc;
            break;
          }
          if(rc > 0 && b.rows < H)
          {
            state->halo_buf = hbuf;
            state->halo_rows = hrows;
            state->row_bytes = rgba_row;
            state->sum_buf = sums;
            state->sum_count = count;
            // planes of [frame rows][segments][4]: each band's own rows are the only non-zero entries of its table
            state->sum_planes = count ? (int32_t)(count / ((size_t)H * ((W + 255) / 256) * 4)) : 0;
            return DT_HIP_BAND_EXCHANGE;
          }
        } while(rc > 0);
        if(err != DT_HIP_SUCCESS) break;
        state->halo_buf = nullptr;
        err = denoiseprofile_band_finish(pv->dn_job, pv->out.base());
        pv->dn_job = nullptr;
        if(err != DT_HIP_SUCCESS) break;
        pv->stage = 3;
      }
      // stage 3: the module's output becomes the current buffer
      if(pv->out)
      {
        retire_cur(gi);
        pv->cur = std::move(pv->out);
      }
      if(final_group && pv->cur.ptr() != dev_out_band)
      {
        err = dt_hip_enqueue_copy_buffer_to_buffer(devid, pv->cur.base(), dev_out_band, pv->cur.offset(), 0, (size_t)b.rows * rgba_row);
        pv->cur = dev_buf_t::borrow(dev_out_band); // stream-ordered; a blend that closes the pipe then works in dev_out_band
      }
      pv->stage = 0;
      pv->next_group++;
      continue;
    }
    // demosaic and pointwise groups
    size_t bytes = 0, lead = 0;
    bool out_halo_layout = false;
    if(!final_group)
    {
      node_t sized = last;
      sized.piece.roi_out.height = b.rows;
      bytes = out_bytes(sized);
      const group_t &nx = pipe->groups[gi + 1];
      if(nx.kind == group_t::SINGLE && (k_ops[pipe->nodes[nx.first].op].flags & OPF_STENCIL) && bytes == (size_t)b.rows * rgba_row)
      {
        // the next group is a stencil: write the own rows where its halo layout wants them
        int top, bottom;
        if(halo_of(gi + 1, top, bottom) >= 0)
        {
          bytes = (size_t)(top + b.rows + bottom) * rgba_row;
          lead = (size_t)top * rgba_row;
          out_halo_layout = true;
        }
      }
    }
    dev_buf_t out = output_of(final_group, bytes, lead);
    if(!out)
    {
      err = DT_HIP_SYSMEM_ALLOCATION;
      break;
    }
    // (of the two modules leaves_unwritten_alpha() names only the demosaic comes here: check_band_mode() refuses the local
    // laplacian, bilat_band_supported(), so the stencil branches need no such clear)
    if(out.owned() && g.kind == group_t::SINGLE && pipe->leaves_unwritten_alpha(g.first)
       && hipMemsetAsync(out.base(), 0, bytes, stream_of(devid)) != hipSuccess)
    {
      err = DT_HIP_DEFAULT_ERROR;
      break;
    }
    if(first.op == OP_DEMOSAIC)
    {
      const dt_hip_demosaic_data_t *d = first.as<dt_hip_demosaic_data_t>();
      if(d->demosaicing_method != DT_HIP_DEMOSAIC_RCD && d->demosaicing_method != DT_HIP_DEMOSAIC_AMAZE)
      {
        set_last_error("band mode: only the RCD and AMaZE demosaics run on row bands");
        err = DT_HIP_INVALID_ARG;
      }
      else
      {
        rcd_band_t rb;
        rb.tv0 = b.tile_row0;
        rb.tv1 = b.tile_row1;
        rb.in_row0 = b.row0 - b.halo_top;
        rb.in_rows = b.halo_top + b.rows + b.halo_bottom;
        rb.out_row0 = b.row0;
        rb.out_rows = b.rows;
        err = dt_hip_iop_demosaic_process_band(devid, &first.piece, d, &rb, pv->cur.ptr(), out.ptr());
      }
    }
    else if(g.kind == group_t::RGB)
    {
      rgb_group_t r = g.rgb;
      r.height = b.rows;
      err = rgb_group_launch(devid, r, pv->cur.ptr(), out.ptr());
    }
    else
    {
      node_t n = first;
      band_piece(n.piece, b);
      err = run_single(devid, n, pv->cur.ptr(), out.ptr());
    }
    retire_cur(gi);
    pv->cur = std::move(out);
    pv->cur_is_halo_layout = out_halo_layout;
    pv->next_group++;
  }
  // the walk has ended, with the pipe's output in dev_out_band or with an error: the state holds nothing any more
  delete pv;
  state->priv = nullptr;
  state->halo_buf = nullptr;
  state->clipped_count = nullptr;
  return err;
}

} // extern "C"
