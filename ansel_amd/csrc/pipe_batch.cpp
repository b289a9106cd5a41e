// pipe_batch.cpp -- a stream of frames through one pipe (include/ansel_hip.h section 3a): upload / kernels / download of
// consecutive frames overlap, and the format's writer runs on a host thread of its own.
#include "pipe_internal.h"

#include "file_copy_body.h"

#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace ansel;

extern "C" {

struct batch_slot_t
{
  dev_buf_t d_in, d_out; // back to the pool with the slot (dt_hip_batch_free())
  hipEvent_t up = nullptr, done = nullptr, down = nullptr;
  hipEvent_t kstart = nullptr; // in front of the frame's first kernel (timed with `done` and `down`: the upload policy below)
  bool in_flight = false;
  // with a writer: the frame's place in the stream, its host buffer, and what became of it (guarded by the batch's mutex)
  long seq = 0;
  void *host_out = nullptr;
  bool written = false;
  int write_err = 0;
  // file output (dt_hip_batch_set_file_output()): the upload between two timed events of its own, made when the mode is first
  // switched on; the length word the download left in host_out, read by whoever awaits `down` (the writer thread, or
  // dt_hip_batch_wait() without a writer); 8 + L of the last frame waited for, 0 before the first
  hipEvent_t fup0 = nullptr, fup1 = nullptr;
  uint64_t file_word = 0;
  size_t file_total = 0;
};

struct dt_hip_batch_t
{
  dt_hip_pipe_t *pipe;
  size_t in_bytes, out_bytes;
  hipStream_t s_up, s_down;
  std::vector<batch_slot_t> slots;
  int next;
  // who awaits a frame's upload -- the host (true) or the compute stream: decided from the frames that have completed
  // (dt_hip_batch_submit())
  bool host_awaits_upload;
  // the fourth leg: the format's write_image() of frame n on a host thread of its own while frames n + 1 ... are on the
  // device (imageio_core.c:965 runs it after the pipe, serially).  The thread takes the slots in submission order
  dt_hip_batch_writer_t writer;
  void *writer_user;
  long submitted;
  std::thread writer_thread;
  std::mutex mtx;
  std::condition_variable cv_job, cv_done;
  std::vector<int> jobs; // slots whose download is enqueued, oldest first
  bool quit;
  // file output: what every host_out holds; the download then moves the frame's length word and file (file_copy.hip) and not
  // out_bytes.  0: off -- nothing of the mode runs
  size_t file_bytes;
};

namespace
{
static uint64_t host_word(const void *host_out)
{
  uint64_t word;
  memcpy(&word, host_out, sizeof(word));
  return word;
}
// the word the download left says whether the file came with it (file_copy_body.h): a length that fits the host buffer
static bool file_arrived(const dt_hip_batch_t *b, const uint64_t word) { return fc_total(word, b->out_bytes, b->file_bytes) == 8 + word; }

static void batch_writer_loop(dt_hip_batch_t *b)
{
  (void)make_current(b->pipe->devid);
  for(;;)
  {
    int k;
    {
      std::unique_lock<std::mutex> lk(b->mtx);
      b->cv_job.wait(lk, [&] { return b->quit || !b->jobs.empty(); });
      if(b->jobs.empty()) return; // quit, and nothing left to write
      k = b->jobs.front();
      b->jobs.erase(b->jobs.begin());
    }
    batch_slot_t &sl = b->slots[k];
    int err = hipEventSynchronize(sl.down) == hipSuccess ? DT_HIP_SUCCESS : DT_HIP_DEFAULT_ERROR;
    if(err == DT_HIP_SUCCESS && b->file_bytes)
    {
      // (the mode changes between frames only, behind a drain: it is this frame's)
      const uint64_t word = host_word(sl.host_out);
      sl.file_word = word; // read by dt_hip_batch_wait() behind `written`
      if(!file_arrived(b, word)) err = DT_HIP_FILE_TOO_LARGE;
      else if(b->writer(b->writer_user, sl.seq, sl.host_out, (size_t)(8 + word)) != 0) err = DT_HIP_WRITER_FAILED;
    }
    else if(err == DT_HIP_SUCCESS && b->writer(b->writer_user, sl.seq, sl.host_out, b->out_bytes) != 0) err = DT_HIP_WRITER_FAILED;
    {
      std::lock_guard<std::mutex> lk(b->mtx);
      sl.write_err = err;
      sl.written = true;
    }
    b->cv_done.notify_all();
  }
}
} // namespace

dt_hip_batch_t *dt_hip_batch_new(dt_hip_pipe_t *pipe, int depth, size_t in_bytes, size_t out_bytes)
{
  if(!pipe || depth < 1 || depth > 8 || !in_bytes || !out_bytes) return nullptr;
  dt_hip_batch_t *b = new dt_hip_batch_t;
  b->pipe = pipe;
  b->in_bytes = in_bytes;
  b->out_bytes = out_bytes;
  b->next = 0;
  b->host_awaits_upload = false;
  b->writer = nullptr;
  b->writer_user = nullptr;
  b->submitted = 0;
  b->quit = false;
  b->file_bytes = 0;
  b->s_up = b->s_down = nullptr;
  if(!pipe->planned) pipe->plan();
  // streams and events belong to the device that is current when they are made: the pipe's, not whatever the
  // calling thread used last (hipEventRecord rejects an event of another device than its stream's)
  bool ok = make_current(pipe->devid) && hipStreamCreateWithFlags(&b->s_up, hipStreamNonBlocking) == hipSuccess
            && hipStreamCreateWithFlags(&b->s_down, hipStreamNonBlocking) == hipSuccess;
  for(int k = 0; k < depth && ok; k++)
  {
    batch_slot_t sl;
    sl.d_in = dev_buf_t::alloc(pipe->devid, in_bytes);
    sl.d_out = dev_buf_t::alloc(pipe->devid, out_bytes);
    ok = sl.d_in && sl.d_out && hipEventCreateWithFlags(&sl.up, hipEventDisableTiming) == hipSuccess
         && hipEventCreate(&sl.kstart) == hipSuccess && hipEventCreate(&sl.done) == hipSuccess && hipEventCreate(&sl.down) == hipSuccess;
    // a pipe that ends in a demosaic or the local laplacian leaves the fourth channel of its output to the buffer's owner, and
    // that is the batch: cleared once, no frame writes those words (dt_hip_pipe_t::leaves_unwritten_alpha())
    if(ok && pipe->output_keeps_the_callers_alpha()) ok = hipMemset(sl.d_out.ptr(), 0, out_bytes) == hipSuccess;
    b->slots.push_back(std::move(sl));
  }
  if(!ok)
  {
    set_last_error("dt_hip_batch_new: could not create %d slots of %zu + %zu bytes", depth, in_bytes, out_bytes);
    dt_hip_batch_free(b);
    return nullptr;
  }
  return b;
}

void dt_hip_batch_free(dt_hip_batch_t *b)
{
  if(!b) return;
  make_current(b->pipe->devid);
  dt_hip_batch_drain(b);
  if(b->writer_thread.joinable())
  {
    {
      std::lock_guard<std::mutex> lk(b->mtx);
      b->quit = true;
    }
    b->cv_job.notify_all();
    b->writer_thread.join();
  }
  // a submit that failed half way leaves its upload (or download) enqueued without marking the slot in flight:
  // the copy streams must be idle before the slot buffers go back to the pool (with `delete b`)
  if(b->s_up) (void)hipStreamSynchronize(b->s_up);
  if(b->s_down) (void)hipStreamSynchronize(b->s_down);
  for(batch_slot_t &sl : b->slots)
  {
    if(sl.up) (void)hipEventDestroy(sl.up);
    if(sl.kstart) (void)hipEventDestroy(sl.kstart);
    if(sl.done) (void)hipEventDestroy(sl.done);
    if(sl.down) (void)hipEventDestroy(sl.down);
    if(sl.fup0) (void)hipEventDestroy(sl.fup0);
    if(sl.fup1) (void)hipEventDestroy(sl.fup1);
  }
  if(b->s_up) (void)hipStreamDestroy(b->s_up);
  if(b->s_down) (void)hipStreamDestroy(b->s_down);
  delete b;
}

namespace
{
// Who awaits the NEXT frames' uploads.  A frame whose kernels take longer than its two transfers (the full pipe: 67 ms against 3.6 +
// 15 at 100 MP) wants the HOST to await the upload: with a stream-wait in front of the kernels AND the download's stream-wait behind
// them, the runtime ran the downloads beside the next frame's kernels at the sum of their times (79 - 83 ms a frame; 71 with the
// host awaiting -- tools/batch_sdma_probe.py, profiles/r06_batch_probe.txt).  A frame whose transfers are the longer leg (the light
// pipe: 5.7 ms of kernels) wants everything asynchronous: the host blocked on an upload cannot enqueue the next download (24.8
// against 16.3 ms a frame).  Measured per completed frame from the slot's events.
static void batch_update_policy(dt_hip_batch_t *b, batch_slot_t &sl)
{
  float kernels_ms = 0.0f, down_ms = 0.0f;
  if(hipEventElapsedTime(&kernels_ms, sl.kstart, sl.done) != hipSuccess || hipEventElapsedTime(&down_ms, sl.done, sl.down) != hipSuccess)
  {
    (void)hipGetLastError();
    return;
  }
  const float up_ms = down_ms * (float)((double)b->in_bytes / (double)b->out_bytes);
  b->host_awaits_upload = kernels_ms > up_ms + down_ms;
}

// The same decision in file mode.  The download moves the file and not out_bytes, so its time says nothing about the upload's:
// the upload is timed itself (the slot's fup0 / fup1 around it on s_up), and the kernels are compared with the two measured legs
static void batch_update_policy_files(dt_hip_batch_t *b, batch_slot_t &sl)
{
  float kernels_ms = 0.0f, down_ms = 0.0f, up_ms = 0.0f;
  if(hipEventElapsedTime(&kernels_ms, sl.kstart, sl.done) != hipSuccess || hipEventElapsedTime(&down_ms, sl.done, sl.down) != hipSuccess
     || hipEventElapsedTime(&up_ms, sl.fup0, sl.fup1) != hipSuccess)
  {
    (void)hipGetLastError();
    return;
  }
  b->host_awaits_upload = kernels_ms > up_ms + down_ms;
}

// file mode, the frame's download has landed and `word` is what it left: the slot's 8 + L, and the frame's code
static int batch_file_result(dt_hip_batch_t *b, batch_slot_t &sl, const uint64_t word, const int err)
{
  sl.file_total = word != FC_NO_FILE && word <= b->out_bytes - 8 ? (size_t)(8 + word) : 8;
  if(err != DT_HIP_FILE_TOO_LARGE) return err;
  if(word == FC_NO_FILE)
    set_last_error("dt_hip_batch_wait: frame %ld has no file: its length word is UINT64_MAX (the encoder refused the frame, or its file "
                   "does not fit the device buffer of %zu bytes); the host buffers hold %zu bytes",
                   sl.seq, b->out_bytes, b->file_bytes);
  else
    set_last_error("dt_hip_batch_wait: the file of frame %ld takes %zu bytes (8 + L) and the host buffers hold %zu "
                   "(dt_hip_batch_set_file_output); its host_out holds the length word alone",
                   sl.seq, sl.file_total, b->file_bytes);
  return err;
}
} // namespace

int dt_hip_batch_wait(dt_hip_batch_t *b, int slot)
{
  if(!b || slot < 0 || slot >= (int)b->slots.size()) return DT_HIP_INVALID_ARG;
  batch_slot_t &sl = b->slots[slot];
  if(!sl.in_flight) return DT_HIP_SUCCESS;
  if(b->writer)
  {
    // the frame is done when its writer has returned: only then may the caller reuse host_out
    std::unique_lock<std::mutex> lk(b->mtx);
    b->cv_done.wait(lk, [&] { return sl.written; });
    sl.in_flight = false;
    if(b->file_bytes)
    {
      if(sl.write_err == DT_HIP_SUCCESS) batch_update_policy_files(b, sl);
      if(sl.write_err != DT_HIP_DEFAULT_ERROR) (void)batch_file_result(b, sl, sl.file_word, sl.write_err);
    }
    else if(sl.write_err == DT_HIP_SUCCESS) batch_update_policy(b, sl);
    if(sl.write_err == DT_HIP_FILE_TOO_LARGE) return sl.write_err; // (batch_file_result() has said which frame and both sizes)
    if(sl.write_err == DT_HIP_WRITER_FAILED) set_last_error("dt_hip_batch_wait: the writer refused frame %ld", sl.seq);
    else if(sl.write_err != DT_HIP_SUCCESS)
      set_last_error("dt_hip_batch_wait: the download of frame %ld did not complete (hipEventSynchronize on the writer thread)", sl.seq);
    return sl.write_err;
  }
  ANSEL_HIP_CHECK(hipEventSynchronize(sl.down));
  sl.in_flight = false;
  if(b->file_bytes)
  {
    const uint64_t word = host_word(sl.host_out);
    const bool arrived = file_arrived(b, word);
    if(arrived) batch_update_policy_files(b, sl);
    return batch_file_result(b, sl, word, arrived ? DT_HIP_SUCCESS : DT_HIP_FILE_TOO_LARGE);
  }
  batch_update_policy(b, sl);
  return DT_HIP_SUCCESS;
}

int dt_hip_batch_set_file_output(dt_hip_batch_t *b, size_t host_bytes)
{
  if(!b) return DT_HIP_INVALID_ARG;
  // between frames only, as dt_hip_batch_set_writer()
  const int e = dt_hip_batch_drain(b);
  if(e != DT_HIP_SUCCESS) return e;
  if(!host_bytes)
  {
    b->file_bytes = 0;
    return DT_HIP_SUCCESS;
  }
  if(!b->pipe->output_is_a_file())
  {
    set_last_error("dt_hip_batch_set_file_output: the pipe's last node is %s, not export_jpeg, export_png, export_tiff or export_webp: "
                   "its output has no length word",
                   b->pipe->nodes.empty() ? "missing" : k_ops[b->pipe->nodes.back().op].name);
    return DT_HIP_INVALID_ARG;
  }
  if(host_bytes < 8 || host_bytes > b->out_bytes)
  {
    set_last_error("dt_hip_batch_set_file_output: host buffers of %zu bytes: at least the 8-byte length word, at most the batch's "
                   "out_bytes (%zu)",
                   host_bytes, b->out_bytes);
    return DT_HIP_INVALID_ARG;
  }
  if(!make_current(b->pipe->devid)) return DT_HIP_INVALID_ARG;
  for(batch_slot_t &sl : b->slots)
  {
    if(!sl.fup0) ANSEL_HIP_CHECK(hipEventCreate(&sl.fup0));
    if(!sl.fup1) ANSEL_HIP_CHECK(hipEventCreate(&sl.fup1));
  }
  b->file_bytes = host_bytes;
  // a slot's 8 + L is of a frame of this mode
  for(batch_slot_t &sl : b->slots) sl.file_total = 0;
  return DT_HIP_SUCCESS;
}

int dt_hip_batch_file_bytes(dt_hip_batch_t *b, int slot, size_t *bytes)
{
  if(!b || !bytes || slot < 0 || slot >= (int)b->slots.size()) return DT_HIP_INVALID_ARG;
  const batch_slot_t &sl = b->slots[slot];
  if(!b->file_bytes || sl.in_flight || !sl.file_total)
  {
    set_last_error("dt_hip_batch_file_bytes: %s", !b->file_bytes  ? "file output is off (dt_hip_batch_set_file_output)"
                                                  : sl.in_flight ? "the slot's frame has not been waited for"
                                                                 : "the slot has not held a frame");
    return DT_HIP_INVALID_ARG;
  }
  *bytes = sl.file_total;
  return DT_HIP_SUCCESS;
}

int dt_hip_batch_set_writer(dt_hip_batch_t *b, dt_hip_batch_writer_t writer, void *user)
{
  if(!b) return DT_HIP_INVALID_ARG;
  // between frames only: no slot may be in flight
  const int e = dt_hip_batch_drain(b);
  if(e != DT_HIP_SUCCESS) return e;
  b->writer = writer;
  b->writer_user = user;
  if(writer && !b->writer_thread.joinable())
  {
    // std::thread's constructor throws std::system_error when the system has no thread to give: not through a C boundary
    try
    {
      b->writer_thread = std::thread(batch_writer_loop, b);
    }
    catch(const std::exception &e)
    {
      b->writer = nullptr;
      b->writer_user = nullptr;
      set_last_error("dt_hip_batch_set_writer: cannot start the writer thread (%s)", e.what());
      return DT_HIP_DEFAULT_ERROR;
    }
  }
  return DT_HIP_SUCCESS;
}

int dt_hip_batch_drain(dt_hip_batch_t *b)
{
  if(!b) return DT_HIP_INVALID_ARG;
  int err = DT_HIP_SUCCESS;
  for(int k = 0; k < (int)b->slots.size(); k++)
  {
    const int e = dt_hip_batch_wait(b, k);
    if(e != DT_HIP_SUCCESS) err = e;
  }
  return err;
}

int dt_hip_batch_submit(dt_hip_batch_t *b, const void *host_in, void *host_out)
{
  if(!b || !host_in || !host_out) return DT_HIP_INVALID_ARG;
  const int k = b->next;
  batch_slot_t &sl = b->slots[k];
  // file mode: the download is a kernel that stores through the device view of host_out
  void *view = nullptr;
  if(b->file_bytes)
  {
    const int e = file_host_view("dt_hip_batch_submit", b->pipe->devid, host_out, b->file_bytes, &view);
    if(e != DT_HIP_SUCCESS) return e;
  }
  // the slot's previous frame must have left the device before its buffers are reused
  const int w = dt_hip_batch_wait(b, k);
  if(w != DT_HIP_SUCCESS)
  {
    // the failure belongs to the frame that held this slot, NOT to the one being submitted (which is not submitted):
    // the message says so, the slot is free again, and the caller may submit the same frame once more
    const std::string prev = dt_hip_last_error();
    set_last_error("dt_hip_batch_submit: the previous frame of slot %d failed (%s); the new frame was not submitted", k, prev.c_str());
    return w;
  }
  hipStream_t compute = stream_of(b->pipe->devid);
  if(b->file_bytes) ANSEL_HIP_CHECK(hipEventRecord(sl.fup0, b->s_up));
  ANSEL_HIP_CHECK(hipMemcpyAsync(sl.d_in.ptr(), host_in, b->in_bytes, hipMemcpyHostToDevice, b->s_up));
  if(b->file_bytes) ANSEL_HIP_CHECK(hipEventRecord(sl.fup1, b->s_up));
  ANSEL_HIP_CHECK(hipEventRecord(sl.up, b->s_up));
  if(b->host_awaits_upload) ANSEL_HIP_CHECK(hipEventSynchronize(sl.up)); // (batch_update_policy(): which, and why)
  else ANSEL_HIP_CHECK(hipStreamWaitEvent(compute, sl.up, 0));
  ANSEL_HIP_CHECK(hipEventRecord(sl.kstart, compute));
  const int err = dt_hip_pipe_process(b->pipe, sl.d_in.ptr(), sl.d_out.ptr());
  if(err != DT_HIP_SUCCESS) return err;
  ANSEL_HIP_CHECK(hipEventRecord(sl.done, compute));
  ANSEL_HIP_CHECK(hipStreamWaitEvent(b->s_down, sl.done, 0));
  if(b->file_bytes)
  {
    const int e = file_to_host_launch(b->s_down, sl.d_out.ptr(), b->out_bytes, view, b->file_bytes);
    if(e != DT_HIP_SUCCESS) return e;
  }
  else
    ANSEL_HIP_CHECK(hipMemcpyAsync(host_out, sl.d_out.ptr(), b->out_bytes, hipMemcpyDeviceToHost, b->s_down));
  ANSEL_HIP_CHECK(hipEventRecord(sl.down, b->s_down));
  sl.in_flight = true;
  if(!b->writer && b->file_bytes)
  {
    // dt_hip_batch_wait() reads the frame's length word from there
    sl.seq = b->submitted;
    sl.host_out = host_out;
  }
  if(b->writer)
  {
    {
      std::lock_guard<std::mutex> lk(b->mtx);
      sl.seq = b->submitted;
      sl.host_out = host_out;
      sl.written = false;
      sl.write_err = DT_HIP_SUCCESS;
      b->jobs.push_back(k);
    }
    b->cv_job.notify_one();
  }
  b->submitted++;
  b->next = (k + 1) % (int)b->slots.size();
  return k;
}

} // extern "C"
