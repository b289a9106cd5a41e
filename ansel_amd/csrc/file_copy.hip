// file_copy.hip -- the download of an exported file: the length word and the file, not the buffer's capacity
// (include/ansel_hip.h: dt_hip_read_file_to_host(); the batch's download leg in file mode, pipe_batch.cpp).
//
// The length exists on the device alone when the copy is enqueued, and waiting for it would put a host round trip into
// every frame: the copy is a kernel that reads the word where it is and stores the file through the device view of the
// pinned host buffer (file_copy_body.h, shared with the host twin of the tests).
#include "hip_common.h"
#include "file_copy_body.h"

#include <stdlib.h>

namespace ansel
{

// Workgroups of 256 lanes.  The kernel runs beside the next frame's compute kernels and is bound by the host link, so it
// takes as few compute units as reach the link's rate.  Measured on one MI355X (tools/bench_batch_files.py --groups, the
// measuring build reads the number from the environment), ms for the 29.2 MB JPEG / the 305 MB TIFF
// of a 100 MP frame: 8 workgroups 0.537 / 6.07, 16: 0.531 / 5.56, 32: 0.533 / 5.49, 64: 0.537 / 5.98, 128: 0.598 / 5.56,
// 256: 0.550 / 5.57 -- 54 - 55 GB/s from 16 on, the runtime's own copy of the same bytes 55 - 57.  16 it is; 64 and 256 gain
// nothing and take the compute units from the kernels beside
#define FC_GROUPS 16
#define FC_BLOCK 256

__global__ void __launch_bounds__(FC_BLOCK) file_to_host(void *__restrict__ host, const void *__restrict__ dev_file,
                                                         const uint64_t capacity, const uint64_t host_bytes)
{
  fc_file_to_host(host, dev_file, capacity, host_bytes, (uint64_t)blockIdx.x * FC_BLOCK + threadIdx.x, (uint64_t)gridDim.x * FC_BLOCK);
}

int file_host_view(const char *who, int devid, void *host, size_t host_bytes, void **view)
{
  if(!valid_device(devid))
  {
    set_last_error("%s: no device %d", who, devid);
    return DT_HIP_INVALID_ARG;
  }
  if(!host || host_bytes < 8)
  {
    set_last_error("%s: a host buffer of %zu bytes cannot hold the length word (8 bytes)", who, host ? host_bytes : (size_t)0);
    return DT_HIP_INVALID_ARG;
  }
  if(((uintptr_t)host & 15) != 0)
  {
    set_last_error("%s: the host buffer %p is not 16-byte aligned", who, host);
    return DT_HIP_INVALID_ARG;
  }
  // both ends: a pinned allocation shorter than host_bytes would have the kernel store beyond it
  if(!dt_hip_is_pinned_memory(host) || !dt_hip_is_pinned_memory((const char *)host + host_bytes - 1))
  {
    set_last_error("%s: the host buffer %p is not pinned over its %zu bytes (dt_hip_alloc_host_pinned)", who, host, host_bytes);
    return DT_HIP_INVALID_ARG;
  }
  make_current(devid);
  *view = nullptr;
  if(hipHostGetDevicePointer(view, host, 0) != hipSuccess || !*view)
  {
    (void)hipGetLastError();
    set_last_error("%s: the pinned host buffer %p has no device view on device %d", who, host, devid);
    return DT_HIP_INVALID_ARG;
  }
  return DT_HIP_SUCCESS;
}

int file_to_host_launch(hipStream_t s, const void *dev_file, size_t capacity, void *view, size_t host_bytes)
{
  unsigned groups = FC_GROUPS;
  if(const char *e = measuring_env("ANSEL_HIP_FILE_COPY_GROUPS"))
  {
    const int g = atoi(e);
    if(g >= 1 && g <= 4096) groups = (unsigned)g;
  }
  file_to_host<<<groups, FC_BLOCK, 0, s>>>(view, dev_file, (uint64_t)capacity, (uint64_t)host_bytes);
  return check_launch("file_to_host");
}

} // namespace ansel

using namespace ansel;

extern "C" int dt_hip_read_file_to_host(int devid, dt_hip_mem_t dev_file, size_t capacity, void *host, size_t host_bytes)
{
  static const char *who = "dt_hip_read_file_to_host";
  void *view = nullptr;
  const int err = file_host_view(who, devid, host, host_bytes, &view);
  if(err != DT_HIP_SUCCESS) return err;
  if(!dev_file || capacity < 8 || ((uintptr_t)dev_file & 15) != 0)
  {
    set_last_error("%s: the device buffer %p of %zu bytes is not a file buffer (16-byte aligned, at least the 8-byte length word)", who,
                   dev_file, capacity);
    return DT_HIP_INVALID_ARG;
  }
  hipStream_t s = stream_of(devid);
  launch_scope ls(devid, "file_to_host");
  return file_to_host_launch(s, dev_file, capacity, view, host_bytes);
}
