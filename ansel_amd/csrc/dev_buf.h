// dev_buf.h -- the handle of a device buffer: what the executor's walks and the host halves of the modules hold their
// scratch in.  Includes the C-ABI and nothing of HIP, so a host program can include it (tests/native/dev_buf_host.cpp).
// Not part of the C-ABI (that is include/ansel_hip.h).
#pragma once
#include <stddef.h>
#include "ansel_hip.h"

namespace ansel
{

// A device buffer: the allocation, the byte offset of the view into it that the launches read or write (a band's
// own rows inside a [halo][rows][halo] layout), and whether the handle owns the allocation.  An owned allocation goes back to
// the runtime's pool when the handle is released, assigned to or destroyed (stream-ordered: safe behind the launches that
// are enqueued); a borrowed one (the caller's dev_in / dev_out) is left alone.
class dev_buf_t
{
  dt_hip_mem_t base_ = nullptr;
  size_t offset_ = 0;
  bool owned_ = false;

public:
  dev_buf_t() = default;
  dev_buf_t(dt_hip_mem_t base, bool owned, size_t offset = 0) : base_(base), offset_(offset), owned_(owned) {}
  // from the pool; empty when the pool has nothing to give
  static dev_buf_t alloc(int devid, size_t bytes, size_t offset = 0) { return dev_buf_t(dt_hip_alloc_device_buffer(devid, bytes), true, offset); }
  static dev_buf_t borrow(dt_hip_mem_t base) { return dev_buf_t(base, false); }
  dev_buf_t(dev_buf_t &&o) noexcept : base_(o.base_), offset_(o.offset_), owned_(o.owned_) { o.base_ = nullptr; }
  dev_buf_t &operator=(dev_buf_t &&o) noexcept
  {
    if(this != &o)
    {
      release();
      base_ = o.base_, offset_ = o.offset_, owned_ = o.owned_;
      o.base_ = nullptr;
    }
    return *this;
  }
  dev_buf_t(const dev_buf_t &) = delete;
  dev_buf_t &operator=(const dev_buf_t &) = delete;
  ~dev_buf_t() { release(); }
  void release()
  {
    if(base_ && owned_) dt_hip_release_mem_object(base_);
    base_ = nullptr;
  }
  explicit operator bool() const { return base_ != nullptr; }
  bool owned() const { return base_ && owned_; }
  dt_hip_mem_t base() const { return base_; }
  size_t offset() const { return offset_; }
  dt_hip_mem_t ptr() const { return base_ ? (dt_hip_mem_t)((char *)base_ + offset_) : nullptr; }
  // ptr() as the typed pointer a kernel takes
  template <typename T> T *as() const { return (T *)ptr(); }
};

} // namespace ansel
