// dev_buf_host.cpp -- ansel::dev_buf_t (ansel_amd/csrc/dev_buf.h) on the host: the runtime's two entries are counting
// stubs over malloc / free here, and every case says how many blocks it took and gave back.  Exits non-zero unless every
// owned block was released exactly once and no borrowed one ever was (tests/test_dev_buf_host.py compiles and runs it).
#include "dev_buf.h"

#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <utility>

static std::map<void *, int> g_released; // block -> times released
static int g_allocs = 0, g_failures = 0;

extern "C" dt_hip_mem_t dt_hip_alloc_device_buffer(int, size_t size)
{
  if(size == 0) return nullptr; // as the runtime: nothing to give for nothing
  void *p = malloc(size);
  g_released[p] = 0;
  g_allocs++;
  return p;
}
extern "C" void dt_hip_release_mem_object(dt_hip_mem_t mem)
{
  if(!mem) return;
  const auto it = g_released.find(mem);
  if(it == g_released.end())
  {
    printf("FAIL: a block the stub never gave out was released (a borrowed one?)\n");
    g_failures++;
    return;
  }
  it->second++; // (the block itself is freed at the end of main(): no address comes round twice)
}

#define EXPECT(cond)                                         \
  do                                                         \
  {                                                          \
    if(!(cond))                                              \
    {                                                        \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_failures++;                                          \
    }                                                        \
  } while(0)

static int released(const void *p) { return g_released.at(const_cast<void *>(p)); }

using ansel::dev_buf_t;

int main()
{
  // alloc -> destroy
  void *a;
  {
    dev_buf_t b = dev_buf_t::alloc(0, 64);
    a = b.base();
    EXPECT(b && b.owned() && b.ptr() == a && b.offset() == 0 && released(a) == 0);
  }
  EXPECT(released(a) == 1);
  // move-construct: the source is empty, the block is released once, by the target
  {
    dev_buf_t b = dev_buf_t::alloc(0, 64);
    a = b.base();
    dev_buf_t c(std::move(b));
    EXPECT(!b && !b.owned() && b.ptr() == nullptr && c.base() == a && c.owned());
  }
  EXPECT(released(a) == 1);
  // move-assign over a live handle: what the target held goes at once, what it takes at its end
  void *first, *second;
  {
    dev_buf_t b = dev_buf_t::alloc(0, 64), c = dev_buf_t::alloc(0, 32);
    first = b.base(), second = c.base();
    b = std::move(c);
    EXPECT(released(first) == 1 && released(second) == 0 && b.base() == second && !c);
  }
  EXPECT(released(first) == 1 && released(second) == 1);
  // self-move-assign: nothing happens
  {
    dev_buf_t b = dev_buf_t::alloc(0, 64);
    a = b.base();
    dev_buf_t &same = b;
    b = std::move(same);
    EXPECT(b.base() == a && b.owned() && released(a) == 0);
  }
  EXPECT(released(a) == 1);
  // release() twice, then the destructor
  {
    dev_buf_t b = dev_buf_t::alloc(0, 64);
    a = b.base();
    b.release();
    EXPECT(!b && released(a) == 1);
    b.release();
    EXPECT(released(a) == 1);
  }
  EXPECT(released(a) == 1);
  // borrow(): never released, whichever way the handle goes
  {
    char mine[16];
    dev_buf_t b = dev_buf_t::borrow(mine);
    EXPECT(b && !b.owned() && b.ptr() == mine);
    dev_buf_t c = std::move(b);
    c.release();
    dev_buf_t d = dev_buf_t::borrow(mine), e = dev_buf_t::alloc(0, 8);
    a = e.base();
    e = std::move(d); // over an owned block: that one goes, the borrowed one stays
    EXPECT(released(a) == 1 && e.ptr() == mine && !e.owned());
  }
  // a zero-byte alloc is an empty handle
  {
    const int before = g_allocs;
    dev_buf_t b = dev_buf_t::alloc(0, 0);
    EXPECT(!b && !b.owned() && b.ptr() == nullptr && b.as<float>() == nullptr && g_allocs == before);
  }
  // as<T>() is ptr() cast: with the view's byte offset
  {
    dev_buf_t b = dev_buf_t::alloc(0, 64, 16);
    EXPECT(b.offset() == 16 && (char *)b.ptr() == (char *)b.base() + 16);
    EXPECT(b.as<float>() == (float *)b.base() + 4 && (const void *)b.as<const double>() == b.ptr());
  }
  // the ledger: every block the stub gave out came back exactly once
  for(const auto &kv : g_released)
  {
    if(kv.second != 1)
    {
      printf("FAIL: a block was released %d times\n", kv.second);
      g_failures++;
    }
    free(kv.first);
  }
  EXPECT(g_allocs == (int)g_released.size() && g_allocs == 8);
  if(g_failures) return 1;
  printf("dev_buf_host ok: %d blocks, each released once\n", g_allocs);
  return 0;
}
