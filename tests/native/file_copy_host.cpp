// tests/native/file_copy_host.cpp -- TEST INFRASTRUCTURE: the body of the trimmed file download
// (ansel_amd/csrc/file_copy_body.h, run by file_to_host of file_copy.hip on gfx950) compiled for the host, its lanes run
// one after the other, with every store counted per destination byte.  tests/test_file_copy_host.py judges what it leaves
// in the destination; tests/test_gpu_file_copy.py checks that the device leaves the same bytes in pinned memory.
//
//   g++ -O2 -std=c++17 -fPIC -shared -I ansel_amd/csrc tests/native/file_copy_host.cpp -o libfile_copy_host.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DFILE_COPY_HOST_MAIN -I ansel_amd/csrc \
//       tests/native/file_copy_host.cpp -o file_copy_host && ./file_copy_host      (a program of its own: the cases of
//       the Python test, source and destination sized exactly so that a read or store beyond them is an error)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

namespace
{
uint8_t *g_count = nullptr; // stores per destination byte (saturating)
uint64_t g_limit = 0;       // the destination's size: a store that leaves it is counted and not made
uint64_t g_outside = 0;

template <typename T> void counted_store(void *dst, const uint64_t off, const T &val)
{
  if(off > g_limit || sizeof(T) > g_limit - off)
  {
    g_outside++;
    return;
  }
  memcpy((uint8_t *)dst + off, &val, sizeof(T));
  for(size_t k = 0; k < sizeof(T); k++)
    if(g_count[off + k] != 255) g_count[off + k]++;
}
} // namespace

#define FC_STORE16(dst, off, val) counted_store(dst, off, val)
#define FC_STORE8(dst, off, val) counted_store<uint64_t>(dst, off, val)
#define FC_STORE1(dst, off, val) counted_store<uint8_t>(dst, off, val)
#include "file_copy_body.h"

extern "C" {

// a file buffer: the length word, then a byte pattern that depends on the position (and does not repeat every 256 bytes)
void fc_host_pattern(uint8_t *buf, uint64_t bytes, uint64_t word)
{
  for(uint64_t p = 8; p < bytes; p++) buf[p] = (uint8_t)(p * 131 + (p >> 8) * 17 + (p >> 16) * 5 + 7);
  if(bytes >= 8) memcpy(buf, &word, 8);
}

uint64_t fc_host_total(uint64_t word, uint64_t capacity, uint64_t host_bytes) { return fc_total(word, capacity, host_bytes); }
uint64_t fc_host_word_of(uint64_t word, uint64_t capacity) { return fc_host_word(word, capacity); }

// fc_copy() alone: dst[0, total) = src[0, total) by `lanes` lanes; counts: one byte per byte of dst_bytes, zeroed here.
// -> stores that would have left the destination
uint64_t fc_host_copy(uint8_t *dst, uint64_t dst_bytes, const uint8_t *src, uint64_t total, uint64_t lanes, uint8_t *counts)
{
  memset(counts, 0, dst_bytes);
  g_count = counts;
  g_limit = dst_bytes;
  g_outside = 0;
  for(uint64_t lane = 0; lane < lanes; lane++) fc_copy(dst, src, total, lane, lanes);
  return g_outside;
}

// the kernel: every lane's fc_file_to_host() in turn
uint64_t fc_host_run(uint8_t *dst, const uint8_t *src, uint64_t capacity, uint64_t host_bytes, uint64_t lanes, uint8_t *counts)
{
  memset(counts, 0, host_bytes);
  g_count = counts;
  g_limit = host_bytes;
  g_outside = 0;
  for(uint64_t lane = 0; lane < lanes; lane++) fc_file_to_host(dst, src, capacity, host_bytes, lane, lanes);
  return g_outside;
}

} // extern "C"

#ifdef FILE_COPY_HOST_MAIN
namespace
{
const uint64_t GUARD = 64;
uint64_t g_cases = 0;

#define REQUIRE(c)                                                                                                            \
  do                                                                                                                          \
  {                                                                                                                           \
    if(!(c))                                                                                                                  \
    {                                                                                                                         \
      printf("file_copy_host: %s fails: word %llx capacity %llu host_bytes %llu lanes %llu\n", #c, (unsigned long long)word, \
             (unsigned long long)capacity, (unsigned long long)host_bytes, (unsigned long long)lanes);                        \
      exit(1);                                                                                                                \
    }                                                                                                                         \
  } while(0)

// source and destination are allocations of exactly capacity and GUARD + host_bytes + GUARD bytes
void one_case(uint64_t word, uint64_t capacity, uint64_t host_bytes, uint64_t lanes)
{
  std::vector<uint8_t> src(capacity), dst(GUARD + host_bytes + GUARD, 0xA5), counts(host_bytes);
  fc_host_pattern(src.data(), capacity, word);
  // what the header promises, worked out without its functions
  const bool is_len = word != UINT64_MAX && word <= UINT64_MAX - 8 && 8 + word <= capacity;
  const uint64_t expected = (is_len && 8 + word <= host_bytes) ? 8 + word : 8;
  const uint64_t host_word = is_len ? word : UINT64_MAX;
  REQUIRE(fc_total(word, capacity, host_bytes) == expected);
  REQUIRE(fc_host_run(dst.data() + GUARD, src.data(), capacity, host_bytes, lanes, counts.data()) == 0);
  uint8_t *d = dst.data() + GUARD;
  uint64_t got;
  memcpy(&got, d, 8);
  REQUIRE(got == host_word);
  REQUIRE(memcmp(d + 8, src.data() + 8, expected - 8) == 0);
  for(uint64_t p = 0; p < host_bytes; p++) REQUIRE(counts[p] == (p < expected ? 1 : 0));
  for(uint64_t p = 0; p < GUARD; p++) REQUIRE(dst[p] == 0xA5 && dst[GUARD + host_bytes + p] == 0xA5);
  for(uint64_t p = expected; p < host_bytes; p++) REQUIRE(d[p] == 0xA5);
  g_cases++;
}
} // namespace

int main()
{
  std::vector<uint64_t> totals;
  for(uint64_t t = 8; t <= 49; t++) totals.push_back(t);
  for(int k = 6; k <= 22; k++)
    for(int e = -1; e <= 1; e++) totals.push_back(((uint64_t)1 << k) + e);
  const uint64_t lanes_of[4] = { 1, 64, 256, 256 * 16 };
  for(const uint64_t lanes : lanes_of)
    for(const uint64_t T : totals)
    {
      const uint64_t caps[3] = { T, T + 1, T - 1 }, hosts[3] = { T, T - 1, 8 };
      for(int c = 0; c < (T > 8 ? 3 : 2); c++)
        for(int h = 0; h < 3; h++)
        {
          if(hosts[h] < 8) continue; // T == 8: T - 1 is no host buffer
          one_case(T - 8, caps[c], hosts[h], lanes);
          // words that are no length: they cost no copy, so the large totals add nothing
          if(T > (1u << 12)) continue;
          one_case(UINT64_MAX, caps[c], hosts[h], lanes);
          one_case(UINT64_MAX - 7, caps[c], hosts[h], lanes);
          one_case((uint64_t)1 << 63, caps[c], hosts[h], lanes);
        }
    }
  printf("file_copy_host: %llu cases\n", (unsigned long long)g_cases);
  return 0;
}
#endif
