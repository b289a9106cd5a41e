// file_copy_body.h -- the body of the trimmed download of an exported file (file_copy.hip), written once and compiled
// twice: the device kernel calls these functions from its threads, and tests/native/file_copy_host.cpp runs the same
// functions lane after lane on the host, where every store is counted.
//
// The four file encoders leave a little-endian uint64 length word L and L file bytes in a device buffer of `capacity`
// bytes.  The host wants 8 + L bytes of it and not the capacity, and L exists on the device alone when the copy is
// enqueued: so the copy is a kernel that reads the word where it is and stores through the device view of a pinned host
// buffer of `host_bytes` bytes.  What the host finds afterwards:
//   the word L and the L file bytes                when 8 + L <= min(capacity, host_bytes)
//   the word UINT64_MAX and nothing else           when the device word is UINT64_MAX (the encoder refused) or 8 + L
//                                                  does not fit the DEVICE buffer (the word cannot be a length)
//   the word L and nothing else                    when the file fits the device buffer and not the host's: the caller
//                                                  learns the size it needs
// Every byte behind what is written keeps what it held: no store beyond the total, no read-modify-write.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define FC_FN __host__ __device__ __forceinline__
#else
#define FC_FN inline
#endif

struct alignas(16) fc_v16_t
{
  uint32_t v[4];
};

// the three stores of the copy.  The host twin defines them before it includes this header, to count what each lane
// stores; both pointers are 16-byte aligned (the entry points check), so the 8- and 16-byte stores are aligned
#ifndef FC_STORE16
#define FC_STORE16(dst, off, val) (*(fc_v16_t *)((uint8_t *)(dst) + (off)) = (val))
#define FC_STORE8(dst, off, val) (*(uint64_t *)((uint8_t *)(dst) + (off)) = (val))
#define FC_STORE1(dst, off, val) (((uint8_t *)(dst))[off] = (val))
#endif

#define FC_NO_FILE UINT64_MAX

// bytes to move: 8 + word when that is a length both buffers hold, else 8 (the word alone).  `word <= lim - 8` says
// 8 + word <= lim without a sum that could wrap, so the result never exceeds min(capacity, host_bytes), whatever the word
// holds (both sizes are >= 8: the entry points check)
FC_FN uint64_t fc_total(const uint64_t word, const uint64_t capacity, const uint64_t host_bytes)
{
  const uint64_t lim = capacity < host_bytes ? capacity : host_bytes;
  return (word != FC_NO_FILE && lim >= 8 && word <= lim - 8) ? 8 + word : 8;
}

// the word the host reads when the file itself does not travel (fc_total() == 8): the length where it is one, so that the
// caller learns the size it needs, FC_NO_FILE where the device buffer cannot hold such a file
FC_FN uint64_t fc_host_word(const uint64_t word, const uint64_t capacity)
{
  return (word != FC_NO_FILE && capacity >= 8 && word <= capacity - 8) ? word : FC_NO_FILE;
}

// lane `lane` of `lanes`: its share of dst[0, total) = src[0, total).  Bytes [0, total & ~15) as 16-byte loads and
// stores, lane i taking words i, i + lanes, ... so that the stores of a wave are consecutive -- four of them in flight
// per lane while there are four to take; the last total & 15 bytes one byte a lane from the first lanes
FC_FN void fc_copy(void *dst, const void *src, const uint64_t total, const uint64_t lane, const uint64_t lanes)
{
  const fc_v16_t *s = (const fc_v16_t *)src;
  const uint64_t n16 = total >> 4;
  uint64_t i = lane;
  for(; n16 > 3 * lanes && i < n16 - 3 * lanes; i += 4 * lanes)
  {
    const fc_v16_t a = s[i], b = s[i + lanes], c = s[i + 2 * lanes], d = s[i + 3 * lanes];
    FC_STORE16(dst, i << 4, a);
    FC_STORE16(dst, (i + lanes) << 4, b);
    FC_STORE16(dst, (i + 2 * lanes) << 4, c);
    FC_STORE16(dst, (i + 3 * lanes) << 4, d);
  }
  for(; i < n16; i += lanes)
  {
    const fc_v16_t a = s[i];
    FC_STORE16(dst, i << 4, a);
  }
  const uint64_t base = n16 << 4;
  for(uint64_t j = base + lane; j < total; j += lanes) FC_STORE1(dst, j, ((const uint8_t *)src)[j]);
}

// the whole job of one lane of file_to_host: every lane reads the word itself (one uniform 8-byte load) and takes its
// share of the copy; where the file does not travel, the first lane stores the host's word and nobody stores anything else
FC_FN void fc_file_to_host(void *dst, const void *src, const uint64_t capacity, const uint64_t host_bytes, const uint64_t lane,
                           const uint64_t lanes)
{
  const uint64_t word = *(const uint64_t *)src;
  const uint64_t total = fc_total(word, capacity, host_bytes);
  if(total > 8) fc_copy(dst, src, total, lane, lanes);
  else if(lane == 0) FC_STORE8(dst, 0, fc_host_word(word, capacity));
}
