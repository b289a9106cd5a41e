// tests/native/jpeg_huff_host.cpp -- TEST INFRASTRUCTURE: the Huffman table builder of the JPEG encoder
// (ansel_amd/csrc/jpeg_huff.h, one wave per table on gfx950) compiled for the host with one lane, so that
// tests/test_jpeg_host.py can compare its tables with libjpeg's.
//
//   g++ -O2 -std=c++17 -fPIC -shared -I ansel_amd/csrc tests/native/jpeg_huff_host.cpp -o libjpeg_huff_host.so
#include "jpeg_huff.h"

extern "C" int jh_host_table(const int64_t *freq, uint8_t *bits, uint8_t *vals)
{
  static jh_work_t w;
  for(int i = 0; i < 256; i++) w.freq[i] = freq[i];
  return jh_gen_optimal_table(&w, 0, 1, [](uint64_t k) { return k; }, []() {}, bits, vals);
}

// jh_derive(): the code and length of every symbol
extern "C" void jh_host_derive(const uint8_t *bits, const uint8_t *vals, uint16_t *code, uint8_t *size)
{
  jh_derive(bits, vals, code, size);
}
