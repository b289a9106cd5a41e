/* tests/native/png_ref.c -- TEST INFRASTRUCTURE: libpng with the settings of Ansel's PNG writer
 * (src/imageio/format/png.c write_image(), as recalled: RGB, 8 or 16 bits, not interlaced, compression level 0..9 with
 * zlib's memory level 8, window bits 15 and the default strategy, libpng's default filter choice, 16-bit samples
 * swapped from the host's order), writing to memory; and a libpng reader for the files the encoder makes.
 *
 *   gcc -O2 -fPIC -shared -I<libpng include> png_ref.c -o libpng_ref.so -L<libpng lib> -lpng16 */
#include <png.h>
#include <stdlib.h>
#include <string.h>

typedef struct
{
  unsigned char *p;
  size_t n, cap;
} membuf_t;

static void mem_write(png_structp png, png_bytep data, png_size_t n)
{
  membuf_t *m = (membuf_t *)png_get_io_ptr(png);
  if(m->n + n > m->cap)
  {
    m->cap = 2 * (m->n + n);
    m->p = (unsigned char *)realloc(m->p, m->cap);
  }
  memcpy(m->p + m->n, data, n);
  m->n += n;
}

static void mem_flush(png_structp png) { (void)png; }

static void quiet(png_structp png, png_const_charp msg) { (void)png; (void)msg; }

/* rgb: h rows of w RGB samples, uint8 or native uint16.  Returns the file length (0: failure); ref_free() it. */
size_t ref_write(const void *rgb, int w, int h, int depth, int level, unsigned char **out)
{
  membuf_t m = { 0, 0, 0 };
  png_structp png = png_create_write_struct(PNG_LIBPNG_VER_STRING, NULL, NULL, quiet);
  png_infop info = png_create_info_struct(png);
  if(setjmp(png_jmpbuf(png)))
  {
    png_destroy_write_struct(&png, &info);
    free(m.p);
    return 0;
  }
  png_set_write_fn(png, &m, mem_write, mem_flush);
  png_set_compression_level(png, level);
  png_set_compression_mem_level(png, 8);
  png_set_compression_strategy(png, 0);
  png_set_compression_window_bits(png, 15);
  png_set_IHDR(png, info, w, h, depth, PNG_COLOR_TYPE_RGB, PNG_INTERLACE_NONE, PNG_COMPRESSION_TYPE_BASE,
               PNG_FILTER_TYPE_BASE);
  png_write_info(png, info);
  if(depth == 16) png_set_swap(png);
  const size_t rb = (size_t)w * 3 * (depth / 8);
  for(int y = 0; y < h; y++) png_write_row(png, (png_const_bytep)rgb + (size_t)y * rb);
  png_write_end(png, info);
  png_destroy_write_struct(&png, &info);
  *out = m.p;
  return m.n;
}

void ref_free(unsigned char *p) { free(p); }

typedef struct
{
  const unsigned char *p;
  size_t n, at;
} memsrc_t;

static void mem_read(png_structp png, png_bytep data, png_size_t n)
{
  memsrc_t *m = (memsrc_t *)png_get_io_ptr(png);
  if(m->at + n > m->n) png_error(png, "read past the end");
  memcpy(data, m->p + m->at, n);
  m->at += n;
}

/* decode a file into rgb (h rows of w RGB samples, uint8 or native uint16); returns 0, or -1 if libpng refuses it or
 * its header is not w x h x depth RGB.  *icc_bytes: the size of the iCCP profile libpng read (0: none), *ppm: pHYs. */
int ref_read(const unsigned char *data, size_t n, int w, int h, int depth, void *rgb, unsigned *icc_bytes,
             unsigned *ppm)
{
  memsrc_t m = { data, n, 0 };
  png_structp png = png_create_read_struct(PNG_LIBPNG_VER_STRING, NULL, NULL, quiet);
  png_infop info = png_create_info_struct(png);
  if(setjmp(png_jmpbuf(png)))
  {
    png_destroy_read_struct(&png, &info, NULL);
    return -1;
  }
  png_set_read_fn(png, &m, mem_read);
  png_set_benign_errors(png, 1);
  /* the tests' profiles are random bytes: keep libpng from judging them as colour profiles */
  png_set_option(png, PNG_SKIP_sRGB_CHECK_PROFILE, PNG_OPTION_ON);
  png_read_info(png, info);
  png_uint_32 W, H;
  int bd, ct, il, cm, fm;
  png_get_IHDR(png, info, &W, &H, &bd, &ct, &il, &cm, &fm);
  if((int)W != w || (int)H != h || bd != depth || ct != PNG_COLOR_TYPE_RGB || il != PNG_INTERLACE_NONE)
  {
    png_destroy_read_struct(&png, &info, NULL);
    return -1;
  }
  png_charp name;
  int comp;
  png_bytep prof;
  png_uint_32 plen = 0;
  *icc_bytes = png_get_iCCP(png, info, &name, &comp, &prof, &plen) ? plen : 0;
  png_uint_32 rx = 0, ry = 0;
  int unit = 0;
  *ppm = png_get_pHYs(png, info, &rx, &ry, &unit) && unit == PNG_RESOLUTION_METER && rx == ry ? rx : 0;
  if(depth == 16) png_set_swap(png);
  const size_t rb = (size_t)w * 3 * (depth / 8);
  for(int y = 0; y < h; y++) png_read_row(png, (png_bytep)rgb + (size_t)y * rb, NULL);
  png_read_end(png, NULL);
  png_destroy_read_struct(&png, &info, NULL);
  return 0;
}
