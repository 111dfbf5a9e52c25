/* dj_jpeg_decode.h -- C ABI of the host half of decoding JPEG files to pixels on the GPU (host code, libdj_jpeg.so, beside
 * the reader of dj_jpeg.h, which stays as it is): the verdict whether the GPU half covers a file, and the batch reader that
 * writes raw coefficient planes into one caller-owned (pinned) buffer.  Conventions as in dj_jpeg.h: 0 or a negative code,
 * text via dj_jpeg_last_error() (thread-local), thread-safe. */
#ifndef DJ_JPEG_DECODE_H
#define DJ_JPEG_DECODE_H

#include "dj_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- For reconstructing the pixels from the coefficients (data/jpeg_pixels.py states it, csrc/dj_jpegpix.hip runs it on
 * the GPU).  dj_jpeg_read_decode_info reports what dj_jpeg_read_info reports plus what libjpeg decides the colour space
 * from, and the verdict `device_decodable`: SOF0 / SOF1, 8-bit, every quantisation table present, and either one component
 * or three that libjpeg's rule calls YCbCr (a JFIF marker; else an Adobe marker whose transform is 1; else, with neither
 * marker, ids other than 'R','G','B') with luma sampled 1x1, 2x1 or 2x2 and both chroma components 1x1.  Everything else
 * (progressive, arithmetic, CMYK / YCCK, Adobe RGB, 4:4:0, other factors) is simply not decodable there. */
typedef struct dj_jpeg_decode_info {
  dj_jpeg_info base;
  int component_id[4];
  int saw_jfif;
  int saw_adobe, adobe_transform; /* the transform byte of the Adobe marker (0 without one) */
  int precision;                  /* sample precision of the frame header */
  int device_decodable;
} dj_jpeg_decode_info;
int dj_jpeg_read_decode_info(const unsigned char* data, long size, dj_jpeg_decode_info* info);

/* n files read by n_threads host threads to RAW (not de-quantised) int16 planes inside ONE caller-owned buffer of
 * buffer_bytes (e.g. a pinned staging blob): component c of file i goes to buffer + plane_offsets[4 * i + c] (an even byte
 * offset) as blocks_h * blocks_w * 64 values, of which plane_capacity[4 * i + c] are the caller's (checked, with the
 * offsets, before anything of that file is written; entries of absent components are not read).  status[i] = 0 or a
 * negative code per file: a file that fails leaves the others alone.  Unlike dj_jpeg_read_coefficients, which zero-fills
 * the tail of a scan that ends early as libjpeg does, this call fails every truncated file -- entropy-coded data that ends
 * before the last MCU or inside a marker, and a file without its end-of-image marker, so every proper prefix of a file --
 * because it stands where a decoder that refuses truncated files stood.  Each file's headers are parsed twice (first
 * alone, against the caller's planes, so that a hostile header allocates nothing), and each worker decodes into planes of
 * its own and copies the logical block grid to the caller's offsets.  Returns the number of files that failed (the text
 * of the first is in dj_jpeg_last_error()), or a negative code for a bad argument.  Worker planes are kept from call to
 * call, so the steady state allocates nothing proportional to an image. */
int dj_jpeg_read_raw_batch(const unsigned char* const* data, const long* sizes, int n, unsigned char* buffer,
                           long buffer_bytes, const long* plane_offsets, const long* plane_capacity, int* status,
                           int n_threads);

#ifdef __cplusplus
}
#endif

/* the pre-pass of entropy decoding on the GPU, kept in a header of its own */
#include "dj_jpeg_segments.h"

#endif
