// Test harness (CPU only) for the two entry points behind the GPU pixel reconstruction: dj_jpeg_read_decode_info and
// dj_jpeg_read_raw_batch of csrc/dj_jpeg.cpp.  tests/test_jpeg_pixels_cpu.py compiles it together with dj_jpeg.cpp under
// -fsanitize=address,undefined and runs it on two small files.  For each file it feeds EVERY prefix length, and a few
// corrupted copies, to both entry points: the planes go into a heap buffer of exactly the size the complete file's header
// asks for, so a write past a plane's capacity is a heap overflow the sanitizer reports.  Each call reads two files (the
// candidate and the complete file) on two threads: the complete file must succeed whatever the candidate does.  Also
// checked: no proper prefix is accepted (the batch reader refuses truncated files), and a capacity one value short and an
// offset that leaves the buffer are refused for that file alone.
#include "../include/dj_jpeg_decode.h"
#include <cstdio>
#include <cstring>
#include <vector>

static std::vector<unsigned char> slurp(const char* path) {
  std::vector<unsigned char> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  unsigned char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

struct Layout {
  long offsets[8], caps[8], bytes;      // two files: the candidate's planes first, then the complete file's
};

static Layout layout_of(const dj_jpeg_info& info) {
  Layout l;
  memset(&l, 0, sizeof(l));
  long end = 0;
  for (int f = 0; f < 2; ++f)
    for (int c = 0; c < info.n_components; ++c) {
      l.offsets[4 * f + c] = end;
      l.caps[4 * f + c] = (long)info.blocks_h[c] * info.blocks_w[c] * 64;
      end += l.caps[4 * f + c] * 2;
    }
  l.bytes = end;
  return l;
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int i = 1; i < argc; ++i) {
    const std::vector<unsigned char> full = slurp(argv[i]);
    dj_jpeg_decode_info info;
    if (full.empty() || dj_jpeg_read_decode_info(full.data(), (long)full.size(), &info) != 0 || !info.device_decodable) {
      printf("%s: not a decodable file\n", argv[i]);
      ++bad;
      continue;
    }
    const Layout l = layout_of(info.base);
    std::vector<unsigned char> want((size_t)l.bytes), got((size_t)l.bytes);
    int status[2];
    {
      const unsigned char* datas[2] = {full.data(), full.data()};
      const long sizes[2] = {(long)full.size(), (long)full.size()};
      const int rc = dj_jpeg_read_raw_batch(datas, sizes, 2, want.data(), l.bytes, l.offsets, l.caps, status, 2);
      if (rc != 0 || status[0] || status[1]) {
        printf("%s: the complete file fails: rc=%d %s\n", argv[i], rc, dj_jpeg_last_error());
        ++bad;
        continue;
      }
    }
    // candidates: every prefix, then copies with one byte changed at positions spread over the file
    long tried = 0, accepted = 0, info_ok = 0;
    const long n_prefix = (long)full.size() - 1, n_corrupt = 64;
    for (long k = 0; k < n_prefix + n_corrupt; ++k) {
      std::vector<unsigned char> cand;      // a fresh heap block of exactly the candidate's size: over-reads are reports
      if (k < n_prefix) {
        cand.assign(full.begin(), full.begin() + (k + 1));
      } else {
        cand = full;
        const size_t pos = (size_t)(((k - n_prefix) * 2654435761UL) % full.size());
        cand[pos] ^= (unsigned char)(1u << ((k - n_prefix) % 8)) | 0x80;
      }
      dj_jpeg_decode_info ci;
      if (dj_jpeg_read_decode_info(cand.data(), (long)cand.size(), &ci) == 0) ++info_ok;
      const unsigned char* datas[2] = {cand.data(), full.data()};
      const long sizes[2] = {(long)cand.size(), (long)full.size()};
      memset(got.data(), 0, got.size());
      const int rc = dj_jpeg_read_raw_batch(datas, sizes, 2, got.data(), l.bytes, l.offsets, l.caps, status, 2);
      ++tried;
      if (status[0] == 0) ++accepted;
      if (status[0] == 0 && k < n_prefix) {      // every proper prefix is a truncated file
        printf("%s: the prefix of %ld bytes was accepted\n", argv[i], k + 1);
        ++bad;
      }
      const long second = l.offsets[4];
      if (rc != (status[0] != 0) || status[1] != 0 || memcmp(got.data() + second, want.data() + second, (size_t)(l.bytes - second))) {
        printf("%s: candidate %ld disturbed the complete file next to it (rc=%d status=%d,%d)\n", argv[i], k, rc, status[0],
               status[1]);
        ++bad;
      }
    }
    // a capacity one value short, and an offset that leaves the buffer: that file is refused, the other one is read
    for (int which = 0; which < 2; ++which) {
      Layout m = l;
      if (which == 0)
        m.caps[0] -= 1;
      else
        m.offsets[0] = l.bytes - 2;
      const unsigned char* datas[2] = {full.data(), full.data()};
      const long sizes[2] = {(long)full.size(), (long)full.size()};
      const int rc = dj_jpeg_read_raw_batch(datas, sizes, 2, got.data(), l.bytes, m.offsets, m.caps, status, 2);
      if (rc != 1 || status[0] == 0 || status[1] != 0) {
        printf("%s: short capacity / bad offset (%d) not refused: rc=%d status=%d,%d\n", argv[i], which, rc, status[0], status[1]);
        ++bad;
      }
    }
    printf("%s: tried=%ld accepted=%ld info_ok=%ld\n", argv[i], tried, accepted, info_ok);
  }
  printf("bad=%d\n", bad);
  return bad ? 1 : 0;
}
