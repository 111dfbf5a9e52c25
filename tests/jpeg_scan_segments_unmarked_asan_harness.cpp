// Stand-alone driver of dj_jpeg_scan_segments_unmarked for a sanitizer build (tests/test_entropy_chunked_cpu.py compiles it
// with csrc/dj_jpeg.cpp under -fsanitize=address,undefined and runs it; the sanitizer never enters a Python process).
// For every file named on the command line: the whole file, every proper prefix, and single-byte changes (every position
// to 0xFF, 0x00, 0xD0, 0xD9 and one bit flipped), each scanned from a heap copy of exactly its size -- so that a read
// past the end is a report -- with a ranges array of exactly n_segments entries.  What an eligible verdict promises is
// checked: ranges ascending, inside the file, two marker bytes apart and followed by two more; a file without restart
// intervals is one segment of all its MCUs; and whatever dj_jpeg_scan_segments accepts comes back identical, info and
// ranges.  Prints "tried=N eligible=M unmarked=K bad=0" per file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/dj_jpeg_decode.h"

static long g_bad = 0, g_unmarked = 0;

static int scan(const std::vector<unsigned char>& bytes) {
  unsigned char* copy = (unsigned char*)malloc(bytes.size());      // exactly as large as the data
  memcpy(copy, bytes.data(), bytes.size());
  dj_jpeg_segment_info* info = (dj_jpeg_segment_info*)malloc(sizeof(dj_jpeg_segment_info));
  dj_jpeg_segment_info* old = (dj_jpeg_segment_info*)malloc(sizeof(dj_jpeg_segment_info));
  int eligible = 0;
  if (dj_jpeg_scan_segments_unmarked(copy, (long)bytes.size(), info, nullptr, 0) != 0) ++g_bad;
  if (dj_jpeg_scan_segments(copy, (long)bytes.size(), old, nullptr, 0) != 0) ++g_bad;
  if (old->entropy_decodable && !info->entropy_decodable) ++g_bad;
  if (info->entropy_decodable) {
    eligible = 1;
    const int n = info->n_segments;
    if (n < 1 || info->reason[0] || info->restart_interval < 1) ++g_bad;
    long* ranges = (long*)malloc(sizeof(long) * 2 * (size_t)n);
    if (dj_jpeg_scan_segments_unmarked(copy, (long)bytes.size(), info, ranges, n) != 0 || !info->entropy_decodable ||
        info->n_segments != n)
      ++g_bad;
    for (int s = 0; s < n; ++s) {
      if (ranges[2 * s] < 0 || ranges[2 * s] > ranges[2 * s + 1] || ranges[2 * s + 1] + 2 > (long)bytes.size()) ++g_bad;
      if (s && ranges[2 * s] != ranges[2 * s - 1] + 2) ++g_bad;
    }
    if (old->entropy_decodable) {      // identical output
      long* same = (long*)malloc(sizeof(long) * 2 * (size_t)n);
      if (dj_jpeg_scan_segments(copy, (long)bytes.size(), old, same, n) != 0 || memcmp(old, info, sizeof(*info)) != 0 ||
          memcmp(same, ranges, sizeof(long) * 2 * (size_t)n) != 0)
        ++g_bad;
      free(same);
    } else {      // a file without restart intervals: one segment of all its MCUs, closed by EOI
      ++g_unmarked;
      if (n != 1 || info->restart_interval != info->mcus_x * info->mcus_y) ++g_bad;
      if (copy[ranges[1]] != 0xFF || copy[ranges[1] + 1] != 0xD9) ++g_bad;
    }
    free(ranges);
  } else if (!info->reason[0] || info->n_segments != 0) {
    ++g_bad;      // a refusal names its reason
  }
  free(old);
  free(info);
  free(copy);
  return eligible;
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<unsigned char> data;
    unsigned char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + got);
    fclose(f);
    long tried = 0, eligible = 0;
    eligible += scan(data);
    ++tried;
    for (size_t n = 1; n < data.size(); ++n, ++tried) {
      std::vector<unsigned char> prefix(data.begin(), data.begin() + (long)n);
      if (scan(prefix)) ++g_bad;      // no proper prefix is eligible
    }
    const unsigned char values[4] = {0xFF, 0x00, 0xD0, 0xD9};
    for (size_t at = 0; at < data.size(); ++at) {
      std::vector<unsigned char> changed(data);
      for (int v = 0; v < 5; ++v, ++tried) {
        changed[at] = v < 4 ? values[v] : (unsigned char)(data[at] ^ (1u << (at & 7)));
        eligible += scan(changed);
      }
    }
    printf("%s: tried=%ld eligible=%ld unmarked=%ld bad=%ld\n", argv[a], tried, eligible, g_unmarked, g_bad);
  }
  return g_bad ? 1 : 0;
}
