// Mutation fuzzer for fp_jpeg_exif_orientation (csrc/jpeg.hip, host code that reads untrusted bytes), built with
// AddressSanitizer + UndefinedBehaviorSanitizer.  Seeds: JPEG files with an Exif APP1 segment; their names end in _t<tag>.jpg and
// the untouched file must give that tag.  Every input lives in an exact-size heap block, so a read past the end is a report.
// Mutations aim at the APP1 segment: bytes inside it rewritten, the file cut inside it, the segment's length field and the TIFF
// block's offset / count fields set to hostile values, the segment cut short with its length field adjusted.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "facepath.h"
static uint64_t s = 88172645463325252ull;
static inline uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }

static int run(const unsigned char* p, size_t n) {
  unsigned char* d = (unsigned char*)malloc(n ? n : 1);
  if (n) memcpy(d, p, n);
  const int r = fp_jpeg_exif_orientation(d, n);
  free(d);
  if (r < 1 || r > 8) {
    fprintf(stderr, "orientation %d outside 1 .. 8\n", r);
    exit(1);
  }
  return r;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const long iters = atol(argv[1]);
  const char* e = getenv("FUZZ_SEED");
  if (e) s ^= strtoull(e, 0, 10) * 0x9e3779b97f4a7c15ull;
  long total = 0, tagged = 0;
  static const uint32_t hostile[] = {0, 1, 2, 6, 7, 8, 9, 12, 0x7f, 0x80, 0xff, 0x100, 0xfffe, 0xffff, 0x10000, 0x7fffffff, 0x80000000u, 0xfffffff0u, 0xffffffffu};
  for (int f = 2; f < argc; ++f) {
    FILE* fp = fopen(argv[f], "rb");
    if (!fp) return 2;
    std::vector<unsigned char> src;
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, fp)) > 0) src.insert(src.end(), buf, buf + n);
    fclose(fp);
    const char* t = strstr(argv[f], "_t");
    const int want = t ? atoi(t + 2) : 0;
    if (want && run(src.data(), src.size()) != (want >= 1 && want <= 8 ? want : 1)) {
      fprintf(stderr, "%s: the untouched seed gives %d\n", argv[f], run(src.data(), src.size()));
      return 1;
    }
    // the APP1 segment
    size_t a = 2;
    while (a + 4 <= src.size() && src[a] == 0xff && src[a + 1] != 0xe1 && src[a + 1] != 0xda) a += 2 + ((size_t)src[a + 2] << 8 | src[a + 3]);
    if (a + 4 > src.size() || src[a + 1] != 0xe1) return 2;
    const size_t seg = 2 + ((size_t)src[a + 2] << 8 | src[a + 3]), end = a + seg;
    for (size_t cut = 0; cut <= end + 4 && cut <= src.size(); ++cut) run(src.data(), cut), ++total;     // every truncation
    for (long it = 0; it < iters; ++it) {
      std::vector<unsigned char> v(src);
      const int mode = rnd() % 6;
      if (mode == 0) {                          // 1 .. 4 bytes of the segment
        for (int k = 1 + rnd() % 4; k > 0; --k) v[a + rnd() % seg] = (unsigned char)rnd();
      } else if (mode == 1) {                   // a 16- or 32-bit field anywhere in the segment gets a hostile value, either order
        const uint32_t h = hostile[rnd() % (sizeof hostile / sizeof *hostile)];
        const int w = (rnd() & 1) ? 2 : 4;
        const size_t pos = a + 2 + rnd() % (seg - 2 - w);
        const bool le = rnd() & 1;
        for (int k = 0; k < w; ++k) v[pos + k] = (unsigned char)(h >> (8 * (le ? k : w - 1 - k)));
      } else if (mode == 2) {                   // the segment cut short, its length field says so
        const size_t keep = rnd() % (seg - 3);  // body bytes kept
        v.erase(v.begin() + a + 4 + keep, v.begin() + end);
        v[a + 2] = (unsigned char)((keep + 2) >> 8), v[a + 3] = (unsigned char)(keep + 2);
      } else if (mode == 3) {                   // the length field lies
        const uint32_t h = (rnd() & 1) ? hostile[rnd() % (sizeof hostile / sizeof *hostile)] : rnd();
        v[a + 2] = (unsigned char)(h >> 8), v[a + 3] = (unsigned char)h;
      } else if (mode == 4) {                   // bit flips
        for (int k = 1 + rnd() % 8; k > 0; --k) v[a + rnd() % seg] ^= (unsigned char)(1u << (rnd() % 8));
      } else {                                  // the file ends inside or right behind the segment, after a byte change
        v[a + rnd() % seg] = (rnd() & 1) ? 0xff : 0x00;
        v.resize(a + rnd() % (seg + 8 < v.size() - a ? seg + 8 : v.size() - a));
      }
      if (run(v.data(), v.size()) != 1) ++tagged;
      ++total;
    }
  }
  printf("%ld inputs: %ld with a tag 2 .. 8, %ld without\n", total, tagged, total - tagged);
  return 0;
}
