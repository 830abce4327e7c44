// Mutation fuzzer for the host half of the JPEG decoder (fp_jpeg_parse + fp_jpeg_entropy_decode), built with AddressSanitizer.
// Fixed seed, in front of each file's mutations: the file with 0xff fill bytes in front of every RSTn (sequential files with
// restart markers) must decode, in an exact-size block, to the coefficients of the file without them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "facepath.h"
static uint64_t s = 88172645463325252ull;
struct SeedInit { SeedInit() { const char* e = getenv("FUZZ_SEED"); if (e) s ^= strtoull(e, 0, 10) * 0x9e3779b97f4a7c15ull; } } seed_init;
static inline uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
// The fixed fill-byte seed (JPEG B.1.1.2: any number of 0xff may stand in front of a marker): a sequential file with restart
// markers gets two 0xff in front of every RSTn of its scan.  false: the file has no RSTn to dress (or is progressive).
static bool fill_byte_variant(const std::vector<unsigned char>& src, std::vector<unsigned char>& out) {
  size_t p = 2;
  bool sequential = false;
  while (p + 4 <= src.size() && src[p] == 0xff && src[p + 1] != 0xda) {
    if (src[p + 1] == 0xc0 || src[p + 1] == 0xc1) sequential = true;
    p += 2 + ((size_t)src[p + 2] << 8 | src[p + 3]);
  }
  if (!sequential || p + 4 > src.size() || src[p] != 0xff) return false;
  p += 2 + ((size_t)src[p + 2] << 8 | src[p + 3]);
  if (p > src.size()) return false;
  out.assign(src.begin(), src.begin() + p);
  int hits = 0;
  for (; p < src.size(); ++p) {                // (in entropy-coded data ff dn is always a marker: a data 0xff is stuffed)
    if (src[p] == 0xff && p + 1 < src.size() && src[p + 1] >= 0xd0 && src[p + 1] <= 0xd7) out.push_back(0xff), out.push_back(0xff), ++hits;
    out.push_back(src[p]);
  }
  return hits > 0;
}

static int fill_byte_seed(const std::vector<unsigned char>& src) {
  std::vector<unsigned char> v;
  if (!fill_byte_variant(src, v)) return 0;
  fp_jpeg_info a, b;
  if (fp_jpeg_parse(src.data(), src.size(), &a) != FP_OK || a.n_coefs > (1L << 24)) return 0;
  unsigned char* d = (unsigned char*)malloc(v.size());
  memcpy(d, v.data(), v.size());
  std::vector<int16_t> ca((size_t)a.n_coefs + 1), cb((size_t)a.n_coefs + 1);
  const int r0 = fp_jpeg_entropy_decode(src.data(), src.size(), &a, ca.data());
  const int r1 = fp_jpeg_parse(d, v.size(), &b);
  const int r2 = r1 == FP_OK && b.n_coefs == a.n_coefs ? fp_jpeg_entropy_decode(d, v.size(), &b, cb.data()) : FP_ERR_INVALID_ARG;
  free(d);
  if (r0 != FP_OK) return 0;
  if (r2 != FP_OK || memcmp(ca.data(), cb.data(), (size_t)a.n_coefs * 2) != 0) {
    fprintf(stderr, "fixed fill-byte seed: parse %d, entropy_decode %d, coefficients %s\n", r1, r2, r2 == FP_OK ? "differ" : "-");
    return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  long iters = atol(argv[1]);
  long ok = 0, err = 0, total = 0;
  for (int f = 2; f < argc; ++f) {
    FILE* fp = fopen(argv[f], "rb");
    if (!fp) return 2;
    std::vector<unsigned char> src;
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, fp)) > 0) src.insert(src.end(), buf, buf + n);
    fclose(fp);
    if (fill_byte_seed(src)) return 1;
    for (long it = 0; it < iters; ++it) {
      // exact-size heap copy: any read past the end is an ASan report
      size_t len = src.size();
      const int mode = rnd() % 6;
      if (mode == 0) len = rnd() % (src.size() + 1);                       // truncate anywhere
      else if (mode == 1) { const size_t t = 2 + rnd() % 1200; len = t < src.size() ? t : src.size(); }   // truncate inside the headers
      unsigned char* d = (unsigned char*)malloc(len ? len : 1);
      memcpy(d, src.data(), len);
      if (len > 4) {
        const int nmut = mode == 2 ? 1 : mode == 3 ? 8 : mode == 4 ? 64 : mode == 5 ? 3 : 0;
        for (int k = 0; k < nmut; ++k) {
          size_t pos = (mode == 5 || (rnd() & 1)) ? rnd() % (len < 700 ? len : 700) : rnd() % len;   // headers get half of the hits
          const int what = rnd() % 4;
          d[pos] = what == 0 ? (unsigned char)rnd() : what == 1 ? 0xff : what == 2 ? 0x00 : (unsigned char)(d[pos] ^ (1u << (rnd() % 8)));
        }
      }
      fp_jpeg_info info;
      const int tag = fp_jpeg_exif_orientation(d, len);   // the marker walk of the orientation reader on the same bytes (its own
      if (tag < 1 || tag > 8) return 1;                   // campaign on the APP1 segment: jpeg_exif_fuzz.cpp)
      int rc = fp_jpeg_parse(d, len, &info);
      if (rc == 0) {
        if (info.n_coefs < 0 || info.n_coefs > (1L << 28)) { free(d); ++err; continue; }   // (a caller allocates this much)
        int16_t* co = (int16_t*)malloc((size_t)info.n_coefs * 2 + 2);
        rc = fp_jpeg_entropy_decode(d, len, &info, co);
        free(co);
      }
      rc == 0 ? ++ok : ++err;
      ++total;
      free(d);
    }
  }
  printf("%ld inputs: %ld decoded, %ld refused\n", total, ok, err);
  return 0;
}
