// Mutation fuzzer for the device Huffman decoder's algorithm (csrc/jpegdec.hip), built with AddressSanitizer +
// UndefinedBehaviorSanitizer: every mutated input the device path takes (fp_jpeg_scan_prepare == FP_OK) runs through
// fp_jpeg_entropy_decode_emulate -- the device phases, serially, from the same per-lane source -- at a small subsequence length,
// and the result must equal fp_jpeg_entropy_decode's: the same status and every coefficient, unless the emulator leaves the
// image to the host (FP_JPEG_DECODE_ON_HOST).  A difference prints the input's index and aborts.
//     jpeg_device_fuzz <iterations per file> <sub_bits> <max_rounds> <files ...>
// The fixed seed of ADVICE r4 (a file cut at its SOS header + ff da 00 02) runs first: both host entries must return
// FP_ERR_INVALID_ARG without reading past the buffer.  The fixed fill-byte seed runs in front of each file's mutations: the file
// with two 0xff in front of every RSTn must decode on the host to the coefficients of the file without them, and the emulator
// must hand it to the host or agree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "facepath.h"
static uint64_t s = 0x243f6a8885a308d3ull;
struct SeedInit { SeedInit() { const char* e = getenv("FUZZ_SEED"); if (e) s ^= strtoull(e, 0, 10) * 0x9e3779b97f4a7c15ull; } } seed_init;
static inline uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }

static fp_jpeg_scan scan;     // (large: static)

// 0 ok / refused alike, 1 host-decided, 2 mismatch
static int check(const unsigned char* d, size_t len, int sub_bits, int rounds, long* n_dev, long* n_host) {
  fp_jpeg_info info;
  if (fp_jpeg_scan_prepare(d, len, &info, &scan) != FP_OK) return 0;
  ++*n_dev;
  std::vector<int16_t> a((size_t)info.n_coefs + 1), b((size_t)info.n_coefs + 1);
  const int rh = fp_jpeg_entropy_decode(d, len, &info, a.data());
  const int re = fp_jpeg_entropy_decode_emulate(d, len, &scan, b.data(), sub_bits, rounds, nullptr);
  if (re == FP_JPEG_DECODE_ON_HOST) {
    ++*n_host;
    return 1;
  }
  if (re != rh || memcmp(a.data(), b.data(), (size_t)info.n_coefs * 2) != 0) {
    long first = -1;
    for (long i = 0; i < info.n_coefs && first < 0; ++i)
      if (a[i] != b[i]) first = i;
    fprintf(stderr, "MISMATCH host %d emulator %d first differing coefficient %ld\n", rh, re, first);
    return 2;
  }
  return 0;
}

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

static int fill_byte_seed(const std::vector<unsigned char>& src, int sub_bits, int rounds) {
  std::vector<unsigned char> v;
  if (!fill_byte_variant(src, v)) return 0;
  fp_jpeg_info a, b;
  if (fp_jpeg_parse(src.data(), src.size(), &a) != FP_OK || a.n_coefs > (1L << 24)) return 0;
  std::vector<int16_t> ca((size_t)a.n_coefs + 1), cb((size_t)a.n_coefs + 1);
  if (fp_jpeg_entropy_decode(src.data(), src.size(), &a, ca.data()) != FP_OK) return 0;
  unsigned char* d = (unsigned char*)malloc(v.size());
  memcpy(d, v.data(), v.size());
  const int r1 = fp_jpeg_parse(d, v.size(), &b);
  const int r2 = r1 == FP_OK && b.n_coefs == a.n_coefs ? fp_jpeg_entropy_decode(d, v.size(), &b, cb.data()) : FP_ERR_INVALID_ARG;
  int bad = r2 != FP_OK || memcmp(ca.data(), cb.data(), (size_t)a.n_coefs * 2) != 0;
  if (bad) fprintf(stderr, "fixed fill-byte seed: parse %d, entropy_decode %d\n", r1, r2);
  long n_dev = 0, n_host = 0;
  if (!bad && check(d, v.size(), sub_bits, rounds, &n_dev, &n_host) == 2) bad = 1;
  if (!bad && n_dev != 1) fprintf(stderr, "fixed fill-byte seed: fp_jpeg_scan_prepare refused the file\n"), bad = 1;
  free(d);
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const long iters = atol(argv[1]);
  const int sub_bits = atoi(argv[2]), rounds = atoi(argv[3]);
  long total = 0, n_dev = 0, n_host = 0, n_ok = 0;
  for (int f = 4; f < argc; ++f) {
    FILE* fp = fopen(argv[f], "rb");
    if (!fp) return 2;
    std::vector<unsigned char> src;
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, fp)) > 0) src.insert(src.end(), buf, buf + n);
    fclose(fp);
    if (f == 4) {                              // the fixed seed: cut at the first SOS, + ff da 00 02, exact-size block
      size_t p = 2;
      while (p + 4 <= src.size() && !(src[p] == 0xff && src[p + 1] == 0xda)) p += 2 + ((size_t)src[p + 2] << 8 | src[p + 3]);
      if (p + 4 > src.size()) return 2;
      unsigned char* d = (unsigned char*)malloc(p + 4);
      memcpy(d, src.data(), p);
      memcpy(d + p, "\xff\xda\x00\x02", 4);
      fp_jpeg_info info;
      static fp_jpeg_scan sc;
      std::vector<int16_t> co(1 << 22);
      const int r1 = fp_jpeg_scan_prepare(d, p + 4, &info, &sc);
      const int r2 = fp_jpeg_parse(d, p + 4, &info) == FP_OK && info.n_coefs < (1 << 22) ? fp_jpeg_entropy_decode(d, p + 4, &info, co.data())
                                                                                           : FP_ERR_INVALID_ARG;
      free(d);
      if (r1 != FP_ERR_INVALID_ARG || r2 != FP_ERR_INVALID_ARG) {
        fprintf(stderr, "fixed seed: prepare %d, entropy_decode %d (want %d)\n", r1, r2, FP_ERR_INVALID_ARG);
        return 1;
      }
    }
    if (fill_byte_seed(src, sub_bits, rounds)) return 1;
    for (long it = 0; it < iters; ++it) {
      size_t len = src.size();
      const int mode = rnd() % 7;
      if (mode == 0) len = rnd() % (src.size() + 1);                       // truncate anywhere
      unsigned char* d = (unsigned char*)malloc(len ? len : 1);
      memcpy(d, src.data(), len);
      if (len > 4 && mode > 0) {
        const int nmut = mode == 1 ? 1 : mode == 2 ? 4 : mode == 3 ? 16 : mode == 4 ? 2 : mode == 5 ? 1 : 0;
        for (int k = 0; k < nmut; ++k) {
          const size_t pos = len > 700 && (rnd() & 3) ? 600 + rnd() % (len - 600) : rnd() % len;   // mostly the scan data
          const int what = rnd() % 5;
          d[pos] = what == 0 ? (unsigned char)rnd() : what == 1 ? 0xff : what == 2 ? 0x00
                 : what == 3 ? (unsigned char)(0xd0 + rnd() % 10) : (unsigned char)(d[pos] ^ (1u << (rnd() % 8)));
        }
        if (mode == 6 && len > 8) {                                      // a marker pair (RSTn / EOI / SOS / fill) somewhere
          const size_t pos = rnd() % (len - 1);
          const unsigned char m[5] = {0xd0, 0xd3, 0xd9, 0xda, 0xff};
          d[pos] = 0xff;
          d[pos + 1] = m[rnd() % 5];
        }
      }
      const int r = check(d, len, sub_bits, rounds, &n_dev, &n_host);
      free(d);
      if (r == 2) {
        fprintf(stderr, "input %ld of file %s (mode %d)\n", it, argv[f], mode);
        return 1;
      }
      if (r == 0) ++n_ok;
      ++total;
    }
  }
  printf("%ld inputs: %ld taken by the device path, %ld left to the host, %ld equal\n", total, n_dev, n_host, n_ok);
  return 0;
}
