// jpeg.hip — JPEG decode (sequential and progressive Huffman files), bit-exact with libjpeg-turbo's default decompressor
// (gfx950 + host).
//
// The step in FRONT of the hot path: the reference reads its frames with cv2.imread
// (fde/modules/utils/inference.py:68-76, fde/face_extraction/extract_faces_from_dataset.py:393-420) and tf.io.decode_jpeg
// (sff/filter_faces_using_reference.py:62) -- both are libjpeg(-turbo).  A batch of frames decoded with PIL / cv2 on the host
// costs 3-4 ms per 576 x 1024 frame and core; here the split is the one hardware decoders use:
//   host    marker parsing + Huffman decoding (inherently serial per scan) -> quantised DCT coefficients, int16
//           (fp_jpeg_parse, fp_jpeg_entropy_decode: plain C, no GPU; callers run one thread per image)
//   device  dequantisation + 8 x 8 inverse DCT (jidctint.c's "islow" integer transform, the library's default), fancy
//           (triangle-filter) chroma upsampling for 4:2:0 / 4:2:2 (jdsample.c h2v2_fancy_upsample / h2v1_fancy_upsample) where
//           the chroma plane is more than 2 samples wide and plain replication (h2v2_upsample / h2v1_upsample) where it is
//           not -- jinit_upsampler's rule: fancy only for downsampled_width > 2 --,
//           YCbCr -> RGB in 16-bit fixed point (jdcolor.c) -> interleaved u8 RGB or BGR frame (fp_jpeg_reconstruct)
// All three device stages are integer arithmetic restated from the library's published algorithm; the result is compared
// byte for byte with Pillow's decode (libjpeg-turbo) of the reference's own test images (tests/golden/jpeg, tests/test_jpeg.py).
// Scope: sequential (SOF0 / SOF1) and PROGRESSIVE (SOF2: spectral selection + successive approximation, jdphuff.c) Huffman
// files, 8-bit, any number of scans, 1 or 3 components, luma sampling 1x1 / 2x1 / 2x2 with 1x1 chroma, restart intervals.
// A sequential file without DHT segments (a Motion-JPEG frame) decodes with the Annex K.3 tables (std_huff_tables below).
// Arithmetic-coded, lossless, 12-bit, CMYK and other sampling layouts are refused (FP_ERR_UNSUPPORTED): the caller falls back
// to its host decoder for those.
#include <string.h>

#include "common.h"
#include "jpegrecon.h"
#include "jpegstd.h"

namespace {

const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  // canonical Huffman table: 9-bit lookahead (code length << 8 | symbol, 0 = longer code) + the classic maxcode walk
  unsigned short look[512];
  int maxcode[18], valptr[17], mincode[17];
  unsigned char vals[256];
  // sequential AC decoding: 10 bits of lookahead that hold a whole run/size code AND its value bits decode in one step:
  // (value << 8) | (run << 4) | bits consumed, 0 = take the two-step path (the same idea as stb_image's fast_ac)
  short fast[1024];
  bool present;
  bool preset;              // installed by std_huff_tables, not by a DHT segment of the file
};

bool build_huff(Huff& h, const unsigned char* bits /*[1..16]*/, const unsigned char* vals, int nvals) {
  memset(&h, 0, sizeof(h));
  int code = 0, k = 0;
  unsigned short codes[256];
  unsigned char lens[256];
  for (int l = 1; l <= 16; ++l) {
    h.valptr[l] = k;
    h.mincode[l] = code;
    for (int i = 0; i < bits[l]; ++i) {
      if (k >= nvals || k >= 256) return false;
      codes[k] = (unsigned short)code;
      lens[k] = (unsigned char)l;
      ++k;
      ++code;
    }
    h.maxcode[l] = bits[l] ? code - 1 : -1;
    if (code > (1 << l)) return false;
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  if (k != nvals) return false;
  memcpy(h.vals, vals, nvals);
  for (int i = 0; i < k; ++i) {
    if (lens[i] <= 9) {
      const int base = codes[i] << (9 - lens[i]);
      for (int j = 0; j < (1 << (9 - lens[i])); ++j) h.look[base + j] = (unsigned short)((lens[i] << 8) | vals[i]);
    }
  }
  for (int i = 0; i < 1024; ++i) {
    const unsigned e = h.look[i >> 1];
    const int len = (int)(e >> 8), run = (int)((e >> 4) & 15), sz = (int)(e & 15);
    if (e && sz && len + sz <= 10) {
      int v = (i >> (10 - len - sz)) & ((1 << sz) - 1);
      if (v < (1 << (sz - 1))) v += 1 - (1 << sz);
      if (v >= -128 && v <= 127) h.fast[i] = (short)((v * 256) | (run << 4) | (len + sz));
    }
  }
  h.present = true;
  return true;
}

struct BitReader {
  const unsigned char* p;
  const unsigned char* end;
  unsigned long long acc;   // bits left-aligned at the top
  int nbits;
  int marker;               // a marker met in the entropy-coded data (0 = none): the reader feeds zeros behind it
  void init(const unsigned char* b, const unsigned char* e) { p = b, end = e, acc = 0, nbits = 0, marker = 0; }
  void fill() {
    if (!marker && end - p >= 8) {             // eight bytes ahead with no 0xff among them: take the whole bytes that fit at once
      unsigned long long w;
      __builtin_memcpy(&w, p, 8);
      if (!((~w - 0x0101010101010101ull) & w & 0x8080808080808080ull)) {
        const int k = (64 - nbits) >> 3;
        if (k > 0) {
          w = __builtin_bswap64(w);
          acc |= (w >> nbits) & (~0ull << (64 - nbits - 8 * k));
          p += k, nbits += 8 * k;
        }
        return;
      }
    }
    while (nbits <= 56) {
      unsigned v = 0;
      if (!marker && p < end) {
        v = *p;
        if (v == 0xff) {
          // any number of 0xff fill bytes may stand in front of a marker code (B.1.1.2); jdhuff.c's fill_bit_buffer reads
          // on while it sees 0xff and only then tells a stuffed zero from a marker
          const unsigned char* q = p + 1;
          while (q < end && *q == 0xff) ++q;
          const unsigned n = q < end ? *q : 0xd9;
          if (n == 0) p = q + 1;               // stuffed zero
          else {
            marker = (int)n;                   // RSTn / EOI / ...: stop consuming (p: the 0xff in front of the code), feed zeros
            p = q - 1;
            v = 0;
          }
        } else {
          ++p;
        }
      }
      acc |= (unsigned long long)v << (56 - nbits);
      nbits += 8;
    }
  }
  inline unsigned peek(int n) { return (unsigned)(acc >> (64 - n)); }
  inline void skip(int n) { acc <<= n, nbits -= n; }
  inline int get(int n) {                     // n in 1..16
    if (nbits < n) fill();
    const unsigned v = peek(n);
    skip(n);
    return (int)v;
  }
};

inline int huff_decode(BitReader& br, const Huff& h) {
  if (br.nbits < 16) br.fill();
  const unsigned e = h.look[br.peek(9)];
  if (e) {
    br.skip(e >> 8);
    return e & 255;
  }
  int code = (int)br.peek(9), l = 9;
  br.skip(9);
  while (l < 17 && code > h.maxcode[l]) {
    code = (code << 1) | br.get(1);
    ++l;
  }
  if (l > 16) return -1;
  return h.vals[h.valptr[l] + code - h.mincode[l]];
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One block of a sequential scan (jdhuff.c decode_mcu): DC difference, then run / size pairs up to EOB.
inline int decode_block_seq(BitReader& br, const Huff& hd, const Huff& ha, int& pred, int16_t* blk) {
  int s = huff_decode(br, hd);
  if (s < 0 || s > 11) return FP_ERR_INVALID_ARG;
  if (s) pred += extend(br.get(s), s);
  blk[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    if (br.nbits < 32) br.fill();                  // a code (<= 16 bits) and its value bits (<= 11) are in the accumulator
    const int fe = ha.fast[br.peek(10)];
    if (fe) {
      k += (fe >> 4) & 15;
      if (k > 63) return FP_ERR_INVALID_ARG;
      blk[kZigzag[k++]] = (int16_t)(fe >> 8);
      br.skip(fe & 15);
      continue;
    }
    const int rs = huff_decode(br, ha);
    if (rs < 0) return FP_ERR_INVALID_ARG;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;                          // EOB
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return FP_ERR_INVALID_ARG;
    blk[kZigzag[k++]] = (int16_t)extend(br.get(s), s);
  }
  return FP_OK;
}

// The tables a SEQUENTIAL file starts with (jdhuff.c jinit_huff_decoder -> std_huff_tables): slots 0 and 1 of both classes
// hold the Annex K.3 luminance and chrominance tables until a DHT segment overwrites them; slots 2 and 3 stay absent.
// Motion-JPEG frames routinely carry no DHT at all.  libjpeg-turbo's progressive decoder (jdphuff.c) installs nothing and
// refuses a scan whose table no DHT defined (JERR_NO_HUFF_TABLE); drop_preset_tables takes the presets out again for SOF2.
void std_huff_tables(Huff* dc /*[4]*/, Huff* ac /*[4]*/) {
  build_huff(dc[0], kDcLumaBits, kDcVals, 12);
  build_huff(ac[0], kAcLumaBits, kAcLumaVals, 162);
  build_huff(dc[1], kDcChromaBits, kDcVals, 12);
  build_huff(ac[1], kAcChromaBits, kAcChromaVals, 162);
  for (int i = 0; i < 2; ++i) dc[i].preset = ac[i].preset = true;
}

void drop_preset_tables(Huff* dc /*[4]*/, Huff* ac /*[4]*/) {
  for (int i = 0; i < 2; ++i) {
    if (dc[i].preset) dc[i].present = dc[i].preset = false;
    if (ac[i].preset) ac[i].present = ac[i].preset = false;
  }
}

inline unsigned be16(const unsigned char* p) { return ((unsigned)p[0] << 8) | p[1]; }

struct Frame {               // what the frame header (SOF) and the tables in front of the first scan say
  int comp_id[3], comp_tq[3];
  unsigned short qt[4][64];
  bool have_qt[4];
  bool have_sof;
};

// DQT / DHT / DRI segment bodies (s .. e)
int read_dqt(const unsigned char* s, const unsigned char* e, Frame& fr) {
  while (s < e) {
    const int pq = s[0] >> 4, tq = s[0] & 15;
    if (tq > 3 || pq > 1) return FP_ERR_INVALID_ARG;
    ++s;
    if (s + (pq ? 128 : 64) > e) return FP_ERR_INVALID_ARG;
    for (int i = 0; i < 64; ++i) fr.qt[tq][kZigzag[i]] = pq ? (unsigned short)be16(s + 2 * i) : s[i];   // natural order
    s += pq ? 128 : 64;
    fr.have_qt[tq] = true;
  }
  return FP_OK;
}

int read_dht(const unsigned char* s, const unsigned char* e, Huff* dc, Huff* ac) {
  while (s < e) {
    const int tc = s[0] >> 4, th = s[0] & 15;
    if (tc > 1 || th > 3 || s + 17 > e) return FP_ERR_INVALID_ARG;
    unsigned char bits[17];
    bits[0] = 0;
    int nv = 0;
    for (int i = 1; i <= 16; ++i) bits[i] = s[i], nv += s[i];
    if (nv > 256 || s + 17 + nv > e) return FP_ERR_INVALID_ARG;
    if (!build_huff(tc ? ac[th] : dc[th], bits, s + 17, nv)) return FP_ERR_INVALID_ARG;
    s += 17 + nv;
  }
  return FP_OK;
}

int read_sof(const unsigned char* s, unsigned len, unsigned m, fp_jpeg_info& info, Frame& fr) {
  if (len < 8 || s[0] != 8) return FP_ERR_UNSUPPORTED;       // 8-bit samples only
  info.progressive = m == 0xc2;
  info.height = (int)be16(s + 1);
  info.width = (int)be16(s + 3);
  info.ncomp = s[5];
  if (info.width <= 0 || info.height <= 0) return FP_ERR_UNSUPPORTED;
  if ((info.ncomp != 1 && info.ncomp != 3) || len < 8u + 3u * info.ncomp) return FP_ERR_UNSUPPORTED;
  for (int c = 0; c < info.ncomp; ++c) {
    fr.comp_id[c] = s[6 + 3 * c];
    info.hs[c] = s[7 + 3 * c] >> 4;
    info.vs[c] = s[7 + 3 * c] & 15;
    fr.comp_tq[c] = s[8 + 3 * c];
    if (fr.comp_tq[c] > 3) return FP_ERR_INVALID_ARG;
  }
  // geometry: luma 1x1 / 2x1 / 2x2, chroma 1x1
  if (info.ncomp == 1) {
    info.hs[0] = info.vs[0] = 1;            // a single-component image is never interleaved: 8 x 8 MCUs
  } else {
    if (info.hs[1] != 1 || info.vs[1] != 1 || info.hs[2] != 1 || info.vs[2] != 1) return FP_ERR_UNSUPPORTED;
    if (!((info.hs[0] == 1 && info.vs[0] == 1) || (info.hs[0] == 2 && info.vs[0] == 1) || (info.hs[0] == 2 && info.vs[0] == 2)))
      return FP_ERR_UNSUPPORTED;
  }
  info.mcux = (info.width + 8 * info.hs[0] - 1) / (8 * info.hs[0]);
  info.mcuy = (info.height + 8 * info.vs[0] - 1) / (8 * info.vs[0]);
  long off = 0;
  for (int c = 0; c < info.ncomp; ++c) {
    info.blocks_w[c] = info.mcux * info.hs[c];
    info.blocks_h[c] = info.mcuy * info.vs[c];
    info.coef_off[c] = off;
    off += (long)info.blocks_w[c] * info.blocks_h[c] * 64;
    // the component's true size (jdmaster.c: ceil(image * samp / max_samp)): what the fancy upsampler's edges see
    info.comp_w[c] = (info.width * info.hs[c] + info.hs[0] - 1) / info.hs[0];
    info.comp_h[c] = (info.height * info.vs[c] + info.vs[0] - 1) / info.vs[0];
  }
  info.n_coefs = off;
  fr.have_sof = true;
  return FP_OK;
}

struct Scan {
  int ns, ci[3], td[3], ta[3], Ss, Se, Ah, Al;
};

int read_sos(const unsigned char* s, unsigned len, const fp_jpeg_info& info, const Frame& fr, Scan& sc) {
  if (len < 3) return FP_ERR_INVALID_ARG;        // an empty segment body: s[0] would lie behind it
  sc.ns = s[0];
  if (sc.ns < 1 || sc.ns > info.ncomp || len != 6u + 2u * sc.ns) return FP_ERR_INVALID_ARG;
  for (int i = 0; i < sc.ns; ++i) {
    int c = 0;
    while (c < info.ncomp && fr.comp_id[c] != s[1 + 2 * i]) ++c;
    if (c == info.ncomp) return FP_ERR_INVALID_ARG;
    sc.ci[i] = c;
    sc.td[i] = s[2 + 2 * i] >> 4;
    sc.ta[i] = s[2 + 2 * i] & 15;
    if (sc.td[i] > 3 || sc.ta[i] > 3) return FP_ERR_INVALID_ARG;
  }
  sc.Ss = s[1 + 2 * sc.ns];
  sc.Se = s[2 + 2 * sc.ns];
  sc.Ah = s[3 + 2 * sc.ns] >> 4;
  sc.Al = s[3 + 2 * sc.ns] & 15;
  if (!info.progressive) {
    if (sc.Ss != 0 || sc.Se != 63 || sc.Ah != 0 || sc.Al != 0) return FP_ERR_INVALID_ARG;
  } else {
    if (sc.Ss > sc.Se || sc.Se > 63 || sc.Al > 13 || (sc.Ss == 0 && sc.Se != 0) || (sc.Ss > 0 && sc.ns != 1)) return FP_ERR_INVALID_ARG;
    if (sc.Ah != 0 && sc.Ah != sc.Al + 1) return FP_ERR_INVALID_ARG;
  }
  return FP_OK;
}

// Walks the markers up to the first SOS; fills info (frame geometry, quantisation tables).  Returns the offset of that SOS
// marker's segment length or a negative fp_status.  dc / ac collect the Huffman tables seen on the way.
long parse_headers(const unsigned char* d, size_t n, fp_jpeg_info& info, Frame& fr, Huff* dc /*[4]*/, Huff* ac /*[4]*/) {
  memset(&info, 0, sizeof(info));
  memset(&fr, 0, sizeof(fr));
  std_huff_tables(dc, ac);
  if (n < 4 || d[0] != 0xff || d[1] != 0xd8) return FP_ERR_INVALID_ARG;
  size_t pos = 2;
  while (pos + 4 <= n) {
    if (d[pos] != 0xff) return FP_ERR_INVALID_ARG;
    const unsigned m = d[pos + 1];
    pos += 2;
    if (m == 0xff) {          // fill byte
      --pos;
      continue;
    }
    if (m == 0xd8 || (m >= 0xd0 && m <= 0xd7) || m == 0x01) continue;
    if (m == 0xd9) return FP_ERR_INVALID_ARG;   // EOI before SOS
    if (pos + 2 > n) return FP_ERR_INVALID_ARG;
    const unsigned len = be16(d + pos);
    if (len < 2 || pos + len > n) return FP_ERR_INVALID_ARG;
    const unsigned char* s = d + pos + 2;
    const unsigned char* e = d + pos + len;
    int rc = FP_OK;
    if (m == 0xdb) rc = read_dqt(s, e, fr);
    else if (m == 0xc0 || m == 0xc1 || m == 0xc2) rc = read_sof(s, len, m, info, fr);   // sequential / progressive, Huffman, 8-bit
    else if (m >= 0xc3 && m <= 0xcf && m != 0xc4 && m != 0xc8 && m != 0xcc) rc = FP_ERR_UNSUPPORTED;   // lossless, arithmetic, differential
    else if (m == 0xc4) rc = read_dht(s, e, dc, ac);
    else if (m == 0xdd) {
      if (len != 4) return FP_ERR_INVALID_ARG;
      info.restart_interval = (int)be16(s);
    } else if (m == 0xda) {
      if (!fr.have_sof) return FP_ERR_INVALID_ARG;
      for (int c = 0; c < info.ncomp; ++c) {
        if (!fr.have_qt[fr.comp_tq[c]]) return FP_ERR_INVALID_ARG;
        memcpy(info.quant[c], fr.qt[fr.comp_tq[c]], 128);
      }
      if (info.progressive) drop_preset_tables(dc, ac);
      return (long)pos;
    }
    if (rc) return rc;
    pos += len;
  }
  return FP_ERR_INVALID_ARG;
}

// One scan's entropy-coded segment -> coefficients (jdhuff.c decode_mcu for sequential files; jdphuff.c's four MCU decoders for
// progressive ones: DC first / DC refine / AC first / AC refine).  Returns FP_OK and leaves br at the marker behind the scan.
int decode_scan(BitReader& br, const fp_jpeg_info& info, const Scan& sc, const Huff* dc, const Huff* ac, int16_t* coefs) {
  for (int i = 0; i < sc.ns; ++i) {
    if ((sc.Ss == 0 && sc.Ah == 0 && !dc[sc.td[i]].present) || (sc.Se > 0 && !ac[sc.ta[i]].present)) return FP_ERR_INVALID_ARG;
  }
  // MCU geometry: interleaved scans walk the frame's MCUs; a one-component scan walks that component's own blocks
  const int c0 = sc.ci[0];
  const bool inter = sc.ns > 1;
  const int nmx = inter ? info.mcux : (info.comp_w[c0] + 7) / 8;
  const int nmy = inter ? info.mcuy : (info.comp_h[c0] + 7) / 8;
  int pred[3] = {0, 0, 0};
  int eobrun = 0;
  int until_restart = info.restart_interval, next_rst = 0;
  const int p1 = 1 << sc.Al, m1 = -(1 << sc.Al);
  for (int my = 0; my < nmy; ++my) {
    for (int mx = 0; mx < nmx; ++mx) {
      if (info.restart_interval && until_restart == 0) {
        br.nbits = 0;                              // byte-align, expect RSTn
        br.acc = 0;
        if (!br.marker) {
          while (br.p + 1 < br.end && !(br.p[0] == 0xff && br.p[1] != 0 && br.p[1] != 0xff)) ++br.p;
          if (br.p + 1 < br.end) br.marker = br.p[1];
        }
        if (br.marker != 0xd0 + next_rst) return FP_ERR_INVALID_ARG;
        br.p += 2;
        br.marker = 0;
        next_rst = (next_rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
        eobrun = 0;
        until_restart = info.restart_interval;
      }
      for (int i = 0; i < sc.ns; ++i) {
        const int c = sc.ci[i];
        const int nv = inter ? info.vs[c] : 1, nh = inter ? info.hs[c] : 1;
        for (int v = 0; v < nv; ++v) {
          for (int hh = 0; hh < nh; ++hh) {
            int16_t* blk = coefs + info.coef_off[c] + ((long)(my * nv + v) * info.blocks_w[c] + (mx * nh + hh)) * 64;
            if (!info.progressive) {
              const int rc = decode_block_seq(br, dc[sc.td[i]], ac[sc.ta[i]], pred[c], blk);
              if (rc) return rc;
            } else if (sc.Ss == 0) {
              if (sc.Ah == 0) {                    // ---- DC first scan ----
                const int s = huff_decode(br, dc[sc.td[i]]);
                if (s < 0 || s > 11) return FP_ERR_INVALID_ARG;
                if (s) pred[c] += extend(br.get(s), s);
                blk[0] = (int16_t)(pred[c] * (1 << sc.Al));
              } else if (br.get(1)) {              // ---- DC refinement: one more bit ----
                blk[0] = (int16_t)(blk[0] | p1);
              }
            } else if (sc.Ah == 0) {               // ---- AC first scan (one component) ----
              if (eobrun > 0) {
                --eobrun;
              } else {
                const Huff& ha = ac[sc.ta[i]];
                for (int k = sc.Ss; k <= sc.Se; ++k) {
                  const int rs = huff_decode(br, ha);
                  if (rs < 0) return FP_ERR_INVALID_ARG;
                  const int r = rs >> 4, s = rs & 15;
                  if (s) {
                    k += r;
                    if (k > 63) return FP_ERR_INVALID_ARG;
                    blk[kZigzag[k]] = (int16_t)(extend(br.get(s), s) * (1 << sc.Al));
                  } else if (r == 15) {
                    k += 15;                       // ZRL
                  } else {
                    eobrun = 1 << r;
                    if (r) eobrun += br.get(r);
                    --eobrun;
                    break;
                  }
                }
              }
            } else {                               // ---- AC refinement scan (one component): jdphuff.c decode_mcu_AC_refine ----
              const Huff& ha = ac[sc.ta[i]];
              int k = sc.Ss;
              if (eobrun == 0) {
                for (; k <= sc.Se; ++k) {
                  const int rs = huff_decode(br, ha);
                  if (rs < 0) return FP_ERR_INVALID_ARG;
                  int r = rs >> 4, s = rs & 15;
                  if (s) {
                    s = br.get(1) ? p1 : m1;       // (size is always 1: the new coefficient's sign)
                  } else if (r != 15) {
                    eobrun = 1 << r;
                    if (r) eobrun += br.get(r);
                    break;                         // end of band: the rest of the block gets correction bits only
                  }
                  // step over r still-zero coefficients, appending a correction bit to every nonzero one on the way
                  do {
                    int16_t* t = blk + kZigzag[k];
                    if (*t != 0) {
                      if (br.get(1) && (*t & p1) == 0) *t = (int16_t)(*t + (*t >= 0 ? p1 : m1));
                    } else if (--r < 0) {
                      break;
                    }
                    ++k;
                  } while (k <= sc.Se);
                  if (s) {
                    if (k > 63) return FP_ERR_INVALID_ARG;
                    blk[kZigzag[k]] = (int16_t)s;
                  }
                }
              }
              if (eobrun > 0) {
                for (; k <= sc.Se; ++k) {
                  int16_t* t = blk + kZigzag[k];
                  if (*t != 0 && br.get(1) && (*t & p1) == 0) *t = (int16_t)(*t + (*t >= 0 ? p1 : m1));
                }
                --eobrun;
              }
            }
          }
        }
      }
      if (info.restart_interval) --until_restart;
    }
  }
  return FP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// device side

// (the arithmetic -- jpeg_idct_block, chroma_sample, jpeg_color_pixel -- stands in jpegrecon.h: csrc/jpegbatch.hip runs the same)

// One thread per 8 x 8 block: dequantise, columns (descale 11), rows (descale 18), + 128, clamp -> the component's sample plane.
__global__ __launch_bounds__(64) void jpeg_idct_kernel(const short* coefs, unsigned char* planes, JpegDevInfo info, long nblocks_total) {
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= nblocks_total) return;
  long bb = b;
  const int c = jpeg_block_component(info, bb);
  const int bx = (int)(bb % info.blocks_w[c]), by = (int)(bb / info.blocks_w[c]);
  const long pitch = info.blocks_w[c] * 8;
  jpeg_idct_block(coefs + info.coef_off[c] + bb * 64, info.quant[c], planes + info.plane_off[c] + ((long)by * 8) * pitch + bx * 8, pitch);
}

// One thread per output pixel: upsample + ycc_rgb_convert (jdcolor.c: SCALEBITS 16) -> interleaved u8
__global__ __launch_bounds__(256) void jpeg_color_kernel(const unsigned char* planes, unsigned char* out, JpegDevInfo info, int bgr) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)info.width * info.height) return;
  const int oy = (int)(i / info.width), ox = (int)(i - (long)oy * info.width);
  jpeg_color_pixel(planes, out + i * 3, info, oy, ox, bgr);
}

}  // namespace

extern "C" {

int fp_jpeg_parse(const uint8_t* data, size_t n, fp_jpeg_info* info) {
  if (!data || !info) return FP_ERR_INVALID_ARG;
  Huff* tabs = new Huff[8];
  memset(tabs, 0, 8 * sizeof(Huff));
  Frame fr;
  const long r = parse_headers(data, n, *info, fr, tabs, tabs + 4);
  delete[] tabs;
  return r < 0 ? (int)r : FP_OK;
}

// The Orientation tag (0x0112) of the first APP1 segment that starts with "Exif\0\0" in front of the first scan: TIFF header,
// IFD0, the 12-byte entry of type SHORT.  Every offset is checked against the end of the TIFF block (tn) before the bytes
// behind it are read; anything that does not fit is "no tag".
int fp_jpeg_exif_orientation(const uint8_t* d, size_t n) {
  if (!d || n < 4 || d[0] != 0xff || d[1] != 0xd8) return 1;
  size_t pos = 2;
  while (pos + 4 <= n) {
    if (d[pos] != 0xff) return 1;
    const unsigned m = d[pos + 1];
    if (m == 0xff) {          // fill byte
      ++pos;
      continue;
    }
    pos += 2;
    if (m == 0xd8 || (m >= 0xd0 && m <= 0xd7) || m == 0x01) continue;
    if (m == 0xd9 || m == 0xda) return 1;        // EOI / the first scan: no Exif segment in front of it
    if (pos + 2 > n) return 1;
    const size_t len = be16(d + pos);
    if (len < 2 || len > n - pos) return 1;
    if (m != 0xe1 || len < 8 || memcmp(d + pos + 2, "Exif\0\0", 6) != 0) {
      pos += len;
      continue;
    }
    const uint8_t* t = d + pos + 8;              // the TIFF block: offsets inside it count from here
    const size_t tn = len - 8;
    if (tn < 8) return 1;
    bool le;
    if (t[0] == 'I' && t[1] == 'I' && t[2] == 0x2a && t[3] == 0) le = true;
    else if (t[0] == 'M' && t[1] == 'M' && t[2] == 0 && t[3] == 0x2a) le = false;
    else return 1;
    auto u16 = [&](size_t o) { return le ? (unsigned)t[o] | ((unsigned)t[o + 1] << 8) : ((unsigned)t[o] << 8) | t[o + 1]; };
    auto u32 = [&](size_t o) { return le ? (size_t)u16(o) | ((size_t)u16(o + 2) << 16) : ((size_t)u16(o) << 16) | u16(o + 2); };
    const size_t ifd = u32(4);
    if (ifd > tn - 2) return 1;                  // (tn >= 8; the entry count's two bytes lie inside)
    const size_t cnt = u16(ifd);
    if (cnt * 12 > tn - 2 - ifd) return 1;       // an entry count that runs past the segment
    for (size_t i = 0; i < cnt; ++i) {
      const size_t e = ifd + 2 + 12 * i;
      if (u16(e) != 0x0112) continue;
      if (u16(e + 2) != 3 || u32(e + 4) != 1) return 1;   // SHORT, one value: it sits in the entry's value field
      const unsigned v = u16(e + 8);
      return v >= 1 && v <= 8 ? (int)v : 1;
    }
    return 1;
  }
  return 1;
}

int fp_jpeg_entropy_decode(const uint8_t* data, size_t n, const fp_jpeg_info* info_in, int16_t* coefs) {
  if (!data || !info_in || !coefs) return FP_ERR_INVALID_ARG;
  fp_jpeg_info info;
  Huff* dc = new Huff[8];
  Huff* ac = dc + 4;
  memset(dc, 0, 8 * sizeof(Huff));
  Frame fr;
  long pos = parse_headers(data, n, info, fr, dc, ac);
  int rc = pos < 0 ? (int)pos : FP_OK;
  if (!rc && (info.n_coefs != info_in->n_coefs || info.width != info_in->width || info.height != info_in->height)) rc = FP_ERR_INVALID_ARG;
  if (rc) {
    delete[] dc;
    return rc;
  }
  memset(coefs, 0, (size_t)info.n_coefs * sizeof(int16_t));
  // pos = the first SOS segment's length field.  One scan after the other; DHT / DRI (/ DQT, ignored: a component's table is
  // latched at its first scan) may stand between scans; EOI or the end of the data ends the image.
  int scans = 0;
  for (;;) {
    if ((size_t)pos + 2 > n) break;
    const unsigned len = be16(data + pos);
    if (len < 2 || (size_t)pos + len > n) {
      rc = FP_ERR_INVALID_ARG;
      break;
    }
    Scan sc;
    rc = read_sos(data + pos + 2, len, info, fr, sc);
    if (rc) break;
    BitReader br;
    br.init(data + pos + len, data + n);
    rc = decode_scan(br, info, sc, dc, ac, coefs);
    if (rc) break;
    ++scans;
    // the marker behind the scan
    const unsigned char* p = br.p;
    if (!br.marker) {
      while (p + 1 < data + n && !(p[0] == 0xff && p[1] != 0 && p[1] != 0xff)) ++p;
    }
    bool next_scan = false;
    while (p + 1 < data + n) {
      if (p[0] != 0xff) break;
      const unsigned m = p[1];
      if (m == 0xff) {
        ++p;
        continue;
      }
      if (m == 0xd9) break;                                        // EOI
      if (m >= 0xd0 && m <= 0xd7) {
        p += 2;
        continue;
      }
      if (p + 4 > data + n) break;
      const unsigned l2 = be16(p + 2);
      if (l2 < 2 || p + 2 + l2 > data + n) {
        rc = FP_ERR_INVALID_ARG;
        break;
      }
      if (m == 0xc4) rc = read_dht(p + 4, p + 2 + l2, dc, ac);
      else if (m == 0xdd && l2 == 4) info.restart_interval = (int)be16(p + 4);
      else if (m == 0xda) {
        pos = (long)(p + 2 - data);
        next_scan = true;
        break;
      }
      if (rc) break;
      p += 2 + l2;
    }
    if (rc || !next_scan) break;
  }
  delete[] dc;
  if (rc) return rc;
  return scans > 0 ? FP_OK : FP_ERR_INVALID_ARG;
}

int fp_jpeg_scan_prepare(const uint8_t* data, size_t n, fp_jpeg_info* info, fp_jpeg_scan* scan) {
  if (!data || !info || !scan) return FP_ERR_INVALID_ARG;
  Huff* dc = new Huff[8];
  Huff* ac = dc + 4;
  memset(dc, 0, 8 * sizeof(Huff));
  Frame fr;
  memset(scan, 0, sizeof(*scan));
  const long pos = parse_headers(data, n, *info, fr, dc, ac);
  int rc = pos < 0 ? (int)pos : FP_OK;
  unsigned len = 0;
  Scan sc;
  if (!rc && info->progressive) rc = FP_ERR_UNSUPPORTED;
  if (!rc && (size_t)pos + 2 > n) rc = FP_ERR_INVALID_ARG;
  if (!rc) {
    len = be16(data + pos);
    if (len < 2 || (size_t)pos + len > n) rc = FP_ERR_INVALID_ARG;
  }
  if (!rc) rc = read_sos(data + pos + 2, len, *info, fr, sc);
  if (!rc && sc.ns != info->ncomp) rc = FP_ERR_UNSUPPORTED;     // the first scan must carry every component
  for (int i = 0; !rc && i < sc.ns; ++i) {
    for (int j = 0; j < i; ++j)
      if (sc.ci[j] == sc.ci[i]) rc = FP_ERR_UNSUPPORTED;
    if (!rc && (!dc[sc.td[i]].present || !ac[sc.ta[i]].present)) rc = FP_ERR_INVALID_ARG;   // decode_scan's check
  }
  const size_t off = (size_t)pos + len;
  long nblocks = 0;
  for (int c = 0; !rc && c < info->ncomp; ++c) nblocks += (long)info->blocks_w[c] * info->blocks_h[c];
  if (!rc && (n - off > (size_t)FP_JPEG_DEV_MAX_BYTES || nblocks > FP_JPEG_DEV_MAX_BLOCKS)) rc = FP_ERR_UNSUPPORTED;
  if (!rc) {
    scan->data_off = (int64_t)off;
    scan->data_len = (int64_t)(n - off);
    scan->n_coefs = info->n_coefs;
    scan->mcux = info->mcux;
    scan->mcuy = info->mcuy;
    scan->restart_interval = info->restart_interval;
    scan->ncomp = info->ncomp;
    int slot = 0;
    for (int i = 0; i < sc.ns; ++i) {
      const int c = sc.ci[i];
      scan->coef_off[c] = info->coef_off[c];
      scan->blocks_w[c] = info->blocks_w[c];
      scan->hs[c] = info->hs[c];
      scan->vs[c] = info->vs[c];
      for (int v = 0; v < info->vs[c]; ++v)
        for (int h = 0; h < info->hs[c]; ++h) {
          scan->slot_comp[slot] = (uint8_t)c;
          scan->slot_tab[slot] = (uint8_t)i;
          scan->slot_dy[slot] = (uint8_t)v;
          scan->slot_dx[slot] = (uint8_t)h;
          ++slot;
        }
      const Huff* src[2] = {&dc[sc.td[i]], &ac[sc.ta[i]]};
      fp_jpeg_huff* dst[2] = {&scan->dc[i], &scan->ac[i]};
      for (int t = 0; t < 2; ++t) {
        memcpy(dst[t]->look, src[t]->look, sizeof(dst[t]->look));
        memcpy(dst[t]->vals, src[t]->vals, sizeof(dst[t]->vals));
        for (int l = 0; l < 18; ++l) {
          dst[t]->maxcode[l] = l >= 1 && l <= 16 ? src[t]->maxcode[l] : -1;
          dst[t]->valoff[l] = l >= 1 && l <= 16 ? src[t]->valptr[l] - src[t]->mincode[l] : 0;
        }
      }
    }
    scan->blocks_per_mcu = slot;
  }
  delete[] dc;
  return rc;
}

size_t fp_jpeg_workspace_bytes(const fp_jpeg_info* info) {
  if (!info) return 0;
  size_t b = 0;
  for (int c = 0; c < info->ncomp; ++c) b += (size_t)info->blocks_w[c] * 8 * info->blocks_h[c] * 8;
  return (b + 15) / 16 * 16;
}

int fp_jpeg_reconstruct(const int16_t* coefs, const fp_jpeg_info* info, uint8_t* workspace, size_t ws_bytes, uint8_t* out, int bgr,
                        void* stream) {
  if (!coefs || !info || !workspace || !out) return FP_ERR_INVALID_ARG;
  if (info->ncomp != 1 && info->ncomp != 3) return FP_ERR_UNSUPPORTED;
  if (ws_bytes < fp_jpeg_workspace_bytes(info)) return FP_ERR_BOUNDS;
  if (((uintptr_t)workspace) % 8 || ((uintptr_t)coefs) % 2) return FP_ERR_ALIGNMENT;
  JpegDevInfo d;
  long nblocks = 0, plane_bytes = 0;
  if (!jpeg_dev_info(info, d, nblocks, plane_bytes)) return FP_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((nblocks + 63) / 64)), dim3(64), 0, s, (const short*)coefs, workspace, d, nblocks);
  FP_CHECK_LAUNCH();
  const long npx = (long)info->width * info->height;
  hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, workspace, out, d, bgr);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
