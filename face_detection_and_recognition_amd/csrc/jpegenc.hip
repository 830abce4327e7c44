// Baseline JPEG encoding of a batch of crops on the device: libjpeg-turbo's default compressor (jpeg_set_defaults +
// jpeg_set_quality(q, TRUE), islow DCT, standard Huffman tables, no restart markers) bit for bit -- the stream cv2.imwrite
// writes for the reference's face crops (fde/face_extraction/extract_faces_from_dataset.py:311-363) and Pillow's save.
//
// The batch is a list of coded blocks: image after image, MCU after MCU, the blocks of each MCU in scan order (luma blocks
// row by row, then Cb, then Cr).  A block of a partial MCU that lies outside its component (beyond width_in_blocks or
// height_in_blocks) is a DUMMY block (jccoefct.c compress_data): zero AC, DC = the DC of the block before it.  Phases:
//   je_blocks  one wave per block, one lane per coefficient: gather (clamped crop, edge replication), RGB -> YCbCr
//              (jccolor.c), h2v1 / h2v2 downsampling (jcsample.c), level shift, islow forward DCT (jfdctint.c), quantisation
//              by libjpeg-turbo's reciprocal tables (jcdctmgr.c compute_reciprocal), the block's AC bit length
//   je_dc      one thread per block: DC difference against the block before it in the component, bit length of the block
//   scan       exclusive prefix sum of the block bit lengths over the batch (an image's offsets: minus its first block's)
//   je_emit    one wave per block: every lane writes its coefficient's codes at its bit offset (atomic OR into zeroed words;
//              image i owns the words from its first block * kWordsPerBlock on)
//   stuffing   per word: bytes of the image (last byte padded with 1-bits) plus one per 0xFF; a prefix sum over the words
//              of the batch places every byte in the compacted output, images back to back
// The per-lane, per-block and per-word functions are __host__ __device__: fp_jpeg_encode_emulate runs the same phases
// serially on the CPU.  The host writes the headers (fp_jpeg_encode_headers); the device writes only the scan data.
#include "common.h"
#include "jpegstd.h"   // Annex K.3 - K.6: kDcLumaBits ... kAcChromaVals

#include <string.h>

#include <vector>

#define HD __host__ __device__

namespace {

constexpr int kWordsPerBlock = 52;    // 1664 bits >= the 1660-bit worst case of one block (facepath.h)
constexpr int kTile = 1024;           // elements per scan tile: 256 threads x 4

// ---- tables ------------------------------------------------------------------------------------------------------

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU T.81 Annex K.1, natural order
const uint8_t kStdLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                              14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                              18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

struct HuffEnc {
  uint16_t code[256];
  uint8_t size[256];   // 0: no code
};

// Quantisation of one component as jcdctmgr.c does it: divisor q << 3 through a reciprocal (natural order)
struct QuantDiv {
  uint32_t recip[64];
  uint32_t corr[64];
  uint32_t shift[64];
};

// Everything the kernels read besides the images: uploaded with the descriptors on every call
struct EncTables {
  HuffEnc huff[4];      // luma DC, luma AC, chroma DC, chroma AC
  QuantDiv quant[2];    // luma, chroma
  uint8_t zigzag[64];   // zigzag index -> natural index
  uint8_t pad[64];
};

struct EncImg {
  int64_t src_off;      // byte offset of the crop's pixel (0, 0) in src
  int64_t block_off;    // first coded block of the image in the batch
  int32_t stride;       // bytes per source row
  int32_t w, h;         // crop size
  int32_t mcux, mcuy;
  int32_t nblocks;
  int32_t wib[2], hib[2];   // blocks per row / column of luma and of each chroma component
};

struct EncParams {
  const uint8_t* src;
  const EncTables* tab;
  const EncImg* img;
  int n_img;
  int64_t n_blocks;
  int hmax, vmax, bpm;  // luma blocks per MCU across / down; blocks per MCU
  int bgr;
  int32_t* blk_img;     // [n_blocks] image of each block
  int16_t* coef;        // [n_blocks][64] quantised coefficients, zigzag order
  int32_t* bits;        // [n_blocks] AC bit length (je_blocks), then whole-block bit length (je_dc)
  int32_t* dcdiff;      // [n_blocks]
  int64_t* bit_off;     // [n_blocks + 1] exclusive prefix sum of bits
  int64_t* partial;     // scan tiles
  uint32_t* words;      // [n_blocks * kWordsPerBlock] the bit stream of image i from word img[i].block_off * kWordsPerBlock
  uint8_t* out;         // compacted, stuffed scan data of the batch
  int64_t* out_off;     // [n_img + 1]
};

void make_huff(HuffEnc& t, const uint8_t* bits, const uint8_t* vals) {   // jchuff.c jpeg_make_c_derived_tbl
  memset(&t, 0, sizeof(t));
  unsigned code = 0;
  int p = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l]; ++i, ++p) {
      t.code[vals[p]] = (uint16_t)code++;
      t.size[vals[p]] = (uint8_t)l;
    }
    code <<= 1;
  }
}

// jcparam.c jpeg_quality_scaling + jpeg_add_quant_table(force_baseline = TRUE): natural order
void quant_table(int quality, int chroma, uint16_t* q) {
  const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
  const uint8_t* base = chroma ? kStdChroma : kStdLuma;
  for (int i = 0; i < 64; ++i) {
    long t = ((long)base[i] * scale + 50L) / 100L;
    q[i] = (uint16_t)(t <= 0 ? 1 : t > 255 ? 255 : t);
  }
}

// jcdctmgr.c compute_reciprocal for a divisor >= 2 (here always >= 8): x / d rounded = ((x + corr) * recip) >> shift
void reciprocal(unsigned divisor, uint32_t& recip, uint32_t& corr, uint32_t& shift) {
  int b = 31 - __builtin_clz(divisor);     // flss(divisor) - 1
  int r = 16 + b;
  uint64_t fq = (1ull << r) / divisor, fr = (1ull << r) % divisor;
  unsigned c = divisor / 2;
  if (fr == 0) {
    fq >>= 1;
    r--;
  } else if (fr <= divisor / 2u) {
    c++;
  } else {
    fq++;
  }
  recip = (uint32_t)fq;
  corr = c;
  shift = (uint32_t)r;
}

void make_tables(EncTables& T, int quality) {
  memset(&T, 0, sizeof(T));
  make_huff(T.huff[0], kDcLumaBits, kDcVals);
  make_huff(T.huff[1], kAcLumaBits, kAcLumaVals);
  make_huff(T.huff[2], kDcChromaBits, kDcVals);
  make_huff(T.huff[3], kAcChromaBits, kAcChromaVals);
  for (int c = 0; c < 2; ++c) {
    uint16_t q[64];
    quant_table(quality, c, q);
    for (int i = 0; i < 64; ++i) reciprocal((unsigned)q[i] << 3, T.quant[c].recip[i], T.quant[c].corr[i], T.quant[c].shift[i]);
  }
  memcpy(T.zigzag, kZigzag, 64);
}

// ---- per-pixel / per-lane arithmetic (host and device) -----------------------------------------------------------

HD inline int imin(int a, int b) { return a < b ? a : b; }

// jccolor.c rgb_ycc_convert: 16-bit fixed point, ONE_HALF rounding, CBCR_OFFSET
HD inline int to_ycc(int comp, int r, int g, int b) {
  constexpr int32_t kHalf = 1 << 15, kCbcrOff = 128 << 16;
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + kHalf) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + kCbcrOff + kHalf - 1) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + kCbcrOff + kHalf - 1) >> 16;
}

HD inline int pixel_ycc(const uint8_t* src, const EncImg& im, int bgr, int comp, int y, int x) {
  const uint8_t* p = src + im.src_off + (int64_t)y * im.stride + (int64_t)x * 3;
  int r = p[0], g = p[1], b = p[2];
  if (bgr) {
    r = p[2];
    b = p[0];
  }
  return to_ycc(comp, r, g, b);
}

// Component sample (cy, cx) of an image, with the encoder's edge handling: the right edge of every row replicated out to
// the component's block boundary (jcsample.c expand_right_edge, before downsampling), the last row group replicated down
// to the row-group height (jcprepct.c), and the last downsampled row down to the iMCU height.  Chroma: h2v1 / h2v2
// downsampling of jcsample.c with its alternating bias.
HD inline int sample(const uint8_t* src, const EncImg& im, int bgr, int hmax, int vmax, int comp, int cy, int cx) {
  if (comp == 0 || hmax == 1) return pixel_ycc(src, im, bgr, comp, imin(cy, im.h - 1), imin(cx, im.w - 1));
  const int x0 = imin(2 * cx, im.w - 1), x1 = imin(2 * cx + 1, im.w - 1);
  if (vmax == 1) {   // h2v1: bias 0, 1, 0, 1, ...
    const int y = imin(cy, im.h - 1);
    return (pixel_ycc(src, im, bgr, comp, y, x0) + pixel_ycc(src, im, bgr, comp, y, x1) + (cx & 1)) >> 1;
  }
  const int rows = (im.h + 1) >> 1;              // downsampled rows the image has; below them: the last one again
  const int yc = imin(cy, rows - 1);
  const int y0 = 2 * yc, y1 = imin(2 * yc + 1, im.h - 1);
  return (pixel_ycc(src, im, bgr, comp, y0, x0) + pixel_ycc(src, im, bgr, comp, y0, x1) + pixel_ycc(src, im, bgr, comp, y1, x0) +
          pixel_ycc(src, im, bgr, comp, y1, x1) + ((cx & 1) ? 2 : 1)) >> 2;   // h2v2: bias 1, 2, 1, 2, ...
}

// jfdctint.c (islow): one pass over 8 values at stride `st`; pass 0 = rows, 1 = columns.  Output scaled by 8.
HD inline void fdct8(int32_t* d, int st, int pass) {
  constexpr int CB = 13, P1 = 2;
  const int sh = pass == 0 ? CB - P1 : CB + P1;
  auto descale = [](int64_t x, int n) { return (int32_t)((x + ((int64_t)1 << (n - 1))) >> n); };
  int64_t tmp0 = d[0] + d[7 * st], tmp7 = d[0] - d[7 * st];
  int64_t tmp1 = d[st] + d[6 * st], tmp6 = d[st] - d[6 * st];
  int64_t tmp2 = d[2 * st] + d[5 * st], tmp5 = d[2 * st] - d[5 * st];
  int64_t tmp3 = d[3 * st] + d[4 * st], tmp4 = d[3 * st] - d[4 * st];
  int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (pass == 0) {
    d[0] = (int32_t)((tmp10 + tmp11) * (1 << P1));
    d[4 * st] = (int32_t)((tmp10 - tmp11) * (1 << P1));
  } else {
    d[0] = descale(tmp10 + tmp11, P1);
    d[4 * st] = descale(tmp10 - tmp11, P1);
  }
  int64_t z1 = (tmp12 + tmp13) * 4433;                      // FIX_0_541196100
  d[2 * st] = descale(z1 + tmp13 * 6270, sh);               // FIX_0_765366865
  d[6 * st] = descale(z1 + tmp12 * -15137, sh);             // FIX_1_847759065
  z1 = tmp4 + tmp7;
  int64_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int64_t z5 = (z3 + z4) * 9633;                      // FIX_1_175875602
  tmp4 *= 2446;                                             // FIX_0_298631336
  tmp5 *= 16819;                                            // FIX_2_053119869
  tmp6 *= 25172;                                            // FIX_3_072711026
  tmp7 *= 12299;                                            // FIX_1_501321110
  z1 *= -7373;                                              // FIX_0_899976223
  z2 *= -20995;                                             // FIX_2_562915447
  z3 *= -16069;                                             // FIX_1_961570560
  z4 *= -3196;                                              // FIX_0_390180644
  z3 += z5;
  z4 += z5;
  d[7 * st] = descale(tmp4 + z1 + z3, sh);
  d[5 * st] = descale(tmp5 + z2 + z4, sh);
  d[3 * st] = descale(tmp6 + z2 + z3, sh);
  d[st] = descale(tmp7 + z1 + z4, sh);
}

HD inline int quantize(int32_t x, const QuantDiv& q, int i) {
  const uint32_t a = (uint32_t)(x < 0 ? -x : x);
  const int v = (int)(((uint64_t)(a + q.corr[i]) * q.recip[i]) >> q.shift[i]);
  return x < 0 ? -v : v;
}

HD inline int nbits(int v) {
  unsigned a = (unsigned)(v < 0 ? -v : v);
  return a ? 32 - __builtin_clz(a) : 0;
}

HD inline int hibit64(uint64_t m) { return 63 - __builtin_clzll(m); }

// One lane's share of a block's AC codes: the lane of coefficient k (zigzag) with v != 0 writes the ZRLs of the zero run in
// front of it, its (run, size) code and its magnitude bits; the lane of the last nonzero AC coefficient (lane 0 if there is
// none) appends EOB unless that coefficient is the 63rd.  nz: bit k set for every nonzero AC coefficient k.  <= 63 bits.
HD inline void ac_lane(int k, int v, uint64_t nz, const HuffEnc& ac, uint64_t& val, int& len) {
  val = 0;
  len = 0;
  if (k > 0 && v != 0) {
    const uint64_t below = nz & ((1ull << k) - 1);
    int run = k - (below ? hibit64(below) : 0) - 1;
    for (; run >= 16; run -= 16) {
      val = (val << ac.size[0xF0]) | ac.code[0xF0];
      len += ac.size[0xF0];
    }
    const int cat = nbits(v), sym = (run << 4) | cat;
    val = (val << ac.size[sym]) | ac.code[sym];
    val = (val << cat) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1));
    len += ac.size[sym] + cat;
  }
  const int last = nz ? hibit64(nz) : 0;
  if (k == last && last < 63) {
    val = (val << ac.size[0]) | ac.code[0];
    len += ac.size[0];
  }
}

HD inline void dc_code(int diff, const HuffEnc& dc, uint64_t& val, int& len) {
  const int cat = nbits(diff);
  val = ((uint64_t)dc.code[cat] << cat) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1));
  len = dc.size[cat] + cat;
}

// Geometry of coded block `local` of an image: component, block row / column in it, real or dummy
struct BlockPos {
  int mcu, slot, comp, first_slot, r, c, real;
};

HD inline BlockPos block_pos(const EncImg& im, int hmax, int vmax, int bpm, int local) {
  BlockPos p;
  p.mcu = local / bpm;
  p.slot = local - p.mcu * bpm;
  const int my = p.mcu / im.mcux, mx = p.mcu - my * im.mcux, nl = hmax * vmax;
  int by = 0, bx = 0, hc = 1, vc = 1;
  if (p.slot < nl) {
    p.comp = 0;
    p.first_slot = 0;
    by = p.slot / hmax;
    bx = p.slot - by * hmax;
    hc = hmax;
    vc = vmax;
  } else {
    p.comp = 1 + p.slot - nl;
    p.first_slot = p.slot;
  }
  p.r = my * vc + by;
  p.c = mx * hc + bx;
  const int ci = p.comp ? 1 : 0;
  p.real = p.r < im.hib[ci] && p.c < im.wib[ci];
  return p;
}

// DC of coded block `slot` of MCU `mcu` as the encoder sees it: a dummy block repeats the block before it in the MCU (the
// first block of a component in an MCU is never a dummy)
HD inline int effective_dc(const EncParams& P, const EncImg& im, int mcu, int slot) {
  for (;; --slot) {
    const int local = mcu * P.bpm + slot;
    if (block_pos(im, P.hmax, P.vmax, P.bpm, local).real) return P.coef[(im.block_off + local) * 64];
  }
}

// je_dc's work for one block
HD inline void block_dc(const EncParams& P, int64_t b) {
  const EncImg& im = P.img[P.blk_img[b]];
  const int local = (int)(b - im.block_off);
  const BlockPos p = block_pos(im, P.hmax, P.vmax, P.bpm, local);
  int diff = 0;
  if (p.real) {
    int pred = 0;
    if (p.slot > p.first_slot) {
      pred = effective_dc(P, im, p.mcu, p.slot - 1);
    } else if (p.mcu > 0) {
      const int last = p.comp == 0 ? P.hmax * P.vmax - 1 : p.slot;
      pred = effective_dc(P, im, p.mcu - 1, last);
    }
    diff = P.coef[b * 64] - pred;
  }
  const HuffEnc& dc = P.tab->huff[p.comp ? 2 : 0];
  P.dcdiff[b] = diff;
  P.bits[b] += dc.size[nbits(diff)] + nbits(diff);
}

HD inline int find_img(const EncImg* img, int n, int64_t b) {   // last image whose block_off <= b
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (img[mid].block_off <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Writes `len` (<= 63) bits of val, most significant first, at bit position pos of a big-endian word stream
HD inline void put_bits(uint32_t* words, int64_t pos, uint64_t val, int len) {
  while (len > 0) {
    const int off = (int)(pos & 31), room = 32 - off, take = len < room ? len : room;
    const uint32_t chunk = (uint32_t)((val >> (len - take)) & ((1ull << take) - 1)) << (room - take);
#ifdef __HIP_DEVICE_COMPILE__
    atomicOr(words + (pos >> 5), chunk);
#else
    words[pos >> 5] |= chunk;
#endif
    pos += take;
    len -= take;
  }
}

// Word w of the batch's bit stream: its bytes (0 .. 4) inside its image's scan data, last byte padded with 1-bits
struct WordBytes {
  int n;
  uint8_t b[4];
  int img;
  int first;   // the image's first word
};

HD inline WordBytes word_bytes(const EncParams& P, int64_t w) {
  WordBytes r;
  r.img = P.blk_img[w / kWordsPerBlock];
  const EncImg& im = P.img[r.img];
  const int64_t lw = w - im.block_off * kWordsPerBlock;
  r.first = lw == 0;
  const int64_t T = P.bit_off[im.block_off + im.nblocks] - P.bit_off[im.block_off];
  const int64_t nbytes = (T + 7) >> 3;
  const uint32_t word = P.words[w];
  r.n = 0;
  for (int j = 0; j < 4; ++j) {
    const int64_t bj = lw * 4 + j;
    if (bj >= nbytes) break;
    uint8_t v = (uint8_t)(word >> (24 - 8 * j));
    if (bj == nbytes - 1 && (T & 7)) v |= (uint8_t)(0xFF >> (T & 7));
    r.b[r.n++] = v;
  }
  return r;
}

HD inline int64_t word_stuffed_len(const EncParams& P, int64_t w) {
  const WordBytes r = word_bytes(P, w);
  int64_t s = r.n;
  for (int j = 0; j < r.n; ++j) s += r.b[j] == 0xFF;
  return s;
}

// ---- kernels -------------------------------------------------------------------------------------------------------

__device__ inline int64_t wave_incl_scan(int64_t x, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// Exclusive prefix sum over the 256 threads of a workgroup; *total = the workgroup's sum.  Every thread must call it.
__device__ inline int64_t block_excl_scan(int64_t v, int64_t* total) {
  __shared__ int64_t wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t inc = wave_incl_scan(v, lane);
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int64_t before = 0, all = 0;
  for (int i = 0; i < 4; ++i) {
    if (i < wv) before += wsum[i];
    all += wsum[i];
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

__global__ void __launch_bounds__(256) je_blocks(EncParams P) {
  __shared__ int32_t d[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * 4 + wv;
  const bool valid = b < P.n_blocks;
  int ii = 0;
  BlockPos p = {};
  if (valid) {
    ii = find_img(P.img, P.n_img, b);
    p = block_pos(P.img[ii], P.hmax, P.vmax, P.bpm, (int)(b - P.img[ii].block_off));
    if (p.real)
      d[wv][lane] = sample(P.src, P.img[ii], P.bgr, P.hmax, P.vmax, p.comp, p.r * 8 + (lane >> 3), p.c * 8 + (lane & 7)) - 128;
  }
  __syncthreads();
  if (valid && p.real && lane < 8) fdct8(&d[wv][lane * 8], 1, 0);
  __syncthreads();
  if (valid && p.real && lane < 8) fdct8(&d[wv][lane], 8, 1);
  __syncthreads();
  if (!valid) return;
  const int ci = p.comp ? 1 : 0;
  const int nat = P.tab->zigzag[lane];
  const int v = p.real ? quantize(d[wv][nat], P.tab->quant[ci], nat) : 0;
  P.coef[b * 64 + lane] = (int16_t)v;
  const uint64_t nz = __ballot(lane > 0 && v != 0);
  uint64_t val;
  int len;
  ac_lane(lane, v, nz, P.tab->huff[ci ? 3 : 1], val, len);
  for (int o = 32; o > 0; o >>= 1) len += __shfl_xor(len, o, 64);
  if (lane == 0) {
    P.bits[b] = len;
    P.blk_img[b] = ii;
  }
}

__global__ void __launch_bounds__(256) je_dc(EncParams P) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < P.n_blocks) block_dc(P, b);
}

// Scan tiles: tile t covers elements [t * kTile, (t + 1) * kTile); thread j of it elements 4 j .. 4 j + 3
struct BitsCount {
  __device__ int64_t operator()(const EncParams& P, int64_t i) const { return P.bits[i]; }
};
struct StuffCount {
  __device__ int64_t operator()(const EncParams& P, int64_t w) const { return word_stuffed_len(P, w); }
};

template <class F>
__global__ void __launch_bounds__(256) je_reduce(EncParams P, int64_t n) {
  const int64_t i0 = (int64_t)blockIdx.x * kTile + threadIdx.x * 4;
  int64_t s = 0;
  for (int j = 0; j < 4; ++j)
    if (i0 + j < n) s += F()(P, i0 + j);
  int64_t tot;
  block_excl_scan(s, &tot);
  if (threadIdx.x == 0) P.partial[blockIdx.x] = tot;
}

// One workgroup: exclusive scan of the tile sums in place; *total = the sum of all
__global__ void __launch_bounds__(256) je_scan_partials(int64_t* partial, int64_t n_tiles, int64_t* total) {
  int64_t carry = 0;
  for (int64_t base = 0; base < n_tiles; base += 256) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = i < n_tiles ? partial[i] : 0;
    int64_t tot;
    const int64_t ex = block_excl_scan(v, &tot);
    if (i < n_tiles) partial[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ void __launch_bounds__(256) je_bits_apply(EncParams P) {
  const int64_t i0 = (int64_t)blockIdx.x * kTile + threadIdx.x * 4;
  int64_t v[4], s = 0;
  for (int j = 0; j < 4; ++j) {
    v[j] = i0 + j < P.n_blocks ? P.bits[i0 + j] : 0;
    s += v[j];
  }
  int64_t tot;
  int64_t off = P.partial[blockIdx.x] + block_excl_scan(s, &tot);
  for (int j = 0; j < 4; ++j) {
    if (i0 + j < P.n_blocks) P.bit_off[i0 + j] = off;
    off += v[j];
  }
}

__global__ void __launch_bounds__(256) je_emit(EncParams P) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= P.n_blocks) return;   // wave-uniform
  const EncImg& im = P.img[P.blk_img[b]];
  const int ci = block_pos(im, P.hmax, P.vmax, P.bpm, (int)(b - im.block_off)).comp ? 1 : 0;
  const int v = P.coef[b * 64 + lane];
  const uint64_t nz = __ballot(lane > 0 && v != 0);
  uint64_t val;
  int len;
  ac_lane(lane, v, nz, P.tab->huff[ci ? 3 : 1], val, len);
  if (lane == 0) {
    uint64_t dv;
    int dl;
    dc_code(P.dcdiff[b], P.tab->huff[ci ? 2 : 0], dv, dl);
    val |= dv << len;
    len += dl;
  }
  const int64_t pre = wave_incl_scan(len, lane) - len;
  const int64_t pos = im.block_off * kWordsPerBlock * 32 + (P.bit_off[b] - P.bit_off[im.block_off]) + pre;
  put_bits(P.words, pos, val, len);
}

__global__ void __launch_bounds__(256) je_stuff_apply(EncParams P, int64_t n_words) {
  const int64_t w0 = (int64_t)blockIdx.x * kTile + threadIdx.x * 4;
  WordBytes r[4];
  int64_t s = 0;
  for (int j = 0; j < 4; ++j) {
    r[j].n = 0;
    if (w0 + j < n_words) r[j] = word_bytes(P, w0 + j);
    s += r[j].n;
    for (int k = 0; k < r[j].n; ++k) s += r[j].b[k] == 0xFF;
  }
  int64_t tot;
  int64_t off = P.partial[blockIdx.x] + block_excl_scan(s, &tot);
  for (int j = 0; j < 4; ++j) {
    if (w0 + j >= n_words) break;
    if (r[j].first) P.out_off[r[j].img] = off;
    for (int k = 0; k < r[j].n; ++k) {
      P.out[off++] = r[j].b[k];
      if (r[j].b[k] == 0xFF) P.out[off++] = 0;
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------

struct EncLayout {
  std::vector<EncImg> imgs;
  int hmax, vmax, bpm;
  int64_t n_blocks, n_words, n_tiles;
  size_t off_tab, off_img, off_blk, off_coef, off_bits, off_dc, off_boff, off_part, off_words, total;
  size_t out_bytes;
};

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Validates the batch and lays out the workspace.  FP_OK or the refusal's status.
int plan(const fp_jpeg_enc_item* items, int n, int subsampling, EncLayout& L) {
  if (!items || n < 1) return FP_ERR_INVALID_ARG;
  if (subsampling < 0 || subsampling > 2) return FP_ERR_UNSUPPORTED;
  L.hmax = subsampling == FP_JPEG_444 ? 1 : 2;
  L.vmax = subsampling == FP_JPEG_420 ? 2 : 1;
  L.bpm = L.hmax * L.vmax + 2;
  L.imgs.resize(n);
  int64_t nb = 0;
  for (int i = 0; i < n; ++i) {
    const fp_jpeg_enc_item& it = items[i];
    if (it.src_off < 0 || it.src_h < 1 || it.src_w < 1) return FP_ERR_INVALID_ARG;
    // the reference's slice: image[max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)]
    const int x0 = it.x0 > 0 ? it.x0 : 0, y0 = it.y0 > 0 ? it.y0 : 0;
    const int x1 = it.x1 < it.src_w ? it.x1 : it.src_w, y1 = it.y1 < it.src_h ? it.y1 : it.src_h;
    if (x1 <= x0 || y1 <= y0) return FP_ERR_INVALID_ARG;     // an empty crop: nothing to encode
    if (x1 - x0 > 65535 || y1 - y0 > 65535) return FP_ERR_UNSUPPORTED;
    EncImg& im = L.imgs[i];
    im.stride = it.src_w * 3;
    if ((int64_t)it.src_w * 3 > INT32_MAX) return FP_ERR_UNSUPPORTED;
    im.src_off = it.src_off + (int64_t)y0 * im.stride + (int64_t)x0 * 3;
    im.w = x1 - x0;
    im.h = y1 - y0;
    im.mcux = (int)ceil_div(im.w, 8 * L.hmax);
    im.mcuy = (int)ceil_div(im.h, 8 * L.vmax);
    im.wib[0] = (int)ceil_div(im.w, 8);
    im.hib[0] = (int)ceil_div(im.h, 8);
    im.wib[1] = (int)ceil_div(ceil_div(im.w, L.hmax), 8);
    im.hib[1] = (int)ceil_div(ceil_div(im.h, L.vmax), 8);
    const int64_t blocks = (int64_t)im.mcux * im.mcuy * L.bpm;
    if (blocks > INT32_MAX) return FP_ERR_UNSUPPORTED;
    im.nblocks = (int)blocks;
    im.block_off = nb;
    nb += blocks;
  }
  if (nb > INT32_MAX) return FP_ERR_UNSUPPORTED;
  L.n_blocks = nb;
  L.n_words = nb * kWordsPerBlock;
  L.n_tiles = ceil_div(L.n_words, kTile);   // >= the block tiles
  size_t o = 0;
  L.off_tab = o;   o = align16(o + sizeof(EncTables));
  L.off_img = o;   o = align16(o + sizeof(EncImg) * n);
  L.off_blk = o;   o = align16(o + sizeof(int32_t) * nb);
  L.off_coef = o;  o = align16(o + sizeof(int16_t) * 64 * nb);
  L.off_bits = o;  o = align16(o + sizeof(int32_t) * nb);
  L.off_dc = o;    o = align16(o + sizeof(int32_t) * nb);
  L.off_boff = o;  o = align16(o + sizeof(int64_t) * (nb + 1));
  L.off_part = o;  o = align16(o + sizeof(int64_t) * (L.n_tiles + 1));
  L.off_words = o; o = align16(o + sizeof(uint32_t) * L.n_words);
  L.total = o;
  L.out_bytes = (size_t)nb * FP_JPEG_ENC_BYTES_PER_BLOCK;
  return FP_OK;
}

EncParams params(const EncLayout& L, int n, int bgr, const uint8_t* src, unsigned char* ws, uint8_t* out, int64_t* out_off) {
  EncParams P;
  P.src = src;
  P.tab = (const EncTables*)(ws + L.off_tab);
  P.img = (const EncImg*)(ws + L.off_img);
  P.n_img = n;
  P.n_blocks = L.n_blocks;
  P.hmax = L.hmax;
  P.vmax = L.vmax;
  P.bpm = L.bpm;
  P.bgr = bgr;
  P.blk_img = (int32_t*)(ws + L.off_blk);
  P.coef = (int16_t*)(ws + L.off_coef);
  P.bits = (int32_t*)(ws + L.off_bits);
  P.dcdiff = (int32_t*)(ws + L.off_dc);
  P.bit_off = (int64_t*)(ws + L.off_boff);
  P.partial = (int64_t*)(ws + L.off_part);
  P.words = (uint32_t*)(ws + L.off_words);
  P.out = out;
  P.out_off = out_off;
  return P;
}

void put_marker(std::vector<uint8_t>& o, int marker, int len) {
  o.push_back(0xFF);
  o.push_back((uint8_t)marker);
  o.push_back((uint8_t)(len >> 8));
  o.push_back((uint8_t)len);
}

void put_dht(std::vector<uint8_t>& o, int cls_id, const uint8_t* bits, const uint8_t* vals) {
  int nv = 0;
  for (int l = 1; l <= 16; ++l) nv += bits[l];
  put_marker(o, 0xC4, 2 + 1 + 16 + nv);
  o.push_back((uint8_t)cls_id);
  for (int l = 1; l <= 16; ++l) o.push_back(bits[l]);
  for (int i = 0; i < nv; ++i) o.push_back(vals[i]);
}

}  // namespace

extern "C" {

int fp_jpeg_encode_workspace_bytes(const fp_jpeg_enc_item* items, int n, int subsampling, size_t* ws_bytes, size_t* out_bytes) {
  if (!ws_bytes || !out_bytes) return FP_ERR_INVALID_ARG;
  *ws_bytes = 0;
  *out_bytes = 0;
  EncLayout L;
  const int rc = plan(items, n, subsampling, L);
  if (rc != FP_OK) return rc;
  *ws_bytes = L.total;
  *out_bytes = L.out_bytes;
  return FP_OK;
}

int fp_jpeg_encode_headers(int width, int height, int quality, int subsampling, uint8_t* out, size_t cap) {
  if (!out || width < 1 || height < 1 || width > 65535 || height > 65535 || quality < 1 || quality > 100)
    return FP_ERR_INVALID_ARG;
  if (subsampling < 0 || subsampling > 2) return FP_ERR_UNSUPPORTED;
  if (cap < FP_JPEG_ENC_HEADER_BYTES) return FP_ERR_BOUNDS;
  std::vector<uint8_t> o;
  o.reserve(FP_JPEG_ENC_HEADER_BYTES);
  o.push_back(0xFF);                           // SOI
  o.push_back(0xD8);
  put_marker(o, 0xE0, 16);                     // JFIF 1.01, no units, 1:1 density, no thumbnail (jcmarker.c emit_jfif_app0)
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  o.insert(o.end(), jfif, jfif + 14);
  for (int c = 0; c < 2; ++c) {                // DQT: one marker per table, 8-bit entries, zigzag order
    uint16_t q[64];
    quant_table(quality, c, q);
    put_marker(o, 0xDB, 67);
    o.push_back((uint8_t)c);
    for (int k = 0; k < 64; ++k) o.push_back((uint8_t)q[kZigzag[k]]);
  }
  const int hmax = subsampling == FP_JPEG_444 ? 1 : 2, vmax = subsampling == FP_JPEG_420 ? 2 : 1;
  put_marker(o, 0xC0, 17);                     // SOF0
  o.push_back(8);
  o.push_back((uint8_t)(height >> 8));
  o.push_back((uint8_t)height);
  o.push_back((uint8_t)(width >> 8));
  o.push_back((uint8_t)width);
  o.push_back(3);
  const uint8_t comps[9] = {1, (uint8_t)(hmax << 4 | vmax), 0, 2, 0x11, 1, 3, 0x11, 1};
  o.insert(o.end(), comps, comps + 9);
  put_dht(o, 0x00, kDcLumaBits, kDcVals);      // in the order write_scan_header sends them
  put_dht(o, 0x10, kAcLumaBits, kAcLumaVals);
  put_dht(o, 0x01, kDcChromaBits, kDcVals);
  put_dht(o, 0x11, kAcChromaBits, kAcChromaVals);
  put_marker(o, 0xDA, 12);                     // SOS: the three components interleaved, Ss = 0, Se = 63, Ah = Al = 0
  const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  o.insert(o.end(), sos, sos + 10);
  if (o.size() != FP_JPEG_ENC_HEADER_BYTES) return FP_ERR_INVALID_ARG;
  memcpy(out, o.data(), o.size());
  return (int)o.size();
}

int fp_jpeg_encode_device(const uint8_t* src, const fp_jpeg_enc_item* items, int n, int quality, int subsampling, int bgr,
                          void* workspace, size_t ws_bytes, uint8_t* out, size_t out_cap, int64_t* out_off, void* stream) {
  if (!src || !workspace || !out || !out_off || quality < 1 || quality > 100 || (bgr != 0 && bgr != 1))
    return FP_ERR_INVALID_ARG;
  if (((uintptr_t)workspace) % 16 || ((uintptr_t)out_off) % 8) return FP_ERR_ALIGNMENT;
  EncLayout L;
  const int rc = plan(items, n, subsampling, L);
  if (rc != FP_OK) return rc;
  if (ws_bytes < L.total || out_cap < L.out_bytes) return FP_ERR_BOUNDS;
  std::vector<unsigned char> stage(L.off_blk, 0);           // tables + descriptors: one copy
  make_tables(*(EncTables*)(stage.data() + L.off_tab), quality);
  memcpy(stage.data() + L.off_img, L.imgs.data(), sizeof(EncImg) * n);
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyWithStream(ws, stage.data(), stage.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws + L.off_words, 0, sizeof(uint32_t) * L.n_words, s);
  if (e != hipSuccess) {
    fp_set_hip_error(e);
    return FP_ERR_LAUNCH;
  }
  EncParams P = params(L, n, bgr, src, ws, out, out_off);
  const unsigned nwg_blocks = (unsigned)ceil_div(L.n_blocks, 4);
  const unsigned nt_blocks = (unsigned)ceil_div(L.n_blocks, kTile), nt_words = (unsigned)ceil_div(L.n_words, kTile);
  hipLaunchKernelGGL(je_blocks, dim3(nwg_blocks), dim3(256), 0, s, P);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(je_dc, dim3((unsigned)ceil_div(L.n_blocks, 256)), dim3(256), 0, s, P);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(je_reduce<BitsCount>, dim3(nt_blocks), dim3(256), 0, s, P, L.n_blocks);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(je_scan_partials, dim3(1), dim3(256), 0, s, P.partial, (int64_t)nt_blocks, P.bit_off + L.n_blocks);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(je_bits_apply, dim3(nt_blocks), dim3(256), 0, s, P);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(je_emit, dim3(nwg_blocks), dim3(256), 0, s, P);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(je_reduce<StuffCount>, dim3(nt_words), dim3(256), 0, s, P, L.n_words);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(je_scan_partials, dim3(1), dim3(256), 0, s, P.partial, (int64_t)nt_words, out_off + n);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(je_stuff_apply, dim3(nt_words), dim3(256), 0, s, P, L.n_words);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

// The same phases, serially, on host memory.
int fp_jpeg_encode_emulate(const uint8_t* src, const fp_jpeg_enc_item* items, int n, int quality, int subsampling, int bgr,
                           uint8_t* out, size_t out_cap, int64_t* out_off) {
  if (!src || !out || !out_off || quality < 1 || quality > 100 || (bgr != 0 && bgr != 1)) return FP_ERR_INVALID_ARG;
  EncLayout L;
  const int rc = plan(items, n, subsampling, L);
  if (rc != FP_OK) return rc;
  if (out_cap < L.out_bytes) return FP_ERR_BOUNDS;
  std::vector<unsigned char> ws(L.total, 0);
  make_tables(*(EncTables*)(ws.data() + L.off_tab), quality);
  memcpy(ws.data() + L.off_img, L.imgs.data(), sizeof(EncImg) * n);
  EncParams P = params(L, n, bgr, src, ws.data(), out, out_off);
  const EncTables& T = *P.tab;
  for (int64_t b = 0; b < L.n_blocks; ++b) {                                         // je_blocks
    const int ii = find_img(P.img, n, b);
    const EncImg& im = P.img[ii];
    const BlockPos p = block_pos(im, P.hmax, P.vmax, P.bpm, (int)(b - im.block_off));
    int32_t d[64];
    if (p.real) {
      for (int lane = 0; lane < 64; ++lane)
        d[lane] = sample(src, im, bgr, P.hmax, P.vmax, p.comp, p.r * 8 + (lane >> 3), p.c * 8 + (lane & 7)) - 128;
      for (int i = 0; i < 8; ++i) fdct8(d + i * 8, 1, 0);
      for (int i = 0; i < 8; ++i) fdct8(d + i, 8, 1);
    }
    const int ci = p.comp ? 1 : 0;
    int v[64];
    uint64_t nz = 0;
    for (int lane = 0; lane < 64; ++lane) {
      const int nat = T.zigzag[lane];
      v[lane] = p.real ? quantize(d[nat], T.quant[ci], nat) : 0;
      P.coef[b * 64 + lane] = (int16_t)v[lane];
      if (lane > 0 && v[lane] != 0) nz |= 1ull << lane;
    }
    int bits = 0;
    for (int lane = 0; lane < 64; ++lane) {
      uint64_t val;
      int len;
      ac_lane(lane, v[lane], nz, T.huff[ci ? 3 : 1], val, len);
      bits += len;
    }
    P.bits[b] = bits;
    P.blk_img[b] = ii;
  }
  for (int64_t b = 0; b < L.n_blocks; ++b) block_dc(P, b);                         // je_dc
  int64_t acc = 0;                                                                   // the scan
  for (int64_t b = 0; b < L.n_blocks; ++b) {
    P.bit_off[b] = acc;
    acc += P.bits[b];
  }
  P.bit_off[L.n_blocks] = acc;
  for (int64_t b = 0; b < L.n_blocks; ++b) {                                         // je_emit
    const EncImg& im = P.img[P.blk_img[b]];
    const int ci = block_pos(im, P.hmax, P.vmax, P.bpm, (int)(b - im.block_off)).comp ? 1 : 0;
    uint64_t nz = 0;
    for (int lane = 1; lane < 64; ++lane)
      if (P.coef[b * 64 + lane]) nz |= 1ull << lane;
    int64_t pos = im.block_off * kWordsPerBlock * 32 + (P.bit_off[b] - P.bit_off[im.block_off]);
    for (int lane = 0; lane < 64; ++lane) {
      uint64_t val;
      int len;
      ac_lane(lane, P.coef[b * 64 + lane], nz, T.huff[ci ? 3 : 1], val, len);
      if (lane == 0) {
        uint64_t dv;
        int dl;
        dc_code(P.dcdiff[b], T.huff[ci ? 2 : 0], dv, dl);
        val |= dv << len;
        len += dl;
      }
      put_bits(P.words, pos, val, len);
      pos += len;
    }
  }
  int64_t off = 0;                                                                   // stuffing
  for (int64_t w = 0; w < L.n_words; ++w) {
    const WordBytes r = word_bytes(P, w);
    if (r.first) out_off[r.img] = off;
    for (int k = 0; k < r.n; ++k) {
      out[off++] = r.b[k];
      if (r.b[k] == 0xFF) out[off++] = 0;
    }
  }
  out_off[n] = off;
  return FP_OK;
}

}  // extern "C"
