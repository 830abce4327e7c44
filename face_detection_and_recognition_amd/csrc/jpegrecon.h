// jpegrecon.h -- the device arithmetic of JPEG reconstruction at full size, shared by the per-frame kernels (csrc/jpeg.hip) and
// the batched kernels for frames of one geometry (csrc/jpegbatch.hip): dequantisation + jidctint.c's "islow" inverse DCT of one
// block, jdsample.c's chroma upsampling of one sample, jdcolor.c's YCbCr -> RGB of one pixel.  Integer arithmetic restated from
// libjpeg's published algorithm; one copy, so that both paths give the same bytes.
#pragma once
#include <string.h>

#include "common.h"

struct JpegDevInfo {
  int width, height, ncomp, hs0, vs0;
  int blocks_w[3], blocks_h[3], comp_w[3], comp_h[3];
  long coef_off[3], plane_off[3];
  unsigned short quant[3][64];
};

// jidctint.c jpeg_idct_islow: CONST_BITS = 13, PASS1_BITS = 2
#define JF_0_298631336 2446
#define JF_0_390180644 3196
#define JF_0_541196100 4433
#define JF_0_765366865 6270
#define JF_0_899976223 7373
#define JF_1_175875602 9633
#define JF_1_501321110 12299
#define JF_1_847759065 15137
#define JF_1_961570560 16069
#define JF_2_053119869 16819
#define JF_2_562915447 20995
#define JF_3_072711026 25172

__device__ __forceinline__ int jdescale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of the islow transform on eight values; SHIFT = the pass's descale
template <int SHIFT, bool FIRST>
__device__ __forceinline__ void idct8(const int in[8], int out[8]) {
  // even part
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * JF_0_541196100;
  const int tmp2 = z1 + z3 * (-JF_1_847759065);
  const int tmp3 = z1 + z2 * JF_0_765366865;
  z2 = in[0];
  z3 = in[4];
  const int tmp0 = (z2 + z3) << 13;
  const int tmp1 = (z2 - z3) << 13;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  // odd part
  int t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
  z1 = t0 + t3;
  z2 = t1 + t2;
  z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * JF_1_175875602;
  t0 *= JF_0_298631336;
  t1 *= JF_2_053119869;
  t2 *= JF_3_072711026;
  t3 *= JF_1_501321110;
  z1 *= -JF_0_899976223;
  z2 *= -JF_2_562915447;
  z3 *= -JF_1_961570560;
  z4 *= -JF_0_390180644;
  z3 += z5;
  z4 += z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  out[0] = jdescale(tmp10 + t3, SHIFT);
  out[7] = jdescale(tmp10 - t3, SHIFT);
  out[1] = jdescale(tmp11 + t2, SHIFT);
  out[6] = jdescale(tmp11 - t2, SHIFT);
  out[2] = jdescale(tmp12 + t1, SHIFT);
  out[5] = jdescale(tmp12 - t1, SHIFT);
  out[3] = jdescale(tmp13 + t0, SHIFT);
  out[4] = jdescale(tmp13 - t0, SHIFT);
}

// the component and the block inside it of block b of a frame whose components' blocks stand one after the other
__device__ __forceinline__ int jpeg_block_component(const JpegDevInfo& info, long& bb) {
  int c = 0;
  while (c + 1 < info.ncomp && bb >= (long)info.blocks_w[c] * info.blocks_h[c]) bb -= (long)info.blocks_w[c] * info.blocks_h[c], ++c;
  return c;
}

// One 8 x 8 block: dequantise by q (natural order), columns (descale 11), rows (descale 18), + 128, clamp -> eight rows of
// eight samples at dst (8-byte aligned), pitch bytes apart.
__device__ __forceinline__ void jpeg_idct_block(const short* src, const unsigned short* q, unsigned char* dst, long pitch) {
  int ws[64];
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    int in[8], out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = (int)src[r * 8 + col] * (int)q[r * 8 + col];
    idct8<11, true>(in, out);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[r * 8 + col] = out[r];
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int in[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = ws[r * 8 + k];
    idct8<18, false>(in, out);
    unsigned long long packed = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int v = min(max(out[k] + 128, 0), 255);      // range_limit (jdmaster.c prepare_range_limit_table)
      packed |= (unsigned long long)v << (8 * k);
    }
    *(unsigned long long*)(dst + (long)r * pitch) = packed;
  }
}

// chroma sample for output pixel (oy, ox) by libjpeg's upsampling (jdsample.c); plane row pitch = pitch, the component's
// true size = cw x ch (edges replicate inside it).  jinit_upsampler takes the fancy (triangle) filters only for
// downsampled_width > 2; a component 1 or 2 samples wide gets plain replication (h2v1_upsample / h2v2_upsample), down as
// well as across
__device__ __forceinline__ int chroma_sample(const unsigned char* pl, int pitch, int cw, int ch, int oy, int ox, int hs0, int vs0) {
  if (hs0 == 1) return pl[(long)oy * pitch + ox];                      // 4:4:4 (vs0 == 1 too)
  const int cx = ox >> 1, hodd = ox & 1;
  if (cw <= 2) return pl[(long)(vs0 == 1 ? oy : oy >> 1) * pitch + cx];   // h2v1_upsample / h2v2_upsample
  if (vs0 == 1) {                                                      // h2v1_fancy_upsample
    const unsigned char* r = pl + (long)oy * pitch;
    const int cur = r[cx];
    if (!hodd) return cx == 0 ? cur : (cur * 3 + r[cx - 1] + 1) >> 2;
    return cx == cw - 1 ? cur : (cur * 3 + r[cx + 1] + 2) >> 2;
  }
  // h2v2_fancy_upsample: the nearer row counts 3/4, the further (above for even output rows, below for odd) 1/4
  const int cy = oy >> 1;
  const int cy1 = (oy & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const unsigned char* r0 = pl + (long)cy * pitch;
  const unsigned char* r1 = pl + (long)cy1 * pitch;
  const int cur = r0[cx] * 3 + r1[cx];
  if (!hodd) {
    if (cx == 0) return (cur * 4 + 8) >> 4;
    return (cur * 3 + (r0[cx - 1] * 3 + r1[cx - 1]) + 8) >> 4;
  }
  if (cx == cw - 1) return (cur * 4 + 7) >> 4;
  return (cur * 3 + (r0[cx + 1] * 3 + r1[cx + 1]) + 7) >> 4;
}

// One output pixel (oy, ox) of a frame whose sample planes stand at `planes`: upsample + ycc_rgb_convert (jdcolor.c:
// SCALEBITS 16) -> three interleaved bytes at o
__device__ __forceinline__ void jpeg_color_pixel(const unsigned char* planes, unsigned char* o, const JpegDevInfo& info, int oy, int ox,
                                                 int bgr) {
  const int y = planes[info.plane_off[0] + (long)oy * (info.blocks_w[0] * 8) + ox];
  int r, g, b;
  if (info.ncomp == 1) {
    r = g = b = y;
  } else {
    const int cb = chroma_sample(planes + info.plane_off[1], info.blocks_w[1] * 8, info.comp_w[1], info.comp_h[1], oy, ox, info.hs0, info.vs0) - 128;
    const int cr = chroma_sample(planes + info.plane_off[2], info.blocks_w[2] * 8, info.comp_w[2], info.comp_h[2], oy, ox, info.hs0, info.vs0) - 128;
    // FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554, ONE_HALF = 32768
    r = y + ((91881 * cr + 32768) >> 16);
    b = y + ((116130 * cb + 32768) >> 16);
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    r = min(max(r, 0), 255);
    g = min(max(g, 0), 255);
    b = min(max(b, 0), 255);
  }
  o[0] = (unsigned char)(bgr ? b : r);
  o[1] = (unsigned char)g;
  o[2] = (unsigned char)(bgr ? r : b);
}

// fp_jpeg_info -> the kernels' argument (planes one after the other, quant copied); false for a component without blocks
inline bool jpeg_dev_info(const fp_jpeg_info* info, JpegDevInfo& d, long& nblocks, long& plane_bytes) {
  memset(&d, 0, sizeof(d));
  d.width = info->width;
  d.height = info->height;
  d.ncomp = info->ncomp;
  d.hs0 = info->hs[0];
  d.vs0 = info->vs[0];
  nblocks = 0;
  long poff = 0;
  for (int c = 0; c < info->ncomp; ++c) {
    if (info->blocks_w[c] <= 0 || info->blocks_h[c] <= 0) return false;
    d.blocks_w[c] = info->blocks_w[c];
    d.blocks_h[c] = info->blocks_h[c];
    d.comp_w[c] = info->comp_w[c];
    d.comp_h[c] = info->comp_h[c];
    d.coef_off[c] = info->coef_off[c];
    d.plane_off[c] = poff;
    poff += (long)info->blocks_w[c] * 8 * info->blocks_h[c] * 8;
    nblocks += (long)info->blocks_w[c] * info->blocks_h[c];
    memcpy(d.quant[c], info->quant[c], 128);
  }
  plane_bytes = poff;
  return true;
}
