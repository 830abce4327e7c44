// jpegscale.hip — the device half of the JPEG decode at libjpeg-turbo's scale_denom = 1 / 2 / 4 / 8, with the EXIF orientation
// applied to the scaled picture (gfx950 + host emulator).  cv2.imread(path, IMREAD_REDUCED_COLOR_2 / _4 / _8) hands the library
// scale_denom and turns the result upright by the Orientation tag; jpeg.hip's fp_jpeg_reconstruct stays the full-size, tag-1 path.
//
// At scale_denom s, m = 8 / s (jdmaster.c jpeg_calc_output_dimensions / use_merged_upsample off, jddctmgr.c start_pass):
//   output     ceil(W / s) x ceil(H / s)
//   luma       m x m samples per block
//   chroma     ss x ss per block, ss = m doubled while ss < 8 and (hmax m) % (h_c ss 2) == 0 and (vmax m) % (v_c ss 2) == 0
//              ("scale chroma up in the IDCT rather than by upsampling"): 4:2:0 gets 2m (capped at 8) and no upsampling below
//              full size, 4:2:2 stays at m with an h2v1 upsample, 4:4:4 and gray at m
//   planes     ceil(W h_c ss / (hmax 8)) x ceil(H v_c ss / (vmax 8))
//   upsampling fancy (triangle) only for m > 1 and a plane more than 2 samples wide (jdsample.c jinit_upsampler:
//              do_fancy = do_fancy_upsampling && min_DCT_scaled_size > 1), else replication
//   transforms jidctint.c islow 8 x 8; jidctred.c 4 x 4 (inputs 0 1 2 3 5 6 7 of a line), 2 x 2 (inputs 0 1 3 5 7), 1 x 1
//              ((dc q0 + 4) >> 3): CONST_BITS 13, PASS1_BITS 2, columns first, + 128, clamp
//   colour     jdcolor.c ycc_rgb_convert, as jpeg.hip
// Two kernels:
//   jpeg_idct_scaled_kernel   one thread per GROUP of 8 / ss horizontally adjacent blocks of a component: every row it
//                             produces is one 8-byte store (1 block at ss = 8, 2 at 4, 4 at 2, 8 at 1); it reads only the
//                             coefficient rows and columns the reduced transform uses (49, 25 or 1 of a block's 64)
//   jpeg_color_scaled_kernel  one workgroup per OUTPUT tile, four adjacent output pixels (12 bytes, three dword stores) per
//                             thread, so the interleaved stores are contiguous for all eight tags.  Tags 1 - 4 read the planes
//                             along rows as they are (forwards or backwards); tags 5 - 8 stage the tile's Y / Cb / Cr through
//                             LDS -- read along the planes' rows, written transposed into a tile padded to an odd pitch, read
//                             back along output rows: no bank conflicts either way
// Everything is integer arithmetic in __host__ __device__ functions; fp_jpeg_reconstruct_scaled_emulate runs the same functions
// serially on the CPU.  (This unit is built with -fwrapv: a damaged file's coefficients may overflow the 32-bit sums, which then
// wrap alike on both sides instead of being undefined.)
#include <string.h>

#include "common.h"

namespace {

struct ScaledInfo {
  int in_w, in_h;            // the scaled picture, before the orientation
  int out_w, out_h;          // the frame written
  int ncomp, orientation;
  int h2, v2, fancy;         // chroma: doubled across / down by the upsampler, with the triangle filters or by replication
  int ss[3];                 // samples per block side
  int groups_w[3];           // groups of 8 / ss blocks per block row
  int blocks_w[3], blocks_h[3];
  int pitch[3];              // plane row pitch, a multiple of 8
  int cw, ch;                // the chroma planes' true size (the upsampler's edges)
  long ngroups[3];
  long coef_off[3], plane_off[3];
  unsigned short quant[3][64];
};

#define FP_HD __host__ __device__ __forceinline__

FP_HD int sdescale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
FP_HD int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// jidctint.c jpeg_idct_islow, one 1-D pass
template <int SHIFT>
FP_HD void sidct8(const int in[8], int out[8]) {
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * 4433;
  const int tmp2 = z1 + z3 * (-15137);
  const int tmp3 = z1 + z2 * 6270;
  z2 = in[0];
  z3 = in[4];
  const int tmp0 = (z2 + z3) * 8192;
  const int tmp1 = (z2 - z3) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  int t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
  z1 = t0 + t3;
  z2 = t1 + t2;
  z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446;
  t1 *= 16819;
  t2 *= 25172;
  t3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 *= -16069;
  z4 *= -3196;
  z3 += z5;
  z4 += z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  out[0] = sdescale(tmp10 + t3, SHIFT);
  out[7] = sdescale(tmp10 - t3, SHIFT);
  out[1] = sdescale(tmp11 + t2, SHIFT);
  out[6] = sdescale(tmp11 - t2, SHIFT);
  out[2] = sdescale(tmp12 + t1, SHIFT);
  out[5] = sdescale(tmp12 - t1, SHIFT);
  out[3] = sdescale(tmp13 + t0, SHIFT);
  out[4] = sdescale(tmp13 - t0, SHIFT);
}

// jidctred.c jpeg_idct_4x4, one 1-D pass: inputs 0 1 2 3 5 6 7 of the line (4 is not used)
template <int SHIFT>
FP_HD void sidct4(int i0, int i1, int i2, int i3, int i5, int i6, int i7, int out[4]) {
  const int t0 = i0 * 16384;
  const int t2 = i2 * 15137 - i6 * 6270;
  const int a = t0 + t2, b = t0 - t2;
  const int o0 = -i7 * 1730 + i5 * 11893 - i3 * 17799 + i1 * 8697;
  const int o2 = -i7 * 4176 - i5 * 4926 + i3 * 7373 + i1 * 20995;
  out[0] = sdescale(a + o2, SHIFT);
  out[3] = sdescale(a - o2, SHIFT);
  out[1] = sdescale(b + o0, SHIFT);
  out[2] = sdescale(b - o0, SHIFT);
}

// jidctred.c jpeg_idct_2x2, one 1-D pass: inputs 0 1 3 5 7
template <int SHIFT>
FP_HD void sidct2(int i0, int i1, int i3, int i5, int i7, int out[2]) {
  const int t = i0 * 32768;
  const int o = -i7 * 5906 + i5 * 6967 - i3 * 10426 + i1 * 29692;
  out[0] = sdescale(t + o, SHIFT);
  out[1] = sdescale(t - o, SHIFT);
}

FP_HD void store8(unsigned char* dst, unsigned long long v) {
#ifdef __HIP_DEVICE_COMPILE__
  *(unsigned long long*)dst = v;               // plane offsets and pitches are multiples of 8, the workspace is 8-byte aligned
#else
  memcpy(dst, &v, 8);
#endif
}

// One block: dequantise, columns, rows, + 128, clamp.  rows[r] receives the block's ss samples of its row r in the low bytes.
FP_HD void block8(const short* src, const unsigned short* q, unsigned long long rows[8]) {
  int ws[64];
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    int in[8], out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = (int)src[r * 8 + col] * (int)q[r * 8 + col];
    sidct8<11>(in, out);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[r * 8 + col] = out[r];
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int in[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = ws[r * 8 + k];
    sidct8<18>(in, out);
    unsigned long long packed = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) packed |= (unsigned long long)clamp255(out[k] + 128) << (8 * k);
    rows[r] = packed;
  }
}

FP_HD void block4(const short* src, const unsigned short* q, unsigned rows[4]) {
  int ws[4][8];                                 // [output row][column]; column 4 stays unused
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    if (col == 4) continue;
#define FP_DQ(r) ((int)src[(r) * 8 + col] * (int)q[(r) * 8 + col])
    int out[4];
    sidct4<12>(FP_DQ(0), FP_DQ(1), FP_DQ(2), FP_DQ(3), FP_DQ(5), FP_DQ(6), FP_DQ(7), out);
#undef FP_DQ
#pragma unroll
    for (int r = 0; r < 4; ++r) ws[r][col] = out[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int out[4];
    sidct4<19>(ws[r][0], ws[r][1], ws[r][2], ws[r][3], ws[r][5], ws[r][6], ws[r][7], out);
    unsigned packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) packed |= (unsigned)clamp255(out[k] + 128) << (8 * k);
    rows[r] = packed;
  }
}

FP_HD void block2(const short* src, const unsigned short* q, unsigned rows[2]) {
  int ws[2][8];                                 // columns 0 1 3 5 7 are used
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    if (col != 0 && !(col & 1)) continue;
#define FP_DQ(r) ((int)src[(r) * 8 + col] * (int)q[(r) * 8 + col])
    int out[2];
    sidct2<13>(FP_DQ(0), FP_DQ(1), FP_DQ(3), FP_DQ(5), FP_DQ(7), out);
#undef FP_DQ
    ws[0][col] = out[0];
    ws[1][col] = out[1];
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    int out[2];
    sidct2<20>(ws[r][0], ws[r][1], ws[r][3], ws[r][5], ws[r][7], out);
    rows[r] = (unsigned)clamp255(out[0] + 128) | ((unsigned)clamp255(out[1] + 128) << 8);
  }
}

FP_HD unsigned block1(const short* src, const unsigned short* q) { return (unsigned)clamp255((((int)src[0] * (int)q[0] + 4) >> 3) + 128); }

// Group g (over all components, component-major) -> its 8-byte row segments of the component's sample plane.  A group past
// the end of a block row (blocks_w no multiple of 8 / ss) fills the rest of its segment with zeros: the pitch has room for it.
FP_HD void idct_group(const short* coefs, unsigned char* planes, const ScaledInfo& d, long g) {
  int c = 0;
  while (c + 1 < d.ncomp && g >= d.ngroups[c]) g -= d.ngroups[c], ++c;
  const int gx = (int)(g % d.groups_w[c]), by = (int)(g / d.groups_w[c]);
  const int ss = d.ss[c], per = 8 / ss;
  const int bx0 = gx * per;
  const int nb = d.blocks_w[c] - bx0 < per ? d.blocks_w[c] - bx0 : per;
  const short* src = coefs + d.coef_off[c] + ((long)by * d.blocks_w[c] + bx0) * 64;
  const unsigned short* q = d.quant[c];
  unsigned char* dst = planes + d.plane_off[c] + ((long)by * ss) * d.pitch[c] + gx * 8;
  if (ss == 8) {
    unsigned long long rows[8];
    block8(src, q, rows);
#pragma unroll
    for (int r = 0; r < 8; ++r) store8(dst + (long)r * d.pitch[c], rows[r]);
  } else if (ss == 4) {
    unsigned long long acc[4] = {0, 0, 0, 0};
    for (int b = 0; b < nb; ++b) {
      unsigned rows[4];
      block4(src + b * 64, q, rows);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] |= (unsigned long long)rows[r] << (32 * b);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) store8(dst + (long)r * d.pitch[c], acc[r]);
  } else if (ss == 2) {
    unsigned long long acc[2] = {0, 0};
    for (int b = 0; b < nb; ++b) {
      unsigned rows[2];
      block2(src + b * 64, q, rows);
      acc[0] |= (unsigned long long)rows[0] << (16 * b);
      acc[1] |= (unsigned long long)rows[1] << (16 * b);
    }
    store8(dst, acc[0]);
    store8(dst + d.pitch[c], acc[1]);
  } else {
    unsigned long long acc = 0;
    for (int b = 0; b < nb; ++b) acc |= (unsigned long long)block1(src + b * 64, q) << (8 * b);
    store8(dst, acc);
  }
}

// chroma sample of the scaled picture's pixel (iy, ix): jdsample.c's upsamplers, as jpeg.hip's chroma_sample
FP_HD int chroma_at(const unsigned char* pl, int pitch, const ScaledInfo& d, int iy, int ix) {
  if (!d.h2) return pl[(long)iy * pitch + ix];                        // no upsampling (fullsize_upsample)
  const int cx = ix >> 1, hodd = ix & 1;
  if (!d.fancy) return pl[(long)(d.v2 ? iy >> 1 : iy) * pitch + cx];   // h2v1_upsample / h2v2_upsample
  if (!d.v2) {                                                        // h2v1_fancy_upsample
    const unsigned char* r = pl + (long)iy * pitch;
    const int cur = r[cx];
    if (!hodd) return cx == 0 ? cur : (cur * 3 + r[cx - 1] + 1) >> 2;
    return cx == d.cw - 1 ? cur : (cur * 3 + r[cx + 1] + 2) >> 2;
  }
  // h2v2_fancy_upsample: the nearer row counts 3/4, the further (above for even rows, below for odd) 1/4
  const int cy = iy >> 1;
  const int cy1 = (iy & 1) ? (cy + 1 < d.ch ? cy + 1 : d.ch - 1) : (cy > 0 ? cy - 1 : 0);
  const unsigned char* r0 = pl + (long)cy * pitch;
  const unsigned char* r1 = pl + (long)cy1 * pitch;
  const int cur = r0[cx] * 3 + r1[cx];
  if (!hodd) {
    if (cx == 0) return (cur * 4 + 8) >> 4;
    return (cur * 3 + (r0[cx - 1] * 3 + r1[cx - 1]) + 8) >> 4;
  }
  if (cx == d.cw - 1) return (cur * 4 + 7) >> 4;
  return (cur * 3 + (r0[cx + 1] * 3 + r1[cx + 1]) + 7) >> 4;
}

// Y | Cb << 8 | Cr << 16 of the scaled picture's pixel (iy, ix), chroma upsampled; a gray file: Y alone
FP_HD unsigned ycc_at(const unsigned char* planes, const ScaledInfo& d, int iy, int ix) {
  unsigned v = planes[d.plane_off[0] + (long)iy * d.pitch[0] + ix];
  if (d.ncomp == 3) {
    v |= (unsigned)chroma_at(planes + d.plane_off[1], d.pitch[1], d, iy, ix) << 8;
    v |= (unsigned)chroma_at(planes + d.plane_off[2], d.pitch[2], d, iy, ix) << 16;
  }
  return v;
}

// jdcolor.c ycc_rgb_convert (SCALEBITS 16) -> the pixel's three bytes in output order, in the low 24 bits
FP_HD unsigned ycc_to_pixel(unsigned ycc, int ncomp, int bgr) {
  const int y = (int)(ycc & 255);
  if (ncomp == 1) return (unsigned)y * 0x010101u;
  const int cb = (int)((ycc >> 8) & 255) - 128, cr = (int)((ycc >> 16) & 255) - 128;
  const int r = clamp255(y + ((91881 * cr + 32768) >> 16));
  const int b = clamp255(y + ((116130 * cb + 32768) >> 16));
  const int g = clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  return bgr ? (unsigned)b | ((unsigned)g << 8) | ((unsigned)r << 16) : (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

// output pixel (y, x) -> the scaled picture's pixel, by the orientation tag
FP_HD void orient(const ScaledInfo& d, int y, int x, int& iy, int& ix) {
  const int o = d.orientation;
  const int a = o >= 5 ? x : y, b = o >= 5 ? y : x;                    // 5 .. 8 transpose
  const bool flip_r = o == 3 || o == 4 || o == 6 || o == 7;
  const bool flip_c = o == 2 || o == 3 || o == 7 || o == 8;
  iy = flip_r ? d.in_h - 1 - a : a;
  ix = flip_c ? d.in_w - 1 - b : b;
}

// up to four pixels (low 24 bits each) -> the 3 n bytes at o: three dword stores for a full quad that starts on a dword (the
// quad's x is a multiple of 4, so every quad of a row does when the row does: always for a width that is a multiple of 4)
FP_HD void store_quad(unsigned char* o, const unsigned px[4], int n) {
#ifdef __HIP_DEVICE_COMPILE__
  if (n == 4 && ((unsigned long long)o & 3) == 0) {
    unsigned* w = (unsigned*)o;
    w[0] = px[0] | (px[1] << 24);
    w[1] = (px[1] >> 8) | (px[2] << 16);
    w[2] = (px[2] >> 16) | (px[3] << 8);
    return;
  }
#endif
  for (int k = 0; k < n; ++k) {
    o[3 * k] = (unsigned char)px[k];
    o[3 * k + 1] = (unsigned char)(px[k] >> 8);
    o[3 * k + 2] = (unsigned char)(px[k] >> 16);
  }
}

__global__ __launch_bounds__(64) void jpeg_idct_scaled_kernel(const short* coefs, unsigned char* planes, ScaledInfo d, long ngroups_total) {
  const long g = (long)blockIdx.x * 64 + threadIdx.x;
  if (g >= ngroups_total) return;
  idct_group(coefs, planes, d, g);
}

// Tags 1 - 4: a 16-row x 64-pixel output tile per workgroup, four adjacent pixels per thread (16 threads = 192 contiguous output
// bytes per row); the planes are read along their rows, forwards or backwards.
#define CT_W 64
#define CT_H 16
__global__ __launch_bounds__(256) void jpeg_color_scaled_kernel(const unsigned char* planes, unsigned char* out, ScaledInfo d, int tiles_x,
                                                                int bgr) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y = ty * CT_H + (int)(threadIdx.x >> 4), x0 = tx * CT_W + (int)(threadIdx.x & 15) * 4;
  if (y >= d.out_h || x0 >= d.out_w) return;
  const int n = d.out_w - x0 < 4 ? d.out_w - x0 : 4;
  unsigned px[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < n) {
      int iy, ix;
      orient(d, y, x0 + k, iy, ix);
      px[k] = ycc_to_pixel(ycc_at(planes, d, iy, ix), d.ncomp, bgr);
    }
  }
  store_quad(out + ((long)y * d.out_w + x0) * 3, px, n);
}

// Tags 5 - 8: a 32 x 32 output tile per workgroup.  Load phase: lanes run along the OUTPUT tile's rows y, which is along a row
// of the planes (32 contiguous samples, forwards or backwards), and write the packed Y / Cb / Cr dword transposed into
// tile[y][x], pitch 33: 32 lanes -> 32 banks.  Store phase: a thread takes tile[y][4 q .. 4 q + 3]: lanes (y = 0 .. 3, q = 0 .. 7)
// of a half wave hit banks y 33 + 4 q + k, all different.
#define TT 32
#define TT_PITCH 33
__global__ __launch_bounds__(256) void jpeg_color_scaled_transpose_kernel(const unsigned char* planes, unsigned char* out, ScaledInfo d,
                                                                          int tiles_x, int bgr) {
  __shared__ unsigned tile[TT * TT_PITCH];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * TT, x0 = tx * TT;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (int)threadIdx.x + 256 * i;
    const int ly = j & 31, lx = j >> 5;
    const int y = y0 + ly, x = x0 + lx;
    if (y < d.out_h && x < d.out_w) {
      int iy, ix;
      orient(d, y, x, iy, ix);
      tile[ly * TT_PITCH + lx] = ycc_at(planes, d, iy, ix);
    }
  }
  __syncthreads();
  const int q = (int)(threadIdx.x & 7), ly = (int)(threadIdx.x >> 3);
  const int y = y0 + ly, x = x0 + 4 * q;
  if (y >= d.out_h || x >= d.out_w) return;
  const int n = d.out_w - x < 4 ? d.out_w - x : 4;
  unsigned px[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n) px[k] = ycc_to_pixel(tile[ly * TT_PITCH + 4 * q + k], d.ncomp, bgr);
  store_quad(out + ((long)y * d.out_w + x) * 3, px, n);
}

bool valid_args(const fp_jpeg_info* info, int s, int o) {
  if (!info || (s != 1 && s != 2 && s != 4 && s != 8) || o < 1 || o > 8) return false;
  if (info->width <= 0 || info->height <= 0 || info->width > 65535 || info->height > 65535) return false;
  if (info->ncomp != 1 && info->ncomp != 3) return false;
  for (int c = 0; c < info->ncomp; ++c)
    if (info->blocks_w[c] <= 0 || info->blocks_h[c] <= 0 || info->blocks_w[c] > 8192 || info->blocks_h[c] > 8192 || info->coef_off[c] < 0 ||
        info->coef_off[c] + (int64_t)info->blocks_w[c] * info->blocks_h[c] * 64 > info->n_coefs)
      return false;
  if (info->ncomp == 3) {
    if (info->hs[1] != 1 || info->vs[1] != 1 || info->hs[2] != 1 || info->vs[2] != 1) return false;
    const int h = info->hs[0], v = info->vs[0];
    if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2))) return false;
    if (info->blocks_w[1] != info->blocks_w[2] || info->blocks_h[1] != info->blocks_h[2]) return false;
  }
  return true;
}

// The geometry of a scaled decode; false for arguments outside the decoder's scope or planes the info's block counts do not cover.
bool make_info(const fp_jpeg_info* info, int s, int o, ScaledInfo& d) {
  if (!valid_args(info, s, o)) return false;
  memset(&d, 0, sizeof(d));
  const int m = 8 / s;
  const int hmax = info->ncomp == 3 ? info->hs[0] : 1, vmax = info->ncomp == 3 ? info->vs[0] : 1;
  d.in_w = (info->width + s - 1) / s;
  d.in_h = (info->height + s - 1) / s;
  d.out_w = o >= 5 ? d.in_h : d.in_w;
  d.out_h = o >= 5 ? d.in_w : d.in_h;
  d.ncomp = info->ncomp;
  d.orientation = o;
  long poff = 0;
  for (int c = 0; c < info->ncomp; ++c) {
    const int hc = info->ncomp == 3 ? info->hs[c] : 1, vc = info->ncomp == 3 ? info->vs[c] : 1;
    int ss = m;
    while (ss < 8 && (hmax * m) % (hc * ss * 2) == 0 && (vmax * m) % (vc * ss * 2) == 0) ss *= 2;
    d.ss[c] = ss;
    d.blocks_w[c] = info->blocks_w[c];
    d.blocks_h[c] = info->blocks_h[c];
    d.groups_w[c] = (info->blocks_w[c] * ss + 7) / 8;
    d.ngroups[c] = (long)d.groups_w[c] * info->blocks_h[c];
    d.pitch[c] = d.groups_w[c] * 8;
    d.coef_off[c] = info->coef_off[c];
    d.plane_off[c] = poff;
    poff += (long)d.pitch[c] * info->blocks_h[c] * ss;
    memcpy(d.quant[c], info->quant[c], 128);
    // the component's scaled size must lie inside what its blocks produce
    const long pw = ((long)info->width * hc * ss + hmax * 8 - 1) / (hmax * 8), ph = ((long)info->height * vc * ss + vmax * 8 - 1) / (vmax * 8);
    if (pw > (long)info->blocks_w[c] * ss || ph > (long)info->blocks_h[c] * ss) return false;
    if (c == 1) {
      d.cw = (int)pw;
      d.ch = (int)ph;
      d.h2 = (hmax * m) / (hc * ss) == 2;
      d.v2 = (vmax * m) / (vc * ss) == 2;
      d.fancy = d.h2 && m > 1 && d.cw > 2;
    }
  }
  return true;
}

long total_groups(const ScaledInfo& d) {
  long n = 0;
  for (int c = 0; c < d.ncomp; ++c) n += d.ngroups[c];
  return n;
}

size_t plane_bytes(const ScaledInfo& d) {
  const int c = d.ncomp - 1;
  return (size_t)(d.plane_off[c] + (long)d.pitch[c] * d.blocks_h[c] * d.ss[c]);
}

}  // namespace

extern "C" {

int fp_jpeg_scaled_size(const fp_jpeg_info* info, int scale_denom, int orientation, int* out_h, int* out_w) {
  ScaledInfo d;
  if (!out_h || !out_w || !make_info(info, scale_denom, orientation, d)) return FP_ERR_INVALID_ARG;
  *out_h = d.out_h;
  *out_w = d.out_w;
  return FP_OK;
}

size_t fp_jpeg_scaled_workspace_bytes(const fp_jpeg_info* info, int scale_denom) {
  ScaledInfo d;
  if (!make_info(info, scale_denom, 1, d)) return 0;
  return (plane_bytes(d) + 15) / 16 * 16;
}

int fp_jpeg_reconstruct_scaled(const int16_t* coefs, const fp_jpeg_info* info, int scale_denom, int orientation, uint8_t* workspace,
                               size_t ws_bytes, uint8_t* out, int bgr, void* stream) {
  if (!coefs || !info || !workspace || !out) return FP_ERR_INVALID_ARG;
  ScaledInfo d;
  if (!make_info(info, scale_denom, orientation, d)) return FP_ERR_INVALID_ARG;
  if (ws_bytes < plane_bytes(d)) return FP_ERR_BOUNDS;
  if (((uintptr_t)workspace) % 8 || ((uintptr_t)coefs) % 2 || ((uintptr_t)out) % 4) return FP_ERR_ALIGNMENT;
  hipStream_t s = (hipStream_t)stream;
  const long ng = total_groups(d);
  hipLaunchKernelGGL(jpeg_idct_scaled_kernel, dim3((unsigned)((ng + 63) / 64)), dim3(64), 0, s, (const short*)coefs, workspace, d, ng);
  FP_CHECK_LAUNCH();
  if (orientation <= 4) {
    const int tx = (d.out_w + CT_W - 1) / CT_W, ty = (d.out_h + CT_H - 1) / CT_H;
    hipLaunchKernelGGL(jpeg_color_scaled_kernel, dim3((unsigned)(tx * ty)), dim3(256), 0, s, workspace, out, d, tx, bgr);
  } else {
    const int tx = (d.out_w + TT - 1) / TT, ty = (d.out_h + TT - 1) / TT;
    hipLaunchKernelGGL(jpeg_color_scaled_transpose_kernel, dim3((unsigned)(tx * ty)), dim3(256), 0, s, workspace, out, d, tx, bgr);
  }
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_jpeg_reconstruct_scaled_emulate(const int16_t* coefs, const fp_jpeg_info* info, int scale_denom, int orientation,
                                       uint8_t* workspace, size_t ws_bytes, uint8_t* out, int bgr) {
  if (!coefs || !info || !workspace || !out) return FP_ERR_INVALID_ARG;
  ScaledInfo d;
  if (!make_info(info, scale_denom, orientation, d)) return FP_ERR_INVALID_ARG;
  if (ws_bytes < plane_bytes(d)) return FP_ERR_BOUNDS;
  const long ng = total_groups(d);
  for (long g = 0; g < ng; ++g) idct_group((const short*)coefs, workspace, d, g);
  for (int y = 0; y < d.out_h; ++y)
    for (int x = 0; x < d.out_w; x += 4) {
      const int n = d.out_w - x < 4 ? d.out_w - x : 4;
      unsigned px[4] = {0, 0, 0, 0};
      for (int k = 0; k < n; ++k) {
        int iy, ix;
        orient(d, y, x + k, iy, ix);
        px[k] = ycc_to_pixel(ycc_at(workspace, d, iy, ix), d.ncomp, bgr);
      }
      store_quad(out + ((long)y * d.out_w + x) * 3, px, n);
    }
  return FP_OK;
}

}  // extern "C"
