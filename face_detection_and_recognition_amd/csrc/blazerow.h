// blazerow.h -- the row step the BlazeFace kernels on row-padded 24-channel maps share (blazewp.hip, blazepair.hip; gfx950).
//
// A WAVE makes one row of 32 pixels x C channels of  y = ReLU( pw1x1( dw3x3(x) ) + x ):
//   * depthwise: 48 of the 64 lanes take an item of 4 pixels x 4 channels (8 pixel groups x C/4 channel groups); the 3 x 6 pixel
//     window of an item is six 16-byte loads per row, the taps and the bias come from LDS (Ws: [10][C] per block);
//   * the 32 x C result goes through the wave's A tile in LDS ([32][C + 4]) to the MFMA pipe: fp32 32x32x2 MFMAs against the
//     1x1 weights, which every lane holds as B fragments in registers for the whole kernel.  The operands are SWAPPED
//     (D^T = W^T x A^T): lane (lr, h) ends up with PIXEL lr and channels (k & 3) + 8 * (k >> 2) + 4h of accumulator register k
//     -- four consecutive channels per register quad, 16-byte pieces of a row-major pixel, so an epilogue is C / 8 x (b128
//     read, packed adds, b128 write) instead of 16 + 16 scalar LDS accesses;
//   * the shortcut (the window's centre tap) carries the 1x1 bias from the depthwise phase on.
// The pair kernels keep the result row in an LDS ring of four rows (blazepair.hip); blaze_ring_step is that whole step.
// Every floating-point statement keeps one form for all users: the kernels' results are equal bit for bit.
#pragma once
#include "common.h"

namespace {

// What a lane does in a row step; built once per kernel.  x0 = first pixel of the wave's strip in a ring row (ring kernels).
template <int C>
struct BlazeLanes {
  static constexpr int C4 = C / 4;
  int lane, lr, h;        // MFMA side: pixel lr of the tile, channels 4h .. 4h + 3 (+ 8j)
  bool dw_lane;           // depthwise item of this lane: pixels 4g .. 4g + 3 of the tile, channels 4c4 .. 4c4 + 3 (lanes >= 8 C4
  int g, c4;              // repeat item 0 and write nothing)
  unsigned voff_in;       // byte offset of the item's window in an input row whose origin is the pixel left of the tile
  int x0;
  int rg_dw;              // ring column x0 + 4g - 1 of this lane's channels
  int rg_ep;              // epilogue: ring pixel x0 + lr, channels 4h (+ 8j)
  __device__ __forceinline__ explicit BlazeLanes(int tid, int x0_ = 0) : x0(x0_) {
    lane = tid & 63;
    lr = lane & 31, h = lane >> 5;
    dw_lane = lane < 8 * C4;
    const int la = dw_lane ? lane : 0;
    g = la / C4, c4 = la - g * C4;
    voff_in = (unsigned)((4 * g * C + 4 * c4) * 4);
    rg_dw = (x0 + 4 * g) * C + 4 * c4;
    rg_ep = (x0 + 1 + lr) * C + 4 * h;
  }
};

// One window row of a depthwise item: six pixels, 16 bytes each.
template <int C>
__device__ __forceinline__ void blaze_load_row(f32x4 (&x)[6], const char* rowp, unsigned voff_in) {
#pragma unroll
  for (int j = 0; j < 6; ++j) x[j] = *(const f32x4*)(rowp + voff_in + j * C * 4);
}

// 3x3 depthwise (stride S) of four output pixels x four channels: rows r0, r1, r2 hold the 3 S + 3 window pixels PX f32x4s
// apart (1: a row in registers; C / 4: a ring row in LDS), wl = this lane's taps [k][4] at wl + k C, bias at k = 9.
template <int S, int C, int PX>
__device__ __forceinline__ void blaze_dw3x3(f32x4 (&acc)[4], const f32x4* r0, const f32x4* r1, const f32x4* r2, const float* wl) {
  const f32x4 dbias = *(const f32x4*)(wl + 9 * C);
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = dbias;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const f32x4* rr = ky == 0 ? r0 : ky == 1 ? r1 : r2;
    f32x4 xv[3 * S + 3];
#pragma unroll
    for (int j = 0; j < 3 * S + 3; ++j) xv[j] = rr[j * PX];
    const f32x4 w0 = *(const f32x4*)(wl + (ky * 3 + 0) * C);
    const f32x4 w1 = *(const f32x4*)(wl + (ky * 3 + 1) * C);
    const f32x4 w2 = *(const f32x4*)(wl + (ky * 3 + 2) * C);
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // three statements: each contracts to one packed FMA on the accumulator
      acc[q] += xv[S * q] * w0;
      acc[q] += xv[S * q + 1] * w1;
      acc[q] += xv[S * q + 2] * w2;
    }
  }
}

// The depthwise item -> the wave's A tile [32][LDT].
template <int C, int LDT>
__device__ __forceinline__ void blaze_store_a(float* At, const BlazeLanes<C>& ln, const f32x4 (&acc)[4]) {
  if (ln.dw_lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *(f32x4*)&At[(4 * ln.g + q) * LDT + 4 * ln.c4] = acc[q];
  }
}

// 1x1 with swapped operands: m0 + m1 = (32 output channels of bf) x (the 32 pixels of the A tile); arow = &At[lr * LDT + 4 h].
template <int KG>
__device__ __forceinline__ void blaze_pw_swapped(const float* arow, const f32x4 (&bf)[KG], f32x16& m0, f32x16& m1) {
#pragma unroll
  for (int k = 0; k < 16; ++k) m0[k] = 0.f, m1[k] = 0.f;
#pragma unroll
  for (int kq = 0; kq < KG; ++kq) {
    const f32x4 a = *(const f32x4*)(arow + kq * 8);
    m0 = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[kq][0], a[0], m0, 0, 0, 0);
    FP_MFMA_ORDER();
    m1 = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[kq][1], a[1], m1, 0, 0, 0);
    FP_MFMA_ORDER();
    m0 = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[kq][2], a[2], m0, 0, 0, 0);
    FP_MFMA_ORDER();
    m1 = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[kq][3], a[3], m1, 0, 0, 0);
    FP_MFMA_ORDER();
  }
}

// ReLU(1x1 + sv) for channels 8j + 4h .. + 3 of this lane's pixel.
__device__ __forceinline__ f32x4 blaze_relu_piece(const f32x16& m0, const f32x16& m1, int j, const f32x4 sv) {
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (m0[4 * j + e] + m1[4 * j + e]) + sv[e];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
  return v;
}

// Prologue, all 256 threads: depthwise taps + bias of NBLK blocks -> Ws [NBLK][10][C].
template <int NBLK, int C>
__device__ __forceinline__ void blaze_stage_taps(float* Ws, const float* wd, const float* bd, int tid) {
  constexpr int Q = 10 * C / 4;
  for (int i = tid; i < NBLK * Q; i += 256) {
    const int b = NBLK > 1 ? i / Q : 0, k = i - b * Q;
    *(f32x4*)&Ws[i * 4] = (k * 4 < 9 * C) ? *(const f32x4*)(wd + b * 9 * C + k * 4) : *(const f32x4*)(bd + b * C + (k * 4 - 9 * C));
  }
}

// ... n floats (a multiple of 4) global -> LDS: the packed 1x1 weights into the staging area.
__device__ __forceinline__ void blaze_stage_copy(float* dst, const float* src, int n, int tid) {
  for (int i = tid; i < n / 4; i += 256) *(f32x4*)&dst[i * 4] = *(const f32x4*)(src + i * 4);
}

// B fragments of one 32-column n tile from staged packed weights [C/4][NCOLS][4]: k-quad 2 kq + h, column col.
template <int KG, int NCOLS>
__device__ __forceinline__ void blaze_load_bfrag(f32x4 (&bf)[KG], const float* staged, int h, int col) {
#pragma unroll
  for (int kq = 0; kq < KG; ++kq) bf[kq] = *(const f32x4*)&staged[((kq * 2 + h) * NCOLS + col) * 4];
}

// Band of a wave in a ring kernel: workgroup slot -> (image, first output row).  Band b of an image starts at output row
// lo + min(b R, span): the last band of a row window is moved up to end with the window.  Slots past the last band repeat it
// and store nothing (live = false).
struct BlazeBand {
  bool live;
  unsigned img;
  int y0;                 // wave-uniform: the row tests of the step are scalar branches
};
template <class Args>
__device__ __forceinline__ BlazeBand blaze_band(const Args& p, int slot) {
  BlazeBand b;
  const int bi = min(slot, p.nbands - 1);
  b.live = slot < p.nbands;
  b.img = __builtin_amdgcn_readfirstlane(fp_fastdiv((unsigned)bi, p.bands_div));
  b.y0 = __builtin_amdgcn_readfirstlane(p.lo + min((bi - (int)b.img * p.bands) * p.R, p.span));
  return b;
}

// Block 1 of a ring kernel, one step: y1 row y of this wave's strip -> ring row ry.  x = the input rows y - 1, y, y + 1 in
// slots r, r + 1, r + 2 (mod 3) of the register ring (r static: the caller unrolls by three).
//   inside: depthwise -> A tile; shortcut (+ 1x1 bias) -> the ring slot the row will occupy; if `fetch`, row y + 2 replaces
//           row y - 1 in the register ring (requested before the MFMAs); MFMAs; y1 = ReLU(1x1 + shortcut) in place in the ring;
//   else:   the row is block 2's zero padding above / below the image.
// The caller's barrier comes after it.
template <int C, int LDT, int KG>
__device__ __forceinline__ void blaze_ring_step(f32x4 (&x)[3][6], int r, int y, bool inside, bool fetch, const BlazeLanes<C>& ln,
                                                const float* wl1, const f32x4 pbias1, const f32x4 (&bf1)[KG], float* At, float* ry,
                                                const char* inb, long in_rb) {
  const int s0 = r, s1 = (r + 1) % 3, s2 = (r + 2) % 3;
  if (inside) {
    {
      f32x4 acc[4];
      blaze_dw3x3<1, C, 1>(acc, x[s0], x[s1], x[s2], wl1);
      if (ln.dw_lane) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          *(f32x4*)&At[(4 * ln.g + q) * LDT + 4 * ln.c4] = acc[q];
          *(f32x4*)&ry[ln.rg_dw + (q + 1) * C] = x[s1][q + 1] + pbias1;
        }
      }
    }
    if (fetch) blaze_load_row<C>(x[s0], inb + fp_uniform((long)(y + 2) * in_rb), ln.voff_in);
    f32x16 m0, m1;
    blaze_pw_swapped<KG>(&At[ln.lr * LDT + 4 * ln.h], bf1, m0, m1);
    float* rpx = ry + ln.rg_ep;
#pragma unroll
    for (int j = 0; j < C / 8; ++j) *(f32x4*)(rpx + 8 * j) = blaze_relu_piece(m0, m1, j, *(const f32x4*)(rpx + 8 * j));
  } else {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 32 * C / 256; ++j) *(f32x4*)&ry[(ln.x0 + 1) * C + (ln.lane + 64 * j) * 4] = z;
  }
}

}  // namespace
