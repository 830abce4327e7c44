// blazepair.hip -- a stride-1 24 -> 24 BlazeBlock and the BlazeBlock behind it in one kernel, row-padded activations (gfx950).
//
//   y1 = ReLU( pw1( dw1(x)  ) + x  )                                           (fde/modules/blazeface/blazeface.py:12-47)
//   y2 = ReLU( pw2( dw2(y1) ) + y1 )                                           stride 1: blazepair_kernel<W>
//   y2 = ReLU( pw2( dw2_s2( pad(y1, (0, 2, 0, 2)) ) ) + cpad( maxpool2x2(y1) ) )        stride 2: blazepair_s2_kernel<W, C2>, C2 = 24 or 48
//
// A 24-channel stage of BlazeFace-back is seven stride-1 blocks and the stride-2 block that halves the map (blazeface.py:122-152)
// = three stride-1 pairs + one stride-2 pair.  One BlazeBlock at a time (blazewp.hip) moves x in and y out per block: the 14
// narrow blocks of the back model are 55 % of its bytes and run at the rate this part copies memory.  Here y1 never leaves the CU.
//
// The ring step both kernels share (blazerow.h blaze_ring_step):
//   * a WORKGROUP owns a band of output rows of one image (128-wide maps: its four waves are the four 32-pixel strips of a y1
//     row; 64-wide maps: two bands, two strips each) and marches down it one y1 row per step;
//   * step for y1 row y:  block 1 makes the row exactly as blazeblock_wp_kernel does (3-row window of x as a ring in registers,
//     depthwise -> wave-private A tile -> 12 MFMAs -> + shortcut -> ReLU) but writes it into an LDS ring of four y1 rows
//     (row-padded like the tensors in memory: a zero pixel left and right, zero rows above / below the image) -- ONE workgroup
//     barrier -- then block 2 reads the ring (its depthwise reads the neighbour strips' columns, which is why the ring is shared);
//   * the shortcut + bias of block 1 are parked in the ring slot the row will occupy, and the epilogue updates them in place, so
//     there is no shortcut tile; y2 goes from block 2's epilogue registers straight to global memory (32-byte pieces: a lane
//     pair = 8 channels of one pixel; L2 merges the pieces of a line);
//   * with a row window (facepath.h "Row windows") the bands cover only the window's rows; y1 rows outside the window but inside
//     the image are computed from x like any other (the caller keeps x right there), only the rows outside the image are zero.
// Stride 1: after every step from the third on, block 2 makes output row y - 1 from ring rows y - 2 .. y, shortcut = ring row
//   y - 1.  A band of R rows needs y1 rows y0 - 1 .. y0 + R: R + 2 block-1 rows (R = 64: 3 % recomputed); 66 KiB of LDS, two
//   workgroups per CU.  Bytes per pair: x once (+ the band halos) and y2 once -- half of what two launches move; the instruction
//   count per pixel is the same as two blazeblock_wp launches (fp32 MFMAs and VALU share the SIMD's ALU: tools/lab/coexec_lab.hip).
// Stride 2: a band of R2 rows of y2 = 2 R2 + 1 rows of y1 (the last one is the stride-2 window's third row: the next band's
//   first, or the zero row below the image).  Every second step, after the barrier, HALF the waves (an output row has half the
//   pixels) make output row yo from ring rows 2 yo .. 2 yo + 2: depthwise stride 2 (window of 9 columns x 3 rows per four output
//   pixels, the two pad columns / the pad row are the ring's zero borders), 12 (C2 = 48: 24) fp32 MFMAs, shortcut = max over the
//   2 x 2 ring pixels for channels < 24 and 0 above, bias, ReLU; the other waves run ahead into the next step's block 1.  As two
//   launches y1 is written (403 MB at 128 x 128, batch 256) and read back: x in + y2 out = 503 MB instead of 1.3 GB.
// Arithmetic per block identical to blazeblock_wp_kernel / blazeblock_persist_kernel<2, ...> (same tap order, same k order).
#include "blazerow.h"

namespace {

struct BlazePairArgs {
  const float* in;    // pixel (0, 0) of image 0, row-padded
  float* out;
  const float* wd;    // [2][9][C]
  const float* bd;    // [2][C]
  const float* wp;    // block 1: packed [C/4][32][4]; block 2 behind it: packed [C/4][Npad2][4], Npad2 = 32 (C2 = 24) / 64 (C2 = 48)
  const float* bp;    // [C] then [C2]
  int H, R, bands;    // R = output rows of y2 per band, bands per image
  int lo, span;       // band b starts at output row lo + min(b R, span): the row window (facepath.h) is rows lo .. lo + span + R - 1
  int nbands;         // N * bands
  int in_rp, out_rp;  // row pitch, floats
  long in_ns, out_ns;
  fp_divisor bands_div;
};

// LDS of a pair kernel, in floats: depthwise taps + bias [2][10][C], 1x1 bias [32] + [BIAS2], the rings [NSUB][4][RROW], four
// wave regions [32][LDT] (A tile; first: weight staging) and TAIL floats behind them that only the weight staging uses.
template <int W, int BIAS2, int TAIL>
struct PairLds {
  static constexpr int C = 24, LDT = C + 4, KG = C / 8, NS = W / 32, NSUB = 4 / NS;
  static constexpr int RROW = (W + 2) * C;                 // floats per ring row: pixels -1 .. W
  static constexpr int RING = 4 * RROW;
  static constexpr int PWF = KG * 2 * 32 * 4;              // packed 1x1 weights of one 32-column n tile
  static constexpr int BP = 2 * 10 * C, RG = BP + 32 + BIAS2, AV = RG + NSUB * RING, FLOATS = AV + 4 * 32 * LDT + TAIL;
};

// Prologue of both kernels (behind the kernel's own 1x1 biases -> Bp): depthwise taps + bias and the zeroed rings into LDS, the
// 1x1 weights through the wave regions into every lane's B fragments (block 2: NB2 n tiles of 32 columns).
template <class G, int NB2>
__device__ __forceinline__ void pair_prologue(float* smem, const BlazePairArgs& p, int tid, const BlazeLanes<24>& ln,
                                              f32x4 (&bf1)[G::KG], f32x4 (&bf2)[NB2][G::KG]) {
  static_assert((1 + NB2) * G::PWF <= G::FLOATS - G::AV, "weight staging fits the wave regions");
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  blaze_stage_taps<2, G::C>(smem, p.wd, p.bd, tid);
  blaze_stage_copy(smem + G::AV, p.wp, (1 + NB2) * G::PWF, tid);
  for (int i = tid; i < G::NSUB * G::RING / 4; i += 256) *(f32x4*)&smem[G::RG + i * 4] = z;     // pads (and everything else) zero
  __syncthreads();
  blaze_load_bfrag<G::KG, 32>(bf1, smem + G::AV, ln.h, ln.lr);
#pragma unroll
  for (int nb = 0; nb < NB2; ++nb) blaze_load_bfrag<G::KG, 32 * NB2>(bf2[nb], smem + G::AV + G::PWF, ln.h, 32 * nb + ln.lr);
  __syncthreads();                                         // staging area becomes the wave regions
}

template <int W>
__global__ __launch_bounds__(256, 2) void blazepair_kernel(BlazePairArgs p) {
  using G = PairLds<W, 32, 0>;
  constexpr int C = G::C, LDT = G::LDT, KG = G::KG, NS = G::NS, NSUB = G::NSUB, RROW = G::RROW;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Bp = smem + G::BP;                                // [2][32]
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = wv / NS, strip = wv - sub * NS, x0 = strip * 32;
  const BlazeLanes<C> ln(tid, x0);
  const int lr = ln.lr, h = ln.h;

  f32x4 bf1[KG], bf2[1][KG];                               // B fragments of both blocks: k-quad 2*kq + h, column lr
  if (tid < 64) Bp[tid] = (tid & 31) < C ? p.bp[(tid >> 5) * C + (tid & 31)] : 0.f;
  pair_prologue<G, 1>(smem, p, tid, ln, bf1, bf2);

  float* At = smem + G::AV + wv * (32 * LDT);              // A tile [32][LDT]
  float* ring = smem + G::RG + sub * G::RING;
  const float* wl1 = &smem[4 * ln.c4];
  const float* wl2 = &smem[10 * C + 4 * ln.c4];
  const f32x4 pbias1 = *(const f32x4*)&Bp[4 * ln.c4];      // block 1's 1x1 bias rides its shortcut

  // this wave's band: (image, band) -> first output row y0; the two halves of a 64-wide workgroup take bands 2b, 2b + 1
  const BlazeBand band = blaze_band(p, (int)blockIdx.x * NSUB + sub);
  const int y0 = band.y0;
  const long in_rb = (long)p.in_rp * 4, out_rb = (long)p.out_rp * 4;
  const char* inb = (const char*)p.in + fp_uniform(((long)band.img * p.in_ns + (long)(x0 - 1) * C) * 4);    // (row 0, column x0 - 1)
  char* outb = (char*)p.out + fp_uniform(((long)band.img * p.out_ns + (long)x0 * C) * 4);                   // (row 0, column x0)

  // x window: ring of three rows in registers; at step i (row y = y0 - 1 + i) rows y-1, y, y+1 sit in slots i%3, (i+1)%3, (i+2)%3
  f32x4 x[3][6];
  const int nsteps = p.R + 2;
  {
    const int ifirst = y0 == 0 ? 1 : 0;                    // the top band's first step only zero-fills ring row -1
    const int yf = y0 - 1 + ifirst;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const char* rowp = inb + fp_uniform((long)(yf - 1 + ky) * in_rb);
      if (ifirst == 0) {
        blaze_load_row<C>(x[ky], rowp, ln.voff_in);
      } else {
        blaze_load_row<C>(x[(ky + 1) % 3], rowp, ln.voff_in);
      }
    }
  }

  for (int ib = 0; ib < nsteps; ib += 3) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int i = ib + r;
      if (i < nsteps) {
        const int y = y0 - 1 + i;
        // ---- block 1: y1 row y -> its ring row (rows -1 and H: block 2's zero padding) ----
        blaze_ring_step<C, LDT, KG>(x, r, y, (unsigned)y < (unsigned)p.H, y + 1 < p.H && i + 1 < nsteps, ln, wl1, pbias1, bf1, At,
                                    ring + ((y + 1) & 3) * RROW, inb, in_rb);
        __syncthreads();
        if (i >= 2) {
          // ---- block 2: output row yo = y - 1 from ring rows yo-1, yo, yo+1 ----
          // (the text of blazerow.h's blaze_dw3x3<1>, blaze_pw_swapped and blaze_relu_piece written out: through the helpers hipcc
          // schedules this kernel's block 2 differently and the launch takes 1 % longer, 500 -> 504 us over the three 128 x 128 pairs
          // at batch 256; blazepair_s2_kernel's block 2 measures the same either way and uses them)
          const int yo = y - 1;
          {
            const f32x4 dbias = *(const f32x4*)(wl2 + 9 * C);
            f32x4 acc[4] = {dbias, dbias, dbias, dbias};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
              const float* rr = ring + ((yo + ky) & 3) * RROW + ln.rg_dw;      // ring row of y1 row yo - 1 + ky
              f32x4 xv[6];
#pragma unroll
              for (int j = 0; j < 6; ++j) xv[j] = *(const f32x4*)(rr + j * C);
              const f32x4 w0 = *(const f32x4*)(wl2 + (ky * 3 + 0) * C);
              const f32x4 w1 = *(const f32x4*)(wl2 + (ky * 3 + 1) * C);
              const f32x4 w2 = *(const f32x4*)(wl2 + (ky * 3 + 2) * C);
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                acc[q] += xv[q] * w0;
                acc[q] += xv[q + 1] * w1;
                acc[q] += xv[q + 2] * w2;
              }
            }
            blaze_store_a<C, LDT>(At, ln, acc);
          }
          f32x16 m0, m1;
#pragma unroll
          for (int k = 0; k < 16; ++k) m0[k] = 0.f, m1[k] = 0.f;
          const float* arow = &At[lr * LDT + 4 * h];
#pragma unroll
          for (int kq = 0; kq < KG; ++kq) {
            const f32x4 a = *(const f32x4*)(arow + kq * 8);
            m0 = __builtin_amdgcn_mfma_f32_32x32x2f32(bf2[0][kq][0], a[0], m0, 0, 0, 0);
            FP_MFMA_ORDER();
            m1 = __builtin_amdgcn_mfma_f32_32x32x2f32(bf2[0][kq][1], a[1], m1, 0, 0, 0);
            FP_MFMA_ORDER();
            m0 = __builtin_amdgcn_mfma_f32_32x32x2f32(bf2[0][kq][2], a[2], m0, 0, 0, 0);
            FP_MFMA_ORDER();
            m1 = __builtin_amdgcn_mfma_f32_32x32x2f32(bf2[0][kq][3], a[3], m1, 0, 0, 0);
            FP_MFMA_ORDER();
          }
          // y2 = ReLU(1x1 + bias + y1 row yo): lane (lr, h) has pixel x0 + lr, channels 8j + 4h .. + 3 -- with its partner lane
          // (h ^ 1) a 32-byte piece
          const float* spx = ring + ((yo + 1) & 3) * RROW + ln.rg_ep;
          char* orow_g = outb + fp_uniform((long)yo * out_rb);
#pragma unroll
          for (int j = 0; j < C / 8; ++j) {
            const f32x4 sv = *(const f32x4*)(spx + 8 * j) + *(const f32x4*)&Bp[32 + 8 * j + 4 * h];
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (m0[4 * j + e] + m1[4 * j + e]) + sv[e];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
            if (band.live) *(f32x4*)(orow_g + (unsigned)((lr * C + 4 * h + 8 * j) * 4)) = v;
          }
        }
      }
    }
  }
}

template <int W, int C2>
__global__ __launch_bounds__(256, 2) void blazepair_s2_kernel(BlazePairArgs p) {
  // (the region behind the A tiles is weight staging only: y2 goes from the epilogue registers to global memory)
  using G = PairLds<W, 64, (C2 > 24 ? (W / 64) * (4 / (W / 32)) * 32 * C2 : 0)>;
  constexpr int C = G::C, LDT = G::LDT, KG = G::KG, NS = G::NS, NSUB = G::NSUB, NS2 = NS / 2, RROW = G::RROW;
  constexpr int NB2 = C2 > 32 ? 2 : 1;                     // 32-column halves of block 2's 1x1
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Bp = smem + G::BP;                                // [32] block 1, [64] block 2
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = wv / NS, strip = wv - sub * NS, x0 = strip * 32;
  const BlazeLanes<C> ln(tid, x0);
  const int lr = ln.lr, h = ln.h;

  f32x4 bf1[KG], bf2[NB2][KG];                             // B fragments: k-quad 2*kq + h, column lr (+ 32 nb)
  if (tid < 96) Bp[tid] = tid < 32 ? (tid < C ? p.bp[tid] : 0.f) : (tid - 32 < C2 ? p.bp[C + tid - 32] : 0.f);
  pair_prologue<G, NB2>(smem, p, tid, ln, bf1, bf2);

  float* At = smem + G::AV + wv * (32 * LDT);              // A tile [32][LDT]
  float* ring = smem + G::RG + sub * G::RING;
  const bool b2wave = strip < NS2;                         // this wave makes output pixels 32 strip .. + 31 of a y2 row
  const float* wl1 = &smem[4 * ln.c4];
  const float* wl2 = &smem[10 * C + 4 * ln.c4];
  const f32x4 pbias1 = *(const f32x4*)&Bp[4 * ln.c4];      // block 1's 1x1 bias rides its shortcut
  const int rg_dw2 = (64 * strip + 8 * ln.g + 1) * C + 4 * ln.c4;   // block 2: ring pixel 2 (32 strip + 4g) of this lane's channels
  const int rg_ep2 = (64 * strip + 2 * lr + 1) * C + 4 * h;         // block 2's shortcut: ring pixel 2 (32 strip + lr)

  // this wave's band: (image, band) -> first output row yo0 of y2; y1 rows 2 yo0 .. 2 yo0 + 2 R
  const BlazeBand band = blaze_band(p, (int)blockIdx.x * NSUB + sub);
  const int yo0 = band.y0;
  const int ya = 2 * yo0;                                  // first y1 row of the band
  const long in_rb = (long)p.in_rp * 4, out_rb = (long)p.out_rp * 4;
  const char* inb = (const char*)p.in + fp_uniform(((long)band.img * p.in_ns + (long)(x0 - 1) * C) * 4);           // (row 0, column x0 - 1)
  char* outb = (char*)p.out + fp_uniform(((long)band.img * p.out_ns + (long)(32 * (b2wave ? strip : 0)) * C2) * 4);   // (row 0, column 32 strip)

  // x window: ring of three rows in registers; at step i (row y = ya + i) rows y-1, y, y+1 sit in slots i%3, (i+1)%3, (i+2)%3
  f32x4 x[3][6];
  const int nsteps = 2 * p.R + 1;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) blaze_load_row<C>(x[ky], inb + fp_uniform((long)(ya - 1 + ky) * in_rb), ln.voff_in);

  for (int ib = 0; ib < nsteps; ib += 3) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int i = ib + r;
      if (i < nsteps) {
        const int y = ya + i;
        // ---- block 1: y1 row y -> its ring row (row H: the zero row of block 2's F.pad(.., (0, 2, 0, 2))) ----
        blaze_ring_step<C, LDT, KG>(x, r, y, y < p.H, y + 1 < p.H && i + 1 < nsteps, ln, wl1, pbias1, bf1, At,
                                    ring + ((y + 1) & 3) * RROW, inb, in_rb);
        __syncthreads();
        if (i >= 2 && !(i & 1) && b2wave) {
          // ---- block 2 (stride 2): output row yo from ring rows 2 yo, 2 yo + 1, 2 yo + 2 = y - 2, y - 1, y ----
          const int yo = yo0 + (i - 2) / 2;
          {
            f32x4 acc[4];
            blaze_dw3x3<2, C, C / 4>(acc, (const f32x4*)(ring + ((y - 1) & 3) * RROW + rg_dw2),
                                     (const f32x4*)(ring + (y & 3) * RROW + rg_dw2),
                                     (const f32x4*)(ring + ((y + 1) & 3) * RROW + rg_dw2), wl2);         // ring rows of y1 rows y - 2 .. y
            blaze_store_a<C, LDT>(At, ln, acc);
          }
          const float* arow = &At[lr * LDT + 4 * h];
          const float* s00 = ring + ((y - 1) & 3) * RROW + rg_ep2;            // y1 row 2 yo, pixel 2 X
          const float* s10 = ring + (y & 3) * RROW + rg_ep2;                  // y1 row 2 yo + 1
          char* orow_g = outb + fp_uniform((long)yo * out_rb);
#pragma unroll
          for (int nb = 0; nb < NB2; ++nb) {
            f32x16 m0, m1;
            blaze_pw_swapped<KG>(arow, bf2[nb], m0, m1);
            // y2 = ReLU(1x1 + bias + shortcut): channels 32 nb + 8j + 4h .. + 3 of output pixel 32 strip + lr; the shortcut is
            // the 2 x 2 max of y1 for channels < 24 and 0 above (blazeface.py:38-45)
            const int nj = (C2 - 32 * nb < 32 ? C2 - 32 * nb : 32) / 8;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (j >= nj) break;
              const int oc = 32 * nb + 8 * j;               // (+ 4h: a lane's four channels are on one side of 24)
              f32x4 sv = *(const f32x4*)&Bp[32 + oc + 4 * h];
              if (oc < C) {
                const f32x4 a0 = *(const f32x4*)(s00 + 8 * j), a1 = *(const f32x4*)(s00 + C + 8 * j);
                const f32x4 b0 = *(const f32x4*)(s10 + 8 * j), b1 = *(const f32x4*)(s10 + C + 8 * j);
#pragma unroll
                for (int e = 0; e < 4; ++e) sv[e] += fmaxf(fmaxf(a0[e], a1[e]), fmaxf(b0[e], b1[e]));
              }
              const f32x4 v = blaze_relu_piece(m0, m1, j, sv);
              // a lane pair (h = 0, 1) writes 32 contiguous bytes of its pixel
              if (band.live) *(f32x4*)(orow_g + (unsigned)((lr * C2 + oc + 4 * h) * 4)) = v;
            }
          }
        }
      }
    }
  }
}

template <class K>
int launch_with_lds(K kernel, int grid, size_t lds, hipStream_t s, const BlazePairArgs& a) {
  const hipError_t ae = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (ae != hipSuccess) {
    fp_set_hip_error(ae);
    return FP_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, s, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

template <int W>
int launch_pair(const BlazePairArgs& a, const fp_launch& L) {
  if (fp_dry_run(L, "blazepair_kernel<%d>", W)) return FP_OK;
  using G = PairLds<W, 32, 0>;
  return launch_with_lds(blazepair_kernel<W>, fp_ceil_div(a.nbands, G::NSUB), 4 * (size_t)G::FLOATS, L.s, a);
}

template <int W, int C2>
int launch_pair_s2(const BlazePairArgs& a, const fp_launch& L) {
  if (fp_dry_run(L, "blazepair_s2_kernel<%d, %d>", W, C2)) return FP_OK;
  using G = PairLds<W, 64, (C2 > 24 ? (W / 64) * (4 / (W / 32)) * 32 * C2 : 0)>;
  return launch_with_lds(blazepair_s2_kernel<W, C2>, fp_ceil_div(a.nbands, G::NSUB), 4 * (size_t)G::FLOATS, L.s, a);
}

}  // namespace

// Output rows per band of an unwindowed launch: the largest divisor of `rows` among first, first + step, .. <= max that leaves
// at least 512 workgroups (two per CU), never below `first`; at least two bands per image (the kernels' band index math).
// Stride 1: 8 .. 64 (batch 256 at 128 x 128: 64-row bands = 512 workgroups, 3 % of block 1 recomputed: 255 us against 269 with
// 32-row bands); stride 2: 4 .. 32 rows of y2 (a band computes 2 R + 1 rows of y1 for its R rows of y2).
static int pair_band_rows(const fp_op& op, int first, int step, int max, int rows) {
  const int nsub = 4 / (op.W / 32);
  int best = 0;
  for (int r = first; r <= max && 2 * r <= rows; r += step) {
    if (rows % r) continue;
    if (best == 0 || (long)op.N * (rows / r) / nsub >= 512) best = r;
  }
  return best;
}
static int blazepair_band_rows(const fp_op& op) { return pair_band_rows(op, 8, 4, 64, op.H); }
static int blazepair_s2_band_rows(const fp_op& op) { return pair_band_rows(op, 4, 4, 32, op.OH); }

// Two stride-1 24 -> 24 blocks on a row-padded 128- or 64-pixel-wide map (include/facepath.h, BLAZEPAIR).
static bool blazepair_supported(const fp_op& op) {
  if (op.kind != FP_OP_BLAZEPAIR || !(op.flags & FP_OPF_IN_ROWPAD)) return false;
  if (op.stride != 1 || op.KH != 3 || op.KW != 3 || op.pad_t != 1 || op.pad_l != 1) return false;
  if (op.Cin != 24 || op.Cout != 24 || op.in_ld != 24 || op.out_ld != 24 || op.out_cmul != 1) return false;
  if (op.OH != op.H || op.OW != op.W || (op.W != 128 && op.W != 64) || op.H % 8 || op.H < 8) return false;
  if (op.in_off % 4 || op.out_off % 4 || op.in_ns % 4 || op.out_ns % 4) return false;
  if (op.w_off % 4 || op.scale_off % 4 || op.slope_off % 4 || op.bias_off % 4) return false;
  if (op.res_mode != FP_RES_ADD_BEFORE_ACT || op.act != FP_ACT_RELU) return false;
  const int r = blazepair_band_rows(op);
  return r > 0 && op.H / r >= 2;
}

// A stride-1 24 -> 24 block and the stride-2 24 -> 24 / 48 block behind it on a row-padded 128- or 64-pixel-wide map
// (include/facepath.h, BLAZEPAIR with stride = 2).
static bool blazepair_s2_supported(const fp_op& op) {
  if (op.kind != FP_OP_BLAZEPAIR || !(op.flags & FP_OPF_IN_ROWPAD) || (op.flags & ~(FP_OPF_IN_ROWPAD | FP_OPF_OUT_ROWPAD))) return false;
  if (op.stride != 2 || op.KH != 3 || op.KW != 3 || op.pad_t != 0 || op.pad_l != 0) return false;
  if (op.Cin != 24 || (op.Cout != 24 && op.Cout != 48) || op.in_ld != 24 || op.out_ld != op.Cout || op.out_cmul != 1) return false;
  if (op.H % 2 || op.W % 2 || op.OH != op.H / 2 || op.OW != op.W / 2 || (op.W != 128 && op.W != 64) || op.H < 16) return false;
  if (op.in_off % 4 || op.out_off % 4 || op.in_ns % 4 || op.out_ns % 4) return false;
  if (op.w_off % 4 || op.scale_off % 4 || op.slope_off % 4 || op.bias_off % 4) return false;
  if (op.res_mode != FP_RES_POOL2_BEFORE_ACT || op.act != FP_ACT_RELU) return false;
  return blazepair_s2_band_rows(op) > 0;
}

// The kernels' arguments for a supported op.  full_R = rows per band of an unwindowed launch (>= 2 bands per image).  A row
// window: bands over its rows only, as many as fill whole rounds of the 512 workgroup slots (two per CU); a band of R output
// rows takes step_mul * R + halo steps (stride 1: R + 2, stride 2: 2 R + 1) and has at least min_rows rows.
static BlazePairArgs pair_args(const fp_op& op, const fp_launch& L, int full_R, int step_mul, int halo, int min_rows) {
  BlazePairArgs a;
  a.in = L.arena + op.in_off;
  a.out = L.arena + op.out_off;
  a.wd = L.weights + op.w_off;
  a.bd = L.weights + op.scale_off;
  a.wp = L.weights + op.slope_off;
  a.bp = L.weights + op.bias_off;
  a.H = op.H;
  if (op.row_end > 0) {
    const int rows = op.row_end - op.row_lo, nsub = 4 / (op.W / 32);
    a.bands = fp_window_bands(rows, op.N, nsub, 512, step_mul, halo, 2, min_rows);
    a.R = fp_ceil_div(rows, a.bands);
    a.lo = op.row_lo;
    a.span = rows - a.R;
  } else {
    a.R = full_R;
    a.bands = op.OH / a.R;
    a.lo = 0;
    a.span = op.OH - a.R;
  }
  a.nbands = op.N * a.bands;
  a.in_rp = (op.W + 1) * 24;
  a.out_rp = (op.OW + ((op.flags & FP_OPF_OUT_ROWPAD) ? 1 : 0)) * op.Cout;
  a.in_ns = op.in_ns;
  a.out_ns = op.out_ns;
  a.bands_div = fp_make_divisor((unsigned)a.bands);
  return a;
}

int fp_launch_blazepair(const fp_op& op, const fp_launch& L) {
  if (!blazepair_supported(op)) return FP_ERR_UNSUPPORTED;
  const BlazePairArgs a = pair_args(op, L, blazepair_band_rows(op), 1, 2, 8);
  return op.W == 128 ? launch_pair<128>(a, L) : launch_pair<64>(a, L);
}

int fp_launch_blazepair_s2(const fp_op& op, const fp_launch& L) {
  if (!blazepair_s2_supported(op)) return FP_ERR_UNSUPPORTED;
  const BlazePairArgs a = pair_args(op, L, blazepair_s2_band_rows(op), 2, 1, 4);
  if (op.Cout == 24) return op.W == 128 ? launch_pair_s2<128, 24>(a, L) : launch_pair_s2<64, 24>(a, L);
  return op.W == 128 ? launch_pair_s2<128, 48>(a, L) : launch_pair_s2<64, 48>(a, L);
}
