// lrn.hip — FP_OP_POOL_LRN (include/facepath.h "POOL_LRN"): a max pool followed by Caffe's cross-channel LRN within
// channel groups, in one kernel: Levi-Hassner's pool1 + norm1 and pool2 + norm2 (the age and the gender net side by side
// in one tensor, one group each).
//   * a workgroup owns `ppb` consecutive output pixels (flattened over the images) and all their channels: it pools them
//     into LDS (16-byte loads, -inf outside the map), then each lane normalises four channels from its pixel's row in LDS;
//   * the LRN sum runs over j = c - n/2 .. c + n/2 inside c's group, in that order, fp32; the power is the device math
//     library's powf.
#include <string.h>

#include "common.h"

namespace {

struct PoolLrnArgs {
  const float* in;
  float* out;
  long in_ns, out_ns, M;
  int H, W, OH, OW, C, C4, KH, KW, stride, pad_t, pad_l, in_ld, out_ld;
  int G, half, ppb;   // LRN group size (0: none), n / 2, output pixels per workgroup
  const float* prm;   // [alpha, beta, k] (weight blob)
  float inv_n;        // 1 / n: Caffe's alpha / n
  fp_divisor div_ohw, div_ow;
};

__global__ __launch_bounds__(256) void pool_lrn_kernel(PoolLrnArgs p) {
  extern __shared__ __attribute__((aligned(16))) float pooled[];   // [ppb][C]
  const long m0 = (long)blockIdx.x * p.ppb;
  const int items = p.ppb * p.C4;
  const float ninf = -__builtin_huge_valf();
  for (int i = threadIdx.x; i < items; i += 256) {
    const int pp = i / p.C4, c4 = i - pp * p.C4;
    const long m = m0 + pp;
    if (m >= p.M) continue;
    const unsigned n = fp_fastdiv((unsigned)m, p.div_ohw);
    const unsigned pix = (unsigned)m - n * (unsigned)(p.OH * p.OW);
    const unsigned oy = p.OW == 1 ? pix : fp_fastdiv(pix, p.div_ow);
    const unsigned ox = pix - oy * (unsigned)p.OW;
    const int iy0 = (int)oy * p.stride - p.pad_t, ix0 = (int)ox * p.stride - p.pad_l;
    const float* base = p.in + (long)n * p.in_ns + 4 * c4;
    f32x4 acc = {ninf, ninf, ninf, ninf};
    for (int ky = 0; ky < p.KH; ++ky) {
      const int iy = iy0 + ky;
      if ((unsigned)iy >= (unsigned)p.H) continue;
      for (int kx = 0; kx < p.KW; ++kx) {
        const int ix = ix0 + kx;
        if ((unsigned)ix >= (unsigned)p.W) continue;
        const f32x4 v = *(const f32x4*)(base + ((long)iy * p.W + ix) * p.in_ld);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], v[e]);
      }
    }
    if (p.G == 0) *(f32x4*)(p.out + (long)n * p.out_ns + (long)pix * p.out_ld + 4 * c4) = acc;
    else *(f32x4*)(pooled + pp * p.C + 4 * c4) = acc;
  }
  if (p.G == 0) return;
  __syncthreads();
  for (int i = threadIdx.x; i < items; i += 256) {
    const int pp = i / p.C4, c4 = i - pp * p.C4;
    const long m = m0 + pp;
    if (m >= p.M) continue;
    const unsigned n = fp_fastdiv((unsigned)m, p.div_ohw);
    const unsigned pix = (unsigned)m - n * (unsigned)(p.OH * p.OW);
    const float* row = pooled + pp * p.C;
    const float alpha_n = p.prm[0] * p.inv_n, beta = p.prm[1], k = p.prm[2];
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * c4 + e;
      const int g0 = c / p.G * p.G, g1 = g0 + p.G;
      const int lo = c - p.half < g0 ? g0 : c - p.half, hi = c + p.half >= g1 ? g1 - 1 : c + p.half;
      float s = 0.f;
      for (int j = lo; j <= hi; ++j) s = __builtin_fmaf(row[j], row[j], s);
      y[e] = row[c] * powf(__builtin_fmaf(alpha_n, s, k), -beta);
    }
    *(f32x4*)(p.out + (long)n * p.out_ns + (long)pix * p.out_ld + 4 * c4) = y;
  }
}

}  // namespace

static bool pool_lrn_eligible(const fp_op& op) {
  if (op.kind != FP_OP_POOL_LRN || op.flags || op.act != FP_ACT_NONE || op.res_mode != FP_RES_NONE || op.out_cmul != 1) return false;
  if (op.Cout != op.Cin || op.Cin % 4 || op.Cin > 4096 || op.KH < 1 || op.KH > 7 || op.KW < 1 || op.KW > 7 || op.stride < 1) return false;
  if (op.pad_t < 0 || op.pad_t >= op.KH || op.pad_l < 0 || op.pad_l >= op.KW) return false;
  if (op.in_ld % 4 || op.out_ld % 4 || op.in_off % 4 || op.out_off % 4 || op.in_ns % 4 || op.out_ns % 4) return false;
  if (op.in_ld < op.Cin || op.out_ld < op.Cin) return false;
  // every window holds at least one pixel of the map (a pool of -inf only is no output Caffe defines)
  if ((long)(op.OH - 1) * op.stride - op.pad_t >= op.H || (long)(op.OW - 1) * op.stride - op.pad_l >= op.W) return false;
  if ((long)op.N * op.OH * op.OW >= (1L << 31) || op.OH * op.OW < 2) return false;   // 32-bit pixel decode (divisor >= 2)
  if (op.Cmid) {
    if (op.Cmid < 0 || op.Cmid % 4 || op.Cin % op.Cmid || op.res_C < 1 || op.res_C > 15 || !(op.res_C & 1) || op.w_off < 0) return false;
  } else if (op.res_C || op.w_off >= 0) {
    return false;
  }
  return true;
}

int fp_launch_pool_lrn(const fp_op& op, const fp_launch& L) {
  if (!pool_lrn_eligible(op)) return FP_ERR_UNSUPPORTED;
  if (fp_dry_run(L, op.Cmid ? "pool_lrn_kernel" : "pool_lrn_kernel<nolrn>")) return FP_OK;
  PoolLrnArgs a;
  memset(&a, 0, sizeof(a));
  a.in = L.arena + op.in_off;
  a.out = L.arena + op.out_off;
  a.in_ns = op.in_ns; a.out_ns = op.out_ns;
  a.M = (long)op.N * op.OH * op.OW;
  a.H = op.H; a.W = op.W; a.OH = op.OH; a.OW = op.OW; a.C = op.Cin; a.C4 = op.Cin / 4;
  a.KH = op.KH; a.KW = op.KW; a.stride = op.stride; a.pad_t = op.pad_t; a.pad_l = op.pad_l;
  a.in_ld = op.in_ld; a.out_ld = op.out_ld;
  a.G = op.Cmid;
  a.half = op.res_C / 2;
  a.ppb = op.Cin >= 4096 ? 1 : 4096 / op.Cin;
  a.prm = op.Cmid ? L.weights + op.w_off : nullptr;
  a.inv_n = op.Cmid ? 1.0f / (float)op.res_C : 0.f;
  a.div_ohw = fp_make_divisor((unsigned)(op.OH * op.OW));
  a.div_ow = fp_make_divisor((unsigned)(op.OW >= 2 ? op.OW : 2));
  const long blocks = (a.M + a.ppb - 1) / a.ppb;
  if (blocks >= (1L << 31)) return FP_ERR_UNSUPPORTED;
  const size_t lds = op.Cmid ? (size_t)a.ppb * op.Cin * sizeof(float) : 0;
  hipLaunchKernelGGL(pool_lrn_kernel, dim3((unsigned)blocks), dim3(256), lds, L.s, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}
