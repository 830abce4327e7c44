// embedhead.hip — FP_OP_EMBED_HEAD (include/facepath.h "EMBED_HEAD"): the embedding head of Inception-ResNet-v1
// (avgpool_1a -> last_linear -> last_bn -> F.normalize) in one kernel, fp32 arithmetic.
//   * a workgroup = 4 waves owns 4 images: their channel means (pixels summed in order, divided by H * W) go to LDS;
//   * the Linear: wave w computes outputs w, w + 4, ... for all four images at once -- lane l sums k = 4 l + 256 i (16-byte
//     weight loads, each used for four images), a butterfly over the wave adds the lanes -- then the BatchNorm1d affine;
//   * the L2 normalisation: one wave per image.
// Every image runs the same instruction sequence whichever images share its workgroup: a row does not depend on the batch.
#include "common.h"

namespace {

constexpr int IMG = 4;   // images per workgroup = waves per workgroup

struct HeadArgs {
  const float* in;
  float* out;
  const float* w;      // [D][Cin]
  const float* scale;  // [D] or null
  const float* bias;   // [D] or null
  long in_ns, out_ns;
  int N, HW, Cin, D, in_ld, l2;
};

__global__ __launch_bounds__(256) void embed_head_kernel(HeadArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* mean = sm;                     // [IMG][Cin]
  float* y = sm + IMG * p.Cin;          // [IMG][D]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * IMG;
  const int nimg = p.N - n0 < IMG ? p.N - n0 : IMG;
  const float hw = (float)p.HW;
  for (int i = tid; i < IMG * p.Cin; i += 256) {
    const int j = i / p.Cin, c = i - j * p.Cin;
    float s = 0.f;
    if (j < nimg) {
      const float* x = p.in + (long)(n0 + j) * p.in_ns + c;
      for (int px = 0; px < p.HW; ++px) s += x[(long)px * p.in_ld];
    }
    mean[i] = s / hw;
  }
  __syncthreads();
  for (int d = wave; d < p.D; d += IMG) {
    const float* wr = p.w + (long)d * p.Cin;
    float acc[IMG];
#pragma unroll
    for (int j = 0; j < IMG; ++j) acc[j] = 0.f;
    for (int k = 4 * lane; k < p.Cin; k += 256) {
      const f32x4 wv = *(const f32x4*)(wr + k);
#pragma unroll
      for (int j = 0; j < IMG; ++j) {
        const f32x4 mv = *(const f32x4*)(mean + j * p.Cin + k);
        acc[j] = __builtin_fmaf(wv[0], mv[0], acc[j]);
        acc[j] = __builtin_fmaf(wv[1], mv[1], acc[j]);
        acc[j] = __builtin_fmaf(wv[2], mv[2], acc[j]);
        acc[j] = __builtin_fmaf(wv[3], mv[3], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < IMG; ++j) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off);
    }
    if (lane == 0) {
      const float sc = p.scale ? p.scale[d] : 1.f, bi = p.bias ? p.bias[d] : 0.f;
#pragma unroll
      for (int j = 0; j < IMG; ++j) y[j * p.D + d] = __builtin_fmaf(acc[j], sc, bi);
    }
  }
  __syncthreads();
  if (wave < nimg) {
    const float* yr = y + wave * p.D;
    float nrm = 1.f;
    if (p.l2) {
      float s = 0.f;
      for (int i = lane; i < p.D; i += 64) s = __builtin_fmaf(yr[i], yr[i], s);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      nrm = __builtin_fmaxf(sqrtf(s), 1e-12f);
    }
    float* o = p.out + (long)(n0 + wave) * p.out_ns;
    for (int i = lane; i < p.D; i += 64) o[i] = p.l2 ? yr[i] / nrm : yr[i];
  }
}

}  // namespace

bool fp_embed_head_eligible(const fp_op& op) {
  if (op.kind != FP_OP_EMBED_HEAD || (op.flags & ~FP_OPF_OUT_L2)) return false;
  if (op.OH != 1 || op.OW != 1 || op.KH != 1 || op.KW != 1 || op.stride != 1 || op.pad_t || op.pad_l) return false;
  if (op.act != FP_ACT_NONE || op.res_mode != FP_RES_NONE || op.out_cmul != 1) return false;
  if (op.Cin % 4 || op.Cin > 2048 || op.Cout > 1024 || op.w_off % 4 || op.out_ld < op.Cout || op.out_ns < op.Cout) return false;
  return (long)op.H * op.W < (1L << 24);
}

int fp_launch_embed_head(const fp_op& op, const fp_launch& L) {
  if (!fp_embed_head_eligible(op)) return FP_ERR_UNSUPPORTED;
  if (fp_dry_run(L, "embed_head_kernel")) return FP_OK;
  HeadArgs a;
  a.in = L.arena + op.in_off;
  a.out = L.arena + op.out_off;
  a.w = L.weights + op.w_off;
  a.scale = op.scale_off >= 0 ? L.weights + op.scale_off : nullptr;
  a.bias = op.bias_off >= 0 ? L.weights + op.bias_off : nullptr;
  a.in_ns = op.in_ns;
  a.out_ns = op.out_ns;
  a.N = op.N;
  a.HW = op.H * op.W;
  a.Cin = op.Cin;
  a.D = op.Cout;
  a.in_ld = op.in_ld;
  a.l2 = (op.flags & FP_OPF_OUT_L2) != 0;
  const size_t lds = (size_t)IMG * (op.Cin + op.Cout) * sizeof(float);
  hipLaunchKernelGGL(embed_head_kernel, dim3((unsigned)fp_ceil_div(op.N, IMG)), dim3(256), lds, L.s, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}
