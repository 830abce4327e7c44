// clshead.hip — FP_OP_CLS_HEAD (include/facepath.h "CLS_HEAD"): Levi-Hassner's fc8 + prob, a Linear layer of at most 64
// outputs followed by softmax, one wave per image, fp32:
//   * output c: lane l sums k = 4 l + 256 i of the row (16-byte loads of the weight row and of the input row), a butterfly
//     adds the lanes; lane c keeps z_c = sum + bias_c;
//   * softmax over lanes 0 .. Cout - 1: the max and the sum of exp(z - max) by butterflies, p_c = e_c / sum (expf of the
//     device math library).
// Each image runs the same instruction sequence whatever the batch: a row does not depend on the batch.
#include <string.h>

#include "common.h"

namespace {

struct ClsArgs {
  const float* in;
  float* out;
  float* logits;       // or null
  const float* w;      // [D][Cin]
  const float* bias;   // [D] or null
  long in_ns, out_ns, logit_ns;
  int N, Cin, D;
};

__global__ __launch_bounds__(256) void cls_head_kernel(ClsArgs p) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= p.N) return;
  const float* x = p.in + (long)n * p.in_ns;
  float zl = -__builtin_huge_valf();
  for (int d = 0; d < p.D; ++d) {
    const float* wr = p.w + (long)d * p.Cin;
    float acc = 0.f;
    for (int k = 4 * lane; k < p.Cin; k += 256) {
      const f32x4 wv = *(const f32x4*)(wr + k), xv = *(const f32x4*)(x + k);
      acc = __builtin_fmaf(wv[0], xv[0], acc);
      acc = __builtin_fmaf(wv[1], xv[1], acc);
      acc = __builtin_fmaf(wv[2], xv[2], acc);
      acc = __builtin_fmaf(wv[3], xv[3], acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == d) zl = acc + (p.bias ? p.bias[d] : 0.f);
  }
  float mx = zl;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  const float e = lane < p.D ? expf(zl - mx) : 0.f;
  float s = e;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane < p.D) {
    p.out[(long)n * p.out_ns + lane] = e / s;
    if (p.logits) p.logits[(long)n * p.logit_ns + lane] = zl;
  }
}

}  // namespace

static bool cls_head_eligible(const fp_op& op) {
  if (op.kind != FP_OP_CLS_HEAD || op.flags || op.act != FP_ACT_NONE || op.res_mode != FP_RES_NONE || op.out_cmul != 1) return false;
  if (op.OH != 1 || op.OW != 1 || op.KH != 1 || op.KW != 1 || op.stride != 1 || op.pad_t || op.pad_l) return false;
  if (op.Cin % 4 || op.Cin > 4096 || op.Cout < 1 || op.Cout > 64) return false;
  if (op.in_off % 4 || op.in_ns % 4 || op.w_off < 0 || op.w_off % 4) return false;
  if (op.out_ns < op.Cout || (op.res_off >= 0 && op.res_ns < op.Cout)) return false;
  return true;
}

int fp_launch_cls_head(const fp_op& op, const fp_launch& L) {
  if (!cls_head_eligible(op)) return FP_ERR_UNSUPPORTED;
  if (fp_dry_run(L, "cls_head_kernel")) return FP_OK;
  ClsArgs a;
  memset(&a, 0, sizeof(a));
  a.in = L.arena + op.in_off;
  a.out = L.arena + op.out_off;
  a.logits = op.res_off >= 0 ? L.arena + op.res_off : nullptr;
  a.w = L.weights + op.w_off;
  a.bias = op.bias_off >= 0 ? L.weights + op.bias_off : nullptr;
  a.in_ns = op.in_ns; a.out_ns = op.out_ns; a.logit_ns = op.res_ns;
  a.N = op.N; a.Cin = op.Cin; a.D = op.Cout;
  hipLaunchKernelGGL(cls_head_kernel, dim3((unsigned)fp_ceil_div(op.N, 4)), dim3(256), 0, L.s, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}
