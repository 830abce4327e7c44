// pnet.hip — the two kernels around MTCNN's proposal net (include/facepath.h section 9).  P-Net itself runs level by level as
// a plan of generic ops (conv + PReLU, ceil-mode max pool, a 1x1 conv for both heads: modules/mtcnn/mtcnn.py); this file holds
// what comes before and after it:
//   * fp_pnet_level_images: the pyramid level of a group of equally sized frames, area-averaged from the u8 frames in exact
//     integer arithmetic, rounded half-to-even to u8 and written as (v - 127.5) / 128 into the plan's input (4-float pixels);
//   * fp_pnet_threshold: softmax over the two class logits of every output cell, and a 24-byte record (regression, score, level
//     and cell) for each cell with p >= t1, through the frame's atomic counter.  fp_mtcnn_stage1 puts the records into
//     (level, cell) order before it uses them, so the order of the atomics does not matter.
// A fused form (level pixels, all three convs and the heads of a 16 x 16 tile out of LDS, fp32 FMAs) was built first and
// measured slower than this one (FINDINGS 64); it was dropped.
#include "common.h"

namespace {

// The u8 value of level pixel (ly, lx): the area-weighted mean of the frame over [lx W / lw, (lx + 1) W / lw) x
// [ly H / lh, (ly + 1) H / lh), in exact integer arithmetic (lengths in units of 1 / lw and 1 / lh source pixels, so the
// weights are integers and the mean is S / (W H)), rounded half-to-even.
__device__ __forceinline__ int round_half_even(long s, long d) {
  // the quotient is a grey level (<= 255): estimate it in fp64, then make it the exact floor (a 64-bit integer division costs
  // far more on this machine)
  long q = (long)((double)s / (double)d);
  long r = s - q * d;
  if (r < 0) { --q; r += d; }
  else if (r >= d) { ++q; r -= d; }
  if (2 * r > d || (2 * r == d && (q & 1))) ++q;
  return (int)q;
}

// 32-bit inner sums: a row's weights add up to W, so a row sum is at most 255 W < 2^32 for every frame width the
// descriptors admit (W <= 32767); only the sum over rows is 64-bit.
__device__ void level_pixel(const uint8_t* f, int H, int W, int lh, int lw, int ly, int lx, float out[3]) {
  // lx W < lw W <= 32767^2 and ly H < lh H <= 65535^2 both fit 32 bits unsigned: 32-bit divisions
  const unsigned X0u = (unsigned)lx * (unsigned)W, Y0u = (unsigned)ly * (unsigned)H;
  const long X0 = X0u, Y0 = Y0u, Y1 = Y0 + H;
  const int xa = (int)(X0u / (unsigned)lw), xb = (int)((unsigned)(X0u + (unsigned)W - 1u) / (unsigned)lw);
  const int ya = (int)(Y0u / (unsigned)lh), yb = (int)((Y0u + (unsigned)H - 1u) / (unsigned)lh);
  // weights of the first and the last column (interior columns weigh lw); one column: the whole cell
  const unsigned w_first = xa == xb ? (unsigned)W : (unsigned)((long)(xa + 1) * lw - X0);
  const unsigned w_last = (unsigned)(X0 + W - (long)xb * lw);
  long acc[3] = {0, 0, 0};
  for (int y = ya; y <= yb; ++y) {
    const long wy = min((long)(y + 1) * lh, Y1) - max((long)y * lh, Y0);
    const uint8_t* row = f + ((size_t)y * W) * 3;
    unsigned r0 = w_first * row[xa * 3], r1 = w_first * row[xa * 3 + 1], r2 = w_first * row[xa * 3 + 2];
    unsigned m0 = 0, m1 = 0, m2 = 0;
    for (int x = xa + 1; x < xb; ++x) {
      m0 += row[x * 3];
      m1 += row[x * 3 + 1];
      m2 += row[x * 3 + 2];
    }
    r0 += m0 * (unsigned)lw; r1 += m1 * (unsigned)lw; r2 += m2 * (unsigned)lw;
    if (xb > xa) {
      r0 += w_last * row[xb * 3]; r1 += w_last * row[xb * 3 + 1]; r2 += w_last * row[xb * 3 + 2];
    }
    acc[0] += wy * r0;
    acc[1] += wy * r1;
    acc[2] += wy * r2;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = ((float)round_half_even(acc[c], (long)W * H) - 127.5f) * 0.0078125f;
}

struct LevelArgs {
  const uint8_t* frames;
  size_t frames_bytes;
  const fp_frame_desc* descs;
  const int32_t* frame_idx;
  float* out;
  int n_frames, n, lh, lw;
};

__global__ __launch_bounds__(256) void level_images_kernel(LevelArgs a) {
  const int per = a.lh * a.lw, pix = (int)(blockIdx.x * 256u + threadIdx.x), i = blockIdx.y;
  if (pix >= per) return;
  const long idx = (long)i * per + pix;
  const int ly = (int)((unsigned)pix / (unsigned)a.lw), lx = pix - ly * a.lw;
  float v[3] = {0.f, 0.f, 0.f};
  const int f = a.frame_idx[i];
  if ((unsigned)f < (unsigned)a.n_frames) {
    const fp_frame_desc d = a.descs[f];
    if (d.h >= a.lh && d.w >= a.lw && d.w <= FP_FRAME_MAX_W && d.h <= 65535 && d.off >= 0 &&
        (size_t)d.off + (size_t)d.h * d.w * 3 <= a.frames_bytes)
      level_pixel(a.frames + d.off, d.h, d.w, a.lh, a.lw, ly, lx, v);
  }
  *(f32x4*)(a.out + idx * 4) = f32x4{v[0], v[1], v[2], 0.f};
}

struct ThrArgs {
  const float* head;
  const int32_t* frame_idx;
  fp_pnet_cand* cand;
  int32_t* counts;
  int32_t* overflow;
  int ld, n_frames, n, cells, level, cap;
  float t1;
};

__global__ __launch_bounds__(256) void threshold_kernel(ThrArgs a) {
  const int cell = (int)(blockIdx.x * 256u + threadIdx.x), i = blockIdx.y;
  if (cell >= a.cells) return;
  const long idx = (long)i * a.cells + cell;
  const int f = a.frame_idx[i];
  if ((unsigned)f >= (unsigned)a.n_frames) return;
  const float* z = a.head + idx * a.ld;
  const f32x4 lo = *(const f32x4*)z;
  const float z4 = z[4], z5 = z[5];
  const float mx = fmaxf(lo[0], lo[1]);
  const float e0 = expf(lo[0] - mx), e1 = expf(lo[1] - mx);
  const float p = e1 / (e0 + e1);
  if (p >= a.t1) {
    const int slot = atomicAdd(&a.counts[f], 1);
    if (slot < a.cap) {
      fp_pnet_cand* o = a.cand + (size_t)f * a.cap + slot;
      *(f32x4*)o->reg = f32x4{lo[2], lo[3], z4, z5};
      o->score = p;
      o->key = ((uint32_t)a.level << 24) | (uint32_t)cell;
    } else {
      a.overflow[f] = 1;
    }
  }
}

}  // namespace

extern "C" int fp_pnet_level_images(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames,
                                    const int32_t* frame_idx, int n, int lh, int lw, float* out, void* stream) {
  if (!frames || !descs || !frame_idx || !out) return FP_ERR_INVALID_ARG;
  if (n_frames < 1 || n < 0 || n > 65535 || lh < 1 || lw < 1 || lh > 65535 || lw > FP_FRAME_MAX_W || ((uintptr_t)out & 15)) return FP_ERR_INVALID_ARG;
  if (n == 0) return FP_OK;
  LevelArgs a{frames, frames_bytes, descs, frame_idx, out, n_frames, n, lh, lw};
  hipLaunchKernelGGL(level_images_kernel, dim3((unsigned)fp_ceil_div((long)lh * lw, 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

extern "C" int fp_pnet_threshold(const float* head, int ld, const int32_t* frame_idx, int n, int n_frames, int oh, int ow, int level,
                                 float t1, int cap, fp_pnet_cand* cand, int32_t* counts, int32_t* overflow, void* stream) {
  if (!head || !frame_idx || !cand || !counts || !overflow) return FP_ERR_INVALID_ARG;
  if (ld < 8 || ld % 4 || ((uintptr_t)head & 15) || n < 0 || n > 65535 || n_frames < 1 || oh < 1 || ow < 1 || (long)oh * ow > (1L << 24) ||
      level < 0 || level > 127 || cap < 1 || cap > FP_MTCNN_MAX_CAP)
    return FP_ERR_INVALID_ARG;
  if (n == 0) return FP_OK;
  ThrArgs a{head, frame_idx, cand, counts, overflow, ld, n_frames, n, oh * ow, level, cap, t1};
  hipLaunchKernelGGL(threshold_kernel, dim3((unsigned)fp_ceil_div((long)oh * ow, 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}
