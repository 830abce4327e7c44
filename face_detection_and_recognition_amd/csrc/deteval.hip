// deteval.hip — detector evaluation against ground truth: the COCO bbox procedure (one category, no crowd) on the device
// (gfx950).  Build-defined restatement: nothing of pycocotools is in the tree, the numpy path of
// evaluation.py states the same procedure sequentially in fp64 and is this file's oracle.  Compiled with
// -ffp-contract=off: an IoU here is the same fp64 number numpy computes, so every >= decision is the same.
//
//  * det_match_kernel: greedy matching, one workgroup per (image, area range), all IoU thresholds at once.
//  * pr_accumulate_kernel: one workgroup per (threshold, area range, maxDet) curve: counts, precision / recall, the
//    suffix maximum and the samples at the recall thresholds, without materialising a curve.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int MATCH_THREADS = 256;
constexpr int GT_STAGE = 512;          // ground-truth boxes of an image kept in LDS; the rest is read from global memory

// xywh boxes, fp64, the operations in the order of section 1 of the specification.
__device__ __forceinline__ double box_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh) {
  const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  const double ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  if (iw <= 0.0 || ih <= 0.0) return 0.0;
  const double i = iw * ih;
  const double u = dw * dh + gw * gh - i;
  return i / u;
}

// Greedy matching of one image's detections (score order, already cut to the largest maxDet) against its ground truth,
// for one area range and all T thresholds.
//   * a lane owns the GTs g = tid, tid + 256, ...; word[g] = bit t: matched at threshold t, bit 31: ignored in this range.
//     Only the owner reads or writes a GT's word (LDS for the first GT_STAGE GTs, the caller's workspace behind them).
//   * per detection the pick "largest IoU >= best, on equal IoU the later GT" is the maximum of the key (IoU, position),
//     taken first over the not ignored and then over the ignored GTs that are unmatched at t.  An IoU in [0, 1] orders as
//     its bit pattern, so the maximum is two rounds of integer LDS atomics per (class, threshold): the largest IoU bits,
//     then the largest position among the GTs that hold exactly those bits.  Integer maxima do not depend on the order in
//     which lanes arrive: the result is independent of scheduling.
//   * slot value 0 = no candidate (IoU bits are stored + 1, so that an IoU of 0 at a threshold of 0 still counts).
__global__ __launch_bounds__(MATCH_THREADS) void det_match_kernel(
    const double* __restrict__ gt_boxes, const double* __restrict__ gt_area, const int* __restrict__ gt_off,
    const double* __restrict__ dt_boxes, const int* __restrict__ dt_off, long n_gt, long n_dt,
    const double* __restrict__ iou_thrs, int T, const double* __restrict__ area_rngs, unsigned char* __restrict__ matched,
    unsigned char* __restrict__ ignored, int* __restrict__ npig, unsigned* __restrict__ words) {
  __shared__ double sx[GT_STAGE], sy[GT_STAGE], sw[GT_STAGE], sh[GT_STAGE], siou[GT_STAGE];
  __shared__ unsigned sword[GT_STAGE];
  __shared__ u64 slot_iou[2][2][FP_DETEVAL_MAX_THRS];     // [buffer][0 = not ignored, 1 = ignored][t]
  __shared__ int slot_pos[2][2][FP_DETEVAL_MAX_THRS];
  __shared__ double sthr[FP_DETEVAL_MAX_THRS];
  __shared__ int s_npig;

  const int tid = threadIdx.x;
  const int img = blockIdx.x, a = blockIdx.y;
  long g0 = gt_off[img], g1 = gt_off[img + 1], d0 = dt_off[img], d1 = dt_off[img + 1];
  g0 = g0 < 0 ? 0 : g0;                                   // a malformed CSR must not reach past the arrays
  d0 = d0 < 0 ? 0 : d0;
  g1 = g1 > n_gt ? n_gt : g1;
  d1 = d1 > n_dt ? n_dt : d1;
  const int G = g1 > g0 ? (int)(g1 - g0) : 0;
  const int D = d1 > d0 ? (int)(d1 - d0) : 0;
  const double lo = area_rngs[2 * a], hi = area_rngs[2 * a + 1];
  unsigned* gword = words + (size_t)a * (size_t)n_gt + g0;
  const size_t out0 = (size_t)a * (size_t)T * (size_t)n_dt + (size_t)d0;

  if (tid == 0) s_npig = 0;
  if (tid < T) sthr[tid] = fmin(iou_thrs[tid], 1.0 - 1e-10);
  if (tid < 2 * FP_DETEVAL_MAX_THRS) {
    (&slot_iou[0][0][0])[tid] = 0;
    (&slot_pos[0][0][0])[tid] = -1;
  }
  __syncthreads();
  int cnt = 0;
  for (int g = tid; g < G; g += MATCH_THREADS) {
    const double* b = gt_boxes + 4 * (g0 + g);
    const double ar = gt_area[g0 + g];
    const bool ig = ar < lo || ar > hi;
    cnt += ig ? 0 : 1;
    const unsigned w = ig ? 0x80000000u : 0u;
    if (g < GT_STAGE) {
      sx[g] = b[0], sy[g] = b[1], sw[g] = b[2], sh[g] = b[3];
      sword[g] = w;
    } else {
      gword[g] = w;
    }
  }
  if (cnt) atomicAdd(&s_npig, cnt);
  __syncthreads();
  if (tid == 0 && s_npig) atomicAdd(&npig[a], s_npig);

  for (int d = 0; d < D; ++d) {
    const double* b = dt_boxes + 4 * (d0 + d);
    const double dx = b[0], dy = b[1], dw = b[2], dh = b[3];
    const int buf = d & 1;
    if (G > 0) {
      // round 1: the largest IoU per (class, threshold)
      for (int g = tid; g < G; g += MATCH_THREADS) {
        double iou;
        unsigned w;
        if (g < GT_STAGE) {
          iou = box_iou(dx, dy, dw, dh, sx[g], sy[g], sw[g], sh[g]);
          siou[g] = iou;
          w = sword[g];
        } else {
          const double* q = gt_boxes + 4 * (g0 + g);
          iou = box_iou(dx, dy, dw, dh, q[0], q[1], q[2], q[3]);
          w = gword[g];
        }
        const int cls = w >> 31;
        const u64 key = (u64)__double_as_longlong(iou) + 1ull;
        for (int t = 0; t < T; ++t)
          if (!((w >> t) & 1u) && iou >= sthr[t]) atomicMax(&slot_iou[buf][cls][t], key);
      }
      __syncthreads();
      // round 2: the last GT among those that hold it
      for (int g = tid; g < G; g += MATCH_THREADS) {
        double iou;
        unsigned w;
        if (g < GT_STAGE) {
          iou = siou[g];
          w = sword[g];
        } else {
          const double* q = gt_boxes + 4 * (g0 + g);
          iou = box_iou(dx, dy, dw, dh, q[0], q[1], q[2], q[3]);
          w = gword[g];
        }
        const int cls = w >> 31;
        const u64 key = (u64)__double_as_longlong(iou) + 1ull;
        for (int t = 0; t < T; ++t)
          if (!((w >> t) & 1u) && iou >= sthr[t] && slot_iou[buf][cls][t] == key) atomicMax(&slot_pos[buf][cls][t], g);
      }
      __syncthreads();
    }
    // decisions: the owner of the chosen GT marks it, lane t writes the detection's flags
    const double da = dw * dh;
    const bool d_out = da < lo || da > hi;
    for (int t = 0; t < T; ++t) {
      const int pn = slot_pos[buf][0][t], pi = slot_pos[buf][1][t];
      const int pick = pn >= 0 ? pn : pi;
      if (pick >= 0 && (pick & (MATCH_THREADS - 1)) == tid) {
        if (pick < GT_STAGE) sword[pick] |= 1u << t;
        else gword[pick] |= 1u << t;
      }
      if (tid == t) {
        const size_t o = out0 + (size_t)t * (size_t)n_dt + (size_t)d;
        matched[o] = pick >= 0 ? 1 : 0;
        ignored[o] = pick >= 0 ? (pn >= 0 ? 0 : 1) : (d_out ? 1 : 0);
      }
    }
    // the other buffer was last read in the decisions of detection d - 1, a barrier ago
    if (tid < 2 * FP_DETEVAL_MAX_THRS) {
      (&slot_iou[buf ^ 1][0][0])[tid] = 0;
      (&slot_pos[buf ^ 1][0][0])[tid] = -1;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Precision / recall of one (threshold t, area range a, maxDet m) curve.
//
// The curve's detections are those with per-image rank < m that are not ignored, in the global stable score order.  With
// tp / fp the running counts, rc = tp / npig and pr = tp / (fp + tp + eps); the published procedure replaces pr by its
// suffix maximum and samples it at the first index with rc >= r.  Two facts let a workgroup do that without storing a curve:
//   * rc >= r is a statement about the integer tp: need(r) = the smallest k with (double)k / npig >= r, found exactly
//     by testing that same quotient.  The sample index is the need(r)-th true positive (the first detection for
//     need(r) <= 0, whose suffix maximum is that of the first true positive, or 0 without one).
//   * between two true positives tp stands still and fp grows, so pr does not increase: the suffix maximum at the k-th
//     true positive is the maximum of p_j = j / (fp_j + j + eps) over the true positives j >= k, fp_j = false positives
//     in front of the j-th true positive.  Quotients of the same integers by the same fp64 operations as numpy's.
// Pass 1 counts TP and FP; pass 2 walks the chunks from the back with the counts behind as a carry: an integer prefix
// sum gives every true positive its ordinal and fp_j, a prefix maximum (exact) its suffix maximum S_k, the chunk's S_k
// go to LDS by ordinal and the recall thresholds whose need falls into the chunk read them.
constexpr int PR_THREADS = 256, PR_E = 4, PR_CHUNK = PR_THREADS * PR_E;
constexpr int PR_RI = FP_DETEVAL_MAX_RECS / PR_THREADS;

__device__ __forceinline__ int pr_flag(const unsigned char* __restrict__ mt, const unsigned char* __restrict__ ig,
                                       const long* __restrict__ order, const int* __restrict__ rank_sorted, long j, int m) {
  // 0: not on the curve, 1: false positive, 2: true positive
  if (rank_sorted[j] >= m) return 0;
  const long i = order[j];
  if (ig[i]) return 0;
  return mt[i] ? 2 : 1;
}

__global__ __launch_bounds__(PR_THREADS) void pr_accumulate_kernel(
    const unsigned char* __restrict__ matched, const unsigned char* __restrict__ ignored, const long* __restrict__ order,
    const int* __restrict__ rank_sorted, long n_dt, const int* __restrict__ npig, int T, int A,
    const int* __restrict__ max_dets, int M, const double* __restrict__ rec_thrs, int R, double* __restrict__ precision,
    double* __restrict__ recall) {
  __shared__ double sS[PR_CHUNK];
  __shared__ long w_tp[4], w_fp[4];
  __shared__ int c_tp[4], c_fp[4];
  __shared__ double c_mx[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int curve = blockIdx.x;                           // (t, a, m), m fastest
  const int mi = curve % M, a = (curve / M) % A, t = curve / (M * A);
  const int m = max_dets[mi];
  const int np = npig[a];
  const size_t rstride = (size_t)A * M;                   // precision[t][r][a][m]
  double* prec = precision + (size_t)t * R * rstride + (size_t)a * M + mi;
  double* rec = recall + ((size_t)t * A + a) * M + mi;
  if (np <= 0) {                                          // no ground truth in this range: the cell stays -1
    for (int r = tid; r < R; r += PR_THREADS) prec[(size_t)r * rstride] = -1.0;
    if (tid == 0) *rec = -1.0;
    return;
  }
  const unsigned char* mt = matched + ((size_t)a * T + t) * (size_t)n_dt;
  const unsigned char* ig = ignored + ((size_t)a * T + t) * (size_t)n_dt;

  // pass 1: totals
  long tp = 0, fp = 0;
  for (long j = tid; j < n_dt; j += PR_THREADS) {
    const int f = pr_flag(mt, ig, order, rank_sorted, j, m);
    tp += f == 2;
    fp += f == 1;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    tp += __shfl_xor(tp, off);
    fp += __shfl_xor(fp, off);
  }
  if (lane == 0) w_tp[wave] = tp, w_fp[wave] = fp;
  __syncthreads();
  const long TP = w_tp[0] + w_tp[1] + w_tp[2] + w_tp[3], FP = w_fp[0] + w_fp[1] + w_fp[2] + w_fp[3];
  const double dnp = (double)np;
  if (tid == 0) *rec = (double)TP / dnp;                  // rc[-1]; 0 / npig = 0 without detections

  // need(r) of this thread's recall thresholds
  long need[PR_RI];
#pragma unroll
  for (int i = 0; i < PR_RI; ++i) {
    const int r = tid + i * PR_THREADS;
    need[i] = -1;
    if (r < R) {
      const double rv = rec_thrs[r];
      double c = ceil(rv * dnp);
      c = c < 0.0 ? 0.0 : (c > dnp + 1.0 ? dnp + 1.0 : c);
      long k = (long)c;
      while (k > 0 && (double)(k - 1) / dnp >= rv) --k;
      while (k <= np && (double)k / dnp < rv) ++k;
      k = k < 1 ? 1 : k;                                  // rc >= r at the first detection: its suffix maximum is S_1
      need[i] = k;
      if (k > TP) prec[(size_t)r * rstride] = 0.0;        // recall never reaches r (or there is no detection at all)
    }
  }

  const double eps = 2.220446049250313e-16;               // np.spacing(1)
  const long n_chunks = (n_dt + PR_CHUNK - 1) / PR_CHUNK;
  long after_tp = 0, after_fp = 0;                        // counts behind the chunk
  double after_mx = 0.0;                                  // every p_j is > 0
  for (long c = n_chunks - 1; c >= 0 && after_tp < TP; --c) {
    const long end = (c + 1) * PR_CHUNK < n_dt ? (c + 1) * PR_CHUNK : n_dt;   // this thread walks backwards from end - 1 - tid * E
    int fl[PR_E];
    int ltp = 0, lfp = 0;
#pragma unroll
    for (int e = 0; e < PR_E; ++e) {
      const long j = end - 1 - ((long)tid * PR_E + e);
      fl[e] = j >= c * PR_CHUNK ? pr_flag(mt, ig, order, rank_sorted, j, m) : 0;
      ltp += fl[e] == 2;
      lfp += fl[e] == 1;
    }
    // exclusive prefix sums over the threads = counts behind this thread's elements, inside the chunk
    int itp = ltp, ifp = lfp;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o1 = __shfl_up(itp, off), o2 = __shfl_up(ifp, off);
      if (lane >= off) itp += o1, ifp += o2;
    }
    if (lane == 63) c_tp[wave] = itp, c_fp[wave] = ifp;
    __syncthreads();
    int btp = 0, bfp = 0, ctp = 0, cfp = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) btp += c_tp[w], bfp += c_fp[w];
      ctp += c_tp[w], cfp += c_fp[w];
    }
    long xtp = after_tp + btp + itp - ltp, xfp = after_fp + bfp + ifp - lfp;   // behind this thread's first element
    // p_j of this thread's true positives, their running maximum
    double pv[PR_E];
    double lmx = 0.0;
#pragma unroll
    for (int e = 0; e < PR_E; ++e) {
      pv[e] = 0.0;
      if (fl[e] == 2) {
        const long k = TP - xtp;                          // ordinal, 1-based
        const long fb = FP - xfp;                         // false positives in front of it
        const double p = (double)k / ((double)fb + (double)k + eps);
        lmx = fmax(lmx, p);
        pv[e] = lmx;
        ++xtp;
      } else if (fl[e] == 1) {
        ++xfp;
      }
    }
    double imx = lmx;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double o = __shfl_up(imx, off);
      if (lane >= off) imx = fmax(imx, o);
    }
    const double emx_w = __shfl_up(imx, 1);               // exclusive, inside the wave
    if (lane == 63) c_mx[wave] = imx;
    __syncthreads();
    double bmx = after_mx, cmx = after_mx;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) bmx = fmax(bmx, c_mx[w]);
      cmx = fmax(cmx, c_mx[w]);
    }
    if (lane > 0) bmx = fmax(bmx, emx_w);
    // S_k by ordinal: the chunk holds the ordinals klo .. klo + ctp - 1
    const long klo = TP - after_tp - ctp + 1;
    long xk = TP - (after_tp + btp + itp - ltp);
#pragma unroll
    for (int e = 0; e < PR_E; ++e)
      if (fl[e] == 2) {
        sS[xk - klo] = fmax(bmx, pv[e]);
        --xk;
      }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PR_RI; ++i) {
      const int r = tid + i * PR_THREADS;
      if (r < R && need[i] >= klo && need[i] < klo + ctp) prec[(size_t)r * rstride] = sS[need[i] - klo];
    }
    after_tp += ctp;
    after_fp += cfp;
    after_mx = cmx;
    __syncthreads();                                      // sS and the wave totals are rewritten by the next chunk
  }
}

}  // namespace

extern "C" {

size_t fp_det_match_workspace(int64_t n_gt, int n_areas) {
  if (n_gt < 0 || n_areas <= 0) return 0;
  return (size_t)n_areas * (size_t)(n_gt > 0 ? n_gt : 1) * sizeof(uint32_t);
}

int fp_det_match(const double* gt_boxes, const double* gt_area, const int32_t* gt_off, const double* dt_boxes,
                 const int32_t* dt_off, int n_images, int64_t n_gt, int64_t n_dt, const double* iou_thrs, int n_thrs,
                 const double* area_rngs, int n_areas, uint8_t* matched, uint8_t* ignored, int32_t* npig, void* workspace,
                 size_t ws_bytes, void* stream) {
  if (!gt_off || !dt_off || !iou_thrs || !area_rngs || !npig || !workspace) return FP_ERR_INVALID_ARG;
  if (n_images < 0 || n_gt < 0 || n_dt < 0 || n_thrs < 1 || n_thrs > FP_DETEVAL_MAX_THRS || n_areas < 1 || n_areas > 65535)
    return FP_ERR_INVALID_ARG;
  if (n_gt >= (1LL << 31) || n_dt >= (1LL << 31)) return FP_ERR_INVALID_ARG;   // int32 CSR offsets
  if ((n_gt > 0 && (!gt_boxes || !gt_area)) || (n_dt > 0 && (!dt_boxes || !matched || !ignored))) return FP_ERR_INVALID_ARG;
  if (ws_bytes < fp_det_match_workspace(n_gt, n_areas)) return FP_ERR_INVALID_ARG;
  if (((uintptr_t)gt_boxes | (uintptr_t)gt_area | (uintptr_t)dt_boxes | (uintptr_t)iou_thrs | (uintptr_t)area_rngs) % 8 ||
      ((uintptr_t)workspace | (uintptr_t)npig | (uintptr_t)gt_off | (uintptr_t)dt_off) % 4)
    return FP_ERR_ALIGNMENT;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(npig, 0, (size_t)n_areas * sizeof(int32_t), s) != hipSuccess) {
    fp_set_hip_error(hipGetLastError());
    return FP_ERR_LAUNCH;
  }
  if (n_images == 0) return FP_OK;
  hipLaunchKernelGGL(det_match_kernel, dim3((unsigned)n_images, (unsigned)n_areas), dim3(MATCH_THREADS), 0, s, gt_boxes, gt_area,
                     (const int*)gt_off, dt_boxes, (const int*)dt_off, (long)n_gt, (long)n_dt, iou_thrs, n_thrs, area_rngs,
                     (unsigned char*)matched, (unsigned char*)ignored, (int*)npig, (unsigned*)workspace);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_pr_accumulate(const uint8_t* matched, const uint8_t* ignored, const int64_t* order, const int32_t* rank_sorted,
                     int64_t n_dt, const int32_t* npig, int n_thrs, int n_areas, const int32_t* max_dets, int n_maxdets,
                     const double* rec_thrs, int n_recs, double* precision, double* recall, void* stream) {
  if (!npig || !max_dets || !rec_thrs || !precision || !recall) return FP_ERR_INVALID_ARG;
  if (n_dt < 0 || n_thrs < 1 || n_areas < 1 || n_maxdets < 1 || n_recs < 1 || n_recs > FP_DETEVAL_MAX_RECS)
    return FP_ERR_INVALID_ARG;
  if (n_dt > 0 && (!matched || !ignored || !order || !rank_sorted)) return FP_ERR_INVALID_ARG;
  if ((long)n_thrs * n_areas * n_maxdets >= (1L << 31)) return FP_ERR_INVALID_ARG;
  if (((uintptr_t)order | (uintptr_t)rec_thrs | (uintptr_t)precision | (uintptr_t)recall) % 8 ||
      ((uintptr_t)rank_sorted | (uintptr_t)npig | (uintptr_t)max_dets) % 4)
    return FP_ERR_ALIGNMENT;
  hipLaunchKernelGGL(pr_accumulate_kernel, dim3((unsigned)(n_thrs * n_areas * n_maxdets)), dim3(PR_THREADS), 0, (hipStream_t)stream,
                     (const unsigned char*)matched, (const unsigned char*)ignored, (const long*)order, (const int*)rank_sorted,
                     (long)n_dt, (const int*)npig, n_thrs, n_areas, (const int*)max_dets, n_maxdets, rec_thrs, n_recs, precision,
                     recall);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
