// moteval.hip — tracker evaluation against ground truth: the CLEAR-MOT matching walk and the pair counts behind IDF1, on the
// device (gfx950).  Build-defined restatement (DESIGN §7 "Tracker evaluation"; include/facepath.h states the procedure):
// nothing of TrackEval or py-motmetrics is in the tree, the numpy path of tracking_eval.py states the same procedure
// sequentially in fp64 and is this file's oracle.  Build with -ffp-contract=off: an IoU, a score and every reduced cost of the
// assignment are the same fp64 numbers on the device, in the host emulator and in numpy, so every decision is the same.
//
// 1. fp_mot_match: ONE launch, one workgroup per sequence, marching the sequence's frames in order (the shape of
//    tracklets.hip).  Per frame:
//      A. wave 0 stages the ground-truth rows (box, dense id, the hypothesis its id held in the previous frame), wave 1 the
//         hypothesis rows, in LDS;
//      B. the whole workgroup fills sim[64][64] (fp64, 32 KiB of LDS) and adds the admissible pairs to the sequence's
//         pot[G][H] in global memory: ids are unique inside a frame, so a cell has one writer per frame, and a sequence's
//         matrix is touched by its own workgroup only -- no atomics;
//      C. wave 0 runs the shortest-augmenting-path assignment with COLUMNS ON LANES (wave_assign of motassign.h, which
//         hota.hip shares; the score comes in as a functor): minv, way, v, used and the column's row
//         p are lane-private, u sits on the lane of its row, the scan of a step is one LDS read and three fp64 operations per
//         lane, delta / j1 come from a wave arg-min over (value, lane), lower lane on equal values (the minimum by DPP row
//         steps and readlanes, then the lowest lane of the ballot of the lanes that hold it) -- the ascending scan with
//         strict comparisons of the written procedure.  Lane indices are wave-uniform: readlanes, no shuffles.  The score is
//         never stored: it is sim, the threshold and one integer comparison;
//      D. lane i of wave 0 owns ground-truth row i: identity switch, hit / run / seen counters, last and cur (stamped with
//         the frame number, so nothing is cleared per frame) in global memory; sum_iou is added one match after the other in
//         ascending row order.
//    No scratch, no global atomics, no host synchronisation: two runs are bit-identical.  A single long sequence is a chain
//    of dependent frames on one workgroup: latency-bound by construction.
// 2. fp_mot_match_emulate: the same __host__ __device__ decision code (IoU, score, reduced cost, the strict comparisons)
//    serially on host memory, the assignment in its textbook form.
#include <math.h>

#include <vector>

#include "common.h"
#include "motassign.h"

namespace {

using namespace motassign;   // mot_iou, mot_reduced, mot_clamp, mot_frame; wave_assign and host_assign
constexpr int TPB = 256;

// rows of the per-id state: state[k][n_gt_ids]
enum { S_LAST = 0, S_CURH = 1, S_STAMP = 2, S_SEEN = 3, S_HIT = 4, S_RUNS = 5, S_ROWS = 6 };

struct MotArgs {
  const double* gt_box;
  const int* gt_id;
  const int* gt_off;
  long n_gt;
  const double* hy_box;
  const int* hy_id;
  const int* hy_off;
  long n_hy;
  const int* frame_base;   // [S + 1]
  const int* gt_id_base;   // [S + 1]
  const int* hy_id_count;  // [S]
  const long* pot_base;    // [S + 1]
  int S;
  long n_frames, n_gt_ids, n_pot;
  double thr;
  long* counts;            // [S][4] TP FN FP IDSW
  double* sum_iou;         // [S]
  int* gt_match;           // [n_gt]
  unsigned char* gt_switch;
  int* state;              // [S_ROWS][n_gt_ids]
  int* pot;                // [n_pot]
};

// ---------------------------------------------------------------------------------------- the decision code, host and device
// prev_h: the hypothesis id the ground-truth id held in the previous frame, -1 for none
__host__ __device__ __forceinline__ double mot_score(double sim, double thr, int prev_h, int h) {
  return sim >= thr ? sim + (prev_h == h ? 1000.0 : 0.0) : 0.0;
}

// The sequence's slice of the arrays; every index derived from device data is clamped into the arrays.
struct MotSeq {
  long f0, f1, id0, pot0;
  int G, H;
};
__host__ __device__ __forceinline__ MotSeq mot_seq(const MotArgs& p, int s) {
  MotSeq q;
  q.f0 = mot_clamp(p.frame_base[s], 0, p.n_frames);
  q.f1 = mot_clamp(p.frame_base[s + 1], q.f0, p.n_frames);
  q.id0 = mot_clamp(p.gt_id_base[s], 0, p.n_gt_ids);
  q.G = (int)(mot_clamp(p.gt_id_base[s + 1], q.id0, p.n_gt_ids) - q.id0);
  q.pot0 = mot_clamp(p.pot_base[s], 0, p.n_pot);
  const long cells = mot_clamp(p.pot_base[s + 1], q.pot0, p.n_pot) - q.pot0;
  int H = p.hy_id_count[s];
  H = H < 0 ? 0 : H;
  if ((long)q.G * (long)H > cells) H = q.G > 0 ? (int)(cells / q.G) : 0;
  q.H = H;
  return q;
}

// ------------------------------------------------------------------------------------------------------------- the kernel
__global__ __launch_bounds__(TPB) void mot_match_kernel(MotArgs p) {
  __shared__ double s_sim[MR * MR];
  __shared__ double s_gb[MR * 4], s_hb[MR * 4];
  __shared__ int s_gid[MR], s_hid[MR], s_prev[MR];

  const int tid = threadIdx.x, lane = tid & (FP_WAVE - 1), wave = tid >> 6;
  const int s = blockIdx.x;
  const MotSeq q = mot_seq(p, s);
  const int G = q.G, H = q.H;
  const long tg = p.n_gt_ids;
  int* st = p.state + q.id0;
  int* pot = p.pot + q.pot0;
  const double thr = p.thr;
  long TP = 0, FN = 0, FP = 0, IDSW = 0;
  double acc = 0.0;

  for (long gf = q.f0; gf < q.f1; ++gf) {
    const int f = (int)(gf - q.f0);
    const MotFrame fr = mot_frame(p, gf, G, H);
    const int n = fr.n, m = fr.m;
    // A. the frame's rows
    if (wave == 0 && lane < n) {
      const double* b = p.gt_box + 4 * (fr.g0 + lane);
      for (int k = 0; k < 4; ++k) s_gb[4 * lane + k] = b[k];
      const int g = (int)mot_clamp(p.gt_id[fr.g0 + lane], 0, G - 1);
      s_gid[lane] = g;
      s_prev[lane] = st[S_STAMP * tg + g] == f + 1 ? st[S_CURH * tg + g] : -1;
    }
    if (wave == 1 && lane < m) {
      const double* b = p.hy_box + 4 * (fr.h0 + lane);
      for (int k = 0; k < 4; ++k) s_hb[4 * lane + k] = b[k];
      s_hid[lane] = (int)mot_clamp(p.hy_id[fr.h0 + lane], 0, H - 1);
    }
    __syncthreads();
    // B. similarities; every admissible pair counts toward the id assignment
    for (int idx = tid; idx < n * m; idx += TPB) {
      const int i = idx / m, j = idx - i * m;
      const double sim = mot_iou(s_gb + 4 * i, s_hb + 4 * j);
      s_sim[i * MR + j] = sim;
      if (sim >= thr) pot[(long)s_gid[i] * H + s_hid[j]] += 1;
    }
    __syncthreads();
    if (wave == 0) {
      // C. assignment (motassign.h): lane = column - 1 (v, minv, way, used, p_row) and lane = row - 1 (u, rowin)
      const int N = n > m ? n : m;
      const int hid = lane < m ? s_hid[lane] : -1;
      const int p_row = wave_assign(n, m, lane, [&](int i0, double ui0, double v) {
        const double sc = (i0 < n && lane < m) ? mot_score(s_sim[i0 * MR + lane], thr, s_prev[i0], hid) : 0.0;
        return mot_reduced(sc, ui0, v);
      });
      // D. lane = ground-truth row
      const int col = wave_column_of_row(p_row, N, lane);
      bool matched = false, sw = false;
      double sv = 0.0;
      int h = -1;
      if (lane < n && col >= 0 && col < m) {
        sv = s_sim[lane * MR + col];
        h = s_hid[col];
        matched = mot_score(sv, thr, s_prev[lane], h) > 0.0;
      }
      if (lane < n) {
        int* e = st + s_gid[lane];
        if (matched) {
          const int last = e[S_LAST * tg];
          sw = last != 0 && last != h + 1;
          e[S_HIT * tg] += 1;
          if (s_prev[lane] < 0) e[S_RUNS * tg] += 1;
          e[S_LAST * tg] = h + 1;
          e[S_CURH * tg] = h;
          e[S_STAMP * tg] = f + 2;                          // read as "held in the previous frame" by frame f + 1 alone
        }
        e[S_SEEN * tg] += 1;
        p.gt_match[fr.g0 + lane] = matched ? (int)(fr.h0 + col) : -1;
        p.gt_switch[fr.g0 + lane] = sw ? 1 : 0;
      }
      const unsigned long long mm = __ballot(matched), ms = __ballot(sw);
      const int k = __popcll(mm);
      IDSW += __popcll(ms);
      TP += k;
      FN += n - k;
      FP += m - k;
      for (unsigned long long b = mm; b; b &= b - 1) acc += lane_d(sv, __ffsll((long long)b) - 1);
    }
    __syncthreads();   // the state and pot of this frame are behind a workgroup barrier before the next frame reads them
  }
  if (tid == 0) {
    long* c = p.counts + 4 * (long)s;
    c[0] = TP, c[1] = FN, c[2] = FP, c[3] = IDSW;
    p.sum_iou[s] = acc;
  }
}

// --------------------------------------------------------------------------------------------------------------- the host
MotArgs mot_args(const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt, const double* hy_boxes,
                 const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy, const int32_t* frame_base,
                 const int32_t* gt_id_base, const int32_t* hy_id_count, const int64_t* pot_base, int n_seqs, int64_t n_frames,
                 int64_t n_gt_ids, int64_t n_pot, double thr, int64_t* counts, double* sum_iou, int32_t* gt_match,
                 uint8_t* gt_switch, void* workspace) {
  MotArgs a;
  a.gt_box = gt_boxes; a.gt_id = gt_id; a.gt_off = gt_off; a.n_gt = (long)n_gt;
  a.hy_box = hy_boxes; a.hy_id = hy_id; a.hy_off = hy_off; a.n_hy = (long)n_hy;
  a.frame_base = frame_base; a.gt_id_base = gt_id_base; a.hy_id_count = hy_id_count; a.pot_base = (const long*)pot_base;
  a.S = n_seqs; a.n_frames = (long)n_frames; a.n_gt_ids = (long)n_gt_ids; a.n_pot = (long)n_pot; a.thr = thr;
  a.counts = (long*)counts; a.sum_iou = sum_iou; a.gt_match = gt_match; a.gt_switch = gt_switch;
  a.state = (int*)workspace;
  a.pot = a.state ? a.state + (long)S_ROWS * (long)(n_gt_ids > 0 ? n_gt_ids : 0) : nullptr;
  return a;
}

size_t mot_ws_bytes(int64_t n_gt_ids, int64_t n_pot) {
  if (n_gt_ids < 0 || n_pot < 0) return 0;
  const int64_t ints = (int64_t)S_ROWS * n_gt_ids + n_pot;
  return (size_t)(ints > 0 ? ints : 1) * sizeof(int32_t);
}

int check_mot(const MotArgs& a, size_t ws_bytes) {
  if (a.S < 0 || a.n_gt < 0 || a.n_hy < 0 || a.n_frames < 0 || a.n_gt_ids < 0 || a.n_pot < 0) return FP_ERR_INVALID_ARG;
  if (a.n_gt >= (1L << 31) || a.n_hy >= (1L << 31) || a.n_frames >= (1L << 31) - 2 || a.n_gt_ids >= (1L << 31))
    return FP_ERR_INVALID_ARG;                              // int32 CSR offsets, ids and frame stamps
  if (!(a.thr == a.thr)) return FP_ERR_INVALID_ARG;
  if (!a.gt_off || !a.hy_off || !a.frame_base || !a.gt_id_base || !a.hy_id_count || !a.pot_base || !a.state) return FP_ERR_INVALID_ARG;
  if (a.S > 0 && (!a.counts || !a.sum_iou)) return FP_ERR_INVALID_ARG;
  if (a.n_gt > 0 && (!a.gt_box || !a.gt_id || !a.gt_match || !a.gt_switch)) return FP_ERR_INVALID_ARG;
  if (a.n_hy > 0 && (!a.hy_box || !a.hy_id)) return FP_ERR_INVALID_ARG;
  if (ws_bytes < mot_ws_bytes(a.n_gt_ids, a.n_pot)) return FP_ERR_INVALID_ARG;
  if (((uintptr_t)a.gt_box | (uintptr_t)a.hy_box | (uintptr_t)a.pot_base | (uintptr_t)a.counts | (uintptr_t)a.sum_iou) % 8 ||
      ((uintptr_t)a.gt_id | (uintptr_t)a.hy_id | (uintptr_t)a.gt_off | (uintptr_t)a.hy_off | (uintptr_t)a.frame_base |
       (uintptr_t)a.gt_id_base | (uintptr_t)a.hy_id_count | (uintptr_t)a.gt_match | (uintptr_t)a.state) % 4)
    return FP_ERR_ALIGNMENT;
  return FP_OK;
}

// One sequence on host memory: the written procedure with the assignment in its textbook form.
void emulate_seq(const MotArgs& p, int s) {
  const MotSeq q = mot_seq(p, s);
  const int G = q.G, H = q.H;
  const long tg = p.n_gt_ids;
  int* st = p.state + q.id0;
  int* pot = p.pot + q.pot0;
  long TP = 0, FN = 0, FP = 0, IDSW = 0;
  double acc = 0.0;
  std::vector<double> sim(MR * MR);
  std::vector<int> gid(MR), hid(MR), prev(MR);
  HostAssign as;
  for (long gf = q.f0; gf < q.f1; ++gf) {
    const int f = (int)(gf - q.f0);
    const MotFrame fr = mot_frame(p, gf, G, H);
    const int n = fr.n, m = fr.m, N = n > m ? n : m;
    for (int i = 0; i < n; ++i) {
      gid[i] = (int)mot_clamp(p.gt_id[fr.g0 + i], 0, G - 1);
      prev[i] = st[S_STAMP * tg + gid[i]] == f + 1 ? st[S_CURH * tg + gid[i]] : -1;
    }
    for (int j = 0; j < m; ++j) hid[j] = (int)mot_clamp(p.hy_id[fr.h0 + j], 0, H - 1);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < m; ++j) {
        const double sv = mot_iou(p.gt_box + 4 * (fr.g0 + i), p.hy_box + 4 * (fr.h0 + j));
        sim[i * MR + j] = sv;
        if (sv >= p.thr) pot[(long)gid[i] * H + hid[j]] += 1;
      }
    auto score = [&](int i, int j) { return (i < n && j < m) ? mot_score(sim[i * MR + j], p.thr, prev[i], hid[j]) : 0.0; };
    host_assign(n, m, score, as);
    int k = 0;
    for (int i = 0; i < n; ++i) {
      const int col = host_column_of_row(as, N, i);
      const bool matched = col >= 0 && col < m && score(i, col) > 0.0;
      int* e = st + gid[i];
      bool sw = false;
      if (matched) {
        const int h = hid[col], last = e[S_LAST * tg];
        sw = last != 0 && last != h + 1;
        e[S_HIT * tg] += 1;
        if (prev[i] < 0) e[S_RUNS * tg] += 1;
        e[S_LAST * tg] = h + 1;
        e[S_CURH * tg] = h;
        e[S_STAMP * tg] = f + 2;
        acc += sim[i * MR + col];
        ++k;
      }
      e[S_SEEN * tg] += 1;
      IDSW += sw;
      p.gt_match[fr.g0 + i] = matched ? (int)(fr.h0 + col) : -1;
      p.gt_switch[fr.g0 + i] = sw ? 1 : 0;
    }
    TP += k;
    FN += n - k;
    FP += m - k;
  }
  long* c = p.counts + 4 * (long)s;
  c[0] = TP, c[1] = FN, c[2] = FP, c[3] = IDSW;
  p.sum_iou[s] = acc;
}

}  // namespace

extern "C" {

size_t fp_mot_match_workspace(int64_t n_gt_ids, int64_t n_pot) { return mot_ws_bytes(n_gt_ids, n_pot); }

int fp_mot_match(const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt, const double* hy_boxes,
                 const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy, const int32_t* frame_base,
                 const int32_t* gt_id_base, const int32_t* hy_id_count, const int64_t* pot_base, int n_seqs, int64_t n_frames,
                 int64_t n_gt_ids, int64_t n_pot, double thr, int64_t* counts, double* sum_iou, int32_t* gt_match,
                 uint8_t* gt_switch, void* workspace, size_t ws_bytes, void* stream) {
  const MotArgs a = mot_args(gt_boxes, gt_id, gt_off, n_gt, hy_boxes, hy_id, hy_off, n_hy, frame_base, gt_id_base, hy_id_count,
                             pot_base, n_seqs, n_frames, n_gt_ids, n_pot, thr, counts, sum_iou, gt_match, gt_switch, workspace);
  const int rc = check_mot(a, ws_bytes);
  if (rc != FP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, mot_ws_bytes(n_gt_ids, n_pot), s) != hipSuccess ||
      (n_gt > 0 && (hipMemsetAsync(gt_match, 0xFF, (size_t)n_gt * sizeof(int32_t), s) != hipSuccess ||
                    hipMemsetAsync(gt_switch, 0, (size_t)n_gt, s) != hipSuccess))) {
    fp_set_hip_error(hipGetLastError());
    return FP_ERR_LAUNCH;
  }
  if (n_seqs == 0) return FP_OK;
  hipLaunchKernelGGL(mot_match_kernel, dim3((unsigned)n_seqs), dim3(TPB), 0, s, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_mot_match_emulate(const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt,
                         const double* hy_boxes, const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy,
                         const int32_t* frame_base, const int32_t* gt_id_base, const int32_t* hy_id_count,
                         const int64_t* pot_base, int n_seqs, int64_t n_frames, int64_t n_gt_ids, int64_t n_pot, double thr,
                         int64_t* counts, double* sum_iou, int32_t* gt_match, uint8_t* gt_switch, void* workspace,
                         size_t ws_bytes) {
  const MotArgs a = mot_args(gt_boxes, gt_id, gt_off, n_gt, hy_boxes, hy_id, hy_off, n_hy, frame_base, gt_id_base, hy_id_count,
                             pot_base, n_seqs, n_frames, n_gt_ids, n_pot, thr, counts, sum_iou, gt_match, gt_switch, workspace);
  const int rc = check_mot(a, ws_bytes);
  if (rc != FP_OK) return rc;
  const size_t ws = mot_ws_bytes(n_gt_ids, n_pot);
  for (size_t i = 0; i < ws; ++i) ((unsigned char*)workspace)[i] = 0;
  for (int64_t i = 0; i < n_gt; ++i) gt_match[i] = -1, gt_switch[i] = 0;
  for (int s = 0; s < n_seqs; ++s) emulate_seq(a, s);
  return FP_OK;
}

}  // extern "C"
