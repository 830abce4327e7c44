// hota.hip — tracker evaluation: the two marches behind HOTA (DetA, AssA, LocA) on the device (gfx950).  Build-defined
// restatement of Luiten et al. 2020 (DESIGN §7 "Tracker evaluation: HOTA"; include/facepath.h states the procedure): nothing of
// TrackEval is in the tree, the numpy path of tracking_eval.py states the same procedure sequentially in fp64 and is this
// file's oracle.  Build with -ffp-contract=off: an IoU, a row sum, an alignment score and every reduced cost of the assignment
// are the same fp64 numbers on the device, in the host emulator and in numpy, so every decision is the same.
//
// 1. fp_hota_match: ONE launch, one workgroup of 256 threads per sequence (the shape of fp_mot_match), three phases:
//      pass 1, alignment, frame after frame: waves 0 / 1 stage the ground-truth / hypothesis rows in LDS; the whole workgroup
//         fills sim[64][65] (fp64; the odd row pitch keeps the serial row sums off one LDS bank); lane i of wave 0 adds row i in
//         ascending j and counts gtc[g_i], lane j of wave 1 adds column j in ascending i and counts hyc[h_j]; the whole
//         workgroup adds sim / ((row + col) - sim) into the sequence's pmc[G][H] in global memory: ids are unique inside a
//         frame, so a cell has one writer per frame, and a sequence's matrix is touched by its own workgroup only -- no atomics;
//      the sweep: pmc -> gas in place, 256 cells at a time, behind a workgroup barrier and fence (nothing device-wide);
//      pass 2, matching, frame after frame: the whole workgroup fills score = gas[g_i][h_j] * sim into the same LDS tile (a
//         gather from the sequence's gas per cell; sim is not kept), wave 0 runs wave_assign of motassign.h on it -- the
//         arithmetic and tie rule of fp_mot_match -- and lane i of wave 0 owns ground-truth row i: gt_match, gt_sim (the IoU of
//         the matched pair, computed again from the staged boxes: the same operations, the same bits) and the number t of alphas
//         it reaches; levels[t] sits on lane t and is bumped one match after the other.
//    No scratch, no global atomics, no host synchronisation between the passes: two runs are bit-identical.  A single long
//    sequence is two chains of dependent frames on one workgroup: latency-bound by construction.
// 2. fp_hota_match_emulate: the same __host__ __device__ decision code serially on host memory, the assignment in its textbook
//    form (host_assign of motassign.h).
#include <math.h>

#include <vector>

#include "common.h"
#include "motassign.h"

namespace {

using namespace motassign;
constexpr int TPB = 256;
constexpr int MAXA = FP_HOTA_MAX_ALPHAS;
constexpr int LD = MR + 1;   // row pitch of the LDS tile
static_assert(MAXA + 1 <= FP_WAVE, "levels[t] sits on lane t of wave 0");

struct HotaArgs {
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
  const int* hy_id_base;   // [S + 1]
  const long* pot_base;    // [S + 1]
  int S, A;
  long n_frames, n_gt_ids, n_hy_ids, n_pot;
  double alphas[MAXA];
  int* gt_match;           // [n_gt]
  double* gt_sim;          // [n_gt]
  long* levels;            // [S][A + 1]
  long* counts;            // [S][2] n_gt n_hy
  double* gas;             // [n_pot]: pmc during pass 1
  int* gtc;                // [n_gt_ids]
  int* hyc;                // [n_hy_ids]
};

// ---------------------------------------------------------------------------------------- the decision code, host and device
// the share of sim in what its row and its column hold together; sim > 0
__host__ __device__ __forceinline__ double hota_soft(double sim, double row, double col) { return sim / ((row + col) - sim); }

// the global alignment score of an id pair from its summed shares and the frames either id occurs in
__host__ __device__ __forceinline__ double hota_gas(double pmc, int gtc, int hyc) {
  return pmc > 0.0 ? pmc / (((double)gtc + (double)hyc) - pmc) : 0.0;
}

// the number of alphas (ascending) that sim reaches
__host__ __device__ __forceinline__ int hota_level(double sim, const double* alphas, int A) {
  int t = 0;
  for (int a = 0; a < A; ++a) t += sim >= alphas[a] ? 1 : 0;
  return t;
}

// The sequence's slice of the arrays; every index derived from device data is clamped into the arrays.
struct HotaSeq {
  long f0, f1, gid0, hid0, pot0;
  int G, H;
};
__host__ __device__ __forceinline__ HotaSeq hota_seq(const HotaArgs& p, int s) {
  HotaSeq q;
  q.f0 = mot_clamp(p.frame_base[s], 0, p.n_frames);
  q.f1 = mot_clamp(p.frame_base[s + 1], q.f0, p.n_frames);
  q.gid0 = mot_clamp(p.gt_id_base[s], 0, p.n_gt_ids);
  q.G = (int)(mot_clamp(p.gt_id_base[s + 1], q.gid0, p.n_gt_ids) - q.gid0);
  q.hid0 = mot_clamp(p.hy_id_base[s], 0, p.n_hy_ids);
  int H = (int)(mot_clamp(p.hy_id_base[s + 1], q.hid0, p.n_hy_ids) - q.hid0);
  q.pot0 = mot_clamp(p.pot_base[s], 0, p.n_pot);
  const long cells = mot_clamp(p.pot_base[s + 1], q.pot0, p.n_pot) - q.pot0;
  if ((long)q.G * (long)H > cells) H = q.G > 0 ? (int)(cells / q.G) : 0;
  q.H = H;
  return q;
}

// ------------------------------------------------------------------------------------------------------------- the kernel
__global__ __launch_bounds__(TPB) void hota_match_kernel(HotaArgs p) {
  __shared__ double s_t[MR * LD];                      // pass 1: sim; pass 2: score
  __shared__ double s_gb[MR * 4], s_hb[MR * 4], s_row[MR], s_col[MR], s_alpha[MAXA];
  __shared__ int s_gid[MR], s_hid[MR];

  const int tid = threadIdx.x, lane = tid & (FP_WAVE - 1), wave = tid >> 6;
  const int s = blockIdx.x;
  const HotaSeq q = hota_seq(p, s);
  const int G = q.G, H = q.H;
  const int A = (int)mot_clamp(p.A, 0, MAXA);
  double* gas = p.gas + q.pot0;
  int* gtc = p.gtc + q.gid0;
  int* hyc = p.hyc + q.hid0;
  if (tid < A) s_alpha[tid] = p.alphas[tid];

  // waves 0 / 1 stage the frame's rows
  auto stage = [&](const MotFrame& fr) {
    if (wave == 0 && lane < fr.n) {
      const double* b = p.gt_box + 4 * (fr.g0 + lane);
      for (int k = 0; k < 4; ++k) s_gb[4 * lane + k] = b[k];
      s_gid[lane] = (int)mot_clamp(p.gt_id[fr.g0 + lane], 0, G - 1);
    }
    if (wave == 1 && lane < fr.m) {
      const double* b = p.hy_box + 4 * (fr.h0 + lane);
      for (int k = 0; k < 4; ++k) s_hb[4 * lane + k] = b[k];
      s_hid[lane] = (int)mot_clamp(p.hy_id[fr.h0 + lane], 0, H - 1);
    }
  };

  // ---- pass 1, alignment
  for (long gf = q.f0; gf < q.f1; ++gf) {
    const MotFrame fr = mot_frame(p, gf, G, H);
    const int n = fr.n, m = fr.m;
    stage(fr);
    __syncthreads();
    for (int idx = tid; idx < n * m; idx += TPB) {
      const int i = idx / m, j = idx - i * m;
      s_t[i * LD + j] = mot_iou(s_gb + 4 * i, s_hb + 4 * j);
    }
    __syncthreads();
    if (wave == 0 && lane < n) {                         // row sums in ascending j; the frames the id occurs in
      double r = 0.0;
      for (int j = 0; j < m; ++j) r += s_t[lane * LD + j];
      s_row[lane] = r;
      gtc[s_gid[lane]] += 1;
    }
    if (wave == 1 && lane < m) {                         // column sums in ascending i
      double c = 0.0;
      for (int i = 0; i < n; ++i) c += s_t[i * LD + lane];
      s_col[lane] = c;
      hyc[s_hid[lane]] += 1;
    }
    __syncthreads();
    for (int idx = tid; idx < n * m; idx += TPB) {
      const int i = idx / m, j = idx - i * m;
      const double sim = s_t[i * LD + j];
      if (sim > 0.0) gas[(long)s_gid[i] * H + s_hid[j]] += hota_soft(sim, s_row[i], s_col[j]);
    }
    __syncthreads();   // pmc, gtc and hyc of this frame are behind a workgroup barrier before the next frame adds to them
  }

  // ---- the sweep: pmc -> gas in place; the sequence's own workgroup wrote every cell it reads here and below
  __threadfence_block();
  __syncthreads();
  for (long c = tid; c < (long)G * (long)H; c += TPB) {
    const int g = (int)(c / H), h = (int)(c - (long)g * H);
    gas[c] = hota_gas(gas[c], gtc[g], hyc[h]);
  }
  __threadfence_block();
  __syncthreads();

  // ---- pass 2, matching
  long n_gt = 0, n_hy = 0, lev = 0;                      // lev: levels[lane], in wave 0
  for (long gf = q.f0; gf < q.f1; ++gf) {
    const MotFrame fr = mot_frame(p, gf, G, H);
    const int n = fr.n, m = fr.m;
    stage(fr);
    __syncthreads();
    for (int idx = tid; idx < n * m; idx += TPB) {
      const int i = idx / m, j = idx - i * m;
      s_t[i * LD + j] = gas[(long)s_gid[i] * H + s_hid[j]] * mot_iou(s_gb + 4 * i, s_hb + 4 * j);
    }
    __syncthreads();
    if (wave == 0) {
      const int N = n > m ? n : m;
      const int p_row = wave_assign(n, m, lane, [&](int i0, double ui0, double v) {
        const double sc = (i0 < n && lane < m) ? s_t[i0 * LD + lane] : 0.0;
        return mot_reduced(sc, ui0, v);
      });
      const int col = wave_column_of_row(p_row, N, lane);   // lane = ground-truth row
      bool matched = false;
      double sv = 0.0;
      int t = 0;
      if (lane < n && col >= 0 && col < m && s_t[lane * LD + col] > 0.0) {
        matched = true;
        sv = mot_iou(s_gb + 4 * lane, s_hb + 4 * col);
        t = hota_level(sv, s_alpha, A);
      }
      if (lane < n) {
        p.gt_match[fr.g0 + lane] = matched ? (int)(fr.h0 + col) : -1;
        p.gt_sim[fr.g0 + lane] = sv;
      }
      for (unsigned long long b = __ballot(matched); b; b &= b - 1) {
        const int tb = lane_i(t, __ffsll((long long)b) - 1);
        if (lane == tb) lev += 1;
      }
      n_gt += n;
      n_hy += m;
    }
    __syncthreads();   // the tile and the staged rows are read to the end before the next frame overwrites them
  }
  if (wave == 0 && lane <= A) p.levels[(long)s * (A + 1) + lane] = lev;
  if (tid == 0) {
    long* c = p.counts + 2 * (long)s;
    c[0] = n_gt, c[1] = n_hy;
  }
}

// --------------------------------------------------------------------------------------------------------------- the host
size_t hota_ws_bytes(int64_t n_gt_ids, int64_t n_hy_ids, int64_t n_pot) {
  if (n_gt_ids < 0 || n_hy_ids < 0 || n_pot < 0) return 0;
  const int64_t bytes = n_pot * (int64_t)sizeof(double) + (n_gt_ids + n_hy_ids) * (int64_t)sizeof(int32_t);
  return (size_t)(bytes > 0 ? bytes : 8);
}

// alphas: HOST memory; refused here unless strictly ascending inside (0, 1]
int hota_args(HotaArgs& a, const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt, const double* hy_boxes,
              const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy, const int32_t* frame_base, const int32_t* gt_id_base,
              const int32_t* hy_id_base, const int64_t* pot_base, int n_seqs, int64_t n_frames, int64_t n_gt_ids, int64_t n_hy_ids,
              int64_t n_pot, const double* alphas, int n_alphas, int32_t* gt_match, double* gt_sim, int64_t* levels,
              int64_t* counts, void* workspace, size_t ws_bytes) {
  if (n_seqs < 0 || n_gt < 0 || n_hy < 0 || n_frames < 0 || n_gt_ids < 0 || n_hy_ids < 0 || n_pot < 0) return FP_ERR_INVALID_ARG;
  if (n_gt >= (1L << 31) || n_hy >= (1L << 31) || n_frames >= (1L << 31) - 2 || n_gt_ids >= (1L << 31) || n_hy_ids >= (1L << 31))
    return FP_ERR_INVALID_ARG;                              // int32 CSR offsets and ids
  if (!alphas || n_alphas < 1 || n_alphas > MAXA) return FP_ERR_INVALID_ARG;
  for (int k = 0; k < n_alphas; ++k)
    if (!(alphas[k] > 0.0 && alphas[k] <= 1.0) || (k > 0 && !(alphas[k] > alphas[k - 1]))) return FP_ERR_INVALID_ARG;
  if (!gt_off || !hy_off || !frame_base || !gt_id_base || !hy_id_base || !pot_base || !workspace) return FP_ERR_INVALID_ARG;
  if (n_seqs > 0 && (!levels || !counts)) return FP_ERR_INVALID_ARG;
  if (n_gt > 0 && (!gt_boxes || !gt_id || !gt_match || !gt_sim)) return FP_ERR_INVALID_ARG;
  if (n_hy > 0 && (!hy_boxes || !hy_id)) return FP_ERR_INVALID_ARG;
  if (ws_bytes < hota_ws_bytes(n_gt_ids, n_hy_ids, n_pot)) return FP_ERR_INVALID_ARG;
  if (((uintptr_t)gt_boxes | (uintptr_t)hy_boxes | (uintptr_t)pot_base | (uintptr_t)levels | (uintptr_t)counts | (uintptr_t)gt_sim |
       (uintptr_t)workspace) % 8 ||
      ((uintptr_t)gt_id | (uintptr_t)hy_id | (uintptr_t)gt_off | (uintptr_t)hy_off | (uintptr_t)frame_base | (uintptr_t)gt_id_base |
       (uintptr_t)hy_id_base | (uintptr_t)gt_match) % 4)
    return FP_ERR_ALIGNMENT;
  a.gt_box = gt_boxes; a.gt_id = gt_id; a.gt_off = gt_off; a.n_gt = (long)n_gt;
  a.hy_box = hy_boxes; a.hy_id = hy_id; a.hy_off = hy_off; a.n_hy = (long)n_hy;
  a.frame_base = frame_base; a.gt_id_base = gt_id_base; a.hy_id_base = hy_id_base; a.pot_base = (const long*)pot_base;
  a.S = n_seqs; a.A = n_alphas;
  a.n_frames = (long)n_frames; a.n_gt_ids = (long)n_gt_ids; a.n_hy_ids = (long)n_hy_ids; a.n_pot = (long)n_pot;
  for (int k = 0; k < MAXA; ++k) a.alphas[k] = k < n_alphas ? alphas[k] : 2.0;
  a.gt_match = gt_match; a.gt_sim = gt_sim; a.levels = (long*)levels; a.counts = (long*)counts;
  a.gas = (double*)workspace;
  a.gtc = (int*)(a.gas + n_pot);
  a.hyc = a.gtc + n_gt_ids;
  return FP_OK;
}

// One sequence on host memory: the written procedure with the assignment in its textbook form.
void emulate_seq(const HotaArgs& p, int s) {
  const HotaSeq q = hota_seq(p, s);
  const int G = q.G, H = q.H, A = p.A;
  double* gas = p.gas + q.pot0;
  int* gtc = p.gtc + q.gid0;
  int* hyc = p.hyc + q.hid0;
  std::vector<double> t(MR * MR), row(MR), col(MR);
  std::vector<int> gid(MR), hid(MR);
  HostAssign as;
  auto stage = [&](const MotFrame& fr) {
    for (int i = 0; i < fr.n; ++i) gid[i] = (int)mot_clamp(p.gt_id[fr.g0 + i], 0, G - 1);
    for (int j = 0; j < fr.m; ++j) hid[j] = (int)mot_clamp(p.hy_id[fr.h0 + j], 0, H - 1);
  };
  for (long gf = q.f0; gf < q.f1; ++gf) {
    const MotFrame fr = mot_frame(p, gf, G, H);
    const int n = fr.n, m = fr.m;
    stage(fr);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < m; ++j) t[i * MR + j] = mot_iou(p.gt_box + 4 * (fr.g0 + i), p.hy_box + 4 * (fr.h0 + j));
    for (int i = 0; i < n; ++i) {
      double r = 0.0;
      for (int j = 0; j < m; ++j) r += t[i * MR + j];
      row[i] = r;
      gtc[gid[i]] += 1;
    }
    for (int j = 0; j < m; ++j) {
      double c = 0.0;
      for (int i = 0; i < n; ++i) c += t[i * MR + j];
      col[j] = c;
      hyc[hid[j]] += 1;
    }
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < m; ++j)
        if (t[i * MR + j] > 0.0) gas[(long)gid[i] * H + hid[j]] += hota_soft(t[i * MR + j], row[i], col[j]);
  }
  for (long c = 0; c < (long)G * (long)H; ++c) gas[c] = hota_gas(gas[c], gtc[c / H], hyc[c % H]);
  long n_gt = 0, n_hy = 0;
  long* lev = p.levels + (long)s * (A + 1);
  for (int k = 0; k <= A; ++k) lev[k] = 0;
  for (long gf = q.f0; gf < q.f1; ++gf) {
    const MotFrame fr = mot_frame(p, gf, G, H);
    const int n = fr.n, m = fr.m, N = n > m ? n : m;
    stage(fr);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < m; ++j)
        t[i * MR + j] = gas[(long)gid[i] * H + hid[j]] * mot_iou(p.gt_box + 4 * (fr.g0 + i), p.hy_box + 4 * (fr.h0 + j));
    auto score = [&](int i, int j) { return (i < n && j < m) ? t[i * MR + j] : 0.0; };
    host_assign(n, m, score, as);
    for (int i = 0; i < n; ++i) {
      const int c = host_column_of_row(as, N, i);
      const bool matched = c >= 0 && c < m && score(i, c) > 0.0;
      const double sv = matched ? mot_iou(p.gt_box + 4 * (fr.g0 + i), p.hy_box + 4 * (fr.h0 + c)) : 0.0;
      if (matched) lev[hota_level(sv, p.alphas, A)] += 1;
      p.gt_match[fr.g0 + i] = matched ? (int)(fr.h0 + c) : -1;
      p.gt_sim[fr.g0 + i] = sv;
    }
    n_gt += n;
    n_hy += m;
  }
  p.counts[2 * (long)s] = n_gt;
  p.counts[2 * (long)s + 1] = n_hy;
}

}  // namespace

extern "C" {

size_t fp_hota_match_workspace(int64_t n_gt_ids, int64_t n_hy_ids, int64_t n_pot) { return hota_ws_bytes(n_gt_ids, n_hy_ids, n_pot); }

int fp_hota_match(const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt, const double* hy_boxes,
                  const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy, const int32_t* frame_base,
                  const int32_t* gt_id_base, const int32_t* hy_id_base, const int64_t* pot_base, int n_seqs, int64_t n_frames,
                  int64_t n_gt_ids, int64_t n_hy_ids, int64_t n_pot, const double* alphas, int n_alphas, int32_t* gt_match,
                  double* gt_sim, int64_t* levels, int64_t* counts, void* workspace, size_t ws_bytes, void* stream) {
  HotaArgs a;
  const int rc = hota_args(a, gt_boxes, gt_id, gt_off, n_gt, hy_boxes, hy_id, hy_off, n_hy, frame_base, gt_id_base, hy_id_base,
                           pot_base, n_seqs, n_frames, n_gt_ids, n_hy_ids, n_pot, alphas, n_alphas, gt_match, gt_sim, levels,
                           counts, workspace, ws_bytes);
  if (rc != FP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, hota_ws_bytes(n_gt_ids, n_hy_ids, n_pot), s) != hipSuccess ||
      (n_gt > 0 && (hipMemsetAsync(gt_match, 0xFF, (size_t)n_gt * sizeof(int32_t), s) != hipSuccess ||
                    hipMemsetAsync(gt_sim, 0, (size_t)n_gt * sizeof(double), s) != hipSuccess))) {
    fp_set_hip_error(hipGetLastError());
    return FP_ERR_LAUNCH;
  }
  if (n_seqs == 0) return FP_OK;
  hipLaunchKernelGGL(hota_match_kernel, dim3((unsigned)n_seqs), dim3(TPB), 0, s, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_hota_match_emulate(const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt,
                          const double* hy_boxes, const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy,
                          const int32_t* frame_base, const int32_t* gt_id_base, const int32_t* hy_id_base,
                          const int64_t* pot_base, int n_seqs, int64_t n_frames, int64_t n_gt_ids, int64_t n_hy_ids,
                          int64_t n_pot, const double* alphas, int n_alphas, int32_t* gt_match, double* gt_sim, int64_t* levels,
                          int64_t* counts, void* workspace, size_t ws_bytes) {
  HotaArgs a;
  const int rc = hota_args(a, gt_boxes, gt_id, gt_off, n_gt, hy_boxes, hy_id, hy_off, n_hy, frame_base, gt_id_base, hy_id_base,
                           pot_base, n_seqs, n_frames, n_gt_ids, n_hy_ids, n_pot, alphas, n_alphas, gt_match, gt_sim, levels,
                           counts, workspace, ws_bytes);
  if (rc != FP_OK) return rc;
  const size_t ws = hota_ws_bytes(n_gt_ids, n_hy_ids, n_pot);
  for (size_t i = 0; i < ws; ++i) ((unsigned char*)workspace)[i] = 0;
  for (int64_t i = 0; i < n_gt; ++i) gt_match[i] = -1, gt_sim[i] = 0.0;
  for (int s = 0; s < n_seqs; ++s) emulate_seq(a, s);
  return FP_OK;
}

}  // extern "C"
