// motassign.h — what the tracker-evaluation kernels share (moteval.hip: CLEAR-MOT / IDF1; hota.hip: HOTA): the fp64 IoU, the
// reduced cost, the clamp of indices read from device memory, the CSR slice of a frame, and the assignment of DESIGN §7 in its
// two forms -- on one wave with COLUMNS ON LANES (the kernels) and as the textbook loops (the host emulators).  Both forms take
// the reduced cost as a functor, so a kernel decides what a score is (sim, threshold and continuity bonus; or the alignment
// score times sim) and the arithmetic and the tie rule of the assignment stay in one place.  Build the including file with
// -ffp-contract=off.
#pragma once
#include <math.h>

#include "common.h"

namespace motassign {

constexpr int MR = FP_MOT_MAX_ROWS;
static_assert(MR == FP_WAVE, "one column of the assignment per lane; one 64-bit ballot of matched rows");

// ---------------------------------------------------------------------------------------- the decision code, host and device
// xywh boxes, the operations of evaluation._iou_matrix in its order
__host__ __device__ __forceinline__ double mot_iou(const double* a, const double* b) {
  const double iw = fmin(a[0] + a[2], b[0] + b[2]) - fmax(a[0], b[0]);
  const double ih = fmin(a[1] + a[3], b[1] + b[3]) - fmax(a[1], b[1]);
  if (iw <= 0.0 || ih <= 0.0) return 0.0;
  const double i = iw * ih;
  const double u = a[2] * a[3] + b[2] * b[3] - i;
  return i / u;
}

// C[i0][j] - u[i0] - v[j] with C = -score
__host__ __device__ __forceinline__ double mot_reduced(double score, double u, double v) { return (-score - u) - v; }

__host__ __device__ __forceinline__ long mot_clamp(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The rows of one frame: CSR offsets kept inside the arrays, at most MR rows taken (the caller refuses longer frames).
struct MotFrame {
  long g0, h0;
  int n, m;
};
template <class Args>
__host__ __device__ __forceinline__ MotFrame mot_frame(const Args& p, long gf, int G, int H) {
  MotFrame fr;
  fr.g0 = mot_clamp(p.gt_off[gf], 0, p.n_gt);
  fr.h0 = mot_clamp(p.hy_off[gf], 0, p.n_hy);
  const long g1 = mot_clamp(p.gt_off[gf + 1], fr.g0, p.n_gt), h1 = mot_clamp(p.hy_off[gf + 1], fr.h0, p.n_hy);
  fr.n = G > 0 ? (int)mot_clamp(g1 - fr.g0, 0, MR) : 0;
  fr.m = H > 0 ? (int)mot_clamp(h1 - fr.h0, 0, MR) : 0;
  return fr;
}

// ------------------------------------------------------------------------------------------------ the assignment on one wave
#if defined(__HIPCC__)
// Wave-uniform lane indices: v_readlane instead of a shuffle through LDS.
__device__ __forceinline__ int lane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ double lane_d(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// The minimum of a wave's values (no NaN among them), in every lane: quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror and
// row_mirror give every lane the minimum of its row of 16, the four rows meet through readlanes.
__device__ __forceinline__ double wave_min(double v) {
  v = fmin(v, dpp_d<0xB1>(v));
  v = fmin(v, dpp_d<0x4E>(v));
  v = fmin(v, dpp_d<0x141>(v));
  v = fmin(v, dpp_d<0x140>(v));
  return fmin(fmin(lane_d(v, 0), lane_d(v, 16)), fmin(lane_d(v, 32), lane_d(v, 48)));
}

// One whole wave runs the shortest-augmenting-path assignment of an n x m score matrix padded with zeros to N x N,
// N = max(n, m): lane = column - 1 holds v, minv, way, used and the column's row; lane = row - 1 holds u and rowin.  The scan of
// a step is one call of reduced(i0 - 1, u[i0], v) per lane -- (C[i0][lane] - u) - v of this lane's column, 0 scores outside
// n x m -- and delta / j1 come from a wave arg-min over (value, lane), lower lane on equal values (wave_min, then the lowest
// lane of the ballot of the lanes that hold it): the ascending scan with strict comparisons of the written procedure.
// -> in lane j: the row (1-based) assigned to column j + 1, 0 for none.
template <class Reduced>
__device__ __forceinline__ int wave_assign(int n, int m, int lane, Reduced reduced) {
  const double INF = __builtin_huge_val();
  const int N = n > m ? n : m;
  int p_row = 0;
  double u = 0.0, v = 0.0;
  if (n > 0 && m > 0) {
    for (int i = 1; i <= N; ++i) {
      double minv = INF;
      int way = 0, j0 = 0;
      bool used = false, rowin = false, found = false;
      for (int it = 0; it <= N; ++it) {                 // a step marks one more column used: N steps at most
        if (lane == j0 - 1) used = true;
        const int i0 = j0 == 0 ? i : lane_i(p_row, j0 - 1);
        if (lane == i0 - 1) rowin = true;
        const double ui0 = lane_d(u, i0 - 1);
        const bool open = lane < N && !used;
        if (open) {
          const double cur = reduced(i0 - 1, ui0, v);
          if (cur < minv) minv = cur, way = j0;
        }
        const double bv = open ? minv : INF;
        const double mn = wave_min(bv);
        if (!(mn < INF)) break;                         // no open column: cannot happen with finite scores
        const int bl = __ffsll((long long)__ballot(bv == mn)) - 1;   // the lowest lane that holds the minimum
        if (bl < 0) break;
        const double delta = lane_d(bv, bl);
        if (rowin) u += delta;
        if (used) v -= delta;
        else minv -= delta;
        j0 = bl + 1;
        if (lane_i(p_row, bl) == 0) {
          found = true;
          break;
        }
      }
      if (!found) break;
      for (int it = 0; it <= N && j0 != 0; ++it) {      // augment along way
        const int j1 = lane_i(way, j0 - 1);
        const int pn = j1 == 0 ? i : lane_i(p_row, j1 - 1);
        if (lane == j0 - 1) p_row = pn;
        j0 = j1;
      }
    }
  }
  return p_row;
}

// lane = ground-truth row: the column (0-based) wave_assign gave it, -1 for none
__device__ __forceinline__ int wave_column_of_row(int p_row, int N, int lane) {
  int col = -1;
  for (int c = 0; c < N; ++c) {
    const int pr = lane_i(p_row, c);
    if (pr == lane + 1) col = c;
  }
  return col;
}
#endif  // __HIPCC__

// ------------------------------------------------------------------------------------------- the assignment, textbook form
// The written procedure on host memory.  score(i, j): the score of row i, column j, 0-based, 0 outside n x m.  The arrays hold
// MR + 1 entries.  -> prow[j]: the row (1-based) assigned to column j (1-based), 0 for none.
struct HostAssign {
  double u[MR + 1], v[MR + 1], minv[MR + 1];
  int prow[MR + 1], way[MR + 1];
  char used[MR + 1];
};
template <class Score>
inline void host_assign(int n, int m, Score score, HostAssign& a) {
  const double INF = __builtin_huge_val();
  const int N = n > m ? n : m;
  for (int j = 0; j <= N; ++j) a.u[j] = a.v[j] = 0.0, a.prow[j] = 0, a.way[j] = 0;
  if (n <= 0 || m <= 0) return;
  for (int i = 1; i <= N; ++i) {
    a.prow[0] = i;
    int j0 = 0;
    for (int j = 0; j <= N; ++j) a.minv[j] = INF, a.used[j] = 0;
    do {
      a.used[j0] = 1;
      const int i0 = a.prow[j0];
      double delta = INF;
      int j1 = 0;
      for (int j = 1; j <= N; ++j) {
        if (a.used[j]) continue;
        const double cur = mot_reduced(score(i0 - 1, j - 1), a.u[i0], a.v[j]);
        if (cur < a.minv[j]) a.minv[j] = cur, a.way[j] = j0;
        if (a.minv[j] < delta) delta = a.minv[j], j1 = j;
      }
      for (int j = 0; j <= N; ++j) {
        if (a.used[j]) a.u[a.prow[j]] += delta, a.v[j] -= delta;
        else a.minv[j] -= delta;
      }
      j0 = j1;                                          // 0: no open column, cannot happen with finite scores
    } while (j0 != 0 && a.prow[j0] != 0);
    do {
      const int j1 = a.way[j0];
      a.prow[j0] = a.prow[j1];
      j0 = j1;
    } while (j0);
  }
}
// the column (0-based) of row i (0-based), -1 for none
inline int host_column_of_row(const HostAssign& a, int N, int i) {
  int col = -1;
  for (int j = 1; j <= N; ++j)
    if (a.prow[j] == i + 1) col = j - 1;
  return col;
}

}  // namespace motassign
