// tracklets.hip — batched face tracking across the frames of many streams (gfx950).  Build-defined, no reference counterpart
// (DESIGN §7 "Tracklets"; include/facepath.h states the procedure; tracker.hip stays the port of the reference's per-frame
// first-match rule).  Build with -ffp-contract=off: the IoU gate and the cosine are the same bits on device and host emulator.
//
// One kernel, tracklets_kernel<MOTION, REID>, one host twin, emulate_step, and one argument struct, TrackArgs, whose motion and
// pool pointers are null where the caller has neither.  The six fp_tracklets_step* entry points build the arguments and hand
// them to run(), which checks them (before any HIP call), then launches the instantiation the arguments name or calls the twin.
//
// The kernel: ONE launch, one workgroup per stream; a workgroup whose stream owns no frame of the step leaves after the first
// pass.  That pass reads frame[] once: the min / max frame index of every chunk of rows goes to LDS (so a frame's rows are later
// looked for only in the chunks that can hold them: one or two when the rows come in frame order, all of them at worst), and
// the rows nobody tracks get their NO_STREAM outputs from the workgroup that owns their chunk.  Then the workgroup marches over
// its frames in ascending batch index with the stream's slot table in LDS:
//   1.  expiry.  REID: every wave finds the expiring slots by a ballot of its own, wave 0 moves their rows into the pool's ring
//       (the stream's FP_TRACK_LOST parked tracks, ints and floats in LDS, embeddings in global memory), everybody copies their
//       embeddings.  1b, MOTION: the slot's four constant-velocity filters and the predicted boxes sit in LDS beside the slot
//       table; one (slot, coordinate) per thread on the first 256 threads.
//   2.  the frame's rows by ballot compaction in row order.
//   3.  live tracks x live detections, one pair per 16 lanes (tk_dot16: float4 loads, xor-shuffle sum; IoU with the predicted
//       box under MOTION) -> 64-bit keys in LDS (~ord(c) << 32 | slot << 8 | position: ascending = c descending, lower slot,
//       lower row) -> tk_sort (bitonic) -> tk_walk: wave 0 takes the keys 64 at a time with a ballot per taken pair.
//       (<true, false> alone carries the text of the two written out, for a measured 0.9 %: WRITTEN_OUT in the kernel.)
//   3b. REID, only in a frame that has parked tracks and unmatched detections: those x those through the same tk_dot16, key[],
//       tk_sort and tk_walk, the cosine alone deciding.  An empty pool costs one workgroup-uniform test.
//   4,5 the unmatched detections open tracks in the lowest free slots by rank (or continue the parked track they took) -> slot
//       fields in LDS, filters updated / opened by wave 0, embeddings copied in global memory by the whole workgroup.
// No global atomics, no scratch, no host synchronisation: two runs are bit-identical.  What an instantiation does not use is
// not compiled into it: <false, *> reads no motion array, <*, false> nothing of the pool.
//
// The twin runs the same __host__ __device__ decision code (liveness, dot product in the device's order, IoU, admissibility,
// key, filters, slot rewrite) serially on host memory, std::sort for the keys (the order is total).
#include <limits.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int SLOTS = FP_TRACK_SLOTS, MAXD = FP_TRACK_MAX_DETS, LOST = FP_TRACK_LOST;
constexpr int TPB = 512, NW = TPB / FP_WAVE;
constexpr int GL = 16, NG = TPB / GL;   // lanes per pair, pairs in flight
constexpr int MAXCH = 1024;             // row chunks whose frame range is kept in LDS
constexpr int NI = FP_TRACK_SLOT_INTS, NF = FP_TRACK_SLOT_FLOATS, MF = FP_TRACK_MOTION_FLOATS;
constexpr unsigned long long KEY_NONE = ~0ull;
static_assert(SLOTS == 64 && MAXD == 64, "one 64-bit mask of tracks and one of detections; slot and position are key bytes");
static_assert(LOST == 64, "one 64-bit mask of parked tracks, one lane of a wave each; the entry is a key byte");

// slot_i columns / slot_f columns
enum { I_ID = 0, I_FIRST = 1, I_LAST = 2, I_HITS = 3, I_BEST_CLOCK = 4 };
enum { F_BOX = 0, F_INV = 4, F_BEST_SCORE = 5, F_BEST_BOX = 6 };
// motion columns of one coordinate c of (cx, cy, w, h): motion[slot][c * MC + ...]
enum { M_X = 0, M_V = 1, M_P00 = 2, M_P01 = 3, M_P11 = 4, MC = 5 };
static_assert(MF == 4 * MC, "four two-state filters per slot");

struct TrackArgs {
  int* hdr;      // [S][2] clock, next_id
  int* si;       // [S][SLOTS][NI]
  float* sf;     // [S][SLOTS][NF]
  float* semb;   // [S][SLOTS][D]
  float* sbest;  // [S][SLOTS][D]
  int S, D;
  const int* frame;
  const float* box;
  const float* emb;
  const float* xinv;
  const float* score;   // may be null
  int n;
  const int* sof;
  int B;
  int max_age;
  float tau_near, tau_far, iou_min;
  int* o_id;
  int* o_hits;
  int* o_clock;
  int* o_flags;
  float* motion;        // [S][SLOTS][MF]; null without motion prediction
  float std_pos, std_vel;
  float* o_pred;        // [n][4]
  int* lhdr;            // [S][2] ring head, spare; the five pool arrays are null without re-identification
  int* li;              // [S][LOST][NI]
  float* lf;            // [S][LOST][NF]
  float* lemb;          // [S][LOST][D]
  float* lbest;         // [S][LOST][D]
  float tau_reid;
  int lost_age;
};

// ---------------------------------------------------------------------------------------- the decision code, host and device
__host__ __device__ __forceinline__ bool tk_live(float inv) { return inv > 0.f && inv - inv == 0.f; }

__host__ __device__ __forceinline__ bool tk_untracked(const TrackArgs& p, int f) {
  if (f < 0 || f >= p.B) return true;
  const int s = p.sof[f];
  return s < 0 || s >= p.S;
}

// lane gl of 16: the products of float4 gl, gl + 16, ... added in index order
__host__ __device__ __forceinline__ float tk_partial(const float* t, const float* d, int D, int gl) {
  float acc = 0.f;
  for (int k = gl * 4; k < D; k += GL * 4) {
    acc += t[k] * d[k];
    acc += t[k + 1] * d[k + 1];
    acc += t[k + 2] * d[k + 2];
    acc += t[k + 3] * d[k + 3];
  }
  return acc;
}

__host__ __device__ __forceinline__ float tk_cos(float dot, float inv_t, float inv_d) { return (dot * inv_t) * inv_d; }

// t: the track's last box, d: the detection's; min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b with a the track's value
__host__ __device__ __forceinline__ float tk_iou(const float* t, const float* d) {
  const float ix1 = t[0] > d[0] ? t[0] : d[0], iy1 = t[1] > d[1] ? t[1] : d[1];
  const float ix2 = t[2] < d[2] ? t[2] : d[2], iy2 = t[3] < d[3] ? t[3] : d[3];
  const float iw = ix2 - ix1, ih = iy2 - iy1;
  if (!(iw > 0.f && ih > 0.f)) return 0.f;
  const float inter = iw * ih;
  const float area_t = (t[2] - t[0]) * (t[3] - t[1]), area_d = (d[2] - d[0]) * (d[3] - d[1]);
  return inter / ((area_t + area_d) - inter);
}

__host__ __device__ __forceinline__ bool tk_admissible(const TrackArgs& p, float c, float iou) {
  return (c > p.tau_near && iou > p.iou_min) || c > p.tau_far;
}

// ascending keys = c descending (-0 counts as +0), then slot ascending, then position in the frame ascending
__host__ __device__ __forceinline__ unsigned long long tk_key(float c, int slot, int pos) {
  if (c == 0.f) c = 0.f;
  unsigned u;
  __builtin_memcpy(&u, &c, 4);
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)(~ord) << 32) | (unsigned)(slot << 8 | pos);
}
__host__ __device__ __forceinline__ int tk_key_slot(unsigned long long k) { return (int)((unsigned)k >> 8) & 0xFF; }
__host__ __device__ __forceinline__ int tk_key_pos(unsigned long long k) { return (int)((unsigned)k & 0xFF); }

__host__ __device__ __forceinline__ void tk_out(const TrackArgs& p, long row, int id, int hits, int clock, int flags) {
  p.o_id[row] = id;
  p.o_hits[row] = hits;
  p.o_clock[row] = clock;
  p.o_flags[row] = flags;
}

// rows of one chunk; TPB * MAXCH chunks of TPB rows cover 2^19 rows, more rows make the chunks longer
__host__ __device__ __forceinline__ int tk_chunk_rows(int n) { return TPB * (int)(((long)n + (long)TPB * MAXCH - 1) / ((long)TPB * MAXCH)); }

// A matched (is_new false) or opened detection rewrites its slot: ints and floats of the slot table (LDS on the device).
// Returns the row's flags.
__host__ __device__ __forceinline__ int tk_update_slot(const TrackArgs& p, int* si, float* sf, long row, float inv, bool is_new,
                                                       int clock, int new_id) {
  const float* b = p.box + row * 4;
  const float sc = p.score ? p.score[row] : 0.f;
  if (is_new) {
    si[I_ID] = new_id;
    si[I_FIRST] = clock;
    si[I_HITS] = 1;
  } else {
    si[I_HITS] += 1;
  }
  si[I_LAST] = clock;
  for (int k = 0; k < 4; ++k) sf[F_BOX + k] = b[k];
  sf[F_INV] = inv;
  int flags = is_new ? FP_TRACK_NEW : 0;
  if (is_new || sc > sf[F_BEST_SCORE]) {
    sf[F_BEST_SCORE] = sc;
    si[I_BEST_CLOCK] = clock;
    for (int k = 0; k < 4; ++k) sf[F_BEST_BOX + k] = b[k];
    flags |= FP_TRACK_BEST;
  }
  return flags;
}

// -------------------------------------------------------------------------- motion prediction, host and device (fp32, no contraction)
__host__ __device__ __forceinline__ float tk_hs(float t) { return t > 1.f ? t : 1.f; }
__host__ __device__ __forceinline__ bool tk_finite(float t) { return t - t == 0.f; }

// coordinate c of the measurement (cx, cy, w, h) of a box x1 y1 x2 y2
__host__ __device__ __forceinline__ float tk_measure(const float* b, int c) { return c < 2 ? 0.5f * (b[c] + b[c + 2]) : b[c] - b[c - 2]; }

__host__ __device__ __forceinline__ void tk_motion_init(const TrackArgs& p, float* m, const float* b) {
  const float H = tk_hs(tk_measure(b, 3));
  const float sp = (2.f * p.std_pos) * H, sv = (10.f * p.std_vel) * H;
  for (int c = 0; c < 4; ++c) {
    float* mc = m + c * MC;
    mc[M_X] = tk_measure(b, c);
    mc[M_V] = 0.f;
    mc[M_P00] = sp * sp;
    mc[M_P01] = 0.f;
    mc[M_P11] = sv * sv;
  }
}

// one coordinate one frame on; H the scale read before any coordinate of the slot moved.  Returns the new x.
__host__ __device__ __forceinline__ float tk_motion_predict(const TrackArgs& p, float* mc, float H) {
  const float q0 = (p.std_pos * H) * (p.std_pos * H), q1 = (p.std_vel * H) * (p.std_vel * H);
  const float x = mc[M_X] + mc[M_V];
  const float a = mc[M_P01] + mc[M_P11];
  mc[M_X] = x;
  mc[M_P00] = ((mc[M_P00] + mc[M_P01]) + a) + q0;
  mc[M_P01] = a;
  mc[M_P11] = mc[M_P11] + q1;
  return x;
}

// half of the predicted box: the centre coordinate and the clamped extent -> (low, high)
__host__ __device__ __forceinline__ void tk_motion_span(float centre, float extent, float* lo, float* hi) {
  const float e = extent > 0.f ? extent : 0.f;
  *lo = centre - 0.5f * e;
  *hi = centre + 0.5f * e;
}

// a match: the four filters take the detection's box; a state that left the finite numbers starts again from the box
__host__ __device__ __forceinline__ void tk_motion_update(const TrackArgs& p, float* m, const float* b) {
  const float H = tk_hs(m[3 * MC + M_X]);
  const float r = (p.std_pos * H) * (p.std_pos * H);
  bool ok = true;
  for (int c = 0; c < 4; ++c) {
    float* mc = m + c * MC;
    const float p00 = mc[M_P00], p01 = mc[M_P01];
    const float s = p00 + r, k0 = p00 / s, k1 = p01 / s, y = tk_measure(b, c) - mc[M_X];
    const float x = mc[M_X] + k0 * y, v = mc[M_V] + k1 * y;
    mc[M_X] = x;
    mc[M_V] = v;
    mc[M_P11] = mc[M_P11] - k1 * p01;
    mc[M_P01] = p01 - k1 * p00;
    mc[M_P00] = p00 - k0 * p00;
    ok = ok && tk_finite(x) && tk_finite(v);
  }
  if (!ok) tk_motion_init(p, m, b);
}

// track_pred of a row: the box its matched track was predicted at (pb), four zeros for every other row (pb null)
__host__ __device__ __forceinline__ void tk_pred(const TrackArgs& p, long row, const float* pb) {
  for (int k = 0; k < 4; ++k) p.o_pred[row * 4 + k] = pb ? pb[k] : 0.f;
}

// ---------------------------------------------------------------------------- re-identification, host and device
// a parked track takes part in step 3b
__host__ __device__ __forceinline__ bool tk_parked(const int* li, const float* lf) { return li[I_ID] != 0 && tk_live(lf[F_INV]); }

// A revived detection's slot continues the parked track: the entry's rows become the slot's, the entry is emptied, the slot is
// then rewritten as by a match.  Returns the row's flags.
__host__ __device__ __forceinline__ int tk_revive_slot(const TrackArgs& p, int* si, float* sf, int* li, const float* lf, long row,
                                                       float inv, int clock) {
  for (int k = 0; k < NI; ++k) si[k] = li[k];
  for (int k = 0; k < NF; ++k) sf[k] = lf[k];
  li[I_ID] = 0;
  return tk_update_slot(p, si, sf, row, inv, false, clock, 0) | FP_TRACK_REVIVED;
}

// ------------------------------------------------------------------------------------------------------------ the kernel
// bitonic sort of key[0, n_sort), n_sort a power of two, by the whole workgroup.  Returns the keys in front of the first KEY_NONE.
__device__ __forceinline__ int tk_sort(unsigned long long* key, int n_sort, int tid) {
  for (int k = 2; k <= n_sort; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n_sort >> 1); t += TPB) {
        const int i = 2 * t - (t & (j - 1)), r = i + j;
        const unsigned long long a = key[i], b = key[r];
        if ((a > b) == ((i & k) == 0)) {
          key[i] = b;
          key[r] = a;
        }
      }
      __syncthreads();
    }
  int n_valid = 0;
  for (int step = n_sort; step > 0; step >>= 1)
    if (n_valid + step <= n_sort && key[n_valid + step - 1] != KEY_NONE) n_valid += step;
  return n_valid;
}

// One wave walks the sorted keys 64 at a time with a ballot per taken pair (two 64-bit masks: tracks and detections already
// taken; at most `most` pairs).  Returns, on the lane that stands for a taken detection's position, the track it took; else -1.
__device__ __forceinline__ int tk_walk(const unsigned long long* key, int n_valid, int most, int lane) {
  int mine = -1;
  unsigned long long t_taken = 0ull, d_taken = 0ull;
  int taken = 0;
  for (int i0 = 0; i0 < n_valid && taken < most; i0 += FP_WAVE) {
    const int i = i0 + lane;
    const bool have = i < n_valid;
    const unsigned long long kk = have ? key[i] : 0ull;
    const int k_slot = tk_key_slot(kk), k_pos = tk_key_pos(kk);
    bool alive = have && !((t_taken >> k_slot) & 1ull) && !((d_taken >> k_pos) & 1ull);
    unsigned long long live = __ballot(alive);
    while (live) {
      const int l = __ffsll((long long)live) - 1;   // the first pair of the batch still free is taken
      const int w_slot = __shfl(k_slot, l), w_pos = __shfl(k_pos, l);
      t_taken |= 1ull << w_slot;
      d_taken |= 1ull << w_pos;
      ++taken;
      if (lane == w_pos) mine = w_slot;
      if (alive && (k_slot == w_slot || k_pos == w_pos)) alive = false;
      live = __ballot(alive);
    }
  }
  return mine;
}

// The dot product of a track-side row and a detection's row by one group of 16 lanes (gl: the lane within the group): the
// partials, then xor 8, 4, 2, 1, so every lane of the group returns the same sum.
__device__ __forceinline__ float tk_dot16(const float* t, const float* d, int D, int gl) {
  float v = tk_partial(t, d, D, gl);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

// the r-th set bit of m (r < popcount)
__device__ __forceinline__ int tk_nth_bit(unsigned long long m, int r) {
  for (int k = 0; k < r; ++k) m &= m - 1ull;
  return __ffsll((long long)m) - 1;
}

template <bool MOTION, bool REID>
__global__ __launch_bounds__(TPB) void tracklets_kernel(TrackArgs p) {
  // <true, false> alone keeps the text of tk_sort and tk_walk written out in step 3.  Measured (FINDINGS 87): through the calls
  // that one instantiation marched 0.9 % slower on 256 frames x 2 faces (1.360 against 1.348 ms) and 0.9 % slower on 256 x 8
  // (6.034 against 5.978 ms), same VGPRs, 2 042 instructions against 2 043; written out it is at the old time again.  The other
  // three go through the calls and are as fast or 1 - 1.5 % faster.  A change of the sort or the walk is made in both places.
  constexpr bool WRITTEN_OUT = MOTION && !REID;
  __shared__ unsigned long long key[SLOTS * MAXD];   // 32 KB
  __shared__ int cmin[MAXCH], cmax[MAXCH];
  __shared__ int s_i[SLOTS][NI];
  __shared__ float s_f[SLOTS][NF];
  __shared__ float s_m[MOTION ? SLOTS : 1][MF];      // <true, *> only: the filters and the predicted boxes
  __shared__ float s_pb[MOTION ? SLOTS : 1][4];
  __shared__ int l_i[REID ? LOST : 1][NI];           // <*, true> only: the parked tracks' rows
  __shared__ float l_f[REID ? LOST : 1][NF];
  __shared__ int le[REID ? LOST : 1], lu[REID ? MAXD : 1], det_ent[REID ? MAXD : 1];   // parked entries / unmatched positions, ascending
  __shared__ int s_nU;
  __shared__ int det_row[MAXD], det_slot[MAXD], det_flag[MAXD];
  __shared__ float det_inv[MAXD];                    // 0 = a dead row
  __shared__ int lt[SLOTS], ld[MAXD];                // the live slots / the positions of the live detections, ascending
  __shared__ int wcount[NW];
  __shared__ unsigned long long fmask[NW];
  __shared__ int s_nT, s_nD;

  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = p.D, D4 = D >> 2, n = p.n;
  const int CH = tk_chunk_rows(n), nch = n > 0 ? (n + CH - 1) / CH : 0;
  const unsigned long long lane_lt = (1ull << lane) - 1ull;

  for (int c = tid; c < nch; c += TPB) {
    cmin[c] = INT_MAX;
    cmax[c] = INT_MIN;
  }
  for (int i = tid; i < SLOTS * NI; i += TPB) (&s_i[0][0])[i] = p.si[(long)s * SLOTS * NI + i];
  for (int i = tid; i < SLOTS * NF; i += TPB) (&s_f[0][0])[i] = p.sf[(long)s * SLOTS * NF + i];
  if constexpr (REID) {
    for (int i = tid; i < LOST * NI; i += TPB) (&l_i[0][0])[i] = p.li[(long)s * LOST * NI + i];
    for (int i = tid; i < LOST * NF; i += TPB) (&l_f[0][0])[i] = p.lf[(long)s * LOST * NF + i];
  }
  __syncthreads();

  // first pass over the rows: frame range of every chunk; the untracked rows of the groups this workgroup owns
  for (int g0 = 0; g0 < n; g0 += TPB) {
    const int i = g0 + tid;
    if (i < n) {
      const int f = p.frame[i], c = i / CH;
      atomicMin(&cmin[c], f);
      atomicMax(&cmax[c], f);
      if ((unsigned)(g0 / TPB) % gridDim.x == (unsigned)s && tk_untracked(p, f)) {
        tk_out(p, i, 0, 0, 0, FP_TRACK_NO_STREAM);
        if constexpr (MOTION) tk_pred(p, i, nullptr);
      }
    }
  }
  __syncthreads();

  int clock = p.hdr[2 * s], next_id = p.hdr[2 * s + 1];   // next_id is kept by wave 0
  float* semb = p.semb + (long)s * SLOTS * D;
  float* sbest = p.sbest + (long)s * SLOTS * D;
  bool owned = false;   // MOTION: the stream has a frame in this step, its filters are in s_m
  int head = 0;         // REID: where the ring parks next, kept by every thread
  float* lemb = nullptr;
  float* lbest = nullptr;
  if constexpr (REID) {
    head = p.lhdr[2 * s];   // taken modulo LOST wherever it is used
    lemb = p.lemb + (long)s * LOST * D;
    lbest = p.lbest + (long)s * LOST * D;
  }

  for (int f0 = 0; f0 < p.B; f0 += TPB) {
    const bool mine = f0 + tid < p.B && p.sof[f0 + tid] == s;
    const unsigned long long mb = __ballot(mine);
    if (lane == 0) fmask[wave] = mb;
    __syncthreads();
    for (int w = 0; w < NW; ++w) {
      unsigned long long mm = fmask[w];
      if constexpr (MOTION) {
        if (mm != 0ull && !owned) {   // the stream's first frame of the step: only now is motion read (and written at the end)
          for (int i = tid; i < SLOTS * MF; i += TPB) (&s_m[0][0])[i] = p.motion[(long)s * SLOTS * MF + i];
          owned = true;
          __syncthreads();
        }
      }
      while (mm) {
        const int f = f0 + w * 64 + (__ffsll((long long)mm) - 1);
        mm &= mm - 1ull;

        // ---- 1. the clock, expiry
        clock += 1;
        unsigned long long exm = 0ull;   // REID: the slots that expire in this frame, found by every wave for itself
        if constexpr (REID) exm = __ballot(s_i[lane][I_ID] != 0 && clock - s_i[lane][I_LAST] > p.max_age);
        // ---- 1b. thread 4 * slot + c moves coordinate c of a slot that survives the expiry; the scale is read first
        const int m_slot = tid >> 2, m_c = tid & 3;
        float m_H = 1.f;
        bool m_live = false;
        if constexpr (MOTION) {
          if (tid < 4 * SLOTS) {
            m_H = tk_hs(s_m[m_slot][3 * MC + M_X]);
            m_live = s_i[m_slot][I_ID] != 0 && !(clock - s_i[m_slot][I_LAST] > p.max_age);
          }
          __syncthreads();
        }
        if constexpr (REID) {
          // ---- 1a. the pool forgets; 1. the expiring slots are parked: the r-th of them, ascending, in entry (head + r) % LOST
          if (tid < LOST && l_i[tid][I_ID] != 0 && clock - l_i[tid][I_LAST] > p.lost_age) l_i[tid][I_ID] = 0;
          if (exm != 0ull) {   // every wave holds the same mask
            if constexpr (!MOTION) __syncthreads();   // every wave has read the slots (MOTION: the barrier above)
            const int n_ex = __popcll(exm);
            if (wave == 0 && ((exm >> lane) & 1ull)) {
              const int e = (head + __popcll(exm & lane_lt)) & (LOST - 1);
              for (int k = 0; k < NI; ++k) l_i[e][k] = s_i[lane][k];
              for (int k = 0; k < NF; ++k) l_f[e][k] = s_f[lane][k];
              s_i[lane][I_ID] = 0;
            }
            for (int idx = tid; idx < n_ex * D4; idx += TPB) {
              const int r = idx / D4, k = idx % D4, slot = tk_nth_bit(exm, r), e = (head + r) & (LOST - 1);
              ((f32x4*)(lemb + (long)e * D))[k] = ((const f32x4*)(semb + (long)slot * D))[k];
              ((f32x4*)(lbest + (long)e * D))[k] = ((const f32x4*)(sbest + (long)slot * D))[k];
            }
            head = (head + n_ex) & (LOST - 1);
            __threadfence_block();   // the barriers of step 2 stand between these copies and step 3b
          }
        } else {
          if (tid < SLOTS && s_i[tid][I_ID] != 0 && clock - s_i[tid][I_LAST] > p.max_age) s_i[tid][I_ID] = 0;
        }
        if constexpr (MOTION) {
          if (tid < 4 * SLOTS) {   // whole waves: the centre lanes (c < 2) fetch their extent from lane + 2
            const float x = m_live ? tk_motion_predict(p, &s_m[m_slot][m_c * MC], m_H) : 0.f;
            const float other = __shfl_xor(x, 2);
            if (m_live && m_c < 2) tk_motion_span(x, other, &s_pb[m_slot][m_c], &s_pb[m_slot][m_c + 2]);
          }
        }

        // ---- 2. the frame's rows in row order: the first MAXD take part
        int base = 0;
        for (int c = 0; c < nch; ++c) {
          if (f < cmin[c] || f > cmax[c]) continue;
          const int g_end = min(c * CH + CH, n);   // n <= FP_TRACK_MAX_ROWS: no index here passes 2^31
          for (int g0 = c * CH; g0 < g_end; g0 += TPB) {
            const int i = g0 + tid;
            const bool pred = i < g_end && p.frame[i] == f;
            const unsigned long long bm = __ballot(pred);
            if (lane == 0) wcount[wave] = __popcll(bm);
            __syncthreads();
            int before = 0, total = 0;
            for (int v = 0; v < NW; ++v) {
              const int cv = wcount[v];
              before += v < wave ? cv : 0;
              total += cv;
            }
            if (pred) {
              const int pos = base + before + __popcll(bm & lane_lt);
              if (pos < MAXD) {
                const float inv = p.xinv[i];
                det_row[pos] = i;
                det_inv[pos] = tk_live(inv) ? inv : 0.f;
              } else {
                tk_out(p, i, 0, 0, clock, FP_TRACK_OVER);
                if constexpr (MOTION) tk_pred(p, i, nullptr);
              }
            }
            base += total;
            __syncthreads();
          }
        }
        const int nd = min(base, MAXD);
        __syncthreads();
        if (nd == 0) continue;
        unsigned long long pm = 0ull;   // REID: the parked tracks that can pair, found by every wave for itself
        if constexpr (REID) pm = __ballot(tk_parked(l_i[lane], l_f[lane]));

        // ---- live slots and live detections, ascending
        if (wave == 0) {
          const bool tl = s_i[lane][I_ID] != 0;
          const unsigned long long tm = __ballot(tl);
          if (tl) lt[__popcll(tm & lane_lt)] = lane;
          if (lane == 0) s_nT = __popcll(tm);
        } else if (wave == 1) {
          const bool dl = lane < nd && det_inv[lane] > 0.f;
          const unsigned long long dm = __ballot(dl);
          if (dl) ld[__popcll(dm & lane_lt)] = lane;
          if (lane == 0) s_nD = __popcll(dm);
          det_slot[lane] = -1;
          det_flag[lane] = 0;
          if constexpr (REID) det_ent[lane] = -1;
        }
        __syncthreads();
        const int nT = s_nT, nD = s_nD, np = nT * nD;

        // ---- 3. the pairs: cosine, IoU, key
        int n_valid = 0;
        if (np > 0) {
          int n_sort = 2;
          while (n_sort < np) n_sort <<= 1;
          const int grp = tid / GL, gl = tid % GL;
          for (int q0 = 0; q0 < np; q0 += NG) {
            const int q = min(q0 + grp, np - 1);
            const int slot = lt[q / nD], pos = ld[q % nD];
            const long row = det_row[pos];
            const float v = tk_dot16(semb + (long)slot * D, p.emb + row * D, D, gl);
            if (gl == 0 && q0 + grp < np) {
              const float c = tk_cos(v, s_f[slot][F_INV], det_inv[pos]);
              const float iou = tk_iou(MOTION ? s_pb[slot] : &s_f[slot][F_BOX], p.box + row * 4);
              key[q] = tk_admissible(p, c, iou) ? tk_key(c, slot, pos) : KEY_NONE;
            }
          }
          for (int i = np + tid; i < n_sort; i += TPB) key[i] = KEY_NONE;
          __syncthreads();
          if constexpr (!WRITTEN_OUT) {
            n_valid = tk_sort(key, n_sort, tid);
          } else {   // tk_sort's text
            for (int k = 2; k <= n_sort; k <<= 1)
              for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (n_sort >> 1); t += TPB) {
                  const int i = 2 * t - (t & (j - 1)), r = i + j;
                  const unsigned long long a = key[i], b = key[r];
                  if ((a > b) == ((i & k) == 0)) {
                    key[i] = b;
                    key[r] = a;
                  }
                }
                __syncthreads();
              }
            for (int step = n_sort; step > 0; step >>= 1)
              if (n_valid + step <= n_sort && key[n_valid + step - 1] != KEY_NONE) n_valid += step;
          }
        }

        // ---- 3 (walk): wave 0; lane j stands for the detection at position j
        int my_slot = -1, my_ent = -1;
        if (wave == 0) {
          if constexpr (!WRITTEN_OUT) {
            my_slot = tk_walk(key, n_valid, min(nT, nD), lane);
          } else {   // tk_walk's text
            unsigned long long t_taken = 0ull, d_taken = 0ull;
            const int most = min(nT, nD);
            int taken = 0;
            for (int i0 = 0; i0 < n_valid && taken < most; i0 += FP_WAVE) {
              const int i = i0 + lane;
              const bool have = i < n_valid;
              const unsigned long long kk = have ? key[i] : 0ull;
              const int k_slot = tk_key_slot(kk), k_pos = tk_key_pos(kk);
              bool alive = have && !((t_taken >> k_slot) & 1ull) && !((d_taken >> k_pos) & 1ull);
              unsigned long long live = __ballot(alive);
              while (live) {
                const int l = __ffsll((long long)live) - 1;
                const int w_slot = __shfl(k_slot, l), w_pos = __shfl(k_pos, l);
                t_taken |= 1ull << w_slot;
                d_taken |= 1ull << w_pos;
                ++taken;
                if (lane == w_pos) my_slot = w_slot;
                if (alive && (k_slot == w_slot || k_pos == w_pos)) alive = false;
                live = __ballot(alive);
              }
            }
          }
        }

        // ---- 3b. the live detections the walk left unmatched x the parked tracks: cosine alone, the same key, sort and walk
        if constexpr (REID) {
          if (pm != 0ull) {   // workgroup-uniform: a frame with an empty pool goes straight on
            if (wave == 0) {
              const bool un = lane < nd && det_inv[lane] > 0.f && my_slot < 0;
              const unsigned long long um = __ballot(un);
              if (un) lu[__popcll(um & lane_lt)] = lane;
              if (lane == 0) s_nU = __popcll(um);
            } else if (wave == 1) {
              if ((pm >> lane) & 1ull) le[__popcll(pm & lane_lt)] = lane;
            }
            __syncthreads();   // wave 0 is through with the keys of step 3
            const int nU = s_nU, nE = __popcll(pm), nq = nE * nU;
            if (nq > 0) {
              int n_sort = 2;
              while (n_sort < nq) n_sort <<= 1;
              const int grp = tid / GL, gl = tid % GL;
              for (int q0 = 0; q0 < nq; q0 += NG) {
                const int q = min(q0 + grp, nq - 1);
                const int ent = le[q / nU], pos = lu[q % nU];
                const float v = tk_dot16(lemb + (long)ent * D, p.emb + (long)det_row[pos] * D, D, gl);
                if (gl == 0 && q0 + grp < nq) {
                  const float c = tk_cos(v, l_f[ent][F_INV], det_inv[pos]);
                  key[q] = c > p.tau_reid ? tk_key(c, ent, pos) : KEY_NONE;
                }
              }
              for (int i = nq + tid; i < n_sort; i += TPB) key[i] = KEY_NONE;
              __syncthreads();
              const int n_valid_b = tk_sort(key, n_sort, tid);
              if (wave == 0) my_ent = tk_walk(key, n_valid_b, min(nE, nU), lane);
            }
          }
        }

        // ---- 4, 5: wave 0.  The unmatched live detections open tracks in the lowest free slots, in row order
        if (wave == 0) {
          const bool dl = lane < nd && det_inv[lane] > 0.f;
          const bool matched = my_slot >= 0;
          const unsigned long long freem = __ballot(s_i[lane][I_ID] == 0);
          const bool need = dl && !matched;
          const unsigned long long needm = __ballot(need);
          const int n_free = __popcll(freem);
          int flags = 0, new_id = 0;
          if (need) {
            const int rank = __popcll(needm & lane_lt);
            if (rank < n_free) {
              unsigned long long fm = freem;
              for (int r = 0; r < rank; ++r) fm &= fm - 1ull;
              my_slot = __ffsll((long long)fm) - 1;
              if constexpr (!REID) new_id = next_id + rank;
            } else {
              flags = FP_TRACK_FULL;
              if constexpr (REID) my_ent = -1;   // no slot: the parked track stays parked
            }
          }
          if constexpr (REID) {   // ids go to the true openings alone, by their rank among themselves
            const unsigned long long openm = __ballot(need && my_slot >= 0 && my_ent < 0);
            new_id = next_id + __popcll(openm & lane_lt);
            next_id += __popcll(openm);
          } else {
            next_id += min(__popcll(needm), n_free);
          }
          if (lane < nd) {
            const long row = det_row[lane];
            if constexpr (MOTION) {
              tk_pred(p, row, matched ? s_pb[my_slot] : nullptr);
              if (matched) tk_motion_update(p, s_m[my_slot], p.box + row * 4);
              else if (dl && my_slot >= 0) tk_motion_init(p, s_m[my_slot], p.box + row * 4);
            }
            if (!dl) {
              tk_out(p, row, 0, 0, clock, FP_TRACK_DEAD_ROW);
            } else if (my_slot < 0) {
              tk_out(p, row, 0, 0, clock, flags);
            } else {
              if (REID && my_ent >= 0) {
                flags = tk_revive_slot(p, s_i[my_slot], s_f[my_slot], l_i[my_ent], l_f[my_ent], row, det_inv[lane], clock);
                det_ent[lane] = my_ent;
              } else {
                flags = tk_update_slot(p, s_i[my_slot], s_f[my_slot], row, det_inv[lane], !matched, clock, new_id);
              }
              tk_out(p, row, s_i[my_slot][I_ID], s_i[my_slot][I_HITS], clock, flags);
              det_slot[lane] = my_slot;
              det_flag[lane] = flags;
            }
          }
        }
        __syncthreads();

        // ---- the embeddings of the rewritten slots
        for (int idx = tid; idx < nD * D4; idx += TPB) {
          const int pos = ld[idx / D4], k = idx % D4, slot = det_slot[pos];
          if (slot < 0) continue;
          const f32x4 v = ((const f32x4*)(p.emb + (long)det_row[pos] * D))[k];
          ((f32x4*)(semb + (long)slot * D))[k] = v;
          if (det_flag[pos] & FP_TRACK_BEST) {
            ((f32x4*)(sbest + (long)slot * D))[k] = v;
          } else if constexpr (REID) {   // a revived track that keeps its best shot keeps that shot's embedding
            const int ent = det_ent[pos];
            if (ent >= 0) ((f32x4*)(sbest + (long)slot * D))[k] = ((const f32x4*)(lbest + (long)ent * D))[k];
          }
        }
        __threadfence_block();
        __syncthreads();   // the rewritten embeddings are what the next frame's pairs read
      }
    }
    __syncthreads();   // fmask is rewritten by the next batch of frames
  }

  for (int i = tid; i < SLOTS * NI; i += TPB) p.si[(long)s * SLOTS * NI + i] = (&s_i[0][0])[i];
  for (int i = tid; i < SLOTS * NF; i += TPB) p.sf[(long)s * SLOTS * NF + i] = (&s_f[0][0])[i];
  if constexpr (MOTION)
    if (owned)
      for (int i = tid; i < SLOTS * MF; i += TPB) p.motion[(long)s * SLOTS * MF + i] = (&s_m[0][0])[i];
  if constexpr (REID) {
    for (int i = tid; i < LOST * NI; i += TPB) p.li[(long)s * LOST * NI + i] = (&l_i[0][0])[i];
    for (int i = tid; i < LOST * NF; i += TPB) p.lf[(long)s * LOST * NF + i] = (&l_f[0][0])[i];
    if (tid == 0) p.lhdr[2 * s] = head;
  }
  if (tid == 0) {
    p.hdr[2 * s] = clock;
    p.hdr[2 * s + 1] = next_id;
  }
}

// ------------------------------------------------------------------------------------------ arguments: one builder, one checker
// The tails an entry point does not have stay at their defaults: no motion array, no pool.
TrackArgs track_args(const fp_track_state* st, int n_streams, int D, const int32_t* frame, const float* box, const float* emb,
                     const float* xinv, const float* score, int n, const int32_t* stream_of_frame, int B, int max_age,
                     float tau_near, float tau_far, float iou_min, int32_t* track_id, int32_t* track_hits, int32_t* track_clock,
                     int32_t* track_flags, float* motion = nullptr, float std_pos = 0.f, float std_vel = 0.f,
                     float* track_pred = nullptr, const fp_track_lost* lost = nullptr, float tau_reid = 0.f, int lost_age = 0) {
  TrackArgs a;
  a.hdr = st ? st->hdr : nullptr;
  a.si = st ? st->slot_i : nullptr;
  a.sf = st ? st->slot_f : nullptr;
  a.semb = st ? st->emb : nullptr;
  a.sbest = st ? st->best_emb : nullptr;
  a.S = n_streams; a.D = D;
  a.frame = frame; a.box = box; a.emb = emb; a.xinv = xinv; a.score = score; a.n = n;
  a.sof = stream_of_frame; a.B = B;
  a.max_age = max_age; a.tau_near = tau_near; a.tau_far = tau_far; a.iou_min = iou_min;
  a.o_id = track_id; a.o_hits = track_hits; a.o_clock = track_clock; a.o_flags = track_flags;
  a.motion = motion; a.std_pos = std_pos; a.std_vel = std_vel; a.o_pred = track_pred;
  a.lhdr = lost ? lost->lost_hdr : nullptr;
  a.li = lost ? lost->lost_i : nullptr;
  a.lf = lost ? lost->lost_f : nullptr;
  a.lemb = lost ? lost->lost_emb : nullptr;
  a.lbest = lost ? lost->lost_best_emb : nullptr;
  a.tau_reid = tau_reid; a.lost_age = lost_age;
  return a;
}

// what an entry point requires of the two optional parts
enum NeedMotion { MOTION_ABSENT, MOTION_OPTIONAL, MOTION_REQUIRED };
struct Needs {
  NeedMotion motion;
  bool pool;
};

int check_args(const TrackArgs& a, Needs need) {
  if (!a.hdr || !a.si || !a.sf || !a.semb || !a.sbest) return FP_ERR_INVALID_ARG;   // a null state struct gave five nulls
  if (a.S < 1 || a.D < 4 || a.D % 4 != 0 || a.D > FP_TRACK_MAX_DIM || a.n < 0 || a.n > FP_TRACK_MAX_ROWS || a.B < 0 || a.max_age < 0) return FP_ERR_INVALID_ARG;
  if (a.B > 0 && !a.sof) return FP_ERR_INVALID_ARG;
  if (a.n > 0 && (!a.frame || !a.box || !a.emb || !a.xinv || !a.o_id || !a.o_hits || !a.o_clock || !a.o_flags))
    return FP_ERR_INVALID_ARG;
  if (((uintptr_t)a.semb | (uintptr_t)a.sbest | (uintptr_t)a.emb) % 16 != 0) return FP_ERR_INVALID_ARG;   // float4 rows
  if (!(a.tau_far >= a.tau_near) || a.iou_min != a.iou_min) return FP_ERR_INVALID_ARG;
  if (a.motion ? need.motion == MOTION_ABSENT : need.motion == MOTION_REQUIRED) return FP_ERR_INVALID_ARG;
  if (a.motion) {
    if (a.n > 0 && !a.o_pred) return FP_ERR_INVALID_ARG;
    if (!(a.std_pos > 0.f && tk_finite(a.std_pos) && a.std_vel > 0.f && tk_finite(a.std_vel))) return FP_ERR_INVALID_ARG;
  } else if (a.o_pred) {   // track_pred is null iff motion is; std_pos / std_vel are not looked at
    return FP_ERR_INVALID_ARG;
  }
  if (need.pool) {
    if (!a.lhdr || !a.li || !a.lf || !a.lemb || !a.lbest) return FP_ERR_INVALID_ARG;   // a null pool struct gave five nulls
    if (((uintptr_t)a.lemb | (uintptr_t)a.lbest) % 16 != 0) return FP_ERR_INVALID_ARG;   // float4 rows
    if (!tk_finite(a.tau_reid) || a.lost_age <= a.max_age) return FP_ERR_INVALID_ARG;
  }
  return FP_OK;
}

// ---------------------------------------------------------------------------------------------------------- the host twin
// the cosine of one pair: the 16 partials, then the xor-shuffle sum as lane 0 sees it
float emu_cos(const float* t, const float* d, int D, float inv_t, float inv_d) {
  float part[GL];
  for (int gl = 0; gl < GL; ++gl) part[gl] = tk_partial(t, d, D, gl);
  for (int off = GL / 2; off > 0; off >>= 1)
    for (int l = 0; l < off; ++l) part[l] = part[l] + part[l + off];
  return tk_cos(part[0], inv_t, inv_d);
}

// the keys in ascending order, each taken unless its track-side partner or its position is: partner[position], -1 where none
void emu_greedy(std::vector<unsigned long long>& key, int* partner) {
  std::sort(key.begin(), key.end());
  for (int j = 0; j < MAXD; ++j) partner[j] = -1;
  unsigned long long t_taken = 0ull, d_taken = 0ull;
  for (size_t i = 0; i < key.size(); ++i) {
    const int k_slot = tk_key_slot(key[i]), k_pos = tk_key_pos(key[i]);
    if (((t_taken >> k_slot) & 1ull) || ((d_taken >> k_pos) & 1ull)) continue;
    t_taken |= 1ull << k_slot;
    d_taken |= 1ull << k_pos;
    partner[k_pos] = k_slot;
  }
}

void emulate_frame(const TrackArgs& p, int s, int f, int& clock, int& next_id, std::vector<unsigned long long>& key) {
  int* si = p.si + (long)s * SLOTS * NI;
  float* sf = p.sf + (long)s * SLOTS * NF;
  float* semb = p.semb + (long)s * SLOTS * p.D;
  float* sbest = p.sbest + (long)s * SLOTS * p.D;
  clock += 1;
  int* li = p.li ? p.li + (long)s * LOST * NI : nullptr;   // the pool; null without re-identification
  float* lf = li ? p.lf + (long)s * LOST * NF : nullptr;
  float* lemb = li ? p.lemb + (long)s * LOST * p.D : nullptr;
  float* lbest = li ? p.lbest + (long)s * LOST * p.D : nullptr;
  for (int e = 0; li && e < LOST; ++e)   // step 1a
    if (li[e * NI + I_ID] != 0 && clock - li[e * NI + I_LAST] > p.lost_age) li[e * NI + I_ID] = 0;
  for (int t = 0; t < SLOTS; ++t)
    if (si[t * NI + I_ID] != 0 && clock - si[t * NI + I_LAST] > p.max_age) {
      if (li) {   // parked in the ring before the slot is freed
        int& head = p.lhdr[2 * s];
        const int e = head & (LOST - 1);
        std::copy(si + t * NI, si + (t + 1) * NI, li + e * NI);
        std::copy(sf + t * NF, sf + (t + 1) * NF, lf + e * NF);
        std::copy(semb + (long)t * p.D, semb + (long)(t + 1) * p.D, lemb + (long)e * p.D);
        std::copy(sbest + (long)t * p.D, sbest + (long)(t + 1) * p.D, lbest + (long)e * p.D);
        head = (e + 1) & (LOST - 1);
      }
      si[t * NI + I_ID] = 0;
    }
  float* sm = p.motion ? p.motion + (long)s * SLOTS * MF : nullptr;
  float pbox[SLOTS][4];   // step 1b: the predicted boxes of the live slots
  for (int t = 0; sm && t < SLOTS; ++t) {
    if (si[t * NI + I_ID] == 0) continue;
    float* m = sm + t * MF;
    const float H = tk_hs(m[3 * MC + M_X]);
    float x[4];
    for (int c = 0; c < 4; ++c) x[c] = tk_motion_predict(p, m + c * MC, H);
    for (int c = 0; c < 2; ++c) tk_motion_span(x[c], x[c + 2], &pbox[t][c], &pbox[t][c + 2]);
  }
  long det_row[MAXD];
  float det_inv[MAXD];
  int nd = 0;
  for (long i = 0; i < p.n; ++i) {
    if (p.frame[i] != f) continue;
    if (nd < MAXD) {
      det_row[nd] = i;
      det_inv[nd] = tk_live(p.xinv[i]) ? p.xinv[i] : 0.f;
      ++nd;
    } else {
      tk_out(p, i, 0, 0, clock, FP_TRACK_OVER);
      if (sm) tk_pred(p, i, nullptr);
    }
  }
  int my_slot[MAXD], my_ent[MAXD];   // step 3: the live track a detection takes; step 3b: the parked track an unmatched one revives
  key.clear();
  for (int t = 0; t < SLOTS; ++t) {
    if (si[t * NI + I_ID] == 0) continue;
    for (int j = 0; j < nd; ++j) {
      if (!(det_inv[j] > 0.f)) continue;
      const float c = emu_cos(semb + (long)t * p.D, p.emb + det_row[j] * p.D, p.D, sf[t * NF + F_INV], det_inv[j]);
      const float iou = tk_iou(sm ? pbox[t] : sf + t * NF + F_BOX, p.box + det_row[j] * 4);
      if (tk_admissible(p, c, iou)) key.push_back(tk_key(c, t, j));
    }
  }
  emu_greedy(key, my_slot);
  key.clear();
  for (int e = 0; li && e < LOST; ++e) {
    if (!tk_parked(li + e * NI, lf + e * NF)) continue;
    for (int j = 0; j < nd; ++j) {
      if (!(det_inv[j] > 0.f) || my_slot[j] >= 0) continue;
      const float c = emu_cos(lemb + (long)e * p.D, p.emb + det_row[j] * p.D, p.D, lf[e * NF + F_INV], det_inv[j]);
      if (c > p.tau_reid) key.push_back(tk_key(c, e, j));
    }
  }
  emu_greedy(key, my_ent);
  int slot_of[MAXD], flag_of[MAXD], ent_of[MAXD];
  for (int j = 0; j < nd; ++j) {
    const long row = det_row[j];
    slot_of[j] = -1;
    flag_of[j] = 0;
    ent_of[j] = -1;
    if (sm) tk_pred(p, row, my_slot[j] >= 0 ? pbox[my_slot[j]] : nullptr);
    if (!(det_inv[j] > 0.f)) {
      tk_out(p, row, 0, 0, clock, FP_TRACK_DEAD_ROW);
      continue;
    }
    int slot = my_slot[j];
    const bool matched = slot >= 0;
    int new_id = 0;
    if (!matched) {
      for (int t = 0; t < SLOTS && slot < 0; ++t)
        if (si[t * NI + I_ID] == 0) slot = t;
      if (slot < 0) {
        tk_out(p, row, 0, 0, clock, FP_TRACK_FULL);
        continue;
      }
      if (my_ent[j] < 0) new_id = next_id++;   // a revived track brings its id along
    }
    if (sm && matched) tk_motion_update(p, sm + slot * MF, p.box + row * 4);
    if (sm && !matched) tk_motion_init(p, sm + slot * MF, p.box + row * 4);
    int flags;
    if (my_ent[j] >= 0) {
      const int e = my_ent[j];
      flags = tk_revive_slot(p, si + slot * NI, sf + slot * NF, li + e * NI, lf + e * NF, row, det_inv[j], clock);
      ent_of[j] = e;
    } else {
      flags = tk_update_slot(p, si + slot * NI, sf + slot * NF, row, det_inv[j], !matched, clock, new_id);
    }
    tk_out(p, row, si[slot * NI + I_ID], si[slot * NI + I_HITS], clock, flags);
    slot_of[j] = slot;
    flag_of[j] = flags;
  }
  for (int j = 0; j < nd; ++j) {   // after every pair of the frame was scored against the old embeddings
    if (slot_of[j] < 0) continue;
    const float* e = p.emb + det_row[j] * p.D;
    std::copy(e, e + p.D, semb + (long)slot_of[j] * p.D);
    if (flag_of[j] & FP_TRACK_BEST) std::copy(e, e + p.D, sbest + (long)slot_of[j] * p.D);
    else if (ent_of[j] >= 0) std::copy(lbest + (long)ent_of[j] * p.D, lbest + (long)(ent_of[j] + 1) * p.D, sbest + (long)slot_of[j] * p.D);
  }
}

void emulate_step(const TrackArgs& p) {
  for (long i = 0; i < p.n; ++i)
    if (tk_untracked(p, p.frame[i])) {
      tk_out(p, i, 0, 0, 0, FP_TRACK_NO_STREAM);
      if (p.motion) tk_pred(p, i, nullptr);
    }
  std::vector<unsigned long long> key;
  for (int f = 0; f < p.B; ++f) {   // streams are independent: batch order is every stream's own order
    const int s = p.sof[f];
    if (s < 0 || s >= p.S) continue;
    emulate_frame(p, s, f, p.hdr[2 * s], p.hdr[2 * s + 1], key);
  }
}

// Every entry point ends here.  The refusals come before any HIP call; the emulate path makes none at all.
int run(const TrackArgs& a, Needs need, bool emulate, void* stream) {
  const int rc = check_args(a, need);
  if (rc != FP_OK) return rc;
  if (emulate) {
    emulate_step(a);
    return FP_OK;
  }
  if (a.B == 0 && a.n == 0) return FP_OK;
  void (*const kernel)(TrackArgs) = !a.li ? (!a.motion ? tracklets_kernel<false, false> : tracklets_kernel<true, false>)
                                          : (a.motion ? tracklets_kernel<true, true> : tracklets_kernel<false, true>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)a.S), dim3(TPB), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // namespace

extern "C" {

int fp_tracklets_step(const fp_track_state* state, int n_streams, int D, const int32_t* frame, const float* box,
                      const float* emb, const float* xinv, const float* score, int n, const int32_t* stream_of_frame, int B,
                      int max_age, float tau_near, float tau_far, float iou_min, int32_t* track_id, int32_t* track_hits,
                      int32_t* track_clock, int32_t* track_flags, void* stream) {
  return run(track_args(state, n_streams, D, frame, box, emb, xinv, score, n, stream_of_frame, B, max_age, tau_near, tau_far,
                        iou_min, track_id, track_hits, track_clock, track_flags),
             {MOTION_ABSENT, false}, false, stream);
}

int fp_tracklets_step_emulate(const fp_track_state* state, int n_streams, int D, const int32_t* frame, const float* box,
                              const float* emb, const float* xinv, const float* score, int n, const int32_t* stream_of_frame,
                              int B, int max_age, float tau_near, float tau_far, float iou_min, int32_t* track_id,
                              int32_t* track_hits, int32_t* track_clock, int32_t* track_flags) {
  return run(track_args(state, n_streams, D, frame, box, emb, xinv, score, n, stream_of_frame, B, max_age, tau_near, tau_far,
                        iou_min, track_id, track_hits, track_clock, track_flags),
             {MOTION_ABSENT, false}, true, nullptr);
}

int fp_tracklets_step_motion(const fp_track_state* state, int n_streams, int D, const int32_t* frame, const float* box,
                             const float* emb, const float* xinv, const float* score, int n, const int32_t* stream_of_frame,
                             int B, int max_age, float tau_near, float tau_far, float iou_min, int32_t* track_id,
                             int32_t* track_hits, int32_t* track_clock, int32_t* track_flags, float* motion, float std_pos,
                             float std_vel, float* track_pred, void* stream) {
  return run(track_args(state, n_streams, D, frame, box, emb, xinv, score, n, stream_of_frame, B, max_age, tau_near, tau_far,
                        iou_min, track_id, track_hits, track_clock, track_flags, motion, std_pos, std_vel, track_pred),
             {MOTION_REQUIRED, false}, false, stream);
}

int fp_tracklets_step_motion_emulate(const fp_track_state* state, int n_streams, int D, const int32_t* frame, const float* box,
                                     const float* emb, const float* xinv, const float* score, int n,
                                     const int32_t* stream_of_frame, int B, int max_age, float tau_near, float tau_far,
                                     float iou_min, int32_t* track_id, int32_t* track_hits, int32_t* track_clock,
                                     int32_t* track_flags, float* motion, float std_pos, float std_vel, float* track_pred) {
  return run(track_args(state, n_streams, D, frame, box, emb, xinv, score, n, stream_of_frame, B, max_age, tau_near, tau_far,
                        iou_min, track_id, track_hits, track_clock, track_flags, motion, std_pos, std_vel, track_pred),
             {MOTION_REQUIRED, false}, true, nullptr);
}

int fp_tracklets_step_reid(const fp_track_state* state, const fp_track_lost* lost, int n_streams, int D, const int32_t* frame,
                           const float* box, const float* emb, const float* xinv, const float* score, int n,
                           const int32_t* stream_of_frame, int B, int max_age, float tau_near, float tau_far, float iou_min,
                           int32_t* track_id, int32_t* track_hits, int32_t* track_clock, int32_t* track_flags, float tau_reid,
                           int lost_age, float* motion, float std_pos, float std_vel, float* track_pred, void* stream) {
  return run(track_args(state, n_streams, D, frame, box, emb, xinv, score, n, stream_of_frame, B, max_age, tau_near, tau_far,
                        iou_min, track_id, track_hits, track_clock, track_flags, motion, std_pos, std_vel, track_pred, lost,
                        tau_reid, lost_age),
             {MOTION_OPTIONAL, true}, false, stream);
}

int fp_tracklets_step_reid_emulate(const fp_track_state* state, const fp_track_lost* lost, int n_streams, int D,
                                   const int32_t* frame, const float* box, const float* emb, const float* xinv, const float* score,
                                   int n, const int32_t* stream_of_frame, int B, int max_age, float tau_near, float tau_far,
                                   float iou_min, int32_t* track_id, int32_t* track_hits, int32_t* track_clock,
                                   int32_t* track_flags, float tau_reid, int lost_age, float* motion, float std_pos, float std_vel,
                                   float* track_pred) {
  return run(track_args(state, n_streams, D, frame, box, emb, xinv, score, n, stream_of_frame, B, max_age, tau_near, tau_far,
                        iou_min, track_id, track_hits, track_clock, track_flags, motion, std_pos, std_vel, track_pred, lost,
                        tau_reid, lost_age),
             {MOTION_OPTIONAL, true}, true, nullptr);
}

}  // extern "C"
