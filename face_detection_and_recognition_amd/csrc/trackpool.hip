// trackpool.hip — a template per track: the weighted sum of a track's embeddings, kept on the device (gfx950).  Build-defined, no
// reference counterpart (DESIGN §7 "Tracklets: templates"; include/facepath.h states the procedure).  Build with
// -ffp-contract=off: sum + ((emb * xinv) * w) is three roundings on the device, in the host twin and in numpy float32, and there
// is no reduction anywhere, so the three share every bit.
//
// The tracker's per-row results (track_id, track_clock, track_flags) come in as DATA; nothing here reads the tracker's state.
// Two launches, nothing read back, no global atomics:
//   pool_directory_kernel   one wave per stream, integers only.  The stream's 128 table entries (id, last_clock, rows) sit two to
//       a lane in registers.  Where the stream's rows come in frame order (the usual batch; the first pass finds out) the wave
//       takes the rows 64 at a time in row order, all loads of a group in flight at once; else it takes the stream's frames in
//       ascending batch index and finds a frame's rows through the per-chunk frame ranges in LDS, which costs two trips to memory
//       per frame.  Either way id / clock / flags / weight test sit one row to a lane and the rows are
//       resolved one after the other with ballots: lookup by id, else lowest free-or-stale entry, else the entry with the
//       smallest last_clock.  Every row that takes part is appended to the stream's ordered list (ord[], code[]) in the
//       workspace, tagged with the SEGMENT it belongs to: a run of rows on one entry between two clearings of that entry.  An
//       entry evicted in the middle of a step so yields two segments.  The stream's list and its segment records live in the
//       workspace at [base, base + rows of the stream), base = the number of rows of lower streams, which every wave counts for
//       itself in its first pass over frame[].
//   pool_accumulate_kernel  one workgroup per row index b, D / 4 lanes with one float4 each.  It passes row b through when the
//       directory says so, and it owns segment record b when that is in use (all other workgroups leave at once).  The running sum
//       stays in registers along the segment; the segment's rows are picked from the stream's list 64 at a time by ballot, their
//       embedding rows, inverse norms and weights are loaded PF at a time ahead of the dependent adds, every row gets one float4
//       store of track_emb per lane.  An entry's segments of one step are chained, and the workgroup of the first walks them all:
//       tpl_sum / tpl_w are read once at the start and written once after the last, by the same workgroup.
// The twin runs the same __host__ __device__ arithmetic and tests serially on host memory.
#include <limits.h>
#include <string.h>

#include "common.h"

namespace {

constexpr int POOL = FP_TRACK_POOL, TI = 3;
constexpr int MAXCH = 1024;   // row chunks whose frame range is kept in LDS
constexpr int PF = 8;         // rows of a segment loaded ahead of their adds
static_assert(POOL == 2 * FP_WAVE, "two table entries per lane of the directory wave");
static_assert(POOL == FP_TRACK_SLOTS + FP_TRACK_LOST, "an entry for every live and every parked track of a stream");

enum { T_ID = 0, T_LAST = 1, T_ROWS = 2 };                                                            // tpl_i columns
// a segment record; G_USED: 0 nobody's, 1 the entry's first segment of the step (a workgroup starts there), 2 a later one
// (reached through G_NEXT of the one before: one workgroup walks an entry's segments in order, so that the sum it read at the
// start is not yet overwritten and is written back once, after the last)
enum { G_USED = 0, G_STREAM, G_ENT, G_KFIRST, G_KLAST, G_INIT, G_NEXT, G_ROWS0, SEG_INTS };

struct PoolArgs {
  int* ti;       // [S][POOL][3]
  float* tw;     // [S][POOL]
  float* tsum;   // [S][POOL][D]
  int S, D;
  const int* frame;
  const float* emb;
  const float* xinv;
  const float* weight;   // may be null
  int n;
  const int* sof;
  int B;
  const int* id;
  const int* clock;
  const int* flags;
  int keep;
  float* o_emb;
  int* o_rows;
  int* o_flags;
  int* ord;    // workspace [n]: the rows that take part, stream after stream, each stream's in its processing order
  int* code;   // workspace [n]: beside ord, 2 * segment record + (the row adds)
  int* pass;   // workspace [n]: 1 = the row has no track, track_emb is its own embedding
  int* seg;    // workspace [n][SEG_INTS]
};

// ---------------------------------------------------------------------------------------- the decision code, host and device
__host__ __device__ __forceinline__ bool tp_finite(float t) { return t - t == 0.f; }

// step 7: the row's weight, 0 where it adds nothing
__host__ __device__ __forceinline__ float tp_weight(const float* weight, long i) {
  if (!weight) return 1.f;
  const float w = weight[i];
  return (w > 0.f && tp_finite(w)) ? w : 0.f;
}

__host__ __device__ __forceinline__ bool tp_stale(int c, int last, int keep) { return (long long)c - (long long)last > (long long)keep; }

// the stream of a row's frame, -1 where it has none
__host__ __device__ __forceinline__ int tp_stream(const PoolArgs& p, int f) {
  if (f < 0 || f >= p.B) return -1;
  const int s = p.sof[f];
  return (s < 0 || s >= p.S) ? -1 : s;
}

// step 8, one element
__host__ __device__ __forceinline__ float tp_add(float sum, float e, float inv, float w) { return sum + ((e * inv) * w); }

// rows of one chunk; 64 * MAXCH rows in chunks of 64, more rows make the chunks longer
__host__ __device__ __forceinline__ int tp_chunk_rows(int n) {
  return FP_WAVE * (int)(((long)n + (long)FP_WAVE * MAXCH - 1) / ((long)FP_WAVE * MAXCH));
}

// ------------------------------------------------------------------------------------------------------------ the kernels
__device__ __forceinline__ int tp_first(unsigned long long m0, unsigned long long m1) {
  return m0 ? __ffsll((long long)m0) - 1 : (m1 ? FP_WAVE + __ffsll((long long)m1) - 1 : -1);
}

__global__ __launch_bounds__(FP_WAVE) void pool_directory_kernel(PoolArgs p) {
  __shared__ int cmin[MAXCH], cmax[MAXCH];
  const int s = blockIdx.x, lane = threadIdx.x, n = p.n;
  const int CH = tp_chunk_rows(n), nch = (n + CH - 1) / CH;
  for (int c = lane; c < nch; c += FP_WAVE) {
    cmin[c] = INT_MAX;
    cmax[c] = INT_MIN;
  }
  __syncthreads();

  // first pass over the rows: where this stream's list starts, the frame range of its rows per chunk, whether its rows come
  // in frame order (then row order is the processing order), and the rows without a stream in the groups this wave owns
  int base = 0, n_mine = 0, n_streamed = 0, run_max = INT_MIN;
  bool in_order = true;
  for (int g0 = 0; g0 < n; g0 += FP_WAVE) {
    const int i = g0 + lane;
    int st = -1, f = 0;
    if (i < n) {
      f = p.frame[i];
      st = tp_stream(p, f);
    }
    const bool mine = st == s;
    if (mine) {
      atomicMin(&cmin[i / CH], f);
      atomicMax(&cmax[i / CH], f);
    }
    const unsigned long long mm = __ballot(mine);
    base += __popcll(__ballot(st >= 0 && st < s));
    n_mine += __popcll(mm);
    n_streamed += __popcll(__ballot(st >= 0));
    if (mm != 0ull) {   // the largest frame among the stream's rows before this one: an inclusive prefix maximum, moved up one lane
      int pm = mine ? f : INT_MIN;
      for (int off = 1; off < FP_WAVE; off <<= 1) {
        const int o = __shfl_up(pm, off);
        if (lane >= off) pm = max(pm, o);
      }
      int before = __shfl_up(pm, 1);
      before = lane == 0 ? run_max : max(before, run_max);
      if (__ballot(mine && f < before) != 0ull) in_order = false;
      run_max = max(run_max, __shfl(pm, FP_WAVE - 1));
    }
    if (i < n && st < 0 && (unsigned)(g0 / FP_WAVE) % gridDim.x == (unsigned)s) {
      p.pass[i] = 1;
      p.o_rows[i] = 0;
      p.o_flags[i] = 0;
    }
  }
  __syncthreads();

  // the table: entry h * 64 + lane in e_*[h]; e_seg: the entry's open segment of this step (stream-local number), e_kl: one
  // past the list position of the entry's latest row
  int e_id[2], e_lc[2], e_rows[2], e_seg[2], e_kl[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int* t = p.ti + ((long)s * POOL + h * FP_WAVE + lane) * TI;
    e_id[h] = t[T_ID];
    e_lc[h] = t[T_LAST];
    e_rows[h] = t[T_ROWS];
    e_seg[h] = -1;
    e_kl[h] = 0;
  }
  int cnt = 0, nseg = 0;   // rows appended to the list, segments opened

  // Up to 64 rows of the stream, one to a lane (pred), in processing order: resolved one after the other with wave-uniform
  // scalars; what a row gets is parked in its own lane and stored by all lanes together afterwards.
  auto group = [&](int g0, bool pred, int r_id, int r_c, int r_fl, int r_add) {
    int my_k = -1, my_code = 0, my_rows = 0, my_flags = 0;
    unsigned long long bm = __ballot(pred && r_id > 0);
    while (bm) {
      const int b = __ffsll((long long)bm) - 1;
      bm &= bm - 1ull;
      const int id = __shfl(r_id, b), c = __shfl(r_c, b), add = __shfl(r_add, b);
      const bool is_new = (__shfl(r_fl, b) & FP_TRACK_NEW) != 0;
      // steps 1-4: the entry
      int ent = tp_first(__ballot(e_id[0] == id), __ballot(e_id[1] == id));
      int oflags = 0;
      bool take = ent >= 0 && is_new;
      if (ent < 0) {
        ent = tp_first(__ballot(e_id[0] == 0 || tp_stale(c, e_lc[0], p.keep)),
                       __ballot(e_id[1] == 0 || tp_stale(c, e_lc[1], p.keep)));
        if (ent < 0) {   // the smallest last_clock, the lowest index on ties: the minimum of last_clock * 256 + index
          const long long k0 = (long long)e_lc[0] * 256 + lane, k1 = (long long)e_lc[1] * 256 + FP_WAVE + lane;
          long long k = k0 < k1 ? k0 : k1;
          for (int off = FP_WAVE / 2; off > 0; off >>= 1) {
            const long long o = __shfl_xor(k, off);
            k = o < k ? o : k;
          }
          ent = (int)(k & 0xFF);
          oflags |= FP_TRACK_TPL_EVICTED;
        }
        take = true;
        if (!is_new) oflags |= FP_TRACK_TPL_RESTART;
      }
      const int el = ent & (FP_WAVE - 1);
      const bool owner = lane == el;
      const int k = base + cnt;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if ((ent >> 6) != h) continue;   // wave-uniform
        int prev = -1;
        if (take && owner) {             // step 5; what the entry gathered before stays a segment of its own
          prev = e_seg[h];
          if (prev >= 0) p.seg[(long)(base + prev) * SEG_INTS + G_KLAST] = e_kl[h];
          e_id[h] = id;
          e_rows[h] = 0;
          e_seg[h] = -1;
        }
        int j = __shfl(e_seg[h], el);
        const int rows_after = __shfl(e_rows[h], el) + add;
        if (j < 0) {
          j = nseg++;
          if (owner) {
            e_seg[h] = j;
            int* g = p.seg + (long)(base + j) * SEG_INTS;
            if (prev >= 0) p.seg[(long)(base + prev) * SEG_INTS + G_NEXT] = base + j;
            g[G_USED] = prev >= 0 ? 2 : 1;
            g[G_NEXT] = -1;
            g[G_STREAM] = s;
            g[G_ENT] = ent;
            g[G_KFIRST] = k;
            g[G_INIT] = take ? 0 : 1;
            g[G_ROWS0] = e_rows[h];
          }
        }
        if (owner) {   // steps 8 (the count) and 9
          e_rows[h] = rows_after;
          e_lc[h] = c;
          e_kl[h] = k + 1;
        }
        if (lane == b) {
          my_k = k;
          my_code = (base + j) * 2 + add;
          my_rows = rows_after;
          my_flags = oflags;
        }
      }
      ++cnt;
    }
    if (pred) {   // a row without a track (my_k < 0) is its own template
      const int i = g0 + lane;
      if (my_k >= 0) {
        p.ord[my_k] = i;
        p.code[my_k] = my_code;
      }
      p.pass[i] = my_k < 0 ? 1 : 0;
      p.o_rows[i] = my_rows;
      p.o_flags[i] = my_flags;
    }
  };

  if (in_order) {
    // the usual batch: the stream's rows in row order are its rows in frame order.  64 rows a time, every load of a group in
    // flight at once, no trip to memory per frame
    for (int g0 = 0; g0 < n; g0 += FP_WAVE) {
      const int ch = g0 / CH;
      if (cmin[ch] > cmax[ch]) continue;   // none of the chunk's rows is this stream's
      const int i = g0 + lane;
      int f = -1, r_id = 0, r_c = 0, r_fl = 0, r_add = 0;
      if (i < n) {
        f = p.frame[i];
        r_id = p.id[i];
        r_c = p.clock[i];
        r_fl = p.flags[i];
        r_add = tp_weight(p.weight, i) > 0.f ? 1 : 0;
      }
      const bool pred = tp_stream(p, f) == s;
      if (__ballot(pred) == 0ull) continue;
      group(g0, pred, r_id, r_c, r_fl, r_add);
    }
  } else {
    // scattered rows: frame by frame in ascending batch index, a frame's rows looked for in the chunks that can hold them
    for (int f0 = 0; f0 < p.B; f0 += FP_WAVE) {
      unsigned long long fm = __ballot(f0 + lane < p.B && p.sof[f0 + lane] == s);
      while (fm) {
        const int f = f0 + __ffsll((long long)fm) - 1;
        fm &= fm - 1ull;
        for (int c0 = 0; c0 < nch; c0 += FP_WAVE) {
          const int c = c0 + lane;
          unsigned long long cm = __ballot(c < nch && f >= cmin[c] && f <= cmax[c]);
          while (cm) {
            const int ch = c0 + __ffsll((long long)cm) - 1;
            cm &= cm - 1ull;
            const int g_end = min(ch * CH + CH, n);   // n <= FP_TRACK_MAX_ROWS: no index here passes 2^31
            for (int g0 = ch * CH; g0 < g_end; g0 += FP_WAVE) {
              const int i = g0 + lane;
              const bool pred = i < g_end && p.frame[i] == f;
              if (__ballot(pred) == 0ull) continue;
              int r_id = 0, r_c = 0, r_fl = 0, r_add = 0;
              if (pred) {
                r_id = p.id[i];
                r_c = p.clock[i];
                r_fl = p.flags[i];
                r_add = tp_weight(p.weight, i) > 0.f ? 1 : 0;
              }
              group(g0, pred, r_id, r_c, r_fl, r_add);
            }
          }
        }
      }
    }
  }

#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (e_seg[h] >= 0) p.seg[(long)(base + e_seg[h]) * SEG_INTS + G_KLAST] = e_kl[h];
    int* t = p.ti + ((long)s * POOL + h * FP_WAVE + lane) * TI;
    t[T_ID] = e_id[h];
    t[T_LAST] = e_lc[h];
    t[T_ROWS] = e_rows[h];
  }
  // the records nobody opened: the rest of this stream's, and a share of those past every stream's
  for (long k = (long)base + nseg + lane; k < (long)base + n_mine; k += FP_WAVE) p.seg[k * SEG_INTS + G_USED] = 0;
  for (long k = (long)n_streamed + (long)s * FP_WAVE + lane; k < n; k += (long)gridDim.x * FP_WAVE) p.seg[k * SEG_INTS + G_USED] = 0;
}

__global__ __launch_bounds__(256) void pool_accumulate_kernel(PoolArgs p) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (FP_WAVE - 1);
  const int D4 = p.D >> 2;
  const bool act = tid < D4;   // the other lanes of the last wave only help with the list
  const f32x4* emb = (const f32x4*)p.emb;
  f32x4* out = (f32x4*)p.o_emb;
  if (p.pass[b] != 0 && act) out[(long)b * D4 + tid] = emb[(long)b * D4 + tid];
  const int* g = p.seg + (long)b * SEG_INTS;
  if (g[G_USED] != 1) return;
  const long e = (long)g[G_STREAM] * POOL + g[G_ENT];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float wsum = 0.f;
  int rows = g[G_ROWS0];
  if (g[G_INIT] != 0) {
    if (act) acc = ((const f32x4*)p.tsum)[e * D4 + tid];
    wsum = p.tw[e];
  }
  for (int sg = b;;) {   // the entry's segments of the step, in order; all but the first start from a cleared entry
    const int k_first = g[G_KFIRST], k_last = g[G_KLAST];
    for (int k0 = k_first; k0 < k_last; k0 += FP_WAVE) {
      const int k = k0 + lane;
      int cd = -2, rw = 0;
      if (k < k_last) {
        cd = p.code[k];
        rw = p.ord[k];
      }
      unsigned long long m = __ballot((cd >> 1) == sg);
      while (m) {
        int r[PF], a[PF];
        f32x4 v[PF];
        float x[PF], w[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) {   // the loads of PF rows before the first add
          r[u] = -1;
          a[u] = 0;
          if (m) {
            const int bit = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            r[u] = __shfl(rw, bit);
            a[u] = __shfl(cd, bit) & 1;
            v[u] = act ? emb[(long)r[u] * D4 + tid] : f32x4{0.f, 0.f, 0.f, 0.f};
            x[u] = p.xinv[r[u]];
            w[u] = p.weight ? p.weight[r[u]] : 1.f;
          }
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
          if (r[u] < 0) continue;
          if (a[u]) {
            acc.x = tp_add(acc.x, v[u].x, x[u], w[u]);
            acc.y = tp_add(acc.y, v[u].y, x[u], w[u]);
            acc.z = tp_add(acc.z, v[u].z, x[u], w[u]);
            acc.w = tp_add(acc.w, v[u].w, x[u], w[u]);
            wsum = wsum + w[u];
            rows += 1;
          }
          if (act) out[(long)r[u] * D4 + tid] = rows > 0 ? acc : v[u];
        }
      }
    }
    sg = g[G_NEXT];
    if (sg < 0) break;
    g = p.seg + (long)sg * SEG_INTS;
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    wsum = 0.f;
    rows = 0;
  }
  if (act) ((f32x4*)p.tsum)[e * D4 + tid] = acc;
  if (tid == 0) p.tw[e] = wsum;
}

// ---------------------------------------------------------------------------------------------------------- the host twin
void emulate_pass(const PoolArgs& p, long i, int rows, int flags) {
  memcpy(p.o_emb + i * p.D, p.emb + i * p.D, sizeof(float) * p.D);
  p.o_rows[i] = rows;
  p.o_flags[i] = flags;
}

void emulate_row(const PoolArgs& p, int s, long i) {
  const int id = p.id[i], c = p.clock[i], D = p.D;
  if (id <= 0) {
    emulate_pass(p, i, 0, 0);
    return;
  }
  int* ti = p.ti + (long)s * POOL * TI;
  const bool is_new = (p.flags[i] & FP_TRACK_NEW) != 0;
  int ent = -1, oflags = 0;
  for (int e = 0; e < POOL && ent < 0; ++e)
    if (ti[e * TI + T_ID] == id) ent = e;
  bool take = ent >= 0 && is_new;
  if (ent < 0) {
    for (int e = 0; e < POOL && ent < 0; ++e)
      if (ti[e * TI + T_ID] == 0 || tp_stale(c, ti[e * TI + T_LAST], p.keep)) ent = e;
    if (ent < 0) {
      ent = 0;
      for (int e = 1; e < POOL; ++e)
        if (ti[e * TI + T_LAST] < ti[ent * TI + T_LAST]) ent = e;
      oflags |= FP_TRACK_TPL_EVICTED;
    }
    take = true;
    if (!is_new) oflags |= FP_TRACK_TPL_RESTART;
  }
  float* sum = p.tsum + ((long)s * POOL + ent) * D;
  float& wsum = p.tw[(long)s * POOL + ent];
  int* t = ti + ent * TI;
  if (take) {
    for (int j = 0; j < D; ++j) sum[j] = 0.f;
    wsum = 0.f;
    t[T_ID] = id;
    t[T_ROWS] = 0;
  }
  const float w = tp_weight(p.weight, i);
  if (w > 0.f) {
    for (int j = 0; j < D; ++j) sum[j] = tp_add(sum[j], p.emb[i * D + j], p.xinv[i], w);
    wsum = wsum + w;
    t[T_ROWS] += 1;
  }
  t[T_LAST] = c;
  if (t[T_ROWS] > 0) {
    memcpy(p.o_emb + i * D, sum, sizeof(float) * D);
    p.o_rows[i] = t[T_ROWS];
    p.o_flags[i] = oflags;
  } else {
    emulate_pass(p, i, 0, oflags);
  }
}

void emulate_step(const PoolArgs& p) {
  for (long i = 0; i < p.n; ++i)
    if (tp_stream(p, p.frame[i]) < 0) emulate_pass(p, i, 0, 0);
  for (int f = 0; f < p.B; ++f) {   // streams are independent: batch order is every stream's own order
    const int s = tp_stream(p, f);
    if (s < 0) continue;
    for (long i = 0; i < p.n; ++i)
      if (p.frame[i] == f) emulate_row(p, s, i);
  }
}

// ---------------------------------------------------------------------------------------------- arguments, checks, launch
int check_args(const PoolArgs& a) {
  if (!a.ti || !a.tw || !a.tsum) return FP_ERR_INVALID_ARG;   // a null struct gave three nulls
  if (a.S < 1 || a.D < 4 || a.D % 4 != 0 || a.D > FP_TRACK_MAX_DIM || a.n < 0 || a.n > FP_TRACK_MAX_ROWS || a.B < 0 || a.keep < 0)
    return FP_ERR_INVALID_ARG;
  if (a.B > 0 && !a.sof) return FP_ERR_INVALID_ARG;
  if (a.n > 0 && (!a.frame || !a.emb || !a.xinv || !a.id || !a.clock || !a.flags || !a.o_emb || !a.o_rows || !a.o_flags))
    return FP_ERR_INVALID_ARG;
  if (((uintptr_t)a.tsum | (uintptr_t)a.emb | (uintptr_t)a.o_emb) % 16 != 0) return FP_ERR_INVALID_ARG;   // float4 rows
  return FP_OK;
}

PoolArgs pool_args(const fp_track_templates* tpl, int n_streams, int D, const int32_t* frame, const float* emb, const float* xinv,
                   const float* weight, int n, const int32_t* stream_of_frame, int B, const int32_t* track_id,
                   const int32_t* track_clock, const int32_t* track_flags, int keep, float* track_emb, int32_t* track_emb_rows,
                   int32_t* track_emb_flags) {
  PoolArgs a;
  a.ti = tpl ? tpl->tpl_i : nullptr;
  a.tw = tpl ? tpl->tpl_w : nullptr;
  a.tsum = tpl ? tpl->tpl_sum : nullptr;
  a.S = n_streams; a.D = D;
  a.frame = frame; a.emb = emb; a.xinv = xinv; a.weight = weight; a.n = n;
  a.sof = stream_of_frame; a.B = B;
  a.id = track_id; a.clock = track_clock; a.flags = track_flags; a.keep = keep;
  a.o_emb = track_emb; a.o_rows = track_emb_rows; a.o_flags = track_emb_flags;
  a.ord = a.code = a.pass = a.seg = nullptr;
  return a;
}

}  // namespace

extern "C" {

size_t fp_track_pool_workspace_bytes(int n) {
  if (n < 0 || n > FP_TRACK_MAX_ROWS) return 0;
  return (size_t)n * (3 + SEG_INTS) * sizeof(int32_t) + 16;
}

int fp_track_pool_step(const fp_track_templates* tpl, int n_streams, int D, const int32_t* frame, const float* emb,
                       const float* xinv, const float* weight, int n, const int32_t* stream_of_frame, int B,
                       const int32_t* track_id, const int32_t* track_clock, const int32_t* track_flags, int keep, float* track_emb,
                       int32_t* track_emb_rows, int32_t* track_emb_flags, void* workspace, size_t workspace_bytes, void* stream) {
  PoolArgs a = pool_args(tpl, n_streams, D, frame, emb, xinv, weight, n, stream_of_frame, B, track_id, track_clock, track_flags,
                         keep, track_emb, track_emb_rows, track_emb_flags);
  const int rc = check_args(a);
  if (rc != FP_OK) return rc;
  if (n == 0) return FP_OK;   // no row, no change: a frame without rows moves nothing here
  if (!workspace || (uintptr_t)workspace % 4 != 0 || workspace_bytes < fp_track_pool_workspace_bytes(n)) return FP_ERR_INVALID_ARG;
  a.ord = (int*)workspace;
  a.code = a.ord + n;
  a.pass = a.code + n;
  a.seg = a.pass + n;
  hipLaunchKernelGGL(pool_directory_kernel, dim3((unsigned)a.S), dim3(FP_WAVE), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  const unsigned threads = (unsigned)fp_round_up(D / 4, FP_WAVE);
  hipLaunchKernelGGL(pool_accumulate_kernel, dim3((unsigned)n), dim3(threads), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_track_pool_step_emulate(const fp_track_templates* tpl, int n_streams, int D, const int32_t* frame, const float* emb,
                               const float* xinv, const float* weight, int n, const int32_t* stream_of_frame, int B,
                               const int32_t* track_id, const int32_t* track_clock, const int32_t* track_flags, int keep,
                               float* track_emb, int32_t* track_emb_rows, int32_t* track_emb_flags) {
  const PoolArgs a = pool_args(tpl, n_streams, D, frame, emb, xinv, weight, n, stream_of_frame, B, track_id, track_clock,
                               track_flags, keep, track_emb, track_emb_rows, track_emb_flags);
  const int rc = check_args(a);
  if (rc != FP_OK) return rc;
  if (n == 0) return FP_OK;
  emulate_step(a);
  return FP_OK;
}

}  // extern "C"
