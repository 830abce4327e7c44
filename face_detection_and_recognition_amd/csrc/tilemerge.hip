// tilemerge.hip — tiled detection (gfx950): cut frames into tile images, and merge the detections of every view of a frame
// (its tiles and the whole frame) into one block of rows in the frame's own pixels.  Build-defined, no reference counterpart
// (DESIGN §7 "Tiled detection"; include/facepath.h states the procedure).  Build with -ffp-contract=off: the numpy
// restatement (tiling.py merge_views_numpy) and the host emulator must reproduce the device's rows bit for bit.
//
// 1. fp_merge_views: one workgroup per frame.  Every row of every view is mapped to frame pixels and tested (cut by an
//    interior view edge, not finite, empty) by one lane; boxes (32 KB) and 64-bit keys (16 KB: ~score << 32 | candidate
//    index, so an ascending sort is score descending, then view, then row) live in LDS.  A bitonic sort of the keys, then
//    wave 0 walks them 64 at a time: every lane tests its candidate against all boxes kept so far (broadcast LDS reads),
//    then the batch is resolved in order with a ballot per survivor.  The kept keys overwrite the head of the key array
//    (a kept position never passes the read position).  Rows are written in walk order, landmarks recomputed from the
//    detector's row.  No global atomics, no scratch: two runs are bit-identical.
// 2. fp_merge_views_emulate: the same __host__ __device__ code run serially on host memory (std::sort for the keys: the
//    order is total, so the result is the same).
// 3. fp_gather_tiles: a byte copy, one lane per 16 / 4 / 1 destination bytes (the widest the tile's row pitch keeps aligned),
//    source loads unaligned.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int CAP = FP_MERGE_CAP;
constexpr unsigned long long KEY_NONE = ~0ull;
static_assert((CAP & (CAP - 1)) == 0, "the candidate index is the low bits of a key");

struct MergeArgs {
  const float* dets;
  const int* counts;
  int S, max_dets, row, fmt, in_w, in_h;
  const fp_tile_view* views;
  const int* view_start;
  const fp_frame_desc* descs;
  int B;
  float merge_thr, edge_px;
  int max_out;
  float* out;
  int* out_counts;
  int* overflow;
};

struct Box {
  float x1, y1, x2, y2;
};

__host__ __device__ __forceinline__ bool finite_f(float v) { return v - v == 0.f; }

__host__ __device__ __forceinline__ int view_rows(const MergeArgs& p, int s) { return min(max(p.counts[s], 0), p.max_dets); }

// Views [lo, hi) of frame f, whatever view_start holds.
__host__ __device__ __forceinline__ void view_range(const MergeArgs& p, int f, int& lo, int& hi) {
  lo = min(max(p.view_start[f], 0), p.S);
  hi = min(max(p.view_start[f + 1], lo), p.S);
}

__host__ __device__ __forceinline__ const float* view_row(const MergeArgs& p, int s, int r) {
  return p.dets + ((long)s * p.max_dets + r) * p.row;
}

// The score as the order sees it (-0 is +0).
__host__ __device__ __forceinline__ float row_score(const MergeArgs& p, const float* d) {
  const float sc = p.fmt == 0 ? d[16] : d[4];
  return sc == 0.f ? 0.f : sc;
}

// Steps 1 - 5 of the procedure for one row d of view v in a W x H frame: false = no candidate.
__host__ __device__ __forceinline__ bool merge_candidate(const MergeArgs& p, const fp_tile_view& v, int W, int H, const float* d,
                                                         Box& b, float& score) {
  float x1, y1, x2, y2;
  score = row_score(p, d);
  if (p.fmt == 0) {
    x1 = d[1] * (float)p.in_w; y1 = d[0] * (float)p.in_h; x2 = d[3] * (float)p.in_w; y2 = d[2] * (float)p.in_h;
  } else {
    x1 = d[0]; y1 = d[1]; x2 = d[2]; y2 = d[3];
  }
  x1 = (x1 - v.pad_x) / v.gain; x2 = (x2 - v.pad_x) / v.gain;
  y1 = (y1 - v.pad_y) / v.gain; y2 = (y2 - v.pad_y) / v.gain;
  if (!(finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2) && finite_f(score))) return false;
  const float vw = (float)v.vw, vh = (float)v.vh;
  if (p.edge_px >= 0.f) {   // cut by an interior edge of the view
    if (v.x0 > 0 && x1 <= p.edge_px) return false;
    if ((long)v.x0 + v.vw < W && x2 >= vw - p.edge_px) return false;
    if (v.y0 > 0 && y1 <= p.edge_px) return false;
    if ((long)v.y0 + v.vh < H && y2 >= vh - p.edge_px) return false;
  }
  x1 = fminf(fmaxf(x1, 0.f), vw); x2 = fminf(fmaxf(x2, 0.f), vw);
  y1 = fminf(fmaxf(y1, 0.f), vh); y2 = fminf(fmaxf(y2, 0.f), vh);
  b.x1 = x1 + (float)v.x0; b.x2 = x2 + (float)v.x0;
  b.y1 = y1 + (float)v.y0; b.y2 = y2 + (float)v.y0;
  return b.x2 > b.x1 && b.y2 > b.y1;
}

// ascending keys = score descending, then candidate index (view, then row) ascending; KEY_NONE is no key of a finite score
__host__ __device__ __forceinline__ unsigned long long merge_key(float score, int slot) {
  unsigned u;
  __builtin_memcpy(&u, &score, 4);
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)(~ord) << 32) | (unsigned)slot;
}

__host__ __device__ __forceinline__ float box_area(const Box& b) { return (b.x2 - b.x1) * (b.y2 - b.y1); }

// step 7: does the kept box k remove the candidate c
__host__ __device__ __forceinline__ bool suppresses(const Box& k, const Box& c, float area_c, float thr) {
  const float iw = fmaxf(fminf(k.x2, c.x2) - fmaxf(k.x1, c.x1), 0.f);
  const float ih = fmaxf(fminf(k.y2, c.y2) - fmaxf(k.y1, c.y1), 0.f);
  const float inter = iw * ih;
  return inter > thr * fminf(box_area(k), area_c);
}

// candidate index -> its view and row (the first CAP rows of the frame's views in order)
__host__ __device__ __forceinline__ void locate(const MergeArgs& p, int lo, int hi, int slot, int& s, int& r) {
  int base = 0;
  for (s = lo; s < hi; ++s) {
    const int n = view_rows(p, s);
    if (slot < base + n) break;
    base += n;
  }
  r = slot - base;
}

// one output row: the box, the landmarks through the same map (unclamped, unrounded), the score
__host__ __device__ __forceinline__ void merge_emit(const MergeArgs& p, const fp_tile_view& v, const float* d, const Box& b,
                                                    float* o) {
  o[0] = b.x1; o[1] = b.y1; o[2] = b.x2; o[3] = b.y2;
  for (int i = 0; i < 5; ++i) {
    float x, y;
    if (p.fmt == 0) {   // keypoints 0 .. 3 (eyes, nose, mouth centre); the mouth centre fills both mouth slots
      const int k = min(i, 3);
      x = d[4 + 2 * k] * (float)p.in_w;
      y = d[5 + 2 * k] * (float)p.in_h;
    } else {
      x = d[5 + 2 * i];
      y = d[6 + 2 * i];
    }
    o[4 + 2 * i] = (x - v.pad_x) / v.gain + (float)v.x0;
    o[5 + 2 * i] = (y - v.pad_y) / v.gain + (float)v.y0;
  }
  o[14] = row_score(p, d);
  o[15] = 0.f;
}

__host__ __device__ __forceinline__ void merge_write(const MergeArgs& p, int f, int lo, int hi, int j, int slot, const Box& b) {
  int s, r;
  locate(p, lo, hi, slot, s, r);
  merge_emit(p, p.views[s], view_row(p, s, r), b, p.out + ((long)f * p.max_out + j) * 16);
}

__global__ __launch_bounds__(256) void merge_views_kernel(MergeArgs p) {
  __shared__ Box box[CAP];
  __shared__ unsigned long long key[CAP];
  __shared__ int kept_s;
  const int f = blockIdx.x, tid = threadIdx.x;
  const fp_frame_desc fd = p.descs[f];
  int lo, hi;
  view_range(p, f, lo, hi);

  // candidates: the first CAP rows of the frame's views
  int base = 0;
  bool more = false;
  for (int s = lo; s < hi; ++s) {
    const int n = view_rows(p, s), take = min(n, CAP - base);
    more |= n > take;
    if (take > 0) {
      const fp_tile_view v = p.views[s];
      for (int r = tid; r < take; r += 256) {
        Box b{0.f, 0.f, 0.f, 0.f};
        float sc;
        const bool ok = merge_candidate(p, v, fd.w, fd.h, view_row(p, s, r), b, sc);
        box[base + r] = b;
        key[base + r] = ok ? merge_key(sc, base + r) : KEY_NONE;
      }
    }
    base += take;
  }
  int n_sort = 2;
  while (n_sort < base) n_sort <<= 1;
  for (int i = base + tid; i < n_sort; i += 256) key[i] = KEY_NONE;
  __syncthreads();

  for (int k = 2; k <= n_sort; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n_sort >> 1); t += 256) {
        const int i = 2 * t - (t & (j - 1)), q = i + j;
        const unsigned long long a = key[i], b = key[q];
        if ((a > b) == ((i & k) == 0)) {
          key[i] = b;
          key[q] = a;
        }
      }
      __syncthreads();
    }

  int n_valid = 0;   // the keys in front of the first KEY_NONE
  for (int step = n_sort; step > 0; step >>= 1)
    if (n_valid + step <= n_sort && key[n_valid + step - 1] != KEY_NONE) n_valid += step;
  __syncthreads();

  if (tid < FP_WAVE) {
    int kept = 0;
    for (int i0 = 0; i0 < n_valid; i0 += FP_WAVE) {
      const int i = i0 + tid;
      const bool have = i < n_valid;
      const unsigned long long kk = have ? key[i] : KEY_NONE;
      const Box c = box[(unsigned)kk & (CAP - 1)];
      const float area_c = box_area(c);
      bool alive = have;
      for (int k = 0; k < kept; ++k)   // the same address in every lane: LDS broadcast
        if (suppresses(box[(unsigned)key[k] & (CAP - 1)], c, area_c, p.merge_thr)) alive = false;
      unsigned long long live = __ballot(alive);
      while (live) {
        const int l = __ffsll((long long)live) - 1;   // the first candidate of the batch still alive is kept
        Box kb;
        kb.x1 = __shfl(c.x1, l); kb.y1 = __shfl(c.y1, l); kb.x2 = __shfl(c.x2, l); kb.y2 = __shfl(c.y2, l);
        if (tid == l) key[kept] = kk;                 // kept <= i0 + l: behind every key still to be read
        if (tid > l && alive && suppresses(kb, c, area_c, p.merge_thr)) alive = false;
        ++kept;
        live = __ballot(alive) & ~((2ull << l) - 1ull);
      }
      __threadfence_block();   // the keys this batch kept are read by other lanes in the next one
    }
    if (tid == 0) kept_s = kept;
  }
  __syncthreads();

  const int kept = kept_s, n_out = min(kept, p.max_out);
  for (int j = tid; j < n_out; j += 256) {
    const int slot = (int)((unsigned)key[j] & (CAP - 1));
    merge_write(p, f, lo, hi, j, slot, box[slot]);
  }
  if (tid == 0) {
    p.out_counts[f] = n_out;
    p.overflow[f] |= (more ? 2 : 0) | (kept > p.max_out ? 4 : 0);
  }
}

int check_merge(const MergeArgs& a) {
  if (!a.dets || !a.counts || !a.views || !a.view_start || !a.descs || !a.out || !a.out_counts || !a.overflow)
    return FP_ERR_INVALID_ARG;
  if (a.B < 0 || a.S < 0 || a.max_dets < 1 || a.max_out < 1 || a.in_w < 1 || a.in_h < 1) return FP_ERR_INVALID_ARG;
  if (a.fmt != 0 && a.fmt != 1) return FP_ERR_INVALID_ARG;
  if (a.row < (a.fmt == 0 ? 17 : 15)) return FP_ERR_INVALID_ARG;
  if (a.merge_thr != a.merge_thr) return FP_ERR_INVALID_ARG;
  return FP_OK;
}

MergeArgs merge_args(const float* dets, const int32_t* counts, int S, int max_dets, int row_floats, int fmt, int in_w, int in_h,
                     const fp_tile_view* views, const int32_t* view_start, const fp_frame_desc* descs, int B, float merge_thr,
                     float edge_px, int max_out, float* out, int32_t* out_counts, int32_t* overflow) {
  return MergeArgs{dets, counts, S, max_dets, row_floats, fmt, in_w, in_h, views, view_start, descs, B, merge_thr, edge_px,
                   max_out, out, out_counts, overflow};
}

// ------------------------------------------------------------------------------------------------ gather
struct GatherArgs {
  const uint8_t* frames;
  uint64_t frames_bytes;
  const fp_frame_desc* descs;
  int n_frames;
  const fp_tile_view* views;
  int S, tw, th;
  uint8_t* out;
  int cpr;   // chunks of CB bytes per tile row
};

// One lane per chunk of CB destination bytes of a tile row; a chunk inside the copied part of its row is one load and one
// store of CB bytes (the source unaligned), any other chunk goes byte by byte (frame bytes, then the pad value).
template <int CB>
__global__ __launch_bounds__(256) void gather_tiles_kernel(GatherArgs p) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= p.th * p.cpr) return;
  const int y = q / p.cpr, b0 = (q - y * p.cpr) * CB, b1 = min(b0 + CB, p.tw * 3);
  for (int s = blockIdx.y; s < p.S; s += gridDim.y) {
    const fp_tile_view v = p.views[s];
    const uint8_t* src = nullptr;
    int cw = 0, ch = 0;   // the part of the tile that holds frame pixels
    if (v.frame >= 0 && v.frame < p.n_frames) {
      const fp_frame_desc d = p.descs[v.frame];
      if (d.off >= 0 && d.h >= 1 && d.h <= FP_FRAME_MAX_H && d.w >= 1 && d.w <= FP_FRAME_MAX_W &&
          (uint64_t)d.off + (uint64_t)d.h * (uint64_t)d.w * 3u <= p.frames_bytes && v.x0 >= 0 && v.y0 >= 0 && v.x0 < d.w &&
          v.y0 < d.h) {
        cw = max(min(min(v.vw, d.w - v.x0), p.tw), 0);
        ch = max(min(min(v.vh, d.h - v.y0), p.th), 0);
        src = p.frames + d.off + ((long)(v.y0 + y) * d.w + v.x0) * 3;
      }
    }
    uint8_t* dst = p.out + ((long)s * p.th + y) * p.tw * 3;
    const int nb = y < ch ? cw * 3 : 0;   // bytes of this row that come from the frame
    bool wide = false;
    if constexpr (CB > 1) {
      if (b1 - b0 == CB && b1 <= nb) {
        typedef unsigned chunk_t __attribute__((ext_vector_type(CB / 4)));
        chunk_t w;
        __builtin_memcpy(&w, src + b0, CB);
        *(chunk_t*)(dst + b0) = w;
        wide = true;
      }
    }
    if (!wide)
      for (int b = b0; b < b1; ++b) dst[b] = b < nb ? src[b] : (uint8_t)125;
  }
}

}  // namespace

extern "C" {

int fp_merge_views(const float* dets, const int32_t* counts, int S, int max_dets, int row_floats, int fmt, int in_w, int in_h,
                   const fp_tile_view* views, const int32_t* view_start, const fp_frame_desc* descs, int B, float merge_thr,
                   float edge_px, int max_out, float* out, int32_t* out_counts, int32_t* overflow, void* stream) {
  const MergeArgs a = merge_args(dets, counts, S, max_dets, row_floats, fmt, in_w, in_h, views, view_start, descs, B, merge_thr,
                                 edge_px, max_out, out, out_counts, overflow);
  const int rc = check_merge(a);
  if (rc != FP_OK || B == 0) return rc;
  hipLaunchKernelGGL(merge_views_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_merge_views_emulate(const float* dets, const int32_t* counts, int S, int max_dets, int row_floats, int fmt, int in_w,
                           int in_h, const fp_tile_view* views, const int32_t* view_start, const fp_frame_desc* descs, int B,
                           float merge_thr, float edge_px, int max_out, float* out, int32_t* out_counts, int32_t* overflow) {
  const MergeArgs p = merge_args(dets, counts, S, max_dets, row_floats, fmt, in_w, in_h, views, view_start, descs, B, merge_thr,
                                 edge_px, max_out, out, out_counts, overflow);
  const int rc = check_merge(p);
  if (rc != FP_OK) return rc;
  std::vector<Box> box(CAP);
  std::vector<unsigned long long> key;
  for (int f = 0; f < B; ++f) {
    int lo, hi;
    view_range(p, f, lo, hi);
    int base = 0;
    bool more = false;
    key.clear();
    for (int s = lo; s < hi; ++s) {
      const int n = view_rows(p, s), take = min(n, CAP - base);
      more |= n > take;
      for (int r = 0; r < take; ++r) {
        Box b{0.f, 0.f, 0.f, 0.f};
        float sc;
        if (merge_candidate(p, p.views[s], descs[f].w, descs[f].h, view_row(p, s, r), b, sc)) key.push_back(merge_key(sc, base + r));
        box[base + r] = b;
      }
      base += take;
    }
    std::sort(key.begin(), key.end());
    int kept = 0;
    for (size_t i = 0; i < key.size(); ++i) {
      const Box& c = box[(unsigned)key[i] & (CAP - 1)];
      const float area_c = box_area(c);
      bool alive = true;
      for (int k = 0; k < kept && alive; ++k)
        if (suppresses(box[(unsigned)key[k] & (CAP - 1)], c, area_c, merge_thr)) alive = false;
      if (alive) key[kept++] = key[i];
    }
    const int n_out = min(kept, max_out);
    for (int j = 0; j < n_out; ++j) {
      const int slot = (int)((unsigned)key[j] & (CAP - 1));
      merge_write(p, f, lo, hi, j, slot, box[slot]);
    }
    out_counts[f] = n_out;
    overflow[f] |= (more ? 2 : 0) | (kept > max_out ? 4 : 0);
  }
  return FP_OK;
}

int fp_gather_tiles(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames,
                    const fp_tile_view* views, int S, int tile_w, int tile_h, uint8_t* out, void* stream) {
  if (!frames || !descs || !views || !out) return FP_ERR_INVALID_ARG;
  if (n_frames < 1 || S < 0 || tile_w < 1 || tile_h < 1 || tile_w > FP_FRAME_MAX_W || tile_h > FP_FRAME_MAX_H)
    return FP_ERR_INVALID_ARG;
  if (S == 0) return FP_OK;
  GatherArgs a{frames, (uint64_t)frames_bytes, descs, n_frames, views, S, tile_w, tile_h, out, 0};
  const int row_bytes = tile_w * 3;
  const int cb = (row_bytes % 16 == 0 && ((uintptr_t)out) % 16 == 0) ? 16 : (row_bytes % 4 == 0 && ((uintptr_t)out) % 4 == 0) ? 4 : 1;
  a.cpr = row_bytes / cb;
  if ((long)tile_h * a.cpr >= (1L << 31) - 256) return FP_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)fp_ceil_div((long)tile_h * a.cpr, 256), (unsigned)min(S, 65535));
  if (cb == 16) hipLaunchKernelGGL(gather_tiles_kernel<16>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (cb == 4) hipLaunchKernelGGL(gather_tiles_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(gather_tiles_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
