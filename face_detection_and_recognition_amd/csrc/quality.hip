// quality.hip — fp_face_quality / fp_face_pose and their host twins (include/facepath.h "Face crop quality", DESIGN §7
// "Face quality"): integer luma statistics and the variance of a block-mean Laplacian per face rectangle, read from the u8 BGR
// frames at native resolution, dense or ragged (gfx950); a pose record from the five landmarks.
//
// fp_face_quality: one workgroup of 256 threads per face.  The clamped rectangle is cut into bw x bh blocks of s x s pixels
// (s = ceil(max(sw, sh) / 112), so bw, bh <= 112) and the workgroup marches down it.  A thread is (rp, j) = (tid / bw,
// tid % bw) with RP = 256 / bw row phases: it reads the s pixels of block column j in a pixel row -- 3 s consecutive bytes,
// the lanes of a wave next to each other, so a wave's loads cover one contiguous run of the frame row -- and keeps the sum of
// their luma.  A step covers G = max(1, RP / s) block rows:
//   s >= RP: one block row; thread (rp, j) takes its pixel rows rp, rp + RP, ... and sums them in a register;
//   s <  RP: G block rows of s pixel rows, one pixel row per thread (faces up to 112 px have s = 1: without this only bw of the
//            256 threads would load at a time).
// The partial sums meet in LDS (part[rp][j]); thread (g, j) adds the row phases of block (i0 + g, j) in ascending order into
// the block-sum rows: the two block rows before the step and the G new ones (the issue's three-row ring, G + 2 rows deep).
// The Laplacian is taken on every row of that window that has both neighbours, then the last two rows move to the front.
// Every lane keeps 64-bit integer accumulators; they are reduced within a wave by shuffles, across the four waves through
// LDS, and thread 0 stores the row.  No atomics and no floating point: the result does not depend on the order of anything.
//
// Occupancy: 256 threads, ~4 KB of LDS and few VGPRs per workgroup, so eight workgroups (8 waves per SIMD) fit a CU.  The
// kernel is a chain of dependent byte loads with two barriers a step and nearly no arithmetic; what hides the load latency is
// other workgroups (other faces) on the same CU, so the aim is simply the full 8 waves per SIMD, which __launch_bounds__(256)
// allows (<= 64 VGPRs per lane at 8 waves; 60 are used).  Measured rates and what was not tried (dword loads staged through
// LDS as draw.hip does): FINDINGS 75.
//
// Bounds: a rectangle is clamped to its frame and a frame is used only when its descriptor lies inside frames_bytes
// (frame_ok), so every load is inside the buffer whatever the items and descriptors hold.
#include "common.h"

namespace {

constexpr int NT = 256;                       // threads per workgroup
constexpr int SIDE = 112;                     // most blocks a side
constexpr int BUF = NT + 2 * SIDE;            // block sums of a step's window: (G + 2) * bw <= RP * bw + 2 * bw

__host__ __device__ inline int luma(const uint8_t* p) {
  return (1868 * (int)p[0] + 9617 * (int)p[1] + 4899 * (int)p[2] + 8192) >> 14;
}

// A frame the ragged kernels take, lying inside the buffer.
__host__ __device__ inline bool frame_ok(const fp_frame_desc& d, size_t frames_bytes) {
  if (d.w < FP_FRAME_MIN_W || d.w > FP_FRAME_MAX_W || d.h < 1 || d.h > FP_FRAME_MAX_H || d.off < 0) return false;
  const unsigned long long bytes = 3ull * (unsigned long long)d.w * (unsigned long long)d.h;
  return (unsigned long long)d.off <= (unsigned long long)frames_bytes && bytes <= (unsigned long long)frames_bytes - (unsigned long long)d.off;
}

struct Geom {
  int flags;
  int x0, y0;        // the clamped rectangle's corner
  int s, bw, bh;     // decimation step, blocks across and down
  long off, w3;      // the frame's byte offset and row pitch
};

// The rectangle of item `it`, clamped, and its blocks.  flags with EMPTY / BAD_FRAME / TOO_LARGE: nothing is loaded.
__host__ __device__ inline Geom quality_geom(const fp_resize_item& it, const fp_frame_desc* descs, int n_frames,
                                             size_t frames_bytes) {
  Geom g{};
  if (it.src_image < 0 || it.src_image >= n_frames) { g.flags = FP_QUALITY_BAD_FRAME; return g; }
  const fp_frame_desc d = descs[it.src_image];
  if (!frame_ok(d, frames_bytes)) { g.flags = FP_QUALITY_BAD_FRAME; return g; }
  const long long xe = (long long)it.sx + it.sw, ye = (long long)it.sy + it.sh;
  const int x0 = it.sx > 0 ? it.sx : 0, y0 = it.sy > 0 ? it.sy : 0;
  const int x1 = xe < d.w ? (int)xe : d.w, y1 = ye < d.h ? (int)ye : d.h;
  if (it.sw <= 0 || it.sh <= 0 || x0 >= x1 || y0 >= y1) { g.flags = FP_QUALITY_EMPTY; return g; }
  const int sw = x1 - x0, sh = y1 - y0, m = sw > sh ? sw : sh;
  g.s = (m + SIDE - 1) / SIDE;
  if (g.s > FP_QUALITY_MAX_STEP) { g.flags = FP_QUALITY_TOO_LARGE; return g; }
  g.x0 = x0; g.y0 = y0;
  g.bw = sw / g.s; g.bh = sh / g.s;
  g.off = (long)d.off; g.w3 = 3L * d.w;
  if (g.bw < 3 || g.bh < 3) g.flags = FP_QUALITY_NO_LAPLACIAN;
  return g;
}

__host__ __device__ inline int lap5(int up, int down, int left, int right, int mid) { return up + down + left + right - 4 * mid; }

__device__ __forceinline__ long long wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(NT) void face_quality_kernel(const uint8_t* __restrict__ frames, size_t frames_bytes,
                                                          const fp_frame_desc* __restrict__ descs, int n_frames,
                                                          const fp_resize_item* __restrict__ items, long long* __restrict__ stats,
                                                          int* __restrict__ flags) {
  __shared__ int part[NT];               // [rp][j], rp < RP, j < bw: RP * bw <= 256
  __shared__ int blk[BUF];               // [slot][j]: slots 0, 1 = the two block rows before the step, 2 .. = the step's
  __shared__ long long red[4][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int face = blockIdx.x;
  const Geom g = quality_geom(items[face], descs, n_frames, frames_bytes);     // uniform over the workgroup
  long long* out = stats + 8L * face;
  if (g.flags & (FP_QUALITY_BAD_FRAME | FP_QUALITY_EMPTY | FP_QUALITY_TOO_LARGE) || g.bw < 1 || g.bh < 1) {
    if (tid < 8) out[tid] = 0;
    if (tid == 0) flags[face] = g.flags;
    return;
  }
  const int s = g.s, bw = g.bw, bh = g.bh;
  const int RP = NT / bw;                          // >= 2
  const int G = RP / s > 1 ? RP / s : 1;           // block rows a step
  // loading: row phase rp of block column j (the threads past RP * bw have rp >= RP and load nothing);
  // reducing: block (i0 + rp, j) of the step, for rp < G (G <= RP)
  const int rp = tid / bw, j = tid - rp * bw;
  const uint8_t* base = frames + g.off + (long)g.y0 * g.w3 + 3L * g.x0 + 3L * j * s;
  const bool lapl = bw >= 3 && bh >= 3;

  long long sum_y = 0, sum_y2 = 0, n_dark = 0, n_bright = 0, sum_lap = 0, sum_lap2 = 0;
  for (int i0 = 0; i0 < bh; i0 += G) {
    const int gs = bh - i0 < G ? bh - i0 : G;      // block rows of this step
    unsigned acc = 0, y2 = 0, nd = 0, nb = 0;      // y2 <= 64 * 64 * 65025 < 2^32 a step
    if (rp < RP) {
      for (int pr = rp; pr < gs * s; pr += RP) {
        const uint8_t* p = base + (long)(i0 * s + pr) * g.w3;
        for (int k = 0; k < s; ++k, p += 3) {
          const int y = luma(p);
          acc += y; y2 += y * y;
          nd += y <= 16; nb += y >= 239;
        }
      }
      part[tid] = (int)acc;                        // tid = rp * bw + j
    }
    sum_y2 += y2; n_dark += nd; n_bright += nb;
    __syncthreads();                               // part; the shift of the step before
    if (rp < gs) {
      const int lo = rp * s, hi = lo + s < RP ? lo + s : RP;      // G > 1: the block row's s phases; G = 1: all RP of them
      int b = 0;
      for (int r = lo; r < hi; ++r) b += part[r * bw + j];
      blk[(2 + rp) * bw + j] = b;
      sum_y += b;
    }
    __syncthreads();                               // blk
    if (lapl) {
      // centres: the block rows c with i0 - 1 <= c <= i0 + gs - 2 and 1 <= c <= bh - 2; slot of row c = c - i0 + 2
      const int c_lo = i0 - 1 > 1 ? i0 - 1 : 1, c_hi = i0 + gs - 2 < bh - 2 ? i0 + gs - 2 : bh - 2;
      const int nc = c_hi - c_lo + 1, iw = bw - 2;
      for (int e = tid; e < nc * iw; e += NT) {
        const int cr = e / iw, cj = 1 + (e - cr * iw);
        const int* m = blk + (c_lo + cr - i0 + 2) * bw + cj;
        const int l = lap5(m[-bw], m[bw], m[-1], m[1], m[0]);
        sum_lap += l;
        sum_lap2 += (long long)l * l;
      }
      __syncthreads();                             // the Laplacian's reads before the shift
      if (tid < bw) {                              // one thread per column: reads and writes of a column do not cross
        const int a = blk[gs * bw + tid], b = blk[(gs + 1) * bw + tid];
        blk[tid] = a;
        blk[bw + tid] = b;
      }
    }
  }
  long long v[6] = {sum_y, sum_y2, n_dark, n_bright, sum_lap, sum_lap2};
  for (int k = 0; k < 6; ++k) {
    v[k] = wave_sum(v[k]);
    if (lane == 0) red[wave][k] = v[k];
  }
  __syncthreads();
  if (tid == 0) {
    long long t[6];
    for (int k = 0; k < 6; ++k) t[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    out[0] = (long long)bw * s * bh * s;
    out[1] = t[0]; out[2] = t[1]; out[3] = t[2]; out[4] = t[3];
    out[5] = lapl ? (long long)(bw - 2) * (bh - 2) : 0;
    out[6] = t[4]; out[7] = t[5];
    flags[face] = g.flags;
  }
}

// The same definitions, one face, serially.
void quality_one(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const fp_resize_item& it,
                 int64_t* out, int32_t* flag) {
  const Geom g = quality_geom(it, descs, n_frames, frames_bytes);
  for (int k = 0; k < 8; ++k) out[k] = 0;
  *flag = g.flags;
  if (g.flags & (FP_QUALITY_BAD_FRAME | FP_QUALITY_EMPTY | FP_QUALITY_TOO_LARGE) || g.bw < 1 || g.bh < 1) return;
  const int s = g.s, bw = g.bw, bh = g.bh;
  int ring[3][SIDE];
  const bool lapl = bw >= 3 && bh >= 3;
  for (int i = 0; i < bh; ++i) {
    int* row = ring[i % 3];
    for (int j = 0; j < bw; ++j) {
      int b = 0;
      for (int r = 0; r < s; ++r) {
        const uint8_t* p = frames + g.off + (long)(g.y0 + i * s + r) * g.w3 + 3L * (g.x0 + j * s);
        for (int k = 0; k < s; ++k, p += 3) {
          const int y = luma(p);
          b += y;
          out[2] += y * y;
          out[3] += y <= 16;
          out[4] += y >= 239;
        }
      }
      row[j] = b;
      out[1] += b;
    }
    if (lapl && i >= 2) {
      const int *up = ring[(i - 2) % 3], *mid = ring[(i - 1) % 3];
      for (int j = 1; j < bw - 1; ++j) {
        const int l = lap5(up[j], row[j], mid[j - 1], mid[j + 1], mid[j]);
        out[6] += l;
        out[7] += (int64_t)l * l;
      }
    }
  }
  out[0] = (int64_t)bw * s * bh * s;
  out[5] = lapl ? (int64_t)(bw - 2) * (bh - 2) : 0;
}

// iod, roll, yaw, pitch of one face's landmarks; fp32, + - * / and sqrtf only, every difference taken from the left eye first
// (the coordinates may be large, the differences are not).  Returns FP_QUALITY_POSE_DEGENERATE or 0.
__host__ __device__ inline int pose_one(const float* lm, int fmt, float* o) {
  const float lx = lm[0], ly = lm[1];
  const float ex = lm[2] - lx, ey = lm[3] - ly;          // the eye axis
  const float nx = lm[4] - lx, ny = lm[5] - ly;          // nose
  float mx = lm[6] - lx, my = lm[7] - ly;                // mouth: fmt 0 its centre, else the midpoint of its corners
  if (fmt != 0) {
    mx = (mx + (lm[8] - lx)) * 0.5f;
    my = (my + (lm[9] - ly)) * 0.5f;
  }
  const float iod2 = ex * ex + ey * ey;
  const float iod = sqrtf(iod2);
  // from the eyes' midpoint, against v = the eye axis turned by +90 degrees = (-ey, ex)
  const float hx = ex * 0.5f, hy = ey * 0.5f;
  const float pn = (ny - hy) * ex - (nx - hx) * ey;
  const float pd = (my - hy) * ex - (mx - hx) * ey;
  if (!(iod >= 1.f) || !(pd > 0.f)) {
    o[0] = o[1] = o[2] = o[3] = 0.f;
    return FP_QUALITY_POSE_DEGENERATE;
  }
  const float t = (nx * ex + ny * ey) / iod2;
  o[0] = iod;
  o[1] = ey / iod;
  o[2] = 2.f * t - 1.f;
  o[3] = pn / pd;
  return 0;
}

__global__ __launch_bounds__(NT) void face_pose_kernel(const float* __restrict__ lmarks, int fmt, int n, float* __restrict__ out,
                                                       int* __restrict__ flags) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  float lm[10], o[4];
  for (int k = 0; k < 10; ++k) lm[k] = lmarks[10L * i + k];
  const int f = pose_one(lm, fmt, o);
  for (int k = 0; k < 4; ++k) out[4L * i + k] = o[k];
  if (f) flags[i] |= f;
}

}  // namespace

extern "C" {

int fp_face_quality(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames,
                    const fp_resize_item* items, int n, int64_t* stats, int32_t* flags, void* stream) {
  if (n < 0 || n_frames < 0) return FP_ERR_INVALID_ARG;
  if (!frames || !descs || !items || !stats || !flags) return FP_ERR_INVALID_ARG;
  if (n == 0) return FP_OK;
  hipLaunchKernelGGL(face_quality_kernel, dim3((unsigned)n), dim3(NT), 0, (hipStream_t)stream, frames, frames_bytes, descs,
                     n_frames, items, (long long*)stats, (int*)flags);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_face_quality_emulate(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames,
                            const fp_resize_item* items, int n, int64_t* stats, int32_t* flags) {
  if (n < 0 || n_frames < 0) return FP_ERR_INVALID_ARG;
  if (!frames || !descs || !items || !stats || !flags) return FP_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i) quality_one(frames, frames_bytes, descs, n_frames, items[i], stats + 8L * i, flags + i);
  return FP_OK;
}

int fp_face_pose(const float* lmarks, int fmt, int n, float* out, int32_t* flags, void* stream) {
  if (n < 0 || fmt < 0 || fmt > 2) return FP_ERR_INVALID_ARG;
  if (!lmarks || !out || !flags) return FP_ERR_INVALID_ARG;
  if (n == 0) return FP_OK;
  hipLaunchKernelGGL(face_pose_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, lmarks, fmt, n, out,
                     (int*)flags);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_face_pose_emulate(const float* lmarks, int fmt, int n, float* out, int32_t* flags) {
  if (n < 0 || fmt < 0 || fmt > 2) return FP_ERR_INVALID_ARG;
  if (!lmarks || !out || !flags) return FP_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i) flags[i] |= pose_one(lmarks + 10L * i, fmt, out + 4L * i);
  return FP_OK;
}

}  // extern "C"
