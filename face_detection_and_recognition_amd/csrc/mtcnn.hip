// mtcnn.hip — the glue of the MTCNN cascade on the device (include/facepath.h section 9): candidate ordering, box
// generation, the "+1" greedy NMS (union / min) per level and per frame, regress / square / truncate, the zero-padded cut +
// area resize to 24 / 48, landmark mapping and the compaction between the stages.  One workgroup of 256 lanes per frame (per
// crop pixel block in fp_mtcnn_cut).  Box arithmetic is fp64 (a handful of boxes per frame; it then equals the float64
// restatement on the same inputs); the IoU is fp32 and this file is compiled without fma contraction, as post.hip is.
//
// Order.  Every list a step consumes is first put into an order that does not depend on how it was produced: a rank sort
// (rank = the number of smaller 64-bit keys; keys are unique) by (level, descending score, cell) or (descending score,
// candidate index).  Equal scores: the lower candidate index wins.
#include "common.h"

namespace {

struct Cand {
  float x1, y1, x2, y2, score;
  float r[4];
  uint32_t key;
};

constexpr int NT = 256;

struct Work {
  Cand* a;
  Cand* b;
  unsigned long long* ck;
};

__host__ __device__ inline size_t per_frame_bytes(int cap) { return (size_t)cap * (2 * sizeof(Cand) + 8); }

__device__ Work work_of(void* scratch, int cap, int f) {
  char* p = (char*)scratch + (size_t)f * per_frame_bytes(cap);
  Work w;
  w.ck = (unsigned long long*)p;
  w.a = (Cand*)(p + (size_t)cap * 8);
  w.b = w.a + cap;
  return w;
}

// descending-score part of a sort key: scores are probabilities (>= 0), whose bit patterns order like the values
__device__ __forceinline__ unsigned long long inv_score(float s) { return (unsigned long long)(~__float_as_uint(s)); }

// b[rank(i)] = a[i] for the n entries of a with keys ck (unique).  Ends with a barrier.
__device__ void rank_scatter(const Cand* a, const unsigned long long* ck, Cand* b, int n) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += NT) {
    const unsigned long long k = ck[i];
    int r = 0;
    for (int j = 0; j < n; ++j) r += ck[j] < k;
    b[r] = a[i];
  }
  __syncthreads();
}

__device__ __forceinline__ bool overlaps(const Cand& p, const Cand& q, float thr, int mode) {
  const float ap = (p.x2 - p.x1 + 1.f) * (p.y2 - p.y1 + 1.f), aq = (q.x2 - q.x1 + 1.f) * (q.y2 - q.y1 + 1.f);
  const float iw = fmaxf(0.f, fminf(p.x2, q.x2) - fmaxf(p.x1, q.x1) + 1.f);
  const float ih = fmaxf(0.f, fminf(p.y2, q.y2) - fmaxf(p.y1, q.y1) + 1.f);
  const float inter = iw * ih;
  const float o = mode ? inter / fminf(ap, aq) : inter / (ap + aq - inter);
  return o > thr;
}

// Greedy NMS over b[s .. e) (already in visiting order); keep[] (LDS, indexed from s) ends up 1 for kept boxes.
__device__ void nms_range(const Cand* b, int s, int e, float thr, int mode, uint8_t* keep) {
  for (int i = s + threadIdx.x; i < e; i += NT) keep[i - s] = 1;
  __syncthreads();
  for (int i = s; i < e; ++i) {
    if (keep[i - s]) {          // uniform: read behind a barrier
      const Cand p = b[i];
      for (int j = i + 1 + threadIdx.x; j < e; j += NT)
        if (keep[j - s] && overlaps(p, b[j], thr, mode)) keep[j - s] = 0;
    }
    __syncthreads();
  }
}

// Ordered compaction: out[k] = in[i] for the k-th i in [0, n) with flag[i]; returns the count (to every lane).
__device__ int compact(const Cand* in, const uint8_t* flag, Cand* out, int n, int* s_scan) {
  const int per = (n + NT - 1) / NT, lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
  int c = 0;
  for (int i = lo; i < hi; ++i) c += flag[i] != 0;
  s_scan[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int t = 0; t < NT; ++t) {
      const int v = s_scan[t];
      s_scan[t] = acc;
      acc += v;
    }
    s_scan[NT] = acc;
  }
  __syncthreads();
  int o = s_scan[threadIdx.x];
  for (int i = lo; i < hi; ++i)
    if (flag[i]) out[o++] = in[i];
  const int total = s_scan[NT];
  __syncthreads();
  return total;
}

// square (l = max(w, h) around the centre) and truncate toward zero
__device__ __forceinline__ void square_trunc(double x1, double y1, double x2, double y2, int out[4]) {
  const double w = x2 - x1, h = y2 - y1, l = fmax(w, h);
  x1 = x1 + w * 0.5 - l * 0.5;
  y1 = y1 + h * 0.5 - l * 0.5;
  x2 = x1 + l;
  y2 = y1 + l;
  out[0] = (int)trunc(x1); out[1] = (int)trunc(y1); out[2] = (int)trunc(x2); out[3] = (int)trunc(y2);
}

// b = box + reg (w, h, w, h) with w = x2 - x1 + plus (plus: 0 in stage 1, 1 in stages 2 and 3), fp64
__device__ __forceinline__ void regressed(float x1, float y1, float x2, float y2, const float* r, double plus, double o[4]) {
  const double bw = (double)x2 - x1 + plus, bh = (double)y2 - y1 + plus;
  o[0] = x1 + r[0] * bw; o[1] = y1 + r[1] * bh; o[2] = x2 + r[2] * bw; o[3] = y2 + r[3] * bh;
}

// the five landmarks on the (integer) input box: X = x1 - 1 + w lx, Y = y1 - 1 + h ly, w = x2 - x1 + 1; lm = (lx x 5, ly x 5)
__device__ __forceinline__ void landmarks(double x1, double y1, double x2, double y2, const float* lm, float* o /*(x, y) x 5*/) {
  const double bw = x2 - x1 + 1.0, bh = y2 - y1 + 1.0;
  for (int k = 0; k < 5; ++k) {
    o[2 * k] = (float)(x1 - 1.0 + bw * lm[k]);
    o[2 * k + 1] = (float)(y1 - 1.0 + bh * lm[5 + k]);
  }
}

// ---- stage 1 ----
struct S1Args {
  const fp_pnet_cand* cand;
  const int32_t* counts;
  const fp_pnet_level* levels;
  const int32_t* frame_level0;
  int32_t* boxes;
  float* scores;
  int32_t* out_counts;
  void* scratch;
  int cap, n_levels;
};

__global__ __launch_bounds__(NT) void stage1_kernel(S1Args p) {
  __shared__ uint8_t keep[FP_MTCNN_MAX_CAP];
  __shared__ int s_scan[NT + 1];
  __shared__ int s_lvl[129];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(p.counts[f], 0), p.cap);
  const Work w = work_of(p.scratch, p.cap, f);
  const int l0 = p.frame_level0[f];
  for (int i = tid; i < 129; i += NT) s_lvl[i] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += NT) {
    const fp_pnet_cand c = p.cand[(size_t)f * p.cap + i];
    const int lvl = (int)(c.key >> 24) & 127, cell = (int)(c.key & 0xFFFFFFu);
    const int gl = min(max(l0 + lvl, 0), p.n_levels - 1);
    const fp_pnet_level lv = p.levels[gl];
    const int ow = max(lv.ow, 1), y = cell / ow, x = cell - y * ow;
    Cand o;
    o.x1 = (float)trunc((2.0 * x + 1.0) / lv.scale);
    o.y1 = (float)trunc((2.0 * y + 1.0) / lv.scale);
    o.x2 = (float)trunc((2.0 * x + 12.0) / lv.scale);
    o.y2 = (float)trunc((2.0 * y + 12.0) / lv.scale);
    o.score = c.score;
    o.r[0] = c.reg[0]; o.r[1] = c.reg[1]; o.r[2] = c.reg[2]; o.r[3] = c.reg[3];
    o.key = c.key & 0x7FFFFFFFu;
    w.a[i] = o;
    w.ck[i] = ((unsigned long long)lvl << 56) | (inv_score(c.score) << 24) | (unsigned long long)cell;
    atomicAdd(&s_lvl[lvl + 1], 1);
  }
  rank_scatter(w.a, w.ck, w.b, n);
  if (tid == 0)
    for (int l = 0; l < 128; ++l) s_lvl[l + 1] += s_lvl[l];
  __syncthreads();
  // per level, IoU 0.5; kept boxes gathered level after level into a
  int n2 = 0;
  for (int l = 0; l < 128; ++l) {
    const int s = s_lvl[l], e = s_lvl[l + 1];
    if (s == e) continue;       // uniform
    nms_range(w.b, s, e, 0.5f, 0, keep);
    n2 += compact(w.b + s, keep, w.a + n2, e - s, s_scan);
  }
  for (int i = tid; i < n2; i += NT) w.ck[i] = (inv_score(w.a[i].score) << 32) | w.a[i].key;
  rank_scatter(w.a, w.ck, w.b, n2);
  nms_range(w.b, 0, n2, 0.7f, 0, keep);
  const int n3 = compact(w.b, keep, w.a, n2, s_scan);
  // regress with (w_q, h_q) = (x2 - x1, y2 - y1), square, truncate; non-positive sides dropped
  for (int i = tid; i < n3; i += NT) {
    const Cand c = w.a[i];
    double b[4];
    int q[4];
    regressed(c.x1, c.y1, c.x2, c.y2, c.r, 0.0, b);
    square_trunc(b[0], b[1], b[2], b[3], q);
    Cand o = c;
    o.x1 = (float)q[0]; o.y1 = (float)q[1]; o.x2 = (float)q[2]; o.y2 = (float)q[3];
    w.b[i] = o;
    keep[i] = q[2] - q[0] + 1 > 0 && q[3] - q[1] + 1 > 0;
  }
  __syncthreads();
  const int n4 = compact(w.b, keep, w.a, n3, s_scan);
  for (int i = tid; i < n4; i += NT) {
    const Cand c = w.a[i];
    int32_t* o = p.boxes + ((size_t)f * p.cap + i) * 4;
    o[0] = (int)c.x1; o[1] = (int)c.y1; o[2] = (int)c.x2; o[3] = (int)c.y2;
    p.scores[(size_t)f * p.cap + i] = c.score;
  }
  if (tid == 0) p.out_counts[f] = n4;
}

// ---- stages 2 and 3 ----
struct S23Args {
  const int32_t* boxes;
  const int32_t* offs;
  const float* prob;
  const float* reg;
  int32_t* out_boxes;
  float* out_scores;
  int32_t* out_counts;
  float* dets;
  int32_t* overflow;
  void* scratch;
  int cap, prob_ld, reg_ld, max_det;
  float t;
};

// rows of the frame with p >= t into b, by descending score (candidate index breaks ties); returns their number
__device__ int gather_passed(const S23Args& p, const Work& w, int f, int* s_cnt) {
  const int r0 = p.offs[f], n = min(max(p.offs[f + 1] - r0, 0), p.cap);
  if (threadIdx.x == 0) *s_cnt = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += NT) {
    const float pr = p.prob[(size_t)(r0 + i) * p.prob_ld + 1];
    const int32_t* bx = p.boxes + ((size_t)f * p.cap + i) * 4;
    Cand o;
    o.x1 = (float)bx[0]; o.y1 = (float)bx[1]; o.x2 = (float)bx[2]; o.y2 = (float)bx[3];
    o.score = pr;
    const float* rg = p.reg + (size_t)(r0 + i) * p.reg_ld;
    o.r[0] = rg[0]; o.r[1] = rg[1]; o.r[2] = rg[2]; o.r[3] = rg[3];
    o.key = (uint32_t)i;
    w.a[i] = o;
    const bool pass = pr >= p.t;      // a NaN never passes
    w.ck[i] = pass ? (inv_score(pr) << 32) | (unsigned)i : (0xFFFFFFFFull << 32) | (unsigned)i | (1ull << 63);
    if (pass) atomicAdd(s_cnt, 1);
  }
  rank_scatter(w.a, w.ck, w.b, n);
  return *s_cnt;
}

__global__ __launch_bounds__(NT) void stage2_kernel(S23Args p) {
  __shared__ uint8_t keep[FP_MTCNN_MAX_CAP];
  __shared__ int s_scan[NT + 1];
  __shared__ int s_cnt;
  const int f = blockIdx.x, tid = threadIdx.x;
  const Work w = work_of(p.scratch, p.cap, f);
  const int n = gather_passed(p, w, f, &s_cnt);
  nms_range(w.b, 0, n, 0.7f, 0, keep);
  const int n2 = compact(w.b, keep, w.a, n, s_scan);
  for (int i = tid; i < n2; i += NT) {
    const Cand c = w.a[i];
    double b[4];
    int q[4];
    regressed(c.x1, c.y1, c.x2, c.y2, c.r, 1.0, b);
    square_trunc(b[0], b[1], b[2], b[3], q);
    Cand o = c;
    o.x1 = (float)q[0]; o.y1 = (float)q[1]; o.x2 = (float)q[2]; o.y2 = (float)q[3];
    w.b[i] = o;
    keep[i] = q[2] - q[0] + 1 > 0 && q[3] - q[1] + 1 > 0;
  }
  __syncthreads();
  const int n3 = compact(w.b, keep, w.a, n2, s_scan);
  for (int i = tid; i < n3; i += NT) {
    const Cand c = w.a[i];
    int32_t* o = p.out_boxes + ((size_t)f * p.cap + i) * 4;
    o[0] = (int)c.x1; o[1] = (int)c.y1; o[2] = (int)c.x2; o[3] = (int)c.y2;
    p.out_scores[(size_t)f * p.cap + i] = c.score;
  }
  if (tid == 0) p.out_counts[f] = n3;
}

__global__ __launch_bounds__(NT) void stage3_kernel(S23Args p) {
  __shared__ uint8_t keep[FP_MTCNN_MAX_CAP];
  __shared__ int s_scan[NT + 1];
  __shared__ int s_cnt;
  const int f = blockIdx.x, tid = threadIdx.x;
  const Work w = work_of(p.scratch, p.cap, f);
  const int r0 = p.offs[f];
  const int n = gather_passed(p, w, f, &s_cnt);
  // the regressed box replaces the input box; the input box is read again from boxes[] for the landmarks
  for (int i = tid; i < n; i += NT) {
    Cand c = w.b[i];
    double b[4];
    regressed(c.x1, c.y1, c.x2, c.y2, c.r, 1.0, b);
    c.x1 = (float)b[0]; c.y1 = (float)b[1]; c.x2 = (float)b[2]; c.y2 = (float)b[3];
    w.a[i] = c;
  }
  __syncthreads();
  nms_range(w.a, 0, n, 0.7f, 1, keep);
  const int n2 = compact(w.a, keep, w.b, n, s_scan);
  const int n_out = min(n2, p.max_det);
  for (int i = tid; i < n_out; i += NT) {
    const Cand c = w.b[i];
    const int32_t* bx = p.boxes + ((size_t)f * p.cap + c.key) * 4;
    const float* rg = p.reg + (size_t)(r0 + (int)c.key) * p.reg_ld;
    float* o = p.dets + ((size_t)f * p.max_det + i) * 15;
    o[0] = c.x1; o[1] = c.y1; o[2] = c.x2; o[3] = c.y2;
    landmarks(bx[0], bx[1], bx[2], bx[3], rg + 4, o + 4);
    o[14] = c.score;
  }
  if (tid == 0) {
    p.out_counts[f] = n_out;
    p.overflow[f] = n2 > p.max_det;
  }
}

// ---- box arithmetic alone ----
struct BoxArgs {
  const float* boxes;
  const float* reg;
  int32_t* out_boxes;
  float* out_rows;
  int reg_ld, n, mode;
};

__global__ __launch_bounds__(NT) void boxes_kernel(BoxArgs p) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= p.n) return;
  const float* bx = p.boxes + (size_t)i * 4;
  const float* r = p.reg + (size_t)i * p.reg_ld;
  double b[4];
  regressed(bx[0], bx[1], bx[2], bx[3], r, p.mode == 1 ? 0.0 : 1.0, b);
  if (p.mode == 3) {
    float* o = p.out_rows + (size_t)i * 14;
    for (int k = 0; k < 4; ++k) o[k] = (float)b[k];
    landmarks(bx[0], bx[1], bx[2], bx[3], r + 4, o + 4);
  } else {
    int q[4];
    square_trunc(b[0], b[1], b[2], b[3], q);
    for (int k = 0; k < 4; ++k) p.out_boxes[(size_t)i * 4 + k] = q[k];
  }
}

// ---- NMS alone ----
struct NmsArgs {
  const float* boxes;
  const float* scores;
  const int32_t* seg;
  int32_t* keep_idx;
  int32_t* keep_count;
  void* scratch;
  int n;
  float thr;
  int mode;
};

__global__ __launch_bounds__(NT) void nms_kernel(NmsArgs p) {
  __shared__ uint8_t keep[FP_MTCNN_MAX_CAP];
  __shared__ int s_scan[NT + 1];
  const int sgm = blockIdx.x, tid = threadIdx.x;
  const int s = min(max(p.seg[sgm], 0), p.n), e = min(max(p.seg[sgm + 1], s), p.n);
  const int n = min(e - s, FP_MTCNN_MAX_CAP);
  const Work w0 = work_of(p.scratch, p.n, 0);
  Cand *a = w0.a + s, *b = w0.b + s;
  unsigned long long* ck = w0.ck + s;
  for (int i = tid; i < n; i += NT) {
    Cand o;
    const float* bx = p.boxes + (size_t)(s + i) * 4;
    o.x1 = bx[0]; o.y1 = bx[1]; o.x2 = bx[2]; o.y2 = bx[3];
    o.score = p.scores[s + i];
    o.r[0] = o.r[1] = o.r[2] = o.r[3] = 0.f;
    o.key = (uint32_t)(s + i);
    a[i] = o;
    ck[i] = (inv_score(o.score) << 32) | (unsigned)i;
  }
  rank_scatter(a, ck, b, n);
  nms_range(b, 0, n, p.thr, p.mode, keep);
  const int n2 = compact(b, keep, a, n, s_scan);
  for (int i = tid; i < n2; i += NT) p.keep_idx[s + i] = (int32_t)a[i].key;
  if (tid == 0) p.keep_count[sgm] = n2;
}

// ---- cut + resize ----
struct CutArgs {
  const uint8_t* frames;
  size_t frames_bytes;
  const fp_frame_desc* descs;
  const int32_t* boxes;
  const int32_t* offs;
  float* out;
  uint8_t* out_u8;
  int n_frames, cap, n, size;
};

__device__ __forceinline__ long patch_px(const uint8_t* f, int H, int W, int x1, int y1, int py, int px, int c) {
  const int y = y1 - 1 + py, x = x1 - 1 + px;
  return ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? (long)f[((size_t)y * W + x) * 3 + c] : 0;
}

// linear tap in area mode, exactly: source index s and the weight a / n_src of its right / lower neighbour
__device__ __forceinline__ void area_tap(int d, int n_src, int n_dst, int& s, long& a) {
  s = (int)(((long)d * n_src) / n_dst);
  a = (long)(d + 1) * n_src - (long)(s + 1) * n_dst;      // f n_src
  a = a <= 0 ? 0 : a % n_src;
  if (s >= n_src - 1) {
    s = n_src - 1;
    a = 0;
  }
}

__device__ __forceinline__ int round_half_even(long s, long d) {
  long q = s / d;
  const long r = s - q * d;
  if (2 * r > d || (2 * r == d && (q & 1))) ++q;
  return (int)q;
}

__global__ __launch_bounds__(NT) void cut_kernel(CutArgs p) {
  const int item = blockIdx.x, pix = blockIdx.y * NT + threadIdx.x;
  if (pix >= p.size * p.size) return;
  // the frame of this item: the last f with offs[f] <= item
  int lo = 0, hi = p.n_frames - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.offs[mid] <= item) lo = mid; else hi = mid - 1;
  }
  const int f = lo, j = item - p.offs[f];
  float* o = p.out + ((size_t)item * p.size * p.size + pix) * 4;
  uint8_t* o8 = p.out_u8 ? p.out_u8 + ((size_t)item * p.size * p.size + pix) * 3 : nullptr;
  int u[3] = {0, 0, 0};
  const fp_frame_desc d = p.descs[f];
  const bool ok = j >= 0 && j < p.cap && d.h >= 1 && d.w >= 1 && d.off >= 0 &&
                  (size_t)d.off + (size_t)d.h * d.w * 3 <= p.frames_bytes;
  if (ok) {
    const int32_t* bx = p.boxes + ((size_t)f * p.cap + j) * 4;
    const int x1 = bx[0], y1 = bx[1];
    const long pw = (long)bx[2] - x1 + 1, ph = (long)bx[3] - y1 + 1;
    if (pw >= 1 && ph >= 1 && pw <= 65536 && ph <= 65536) {
      const uint8_t* fr = p.frames + d.off;
      const int n = p.size, dy = pix / n, dx = pix - dy * n;
      long acc[3] = {0, 0, 0};
      if (pw >= n && ph >= n) {
        // lengths in units of 1 / n patch pixels: destination cell dx covers [dx pw, (dx + 1) pw)
        const long X0 = dx * pw, X1 = X0 + pw, Y0 = dy * ph, Y1 = Y0 + ph;
        const int xa = (int)(X0 / n), xb = (int)((X1 - 1) / n), ya = (int)(Y0 / n), yb = (int)((Y1 - 1) / n);
        for (int y = ya; y <= yb; ++y) {
          const long wy = min((long)(y + 1) * n, Y1) - max((long)y * n, Y0);
          long r[3] = {0, 0, 0};
          for (int x = xa; x <= xb; ++x) {
            const long wx = min((long)(x + 1) * n, X1) - max((long)x * n, X0);
            for (int c = 0; c < 3; ++c) r[c] += wx * patch_px(fr, d.h, d.w, x1, y1, y, x, c);
          }
          for (int c = 0; c < 3; ++c) acc[c] += wy * r[c];
        }
      } else {
        int sx, sy;
        long ax, ay;
        area_tap(dx, (int)pw, n, sx, ax);
        area_tap(dy, (int)ph, n, sy, ay);
        const int sx1 = min(sx + 1, (int)pw - 1), sy1 = min(sy + 1, (int)ph - 1);
        for (int c = 0; c < 3; ++c) {
          const long top = (pw - ax) * patch_px(fr, d.h, d.w, x1, y1, sy, sx, c) + ax * patch_px(fr, d.h, d.w, x1, y1, sy, sx1, c);
          const long bot = (pw - ax) * patch_px(fr, d.h, d.w, x1, y1, sy1, sx, c) + ax * patch_px(fr, d.h, d.w, x1, y1, sy1, sx1, c);
          acc[c] = (ph - ay) * top + ay * bot;
        }
      }
      for (int c = 0; c < 3; ++c) u[c] = round_half_even(acc[c], pw * ph);
    }
  }
  float q[3];
  for (int c = 0; c < 3; ++c) {
    q[c] = ((float)u[c] - 127.5f) * 0.0078125f;
    if (o8) o8[c] = (uint8_t)u[c];
  }
  *(f32x4*)o = f32x4{q[0], q[1], q[2], 0.f};
}

}  // namespace

extern "C" {

size_t fp_mtcnn_scratch_bytes(int n_frames, int cap) {
  if (n_frames < 0 || cap < 1) return 0;
  return (size_t)n_frames * per_frame_bytes(cap);
}

int fp_mtcnn_stage1(const fp_pnet_cand* cand, const int32_t* counts, int n_frames, int cap, const fp_pnet_level* levels,
                    int n_levels, const int32_t* frame_level0, int32_t* boxes, float* scores, int32_t* out_counts,
                    void* scratch, size_t scratch_bytes, void* stream) {
  if (!cand || !counts || !levels || !frame_level0 || !boxes || !scores || !out_counts || !scratch) return FP_ERR_INVALID_ARG;
  if (n_frames < 0 || n_levels < 1 || cap < 1 || cap > FP_MTCNN_MAX_CAP) return FP_ERR_INVALID_ARG;
  if (scratch_bytes < fp_mtcnn_scratch_bytes(n_frames, cap) || ((uintptr_t)scratch & 7)) return FP_ERR_INVALID_ARG;
  if (n_frames == 0) return FP_OK;
  S1Args a{cand, counts, levels, frame_level0, boxes, scores, out_counts, scratch, cap, n_levels};
  hipLaunchKernelGGL(stage1_kernel, dim3((unsigned)n_frames), dim3(NT), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_mtcnn_cut(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const int32_t* boxes,
                 int cap, const int32_t* offs, int n, int size, float* out, uint8_t* out_u8, void* stream) {
  if (!frames || !descs || !boxes || !offs || !out) return FP_ERR_INVALID_ARG;
  if (n_frames < 1 || cap < 1 || n < 0 || size < 1 || size > 256 || ((uintptr_t)out & 15)) return FP_ERR_INVALID_ARG;
  if (n == 0) return FP_OK;
  CutArgs a{frames, frames_bytes, descs, boxes, offs, out, out_u8, n_frames, cap, n, size};
  hipLaunchKernelGGL(cut_kernel, dim3((unsigned)n, (unsigned)fp_ceil_div(size * size, NT)), dim3(NT), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

static int stage23(bool third, const int32_t* boxes, int n_frames, int cap, const int32_t* offs, const float* prob, int prob_ld,
                   const float* reg, int reg_ld, float t, int max_det, int32_t* out_boxes, float* out_scores, float* dets,
                   int32_t* out_counts, int32_t* overflow, void* scratch, size_t scratch_bytes, void* stream) {
  if (!boxes || !offs || !prob || !reg || !out_counts || !scratch) return FP_ERR_INVALID_ARG;
  if (third ? (!dets || !overflow || max_det < 1) : (!out_boxes || !out_scores)) return FP_ERR_INVALID_ARG;
  if (n_frames < 0 || cap < 1 || cap > FP_MTCNN_MAX_CAP || prob_ld < 2 || reg_ld < (third ? 14 : 4)) return FP_ERR_INVALID_ARG;
  if (scratch_bytes < fp_mtcnn_scratch_bytes(n_frames, cap) || ((uintptr_t)scratch & 7)) return FP_ERR_INVALID_ARG;
  if (n_frames == 0) return FP_OK;
  S23Args a{boxes, offs, prob, reg, out_boxes, out_scores, out_counts, dets, overflow, scratch, cap, prob_ld, reg_ld, max_det, t};
  if (third) hipLaunchKernelGGL(stage3_kernel, dim3((unsigned)n_frames), dim3(NT), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(stage2_kernel, dim3((unsigned)n_frames), dim3(NT), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_mtcnn_stage2(const int32_t* boxes, int n_frames, int cap, const int32_t* offs, const float* prob, int prob_ld,
                    const float* reg, int reg_ld, float t2, int32_t* out_boxes, float* out_scores, int32_t* out_counts,
                    void* scratch, size_t scratch_bytes, void* stream) {
  return stage23(false, boxes, n_frames, cap, offs, prob, prob_ld, reg, reg_ld, t2, 0, out_boxes, out_scores, nullptr, out_counts,
                 nullptr, scratch, scratch_bytes, stream);
}

int fp_mtcnn_stage3(const int32_t* boxes, int n_frames, int cap, const int32_t* offs, const float* prob, int prob_ld,
                    const float* reg, int reg_ld, float t3, int max_det, float* dets, int32_t* counts, int32_t* overflow,
                    void* scratch, size_t scratch_bytes, void* stream) {
  return stage23(true, boxes, n_frames, cap, offs, prob, prob_ld, reg, reg_ld, t3, max_det, nullptr, nullptr, dets, counts,
                 overflow, scratch, scratch_bytes, stream);
}

int fp_mtcnn_boxes(const float* boxes, const float* reg, int reg_ld, int n, int mode, int32_t* out_boxes, float* out_rows,
                   void* stream) {
  if (!boxes || !reg || n < 0 || mode < 1 || mode > 3 || reg_ld < (mode == 3 ? 14 : 4)) return FP_ERR_INVALID_ARG;
  if (mode == 3 ? !out_rows : !out_boxes) return FP_ERR_INVALID_ARG;
  if (n == 0) return FP_OK;
  BoxArgs a{boxes, reg, out_boxes, out_rows, reg_ld, n, mode};
  hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)fp_ceil_div(n, NT)), dim3(NT), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_mtcnn_nms(const float* boxes, const float* scores, const int32_t* seg, int n_seg, int n, float thr, int mode,
                 int32_t* keep_idx, int32_t* keep_count, void* scratch, size_t scratch_bytes, void* stream) {
  if (!boxes || !scores || !seg || !keep_idx || !keep_count || !scratch) return FP_ERR_INVALID_ARG;
  if (n_seg < 0 || n < 1 || (mode != 0 && mode != 1)) return FP_ERR_INVALID_ARG;
  if (scratch_bytes < fp_mtcnn_scratch_bytes(1, n) || ((uintptr_t)scratch & 7)) return FP_ERR_INVALID_ARG;
  if (n_seg == 0) return FP_OK;
  NmsArgs a{boxes, scores, seg, keep_idx, keep_count, scratch, n, thr, mode};
  hipLaunchKernelGGL(nms_kernel, dim3((unsigned)n_seg), dim3(NT), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
