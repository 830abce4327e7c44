// simi8.hip — the compressed gallery (gfx950): int8 row quantisation, the coarse top-pool search on the i8 matrix cores and
// the exact rerank of its candidates (DESIGN S7 "Compressed gallery").
//
//  * quantize_rows_i8_kernel: q = rint(x * (127 / amax)) per row, scale = amax / 127, in the layout the walk stages:
//    [D / 64][round_up(N, 128)][64] int8 -- one k-slab (64 features) of a 128-column chunk is 8 KiB contiguous.
//  * cosine_topk_i8_kernel: the i8 twin of cosine_topk_x6_kernel (sim.hip).  S = Qq Gq^T on v_mfma_i32_16x16x64_i8 (one MFMA
//    where the split walk issues twelve), exact in int32; coarse score c = float(dot) * w[column], one rounding.  The keys,
//    the filter, the turn-taking of the insertion path and the final merge (topk_merge_kernel, sim.hip) are those of the fp32
//    search; the lists are unsorted with a tracked minimum (below).
//  * rerank_topk_kernel: one wave per query; the exact fp32 cosine of its <= 64 candidates, the k best by key.
// Built with -ffp-contract=off: device and numpy restatement agree bit for bit.
#include "cosinewalk.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int I8_K = 64;                   // features of a k-slab: the K of one v_mfma_i32_16x16x64_i8
constexpr int I8_SLAB = CW_NC * I8_K;      // bytes of one k-slab of a chunk
constexpr int I8_LDS = 2 * I8_SLAB;        // the staging buffer: two slabs

// One wave per row n < Npad.  Rows past N (the padding) are written as zeros; scale only for n < N.
__global__ __launch_bounds__(256) void quantize_rows_i8_kernel(const float* __restrict__ X, int N, int D, int Npad,
                                                               signed char* __restrict__ q8, float* __restrict__ scale) {
  const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= Npad) return;
  const int lane = threadIdx.x & 63;
  const int nv = D / 4;                                  // float4s of a row: a multiple of 16, at most 256
  f32x4 v[4];
  float amax = 0.f;
  bool bad = false;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = lane + 64 * t;
    v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (n < N && c < nv) v[t] = *(const f32x4*)(X + n * D + 4 * c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = fabsf(v[t][i]);
      bad = bad || !(a <= 3.402823466e+38f);             // inf or NaN
      amax = fmaxf(amax, a);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
  const bool dead = __ballot(bad) != 0 || amax == 0.f;
  const float r = dead ? 0.f : 127.0f / amax;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = lane + 64 * t;
    if (c >= nv) continue;
    unsigned pk = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float y = rintf(v[t][i] * r);                      // one multiply, round half to even
      y = y != y ? 0.f : fminf(fmaxf(y, -127.f), 127.f);
      pk |= ((unsigned)(int)y & 0xFFu) << (8 * i);
    }
    const int k = 4 * c;
    *(unsigned*)(q8 + ((long)(k / I8_K) * Npad + n) * I8_K + (k % I8_K)) = pk;
  }
  if (lane == 0 && n < N) scale[n] = dead ? 0.f : amax / 127.0f;
}

// Grid (row tile) x (split), 4 waves, a wave owns MT x 16 query rows.  Qq / Gq in the quantiser's layout (Mpad / Npad rows per
// k-slab, both multiples of 128 >= the rows any tile touches: no load leaves the buffers).  Swapped operands as cw_walk: per
// accumulator acc[t][n] a lane holds query row 16 t + (lane & 15) x the 4 consecutive gallery columns c0 + 16 n + 4 (lane >> 4) + i;
// lane l feeds features 16 (l >> 4) .. + 15 of the slab to both operands, so whatever order the MFMA sums them in, the two
// sides agree.  B goes through LDS by LDS-DMA, ONE flat double-buffered pipeline over all chunks, ONE barrier per step.
template <int MT>
__global__ __launch_bounds__(256, 3) void cosine_topk_i8_kernel(const signed char* __restrict__ Q8, const float* __restrict__ u,
                                                                long M, int Mpad, const signed char* __restrict__ G8,
                                                                const float* __restrict__ w, int N, int Npad, int nchunk, int D,
                                                                int k, int n_splits, const float* __restrict__ floor0,
                                                                u64* __restrict__ partial) {
  constexpr int NT16 = CW_NT16, XBM = 4 * MT * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  // behind the staging buffer: [XBM][LS] running keys.  Unlike the fp32 search's sorted lists these are UNSORTED: slot k of a row
  // holds the position of its smallest key, an insertion overwrites that key and rescans the row for the next smallest.  With
  // k up to 64 the sorted insertion's chain of dependent LDS moves dominated the search; the merge kernel needs no order.
  volatile u64* Ls = (volatile u64*)(smem_raw + I8_LDS);
  const int LS = (k + 1) | 1;                            // odd stride: the rows' entries fall in different banks
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const unsigned vb = fp_xcd_block();                    // the splits of one row tile on ONE XCD (query rows from its L2)
  const int split = vb % (unsigned)n_splits;
  const long row0 = (long)(vb / (unsigned)n_splits) * XBM + wave * (MT * 16);
  const int base = nchunk / n_splits, rem = nchunk - base * n_splits;
  const int cb = split * base + (split < rem ? split : rem);
  const int nck = base + (split < rem ? 1 : 0);          // >= 1 (the launcher clamps n_splits to nchunk)
  const i32x4 z = {0, 0, 0, 0};
  const float ninf = -__builtin_huge_valf(), qnan = __builtin_nanf("");

  for (int i = lane; i < MT * 16 * LS; i += 64) Ls[wave * (MT * 16) * LS + i] = 0;
  u64 lower = 0;                                         // the lanes of my row with a smaller q
  for (int qq = 0; qq < q; ++qq) lower |= 1ull << (l15 + 16 * qq);
  // thr: the k-th best score of my rows so far, never below flo, the k-th best of an earlier pass over a PART of the columns
  // (floor0[m][k - 1], -inf where that pass found fewer than k): k candidates reach it, so nothing below it can be among the k
  // best of all columns.  live: 1, or NaN for a dead query row.
  float thr[MT], flo[MT], live[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const long m = row0 + 16 * t + l15;
    flo[t] = (floor0 && m < M) ? floor0[m * k + k - 1] : ninf;
    thr[t] = flo[t];
    const float um = m < M ? u[m] : 0.f;
    live[t] = (um > 0.f && um <= 3.402823466e+38f) ? 1.f : qnan;
  }

  const int KS = D / I8_K;
  auto stage = [&](int chunk, int ks, int buf) {
    unsigned char* dst = smem_raw + buf * I8_SLAB;
    const unsigned char* src = (const unsigned char*)G8 + ((long)ks * Npad + (long)chunk * CW_NC) * I8_K + lane * 16;
#pragma unroll
    for (int j = 0; j < I8_SLAB / 4096; ++j) {
      const int c = j * 4 + wave;
      __builtin_amdgcn_global_load_lds((gbl_ptr)(src + c * 1024), (lds_ptr)(dst + c * 1024), 16, 0, 0);
    }
  };
  const signed char* Aw = Q8 + fp_uniform(row0 * I8_K);   // this wave's rows of slab 0
  const long aslab = fp_uniform((long)Mpad * I8_K);
  i32x4 araw[MT];
  auto load_a = [&](int ks) {
#pragma unroll
    for (int t = 0; t < MT; ++t) araw[t] = *(const i32x4*)(Aw + ks * aslab + ((16 * t + l15) * I8_K + 16 * q));
  };
  i32x4 acc[MT][NT16];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int n = 0; n < NT16; ++n) acc[t][n] = z;

  // epilogue of a chunk: lane = query row 16 t + l15, gallery columns c0 + 16 n + 4 q + i
  // Two halves of 64 columns.  Per half: first every candidate's score and one bit per candidate that reaches its row's
  // threshold (the common case ends there: one ballot per 16 rows x 64 columns), then the pending candidates of all groups at
  // once -- the four lanes that share a row take turns by one ballot, rows proceed side by side -- so the number of trips
  // through the insertion path follows the candidates of the busiest row, not the number of groups that hold one.
  auto epi = [&](int c0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 sv[MT][4];
      unsigned pm[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) pm[t] = 0;
#pragma unroll
      for (int nn = 0; nn < 4; ++nn) {
        const int n = 4 * h + nn;
        const int colb = c0 + 16 * n + 4 * q;
        f32x4 rn;
        if (colb + 3 < N) {
          rn = *(const f32x4*)(w + colb);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) rn[i] = colb + i < N ? w[colb + i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) rn[i] = cw_nan_if_zero(rn[i]);          // masked / padding: never a candidate
#pragma unroll
        for (int t = 0; t < MT; ++t) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sv[t][nn][i] = (float)acc[t][n][i] * rn[i] * live[t];           // |dot| < 2^24: exact; x w: ONE rounding; x 1
            pm[t] |= (sv[t][nn][i] >= thr[t] ? 1u : 0u) << (4 * nn + i);    // NaN compares false
          }
          acc[t][n] = z;
        }
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (__ballot(pm[t] != 0) == 0) continue;         // the common case: nothing in this half reaches the k-th best
        volatile u64* Lr = Ls + (wave * (MT * 16) + 16 * t + l15) * LS;
        for (;;) {
          const bool have = pm[t] != 0;
          const u64 mask = __ballot(have);
          if (!mask) break;
          if (have && !(mask & lower)) {                 // my turn: no lower-q lane of my row is waiting
            const int b = __builtin_ctz(pm[t]);
            pm[t] &= pm[t] - 1;
            float v = 0.f;
#pragma unroll
            for (int nn = 0; nn < 4; ++nn)
#pragma unroll
              for (int i = 0; i < 4; ++i) v = b == 4 * nn + i ? sv[t][nn][i] : v;
            const u64 key = cw_key(v, (unsigned)(c0 + 16 * (4 * h + (b >> 2)) + 4 * q + (b & 3)));
            const int p = (int)Lr[k];
            if (key > Lr[p]) {                           // replaces the smallest key (an empty slot while there is one) ...
              Lr[p] = key;
              u64 mn = ~0ull;
              int mp = 0;
#pragma unroll 8
              for (int j = 0; j < k; ++j) {              // ... and finds the next one: independent reads, no chain
                const u64 e = Lr[j];
                if (e < mn) mn = e, mp = j;
              }
              Lr[k] = (u64)mp;
            }
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {                       // my row's threshold, as every lane of the row left it
        volatile u64* Lr = Ls + (wave * (MT * 16) + 16 * t + l15) * LS;
        const u64 kth = Lr[(int)Lr[k]];
        thr[t] = kth ? fmaxf(cw_key_score(kth), flo[t]) : flo[t];
      }
    }
  };

  const int steps = nck * KS;
  int ks = 0, chunk = cb;                                // of the step being computed
  stage(cb, 0, 0);
  load_a(0);
  for (int s = 0; s < steps; ++s) {
    i32x4 af[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) af[t] = araw[t];
    __syncthreads();                                     // this step's slab has landed; every wave has left the other one
    if (s + 1 < steps) {
      const bool last = ks + 1 == KS;
      stage(last ? chunk + 1 : chunk, last ? 0 : ks + 1, (s + 1) & 1);
      load_a(last ? 0 : ks + 1);
    }
    const unsigned char* Bc = smem_raw + (s & 1) * I8_SLAB + (l15 * I8_K + 16 * q);
    i32x4 bf[2];
    bf[0] = *(const i32x4*)Bc;
#pragma unroll
    for (int n = 0; n < NT16; ++n) {
      if (n + 1 < NT16) bf[(n + 1) & 1] = *(const i32x4*)(Bc + (n + 1) * 16 * I8_K);
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bf[n & 1], af[t], acc[t][n], 0, 0, 0);
    }
    if (++ks < KS) continue;
    ks = 0;
    epi(chunk * CW_NC);
    ++chunk;
  }

  // the lists of this wave's rows -> partial[m][split][0 .. k)
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < MT * 16 * k; i += 64) {
    const int r = i / k, j = i - r * k;
    const long m = row0 + r;
    if (m < M) partial[(m * n_splits + split) * k + j] = Ls[(wave * (MT * 16) + r) * LS + j];
  }
}

// coarse_score = c * u[m] on the merged (M, pool) result; empty slots (idx < 0) stay -inf.
__global__ __launch_bounds__(256) void coarse_scale_kernel(float* __restrict__ scores, const int* __restrict__ idx,
                                                           const float* __restrict__ u, long M, int pool) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * pool) return;
  if (idx[i] >= 0) scores[i] = scores[i] * u[i / pool];
}

// One wave per query row.  Candidate j (indexed mode: row cand[m][j] of G; compact mode: row m * pool + j of `rows`) gets
// score = dot * qinv[m] * ginv[cand], dot = every lane's products summed in feature order, then the xor butterfly: a fixed
// order.  -1 / out-of-range entries and masked rows (ginv == 0) carry no key.  Lane j then holds the key of candidate j; its
// rank among the keys (larger first; keys of distinct rows are distinct, a row that the list names again keeps its first
// entry only) is its output slot.
__global__ __launch_bounds__(256) void rerank_topk_kernel(const float* __restrict__ Q, const float* __restrict__ qinv, long M,
                                                          int D, const int* __restrict__ cand, int pool,
                                                          const float* __restrict__ G, const float* __restrict__ rows,
                                                          const float* __restrict__ ginv, int N, int k,
                                                          float* __restrict__ scores, int* __restrict__ idx) {
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int lane = threadIdx.x & 63;
  const int nv = D / 4;
  f32x4 qv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = lane + 64 * t;
    qv[t] = c < nv ? *(const f32x4*)(Q + m * D + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float qi = qinv[m];
  u64 mine = 0;
  for (int j = 0; j < pool; ++j) {
    const int g = cand[m * pool + j];                    // wave-uniform
    if (g < 0 || g >= N) continue;
    const float gi = ginv[g];
    if (gi == 0.f) continue;
    const float* row = G ? G + (long)g * D : rows + (m * pool + j) * D;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = lane + 64 * t;
      if (c < nv) {
        const f32x4 r = *(const f32x4*)(row + 4 * c);
#pragma unroll
        for (int i = 0; i < 4; ++i) s += qv[t][i] * r[i];
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const float sc = s * qi * gi;
    if (lane == j && sc == sc) mine = cw_key(sc, (unsigned)g);
  }
  // a gallery row that the list names again has the key of its first entry (the same row, the same sum): it counts once
  bool again = false;
  for (int j = 0; j < pool; ++j) {
    const u64 o = __shfl(mine, j);
    again |= o == mine && j < lane;
  }
  if (again) mine = 0;
  int rank = 0;
  for (int j = 0; j < pool; ++j) rank += __shfl(mine, j) > mine ? 1 : 0;
  const int valid = __popcll(__ballot(mine != 0));
  if (mine && rank < k) {
    scores[m * k + rank] = cw_key_score(mine);
    idx[m * k + rank] = cw_key_index(mine);
  }
  if (lane >= valid && lane < k) {
    scores[m * k + lane] = -__builtin_huge_valf();
    idx[m * k + lane] = -1;
  }
}

// rows of a workgroup: 128 while the lists leave room for three workgroups per CU beside the 16 KiB of staging (pool <= 32:
// 128 x 33 x 8 B = 33 KiB), else 64 (pool 64: 64 x 65 x 8 B = 33 KiB again).  Either way <= 50 KiB of LDS.
inline int i8_rows(int pool) { return pool <= 32 ? 128 : 64; }
// splits of the column range when the row tiles alone do not fill the device's workgroup slots (three per CU): enough for ONE
// round of the slots at pool <= 32, for half a round above.  Every split pays the ramp in which its lists fill, and that ramp
// grows with pool (measured, 512 x 1 000 000 x 512: pool 4 / 20 / 64 are fastest at 192 / 192 / 48 splits of 4 / 4 / 8 tiles).
constexpr int I8_PER_CU = 3;
constexpr int I8_PREFIX = 16384;           // columns of the first pass of a large gallery (fp_cosine_topk_i8)
int i8_auto_splits(int64_t M, int pool, int cus) {
  const int rows = i8_rows(pool);
  const long tiles = (M + rows - 1) / rows;
  const long slots = (long)I8_PER_CU * cus;
  if (tiles >= slots) return 1;
  const long want = pool <= 32 ? slots : slots / 2;
  const long s = (want + tiles - 1) / (tiles > 0 ? tiles : 1);
  return (int)(s > 4096 ? 4096 : s);
}

}  // namespace

extern "C" {

size_t fp_quant_i8_bytes(int N, int D) {
  if (N <= 0 || D <= 0 || D % I8_K) return 0;
  return (size_t)D * (size_t)fp_round_up(N, CW_NC);
}

int fp_quantize_rows_i8(const float* X, int N, int D, void* q8, float* scale, void* stream) {
  if (!X || !q8 || !scale || N <= 0 || D <= 0 || D > FP_QUANT_MAX_D) return FP_ERR_INVALID_ARG;
  if (D % I8_K || ((uintptr_t)X) % 16 || ((uintptr_t)q8) % 16) return FP_ERR_ALIGNMENT;
  const long Npad = fp_round_up(N, CW_NC);
  if (Npad >= (1L << 31)) return FP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(quantize_rows_i8_kernel, dim3((unsigned)fp_ceil_div(Npad, 4)), dim3(256), 0, (hipStream_t)stream, X, N, D,
                     (int)Npad, (signed char*)q8, scale);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

size_t fp_cosine_topk_i8_workspace(int64_t M, int N, int pool, int n_splits) {
  if (M <= 0 || N <= 0 || pool < 1 || pool > FP_COARSE_MAX || n_splits < 0) return 0;
  const size_t nchunk = (size_t)(fp_round_up(N, CW_NC) / CW_NC);
  if (n_splits) return (size_t)M * (nchunk < (size_t)n_splits ? nchunk : (size_t)n_splits) * (size_t)pool * sizeof(uint64_t);
  // automatic: tiles * n_splits is at most (workgroups wanted) + tiles, and never above tiles * nchunk
  const size_t rows = (size_t)i8_rows(pool);
  const size_t tiles = (size_t)((M + rows - 1) / rows);
  const size_t want = (size_t)I8_PER_CU * fp_num_cus() + tiles;
  const size_t lists = tiles * nchunk < want ? tiles * nchunk : want;
  return lists * rows * (size_t)pool * sizeof(uint64_t);
}

int fp_cosine_topk_i8(const void* Q8, const float* u, int64_t M, const void* G8, const float* w, int N, int D, int pool,
                      int n_splits, float* scores, int32_t* idx, void* workspace, size_t ws_bytes, void* stream) {
  if (!Q8 || !u || !G8 || !w || !scores || !idx || !workspace) return FP_ERR_INVALID_ARG;
  if (M < 0 || N <= 0 || D <= 0 || D > FP_QUANT_MAX_D || pool < 1 || pool > FP_COARSE_MAX || n_splits < 0) return FP_ERR_INVALID_ARG;
  if (D % I8_K || ((uintptr_t)Q8) % 16 || ((uintptr_t)G8) % 16 || ((uintptr_t)w) % 16 || ((uintptr_t)workspace) % 8)
    return FP_ERR_ALIGNMENT;
  if (M == 0) return FP_OK;
  if (ws_bytes < fp_cosine_topk_i8_workspace(M, N, pool, n_splits)) return FP_ERR_INVALID_ARG;
  const long Mpad = fp_round_up(M, CW_NC), Npad = fp_round_up(N, CW_NC);
  if (Mpad >= (1L << 31) || Npad >= (1L << 31)) return FP_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int nchunk = (int)(Npad / CW_NC);
  const int rows = i8_rows(pool);
  const int lds = I8_LDS + rows * ((pool + 1) | 1) * 8;  // <= 50 KiB
  const long tiles = (M + rows - 1) / rows;
  // Passes over growing prefixes of the columns, the last one over all of them.  A split starts with empty lists, and until a
  // row's list holds scores near its final ones almost every group of candidates takes the insertion path; the pool-th best
  // score of a prefix is a lower bound of the final one, so each pass hands the next one a floor (through `scores`, which the
  // last merge overwrites) and only a pool * (columns / prefix) candidates per row pass it.  Prefixes grow 8-fold from
  // I8_PREFIX columns while the next pass is still at least 4 times larger; galleries below 4 * I8_PREFIX take one pass.
  long level = (long)I8_PREFIX / CW_NC;                  // chunks of the pass
  const float* floor0 = nullptr;
  for (;;) {
    const bool last = level * 4 > nchunk;
    const int nc = last ? nchunk : (int)level;
    int ns = n_splits ? n_splits : i8_auto_splits(M, pool, fp_num_cus());
    ns = ns > nc ? nc : ns;
    const long blocks = tiles * ns;
    if (blocks >= (1L << 31)) return FP_ERR_UNSUPPORTED;
    if (rows == 128)
      hipLaunchKernelGGL((cosine_topk_i8_kernel<2>), dim3((unsigned)blocks), dim3(256), lds, s, (const signed char*)Q8, u, (long)M,
                         (int)Mpad, (const signed char*)G8, w, N, (int)Npad, nc, D, pool, ns, floor0, (u64*)workspace);
    else
      hipLaunchKernelGGL((cosine_topk_i8_kernel<1>), dim3((unsigned)blocks), dim3(256), lds, s, (const signed char*)Q8, u, (long)M,
                         (int)Mpad, (const signed char*)G8, w, N, (int)Npad, nc, D, pool, ns, floor0, (u64*)workspace);
    FP_CHECK_LAUNCH();
    const int rc = fp_launch_topk_merge((const uint64_t*)workspace, M, ns * pool, pool, scores, idx, s);
    if (rc != FP_OK) return rc;
    if (last) break;
    floor0 = scores;
    level *= 8;
  }
  hipLaunchKernelGGL(coarse_scale_kernel, dim3((unsigned)fp_ceil_div((long)M * pool, 256)), dim3(256), 0, s, scores, idx, u, (long)M, pool);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_rerank_topk(const float* Q, const float* qinv, int64_t M, int D, const int32_t* cand, int pool, const float* G,
                   const float* rows, const float* ginv, int N, int k, float* scores, int32_t* idx, void* stream) {
  if (!Q || !qinv || !cand || !ginv || !scores || !idx || (G == nullptr) == (rows == nullptr)) return FP_ERR_INVALID_ARG;
  if (M < 0 || N <= 0 || D <= 0 || D > FP_QUANT_MAX_D || pool < 1 || pool > FP_COARSE_MAX || k < 1 || k > FP_TOPK_MAX || k > pool)
    return FP_ERR_INVALID_ARG;
  if (D % I8_K || ((uintptr_t)Q) % 16 || ((uintptr_t)(G ? G : rows)) % 16) return FP_ERR_ALIGNMENT;
  if (M == 0) return FP_OK;
  if (fp_ceil_div(M, 4) <= 0) return FP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(rerank_topk_kernel, dim3((unsigned)fp_ceil_div(M, 4)), dim3(256), 0, (hipStream_t)stream, Q, qinv, (long)M, D, cand,
                     pool, G, rows, ginv, N, k, scores, idx);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
