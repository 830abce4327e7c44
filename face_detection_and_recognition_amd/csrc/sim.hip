// sim.hip — similarity filter kernels (gfx950).
//
//  * cosine filter (cosine formula of extract_and_label_faces_from_dataset.py:106):
//      best[g] = max_j <G[g], R[j]> / (|G[g]| |R[j]|),  arg, keep = best >= tau.
//    S = G R^T is a plain fp32 GEMM (K = D), computed tile by tile on v_mfma_f32_32x32x2_f32 and reduced
//    in the epilogue (row max over the tile with wavefront shuffles, then one 64-bit atomicMax per row and
//    tile) so the M x Nr score matrix is never written to HBM.
//  * L2-to-class-mean filter, the reference's actual semantics
//    (similar_face_filtering/filter_faces_using_reference.py:71-100,183-197).
#include "cosinewalk.h"

namespace {

constexpr int BM = 128, BN = 128, KC = 32, LDA = KC + 4;

__global__ __launch_bounds__(256) void cosine_tile_kernel(const float* __restrict__ G, const float* __restrict__ ginv,
                                                          long M, const float* __restrict__ R,
                                                          const float* __restrict__ rinv, int Nr, int D,
                                                          unsigned long long* __restrict__ packed) {
  __shared__ __attribute__((aligned(16))) float As[BM * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[BN * LDA];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, h = lane >> 5;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int c4 = tid & 7, r0 = tid >> 3;

  f32x4 areg[4], breg[4];
  auto load_chunk = [&](int kbase) {
    const int k = kbase + c4 * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long m = m0 + r0 + 32 * i;
      const int n = n0 + r0 + 32 * i;
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      areg[i] = (m < M && k < D) ? *(const f32x4*)(G + m * D + k) : z;
      breg[i] = (n < Nr && k < D) ? *(const f32x4*)(R + (long)n * D + k) : z;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(f32x4*)&As[(r0 + 32 * i) * LDA + c4 * 4] = areg[i];
      *(f32x4*)&Bs[(r0 + 32 * i) * LDA + c4 * 4] = breg[i];
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

  const int nchunks = (D + KC - 1) / KC;
  load_chunk(0);
  for (int ch = 0; ch < nchunks; ++ch) {
    store_chunk();
    __syncthreads();
    if (ch + 1 < nchunks) load_chunk((ch + 1) * KC);
    const float* arow = &As[(wave * 32 + lr) * LDA + 4 * h];
#pragma unroll
    for (int kq = 0; kq < KC / 8; ++kq) {
      const f32x4 a = *(const f32x4*)(arow + kq * 8);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const f32x4 b = *(const f32x4*)&Bs[(nb * 32 + lr) * LDA + kq * 8 + 4 * h];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc[nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  float rn[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int n = n0 + nb * 32 + lr;
    rn[nb] = n < Nr ? rinv[n] : 0.f;
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
    const long m = m0 + wave * 32 + row;
    const float gi = m < M ? ginv[m] : 0.f;
    float best = -__builtin_huge_valf();
    int bidx = 0x7FFFFFFF;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const int n = n0 + nb * 32 + lr;
      if (n < Nr) {
        const float s = acc[nb][reg] * gi * rn[nb];
        if (s > best) {  // nb ascending => smaller index wins ties
          best = s;
          bidx = n;
        }
      }
    }
    // max over the 32 lanes that hold this row (xor offsets < 32 stay inside the half-wave)
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off);
      const int oi = __shfl_xor(bidx, off);
      if (ob > best || (ob == best && oi < bidx)) {
        best = ob;
        bidx = oi;
      }
    }
    if (lr == 0 && m < M && bidx != 0x7FFFFFFF) atomicMax(&packed[m], cw_key(best, (unsigned)bidx));
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// The same filter with S = G R^T on the bf16 matrix cores (fp32-equivalent split arithmetic, split.h): the fp32 kernel above
// reaches 117 TFLOP/s = 74 % of the fp32 MFMA peak; six bf16 products per fp32 product have a peak of 417.
//   * R is split ONCE into three bf16 planes [D / 32][3][Npad][32] (split3_rows_kernel; the reference set of a filter run is
//     fixed) -- the B operand of cw_walk (cosinewalk.h), streamed slab by slab through LDS by LDS-DMA;
//   * a workgroup = 4 waves x (MT x 16) gallery rows x 128 reference columns, the one-chunk case of the walk; column chunks
//     of one row tile are adjacent in the grid, so the gallery rows are re-read from L2;
//   * swapped operands: a lane holds 4 consecutive COLUMNS of one gallery row per accumulator -> the row max over the lane's
//     32 columns is plain VALU, then two shuffles across the four k-groups, one 64-bit atomicMax per row and workgroup.
__global__ __launch_bounds__(256) void split3_rows_kernel(const float* __restrict__ R, int Nr, int D, int Npad,
                                                          unsigned short* __restrict__ out) {
  // one thread per (row n < Npad, 8 consecutive k): out[((k / 32) * 3 + pl) * Npad + n][k % 32]
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int k8 = D / 8;
  if (i >= (long)Npad * k8) return;
  const int n = (int)(i / k8), k = (int)(i - (long)n * k8) * 8;
  f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
  if (n < Nr) {
    a = *(const f32x4*)(R + (long)n * D + k);
    b = *(const f32x4*)(R + (long)n * D + k + 4);
  }
  const fp_frag3 f = fp_split8(a, b);
  unsigned short* o = out + ((long)((k / 32) * 3) * Npad + n) * 32 + (k % 32);
  *(u32x4*)o = f.h;
  *(u32x4*)(o + (long)Npad * 32) = f.m;
  *(u32x4*)(o + 2L * Npad * 32) = f.l;
}

template <int MT>
__global__ __launch_bounds__(256, MT == 4 ? 2 : 3) void cosine_x6_kernel(const float* __restrict__ G, const float* __restrict__ ginv,
                                                                          long M, const unsigned short* __restrict__ R3,
                                                                          const float* __restrict__ rinv, int Nr, int Npad, int D,
                                                                          unsigned long long* __restrict__ packed) {
  constexpr int NT16 = CW_NT16, XBM = 4 * MT * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int nchunk = Npad / CW_NC;
  const unsigned vb = fp_xcd_block();                    // the reference chunks of one gallery row tile on ONE XCD (gallery rows from its L2)
  const long row0 = (long)(vb / nchunk) * XBM + wave * (MT * 16);

  // one chunk; its epilogue: lane = gallery row 16 t + l15, reference columns c0 + 16 n + 4 q + i
  cw_walk<MT>(G, M, row0, R3, Npad, D, (int)(vb % nchunk), 1, (unsigned short*)smem_raw, [&](int c0, f32x4 (&acc)[MT][NT16]) {
    f32x4 rn[NT16];
#pragma unroll
    for (int n = 0; n < NT16; ++n) {
      const int col = c0 + 16 * n + 4 * q;
      if (col + 3 < Nr) {
        rn[n] = *(const f32x4*)(rinv + col);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) rn[n][i] = col + i < Nr ? rinv[col + i] : 0.f;
      }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const long m = row0 + 16 * t + l15;
      const float gi = m < M ? ginv[m] : 0.f;
      float best = -__builtin_huge_valf();
      int bidx = 0x7FFFFFFF;
#pragma unroll
      for (int n = 0; n < NT16; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int col = c0 + 16 * n + 4 * q + i;
          if (col < Nr) {
            const float sv = acc[t][n][i] * gi * rn[n][i];
            if (sv > best || (sv == best && col < bidx)) {
              best = sv;
              bidx = col;
            }
          }
        }
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {                  // the four k-group lanes of this row
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bidx, off);
        if (ob > best || (ob == best && oi < bidx)) {
          best = ob;
          bidx = oi;
        }
      }
      if (q == 0 && m < M && bidx != 0x7FFFFFFF) atomicMax(&packed[m], cw_key(best, (unsigned)bidx));
    }
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// Top-k search (identify against an enrolled gallery): S = Q G^T on the same walk as cosine_x6_kernel (gallery planes
// from split3_rows_kernel, queries split in registers, score = acc * qinv[m] * ginv[n]), reduced to the k
// best columns of every row.  One 64-bit atomicMax cannot carry k candidates, so the grid is (row tile) x (split): a
// workgroup walks a CONTIGUOUS range of 128-column chunks (cw_walk, cosinewalk.h: one flat, double-buffered pipeline) and
// keeps a running top-k per row in LDS, as sorted 64-bit keys (cw_key: larger = better, higher score, then LOWER column;
// 0 = empty slot).
// The keys of all candidates are distinct and totally ordered, so the k largest are one well-defined set: inserting in any
// order, in any partition of the columns, gives the same list -- the result does not depend on n_splits, on the order in
// which lanes insert, or on workgroup scheduling.
//   * epilogue of a chunk: a lane holds 4 consecutive columns of one row per accumulator; it keeps the row's k-th best
//     score in a register and compares the maximum of the 4 with it (3 v_max + 1 compare per 4 candidates); only a group
//     that reaches it takes the insertion path.  A masked column (ginv == 0) or one past N carries a NaN factor: its score
//     compares false and never enters.
//   * insertion path: the four lanes that share a row (q = 0..3) take turns -- a lane goes when no lower-q lane of its
//     row is pending (one ballot) -- and the lists are private to the wave that owns the rows: no barrier, LDS operations
//     of one wave complete in program order.
//   * the list leaves the workgroup once, as k keys per (row, split); topk_merge_kernel picks the k largest keys of a
//     row's n_splits lists (one wave per row) and unpacks them.
template <int MT>
__global__ __launch_bounds__(256, 3) void cosine_topk_x6_kernel(const float* __restrict__ Q, const float* __restrict__ qinv,
                                                                               long M, const unsigned short* __restrict__ G3,
                                                                               const float* __restrict__ ginv, int N, int Npad, int D,
                                                                               int k, int n_splits,
                                                                               unsigned long long* __restrict__ partial) {
  constexpr int NT16 = CW_NT16, XBM = 4 * MT * 16;
  typedef unsigned long long u64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  volatile u64* Ls = (volatile u64*)(smem_raw + CW_LDS);   // behind the staging buffer: [XBM][LS] running top-k keys, descending
  const int LS = k | 1;                                  // odd stride: the rows' k-th entries fall in different banks
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int nchunk = Npad / CW_NC;
  const unsigned vb = fp_xcd_block();                    // the splits of one row tile on ONE XCD (query rows from its L2)
  const int split = vb % (unsigned)n_splits;
  const long row0 = (long)(vb / (unsigned)n_splits) * XBM + wave * (MT * 16);
  // chunks [cb, cb + nck) of this split: nchunk = n_splits * base + rem, the first rem splits take one more
  const int base = nchunk / n_splits, rem = nchunk - base * n_splits;
  const int cb = split * base + (split < rem ? split : rem);
  const int nck = base + (split < rem ? 1 : 0);          // >= 1 (the launcher clamps n_splits to nchunk)
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const float ninf = -__builtin_huge_valf(), qnan = __builtin_nanf("");

  for (int i = lane; i < MT * 16 * LS; i += 64) Ls[wave * (MT * 16) * LS + i] = 0;
  u64 lower = 0;                                         // the lanes of my row with a smaller q
  for (int qq = 0; qq < q; ++qq) lower |= 1ull << (l15 + 16 * qq);
  float thr[MT];                                         // the k-th best score of my rows so far
#pragma unroll
  for (int t = 0; t < MT; ++t) thr[t] = ninf;

  // epilogue of a chunk: lane = query row 16 t + l15, gallery columns c0 + 16 n + 4 q + i
  cw_walk<MT>(Q, M, row0, G3, Npad, D, cb, nck, (unsigned short*)smem_raw, [&](int c0, f32x4 (&acc)[MT][NT16]) {
    float gi[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const long m = row0 + 16 * t + l15;
      gi[t] = m < M ? qinv[m] : qnan;
    }
#pragma unroll
    for (int n = 0; n < NT16; ++n) {
      const int colb = c0 + 16 * n + 4 * q;
      f32x4 rn;
      if (colb + 3 < N) {
        rn = *(const f32x4*)(ginv + colb);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) rn[i] = colb + i < N ? ginv[colb + i] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) rn[i] = cw_nan_if_zero(rn[i]);            // masked / padding: never a candidate
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        volatile u64* Lr = Ls + (wave * (MT * 16) + 16 * t + l15) * LS;
        f32x4 sv;
#pragma unroll
        for (int i = 0; i < 4; ++i) sv[i] = acc[t][n][i] * gi[t] * rn[i];
        acc[t][n] = z;
        // fmaxf drops NaNs: the maximum of the valid candidates (NaN if none is)
        const float mx = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
        if (__ballot(mx >= thr[t]) == 0) continue;       // the common case: nothing in this group reaches the k-th best
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
          const float v = i == 0 ? sv[0] : i == 1 ? sv[1] : i == 2 ? sv[2] : sv[3];
          bool pend = v >= thr[t];
          const u64 key = cw_key(v, (unsigned)(colb + i));
          for (;;) {
            const u64 mask = __ballot(pend);
            if (!mask) break;
            if (pend && !(mask & lower)) {               // my turn: no lower-q lane of my row is waiting
              pend = false;
              if (key > Lr[k - 1]) {
                int j = k - 1;
                while (j > 0) {
                  const u64 p = Lr[j - 1];
                  if (p > key) break;
                  Lr[j] = p;
                  --j;
                }
                Lr[j] = key;
              }
            }
            __builtin_amdgcn_wave_barrier();
          }
        }
        const u64 kth = Lr[k - 1];
        thr[t] = kth ? cw_key_score(kth) : ninf;
      }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {                         // other lanes of the row may have raised it
      const u64 kth = Ls[(wave * (MT * 16) + 16 * t + l15) * LS + k - 1];
      thr[t] = kth ? cw_key_score(kth) : ninf;
    }
  });

  // the lists of this wave's rows -> partial[m][split][0 .. k)
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < MT * 16 * k; i += 64) {
    const int r = i / k, j = i - r * k;
    const long m = row0 + r;
    if (m < M) partial[(m * n_splits + split) * k + j] = Ls[(wave * (MT * 16) + r) * LS + j];
  }
}

// One wave per row: the k largest of the row's n_splits * k keys (all distinct, except empty slots = 0), descending, unpacked.
__global__ __launch_bounds__(256) void topk_merge_kernel(const unsigned long long* __restrict__ partial, long M, int cnt, int k,
                                                         float* __restrict__ scores, int* __restrict__ idx) {
  typedef unsigned long long u64;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int lane = threadIdx.x & 63;
  const u64* p = partial + m * cnt;
  u64 prev = ~0ull, mine = 0;
  for (int j = 0; j < k; ++j) {
    u64 best = 0;
    for (int e = lane; e < cnt; e += 64) {
      const u64 v = p[e];
      if (v < prev && v > best) best = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const u64 o = __shfl_xor(best, off);
      best = o > best ? o : best;
    }
    if (lane == j) mine = best;
    prev = best;                                         // 0 once the keys run out: every later round finds nothing
    if (best == 0) break;
  }
  if (lane < k) {
    scores[m * k + lane] = mine ? cw_key_score(mine) : -__builtin_huge_valf();
    idx[m * k + lane] = mine ? cw_key_index(mine) : -1;
  }
}

// fp_topk_vote: one thread per row of a (M, k) top-k result.
__global__ __launch_bounds__(256) void topk_vote_kernel(const float* __restrict__ scores, const int* __restrict__ idx, long M, int k,
                                                        const int* __restrict__ labels, int N, float tau, int mode,
                                                        int* __restrict__ out_label, float* __restrict__ out_score,
                                                        int* __restrict__ out_votes) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const float* s = scores + m * k;
  const int* ix = idx + m * k;
  auto passes = [&](int j) { return ix[j] >= 0 && ix[j] < N && s[j] >= tau; };
  int wl = -1, wv = 0;
  float wbest = s[0], wsum = 0.f;
  if (mode == 0) {
    if (passes(0)) wl = labels[ix[0]], wv = 1;
  } else {
    for (int j = 0; j < k; ++j) {
      if (!passes(j)) continue;
      const int lab = labels[ix[j]];
      bool first = true;
      for (int i = 0; i < j; ++i) first = first && !(passes(i) && labels[ix[i]] == lab);
      if (!first) continue;                              // counted at the label's first candidate (its best score: rows are descending)
      int v = 0;
      float sum = 0.f;
      for (int i = j; i < k; ++i)
        if (passes(i) && labels[ix[i]] == lab) ++v, sum += s[i];
      if (wl < 0 || v > wv || (v == wv && (sum > wsum || (sum == wsum && lab < wl)))) wl = lab, wv = v, wsum = sum, wbest = s[j];
    }
  }
  out_label[m] = wl;
  out_score[m] = wbest;
  out_votes[m] = wv;
}

__global__ __launch_bounds__(256) void cosine_finalize_kernel(const unsigned long long* __restrict__ packed, long M,
                                                              float tau, float* __restrict__ best,
                                                              int* __restrict__ arg, unsigned char* __restrict__ keep) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const unsigned long long key = packed[m];
  const float s = cw_key_score(key);
  best[m] = s;
  arg[m] = cw_key_index(key);
  keep[m] = s >= tau ? 1 : 0;
}

__global__ __launch_bounds__(256) void row_inv_norm_kernel(const float* __restrict__ x, long M, int D,
                                                           float* __restrict__ inv) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const float* p = x + row * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s += p[i] * p[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) inv[row] = 1.0f / sqrtf(s);
}

// mean over R rows (sequential row order, like np.mean(axis=0) on a C-contiguous array), then
// thres = max_i ||mean - f_i||  (filter_faces_using_reference.py:86-99).  One workgroup.
__global__ __launch_bounds__(256) void l2_mean_thres_kernel(const float* __restrict__ ref, int R, int D,
                                                            float* __restrict__ mean, float* __restrict__ thres) {
  __shared__ float wmax[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int d = tid; d < D; d += 256) {
    float s = 0.f;
    for (int i = 0; i < R; ++i) s += ref[(long)i * D + d];
    mean[d] = s / (float)R;
  }
  __threadfence_block();
  __syncthreads();
  float mx = 0.f;
  for (int i = wave; i < R; i += 4) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float t = mean[d] - ref[(long)i * D + d];
      s += t * t;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    mx = fmaxf(mx, sqrtf(s));
  }
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  if (tid == 0) thres[0] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// dist = ||e - mean||, keep = dist <= thres (filter_faces_using_reference.py:189).  One wave per row.
__global__ __launch_bounds__(256) void l2_filter_kernel(const float* __restrict__ E, long M, int D,
                                                        const float* __restrict__ mean, const float* __restrict__ thres,
                                                        float* __restrict__ dist, unsigned char* __restrict__ keep) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const float* p = E + row * D;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float t = p[d] - mean[d];
    s += t * t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) {
    const float dd = sqrtf(s);
    dist[row] = dd;
    keep[row] = dd <= thres[0] ? 1 : 0;
  }
}

}  // namespace

extern "C" {

int fp_row_inv_norm(const float* x, int64_t M, int D, float* inv_norm, void* stream) {
  if (!x || !inv_norm || M < 0 || D <= 0) return FP_ERR_INVALID_ARG;
  if (M == 0) return FP_OK;
  hipLaunchKernelGGL(row_inv_norm_kernel, dim3((unsigned)fp_ceil_div(M, 4)), dim3(256), 0, (hipStream_t)stream, x,
                     (long)M, D, inv_norm);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_cosine_filter(const float* G, const float* ginv, int64_t M, const float* R, const float* rinv, int Nr, int D,
                     float tau, float* best, int32_t* arg, uint8_t* keep, uint64_t* packed, void* stream) {
  if (!G || !ginv || !R || !rinv || !best || !arg || !keep || !packed) return FP_ERR_INVALID_ARG;
  if (M < 0 || Nr <= 0 || D <= 0) return FP_ERR_INVALID_ARG;
  if (D % 4 || ((uintptr_t)G) % 16 || ((uintptr_t)R) % 16) return FP_ERR_ALIGNMENT;
  if (M == 0) return FP_OK;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(packed, 0, (size_t)M * sizeof(uint64_t), s) != hipSuccess) {
    fp_set_hip_error(hipGetLastError());
    return FP_ERR_LAUNCH;
  }
  dim3 grid((unsigned)fp_ceil_div(M, BM), (unsigned)fp_ceil_div(Nr, BN));
  hipLaunchKernelGGL(cosine_tile_kernel, grid, dim3(256), 0, s, G, ginv, (long)M, R, rinv, Nr, D,
                     (unsigned long long*)packed);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(cosine_finalize_kernel, dim3((unsigned)fp_ceil_div(M, 256)), dim3(256), 0, s,
                     (const unsigned long long*)packed, (long)M, tau, best, arg, keep);
  FP_CHECK_LAUNCH();
  return FP_OK;
}


size_t fp_split3_bytes(int Nr, int D) { return (size_t)(D / 32) * 3 * (size_t)fp_round_up(Nr, CW_NC) * 32 * 2; }

int fp_split3_rows(const float* R, int Nr, int D, void* out, void* stream) {
  if (!R || !out || Nr <= 0 || D <= 0) return FP_ERR_INVALID_ARG;
  if (D % 32 || ((uintptr_t)R) % 16 || ((uintptr_t)out) % 16) return FP_ERR_ALIGNMENT;
  const int Npad = (int)fp_round_up(Nr, CW_NC);
  const long items = (long)Npad * (D / 8);
  hipLaunchKernelGGL(split3_rows_kernel, dim3((unsigned)fp_ceil_div(items, 256)), dim3(256), 0, (hipStream_t)stream, R, Nr, D, Npad,
                     (unsigned short*)out);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

// 256-row tiles (two workgroups per CU) when they fill several rounds of workgroups, else 128-row tiles (three per CU).  The one
// place where fp_cosine_filter_x6's form is chosen; 0: a grid the launcher refuses.
int fp_cosine_filter_x6_tile_rows(int64_t M, int Nr) {
  if (M < 0 || Nr <= 0) return 0;
  const long nchunk = fp_round_up(Nr, CW_NC) / CW_NC;
  const long big = (M + 255) / 256 * nchunk;
  if (big >= (1L << 31)) return 0;
  return big >= 2048 ? 256 : 128;
}

int fp_cosine_filter_x6(const float* G, const float* ginv, int64_t M, const void* R3, const float* rinv, int Nr, int D,
                        float tau, float* best, int32_t* arg, uint8_t* keep, uint64_t* packed, void* stream) {
  if (!G || !ginv || !R3 || !rinv || !best || !arg || !keep || !packed) return FP_ERR_INVALID_ARG;
  if (M < 0 || Nr <= 0 || D <= 0) return FP_ERR_INVALID_ARG;
  if (D % 32 || ((uintptr_t)G) % 16 || ((uintptr_t)R3) % 16 || ((uintptr_t)rinv) % 16) return FP_ERR_ALIGNMENT;
  if (M == 0) return FP_OK;
  const int tile_rows = fp_cosine_filter_x6_tile_rows(M, Nr);
  if (!tile_rows) return FP_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(packed, 0, (size_t)M * sizeof(uint64_t), s) != hipSuccess) {
    fp_set_hip_error(hipGetLastError());
    return FP_ERR_LAUNCH;
  }
  const int Npad = (int)fp_round_up(Nr, CW_NC);
  const long nchunk = Npad / CW_NC;
  const long tiles = (M + tile_rows - 1) / tile_rows * nchunk;
  if (tile_rows == 256) {
    hipLaunchKernelGGL((cosine_x6_kernel<4>), dim3((unsigned)tiles), dim3(256), CW_LDS, s, G, ginv, (long)M, (const unsigned short*)R3, rinv,
                       Nr, Npad, D, (unsigned long long*)packed);
  } else {
    hipLaunchKernelGGL((cosine_x6_kernel<2>), dim3((unsigned)tiles), dim3(256), CW_LDS, s, G, ginv, (long)M, (const unsigned short*)R3, rinv,
                       Nr, Npad, D, (unsigned long long*)packed);
  }
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(cosine_finalize_kernel, dim3((unsigned)fp_ceil_div(M, 256)), dim3(256), 0, s,
                     (const unsigned long long*)packed, (long)M, tau, best, arg, keep);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"

namespace {
// 128-row tiles (MT = 2).  The 256-row form of cosine_x6_kernel does not fit here: the flat chunk loop and the rows' thresholds
// on top of its 250 registers spill (checked with tools/kernel_resources.py), and a spill is worse than the smaller tile.
constexpr int TOPK_ROWS = 128;
// splits of the column range, from M, k and the CU count, never from N.  slots = workgroups the device holds at once (three per
// CU while the key lists leave room beside the B slabs, k <= 5, else two).  Row tiles that fill the slots alone are not split
// (measured, 125 000 rows x 10 000 x 512, k = 5: 7.20 ms unsplit, 7.66 / 8.28 / 9.49 ms at 2 / 4 / 8 splits: every split pays the
// ramp in which a list fills); fewer tiles are split into TOPK_ROUNDS rounds of the slots (512 rows x 1 000 000: 3.36 ms at 384
// splits, 3.68 at 64, 3.90 at 768).
constexpr int TOPK_ROUNDS = 2;
int topk_auto_splits(int64_t M, int k, int cus) {
  const long tiles = (M + TOPK_ROWS - 1) / TOPK_ROWS;
  const long slots = (long)(k <= 5 ? 3 : 2) * cus;
  if (tiles >= slots) return 1;
  const long s = (TOPK_ROUNDS * slots + tiles - 1) / (tiles > 0 ? tiles : 1);
  return (int)(s > 4096 ? 4096 : s);
}
}  // namespace

extern "C" {

size_t fp_cosine_topk_workspace(int64_t M, int N, int k, int n_splits) {
  if (M <= 0 || N <= 0 || k < 1 || k > FP_TOPK_MAX || n_splits < 0) return 0;
  const size_t nchunk = (size_t)(fp_round_up(N, CW_NC) / CW_NC);
  if (n_splits) return (size_t)M * (nchunk < (size_t)n_splits ? nchunk : (size_t)n_splits) * (size_t)k * sizeof(uint64_t);
  // automatic: a bound on M * n_splits that grows with M and k whatever the choice rounds to -- tiles * n_splits is at most
  // (workgroups wanted at the smallest k) + tiles, and never above tiles * nchunk
  const size_t tiles = (size_t)((M + TOPK_ROWS - 1) / TOPK_ROWS);
  const size_t want = (size_t)TOPK_ROUNDS * 3 * fp_num_cus() + tiles;
  const size_t lists = tiles * nchunk < want ? tiles * nchunk : want;
  return lists * TOPK_ROWS * (size_t)k * sizeof(uint64_t);
}

int fp_cosine_topk_x6(const float* Q, const float* qinv, int64_t M, const void* G3, const float* ginv, int N, int D, int k,
                      int n_splits, float* scores, int32_t* idx, void* workspace, size_t ws_bytes, void* stream) {
  if (!Q || !qinv || !G3 || !ginv || !scores || !idx || !workspace) return FP_ERR_INVALID_ARG;
  if (M < 0 || N <= 0 || D <= 0 || k < 1 || k > FP_TOPK_MAX || n_splits < 0) return FP_ERR_INVALID_ARG;
  if (D % 32 || ((uintptr_t)Q) % 16 || ((uintptr_t)G3) % 16 || ((uintptr_t)ginv) % 16 || ((uintptr_t)workspace) % 8)
    return FP_ERR_ALIGNMENT;
  if (M == 0) return FP_OK;
  if (ws_bytes < fp_cosine_topk_workspace(M, N, k, n_splits)) return FP_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int Npad = (int)fp_round_up(N, CW_NC);
  const int nchunk = Npad / CW_NC;
  const int cus = fp_num_cus();
  int ns = n_splits ? n_splits : topk_auto_splits(M, k, cus);
  ns = ns > nchunk ? nchunk : ns;
  const int rows = TOPK_ROWS;
  const long blocks = (M + rows - 1) / rows * ns;
  if (blocks >= (1L << 31)) return FP_ERR_UNSUPPORTED;
  const int lds = CW_LDS + rows * (k | 1) * 8;        // B slabs + the rows' key lists: 53 KiB at k = 5 (three per CU), 65 KiB at 16 (two)
  static bool attr_set = false;                          // dynamic LDS above 64 KiB (k > 14) needs the attribute
  if (!attr_set) {
    const int mx = CW_LDS + TOPK_ROWS * (FP_TOPK_MAX | 1) * 8;
    if (hipFuncSetAttribute((const void*)cosine_topk_x6_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, mx) != hipSuccess) {
      fp_set_hip_error(hipGetLastError());
      return FP_ERR_LAUNCH;
    }
    attr_set = true;
  }
  unsigned long long* part = (unsigned long long*)workspace;
  hipLaunchKernelGGL((cosine_topk_x6_kernel<2>), dim3((unsigned)blocks), dim3(256), lds, s, Q, qinv, (long)M, (const unsigned short*)G3,
                     ginv, N, Npad, D, k, ns, part);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)fp_ceil_div(M, 4)), dim3(256), 0, s, (const unsigned long long*)part, (long)M,
                     ns * k, k, scores, idx);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"

// topk_merge_kernel for the other searches that keep cw_key lists (simi8.hip): cnt keys per row, the k <= 64 largest unpacked.
int fp_launch_topk_merge(const uint64_t* partial, int64_t M, int cnt, int k, float* scores, int32_t* idx, hipStream_t s) {
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)fp_ceil_div(M, 4)), dim3(256), 0, s, (const unsigned long long*)partial, (long)M,
                     cnt, k, scores, idx);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

extern "C" {

int fp_topk_vote(const float* scores, const int32_t* idx, int64_t M, int k, const int32_t* labels, int N, float tau, int mode,
                 int32_t* out_label, float* out_score, int32_t* out_votes, void* stream) {
  if (!scores || !idx || !labels || !out_label || !out_score || !out_votes) return FP_ERR_INVALID_ARG;
  if (M < 0 || N <= 0 || k < 1 || k > FP_TOPK_MAX || (mode != 0 && mode != 1)) return FP_ERR_INVALID_ARG;
  if (M == 0) return FP_OK;
  hipLaunchKernelGGL(topk_vote_kernel, dim3((unsigned)fp_ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, scores, idx, (long)M, k,
                     labels, N, tau, mode, out_label, out_score, out_votes);
  FP_CHECK_LAUNCH();
  return FP_OK;
}
int fp_l2_mean_thres(const float* ref, int R, int D, float* out_mean, float* out_thres, void* stream) {
  if (!ref || !out_mean || !out_thres || R <= 0 || D <= 0) return FP_ERR_INVALID_ARG;
  hipLaunchKernelGGL(l2_mean_thres_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ref, R, D, out_mean, out_thres);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_l2_filter(const float* E, int64_t M, int D, const float* mean, const float* thres, float* dist, uint8_t* keep,
                 void* stream) {
  if (!E || !mean || !thres || !dist || !keep || M < 0 || D <= 0) return FP_ERR_INVALID_ARG;
  if (M == 0) return FP_OK;
  hipLaunchKernelGGL(l2_filter_kernel, dim3((unsigned)fp_ceil_div(M, 4)), dim3(256), 0, (hipStream_t)stream, E, (long)M,
                     D, mean, thres, dist, keep);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
