// cosinewalk.h — the one tile walk under every cosine kernel on the split matrix cores (sim.hip: cosine_x6_kernel,
// cosine_topk_x6_kernel; cluster.hip: cluster_walk_kernel; pairhist.hip: pair_histogram_kernel), and what goes with it: the
// tile constants, the (score, index) keys and the mask of a zero inverse norm.  The kernels differ in which chunks a workgroup
// owns and in what they do with a finished chunk (the epilogue), not in how A · Bᵀ is computed.
#pragma once
#include "split.h"

typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* gbl_ptr;

constexpr int CW_NC = 128;                 // columns of a chunk (the planes of fp_split3_rows are padded to a multiple)
constexpr int CW_NT16 = CW_NC / 16;        // 16-column accumulators of a chunk
constexpr int CW_SLAB = 3 * CW_NC * 32;    // bf16 elements of one k-slab of a chunk: [3 planes][NC][32]
constexpr int CW_LDS = 2 * CW_SLAB * 2;    // bytes of the staging buffer: two slabs

// ---- keys: ord(score) << 32 | ~index.  Larger = better: the higher score, then the LOWER index; one 64-bit max (atomic or
// not) picks the winner.  ord() maps the floats to unsigned in their order; 0 is no key of a real score (an empty slot).
__device__ __forceinline__ unsigned long long cw_key(float score, unsigned index) {
  const unsigned u = __float_as_uint(score);
  const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)o << 32) | (0xFFFFFFFFu - index);
}
__device__ __forceinline__ float cw_key_score(unsigned long long key) {
  const unsigned o = (unsigned)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ int cw_key_index(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

// The final merge of the searches that keep cw_key lists (sim.hip: topk_merge_kernel, one wave per row: the k <= 64 largest of a
// row's cnt keys, unpacked), shared with the int8 coarse search (simi8.hip).
int fp_launch_topk_merge(const uint64_t* partial, int64_t M, int cnt, int k, float* scores, int32_t* idx, hipStream_t s);

// A zero inverse norm is the library's mask (a dead row, the padding): as a NaN factor every score it enters compares false.
__device__ __forceinline__ float cw_nan_if_zero(float inv) { return inv == 0.f ? __builtin_nanf("") : inv; }

// ---- the walk.  A workgroup of 4 waves; a wave owns the MT x 16 rows of A (fp32, A_rows x D, D % 32 == 0) from row0 and
// computes them against the chunks [cb, cb + nck) of B, given as the planes of fp_split3_rows ([D / 32][3][Npad][32] bf16).
//   * B goes plane by plane through LDS by LDS-DMA, one k-slab of 32 per step, into the two slabs at Bl (CW_LDS bytes): the
//     steps of all chunks form ONE flat double-buffered pipeline with ONE barrier per step -- behind it every wave has left
//     the slab of the step before, which the DMA of the next step then overwrites while this step's slab is read; the next
//     chunk's first slab is staged under the last MFMAs of this one.  All four waves must make the same calls (barriers).
//   * A goes global -> registers -> fp_split8, one step ahead.  Rows past the end read row A_rows - 1 (their results are the
//     caller's to drop); for a wave wholly past the end (row0 >= A_rows) that offset from row0 is negative.  Offsets are
//     32-bit: at most 64 rows x D floats.
//   * swapped operands: per accumulator acc[t][n] a lane holds row 16 t + (lane & 15) x the 4 CONSECUTIVE columns
//     c0 + 16 n + 4 (lane >> 4) + i of the chunk.
// After the last k-slab of a chunk the walk calls epi(c0, acc), c0 the chunk's first column.  The epilogue leaves every
// accumulator it has consumed at zero (the walk zeroes them only once, before the first chunk); after the last chunk it need not.
template <int MT, class Epi>
__device__ __forceinline__ void cw_walk(const float* __restrict__ A, long A_rows, long row0, const unsigned short* __restrict__ B3,
                                        int Npad, int D, int cb, int nck, unsigned short* Bl, Epi&& epi) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int KS = D / 32;

  auto stage = [&](int chunk, int ks, int buf) {
    unsigned char* dst = (unsigned char*)(Bl + buf * CW_SLAB);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      const unsigned char* src = (const unsigned char*)(B3 + ((long)(ks * 3 + pl) * Npad + (long)chunk * CW_NC) * 32) + lane * 16;
#pragma unroll
      for (int j = 0; j < CW_NT16 / 4; ++j) {
        const int c = j * 4 + wave;
        __builtin_amdgcn_global_load_lds((gbl_ptr)(src + c * 1024), (lds_ptr)(dst + (pl * CW_NC * 32 + c * 512) * 2), 16, 0, 0);
      }
    }
  };
  const float* Aw = A + fp_uniform(row0 * D);             // this wave's rows
  int arow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    long r = row0 + 16 * t + l15;
    r = r < A_rows ? r : A_rows - 1;
    arow[t] = (int)(r - row0) * D + 8 * q;
  }
  f32x4 araw[MT][2];
  auto load_a = [&](int ks) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      araw[t][0] = *(const f32x4*)(Aw + arow[t] + 32 * ks);
      araw[t][1] = *(const f32x4*)(Aw + arow[t] + 32 * ks + 4);
    }
  };
  f32x4 acc[MT][CW_NT16];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int n = 0; n < CW_NT16; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int steps = nck * KS;
  int ks = 0, chunk = cb;                                // of the step being computed
  stage(cb, 0, 0);
  load_a(0);
  for (int s = 0; s < steps; ++s) {
    fp_frag3 af[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) af[t] = fp_split8(araw[t][0], araw[t][1]);
    __syncthreads();
    if (s + 1 < steps) {
      const bool last = ks + 1 == KS;
      stage(last ? chunk + 1 : chunk, last ? 0 : ks + 1, (s + 1) & 1);
      load_a(last ? 0 : ks + 1);
    }
    const unsigned short* Bc = Bl + (s & 1) * CW_SLAB + (l15 * 32 + 8 * q);
    fp_frag3 bf[2];
    auto ldb = [&](int n, fp_frag3& b) {
      b.h = *(const u32x4*)(Bc + n * 512);
      b.m = *(const u32x4*)(Bc + CW_NC * 32 + n * 512);
      b.l = *(const u32x4*)(Bc + 2 * CW_NC * 32 + n * 512);
    };
    ldb(0, bf[0]);
#pragma unroll
    for (int n = 0; n < CW_NT16; ++n) {
      if (n + 1 < CW_NT16) ldb(n + 1, bf[(n + 1) & 1]);
      const fp_frag3& b = bf[n & 1];
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t][n] = fp_mfma_x6(b.h, b.m, b.l, af[t].h, af[t].m, af[t].l, acc[t][n]);
    }
    if (++ks < KS) continue;
    ks = 0;
    epi(chunk * CW_NC, acc);
    ++chunk;
  }
}
