// pairhist.hip — score an embedder on labelled faces: the genuine / impostor histogram of ALL pairs (gfx950).  Build-defined,
// DESIGN §7 "Embedder evaluation".
//
// As cluster_walk_kernel (cluster.hip): the work list of triwalk.h over the upper triangle, walked by cw_walk (cosinewalk.h:
// planes of fp_split3_rows staged by LDS-DMA into a flat double buffer, row i split in registers, column j from the planes),
// s = acc * inv[i] * inv[j]; each unordered pair is evaluated once and `column > row` drops the diagonal and the lower half.
// Only the epilogue of a chunk differs, and it has to touch every pair (the DBSCAN walk leaves a 32 x 128 block with one ballot):
//   live:   inverse norm finite and non-zero AND label >= 0, folded into the padded inverse-norm copy by the init kernel (a
//           zero inverse norm is the library's mask, it becomes a NaN factor: one `s == s` covers dead rows, dead columns,
//           the padding and a NaN score);
//   bin:    t = (s - lo) * scale, two separately rounded fp32 operations (this file is built without FMA contraction),
//           b = t < 0 ? 0 : min((int)t, nbins - 1); scale = (float)(nbins / ((double)hi - lo)) comes from the host;
//   class:  labels[i] == labels[j] -> genuine[b], else impostor[b].
// A workgroup counts into ONE private histogram in LDS behind the staging buffer, [2][nbins] u32 (at most 16 chunks x 128^2
// = 262 144 pairs: no overflow), with one LDS atomic add per score and no branch (a pair that is not counted adds 0), and
// flushes it after its last chunk with one 64-bit global atomic add per non-empty bin.  Integer adds commute: two runs are
// bit-identical whatever the geometry.  LDS: 48 KiB + 8 nbins bytes -- up to 512 bins three workgroups share a CU as in
// the DBSCAN walk, above that two (FINDINGS 73 has both prices).
#include "cosinewalk.h"
#include "triwalk.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int PH_MAX_BINS = FP_PAIRHIST_MAX_BINS;
constexpr int PH_LDS_PER_CU = 160 * 1024;

__global__ __launch_bounds__(256, 3) void pair_histogram_kernel(const float* __restrict__ X, const float* __restrict__ inv,
                                                                 const int* __restrict__ lab, int N,
                                                                 const unsigned short* __restrict__ X3, int Npad, int D, int P,
                                                                 float lo, float scale, int nbins, u64* __restrict__ genuine,
                                                                 u64* __restrict__ impostor) {
  constexpr int MT = 2, NT16 = CW_NT16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned* hist = (unsigned*)(smem_raw + CW_LDS);       // behind the staging buffer: [2][nbins] genuine, impostor
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int nchunk = Npad / CW_NC;
  const cl_item it = cl_decode((long)gridDim.x - 1 - (long)fp_xcd_block(), nchunk, P);
  const int cb = __builtin_amdgcn_readfirstlane(it.first), nck = __builtin_amdgcn_readfirstlane(it.count);
  const long row0 = (long)__builtin_amdgcn_readfirstlane(it.tile) * CL_ROWS + wave * (MT * 16);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const float top = (float)(nbins - 1);
  const unsigned imp = (unsigned)nbins * 4u;              // byte offset of the impostor half

  for (int i = tid; i < 2 * nbins; i += 256) hist[i] = 0;   // seen by everyone behind the first barrier of the walk

  // rows past N - 1 read row N - 1, their inv is 0.  Epilogue of a chunk: lane = row 16 t + l15, columns c0 + 16 n + 4 q + i
  cw_walk<MT>(X, N, row0, X3, Npad, D, cb, nck, (unsigned short*)smem_raw, [&](int c0, f32x4 (&acc)[MT][NT16]) {
    float gi[MT];
    int rowi[MT], li[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      rowi[t] = (int)row0 + 16 * t + l15;                // < Npad
      gi[t] = cw_nan_if_zero(inv[rowi[t]]);              // not live / past N: every score is NaN and counts nowhere
      li[t] = lab[rowi[t]];
    }
#pragma unroll
    for (int n = 0; n < NT16; ++n) {
      const int colb = c0 + 16 * n + 4 * q;
      f32x4 rn = *(const f32x4*)(inv + colb);
      const i32x4 ln = *(const i32x4*)(lab + colb);
#pragma unroll
      for (int i = 0; i < 4; ++i) rn[i] = cw_nan_if_zero(rn[i]);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float sv = acc[t][n][i] * gi[t] * rn[i];
          const float tb = (sv - lo) * scale;
          const int b = (int)fminf(fmaxf(tb, 0.f), top);  // fmaxf(NaN, 0) = 0: the index stays inside the histogram
          const unsigned one = (sv == sv && colb + i > rowi[t]) ? 1u : 0u;
          unsigned* slot = (unsigned*)((unsigned char*)hist + (((unsigned)b << 2) + (li[t] == ln[i] ? 0u : imp)));
          __hip_atomic_fetch_add(slot, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        acc[t][n] = z;
      }
    }
  });

  __syncthreads();
  for (int i = tid; i < 2 * nbins; i += 256) {
    const unsigned v = hist[i];
    if (v) atomicAdd(i < nbins ? genuine + i : impostor + (i - nbins), (u64)v);
  }
}

// inv1 = the caller's inverse norms with rows that are not live (inverse norm 0 or not finite, or label < 0) and the padding
// as 0; lab1 = the labels, padded; both outputs zeroed.
__global__ __launch_bounds__(256) void pair_histogram_init_kernel(const float* __restrict__ xinv, const int* __restrict__ labels,
                                                                  int N, int Npad, int nbins, float* __restrict__ inv1,
                                                                  int* __restrict__ lab1, u64* __restrict__ genuine,
                                                                  u64* __restrict__ impostor) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < nbins) {
    genuine[i] = 0;
    impostor[i] = 0;
  }
  if (i >= Npad) return;
  float v = 0.f;
  int l = -1;
  if (i < N) {
    const float x = xinv[i];
    l = labels[i];
    v = (x != 0.f && fabsf(x) < __builtin_huge_valf() && l >= 0) ? x : 0.f;     // NaN compares false
  }
  inv1[i] = v;
  lab1[i] = l;
}

}  // namespace

extern "C" {

size_t fp_pair_histogram_workspace(int64_t N) {
  if (N <= 0 || N >= (1LL << 31)) return 0;
  return (size_t)fp_round_up(N, CW_NC) * 8;              // inv1, lab1
}

int fp_pair_histogram_x6(const float* X, const float* xinv, const void* X3, const int32_t* labels, int64_t N, int D, float lo,
                         float hi, int nbins, int64_t* genuine, int64_t* impostor, void* ws, size_t ws_bytes, void* stream) {
  if (!genuine || !impostor || N < 0 || D <= 0) return FP_ERR_INVALID_ARG;
  if (nbins < 2 || nbins > PH_MAX_BINS || !(lo < hi) || !(fabsf(lo) < __builtin_huge_valf()) || !(fabsf(hi) < __builtin_huge_valf()))
    return FP_ERR_INVALID_ARG;
  if (D % 32) return FP_ERR_INVALID_ARG;
  const float scale = (float)(nbins / ((double)hi - (double)lo));
  if (!(scale < __builtin_huge_valf())) return FP_ERR_INVALID_ARG;       // a range too narrow for fp32 bins
  if (N >= (1LL << 31)) return FP_ERR_UNSUPPORTED;
  if (N > 0 && (!X || !xinv || !X3 || !labels || !ws)) return FP_ERR_INVALID_ARG;
  if (N > 0 && (((uintptr_t)X) % 16 || ((uintptr_t)X3) % 16 || ((uintptr_t)ws) % 16)) return FP_ERR_ALIGNMENT;
  if (ws_bytes < fp_pair_histogram_workspace(N)) return FP_ERR_INVALID_ARG;
  const int n = (int)N, Npad = (int)fp_round_up(N, CW_NC), nchunk = Npad / CW_NC;
  const size_t lds = (size_t)CW_LDS + (size_t)nbins * 8;
  const int wg_per_cu = 3 * (size_t)fp_round_up((long)lds, 2048) <= (size_t)PH_LDS_PER_CU ? 3 : 2;   // allocation granules: 512 bins
  const long P = cl_chunks_per_group(nchunk, wg_per_cu);
  const long groups = cl_groups(nchunk, P);
  if (groups >= (1L << 31)) return FP_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  float* inv1 = (float*)ws;
  int* lab1 = (int*)((char*)ws + (size_t)Npad * 4);
  const int cover = Npad > nbins ? Npad : nbins;
  hipLaunchKernelGGL(pair_histogram_init_kernel, dim3((unsigned)fp_ceil_div(cover, 256)), dim3(256), 0, s, xinv, labels, n, Npad,
                     nbins, inv1, lab1, (u64*)genuine, (u64*)impostor);
  FP_CHECK_LAUNCH();
  if (N < 2) return FP_OK;                               // no pair
  hipLaunchKernelGGL(pair_histogram_kernel, dim3((unsigned)groups), dim3(256), lds, s, X, (const float*)inv1, (const int*)lab1, n,
                     (const unsigned short*)X3, Npad, D, (int)P, lo, scale, nbins, (u64*)genuine, (u64*)impostor);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
