// pairhist.hip — score an embedder on labelled faces: the genuine / impostor histogram of ALL pairs (gfx950).  Build-defined,
// DESIGN §7 "Embedder evaluation".
//
// The walk is cluster_walk_kernel's (cluster.hip): the work list of triwalk.h over the upper triangle, planes of fp_split3_rows
// staged by LDS-DMA into a flat double buffer, row i split in registers, column j from the planes, fp_mfma_x6,
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
#include "split.h"
#include "triwalk.h"

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* gbl_ptr;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int PH_MAX_BINS = FP_PAIRHIST_MAX_BINS;
constexpr int PH_LDS_PER_CU = 160 * 1024;

__global__ __launch_bounds__(256, 3) void pair_histogram_kernel(const float* __restrict__ X, const float* __restrict__ inv,
                                                                 const int* __restrict__ lab, int N,
                                                                 const unsigned short* __restrict__ X3, int Npad, int D, int P,
                                                                 float lo, float scale, int nbins, u64* __restrict__ genuine,
                                                                 u64* __restrict__ impostor) {
  constexpr int MT = 2, NT16 = 8, NC = CL_NC, SLAB = 3 * NC * 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned short* Bl = (unsigned short*)smem_raw;        // [2][3][NC][32]
  unsigned* hist = (unsigned*)(smem_raw + CL_LDS);       // [2][nbins]: genuine, impostor
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int nchunk = Npad / NC;
  const cl_item it = cl_decode((long)gridDim.x - 1 - (long)fp_xcd_block(), nchunk, P);
  const int cb = __builtin_amdgcn_readfirstlane(it.first), nck = __builtin_amdgcn_readfirstlane(it.count);
  const long row0 = (long)__builtin_amdgcn_readfirstlane(it.tile) * CL_ROWS + wave * (MT * 16);
  const int KS = D / 32;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const float qnan = __builtin_nanf("");
  const float top = (float)(nbins - 1);
  const unsigned imp = (unsigned)nbins * 4u;              // byte offset of the impostor half

  for (int i = tid; i < 2 * nbins; i += 256) hist[i] = 0;   // seen by everyone behind the first barrier of the loop

  auto stage = [&](int chunk, int ks, int buf) {
    unsigned char* dst = (unsigned char*)(Bl + buf * SLAB);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      const unsigned char* src = (const unsigned char*)(X3 + ((long)(ks * 3 + pl) * Npad + (long)chunk * NC) * 32) + lane * 16;
#pragma unroll
      for (int j = 0; j < NT16 / 4; ++j) {
        const int c = j * 4 + wave;
        __builtin_amdgcn_global_load_lds((gbl_ptr)(src + c * 1024), (lds_ptr)(dst + (pl * NC * 32 + c * 512) * 2), 16, 0, 0);
      }
    }
  };
  const float* Xw = X + fp_uniform(row0 * D);             // this wave's rows (rows past N - 1 read row N - 1, their inv is 0)
  int arow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    long r = row0 + 16 * t + l15;
    r = r < N ? r : N - 1;
    arow[t] = (int)(r - row0) * D + 8 * q;
  }
  f32x4 araw[MT][2];
  auto load_a = [&](int ks) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      araw[t][0] = *(const f32x4*)(Xw + arow[t] + 32 * ks);
      araw[t][1] = *(const f32x4*)(Xw + arow[t] + 32 * ks + 4);
    }
  };
  f32x4 acc[MT][NT16];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int n = 0; n < NT16; ++n) acc[t][n] = z;

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
    const unsigned short* Bc = Bl + (s & 1) * SLAB + (l15 * 32 + 8 * q);
    fp_frag3 bf[2];
    auto ldb = [&](int n, fp_frag3& b) {
      b.h = *(const u32x4*)(Bc + n * 512);
      b.m = *(const u32x4*)(Bc + NC * 32 + n * 512);
      b.l = *(const u32x4*)(Bc + 2 * NC * 32 + n * 512);
    };
    ldb(0, bf[0]);
#pragma unroll
    for (int n = 0; n < NT16; ++n) {
      if (n + 1 < NT16) ldb(n + 1, bf[(n + 1) & 1]);
      const fp_frag3& b = bf[n & 1];
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t][n] = fp_mfma_x6(b.h, b.m, b.l, af[t].h, af[t].m, af[t].l, acc[t][n]);
    }
    if (++ks < KS) continue;
    ks = 0;

    // epilogue of a chunk: lane = row 16 t + l15, columns c0 + 16 n + 4 q + i
    const int c0 = chunk * NC;
    ++chunk;
    float gi[MT];
    int rowi[MT], li[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      rowi[t] = (int)row0 + 16 * t + l15;                // < Npad
      const float g = inv[rowi[t]];
      gi[t] = g == 0.f ? qnan : g;                       // not live / past N: every score is NaN and counts nowhere
      li[t] = lab[rowi[t]];
    }
#pragma unroll
    for (int n = 0; n < NT16; ++n) {
      const int colb = c0 + 16 * n + 4 * q;
      f32x4 rn = *(const f32x4*)(inv + colb);
      const i32x4 ln = *(const i32x4*)(lab + colb);
#pragma unroll
      for (int i = 0; i < 4; ++i) rn[i] = rn[i] == 0.f ? qnan : rn[i];
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
  }

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
  return (size_t)fp_round_up(N, CL_NC) * 8;              // inv1, lab1
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
  const int n = (int)N, Npad = (int)fp_round_up(N, CL_NC), nchunk = Npad / CL_NC;
  const size_t lds = (size_t)CL_LDS + (size_t)nbins * 8;
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
