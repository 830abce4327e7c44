// cluster.hip — group unlabelled faces by identity: cosine DBSCAN on the device (gfx950).  Build-defined, DESIGN §7.
//
// The threshold graph  i ~ j  <=>  <X[i], X[j]> * inv[i] * inv[j] >= tau  is never stored.  It is walked twice, each time over
// the UPPER TRIANGLE only (row tiles of 128 rows x 128-column chunks, a chunk is walked when it is not wholly at or below its
// row tile's first row), on the walk of cosinewalk.h (cw_walk: planes of fp_split3_rows staged by LDS-DMA, double-buffered,
// rows split in registers), score = acc * inv[i] * inv[j].  A pair (i < j) is evaluated once, row i the register-split
// operand: the decision is unique.
//   pass 1 (degree): every edge adds one to the degree of both endpoints and enters both neighbour lists (min_samples - 2
//           slots per point: complete for every non-core point, truncated and never read for a core point);
//   pass 2 (union):  the same walk with the inverse norms of the non-core points zeroed -- a zero inverse norm is the library's
//           mask, so only core-core edges survive the same epilogue -- and every edge unites its endpoints in a lock-free
//           union-find: parent[x] <= x, parent[x] only decreases and stays in x's component, the larger root is hooked under
//           the smaller by compare-and-swap.  A failed CAS means another lane hooked that root: no lock, no wait on anyone.
//           Every access to parent[] in the walk is an agent-scope relaxed atomic (the L2s of the XCDs are not coherent).
//   min_samples <= 2: every endpoint of an edge is core, one walk does both.
// Then: flatten (root of every core point = the smallest row of its cluster), rank the roots (exclusive scan), label.
// The result is a function of the edge set: degrees are sums, the root of a component is its minimum, a border point takes the
// minimum over its complete list -- no arrival order, launch geometry or schedule enters.
#include "cosinewalk.h"
#include "triwalk.h"

namespace {

constexpr int CL_MAX_MS = 64;

// ---- lock-free union-find ------------------------------------------------------------------------------------------
#define CL_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
__device__ __forceinline__ int uf_load(int* parent, int x) { return __hip_atomic_load(parent + x, CL_RLX); }
// read-only
__device__ __forceinline__ int uf_root(int* parent, int x) {
  for (;;) {
    const int p = uf_load(parent, x);
    if (p == x) return x;
    x = p;
  }
}
// with path halving: parent[x] <- its grandparent (an ancestor: smaller, same component), by atomic min
__device__ __forceinline__ int uf_find(int* parent, int x) {
  for (;;) {
    const int p = uf_load(parent, x);
    if (p == x) return x;
    const int gp = uf_load(parent, p);
    if (gp == p) return p;
    __hip_atomic_fetch_min(parent + x, gp, CL_RLX);
    x = gp;
  }
}
__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
  a = uf_find(parent, a);
  b = uf_find(parent, b);
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    int seen = a;                                        // hook the larger root a under b < a
    if (__hip_atomic_compare_exchange_strong(parent + a, &seen, b, __ATOMIC_RELAXED, CL_RLX)) return;
    a = uf_find(parent, seen);                           // someone else hooked a: go on from what they wrote
    b = uf_find(parent, b);
  }
}

// ---- the walk --------------------------------------------------------------------------------------------------------
// inv: N inverse norms padded with zeros to Npad (0 = dead / masked / padding).  DEG: degree[] and the neighbour lists
// (L slots per point); UNI: union of the endpoints in parent[].
template <bool DEG, bool UNI>
__global__ __launch_bounds__(256, 3) void cluster_walk_kernel(const float* __restrict__ X, const float* __restrict__ inv, int N,
                                                               const unsigned short* __restrict__ X3, int Npad, int D, float tau,
                                                               int P, int* __restrict__ degree, int* __restrict__ nbr, int L,
                                                               int* __restrict__ parent) {
  constexpr int MT = 2, NT16 = CW_NT16;
  typedef unsigned long long u64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int nchunk = Npad / CW_NC;
  // the longest rows first; the groups of one row tile next to each other on ONE XCD (its rows from that L2)
  const cl_item it = cl_decode((long)gridDim.x - 1 - (long)fp_xcd_block(), nchunk, P);
  const int cb = __builtin_amdgcn_readfirstlane(it.first), nck = __builtin_amdgcn_readfirstlane(it.count);
  const long row0 = (long)__builtin_amdgcn_readfirstlane(it.tile) * CL_ROWS + wave * (MT * 16);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};

  // rows past N - 1 read row N - 1, their inv is 0.  Epilogue of a chunk: lane = row 16 t + l15, columns c0 + 16 n + 4 q + i.
  // Bit 4 n + i of eb[t]: that pair is an edge.
  cw_walk<MT>(X, N, row0, X3, Npad, D, cb, nck, (unsigned short*)smem_raw, [&](int c0, f32x4 (&acc)[MT][NT16]) {
    float gi[MT];
    int rowi[MT];
    unsigned eb[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      rowi[t] = (int)row0 + 16 * t + l15;                // < Npad
      gi[t] = cw_nan_if_zero(inv[rowi[t]]);              // dead row / past N: every score is NaN, NaN >= tau is false
      eb[t] = 0;
    }
#pragma unroll
    for (int n = 0; n < NT16; ++n) {
      const int colb = c0 + 16 * n + 4 * q;
      f32x4 rn = *(const f32x4*)(inv + colb);
#pragma unroll
      for (int i = 0; i < 4; ++i) rn[i] = cw_nan_if_zero(rn[i]);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float sv = acc[t][n][i] * gi[t] * rn[i];
          if (sv >= tau && colb + i > rowi[t]) eb[t] |= 1u << (4 * n + i);
        }
        acc[t][n] = z;
      }
    }
    if (__ballot((eb[0] | eb[1]) != 0) == 0) return;     // the common case of a sparse graph: no edge in this wave's 32 x 128

#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int row = rowi[t];
      if (DEG) {
        // row side: one add per lane, its edges take consecutive slots
        unsigned bits = eb[t];
        if (bits) {
          int slot = atomicAdd(&degree[row], __popc(bits)) - 1;     // degree starts at 1 (the point itself)
          while (bits && slot < L) {
            const int b = __ffs(bits) - 1;
            bits &= bits - 1;
            nbr[(long)row * L + slot] = c0 + 16 * (b >> 2) + 4 * q + (b & 3);
            ++slot;
          }
        }
        // column side: the 16 lanes of a k-group hold 16 rows of the same column; their edges go in one add
#pragma unroll 1
        for (int b = 0; b < 32; ++b) {
          const bool e = (eb[t] >> b) & 1u;
          const u64 mask = __ballot(e);
          if (!mask) continue;
          const unsigned g = (unsigned)(mask >> (16 * q)) & 0xffffu;
          const int leader = g ? __ffs(g) - 1 : 0;
          const int col = c0 + 16 * (b >> 2) + 4 * q + (b & 3);
          int base = 0;
          if (e && l15 == leader) base = atomicAdd(&degree[col], __popc(g)) - 1;
          if (L) {
            base = __shfl(base, 16 * q + leader);
            const int slot = base + __popc(g & ((1u << l15) - 1u));
            if (e && slot < L) nbr[(long)col * L + slot] = row;
          }
        }
      }
      if (UNI) {
        unsigned bits = eb[t];
        if (bits) {
          int rr = uf_root(parent, row);                 // read-only fast path: already in one tree
          while (bits) {
            const int b = __ffs(bits) - 1;
            bits &= bits - 1;
            const int col = c0 + 16 * (b >> 2) + 4 * q + (b & 3);
            if (uf_root(parent, col) != rr) {
              uf_unite(parent, row, col);
              rr = uf_root(parent, row);
            }
          }
        }
      }
    }
  });
}

// ---- the small kernels around the walks ----------------------------------------------------------------------------
// inv1 = the caller's inverse norms with dead rows (0 or not finite) and the padding as 0; degree = 1 for a live row;
// parent[i] = i.
__global__ __launch_bounds__(256) void cluster_init_kernel(const float* __restrict__ xinv, int N, int Npad, float* __restrict__ inv1,
                                                           int* __restrict__ degree, int* __restrict__ parent) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= Npad) return;
  float v = 0.f;
  if (i < N) {
    const float x = xinv[i];
    v = (x != 0.f && fabsf(x) < __builtin_huge_valf()) ? x : 0.f;     // NaN compares false
    degree[i] = v != 0.f ? 1 : 0;
  }
  inv1[i] = v;
  parent[i] = (int)i;
}

// core = degree >= min_samples; inv2 = inv1 of the core points, 0 elsewhere
__global__ __launch_bounds__(256) void cluster_core_kernel(const float* __restrict__ inv1, const int* __restrict__ degree, int N,
                                                           int Npad, int min_samples, unsigned char* __restrict__ core,
                                                           float* __restrict__ inv2) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= Npad) return;
  float v = 0.f;
  if (i < N) {
    const bool c = inv1[i] != 0.f && degree[i] >= min_samples;
    core[i] = c ? 1 : 0;
    v = c ? inv1[i] : 0.f;
  }
  inv2[i] = v;
}

// root[i] of every core point (-1 otherwise), rank[i] = 1 where a core point is its own root
__global__ __launch_bounds__(256) void cluster_flatten_kernel(const unsigned char* __restrict__ core, int* parent, int N,
                                                              int* __restrict__ root, int* __restrict__ rank) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int r = core[i] ? uf_root(parent, (int)i) : -1;
  root[i] = r;
  rank[i] = r == (int)i ? 1 : 0;
}

// exclusive prefix sum of rank[0 .. N) in place, the total to n_clusters.  One workgroup: thread t owns a contiguous segment.
__global__ __launch_bounds__(1024) void cluster_rank_kernel(int* __restrict__ rank, int N, int* __restrict__ n_clusters) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  const long per = ((long)N + 1023) / 1024;
  const long b = (long)tid * per, e = b + per < N ? b + per : N;
  int s = 0;
  for (long i = b; i < e; ++i) s += rank[i];
  part[tid] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {             // inclusive scan of the 1024 sums
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (long i = b; i < e; ++i) {
    const int v = rank[i];
    rank[i] = run;
    run += v;
  }
  if (tid == 1023) n_clusters[0] = part[1023];
}

// core: the rank of its root.  Live non-core: the smallest cluster among the core points of its (complete) list, else -1.
__global__ __launch_bounds__(256) void cluster_label_kernel(const unsigned char* __restrict__ core, const int* __restrict__ degree,
                                                            const int* __restrict__ root, const int* __restrict__ rank,
                                                            const int* __restrict__ nbr, int L, int N, int* __restrict__ labels) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int lab = -1;
  if (core[i]) {
    lab = rank[root[i]];
  } else {
    int cnt = degree[i] - 1;
    cnt = cnt < L ? cnt : L;
    int best = 0x7FFFFFFF;
    for (int j = 0; j < cnt; ++j) {
      const int nb = nbr[i * L + j];
      if (core[nb]) {
        const int c = rank[root[nb]];
        best = c < best ? c : best;
      }
    }
    lab = best == 0x7FFFFFFF ? -1 : best;
  }
  labels[i] = lab;
}

// One workgroup per cluster: centroid = normalised sum of the members' normalised rows, summed in the order given (thread d
// owns feature d: a sequential fp32 sum, no atomics), and the medoid: the member with the largest cosine to the centroid,
// the lower row on ties.  An empty cluster: a zero centroid, medoid -1.
__global__ __launch_bounds__(256) void cluster_centroid_kernel(const float* __restrict__ X, const float* __restrict__ xinv,
                                                               const int* __restrict__ order, const int* __restrict__ offsets, int D,
                                                               float* __restrict__ centroids, int* __restrict__ medoid) {
  typedef unsigned long long u64;
  extern __shared__ float cs[];                          // [D]
  __shared__ float red[4];
  __shared__ u64 bestk[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x, mb = offsets[c], me = offsets[c + 1];
  float ss = 0.f;
  for (int d = tid; d < D; d += 256) {
    float s = 0.f;
    for (int j = mb; j < me; ++j) {
      const int m = order[j];
      s += X[(long)m * D + d] * xinv[m];
    }
    cs[d] = s;
    ss += s * s;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
  if (lane == 0) red[wave] = ss;
  __syncthreads();
  const float tot = (red[0] + red[1]) + (red[2] + red[3]);
  const float sc = tot > 0.f ? 1.0f / sqrtf(tot) : 0.f;
  for (int d = tid; d < D; d += 256) {
    const float v = cs[d] * sc;
    cs[d] = v;
    centroids[(long)c * D + d] = v;
  }
  __syncthreads();
  u64 best = 0;                                          // cw_key(score, row): larger = better, then the lower row
  for (int j = mb + wave; j < me; j += 4) {
    const int m = order[j];
    const float* p = X + (long)m * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += p[d] * cs[d];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    s *= xinv[m];
    if (!(s == s)) s = -__builtin_huge_valf();
    const u64 key = cw_key(s, (unsigned)m);
    best = key > best ? key : best;
  }
  if (lane == 0) bestk[wave] = best;
  __syncthreads();
  if (tid == 0) {
    u64 b = bestk[0];
    for (int w = 1; w < 4; ++w) b = bestk[w] > b ? bestk[w] : b;
    medoid[c] = b ? cw_key_index(b) : -1;
  }
}

// the workspace: five int32 / fp32 arrays of Npad entries (inv1, inv2, parent, root, rank) and the neighbour lists
struct cl_ws {
  float *inv1, *inv2;
  int *parent, *root, *rank, *nbr;
  int L;
  size_t bytes;
};
cl_ws cl_layout(void* ws, int64_t N, int min_samples) {
  const size_t Npad = (size_t)fp_round_up(N, CW_NC);
  cl_ws w;
  char* p = (char*)ws;
  w.inv1 = (float*)p;
  w.inv2 = (float*)(p + Npad * 4);
  w.parent = (int*)(p + Npad * 8);
  w.root = (int*)(p + Npad * 12);
  w.rank = (int*)(p + Npad * 16);
  w.nbr = (int*)(p + Npad * 20);
  w.L = min_samples > 2 ? min_samples - 2 : 0;
  w.bytes = Npad * 20 + (size_t)N * (size_t)w.L * 4;
  return w;
}

}  // namespace

extern "C" {

size_t fp_cosine_dbscan_workspace(int64_t N, int min_samples) {
  if (N <= 0 || N >= (1LL << 31) || min_samples < 1 || min_samples > CL_MAX_MS) return 0;
  return cl_layout(nullptr, N, min_samples).bytes;
}

int fp_cosine_dbscan_x6(const float* X, const float* xinv, const void* X3, int64_t N, int D, float tau, int min_samples,
                        int32_t* degree, uint8_t* core, int32_t* labels, int32_t* n_clusters, void* ws, size_t ws_bytes,
                        void* stream) {
  if (!X || !xinv || !X3 || !degree || !core || !labels || !n_clusters || !ws) return FP_ERR_INVALID_ARG;
  if (N <= 0 || D <= 0 || min_samples < 1 || min_samples > CL_MAX_MS) return FP_ERR_INVALID_ARG;
  if (N >= (1LL << 31)) return FP_ERR_UNSUPPORTED;
  if (D % 32 || ((uintptr_t)X) % 16 || ((uintptr_t)X3) % 16 || ((uintptr_t)ws) % 16) return FP_ERR_ALIGNMENT;
  const cl_ws w = cl_layout(ws, N, min_samples);
  if (ws_bytes < w.bytes) return FP_ERR_INVALID_ARG;
  const int n = (int)N, Npad = (int)fp_round_up(N, CW_NC), nchunk = Npad / CW_NC;
  const long P = cl_chunks_per_group(nchunk, 3);   // the walk runs three workgroups per CU
  const long groups = cl_groups(nchunk, P);
  if (groups >= (1L << 31)) return FP_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 gN((unsigned)fp_ceil_div(N, 256)), gP((unsigned)fp_ceil_div(Npad, 256)), b256(256);
  const unsigned short* x3 = (const unsigned short*)X3;

  hipLaunchKernelGGL(cluster_init_kernel, gP, b256, 0, s, xinv, n, Npad, w.inv1, degree, w.parent);
  FP_CHECK_LAUNCH();
  if (min_samples <= 2) {
    hipLaunchKernelGGL((cluster_walk_kernel<true, true>), dim3((unsigned)groups), b256, CW_LDS, s, X, (const float*)w.inv1, n, x3,
                       Npad, D, tau, (int)P, degree, w.nbr, w.L, w.parent);
    FP_CHECK_LAUNCH();
    hipLaunchKernelGGL(cluster_core_kernel, gP, b256, 0, s, (const float*)w.inv1, (const int*)degree, n, Npad, min_samples, core, w.inv2);
    FP_CHECK_LAUNCH();
  } else {
    hipLaunchKernelGGL((cluster_walk_kernel<true, false>), dim3((unsigned)groups), b256, CW_LDS, s, X, (const float*)w.inv1, n, x3,
                       Npad, D, tau, (int)P, degree, w.nbr, w.L, w.parent);
    FP_CHECK_LAUNCH();
    hipLaunchKernelGGL(cluster_core_kernel, gP, b256, 0, s, (const float*)w.inv1, (const int*)degree, n, Npad, min_samples, core, w.inv2);
    FP_CHECK_LAUNCH();
    hipLaunchKernelGGL((cluster_walk_kernel<false, true>), dim3((unsigned)groups), b256, CW_LDS, s, X, (const float*)w.inv2, n, x3,
                       Npad, D, tau, (int)P, degree, w.nbr, w.L, w.parent);
    FP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(cluster_flatten_kernel, gN, b256, 0, s, (const unsigned char*)core, w.parent, n, w.root, w.rank);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(cluster_rank_kernel, dim3(1), dim3(1024), 0, s, w.rank, n, n_clusters);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(cluster_label_kernel, gN, b256, 0, s, (const unsigned char*)core, (const int*)degree, (const int*)w.root,
                     (const int*)w.rank, (const int*)w.nbr, w.L, n, labels);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_cluster_centroids(const float* X, const float* xinv, const int32_t* order, const int32_t* offsets, int C, int D,
                         float* centroids, int32_t* medoid, void* stream) {
  if (!X || !xinv || !order || !offsets || !centroids || !medoid || C < 0 || D <= 0) return FP_ERR_INVALID_ARG;
  if (D > 16000) return FP_ERR_UNSUPPORTED;              // the centroid of a workgroup lives in LDS
  if (C == 0) return FP_OK;
  hipLaunchKernelGGL(cluster_centroid_kernel, dim3((unsigned)C), dim3(256), (size_t)D * sizeof(float), (hipStream_t)stream, X, xinv,
                     order, offsets, D, centroids, medoid);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
