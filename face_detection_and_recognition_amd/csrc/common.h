// Internal helpers shared by the HIP translation units of libfacepath.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/facepath.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
// Pins the ISSUE ORDER of MFMAs (everything else may still move across): hipcc regroups v_mfma instructions by
// accumulator, and a 32x32x2 f32 MFMA that accumulates into the previous MFMA's result issues at HALF rate (128 instead
// of 64 cycles, tools/lab/mfma_chain_lab.hip).  Sources write the MFMAs round-robin over >= 2 accumulators and put
// this after each one.  Mask = every class but MFMA / generic-ALU may be scheduled across (LLVM sched_barrier bits).
#define FP_MFMA_ORDER() __builtin_amdgcn_sched_barrier(0x7F6)

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define FP_WAVE 64

// SiLU x * sigmoid(x) (nn.SiLU, y5/models/common.py:47) with the hardware exp2 / rcp (v_exp_f32, v_rcp_f32: <= 1 ulp
// each, relative error of the result ~1e-6 x |x|/16): 5 VALU instructions.  The IEEE expf + division form costs 26 and,
// applied to every conv output of YOLOv5-face, was ~3 ms of VALU issue per 256-image forward pass.  x -> -inf gives
// exp2 = +inf, rcp = 0, result -0; x -> +inf gives x.  Decisions that must be bit-exact (decode / NMS, post.hip)
// do not use this.
__device__ __forceinline__ float fp_silu(float x) {
  const float e = __builtin_amdgcn_exp2f(-1.44269504088896341f * x);
  return x * __builtin_amdgcn_rcpf(1.0f + e);
}

// Test knob of the launchers, taken from the environment ONCE when the library is loaded (a launch never calls getenv);
// fp_debug_reload_env() (facepath.h) re-reads it.
struct fp_knobs {
  int resize_per_pixel;  // FP_RESIZE_PER_PIXEL: fp_resize_normalize takes the per-pixel kernel (the tabled kernel's reference in tests)
};
const fp_knobs& fp_get_knobs();

// Per-thread record of the last HIP error text (fp_last_hip_error()).
void fp_set_hip_error(hipError_t e);

#define FP_CHECK_LAUNCH()                         \
  do {                                            \
    hipError_t e__ = hipGetLastError();           \
    if (e__ != hipSuccess) {                      \
      fp_set_hip_error(e__);                      \
      return FP_ERR_LAUNCH;                       \
    }                                             \
  } while (0)

// n / d by multiply-high for 0 <= n < 2^31 and d >= 2: with s = ceil(log2 d), k = 31 + s and M = floor(2^k / d) + 1
// (M < 2^32 because d > 2^(s-1)), floor(n * M / 2^k) = floor(n / d): the error M*d - 2^k lies in (0, d], and
// n * d < 2^31 * 2^s = 2^k.  Device side: __umulhi(n, M) >> (s - 1).
struct fp_divisor {
  unsigned mul, shift;
};
static inline fp_divisor fp_make_divisor(unsigned d) {
  unsigned s = 0;
  while ((1ull << s) < d) ++s;
  fp_divisor r;
  r.mul = (unsigned)((1ull << (31 + s)) / d + 1ull);
  r.shift = s - 1;   // d >= 2 -> s >= 1
  return r;
}
__device__ __forceinline__ unsigned fp_fastdiv(unsigned n, fp_divisor d) { return __umulhi(n, d.mul) >> d.shift; }

// Workgroup -> work item for 1-D grids.  Workgroups are dealt round-robin to the 8 XCDs (blockIdx & 7), each with its own
// L2: XCD x gets the contiguous range [x G/8, (x + 1) G/8) of items, so items next to each other -- the column chunks of one
// row tile, the bands of one image -- run on the same XCD close in time and share their re-read operands in that L2.
__device__ __forceinline__ unsigned fp_xcd_block() {
  const unsigned G = gridDim.x, b = blockIdx.x, q = G >> 3, rr = G & 7u, xcd = b & 7u, k = b >> 3;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + k;
}

// A 64-bit offset the caller knows to be wave-uniform, rebuilt from readfirstlane'd halves so that the compiler keeps
// it in SGPRs: base + offset stays a scalar address and `global_load v, v_offset32, s[addr:addr+1] offset:imm` needs no
// 64-bit vector address arithmetic.  (Offsets, not pointers: an integer -> pointer cast loses the global address space
// and turns the accesses into flat_load / flat_store.)
__device__ __forceinline__ long fp_uniform(long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
  return (long)(((unsigned long long)hi << 32) | lo);
}

static inline int fp_ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// Bands per image for a launch over a row window of `rows` output rows of N images (facepath.h "Row windows"): a workgroup
// takes `per_wg` bands, `slots` workgroups run at once on the device, and a band of R rows costs step_mul * R + halo steps.
// Minimises (rounds of slots) x (steps per band) over bmin .. rows / min_rows bands (at least bmin); ties keep fewer bands.
// A band of ceil(rows / bands) rows: the last one is moved up to end at the window's end, overlapping its neighbour.
static inline int fp_window_bands(int rows, int N, int per_wg, int slots, int step_mul, int halo, int bmin, int min_rows) {
  int best = bmin;
  long best_cost = -1;
  for (int b = bmin; b == bmin || b <= rows / min_rows; ++b) {
    const long rounds = fp_ceil_div(fp_ceil_div((long)N * b, per_wg), slots);
    const long cost = rounds * ((long)step_mul * fp_ceil_div(rows, b) + halo);
    if (best_cost < 0 || cost < best_cost) best = b, best_cost = cost;
  }
  return best;
}
static inline long fp_round_up(long a, long b) { return (a + b - 1) / b * b; }

// Compute units of the current device, asked once (256 if the runtime does not say): what launchers size their grids by.
static inline int fp_num_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus = n;
  }
  return cus;
}

// True if two NHWC views of the arena may share a float: each is (offset, per-image stride, pixels, pixel stride, channels)
// over N images.  Plans lay the arena out image-major, so views with the same image stride overlap only if one image's
// extents do; otherwise the whole-batch extents are compared.
static inline bool fp_views_overlap(int N, long off_a, long ns_a, long hw_a, long ld_a, long c_a, long off_b, long ns_b,
                                    long hw_b, long ld_b, long c_b) {
  const long img_a = (hw_a - 1) * ld_a + c_a, img_b = (hw_b - 1) * ld_b + c_b;   // exact extents of one image
  if (ns_a == ns_b) return off_a < off_b + img_b && off_b < off_a + img_a;
  return off_a < off_b + (long)(N - 1) * ns_b + img_b && off_b < off_a + (long)(N - 1) * ns_a + img_a;
}

// What a plan-op launcher is given (capi.cpp).  A launcher alone decides whether it takes an op and which kernel
// instance runs it.  With `dry` set it makes every check and that choice exactly as a launch would, writes the
// instance's name to `name` (when not null, FP_KERNEL_NAME_MAX bytes) and returns FP_OK before any HIP call and without
// touching the weights, the arena or `ext`: fp_plan_validate and fp_op_kernel_name are such dry runs.
#define FP_KERNEL_NAME_MAX 64
struct fp_launch {
  const float* weights;
  float* arena;
  const fp_ext* ext;
  int n_ext;
  hipStream_t s;
  bool dry;
  char* name;
};
// In a dry run: record the kernel's name (printf format) and return true, the launcher then returns FP_OK.
bool fp_dry_run(const fp_launch& L, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// launchers implemented in the .hip files, one per op family, dispatched by the plan executor (capi.cpp)
int fp_launch_conv(const fp_op& op, const fp_launch& L);
int fp_launch_dwconv(const fp_op& op, const fp_launch& L);
int fp_launch_maxpool(const fp_op& op, const fp_launch& L);
int fp_launch_upsample2x(const fp_op& op, const fp_launch& L);
int fp_launch_copy(const fp_op& op, const fp_launch& L);
int fp_launch_l2norm(const fp_op& op, const fp_launch& L);
int fp_launch_embed_head(const fp_op& op, const fp_launch& L);   // embedhead.hip
int fp_launch_pool_lrn(const fp_op& op, const fp_launch& L);     // lrn.hip
int fp_launch_cls_head(const fp_op& op, const fp_launch& L);     // clshead.hip
int fp_launch_blazeblock(const fp_op& op, const fp_launch& L);
int fp_launch_blazeblock_rowpad(const fp_op& op, const fp_launch& L);   // blazewp.hip
int fp_launch_dwpw(const fp_op& op, const fp_launch& L);
int fp_launch_dwpwx6(const fp_op& op, const fp_launch& L);   // DWPW with FP_OPF_SPLIT3 (dwpwx6.hip)
int fp_launch_blazepair(const fp_op& op, const fp_launch& L);
int fp_launch_blazepair_s2(const fp_op& op, const fp_launch& L);
int fp_launch_blazechain(const fp_op& op, const fp_launch& L);
int fp_launch_dwblock(const fp_op& op, const fp_launch& L);
int fp_launch_dwblock_x6(const fp_op& op, const fp_launch& L);   // DWBLOCK with FP_OPF_SPLIT3 (dwblockx6.hip)
int fp_launch_shufdown(const fp_op& op, const fp_launch& L);
int fp_launch_shufunit(const fp_op& op, const fp_launch& L);
int fp_launch_ystem2(const fp_op& op, const fp_launch& L);
int fp_launch_ystem(const fp_op& op, const fp_launch& L);
int fp_launch_ystem_u8(const fp_op& op, const fp_launch& L);
int fp_launch_stem_u8(const fp_op& op, const fp_launch& L);
// ... and the kernels fp_launch_conv dispatches to, with the predicates that pick them
int fp_launch_stemdw(const fp_op& op, const fp_launch& L);   // FP_OPF_OUT_DW (stemdw.hip)
bool fp_pwx6_eligible(const fp_op& op);   // FP_OPF_SPLIT3 pointwise: pwx6_kernel, else convx6_kernel (pwx6.hip)
int fp_launch_pwx6(const fp_op& op, const fp_launch& L);
int fp_launch_convx6(const fp_op& op, const fp_launch& L);
bool fp_pws_eligible(const fp_op& op);    // pointwise K = 64 / 128 convs on the wave-private streaming kernel (pws.hip)
int fp_launch_pws(const fp_op& op, const fp_launch& L);
bool fp_stem_eligible(const fp_op& op);   // KxK stride-2 convs on a 4-float-pixel image, network stems (stem.hip)
int fp_launch_stem(const fp_op& op, const fp_launch& L);
bool fp_conv3_eligible(const fp_op& op);  // dense 3x3 pad-1 convs on the LDS-image kernel (conv3.hip)
int fp_launch_conv3(const fp_op& op, const fp_launch& L);

// floats of the weight blob behind an op's offsets (the span checks of fp_plan_validate)
int64_t fp_stemdw_w_floats(const fp_op& op);
int64_t fp_convx6_w_floats(const fp_op& op);
int64_t fp_dwpwx6_w_floats(const fp_op& op);
int64_t fp_blazechain_w_floats(const fp_op& op);
int64_t fp_dwblock_x6_we_floats(const fp_op& op);   // behind w_off / slope_off of a DWBLOCK with FP_OPF_SPLIT3
int64_t fp_dwblock_x6_wp_floats(const fp_op& op);
int64_t fp_shufdown_w_floats(const fp_op& op);
int64_t fp_shufunit_w_floats(const fp_op& op);
int64_t fp_ystem2_w_floats(const fp_op& op);
int fp_ystem_nb2(const fp_op& op);   // 16-channel column blocks of ystem_kernel's packed stem_1 weights
