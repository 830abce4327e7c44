// capi.cpp — plan validation + executor and the small ABI utilities of libfacepath.so.
// Compiled by hipcc as host code; kernels live in the .hip files.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"

static thread_local char g_hip_err[256] = "";

void fp_set_hip_error(hipError_t e) {
  const char* s = hipGetErrorString(e);
  strncpy(g_hip_err, s ? s : "unknown", sizeof(g_hip_err) - 1);
  g_hip_err[sizeof(g_hip_err) - 1] = 0;
}

static fp_knobs read_knobs() {
  fp_knobs k;
  k.resize_per_pixel = getenv("FP_RESIZE_PER_PIXEL") != nullptr;
  return k;
}
static fp_knobs g_knobs = read_knobs();
const fp_knobs& fp_get_knobs() { return g_knobs; }

bool fp_dry_run(const fp_launch& L, const char* fmt, ...) {
  if (!L.dry) return false;
  if (L.name) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(L.name, FP_KERNEL_NAME_MAX, fmt, ap);
    va_end(ap);
  }
  return true;
}

static bool span_ok(int64_t off, int64_t extent, size_t limit) {
  return off >= 0 && extent >= 0 && (uint64_t)(off + extent) <= (uint64_t)limit;
}

// floats of a GEMM weight matrix packed for the fp32 kernels (facepath.h "CONV"): Kpad x Npad
static int64_t packed_floats(int64_t K, int Cout) { return fp_round_up(K, 8) * fp_round_up(Cout, 32); }

// floats of N images of a res-style view: hw pixels of `ld` floats, the last one `c` wide
static int64_t res_extent(const fp_op& op, int64_t hw, int64_t c) {
  return (int64_t)(op.N - 1) * op.res_ns + (hw - 1) * op.res_ld + c;
}

// Status of an NHWC view of the arena whose last pixel holds `last` floats: dense, or row-padded (facepath.h "Row-padded
// activation layout": the pads lie inside the image stride and in front of off)
static int view_status(bool rowpad, int64_t off, int64_t ns, int ld, int N, int H, int W, int64_t last, size_t arena_floats) {
  if (!rowpad) return span_ok(off, (int64_t)(N - 1) * ns + ((int64_t)H * W - 1) * ld + last, arena_floats) ? FP_OK : FP_ERR_BOUNDS;
  const int64_t lead = (int64_t)(W + 2) * ld;
  if (ns < ((int64_t)(H + 2) * (W + 1) + 1) * ld) return FP_ERR_INVALID_ARG;
  return off >= lead && span_ok(off - lead, (int64_t)N * ns, arena_floats) ? FP_OK : FP_ERR_BOUNDS;
}

// ---- the spans of each kind's parameter blocks (weight blob) and extra views (arena), in the order they are checked ----
typedef int spans_fn(const fp_op& op, size_t weight_floats, size_t arena_floats);

static int spans_w(const fp_op& op, int64_t floats, size_t wf) { return span_ok(op.w_off, floats, wf) ? FP_OK : FP_ERR_BOUNDS; }
static int spans_conv(const fp_op& op, size_t wf, size_t) {
  int64_t wext = packed_floats((int64_t)op.KH * op.KW * op.Cin, op.Cout);
  if (op.flags & FP_OPF_SPLIT3) wext = fp_convx6_w_floats(op);   // three bf16 planes: 1.5 floats per (padded) weight
  if (op.flags & FP_OPF_OUT_DW) wext = fp_stemdw_w_floats(op);
  return spans_w(op, wext, wf);
}
static int spans_stem_u8(const fp_op& op, size_t wf, size_t) {
  // packed for a 4-float pixel; FP_OPF_SPLIT3: [3 slabs][2][3][16][32] bf16
  const int64_t wext = (op.flags & FP_OPF_SPLIT3) ? 3 * 2 * 3 * 16 * 32 / 2 : packed_floats((int64_t)op.KH * op.KW * 4, op.Cout);
  return spans_w(op, wext, wf);
}
static int spans_dwconv(const fp_op& op, size_t wf, size_t) {
  return spans_w(op, (int64_t)op.KH * op.KW * op.Cin, wf);
}
static int spans_blazeblock(const fp_op& op, size_t wf, size_t) {
  // w_off addresses the dw weights [9][Cin], scale_off the dw bias, slope_off the packed pointwise weights, bias_off the
  // pointwise bias
  if (!span_ok(op.slope_off, packed_floats(op.Cin, op.Cout), wf)) return FP_ERR_BOUNDS;
  if (!span_ok(op.scale_off, op.Cin, wf)) return FP_ERR_BOUNDS;
  if (!span_ok(op.bias_off, op.Cout, wf)) return FP_ERR_BOUNDS;
  return spans_w(op, 9 * (int64_t)op.Cin, wf);
}
static int spans_dwpw(const fp_op& op, size_t wf, size_t) {
  // w_off: [9*G taps][G scale][G bias][G slope]; slope_off: [Kpad*Npad packed 1x1][Cout4 scale][Cout4 bias]
  const int64_t cout4 = fp_round_up(op.Cout, 4);
  const int64_t pw = (op.flags & FP_OPF_SPLIT3) ? fp_dwpwx6_w_floats(op) : packed_floats(op.Cin, op.Cout) + 2 * cout4;
  if (!span_ok(op.w_off, 12 * (int64_t)op.Cin, wf)) return FP_ERR_BOUNDS;
  if (!span_ok(op.slope_off, pw, wf)) return FP_ERR_BOUNDS;
  if (op.act != FP_ACT_NONE && op.act != FP_ACT_PRELU) return FP_ERR_INVALID_ARG;
  // bias_off: optional [Cout4] PReLU slopes of the projection output
  if (op.bias_off >= 0 && !span_ok(op.bias_off, cout4, wf)) return FP_ERR_BOUNDS;
  if (op.act2 != FP_ACT_NONE && op.act2 != FP_ACT_SILU) return FP_ERR_INVALID_ARG;
  return FP_OK;
}
static int spans_ystem(const fp_op& op, size_t wf, size_t af) {   // YSTEM and YSTEM_U8
  if (op.Cin != (op.kind == FP_OP_YSTEM_U8 ? 3 : 4) || op.res_C <= 0 || op.res_C > 32 || op.Cout > 32) return FP_ERR_UNSUPPORTED;
  if (op.res_H <= 0 || op.res_W <= 0 || op.res_ld < op.res_C || op.res_ns < 0) return FP_ERR_INVALID_ARG;
  if (!span_ok(op.w_off, 40 * 32, wf) || !span_ok(op.bias_off, 32, wf)) return FP_ERR_BOUNDS;
  if (op.scale_off >= 0 && !span_ok(op.scale_off, 32, wf)) return FP_ERR_BOUNDS;
  if (!span_ok(op.slope_off, (int64_t)fp_ystem_nb2(op) * 16 * (32 + 2), wf)) return FP_ERR_BOUNDS;
  // the res view receives maxpool2x2(stem_1)
  return span_ok(op.res_off, res_extent(op, (int64_t)(op.OH / 2) * (op.OW / 2), op.res_C), af) ? FP_OK : FP_ERR_BOUNDS;
}
static int spans_dwblock(const fp_op& op, size_t wf, size_t) {
  // w_off: expand packed as CONV (K = Cin, Npad = Cmid); scale_off: [15][Cmid]; slope_off: project packed as CONV
  // (K = Cmid, Npad = Cout) + [Cout] scale + [Cout] bias.
  // FP_OPF_SPLIT3: both weight matrices as three bf16 planes (1.5 floats per weight), see facepath.h
  const bool x6 = (op.flags & FP_OPF_SPLIT3) != 0;
  if (!span_ok(op.w_off, x6 ? fp_dwblock_x6_we_floats(op) : (int64_t)op.Cin * op.Cmid, wf)) return FP_ERR_BOUNDS;
  if (!span_ok(op.scale_off, 15 * (int64_t)op.Cmid, wf)) return FP_ERR_BOUNDS;
  const int64_t wp = x6 ? fp_dwblock_x6_wp_floats(op) : (int64_t)op.Cmid * op.Cout + 2 * (int64_t)op.Cout;
  return span_ok(op.slope_off, wp, wf) ? FP_OK : FP_ERR_BOUNDS;
}
static int spans_blazepair(const fp_op& op, size_t wf, size_t) {
  // both blocks' parameters back to back (facepath.h BLAZEPAIR)
  // stride 2: the second block is the stride-2 block behind a stride-1 block (24 -> 24 or 24 -> 48; blazepair_s2_kernel in blazepair.hip)
  const int64_t pw2 = op.stride == 2 && op.Cout == 48 ? 2 * 768 : 768, c2 = op.stride == 2 ? op.Cout : 24;
  return span_ok(op.w_off, 2 * 9 * 24, wf) && span_ok(op.scale_off, 2 * 24, wf) && span_ok(op.slope_off, 768 + pw2, wf) &&
                 span_ok(op.bias_off, 24 + c2, wf) ? FP_OK : FP_ERR_BOUNDS;
}
// one parameter block at w_off (facepath.h BLAZECHAIN, SHUFDOWN, SHUFUNIT, YSTEM2; YSTEM2's pooled map: validate_op)
static int spans_blazechain(const fp_op& op, size_t wf, size_t) { return spans_w(op, fp_blazechain_w_floats(op), wf); }
static int spans_shufdown(const fp_op& op, size_t wf, size_t) { return spans_w(op, fp_shufdown_w_floats(op), wf); }
static int spans_shufunit(const fp_op& op, size_t wf, size_t) { return spans_w(op, fp_shufunit_w_floats(op), wf); }
static int spans_ystem2(const fp_op& op, size_t wf, size_t) { return spans_w(op, fp_ystem2_w_floats(op), wf); }
static int spans_embed_head(const fp_op& op, size_t wf, size_t) {
  // [Cout][Cin] Linear weight, optional [Cout] affine (facepath.h EMBED_HEAD)
  if (!span_ok(op.w_off, (int64_t)op.Cout * op.Cin, wf)) return FP_ERR_BOUNDS;
  if (op.scale_off >= 0 && !span_ok(op.scale_off, op.Cout, wf)) return FP_ERR_BOUNDS;
  if (op.bias_off >= 0 && !span_ok(op.bias_off, op.Cout, wf)) return FP_ERR_BOUNDS;
  return FP_OK;
}
static int spans_pool_lrn(const fp_op& op, size_t wf, size_t) {
  return op.Cmid ? spans_w(op, 4, wf) : FP_OK;   // [alpha, beta, k, unused] (facepath.h POOL_LRN)
}
static int spans_cls_head(const fp_op& op, size_t wf, size_t af) {
  // [Cout][Cin] weight, optional [Cout] bias, optional logits view at res_off (facepath.h CLS_HEAD)
  if (!span_ok(op.w_off, (int64_t)op.Cout * op.Cin, wf)) return FP_ERR_BOUNDS;
  if (op.bias_off >= 0 && !span_ok(op.bias_off, op.Cout, wf)) return FP_ERR_BOUNDS;
  if (op.res_off >= 0 && !span_ok(op.res_off, res_extent(op, 1, op.Cout), af)) return FP_ERR_BOUNDS;
  return FP_OK;
}

// ---- k_kinds[kind]: one row per fp_op_kind, in the order of their values: who launches it and what validate_op checks ----
enum : unsigned {
  T_COUT = 1,        // has output channels of its own (fp_op.Cout); the others write Cin channels
  T_OUT_HW = 2,      // the output map is OH x OW; the others write the H x W map
  T_WINDOW = 4,      // KH / KW / stride / pad_t / pad_l are checked
  T_EXT_IN = 8,      // the input is an external buffer (in_off indexes fp_ext; sizes are checked at launch)
  T_CMID = 16,       // may carry Cmid
  T_ROWWIN = 32,     // may carry a row window (facepath.h "Row windows")
  T_EPILOGUE = 64,   // [Cout] scale / bias / slope epilogue with act in FP_ACT_NONE .. FP_ACT_SILU
  T_RES = 128,       // has a residual view (res_mode)
  T_SHUFFLE2 = 256,  // ... and may be FP_RES_SHUFFLE2, writing 2 * Cout channels
  T_ACT2 = 512,      // may carry act2 (its value is the launcher's business, or the spans function's)
  T_W_FIRST = 1024,  // a refused act2 is reported after the spans function, not before it (the unfused ops)
};
typedef int launch_fn(const fp_op& op, const fp_launch& L);
static bool is_split3(const fp_op& op) { return (op.flags & FP_OPF_SPLIT3) != 0; }
static bool is_stride2(const fp_op& op) { return op.stride == 2; }

struct kind_row {
  launch_fn* launch;
  unsigned traits;
  int32_t flags;                             // FP_OPF_* bits the kind may carry
  spans_fn* spans = nullptr;                 // null: no parameters
  bool (*use_alt)(const fp_op&) = nullptr;   // where two launchers exist: launch_alt takes the ops this selects
  launch_fn* launch_alt = nullptr;
};
static constexpr unsigned T_CONVLIKE = T_COUT | T_OUT_HW | T_WINDOW;
static constexpr int32_t ROWPADS = FP_OPF_IN_ROWPAD | FP_OPF_OUT_ROWPAD;
static constexpr kind_row k_kinds[] = {
    {nullptr, T_OUT_HW, 0},   // 0: no such kind
    {fp_launch_conv, T_CONVLIKE | T_EPILOGUE | T_RES | T_SHUFFLE2 | T_W_FIRST,
     FP_OPF_OUT_ROWPAD | FP_OPF_IN_C3 | FP_OPF_SPLIT3 | FP_OPF_IN_UP2 | FP_OPF_OUT_DW, spans_conv},
    {fp_launch_dwconv, T_OUT_HW | T_WINDOW | T_EPILOGUE | T_W_FIRST, 0, spans_dwconv},
    {fp_launch_maxpool, T_OUT_HW | T_WINDOW, 0},
    {fp_launch_upsample2x, T_OUT_HW, 0},
    {fp_launch_copy, 0, FP_OPF_OUT_ROWPAD},
    {fp_launch_l2norm, 0, 0},
    {fp_launch_blazeblock, T_CONVLIKE | T_RES | T_W_FIRST, ROWPADS, spans_blazeblock},
    {fp_launch_dwpw, T_CONVLIKE | T_RES | T_SHUFFLE2 | T_ACT2, FP_OPF_SPLIT3, spans_dwpw, is_split3, fp_launch_dwpwx6},
    {fp_launch_ystem, T_CONVLIKE, FP_OPF_IN_C3, spans_ystem},
    {fp_launch_ystem_u8, T_CONVLIKE | T_EXT_IN, 0, spans_ystem},
    {fp_launch_stem_u8, T_CONVLIKE | T_EXT_IN | T_ROWWIN | T_EPILOGUE | T_W_FIRST, FP_OPF_OUT_ROWPAD | FP_OPF_SPLIT3, spans_stem_u8},
    {fp_launch_dwblock, T_CONVLIKE | T_CMID | T_RES, FP_OPF_SPLIT3, spans_dwblock, is_split3, fp_launch_dwblock_x6},
    {fp_launch_blazepair, T_CONVLIKE | T_ROWWIN, ROWPADS, spans_blazepair, is_stride2, fp_launch_blazepair_s2},
    {fp_launch_blazechain, T_CONVLIKE | T_CMID, FP_OPF_SPLIT3, spans_blazechain},
    {fp_launch_shufdown, T_CONVLIKE | T_CMID | T_ACT2, FP_OPF_SPLIT3, spans_shufdown},
    {fp_launch_shufunit, T_CONVLIKE | T_CMID | T_ACT2, FP_OPF_SPLIT3, spans_shufunit},
    {fp_launch_ystem2, T_CONVLIKE | T_ACT2, FP_OPF_SPLIT3, spans_ystem2},
    {fp_launch_embed_head, T_COUT | T_OUT_HW, FP_OPF_OUT_L2, spans_embed_head},
    {fp_launch_pool_lrn, T_OUT_HW | T_WINDOW | T_CMID, 0, spans_pool_lrn},
    {fp_launch_cls_head, T_COUT | T_OUT_HW, 0, spans_cls_head},
};
constexpr int N_KINDS = sizeof(k_kinds) / sizeof(k_kinds[0]);
static_assert(N_KINDS == FP_OP_CLS_HEAD + 1, "one row per fp_op_kind, in the order of their values");

static const kind_row& row_of(const fp_op& op) { return k_kinds[op.kind > 0 && op.kind < N_KINDS ? op.kind : 0]; }

static int launch_op(const fp_op& op, const fp_launch& L) {
  const kind_row& k = row_of(op);
  if (!k.launch) return FP_ERR_UNSUPPORTED;
  return (k.use_alt && k.use_alt(op) ? k.launch_alt : k.launch)(op, L);
}

// The launcher's dry run (common.h fp_launch): its status, and with `name` the kernel instance it would launch.
static int dry_run(const fp_op& op, char* name) {
  const fp_launch L = {nullptr, nullptr, nullptr, 0, nullptr, true, name};
  return launch_op(op, L);
}

// What every kind shares: dimensions, row window, flags, window geometry, the launcher's dry run, the in / out views, then
// the kind's own spans, the [Cout] epilogue and the residual view.  The order of the checks decides the status of an op
// that breaks several of them; tests/test_validate_statuses.py pins it.
static int validate_op(const fp_op& op, size_t weight_floats, size_t arena_floats) {
  const kind_row& k = row_of(op);
  const auto has = [&](unsigned t) { return (k.traits & t) != 0; };
  if (op.N <= 0 || op.H <= 0 || op.W <= 0 || op.Cin <= 0) return FP_ERR_INVALID_ARG;
  const int OH = has(T_OUT_HW) ? op.OH : op.H, OW = has(T_OUT_HW) ? op.OW : op.W;
  if (OH <= 0 || OW <= 0) return FP_ERR_INVALID_ARG;
  const int Cout = has(T_COUT) ? op.Cout : op.Cin;
  if (op.Cmid != 0 && !has(T_CMID)) return FP_ERR_INVALID_ARG;
  if (op.kind == FP_OP_POOL_LRN && op.Cout != op.Cin) return FP_ERR_INVALID_ARG;
  if (op.row_lo != 0 || op.row_end != 0) {
    // a row window: only the kernels that take one (of the u8 stems, the launcher refuses it outside the band kernel),
    // never empty, inside the output map
    if (!has(T_ROWWIN)) return FP_ERR_UNSUPPORTED;
    if (op.row_lo < 0 || op.row_end <= op.row_lo || op.row_end > OH) return FP_ERR_INVALID_ARG;
  }
  if (Cout <= 0 || op.out_cmul < 1 || op.in_ld < op.Cin) return FP_ERR_INVALID_ARG;
  // flags (facepath.h FP_OPF_*): a bit the kind may not carry is an argument error, a row-padded view it does not take is
  // unsupported
  const int32_t refused = op.flags & ~k.flags;
  if (refused & ~ROWPADS) return FP_ERR_INVALID_ARG;
  if (op.flags & FP_OPF_OUT_DW) {
    // Mobile-FaceNet's conv1 + conv2_dw: the conv's slopes are followed by the depthwise block's [12][Cout]
    if (!span_ok(op.slope_off, 13 * (int64_t)op.Cout, weight_floats)) return FP_ERR_BOUNDS;
    if (!span_ok(op.w_off, fp_stemdw_w_floats(op), weight_floats)) return FP_ERR_BOUNDS;
  }
  if (op.flags & FP_OPF_IN_UP2) {
    // channels [0, res_C) come from the res view at half resolution: only the split-MFMA pointwise kernel reads that
    if (!(op.flags & FP_OPF_SPLIT3)) return FP_ERR_INVALID_ARG;
    if (!span_ok(op.res_off, res_extent(op, (int64_t)op.res_H * op.res_W, op.res_C), arena_floats)) return FP_ERR_BOUNDS;
  }
  if ((op.flags & FP_OPF_IN_C3) && op.Cin != 4) return FP_ERR_INVALID_ARG;
  const bool in_rp = (op.flags & FP_OPF_IN_ROWPAD) != 0, out_rp = (op.flags & FP_OPF_OUT_ROWPAD) != 0;
  if (refused) return FP_ERR_UNSUPPORTED;
  if (out_rp && (op.out_cmul != 1 || op.out_ld != Cout)) return FP_ERR_UNSUPPORTED;
  if (has(T_WINDOW)) {
    if (op.KH <= 0 || op.KW <= 0 || op.stride <= 0 || op.pad_t < 0 || op.pad_l < 0) return FP_ERR_INVALID_ARG;
    // every output pixel must have at least its first tap row/col addressable without overflow of int math
    if ((int64_t)(OH - 1) * op.stride - op.pad_t >= op.H || (int64_t)(OW - 1) * op.stride - op.pad_l >= op.W)
      return FP_ERR_INVALID_ARG;
  }
  // YSTEM2's pooled map (the res view) first: a view outside the arena is a bounds error before the launcher compares it
  // with the output (it refuses an output that aliases either input)
  if (op.kind == FP_OP_YSTEM2 && !span_ok(op.res_off, res_extent(op, (int64_t)op.OH * op.OW, op.res_C), arena_floats))
    return FP_ERR_BOUNDS;
  // what the kernel itself requires: the launcher's checks, in a dry run
  int rc = dry_run(op, nullptr);
  if (rc != FP_OK) return rc;
  // the in view (an external input only names its fp_ext) and the out view
  rc = has(T_EXT_IN) ? (op.in_off < 0 ? FP_ERR_INVALID_ARG : FP_OK)
                     : view_status(in_rp, op.in_off, op.in_ns, op.in_ld, op.N, op.H, op.W, op.Cin, arena_floats);
  if (rc != FP_OK) return rc;
  const int64_t out_ch = has(T_SHUFFLE2) && op.res_mode == FP_RES_SHUFFLE2 ? 2 * (int64_t)Cout : Cout;
  rc = view_status(out_rp, op.out_off, op.out_ns, op.out_ld, op.N, OH, OW, (out_ch - 1) * op.out_cmul + 1, arena_floats);
  if (rc != FP_OK) return rc;
  if (op.in_ns < 0 || op.out_ns < 0) return FP_ERR_INVALID_ARG;

  const bool act2_refused = op.act2 != FP_ACT_NONE && !has(T_ACT2);
  if (act2_refused && !has(T_W_FIRST)) return FP_ERR_INVALID_ARG;
  if (k.spans && (rc = k.spans(op, weight_floats, arena_floats)) != FP_OK) return rc;
  if (act2_refused) return FP_ERR_INVALID_ARG;
  if (has(T_EPILOGUE)) {
    if (op.scale_off >= 0 && !span_ok(op.scale_off, Cout, weight_floats)) return FP_ERR_BOUNDS;
    if (op.bias_off >= 0 && !span_ok(op.bias_off, Cout, weight_floats)) return FP_ERR_BOUNDS;
    if (op.slope_off >= 0 && !span_ok(op.slope_off, Cout, weight_floats)) return FP_ERR_BOUNDS;
    if (op.act == FP_ACT_PRELU && op.slope_off < 0) return FP_ERR_INVALID_ARG;
    if (op.act < FP_ACT_NONE || op.act > FP_ACT_SILU) return FP_ERR_INVALID_ARG;
  }
  if (has(T_RES) && op.res_mode != FP_RES_NONE) {
    if (op.res_mode < FP_RES_NONE || op.res_mode > FP_RES_SHUFFLE2) return FP_ERR_INVALID_ARG;
    if (op.res_mode == FP_RES_SHUFFLE2 && (!has(T_SHUFFLE2) || op.out_cmul != 1 || op.out_ld < 2 * op.Cout))
      return FP_ERR_INVALID_ARG;
    if (op.res_C <= 0 || op.res_ld < op.res_C || op.res_ns < 0) return FP_ERR_INVALID_ARG;
    const bool pool2 = op.res_mode == FP_RES_POOL2_BEFORE_ACT;   // the res view is the un-pooled map
    if (pool2 && (op.res_H < 2 * OH || op.res_W < 2 * OW)) return FP_ERR_INVALID_ARG;
    const int64_t res_hw = pool2 ? (int64_t)op.res_H * op.res_W : (int64_t)OH * OW;
    if (!span_ok(op.res_off, res_extent(op, res_hw, op.res_C), arena_floats)) return FP_ERR_BOUNDS;
  }
  return FP_OK;
}

extern "C" {

int fp_abi_version(void) { return FP_ABI_VERSION; }

void fp_debug_reload_env(void) { g_knobs = read_knobs(); }

const char* fp_last_hip_error(void) { return g_hip_err; }

// host mirror of the device-side fp_fastdiv (common.h): __umulhi(n, mul) >> shift
static unsigned fastdiv_host(unsigned n, fp_divisor d) { return (unsigned)(((unsigned long long)n * d.mul) >> 32) >> d.shift; }

int fp_selftest(void) {
  auto check = [&](unsigned d) -> bool {
    const fp_divisor dv = fp_make_divisor(d);
    const unsigned nmax = 0x7fffffffu, qmax = nmax / d;
    const unsigned qs[] = {0u, 1u, 2u, qmax / 3, qmax / 2, qmax - 1, qmax};
    for (unsigned q : qs) {
      const unsigned long long lo = (unsigned long long)q * d;
      const unsigned long long cand[] = {lo, lo + 1, lo + d - 1, lo + d / 2};
      for (unsigned long long n64 : cand) {
        if (n64 > nmax) continue;
        const unsigned n = (unsigned)n64;
        if (fastdiv_host(n, dv) != n / d) {
          snprintf(g_hip_err, sizeof(g_hip_err), "fp_fastdiv(%u, %u) = %u, expected %u", n, d, fastdiv_host(n, dv), n / d);
          return false;
        }
      }
    }
    if (fastdiv_host(nmax, dv) != nmax / d) {
      snprintf(g_hip_err, sizeof(g_hip_err), "fp_fastdiv(%u, %u) wrong at the top of the range", nmax, d);
      return false;
    }
    return true;
  };
  for (unsigned d = 2; d <= 4096; ++d)
    if (!check(d)) return FP_ERR_INVALID_ARG;
  const unsigned big[] = {4097u, 12321u, 16384u, 65535u, 65536u, 65537u, 1000003u, 16777216u, 123456789u, 1u << 30, (1u << 30) + 1u};
  for (unsigned d : big)
    if (!check(d)) return FP_ERR_INVALID_ARG;
  return FP_OK;
}

const char* fp_strerror(int status) {
  switch (status) {
    case FP_OK: return "ok";
    case FP_ERR_INVALID_ARG: return "invalid argument";
    case FP_ERR_BOUNDS: return "op touches memory outside the arena or weight blob";
    case FP_ERR_UNSUPPORTED: return "unsupported op or parameter combination";
    case FP_ERR_LAUNCH: return "HIP kernel launch failed";
    case FP_ERR_ALIGNMENT: return "channel count / stride / offset not a multiple of 4 floats";
    default: return "unknown status";
  }
}

// Name of the HIP kernel an op launches (the family rocprofv3's kernel trace shows), for measurement tools: the
// launcher's own choice, "?" for an op it refuses.
const char* fp_op_kernel_name(const fp_op* op) {
  static thread_local char buf[FP_KERNEL_NAME_MAX];
  if (!op || dry_run(*op, buf) != FP_OK) return "?";
  return buf;
}

int fp_plan_validate(const fp_op* ops, int n_ops, size_t weight_floats, size_t arena_floats) {
  if (!ops || n_ops < 0) return FP_ERR_INVALID_ARG;
  for (int i = 0; i < n_ops; ++i) {
    int rc = validate_op(ops[i], weight_floats, arena_floats);
    if (rc != FP_OK) return rc;
  }
  return FP_OK;
}

struct fp_timer {
  int n;
  hipEvent_t* start;
  hipEvent_t* stop;
  unsigned char* used;
};

// The plan executor: validates every op, then launches them in order.  With a timer, the ops op_mask selects are
// bracketed by its events.
static int run_plan(const fp_op* ops, int n_ops, const float* weights, size_t weight_floats, float* arena, size_t arena_floats,
                    const fp_ext* ext, int n_ext, void* stream, fp_timer* t, const unsigned char* op_mask) {
  if (!weights || !arena || n_ext < 0 || (n_ext > 0 && !ext)) return FP_ERR_INVALID_ARG;
  const fp_launch L = {weights, arena, ext, n_ext, (hipStream_t)stream, false, nullptr};
  int rc = fp_plan_validate(ops, n_ops, weight_floats, arena_floats);
  if (rc != FP_OK) return rc;
  for (int i = 0; i < n_ops; ++i) {
    const bool timed = t && op_mask[i];
    if (t) t->used[i] = op_mask[i];
    if (timed) (void)hipEventRecord(t->start[i], L.s);
    rc = launch_op(ops[i], L);
    if (rc != FP_OK) return rc;
    if (timed) (void)hipEventRecord(t->stop[i], L.s);
  }
  return FP_OK;
}

int fp_plan_run_ext(const fp_op* ops, int n_ops, const float* weights, size_t weight_floats, float* arena,
                    size_t arena_floats, const fp_ext* ext, int n_ext, void* stream) {
  return run_plan(ops, n_ops, weights, weight_floats, arena, arena_floats, ext, n_ext, stream, nullptr, nullptr);
}

int fp_plan_run(const fp_op* ops, int n_ops, const float* weights, size_t weight_floats, float* arena,
                size_t arena_floats, void* stream) {
  return fp_plan_run_ext(ops, n_ops, weights, weight_floats, arena, arena_floats, nullptr, 0, stream);
}

int fp_timer_create(int n_ops, void** out) {
  if (!out || n_ops <= 0) return FP_ERR_INVALID_ARG;
  fp_timer* t = new fp_timer;
  t->n = n_ops;
  t->start = new hipEvent_t[n_ops];
  t->stop = new hipEvent_t[n_ops];
  t->used = new unsigned char[n_ops];
  for (int i = 0; i < n_ops; ++i) {
    t->used[i] = 0;
    if (hipEventCreate(&t->start[i]) != hipSuccess || hipEventCreate(&t->stop[i]) != hipSuccess) {
      fp_set_hip_error(hipGetLastError());
      return FP_ERR_LAUNCH;
    }
  }
  *out = t;
  return FP_OK;
}

void fp_timer_destroy(void* timer) {
  fp_timer* t = (fp_timer*)timer;
  if (!t) return;
  for (int i = 0; i < t->n; ++i) {
    (void)hipEventDestroy(t->start[i]);
    (void)hipEventDestroy(t->stop[i]);
  }
  delete[] t->start;
  delete[] t->stop;
  delete[] t->used;
  delete t;
}

int fp_plan_run_timed_ext(const fp_op* ops, int n_ops, const float* weights, size_t weight_floats, float* arena,
                          size_t arena_floats, const fp_ext* ext, int n_ext, void* stream, void* timer,
                          const unsigned char* op_mask) {
  fp_timer* t = (fp_timer*)timer;
  if (!t || !op_mask || t->n < n_ops) return FP_ERR_INVALID_ARG;
  return run_plan(ops, n_ops, weights, weight_floats, arena, arena_floats, ext, n_ext, stream, t, op_mask);
}

int fp_plan_run_timed(const fp_op* ops, int n_ops, const float* weights, size_t weight_floats, float* arena,
                      size_t arena_floats, void* stream, void* timer, const unsigned char* op_mask) {
  return fp_plan_run_timed_ext(ops, n_ops, weights, weight_floats, arena, arena_floats, nullptr, 0, stream, timer, op_mask);
}

int fp_timer_accumulate(void* timer, float* ms_accum, int n_ops) {
  fp_timer* t = (fp_timer*)timer;
  if (!t || !ms_accum || n_ops > t->n) return FP_ERR_INVALID_ARG;
  for (int i = 0; i < n_ops; ++i) {
    if (!t->used[i]) continue;
    if (hipEventSynchronize(t->stop[i]) != hipSuccess) {
      fp_set_hip_error(hipGetLastError());
      return FP_ERR_LAUNCH;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t->start[i], t->stop[i]) != hipSuccess) {
      fp_set_hip_error(hipGetLastError());
      return FP_ERR_LAUNCH;
    }
    ms_accum[i] += ms;
  }
  return FP_OK;
}

}  // extern "C"
