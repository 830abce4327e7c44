/*
 * facepath.h — C ABI of libfacepath.so (MI355X / gfx950 only).
 *
 * The drop-in boundary for the detect -> embed -> similarity-filter hot path of
 * SamSamhuns/face_detection_and_recognition.  The reference is 100 % Python and
 * has no native boundary of its own; every entry point below
 * therefore names the *Python* symbol of the reference whose arithmetic it
 * replaces (paths relative to the reference root, fde = face_detection_and_extraction).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - Every pointer is a DEVICE pointer unless the parameter is documented "host".
 *   - The caller owns every buffer (activations arena, weights, outputs).  The
 *     library never allocates device memory and keeps no mutable global state.
 *   - Stream-ordered: work is enqueued on `stream` (a hipStream_t passed as void*;
 *     NULL = the null stream) and the call returns without synchronising.
 *   - Return value: FP_OK (0) or a negative fp_status; fp_strerror() gives text.
 *   - Activations are NHWC fp32: element (n,y,x,c) of a view lives at
 *     base + n*ns + (y*W + x)*ld + c   (ns, ld in floats).
 */
#ifndef FACEPATH_H
#define FACEPATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FP_ABI_VERSION 15

typedef enum fp_status {
  FP_OK = 0,
  FP_ERR_INVALID_ARG = -1,   /* NULL pointer, negative size, unsupported shape */
  FP_ERR_BOUNDS = -2,        /* an op would touch memory outside the arena / weight blob */
  FP_ERR_UNSUPPORTED = -3,   /* op kind / parameter combination not implemented */
  FP_ERR_LAUNCH = -4,        /* hipGetLastError() != hipSuccess after a launch */
  FP_ERR_ALIGNMENT = -5      /* channel counts / strides / offsets not multiples of 4 floats where required */
} fp_status;

int fp_abi_version(void);
const char* fp_strerror(int status);
/* Last HIP error string seen by this thread's failing call ("" if none). */
const char* fp_last_hip_error(void);
/*
 * Host-only consistency check of the library's integer helpers (no GPU needed): the reciprocal-multiply division the
 * persistent kernels use for pixel -> (image, row, column) decode, fp_make_divisor / fp_fastdiv, against the hardware
 * division for every divisor 2 .. 4096 and selected ones up to 2^30, at the boundaries of each quotient and at 2^31 - 1.
 * Returns FP_OK or FP_ERR_INVALID_ARG (with the failing pair in fp_last_hip_error's buffer).
 */
int fp_selftest(void);
/*
 * The test knob FP_RESIZE_PER_PIXEL is read from the environment ONCE, when the library is loaded; no launch calls
 * getenv.  This re-reads it (tests that switch it at run time call this after changing the environment).  Not for production use: it is the library's only
 * process-wide mutable state, and it must not be called while another thread is launching.
 */
void fp_debug_reload_env(void);

/* ------------------------------------------------------------------------- */
/* 1. Network plans: one flat array of ops, executed back-to-back on a stream. */
/* ------------------------------------------------------------------------- */

enum fp_op_kind {
  FP_OP_CONV = 1,       /* dense conv KHxKW (1x1 = pointwise GEMM), fp32 MFMA implicit GEMM */
  FP_OP_DWCONV = 2,     /* depthwise conv KHxKW */
  FP_OP_MAXPOOL = 3,    /* max pool, -inf padding, OH/OW given by caller (covers ceil_mode) */
  FP_OP_UPSAMPLE2X = 4, /* nearest-neighbour 2x */
  FP_OP_COPY = 5,       /* channel-slice copy (concat / chunk / shuffle interleave) */
  FP_OP_L2NORM = 6,     /* out[m,:] = in[m,:] / ||in[m,:]||_2 over Cin channels (mobile_facenet.py:30-33), no epsilon; row m = pixel
                           m % (H*W) of image m / (H*W), both views by the general rule (off + n*ns + pix*ld + c, any ns / ld) */
  FP_OP_BLAZEBLOCK = 7, /* fused BlazeBlock: dw3x3 -> 1x1 -> (+shortcut) -> ReLU (blazeface.py:12-47) */
  FP_OP_DWPW = 8,       /* fused Depth_Wise tail: dw3x3(+BN,+PReLU) -> 1x1(+BN) [+x] (mobile_facenet.py:72-85) */
  FP_OP_YSTEM = 9,      /* head of YOLOv5-face's StemBlock (y5/models/common.py:58-73): stem_1 (3x3 s2, SiLU) kept in LDS ->
                           stem_2a (1x1, SiLU) -> out, and maxpool2x2(stem_1) -> res view (the concat half stem_3 reads) */
  FP_OP_YSTEM_U8 = 10,  /* FP_OP_YSTEM reading the u8 frames directly: the letterbox (fp_resize_normalize's arithmetic through
                           fp_letterbox_tables) happens while the input tile is staged; needs fp_plan_run_ext */
  FP_OP_STEM_U8 = 11,   /* first conv of a network (KxK in {3,5}, stride 2, Cout <= 64, dense NHWC output; BlazeFace's stem,
                           blazeface.py:118-120,195) reading the u8 frames the same way; needs fp_plan_run_ext */
  FP_OP_BLAZEPAIR = 13, /* TWO consecutive stride-1 24 -> 24 BlazeBlocks (blazeface.py:12-47,122-152) in one kernel: the tensor
                           between them stays in an LDS ring.  Row-padded input, 128- or 64-pixel-wide map; with stride = 2 the second block is
                           the stride-2 block that ends the stage (24 -> 24 / 48, half-size output); see "BLAZEPAIR" */
  FP_OP_BLAZECHAIN = 14, /* a RUN of fp_op.Cmid consecutive stride-1 96 -> 96 BlazeBlocks on the 16 x 16 map (blazeface.py:12-47,
                           146-152) in one kernel: one image per workgroup stays in LDS for the whole run.  See "BLAZECHAIN" */
  FP_OP_DWBLOCK = 12,   /* a WHOLE Depth_Wise block (mobile_facenet.py:67-88) in one kernel: 1x1 expand (+BN, PReLU) ->
                           dw3x3 stride 1 (+BN, PReLU) -> 1x1 project (+BN) [+ x]; the expanded tensor (Cmid channels)
                           lives in LDS only.  Shapes: see "DWBLOCK" below; anything else fails validation */
  FP_OP_YSTEM2 = 17,    /* ABI 10.  the tail of YOLOv5-face's StemBlock (y5/models/common.py:58-73) in one kernel: stem_2b (3x3 stride 2, c/2 -> c,
                           SiLU) -> cat with the pooled stem_1 map -> stem_3 (1x1, 2c -> c, SiLU); stem_2b's output never reaches HBM.  See "YSTEM2" */
  FP_OP_SHUFUNIT = 16,  /* ABI 10.  a WHOLE stride-1 ShuffleV2Block (y5/models/common.py:127-176): x1, x2 = x.chunk(2); branch2(x2) = 1x1 + BN
                           + SiLU -> dw3x3 + BN -> 1x1 + BN + SiLU; out = channel_shuffle(cat(x1, branch2)) in one kernel.  See "SHUFUNIT" */
  FP_OP_SHUFDOWN = 15,  /* ABI 10.  a WHOLE stride-2 ShuffleV2Block (y5/models/common.py:127-176) in one kernel: branch1 = dw3x3 s2 + BN
                           -> 1x1 + BN + SiLU, branch2 = 1x1 + BN + SiLU -> dw3x3 s2 + BN -> 1x1 + BN + SiLU, cat + channel_shuffle(2)
                           as the store pattern; nothing but x and the shuffled output touches HBM.  See "SHUFDOWN" */
  FP_OP_EMBED_HEAD = 18, /* (appended at ABI 14) an embedding head in one kernel: mean over the H x W pixels of each image -> Linear Cin -> Cout
                           (no bias) -> per-channel affine (BatchNorm1d) -> with FP_OPF_OUT_L2, x / max(||x||_2, 1e-12) (F.normalize).
                           Inception-ResNet-v1's avgpool_1a + last_linear + last_bn (+ normalize).  See "EMBED_HEAD" */
  FP_OP_POOL_LRN = 19,  /* (appended at ABI 14) max pool (-inf padding, OH/OW given: covers Caffe's ceil mode) followed by Caffe's
                           cross-channel LRN within channel groups: Levi-Hassner's pool1 + norm1, pool2 + norm2.  See "POOL_LRN" */
  FP_OP_CLS_HEAD = 20   /* (appended at ABI 14) classifier head: Linear Cin -> Cout (+ bias) on every row, then softmax over the Cout
                           logits (Levi-Hassner's fc8 + prob).  See "CLS_HEAD" */
};

enum fp_act { FP_ACT_NONE = 0, FP_ACT_RELU = 1, FP_ACT_PRELU = 2, FP_ACT_SILU = 3 };

enum fp_res_mode {
  FP_RES_NONE = 0,
  FP_RES_ADD_BEFORE_ACT = 1, /* act(conv + res): BlazeBlock (blazeface.py:47) */
  FP_RES_ADD_AFTER_ACT = 2,  /* res + act(conv): Depth_Wise residual (mobile_facenet.py:84-85), Bottleneck (common.py:87) */
  FP_RES_POOL2_BEFORE_ACT = 3, /* res = maxpool2x2(input map) zero-padded on channels (blazeface.py:38-45) */
  FP_RES_SHUFFLE2 = 4        /* ShuffleV2Block tail, cat + channel_shuffle(2) (y5/models/common.py:169-176,21-31): the op
                                writes 2*Cout channels, out[2n] = res[n] (the other branch / pass-through half),
                                out[2n+1] = act(conv)[n]; out_cmul = 1, 16-byte stores (vector epilogue only) */
};

/*
 * One op.  All *_off fields are offsets in FLOATS: in/out/res into the
 * activation arena, w/scale/bias/slope into the weight blob (-1 = absent).
 * Epilogue of CONV / DWCONV:  v = acc * scale[c] + bias[c]  (scale absent = 1,
 * bias absent = 0), then residual/activation per res_mode/act; PReLU uses slope[c].
 * Output element (n, oy, ox, c) is written at
 *   out_off + n*out_ns + (oy*OW + ox)*out_ld + c*out_cmul        (out_cmul >= 1)
 * Zero padding: taps that fall outside [0,H)x[0,W) read 0 (MAXPOOL: -inf), so
 * asymmetric TFLite-style padding (blazeface.py:195, :38) is pad_t/pad_l plus OH/OW.
 */
typedef struct fp_op {
  int32_t kind;
  int32_t act;
  int32_t res_mode;
  int32_t N, H, W;        /* input batch / height / width */
  int32_t OH, OW;         /* output height / width */
  int32_t Cin, Cout;
  int32_t KH, KW, stride;
  int32_t pad_t, pad_l;
  int32_t in_ld, out_ld, res_ld;   /* per-pixel stride (floats) */
  int32_t out_cmul;                /* output channel multiplier (1 = dense, 2 = shuffle interleave) */
  int32_t res_C;                   /* channels available in the residual; c >= res_C adds 0 */
  int32_t res_H, res_W;            /* spatial dims of the residual map (POOL2: the un-pooled map) */
  int64_t in_ns, out_ns, res_ns;   /* per-image stride (floats) */
  int64_t in_off, out_off, res_off;
  int64_t w_off, scale_off, bias_off, slope_off;
  int32_t act2;                    /* fused ops: activation of the SECOND conv's output (DWPW: FP_ACT_NONE / FP_ACT_SILU) */
  int32_t flags;                   /* FP_OPF_* bits (0 for dense tensors) */
  int32_t Cmid;                    /* ABI 4.  DWBLOCK: channels of the expanded tensor (Depth_Wise `groups`); BLAZECHAIN: number of blocks; 0 elsewhere */
  int16_t row_lo, row_end;         /* output row window [row_lo, row_end); 0, 0: the whole map.  See "Row windows" (these two
                                      halves were ABI 4's reserved0, which had to be 0: the layout and every existing caller are
                                      unchanged) */
} fp_op;

/*
 * Row windows.  An op with row_end > 0 computes output rows row_lo .. row_end - 1 of every image and MAY leave
 * every other output row as it was: the caller guarantees that those rows already hold what the op would write there
 * (BlazeFace on letterboxed frames: the rows whose receptive field holds only the canvas pad are the same in every
 * frame, so one unrestricted run leaves them right for the plan's life).  Rows outside the window are still READ where a
 * window row's receptive field reaches them.  0 <= row_lo < row_end <= OH; an empty or out-of-range window is
 * FP_ERR_INVALID_ARG.  Only these ops take a window (anything else with row_end > 0: FP_ERR_UNSUPPORTED):
 *   FP_OP_STEM_U8 on the 5x5 band kernels (fp_stem_u8_band_eligible: BlazeFace-back's stem, N >= 16) and
 *   FP_OP_BLAZEPAIR (stride 1 and 2).
 * A windowed launch spreads the window's rows over its bands (band heights are chosen to fill whole rounds of workgroup
 * slots); bands may overlap by a few rows, which are then written twice with the same values.
 */

/*
 * Row-padded activation layout (ABI 3).  A tensor in this layout keeps one ZERO pixel after every image row, one zero
 * row above and one below every image, and one zero pixel in front of the first pad row:
 *     pixel (y, x) of image n  at  off + n*ns + (y*(W + 1) + x)*ld          y in [-1, H], x in [-1, W]
 * (x = -1 is the pad pixel of the row above, so a 3x3 window never needs a bounds check), with
 * ns >= ((H + 2)*(W + 1) + 1)*ld and off - (W + 2)*ld >= 0 the first float of image 0.  Producers write only
 * y in [0, H), x in [0, W); whoever owns the arena zeroes the pads once (plan.py allocates such buffers from a region
 * it never recycles).  The depthwise taps of the BlazeBlocks (blazeface.py:12-47) read it without clamps or masks.
 *   FP_OPF_IN_ROWPAD  : the input view is row-padded.  Accepted (exactly fp_plan_validate's list):
 *                       FP_OP_BLAZEBLOCK stride 1, 24 -> 24, OW % 32 == 0, OW >= 64, OH % 4 == 0, OH >= 8 (blazeblock_wp_kernel);
 *                       FP_OP_BLAZEBLOCK stride 1, 48 -> 48 or 96 -> 96, W = 16 or 32, H*W % 32 == 0, H*W >= 64
 *                       (blazeblock_wps_kernel); FP_OP_BLAZEPAIR (always).  Anything else: FP_ERR_UNSUPPORTED.
 *   FP_OPF_OUT_ROWPAD : the output view is row-padded (out_cmul = 1, out_ld = Cout).  Accepted: FP_OP_BLAZEBLOCK (every
 *                       kernel form), FP_OP_BLAZEPAIR, FP_OP_STEM_U8, FP_OP_CONV on the stem kernel (KxK stride 2 on a
 *                       4-float pixel), FP_OP_COPY with 16-byte-aligned views (Cin, strides and offsets multiples of 4:
 *                       copy4_kernel; the scalar copy cannot write the layout and fails validation).
 */
#define FP_OPF_IN_ROWPAD 1
#define FP_OPF_OUT_ROWPAD 2
/*
 * FP_OPF_IN_C3 : the op reads a 4-float pixel (Cin = in_ld = 4) whose FOURTH channel meets zero weights -- a 3-channel
 *                image padded to 16 bytes, as every network stem here is.  FP_OP_CONV on the stem kernel and
 *                FP_OP_YSTEM skip that channel's MFMAs (a quarter of the stem's matrix work); the result is
 *                unchanged.  The *_U8 ops (Cin = 3) always do.  Only valid with Cin = 4.
 */
#define FP_OPF_IN_C3 4
/*
 * FP_OPF_SPLIT3 (ABI 5) : the op's 1x1-conv weight matrices are packed as THREE bf16 planes (the exact three-way split
 *                of every fp32 weight, w == h + m + l with h = bf16(w), m = bf16(w - h), l = bf16(w - h - m), every conversion
 *                round-to-nearest-even; planes = the bf16 bit patterns of h, m, l) for the "bf16x6" kernels: fp32 operands on
 *                v_mfma_f32_16x16x32_bf16, six products per operand pair, fp32 accumulation; the three dropped products are
 *                < 2^-22.99 of a product and carry either sign (csrc/split.h; gfx950 has no TF32 and its fp32 MFMA runs at
 *                the vector rate).  Accepted (exactly fp_plan_validate's list): FP_OP_DWBLOCK stride 1 with (Cin, H = W) in
 *                {(128, 14), (128, 7), (64, 28)} and stride 2 with (Cin, Cmid, Cout, H) in {(64, 128, 64, 56),
 *                (64, 256, 128, 28), (128, 512, 128, 14)} (layouts under "DWBLOCK"); FP_OP_CONV 1x1 stride 1 or 3x3 pad 1
 *                stride 1 / 2, dense views, Cin and Cout multiples of 4 and >= 32, or 3x3 with Cin 8 / 16 / 24 (K flattened: k = tap * Cin
 *                + channel in slabs of 32) (weights [tap * ceil(Cin / 32) + slab][3
 *                planes][Npad][32] bf16, zero rows / columns in the padding); FP_OP_DWPW 3x3 pad 1 with Cin a multiple of
 *                32 (<= 256) and Cout 64 or 128; FP_OP_BLAZECHAIN (always); FP_OP_CONV with
 *                FP_OPF_OUT_DW (planes [Cout / 16][3][16][32] over k = tap * 3 + channel); FP_OP_STEM_U8 (ABI 11) in BlazeFace's
 *                band shape only (5x5 stride 2 pad 1 on a 256 x 256 canvas, Cout 24, bias + ReLU, N >= 16: stem5_u8_x6_kernel) with
 *                planes [3 slabs][2 channel tiles][3 planes][16][32] over k = 16 (ky - 2 slab) + 3 kx + channel (every ky padded
 *                to 16 k, the sixth ky and channels 24 .. 31 zero).  The semantics of the ops do not change.
 */
#define FP_OPF_SPLIT3 8
/* (bit 16 is unassigned since ABI 15: an op carrying it is FP_ERR_INVALID_ARG, as any unknown bit) */
/*
 * FP_OPF_IN_UP2 (ABI 7) : a pointwise (1x1) FP_OP_CONV on the split-MFMA kernels (FP_OPF_SPLIT3) whose input is
 *                cat(upsample2x_nearest(u), v) -- nn.Upsample + Concat in front of a C3 in YOLOv5-face's head
 *                (y5/models/yolo.py:177-198, common.py:235-242): channels [0, res_C) of pixel (y, x) are read from pixel
 *                (y / 2, x / 2) of the res view (res_H = H / 2, res_W = W / 2, res_C a multiple of 8, res_ld, res_ns,
 *                res_off as for a residual; res_mode must be FP_RES_NONE), channels [res_C, Cin) from the in view as
 *                usual (in_off is the address of channel 0 of the concatenated row; its first res_C floats are never
 *                read).  The upsampled tensor does not exist.
 */
#define FP_OPF_IN_UP2 32
/*
 * FP_OPF_OUT_DW (ABI 9) : an FP_OP_CONV followed by a depthwise 3x3 stride-1 pad-1 Conv_block (conv + BN + PReLU,
 *                mobile_facenet.py:39-51) computed in the same kernel -- Mobile-FaceNet's conv1 + conv2_dw (:107-108, :141-142):
 *                the conv's output tile stays in LDS, the depthwise conv runs on it there and the op writes the DEPTHWISE
 *                output (same shape: OH x OW x Cout).  slope_off -> [Cout] PReLU slopes of the conv followed by [12][Cout] of
 *                the depthwise block: its nine taps (ky*3 + kx), BN scale, BN bias, PReLU slope.  Only the stem shape:
 *                3x3 stride 2 pad 1 on a dense 112 x 112 four-float-pixel image (FP_OPF_IN_C3), Cout 64, scale / bias / PReLU
 *                (csrc/stemdw.hip).
 */
#define FP_OPF_OUT_DW 64
/*
 * FP_OPF_OUT_L2 (appended at ABI 14) : FP_OP_EMBED_HEAD only: each output row is L2-normalised (F.normalize, eps 1e-12).
 */
#define FP_OPF_OUT_L2 128

/*
 * Weight blob layouts (packed by the host side, see
 * face_detection_and_recognition_amd/plan.py):
 *   CONV   : Wp[Kpad/4][Npad][4]  with k = (ky*KW + kx)*Cin + ci, Kpad = roundup(KH*KW*Cin, 8),
 *            Npad = roundup(Cout, 32); element (k, n) at ((k/4)*Npad + n)*4 + k%4; zero padded.
 *   DWCONV : Wd[KH*KW][C]
 *   scale / bias / slope : [Cout]
 *   DWPW   : w_off     -> [9][G] depthwise taps, [G] scale, [G] bias, [G] PReLU slope   (12*G floats)
 *            slope_off -> packed 1x1 weights as for CONV (K = G), then [roundup(Cout,4)] scale, [roundup(Cout,4)] bias
 *            act = FP_ACT_PRELU if the depthwise has a PReLU; res_mode = FP_RES_ADD_AFTER_ACT adds res after the 1x1.
 *            bias_off  -> optional [roundup(Cout,4)] PReLU slopes applied to the 1x1 output (a depthwise Conv_block
 *            followed by a 1x1 Conv_block, mobile_facenet.py:117-118,70); not combined with a residual.
 *            act2 = FP_ACT_SILU applies SiLU to the 1x1 output; res_mode = FP_RES_SHUFFLE2 then writes the tail of a
 *            ShuffleV2Block branch (y5/models/common.py:127-176: dw3x3 + BN -> 1x1 + BN + SiLU, cat with the other
 *            half, channel_shuffle(2)) exactly as FP_OP_CONV does: out[2n] = res[n], out[2n+1] = y[n].
 *   BLAZEBLOCK : w_off -> [9][Cin] taps, scale_off -> [Cin] depthwise bias, slope_off -> packed 1x1, bias_off -> [Cout]
 *   YSTEM  : in = the 4-float-pixel image (Cin = in_ld = 4), H and W multiples of 4; OH x OW = H/2 x W/2 (stem_1 / stem_2a
 *            map), Cout = stem_2a's physical channels (<= 32); the res_* view receives maxpool2x2(stem_1):
 *            res_C = stem_1's physical channels (<= 32), res_H x res_W = OH/2 x OW/2.
 *            w_off -> stem_1 packed as CONV (K = 36 -> 40, Npad = 32), scale_off (-1 = none) / bias_off -> [32];
 *            slope_off -> stem_2a: [2][4][NB2*16][4] with element e of (j, g, n) = W[n][16j + 4g + e] (NB2 =
 *            ceil(Cout/16), zero padded), then [NB2*16] scale, [NB2*16] bias.  Both convs end in SiLU.
 *   YSTEM_U8 : as YSTEM, but the input is EXTERNAL: in_off = index e into the ext[] array of fp_plan_run_ext with
 *            ext[e] = frames [N][fh][fw][3] u8, ext[e+1] = the tap tables fp_letterbox_tables wrote for an H x W canvas
 *            ((W + H + 2) x 8 bytes, W + H <= 2048), ext[e+2] = 256-float normalisation LUT.  H, W = the canvas (model input) size,
 *            Cin = 3, res_H = fh, res_W = fw (the pooled map is OH/2 x OW/2 as for YSTEM).
 *   STEM_U8 : a CONV (weights packed for Cin = 4: k = tap*4 + c, zero fourth channel; scale / bias / slope / act as
 *            CONV, no residual) whose H x W input is the letterbox canvas of external u8 frames: in_off = e with
 *            ext[e .. e+2] = frames, tap tables, LUT as for YSTEM_U8; Cin = 3, res_H = fh, res_W = fw.
 */

/*
 *   DWBLOCK : in = x [N][H][W][Cin] dense NHWC, out = y [N][H][W][Cout], Cout == Cin, stride 1, pad 1, KH = KW = 3.
 *            (Cin, H = W) in {(128, 14), (128, 7), (64, 28)} (every residual block of Mobile-FaceNet,
 *            mobile_facenet.py:119-122,126-130), Cmid a multiple of 32.  res_mode = FP_RES_ADD_AFTER_ACT adds x itself
 *            (the res_* view must be the in_* view), FP_RES_NONE omits the shortcut.
 *            w_off     -> expand weights packed as CONV (K = Cin, Npad = Cmid)
 *            scale_off -> [15][Cmid]: rows 0..2 expand BN scale / BN bias / PReLU slope, rows 3..11 the depthwise taps
 *                         (ky*3 + kx), rows 12..14 depthwise BN scale / BN bias / PReLU slope
 *            slope_off -> project weights packed as CONV (K = Cmid, Npad = Cout), then [Cout] BN scale, [Cout] BN bias
 *            With FP_OPF_SPLIT3 (bf16 elements, 2 per float of the blob; R = Cmid / 32 rounds of 32 expanded channels):
 *            w_off     -> [R][3 planes][Cin / 32][32 g][32 k]: plane p of expand weight (g = 32 r + g', k = 32 ks + k')
 *            slope_off -> [R][3 planes][Cout][32 g]: plane p of project weight (co, g = 32 r + g'), then (fp32) [Cout]
 *                         BN scale, [Cout] BN bias;  scale_off as above.
 *   BLAZEPAIR : in = x (row-padded, FP_OPF_IN_ROWPAD, 24 channels, W = 128 or 64, H a multiple of 8 with H / band rows
 *            >= 2), out = y2 (dense or FP_OPF_OUT_ROWPAD); act = FP_ACT_RELU, res_mode = FP_RES_ADD_BEFORE_ACT (each
 *            block's shortcut is its own input).  The two blocks' parameters back to back, each as for BLAZEBLOCK:
 *            w_off -> [2][9][24] taps, scale_off -> [2][24] depthwise bias, slope_off -> [2] packed 1x1 (K = 24,
 *            Npad = 32: 768 floats each), bias_off -> [2][24] 1x1 bias.
 *            With stride = 2 (ABI 8; blazepair_s2_kernel in csrc/blazepair.hip) the SECOND block is the stride-2 block that ends a stage
 *            (blazeface.py:34-47: F.pad(0, 2, 0, 2), depthwise stride 2, shortcut = 2 x 2 max pool padded on channels): in = x
 *            as above, out = y2 on the H/2 x W/2 map (dense or FP_OPF_OUT_ROWPAD, out_ld = Cout), Cout = 24 or 48, pad_t =
 *            pad_l = 0, res_mode = FP_RES_POOL2_BEFORE_ACT; parameters as above with the second block's 1x1 packed for its
 *            own width (K = 24, Npad = 32 or 64) and bias_off -> [24] then [Cout].
 *   BLAZECHAIN : in = x, out = y (both dense, 96 channels, H = W = 16; in and out may be the same view), Cmid = number of
 *            blocks (1..16); act = FP_ACT_RELU, res_mode = FP_RES_ADD_BEFORE_ACT (each block's shortcut is its own input);
 *            flags = FP_OPF_SPLIT3: the 1x1 convs run as bf16x6 split MFMAs.  w_off -> Cmid blocks back to back, each
 *            [1280 floats: [9][96] depthwise taps (ky*3 + kx), [96] depthwise bias, [96] 1x1 bias, 224 pad] followed by
 *            three slabs (k = 32 s .. 32 s + 31) of [3 planes][96 output channels][32 k] bf16 (13 824 floats).
 *   SHUFDOWN : in = x (H x W even, Cin = 32 channels), out = the block's output (OH x OW = H/2 x W/2, Cout = 128 = 2 * Cmid dense
 *            channels at out_off, out_ld >= 128), Cmid = 64 (the width of a branch), 3x3 stride 2 pad 1, act = act2 = FP_ACT_SILU,
 *            flags = FP_OPF_SPLIT3 (all three 1x1 convs run as bf16x6 split MFMAs).  One parameter block at w_off (floats; a weight
 *            plane holds two bf16 per float, planes in the order h, m, l of plan.py split3_bf16):
 *              [9][32] branch1 depthwise taps (ky*3 + kx), [32] BN scale, [32] BN bias;
 *              [3 planes][64 co][32 k] branch1 1x1;  [64] BN scale, [64] BN bias;
 *              [2 rounds][3 planes][32 g][32 k] branch2 first 1x1 (round r = output channels 32 r .. 32 r + 31);  [64] scale, [64] bias;
 *              [9][64] branch2 depthwise taps, [64] BN scale, [64] BN bias;
 *              [2 rounds][3 planes][64 co][32 g] branch2 second 1x1 (round r = input channels 32 r ..);  [64] scale, [64] bias.
 *            out[2 c] = branch1[c], out[2 c + 1] = branch2[c].
 *   SHUFUNIT : in = x and out = the block's output, both H x W x 128 dense channels (distinct buffers: tiles read their neighbours'
 *            pixels), Cin = Cout = 128, Cmid = 64, 3x3 stride 1 pad 1, act = act2 = FP_ACT_SILU, flags = FP_OPF_SPLIT3.  Parameter
 *            block at w_off: [2 rounds][3 planes][2 slabs][32 g][32 k] first 1x1 of branch2 (on channels 64 .. 127 of x);  [64] scale,
 *            [64] bias;  [9][64] depthwise taps, [64] BN scale, [64] BN bias;  [2 rounds][3 planes][64 co][32 g] second 1x1;  [64] scale,
 *            [64] bias.  out[2 c] = x[c] (c < 64), out[2 c + 1] = branch2[c].
 *   YSTEM2 : in = a (stem_2a's output: H x W even, Cin = 16 channels), res_* = the pooled stem_1 map (res_H x res_W = OH x OW = H/2 x W/2,
 *            res_C = 32 channels), out = stem_3's output (Cout = 32), 3x3 stride 2 pad 1, act = act2 = FP_ACT_SILU, flags = FP_OPF_SPLIT3.
 *            Parameter block at w_off: [5 slabs][3 planes][32 co][32 k] stem_2b with k = (ky*3 + kx)*16 + c (zero for k >= 144);
 *            [32] scale, [32] bias;  [2 slabs][3 planes][32 co][32 k] stem_3 (k: stem_2b's 32 channels, then the pooled map's);  [32] scale,
 *            [32] bias (scale = 1 where the BatchNorm is folded into the conv).
 *   EMBED_HEAD : in = an NHWC map (H x W x Cin, any in_ld / in_ns), OH = OW = 1, out = [N][Cout] rows (out_ns per image, out_cmul 1),
 *            KH = KW = stride = 1, no padding, act = FP_ACT_NONE, res_mode = FP_RES_NONE.  w_off -> [Cout][Cin] fp32 Linear weight
 *            (row-major, torch's [out, in]); scale_off / bias_off -> [Cout] affine (-1: 1 / 0); flags: FP_OPF_OUT_L2 or 0.
 *            fp32 arithmetic: the mean sums the pixels in order and divides by H * W; each image's result does not depend on the
 *            batch.  Cin <= 2048, Cout <= 1024.
 *   POOL_LRN : in = an NHWC map, out = OH x OW x Cin (Cout = Cin), KH x KW max pool (KH, KW in 1 .. 7), stride, pad_t /
 *            pad_l, -inf outside the map (OH / OW as the caller computed them, Caffe's ceil mode included), then Caffe's / OpenCV's
 *            LRN ACROSS_CHANNELS on the pooled values: y_c = x_c * (k + alpha / n * sum_{|j - c| <= n / 2} x_j^2)^-beta with
 *            n = res_C (odd, 1 .. 15) and the sum running over the channel group of c only: groups of Cmid channels
 *            [g Cmid, (g + 1) Cmid), channels outside the group count as zero (two networks' maps side by side in one tensor
 *            never mix).  Cmid = 0: no LRN (plain max pool).  w_off -> [4] floats: alpha, beta, k, unused (-1 when Cmid = 0).
 *            Cin, Cmid, in_ld, out_ld, offsets and image strides multiples of 4, Cin % Cmid == 0, out_cmul = 1, act = FP_ACT_NONE,
 *            res_mode = FP_RES_NONE.  fp32: the sum of squares in channel order j = c - n/2 .. c + n/2, pow from the device math
 *            library (powf).
 *   CLS_HEAD : in = one row of Cin floats per image at (image n, pixel 0) of the input view (H = W = 1, or a map's first
 *            pixel), OH = OW = 1, out = [N][Cout] probabilities (out_ns per image, out_cmul 1), KH = KW = stride = 1.  w_off ->
 *            [Cout][Cin] fp32 weight (torch's [out, in]), bias_off -> [Cout] (-1: none).  softmax: p_c = exp(z_c - max z) / sum.
 *            res_off >= 0: the logits z are written there too (res_ns per image, res_ld ignored).  Cin % 4 == 0, Cin <= 4096,
 *            Cout <= 64, act = FP_ACT_NONE, res_mode = FP_RES_NONE.  One wave per image, fp32; a row does not depend on the batch.
 * ABI history: 1 = round-1 ops; 2 = fp_ext / *_U8 ops (never shipped in a VERDICT-ed tree); 3 = fp_op.flags, row-padded
 * views; 4 = fp_op.Cmid / reserved0, FP_OP_DWBLOCK, FP_OP_BLAZEPAIR; 5 = FP_OPF_SPLIT3; 6 = FP_OP_BLAZECHAIN; 7 = FP_OPF_IN_UP2; 8 = FP_OP_BLAZEPAIR with stride 2; 9 = FP_OPF_OUT_DW, fp_debug_reload_env; 10 = FP_OP_SHUFDOWN, FP_OP_SHUFUNIT, FP_OP_YSTEM2; 11 = FP_OPF_SPLIT3 on FP_OP_STEM_U8;
 * 12 = device Huffman decoding of sequential JPEG scans (fp_jpeg_scan, fp_jpeg_scan_prepare, fp_jpeg_entropy_decode_device, section 7);
 * 13 = baseline JPEG encoding of crop batches (fp_jpeg_enc_item, fp_jpeg_encode_device, section 8);
 * 14 = ragged batches: frames of different sizes in one packed buffer (fp_frame_desc, fp_resize_ragged,
 * fp_dets_to_crops_ragged, section 2).
 */

/* Validates every op against arena_floats / weight_floats, then launches them in order. */
int fp_plan_run(const fp_op* ops /*host*/, int n_ops,
                const float* weights, size_t weight_floats,
                float* arena, size_t arena_floats,
                void* stream);

/*
 * External buffers of a plan: device memory that is not part of the arena (the u8 frames a *_U8 op reads, its tap
 * tables and LUT).  fp_plan_run_ext = fp_plan_run with such buffers; ops that need them fail with FP_ERR_INVALID_ARG
 * under plain fp_plan_run.
 */
typedef struct fp_ext {
  const void* ptr;   /* device pointer */
  size_t bytes;      /* extent the library may read */
} fp_ext;

int fp_plan_run_ext(const fp_op* ops /*host*/, int n_ops,
                    const float* weights, size_t weight_floats,
                    float* arena, size_t arena_floats,
                    const fp_ext* ext /*host*/, int n_ext, void* stream);

/*
 * Validation only (no GPU needed): the checks fp_plan_run makes before its first launch, which end with each op's
 * launcher deciding, without launching, whether it takes the op.  A plan that validates is refused at launch only for
 * an fp_ext buffer it is given at run time (the frame, tap-table and LUT sizes of FP_OP_STEM_U8 / FP_OP_YSTEM_U8) or a
 * HIP error.
 */
int fp_plan_validate(const fp_op* ops /*host*/, int n_ops, size_t weight_floats, size_t arena_floats);

/*
 * Per-op timing for measurement (bench.py): fp_plan_run with a hipEvent pair recorded ON `stream`
 * around every op whose op_mask[i] != 0.  A timer owns n_ops event pairs (host objects, no device
 * memory); fp_timer_accumulate waits for the events of the last timed run of that timer and adds
 * each op's elapsed milliseconds into ms_accum[i] (host array).  Use one timer per in-flight run.
 */
int fp_timer_create(int n_ops, void** out_timer);
void fp_timer_destroy(void* timer);
int fp_plan_run_timed(const fp_op* ops /*host*/, int n_ops,
                      const float* weights, size_t weight_floats,
                      float* arena, size_t arena_floats,
                      void* stream, void* timer, const unsigned char* op_mask /*host, n_ops*/);
int fp_plan_run_timed_ext(const fp_op* ops /*host*/, int n_ops,
                          const float* weights, size_t weight_floats,
                          float* arena, size_t arena_floats,
                          const fp_ext* ext /*host*/, int n_ext,
                          void* stream, void* timer, const unsigned char* op_mask /*host, n_ops*/);
int fp_timer_accumulate(void* timer, float* ms_accum /*host, n_ops*/, int n_ops);
/* Name of the HIP kernel instance an op launches (as rocprofv3's kernel trace shows it), the launcher's own choice; "?" for
 * an op its launcher refuses.  Thread-local buffer. */
const char* fp_op_kernel_name(const fp_op* op /*host*/);

/* ------------------------------------------------------------------------- */
/* 2. Image front end                                                          */
/* ------------------------------------------------------------------------- */

/*
 * Bilinear u8 resize of a source rectangle into a destination rectangle of an
 * fp32 NHWC canvas, then per-value LUT normalisation; pixels of the canvas
 * outside the destination rectangle are set to lut[pad_value].
 * Replaces: pad_resize_image (fde/modules/utils/image.py:31-59) + BGR->RGB
 * (fde/modules/blazeface/model.py:75, y5/__init__.py:15) + normalisation
 * (blazeface.py:248-250  x/127.5-1 ; y5/__init__.py:19-20  x/255 ;
 *  mobile_facenet/utils.py:13  (x-127.5)/127.5) and the per-face crop + resize of
 * extract_faces_from_dataset.py:289-303.  Resize arithmetic is OpenCV's
 * INTER_LINEAR u8 fixed-point scheme (11-bit coefficients); cv2 is absent in
 * the build container so this boundary is "parity unpinned" (DESIGN.md).
 *
 * One item = one canvas: item i resizes its source rectangle of frame src_image into the
 * destination rectangle (dx,dy,dw,dh) of canvas i (letterbox: the padded sub-rectangle; face crop:
 * the whole 112x112 canvas).  Items live in DEVICE memory (they may be produced by
 * fp_dets_to_crops); source rectangles are clamped to the frame inside the kernel.
 */
typedef struct fp_resize_item {
  int32_t src_image;   /* index into frames */
  int32_t sx, sy, sw, sh; /* source rectangle (pixels, inside the frame) */
  int32_t dx, dy, dw, dh; /* destination rectangle inside the canvas */
} fp_resize_item;

int fp_resize_normalize(const uint8_t* frames, int n_frames, int frame_h, int frame_w, /* [n,H,W,3] u8 */
                        const fp_resize_item* items /*device*/, int n_items,
                        float* canvas, int canvas_h, int canvas_w, int canvas_c /* >=3, extra channels zeroed */,
                        const float* lut256 /*device, 256 floats*/, int pad_value, int swap_rb,
                        void* stream);

/*
 * Tap tables of ONE resize geometry, for the network stems that read u8 frames themselves (FP_OP_YSTEM_U8,
 * FP_OP_STEM_U8): source rectangle (sx, sy, sw, sh) of a frame_h x frame_w frame -> destination rectangle
 * (dx, dy, dw, dh) of a canvas_h x canvas_w canvas, everything else pad_value.  Same arithmetic as
 * fp_resize_normalize (pad_resize_image, fde/modules/utils/image.py:31-59), evaluated once per column and row:
 * tables = (canvas_w + canvas_h + 2) entries of 2 int32 (layout: csrc/letterbox.h); frame_h, canvas_h <= 65535,
 * frame_w, canvas_w <= 32767.  The last entry records (frame_h, frame_w, canvas_h, canvas_w): a *_U8 op that is handed
 * tables built for another geometry writes NOTHING (a device-side check per workgroup; the host cannot read the device
 * buffer without a sync).  Trust boundary: the library checks the BYTE SIZES of the three external buffers and that
 * geometry record; that the frames buffer really holds N frames of res_H x res_W x 3 bytes is the caller's contract.
 */
int fp_letterbox_tables(int frame_h, int frame_w, int canvas_h, int canvas_w, int sx, int sy, int sw, int sh,
                        int dx, int dy, int dw, int dh, int pad_value, int swap_rb, int32_t* tables /*device*/,
                        void* stream);

/*
 * Detections -> face crop rectangles on device.  fmt 0: BlazeFace rows (ymin,xmin,ymax,xmax,...,score@16)
 * normalised to the model input — column reorder (fde/modules/blazeface/model.py:70) +
 * get_dets_bboxes_confs_lmarks_areas (fde/modules/utils/inference.py:11-58).  fmt 1: YOLOv5-face rows
 * (x1,y1,x2,y2,conf@4) in input pixels — get_bboxes_confs_areas (fde/modules/yolov5_face/onnx/onnx_utils.py:313-340).
 * Then scale_coords/clip/round (fde/modules/utils/image.py:62-99) and the crop arithmetic of
 * fde/face_extraction/extract_faces_from_dataset.py:289-303 (int(), offsets, clamp).  gain/pad are
 * scale_coords' values computed by the caller.  items[max_faces], face_info[max_faces][7] =
 * (frame, x1, y1, x2, y2 in original-frame pixels (rounded), conf, bbox area: fmt 0 the FRACTION of the model input
 * as inference.py:40-46 reports it (filter 100*(area/total) > thr); fmt 1 the PERCENT (100*area)/total as
 * onnx_utils.py:329-332 computes, compares and returns it), n_faces[1] = total found (the caller
 * must check n_faces <= max_faces).  Faces are ordered by (frame, detection).
 */
int fp_dets_to_crops(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt,
                     int in_w, int in_h, int orig_w, int orig_h, float det_thres, float area_thres,
                     float gain, float pad_x, float pad_y, int off_tx, int off_ty, int off_bx, int off_by,
                     int dst_w, int dst_h, int max_faces,
                     fp_resize_item* items, float* face_info, int32_t* n_faces, void* stream);

/*
 * Ragged batches (ABI 14): frames of DIFFERENT sizes (u8 BGR, HWC, rows packed) back to back in one buffer, each described
 * by an fp_frame_desc in device memory.  frame i = frames[descs[i].off ...], descs[i].h x descs[i].w pixels.  The frames
 * the reference's dataset driver reads (one photo per media item, fde/face_extraction/extract_faces_from_dataset.py:380-405)
 * are of any size; these entry points take a whole batch of them in one launch.
 */
typedef struct fp_frame_desc {
  int64_t off;        /* byte offset of the frame's pixel (0, 0) in the packed buffer */
  int32_t h, w;       /* the frame's size (pixels) */
} fp_frame_desc;

#define FP_FRAME_MIN_W 3        /* a frame row holds the 8-byte tap window of the resize (csrc/letterbox.h) */
#define FP_FRAME_MAX_W 32767
#define FP_FRAME_MAX_H 65535
#define FP_RAGGED_U8 0          /* fp_resize_ragged output: u8 canvas, 3 channels in frame order, no LUT, no R/B swap */
#define FP_RAGGED_F32_LUT 1     /* fp_resize_ragged output: fp32 canvas, 4 channels, lut256[value] (+ swap_rb), 4th = 0 */

/*
 * fp_resize_normalize over a ragged batch: item i resizes its source rectangle of frame items[i].src_image (an index into
 * descs) into the destination rectangle of canvas i, pad_value elsewhere.  Every output value equals what
 * fp_resize_normalize computes on the same source rectangle of the same frame (FP_RAGGED_F32_LUT: bit for bit; FP_RAGGED_U8:
 * the u8 value before the LUT).  One workgroup per (item, band of canvas rows): the work of an item depends on its canvas,
 * not on its frame.  canvas: [n_items][canvas_h][canvas_w][canvas_c], canvas_c = 3 (u8, lut256 unused, swap_rb = 0) or
 * 4 (fp32, 16-byte aligned, lut256 = 256 device floats); canvas_w <= 4096, canvas_h <= 65535.
 * Refusals before any launch: NULL pointers, sizes out of range, a canvas_c or swap_rb the mode does not take, frames_bytes
 * < 9 (FP_ERR_INVALID_ARG); a misaligned fp32 canvas (FP_ERR_ALIGNMENT).
 * Trust boundary: descs and items are device memory the host does not read.  The kernel clamps each source rectangle to its
 * frame and writes pad_value for an item whose descriptor is outside [FP_FRAME_MIN_W, FP_FRAME_MAX_W] x [1, FP_FRAME_MAX_H]
 * or whose frame does not end inside frames_bytes, so it never loads outside the buffer; that the descriptors describe the
 * frames the caller meant (no overlap, the right sizes) is the caller's contract.
 */
int fp_resize_ragged(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs /*device*/, int n_frames,
                     const fp_resize_item* items /*device*/, int n_items, void* canvas, int canvas_h, int canvas_w,
                     int canvas_c, int mode, const float* lut256 /*device, 256 floats; FP_RAGGED_F32_LUT only*/,
                     int pad_value, int swap_rb, void* stream);

/*
 * fp_dets_to_crops over a ragged batch: frame f's orig_w / orig_h come from descs[f] (w, h) and its scale_coords values
 * from geom[f] = (gain, pad_x, pad_y) fp32 (device, B x 3; the caller computes them per frame as for fp_dets_to_crops).
 * Same kernel body, same rows, same order.  A frame whose descriptor has h or w <= 0 or whose gain is not > 0 contributes
 * no faces.  Refusals as fp_dets_to_crops (FP_ERR_INVALID_ARG before any launch).
 */
int fp_dets_to_crops_ragged(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt,
                            int in_w, int in_h, const fp_frame_desc* descs /*device, B*/, const float* geom /*device, B x 3*/,
                            float det_thres, float area_thres, int off_tx, int off_ty, int off_bx, int off_by,
                            int dst_w, int dst_h, int max_faces,
                            fp_resize_item* items, float* face_info, int32_t* n_faces, void* stream);

/*
 * Crop rectangles of the age / gender nets (Levi-Hassner) from face rows: OpenCVFaceDetAgeGenderModel.__call__ of the
 * reference (modules/opencv2_dnn/model.py): box = round-half-to-even(info[1..4]) -> int, then
 *   x0 = max(0, x1 - pad), x_end = min(x2 + pad, W - 1), y0 = max(0, y1 - pad), y_end = min(y2 + pad, H - 1)
 * (the reference's exclusive ends at W - 1 / H - 1, kept), the crop frame[y0:y_end, x0:x_end] resized to dst_w x dst_h
 * (cv2 INTER_LINEAR: fp_resize_normalize / fp_resize_ragged with the item written here).
 * info: [n][info_floats] rows (frame index, x1, y1, x2, y2, ...), e.g. fp_dets_to_crops' info (info_floats = 7).
 * Frame sizes: descs (device, ragged batch, indexed by the row's frame) or, with descs = NULL, frame_w x frame_h for every
 * row.  items[i] = {frame, x0, y0, x_end - x0, y_end - y0, 0, 0, dst_w, dst_h}; a crop with zero width or height (the
 * reference's cv2.resize would raise on it) gets sw = sh = dw = dh = 0: the resize writes pad colour and the caller marks
 * the face's outputs undefined (AgeGenderNet: NaN probabilities).  A row whose frame index is outside [0, n_frames) is
 * such an empty item too.  Refusals before any launch: NULL pointers, n < 0, info_floats < 5, pad < 0, dst sizes < 1
 * (FP_ERR_INVALID_ARG).  fp_attr_crop_items_emulate: the same arithmetic on host arrays (descs host too).
 */
int fp_attr_crop_items(const float* info /*device*/, int n, int info_floats, const fp_frame_desc* descs /*device or NULL*/,
                       int n_frames, int frame_w, int frame_h, int pad, int dst_w, int dst_h,
                       fp_resize_item* items /*device*/, void* stream);
int fp_attr_crop_items_emulate(const float* info /*host*/, int n, int info_floats, const fp_frame_desc* descs /*host or NULL*/,
                               int n_frames, int frame_w, int frame_h, int pad, int dst_w, int dst_h,
                               fp_resize_item* items /*host*/);

/* ------------------------------------------------------------------------- */
/* 3. BlazeFace post-processing                                                */
/* ------------------------------------------------------------------------- */

/*
 * _tensors_to_detections + _decode_boxes (blazeface.py:321-402): clamp +-clip,
 * sigmoid, score >= min_score_thresh, anchor decode.  Candidates are compacted
 * per image in anchor order into cand[B][num_anchors][17] / cand_count[B].
 */
int fp_blaze_decode(const float* raw_boxes /*[B,A,16]*/, const float* raw_scores /*[B,A]*/,
                    const float* anchors /*[A,4]*/, int B, int A,
                    float x_scale, float y_scale, float w_scale, float h_scale,
                    float score_clip, float min_score_thresh,
                    float* cand /*[B,A,17]*/, int32_t* cand_count /*[B]*/, void* stream);

/*
 * _weighted_non_max_suppression (blazeface.py:404-458) + overlap_similarity
 * (:463-526) for a batch: one workgroup per image.  dets [B][max_in][17] with
 * counts[B]; out [B][max_in][17], out_count[B]; member_of [B][max_in] (optional,
 * may be NULL) receives, per INPUT detection, the index of the output cluster it
 * was blended into (the bit-exact parity object).  Ties in score are ordered by
 * input index (stable).  A box whose self-IoU is not > thr (degenerate, SURVEY F8:
 * the reference never terminates) is emitted alone and removed.
 */
int fp_blaze_weighted_nms(const float* dets, const int32_t* counts, int B, int max_in,
                          float iou_thresh, float* out, int32_t* out_count, int32_t* member_of,
                          void* stream);

/* ------------------------------------------------------------------------- */
/* 4. YOLOv5-face post-processing                                              */
/* ------------------------------------------------------------------------- */

/*
 * Detect.forward inference decode (y5/models/yolo.py:62-108): heads are the raw
 * 1x1-conv outputs in NHWC [B,ny,nx,na*16]; out is [B, sum(na*ny*nx), 16] in the
 * reference's (level, anchor, y, x) order.
 */
int fp_yolo_decode(const float* head, int B, int ny, int nx, int na,
                   float stride, const float* anchors_px /*host [na][2]*/,
                   float* out, int64_t out_image_stride /*floats*/, int64_t out_row_offset /*rows*/,
                   void* stream);

/*
 * non_max_suppression_face (y5/utils/general.py:370-453), nc = 1: obj > conf,
 * conf = obj*cls > conf, xywh->xyxy, torchvision.ops.nms(iou) semantics
 * (greedy, IoU = inter/(a+b-inter), suppress IoU > thr, score-descending, ties by index).
 * pred [B][n_rows][16]; out [B][max_out][16] rows = (x1,y1,x2,y2,conf,lmk[10],cls);
 * out_count[B]; keep_idx [B][max_out] = row index into pred (bit-exact parity object);
 * overflow[B] is set to 1 when an image had more than max_cand candidates
 * (the host raises; the reference has no cap).
 */
int fp_yolo_nms(const float* pred, int B, int n_rows, float conf_thres, float iou_thres,
                int max_cand, int max_out,
                float* out, int32_t* out_count, int32_t* keep_idx, int32_t* overflow,
                void* scratch, size_t scratch_bytes, void* stream);
size_t fp_yolo_nms_scratch_bytes(int B, int max_cand);

/*
 * w_non_max_suppression (fde/modules/yolov5_face/onnx/onnx_utils.py:107-163), num_classes=1:
 * obj >= conf, +1-pixel IoU (:76-104), keep iou < nms_thres.  out rows = (x1,y1,x2,y2,obj,cls_conf,cls).
 */
int fp_yolo_w_nms(const float* pred, int B, int n_rows, float conf_thres, float nms_thres,
                  int max_cand, int max_out,
                  float* out /*[B][max_out][7]*/, int32_t* out_count, int32_t* keep_idx, int32_t* overflow,
                  void* scratch, size_t scratch_bytes, void* stream);

/*
 * Augmented inference (y5/models/yolo.py:156-175, scale_img of y5/utils/torch_utils.py:230-240): the network runs on the
 * input, on the input mirrored left-right and scaled by 0.83, and on the input scaled by 0.67; the rows of the three runs,
 * mapped back to the input's pixels, go through one NMS.  Additions of ABI 15, csrc/tta.hip.
 *
 * fp_tta_views fills the inputs of the two scaled views in ONE launch.  canvas [N][H][W][4] fp32 is the view-1 input (channel
 * 3 is zero and is not read for its value); out_a / out_b are [N][padded_h][padded_w][4] of views[0] / views[1].  Inside the
 * content rectangle (content_h x content_w, top left) a pixel is F.interpolate(mode="bilinear", align_corners=False) of the
 * canvas -- of the canvas mirrored left-right when flip is 1 --: scale = (float)in / content, src = max(fmaf(scale, dst + 0.5f,
 * -0.5f), 0) (one fma, as torch's CPU build evaluates it), i0 = (int)src, i1 = min(i0 + 1, in - 1), l = src - i0, value = (a (1 - lx) + b lx)(1 - ly) + (c (1 - lx) + d lx)
 * ly in that order, no fma.  Everywhere else channels 0..2 are pad_value (the reference pads with 0.447); channel 3 is 0 in every
 * pixel.  Every float of both outputs is written, nothing else is.  Refusals before any launch: a NULL pointer, N < 0 or >
 * 65535, a content size outside 1 .. min(padded, canvas) per axis, flip outside 0 / 1, 2^31 pixels or more in an image
 * (FP_ERR_INVALID_ARG); a pointer not 16-byte aligned (FP_ERR_ALIGNMENT).  N == 0: FP_OK, nothing launched.  out_a / out_b must
 * not overlap the canvas.
 *
 * fp_yolo_decode_view = fp_yolo_decode followed, in the same lane, by the view's un-mapping in the reference's order:
 * columns 0..3 divided by si (an fp32 IEEE division by the float nearest the ratio, as torch's `/= si`; not a multiplication by
 * a reciprocal: the rows feed NMS threshold decisions), then for flip = 1 cx = (float)img_w - cx.  lm_mode 0 leaves columns
 * 5..14 as decoded -- the reference's behaviour: its landmarks of a scaled view stay in that view's pixels, unmirrored.
 * lm_mode 1 divides every landmark coordinate by si and, for flip = 1, sets x = (float)img_w - x and exchanges points 0 <-> 1
 * (eyes) and 3 <-> 4 (mouth corners), so that columns 5..14 mean the same in every row.  With si = 1, flip = 0 the rows equal
 * fp_yolo_decode's bit for bit.  Refusals: fp_yolo_decode's, and si <= 0 or NaN, flip / lm_mode outside 0 / 1, img_w <= 0, a
 * negative stride or offset (FP_ERR_INVALID_ARG); out not 16-byte aligned or out_image_stride % 4 (FP_ERR_ALIGNMENT).
 */
typedef struct fp_tta_view {
  int32_t content_h, content_w;   /* (int)(h * ratio), (int)(w * ratio) */
  int32_t padded_h, padded_w;     /* ceil(x * ratio / 32) * 32: the view's network input */
  int32_t flip;                   /* 1: the view looks at the canvas mirrored left-right */
  int32_t reserved;
} fp_tta_view;

int fp_tta_views(const float* canvas, int N, int H, int W, const fp_tta_view* views /*host [2]*/,
                 float* out_a, float* out_b, float pad_value, void* stream);

int fp_yolo_decode_view(const float* head, int B, int ny, int nx, int na,
                        float stride, const float* anchors_px /*host [na][2]*/,
                        float* out, int64_t out_image_stride /*floats*/, int64_t out_row_offset /*rows*/,
                        float si, int flip, int img_w, int lm_mode, void* stream);

/* ------------------------------------------------------------------------- */
/* 5. Similarity filter                                                        */
/* ------------------------------------------------------------------------- */

/* inv_norm[m] = 1/||x[m,:]||  (cosine: extract_and_label_faces_from_dataset.py:106) */
int fp_row_inv_norm(const float* x, int64_t M, int D, float* inv_norm, void* stream);

/*
 * Cosine filter: for each gallery row g: best = max_j <g, r_j> * ginv[g] * rinv[j],
 * arg = the smallest j attaining it, keep = best >= tau.  S is never materialised.
 * packed is a caller-provided [M] uint64 scratch.
 */
int fp_cosine_filter(const float* G, const float* ginv, int64_t M,
                     const float* R, const float* rinv, int Nr, int D, float tau,
                     float* best, int32_t* arg, uint8_t* keep,
                     uint64_t* packed, void* stream);

/*
 * The same filter with S = G R^T on the bf16 matrix cores, fp32-equivalent split arithmetic (ABI 5, csrc/split.h): the
 * reference rows are split ONCE into three bf16 planes (fp_split3_rows: out holds fp_split3_bytes(Nr, D) bytes, layout
 * [D / 32][3][round_up(Nr, 128)][32] bf16, zero rows in the padding; D a multiple of 32), then every gallery batch runs
 * fp_cosine_filter_x6 against them.  Same results within fp32 rounding (best: 1e-6; arg: equal unless two scores tie within
 * it), 2x the rate of the fp32-MFMA kernel at 1 M x 10 k x 512.  rinv must be 16-byte aligned.
 * fp_cosine_filter_x6_tile_rows (host only; added within ABI 15: a function only): the gallery rows of a workgroup's tile that
 * fp_cosine_filter_x6 chooses for M x Nr -- 256 when ceil(M / 256) * ceil(Nr / 128) >= 2048, else 128; 0 for M < 0, Nr <= 0 and
 * a grid of 2^31 workgroups or more, which the launcher refuses.  The launcher asks this function; results do not depend on it.
 */
int fp_cosine_filter_x6_tile_rows(int64_t M, int Nr);
size_t fp_split3_bytes(int Nr, int D);
int fp_split3_rows(const float* R, int Nr, int D, void* out, void* stream);
int fp_cosine_filter_x6(const float* G, const float* ginv, int64_t M,
                        const void* R3, const float* rinv, int Nr, int D, float tau,
                        float* best, int32_t* arg, uint8_t* keep,
                        uint64_t* packed, void* stream);

/*
 * Top-k cosine search against an enrolled gallery (build-defined; the reference has no counterpart).  S = Q G^T with the
 * arithmetic of fp_cosine_filter_x6: G3 = fp_split3_rows(G) (D a multiple of 32), score[m][n] = <Q[m], G[n]> * qinv[m] * ginv[n].
 * Per query row the k largest scores in descending order and their gallery rows: scores [M][k] fp32, idx [M][k] int32; on
 * equal scores the lower gallery index first.  A gallery row with ginv == 0 is excluded (masking: padding, removed rows);
 * slots beyond the number of valid rows hold -inf / -1.  S is never materialised: a workgroup keeps a running top-k per row
 * over a contiguous range of 128-column chunks (one of n_splits ranges) and a second kernel merges the n_splits lists of a
 * row.  n_splits == 0: chosen from M and the number of CUs; a positive value is honoured, clamped to the number of chunks.
 * The result is deterministic and the same for every n_splits.  workspace: fp_cosine_topk_workspace(M, N, k, n_splits) bytes
 * of device memory, 8-byte aligned (M * n_splits * k keys; for n_splits == 0 a bound on what the launcher may choose; 0 for
 * arguments fp_cosine_topk_x6 refuses; it grows with M, k and n_splits).  1 <= k <= FP_TOPK_MAX.  Refusals: a NULL pointer, k out of range,
 * N <= 0, n_splits < 0 or a workspace that is too small: FP_ERR_INVALID_ARG; D % 32 or Q / G3 / ginv not 16-byte aligned:
 * FP_ERR_ALIGNMENT.  M == 0: FP_OK, nothing launched.
 */
#define FP_TOPK_MAX 16
size_t fp_cosine_topk_workspace(int64_t M, int N, int k, int n_splits);
int fp_cosine_topk_x6(const float* Q, const float* qinv, int64_t M, const void* G3, const float* ginv, int N, int D, int k,
                      int n_splits, float* scores, int32_t* idx, void* workspace, size_t ws_bytes, void* stream);

/*
 * Compressed gallery (build-defined, DESIGN S7 "Compressed gallery"): an int8 coarse search over everything and an exact
 * rerank of a short candidate list.  Additions to ABI 14.
 *
 * fp_quantize_rows_i8: X [N][D] fp32, D a multiple of 64 and <= FP_QUANT_MAX_D.  Per row: amax = max |x|; a row with amax == 0
 * or a non-finite value is dead (q = 0, scale = 0); else r = 127 / amax, q = int8(rint(x * r)) (one fp32 multiply, round half
 * to even, clamped to +-127), scale = amax / 127.  q8 holds fp_quant_i8_bytes(N, D) bytes in the layout
 * [D / 64][round_up(N, 128)][64] int8 with zero rows in the padding, scale [N] fp32.  16-byte aligned X and q8.
 *
 * fp_cosine_topk_i8: per query row the `pool` best gallery rows by coarse score.  Q8 = the codes of the M query rows, G8
 * those of the N gallery rows (both from fp_quantize_rows_i8).  c[m][n] = float(dot_i32(Q8[m], G8[n])) * w[n] in one rounding
 * (|dot| <= 1024 * 127^2 < 2^24); rows are ordered by c, higher first, then the LOWER index; the score written is c * u[m].
 * w[n] == 0 masks gallery row n (dead, removed); a query row whose u is not a positive finite number is dead: all its slots
 * are -inf / -1, as are the slots beyond the live rows.  scores [M][pool] fp32, idx [M][pool] int32.  n_splits and the
 * workspace as fp_cosine_topk_x6 (fp_cosine_topk_i8_workspace bytes, 8-byte aligned); the result is the same for every
 * n_splits.  1 <= pool <= FP_COARSE_MAX.  w must be 16-byte aligned.  Galleries of 65 536 rows and more are searched in several
 * passes over growing prefixes of the rows, each handing the next a lower bound per query through `scores` (which therefore
 * holds intermediate values until the call's last kernel has run); the result is that of one pass.
 *
 * fp_rerank_topk: the exact scores of the candidates.  cand [M][pool] int32 gallery rows; -1 (or any index outside 0 .. N-1)
 * and rows with ginv == 0 are skipped; a list is a SET of rows: an index it names more than once counts once (its first
 * entry), so no gallery row comes back twice.  score = dot_fp32(Q[m], row) * qinv[m] * ginv[cand], the dot
 * summed in a fixed order (two runs agree bit for bit); the k best by (score descending, index ascending) to scores [M][k],
 * idx [M][k] (gallery rows), -inf / -1 behind them.  The fp32 rows come from G [N][D] (rows == NULL) or, for a gallery whose
 * rows stay on the host, from the compact block rows [M][pool][D] gathered in the order of cand (G == NULL); exactly one of
 * the two is given and both modes compute the same bits.  1 <= k <= min(pool, FP_TOPK_MAX), pool <= FP_COARSE_MAX.
 *
 * Refusals, before any launch: a NULL pointer, D > FP_QUANT_MAX_D, pool or k out of range, k > pool, N <= 0, n_splits < 0, a
 * workspace that is too small: FP_ERR_INVALID_ARG; D % 64 or a misaligned pointer: FP_ERR_ALIGNMENT.  M == 0: FP_OK,
 * nothing launched.
 */
#define FP_COARSE_MAX 64
#define FP_QUANT_MAX_D 1024
size_t fp_quant_i8_bytes(int N, int D);
int fp_quantize_rows_i8(const float* X, int N, int D, void* q8, float* scale, void* stream);
size_t fp_cosine_topk_i8_workspace(int64_t M, int N, int pool, int n_splits);
int fp_cosine_topk_i8(const void* Q8, const float* u, int64_t M, const void* G8, const float* w, int N, int D, int pool,
                      int n_splits, float* scores, int32_t* idx, void* workspace, size_t ws_bytes, void* stream);
int fp_rerank_topk(const float* Q, const float* qinv, int64_t M, int D, const int32_t* cand, int pool, const float* G,
                   const float* rows, const float* ginv, int N, int k, float* scores, int32_t* idx, void* stream);

/*
 * Identity of every row of a top-k result (one thread per row).  labels [N] int32: the label of every gallery row.  A
 * candidate counts when its index is >= 0 and its score >= tau.  mode 0 (top-1): the label of the best candidate if it
 * counts, else -1.  mode 1 (majority): the label with the most counting candidates; ties go to the larger summed score, then
 * to the smaller label id; -1 when none counts.  out_score: the best score among the winning label's candidates, or the row's
 * best score when the label is -1; out_votes: the winner's vote count (0 for -1).
 */
int fp_topk_vote(const float* scores, const int32_t* idx, int64_t M, int k, const int32_t* labels, int N, float tau, int mode,
                 int32_t* out_label, float* out_score, int32_t* out_votes, void* stream);

/*
 * Cosine DBSCAN: group the N rows of X by identity without labels (build-defined; the reference has no counterpart).  X3 =
 * fp_split3_rows(X) (D a multiple of 32), xinv = fp_row_inv_norm(X).  Semantics, on which the labels equal scikit-learn's
 * DBSCAN(metric="precomputed") on the same edge set:
 *   - a row is live when its xinv is finite and non-zero; a dead row has degree 0, core 0, label -1 and no neighbours;
 *   - for live i < j: i ~ j iff <X[i], X[j]> * xinv[i] * xinv[j] >= tau, in the arithmetic of fp_cosine_topk_x6 with row i the
 *     register-split operand and column j from the planes; each unordered pair is evaluated once; NaN compares false;
 *   - degree[i] = 1 + the number of neighbours (the point counts itself), core[i] = degree[i] >= min_samples;
 *   - clusters = connected components of the core points under core-core edges, numbered 0 .. C-1 by their smallest row;
 *   - a live non-core point with a core neighbour (border) takes the smallest cluster number among its core neighbours;
 *     every other non-core point is noise, label -1.  n_clusters[0] = C.
 * Two walks of the upper triangle of S = X X^T (S is never stored; one walk when min_samples <= 2), a lock-free union-find in
 * between, then flatten / rank / label launches.  The result is a function of the edge set only: two runs are bit-identical.
 * degree [N] int32, core [N] uint8, labels [N] int32, n_clusters [1] int32.  ws: fp_cosine_dbscan_workspace(N, min_samples)
 * bytes of device memory, 16-byte aligned (0 for arguments the call refuses; grows with N and min_samples).
 * 1 <= min_samples <= 64, 0 < N < 2^31.  Refusals, before any launch: a NULL pointer, N <= 0, min_samples out of range or a
 * workspace that is too small: FP_ERR_INVALID_ARG; D % 32 or X / X3 / ws not 16-byte aligned: FP_ERR_ALIGNMENT;
 * N >= 2^31, or a triangular work list of 2^31 workgroups or more (N above about 33 million rows): FP_ERR_UNSUPPORTED.
 */
size_t fp_cosine_dbscan_workspace(int64_t N, int min_samples);
int fp_cosine_dbscan_x6(const float* X, const float* xinv, const void* X3, int64_t N, int D, float tau, int min_samples,
                        int32_t* degree, uint8_t* core, int32_t* labels, int32_t* n_clusters, void* ws, size_t ws_bytes,
                        void* stream);

/*
 * Centroid and medoid of C clusters.  order: the member rows sorted by (cluster, row); offsets [C + 1]: cluster c owns
 * order[offsets[c] .. offsets[c + 1]).  centroids [C][D]: the members' normalised rows (X[m] * xinv[m]) summed in that order
 * and renormalised (an empty cluster: zeros); medoid [C]: the member with the largest cosine to the centroid, the lower row
 * on equal scores (-1 for an empty cluster).  One workgroup per cluster, no float atomics: two runs are bit-identical.
 * Any D up to 16000.
 */
int fp_cluster_centroids(const float* X, const float* xinv, const int32_t* order, const int32_t* offsets, int C, int D,
                         float* centroids, int32_t* medoid, void* stream);

/*
 * Pair histogram: score an embedder on N labelled rows (build-defined; the reference has no counterpart).  The cosine scores of
 * ALL pairs i < j of live rows are counted into two histograms of nbins equal bins over [lo, hi): genuine (labels[i] ==
 * labels[j]) and impostor (otherwise).  ROC, TAR at FAR, EER and AUC follow from the 2 x nbins integers on the host.  X3 =
 * fp_split3_rows(X) (D a multiple of 32), xinv = fp_row_inv_norm(X), labels [N] int32.  Semantics:
 *   - a row is live when its xinv is finite and non-zero AND its label is >= 0; a row that is not live takes part in no pair;
 *   - for live i < j: s = <X[i], X[j]> * xinv[i] * xinv[j] in the arithmetic and orientation of fp_cosine_dbscan_x6 (row i the
 *     register-split operand, column j from the planes); each unordered pair is evaluated once, the diagonal never;
 *   - bin: scale = (float)(nbins / ((double)hi - lo)) on the host, t = (s - lo) * scale in fp32 as two separately rounded
 *     operations, b = t < 0 ? 0 : min((int)t, nbins - 1): a score below lo or at or above hi lands in an end bin, so the
 *     counts total the number of live pairs.  A NaN score (overflow only) is counted nowhere;
 *   - the counters are integers: two runs are bit-identical whatever the launch geometry.
 * genuine [nbins], impostor [nbins] int64 on the device: the call zeroes them itself.  Stream-ordered, allocates nothing.
 * ws: fp_pair_histogram_workspace(N) bytes of device memory, 16-byte aligned (the masked inverse norms and the labels, both
 * padded to round_up(N, 128); 0 for N <= 0 or N >= 2^31).  N == 0 and N == 1: FP_OK, all zeros (N == 0 reads no input
 * pointer).  Refusals, before any launch: nbins outside 2 .. FP_PAIRHIST_MAX_BINS, !(lo < hi), lo or hi not finite (or a
 * range so narrow that scale is not), D <= 0 or D % 32, N < 0, a NULL pointer or a workspace that is too small:
 * FP_ERR_INVALID_ARG; X / X3 / ws not 16-byte aligned: FP_ERR_ALIGNMENT; N >= 2^31 or a work list of 2^31 workgroups:
 * FP_ERR_UNSUPPORTED.
 */
#define FP_PAIRHIST_MAX_BINS 1024
size_t fp_pair_histogram_workspace(int64_t N);
int fp_pair_histogram_x6(const float* X, const float* xinv, const void* X3, const int32_t* labels, int64_t N, int D, float lo,
                         float hi, int nbins, int64_t* genuine, int64_t* impostor, void* ws, size_t ws_bytes, void* stream);

/*
 * get_ref_mean_vec_and_thres_from_imgs (sff/filter_faces_using_reference.py:71-100):
 * mean over the R reference rows, thres = max_i ||mean - f_i||_2.  out_mean [D], out_thres [1].
 */
int fp_l2_mean_thres(const float* ref, int R, int D, float* out_mean, float* out_thres, void* stream);

/* filter loop (sff/filter_faces_using_reference.py:183-197): dist = ||e - mean||_2 ; keep = dist <= thres. */
int fp_l2_filter(const float* E, int64_t M, int D, const float* mean, const float* thres /*device [1]*/,
                 float* dist, uint8_t* keep, void* stream);

/*
 * TF-style preprocess of the FaceNet filter (similar_face_filtering/filter_faces_using_reference.py:60-68):
 * frames [n][H][W][3] u8 RGB -> [0,1] -> tf.image.resize bilinear (half-pixel centres, no antialias) to
 * (out_h, out_w) -> per_image_standardization (x - mean)/max(std, 1/sqrt(out_h*out_w*3)).  out [n][out_h][out_w][3]
 * fp32; stats_scratch = 2*n doubles of device scratch.  The formula is pinned by the reference's own test
 * (sff/tests/base/test_similar_faces_filter.py:19-27); the resize is restated (TF absent offline).
 */
int fp_resize_standardize(const uint8_t* frames, int n, int H, int W, float* out, int out_h, int out_w,
                          double* stats_scratch, void* stream);

/*
 * Face crops from a float CHW image, the tail of the Triton python post-process model
 * (fde/modules/face_detection_trt_server/models/yolov5_face_postprocess/1/model.py:47-49,85-103): image (3,H,W) fp32
 * RGB in [0,1] -> *255, RGB->BGR -> crop [y:yh, x:xw] -> cv2.resize (float INTER_LINEAR) to (out_w, out_h) ->
 * (v - 127.5)/127.5 -> out [n][3][out_h][out_w].  boxes [n][4] int32 (x, y, xw, yh) in DEVICE memory, already clamped
 * to the image with xw > x and yh > y.  cv2 is absent offline: parity unpinned (restated in oracle/).
 */
int fp_crop_resize_f32(const float* image_chw, int H, int W, const int32_t* boxes, int n_boxes, float* out,
                       int out_h, int out_w, void* stream);

/*
 * Face-tracker matching for one frame (fde/face_extraction/extract_and_label_faces_from_dataset.py:101-121,
 * Net.check_if_face_exists + Net.add_face; IoU = fde/modules/utils/image.py:124-143).  The F new faces are
 * processed in order; each is compared with the known faces in insertion order and takes the FIRST one with
 * (dist < normal_thres && iou > 0.1) || dist < harsh_thres, whose stored feature and box it then replaces; without
 * a match it is appended (id = count + 1).  mode 0: dist = ||a - b||_2 (MOBILE_FACENET), mode 1: cosine distance.
 * feats [cap][D] fp32, bboxes [cap][4] int32 (x, y, xw, yh), count [1] int32 are device state updated in place;
 * ids[f] = 1-based face id (0 when the gallery is full), exists[f] = 1 if an existing face was matched.
 */
int fp_tracker_step(float* feats, int* bboxes, int* count, int cap, int D, const float* new_feats,
                    const int* new_bboxes, int F, int mode, float normal_thres, float harsh_thres,
                    int* ids, uint8_t* exists, void* stream);

/* ------------------------------------------------------------------------- */
/* 7. JPEG decode (the step in front of the path)           */
/* ------------------------------------------------------------------------- */

/*
 * Baseline JPEG decode, byte-identical to libjpeg-turbo's default decompressor -- what cv2.imread
 * (fde/modules/utils/inference.py:68-76, fde/face_extraction/extract_faces_from_dataset.py:393-420) and Pillow return.
 * Split as hardware decoders split it: marker parsing and Huffman decoding on the HOST (serial per scan; plain C, no GPU:
 * fp_jpeg_parse, fp_jpeg_entropy_decode -- run one thread per image), everything after it on the DEVICE
 * (fp_jpeg_reconstruct: dequantisation + the "islow" integer inverse DCT of jidctint.c, the chroma upsampling of
 * jdsample.c for 4:2:0 / 4:2:2 -- fancy (triangle) where the chroma plane is more than 2 samples wide, replication where it
 * is not, as jinit_upsampler chooses --, YCbCr -> RGB of jdcolor.c, csrc/jpeg.hip).  Any number of 0xff fill bytes may stand
 * in front of a marker, RSTn inside a scan included.  Accepted: SOF0 / SOF1 (sequential) and SOF2
 * (progressive: spectral selection and successive approximation), 8-bit, Huffman, any number of scans, 1 or 3 components, luma
 * sampling 1x1 / 2x1 / 2x2 with 1x1 chroma, restart intervals.  Everything else (arithmetic, lossless, 12-bit, CMYK, other
 * sampling layouts): FP_ERR_UNSUPPORTED, the caller decodes those on the host.
 *
 * ABI 12: the Huffman stage of SEQUENTIAL files on the DEVICE as well (csrc/jpegdec.hip), for a whole batch in one call.
 * fp_jpeg_scan_prepare (host) parses the headers into an fp_jpeg_scan descriptor; it takes SOF0 / SOF1 files whose first scan
 * is interleaved over every component (a single scan for gray files), with or without restart intervals, up to
 * FP_JPEG_DEV_MAX_BYTES of scan data and FP_JPEG_DEV_MAX_BLOCKS blocks, and returns FP_ERR_UNSUPPORTED for everything else
 * (progressive files among them).  fp_jpeg_entropy_decode_device splits every scan without regard to restart markers
 * into subsequences of sub_bits bits, decodes each from a guessed codeword boundary, re-decodes each from its predecessor's
 * exit until a whole pass reproduces every exit (at most max_rounds passes: the decodes are then proven to be the serial
 * decode's), places the blocks by a prefix sum of the block counts and writes them.  The result, for every image it reports
 * FP_OK or FP_ERR_INVALID_ARG for, equals fp_jpeg_entropy_decode's status and coefficients bit for bit, damaged files
 * included.  FP_JPEG_DECODE_ON_HOST: the device did not decide this image (a second scan or another segment behind the
 * first scan, fill bytes 0xff 0xff inside the scan, no proof within max_rounds): run fp_jpeg_entropy_decode on it.
 * fp_jpeg_entropy_decode_emulate runs the same phases serially on the CPU from the same per-subsequence code.
 */
typedef struct fp_jpeg_info {
  int32_t width, height, ncomp, restart_interval;
  int32_t progressive, reserved;      /* 1: SOF2 (several scans build the coefficients up) */
  int32_t hs[3], vs[3];               /* sampling factors */
  int32_t mcux, mcuy;                 /* MCUs per row / column */
  int32_t blocks_w[3], blocks_h[3];   /* 8 x 8 blocks per component, padded to whole MCUs */
  int32_t comp_w[3], comp_h[3];       /* a component's true size: ceil(image * samp / max samp) */
  int64_t coef_off[3];                /* component c: coefs + coef_off[c], [blocks_h][blocks_w][64] int16, natural (row-major) order */
  int64_t n_coefs;                    /* total int16 coefficients */
  uint16_t quant[3][64];              /* quantisation table of each component, natural order */
} fp_jpeg_info;

/* HOST.  Parses the markers up to the scan header. */
int fp_jpeg_parse(const uint8_t* data, size_t n, fp_jpeg_info* info);
/* HOST.  Huffman-decodes the scan into coefs (HOST memory, info->n_coefs int16: quantised, de-zigzagged). */
int fp_jpeg_entropy_decode(const uint8_t* data, size_t n, const fp_jpeg_info* info, int16_t* coefs);
/* Bytes of device workspace fp_jpeg_reconstruct needs (the components' sample planes). */
size_t fp_jpeg_workspace_bytes(const fp_jpeg_info* info);
/*
 * DEVICE.  coefs: the coefficients in DEVICE memory; info: HOST struct (passed by value to the kernels); workspace:
 * device, 8-byte aligned; out: device u8 [height][width][3], RGB (bgr = 0) or BGR (bgr = 1, cv2.imread's order);
 * a one-component image is replicated into the three channels (cv2.imread's default IMREAD_COLOR).
 */
int fp_jpeg_reconstruct(const int16_t* coefs, const fp_jpeg_info* info, uint8_t* workspace, size_t ws_bytes, uint8_t* out,
                        int bgr, void* stream);

/*
 * Frames of ONE geometry in one launch sequence (added within ABI 15: functions only; csrc/jpegbatch.hip) -- the frames of a
 * Motion-JPEG video.  A SEQUENTIAL file that defines no Huffman table decodes with the tables of ITU T.81 Annex K.3 in slots 0
 * (luminance) and 1 (chrominance) of both classes, as libjpeg-turbo's std_huff_tables installs them; DHT segments overwrite
 * them, slots 2 and 3 stay absent (fp_jpeg_parse, fp_jpeg_entropy_decode, fp_jpeg_scan_prepare).  A progressive file gets no
 * presets, as in libjpeg-turbo's jdphuff.c: a scan whose table no DHT defined is FP_ERR_INVALID_ARG.
 * DEVICE.  fp_jpeg_reconstruct_batch: fp_jpeg_reconstruct for n_frames frames that all have info's width, height, components
 * and sampling; info->quant is NOT read.  coefs: device; frame f's coefficients stand at coefs + coef_off[f] (int16 elements,
 * laid out by info->coef_off as for one frame) -- the host path's arena and the device entropy decoder's padded arena both
 * fit.  coef_off: DEVICE, n_frames int64.  quant: DEVICE, [n_frames][3][64] uint16, natural order: frame f's tables (rows
 * behind ncomp are not read).  workspace: device, 8-byte aligned, fp_jpeg_batch_workspace_bytes (= n_frames x
 * fp_jpeg_workspace_bytes).  out: device u8 [n_frames][height][width][3].  Two launches whatever n_frames is, 64-bit indices;
 * out[f] equals fp_jpeg_reconstruct's frame byte for byte (the same device functions, csrc/jpegrecon.h).  The coefficient
 * offsets live on the device and are not checked: the caller vouches that coef_off[f] + info->n_coefs stays inside coefs.
 * FP_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups in one launch (split the batch).  Full size, no orientation.
 */
size_t fp_jpeg_batch_workspace_bytes(const fp_jpeg_info* info, int n_frames);
int fp_jpeg_reconstruct_batch(const int16_t* coefs, const int64_t* coef_off, const uint16_t* quant, const fp_jpeg_info* info,
                              int n_frames, uint8_t* workspace, size_t ws_bytes, uint8_t* out, int bgr, void* stream);

/*
 * EXIF orientation and reduced-size output (added within ABI 15: functions only, no struct changes).
 * HOST.  fp_jpeg_exif_orientation: the Orientation tag (0x0112, type SHORT, IFD0) of the first APP1 segment that starts
 * with "Exif\0\0" in front of the first scan: 1 .. 8; 1 for no tag, a value outside 1 .. 8, or a truncated or inconsistent
 * segment.  Never reads outside data[0 .. n).
 * fp_jpeg_reconstruct_scaled (csrc/jpegscale.hip): what libjpeg-turbo returns at scale_denom = 1 / 2 / 4 / 8 -- cv2.imread's
 * IMREAD_REDUCED_COLOR_2 / _4 / _8 -- turned upright by the orientation tag afterwards, as cv2.imread does.  At scale_denom s
 * the picture is ceil(width / s) x ceil(height / s) and comes out of reduced inverse DCTs, no resize: luma blocks of
 * m = 8 / s samples (jidctred.c's 4 x 4 and 2 x 2 transforms, the DC term alone at 1 / 8), chroma blocks of up to 2m where
 * jdmaster.c scales chroma up in the IDCT rather than by upsampling (4:2:0: no upsampling at all below full size), h2v1
 * upsampling for 4:2:2 -- fancy only for m > 1 and a chroma plane more than 2 samples wide.  Orientation o maps the scaled
 * H' x W' picture `in` to out[y][x] = in[y][x] (1), in[y][W'-1-x] (2), in[H'-1-y][W'-1-x] (3), in[H'-1-y][x] (4), in[x][y] (5),
 * in[H'-1-x][y] (6), in[H'-1-x][W'-1-y] (7), in[x][W'-1-y] (8); 5 .. 8 give a W' x H' x 3 frame.  fp_jpeg_scaled_size writes
 * the OUTPUT frame's rows and columns.  workspace: device, 8-byte aligned, fp_jpeg_scaled_workspace_bytes; out: device,
 * 4-byte aligned.  Integer arithmetic only, no atomics: runs are bit-identical.  fp_jpeg_reconstruct_scaled_emulate runs the
 * same __host__ __device__ arithmetic serially on the CPU (coefs, workspace, out: HOST memory).
 */
int fp_jpeg_exif_orientation(const uint8_t* data, size_t n);
int fp_jpeg_scaled_size(const fp_jpeg_info* info, int scale_denom, int orientation, int* out_h, int* out_w);
size_t fp_jpeg_scaled_workspace_bytes(const fp_jpeg_info* info, int scale_denom);
int fp_jpeg_reconstruct_scaled(const int16_t* coefs, const fp_jpeg_info* info, int scale_denom, int orientation, uint8_t* workspace,
                               size_t ws_bytes, uint8_t* out, int bgr, void* stream);
int fp_jpeg_reconstruct_scaled_emulate(const int16_t* coefs, const fp_jpeg_info* info, int scale_denom, int orientation,
                                       uint8_t* workspace, size_t ws_bytes, uint8_t* out, int bgr);

#define FP_JPEG_DECODE_ON_HOST 1                /* device status: decode this image with fp_jpeg_entropy_decode */
#define FP_JPEG_DEV_MAX_BYTES (64ll << 20)       /* scan data of one file the device path takes */
#define FP_JPEG_DEV_MAX_BLOCKS (1 << 20)         /* 8 x 8 blocks of one image the device path takes */

/* One canonical Huffman table in the device decoder's lookup form. */
typedef struct fp_jpeg_huff {
  uint16_t look[512];      /* the next 9 bits -> code length << 8 | symbol; 0 = the code is longer than 9 bits */
  int32_t maxcode[18];     /* largest code of each length (-1: none of that length) */
  int32_t valoff[18];      /* a code of length l is symbol vals[code + valoff[l]] */
  uint8_t vals[256];
} fp_jpeg_huff;

/* The first scan of a sequential file, as fp_jpeg_entropy_decode_device reads it. */
typedef struct fp_jpeg_scan {
  int64_t data_off;        /* byte offset of the entropy-coded data in the file (behind the SOS header) */
  int64_t data_len;        /* bytes from there to the end of the file */
  int64_t n_coefs;         /* = fp_jpeg_info.n_coefs */
  int64_t coef_off[3];     /* = fp_jpeg_info.coef_off */
  int32_t blocks_w[3];     /* = fp_jpeg_info.blocks_w */
  int32_t mcux, mcuy;      /* MCUs per row / column */
  int32_t restart_interval;   /* MCUs per restart segment, 0 = none */
  int32_t blocks_per_mcu;  /* 1 .. 6 */
  int32_t ncomp;
  uint8_t slot_comp[8];    /* per block slot of an MCU, in decode order: component */
  uint8_t slot_tab[8];     /* ... its tables: dc[slot_tab] / ac[slot_tab] */
  uint8_t slot_dy[8];      /* ... its block row / column inside the MCU */
  uint8_t slot_dx[8];
  int32_t hs[3], vs[3];    /* blocks of each component per MCU */
  fp_jpeg_huff dc[3], ac[3];  /* the tables of the scan's components, in scan order */
} fp_jpeg_scan;

/* HOST.  Headers of a file -> info (as fp_jpeg_parse) and scan.  FP_ERR_UNSUPPORTED: not for the device path (see above). */
int fp_jpeg_scan_prepare(const uint8_t* data, size_t n, fp_jpeg_info* info, fp_jpeg_scan* scan);
/* Bytes of device workspace fp_jpeg_entropy_decode_device needs for these n files (scans: HOST). */
size_t fp_jpeg_entropy_workspace_bytes(const fp_jpeg_scan* scans, int n, int sub_bits, int max_rounds);
/*
 * DEVICE.  files: device, file i at files + file_off[i]; scans, file_off, coef_off: HOST arrays of n; coefs: device int16, image i
 * at coefs + coef_off[i] (scans[i].n_coefs values, zeroed here first); status: device int32 [n], FP_OK / FP_ERR_INVALID_ARG /
 * FP_JPEG_DECODE_ON_HOST; workspace: device, 16-byte aligned, fp_jpeg_entropy_workspace_bytes.  sub_bits (>= 32, a multiple of
 * 8): subsequence length; max_rounds (>= 1): synchronisation passes.  Copies the descriptors into the workspace before it returns.
 */
int fp_jpeg_entropy_decode_device(const uint8_t* files, const fp_jpeg_scan* scans, const int64_t* file_off, int n, int16_t* coefs,
                                  const int64_t* coef_off, int32_t* status, void* workspace, size_t ws_bytes, int sub_bits,
                                  int max_rounds, void* stream);
/* HOST.  The device algorithm run serially on one file: returns the status the device would report, coefs (HOST, n_coefs) as
 * the device would write them; rounds (may be NULL) = synchronisation passes until the proof (max_rounds + 1: none). */
int fp_jpeg_entropy_decode_emulate(const uint8_t* data, size_t n, const fp_jpeg_scan* scan, int16_t* coefs, int sub_bits,
                                   int max_rounds, int32_t* rounds);

/* ------------------------------------------------------------------------- */
/* 8. JPEG encode (the face crops the reference's driver saves)                */
/* ------------------------------------------------------------------------- */

/*
 * Face alignment (csrc/align.hip).  The embedder's input as a similarity warp of the frame onto the ArcFace 112 x 112
 * five-point template (38.2946, 51.6963) (73.5318, 51.5014) (56.0252, 71.7366) (41.5493, 92.3655) (70.7299, 92.2041)
 * instead of the stretched box crop.  All additive: fp_dets_to_crops and fp_resize_* are unchanged.
 *
 * fp_dets_to_crops_aligned / _ragged take fp_dets_to_crops' / _ragged's arguments and write the same items, face_info and
 * n_faces bit for bit, plus, per face (device memory, max_faces rows):
 *   lmarks[10]: landmarks in frame pixels, fp32, in numpy's float32 operation order.  fmt 0 (BlazeFace; row_floats >= 17):
 *               keypoints 0..3 (x, y) * (in_w, in_h), - pad, / gain, round half-to-even, not clipped (bbox_lmarks of
 *               get_dets_bboxes_confs_lmarks_areas), slots 8 and 9 = 0.  fmt 1 (YOLOv5-face; row_floats >= 15): columns
 *               5..14 - pad, / gain, clamped to [0, w] / [0, h], not rounded (scale_coords_landmarks).
 *   M[6]:       the least-squares similarity frame -> template (a, -b, tx, b, a, ty), fp64 (Umeyama's estimate in closed
 *               form).  fmt 1: landmark i -> template point i; fmt 0: keypoints 0, 1, 2, 3 -> points 0, 1, 2 and the
 *               midpoint of 3 and 4.
 *   flags:      FP_ALIGN_DEGENERATE when the centred landmarks' sum of squares is < 1 px^2 (or the fit is not finite);
 *               M is then 0 and the face's embedder input is its box crop.
 * Refusals before any launch: those of fp_dets_to_crops, a NULL lmarks / M / flags, fmt 1 with row_floats < 15
 * (FP_ERR_INVALID_ARG); M not 8-byte aligned (FP_ERR_ALIGNMENT).
 */
#define FP_ALIGN_SIZE 112
#define FP_ALIGN_DEGENERATE 1

int fp_dets_to_crops_aligned(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt,
                             int in_w, int in_h, int orig_w, int orig_h, float det_thres, float area_thres,
                             float gain, float pad_x, float pad_y, int off_tx, int off_ty, int off_bx, int off_by,
                             int dst_w, int dst_h, int max_faces,
                             fp_resize_item* items, float* face_info, int32_t* n_faces,
                             float* lmarks, double* M, int32_t* flags, void* stream);
int fp_dets_to_crops_aligned_ragged(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt,
                                    int in_w, int in_h, const fp_frame_desc* descs /*device, B*/,
                                    const float* geom /*device, B x 3*/, float det_thres, float area_thres,
                                    int off_tx, int off_ty, int off_bx, int off_by, int dst_w, int dst_h, int max_faces,
                                    fp_resize_item* items, float* face_info, int32_t* n_faces,
                                    float* lmarks, double* M, int32_t* flags, void* stream);
/* HOST.  fp_dets_to_crops_aligned_ragged run serially on host memory (every pointer HOST); the same values. */
int fp_dets_to_crops_aligned_emulate(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt,
                                     int in_w, int in_h, const fp_frame_desc* descs, const float* geom, float det_thres,
                                     float area_thres, int off_tx, int off_ty, int off_bx, int off_by, int dst_w, int dst_h,
                                     int max_faces, fp_resize_item* items, float* face_info, int32_t* n_faces,
                                     float* lmarks, double* M, int32_t* flags);

/*
 * The embedder's input of n faces: canvas k = face k warped by M[k] (frame -> template) out of frame (int)face_info[k][0]
 * (cv2.warpAffine's convention: output pixel (x, y), 0 <= x, y < 112, samples the frame at M^-1 (x, y), no half-pixel
 * shift), bilinear in fp32 over the u8 BGR frame, taps outside the frame 0 (BORDER_CONSTANT 0).  A face whose flags carry
 * FP_ALIGN_DEGENERATE gets the box crop of items[k] instead, bit for bit what fp_resize_normalize / fp_resize_ragged
 * make of it (pad 0, no R/B swap).  Outputs (either may be NULL, not both; device):
 *   out_u8  [n][112][112][3]: the value rounded half-to-even, clamped to [0, 255], channels in frame order;
 *   out_f32 [n][112][112][out_c], out_c = 3 or 4 (4: 16-byte aligned, the 4th channel 0): lut256[u8] (256 device floats).
 * M, face_info, flags and items are device memory the host does not read: a frame index outside the batch, a descriptor
 * outside the limits of fp_resize_ragged or a non-invertible M gives a canvas of 0s, never a load outside the frames.
 * Refusals before any launch: NULL pointers, n < 0, n_frames <= 0, sizes out of range, out_c not 3 / 4, no output
 * (FP_ERR_INVALID_ARG); M not 8-byte aligned, face_info / flags / items not 4-byte aligned, a misaligned out_f32
 * (FP_ERR_ALIGNMENT).  fp_align_warp: frames [n_frames][frame_h][frame_w][3], frame_h <= 65535, frame_w <= 32767;
 * fp_align_warp_ragged: a ragged batch (section 2, the trust boundary of fp_resize_ragged).
 */
int fp_align_warp(const uint8_t* frames, int n_frames, int frame_h, int frame_w, const double* M /*device, n x 6*/,
                  const float* face_info /*device, n x 7*/, const int32_t* flags /*device, n*/,
                  const fp_resize_item* items /*device, n*/, int n, uint8_t* out_u8, float* out_f32, int out_c,
                  const float* lut256, void* stream);
int fp_align_warp_ragged(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs /*device*/, int n_frames,
                         const double* M, const float* face_info, const int32_t* flags, const fp_resize_item* items, int n,
                         uint8_t* out_u8, float* out_f32, int out_c, const float* lut256, void* stream);
/*
 * HOST.  The device's estimate and per-pixel code run serially on host memory (every pointer HOST).  lmarks non-NULL
 * (n x 10, fmt as above): M and flags are computed from them; NULL: M and flags are inputs.  out_u8 non-NULL: the u8
 * canvases of fp_align_warp_ragged over frames described by descs (a uniform batch is n_frames equal descriptors).
 */
int fp_align_emulate(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const float* lmarks,
                     int fmt, double* M, const float* face_info, int32_t* flags, const fp_resize_item* items, int n,
                     uint8_t* out_u8);

/*
 * ABI 13.  Baseline (SOF0) encoding of a batch of 8-bit RGB / BGR crops, byte-identical to libjpeg-turbo's default compressor
 * (jpeg_set_defaults + jpeg_set_quality(quality, TRUE): islow DCT, the Annex K tables scaled by quality, standard Huffman
 * tables, no restart markers, no Huffman optimisation) -- what cv2.imwrite writes for the reference's face crops
 * (fde/face_extraction/extract_faces_from_dataset.py:311-363) and Pillow's save(quality=q, subsampling=s).  csrc/jpegenc.hip.
 * A file = fp_jpeg_encode_headers (host: SOI, JFIF APP0, 2 x DQT, SOF0, 4 x DHT, SOS) + the image's scan data
 * + EOI (FF D9).  Subsampling 4:4:4, 4:2:2, 4:2:0 (the default of both); quality 1 .. 100; crops of 1 .. 65535 pixels a side.
 *
 * Item i encodes src[src_off + y * src_w * 3 + x * 3 ...] (3 bytes per pixel, packed rows) over the rectangle clamped the
 * way the reference slices it, image[max(y0, 0):min(y1, src_h), max(x0, 0):min(x1, src_w)].  An empty rectangle after the
 * clamp: FP_ERR_INVALID_ARG; subsampling outside 0 .. 2, a side over 65535 or more than 2^31 - 1 blocks: FP_ERR_UNSUPPORTED.
 *
 * Sizing: one 8 x 8 block codes to at most 22 (DC) + 63 x 26 (AC) = 1660 bits, 208 bytes; byte stuffing at most doubles
 * that.  So n_blocks x FP_JPEG_ENC_BYTES_PER_BLOCK bytes hold the scan data of any batch, whatever the pixels; the call needs
 * no host sync to size its output.
 */
#define FP_JPEG_444 0
#define FP_JPEG_422 1
#define FP_JPEG_420 2
#define FP_JPEG_ENC_BYTES_PER_BLOCK 416
#define FP_JPEG_ENC_HEADER_BYTES 623   /* what fp_jpeg_encode_headers writes, for every size, quality and subsampling */

typedef struct fp_jpeg_enc_item {
  int64_t src_off;          /* byte offset of the source image's pixel (0, 0) in src */
  int32_t src_h, src_w;     /* the source image's size (pixels) */
  int32_t x0, y0, x1, y1;   /* the crop, [y0, y1) x [x0, x1), clamped to the source image */
} fp_jpeg_enc_item;

/* HOST.  Checks the batch (items: HOST) and sizes it: *ws_bytes of device workspace, *out_bytes of output
 * (= n_blocks * FP_JPEG_ENC_BYTES_PER_BLOCK).  FP_OK or the refusal's status. */
int fp_jpeg_encode_workspace_bytes(const fp_jpeg_enc_item* items, int n, int subsampling, size_t* ws_bytes, size_t* out_bytes);
/* HOST.  The headers of a width x height file (FP_JPEG_ENC_HEADER_BYTES bytes into out): returns that count or a status < 0. */
int fp_jpeg_encode_headers(int width, int height, int quality, int subsampling, uint8_t* out, size_t cap);
/*
 * DEVICE.  src: device u8; items: HOST array of n; workspace: device, 16-byte aligned, fp_jpeg_encode_workspace_bytes; out: device,
 * >= out_bytes.  Writes the scan data (stuffed, last byte padded with 1-bits) of image i at out + out_off[i], images back to back,
 * out_off[n] = the total (out_off: device int64 [n + 1]).  bgr = 1: the pixels are B, G, R (cv2's order).  Copies the
 * descriptors into the workspace before it returns.
 */
int fp_jpeg_encode_device(const uint8_t* src, const fp_jpeg_enc_item* items, int n, int quality, int subsampling, int bgr,
                          void* workspace, size_t ws_bytes, uint8_t* out, size_t out_cap, int64_t* out_off, void* stream);
/* HOST.  The device's phases run serially on host memory (src, out, out_off: HOST); the same bytes. */
int fp_jpeg_encode_emulate(const uint8_t* src, const fp_jpeg_enc_item* items, int n, int quality, int subsampling, int bgr,
                           uint8_t* out, size_t out_cap, int64_t* out_off);

/* ------------------------------------------------------------------------- */
/* 9. MTCNN (P-Net / R-Net / O-Net cascade, Zhang et al. 2016)                 */
/* ------------------------------------------------------------------------- */
/*
 * Appended in ABI 14 (nothing existing changes).  The procedure is written down in DESIGN.md section 7 ("MTCNN"); the
 * float64 restatement the tests compare with is tests/mtcnn_restatement.py.
 *
 * Stage 1: P-Net runs level by level as a plan of generic ops (conv + PReLU, ceil-mode max pool, a 1x1 conv for both heads)
 * on groups of equally sized frames.  csrc/pnet.hip holds what surrounds it: fp_pnet_level_images writes a pyramid level of the
 * group into the plan's input, fp_pnet_threshold turns the head map into 24-byte fp_pnet_cand records of the cells with
 * p >= t1, handed out by a per-frame atomic counter.  fp_mtcnn_stage1 puts them into (level, cell) order before it uses
 * them, so the result does not depend on the order of the atomics.  A frame with more than `cap` candidates sets
 * overflow[frame] = 1 (the host raises); counts[frame] still holds the true number.
 */
#define FP_MTCNN_MAX_CAP 8192
typedef struct fp_pnet_level {
  double scale;          /* s_k: boxes are generated with it */
  int32_t lh, lw;        /* level size: ceil(h s), ceil(w s) */
  int32_t oh, ow;        /* P-Net output map: ceil((l - 2) / 2) - 4 */
} fp_pnet_level;
typedef struct fp_pnet_cand {
  float reg[4];          /* box regression (x1, y1, x2, y2) */
  float score;           /* face probability */
  uint32_t key;          /* (level within the frame) << 24 | (y * ow + x) */
} fp_pnet_cand;
/*
 * fp_pnet_level_images: out[i] ([n][lh][lw][4] fp32, 16-byte aligned) = the lh x lw level of frame frame_idx[i] (device int32
 * [n]; every frame at least lh x lw): each pixel the exact area-weighted mean of its source rectangle (integer arithmetic),
 * rounded half-to-even to u8, then (v - 127.5) / 128; fourth channel 0.  A frame index or extent outside the tables / the
 * frames buffer gives zeros.
 * fp_pnet_threshold: head ([n][oh * ow][ld] fp32, ld >= 8 a multiple of 4: class logits 0, 1, regression 2 .. 5) of the same
 * frames at level `level` (the level's index within its frame's pyramid): p = softmax(logits)[1]; cells with p >= t1 are
 * appended to cand[frame] with key = level << 24 | cell.  counts / overflow ([n_frames]) accumulate over calls: the caller zeroes
 * them before the first level.  Refusals (FP_ERR_INVALID_ARG) before any launch: a NULL or misaligned pointer, sizes out of range,
 * oh * ow > 2^24, level > 127, cap < 1 or > FP_MTCNN_MAX_CAP.
 */
int fp_pnet_level_images(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs /*device*/, int n_frames,
                         const int32_t* frame_idx /*device*/, int n, int lh, int lw, float* out, void* stream);
int fp_pnet_threshold(const float* head, int ld, const int32_t* frame_idx /*device*/, int n, int n_frames, int oh, int ow, int level,
                      float t1, int cap, fp_pnet_cand* cand /*[n_frames][cap]*/, int32_t* counts, int32_t* overflow, void* stream);

/*
 * The cascade's glue (csrc/mtcnn.hip), one workgroup per frame, fp64 box arithmetic, fp32 IoU without contraction.
 * NMS everywhere: area (x2 - x1 + 1)(y2 - y1 + 1), intersection with the same + 1, visit by descending score (equal
 * scores: the lower candidate index wins), drop a box when o > thr against a kept one; o = inter / union, or inter /
 * min(a_i, a_j) in stage 3.
 * boxes: [n_frames][cap][4] int32 (x1, y1, x2, y2) + scores [n_frames][cap], in kept order (descending score);
 * scratch: fp_mtcnn_scratch_bytes(n_frames, cap) bytes.
 *
 * fp_mtcnn_stage1: candidates -> (level, cell) order -> boxes q1 = trunc((2 (x, y) + 1) / s), q2 = trunc((2 (x, y) + 12)
 * / s) -> NMS 0.5 per level -> NMS 0.7 per frame -> b = q + reg (w_q, h_q), squared, truncated; boxes with a side
 * x2 - x1 + 1 <= 0 are dropped.
 */
size_t fp_mtcnn_scratch_bytes(int n_frames, int cap);
int fp_mtcnn_stage1(const fp_pnet_cand* cand, const int32_t* counts, int n_frames, int cap, const fp_pnet_level* levels,
                    int n_levels, const int32_t* frame_level0, int32_t* boxes, float* scores, int32_t* out_counts,
                    void* scratch, size_t scratch_bytes, void* stream);
/*
 * fp_mtcnn_cut: candidate i of the flat list (frame f = the one with offs[f] <= i < offs[f + 1], box boxes[f][i - offs[f]])
 * -> the zero-filled (y2 - y1 + 1) x (x2 - x1 + 1) patch whose pixel (py, px) is frame pixel (y1 - 1 + py, x1 - 1 + px)
 * where that lies inside the frame, resized to size x size: the area mean when neither axis grows, else linear taps in
 * "area mode" (sx = floor(dx scale), fx = (dx + 1) - (sx + 1) / scale, fx <= 0 ? 0 : fx - floor(fx)); both in exact integer
 * arithmetic (the weights are multiples of 1 / patch size), rounded half-to-even to u8.  out: [n][size][size][4] fp32 (v - 127.5) / 128, fourth channel 0; out_u8 (or NULL): [n][size][size][3].
 */
int fp_mtcnn_cut(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const int32_t* boxes,
                 int cap, const int32_t* offs /*device [n_frames + 1]*/, int n, int size, float* out, uint8_t* out_u8,
                 void* stream);
/*
 * fp_mtcnn_stage2: rows offs[f] .. offs[f + 1] of prob ([n][prob_ld], face = column 1) and reg ([n][reg_ld], 4 columns)
 * belong to boxes[f]: keep p >= t2 -> NMS 0.7 -> b = box + reg (w, h), w = x2 - x1 + 1 -> squared, truncated -> out_boxes.
 */
int fp_mtcnn_stage2(const int32_t* boxes, int n_frames, int cap, const int32_t* offs, const float* prob, int prob_ld,
                    const float* reg, int reg_ld, float t2, int32_t* out_boxes, float* out_scores, int32_t* out_counts,
                    void* scratch, size_t scratch_bytes, void* stream);
/*
 * fp_mtcnn_stage3: keep p >= t3; landmarks X = x1 - 1 + w lx, Y = y1 - 1 + h ly (reg columns 4 .. 8 = x, 9 .. 13 = y) on the
 * input box; b = box + reg (w, h); NMS 0.7 "min".  dets: [n_frames][max_det][15] = (x1, y1, x2, y2, (X, Y) x 5, score) in
 * frame pixels by descending score; counts[f] = min(found, max_det), overflow[f] = found > max_det.
 */
int fp_mtcnn_stage3(const int32_t* boxes, int n_frames, int cap, const int32_t* offs, const float* prob, int prob_ld,
                    const float* reg, int reg_ld, float t3, int max_det, float* dets, int32_t* counts, int32_t* overflow,
                    void* scratch, size_t scratch_bytes, void* stream);
/*
 * MTCNN rows -> face crops: fp_dets_to_crops_ragged / fp_dets_to_crops_aligned_ragged for rows that are ALREADY in each frame's
 * own pixels (dets [B][max_dets][row_floats >= 15] = fp_mtcnn_stage3's rows; "fmt 2" of csrc/align.hip).  conf > det_thres, the
 * box's share of the FRAME (100 * area / (w h) > area_thres; info[6] = the fraction), clip to the frame, round half-to-even,
 * then the same crop arithmetic, items and face_info.  lmarks / M / flags all NULL: box crops; all given: also the five
 * landmarks (clipped to the frame), the alignment transform and flags of fp_dets_to_crops_aligned.  Dense batches pass descs
 * with equal sizes.  fp_align_emulate accepts fmt 2 (five points, as fmt 1).
 */
int fp_dets_to_crops_px(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats,
                        const fp_frame_desc* descs /*device, B*/, float det_thres, float area_thres, int off_tx, int off_ty,
                        int off_bx, int off_by, int dst_w, int dst_h, int max_faces, fp_resize_item* items, float* face_info,
                        int32_t* n_faces, float* lmarks, double* M, int32_t* flags, void* stream);
/*
 * The box arithmetic of the stages alone (the same device functions the stage kernels call; tests feed it the restatement's
 * kept boxes): boxes [n][4] fp32 (integers in value), reg [n][reg_ld].  mode 1: b = box + reg (w, h), w = x2 - x1, squared,
 * truncated -> out_boxes [n][4] int32; mode 2: the same with w = x2 - x1 + 1; mode 3: b = box + reg (w, h), w = x2 - x1 + 1, not
 * squared, and the landmarks X = x1 - 1 + w lx, Y = y1 - 1 + h ly (reg columns 4 .. 8 = lx, 9 .. 13 = ly) -> out_rows [n][14] fp32
 * = (x1, y1, x2, y2, (X, Y) x 5).
 */
int fp_mtcnn_boxes(const float* boxes, const float* reg, int reg_ld, int n, int mode, int32_t* out_boxes, float* out_rows,
                   void* stream);
/*
 * The NMS of the stages alone (tests feed it the restatement's boxes): segment s = rows seg[s] .. seg[s + 1] of boxes
 * ([n][4] fp32) / scores; mode 0 = union, 1 = min.  keep_idx[seg[s] + k] = row index (within the whole list) of the k-th
 * kept box of segment s in visiting order, keep_count[s] their number.  A segment takes at most FP_MTCNN_MAX_CAP rows.
 */
int fp_mtcnn_nms(const float* boxes, const float* scores, const int32_t* seg /*device [n_seg + 1]*/, int n_seg, int n,
                 float thr, int mode, int32_t* keep_idx, int32_t* keep_count, void* scratch, size_t scratch_bytes,
                 void* stream);

/* ------------------------------------------------------------------------- */
/* Detector evaluation: COCO-style bbox AP / AR (build-defined)      */
/* ------------------------------------------------------------------------- */

/*
 * The published COCO bbox procedure for one category without crowd boxes, restated (pycocotools is not in the reference
 * tree; face_detection_and_recognition_amd/evaluation.py states the same procedure in numpy fp64 and is the oracle).  All
 * boxes are xywh fp64; IoU = i / (dw dh + gw gh - i) in fp64 without contraction, 0 when the intersection's width or height
 * is <= 0.
 *
 * fp_det_match: greedy matching of every image's detections against its ground truth, for n_areas area ranges and n_thrs
 * IoU thresholds in one launch (one workgroup per (image, area range), no host synchronisation).  gt_off / dt_off
 * [n_images + 1] int32 are CSR offsets into gt_boxes [n_gt][4] / gt_area [n_gt] and dt_boxes [n_dt][4]; an image's
 * detections are already in descending stable score order and cut to the largest maxDet.  area_rngs [n_areas][2] = (lo, hi):
 * a GT is ignored in a range when area < lo or area > hi.  Per detection in order, at threshold t: among the GTs that are
 * not ignored and not yet matched at t, the one with the largest IoU >= min(t, 1 - 1e-10), on equal IoU the LATER one;
 * failing that the same among the ignored GTs (the detection is then matched AND ignored); a detection left unmatched is
 * ignored when its own w h lies outside the range.  Outputs: matched / ignored [n_areas][n_thrs][n_dt] uint8, npig
 * [n_areas] int32 = GTs not ignored (zeroed here, summed with integer atomics).  workspace: fp_det_match_workspace(n_gt,
 * n_areas) bytes of device memory, 4-byte aligned.  Any number of GTs and detections per image, zero included; the
 * result does not depend on scheduling.  1 <= n_thrs <= FP_DETEVAL_MAX_THRS.  Refusals: a NULL pointer that is needed,
 * a count out of range, n_gt or n_dt >= 2^31, a workspace that is too small: FP_ERR_INVALID_ARG; a misaligned array:
 * FP_ERR_ALIGNMENT.
 *
 * fp_pr_accumulate: precision [n_thrs][n_recs][n_areas][n_maxdets] and recall [n_thrs][n_areas][n_maxdets] (fp64), one
 * workgroup per (threshold, area range, maxDet m) curve.  order [n_dt] int64 = the stable descending score order of the
 * n_dt detections fp_det_match saw (indices into its flag arrays), rank_sorted [n_dt] int32 = the per-image rank of
 * order[j].  A curve takes the detections with rank < m that are not ignored, in that order: tp / fp are exact integer
 * running counts, rc = tp / npig, pr = tp / (fp + tp + 2^-52), pr is replaced by its suffix maximum, and for every
 * recall threshold r precision = pr at the first index with rc >= r (0 if there is none); recall = the last rc (0
 * without detections).  npig[a] == 0: the cell's precision and recall are -1.  Every output element is written.
 * 1 <= n_recs <= FP_DETEVAL_MAX_RECS.
 */
#define FP_DETEVAL_MAX_THRS 31
#define FP_DETEVAL_MAX_RECS 1024
size_t fp_det_match_workspace(int64_t n_gt, int n_areas);
int fp_det_match(const double* gt_boxes, const double* gt_area, const int32_t* gt_off, const double* dt_boxes,
                 const int32_t* dt_off, int n_images, int64_t n_gt, int64_t n_dt, const double* iou_thrs, int n_thrs,
                 const double* area_rngs, int n_areas, uint8_t* matched, uint8_t* ignored, int32_t* npig, void* workspace,
                 size_t ws_bytes, void* stream);
int fp_pr_accumulate(const uint8_t* matched, const uint8_t* ignored, const int64_t* order, const int32_t* rank_sorted,
                     int64_t n_dt, const int32_t* npig, int n_thrs, int n_areas, const int32_t* max_dets, int n_maxdets,
                     const double* rec_thrs, int n_recs, double* precision, double* recall, void* stream);

/*
 * Drawing on device frames (build-defined, parity-unpinned against OpenCV; DESIGN §7 "Drawing"): boxes, landmark rings,
 * captions and pixelated (mosaic) rectangles rasterised in place into u8 BGR frames of either kind of batch (a dense batch is
 * n_frames equal descriptors).  A draw list is an array of fp_draw_cmd sorted by frame, with cmd_ranges [n_frames + 1]:
 * frame f owns cmds[cmd_ranges[f] .. cmd_ranges[f + 1]).  The commands of a frame apply IN LIST ORDER, each to the frame as
 * the commands before it left it; a pixel outside its frame is never touched.  All arithmetic is integer.  With (x, y) a
 * pixel of the frame and c the command:
 *   FP_DRAW_RECT    outline of thickness t = arg of the rectangle [x0, x1) x [y0, y1): the pixels of the rectangle grown by
 *                   t / 2 (floor) on every side that are not in the rectangle shrunk by (t + 1) / 2; 1 <= t <= FP_DRAW_MAX_ARG.
 *   FP_DRAW_FILL    every pixel of [x0, x1) x [y0, y1).
 *   FP_DRAW_RING    centre (x0, y0), radius r = arg (x1, y1 unused): (2r - 1)^2 <= 4 (dx^2 + dy^2) < (2r + 1)^2;
 *                   0 <= r <= FP_DRAW_MAX_ARG (r = 0 sets nothing).
 *   FP_DRAW_GLYPH   arg = code | scale << 8, code 32 .. 126, 1 <= scale s <= FP_DRAW_MAX_SCALE, cell [x0, x0 + 6s) x [y0, y0 + 8s)
 *                   (x1, y1 unused): set where bit (0x80 >> (x - x0) / s) of font[(code - 32) * 8 + (y - y0) / s] is 1.
 *   a pixel these four set becomes dst = (dst * (255 - a) + colour * a + 127) / 255 per channel (a = 255 overwrites).
 *   FP_DRAW_MOSAIC  cell = arg in {4, 8, 16, 32}, grid anchored at the frame's origin: within each cell, the pixels that lie
 *                   in [x0, x1) x [y0, y1) and in the frame are replaced by their per-channel mean (sum + cnt / 2) / cnt of
 *                   the current content.  Colour and alpha unused.
 * A command whose kind, glyph code, scale, thickness or radius is outside these ranges, whose frame field is not the frame
 * of its range, or with a coordinate outside [-FP_DRAW_MAX_COORD, FP_DRAW_MAX_COORD] is SKIPPED (by the kernel and by the
 * emulator alike: commands are device memory the host does not read).
 *
 * fp_draw: one workgroup per entry of tiles [n_tiles][3] int32 = (frame, tx, ty), the FP_DRAW_TILE x FP_DRAW_TILE tiles the
 * commands' bounding boxes touch (the caller built the commands and knows them; a tile that is not listed is not drawn; no
 * tile twice).  The workgroup holds its tile in LDS, keeps the frame's commands that meet it in order and applies them one
 * after another, then stores the tile: tiles are disjoint, so the call is race-free without atomics or scratch and two runs are
 * bit-identical.  font: FP_DRAW_FONT_BYTES bytes of device memory (95 glyphs x 8 row bytes; modules/utils/font6x8.py is the
 * only copy).  Stream-ordered, allocates nothing.  Refusals before any launch (FP_ERR_INVALID_ARG): a NULL pointer (cmds
 * may be NULL when n_cmds == 0, tiles when n_tiles == 0), a negative count.  n_tiles == 0: FP_OK, nothing launched.  The
 * kernel leaves a tile alone whose frame or tile index is outside the batch or whose frame does not lie inside frames_bytes.
 *
 * fp_draw_check (HOST arrays): what the host can refuse about lists it built, FP_ERR_INVALID_ARG for: a descriptor outside
 * 1 .. FP_FRAME_MAX_W x 1 .. FP_FRAME_MAX_H or not inside frames_bytes; cmd_ranges not starting at 0, ending at n_cmds and
 * non-decreasing; a command whose frame is not its range's; a mosaic cell not in {4, 8, 16, 32}; a tile whose frame or
 * position is outside the batch; tiles not in strictly ascending (frame, tx, ty) order.
 * fp_draw_emulate (HOST memory throughout): fp_draw_check, then the same procedure serially, tile by tile.
 */
typedef enum fp_draw_kind { FP_DRAW_RECT = 1, FP_DRAW_FILL = 2, FP_DRAW_RING = 3, FP_DRAW_GLYPH = 4, FP_DRAW_MOSAIC = 5 } fp_draw_kind;
typedef struct fp_draw_cmd {
  int32_t frame;            /* index into descs */
  int32_t kind;             /* fp_draw_kind */
  int32_t x0, y0, x1, y1;   /* inclusive-exclusive, frame pixels; may lie outside the frame */
  uint8_t b, g, r, a;       /* colour (BGR, the frames' order) and alpha */
  int32_t arg;              /* thickness / radius / code | scale << 8 / cell */
} fp_draw_cmd;              /* 32 bytes */
#define FP_DRAW_TILE 64
#define FP_DRAW_FONT_BYTES 760
#define FP_DRAW_MAX_ARG 4096
#define FP_DRAW_MAX_SCALE 64
#define FP_DRAW_MAX_COORD (1 << 20)
int fp_draw(uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs /*device*/, int n_frames,
            const fp_draw_cmd* cmds /*device*/, const int32_t* cmd_ranges /*device, n_frames + 1*/, int n_cmds,
            const int32_t* tiles /*device, n_tiles x 3*/, int n_tiles, const uint8_t* font /*device*/, void* stream);
int fp_draw_check(size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const fp_draw_cmd* cmds,
                  const int32_t* cmd_ranges, int n_cmds, const int32_t* tiles, int n_tiles);
int fp_draw_emulate(uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const fp_draw_cmd* cmds,
                    const int32_t* cmd_ranges, int n_cmds, const int32_t* tiles, int n_tiles, const uint8_t* font);

/*
 * Face crop quality (build-defined, parity-unpinned against OpenCV; DESIGN §7 "Face quality"; csrc/quality.hip): per face
 * rectangle, integer luma statistics and the sums of a Laplacian, read from the u8 BGR frames of either kind of batch; per
 * face, a pose record from its five landmarks.  All additive: ABI 14.
 *
 * Face i is items[i]'s source rectangle (src_image, sx, sy, sw, sh; the destination fields are ignored), clamped to its frame:
 * sw x sh below are the clamped sizes.  s = max(1, ceil(max(sw, sh) / 112)), bw = sw / s, bh = sh / s (floor); everything is
 * taken over the bw * s columns by bh * s rows anchored at the clamped corner, trailing pixels that fill no s x s block are
 * left out.  Y = (1868 B + 9617 G + 4899 R + 8192) >> 14.  stats[i] = eight int64:
 *   n_px, sum Y, sum Y^2, n_dark (Y <= 16), n_bright (Y >= 239), n_lap, sum L, sum L^2
 * with Bk[r][c] the sum of Y over block (r, c) and, for 1 <= r < bh - 1, 1 <= c < bw - 1,
 *   L = Bk[r-1][c] + Bk[r+1][c] + Bk[r][c-1] + Bk[r][c+1] - 4 Bk[r][c],   n_lap = (bw - 2) (bh - 2)
 * (interior samples only: no mirrored border, unlike cv2.Laplacian).  flags[i] (written, not OR-ed):
 *   FP_QUALITY_BAD_FRAME     src_image outside [0, n_frames), or the frame's descriptor outside [FP_FRAME_MIN_W, FP_FRAME_MAX_W]
 *                            x [1, FP_FRAME_MAX_H] or not inside frames_bytes: nothing is loaded, stats 0
 *   FP_QUALITY_EMPTY         the clamped rectangle holds no pixel: stats 0
 *   FP_QUALITY_TOO_LARGE     s > FP_QUALITY_MAX_STEP: stats 0 (at s = 64, sum L^2 <= (4 * 255 * 64^2)^2 * 110^2 < 2^63)
 *   FP_QUALITY_NO_LAPLACIAN  bw < 3 or bh < 3: the three Laplacian fields are 0 (bw or bh = 0: the whole row is)
 * The first three exclude each other and the fourth.  One workgroup per face, integer arithmetic, no atomics: two runs are
 * bit-identical.  Stream-ordered, allocates nothing.  Refusals before any launch (FP_ERR_INVALID_ARG): a NULL pointer, a
 * negative count.  n == 0: FP_OK, nothing launched.  Trust boundary as fp_resize_ragged: descs and items are device memory the
 * host does not read; the kernel never loads outside frames_bytes.
 *
 * Pose: lmarks [n][10] fp32 and fmt as fp_dets_to_crops_aligned writes and takes them (fmt 0: eyes, nose, mouth centre, slots
 * 8, 9 unused; fmt 1, 2: eyes, nose, mouth corners).  With le, re the eyes, e = re - le, mouth the mouth centre (fmt 0) or the
 * midpoint of its corners, mid the midpoint of the eyes and v = (-e.y, e.x) (e turned by +90 degrees: down the face), in fp32
 * with + - * / and sqrtf only, every point taken relative to le first:
 *   out[i] = (iod = |e|,  roll = e.y / iod,  yaw = 2 ((nose - le) . e) / iod^2 - 1,  pitch = ((nose - mid) . v) / ((mouth - mid) . v))
 * FP_QUALITY_POSE_DEGENERATE is OR-ed into flags[i] and out[i] = 0 when iod < 1 or the pitch denominator is <= 0 (or either is
 * not a number).  One lane per face.  Refusals: a NULL pointer, n < 0, fmt outside 0 .. 2 (FP_ERR_INVALID_ARG).
 * The *_emulate forms run the same code serially on HOST memory (every pointer HOST) and give the same bits.
 */
#define FP_QUALITY_MAX_STEP 64
#define FP_QUALITY_EMPTY 1
#define FP_QUALITY_BAD_FRAME 2
#define FP_QUALITY_NO_LAPLACIAN 4
#define FP_QUALITY_TOO_LARGE 8
#define FP_QUALITY_POSE_DEGENERATE 16
int fp_face_quality(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs /*device*/, int n_frames,
                    const fp_resize_item* items /*device*/, int n, int64_t* stats /* n x 8 */, int32_t* flags, void* stream);
int fp_face_quality_emulate(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames,
                            const fp_resize_item* items, int n, int64_t* stats, int32_t* flags);
int fp_face_pose(const float* lmarks /* n x 10 */, int fmt, int n, float* out /* n x 4 */, int32_t* flags /* OR-ed into */,
                 void* stream);
int fp_face_pose_emulate(const float* lmarks, int fmt, int n, float* out, int32_t* flags);

/*
 * Tiled detection (build-defined, no reference counterpart; DESIGN §7 "Tiled detection"; csrc/tilemerge.hip).  A detector
 * that sees a frame through one letterbox loses small faces; tiling.py runs it on overlapping tiles of every frame and on
 * the whole frame.  Each such image is a VIEW of its frame.  All additive: ABI 14.
 *
 * fp_tile_view, 32 bytes: frame = index into descs; (x0, y0) = the view's origin in the frame; vw x vh = the part of the
 * view's image that holds frame pixels (a tile larger than its frame: the frame's size); gain, pad_x, pad_y = the
 * scale_coords values (modules/utils/image.py) of the image the detector was given (tile_w x tile_h for a tile, the frame
 * for a whole-frame view) against the detector's input size.  The views of one frame are contiguous: frame f owns
 * views[view_start[f] .. view_start[f + 1]), and dets [S][max_dets][row_floats] / counts [S] are the detector's rows of the
 * views in the same order (fmt 0: BlazeFace rows, row_floats >= 17; fmt 1: YOLOv5-face rows with landmarks, >= 15).
 *
 * fp_merge_views: one workgroup per frame, all arithmetic fp32 in the written order, no contraction.
 *   1. Every row r < min(max(counts[s], 0), max_dets) of every view s of the frame is a candidate, in (view, row) order; only
 *      the first FP_MERGE_CAP are taken (overflow[f] |= 2 when there were more).  Model-input coordinates c as
 *      fp_dets_to_crops takes them: fmt 0 column * in_w / in_h with the (y, x) column swap, fmt 1 as stored.
 *   2. View pixels: v = (c - pad) / gain.
 *   3. Cut rule.  A view edge is interior when it is not the frame's: x0 > 0, x0 + vw < W, y0 > 0, y0 + vh < H.  With
 *      edge_px >= 0 a candidate is dropped when v_x1 <= edge_px at an interior left edge, v_x2 >= vw - edge_px at an interior
 *      right edge, and the same in y.  Frame edges never cut; a whole-frame view has no interior edge; edge_px < 0: no cut.
 *   4. The box is clamped to [0, vw] x [0, vh], then (float)x0, (float)y0 are added.  Landmarks take v = (c - pad) / gain +
 *      origin, unclamped and unrounded: fmt 1 landmark i -> slot i; fmt 0 keypoints 0, 1, 2 -> slots 0, 1, 2, keypoint 3 (the
 *      mouth centre) -> slots 3 AND 4, the ears are dropped.
 *   5. Dropped: a candidate whose score or unclamped view box is not finite, and one with x2 <= x1 or y2 <= y1.
 *   6. Order: score descending (-0 counts as +0), then view ascending, then row ascending.
 *   7. Greedy hard suppression: walking in that order, a candidate c is kept unless an earlier kept box k has
 *      inter > merge_thr * fminf(area_k, area_c), inter = max(min(x2) - max(x1), 0) * max(min(y2) - max(y1), 0):
 *      intersection over the SMALLER area.  merge_thr = +inf suppresses nothing.
 *   8. Kept rows go to out [B][max_out][16] in walk order = x1, y1, x2, y2, (x, y) x 5, score @ 14, 0: the fmt-2 row of
 *      fp_dets_to_crops_px, in the frame's own pixels.  out_counts[f] = rows written (at most max_out; overflow[f] |= 4
 *      when more were kept); rows behind the count are not written.  overflow [B] is OR-ed into: the caller presets it
 *      (0, or 1 where the detector cut a view of the frame at its own cap).
 * No global atomics, no workspace; two runs are bit-identical.  Refusals before any launch (FP_ERR_INVALID_ARG): a NULL
 * pointer, fmt other than 0 / 1, a row too short for its format, max_dets, max_out, in_w or in_h < 1, a NaN merge_thr,
 * B < 0 or S < 0.  B == 0: FP_OK, nothing launched.  views, view_start, counts and descs are device memory the host does
 * not read: the kernel clamps view ranges to [0, S] and row counts to max_dets and writes nothing outside out[f].
 * fp_merge_views_emulate: the same code serially on HOST memory (every pointer HOST), the same bits.
 *
 * fp_gather_tiles: out [S][tile_h][tile_w][3] u8 <- the rectangle (x0, y0, vw, vh) of every view's frame at the tile's top
 * left, every other byte 125 (the letterbox pad value); either kind of batch (a dense batch is n_frames equal descriptors),
 * one launch.  A view whose frame index, descriptor or origin is unusable becomes all 125.  Refusals: a NULL pointer,
 * n_frames < 1, S < 0, a tile size outside 1 .. FP_FRAME_MAX_W x 1 .. FP_FRAME_MAX_H (FP_ERR_INVALID_ARG).  S == 0: FP_OK.
 */
typedef struct fp_tile_view {
  int32_t frame;
  int32_t x0, y0, vw, vh;
  float gain, pad_x, pad_y;
} fp_tile_view;              /* 32 bytes */
#define FP_MERGE_CAP 2048
int fp_merge_views(const float* dets, const int32_t* counts, int S, int max_dets, int row_floats, int fmt, int in_w, int in_h,
                   const fp_tile_view* views, const int32_t* view_start /* B + 1 */, const fp_frame_desc* descs, int B,
                   float merge_thr, float edge_px, int max_out, float* out, int32_t* out_counts, int32_t* overflow,
                   void* stream);
int fp_merge_views_emulate(const float* dets, const int32_t* counts, int S, int max_dets, int row_floats, int fmt, int in_w,
                           int in_h, const fp_tile_view* views, const int32_t* view_start, const fp_frame_desc* descs, int B,
                           float merge_thr, float edge_px, int max_out, float* out, int32_t* out_counts, int32_t* overflow);
int fp_gather_tiles(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs /*device*/, int n_frames,
                    const fp_tile_view* views /*device*/, int S, int tile_w, int tile_h, uint8_t* out, void* stream);

/*
 * Tracklets (build-defined, no reference counterpart; DESIGN §7 "Tracklets"; csrc/tracklets.hip): faces tracked across the
 * frames of many streams, one launch per step, nothing read back.  fp_tracker_step stays the port of the reference's
 * per-frame first-match rule; this is the batched tracker of the pipeline's 256-frame steps (256 frames of one video, one
 * frame of each of 256 cameras, or any mix).  All additive: ABI 14.
 *
 * State, owned by the caller (fp_track_state: five arrays, zero-filled except next_id = 1 for a fresh tracker), per stream s:
 *   hdr      [S][2] int32                       clock (frames processed so far), next_id (starts at 1)
 *   slot_i   [S][FP_TRACK_SLOTS][5] int32       id (0 = free), first_clock, last_clock, hits, best_clock
 *   slot_f   [S][FP_TRACK_SLOTS][10] fp32       last box x1 y1 x2 y2, inverse norm of the last embedding, best_score,
 *                                               best box x1 y1 x2 y2
 *   emb      [S][FP_TRACK_SLOTS][D] fp32        last embedding;    best_emb likewise: the best row's embedding
 * Inputs of a step: n face rows -- frame[i] (index into the batch), box[i] (4 fp32), emb [n][D] fp32, xinv[i] =
 * fp_row_inv_norm(emb), score[i] (NULL: every score is 0) -- and stream_of_frame [B] (-1: the frame is not tracked).  A row is
 * LIVE when xinv is finite and > 0 (the rule of fp_cosine_dbscan_x6 and fp_pair_histogram_x6).  Frames of one stream are
 * processed in ascending batch index, the rows of a frame in row order (they need not be contiguous); streams are independent.
 * A row's POSITION is its rank among the rows of its frame, dead rows included; rows at positions >= FP_TRACK_MAX_DETS take
 * no part (flag OVER).  For each frame of stream s, all arithmetic fp32 in the written order, no contraction:
 *   1. clock += 1; every slot with clock - last_clock > max_age is freed.
 *   2. For every live track t and every live detection d: c = (dot(emb_t, emb_d) * inv_t) * inv_d (the order of the dot
 *      product's additions is the kernel's own: the device and the emulator share it, another implementation agrees wherever
 *      no c lies within D * 2^-24 of a threshold or of another c).  With min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b
 *      and a the track's value: iw = min(x2) - max(x1), ih likewise; if not (iw > 0 and ih > 0) iou = 0, else inter = iw * ih,
 *      iou = inter / ((area_t + area_d) - inter), area = (x2 - x1) * (y2 - y1).  The pair is admissible when
 *      (c > tau_near && iou > iou_min) || c > tau_far; comparisons with NaN are false.
 *   3. Admissible pairs in the order c descending (-0 counts as +0), then lower slot, then lower position; walking them, a pair
 *      is taken when its track and its detection are both still free.  A match rewrites the slot's last box, last embedding
 *      and inverse norm, sets last_clock = clock and increments hits.
 *   4. Every live detection left unmatched, in row order, opens a track in the lowest free slot: id = next_id++, hits = 1,
 *      first_clock = last_clock = clock.  No free slot: the row gets id 0 and FP_TRACK_FULL.  (A track opened in a frame is
 *      not matched in that frame.)
 *   5. A matched row whose score is strictly greater than the slot's best_score, and every opening row, becomes the track's
 *      best: best_score, best_clock, best box and best_emb are rewritten and the row gets FP_TRACK_BEST.
 * Per-row outputs: track_id (0: none), track_hits (the slot's hits after the row; 0 without an id), track_clock (the
 * stream's clock at the row's frame; 0 for NO_STREAM) and track_flags: NEW, BEST, DEAD_ROW (a row that is not live), FULL,
 * NO_STREAM (frame[i] outside [0, B), or its stream -1 or outside [0, n_streams)), OVER.  DEAD_ROW, FULL, NO_STREAM and OVER
 * rows change no state; an OVER row is flagged OVER alone.
 * The defaults of tracking.py restate the reference's thresholds (fp_tracker_step) for unit vectors through
 * cos = 1 - dist^2 / 2: dist < 1.0 with IoU > 0.1 -> tau_near = 0.5, iou_min = 0.1; dist < 0.72 alone -> tau_far = 0.7408.
 * They are the reference's numbers, unmeasured on real video.  max_age has no reference counterpart and no default.
 *
 * fp_tracklets_step: one launch, one workgroup per stream (one whose stream has no frame in the step leaves at once); no
 * global atomics, no workspace, no host synchronisation; two runs are bit-identical.  Every pointer but `state` itself (a
 * HOST struct of device pointers) is device memory the host does not read.  Refusals before any launch (FP_ERR_INVALID_ARG): a
 * NULL state or state array, n_streams < 1, D not a multiple of 4, D < 4 or D > FP_TRACK_MAX_DIM, n < 0 or n >
 * FP_TRACK_MAX_ROWS, B < 0, max_age < 0, a NULL stream_of_frame with B > 0, a NULL row input or output with n > 0, emb or a
 * state embedding array not 16-byte aligned, tau_far < tau_near or a NaN threshold.  B == 0 and n == 0: FP_OK, nothing launched;
 * frames without rows still advance their stream's clock.
 * fp_tracklets_step_emulate: the same decision code serially on HOST memory (every pointer HOST), the same bits.
 */
#define FP_TRACK_SLOTS 64
#define FP_TRACK_MAX_DETS 64
#define FP_TRACK_MAX_DIM 1024
#define FP_TRACK_MAX_ROWS (1 << 30)
#define FP_TRACK_SLOT_INTS 5
#define FP_TRACK_SLOT_FLOATS 10
#define FP_TRACK_NEW 1
#define FP_TRACK_BEST 2
#define FP_TRACK_DEAD_ROW 4
#define FP_TRACK_FULL 8
#define FP_TRACK_NO_STREAM 16
#define FP_TRACK_OVER 32
typedef struct fp_track_state {
  int32_t* hdr;
  int32_t* slot_i;
  float* slot_f;
  float* emb;
  float* best_emb;
} fp_track_state;
int fp_tracklets_step(const fp_track_state* state /*host struct*/, int n_streams, int D, const int32_t* frame, const float* box,
                      const float* emb, const float* xinv, const float* score /* or NULL */, int n,
                      const int32_t* stream_of_frame /* B */, int B, int max_age, float tau_near, float tau_far, float iou_min,
                      int32_t* track_id, int32_t* track_hits, int32_t* track_clock, int32_t* track_flags, void* stream);
int fp_tracklets_step_emulate(const fp_track_state* state, int n_streams, int D, const int32_t* frame, const float* box,
                              const float* emb, const float* xinv, const float* score, int n, const int32_t* stream_of_frame,
                              int B, int max_age, float tau_near, float tau_far, float iou_min, int32_t* track_id,
                              int32_t* track_hits, int32_t* track_clock, int32_t* track_flags);

/*
 * Tracklets: motion prediction (build-defined; DESIGN §7 "Tracklets: motion prediction"; csrc/tracklets.hip,
 * tracklets_kernel<true, REID>).  Opt-in: fp_tracklets_step and its state are untouched.  All additive: ABI 14.
 *
 * Each slot carries four independent two-state filters, one per coordinate c of the centre form (cx, cy, w, h): the
 * decomposition that DeepSORT's 8-state constant-velocity filter has anyway, its covariance never couples two coordinates.  Per
 * slot and coordinate five fp32 values x, v, p00, p01, p11 (position, velocity per frame, covariance), in that order,
 * coordinate after coordinate: a caller-owned state array
 *   motion   [S][FP_TRACK_SLOTS][FP_TRACK_MOTION_FLOATS = 20] fp32, zero-filled for a fresh tracker.
 * Two parameters, std_pos and std_vel, both finite and > 0: noise as a fraction of the box height.  All arithmetic fp32, one
 * rounding per written operation, in the written order.
 *   Measurement of a box.  z = (0.5f*(x1+x2), 0.5f*(y1+y2), x2-x1, y2-y1).
 *   Scale.  hs(t) = t > 1.f ? t : 1.f (a NaN gives 1).
 *   Init (a row opens a track; re-init below).  With H = hs(z_h): x = z, v = 0, p01 = 0, p00 = (2*std_pos*H)*(2*std_pos*H),
 *     p11 = (10*std_vel*H)*(10*std_vel*H).
 *   Predict: step 1b, in every frame of the stream, after expiry, for every live slot, whether or not the frame has rows.
 *     H = hs(x_h), read before any coordinate of the slot is advanced; q0 = (std_pos*H)*(std_pos*H), q1 = (std_vel*H)*(std_vel*H).
 *     Per coordinate, in this order: x = x + v; a = p01 + p11; p00 = ((p00 + p01) + a) + q0; p01 = a; p11 = p11 + q1.
 *     The predicted box: pw = w > 0 ? w : 0, ph likewise; x1 = cx - 0.5f*pw, x2 = cx + 0.5f*pw, y1 = cy - 0.5f*ph, y2 = cy + 0.5f*ph.
 *   Gate: step 2 takes its IoU with the predicted box where it took the last box.  Nothing else of steps 2-5 changes: the
 *     admissibility rule, the key, the greedy walk, openings and best shot stay; slot_f's last box still receives the detection's.
 *   Update, on a match, beside the slot rewrite.  H = hs(x_h) after this frame's prediction, r = (std_pos*H)*(std_pos*H).  Per
 *     coordinate, the old p00 and p01 on the right-hand sides: s = p00 + r, k0 = p00/s, k1 = p01/s, y = z - x; x = x + k0*y,
 *     v = v + k1*y; p11 = p11 - k1*p01, p01 = p01 - k1*p00, p00 = p00 - k0*p00.  If afterwards any of the slot's eight x, v values
 *     fails t - t == 0, the slot is re-initialised from z as at opening.
 *   Coasting.  Unmatched tracks keep their predicted state.
 * New per-row output: track_pred [n][4] fp32, the predicted box the matched track had in that frame; every row that is not a
 * match (an opening row, DEAD_ROW, FULL, NO_STREAM, OVER) gets four zeros.
 * Out of scope: emitting rows for coasting tracks, Mahalanobis gating, camera-motion compensation, and any measured value of
 * std_pos / std_vel (tracking.ConstantVelocity names DeepSORT's published 1/20 and 1/160, unmeasured here).
 *
 * fp_tracklets_step_motion: fp_tracklets_step's launch shape and promises (one launch, one workgroup per stream; the filters and
 * the predicted boxes in LDS; no global atomics, no scratch, no host synchronisation); a workgroup whose stream owns no frame
 * leaves without touching motion.  Refusals before any launch: everything fp_tracklets_step refuses, a NULL motion, a NULL
 * track_pred with n > 0, a std_pos or std_vel that is not finite and > 0.
 * fp_tracklets_step_motion_emulate: the same filter code serially on HOST memory (every pointer HOST), the same bits.
 */
#define FP_TRACK_MOTION_FLOATS 20
int fp_tracklets_step_motion(const fp_track_state* state /*host struct*/, int n_streams, int D, const int32_t* frame,
                             const float* box, const float* emb, const float* xinv, const float* score /* or NULL */, int n,
                             const int32_t* stream_of_frame /* B */, int B, int max_age, float tau_near, float tau_far,
                             float iou_min, int32_t* track_id, int32_t* track_hits, int32_t* track_clock, int32_t* track_flags,
                             float* motion, float std_pos, float std_vel, float* track_pred /* n x 4 */, void* stream);
int fp_tracklets_step_motion_emulate(const fp_track_state* state, int n_streams, int D, const int32_t* frame, const float* box,
                                     const float* emb, const float* xinv, const float* score, int n,
                                     const int32_t* stream_of_frame, int B, int max_age, float tau_near, float tau_far,
                                     float iou_min, int32_t* track_id, int32_t* track_hits, int32_t* track_clock,
                                     int32_t* track_flags, float* motion, float std_pos, float std_vel, float* track_pred);

/*
 * Tracklets: re-identification (build-defined; DESIGN §7 "Tracklets: re-identification"; csrc/tracklets.hip,
 * tracklets_kernel<MOTION, true>).  Opt-in: fp_tracklets_step, fp_tracklets_step_motion and their state are untouched.  All
 * additive: ABI 15.
 *
 * A track that expires is PARKED instead of dropped, and a face that no live track takes is compared with the parked tracks of
 * its stream before it opens a new one: a returning face gets its old id back.  Two parameters: tau_reid, a cosine (finite),
 * and lost_age > max_age, the number of frames after its last sighting for which a track is remembered.  Neither has a default:
 * nothing has been measured on real video.
 * State, owned by the caller beside the five arrays of "Tracklets" (fp_track_lost: five more, zero-filled for a fresh
 * tracker), per stream s a ring of FP_TRACK_LOST = 64 entries; a parked track is literally its slot row:
 *   lost_hdr      [S][2] int32                       ring head (used modulo FP_TRACK_LOST), spare
 *   lost_i        [S][FP_TRACK_LOST][5] int32        the slot's slot_i row (id 0 = empty entry)
 *   lost_f        [S][FP_TRACK_LOST][10] fp32        the slot's slot_f row
 *   lost_emb      [S][FP_TRACK_LOST][D] fp32         the slot's last embedding;  lost_best_emb likewise: its best row's
 * Per frame of stream s, numbered against the steps of "Tracklets":
 *   1a. After clock += 1, every entry with id != 0 and clock - last_clock > lost_age is emptied (id = 0).
 *   1.  The slots that expire (clock - last_clock > max_age) are parked, then freed: in ascending slot order the r-th of them goes
 *       to entry (head + r) % 64, then head = (head + count) % 64.  The entry receives the slot's slot_i and slot_f rows, emb[slot]
 *       and best_emb[slot]; what it held is overwritten (it is the oldest parked track).  A track parked in a frame can be revived
 *       in that same frame.
 *   2, 3. Unchanged (with motion, 1b too: a parked track has no filter).
 *   3b. For every live detection d that the walk of step 3 left unmatched and every entry e with id != 0 whose stored inverse
 *       norm is live: c = (dot(lost_emb_e, emb_d) * inv_e) * inv_d, the dot product in step 2's order; inv_e is the parked row's
 *       inverse norm, so the pool compares LAST embeddings (a slot keeps no norm for best_emb).  The pair is admissible when
 *       c > tau_reid (false for a NaN); there is no IoU gate, the person has moved.  Admissible pairs in the order of step 3 (c
 *       descending, then lower entry, then lower position), walked the same greedy one-to-one way.
 *   4.  Every live detection that step 3 left unmatched, revived or not, takes the lowest free slot by its rank among them in row
 *       order, as before; one without a free slot gets id 0 and FP_TRACK_FULL, and the entry it had taken stays parked.  A
 *       revived detection with a slot: the slot's slot_i and slot_f rows become the entry's (id, first_clock, hits, best_score,
 *       best_clock and the best box continue), the entry is emptied, and the slot is then rewritten as by a match (hits + 1,
 *       last_clock, last box, inverse norm, last embedding).  Step 5 holds for it as for a match: FP_TRACK_BEST only when score
 *       is strictly greater than the carried best_score, otherwise best_emb[slot] = lost_best_emb[entry].  Its flags gain
 *       FP_TRACK_REVIVED and never FP_TRACK_NEW.  next_id advances for true openings only: the k-th opening detection of the
 *       frame, in row order, gets id next_id + k.
 *   Motion.  With a motion array a revived slot's filters are initialised from the detection's box as at an opening, and its
 *       track_pred row is zeros.
 * As for the parent: a step equals the same frames split anywhere, interleaved streams equal each stream alone, scattered rows
 * equal contiguous rows, two runs are bit-identical; the device and the emulator share every bit, another implementation agrees
 * wherever no c of step 2 or 3b lies within D * 2^-24 of its threshold or of another c.
 * Out of scope: re-identification across streams, pools of more than 64 tracks, a best-shot descriptor in place of the last
 * embedding, and any measured value of tau_reid / lost_age.
 *
 * fp_tracklets_step_reid: fp_tracklets_step's launch shape and promises (one launch, one workgroup per stream; the pool's rows in
 * LDS beside the slot table; no global atomics, no scratch, no host synchronisation).  Step 3b runs only in a frame that has
 * both an unmatched live detection and a parked track.  motion NULL: the kernel of fp_tracklets_step plus the pool (std_pos,
 * std_vel are ignored, track_pred must be NULL); motion not NULL: that of fp_tracklets_step_motion plus the pool.  Refusals before
 * any launch: everything fp_tracklets_step (with motion: fp_tracklets_step_motion) refuses, a NULL lost or pool array, a pool
 * embedding array not 16-byte aligned, lost_age <= max_age, a tau_reid that is not finite, a track_pred without motion.
 * fp_tracklets_step_reid_emulate: the same decision code serially on HOST memory (every pointer HOST), the same bits.
 */
#define FP_TRACK_LOST 64
#define FP_TRACK_REVIVED 64
typedef struct fp_track_lost {
  int32_t* lost_hdr;
  int32_t* lost_i;
  float* lost_f;
  float* lost_emb;
  float* lost_best_emb;
} fp_track_lost;
int fp_tracklets_step_reid(const fp_track_state* state /*host struct*/, const fp_track_lost* lost /*host struct*/, int n_streams,
                           int D, const int32_t* frame, const float* box, const float* emb, const float* xinv,
                           const float* score /* or NULL */, int n, const int32_t* stream_of_frame /* B */, int B, int max_age,
                           float tau_near, float tau_far, float iou_min, int32_t* track_id, int32_t* track_hits,
                           int32_t* track_clock, int32_t* track_flags, float tau_reid, int lost_age, float* motion /* or NULL */,
                           float std_pos, float std_vel, float* track_pred /* n x 4, NULL iff motion is */, void* stream);
int fp_tracklets_step_reid_emulate(const fp_track_state* state, const fp_track_lost* lost, int n_streams, int D,
                                   const int32_t* frame, const float* box, const float* emb, const float* xinv,
                                   const float* score, int n, const int32_t* stream_of_frame, int B, int max_age, float tau_near,
                                   float tau_far, float iou_min, int32_t* track_id, int32_t* track_hits, int32_t* track_clock,
                                   int32_t* track_flags, float tau_reid, int lost_age, float* motion, float std_pos,
                                   float std_vel, float* track_pred);

/*
 * Tracklets: templates (build-defined; DESIGN §7 "Tracklets: templates"; csrc/trackpool.hip).  Opt-in: the tracker kernels,
 * their state and every result of theirs are untouched.  All additive; FP_ABI_VERSION stays 15.
 *
 * A TEMPLATE sums up a sighting: the weighted sum of the normalised embeddings of every row of a track, kept per stream on the
 * device and handed back with every row, so that a gallery search can ask "who is this track" instead of "who is this row".
 * The entry points take the tracker's per-row results as DATA and read nothing of the tracker's state.
 * State, owned by the caller (fp_track_templates: three arrays, zero-filled for a fresh table), per stream s a table of
 * FP_TRACK_POOL = 128 entries (FP_TRACK_SLOTS + FP_TRACK_LOST: one for every live and every parked track):
 *   tpl_i    [S][FP_TRACK_POOL][3] int32     id (0 = free), last_clock, rows
 *   tpl_w    [S][FP_TRACK_POOL] fp32         the sum of the weights of the rows that were added
 *   tpl_sum  [S][FP_TRACK_POOL][D] fp32      the sum itself
 * Inputs of a step: frame, emb, xinv, stream_of_frame, B as for "Tracklets"; track_id, track_clock, track_flags as
 * fp_tracklets_step* wrote them (or crafted); weight [n] fp32, or NULL for 1.0 everywhere; keep >= 0, the clocks an entry
 * outlives its last row (the tracker's lost_age with re-identification, else its max_age).
 * Order: the rows of a stream in the tracker's order -- its frames in ascending batch index, the rows of a frame in row order
 * (they need not be contiguous); streams are independent.  A row TAKES PART when its frame has a stream (frame[i] in [0, B),
 * stream_of_frame in [0, n_streams)) and track_id[i] > 0.  For such a row, with c = track_clock[i]:
 *   1. The entry of the stream whose id is track_id[i] is looked up (the lowest index, should a crafted table hold it twice).
 *   2. Found, and the row carries FP_TRACK_NEW: the id is being given out again; the entry is cleared (5) and reused.
 *   3. Not found: the lowest-index entry that is free (id 0) or stale (c - last_clock > keep, in 64-bit integers) is taken.
 *   4. None free or stale: the entry with the smallest last_clock is taken, the lowest index on ties, and the row is flagged
 *      FP_TRACK_TPL_EVICTED.
 *   5. An entry cleared or taken: rows = 0, its weight sum and its D sums = +0, id = track_id[i].
 *   6. A row that is neither NEW nor found is flagged FP_TRACK_TPL_RESTART: the track goes on, its template starts again.
 *   7. w = weight[i] if that is finite and > 0, else 0 (NULL weight: 1).
 *   8. If w > 0: for every j, sum[j] = sum[j] + ((emb[i][j] * xinv[i]) * w) -- fp32, three roundings, in that order, no
 *      contraction --, the weight sum = the weight sum + w, rows += 1.
 *   9. last_clock = c, whether or not the row added.
 * Per-row outputs: track_emb[i] [D] = the entry's sum after the row (unnormalised: nothing divides, a cosine does not mind the
 * scale); track_emb_rows[i] = the entry's rows after the row; track_emb_flags[i] (TPL_EVICTED, TPL_RESTART).  A row that does
 * not take part, or whose entry has rows == 0 after it, gets its own emb[i] bit for bit and track_emb_rows = 0 (a face without a
 * track is its own template, a dead row stays dead for a search); a row that does not take part has flags 0.
 * There is no reduction: the device, the host twin and numpy float32 share every bit of every output and of the state.  (One
 * exception no caller meets through the tracker: where a sum turns NaN, all three hold a NaN, of the machine's own sign and
 * payload.)  A step equals the same frames split anywhere with the state carried; two runs are bit-identical.
 * Out of scope: decaying or windowed templates, vote ledgers, templates across streams, tables of more than 128 entries, and
 * any measured value of `weight` or `keep`, or of the gain on real video.
 *
 * fp_track_pool_step: two launches, nothing read back, no global atomics.  The directory launch, one wave per stream and
 * integers only, resolves every row's entry and flags and writes, per (stream, entry) SEGMENT -- a run of rows on one entry
 * between two clearings; an entry evicted in the middle of a step yields two --, the ordered list of its rows to the workspace.
 * The accumulate launch runs one workgroup of D / 4 lanes per touched entry, a float4 of the running sum in each lane's
 * registers along its segments; tpl_sum is read at most once and written once per touched entry.  workspace: device memory of
 * fp_track_pool_workspace_bytes(n) bytes, 4-byte aligned, contents irrelevant before and after.  Every pointer but `tpl` itself
 * (a HOST struct of device pointers) is device memory the host does not read.  Refusals before any launch
 * (FP_ERR_INVALID_ARG): a NULL tpl or table array, n_streams < 1, D not a multiple of 4, D < 4 or D > FP_TRACK_MAX_DIM, n < 0
 * or n > FP_TRACK_MAX_ROWS, B < 0, keep < 0, a NULL stream_of_frame with B > 0, a NULL row input or output with n > 0 (weight
 * may be NULL), emb, track_emb or tpl_sum not 16-byte aligned, with n > 0 a NULL or too small workspace.  n == 0: FP_OK, nothing
 * launched, nothing changed (a frame without rows moves no template).  B == 0 with n > 0: every row passes through.
 * fp_track_pool_step_emulate: the same tests and the same arithmetic serially on HOST memory (every pointer HOST), the same bits.
 */
#define FP_TRACK_POOL 128
#define FP_TRACK_TPL_EVICTED 1
#define FP_TRACK_TPL_RESTART 2
typedef struct fp_track_templates {
  int32_t* tpl_i;
  float* tpl_w;
  float* tpl_sum;
} fp_track_templates;
size_t fp_track_pool_workspace_bytes(int n);
int fp_track_pool_step(const fp_track_templates* tpl /*host struct*/, int n_streams, int D, const int32_t* frame, const float* emb,
                       const float* xinv, const float* weight /* or NULL */, int n, const int32_t* stream_of_frame /* B */, int B,
                       const int32_t* track_id, const int32_t* track_clock, const int32_t* track_flags, int keep,
                       float* track_emb /* n x D */, int32_t* track_emb_rows, int32_t* track_emb_flags, void* workspace,
                       size_t workspace_bytes, void* stream);
int fp_track_pool_step_emulate(const fp_track_templates* tpl, int n_streams, int D, const int32_t* frame, const float* emb,
                               const float* xinv, const float* weight, int n, const int32_t* stream_of_frame, int B,
                               const int32_t* track_id, const int32_t* track_clock, const int32_t* track_flags, int keep,
                               float* track_emb, int32_t* track_emb_rows, int32_t* track_emb_flags);

/*
 * Tracker evaluation: CLEAR-MOT and IDF1 (build-defined, the reference calls no tracking scorer; DESIGN §7 "Tracker
 * evaluation"; csrc/moteval.hip; tracking_eval.py holds the numpy restatement and the host half).  All additive: ABI 14.
 *
 * Inputs.  Ground-truth rows (seq, frame, id, box xywh) and hypothesis rows (seq, frame, id, box xywh); n_seqs, n_frames[seq]
 * and one IoU threshold thr (default 0.5).  One class, no ignore regions, no distractors.  Ids are arbitrary integers: Python
 * remaps them to dense 0 .. G_s - 1 / 0 .. H_s - 1 per sequence.  An id twice in one frame of one sequence, or more than
 * FP_MOT_MAX_ROWS = 64 ground-truth rows or hypothesis rows in one frame of one sequence, is refused in Python (ValueError);
 * 64 is the wave width and the tracker's FP_TRACK_MAX_DETS.
 * Order.  Sequences are independent.  The frames of a sequence run 0 .. n_frames - 1 in ascending order, every frame
 * processed, the empty ones too.  Inside a frame the rows keep the caller's relative order (stable sort by (seq, frame)); a
 * row's POSITION is its rank in that order.
 * State.  Per ground-truth id g: last[g] (hypothesis id of its most recent match ever, or none), cur[g] (the hypothesis id it
 * was matched to in the previous frame of the sequence, or none), counters seen[g], hit[g], runs[g].  Per sequence: TP, FN,
 * FP, IDSW (int64), sum_iou (fp64), pot[G_s][H_s] (int32).
 * Per frame, with n ground-truth rows and m hypothesis rows:
 *   1. sim[i][j] = IoU in fp64: iw = min(ax + aw, bx + bw) - max(ax, bx), ih likewise; 0 if iw <= 0 or ih <= 0, else
 *      i = iw * ih, i / (aw * ah + bw * bh - i) -- the operations and order of evaluation._iou_matrix.  adm = sim >= thr.
 *   2. pot[g_i][h_j] += 1 for every admissible pair (all pairs, not one-to-one).
 *   3. score[i][j] = adm ? sim + (cur[g_i] == h_j ? 1000.0 : 0.0) : 0.0.
 *   4. Assignment: score padded with zeros to N x N, N = max(n, m); C = -score; the shortest-augmenting-path Hungarian
 *      method with potentials u, v in fp64, rows inserted in ascending order.  For row i: p[0] = i, j0 = 0, minv[] = inf,
 *      used[] = false; repeat { used[j0] = true; i0 = p[j0]; delta = inf; for the columns j = 1 .. N not used, ascending:
 *      cur = (C[i0][j] - u[i0]) - v[j]; if cur < minv[j]: minv[j] = cur, way[j] = j0; if minv[j] < delta: delta = minv[j],
 *      j1 = j (strict comparisons: the lowest column wins a tie); then for j = 0 .. N: used ? (u[p[j]] += delta, v[j] -= delta)
 *      : (minv[j] -= delta); j0 = j1 } until p[j0] == 0; then augment: repeat { j1 = way[j0]; p[j0] = p[j1]; j0 = j1 } until
 *      j0 == 0.  Matched pairs are the assigned (i, j) with i < n, j < m and score[i][j] > 0.
 *   5. For each matched pair in ascending ground-truth position: IDSW += (last[g] exists and last[g] != h); hit[g] += 1;
 *      runs[g] += (cur[g] was none before this frame); sum_iou += sim[i][j] (one fp64 addition per match, in this order).
 *   6. seen[g] += 1 for every ground-truth row; last[g] = h for matched rows; cur[] = none for every id of the sequence, then
 *      cur[g] = h for matched rows.
 *   7. TP += k, FN += n - k, FP += m - k, k = number of matches.
 * Per-row outputs: gt_match [n_gt] int32 = the index of the matched hypothesis row (in the order given to the call), -1
 * without one; gt_switch [n_gt] uint8.
 * Derived on the host in fp64 from the integers (tracking_eval.py): MOTA = (TP - FP - IDSW) / (TP + FN), MOTP = sum_iou / TP,
 * Frag = sum over g of max(runs[g] - 1, 0), MT / PT / ML from hit / seen (> 0.8; >= 0.2 and not MT; the rest) over ids with
 * seen > 0, precision, recall; IDTP = the maximum over one-to-one assignments of ground-truth ids to hypothesis ids of the
 * sequence of the sum of pot[g][h] (equal to the published IDFN + IDFP minimum: matching g with h saves 2 pot[g][h]);
 * IDFN = rows of ground truth - IDTP, IDFP = hypothesis rows - IDTP, IDF1 = IDTP / (IDTP + (IDFN + IDFP) / 2).  The combined
 * result sums the integers and sum_iou in sequence order, then derives.  -1 where a denominator is 0.
 * Known departures: parity with TrackEval / py-motmetrics is unpinned; every frame is processed (step 6 always runs, so a
 * target missed in a frame without any hypothesis starts a new run); admissibility is sim >= thr without an epsilon.  HOTA: below.
 *
 * fp_mot_match: one launch, one workgroup per sequence marching its frames; no global atomics, no scratch, no host
 * synchronisation; two runs are bit-identical.  A single long sequence is a chain of dependent frames: latency-bound.
 * Rows sorted by (sequence, frame), stable: gt_boxes [n_gt][4] fp64, gt_id [n_gt] int32 dense per sequence, gt_off
 * [n_frames + 1] int32 CSR over the global frame index frame_base[seq] + frame; hy_* likewise.  frame_base [n_seqs + 1] int32,
 * gt_id_base [n_seqs + 1] int32 (prefix sums of G_s), hy_id_count [n_seqs] int32 (H_s), pot_base [n_seqs + 1] int64 (prefix
 * sums of G_s * H_s); n_frames, n_gt_ids, n_pot: their last entries, as host integers.  Outputs: counts [n_seqs][4] int64 =
 * TP, FN, FP, IDSW; sum_iou [n_seqs] fp64; gt_match, gt_switch.  workspace (fp_mot_match_workspace(n_gt_ids, n_pot) bytes,
 * zeroed here) is an output too: six int32 rows of n_gt_ids entries -- last + 1, cur, the stamp of cur, seen, hit, runs --
 * and behind them pot, n_pot int32.  Every pointer is device memory the host does not read.  Indices read from device
 * memory are clamped into the arrays.  Refusals (FP_ERR_INVALID_ARG): a NULL pointer that is needed, a negative count, 2^31
 * or more rows, ids or frames, a NaN thr, a workspace that is too small; FP_ERR_ALIGNMENT: an fp64 / int64 array not 8-byte
 * aligned, an int32 array not 4-byte aligned.
 * fp_mot_match_emulate: the same decision code serially on HOST memory (every pointer HOST), the same bits.
 */
#define FP_MOT_MAX_ROWS 64
size_t fp_mot_match_workspace(int64_t n_gt_ids, int64_t n_pot);
int fp_mot_match(const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt, const double* hy_boxes,
                 const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy, const int32_t* frame_base,
                 const int32_t* gt_id_base, const int32_t* hy_id_count, const int64_t* pot_base, int n_seqs, int64_t n_frames,
                 int64_t n_gt_ids, int64_t n_pot, double thr, int64_t* counts, double* sum_iou, int32_t* gt_match,
                 uint8_t* gt_switch, void* workspace, size_t ws_bytes, void* stream);
int fp_mot_match_emulate(const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt,
                         const double* hy_boxes, const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy,
                         const int32_t* frame_base, const int32_t* gt_id_base, const int32_t* hy_id_count,
                         const int64_t* pot_base, int n_seqs, int64_t n_frames, int64_t n_gt_ids, int64_t n_pot, double thr,
                         int64_t* counts, double* sum_iou, int32_t* gt_match, uint8_t* gt_switch, void* workspace,
                         size_t ws_bytes);

/*
 * Tracker evaluation: HOTA (DetA, AssA, LocA; build-defined restatement of Luiten et al. 2020 as TrackEval computes it; DESIGN §7
 * "Tracker evaluation: HOTA"; csrc/hota.hip; tracking_eval.py holds the numpy restatement and the host half).  Parity with
 * TrackEval is unpinned: it is not installed.  All additive: ABI 15.
 *
 * Inputs.  Those of fp_mot_match (rows, n_frames, dense ids, at most FP_MOT_MAX_ROWS rows per side and frame, an id at most once
 * per frame) without thr; in its place alphas: fp64, strictly ascending, every value in (0, 1], 1 .. FP_HOTA_MAX_ALPHAS = 32 of
 * them (default in Python: numpy.arange(1, 20) / 20.0, passed as data).
 * Pass 1, alignment, frames ascending, every frame, with n ground-truth and m hypothesis rows:
 *   1. sim[i][j] = the fp64 IoU of fp_mot_match, the same operations and order.
 *   2. row[i] = sum of sim[i][0 .. m-1] in ascending j, one fp64 addition each, from 0.0; col[j] the same over ascending i.
 *   3. den = (row[i] + col[j]) - sim[i][j]; soft[i][j] = sim[i][j] > 0 ? sim[i][j] / den : 0.
 *   4. pmc[g_i][h_j] += soft[i][j] (one fp64 addition per pair and frame).   5. gtc[g_i] += 1, hyc[h_j] += 1.
 * After the last frame: gas[g][h] = pmc > 0 ? pmc / ((double(gtc[g]) + double(hyc[h])) - pmc) : 0.
 * Pass 2, matching, frames ascending again:
 *   1. score[i][j] = gas[g_i][h_j] * sim[i][j], one multiplication.
 *   2. The assignment of fp_mot_match (step 4 there) on C = -score padded with zeros to N x N; matched pairs are the assigned
 *      (i, j) with i < n, j < m, score > 0.
 *   3. Per ground-truth row: gt_match = the index of the matched hypothesis row (in the order given to the call) or -1; gt_sim =
 *      sim[i][j] of that pair or 0.0.
 *   4. Per sequence: levels[t] += 1 for each matched pair, t = the number of alphas with gt_sim >= alpha (no epsilon);
 *      n_gt += n, n_hy += m.
 * Derived on the host in fp64 per alpha a (tracking_eval.py): a pair counts iff gt_sim >= alphas[a]; TP = their number (= sum of
 * levels[t] over t > a), FN = n_gt - TP, FP = n_hy - TP, loc_sum = the sum of their gt_sim in ascending caller row order;
 * mc[(g, h)] = pairs per id pair (sparse); ass = mc / max(1, gtc[g] + hyc[h] - mc); ass_num / re_num / pr_num = the sums over id
 * pairs in ascending (g, h) of mc * ass, mc * mc / max(1, gtc[g]), mc * mc / max(1, hyc[h]); DetA = TP / (TP + FN + FP), DetRe,
 * DetPr, AssA = ass_num / TP, AssRe, AssPr, LocA = loc_sum / TP, HOTA = sqrt(DetA * AssA); headline numbers = means over the
 * alphas, LocA over the alphas with TP > 0.  The combined row sums TP, FN, FP and the numerators in sequence order, then derives.
 * Known departures: where TP == 0, AssA = AssRe = AssPr = 0 and LocA = -1 (TrackEval reports 1); -1 where a Det* denominator is 0.
 *
 * fp_hota_match: ONE launch, one workgroup of 256 threads per sequence: pass 1, the sweep pmc -> gas and pass 2, ordered by
 * workgroup barriers and fences; no global atomics, no scratch, no host synchronisation; two runs are byte-identical.  The row
 * arrays, CSR offsets, frame_base, gt_id_base and pot_base are those of fp_mot_match; hy_id_base [n_seqs + 1] int32 = prefix
 * sums of H_s, n_hy_ids its last entry.  alphas [n_alphas] is HOST memory (validated here, copied into the kernel arguments).
 * Outputs (device): gt_match [n_gt] int32, gt_sim [n_gt] fp64, levels [n_seqs][n_alphas + 1] int64, counts [n_seqs][2] int64 =
 * n_gt, n_hy.  workspace (fp_hota_match_workspace(n_gt_ids, n_hy_ids, n_pot) bytes, 8-byte aligned, zeroed here) is an output
 * too: gas, n_pot fp64, and behind it gtc [n_gt_ids] and hyc [n_hy_ids] int32.  Indices read from device memory are clamped
 * into the arrays.  Refusals as fp_mot_match, and FP_ERR_INVALID_ARG for alphas that are NULL, fewer than 1, more than 32, not
 * strictly ascending or outside (0, 1].
 * fp_hota_match_emulate: the same decision code serially on HOST memory (every pointer HOST), the same bits.
 */
#define FP_HOTA_MAX_ALPHAS 32
size_t fp_hota_match_workspace(int64_t n_gt_ids, int64_t n_hy_ids, int64_t n_pot);
int fp_hota_match(const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt, const double* hy_boxes,
                  const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy, const int32_t* frame_base,
                  const int32_t* gt_id_base, const int32_t* hy_id_base, const int64_t* pot_base, int n_seqs, int64_t n_frames,
                  int64_t n_gt_ids, int64_t n_hy_ids, int64_t n_pot, const double* alphas /* HOST */, int n_alphas,
                  int32_t* gt_match, double* gt_sim, int64_t* levels, int64_t* counts, void* workspace, size_t ws_bytes,
                  void* stream);
int fp_hota_match_emulate(const double* gt_boxes, const int32_t* gt_id, const int32_t* gt_off, int64_t n_gt,
                          const double* hy_boxes, const int32_t* hy_id, const int32_t* hy_off, int64_t n_hy,
                          const int32_t* frame_base, const int32_t* gt_id_base, const int32_t* hy_id_base,
                          const int64_t* pot_base, int n_seqs, int64_t n_frames, int64_t n_gt_ids, int64_t n_hy_ids,
                          int64_t n_pot, const double* alphas, int n_alphas, int32_t* gt_match, double* gt_sim, int64_t* levels,
                          int64_t* counts, void* workspace, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* FACEPATH_H */
