// align.hip — detections -> per-face crop rectangles, and five-point face alignment between detection and embedding
// (gfx950).  Build with -ffp-contract=off: boxes and landmarks follow numpy's operation order for float32 inputs and must
// not be contracted into fmas, and the host emulator must reproduce the device's records, estimate and samples bit for bit.
//
// 1. fp_dets_to_crops and its five siblings (_ragged, _aligned, _aligned_ragged, _px, _aligned_emulate): one kernel, one
//    argument check (check_crops) and one launcher (launch_crops); an entry point fills the fields that differ.
//      fmt 0: BlazeFaceModel rows (ymin,xmin,ymax,xmax,...,score@16), normalised to the model input:
//             column reorder (blazeface/model.py:70) + get_dets_bboxes_confs_lmarks_areas (utils/inference.py:11-58).
//      fmt 1: YOLOv5-face rows (x1,y1,x2,y2,conf@4,...) in model-input pixels: get_bboxes_confs_areas
//             (yolov5_face/onnx/onnx_utils.py:313-340).
//      fmt 2: MTCNN rows (x1,y1,x2,y2,(x,y) x 5,conf@14) in the FRAME's own pixels (the wrappers' input size is the image):
//             only fp_dets_to_crops_px passes it (no geom: gain 1, pad 0); the area share is taken of the frame, as fmt 0
//             takes it of the model input.  The entry points of fmt 0 / 1 refuse it.
//    All: conf > det_thres, area filter (fmt 0: 100*(area/total) > thr, info[6] = fraction; fmt 1: (100*area)/total > thr,
//    info[6] = percent -- each in its reference's operation order), scale_coords (utils/image.py:79-99: subtract pad,
//    divide by gain, clip to the frame), round half-to-even, then the crop of
//    face_extraction/extract_faces_from_dataset.py:289-303: int(), offsets (tx,ty,bx,by), clamp to the frame.
//    Faces are emitted in (frame, detection) order.
//    With lmarks / M / flags (the aligned entry points) each face also gets its landmarks in frame pixels, the least-squares
//    similarity onto the ArcFace 112 x 112 template (Umeyama's estimate, closed form in 2-D, fp64) and a flag for a
//    degenerate landmark set.
//      fmt 0 (BlazeFace, bbox_lmarks of get_dets_bboxes_confs_lmarks_areas, utils/inference.py:11-58): keypoint * [iw, ih],
//            - pad, / gain, round half-to-even, no clip.  Keypoints 0..3 (eyes, nose tip, mouth centre) -> template points
//            0, 1, 2 and the midpoint of 3 and 4; the ears are unused.
//      fmt 1 (YOLOv5-face, scale_coords_landmarks, y5/detect_face_pytorch.py:20-46): - pad, / gain, clamp to [0, w] /
//            [0, h], no rounding.  Landmark i -> template point i.
// 2. fp_align_warp / _ragged: one workgroup per (face, band of output rows), one lane per output pixel.  Each pixel
//    (x, y) samples the frame at M^-1 (x, y) (cv2.warpAffine's convention: integer coordinates, no half-pixel shift),
//    bilinear in fp32 over the u8 frame, taps outside the frame 0; u8 = round half-to-even, clamped; fp32 = lut[u8].
//    A degenerate face gets its box crop instead, bit for bit what fp_resize_normalize / fp_resize_ragged make of its
//    item.  The 2 x 2 gathers of a face touch a few KB of its frame, which stay in L2: no LDS staging.
// 3. fp_dets_to_crops_aligned_emulate / fp_align_emulate: the same __host__ __device__ code run serially on host memory.
#include <math.h>

#include "common.h"

namespace {

struct CropArgs {
  const float* dets;
  const int* counts;
  int B, max_dets, row, fmt, in_w, in_h, orig_w, orig_h;
  float det_thres, area_thres, gain, pad_x, pad_y;
  int tx, ty, bx, by, dst_w, dst_h, max_faces;
  fp_resize_item* items;
  float* info;
  int* n_faces;
  const fp_frame_desc* descs;   // ragged batch (ABI 14): per-frame orig_w / orig_h (descs) and gain, pad_x, pad_y (geom [B][3]);
  const float* geom;            // nullptr: the scalars above hold for every frame
  float* lmarks;                // aligned entry points only: [max_faces][10] landmarks in frame pixels,
  double* M;                    // [max_faces][6] frame -> template similarity,
  int* flags;                   // [max_faces] FP_ALIGN_* flags
};

// The scale_coords / clamp geometry of one frame.
struct FrameGeom {
  int orig_w, orig_h;
  float gain, pad_x, pad_y;
};

__host__ __device__ __forceinline__ FrameGeom frame_geom(const CropArgs& p, int f) {
  if (!p.descs) return FrameGeom{p.orig_w, p.orig_h, p.gain, p.pad_x, p.pad_y};
  const fp_frame_desc d = p.descs[f];
  if (!p.geom) return FrameGeom{d.w, d.h, 1.f, 0.f, 0.f};   // fmt 2: rows already in frame pixels
  return FrameGeom{d.w, d.h, p.geom[3 * f], p.geom[3 * f + 1], p.geom[3 * f + 2]};
}

// Detection rows of frame f to look at: none for a (ragged) frame with no usable geometry.
__host__ __device__ __forceinline__ int frame_dets(const CropArgs& p, const FrameGeom& g, int f) {
  if (g.orig_w <= 0 || g.orig_h <= 0 || !(g.gain > 0.f)) return 0;
  return min(max(p.counts[f], 0), p.max_dets);
}

__host__ __device__ __forceinline__ bool crop_one(const CropArgs& p, const FrameGeom& g, const float* d, float& x1,
                                                  float& y1, float& x2, float& y2, float& conf, float& perc) {
  if (p.fmt == 0) {
    conf = d[16];
    if (!(conf > p.det_thres)) return false;
    x1 = d[1] * (float)p.in_w; y1 = d[0] * (float)p.in_h; x2 = d[3] * (float)p.in_w; y2 = d[2] * (float)p.in_h;
  } else if (p.fmt == 2) {
    conf = d[14];
    if (!(conf > p.det_thres)) return false;
    x1 = d[0]; y1 = d[1]; x2 = d[2]; y2 = d[3];
  } else {
    conf = d[4];
    if (!(conf > p.det_thres)) return false;
    x1 = d[0]; y1 = d[1]; x2 = d[2]; y2 = d[3];
  }
  const float area = (x2 - x1) * (y2 - y1);
  if (p.fmt == 2) {  // the wrappers' input size is the frame: inference.py:40-42 with total = the frame's area
    perc = area / (float)(g.orig_w * g.orig_h);
    if (!(100.f * perc > p.area_thres)) return false;
  } else if (p.fmt == 0) {  // inference.py:40-42: perc = area / total (the FRACTION is reported), filter on 100 * perc
    perc = area / (float)(p.in_w * p.in_h);
    if (!(100.f * perc > p.area_thres)) return false;
  } else {           // onnx_utils.py:329-332: perc = 100 * area / total (the PERCENT is reported and compared)
    perc = (100.f * area) / (float)(p.in_w * p.in_h);
    if (!(perc > p.area_thres)) return false;
  }
  x1 = (x1 - g.pad_x) / g.gain; x2 = (x2 - g.pad_x) / g.gain;
  y1 = (y1 - g.pad_y) / g.gain; y2 = (y2 - g.pad_y) / g.gain;
  x1 = fminf(fmaxf(x1, 0.f), (float)g.orig_w); x2 = fminf(fmaxf(x2, 0.f), (float)g.orig_w);
  y1 = fminf(fmaxf(y1, 0.f), (float)g.orig_h); y2 = fminf(fmaxf(y2, 0.f), (float)g.orig_h);
  x1 = rintf(x1); y1 = rintf(y1); x2 = rintf(x2); y2 = rintf(y2);
  return true;
}

// The record every entry point writes (fp_dets_to_crops' items / info).
__host__ __device__ __forceinline__ void crop_emit_box(const CropArgs& p, const FrameGeom& g, int f, int slot, float x1,
                                                       float y1, float x2, float y2, float c, float pc) {
  int x = (int)x1 + p.tx, y = (int)y1 + p.ty, xw = (int)x2 + p.bx, yh = (int)y2 + p.by;
  x = max(x, 0); y = max(y, 0); xw = min(xw, g.orig_w); yh = min(yh, g.orig_h);
  fp_resize_item it;
  it.src_image = f;
  it.sx = x; it.sy = y; it.sw = xw - x; it.sh = yh - y;
  it.dx = 0; it.dy = 0; it.dw = p.dst_w; it.dh = p.dst_h;
  if (it.sw <= 0 || it.sh <= 0) { it.dw = 0; it.dh = 0; }  // empty crop: canvas becomes pad colour
  p.items[slot] = it;
  float* o = p.info + (long)slot * 7;
  o[0] = (float)f; o[1] = x1; o[2] = y1; o[3] = x2; o[4] = y2; o[5] = c; o[6] = pc;
}

constexpr int AL = FP_ALIGN_SIZE;
// ArcFace 112 x 112 five-point template (x, y): left eye, right eye, nose tip, left / right mouth corner
__host__ __device__ __forceinline__ double tmpl_x(int i) {
  return i == 0 ? 38.2946 : i == 1 ? 73.5318 : i == 2 ? 56.0252 : i == 3 ? 41.5493 : 70.7299;
}
__host__ __device__ __forceinline__ double tmpl_y(int i) {
  return i == 0 ? 51.6963 : i == 1 ? 51.5014 : i == 2 ? 71.7366 : i == 3 ? 92.3655 : 92.2041;
}

// Landmarks of one accepted face in frame pixels (slots 8, 9 are 0 for fmt 0).
__host__ __device__ __forceinline__ void crop_lmarks(const CropArgs& p, const FrameGeom& g, const float* d, float* o) {
  if (p.fmt == 0) {
    for (int k = 0; k < 4; ++k) {
      float x = d[4 + 2 * k] * (float)p.in_w, y = d[5 + 2 * k] * (float)p.in_h;
      x = (x - g.pad_x) / g.gain;
      y = (y - g.pad_y) / g.gain;
      o[2 * k] = rintf(x);
      o[2 * k + 1] = rintf(y);
    }
    o[8] = 0.f;
    o[9] = 0.f;
  } else if (p.fmt == 2) {
    for (int k = 0; k < 5; ++k) {
      o[2 * k] = fminf(fmaxf(d[4 + 2 * k], 0.f), (float)g.orig_w);
      o[2 * k + 1] = fminf(fmaxf(d[5 + 2 * k], 0.f), (float)g.orig_h);
    }
  } else {
    for (int k = 0; k < 5; ++k) {
      float x = (d[5 + 2 * k] - g.pad_x) / g.gain, y = (d[6 + 2 * k] - g.pad_y) / g.gain;
      o[2 * k] = fminf(fmaxf(x, 0.f), (float)g.orig_w);
      o[2 * k + 1] = fminf(fmaxf(y, 0.f), (float)g.orig_h);
    }
  }
}

__host__ __device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

// Least-squares similarity p_i -> q_i (no reflection): centre both sets, S = sum |p~|^2, a = sum p~.q~ / S,
// b = sum (p~x q~y - p~y q~x) / S, t = q_mean - [[a, -b], [b, a]] p_mean.  M = (a, -b, tx, b, a, ty).
// S < 1 px^2, or a result that is not finite / not invertible: FP_ALIGN_DEGENERATE and M = 0.
__host__ __device__ int align_estimate(const float* lm, int fmt, double* M) {
  const int n = fmt == 0 ? 4 : 5;
  double px[5], py[5], qx[5], qy[5];
  for (int i = 0; i < n; ++i) {
    px[i] = (double)lm[2 * i];
    py[i] = (double)lm[2 * i + 1];
    if (fmt == 0 && i == 3) {
      qx[i] = (tmpl_x(3) + tmpl_x(4)) * 0.5;
      qy[i] = (tmpl_y(3) + tmpl_y(4)) * 0.5;
    } else {
      qx[i] = tmpl_x(i);
      qy[i] = tmpl_y(i);
    }
  }
  double mpx = 0.0, mpy = 0.0, mqx = 0.0, mqy = 0.0;
  for (int i = 0; i < n; ++i) mpx += px[i], mpy += py[i], mqx += qx[i], mqy += qy[i];
  mpx /= n; mpy /= n; mqx /= n; mqy /= n;
  double S = 0.0, sa = 0.0, sb = 0.0;
  for (int i = 0; i < n; ++i) {
    const double dpx = px[i] - mpx, dpy = py[i] - mpy, dqx = qx[i] - mqx, dqy = qy[i] - mqy;
    S += dpx * dpx + dpy * dpy;
    sa += dpx * dqx + dpy * dqy;
    sb += dpx * dqy - dpy * dqx;
  }
  for (int i = 0; i < 6; ++i) M[i] = 0.0;
  if (!(S >= 1.0)) return FP_ALIGN_DEGENERATE;
  const double a = sa / S, b = sb / S;
  const double tx = mqx - (a * mpx - b * mpy), ty = mqy - (b * mpx + a * mpy);
  const double det = a * a + b * b;
  if (!(det > 0.0) || !finite_d(det) || !finite_d(tx) || !finite_d(ty)) return FP_ALIGN_DEGENERATE;
  M[0] = a; M[1] = -b; M[2] = tx;
  M[3] = b; M[4] = a; M[5] = ty;
  return 0;
}

// Writes the crop record of a face crop_one accepted into slot `slot` (< max_faces); with ALIGN also its landmarks,
// alignment transform and flags.
template <bool ALIGN>
__host__ __device__ __forceinline__ void crop_emit(const CropArgs& p, const FrameGeom& g, int f, const float* d, int slot,
                                                   float x1, float y1, float x2, float y2, float c, float pc) {
  crop_emit_box(p, g, f, slot, x1, y1, x2, y2, c, pc);
  if (ALIGN) {
    float* lm = p.lmarks + (long)slot * 10;
    crop_lmarks(p, g, d, lm);
    p.flags[slot] = align_estimate(lm, p.fmt, p.M + (long)slot * 6);
  }
}

// The faces among the first n rows of frame f, in order, into slots slot, slot + 1, ... (written while < max_faces, counted
// beyond): the kernel's emit pass and the whole of the host emulator.  Returns the slot after the frame's last face.
template <bool ALIGN>
__host__ __device__ int crop_frame(const CropArgs& p, const FrameGeom& g, int f, int n, int slot) {
  const float* D = p.dets + (long)f * p.max_dets * p.row;
  for (int i = 0; i < n; ++i) {
    float x1, y1, x2, y2, c, pc;
    if (!crop_one(p, g, D + (long)i * p.row, x1, y1, x2, y2, c, pc)) continue;
    if (slot < p.max_faces) crop_emit<ALIGN>(p, g, f, D + (long)i * p.row, slot, x1, y1, x2, y2, c, pc);
    ++slot;
  }
  return slot;
}

// One workgroup over all frames: a per-frame count pass, a block scan, then each frame's faces in order.
template <bool ALIGN>
__global__ __launch_bounds__(256) void dets_to_crops_kernel(CropArgs p) {
  __shared__ int scan[256];
  __shared__ int base_s;
  const int tid = threadIdx.x;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int f0 = 0; f0 < p.B; f0 += 256) {
    const int f = f0 + tid;
    int n = 0, cnt = 0;
    FrameGeom g{1, 1, 1.f, 0.f, 0.f};
    if (f < p.B) {
      g = frame_geom(p, f);
      n = frame_dets(p, g, f);
      const float* D = p.dets + (long)f * p.max_dets * p.row;
      for (int i = 0; i < n; ++i) {
        float x1, y1, x2, y2, c, pc;
        if (crop_one(p, g, D + (long)i * p.row, x1, y1, x2, y2, c, pc)) ++cnt;
      }
    }
    scan[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive Hillis-Steele scan over the 256 frames of this chunk
      int v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    crop_frame<ALIGN>(p, g, f, n, base_s + scan[tid] - cnt);   // n = 0 past the last frame
    __syncthreads();
    if (tid == 255) base_s += scan[255];
    __syncthreads();
  }
  if (tid == 0) p.n_faces[0] = base_s;  // may exceed max_faces: the host checks and raises
}

// What an entry point asks of its arguments beyond the checks all six share.
enum CropFrames { CROPS_DENSE, CROPS_RAGGED, CROPS_PX };   // frame geometry: orig_* / gain scalars, descs + geom, descs alone
struct CropForm {
  CropFrames frames;
  int fmt_lo, fmt_hi;   // row formats taken
  int min_row1;         // least row_floats of fmt 1 (15: rows with landmarks), fmt 0 needs 17, fmt 2 15
  bool align;           // lmarks / M / flags are required (CROPS_PX: all three or none)
};

// Everything the host can see, before any launch; FP_ERR_INVALID_ARG for the shared arguments comes before FP_ERR_ALIGNMENT,
// and that before the frame geometry of the dense and ragged forms.
int check_crops(const CropArgs& a, const CropForm& form) {
  if (!a.dets || !a.counts || !a.items || !a.info || !a.n_faces) return FP_ERR_INVALID_ARG;
  if (form.align && (!a.lmarks || !a.M || !a.flags)) return FP_ERR_INVALID_ARG;
  if (form.frames == CROPS_PX && !a.descs) return FP_ERR_INVALID_ARG;
  if (a.B < 0 || a.max_dets <= 0 || a.max_faces <= 0 || a.in_w <= 0 || a.in_h <= 0 || a.dst_w <= 0 || a.dst_h <= 0)
    return FP_ERR_INVALID_ARG;
  if (a.fmt < form.fmt_lo || a.fmt > form.fmt_hi) return FP_ERR_INVALID_ARG;
  if (a.row < (a.fmt == 0 ? 17 : a.fmt == 1 ? form.min_row1 : 15)) return FP_ERR_INVALID_ARG;
  if ((a.lmarks || a.M || a.flags) && (!a.lmarks || !a.M || !a.flags)) return FP_ERR_INVALID_ARG;
  if (a.M && ((uintptr_t)a.M) % 8) return FP_ERR_ALIGNMENT;
  if (form.frames == CROPS_DENSE && (a.orig_w <= 0 || a.orig_h <= 0 || !(a.gain > 0.f))) return FP_ERR_INVALID_ARG;
  if (form.frames == CROPS_RAGGED && (!a.descs || !a.geom)) return FP_ERR_INVALID_ARG;
  return FP_OK;
}

int launch_crops(const CropArgs& a, hipStream_t s) {
  if (a.lmarks) hipLaunchKernelGGL(dets_to_crops_kernel<true>, dim3(1), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(dets_to_crops_kernel<false>, dim3(1), dim3(256), 0, s, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

// The arguments all six entry points pass on as they are; everything else starts at 0 / nullptr and is assigned by name.
CropArgs crop_args(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt, int in_w, int in_h,
                   float det_thres, float area_thres, int off_tx, int off_ty, int off_bx, int off_by, int dst_w, int dst_h,
                   int max_faces, fp_resize_item* items, float* face_info, int32_t* n_faces) {
  CropArgs a{};
  a.dets = dets; a.counts = counts; a.B = B; a.max_dets = max_dets; a.row = row_floats;
  a.fmt = fmt; a.in_w = in_w; a.in_h = in_h;
  a.det_thres = det_thres; a.area_thres = area_thres;
  a.tx = off_tx; a.ty = off_ty; a.bx = off_bx; a.by = off_by;
  a.dst_w = dst_w; a.dst_h = dst_h; a.max_faces = max_faces;
  a.items = items; a.info = face_info; a.n_faces = n_faces;
  return a;
}

// ------------------------------------------------------------------------------------------------ warp
struct WarpArgs {
  const uint8_t* frames;
  uint64_t frames_bytes;
  const fp_frame_desc* descs;   // nullptr: uniform frames of fh x fw
  int n_frames, fh, fw;
  const double* M;
  const float* info;
  const int* flags;
  const fp_resize_item* items;
  int n;
  uint8_t* out_u8;
  float* out_f32;
  int out_c;
  const float* lut;
  int rpb, bands;
};

struct WarpFace {
  const uint8_t* frame;   // pixel (0, 0) of the face's frame (nullptr: no usable frame, the face's canvas is 0)
  long avail;             // readable bytes from `frame` to the end of the buffer
  int w, h;
  bool degenerate;
  double ia, ib, tx, ty;  // inverse map: (sx, sy) = (ia u + ib v, ia v - ib u), (u, v) = (x - tx, y - ty)
  fp_resize_item it;      // box crop (degenerate faces), clamped as the resize kernels clamp it
};

// frame f of the batch: nullptr when f or its descriptor is out of range (the checks of resize_ragged_kernel)
__host__ __device__ __forceinline__ const uint8_t* warp_frame(const WarpArgs& p, int f, int& w, int& h, long& avail) {
  w = 3; h = 1; avail = 0;
  if (f < 0 || f >= p.n_frames) return nullptr;
  if (!p.descs) {
    w = p.fw; h = p.fh;
    const long off = (long)f * p.fh * p.fw * 3;
    avail = (long)p.frames_bytes - off;
    return p.frames + off;
  }
  const fp_frame_desc d = p.descs[f];
  if (!(d.off >= 0 && d.h >= 1 && d.h <= FP_FRAME_MAX_H && d.w >= FP_FRAME_MIN_W && d.w <= FP_FRAME_MAX_W &&
        (uint64_t)d.off + (uint64_t)d.h * (uint64_t)d.w * 3u <= p.frames_bytes))
    return nullptr;
  w = d.w; h = d.h;
  avail = (long)(p.frames_bytes - (uint64_t)d.off);
  return p.frames + d.off;
}

__host__ __device__ WarpFace warp_face(const WarpArgs& p, int k) {
  WarpFace F;
  F.degenerate = (p.flags[k] & FP_ALIGN_DEGENERATE) != 0;
  F.ia = F.ib = F.tx = F.ty = 0.0;
  F.it = p.items[k];
  if (F.degenerate) {
    F.frame = warp_frame(p, F.it.src_image, F.w, F.h, F.avail);
    F.it.sx = min(max(F.it.sx, 0), F.w - 1);
    F.it.sy = min(max(F.it.sy, 0), F.h - 1);
    F.it.sw = min(max(F.it.sw, 1), F.w - F.it.sx);
    F.it.sh = min(max(F.it.sh, 1), F.h - F.it.sy);
    if (!(F.it.dw > 0 && F.it.dh > 0)) F.frame = nullptr;
    return F;
  }
  const float fi = p.info[(long)k * 7];
  const int f = (fi >= 0.f && fi < (float)p.n_frames) ? (int)fi : -1;
  F.frame = warp_frame(p, f, F.w, F.h, F.avail);
  const double* m = p.M + (long)k * 6;
  const double a = m[0], b = m[3], det = a * a + b * b;
  if (!(det > 0.0) || !finite_d(det) || !finite_d(m[2]) || !finite_d(m[5])) {
    F.frame = nullptr;
    return F;
  }
  F.ia = a / det;
  F.ib = b / det;
  F.tx = m[2];
  F.ty = m[5];
  return F;
}

// fp_lb_coef (letterbox.h) as the resize kernels execute it: their ((d + 0.5) * scale - 0.5) is contracted into one fma
// by the compiler, written out here so that this file (built without contraction) and the host get the same taps.
__host__ __device__ __forceinline__ void box_coef(int d, double scale, int ssize, int& s0, int& s1, int& a0, int& a1) {
  float f = (float)fma((double)d + 0.5, scale, -0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    f = 0.f;
    s = 0;
  }
  if (s >= ssize - 1) {
    f = 0.f;
    s = ssize - 1;
  }
  s0 = s;
  s1 = min(s + 1, ssize - 1);
  a0 = (int)rintf((1.f - f) * 2048.f);
  a1 = (int)rintf(f * 2048.f);
}

// Box crop pixel of a degenerate face: resize_normalize_kernel's arithmetic (image.hip), pad 0.
__host__ __device__ __forceinline__ void box_pixel(const WarpFace& F, int x, int y, int v[3]) {
  const fp_resize_item& it = F.it;
  if (!F.frame || x < it.dx || x >= it.dx + it.dw || y < it.dy || y >= it.dy + it.dh) {
    v[0] = v[1] = v[2] = 0;
    return;
  }
  int sx0, sx1, ax0, ax1, sy0, sy1, by0, by1;
  box_coef(x - it.dx, (double)it.sw / (double)it.dw, it.sw, sx0, sx1, ax0, ax1);
  box_coef(y - it.dy, (double)it.sh / (double)it.dh, it.sh, sy0, sy1, by0, by1);
  const uint8_t* r0 = F.frame + ((long)(it.sy + sy0) * F.w + it.sx) * 3;
  const uint8_t* r1 = F.frame + ((long)(it.sy + sy1) * F.w + it.sx) * 3;
  for (int c = 0; c < 3; ++c) {
    const int h0 = (int)r0[sx0 * 3 + c] * ax0 + (int)r0[sx1 * 3 + c] * ax1;
    const int h1 = (int)r1[sx0 * 3 + c] * ax0 + (int)r1[sx1 * 3 + c] * ax1;
    const int o = (((by0 * (h0 >> 4)) >> 16) + ((by1 * (h1 >> 4)) >> 16) + 2) >> 2;
    v[c] = min(max(o, 0), 255);
  }
}

// Source position of output pixel (x, y); false when every tap is outside the frame (or not finite).
__host__ __device__ __forceinline__ bool warp_src(const WarpFace& F, int x, int y, int& x0, int& y0, float& fx, float& fy) {
  const double u = (double)x - F.tx, t = (double)y - F.ty;
  const double sx = F.ia * u + F.ib * t;
  const double sy = F.ia * t - F.ib * u;
  if (!(sx > -1.0 && sx < (double)F.w && sy > -1.0 && sy < (double)F.h)) return false;
  const double flx = floor(sx), fly = floor(sy);
  x0 = (int)flx;
  y0 = (int)fly;
  fx = (float)(sx - flx);
  fy = (float)(sy - fly);
  return true;
}

// The four taps (rows y0, y0 + 1; columns x0, x0 + 1; 3 channels each), 0 outside the frame.
__host__ __device__ __forceinline__ void warp_taps_bytes(const WarpFace& F, int x0, int y0, int t[2][2][3]) {
  for (int r = 0; r < 2; ++r)
    for (int k = 0; k < 2; ++k) {
      const int xx = x0 + k, yy = y0 + r;
      if (xx >= 0 && xx < F.w && yy >= 0 && yy < F.h) {
        const uint8_t* q = F.frame + ((long)yy * F.w + xx) * 3;
        for (int c = 0; c < 3; ++c) t[r][k][c] = (int)q[c];
      } else {
        for (int c = 0; c < 3; ++c) t[r][k][c] = 0;
      }
    }
}

__host__ __device__ __forceinline__ void warp_blend(const int t[2][2][3], float fx, float fy, int v[3]) {
  const float wx0 = 1.f - fx, wy0 = 1.f - fy;
  for (int c = 0; c < 3; ++c) {
    const float top = (float)t[0][0][c] * wx0 + (float)t[0][1][c] * fx;
    const float bot = (float)t[1][0][c] * wx0 + (float)t[1][1][c] * fx;
    const float val = top * wy0 + bot * fy;
    v[c] = min(max((int)rintf(val), 0), 255);
  }
}

__device__ __forceinline__ void warp_pixel_dev(const WarpFace& F, int x, int y, int v[3]) {
  int x0, y0;
  float fx, fy;
  if (!F.frame || !warp_src(F, x, y, x0, y0, fx, fy)) {
    v[0] = v[1] = v[2] = 0;
    return;
  }
  int t[2][2][3];
  const long o0 = ((long)y0 * F.w + x0) * 3;
  if (x0 >= 0 && x0 + 1 < F.w && y0 >= 0 && y0 + 1 < F.h && o0 + (long)F.w * 3 + 8 <= F.avail) {
    // both taps of a row in one unaligned 8-byte load (bytes 0..5 used)
    unsigned long long r0, r1;
    __builtin_memcpy(&r0, F.frame + o0, 8);
    __builtin_memcpy(&r1, F.frame + o0 + (long)F.w * 3, 8);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        t[0][k][c] = (int)((r0 >> (8 * (3 * k + c))) & 0xff);
        t[1][k][c] = (int)((r1 >> (8 * (3 * k + c))) & 0xff);
      }
  } else {
    warp_taps_bytes(F, x0, y0, t);
  }
  warp_blend(t, fx, fy, v);
}

__host__ __device__ __forceinline__ void warp_store(const WarpArgs& p, const float* lut, int k, int pix, const int v[3]) {
  const long px = (long)k * AL * AL + pix;
  if (p.out_u8) {
    uint8_t* o = p.out_u8 + px * 3;
    o[0] = (uint8_t)v[0];
    o[1] = (uint8_t)v[1];
    o[2] = (uint8_t)v[2];
  }
  if (p.out_f32) {
    float* o = p.out_f32 + px * p.out_c;
    if (p.out_c == 4) {
      f32x4 w = {lut[v[0]], lut[v[1]], lut[v[2]], 0.f};
      *(f32x4*)o = w;
    } else {
      o[0] = lut[v[0]];
      o[1] = lut[v[1]];
      o[2] = lut[v[2]];
    }
  }
}

__global__ __launch_bounds__(256) void align_warp_kernel(WarpArgs p) {
  __shared__ float lut[256];
  const int tid = threadIdx.x;
  const int k = blockIdx.x / p.bands, y0 = (blockIdx.x - k * p.bands) * p.rpb;
  if (p.out_f32) lut[tid] = p.lut[tid];
  __syncthreads();
  const WarpFace F = warp_face(p, k);
  const int npx = min(p.rpb, AL - y0) * AL;
  for (int i = tid; i < npx; i += 256) {
    const int pix = y0 * AL + i;
    const int y = pix / AL, x = pix - y * AL;
    int v[3];
    if (F.degenerate) box_pixel(F, x, y, v);
    else warp_pixel_dev(F, x, y, v);
    warp_store(p, lut, k, pix, v);
  }
}

int launch_warp(WarpArgs a, hipStream_t s) {
  a.rpb = 16;                                   // 1792 pixels = 7 per lane
  a.bands = fp_ceil_div(AL, a.rpb);
  if ((long)a.n * a.bands >= (1L << 31)) return FP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(align_warp_kernel, dim3((unsigned)(a.n * a.bands)), dim3(256), 0, s, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

// Checks shared by both warp entry points (everything the host can see; device memory is bounded in the kernel).
int check_warp(const WarpArgs& a) {
  if (!a.frames || !a.M || !a.info || !a.flags || !a.items) return FP_ERR_INVALID_ARG;
  if (a.n < 0 || a.n_frames <= 0 || (!a.out_u8 && !a.out_f32)) return FP_ERR_INVALID_ARG;
  if (a.out_f32 && (!a.lut || (a.out_c != 3 && a.out_c != 4))) return FP_ERR_INVALID_ARG;
  if (((uintptr_t)a.M) % 8 || ((uintptr_t)a.info) % 4 || ((uintptr_t)a.flags) % 4 || ((uintptr_t)a.items) % 4)
    return FP_ERR_ALIGNMENT;
  if (a.out_f32 && (((uintptr_t)a.out_f32) % (a.out_c == 4 ? 16 : 4))) return FP_ERR_ALIGNMENT;
  return FP_OK;
}

}  // namespace

extern "C" {

int fp_dets_to_crops(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt, int in_w,
                     int in_h, int orig_w, int orig_h, float det_thres, float area_thres, float gain, float pad_x,
                     float pad_y, int off_tx, int off_ty, int off_bx, int off_by, int dst_w, int dst_h, int max_faces,
                     fp_resize_item* items, float* face_info, int32_t* n_faces, void* stream) {
  CropArgs a = crop_args(dets, counts, B, max_dets, row_floats, fmt, in_w, in_h, det_thres, area_thres, off_tx, off_ty, off_bx,
                         off_by, dst_w, dst_h, max_faces, items, face_info, n_faces);
  a.orig_w = orig_w; a.orig_h = orig_h; a.gain = gain; a.pad_x = pad_x; a.pad_y = pad_y;
  const int rc = check_crops(a, CropForm{CROPS_DENSE, 0, 1, 5, false});
  return rc != FP_OK ? rc : launch_crops(a, (hipStream_t)stream);
}

int fp_dets_to_crops_ragged(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt,
                            int in_w, int in_h, const fp_frame_desc* descs, const float* geom, float det_thres,
                            float area_thres, int off_tx, int off_ty, int off_bx, int off_by, int dst_w, int dst_h,
                            int max_faces, fp_resize_item* items, float* face_info, int32_t* n_faces, void* stream) {
  CropArgs a = crop_args(dets, counts, B, max_dets, row_floats, fmt, in_w, in_h, det_thres, area_thres, off_tx, off_ty, off_bx,
                         off_by, dst_w, dst_h, max_faces, items, face_info, n_faces);
  a.descs = descs; a.geom = geom;
  const int rc = check_crops(a, CropForm{CROPS_RAGGED, 0, 1, 5, false});
  return rc != FP_OK ? rc : launch_crops(a, (hipStream_t)stream);
}

int fp_dets_to_crops_aligned(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt, int in_w,
                             int in_h, int orig_w, int orig_h, float det_thres, float area_thres, float gain, float pad_x,
                             float pad_y, int off_tx, int off_ty, int off_bx, int off_by, int dst_w, int dst_h, int max_faces,
                             fp_resize_item* items, float* face_info, int32_t* n_faces, float* lmarks, double* M,
                             int32_t* flags, void* stream) {
  CropArgs a = crop_args(dets, counts, B, max_dets, row_floats, fmt, in_w, in_h, det_thres, area_thres, off_tx, off_ty, off_bx,
                         off_by, dst_w, dst_h, max_faces, items, face_info, n_faces);
  a.orig_w = orig_w; a.orig_h = orig_h; a.gain = gain; a.pad_x = pad_x; a.pad_y = pad_y;
  a.lmarks = lmarks; a.M = M; a.flags = flags;
  const int rc = check_crops(a, CropForm{CROPS_DENSE, 0, 1, 15, true});
  return rc != FP_OK ? rc : launch_crops(a, (hipStream_t)stream);
}

int fp_dets_to_crops_aligned_ragged(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt,
                                    int in_w, int in_h, const fp_frame_desc* descs, const float* geom, float det_thres,
                                    float area_thres, int off_tx, int off_ty, int off_bx, int off_by, int dst_w, int dst_h,
                                    int max_faces, fp_resize_item* items, float* face_info, int32_t* n_faces,
                                    float* lmarks, double* M, int32_t* flags, void* stream) {
  CropArgs a = crop_args(dets, counts, B, max_dets, row_floats, fmt, in_w, in_h, det_thres, area_thres, off_tx, off_ty, off_bx,
                         off_by, dst_w, dst_h, max_faces, items, face_info, n_faces);
  a.descs = descs; a.geom = geom;
  a.lmarks = lmarks; a.M = M; a.flags = flags;
  const int rc = check_crops(a, CropForm{CROPS_RAGGED, 0, 1, 15, true});
  return rc != FP_OK ? rc : launch_crops(a, (hipStream_t)stream);
}

int fp_dets_to_crops_px(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats,
                        const fp_frame_desc* descs, float det_thres, float area_thres, int off_tx, int off_ty, int off_bx,
                        int off_by, int dst_w, int dst_h, int max_faces, fp_resize_item* items, float* face_info,
                        int32_t* n_faces, float* lmarks, double* M, int32_t* flags, void* stream) {
  CropArgs a = crop_args(dets, counts, B, max_dets, row_floats, 2, 1, 1, det_thres, area_thres, off_tx, off_ty, off_bx, off_by,
                         dst_w, dst_h, max_faces, items, face_info, n_faces);
  a.descs = descs;                                // no geom: the rows are in each frame's own pixels
  a.lmarks = lmarks; a.M = M; a.flags = flags;    // all three or none
  const int rc = check_crops(a, CropForm{CROPS_PX, 2, 2, 15, false});
  return rc != FP_OK ? rc : launch_crops(a, (hipStream_t)stream);
}

int fp_dets_to_crops_aligned_emulate(const float* dets, const int32_t* counts, int B, int max_dets, int row_floats, int fmt,
                                     int in_w, int in_h, const fp_frame_desc* descs, const float* geom, float det_thres,
                                     float area_thres, int off_tx, int off_ty, int off_bx, int off_by, int dst_w, int dst_h,
                                     int max_faces, fp_resize_item* items, float* face_info, int32_t* n_faces,
                                     float* lmarks, double* M, int32_t* flags) {
  CropArgs a = crop_args(dets, counts, B, max_dets, row_floats, fmt, in_w, in_h, det_thres, area_thres, off_tx, off_ty, off_bx,
                         off_by, dst_w, dst_h, max_faces, items, face_info, n_faces);
  a.descs = descs; a.geom = geom;
  a.lmarks = lmarks; a.M = M; a.flags = flags;
  const int rc = check_crops(a, CropForm{CROPS_RAGGED, 0, 1, 15, true});
  if (rc != FP_OK) return rc;
  int slot = 0;
  for (int f = 0; f < B; ++f) {   // dets_to_crops_kernel's order: frame by frame, each frame's detections in order
    const FrameGeom g = frame_geom(a, f);
    slot = crop_frame<true>(a, g, f, frame_dets(a, g, f), slot);
  }
  n_faces[0] = slot;
  return FP_OK;
}

int fp_align_warp(const uint8_t* frames, int n_frames, int frame_h, int frame_w, const double* M, const float* face_info,
                  const int32_t* flags, const fp_resize_item* items, int n, uint8_t* out_u8, float* out_f32, int out_c,
                  const float* lut256, void* stream) {
  if (frame_h <= 0 || frame_h > FP_FRAME_MAX_H || frame_w <= 0 || frame_w > FP_FRAME_MAX_W) return FP_ERR_INVALID_ARG;
  WarpArgs a{frames, (uint64_t)n_frames * frame_h * frame_w * 3, nullptr, n_frames, frame_h, frame_w, M, face_info, flags,
             items, n, out_u8, out_f32, out_c, lut256, 0, 0};
  int rc = check_warp(a);
  if (rc != FP_OK || n == 0) return rc;
  return launch_warp(a, (hipStream_t)stream);
}

int fp_align_warp_ragged(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const double* M,
                         const float* face_info, const int32_t* flags, const fp_resize_item* items, int n, uint8_t* out_u8,
                         float* out_f32, int out_c, const float* lut256, void* stream) {
  if (!descs || frames_bytes < 3 * FP_FRAME_MIN_W) return FP_ERR_INVALID_ARG;
  WarpArgs a{frames, (uint64_t)frames_bytes, descs, n_frames, 0, 0, M, face_info, flags, items, n, out_u8, out_f32, out_c,
             lut256, 0, 0};
  int rc = check_warp(a);
  if (rc != FP_OK || n == 0) return rc;
  return launch_warp(a, (hipStream_t)stream);
}

int fp_align_emulate(const uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const float* lmarks,
                     int fmt, double* M, const float* face_info, int32_t* flags, const fp_resize_item* items, int n,
                     uint8_t* out_u8) {
  if (n < 0 || !M || !flags || fmt < 0 || fmt > 2) return FP_ERR_INVALID_ARG;
  if (lmarks)
    for (int k = 0; k < n; ++k) flags[k] = align_estimate(lmarks + (long)k * 10, fmt, M + (long)k * 6);
  if (!out_u8) return FP_OK;
  if (!frames || !descs || !face_info || !items || n_frames <= 0) return FP_ERR_INVALID_ARG;
  const WarpArgs p{frames, (uint64_t)frames_bytes, descs, n_frames, 0, 0, M, face_info, flags, items, n, out_u8, nullptr, 0,
                   nullptr, 0, 0};
  for (int k = 0; k < n; ++k) {
    const WarpFace F = warp_face(p, k);
    for (int y = 0; y < AL; ++y)
      for (int x = 0; x < AL; ++x) {
        int v[3];
        if (F.degenerate) {
          box_pixel(F, x, y, v);
        } else {
          int x0, y0, t[2][2][3];
          float fx, fy;
          if (F.frame && warp_src(F, x, y, x0, y0, fx, fy)) {
            warp_taps_bytes(F, x0, y0, t);
            warp_blend(t, fx, fy, v);
          } else {
            v[0] = v[1] = v[2] = 0;
          }
        }
        warp_store(p, nullptr, k, y * AL + x, v);
      }
  }
  return FP_OK;
}

}  // extern "C"
