// crops.h — detections -> per-face crop rectangles (and, for the aligned entry points, landmarks and the alignment
// transform), shared by post.hip (fp_dets_to_crops / _ragged) and align.hip (fp_dets_to_crops_aligned / _ragged and
// the host emulator).  Every translation unit that includes it is built with -ffp-contract=off: the arithmetic below
// follows numpy's operation order for float32 inputs and must not be contracted into fmas.
//
// fmt 0: BlazeFaceModel rows (ymin,xmin,ymax,xmax,...,score@16), normalised to the model input:
//        column reorder (blazeface/model.py:70) + get_dets_bboxes_confs_lmarks_areas (utils/inference.py:11-58).
// fmt 1: YOLOv5-face rows (x1,y1,x2,y2,conf@4,...) in model-input pixels: get_bboxes_confs_areas
//        (yolov5_face/onnx/onnx_utils.py:313-340).
// fmt 2: MTCNN rows (x1,y1,x2,y2,(x,y) x 5,conf@14) in the FRAME's own pixels (the wrappers' input size is the image): only
//        fp_dets_to_crops_px passes it (no geom: gain 1, pad 0); the area share is taken of the frame, as fmt 0 takes it of
//        the model input.  The entry points of fmt 0 / 1 refuse it.
// Both: conf > det_thres, area filter (fmt 0: 100*(area/total) > thr, info[6] = fraction; fmt 1: (100*area)/total > thr,
// info[6] = percent -- each in its reference's operation order), scale_coords (utils/image.py:79-99: subtract pad,
// divide by gain, clip to the frame), round half-to-even, then the crop of
// face_extraction/extract_faces_from_dataset.py:289-303: int(), offsets (tx,ty,bx,by), clamp to the frame.
// All fp32, in numpy's operation order for float32 inputs.  Faces are emitted in (frame, detection) order.
#pragma once
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
  int* flags;                   // [max_faces] FP_ALIGN_* flags (align.hip)
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

// Writes the crop record of a face crop_one accepted into slot `slot` (< max_faces); with p.lmarks also its landmarks,
// alignment transform and flags (align_face, align.hip, defined by the including unit when ALIGN is used).
template <bool ALIGN>
__host__ __device__ void crop_emit(const CropArgs& p, const FrameGeom& g, int f, const float* d, int slot, float x1,
                                   float y1, float x2, float y2, float c, float pc);

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
    const float* D = nullptr;
    FrameGeom g{1, 1, 1.f, 0.f, 0.f};
    if (f < p.B) {
      g = frame_geom(p, f);
      n = min(max(p.counts[f], 0), p.max_dets);
      if (g.orig_w <= 0 || g.orig_h <= 0 || !(g.gain > 0.f)) n = 0;   // a ragged frame with no usable geometry: no faces
      D = p.dets + (long)f * p.max_dets * p.row;
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
    int slot = base_s + scan[tid] - cnt;
    for (int i = 0; i < n; ++i) {
      float x1, y1, x2, y2, c, pc;
      if (!crop_one(p, g, D + (long)i * p.row, x1, y1, x2, y2, c, pc)) continue;
      if (slot < p.max_faces) crop_emit<ALIGN>(p, g, f, D + (long)i * p.row, slot, x1, y1, x2, y2, c, pc);
      ++slot;
    }
    __syncthreads();
    if (tid == 255) base_s += scan[255];
    __syncthreads();
  }
  if (tid == 0) p.n_faces[0] = base_s;  // may exceed max_faces: the host checks and raises
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

template <>
__host__ __device__ __forceinline__ void crop_emit<false>(const CropArgs& p, const FrameGeom& g, int f, const float*, int slot,
                                                          float x1, float y1, float x2, float y2, float c, float pc) {
  crop_emit_box(p, g, f, slot, x1, y1, x2, y2, c, pc);
}

}  // namespace
