// attrcrop.hip — fp_attr_crop_items / _emulate (include/facepath.h): the crop rectangles the reference's
// OpenCVFaceDetAgeGenderModel feeds its age and gender nets (modules/opencv2_dnn/model.py): the rounded box, 5 px of padding,
// clamped to [0, W - 1) x [0, H - 1) (the reference's exclusive ends at W - 1 and H - 1), resized to the nets' 227 x 227.
// One lane per face; the host emulator runs the same function.
#include "common.h"

namespace {

struct AttrArgs {
  const float* info;
  int n, info_floats;
  const fp_frame_desc* descs;
  int n_frames, frame_w, frame_h, pad, dst_w, dst_h;
  fp_resize_item* items;
};

__host__ __device__ inline void attr_item(const AttrArgs& p, int i) {
  const float* r = p.info + (long)i * p.info_floats;
  const float ff = r[0];
  fp_resize_item it = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const bool fok = ff >= 0.f && ff < (float)p.n_frames;
  const int f = fok ? (int)ff : 0;
  it.src_image = f;
  int W = p.frame_w, H = p.frame_h;
  if (fok && p.descs) {
    W = p.descs[f].w;
    H = p.descs[f].h;
  }
  if (fok) {
    // scale_coords(...).round() (half to even) then int(); info boxes lie inside the frame
    const int x1 = (int)rintf(r[1]), y1 = (int)rintf(r[2]), x2 = (int)rintf(r[3]), y2 = (int)rintf(r[4]);
    const int x0 = x1 - p.pad > 0 ? x1 - p.pad : 0, y0 = y1 - p.pad > 0 ? y1 - p.pad : 0;
    const int xe = x2 + p.pad < W - 1 ? x2 + p.pad : W - 1, ye = y2 + p.pad < H - 1 ? y2 + p.pad : H - 1;
    if (xe > x0 && ye > y0) {
      it.sx = x0; it.sy = y0; it.sw = xe - x0; it.sh = ye - y0;
      it.dw = p.dst_w; it.dh = p.dst_h;
    }
  }
  p.items[i] = it;
}

__global__ __launch_bounds__(256) void attr_crop_items_kernel(AttrArgs p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < p.n) attr_item(p, i);
}

int fill(AttrArgs& a, const float* info, int n, int info_floats, const fp_frame_desc* descs, int n_frames, int frame_w,
         int frame_h, int pad, int dst_w, int dst_h, fp_resize_item* items) {
  if (n < 0 || info_floats < 5 || pad < 0 || dst_w < 1 || dst_h < 1 || n_frames < 0) return FP_ERR_INVALID_ARG;
  if (n > 0 && (!info || !items)) return FP_ERR_INVALID_ARG;
  if (!descs && (frame_w < 1 || frame_h < 1)) return FP_ERR_INVALID_ARG;
  a.info = info; a.n = n; a.info_floats = info_floats; a.descs = descs; a.n_frames = n_frames;
  a.frame_w = frame_w; a.frame_h = frame_h; a.pad = pad; a.dst_w = dst_w; a.dst_h = dst_h; a.items = items;
  return FP_OK;
}

}  // namespace

extern "C" int fp_attr_crop_items(const float* info, int n, int info_floats, const fp_frame_desc* descs, int n_frames,
                                  int frame_w, int frame_h, int pad, int dst_w, int dst_h, fp_resize_item* items,
                                  void* stream) {
  AttrArgs a;
  const int rc = fill(a, info, n, info_floats, descs, n_frames, frame_w, frame_h, pad, dst_w, dst_h, items);
  if (rc != FP_OK || n == 0) return rc;
  hipLaunchKernelGGL(attr_crop_items_kernel, dim3((unsigned)fp_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

extern "C" int fp_attr_crop_items_emulate(const float* info, int n, int info_floats, const fp_frame_desc* descs, int n_frames,
                                          int frame_w, int frame_h, int pad, int dst_w, int dst_h, fp_resize_item* items) {
  AttrArgs a;
  const int rc = fill(a, info, n, info_floats, descs, n_frames, frame_w, frame_h, pad, dst_w, dst_h, items);
  if (rc != FP_OK) return rc;
  for (int i = 0; i < n; ++i) attr_item(a, i);
  return FP_OK;
}
