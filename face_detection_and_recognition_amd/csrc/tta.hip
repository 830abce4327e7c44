// tta.hip — YOLOv5-face augmented inference (y5/models/yolo.py:156-175, y5/utils/torch_utils.py:230-240) on gfx950: the
// inputs of the scaled / mirrored views from the view-1 canvas, and the Detect decode with the view's un-mapping behind it.
// Build with -ffp-contract=off, as post.o: the decoded rows feed the NMS threshold decisions, and the numpy restatements
// (modules/yolov5_face/tta.py) reproduce both kernels in the written order of operations.
#include "common.h"

namespace {

struct view_geom {
  int ch, cw, ph, pw, flip;
  float sh, sw;   // (float)H / ch, (float)W / cw: area_pixel_compute_scale with align_corners = False and no scale factor
};

// F.interpolate(mode="bilinear", align_corners=False) source coordinate of output index d (upsample_bilinear2d's
// area_pixel_compute_source_index): tap i0, its neighbour i1 (clamped at the edge) and the weight of i1.  torch's CPU build
// contracts scale * (d + 0.5) - 0.5 into ONE fma; a separately rounded product moves src by an ulp of src (1.5e-5 at column
// 128), and the weight src - i0 with it: 1.5e-5 off torch at 640 x 640.  So the fma is written out here (the file is built
// with -ffp-contract=off, which leaves an explicit fmaf alone).
__device__ __forceinline__ void bilinear_tap(float scale, int d, int in, int& i0, int& i1, float& l1) {
  const float src = fmaxf(__builtin_fmaf(scale, (float)d + 0.5f, -0.5f), 0.f);
  i0 = min((int)src, in - 1);
  i1 = min(i0 + 1, in - 1);
  l1 = src - (float)i0;
}

// One lane per output pixel (a 4-float NHWC pixel: one 16-byte load per tap, one 16-byte store), 256 consecutive pixels of
// one view of one image per workgroup: grid = (chunks of the larger view, images, 2 views).  Bandwidth-bound; the taps of
// neighbouring lanes are neighbouring or equal canvas pixels, so the canvas is read from HBM about once.
__global__ __launch_bounds__(256) void tta_views_kernel(const f32x4* __restrict__ canvas, int H, int W, f32x4* __restrict__ out_a,
                                                        view_geom ga, f32x4* __restrict__ out_b, view_geom gb, float pad) {
  const bool second = blockIdx.z != 0;
  const view_geom g = second ? gb : ga;
  f32x4* __restrict__ out = second ? out_b : out_a;
  const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (idx >= g.ph * g.pw) return;
  const int y = idx / g.pw, x = idx - y * g.pw;
  const long n = blockIdx.y;
  f32x4 v;
  if (y < g.ch && x < g.cw) {
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_tap(g.sh, y, H, y0, y1, ly);
    bilinear_tap(g.sw, x, W, x0, x1, lx);
    if (g.flip) {   // x.flip(3) first: column j of the mirrored image is column W - 1 - j of the canvas
      x0 = W - 1 - x0;
      x1 = W - 1 - x1;
    }
    const f32x4* img = canvas + n * H * W;
    const f32x4 a = img[(long)y0 * W + x0], b = img[(long)y0 * W + x1];
    const f32x4 c = img[(long)y1 * W + x0], d = img[(long)y1 * W + x1];
    const float hx = 1.f - lx, hy = 1.f - ly;
    const f32x4 top = a * hx + b * lx, bot = c * hx + d * lx;
    v = top * hy + bot * ly;
    v.w = 0.f;
  } else {
    v = f32x4{pad, pad, pad, 0.f};     // F.pad(value=0.447) right of and below the content
  }
  out[(n * g.ph + y) * g.pw + x] = v;
}

// yolo_decode_kernel's arithmetic (post.hip; y5/models/yolo.py:62-108), then in the same lane the view's un-mapping
// (yolo.py:166-170): columns 0..3 / si as an IEEE division, then cx = W - cx for the mirrored view.  lm_mode 0 leaves the
// landmark columns as decoded (the reference); 1 divides them by si, mirrors x and swaps the left / right points.
__global__ __launch_bounds__(256) void yolo_decode_view_kernel(const float* __restrict__ head, int B, int ny, int nx, int na,
                                                               float stride, float aw0, float ah0, float aw1, float ah1,
                                                               float aw2, float ah2, float* __restrict__ out,
                                                               long out_image_stride, long out_row_offset, float si, int flip,
                                                               float img_w, int lm_mode) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)na * ny * nx;
  if (idx >= per * B) return;
  const int b = (int)(idx / per);
  int rem = (int)(idx - (long)b * per);
  const int a = rem / (ny * nx);
  rem -= a * ny * nx;
  const int y = rem / nx, x = rem - y * nx;
  const float aw = a == 0 ? aw0 : (a == 1 ? aw1 : aw2);
  const float ah = a == 0 ? ah0 : (a == 1 ? ah1 : ah2);
  const float* v = head + (((long)b * ny + y) * nx + x) * (na * 16) + a * 16;
  float* o = out + (long)b * out_image_stride + (out_row_offset + (long)a * ny * nx + (long)y * nx + x) * 16;
  float r[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) r[c] = v[c];
  const float gx = (float)x, gy = (float)y;
  float s0 = 1.0f / (1.0f + expf(-r[0])), s1 = 1.0f / (1.0f + expf(-r[1]));
  float s2 = 1.0f / (1.0f + expf(-r[2])), s3 = 1.0f / (1.0f + expf(-r[3]));
  float q[16];
  q[0] = (s0 * 2.f - 0.5f + gx) * stride;
  q[1] = (s1 * 2.f - 0.5f + gy) * stride;
  const float w2 = s2 * 2.f, h2 = s3 * 2.f;
  q[2] = w2 * w2 * aw;
  q[3] = h2 * h2 * ah;
  q[4] = 1.0f / (1.0f + expf(-r[4]));
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    q[5 + 2 * k] = r[5 + 2 * k] * aw + gx * stride;
    q[6 + 2 * k] = r[6 + 2 * k] * ah + gy * stride;
  }
  q[15] = 1.0f / (1.0f + expf(-r[15]));
#pragma unroll
  for (int c = 0; c < 4; ++c) q[c] = q[c] / si;          // yi[..., :4] /= si
  if (flip) q[0] = img_w - q[0];                          // yi[..., 0] = img_size[1] - yi[..., 0]
  if (lm_mode == 1) {
#pragma unroll
    for (int c = 5; c < 15; ++c) q[c] = q[c] / si;
    if (flip) {
#pragma unroll
      for (int k = 0; k < 5; ++k) q[5 + 2 * k] = img_w - q[5 + 2 * k];
      // mirrored: the eyes (points 0, 1) and the mouth corners (3, 4) change places, the nose (2) stays
      float t;
      t = q[5], q[5] = q[7], q[7] = t;
      t = q[6], q[6] = q[8], q[8] = t;
      t = q[11], q[11] = q[13], q[13] = t;
      t = q[12], q[12] = q[14], q[14] = t;
    }
  }
  f32x4* o4 = reinterpret_cast<f32x4*>(o);                // rows are 64 bytes; `out` is checked 16-byte aligned
#pragma unroll
  for (int c = 0; c < 4; ++c) o4[c] = f32x4{q[4 * c], q[4 * c + 1], q[4 * c + 2], q[4 * c + 3]};
}

bool view_ok(const fp_tta_view& v, int H, int W) {
  return v.content_h >= 1 && v.content_w >= 1 && v.content_h <= v.padded_h && v.content_w <= v.padded_w && v.content_h <= H &&
         v.content_w <= W && (v.flip == 0 || v.flip == 1) && (long)v.padded_h * v.padded_w < (1l << 31) - 256;
}

view_geom geom(const fp_tta_view& v, int H, int W) {
  return view_geom{v.content_h, v.content_w, v.padded_h, v.padded_w, v.flip, (float)H / (float)v.content_h,
                   (float)W / (float)v.content_w};
}

}  // namespace

extern "C" {

int fp_tta_views(const float* canvas, int N, int H, int W, const fp_tta_view* views, float* out_a, float* out_b, float pad_value,
                 void* stream) {
  if (!canvas || !views || !out_a || !out_b || N < 0 || H <= 0 || W <= 0 || N > 65535) return FP_ERR_INVALID_ARG;
  if ((long)H * W >= (1l << 31) || !view_ok(views[0], H, W) || !view_ok(views[1], H, W)) return FP_ERR_INVALID_ARG;
  if (((uintptr_t)canvas | (uintptr_t)out_a | (uintptr_t)out_b) % 16) return FP_ERR_ALIGNMENT;
  if (N == 0) return FP_OK;
  const long pa = (long)views[0].padded_h * views[0].padded_w, pb = (long)views[1].padded_h * views[1].padded_w;
  hipLaunchKernelGGL(tta_views_kernel, dim3((unsigned)fp_ceil_div(pa > pb ? pa : pb, 256), (unsigned)N, 2), dim3(256), 0,
                     (hipStream_t)stream, reinterpret_cast<const f32x4*>(canvas), H, W, reinterpret_cast<f32x4*>(out_a),
                     geom(views[0], H, W), reinterpret_cast<f32x4*>(out_b), geom(views[1], H, W), pad_value);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_yolo_decode_view(const float* head, int B, int ny, int nx, int na, float stride, const float* anchors_px, float* out,
                        int64_t out_image_stride, int64_t out_row_offset, float si, int flip, int img_w, int lm_mode,
                        void* stream) {
  if (!head || !anchors_px || !out || B < 0 || ny <= 0 || nx <= 0 || na != 3) return FP_ERR_INVALID_ARG;
  if (!(si > 0.f) || (flip != 0 && flip != 1) || img_w <= 0 || (lm_mode != 0 && lm_mode != 1) || out_image_stride < 0 ||
      out_row_offset < 0)
    return FP_ERR_INVALID_ARG;
  if (((uintptr_t)out) % 16 || out_image_stride % 4) return FP_ERR_ALIGNMENT;
  if (B == 0) return FP_OK;
  const long total = (long)B * na * ny * nx;
  hipLaunchKernelGGL(yolo_decode_view_kernel, dim3((unsigned)fp_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     head, B, ny, nx, na, stride, anchors_px[0], anchors_px[1], anchors_px[2], anchors_px[3], anchors_px[4],
                     anchors_px[5], out, (long)out_image_stride, (long)out_row_offset, si, flip, (float)img_w, lm_mode);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
