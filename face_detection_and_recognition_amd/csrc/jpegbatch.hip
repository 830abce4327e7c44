// jpegbatch.hip — JPEG reconstruction of a BATCH of frames that share one geometry (the frames of a Motion-JPEG video): the
// device half of csrc/jpeg.hip for n frames in one launch sequence, writing straight into an (n, H, W, 3) u8 tensor (gfx950).
//
// fp_jpeg_reconstruct takes one frame: a workspace and two launches each, and the caller stacks the frames afterwards.  Where
// every frame has the same size and sampling the two kernels simply get a frame index:
//   jpeg_idct_batch_kernel    one thread per 8 x 8 block of the batch: frame f = block / blocks-per-frame; the frame's own
//                             coefficient offset (coef_off[f], device) and quantisation tables (quant[f], device: a camera may
//                             change its quality mid-stream) -> the frame's sample planes in the workspace
//   jpeg_color_batch_kernel   one thread per output pixel of the batch -> out[f][y][x][0..2]
// The arithmetic is jpegrecon.h's (jpeg_idct_block, chroma_sample, jpeg_color_pixel), the functions fp_jpeg_reconstruct's
// kernels call: the bytes are the same.  All indices are 64-bit: n x blocks x 64 passes 2^31 at 4K from 21 frames on.
// Scope: full size, no orientation (AVI carries no EXIF); reduced sizes go frame by frame through csrc/jpegscale.hip.
#include "common.h"
#include "jpegrecon.h"

namespace {

__global__ __launch_bounds__(64) void jpeg_idct_batch_kernel(const short* coefs, const long* coef_off, const unsigned short* quant,
                                                             unsigned char* planes, JpegDevInfo info, long nblocks, long plane_stride,
                                                             long total) {
  const long g = (long)blockIdx.x * 64 + threadIdx.x;
  if (g >= total) return;
  const long f = g / nblocks;
  long bb = g - f * nblocks;
  const int c = jpeg_block_component(info, bb);
  const int bx = (int)(bb % info.blocks_w[c]), by = (int)(bb / info.blocks_w[c]);
  const long pitch = info.blocks_w[c] * 8;
  jpeg_idct_block(coefs + coef_off[f] + info.coef_off[c] + bb * 64, quant + (f * 3 + c) * 64,
                  planes + f * plane_stride + info.plane_off[c] + ((long)by * 8) * pitch + bx * 8, pitch);
}

__global__ __launch_bounds__(256) void jpeg_color_batch_kernel(const unsigned char* planes, unsigned char* out, JpegDevInfo info,
                                                               long plane_stride, long npx, long total, int bgr) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long f = i / npx;
  const long p = i - f * npx;
  const int oy = (int)(p / info.width), ox = (int)(p - (long)oy * info.width);
  jpeg_color_pixel(planes + f * plane_stride, out + i * 3, info, oy, ox, bgr);
}

// what the kernels' addressing relies on: every read of a plane stays inside it
bool geometry_ok(const fp_jpeg_info* info) {
  if (info->ncomp != 1 && info->ncomp != 3) return false;
  if (info->width <= 0 || info->height <= 0) return false;
  for (int c = 0; c < info->ncomp; ++c) {
    if (info->blocks_w[c] <= 0 || info->blocks_h[c] <= 0 || info->coef_off[c] < 0) return false;
    if (info->comp_w[c] <= 0 || info->comp_h[c] <= 0) return false;
    if (info->comp_w[c] > (long)info->blocks_w[c] * 8 || info->comp_h[c] > (long)info->blocks_h[c] * 8) return false;
  }
  if (info->width > (long)info->blocks_w[0] * 8 || info->height > (long)info->blocks_h[0] * 8) return false;
  if (info->ncomp == 3) {
    const int hs = info->hs[0], vs = info->vs[0];
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    for (int c = 1; c < 3; ++c)
      if (info->comp_w[c] < (info->width + hs - 1) / hs || info->comp_h[c] < (info->height + vs - 1) / vs) return false;
  }
  return true;
}

}  // namespace

extern "C" {

size_t fp_jpeg_batch_workspace_bytes(const fp_jpeg_info* info, int n_frames) {
  if (!info || n_frames <= 0) return 0;
  return fp_jpeg_workspace_bytes(info) * (size_t)n_frames;
}

int fp_jpeg_reconstruct_batch(const int16_t* coefs, const int64_t* coef_off, const uint16_t* quant, const fp_jpeg_info* info,
                              int n_frames, uint8_t* workspace, size_t ws_bytes, uint8_t* out, int bgr, void* stream) {
  if (!coefs || !coef_off || !quant || !info || !workspace || !out || n_frames <= 0) return FP_ERR_INVALID_ARG;
  if (info->ncomp != 1 && info->ncomp != 3) return FP_ERR_UNSUPPORTED;
  if (!geometry_ok(info)) return FP_ERR_INVALID_ARG;
  if (ws_bytes < fp_jpeg_batch_workspace_bytes(info, n_frames)) return FP_ERR_BOUNDS;
  if (((uintptr_t)workspace) % 8 || ((uintptr_t)coefs) % 2 || ((uintptr_t)coef_off) % 8 || ((uintptr_t)quant) % 2) return FP_ERR_ALIGNMENT;
  JpegDevInfo d;
  long nblocks = 0, plane_bytes = 0;
  if (!jpeg_dev_info(info, d, nblocks, plane_bytes)) return FP_ERR_INVALID_ARG;
  const long plane_stride = (long)fp_jpeg_workspace_bytes(info);       // a multiple of 16: every frame's planes 8-byte aligned
  const long npx = (long)info->width * info->height;
  const long total_blocks = nblocks * n_frames, total_px = npx * n_frames;
  const long g0 = (total_blocks + 63) / 64, g1 = (total_px + 255) / 256;
  if (g0 > 0x7fffffffL || g1 > 0x7fffffffL) return FP_ERR_UNSUPPORTED;  // one launch's grid: split the batch
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_idct_batch_kernel, dim3((unsigned)g0), dim3(64), 0, s, (const short*)coefs, (const long*)coef_off,
                     (const unsigned short*)quant, workspace, d, nblocks, plane_stride, total_blocks);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_color_batch_kernel, dim3((unsigned)g1), dim3(256), 0, s, workspace, out, d, plane_stride, npx, total_px, bgr);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

}  // extern "C"
