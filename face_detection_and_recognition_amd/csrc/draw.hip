// draw.hip — fp_draw / fp_draw_check / fp_draw_emulate (include/facepath.h "Drawing on device frames", DESIGN §7 "Drawing"):
// boxes, landmark rings, captions and mosaic rectangles rasterised in place into u8 BGR frames, dense or ragged (gfx950).
//
// One workgroup of 256 threads per touched 64 x 64 tile:
//   1. the tile's rows (at most 64 x 192 bytes, at byte-granular global offsets) go to LDS: a wave per row, head bytes up to
//      the first 4-byte aligned address, dwords, tail bytes.  The LDS row keeps the global row's offset mod 4 (LDS byte =
//      row * 196 + (address & 3) + i), so the dword stores to LDS are aligned too;
//   2. the frame's command range is walked in chunks of 256: a lane per command tests kind, ranges and bounding box against
//      the tile, a ballot and the waves' counts give each kept command its place in an LDS list that preserves list order;
//   3. the kept commands are applied one after another to the LDS tile, a barrier between them; every thread takes the
//      pixels i, i + 256, ... of (bounding box ∩ tile ∩ frame).  MOSAIC: a thread per 4 x 4 block sums its pixels inside the
//      rectangle (reduce), barrier, then adds up the blocks of its cell and writes the mean to its own pixels (write): a
//      tile is a multiple of every cell and tiles are anchored at the frame's origin as the cells are, so no cell straddles two;
//   4. the rows are stored the way they were loaded.
// Tiles are disjoint byte ranges and only dwords that lie wholly inside a row segment are moved as dwords: no byte of another
// tile is read-modify-written, drawing in place is race-free, there are no atomics and no scratch.
// The predicates and the blend are shared with the serial host emulator; the numpy restatement (annotate.draw_numpy) is
// written independently of them.
#include "common.h"

namespace {

constexpr int TILE = FP_DRAW_TILE;
constexpr int LROW = TILE * 3 + 4;          // LDS bytes per tile row: 192 + the row's address mod 4, a multiple of 4
constexpr int CHUNK = 256;                  // commands per compaction chunk = threads per workgroup

struct Box {
  int x0, y0, x1, y1;
};

__host__ __device__ inline bool coord_ok(int v) { return v >= -FP_DRAW_MAX_COORD && v <= FP_DRAW_MAX_COORD; }

// The bounding box of the pixels a command may set (not clipped); false for a command the procedure skips.
__host__ __device__ inline bool cmd_box(const fp_draw_cmd& c, Box& b) {
  if (!coord_ok(c.x0) || !coord_ok(c.y0)) return false;
  const int a = c.arg;
  switch (c.kind) {
    case FP_DRAW_RECT:
      if (a < 1 || a > FP_DRAW_MAX_ARG || !coord_ok(c.x1) || !coord_ok(c.y1)) return false;
      b = {c.x0 - a / 2, c.y0 - a / 2, c.x1 + a / 2, c.y1 + a / 2};
      break;
    case FP_DRAW_FILL:
      if (!coord_ok(c.x1) || !coord_ok(c.y1)) return false;
      b = {c.x0, c.y0, c.x1, c.y1};
      break;
    case FP_DRAW_MOSAIC:
      if ((a != 4 && a != 8 && a != 16 && a != 32) || !coord_ok(c.x1) || !coord_ok(c.y1)) return false;
      b = {c.x0, c.y0, c.x1, c.y1};
      break;
    case FP_DRAW_RING:
      if (a < 0 || a > FP_DRAW_MAX_ARG) return false;
      b = {c.x0 - a, c.y0 - a, c.x0 + a + 1, c.y0 + a + 1};
      break;
    case FP_DRAW_GLYPH: {
      const int code = a & 255, s = a >> 8;
      if (a < 0 || code < 32 || code > 126 || s < 1 || s > FP_DRAW_MAX_SCALE) return false;
      b = {c.x0, c.y0, c.x0 + 6 * s, c.y0 + 8 * s};
      break;
    }
    default:
      return false;
  }
  return b.x0 < b.x1 && b.y0 < b.y1;
}

__host__ __device__ inline Box clip(const Box& a, int x0, int y0, int x1, int y1) {
  return {a.x0 > x0 ? a.x0 : x0, a.y0 > y0 ? a.y0 : y0, a.x1 < x1 ? a.x1 : x1, a.y1 < y1 ? a.y1 : y1};
}

// RECT / FILL / RING / GLYPH: does the command set pixel (x, y) of its bounding box?
__host__ __device__ inline bool cmd_sets(const fp_draw_cmd& c, int x, int y, const uint8_t* font) {
  switch (c.kind) {
    case FP_DRAW_RECT: {
      const int s = (c.arg + 1) / 2;     // inside the shrunk rectangle: not set
      return !(x >= c.x0 + s && x < c.x1 - s && y >= c.y0 + s && y < c.y1 - s);
    }
    case FP_DRAW_FILL:
      return true;
    case FP_DRAW_RING: {
      const int dx = x - c.x0, dy = y - c.y0, r2 = 2 * c.arg;
      const int d = 4 * (dx * dx + dy * dy);       // |dx|, |dy| <= r <= 4096 inside the bounding box
      return (r2 - 1) * (r2 - 1) <= d && d < (r2 + 1) * (r2 + 1);
    }
    case FP_DRAW_GLYPH: {
      const int code = c.arg & 255, s = c.arg >> 8;
      const int gx = (x - c.x0) / s, gy = (y - c.y0) / s;
      return (font[(code - 32) * 8 + gy] >> (7 - gx)) & 1;
    }
  }
  return false;
}

__host__ __device__ inline uint8_t blend(unsigned dst, unsigned col, unsigned a) {
  return (uint8_t)((dst * (255u - a) + col * a + 127u) / 255u);
}

__host__ __device__ inline bool desc_ok(const fp_frame_desc& d, size_t frames_bytes) {
  if (d.w < 1 || d.w > FP_FRAME_MAX_W || d.h < 1 || d.h > FP_FRAME_MAX_H || d.off < 0) return false;
  const unsigned long long bytes = 3ull * (unsigned long long)d.w * (unsigned long long)d.h;
  return (unsigned long long)d.off <= (unsigned long long)frames_bytes && bytes <= (unsigned long long)frames_bytes - (unsigned long long)d.off;
}

// Rows of the tile between global memory and LDS.  g = the tile's pixel (0, 0), row pitch w3 bytes, n bytes per row.
template <bool STORE>
__device__ __forceinline__ void move_rows(uint8_t* g, long w3, int n, int th, uint8_t* tile, int wave, int lane) {
  for (int py = wave; py < th; py += 4) {
    uint8_t* gr = g + py * w3;
    const int sh = (int)((uintptr_t)gr & 3);
    uint8_t* lr = tile + py * LROW + sh;
    int head = (4 - sh) & 3;
    head = head < n ? head : n;
    const int nd = (n - head) >> 2, tail = n - head - 4 * nd;     // nd <= 48
    if (lane < nd) {
      if (STORE) *(unsigned*)(gr + head + 4 * lane) = *(const unsigned*)(lr + head + 4 * lane);
      else *(unsigned*)(lr + head + 4 * lane) = *(const unsigned*)(gr + head + 4 * lane);
    } else if (lane >= 48 && lane < 48 + head) {
      const int i = lane - 48;
      if (STORE) gr[i] = lr[i];
      else lr[i] = gr[i];
    } else if (lane >= 52 && lane < 52 + tail) {
      const int i = head + 4 * nd + (lane - 52);
      if (STORE) gr[i] = lr[i];
      else lr[i] = gr[i];
    }
  }
}

__global__ __launch_bounds__(256) void draw_tiles_kernel(uint8_t* __restrict__ frames, size_t frames_bytes,
                                                         const fp_frame_desc* __restrict__ descs, int n_frames,
                                                         const fp_draw_cmd* __restrict__ cmds, const int* __restrict__ ranges,
                                                         int n_cmds, const int* __restrict__ tiles,
                                                         const uint8_t* __restrict__ font_g) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[TILE * LROW];
  __shared__ __attribute__((aligned(16))) fp_draw_cmd kept[CHUNK];
  __shared__ __attribute__((aligned(8))) unsigned short part[256][4];   // MOSAIC: per 4 x 4 block, sums of B, G, R and the count
  __shared__ uint8_t font[FP_DRAW_FONT_BYTES + 8];
  __shared__ int wcount[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = tiles[blockIdx.x * 3], tx = tiles[blockIdx.x * 3 + 1], ty = tiles[blockIdx.x * 3 + 2];
  if (f < 0 || f >= n_frames || tx < 0 || ty < 0) return;               // uniform: the whole workgroup leaves
  const fp_frame_desc d = descs[f];
  if (!desc_ok(d, frames_bytes) || tx > d.w / TILE || ty > d.h / TILE) return;
  const int ox = tx * TILE, oy = ty * TILE;
  if (ox >= d.w || oy >= d.h) return;
  const int tw = d.w - ox < TILE ? d.w - ox : TILE, th = d.h - oy < TILE ? d.h - oy : TILE;
  int r0 = ranges[f], r1 = ranges[f + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > n_cmds ? n_cmds : r1;
  if (r0 >= r1) return;

  const long w3 = 3L * d.w;
  uint8_t* g = frames + d.off + (long)oy * w3 + 3L * ox;
  for (int i = tid; i < FP_DRAW_FONT_BYTES; i += 256) font[i] = font_g[i];
  move_rows<false>(g, w3, tw * 3, th, tile, wave, lane);
  // LDS byte of channel 0 of tile pixel (px, py): the row's global address mod 4 in front
  const int a0 = (int)((uintptr_t)g & 3), wm = (int)(w3 & 3);
  auto at = [&](int px, int py) { return tile + py * LROW + ((a0 + py * wm) & 3) + px * 3; };

  for (int base = r0; base < r1; base += CHUNK) {
    const int i = base + tid;
    fp_draw_cmd c;
    bool keep = false;
    if (i < r1) {
      c = cmds[i];
      Box b;
      if (c.frame == f && cmd_box(c, b)) keep = b.x0 < ox + tw && b.x1 > ox && b.y0 < oy + th && b.y1 > oy;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wcount[wave] = __popcll(m);
    __syncthreads();                       // the counts; the tile and the font before the first chunk's commands
    int pos = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
    for (int k = 0; k < 4; ++k) {
      const int n = wcount[k];
      pos += k < wave ? n : 0;
      total += n;
    }
    if (keep) kept[pos] = c;
    __syncthreads();
    for (int k = 0; k < total; ++k) {
      const fp_draw_cmd q = kept[k];       // the same address in every lane
      Box b;
      cmd_box(q, b);
      b = clip(b, ox, oy, ox + tw, oy + th);
      if (q.kind == FP_DRAW_MOSAIC) {
        const int bx = ox + 4 * (tid & 15), by = oy + 4 * (tid >> 4);
        const Box mine = clip(b, bx, by, bx + 4, by + 4);
        unsigned s0 = 0, s1 = 0, s2 = 0, n = 0;
        for (int y = mine.y0; y < mine.y1; ++y)
          for (int x = mine.x0; x < mine.x1; ++x) {
            const uint8_t* p = at(x - ox, y - oy);
            s0 += p[0]; s1 += p[1]; s2 += p[2]; ++n;
          }
        part[tid][0] = (unsigned short)s0; part[tid][1] = (unsigned short)s1;      // <= 16 * 255
        part[tid][2] = (unsigned short)s2; part[tid][3] = (unsigned short)n;
        __syncthreads();
        if (n) {
          const int qn = q.arg >> 2;                                                // blocks per cell side: 1, 2, 4, 8
          const int cx = (tid & 15) & ~(qn - 1), cy = (tid >> 4) & ~(qn - 1);
          unsigned t0 = 0, t1 = 0, t2 = 0, cnt = 0;
          for (int j = 0; j < qn; ++j)
            for (int ii = 0; ii < qn; ++ii) {
              const unsigned short* pp = part[(cy + j) * 16 + cx + ii];
              t0 += pp[0]; t1 += pp[1]; t2 += pp[2]; cnt += pp[3];
            }
          const uint8_t m0 = (uint8_t)((t0 + cnt / 2) / cnt), m1 = (uint8_t)((t1 + cnt / 2) / cnt), m2 = (uint8_t)((t2 + cnt / 2) / cnt);
          for (int y = mine.y0; y < mine.y1; ++y)
            for (int x = mine.x0; x < mine.x1; ++x) {
              uint8_t* p = at(x - ox, y - oy);
              p[0] = m0; p[1] = m1; p[2] = m2;
            }
        }
      } else {
        const int bw = b.x1 - b.x0, n = bw * (b.y1 - b.y0);
        for (int j = tid; j < n; j += 256) {
          const int yy = j / bw, x = b.x0 + (j - yy * bw), y = b.y0 + yy;
          if (!cmd_sets(q, x, y, font)) continue;
          uint8_t* p = at(x - ox, y - oy);
          p[0] = blend(p[0], q.b, q.a);
          p[1] = blend(p[1], q.g, q.a);
          p[2] = blend(p[2], q.r, q.a);
        }
      }
      __syncthreads();
    }
  }
  move_rows<true>(g, w3, tw * 3, th, tile, wave, lane);
}

bool cell_ok(int a) { return a == 4 || a == 8 || a == 16 || a == 32; }

}  // namespace

extern "C" {

int fp_draw(uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const fp_draw_cmd* cmds,
            const int32_t* cmd_ranges, int n_cmds, const int32_t* tiles, int n_tiles, const uint8_t* font, void* stream) {
  if (n_frames < 0 || n_cmds < 0 || n_tiles < 0) return FP_ERR_INVALID_ARG;
  if (!frames || !descs || !cmd_ranges || !font || (n_cmds > 0 && !cmds) || (n_tiles > 0 && !tiles)) return FP_ERR_INVALID_ARG;
  if (n_tiles == 0 || n_cmds == 0 || n_frames == 0) return FP_OK;
  hipLaunchKernelGGL(draw_tiles_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, frames, frames_bytes, descs,
                     n_frames, cmds, (const int*)cmd_ranges, n_cmds, (const int*)tiles, font);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

int fp_draw_check(size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const fp_draw_cmd* cmds,
                  const int32_t* cmd_ranges, int n_cmds, const int32_t* tiles, int n_tiles) {
  if (n_frames < 0 || n_cmds < 0 || n_tiles < 0) return FP_ERR_INVALID_ARG;
  if (!descs || !cmd_ranges || (n_cmds > 0 && !cmds) || (n_tiles > 0 && !tiles)) return FP_ERR_INVALID_ARG;
  for (int f = 0; f < n_frames; ++f)
    if (!desc_ok(descs[f], frames_bytes)) return FP_ERR_INVALID_ARG;
  if (cmd_ranges[0] != 0 || cmd_ranges[n_frames] != n_cmds) return FP_ERR_INVALID_ARG;
  for (int f = 0; f < n_frames; ++f) {
    if (cmd_ranges[f] < 0 || cmd_ranges[f] > cmd_ranges[f + 1] || cmd_ranges[f + 1] > n_cmds) return FP_ERR_INVALID_ARG;
    for (int i = cmd_ranges[f]; i < cmd_ranges[f + 1]; ++i) {
      if (cmds[i].frame != f) return FP_ERR_INVALID_ARG;
      if (cmds[i].kind == FP_DRAW_MOSAIC && !cell_ok(cmds[i].arg)) return FP_ERR_INVALID_ARG;
    }
  }
  for (int t = 0; t < n_tiles; ++t) {
    const int32_t* q = tiles + 3 * t;
    if (q[0] < 0 || q[0] >= n_frames || q[1] < 0 || q[2] < 0) return FP_ERR_INVALID_ARG;
    if ((long)q[1] * TILE >= descs[q[0]].w || (long)q[2] * TILE >= descs[q[0]].h) return FP_ERR_INVALID_ARG;
    if (t > 0) {
      const int32_t* p = q - 3;
      const bool asc = p[0] != q[0] ? p[0] < q[0] : p[1] != q[1] ? p[1] < q[1] : p[2] < q[2];
      if (!asc) return FP_ERR_INVALID_ARG;
    }
  }
  return FP_OK;
}

int fp_draw_emulate(uint8_t* frames, size_t frames_bytes, const fp_frame_desc* descs, int n_frames, const fp_draw_cmd* cmds,
                    const int32_t* cmd_ranges, int n_cmds, const int32_t* tiles, int n_tiles, const uint8_t* font) {
  if (!frames || !font) return FP_ERR_INVALID_ARG;
  const int rc = fp_draw_check(frames_bytes, descs, n_frames, cmds, cmd_ranges, n_cmds, tiles, n_tiles);
  if (rc != FP_OK) return rc;
  for (int t = 0; t < n_tiles; ++t) {
    const int f = tiles[3 * t], ox = tiles[3 * t + 1] * TILE, oy = tiles[3 * t + 2] * TILE;
    const fp_frame_desc& d = descs[f];
    const int ex = ox + TILE < d.w ? ox + TILE : d.w, ey = oy + TILE < d.h ? oy + TILE : d.h;
    uint8_t* img = frames + d.off;
    auto at = [&](int x, int y) { return img + ((long)y * d.w + x) * 3; };
    for (int i = cmd_ranges[f]; i < cmd_ranges[f + 1]; ++i) {
      const fp_draw_cmd& c = cmds[i];
      Box b;
      if (c.frame != f || !cmd_box(c, b)) continue;
      b = clip(b, ox, oy, ex, ey);
      if (b.x0 >= b.x1 || b.y0 >= b.y1) continue;
      if (c.kind == FP_DRAW_MOSAIC) {
        const int cell = c.arg;
        for (int cy = b.y0 / cell * cell; cy < b.y1; cy += cell)
          for (int cx = b.x0 / cell * cell; cx < b.x1; cx += cell) {
            const Box m = clip(b, cx, cy, cx + cell, cy + cell);
            unsigned s[3] = {0, 0, 0}, n = 0;
            for (int y = m.y0; y < m.y1; ++y)
              for (int x = m.x0; x < m.x1; ++x, ++n)
                for (int k = 0; k < 3; ++k) s[k] += at(x, y)[k];
            if (!n) continue;
            for (int y = m.y0; y < m.y1; ++y)
              for (int x = m.x0; x < m.x1; ++x)
                for (int k = 0; k < 3; ++k) at(x, y)[k] = (uint8_t)((s[k] + n / 2) / n);
          }
        continue;
      }
      for (int y = b.y0; y < b.y1; ++y)
        for (int x = b.x0; x < b.x1; ++x) {
          if (!cmd_sets(c, x, y, font)) continue;
          uint8_t* p = at(x, y);
          p[0] = blend(p[0], c.b, c.a);
          p[1] = blend(p[1], c.g, c.a);
          p[2] = blend(p[2], c.r, c.a);
        }
    }
  }
  return FP_OK;
}

}  // extern "C"
