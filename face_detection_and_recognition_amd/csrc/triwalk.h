// triwalk.h — the triangular work list of the all-pairs walks over the upper triangle of X X^T (cluster.hip, pairhist.hip):
// row tiles of 128 rows x 128-column chunks, a chunk is walked when it is not wholly at or below its row tile's first row.
#pragma once
#include "cosinewalk.h"

constexpr int CL_ROWS = CW_NC;   // rows of a row tile = columns of a chunk: tile r starts on the diagonal at chunk r

// Row tile r walks the m = nchunk - r chunks r .. nchunk - 1, cut into ceil(m / P) workgroups of nearly equal, contiguous
// chunk ranges (at most P each).  Items are numbered by increasing m: tile m = P b + e + 1 (0 <= e < P) has b + 1 groups and
// the tiles before it hold  P b (b + 1) / 2 + e (b + 1)  groups.  A kernel decodes item gridDim.x - 1 - fp_xcd_block(): the
// longest rows first, the groups of one row tile next to each other on ONE XCD (its rows from that L2).
struct cl_item {
  int tile, first, count;   // row tile, first chunk, chunks
};
__host__ __device__ inline long cl_groups(long nchunk, long P) {
  const long b = nchunk / P, e = nchunk - b * P;
  return P * b * (b + 1) / 2 + e * (b + 1);
}
__host__ __device__ inline cl_item cl_decode(long v, int nchunk, int P) {
  long b = (long)((sqrt(1.0 + 8.0 * (double)v / (double)P) - 1.0) * 0.5);
  while (b > 0 && P * b * (b + 1) / 2 > v) --b;
  while (P * (b + 1) * (b + 2) / 2 <= v) ++b;
  const long rem = v - P * b * (b + 1) / 2;
  const long e = rem / (b + 1), g = rem - e * (b + 1);
  const long m = P * b + e + 1, base = m / (b + 1), extra = m - base * (b + 1);
  cl_item it;
  it.tile = (int)(nchunk - m);
  it.first = it.tile + (int)(g * base + (g < extra ? g : extra));
  it.count = (int)(base + (g < extra ? 1 : 0));
  return it;
}

// Chunks per workgroup: about four rounds of the workgroups the device holds (wg_per_cu per CU), at most 16 chunks each.
static inline long cl_chunks_per_group(int nchunk, int wg_per_cu) {
  const long total = (long)nchunk * (nchunk + 1) / 2;
  const long P = total / (4L * wg_per_cu * fp_num_cus());
  return P < 1 ? 1 : P > 16 ? 16 : P;
}
