// jpegdec.hip — Huffman decoding of sequential JPEG scans on the device (gfx950 + host emulator), bit-exact with
// fp_jpeg_entropy_decode (csrc/jpeg.hip), damaged files included.
//
// A scan without restart markers is one serial bit stream: a codeword boundary is known only at its start.  The decoder
// splits every restart segment into subsequences of S bits, one lane each, and uses that Huffman codes resynchronise
// after a few symbols (the self-synchronising scheme):
//   unstuff    one workgroup per image: drops the 0x00 behind each 0xff, cuts the data at the first marker that is not the
//              next expected RSTn (zero bits follow it, as BitReader::fill feeds them), records where each restart segment
//              starts, lays the lanes out (jd_unstuff).  0xff 0xff in the scan -- fill bytes, which may stand in front of
//              any marker, an RSTn included (JPEG B.1.1.2) -- ends the device attempt: the image is handed to the host
//              decoder (FP_JPEG_DECODE_ON_HOST), which skips them as libjpeg does; never refused, never decoded differently
//   speculate  every lane decodes the symbols that START in its subsequence from state (block slot 0, k = 0) -- exact at a
//              segment start -- and records its exit (bit offset, slot, k at the first boundary at or past its end) and the
//              number of DC symbols it decoded (jd_spec)
//   sync       lane i re-decodes from lane i-1's exit; inside a workgroup this iterates in LDS, across workgroups the round
//              kernel is launched again (jd_round, at most max_rounds launches, no inter-workgroup waits).  A round in
//              which no exit of an image changed proves, by induction from the exact first lane of every segment, that every
//              lane's entry is the serial decode's: the image is synchronised.  An image not proven after max_rounds is
//              left to the host (FP_JPEG_DECODE_ON_HOST).  The block counts are those of the proving round: every lane
//              decoded from its true entry there (a lane that resynchronised reproduces its exit, not its speculative count)
//   locate     one workgroup per image: an exclusive scan of the block counts places every lane's first block; errors on the
//              proven path (invalid code, k > 63, DC size > 11 -- before the segment's last block), a segment the data runs
//              out in (decoded on from zero bits up to its last block) and a missing RSTn give the image's first error in
//              decode order and its status (jd_locate)
//   write      every lane re-decodes from its proven entry: AC coefficients de-zigzagged into their blocks (zeroed first,
//              jd_zero), DC differences into per-block scratch, nothing behind the first error (jd_write)
//   dc         one workgroup per image: per-component prefix sums of the DC differences in decode order, reset at every
//              restart segment, stored as (int16_t) of the running int (jd_dc)
// The per-lane decode (lane_run: symbol decode, state transition, block-slot walk) is __host__ __device__ code: the emulator
// (fp_jpeg_entropy_decode_emulate) runs the same phases serially on the CPU with it, which is what the CPU tests and the
// sanitizer fuzzer (tools/fuzz/jpeg_device_fuzz.cpp) check against fp_jpeg_entropy_decode.
#include <string.h>

#include <vector>

#include "common.h"

namespace {

#define HD __host__ __device__

constexpr int kLanesPerWg = 64;        // one wave per workgroup in the lane kernels
constexpr int kImgThreads = 256;       // the per-image kernels (unstuff, locate, dc)
constexpr int kLocalIters = 8;         // LDS iterations of jd_round inside one workgroup
constexpr int kChunk = 16;             // bytes per thread and step in jd_unstuff

// term: what ended the scan data
constexpr int kTermEnd = 0;            // EOI, the end of the file (a lone 0xff as its last byte included)
constexpr int kTermMarker = 1;         // another marker (DHT / SOS / COM / an RSTn behind the last segment ...): host
constexpr int kTermHost = 2;           // 0xff 0xff fill bytes in the scan, too many lanes: host

// lane exit word: bit offset | slot << 32 | k << 36 | flags
constexpr unsigned long long kErr = 1ull << 48;    // the decode met an invalid symbol (the error block index in the count)
constexpr unsigned long long kDcOk = 1ull << 49;   // ... after the block's DC symbol
constexpr unsigned long long kDead = 1ull << 50;   // (lane_entry only) the predecessor ended in an error: no entry

HD inline unsigned long long pack_exit(unsigned pos, int slot, int k) {
  return (unsigned long long)pos | ((unsigned long long)slot << 32) | ((unsigned long long)k << 36);
}
HD inline unsigned exit_pos(unsigned long long e) { return (unsigned)e; }
HD inline int exit_slot(unsigned long long e) { return (int)((e >> 32) & 15); }
HD inline int exit_k(unsigned long long e) { return (int)((e >> 36) & 127); }

HD inline int jd_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

#ifdef __HIP_DEVICE_COMPILE__
__device__ __constant__ unsigned char kZigzagDev[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
#else
const unsigned char kZigzagHost[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
#endif

HD inline int zigzag(int k) {
#ifdef __HIP_DEVICE_COMPILE__
  return kZigzagDev[k];
#else
  return kZigzagHost[k];
#endif
}

// next 32 bits from bit pos (zero-extended to 16 bits of symbol lookahead: jpeg.hip's huff_decode semantics)
HD inline int huff_sym(const fp_jpeg_huff* h, unsigned w, int& len) {
  const unsigned e = h->look[w >> 23];
  if (e) {
    len = (int)(e >> 8);
    return (int)(e & 255);
  }
  for (int l = 10; l <= 16; ++l) {
    const int code = (int)(w >> (32 - l));
    if (code <= h->maxcode[l]) {
      len = l;
      return h->vals[(code + h->valoff[l]) & 255];
    }
  }
  return -1;
}

// The geometry one image's lanes need (from its fp_jpeg_scan).
struct Geo {
  int bpm, mcux;
  int slot_tab[8];
  long slot_base[8];            // coefficient offset of slot s's block in MCU (0, 0)
  long slot_mcu_col[8];         // ... added per MCU column
  long slot_mcu_row[8];         // ... per MCU row
  HD void init(const fp_jpeg_scan& s) {
    bpm = s.blocks_per_mcu;
    mcux = s.mcux;
    for (int i = 0; i < 8; ++i) {
      slot_tab[i] = s.slot_tab[i];
      const int c = s.slot_comp[i];
      slot_base[i] = i < bpm ? s.coef_off[c] + ((long)s.slot_dy[i] * s.blocks_w[c] + s.slot_dx[i]) * 64 : 0;
      slot_mcu_col[i] = i < bpm ? (long)s.hs[c] * 64 : 0;
      slot_mcu_row[i] = i < bpm ? (long)s.vs[c] * s.blocks_w[c] * 64 : 0;
    }
  }
  HD long block_addr(int b) const {     // jpeg.hip decode_scan's address of the b-th block in decode order
    const int mcu = b / bpm, slot = b - mcu * bpm;
    const int my = mcu / mcux, mx = mcu - my * mcux;
    return slot_base[slot] + (long)my * slot_mcu_row[slot] + (long)mx * slot_mcu_col[slot];
  }
};

// One lane's bit reader over an unstuffed restart segment: bits at or past end_byte read as zeros.
struct Bits {
  const unsigned char* u;
  unsigned end_byte;
  unsigned cbyte;
  unsigned long long cache;     // bytes cbyte .. cbyte + 7, big-endian
  HD void load(unsigned b) {
    cbyte = b;
    unsigned long long c = 0;
    for (int i = 0; i < 8; ++i) c = (c << 8) | (b + i < end_byte ? u[b + i] : 0u);
    cache = c;
  }
  HD unsigned peek(unsigned pos) {
    const unsigned b = pos >> 3;
    if (b - cbyte > 3) load(b);
    return (unsigned)((cache << (pos - cbyte * 8)) >> 32);
  }
};

struct Tabs {
  const fp_jpeg_huff* dc;       // [3]
  const fp_jpeg_huff* ac;       // [3]
};

// The per-lane decode step.  From state (pos, slot, k) with b = the index of the block in progress (k > 0) or of the next
// block (k == 0): decodes symbol after symbol until the first boundary at or past `end`, or, at a block boundary, until
// the next block would be stop_block, or an error.  Returns the exit word; b is the block index at exit and count the number of
// DC symbols decoded.  WRITE: AC coefficients into coefs (de-zigzagged), DC differences into dcdiff[b].
template <bool WRITE>
HD unsigned long long lane_run(Bits& br, const Tabs& t, const Geo& g, unsigned pos, int slot, int k, unsigned end, int& b,
                               int stop_block, int& count, short* coefs, int* dcdiff) {
  count = 0;
  long blk = 0;
  if (WRITE && k > 0) blk = g.block_addr(b);
  for (;;) {
    if (pos >= end) break;
    if (k == 0 && b >= stop_block) break;
    const unsigned w = br.peek(pos);
    const int tb = g.slot_tab[slot];
    int len = 0;
    if (k == 0) {
      const int s = huff_sym(t.dc + tb, w, len);
      if (s < 0 || s > 11) return pack_exit(pos, slot, k) | kErr;
      int diff = 0;
      if (s) diff = jd_extend((int)((w << len) >> (32 - s)), s);
      pos += (unsigned)(len + s);
      if (WRITE) {
        dcdiff[b] = diff;
        blk = g.block_addr(b);
      }
      ++count;
      k = 1;
    } else {
      const int rs = huff_sym(t.ac + tb, w, len);
      if (rs < 0) return pack_exit(pos, slot, k) | kErr | kDcOk;
      const int r = rs >> 4, s = rs & 15;
      if (s == 0) {
        pos += (unsigned)len;
        k = r == 15 ? k + 16 : 64;                  // ZRL / EOB
      } else {
        k += r;
        if (k > 63) return pack_exit(pos, slot, k - r) | kErr | kDcOk;
        const int v = jd_extend((int)((w << len) >> (32 - s)), s);
        pos += (unsigned)(len + s);
        if (WRITE) coefs[blk + zigzag(k)] = (short)v;
        ++k;
      }
    }
    if (k >= 64) {
      k = 0;
      ++b;
      if (++slot == g.bpm) slot = 0;
    }
  }
  return pack_exit(pos, slot, k);
}

// ---------------------------------------------------------------------------------------------------------------------
// batch layout

struct JdImg {                  // per image, built on the host
  long file_off, coef_off;      // files + file_off: the file; coefs + coef_off: its coefficients
  long u_off;                   // unstuffed scan data (data_len bytes of capacity)
  long lane_base;               // first lane (a multiple of kLanesPerWg)
  long seg_base;                // seg_start / first_lane: seg_cap + 1 entries each
  long blk_base;                // dcdiff: nblocks entries
  long chg_base;                // changed flags of the rounds: max_rounds + 1 entries
  int lane_cap, seg_cap, nblocks, nseg;   // nseg: restart segments the image has
};

struct JdState {                // per image, written on the device
  int nl, nf, term, status;     // lanes, restart segments found, what ended the data, result
  int errkey, lim, ndc, pad;    // 2 * (first error block) + (its DC decoded); blocks written / with a DC
};

struct JdLayout {
  std::vector<JdImg> imgs;
  std::vector<int> wg_img;      // lane workgroup -> image
  size_t off_desc, off_img, off_state, off_wg, off_u, off_seg, off_first, off_serr, off_chg, off_dc, off_lseg, off_exit, off_cnt, off_b0;
  size_t total;
  long nlanes;
};

inline size_t align16(size_t x) { return (x + 15) / 16 * 16; }

inline int image_segments(const fp_jpeg_scan& s) {
  const long mcus = (long)s.mcux * s.mcuy;
  return s.restart_interval > 0 ? (int)((mcus + s.restart_interval - 1) / s.restart_interval) : 1;
}

bool plan_layout(const fp_jpeg_scan* scans, int n, int sub_bits, int max_rounds, JdLayout& L) {
  L.imgs.resize(n);
  L.wg_img.clear();
  long u = 0, seg = 0, blk = 0, lane = 0, chg = 0;
  for (int i = 0; i < n; ++i) {
    const fp_jpeg_scan& s = scans[i];
    if (s.data_len < 0 || s.data_len > FP_JPEG_DEV_MAX_BYTES || s.blocks_per_mcu < 1 || s.blocks_per_mcu > 6) return false;
    const long nblocks = (long)s.mcux * s.mcuy * s.blocks_per_mcu;
    if (s.mcux < 1 || s.mcuy < 1 || nblocks > FP_JPEG_DEV_MAX_BLOCKS) return false;
    JdImg& m = L.imgs[i];
    m.nseg = image_segments(s);
    m.seg_cap = m.nseg;
    m.nblocks = (int)nblocks;
    const long lanes = s.data_len * 8 / sub_bits + m.seg_cap + 1;
    m.lane_cap = (int)((lanes + kLanesPerWg - 1) / kLanesPerWg * kLanesPerWg);
    m.u_off = u;
    u += (s.data_len + 15) / 16 * 16;
    m.seg_base = seg;
    seg += m.seg_cap + 1;
    m.blk_base = blk;
    blk += nblocks;
    m.lane_base = lane;
    lane += m.lane_cap;
    m.chg_base = chg;
    chg += max_rounds + 1;
    for (int w = 0; w < m.lane_cap / kLanesPerWg; ++w) L.wg_img.push_back(i);
  }
  L.nlanes = lane;
  size_t o = 0;
  L.off_desc = o, o = align16(o + sizeof(fp_jpeg_scan) * n);
  L.off_img = o, o = align16(o + sizeof(JdImg) * n);
  L.off_state = o, o = align16(o + sizeof(JdState) * n);
  L.off_wg = o, o = align16(o + sizeof(int) * L.wg_img.size());
  L.off_u = o, o = align16(o + (size_t)u);
  L.off_seg = o, o = align16(o + sizeof(int) * seg);
  L.off_first = o, o = align16(o + sizeof(int) * seg);
  L.off_serr = o, o = align16(o + sizeof(int) * seg);
  L.off_chg = o, o = align16(o + sizeof(int) * chg);
  L.off_dc = o, o = align16(o + sizeof(int) * blk);
  L.off_lseg = o, o = align16(o + sizeof(int) * lane);
  L.off_exit = o, o = align16(o + 2 * sizeof(unsigned long long) * lane);
  L.off_cnt = o, o = align16(o + 2 * sizeof(int) * lane);
  L.off_b0 = o, o = align16(o + sizeof(int) * lane);
  L.total = o;
  return true;
}

struct JdPtrs {                 // device views of the workspace (the emulator fills the same with host memory)
  const unsigned char* files;
  short* coefs;
  int* status;
  const fp_jpeg_scan* desc;
  const JdImg* img;
  JdState* state;
  const int* wg_img;
  unsigned char* u;
  int* seg_start;               // byte offset of every found segment in the unstuffed data, [nf] = its end
  int* first_lane;              // first lane of every found segment, [nf] = nl
  int* seg_err;                 // first lane of every found segment whose exit is an error (INT_MAX: none)
  int* changed;
  int* dcdiff;
  int* lane_seg;
  unsigned long long* exits;    // [2][nlanes]
  int* counts;                  // [2][nlanes]
  int* b0;
  long nlanes;
  int sub_bits, max_rounds;
};

// ---- per-lane steps, shared by the kernels and the emulator ----

HD inline int quota_end(const fp_jpeg_scan& s, const JdImg& m, int seg) {     // one past the segment's last block
  if (s.restart_interval <= 0) return m.nblocks;
  const long e = (long)(seg + 1) * s.restart_interval * s.blocks_per_mcu;
  return e < m.nblocks ? (int)e : m.nblocks;
}

HD inline void lane_bounds(const JdPtrs& P, const JdImg& m, int li, int seg, unsigned& start, unsigned& end, bool& last) {
  const int* ss = P.seg_start + m.seg_base;
  const int* fl = P.first_lane + m.seg_base;
  const unsigned seg_end = (unsigned)ss[seg + 1] * 8u;
  start = (unsigned)ss[seg] * 8u + (unsigned)(li - fl[seg]) * (unsigned)P.sub_bits;
  last = li + 1 == fl[seg + 1];
  end = last ? seg_end : start + (unsigned)P.sub_bits;
}

HD inline void bits_for(const JdPtrs& P, const JdImg& m, int seg, Bits& br) {
  br.u = P.u + m.u_off;
  br.end_byte = (unsigned)P.seg_start[m.seg_base + seg + 1];
  br.load(0);
}

// entry of lane li in round r (reading exits buffer `in`): exact at a segment start, else the predecessor's exit
HD inline unsigned long long lane_entry(const JdPtrs& P, const JdImg& m, int li, int seg, unsigned start,
                                        const unsigned long long* in_pred) {
  if (li == P.first_lane[m.seg_base + seg]) return pack_exit(start, 0, 0);
  const unsigned long long e = *in_pred;
  return (e & (kErr | kDead)) ? kDead : e;
}

HD inline unsigned long long lane_sync(const JdPtrs& P, const Tabs& t, const Geo& g, const JdImg& m, int li, int seg,
                                       unsigned long long entry, int& count) {
  count = 0;
  unsigned start, end;
  bool last;
  lane_bounds(P, m, li, seg, start, end, last);
  Bits br;
  bits_for(P, m, seg, br);
  int b = 0;
  const unsigned long long e = lane_run<false>(br, t, g, exit_pos(entry), exit_slot(entry), exit_k(entry), end, b, 0x7fffffff, count,
                                               nullptr, nullptr);
  return e;
}

// locate step of one lane (after the scan placed b0): the error of the segment's first error lane -- proven by induction,
// every lane behind it in the segment is meaningless -- and the tail of a segment the data ran out in.  Returns the error key
// (2 * block + DC decoded) or INT_MAX.
HD inline int lane_locate(const JdPtrs& P, const Tabs& t, const Geo& g, const fp_jpeg_scan& s, const JdImg& m, int li, int seg,
                          unsigned long long ex, int count, int b0, int seg_err) {
  if (li > seg_err) return 0x7fffffff;
  const int qe = quota_end(s, m, seg);
  if (li == seg_err) {
    const int dcok = (ex & kDcOk) ? 1 : 0;
    const int x = b0 + count - dcok;
    return x < qe ? 2 * x + dcok : 0x7fffffff;
  }
  unsigned start, end;
  bool last;
  lane_bounds(P, m, li, seg, start, end, last);
  if (!last) return 0x7fffffff;
  int b = exit_k(ex) ? b0 + count - 1 : b0 + count;
  if (b >= qe) return 0x7fffffff;
  Bits br;                                     // the data ended before the segment's last block: zero bits decode on
  bits_for(P, m, seg, br);
  int cnt;
  const unsigned long long e = lane_run<false>(br, t, g, exit_pos(ex), exit_slot(ex), exit_k(ex), 0xffffffffu, b, qe, cnt, nullptr,
                                               nullptr);
  if (e & kErr) return 2 * b + ((e & kDcOk) ? 1 : 0);
  return 0x7fffffff;
}

HD inline void lane_write(const JdPtrs& P, const Tabs& t, const Geo& g, const fp_jpeg_scan& s, const JdImg& m, const JdState& st,
                          int li, int seg, int seg_err, unsigned long long entry, int b0, short* coefs, int* dcdiff) {
  if (li > seg_err || (entry & kDead)) return;
  unsigned start, end;
  bool last;
  lane_bounds(P, m, li, seg, start, end, last);
  const int qe = quota_end(s, m, seg);
  const int stop = qe < st.lim ? qe : st.lim;
  int b = exit_k(entry) ? b0 - 1 : b0;
  if (b >= stop) return;
  Bits br;
  bits_for(P, m, seg, br);
  int cnt;
  lane_run<true>(br, t, g, exit_pos(entry), exit_slot(entry), exit_k(entry), last ? 0xffffffffu : end, b, stop, cnt, coefs, dcdiff);
}

// first block of lane li: the segment's first block + the exclusive count scan relative to the segment's first lane
HD inline int lane_b0(const fp_jpeg_scan& s, int seg, int scan_li, int scan_first) {
  const long seg_blocks = s.restart_interval > 0 ? (long)s.restart_interval * s.blocks_per_mcu : 0;
  return (int)(seg * seg_blocks) + scan_li - scan_first;
}

// the first round that changed no exit (1 .. max_rounds), 0 = none
HD inline int proof_round(const int* chg, int max_rounds) {
  for (int r = 1; r <= max_rounds; ++r)
    if (chg[r] == 0) return r;
  return 0;
}

HD inline void finish_status(const JdImg& m, const fp_jpeg_scan& s, JdState& st, int errkey) {
  if (st.nf < m.nseg) {                                  // the RSTn in front of segment nf is missing or wrong
    const long e = 2l * st.nf * s.restart_interval * s.blocks_per_mcu;
    if (e < errkey) errkey = (int)e;
  }
  st.errkey = errkey;
  if (errkey != 0x7fffffff) {
    st.status = FP_ERR_INVALID_ARG;
    st.lim = (errkey >> 1) + 1;
    st.ndc = (errkey >> 1) + (errkey & 1);
  } else {
    st.status = st.term == kTermEnd ? FP_OK : FP_JPEG_DECODE_ON_HOST;
    st.lim = st.ndc = m.nblocks;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// kernels

__device__ inline void load_tables(const fp_jpeg_scan& s, fp_jpeg_huff* lds, int tid, int nthreads) {
  const int ntab = s.ncomp;
  const int words = (int)(sizeof(fp_jpeg_huff) / 4);
  const unsigned* dc = (const unsigned*)s.dc;
  const unsigned* ac = (const unsigned*)s.ac;
  unsigned* d = (unsigned*)lds;
  for (int i = tid; i < ntab * words; i += nthreads) {
    d[i] = dc[i];
    d[3 * words + i] = ac[i];
  }
}

__global__ __launch_bounds__(256) void jd_zero(JdPtrs P) {
  const int i = blockIdx.y;
  const JdImg& m = P.img[i];
  short* c = P.coefs + m.coef_off;
  const long n = P.desc[i].n_coefs;
  long head = (long)((16 - ((uintptr_t)c & 15)) & 15) / 2;
  if (((uintptr_t)c & 1) || head > n) head = n;
  const long stride = (long)gridDim.x * blockDim.x;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long j = t; j < head; j += stride) c[j] = 0;
  const long nv = (n - head) / 8;
  uint4* v = (uint4*)(c + head);
  for (long j = t; j < nv; j += stride) v[j] = make_uint4(0, 0, 0, 0);
  for (long j = head + nv * 8 + t; j < n; j += stride) c[j] = 0;
}

// block-wide exclusive scan of one int per thread (kImgThreads); returns the total
__device__ inline int block_scan(int v, int* lds, int& excl) {
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int o = 1; o < kImgThreads; o <<= 1) {
    const int a = tid >= o ? lds[tid - o] : 0;
    __syncthreads();
    lds[tid] += a;
    __syncthreads();
  }
  excl = lds[tid] - v;
  const int total = lds[kImgThreads - 1];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(kImgThreads) void jd_unstuff(JdPtrs P) {
  __shared__ int scan_lds[kImgThreads];
  __shared__ int s_marker, s_done;
  __shared__ long s_pos;
  const int i = blockIdx.x, tid = threadIdx.x;
  const fp_jpeg_scan& s = P.desc[i];
  const JdImg& m = P.img[i];
  JdState& st = P.state[i];
  const unsigned char* d = P.files + m.file_off + s.data_off;     // the scan data: d[0 .. len)
  const long len = s.data_len;
  unsigned char* u = P.u + m.u_off;
  int* ss = P.seg_start + m.seg_base;
  int* fl = P.first_lane + m.seg_base;
  // ---- unstuff + segments (thread 0 keeps the serial state) ----
  long pos = 0;
  int out = 0, nf = 1, term = kTermEnd;
  if (tid == 0) ss[0] = 0;
  for (;;) {
    const long base = pos + (long)tid * kChunk;
    int mk = 0x7fffffff;                      // first marker in my bytes (offset from pos)
    for (int j = 0; j < kChunk; ++j) {
      const long q = base + j;
      if (q >= len) break;
      if (d[q] == 0xff && (q + 1 == len || d[q + 1] != 0)) {
        mk = (int)(q - pos);
        break;
      }
    }
    if (tid == 0) s_marker = 0x7fffffff;
    __syncthreads();
    if (mk != 0x7fffffff) atomicMin(&s_marker, mk);
    __syncthreads();
    const int marker = s_marker;
    const long lim = marker == 0x7fffffff ? (pos + (long)kImgThreads * kChunk < len ? pos + (long)kImgThreads * kChunk : len)
                                          : pos + marker;
    int keep = 0;
    for (int j = 0; j < kChunk; ++j) {
      const long q = base + j;
      if (q >= lim) break;
      keep += !(d[q] == 0 && q > 0 && d[q - 1] == 0xff);
    }
    int excl;
    const int total = block_scan(keep, scan_lds, excl);
    int o = out + excl;
    for (int j = 0; j < kChunk; ++j) {
      const long q = base + j;
      if (q >= lim) break;
      if (!(d[q] == 0 && q > 0 && d[q - 1] == 0xff)) u[o++] = d[q];
    }
    out += total;
    if (tid == 0) {
      s_done = 0;
      if (marker == 0x7fffffff) {
        s_pos = lim;
        if (lim >= len) s_done = 1;
      } else {
        const long q = pos + marker;
        const int code = q + 1 < len ? d[q + 1] : -1;
        if (code == 0xff) {
          term = kTermHost;
          s_done = 1;
        } else if (nf < m.nseg && code == 0xd0 + ((nf - 1) & 7)) {
          ss[nf++] = out;
          s_pos = q + 2;
        } else {
          term = (code == 0xd9 || code < 0) ? kTermEnd : kTermMarker;
          s_done = 1;
        }
      }
    }
    __syncthreads();
    if (s_done) break;
    pos = s_pos;
    __syncthreads();
  }
  // ---- lanes: max(1, ceil(bits / S)) per found segment ----
  __shared__ int s_nf, s_term;
  if (tid == 0) {
    ss[nf] = out;
    s_nf = nf;
    s_term = term;
  }
  __syncthreads();
  nf = s_nf;
  int carry = 0;
  for (int c0 = 0; c0 < nf; c0 += kImgThreads) {
    const int j = c0 + tid;
    int nlj = 0;
    if (j < nf) {
      const long bits = (long)(ss[j + 1] - ss[j]) * 8;
      nlj = bits > 0 ? (int)((bits + P.sub_bits - 1) / P.sub_bits) : 1;
    }
    int excl;
    const int total = block_scan(nlj, scan_lds, excl);
    if (j < nf) fl[j] = carry + excl;
    carry += total;
  }
  const int nl = carry;
  if (tid == 0) {
    fl[nf] = nl;
    st.nf = nf;
    st.nl = nl > m.lane_cap ? 0 : nl;
    st.term = nl > m.lane_cap ? kTermHost : s_term;
    st.status = FP_JPEG_DECODE_ON_HOST;
  }
  if (nl > m.lane_cap) return;
  __syncthreads();
  int* lseg = P.lane_seg + m.lane_base;
  for (int li = tid; li < nl; li += kImgThreads) {
    int lo = 0, hi = nf - 1;                   // the last segment whose first lane <= li
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (fl[mid] <= li) lo = mid;
      else hi = mid - 1;
    }
    lseg[li] = lo;
  }
}

struct LaneCtx {
  int img, li;
  bool active;
};

__device__ inline LaneCtx lane_ctx(const JdPtrs& P) {
  LaneCtx c;
  c.img = P.wg_img[blockIdx.x];
  const JdImg& m = P.img[c.img];
  c.li = (int)((long)blockIdx.x * kLanesPerWg + threadIdx.x - m.lane_base);
  const JdState& st = P.state[c.img];
  c.active = st.term != kTermHost && c.li < st.nl;
  return c;
}

__global__ __launch_bounds__(kLanesPerWg) void jd_spec(JdPtrs P) {
  __shared__ fp_jpeg_huff tabs[6];
  const LaneCtx c = lane_ctx(P);
  const fp_jpeg_scan& s = P.desc[c.img];
  __shared__ Geo g;
  if (P.state[c.img].term == kTermHost) return;          // uniform over the workgroup
  load_tables(s, tabs, threadIdx.x, kLanesPerWg);
  if (threadIdx.x == 0) g.init(s);
  __syncthreads();
  if (!c.active) return;
  const JdImg& m = P.img[c.img];
  const Tabs t = {tabs, tabs + 3};
  const int seg = P.lane_seg[m.lane_base + c.li];
  unsigned start, end;
  bool last;
  lane_bounds(P, m, c.li, seg, start, end, last);
  int count;
  const unsigned long long e = lane_sync(P, t, g, m, c.li, seg, pack_exit(start, 0, 0), count);
  P.exits[m.lane_base + c.li] = e;
  P.counts[m.lane_base + c.li] = count;
}

__global__ __launch_bounds__(kLanesPerWg) void jd_round(JdPtrs P, int r) {
  __shared__ fp_jpeg_huff tabs[6];
  __shared__ unsigned long long cur[kLanesPerWg];
  __shared__ int any;
  const LaneCtx c = lane_ctx(P);
  const JdImg& m = P.img[c.img];
  int* chg = P.changed + m.chg_base;
  if (P.state[c.img].term == kTermHost || (r >= 2 && chg[r - 1] == 0)) return;    // host, or proven in an earlier round
  const fp_jpeg_scan& s = P.desc[c.img];
  __shared__ Geo g;
  load_tables(s, tabs, threadIdx.x, kLanesPerWg);
  if (threadIdx.x == 0) g.init(s);
  const unsigned long long* in = P.exits + ((r - 1) & 1) * P.nlanes + m.lane_base;
  unsigned long long* outx = P.exits + (r & 1) * P.nlanes + m.lane_base;
  int* outc = P.counts + (r & 1) * P.nlanes + m.lane_base;
  const int tid = threadIdx.x;
  const unsigned long long mine = c.active ? in[c.li] : 0;
  cur[tid] = mine;
  __syncthreads();
  const Tabs t = {tabs, tabs + 3};
  int seg = 0;
  unsigned start = 0, end;
  bool last;
  if (c.active) {
    seg = P.lane_seg[m.lane_base + c.li];
    lane_bounds(P, m, c.li, seg, start, end, last);
  }
  unsigned long long e = mine;
  int count = c.active ? P.counts[((r - 1) & 1) * P.nlanes + m.lane_base + c.li] : 0;
  bool unstable = false;
  for (int it = 0; it < kLocalIters; ++it) {
    if (c.active) {
      const unsigned long long* pred = tid > 0 ? &cur[tid - 1] : in + c.li - 1;
      const unsigned long long entry = lane_entry(P, m, c.li, seg, start, pred);
      if (!(entry & kDead)) e = lane_sync(P, t, g, m, c.li, seg, entry, count);   // behind an error: keep what we have
    }
    if (tid == 0) any = 0;
    __syncthreads();
    if (c.active && e != cur[tid]) any = 1;
    __syncthreads();
    const int changed = any;
    if (c.active) cur[tid] = e;
    __syncthreads();
    unstable = changed != 0;
    if (!changed) break;
  }
  if (c.active) {
    outx[c.li] = e;
    outc[c.li] = count;
    if (e != mine || unstable) atomicOr(&chg[r], 1);
  }
}

__global__ __launch_bounds__(kImgThreads) void jd_locate(JdPtrs P) {
  __shared__ fp_jpeg_huff tabs[6];
  __shared__ int scan_lds[kImgThreads];
  __shared__ int s_err;
  const int i = blockIdx.x, tid = threadIdx.x;
  const fp_jpeg_scan& s = P.desc[i];
  const JdImg& m = P.img[i];
  JdState& st = P.state[i];
  if (st.term == kTermHost) {
    if (tid == 0) P.status[i] = FP_JPEG_DECODE_ON_HOST;
    return;
  }
  const int pr = proof_round(P.changed + m.chg_base, P.max_rounds);
  if (pr == 0) {                                         // not proven within max_rounds
    if (tid == 0) {
      st.status = FP_JPEG_DECODE_ON_HOST;
      P.status[i] = FP_JPEG_DECODE_ON_HOST;
    }
    return;
  }
  __shared__ Geo g;
  load_tables(s, tabs, tid, kImgThreads);
  if (tid == 0) {
    s_err = 0x7fffffff;
    g.init(s);
  }
  const unsigned long long* ex = P.exits + (pr & 1) * P.nlanes + m.lane_base;
  const int* cnt = P.counts + (pr & 1) * P.nlanes + m.lane_base;
  const int* lseg = P.lane_seg + m.lane_base;
  const int* fl = P.first_lane + m.seg_base;
  int* b0 = P.b0 + m.lane_base;
  int* serr = P.seg_err + m.seg_base;
  for (int j = tid; j < st.nf; j += kImgThreads) serr[j] = 0x7fffffff;
  __syncthreads();
  for (int li = tid; li < st.nl; li += kImgThreads)
    if (ex[li] & kErr) atomicMin(&serr[lseg[li]], li);
  __syncthreads();
  // exclusive scan of the counts over the image's lanes -> b0; lane_b0 makes it segment-relative
  int carry = 0;
  for (int c0 = 0; c0 < st.nl; c0 += kImgThreads) {
    const int li = c0 + tid;
    const int v = li < st.nl ? cnt[li] : 0;
    int excl;
    const int total = block_scan(v, scan_lds, excl);
    if (li < st.nl) b0[li] = carry + excl;
    carry += total;
  }
  __syncthreads();
  const Tabs t = {tabs, tabs + 3};
  int myerr = 0x7fffffff;
  for (int li = tid; li < st.nl; li += kImgThreads) {
    const int seg = lseg[li];
    const int e = lane_locate(P, t, g, s, m, li, seg, ex[li], cnt[li], lane_b0(s, seg, b0[li], b0[fl[seg]]), serr[seg]);
    myerr = e < myerr ? e : myerr;
  }
  if (myerr != 0x7fffffff) atomicMin(&s_err, myerr);
  __syncthreads();
  if (tid == 0) {
    finish_status(m, s, st, s_err);
    P.status[i] = st.status;
  }
}

__global__ __launch_bounds__(kLanesPerWg) void jd_write(JdPtrs P) {
  __shared__ fp_jpeg_huff tabs[6];
  const LaneCtx c = lane_ctx(P);
  const JdState& st = P.state[c.img];
  if (st.term == kTermHost || (st.status != FP_OK && st.status != FP_ERR_INVALID_ARG)) return;     // uniform over the workgroup
  const fp_jpeg_scan& s = P.desc[c.img];
  __shared__ Geo g;
  load_tables(s, tabs, threadIdx.x, kLanesPerWg);
  if (threadIdx.x == 0) g.init(s);
  __syncthreads();
  if (!c.active) return;
  const JdImg& m = P.img[c.img];
  const Tabs t = {tabs, tabs + 3};
  const unsigned long long* fin = P.exits + (proof_round(P.changed + m.chg_base, P.max_rounds) & 1) * P.nlanes + m.lane_base;
  const int* b0 = P.b0 + m.lane_base;
  const int seg = P.lane_seg[m.lane_base + c.li];
  unsigned start, end;
  bool last;
  lane_bounds(P, m, c.li, seg, start, end, last);
  const unsigned long long entry = lane_entry(P, m, c.li, seg, start, fin + c.li - 1);
  const int fl = P.first_lane[m.seg_base + seg];
  lane_write(P, t, g, s, m, st, c.li, seg, P.seg_err[m.seg_base + seg], entry, lane_b0(s, seg, b0[c.li], b0[fl]), P.coefs + m.coef_off,
             P.dcdiff + m.blk_base);
}

struct Dc3 {                    // running DC predictions of the three components (scalars: no indexed private array)
  unsigned a, b, c;
  HD unsigned add(int comp, unsigned v) {
    if (comp == 0) return a += v;
    if (comp == 1) return b += v;
    return c += v;
  }
};

__global__ __launch_bounds__(kImgThreads) void jd_dc(JdPtrs P) {
  __shared__ unsigned sums[3][kImgThreads];
  __shared__ int resets[kImgThreads];
  __shared__ Geo g;
  const int i = blockIdx.x, tid = threadIdx.x;
  const JdState& st = P.state[i];
  if (st.term == kTermHost || (st.status != FP_OK && st.status != FP_ERR_INVALID_ARG)) return;
  const fp_jpeg_scan& s = P.desc[i];
  const JdImg& m = P.img[i];
  if (tid == 0) g.init(s);
  const int* diff = P.dcdiff + m.blk_base;
  short* coefs = P.coefs + m.coef_off;
  const int seg_blocks = s.restart_interval > 0 ? s.restart_interval * s.blocks_per_mcu : 0;
  const int per = (st.ndc + kImgThreads - 1) / kImgThreads;
  const int b_lo = tid * per, b_hi = b_lo + per < st.ndc ? b_lo + per : st.ndc;
  Dc3 acc = {0, 0, 0};
  int reset = 0;
  for (int b = b_lo; b < b_hi; ++b) {
    if (seg_blocks && b % seg_blocks == 0) acc = {0, 0, 0}, reset = 1;
    acc.add(s.slot_comp[b % s.blocks_per_mcu], (unsigned)diff[b]);
  }
  sums[0][tid] = acc.a;
  sums[1][tid] = acc.b;
  sums[2][tid] = acc.c;
  resets[tid] = reset;
  __syncthreads();
  if (tid < 3) {                               // carry into every thread's range, one component per thread
    unsigned carry = 0;
    for (int t = 0; t < kImgThreads; ++t) {
      const unsigned v = sums[tid][t];
      sums[tid][t] = carry;
      carry = resets[t] ? v : carry + v;
    }
  }
  __syncthreads();
  Dc3 pred = {sums[0][tid], sums[1][tid], sums[2][tid]};
  for (int b = b_lo; b < b_hi; ++b) {
    if (seg_blocks && b % seg_blocks == 0) pred = {0, 0, 0};
    coefs[g.block_addr(b)] = (short)pred.add(s.slot_comp[b % s.blocks_per_mcu], (unsigned)diff[b]);
  }
}

bool valid_params(int sub_bits, int max_rounds) {
  return sub_bits >= 32 && sub_bits <= (1 << 20) && sub_bits % 8 == 0 && max_rounds >= 1 && max_rounds <= 64;
}

}  // namespace

extern "C" {

size_t fp_jpeg_entropy_workspace_bytes(const fp_jpeg_scan* scans, int n, int sub_bits, int max_rounds) {
  if (!scans || n < 1 || !valid_params(sub_bits, max_rounds)) return 0;
  JdLayout L;
  return plan_layout(scans, n, sub_bits, max_rounds, L) ? L.total : 0;
}

int fp_jpeg_entropy_decode_device(const uint8_t* files, const fp_jpeg_scan* scans, const int64_t* file_off, int n, int16_t* coefs,
                                  const int64_t* coef_off, int32_t* status, void* workspace, size_t ws_bytes, int sub_bits,
                                  int max_rounds, void* stream) {
  if (n == 0) return FP_OK;
  if (!files || !scans || !file_off || !coefs || !coef_off || !status || !workspace || n < 0 || n > 65535 ||
      !valid_params(sub_bits, max_rounds))
    return FP_ERR_INVALID_ARG;
  if (((uintptr_t)workspace) % 16 || ((uintptr_t)coefs) % 2) return FP_ERR_ALIGNMENT;
  JdLayout L;
  if (!plan_layout(scans, n, sub_bits, max_rounds, L)) return FP_ERR_INVALID_ARG;
  if (ws_bytes < L.total) return FP_ERR_BOUNDS;
  for (int i = 0; i < n; ++i) {
    if (file_off[i] < 0 || coef_off[i] < 0) return FP_ERR_INVALID_ARG;
    L.imgs[i].file_off = file_off[i];
    L.imgs[i].coef_off = coef_off[i];
  }
  // descriptors, images, zeroed image states, the workgroup map: one copy
  std::vector<unsigned char> stage(L.off_u, 0);
  memcpy(stage.data() + L.off_desc, scans, sizeof(fp_jpeg_scan) * n);
  memcpy(stage.data() + L.off_img, L.imgs.data(), sizeof(JdImg) * n);
  memcpy(stage.data() + L.off_wg, L.wg_img.data(), sizeof(int) * L.wg_img.size());
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyWithStream(ws, stage.data(), stage.size(), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    fp_set_hip_error(e);
    return FP_ERR_LAUNCH;
  }
  e = hipMemsetAsync(ws + L.off_chg, 0, L.off_dc - L.off_chg, s);
  if (e != hipSuccess) {
    fp_set_hip_error(e);
    return FP_ERR_LAUNCH;
  }
  JdPtrs P;
  P.files = files;
  P.coefs = coefs;
  P.status = status;
  P.desc = (const fp_jpeg_scan*)(ws + L.off_desc);
  P.img = (const JdImg*)(ws + L.off_img);
  P.state = (JdState*)(ws + L.off_state);
  P.wg_img = (const int*)(ws + L.off_wg);
  P.u = ws + L.off_u;
  P.seg_start = (int*)(ws + L.off_seg);
  P.first_lane = (int*)(ws + L.off_first);
  P.seg_err = (int*)(ws + L.off_serr);
  P.changed = (int*)(ws + L.off_chg);
  P.dcdiff = (int*)(ws + L.off_dc);
  P.lane_seg = (int*)(ws + L.off_lseg);
  P.exits = (unsigned long long*)(ws + L.off_exit);
  P.counts = (int*)(ws + L.off_cnt);
  P.b0 = (int*)(ws + L.off_b0);
  P.nlanes = L.nlanes;
  P.sub_bits = sub_bits;
  P.max_rounds = max_rounds;
  const unsigned nwg = (unsigned)L.wg_img.size();
  hipLaunchKernelGGL(jd_zero, dim3(16, (unsigned)n), dim3(256), 0, s, P);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(jd_unstuff, dim3((unsigned)n), dim3(kImgThreads), 0, s, P);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(jd_spec, dim3(nwg), dim3(kLanesPerWg), 0, s, P);
  FP_CHECK_LAUNCH();
  for (int r = 1; r <= max_rounds; ++r) {
    hipLaunchKernelGGL(jd_round, dim3(nwg), dim3(kLanesPerWg), 0, s, P, r);
    FP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(jd_locate, dim3((unsigned)n), dim3(kImgThreads), 0, s, P);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(jd_write, dim3(nwg), dim3(kLanesPerWg), 0, s, P);
  FP_CHECK_LAUNCH();
  hipLaunchKernelGGL(jd_dc, dim3((unsigned)n), dim3(kImgThreads), 0, s, P);
  FP_CHECK_LAUNCH();
  return FP_OK;
}

// The same phases, serially, on one file in host memory.
int fp_jpeg_entropy_decode_emulate(const uint8_t* data, size_t n, const fp_jpeg_scan* scan, int16_t* coefs, int sub_bits,
                                   int max_rounds, int32_t* rounds) {
  if (!data || !scan || !coefs || !valid_params(sub_bits, max_rounds)) return FP_ERR_INVALID_ARG;
  if (scan->data_off < 0 || scan->data_len < 0 || (uint64_t)(scan->data_off + scan->data_len) > (uint64_t)n) return FP_ERR_INVALID_ARG;
  JdLayout L;
  if (!plan_layout(scan, 1, sub_bits, max_rounds, L)) return FP_ERR_INVALID_ARG;
  JdImg m = L.imgs[0];
  m.file_off = 0;
  m.coef_off = 0;
  m.u_off = m.seg_base = m.blk_base = m.lane_base = m.chg_base = 0;
  const long nl_cap = m.lane_cap;
  std::vector<unsigned char> u((size_t)scan->data_len + 1);
  std::vector<int> ss(m.seg_cap + 1), fl(m.seg_cap + 1), serr(m.seg_cap + 1, 0x7fffffff), chg(max_rounds + 1, 0), dcdiff(m.nblocks + 1), lseg(nl_cap),
      counts(2 * nl_cap), b0(nl_cap);
  std::vector<unsigned long long> exits(2 * nl_cap);
  JdState st;
  memset(&st, 0, sizeof(st));
  JdPtrs P;
  memset(&P, 0, sizeof(P));
  P.files = data;
  P.coefs = coefs;
  P.desc = scan;
  P.img = &m;
  P.state = &st;
  P.u = u.data();
  P.seg_start = ss.data();
  P.first_lane = fl.data();
  P.seg_err = serr.data();
  P.changed = chg.data();
  P.dcdiff = dcdiff.data();
  P.lane_seg = lseg.data();
  P.exits = exits.data();
  P.counts = counts.data();
  P.b0 = b0.data();
  P.nlanes = nl_cap;
  P.sub_bits = sub_bits;
  P.max_rounds = max_rounds;
  const fp_jpeg_scan& s = *scan;
  memset(coefs, 0, sizeof(int16_t) * (size_t)s.n_coefs);
  if (rounds) *rounds = max_rounds + 1;
  // unstuff
  const unsigned char* d = data + s.data_off;
  const long len = s.data_len;
  int out = 0, nf = 1, term = kTermEnd;
  ss[0] = 0;
  for (long q = 0; q < len;) {
    if (d[q] == 0xff && (q + 1 == len || d[q + 1] != 0)) {
      const int code = q + 1 < len ? d[q + 1] : -1;
      if (code == 0xff) {
        term = kTermHost;
        break;
      }
      if (nf < m.nseg && code == 0xd0 + ((nf - 1) & 7)) {
        ss[nf++] = out;
        q += 2;
        continue;
      }
      term = (code == 0xd9 || code < 0) ? kTermEnd : kTermMarker;
      break;
    }
    if (!(d[q] == 0 && q > 0 && d[q - 1] == 0xff)) u[out++] = d[q];
    ++q;
  }
  ss[nf] = out;
  int nl = 0;
  for (int j = 0; j < nf; ++j) {
    fl[j] = nl;
    const long bits = (long)(ss[j + 1] - ss[j]) * 8;
    nl += bits > 0 ? (int)((bits + sub_bits - 1) / sub_bits) : 1;
  }
  fl[nf] = nl;
  if (term == kTermHost || nl > m.lane_cap) return FP_JPEG_DECODE_ON_HOST;
  st.nf = nf;
  st.nl = nl;
  st.term = term;
  for (int j = 0; j < nf; ++j)
    for (int li = fl[j]; li < fl[j + 1]; ++li) lseg[li] = j;
  Geo g;
  g.init(s);
  const Tabs t = {s.dc, s.ac};
  // speculate
  for (int li = 0; li < nl; ++li) {
    unsigned start, end;
    bool last;
    lane_bounds(P, m, li, lseg[li], start, end, last);
    exits[li] = lane_sync(P, t, g, m, li, lseg[li], pack_exit(start, 0, 0), counts[li]);
  }
  // synchronise: rounds of workgroups of kLanesPerWg lanes, each iterating as jd_round does in LDS
  for (int r = 1; r <= max_rounds; ++r) {
    if (r >= 2 && chg[r - 1] == 0) continue;
    const unsigned long long* in = exits.data() + ((r - 1) & 1) * nl_cap;
    unsigned long long* outx = exits.data() + (r & 1) * nl_cap;
    int* outc = counts.data() + (r & 1) * nl_cap;
    for (int w = 0; w < nl; w += kLanesPerWg) {
      const int nw = nl - w < kLanesPerWg ? nl - w : kLanesPerWg;
      unsigned long long cur[kLanesPerWg], nxt[kLanesPerWg];
      int cnt[kLanesPerWg];
      for (int j = 0; j < nw; ++j) cur[j] = in[w + j], cnt[j] = counts[((r - 1) & 1) * nl_cap + w + j];
      bool unstable = false;
      for (int it = 0; it < kLocalIters; ++it) {
        bool changed = false;
        for (int j = 0; j < nw; ++j) {
          const int li = w + j;
          unsigned start, end;
          bool last;
          lane_bounds(P, m, li, lseg[li], start, end, last);
          const unsigned long long entry = lane_entry(P, m, li, lseg[li], start, j > 0 ? &cur[j - 1] : in + li - 1);
          nxt[j] = (entry & kDead) ? cur[j] : lane_sync(P, t, g, m, li, lseg[li], entry, cnt[j]);
          changed |= nxt[j] != cur[j];
        }
        for (int j = 0; j < nw; ++j) cur[j] = nxt[j];
        unstable = changed;
        if (!changed) break;
      }
      for (int j = 0; j < nw; ++j) {
        outx[w + j] = cur[j];
        outc[w + j] = cnt[j];
        if (cur[j] != in[w + j] || unstable) chg[r] = 1;
      }
    }
  }
  const int pr = proof_round(chg.data(), max_rounds);
  if (pr == 0) return FP_JPEG_DECODE_ON_HOST;
  if (rounds) *rounds = pr;
  // locate
  const unsigned long long* fin = exits.data() + (pr & 1) * nl_cap;
  const int* cnt = counts.data() + (pr & 1) * nl_cap;
  int acc = 0;
  for (int li = 0; li < nl; ++li) {
    b0[li] = acc;
    acc += cnt[li];
    if ((fin[li] & kErr) && serr[lseg[li]] > li) serr[lseg[li]] = li;
  }
  int err = 0x7fffffff;
  for (int li = 0; li < nl; ++li) {
    const int seg = lseg[li];
    const int e = lane_locate(P, t, g, s, m, li, seg, fin[li], cnt[li], lane_b0(s, seg, b0[li], b0[fl[seg]]), serr[seg]);
    err = e < err ? e : err;
  }
  finish_status(m, s, st, err);
  if (st.status == FP_JPEG_DECODE_ON_HOST) return st.status;
  // write
  for (int li = 0; li < nl; ++li) {
    const int seg = lseg[li];
    unsigned start, end;
    bool last;
    lane_bounds(P, m, li, seg, start, end, last);
    const unsigned long long entry = lane_entry(P, m, li, seg, start, fin + li - 1);
    lane_write(P, t, g, s, m, st, li, seg, serr[seg], entry, lane_b0(s, seg, b0[li], b0[fl[seg]]), coefs, dcdiff.data());
  }
  // dc
  const int seg_blocks = s.restart_interval > 0 ? s.restart_interval * s.blocks_per_mcu : 0;
  Dc3 pred = {0, 0, 0};
  for (int b = 0; b < st.ndc; ++b) {
    if (seg_blocks && b % seg_blocks == 0) pred = {0, 0, 0};
    coefs[g.block_addr(b)] = (int16_t)pred.add(s.slot_comp[b % s.blocks_per_mcu], (unsigned)dcdiff[b]);
  }
  return st.status;
}

}  // extern "C"
