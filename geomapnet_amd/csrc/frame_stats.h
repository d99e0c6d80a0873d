// Pixel statistics of uint8 frames on the device (mn_op_frame_stats_u8): the per-channel sum and sum of squares of the bytes of
// `images` NHWC frames [images][H][W][3] -- what the reference's scripts/dataset_mean.py accumulates in numpy on the host to write
// the stats.txt its Normalize reads.  On bytes the sums are integers: six unsigned 64-bit totals, exact and independent of the
// order they are taken in.  With an index the input is a frame store and image b is frame index[b] of it (gather.h's convention:
// an index outside the store reads frame 0 and sets *bad).
//
// Addressing.  A frame is one run of L = H*W*3 bytes that starts on channel 0, at any byte address.  It is read as the aligned
// 16-byte pieces that lie wholly inside it; the `head` (0..15) bytes ahead of the first piece and the bytes behind the last one
// are read one by one.  Nothing outside the frame is touched.  Byte e of piece v (counted from the first piece) sits at frame
// offset head + 16 v + e, so its channel is (head + v + e) mod 3, 16 being 1 mod 3.
//
// Work.  A UNIT is kStatsUnitPieces = 768 consecutive pieces of one frame (12 KiB): thread t of the 256 loads pieces
// t, t + 256, t + 512 of the unit -- three fully coalesced 16-byte loads, a piece beyond the frame's last counting as zeros.  768 and
// 256 are 0 and 1 mod 3: over the whole frame the thread's k-th piece has channel phase (head + t + k) mod 3, so the thread
// keeps its sums in a frame of reference ROTATED by p0 = (head + t) mod 3 -- byte j of dword d of piece k belongs to rotated
// channel (k + d + j) mod 3, a compile-time constant -- and turns them back by p0 when it widens them.  Per dword and rotated channel
// the sum is a dot product of the dword's bytes with a 0/1 byte mask and the sum of squares one with the dword itself, masked
// (stats_dot4: plain integer C++, which hipcc lowers to v_perm_b32, v_bfe_u32 and v_dot4_u32_u8).
//
// The grid is one-dimensional: workgroup w of `blocks` takes the units [w U / blocks, (w + 1) U / blocks) of the U = images * G
// units (G units per frame), frame after frame, the next unit's pieces loading while the current one is summed.
//
// Overflow.  A unit gives a thread exactly 16 bytes of each rotated channel (48 bytes, every third one): at most 16 * 255^2 per
// 32-bit accumulator.  The accumulators are widened into the thread's six 64-bit sums after at most kStatsWidenUnits units, i.e.
// after at most kStatsWidenUnits * 16 = 65 536 bytes; a 32-bit accumulator holds 66 051 saturated squares.  Heads and tails go
// into the 64-bit sums directly; everything past a thread's accumulators (wave shuffles, LDS, the work buffer, the fold) is 64-bit.
//
// Two launches, no atomics (launch_saliency's shape): every workgroup writes its six partials to work[w][6]; one workgroup then
// folds them in a fixed order into sums[6], adding to what is there when `accumulate` is set, so a store is processed chunk by
// chunk without a host round trip.  No scratch memory; LDS: 4 waves x 6 sums.
#pragma once
#include "common.h"
#include "gather.h"

namespace mn {

typedef unsigned long long u64;

constexpr int kStatsUnitPieces = 768;   // pieces of a unit: three per thread
constexpr int kStatsWidenUnits = 4096;  // units a thread's 32-bit accumulators take before they are widened
constexpr long kStatsAccBytes = (long)kStatsWidenUnits * (kStatsUnitPieces / 256) * 16 / 3;  // bytes one accumulator can see
static_assert(kStatsUnitPieces == 3 * 256 && kStatsUnitPieces % 3 == 0 && 256 % 3 == 1 && 16 % 3 == 1,
              "the rotated-channel bookkeeping needs 3 pieces per thread at a stride that is 1 mod 3");
static_assert(kStatsAccBytes == 65536 && kStatsAccBytes <= 66051 && 66051ull * 255 * 255 <= 0xffffffffull,
              "a 32-bit accumulator overflows before it is widened");

// sum of the four byte products of a and b, added to c.  Plain integer C++, one form for the device and the emulator: hipcc
// regroups the bytes of a channel with v_perm_b32 and takes the squares with v_dot4_u32_u8 on its own (12 per unit where the
// explicit __builtin_amdgcn_udot4 against these masks took 72); measured, the explicit form was as fast at 256x341 frames and 3 %
// slower at 480x640, so it is not kept.
__device__ __forceinline__ unsigned stats_dot4(unsigned a, unsigned b, unsigned c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c += ((a >> (8 * j)) & 255u) * ((b >> (8 * j)) & 255u);
  return c;
}

// 0x01 in every byte j of a dword with (r + j) mod 3 == c: the bytes of rotated channel c in a dword whose first byte has phase r
constexpr unsigned stats_mask(int r, int c) {
  unsigned m = 0;
  for (int j = 0; j < 4; ++j)
    if ((r + j) % 3 == c) m |= 1u << (8 * j);
  return m;
}

// piece k (0..2) of a thread's unit into its rotated 32-bit accumulators s[3] (sums) and q[3] (sums of squares)
template <int K>
__device__ __forceinline__ void stats_piece(const piece_t& p, unsigned (&s)[3], unsigned (&q)[3]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const unsigned x = p[d];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned m = stats_mask((K + d) % 3, c);
      s[c] = stats_dot4(x, m, s[c]);
      q[c] = stats_dot4(x, x & (m * 255u), q[c]);
    }
  }
}

struct StatsUnit {
  piece_t p[3];
};

// the three pieces thread `tid` owns of unit g of a frame with `pieces` whole pieces starting at `first`
__device__ __forceinline__ StatsUnit stats_load(const piece_t* __restrict__ first, long pieces, long g, int tid) {
  StatsUnit u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long v = g * kStatsUnitPieces + tid + 256 * k;
    u.p[k] = v < pieces ? first[v] : zero_piece();
  }
  return u;
}

// units of one frame of L bytes: its whole pieces in groups of kStatsUnitPieces, at least one (the head and the tail ride on unit 0).
// At most 15 bytes go to the head, so ceil((L / 16) / 768) bounds the count from any alignment; the last unit may be empty.
__host__ __device__ inline long stats_units_per_frame(long L) {
  const long g = (L / 16 + kStatsUnitPieces - 1) / kStatsUnitPieces;
  return g < 1 ? 1 : g;
}

static __global__ void __launch_bounds__(256) frame_stats_partials_kernel(const unsigned char* __restrict__ frames,
                                                                           const int32_t* __restrict__ index, long store_frames,
                                                                           long images, long L, u64* __restrict__ work, float* bad) {
  __shared__ u64 red[4][6];
  const int tid = threadIdx.x;
  const long G = stats_units_per_frame(L), U = images * G;
  const long nb = gridDim.x, w = blockIdx.x;
  const long u1 = (w + 1) * U / nb;
  long u = w * U / nb;
  u64 acc[6] = {0, 0, 0, 0, 0, 0};  // true channels: sums 0..2, sums of squares 3..5

  while (u < u1) {
    const long b = u / G, g0 = u - b * G;
    const long g1 = (G - g0 < u1 - u) ? G : g0 + (u1 - u);  // this workgroup's units [g0, g1) of frame b
    const long f = index ? checked_frame(index, (int)b, store_frames, bad, g0 == 0 && tid == 0) : b;
    const unsigned char* __restrict__ fr = frames + f * L;
    long head = (long)((16 - (int)((uintptr_t)fr & 15)) & 15);
    if (head > L) head = L;
    const long pieces = (L - head) / 16;
    const piece_t* __restrict__ first = reinterpret_cast<const piece_t*>(fr + head);
    const int p0 = (int)((head + tid) % 3);

    long g = g0;
    StatsUnit cur = stats_load(first, pieces, g, tid);
    while (g < g1) {
      const long ge = (g1 - g > kStatsWidenUnits) ? g + kStatsWidenUnits : g1;  // widen after at most kStatsWidenUnits units
      unsigned s[3] = {0, 0, 0}, q[3] = {0, 0, 0};
      for (; g < ge; ++g) {
        StatsUnit nxt;
        if (g + 1 < g1) nxt = stats_load(first, pieces, g + 1, tid);
        stats_piece<0>(cur.p[0], s, q);
        stats_piece<1>(cur.p[1], s, q);
        stats_piece<2>(cur.p[2], s, q);
        if (g + 1 < g1) cur = nxt;
      }
      // rotated channel c' is true channel (c' + p0) mod 3
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int r = (c + 3 - p0) % 3;  // the rotated channel that is true channel c
        acc[c] += r == 0 ? s[0] : (r == 1 ? s[1] : s[2]);
        acc[3 + c] += r == 0 ? q[0] : (r == 1 ? q[1] : q[2]);
      }
    }
    if (g0 == 0) {  // the ragged ends, fewer than 16 bytes each: one byte per thread
      const long tail0 = head + pieces * 16;
      long o = -1;
      if (tid < head) o = tid;
      else if (tid >= 16 && tail0 + (tid - 16) < L) o = tail0 + (tid - 16);
      if (o >= 0) {
        const u64 x = fr[o];
        const int c = (int)(o % 3);
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          acc[cc] += c == cc ? x : 0;
          acc[3 + cc] += c == cc ? x * x : 0;
        }
      }
    }
    u += g1 - g0;
  }

#pragma unroll
  for (int i = 0; i < 6; ++i) {
    u64 v = acc[i];
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((tid & 63) == 0) red[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < 6) work[w * 6 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// sums[i] = (accumulate ? sums[i] : 0) + sum over the `blocks` partials work[.][i]
static __global__ void __launch_bounds__(256) frame_stats_fold_kernel(const u64* __restrict__ work, long blocks, u64* __restrict__ sums,
                                                                       int accumulate) {
  __shared__ u64 red[4][6];
  const int tid = threadIdx.x;
  u64 acc[6] = {0, 0, 0, 0, 0, 0};
  for (long i = tid; i < blocks; i += 256)
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] += work[i * 6 + c];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    u64 v = acc[c];
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((tid & 63) == 0) red[tid >> 6][c] = v;
  }
  __syncthreads();
  if (tid < 6) sums[tid] = (accumulate ? sums[tid] : 0) + red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

constexpr long kStatsMaxBlocks = 1 << 16;

// workgroups of one call: `blocks` as asked (0: eight per compute unit, the streaming kernels' grid), never more than there are units
inline long frame_stats_blocks(long images, long L, long blocks, int compute_units) {
  const long U = images * stats_units_per_frame(L);
  long n = blocks > 0 ? blocks : 8L * (compute_units > 0 ? compute_units : 256);
  if (n > kStatsMaxBlocks) n = kStatsMaxBlocks;
  return n > U ? U : n;
}

// work: [blocks][6] u64, 8-byte aligned; sums: device u64[6].  index null: frames = the batch; else a store of store_frames frames.
inline void launch_frame_stats(const unsigned char* frames, const int32_t* index, long store_frames, long images, long L, u64* sums,
                               int accumulate, long blocks, u64* work, float* bad, hipStream_t s) {
  hipLaunchKernelGGL(frame_stats_partials_kernel, dim3((unsigned)blocks), dim3(256), 0, s, frames, index, store_frames, images, L,
                     work, bad);
  hipLaunchKernelGGL(frame_stats_fold_kernel, dim3(1), dim3(256), 0, s, (const u64*)work, blocks, sums, accumulate);
}

}  // namespace mn
