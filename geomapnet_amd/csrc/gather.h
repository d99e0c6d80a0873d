// Batches gathered by index from a device-resident frame store (mn_set_input_index, mn_op_gather_frames): out[b] = store[index[b]]
// for `images` frames of `frame_bytes` bytes each -- the batch assembly the reference does on the host (DataLoader +
// default_collate, common/train.py:180-188; MF.__getitem__'s torch.stack, dataset_loaders/composite.py:77-83), as one copy kernel
// over frames that already sit in HBM.  Frames are opaque byte rows: uint8 NHWC and fp32 NCHW frames go through the same code.
//
// One workgroup column (blockIdx.y) per output frame, so index[b] is uniform over the workgroup and read once; the frame's byte
// offset in the store is 64-bit (a store may exceed 4 GiB).  A frame is copied in pieces of W bytes, W the largest of 16, 8, 4, 1
// at which source and destination share their alignment (both 16-byte aligned frames -- every allocation with frame_bytes a multiple
// of 16 -- take 16): the bytes ahead of the destination's first W-aligned address and behind its last whole piece go as single bytes,
// everything between as aligned W-byte loads and stores, four pieces in flight per thread.  No LDS, no atomics.
//
// An index outside [0, store_frames) never becomes an address: the frame reads store frame 0 and *bad = 1 (checked_frame, shared
// with the indexed resize_u8_kernel).
#pragma once
#include "common.h"

namespace mn {

// the store frame output image `b` reads: index[b], or 0 with *bad = 1 when that lies outside the store
__device__ __forceinline__ long checked_frame(const int32_t* __restrict__ index, int b, long store_frames, float* bad, bool reporter) {
  const long v = (long)index[b];
  if (v >= 0 && v < store_frames) return v;
  if (reporter && bad) *bad = 1.f;
  return 0;
}

constexpr int kGatherUnroll = 4;                         // pieces in flight per thread
constexpr long kGatherBlockBytes = 256 * 16 * kGatherUnroll;  // bytes one workgroup moves per round at the 16-byte width

template <typename V>
__device__ __forceinline__ void gather_copy(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, long n) {
  constexpr int W = (int)sizeof(V);
  const int tid = threadIdx.x;
  long head = (long)((W - (int)((uintptr_t)dst & (W - 1))) & (W - 1));  // bytes ahead of dst's first W-aligned address
  if (head > n) head = n;
  const long pieces = (n - head) / W;
  const long tail0 = head + pieces * W;  // first byte behind the last whole piece
  const V* __restrict__ s = reinterpret_cast<const V*>(src + head);
  V* __restrict__ d = reinterpret_cast<V*>(dst + head);
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + tid;
  for (; i + (kGatherUnroll - 1) * stride < pieces; i += kGatherUnroll * stride) {
    V v[kGatherUnroll];
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) v[u] = s[i + u * stride];
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) d[i + u * stride] = v[u];
  }
  for (; i < pieces; i += stride) d[i] = s[i];
  if (blockIdx.x == 0) {  // the ragged ends: fewer than 2 W bytes
    if (tid < head) dst[tid] = src[tid];
    const long t = tail0 + tid;
    if (t < n) dst[t] = src[t];
  }
}

static __global__ void __launch_bounds__(256) gather_frames_kernel(const unsigned char* __restrict__ store,
                                                                   const int32_t* __restrict__ index,
                                                                   unsigned char* __restrict__ out, long frame_bytes,
                                                                   long store_frames, float* bad) {
  const int b = blockIdx.y;
  const long f = checked_frame(index, b, store_frames, bad, blockIdx.x == 0 && threadIdx.x == 0);
  const unsigned char* __restrict__ src = store + f * frame_bytes;
  unsigned char* __restrict__ dst = out + (long)b * frame_bytes;
  const unsigned mis = (unsigned)(((uintptr_t)src ^ (uintptr_t)dst) & 15);  // where the two alignments differ
  if (mis == 0)
    gather_copy<piece_t>(src, dst, frame_bytes);
  else if ((mis & 7) == 0)
    gather_copy<unsigned long long>(src, dst, frame_bytes);
  else if ((mis & 3) == 0)
    gather_copy<unsigned>(src, dst, frame_bytes);
  else
    gather_copy<unsigned char>(src, dst, frame_bytes);
}

// empty on success; `images` is the grid's y extent
inline const char* gather_frames_error(long frame_bytes, long images, long store_frames) {
  if (frame_bytes < 1 || images < 1 || store_frames < 1) return "frame_bytes, images and store_frames must be positive";
  if (images > 65535) return "at most 65535 frames per call (the grid's y extent)";
  return "";
}

inline void launch_gather_frames(const void* store, const int32_t* index, void* out, long frame_bytes, int images, long store_frames,
                                 float* bad, hipStream_t s) {
  long gx = (frame_bytes + kGatherBlockBytes - 1) / kGatherBlockBytes;
  gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
  hipLaunchKernelGGL(gather_frames_kernel, dim3((unsigned)gx, (unsigned)images), dim3(256), 0, s, (const unsigned char*)store, index,
                     (unsigned char*)out, frame_bytes, store_frames, bad);
}

}  // namespace mn
