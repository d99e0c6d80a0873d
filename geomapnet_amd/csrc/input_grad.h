// Input gradient of the poses at inference ("attention maps", the reference's scripts/plot_activations.py:117-133):
// the three kernels the eval-mode backward pass needs beyond the training pass's data-gradient launches.
//   stem_dgrad_kernel<T>    d(conv1 output) NHWC -> d(image) fp32 NCHW, on the matrix pipe
//   bn_eval_bwd_kernel<T>   BatchNorm backward with running statistics: a per-channel scale and the unit's ReLU gate
//   saliency_*_kernel       max_c |gx * x| per pixel, shifted and scaled to [0, 1] per image
// None of them takes a sum across workgroups, reads or writes training state, or uses an atomic.
#pragma once
#include "common.h"
#include "elementwise.h"

namespace mn {

// ---- stem data gradient -------------------------------------------------------------------------------------------------------
// gx[b][c][h][w] = alpha * sum_{r,s,co} gy[b][(h+3-r)/2][(w+3-s)/2][co] * W[co][r][s][c]   (7x7, stride 2, pad 3, 3 <- 64 channels;
// taps whose (h+3-r) or (w+3-s) is odd or whose source pixel lies outside [H0][W0] do not exist).
//
// Mapping: with 3 output channels neither GEMM side of the usual data gradient fills an MFMA tile, so the
// kernel is split into a row GEMM and a column overlap-add.  One wave owns output row h and 56 output columns.  Row h receives the
// 3 (h even) or 4 (h odd) vertical taps r = r0, r0+2, ... of its parity class, each from one gy row p = (h+3-r)/2.  The wave computes
//     V[q][s*3+c] = sum_{r in class} sum_co gy[p(r)][q][co] * W[co][r][s][c]          q = q0 .. q0+31, 21 of 32 columns used
// as ONE 32x32 MFMA tile with K = taps * 64 (fp32: v_mfma_f32_32x32x2_f32, fp16: v_mfma_f32_32x32x16_f16, fp32 accumulate), i.e. the
// horizontal taps and the channels share the MFMA's column side (21 / 32 useful instead of 3 / 32).  The horizontal part is then an
// overlap-add of at most 4 terms per output, gx[h][w][c] = sum_{s in class(w)} V[(w+3-s)/2][s*3+c], GATHERED from the wave's V tile in
// LDS in a fixed order.  Consecutive column tiles advance by 28 gy columns (56 outputs) and start 2 columns early, so every output
// finds its 3-4 terms in its own wave's tile: no cross-wave sums, no atomics, stores of 56 consecutive floats per channel.
//   A operand: straight from global memory -- lane (i = lane & 31, half = lane >> 5) loads the 32 channels [32 half, 32 half + 32) of
//     pixel q0 + i, 128 (fp32) / 64 (fp16) contiguous bytes, and feeds them to consecutive MFMAs (the K order is a permutation both
//     operands share).
//   B operand: all 7 x 64 x 32 weights in LDS for the life of the workgroup, converted from the fp32 OHWI master on the way in:
//     fp32  [r][co][32]: a wave's ds_read_b32 addresses are consecutive per half-wave -- conflict-free;
//     fp16  [r][n][64 + 8 pad] halves: one 16-byte read per lane per MFMA, rows 144 bytes apart.
// Workgroups are persistent over tiles (the weights are staged once); every wave of a workgroup runs the same number of rounds, so
// the two barriers per round are uniform.
constexpr int kSdTile = 56;   // output columns per wave tile
constexpr int kSdVRow = 33;   // floats per V row in LDS (32 + 1 pad)
constexpr int kSdBRowH = 72;  // halves per fp16 weight row in LDS (64 + 8 pad)

template <typename T>
struct StemDgradLds;
template <>
struct StemDgradLds<float> {
  static constexpr int kWeightBytes = 7 * 64 * 32 * 4;
};
template <>
struct StemDgradLds<half> {
  static constexpr int kWeightBytes = 7 * 32 * kSdBRowH * 2;
};

inline int stem_dgrad_tiles(int B, int H, int W) { return B * H * cdiv(W, kSdTile); }

template <typename T>
static __global__ void __launch_bounds__(256) stem_dgrad_kernel(const T* __restrict__ gy, const float* __restrict__ w_ohwi,
                                                                 float* __restrict__ gx, int B, int H, int W, int H0, int W0,
                                                                 float alpha, float* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_w[StemDgradLds<T>::kWeightBytes];
  __shared__ float lds_v[4][32 * kSdVRow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  // weights: fp32 OHWI [co][r][s][c] -> the B image; columns 21..31 are zero
  if constexpr (sizeof(T) == 4) {
    float* bs = reinterpret_cast<float*>(lds_w);
    for (int i = threadIdx.x; i < 7 * 64 * 32; i += 256) {
      const int n = i & 31, co = (i >> 5) & 63, r = i >> 11;
      bs[i] = n < 21 ? w_ohwi[(co * 7 + r) * 21 + n] : 0.f;
    }
  } else {
    half* bs = reinterpret_cast<half*>(lds_w);
    for (int i = threadIdx.x; i < 7 * 32 * kSdBRowH; i += 256) {
      const int co = i % kSdBRowH, n = (i / kSdBRowH) & 31, r = i / (kSdBRowH * 32);
      bs[i] = (n < 21 && co < 64) ? (half)w_ohwi[(co * 7 + r) * 21 + n] : (half)0.f;
    }
  }
  __syncthreads();
  const int tiles_w = (W + kSdTile - 1) / kSdTile;
  const int ntiles = B * H * tiles_w;
  float* vs = lds_v[wave];
  for (int base = blockIdx.x * 4; base < ntiles; base += gridDim.x * 4) {
    const int tile = base + wave;
    const bool live = tile < ntiles;  // wave-uniform
    int tw = 0, h = 0, b = 0;
    if (live) {
      tw = tile % tiles_w;
      h = (tile / tiles_w) % H;
      b = tile / (tiles_w * H);
    }
    const int q0 = (kSdTile / 2) * tw - 2;
    if (live) {
      floatx16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      const int q = q0 + li;
      const bool qok = (unsigned)q < (unsigned)W0;
      for (int r = (h + 1) & 1; r < 7; r += 2) {
        const int p2 = h + 3 - r;  // even by construction
        const int p = p2 >> 1;
        if (p2 < 0 || p >= H0) continue;  // wave-uniform
        const T* src = gy + (((long)b * H0 + p) * W0 + (qok ? q : 0)) * 64 + 32 * lh;
        if constexpr (sizeof(T) == 4) {
          floatx4 a[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            a[j] = floatx4{0.f, 0.f, 0.f, 0.f};
            if (qok) a[j] = reinterpret_cast<const floatx4*>(src)[j];
          }
          const float* bs = reinterpret_cast<const float*>(lds_w) + (r * 64 + 32 * lh) * 32 + li;
#pragma unroll
          for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j][e], bs[(4 * j + e) * 32], acc, 0, 0, 0);
        } else {
          half8 a[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[j][e] = (half)0.f;
            if (qok) a[j] = reinterpret_cast<const half8*>(src)[j];
          }
          const half* bs = reinterpret_cast<const half*>(lds_w) + (r * 32 + li) * kSdBRowH + 32 * lh;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[j], *reinterpret_cast<const half8*>(bs + 8 * j), acc, 0, 0, 0);
        }
      }
      // C/D map of the 32x32 MFMAs: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int i = 0; i < 16; ++i) vs[((i & 3) + 8 * (i >> 2) + 4 * lh) * kSdVRow + li] = acc[i];
    }
    __syncthreads();
    if (live && lane < kSdTile) {
      const int w = kSdTile * tw + lane;
      if (w < W) {
        float sum[3] = {0.f, 0.f, 0.f};
        for (int s = (w + 1) & 1; s < 7; s += 2) {
          const int ql = ((w + 3 - s) >> 1) - q0;  // 0..31 (tile geometry above); columns outside [0, W0) hold zeros
          const float* v = vs + ql * kSdVRow + s * 3;
          sum[0] += v[0];
          sum[1] += v[1];
          sum[2] += v[2];
        }
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float o = alpha * sum[c];
          bad = bad || !(fabsf(o) <= 3.402823466e38f);
          gx[(((long)b * 3 + c) * H + h) * W + w] = o;
        }
        if (bad && nonfinite) nonfinite[0] = 1.f;  // (every writer stores the same value)
      }
    }
    __syncthreads();
  }
}

template <typename T>
inline void launch_stem_dgrad(const T* gy, const float* w_ohwi, float* gx, int B, int H, int W, float alpha, float* nonfinite,
                              hipStream_t s) {
  const int H0 = (H - 1) / 2 + 1, W0 = (W - 1) / 2 + 1;
  // two workgroups per CU (LDS: 74 KB fp32 / 49 KB fp16 each); fewer when there are not that many tiles
  const int blocks = cdiv(stem_dgrad_tiles(B, H, W), 4);
  const int grid = blocks < 512 ? blocks : 512;
  hipLaunchKernelGGL((stem_dgrad_kernel<T>), dim3(grid), dim3(256), 0, s, gy, w_ohwi, gx, B, H, W, H0, W0, alpha, nonfinite);
}

// ---- seed: d(poses) ------------------------------------------------------------------------------------------------------------
// dposes = scale * cot, or scale * fill everywhere when there is no cotangent (pose.mean(): fill = 1 / (6 B))
static __global__ void __launch_bounds__(256) input_grad_seed_kernel(const float* __restrict__ cot, float* __restrict__ dposes, int n,
                                                                      float fill, float scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dposes[i] = scale * (cot ? cot[i] : fill);
}
inline void launch_input_grad_seed(const float* cot, float* dposes, int n, float fill, float scale, hipStream_t s) {
  hipLaunchKernelGGL(input_grad_seed_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, cot, dposes, n, fill, scale);
}

// ---- BatchNorm backward at inference ------------------------------------------------------------------------------------------
// y_bn = y * scale[c] + shift[c] with scale = gamma / sqrt(running_var + eps) (the first half of a unit's coef_f in eval mode), so
// gy = g * scale[c], times the unit's ReLU gate where the unit has one of its own:
//   gate == nullptr                 no gate (bn2 and the projection: their incoming gradient is stored already gated)
//   gate, shift == nullptr          gate = the unit's ReLU output (a1, a0)
//   gate, shift                     gate = the unit's raw conv output y; the ReLU's outcome is recomputed as the forward pass
//                                   computed it (the fused BatchNorm + ReLU + max-pool pass of the stem never stores a0)
// No sums, no d(gamma) / d(beta).  One 16-byte piece per lane; one rounding to T.
template <typename T>
static __global__ void __launch_bounds__(256) bn_eval_bwd_kernel(const T* __restrict__ g, const T* __restrict__ gate,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  T* __restrict__ gy, long npieces, int C) {
  constexpr int VEC = ElemTraits<T>::VEC;
  const int cpr = C / VEC;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npieces; i += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % cpr) * VEC;
    PieceView<T> v, k, o;
    v.p = reinterpret_cast<const piece_t*>(g)[i];
    if (gate) k.p = reinterpret_cast<const piece_t*>(gate)[i];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const float sc = scale[c0 + e];
      float f = (float)v.e[e];
      if (gate) {
        float a = (float)k.e[e];
        if (shift) a = (float)(T)fmaxf(a * sc + shift[c0 + e], 0.f);
        if (!(a > 0.f)) f = 0.f;
      }
      o.e[e] = (T)(f * sc);
    }
    reinterpret_cast<piece_t*>(gy)[i] = o.p;
  }
}

template <typename T>
inline void launch_bn_eval_bwd(const T* g, const T* gate, const float* scale, const float* shift, T* gy, long M, int C,
                               hipStream_t s) {
  const long np = M * C / ElemTraits<T>::VEC;
  hipLaunchKernelGGL((bn_eval_bwd_kernel<T>), dim3(ew_grid(np)), dim3(256), 0, s, g, gate, scale, shift, gy, np, C);
}

// ---- saliency map ---------------------------------------------------------------------------------------------------------------
// plot_activations.py:130-133: act = max_c |gx * x|; act -= act.min(); act /= act.max(), per image.  x is the normalised image as
// the network saw it: fp32 NCHW, or recomputed from the uint8 NHWC frame exactly as the input conversion computes it.
// Two launches: (1) act -> out and the (min, max) of each chunk of pixels -> work[img][chunk][2]; (2) every workgroup folds its
// image's chunk partials and normalises its chunk.  Minimum and maximum do not depend on the order they are taken in, so the map is
// bit-reproducible.  A constant act (range 0) gives an all-zero map where the reference's division gives NaN.
constexpr int kSalChunks = 64;

static __global__ void __launch_bounds__(256) saliency_partials_kernel(const float* __restrict__ gx, const float* __restrict__ x,
                                                                        const unsigned char* __restrict__ x_u8, InputNorm nm,
                                                                        float* __restrict__ out, float* __restrict__ work, int HW) {
  __shared__ float red[2][4];
  const int img = blockIdx.y, chunk = (HW + kSalChunks - 1) / kSalChunks;
  const int p0 = blockIdx.x * chunk, p1 = min(HW, p0 + chunk);
  float lo = INFINITY, hi = -INFINITY;
  for (int p = p0 + (int)threadIdx.x; p < p1; p += blockDim.x) {
    float act = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long i = ((long)img * 3 + c) * HW + p;
      const float xv = x_u8 ? (float)x_u8[((long)img * HW + p) * 3 + c] * nm.scale[c] + nm.shift[c] : x[i];
      act = fmaxf(act, fabsf(gx[i] * xv));
    }
    out[(long)img * HW + p] = act;
    lo = fminf(lo, act);
    hi = fmaxf(hi, act);
  }
  for (int d = 32; d >= 1; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d));
    hi = fmaxf(hi, __shfl_xor(hi, d));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = lo;
    red[1][threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = work + ((long)img * kSalChunks + blockIdx.x) * 2;
    o[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    o[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

static __global__ void __launch_bounds__(256) saliency_normalise_kernel(float* __restrict__ out, const float* __restrict__ work,
                                                                         int HW) {
  __shared__ float range[2];
  const int img = blockIdx.y, chunk = (HW + kSalChunks - 1) / kSalChunks;
  const int p0 = blockIdx.x * chunk, p1 = min(HW, p0 + chunk);
  if (threadIdx.x < 64) {
    const float* wk = work + ((long)img * kSalChunks + threadIdx.x) * 2;  // kSalChunks = 64: one chunk per lane
    float lo = wk[0], hi = wk[1];
    for (int d = 32; d >= 1; d >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, d));
      hi = fmaxf(hi, __shfl_xor(hi, d));
    }
    if (threadIdx.x == 0) {
      range[0] = lo;
      range[1] = hi - lo;
    }
  }
  __syncthreads();
  const float lo = range[0], span = range[1];
  for (int p = p0 + (int)threadIdx.x; p < p1; p += blockDim.x) {
    const long i = (long)img * HW + p;
    out[i] = span > 0.f ? (out[i] - lo) / span : 0.f;
  }
}

// work: [B][kSalChunks][2] floats.  Exactly one of x (fp32 NCHW) / x_u8 (uint8 NHWC, with nm) is given.
inline void launch_saliency(const float* gx, const float* x, const unsigned char* x_u8, InputNorm nm, float* out, float* work, int B,
                            int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(saliency_partials_kernel, dim3(kSalChunks, B), dim3(256), 0, s, gx, x, x_u8, nm, out, work, H * W);
  hipLaunchKernelGGL(saliency_normalise_kernel, dim3(kSalChunks, B), dim3(256), 0, s, out, (const float*)work, H * W);
}

}  // namespace mn
