// ColorJitter on the device for uint8 input frames (mn_set_color_jitter): torchvision's ColorJitter(brightness, contrast,
// saturation, hue) on the float image x = u8 / 255 (its tensor implementation: _blend, rgb_to_grayscale, _rgb2hsv, _hsv2rgb),
// applied inside the uint8 -> normalised NHWC4 conversion, before Normalize.  Per image of a forward pass: four factors and a
// uniformly random order of the four ops, drawn from Philox4x32-10 keyed by the seed, counter (image, pass, kJitterDomain, word):
// a draw depends on (seed, pass, image) alone, never on the launch shape.  An op whose range is zero is skipped (its bit is
// clear in `active`), as torchvision skips it.  Contrast blends with the mean gray level of the image as it stands at that
// point of its order: a separate pass sums gray over (image x pixel chunk) workgroups and a one-lane-per-image pass adds the
// chunk partials in a fixed order -- no float atomics, the mean is bit-reproducible.
#pragma once
#include "common.h"
#include "elementwise.h"
#include "head.h"

namespace mn {

constexpr unsigned kJitterDomain = 0x4A495454u;  // Philox counter word 2 ("JITT"; dropout uses 0 there)
constexpr int kJitterChunks = 8;                 // gray-sum workgroups per image
enum { kJitBright = 0, kJitContrast = 1, kJitSat = 2, kJitHue = 3 };  // torchvision's op ids

struct JitterParams {
  float lo[4], hi[4];  // factor ranges: brightness / contrast / saturation [max(0, 1-v), 1+v], hue [-v, v]
  unsigned active;     // bit op: the op's range is non-zero
  unsigned seed_lo, seed_hi, call;
};

__device__ __forceinline__ float jit_u24(unsigned r) { return (float)(r >> 8) * (1.f / 16777216.f); }  // [0, 1)

// draws[img][8] = {b, c, s, h, op0, op1, op2, op3}: the factors, then the op ids in the order they are applied (a uniform
// permutation by Fisher-Yates).  A skipped op reports its identity factor (1, 1, 1, 0) and keeps its place in the order.
static __global__ void __launch_bounds__(256) jitter_draw_kernel(float* __restrict__ draws, int images, JitterParams jp) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= images) return;
  unsigned r[4], q[4];
  philox4x32_10((unsigned)img, jp.call, kJitterDomain, 0u, jp.seed_lo, jp.seed_hi, r);
  philox4x32_10((unsigned)img, jp.call, kJitterDomain, 1u, jp.seed_lo, jp.seed_hi, q);
  float* d = draws + (long)img * 8;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    d[k] = (jp.active >> k & 1u) ? jp.lo[k] + jit_u24(r[k]) * (jp.hi[k] - jp.lo[k]) : (k == kJitHue ? 0.f : 1.f);
  int op[4] = {0, 1, 2, 3};
#pragma unroll
  for (int i = 3; i > 0; --i) {
    int j = (int)(jit_u24(q[i]) * (float)(i + 1));
    j = j > i ? i : j;
    const int t = op[i];
    op[i] = op[j];
    op[j] = t;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) d[4 + k] = (float)op[k];
}

__device__ __forceinline__ float jit_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float jit_gray(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// adjust_hue: _rgb2hsv, H = (H + f) mod 1, _hsv2rgb (torchvision/transforms/_functional_tensor.py)
__device__ __forceinline__ void jit_hue(float& r, float& g, float& b, float f) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.f : maxc);
  const float crd = eqc ? 1.f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  float h;
  if (maxc == r)
    h = bc - gc;
  else if (maxc == g)
    h = 2.f + rc - bc;
  else
    h = 4.f + gc - rc;
  h = fmodf(h / 6.f + 1.f, 1.f);
  h = h + f;
  h = h - floorf(h);  // Python's % 1.0: the result takes the divisor's sign
  const float v = maxc;
  const float h6 = h * 6.f, fi = floorf(h6), fr = h6 - fi;
  const int i = ((int)fi) % 6;
  const float p = jit_clamp01(v * (1.f - s)), q = jit_clamp01(v * (1.f - s * fr)), t = jit_clamp01(v * (1.f - s * (1.f - fr)));
  switch (i) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// one op of the chain on one pixel (m: the image's mean gray at the contrast op)
__device__ __forceinline__ void jit_op(int op, float f, float m, float& r, float& g, float& b) {
  if (op == kJitBright) {
    r = jit_clamp01(f * r);
    g = jit_clamp01(f * g);
    b = jit_clamp01(f * b);
  } else if (op == kJitContrast) {
    const float o = (1.f - f) * m;
    r = jit_clamp01(f * r + o);
    g = jit_clamp01(f * g + o);
    b = jit_clamp01(f * b + o);
  } else if (op == kJitSat) {
    const float o = (1.f - f) * jit_gray(r, g, b);
    r = jit_clamp01(f * r + o);
    g = jit_clamp01(f * g + o);
    b = jit_clamp01(f * b + o);
  } else {
    jit_hue(r, g, b, f);
  }
}

// contrast mean, stage 1: grid (kJitterChunks, images).  Each workgroup applies the ops its image draws BEFORE contrast to one
// chunk of pixels and sums their gray level; lanes, then the four waves, add in a fixed order -> partials[img][chunk].
static __global__ void __launch_bounds__(256) jitter_gray_partials_kernel(const unsigned char* __restrict__ in,
                                                                          const float* __restrict__ draws,
                                                                          float* __restrict__ partials, int HW, unsigned active) {
  __shared__ float red[4];
  const int img = blockIdx.y, chunk = (HW + kJitterChunks - 1) / kJitterChunks;
  const int p0 = blockIdx.x * chunk, p1 = min(HW, p0 + chunk);
  const float* d = draws + (long)img * 8;
  int ops[4];
  float fs[4];
  int nbefore = 0;
  for (int k = 0; k < 4; ++k) {
    const int op = (int)d[4 + k];
    if (op == kJitContrast) break;
    if (active >> op & 1u) {
      ops[nbefore] = op;
      fs[nbefore] = d[op];
      ++nbefore;
    }
  }
  float sum = 0.f;
  const unsigned char* src = in + (long)img * HW * 3;
  for (int p = p0 + (int)threadIdx.x; p < p1; p += blockDim.x) {
    float r = (float)src[(long)p * 3 + 0] / 255.f, g = (float)src[(long)p * 3 + 1] / 255.f, b = (float)src[(long)p * 3 + 2] / 255.f;
    for (int k = 0; k < nbefore; ++k) jit_op(ops[k], fs[k], 0.f, r, g, b);
    sum += jit_gray(r, g, b);
  }
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partials[(long)img * kJitterChunks + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// contrast mean, stage 2: one lane per image, the chunk partials in chunk order
static __global__ void __launch_bounds__(256) jitter_mean_kernel(const float* __restrict__ partials, float* __restrict__ mean,
                                                                 int images, int HW) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= images) return;
  float s = 0.f;
  for (int k = 0; k < kJitterChunks; ++k) s += partials[(long)img * kJitterChunks + k];
  mean[img] = s / (float)HW;
}

// ---- input: uint8 NHWC -> ColorJitter -> normalised, zero-padded NHWC4 ----------------------------------------------------
// The loop of u8nhwc_to_padded_nhwc4_kernel with the image's op chain between the load and Normalize; padding and out16 exactly
// as there.  nm: scale = 1/std, shift = -mean/std (Normalize on x in [0, 1]).  mean: per image, read only when contrast is active.
template <typename T>
static __global__ void __launch_bounds__(256) u8nhwc_jitter_to_padded_nhwc4_kernel(
    const unsigned char* __restrict__ in, T* __restrict__ out, int B, int H, int W, int Hp, int Wp, InputNorm nm,
    half* __restrict__ out16, const float* __restrict__ draws, const float* __restrict__ mean, unsigned active) {
  long total = (long)B * Hp * Wp;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int wp = (int)(i % Wp);
    long tmp = i / Wp;
    int hp = (int)(tmp % Hp);
    int b = (int)(tmp / Hp);
    int h = hp - 3, w = wp - 3;
    T v[4] = {(T)0.f, (T)0.f, (T)0.f, (T)0.f};
    if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
      const unsigned char* p = in + (((long)b * H + h) * W + w) * 3;
      float x0 = (float)p[0] / 255.f, x1 = (float)p[1] / 255.f, x2 = (float)p[2] / 255.f;
      const float* d = draws + (long)b * 8;
      const float m = (active >> kJitContrast & 1u) ? mean[b] : 0.f;
      for (int k = 0; k < 4; ++k) {
        const int op = (int)d[4 + k];
        if (active >> op & 1u) jit_op(op, d[op], m, x0, x1, x2);
      }
      v[0] = (T)(x0 * nm.scale[0] + nm.shift[0]);
      v[1] = (T)(x1 * nm.scale[1] + nm.shift[1]);
      v[2] = (T)(x2 * nm.scale[2] + nm.shift[2]);
    }
    T* o = out + i * 4;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
    o[3] = v[3];
    if (out16) {
      half4 h = {(half)(float)v[0], (half)(float)v[1], (half)(float)v[2], (half)0.f};
      *reinterpret_cast<half4*>(out16 + i * 4) = h;
    }
  }
}

// host side: the ranges (brightness, contrast, saturation, hue) of mn_set_color_jitter -> the kernels' parameters
inline JitterParams jitter_params(const float range[4], unsigned long long seed, unsigned call) {
  JitterParams jp;
  jp.active = 0;
  for (int k = 0; k < 4; ++k) {
    const float v = range[k];
    jp.lo[k] = k == kJitHue ? -v : fmaxf(0.f, 1.f - v);
    jp.hi[k] = k == kJitHue ? v : 1.f + v;
    if (v > 0.f) jp.active |= 1u << k;
  }
  jp.seed_lo = (unsigned)(seed & 0xffffffffu);
  jp.seed_hi = (unsigned)(seed >> 32);
  jp.call = call;
  return jp;
}

// one jittered input conversion: the draws of the pass, the contrast means when contrast is active, then the conversion with the
// op chain.  draws [B][8], partials [B][kJitterChunks], mean [B] floats of device memory.
template <typename T>
inline void launch_u8_jitter(const unsigned char* in, T* out, int B, int H, int W, int Hp, int Wp, InputNorm nm, half* out16,
                             const JitterParams& jp, float* draws, float* partials, float* mean, hipStream_t s) {
  hipLaunchKernelGGL(jitter_draw_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, draws, B, jp);
  if (jp.active >> kJitContrast & 1u) {
    hipLaunchKernelGGL(jitter_gray_partials_kernel, dim3(kJitterChunks, B), dim3(256), 0, s, in, (const float*)draws, partials,
                       H * W, jp.active);
    hipLaunchKernelGGL(jitter_mean_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, (const float*)partials, mean, B, H * W);
  }
  hipLaunchKernelGGL((u8nhwc_jitter_to_padded_nhwc4_kernel<T>), dim3(ew_grid((long)B * Hp * Wp)), dim3(256), 0, s, in, out, B, H,
                     W, Hp, Wp, nm, out16, (const float*)draws, (const float*)mean, jp.active);
}

}  // namespace mn
