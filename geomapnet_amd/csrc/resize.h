// Resize on the device for uint8 input frames (mn_set_input_resize, mn_op_resize_u8): `transforms.Resize(256)`, the first link of
// the reference's image transform, i.e. PIL's Image.resize((W, H), Image.BILINEAR) per frame -- Pillow's two-pass resample in
// 8-bit fixed point, bit for bit.  Per axis (in -> out pixels) the host computes Pillow's coefficient table in double:
//   scale = in / out, fs = max(scale, 1), support = fs, ksize = (int)ceil(support) * 2 + 1; per output index xx:
//   center = (xx + 0.5) * scale, xmin = max(0, (int)(center - support + 0.5)), xmax = min(in, (int)(center + support + 0.5)),
//   w[x] = tri((x + xmin - center + 0.5) / fs), k[x] = w[x] / sum(w), K[x] = (int)(0.5 + k[x] * 2^22)   (-0.5 below zero)
// One pass along an axis: out = clamp((2^21 + sum_x K[x] * pixel[xmin + x]) >> 22, 0, 255) in 32-bit integers per channel.  The
// horizontal pass runs first and is ROUNDED TO uint8; the vertical pass runs over that.  An axis whose size does not change has
// no pass in Pillow; here it gets the identity table (one tap of 2^22), which passes every byte through unchanged.
//
// One fused kernel: a workgroup owns a tile of th output rows x tw output columns of one frame.  It (1) loads the band of source
// rows and columns the tile needs into LDS as 16-byte pieces of each row's byte span (pixels are 3 bytes: a span starts at any
// byte, so each row keeps its own skew of 0..15 bytes), (2) runs the horizontal pass over every band row into a uint8 LDS
// intermediate, (3) runs the vertical pass from that into an LDS image of the output rows with the skew of their global
// addresses, and (4) stores it as 16-byte pieces, the ragged ends of a row as dwords and bytes.  The [B][sh][W][3] intermediate
// never leaves LDS; source bytes are read once plus the tile halo.  No atomics, no scratch memory.
// With an index (mn_set_input_index, mn_op_resize_u8_indexed) the input is a frame store and image b reads frame index[b] of it: the
// batch is gathered by the resample itself; without one every address is what it was.
#pragma once
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "gather.h"

namespace mn {

constexpr int kResizeBits = 22;  // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int kResizeLdsSmall = 24 * 1024, kResizeLdsLarge = 48 * 1024;  // the kernel's two LDS budgets (6 / 3 workgroups per CU)

// Pillow's coefficients of one axis: bounds[out][2] = (xmin, taps), k[out][ksize] fixed-point weights (zero beyond `taps`)
struct ResizeAxis {
  int in = 0, out = 0, ksize = 0;
  std::vector<int> bounds, k;
};

inline ResizeAxis resize_axis(int in, int out) {
#pragma clang fp contract(off)  // the table must equal the plain double evaluation: no fused multiply-add
  ResizeAxis a;
  a.in = in;
  a.out = out;
  if (in == out) {  // no pass along this axis: the identity
    a.ksize = 1;
    a.bounds.resize((size_t)out * 2);
    a.k.assign((size_t)out, 1 << kResizeBits);
    for (int i = 0; i < out; ++i) {
      a.bounds[2 * i] = i;
      a.bounds[2 * i + 1] = 1;
    }
    return a;
  }
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = fs;
  a.ksize = (int)ceil(support) * 2 + 1;
  a.bounds.resize((size_t)out * 2);
  a.k.assign((size_t)out * a.ksize, 0);
  std::vector<double> w((size_t)a.ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      double t = (x + xmin - center + 0.5) / fs;
      if (t < 0.0) t = -t;
      w[x] = t < 1.0 ? 1.0 - t : 0.0;
      ww += w[x];
    }
    for (int x = 0; x < n; ++x) {
      const double k = ww != 0.0 ? w[x] / ww : w[x];
      a.k[(size_t)xx * a.ksize + x] = (int)(k < 0.0 ? -0.5 + k * (double)(1 << kResizeBits) : 0.5 + k * (double)(1 << kResizeBits));
    }
    a.bounds[2 * xx] = xmin;
    a.bounds[2 * xx + 1] = n;
  }
  return a;
}

// what the kernel needs to know of one conversion: sizes, the tile the host chose, LDS pitches and offsets (bytes), device tables
struct ResizeGeom {
  int B, sh, sw, H, W;
  int th, tw, tw_log2;  // output rows x columns of a tile; tw is a power of two
  int ksh, ksv;
  int pitch_s, pitch_i, pitch_o;  // LDS row pitches: source band (16-byte pieces), intermediate (dwords), output image (pieces)
  int off_inter, off_hb, off_hk, off_vb, off_vk;  // LDS offsets; the source band and, after it, the output image sit at 0
  int lds_bytes;
  const int *hb, *hk, *vb, *vk;  // device: bounds and weights of the horizontal and the vertical pass
};

inline int resize_align(int v, int a) { return (v + a - 1) / a * a; }
inline int64_t resize_table_ints(const ResizeAxis& h, const ResizeAxis& v) {
  return (int64_t)h.out * (2 + h.ksize) + (int64_t)v.out * (2 + v.ksize);
}
// bytes of the resized frames [B][H][W][3] at the head of a work buffer (the tables follow, 256-byte aligned)
inline int64_t resize_frames_bytes(int64_t B, int H, int W) { return (B * H * W * 3 + 255) / 256 * 256; }

// largest span of source indices any tile of `t` outputs needs; -1 if the bounds are not monotone (the kernel takes the band
// from the first and the last output of a tile)
inline int resize_max_span(const ResizeAxis& a, int t) {
  int best = 0;
  for (int i = 0; i < a.out; ++i)
    if (i > 0 && (a.bounds[2 * i] < a.bounds[2 * i - 2] || a.bounds[2 * i] + a.bounds[2 * i + 1] < a.bounds[2 * i - 2] + a.bounds[2 * i - 1]))
      return -1;
  for (int i0 = 0; i0 < a.out; i0 += t) {
    const int i1 = (i0 + t < a.out ? i0 + t : a.out) - 1;
    const int span = a.bounds[2 * i1] + a.bounds[2 * i1 + 1] - a.bounds[2 * i0];
    best = span > best ? span : best;
  }
  return best;
}

// LDS layout of a (th, tw) tile; false if it does not fit `budget`
inline bool resize_layout(const ResizeAxis& h, const ResizeAxis& v, int th, int tw, int budget, ResizeGeom& g) {
  const int sr = resize_max_span(v, th), sc = resize_max_span(h, tw);
  if (sr < 0 || sc < 0) return false;
  g.th = th;
  g.tw = tw;
  g.tw_log2 = 0;
  while ((1 << g.tw_log2) < tw) ++g.tw_log2;
  g.pitch_s = resize_align(sc * 3 + 15, 16);
  g.pitch_i = resize_align(tw * 3, 4);
  g.pitch_o = resize_align(tw * 3 + 15, 16);
  const long band = (long)sr * g.pitch_s, image = (long)th * g.pitch_o;
  long off = resize_align((int)(band > image ? band : image), 16);
  if (off > budget) return false;
  g.off_inter = (int)off;
  off += resize_align(sr * g.pitch_i, 16);
  if (off > budget) return false;
  g.off_hb = (int)off;
  off += (long)tw * 8;
  g.off_hk = (int)off;
  off += (long)tw * h.ksize * 4;
  g.off_vb = (int)off;
  off += (long)th * 8;
  g.off_vk = (int)off;
  off += (long)th * v.ksize * 4;
  g.lds_bytes = (int)off;
  return off <= budget;
}

// The tile: the largest th x tw (th <= 16 rows, tw <= 128 columns, powers of two) whose source band, intermediate and tables fit
// the small LDS budget; when that leaves fewer than 512 output pixels per workgroup (a shrink beyond ~2.5x), the large budget.
// A band that fits neither at 1 x 1 (a shrink beyond ~60x) is an error.
inline bool resize_choose_tile(const ResizeAxis& h, const ResizeAxis& v, ResizeGeom& g) {
  for (int budget : {kResizeLdsSmall, kResizeLdsLarge}) {
    ResizeGeom best;
    int area = 0;
    for (int th = 16; th >= 1; th >>= 1)
      for (int tw = 128; tw >= 1; tw >>= 1) {
        ResizeGeom c = g;
        if (th * tw > area && resize_layout(h, v, th, tw, budget, c)) {
          best = c;
          area = th * tw;
        }
      }
    if (area >= 512 || (area > 0 && budget == kResizeLdsLarge)) {
      g = best;
      return true;
    }
  }
  return false;
}

__device__ __forceinline__ unsigned resize_clip8(int acc) {
  const int v = acc >> kResizeBits;  // arithmetic shift
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

template <int LDS>
static __global__ void __launch_bounds__(256) resize_u8_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                               ResizeGeom g, const int32_t* __restrict__ index, long store_frames,
                                                               float* bad) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * g.tw, y0 = blockIdx.y * g.th, b = blockIdx.z;
  const int tw = min(g.tw, g.W - x0), th = min(g.th, g.H - y0);
  int* const hb = reinterpret_cast<int*>(lds + g.off_hb);
  int* const hk = reinterpret_cast<int*>(lds + g.off_hk);
  int* const vb = reinterpret_cast<int*>(lds + g.off_vb);
  int* const vk = reinterpret_cast<int*>(lds + g.off_vk);
  unsigned char* const inter = lds + g.off_inter;
  // the tile's slices of the tables
  for (int i = tid; i < tw * 2; i += 256) hb[i] = g.hb[x0 * 2 + i];
  for (int i = tid; i < tw * g.ksh; i += 256) hk[i] = g.hk[(long)x0 * g.ksh + i];
  for (int i = tid; i < th * 2; i += 256) vb[i] = g.vb[y0 * 2 + i];
  for (int i = tid; i < th * g.ksv; i += 256) vk[i] = g.vk[(long)y0 * g.ksv + i];
  // the band of source rows [r0, r0 + SR) and columns [c0, c0 + len / 3): bounds are monotone, first and last output decide
  const int c0 = g.hb[x0 * 2], len = (g.hb[(x0 + tw - 1) * 2] + g.hb[(x0 + tw - 1) * 2 + 1] - c0) * 3;
  const int r0 = g.vb[y0 * 2], SR = g.vb[(y0 + th - 1) * 2] + g.vb[(y0 + th - 1) * 2 + 1] - r0;
  // the source frame: image b of the batch, or -- gathered from a frame store (mn_set_input_index) -- frame index[b] of
  // `store_frames`; an index outside the store reads frame 0 and sets *bad (gather.h)
  const long frames = index ? store_frames : (long)g.B;
  const long sb = index ? checked_frame(index, b, store_frames, bad, blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) : (long)b;
  const uintptr_t in_lo = (uintptr_t)in, in_hi = in_lo + (uintptr_t)(frames * g.sh * g.sw * 3);
  const uintptr_t band = in_lo + (uintptr_t)(((sb * g.sh + r0) * g.sw + c0) * 3);  // first byte of the band's first row
  const long row_bytes = (long)g.sw * 3;

  // (1) source rows -> LDS, 16-byte pieces at their global alignment; a piece that leaves the input buffer is read by bytes
  const int vpr = g.pitch_s >> 4;
  for (int i = tid; i < SR * vpr; i += 256) {
    const int j = i / vpr, v = i - j * vpr;
    const uintptr_t a = band + (uintptr_t)(j * row_bytes);
    const int sk = (int)(a & 15);
    if (v * 16 >= sk + len) continue;
    const uintptr_t p = a - sk + (uintptr_t)(v * 16);
    piece_t val;
    if (p >= in_lo && p + 16 <= in_hi) {
      val = *reinterpret_cast<const piece_t*>(p);
    } else {
      union {
        piece_t p;
        unsigned char e[16];
      } u;
#pragma unroll
      for (int e = 0; e < 16; ++e) u.e[e] = (p + e >= in_lo && p + e < in_hi) ? *reinterpret_cast<const unsigned char*>(p + e) : 0;
      val = u.p;
    }
    *reinterpret_cast<piece_t*>(lds + j * g.pitch_s + v * 16) = val;
  }
  __syncthreads();

  // (2) horizontal pass over every band row -> uint8 intermediate [SR][tw][3]
  for (int i = tid; i < (SR << g.tw_log2); i += 256) {
    const int j = i >> g.tw_log2, x = i & (g.tw - 1);
    if (x >= tw) continue;
    const int sk = (int)((band + (uintptr_t)(j * row_bytes)) & 15);
    const unsigned char* s = lds + j * g.pitch_s + sk + (hb[2 * x] - c0) * 3;
    const int n = hb[2 * x + 1];
    const int* k = hk + x * g.ksh;
    int a0 = 1 << (kResizeBits - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t) {
      const int kk = k[t];
      a0 += kk * (int)s[3 * t];
      a1 += kk * (int)s[3 * t + 1];
      a2 += kk * (int)s[3 * t + 2];
    }
    unsigned char* d = inter + j * g.pitch_i + x * 3;
    d[0] = (unsigned char)resize_clip8(a0);
    d[1] = (unsigned char)resize_clip8(a1);
    d[2] = (unsigned char)resize_clip8(a2);
  }
  __syncthreads();  // (the source band is dead from here on: the output image takes its place)

  // (3) vertical pass, four bytes of an intermediate row per item -> the output rows in LDS at the skew of their global address
  const uintptr_t obase = (uintptr_t)out + (uintptr_t)((((long)b * g.H + y0) * g.W + x0) * 3);
  const long orow_bytes = (long)g.W * 3;
  const int L = tw * 3;
  const int nq = g.pitch_i >> 2;
  for (int i = tid; i < th * nq; i += 256) {
    const int y = i / nq, q = i - y * nq;
    if (q * 4 >= L) continue;
    const unsigned char* s = inter + (vb[2 * y] - r0) * g.pitch_i + q * 4;
    const int n = vb[2 * y + 1];
    const int* k = vk + y * g.ksv;
    int a0 = 1 << (kResizeBits - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int t = 0; t < n; ++t) {
      const int kk = k[t];
      const unsigned w = *reinterpret_cast<const unsigned*>(s + t * g.pitch_i);
      a0 += kk * (int)(w & 255u);
      a1 += kk * (int)(w >> 8 & 255u);
      a2 += kk * (int)(w >> 16 & 255u);
      a3 += kk * (int)(w >> 24);
    }
    const int so = (int)((obase + (uintptr_t)(y * orow_bytes)) & 15);
    unsigned char* d = lds + y * g.pitch_o + so + q * 4;
    const unsigned r[4] = {resize_clip8(a0), resize_clip8(a1), resize_clip8(a2), resize_clip8(a3)};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (q * 4 + e < L) d[e] = (unsigned char)r[e];
  }
  __syncthreads();

  // (4) output rows -> global: whole 16-byte pieces inside the row's span; at its ragged ends whole dwords, then bytes
  const int opr = g.pitch_o >> 4;
  for (int i = tid; i < th * opr; i += 256) {
    const int y = i / opr, v = i - y * opr;
    const uintptr_t a = obase + (uintptr_t)(y * orow_bytes);
    const int so = (int)(a & 15);
    const int lo = v * 16, hi = lo + 16;  // this piece, relative to the aligned base; the row's bytes are [so, so + L)
    if (lo >= so + L || hi <= so) continue;
    const unsigned char* src = lds + y * g.pitch_o + lo;
    const uintptr_t p = a - so + (uintptr_t)lo;
    if (lo >= so && hi <= so + L) {
      *reinterpret_cast<piece_t*>(p) = *reinterpret_cast<const piece_t*>(src);
      continue;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int dl = lo + d * 4;
      if (dl >= so && dl + 4 <= so + L) {
        *reinterpret_cast<unsigned*>(p + d * 4) = *reinterpret_cast<const unsigned*>(src + d * 4);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (dl + e >= so && dl + e < so + L) *reinterpret_cast<unsigned char*>(p + d * 4 + e) = src[d * 4 + e];
      }
    }
  }
}

// host side of one conversion: the two tables, the tile, where the tables sit in device memory
struct ResizePlan {
  ResizeGeom g;
  std::vector<int> tables;  // hb | hk | vb | vk, as they are copied to the device
  std::string error;
};

// -> plan.error empty on success.  `tables_dev`: device memory of resize_table_ints() ints, 4-byte aligned.
inline ResizePlan resize_plan(int B, int sh, int sw, int H, int W, int* tables_dev) {
  ResizePlan p;
  if (B < 1 || sh < 1 || sw < 1 || H < 1 || W < 1) {
    p.error = "B, source and output sizes must be positive";
    return p;
  }
  if (B > 65535) {
    p.error = "at most 65535 frames per call (the grid's z extent)";
    return p;
  }
  const ResizeAxis h = resize_axis(sw, W), v = resize_axis(sh, H);
  ResizeGeom& g = p.g;
  g.B = B; g.sh = sh; g.sw = sw; g.H = H; g.W = W;
  g.ksh = h.ksize;
  g.ksv = v.ksize;
  if (!resize_choose_tile(h, v, g)) {
    p.error = "the source band of a single output pixel does not fit LDS (a shrink beyond ~60x); resize in two steps";
    return p;
  }
  p.tables.reserve((size_t)resize_table_ints(h, v));
  p.tables.insert(p.tables.end(), h.bounds.begin(), h.bounds.end());
  p.tables.insert(p.tables.end(), h.k.begin(), h.k.end());
  p.tables.insert(p.tables.end(), v.bounds.begin(), v.bounds.end());
  p.tables.insert(p.tables.end(), v.k.begin(), v.k.end());
  g.hb = tables_dev;
  g.hk = g.hb + (size_t)W * 2;
  g.vb = g.hk + (size_t)W * h.ksize;
  g.vk = g.vb + (size_t)H * 2;
  return p;
}
inline int64_t resize_table_bytes(int sh, int sw, int H, int W) {
  const double fh = sw > W ? (double)sw / W : 1.0, fv = sh > H ? (double)sh / H : 1.0;
  const int64_t ksh = sw == W ? 1 : (int64_t)ceil(fh) * 2 + 1, ksv = sh == H ? 1 : (int64_t)ceil(fv) * 2 + 1;
  return ((int64_t)W * (2 + ksh) + (int64_t)H * (2 + ksv)) * 4;
}

// index null: in = the batch [B][sh][sw][3]; else in = a frame store [store_frames][sh][sw][3] and image b reads frame index[b]
inline void launch_resize_u8(const unsigned char* in, unsigned char* out, const ResizeGeom& g, hipStream_t s,
                             const int32_t* index = nullptr, long store_frames = 0, float* bad = nullptr) {
  const dim3 grid(cdiv(g.W, g.tw), cdiv(g.H, g.th), g.B);
  if (g.lds_bytes <= kResizeLdsSmall)
    hipLaunchKernelGGL((resize_u8_kernel<kResizeLdsSmall>), grid, dim3(256), 0, s, in, out, g, index, store_frames, bad);
  else
    hipLaunchKernelGGL((resize_u8_kernel<kResizeLdsLarge>), grid, dim3(256), 0, s, in, out, g, index, store_frames, bad);
}

}  // namespace mn
