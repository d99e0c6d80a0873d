// Sequence evaluation: the windows of a whole sequence assembled on the device from one pose per frame (mn_seq_windows).
//
// Replaces the per-window host work of the reference's inference loop: scripts/eval.py:166-182 turns every window's predictions
// and VO targets into (t, unit quaternion) rows with the numpy qexp, and dataset_loaders/composite.py:88 computes the window's VOs
// with vo_func (calc_vos_safe / calc_vos_safe_fc, common/pose_utils.py:219-232, :276-304) inside MF.__getitem__.  In eval mode a
// frame's pose does not depend on the window that asks for it, so both are functions of two tables of one row per frame and the
// matrix `win` of frame indices:
//   poses7[w][k] = (t, qexp(log q)) of pose_table[win[w][k]], in fp64 from the fp32 row     (evaluate.to_pose7(row, 0, 1))
//   vos7[w][p]   = the same of the fp32 VO six-vector of vo_table[win[w][i]], vo_table[win[w][j]], pair p = (i, j)
// which is what mn_pgo_optimize reads.
//
// The VO six-vector is data._calc_vos_safe_pairs in fp32 and in its operation order: fp32 qexp of both log-quaternions, conjugate,
// _rotate of the translation difference, normalised _qmult, qlog with its all-zero-vector case.  cos, sin and arccos are evaluated
// in fp64 and rounded once (numpy's fp32 routines are within an ulp of that).  CONTRACTION IS OFF in every function of this file:
// windows at the ends of a sequence repeat the boundary frame, and for a repeated frame the vector part of the product
// a0 b_v + b0 a_v + a_v x b_v cancels exactly only if each product is rounded on its own; an FMA leaves ~1e-8 beside w = 1 - ulp,
// which arccos turns into a rotation of ~3e-4 where the host returns exact zeros.
//
// One thread per (window, slot) and one per (window, pair): item e of window w is slot e for e < N, else pair e - N; the grid
// strides over the windows.  No LDS, no atomics, every output element has one writer.  An index outside [0, L) never becomes an
// address: the slot reads row 0 and *bad = 1 (the convention of csrc/gather.h), reported by the slot's own thread.
#pragma once
#include "common.h"
#include "pgo.h"

namespace mn {

struct SeqWinArgs {
  const float* pose_table;  // [L][6]
  const float* vo_table;    // [L][6] or NULL
  const int32_t* win;       // [W][N]
  int L, W, N, fc;
  double* poses7;  // [W][N][7]
  double* vos7;    // [W][P][7] or NULL
  float* bad;      // or NULL
};

// row of the table slot `k` of window `w` reads
__device__ __forceinline__ int seq_row(const SeqWinArgs& a, long w, int k, bool reporter) {
  const int v = a.win[w * a.N + k];
  if (v >= 0 && v < a.L) return v;
  if (reporter && a.bad) *a.bad = 1.f;
  return 0;
}

// evaluate.qexp in fp64: [cos n, sinc(n / pi) q], numpy.sinc's own evaluation (as the update step of csrc/pgo.h)
__device__ __forceinline__ void seq_qexp64(const double* q, double* o) {
#pragma clang fp contract(off)
  const double n = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  const double xs = n / 3.141592653589793;
  const double y = 3.141592653589793 * (xs == 0.0 ? 1.0e-20 : xs);
  const double sc = sin(y) / y;
  o[0] = cos(n);
  o[1] = sc * q[0];
  o[2] = sc * q[1];
  o[3] = sc * q[2];
}

// (t, log q) -> the seven doubles of a pose row
__device__ __forceinline__ void seq_store7(const float* p, double* out) {
  const double q[3] = {(double)p[3], (double)p[4], (double)p[5]};
  double e[4];
  seq_qexp64(q, e);
  out[0] = (double)p[0]; out[1] = (double)p[1]; out[2] = (double)p[2];
  out[3] = e[0]; out[4] = e[1]; out[5] = e[2]; out[6] = e[3];
}

// the same map in fp32, as numpy evaluates it on float32 operands
__device__ __forceinline__ void seq_qexp32(const float* q, float* o) {
#pragma clang fp contract(off)
  const float pi = 3.14159265358979f;
  const float n = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  const float xs = n / pi;
  const float y = pi * (xs == 0.f ? 1.0e-20f : xs);
  const float sc = (float)sin((double)y) / y;
  o[0] = (float)cos((double)n);
  o[1] = sc * q[0];
  o[2] = sc * q[1];
  o[3] = sc * q[2];
}

__device__ __forceinline__ void seq_cross32(const float* a, const float* b, float* o) {
#pragma clang fp contract(off)
  const float x = a[1] * b[2] - a[2] * b[1];
  const float y = a[2] * b[0] - a[0] * b[2];
  const float z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}

// data._calc_vos_safe_pairs for one pair: p0, p1 [6] -> vo [6]
__device__ __forceinline__ void seq_vo32(const float* p0, const float* p1, float* vo) {
#pragma clang fp contract(off)
  float q0[4], q1[4];
  seq_qexp32(p0 + 3, q0);
  seq_qexp32(p1 + 3, q1);
  const float a0 = q0[0], av[3] = {-q0[1], -q0[2], -q0[3]};  // q0i: the conjugate
  // _rotate(t1 - t0, q0i) = t + 2 q_s (q_v x t) + 2 q_v x (q_v x t)
  const float t[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  float b[3], c[3];
  seq_cross32(av, t, b);
  seq_cross32(av, b, c);
  const float s2 = 2.f * a0;
#pragma unroll
  for (int i = 0; i < 3; ++i) vo[i] = (t[i] + s2 * b[i]) + 2.f * c[i];
  // _qmult(q0i, q1), normalised
  const float b0 = q1[0], *bv = q1 + 1;
  float x[3], q[4];
  seq_cross32(av, bv, x);
  q[0] = a0 * b0 - ((av[0] * bv[0] + av[1] * bv[1]) + av[2] * bv[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) q[1 + i] = (a0 * bv[i] + b0 * av[i]) + x[i];
  const float nq = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = q[i] / nq;
  // qlog
  if (q[1] == 0.f && q[2] == 0.f && q[3] == 0.f) {
    vo[3] = vo[4] = vo[5] = 0.f;
    return;
  }
  const float ang = (float)acos((double)q[0]);
  const float nv = sqrtf((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
  for (int i = 0; i < 3; ++i) vo[3 + i] = (ang * q[1 + i]) / nv;
}

static __global__ void __launch_bounds__(128) seq_windows_kernel(SeqWinArgs a) {
  const int N = a.N;
  const int P = a.vos7 ? (a.fc ? N * (N - 1) / 2 : N - 1) : 0;
  const int e = threadIdx.x;  // item of the window: slots, then pairs (N + P <= 78 < 128)
  if (e >= N + P) return;
  int i = 0, j = 0;
  if (e >= N) {  // pair e - N -> (i, j): consecutive, or i < j in lexicographic order
    int k = e - N;
    if (a.fc) {
      for (; k >= N - 1 - i; ++i) k -= N - 1 - i;  // row i of the upper triangle holds N - 1 - i pairs
      j = i + 1 + k;
    } else {
      i = k;
      j = k + 1;
    }
  }
  for (long w = blockIdx.x; w < a.W; w += gridDim.x) {
    if (e < N) {
      seq_store7(a.pose_table + 6l * seq_row(a, w, e, true), a.poses7 + (w * N + e) * 7);
    } else {
      float vo[6];
      seq_vo32(a.vo_table + 6l * seq_row(a, w, i, false), a.vo_table + 6l * seq_row(a, w, j, false), vo);
      seq_store7(vo, a.vos7 + (w * P + (e - N)) * 7);
    }
  }
}

// empty on success
inline const char* seq_windows_error(const SeqWinArgs& a) {
  if (!a.pose_table || !a.win || !a.poses7) return "pose_table, win and poses7 are required";
  if ((a.vo_table == nullptr) != (a.vos7 == nullptr)) return "vo_table and vos7 go together: both or neither";
  if (a.L < 1 || a.W < 1) return "L and W must be at least 1";
  if (a.N < 2 || a.N > kPgoMaxN) return "2 <= poses per window <= 12";
  if (((uintptr_t)a.pose_table & 3) || ((uintptr_t)a.vo_table & 3) || ((uintptr_t)a.win & 3)) return "tables and win must be 4-byte aligned";
  if (((uintptr_t)a.poses7 & 7) || ((uintptr_t)a.vos7 & 7)) return "poses7 and vos7 must be 8-byte aligned";
  return "";
}

inline void launch_seq_windows(const SeqWinArgs& a, hipStream_t s) {  // one 128-thread workgroup per window, at most 4096 of them
  hipLaunchKernelGGL(seq_windows_kernel, dim3(a.W < 4096 ? a.W : 4096), dim3(128), 0, s, a);
}

}  // namespace mn
