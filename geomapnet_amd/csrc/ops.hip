// Operator-level C-ABI entry points (include/mapnet_hip.h, "Operator-level entry points").
#include "../../include/mapnet_hip.h"

#include <string>

#include "common.h"
#include "criterion.h"
#include "elementwise.h"
#include "elementwise_h2.h"
#include "frame_stats.h"
#include "head.h"
#include "jitter.h"
#include "knobs.h"
#include "dense.h"
#include "igemm.h"
#include "dgrad.h"
#include "halo_pp.h"
#include "input_grad.h"
#include "optim.h"
#include "pgo.h"
#include "pool.h"
#include "rehearsal.h"
#include "resize.h"
#include "seq_eval.h"
#include "stem.h"
#include "stem_bwd.h"
#include "wgrad.h"
#include "util.h"

using namespace mn;

namespace mn {
thread_local std::string g_last_error;
}

extern "C" const char* mn_last_error(void) { return mn::g_last_error.c_str(); }

#ifndef MN_BACKEND_NAME
#define MN_BACKEND_NAME "hip"
#endif
extern "C" const char* mn_backend(void) { return MN_BACKEND_NAME; }

// entry of a stand-alone operator: the knob table follows the environment of THIS call (knobs.h, read rule)
static void begin_op() {
  begin_call();
  load_knobs();
}

static GatherGeom to_geom(const mn_gather_geom* g) {
  GatherGeom r;
  r.B = g->B; r.Hi = g->Hi; r.Wi = g->Wi; r.C = g->C; r.P = g->P; r.Q = g->Q; r.R = g->R; r.S = g->S;
  r.mul_p = g->mul_p; r.mul_q = g->mul_q; r.rsign = g->rsign; r.ssign = g->ssign;
  r.off_h = g->off_h; r.off_w = g->off_w; r.div = g->div; r.M = g->M; r.N = g->N; r.K = g->K;
  return r;
}

static int check_geom(const GatherGeom& g, int dtype) {
  int vec = dtype == MN_F16 ? 8 : 4;
  if ((dtype == MN_DTYPE_F16X2 || dtype == MN_DTYPE_F16X2Q) && (g.C % 32 != 0 || g.N % 4 != 0))
    return fail("igemm: h2 operands need C % 32 == 0");
  if (g.C % vec != 0) return fail("igemm: C must be a multiple of the 16-byte piece");
  if (g.K != g.R * g.S * g.C) return fail("igemm: K != R*S*C");
  if (g.K % (4 * vec) != 0) return fail("igemm: K must be a multiple of the 64-byte K-step");
  if (g.M != g.B * g.P * g.Q) return fail("igemm: M != B*P*Q");
  if (g.div != 1 && g.div != 2) return fail("igemm: div must be 1 or 2");
  if (g.div == 2 && (g.rsign != -1 || g.ssign != -1)) return fail("igemm: div = 2 requires rsign = ssign = -1");
  if (g.R * g.S > 32) return fail("igemm: at most 32 taps");
  if ((long)g.B * g.Hi * g.Wi * g.C >= (1L << 31)) return fail("igemm: A tensor exceeds 2^31 elements");
  return 0;
}

extern "C" int mn_op_igemm_grid_m(int M) { return igemm_grid_m(M); }

extern "C" int mn_op_igemm(int dtype, const mn_gather_geom* gg, const void* A, const void* Bw, void* out, int ldc,
                           float* stats, const float* bias, int relu, const void* res, const void* res_gate, float alpha,
                           const void* zero_page, void* stream) {
  begin_op();
  GatherGeom g = to_geom(gg);
  if (int e = check_geom(g, dtype)) return e;
  if (!zero_page) return fail("igemm: zero_page (>= 16 zero bytes of device memory) is required");
  {
    const long es = dtype == MN_DTYPE_F16 ? 2 : 4;
    if ((long)gg->B * gg->Hi * gg->Wi * gg->C * es >= 0xfffffff0l || (long)gg->N * gg->K * es >= 0xfffffff0l)
      return fail("igemm: operands must be smaller than 4 GiB (32-bit buffer offsets)");
  }
  Epilogue ep;
  ep.out = out; ep.ldc = ldc; ep.stats = stats; ep.bias = bias; ep.relu = relu; ep.res = res; ep.res_gate = res_gate;
  ep.alpha = alpha;
  if (dtype == MN_DTYPE_F32X3) g.mma = MMA_F16X3;  // fp32 tensors, f16 matrix pipe with split operands
  if (dtype == MN_DTYPE_F16X2 || dtype == MN_DTYPE_F16X2Q) {  // h2 / h2q operands (A, Bw, res_gate), fp32 out / res
    launch_igemm_h2(g, (const half*)A, (const half*)Bw, ep, (hipStream_t)stream, (const half*)zero_page, dtype == MN_DTYPE_F16X2Q);
    return check_launch("igemm");
  }
  if (dtype == MN_F16)
    launch_igemm<half>(g, (const half*)A, (const half*)Bw, ep, (hipStream_t)stream, (const half*)zero_page);
  else
    launch_igemm<float>(g, (const float*)A, (const float*)Bw, ep, (hipStream_t)stream, (const float*)zero_page);
  return check_launch("igemm");
}

// The fused inference convolution of mn_set_eval_fused on its own: out(h2) = [relu](conv(A; Bw) * scale + shift [+ res(h2)]).
// The launch goes through the plan's dispatcher, so the kernel and tile shape are the ones mn_op_igemm(MN_DTYPE_F16X2) takes for
// the same geometry (and the same MN_* knobs) with stats = bias = res = NULL, relu = 0, alpha = 1.
extern "C" int mn_op_conv_bn_eval(int dtype, const mn_gather_geom* gg, const void* A, const void* Bw, const float* coef,
                                  const void* res, int relu, void* out, int ldc, const void* zero_page, void* stream) {
  begin_op();
  if (dtype != MN_DTYPE_F16X2 && dtype != MN_DTYPE_F16X2M)
    return fail("conv_bn_eval: dtype must be MN_DTYPE_F16X2 or MN_DTYPE_F16X2M (h2 operands, residual and output)");
  if (!gg || !A || !Bw || !out) return fail("conv_bn_eval: geometry, A, Bw and out are required");
  GatherGeom g = to_geom(gg);
  if (g.C % 32 != 0) return fail("conv_bn_eval: h2 operands need C % 32 == 0");
  if (g.N % 8 != 0) return fail("conv_bn_eval: N % 8 == 0 required (a store-pass thread writes 8 channels)");
  if (int e = check_geom(g, MN_DTYPE_F16X2)) return e;
  if (!coef) return fail("conv_bn_eval: coef (fp32 [2][N]: scale | shift) is required");
  if (((uintptr_t)coef & 15) != 0) return fail("conv_bn_eval: coef must be 16-byte aligned");
  if (ldc < g.N || ldc % 32 != 0) return fail("conv_bn_eval: ldc must be a multiple of 32 (h2 rows) and at least N");
  if (!zero_page) return fail("conv_bn_eval: zero_page (>= 16 zero bytes of device memory) is required");
  if ((long)gg->B * gg->Hi * gg->Wi * gg->C * 4 >= 0xfffffff0l || (long)gg->N * gg->K * 4 >= 0xfffffff0l)
    return fail("conv_bn_eval: operands must be smaller than 4 GiB (32-bit buffer offsets)");
  const Epilogue ep = eval_epilogue(out, ldc, coef, res, relu);
  launch_igemm_h2<true>(g, (const half*)A, (const half*)Bw, ep, (hipStream_t)stream, (const half*)zero_page, false);
  return check_launch("conv_bn_eval");
}

static int op_conv_halo_pp(const mn_gather_geom* gg, const void* A, const void* Bw, void* out, int ldc, double* stats_accum,
                           int stats_rows, int relu, const void* res, const void* res_gate, const void* out_gate, float alpha, int wgs,
                           bool gate_h2, void* stream) {
  begin_op();
  GatherGeom g = to_geom(gg);
  if (int e = check_geom(g, MN_F16)) return e;
  Epilogue ep;
  ep.out = out; ep.ldc = ldc; ep.relu = relu; ep.res = res; ep.res_gate = res_gate; ep.out_gate = out_gate; ep.alpha = alpha;
  ep.stats_accum = stats_accum; ep.stats_rows = stats_rows; ep.gate_h2 = gate_h2;
  if (!conv_halo_pp_applies(g, ep))
    return fail("conv_halo_pp: fp16 3x3 stride-1 same-size convolutions of 64 -> 64 channels only (stats_rows > 0 with stats_accum)");
  launch_conv_halo_pp(g, (const half*)A, (const half*)Bw, ep, (hipStream_t)stream, wgs);
  return check_launch("conv_halo_pp");
}
extern "C" int mn_op_conv_halo_pp(const mn_gather_geom* gg, const void* A, const void* Bw, void* out, int ldc, double* stats_accum,
                                 int stats_rows, int relu, const void* res, const void* res_gate, const void* out_gate,
                                 float alpha, int wgs, void* stream) {
  return op_conv_halo_pp(gg, A, Bw, out, ldc, stats_accum, stats_rows, relu, res, res_gate, out_gate, alpha, wgs, false, stream);
}
extern "C" int mn_op_conv_halo_pp_h2gates(const mn_gather_geom* gg, const void* A, const void* Bw, void* out, int ldc,
                                          double* stats_accum, int stats_rows, int relu, const void* res, const void* res_gate,
                                          const void* out_gate, float alpha, int wgs, void* stream) {
  return op_conv_halo_pp(gg, A, Bw, out, ldc, stats_accum, stats_rows, relu, res, res_gate, out_gate, alpha, wgs, true, stream);
}

static int op_wgrad(int dtype, const mn_gather_geom* gg, const void* dY, int ldy, const void* X, float* dW, int ldw,
                    const int32_t* colmap, float alpha, int target_blocks, const void* zero_page, float* ws, long ws_floats,
                    void* stream);
extern "C" int mn_op_conv_halo_h2(const mn_gather_geom* gg, const void* A, const void* Bw, float* out, int ldc, double* stats_accum,
                                  int stats_rows, void* stream) {
  begin_op();
  GatherGeom g = to_geom(gg);
  if (int e = check_geom(g, MN_DTYPE_F16X2)) return e;
  Epilogue ep;
  ep.out = out; ep.ldc = ldc; ep.stats_accum = stats_accum; ep.stats_rows = stats_rows;
  if (!conv_halo_h2_applies(g, ep))
    return fail("conv_halo_h2: 3x3 stride-1 same-size forward convolutions of 64 -> 64 channel h2 tensors only (stats_rows > 0 with stats_accum)");
  launch_conv_halo_h2(g, (const half*)A, (const half*)Bw, ep, (hipStream_t)stream);
  return check_launch("conv_halo_h2");
}

extern "C" int mn_op_wgrad(int dtype, const mn_gather_geom* gg, const void* dY, int ldy, const void* X, float* dW, int ldw,
                           const int32_t* colmap, float alpha, int target_blocks, const void* zero_page, void* stream) {
  return op_wgrad(dtype, gg, dY, ldy, X, dW, ldw, colmap, alpha, target_blocks, zero_page, nullptr, 0, stream);
}
extern "C" int64_t mn_op_wgrad_ws_floats(void) { return wgrad_fused_ws_floats(WGF_BLOCKS); }
extern "C" int mn_op_wgrad_ws(int dtype, const mn_gather_geom* gg, const void* dY, int ldy, const void* X, float* dW, int ldw,
                              float alpha, float* ws, int64_t ws_floats, const void* zero_page, void* stream) {
  if (!ws || ws_floats <= 0) return fail("wgrad_ws: workspace required (mn_op_wgrad_ws_floats() floats)");
  return op_wgrad(dtype, gg, dY, ldy, X, dW, ldw, nullptr, alpha, 512, zero_page, ws, (long)ws_floats, stream);
}
static int op_wgrad(int dtype, const mn_gather_geom* gg, const void* dY, int ldy, const void* X, float* dW, int ldw,
                    const int32_t* colmap, float alpha, int target_blocks, const void* zero_page, float* ws, long ws_floats,
                    void* stream) {
  begin_op();
  WgradArgs a;
  a.ws = ws;
  a.ws_floats = ws_floats;
  a.g = to_geom(gg);
  if (dtype < MN_DTYPE_F32 || dtype > MN_DTYPE_F16X2M)
    return fail("wgrad: dtype must be MN_DTYPE_F32, _F16, _F32X3, _F16X2 or _F16X2M");
  const bool mixed = dtype == MN_DTYPE_F16X2M;  // the fp16 kernels: dY plain fp16, X the hi halves of an h2 tensor
  int vec = dtype == MN_F16 || mixed ? 8 : 4;
  if (a.g.C % vec != 0 || a.g.N % vec != 0) return fail("wgrad: channel counts must be multiples of the piece");
  if (dtype == MN_DTYPE_F16X2 && (a.g.C % 32 != 0 || ldy % 32 != 0)) return fail("wgrad: h2 operands need channel counts % 32 == 0");
  if (mixed && a.g.C % 32 != 0) return fail("wgrad: an h2 X operand needs C % 32 == 0");
  a.dY = dY; a.ldy = ldy; a.X = X; a.dW = dW; a.ldw = ldw; a.colmap = colmap; a.alpha = alpha; a.rows_per_split = 0;
  if (dtype == MN_DTYPE_F32X3) a.g.mma = MMA_BF16X3;  // fp32 tensors, bf16 matrix pipe with split operands
  if (dtype == MN_DTYPE_F16X2) a.g.mma = MMA_H2;      // h2 tensors (dY, X), fp32 dW
  a.x_h2 = mixed;
  if (dtype == MN_F16 || dtype == MN_DTYPE_F16X2 || mixed)
    launch_wgrad<half>(a, target_blocks, (hipStream_t)stream, zero_page);
  else
    launch_wgrad<float>(a, target_blocks, (hipStream_t)stream);
  return check_launch("wgrad");
}

extern "C" int mn_op_stem_conv(const void* xpad, const void* wf, void* y, double* stats_accum, int stats_rows, int B, int H, int W,
                               int Wp, void* stream) {
  begin_op();
  if (Wp % 2 != 0 || Wp < W + 7) return fail("stem_conv: Wp must be even and >= W + 7");
  if ((long)B * (H + 6) * Wp * 8 >= 0xfffffff0l) return fail("stem_conv: padded input exceeds 4 GiB");
  launch_stem_conv((const half*)xpad, (const half*)wf, (half*)y, stats_accum, stats_rows, B, H, W, Wp, (hipStream_t)stream);
  return check_launch("stem_conv");
}

extern "C" int mn_op_stem_conv_x3(const float* xpad, const float* wf, float* y, double* stats_accum, int stats_rows, int B, int H,
                                  int W, int Wp, void* stream) {
  begin_op();
  if (Wp % 2 != 0 || Wp < W + 7) return fail("stem_conv_x3: Wp must be even and >= W + 7");
  launch_stem_conv_x3(xpad, wf, y, stats_accum, stats_rows, B, H, W, Wp, (hipStream_t)stream);
  return check_launch("stem_conv_x3");
}

extern "C" int mn_op_dense(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int relu, void* stream) {
  begin_op();
  DenseArgs a;
  a.A = A; a.W = W; a.bias = bias; a.C = C; a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldc = N; a.relu = relu;
  if (M <= 0 || N <= 0 || !dense_nt_applies(a)) return fail("dense: K must be a multiple of 128, A and W 16-byte aligned");
  launch_dense_nt(a, (hipStream_t)stream);
  return check_launch("dense");
}

extern "C" int mn_op_dense_wgrad(const float* dY, const float* X, float* dW, float* db, int B, int F, int Cin, float alpha,
                                 void* stream) {
  begin_op();
  if (B <= 0 || F <= 0 || Cin <= 0) return fail("dense_wgrad: empty problem");
  DenseWgradArgs a;
  a.dY = dY; a.X = X; a.dW = dW; a.db = db; a.B = B; a.F = F; a.Cin = Cin; a.ldy = F; a.ldx = Cin; a.ldw = Cin; a.alpha = alpha;
  launch_dense_wgrad(a, (hipStream_t)stream);
  return check_launch("dense_wgrad");
}

extern "C" int mn_op_head_wgrad(const float* dposes, const float* feat, float* dWx, float* dbx, float* dWq, float* dbq, int B, int K,
                                float scale, int filter_nans, void* stream) {
  begin_op();
  if (B <= 0 || K <= 0) return fail("head_wgrad: empty problem");
  launch_head_bwd_weight(dposes, feat, dWx, dbx, dWq, dbq, B, K, scale, filter_nans, (hipStream_t)stream);
  return check_launch("head_wgrad");
}

static int op_stem_bwd(const void* y, const unsigned char* idx, const void* gp, const float* gamma, const float* beta,
                       const float* mean, const float* invstd, const void* xpad, float* dW, int ldw, const int32_t* colmap,
                              float* dgamma, float* dbeta, float* coef_scratch, double* accum_scratch, int B, int H, int W, int Wp,
                              float alpha, int pre_gated, void* stream) {
  begin_op();
  if (Wp % 2 != 0 || Wp < W + 7) return fail("stem_bwd: Wp must be even and >= W + 7");
  hipStream_t s = (hipStream_t)stream;
  const int H0 = (H - 1) / 2 + 1, W0 = (W - 1) / 2 + 1;
  StemBwdArgs a;
  a.y = (const half*)y; a.idx = idx; a.gp = (const half*)gp; a.gamma = gamma; a.beta = beta; a.coef = coef_scratch; a.mean = mean;
  a.invstd = invstd; a.accum = accum_scratch; a.accum_rows = 1; a.xpad = (const half*)xpad; a.dW = dW; a.colmap = colmap;
  a.ldw = ldw; a.alpha = alpha;
  a.pre_gated = pre_gated;
  hipMemsetAsync(accum_scratch, 0, 2 * 64 * sizeof(double), s);
  launch_stem_bn_reduce(a, B, H, W, Wp, s);
  launch_bn_finalize_bwd(accum_scratch, (long)B * H0 * W0, gamma, mean, invstd, dgamma, dbeta, alpha, beta, coef_scratch, 64, 1, s);
  launch_stem_wgrad(a, B, H, W, Wp, s);
  return check_launch("stem_bwd");
}

extern "C" int mn_op_stem_bwd(const void* y, const unsigned char* idx, const void* gp, const float* gamma, const float* beta,
                              const float* mean, const float* invstd, const void* xpad, float* dW, int ldw, const int32_t* colmap,
                              float* dgamma, float* dbeta, float* coef_scratch, double* accum_scratch, int B, int H, int W, int Wp,
                              float alpha, void* stream) {
  return op_stem_bwd(y, idx, gp, gamma, beta, mean, invstd, xpad, dW, ldw, colmap, dgamma, dbeta, coef_scratch, accum_scratch, B, H,
                     W, Wp, alpha, 0, stream);
}
extern "C" int mn_op_stem_bwd_pregated(const void* y, const unsigned char* idx, const void* gp, const float* gamma, const float* beta,
                                       const float* mean, const float* invstd, const void* xpad, float* dW, int ldw,
                                       const int32_t* colmap, float* dgamma, float* dbeta, float* coef_scratch,
                                       double* accum_scratch, int B, int H, int W, int Wp, float alpha, void* stream) {
  return op_stem_bwd(y, idx, gp, gamma, beta, mean, invstd, xpad, dW, ldw, colmap, dgamma, dbeta, coef_scratch, accum_scratch, B, H,
                     W, Wp, alpha, 1, stream);
}

extern "C" int mn_op_oihw_to_ohwi(const float* src, float* dst, int O, int I, int H, int W, int to_ohwi, void* stream) {
  begin_op();
  launch_oihw_ohwi(src, dst, O, I, H, W, to_ohwi, (hipStream_t)stream);
  return check_launch("oihw_ohwi");
}

static_assert(kLossL1 == MN_LOSS_L1 && kLossMSE == MN_LOSS_MSE && kLossSmoothL1 == MN_LOSS_SMOOTH_L1 && kLossHuber == MN_LOSS_HUBER &&
                  kLossQuaternion == MN_LOSS_QUATERNION,
              "criterion.h's kinds are enum mn_loss_kind");

static int op_criterion(int mode, int N, int T, const float* pred, const float* targ, const float* s, float* loss, float* dpred,
                        float* ds, float* vos_out, float grad_scale, int t_kind, float t_param, int q_kind, float q_param,
                        void* stream) {
  if (T < 1 || T > kMaxT) return fail("criterion: T out of range");
  if (mode < 0 || mode > 3) return fail("criterion: bad mode");
  if (const char* why = loss_fn_error(t_kind, t_param, q_kind, q_param)) return fail(std::string("criterion: ") + why);
  CriterionArgs a;
  a.mode = mode; a.N = N; a.T = T; a.pred = pred; a.targ = targ; a.s = s; a.loss = loss; a.dpred = dpred; a.ds = ds;
  a.vos_out = vos_out; a.grad_scale = grad_scale;
  a.t_kind = t_kind; a.t_param = t_param; a.q_kind = q_kind; a.q_param = q_param;
  launch_criterion(a, (hipStream_t)stream);
  return check_launch("criterion");
}

extern "C" int mn_op_criterion(int mode, int N, int T, const float* pred, const float* targ, const float* s, float* loss,
                               float* dpred, float* ds, float* vos_out, float grad_scale, void* stream) {
  begin_op();
  return op_criterion(mode, N, T, pred, targ, s, loss, dpred, ds, vos_out, grad_scale, kLossL1, 0.f, kLossL1, 0.f, stream);
}

extern "C" int mn_op_criterion_fn(int mode, int N, int T, const float* pred, const float* targ, const float* s, float* loss,
                                  float* dpred, float* ds, float* vos_out, float grad_scale, int t_kind, float t_param,
                                  int q_kind, float q_param, void* stream) {
  begin_op();
  return op_criterion(mode, N, T, pred, targ, s, loss, dpred, ds, vos_out, grad_scale, t_kind, t_param, q_kind, q_param,
                      stream);
}

extern "C" int mn_op_calc_vos(const float* poses, int N, int T, float* vos, const float* cot, float* dposes,
                              void* stream) {
  begin_op();
  if (T < 2 || T > kMaxT) return fail("calc_vos: T out of range");
  launch_calc_vos(poses, N, T, vos, cot, dposes, (hipStream_t)stream);
  return check_launch("calc_vos");
}

extern "C" int mn_op_conv_dgrad(int dtype, int B, int Hin, int Win, int Cin, int Cout, int k, int stride, int pad,
                               const void* gy, const void* wd, void* gx, const void* res, const void* res_gate,
                               const void* out_gate, int parity, const void* zero_page, void* stream) {
  begin_op();
  if (stride != 1 && stride != 2) return fail("conv_dgrad: stride must be 1 or 2");
  if (k < 1 || k > 5 || pad < 0 || pad >= k) return fail("conv_dgrad: kernel / padding out of range");
  if (!zero_page) return fail("conv_dgrad: zero_page (>= 16 zero bytes of device memory) is required");
  const int Hout = (Hin + 2 * pad - k) / stride + 1, Wout = (Win + 2 * pad - k) / stride + 1;
  if (dtype < MN_DTYPE_F32 || dtype > MN_DTYPE_F16X2M)
    return fail("conv_dgrad: dtype must be MN_DTYPE_F32, _F16, _F32X3, _F16X2 or _F16X2M");
  const bool mixed = dtype == MN_DTYPE_F16X2M;  // the fp16 kernels with h2 gates (hi halves read)
  const int vec = dtype == MN_F16 || mixed ? 8 : 4;
  if (dtype == MN_DTYPE_F16X2 && (Cin % 32 != 0 || Cout % 32 != 0)) return fail("conv_dgrad: h2 operands need channel counts % 32 == 0");
  if (mixed && (res_gate || out_gate) && Cin % 32 != 0) return fail("conv_dgrad: h2 gates need Cin % 32 == 0");
  DgradGeom d = make_dgrad_geom(B, Hin, Win, Cin, Cout, k, stride, pad, Hout, Wout, vec);
  if (int e = check_geom(d.full, mixed ? MN_F16 : dtype)) return e;
  if (Cin % vec != 0) return fail("conv_dgrad: Cin must be a multiple of the 16-byte piece");
  Epilogue ep;
  ep.out = gx; ep.ldc = Cin; ep.res = res; ep.res_gate = res_gate; ep.out_gate = out_gate; ep.gate_h2 = mixed;
  if (dtype == MN_DTYPE_F32X3) {
    d.full.mma = MMA_BF16X3;
    for (int i = 0; i < d.n_pc; ++i) d.pc[i].g.mma = MMA_BF16X3;
  }
  if (dtype == MN_DTYPE_F16X2)  // gy, wd, res_gate, out_gate h2; gx, res fp32
    launch_conv_dgrad<half>(d, (const half*)gy, (const half*)wd, ep, (hipStream_t)stream, (const half*)zero_page, parity != 0, true);
  else if (dtype == MN_F16 || mixed)
    launch_conv_dgrad<half>(d, (const half*)gy, (const half*)wd, ep, (hipStream_t)stream, (const half*)zero_page, parity != 0);
  else
    launch_conv_dgrad<float>(d, (const float*)gy, (const float*)wd, ep, (hipStream_t)stream, (const float*)zero_page,
                             parity != 0);
  return check_launch("conv_dgrad");
}

extern "C" int mn_pgo_optimize(const double* poses, const double* vos, double* out, int32_t* status, int W, int N,
                               int fc_vos, double sax, double saq, double srx, double srq, int n_iters, void* stream) {
  begin_op();
  if (W <= 0) return fail("pgo: no windows");
  if (N < 2 || N > kPgoMaxN) return fail("pgo: 2 <= poses per window <= 12");
  if (!(sax > 0.0 && saq > 0.0 && srx > 0.0 && srq > 0.0)) return fail("pgo: covariances must be positive");
  if (n_iters < 0) return fail("pgo: n_iters < 0");
  if (!poses || !vos || !out || !status) return fail("pgo: null pointer");
  PgoArgs a;
  a.poses = poses; a.vos = vos; a.out = out; a.status = status; a.W = W; a.N = N; a.fc = fc_vos ? 1 : 0; a.n_iters = n_iters;
  a.w_ax = sqrt(1.0 / sax); a.w_aq = sqrt(1.0 / saq); a.w_rx = sqrt(1.0 / srx); a.w_rq = sqrt(1.0 / srq);
  launch_pgo(a, (hipStream_t)stream);
  return check_launch("pgo");
}

extern "C" int mn_seq_windows(const float* pose_table, const float* vo_table, const int32_t* win, int L, int W, int N, int fc_vos,
                              double* poses7, double* vos7, float* bad_flag, void* stream) {
  begin_op();
  SeqWinArgs a;
  a.pose_table = pose_table; a.vo_table = vo_table; a.win = win; a.L = L; a.W = W; a.N = N; a.fc = fc_vos ? 1 : 0;
  a.poses7 = poses7; a.vos7 = vos7; a.bad = bad_flag;
  const std::string err = seq_windows_error(a);
  if (!err.empty()) return fail("mn_seq_windows: " + err);
  if (bad_flag) hipMemsetAsync(bad_flag, 0, sizeof(float), (hipStream_t)stream);
  launch_seq_windows(a, (hipStream_t)stream);
  return check_launch("seq_windows");
}

extern "C" int mn_op_optim(int method, int nesterov, float* p, const float* g, float* m, float* v, int64_t n, int64_t n_clip,
                           float lr, float wd, float beta1, float beta2, float eps, int64_t step, float grad_mul, float max_norm,
                           double* sqnorm_scratch, int eps_mode, void* stream);
extern "C" int mn_op_adam(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_clip, float lr, float wd,
                          float beta1, float beta2, float eps, int64_t step, float grad_mul, float max_norm,
                          double* sqnorm_scratch, int eps_mode, void* stream) {
  return mn_op_optim(0, 0, p, g, m, v, n, n_clip, lr, wd, beta1, beta2, eps, step, grad_mul, max_norm, sqnorm_scratch, eps_mode,
                     stream);
}
extern "C" int mn_op_optim(int method, int nesterov, float* p, const float* g, float* m, float* v, int64_t n, int64_t n_clip,
                           float lr, float wd, float beta1, float beta2, float eps, int64_t step, float grad_mul, float max_norm,
                           double* sqnorm_scratch, int eps_mode, void* stream) {
  begin_op();
  if (method < 0 || method > 2) return fail("optim: method must be 0 (adam), 1 (sgd) or 2 (rmsprop)");
  hipStream_t s = (hipStream_t)stream;
  if (max_norm > 0.f) {
    if (!sqnorm_scratch) return fail("adam: clipping needs a scratch double");
    hipMemsetAsync(sqnorm_scratch, 0, sizeof(double), s);
    launch_grad_sqnorm(g, (long)n_clip, sqnorm_scratch, nullptr, s);
  }
  AdamArgs a;
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.n_clip = n_clip; a.lr = lr; a.wd = wd; a.beta1 = beta1; a.beta2 = beta2;
  a.eps = eps; a.bc1 = (float)(1.0 - pow((double)beta1, (double)step)); a.bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  a.grad_mul = grad_mul; a.max_norm = max_norm; a.sqnorm = sqnorm_scratch; a.frozen = nullptr; a.eps_mode = eps_mode;
  a.bc_dev = nullptr;
  a.method = method; a.nesterov = nesterov ? 1 : 0; a.first_step = step <= 1 ? 1 : 0;
  launch_adam(a, s);
  return check_launch("optim");
}

// standalone operator: statistics by a direct reduction (the network path takes them from the conv epilogue instead), then the
// finalize launch.  accum: [2][C] doubles + [2][C] floats of (scale, shift) after it; returns the coefficients.
template <typename T>
static const float* bn_stats_finalize(const void* y, int64_t M, int C, const float* gamma, const float* beta, float* running_mean,
                                      float* running_var, float* mean, float* invstd, float eps, float momentum, double* accum,
                                      hipStream_t s) {
  hipMemsetAsync(accum, 0, 2 * C * sizeof(double), s);
  launch_bn_fwd_stats<T>((const T*)y, (long)M, C, accum, s);
  BnParams p;
  p.gamma = gamma; p.beta = beta; p.running_mean = running_mean; p.running_var = running_var;
  p.num_batches_tracked = nullptr; p.mean = mean; p.invstd = invstd; p.eps = eps; p.momentum = momentum;
  float* coef = reinterpret_cast<float*>(accum + 2 * C);  // [2][C] floats behind the accumulators
  launch_bn_finalize_fwd(accum, (long)M, p, 1, coef, C, 1, s);
  return coef;
}

template <typename T>
static int bn_train_fwd_t(const void* y, int64_t M, int C, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float* mean, float* invstd, const void* res, int relu, void* out, float eps,
                          float momentum, double* accum, hipStream_t s) {
  const float* coef = bn_stats_finalize<T>(y, M, C, gamma, beta, running_mean, running_var, mean, invstd, eps, momentum, accum, s);
  launch_bn_apply<T>((const T*)y, coef, (const T*)res, (T*)out, (long)M, C, relu, s);
  return check_launch("bn_train_fwd");
}

// the apply kernels keep a thread's per-channel coefficients in registers: its channel piece must be the same in every
// grid-stride iteration, i.e. C / VEC pieces per row must be a power of two that divides the 256-thread workgroup
static int check_bn_channels(int dtype, int C) {
  const int vec = dtype == MN_F16 ? 8 : 4;
  const int cpr = C / vec;
  if (C <= 0 || C % vec != 0 || C > 512 || cpr > 256 || (cpr & (cpr - 1)) != 0)
    return fail("bn: C must be a power of two times the 16-byte piece (8 halves / 4 floats), at most 512");
  return 0;
}
// the h2 / record kernels (elementwise_h2.h): a thread owns 8 channels, rows hold whole 32-channel groups
static int check_bn_channels_h2(int C) {
  if (C < 32 || C > 512 || (C & (C - 1)) != 0) return fail("bn: the h2 / record kernels need C = 32, 64, 128, 256 or 512");
  return 0;
}

extern "C" int mn_op_bn_train_fwd(int dtype, const void* y, int64_t M, int C, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, float* mean, float* invstd, const void* res,
                                  int relu, void* out, float eps, float momentum, double* accum_scratch, void* stream) {
  begin_op();
  if (dtype != MN_F32 && dtype != MN_F16 && dtype != MN_DTYPE_F32X3)
    return fail("bn_train_fwd: dtype must be MN_DTYPE_F32 (or _F32X3: the same fp32 tensors) or MN_DTYPE_F16; the h2 form is "
                "mn_op_bn_train_fwd_h2");
  if (int e = check_bn_channels(dtype, C)) return e;
  if (dtype == MN_F16)
    return bn_train_fwd_t<half>(y, M, C, gamma, beta, running_mean, running_var, mean, invstd, res, relu, out, eps,
                                momentum, accum_scratch, (hipStream_t)stream);
  return bn_train_fwd_t<float>(y, M, C, gamma, beta, running_mean, running_var, mean, invstd, res, relu, out, eps,
                               momentum, accum_scratch, (hipStream_t)stream);
}

extern "C" int mn_op_bn_train_fwd_h2(const float* y, int64_t M, int C, const float* gamma, const float* beta, float* running_mean,
                                     float* running_var, float* mean, float* invstd, const void* res, int relu, void* out,
                                     void* rec, float eps, float momentum, double* accum_scratch, void* stream) {
  begin_op();
  if (int e = check_bn_channels_h2(C)) return e;
  if (M < 1 || !y || !gamma || !beta || !running_mean || !running_var || !out || !mean || !invstd || !accum_scratch)
    return fail("bn_train_fwd_h2: M >= 1 and every pointer but res and rec required");
  hipStream_t s = (hipStream_t)stream;
  const float* coef = bn_stats_finalize<float>(y, M, C, gamma, beta, running_mean, running_var, mean, invstd, eps, momentum,
                                               accum_scratch, s);
  launch_bn_apply_h2(y, coef, (const half*)res, (half*)out, (long)M, C, relu, 0, (half*)rec, mean, invstd, s);
  return check_launch("bn_train_fwd_h2");
}

template <typename T>
static int bn_bwd_t(const void* g, const void* gate, const void* y, int64_t M, int C, const float* gamma, const float* beta,
                    const float* mean, const float* invstd, float* dgamma, float* dbeta, void* gy, float* coef, double* accum,
                    int accum_rows, float grad_unscale, hipStream_t s) {
  launch_bn_bwd<T>((const T*)g, (const T*)gate, (const T*)y, (long)M, C, gamma, mean, invstd, dgamma, dbeta, (T*)gy, accum,
                   coef, grad_unscale, s, beta, PoolGradSrc(), accum_rows);
  return 0;
}

static int op_bn_bwd(int dtype, const void* g, const void* gate, const void* y, int64_t M, int C, const float* gamma,
                     const float* beta, const float* mean, const float* invstd, float* dgamma, float* dbeta, void* gy,
                     float* coef, double* accum, int accum_rows, float grad_unscale, void* stream) {
  begin_op();
  hipStream_t s = (hipStream_t)stream;
  const bool h2 = dtype == MN_DTYPE_F16X2, rec = dtype == MN_DTYPE_F16X2M;
  if (dtype != MN_F32 && dtype != MN_F16 && dtype != MN_DTYPE_F32X3 && !h2 && !rec)
    return fail("bn_bwd: dtype must be MN_DTYPE_F32 (or _F32X3: the same fp32 tensors), _F16, _F16X2 or _F16X2M");
  if (int e = (h2 || rec) ? check_bn_channels_h2(C) : check_bn_channels(dtype, C)) return e;
  if (accum_rows < 1 || accum_rows > 4096) return fail("bn_bwd: 1 <= accum_rows <= 4096");
  if (!coef) return fail("bn_bwd: coef_scratch (3*C floats, 4*C with a self gate) is required");
  if ((h2 || rec) && (M < 1 || !g || !y || !gy || !gamma || !mean || !invstd || !dgamma || !dbeta || !accum))
    return fail("bn_bwd: M >= 1 and every pointer but gate and beta required");
  if (h2 && gate) return fail("bn_bwd: MN_DTYPE_F16X2 takes the gradient as stored (already gated) or recomputes the unit's own ReLU (beta)");
  const long an = (long)accum_rows * 2 * C;
  hipMemsetAsync(accum, 0, an * sizeof(double), s);
  if (rec)  // g fp16, y = the 2-byte record of the forward apply; gate selects use_gate (the gate bits are the record's)
    launch_bn_bwd_rec((const half*)g, (const half*)y, (long)M, C, gamma, mean, invstd, dgamma, dbeta, (half*)gy, accum, coef,
                      grad_unscale, s, gate != nullptr, accum_rows);
  else if (h2)  // g, y fp32; gy h2; beta: the unit's own ReLU, recomputed from y
    launch_bn_bwd_h2((const float*)g, (const float*)y, (long)M, C, gamma, mean, invstd, dgamma, dbeta, (half*)gy, accum, coef,
                     grad_unscale, s, beta, accum_rows);
  else if (dtype == MN_F16)
    bn_bwd_t<half>(g, gate, y, M, C, gamma, beta, mean, invstd, dgamma, dbeta, gy, coef, accum, accum_rows, grad_unscale, s);
  else
    bn_bwd_t<float>(g, gate, y, M, C, gamma, beta, mean, invstd, dgamma, dbeta, gy, coef, accum, accum_rows, grad_unscale, s);
  hipMemsetAsync(accum, 0, an * sizeof(double), s);  // hand the scratch back zeroed
  return check_launch("bn_bwd");
}

extern "C" int mn_op_bn_bwd(int dtype, const void* g, const void* gate, const void* y, int64_t M, int C, const float* gamma,
                            const float* mean, const float* invstd, float* dgamma, float* dbeta, void* gy,
                            float* coef_scratch, double* accum_scratch, float grad_unscale, void* stream) {
  return op_bn_bwd(dtype, g, gate, y, M, C, gamma, nullptr, mean, invstd, dgamma, dbeta, gy, coef_scratch, accum_scratch, 1,
                   grad_unscale, stream);
}
extern "C" int mn_op_bn_bwd_rows(int dtype, const void* g, const void* gate, const void* y, int64_t M, int C, const float* gamma,
                                 const float* beta, const float* mean, const float* invstd, float* dgamma, float* dbeta, void* gy,
                                 float* coef_scratch, double* accum_scratch, int accum_rows, float grad_unscale, void* stream) {
  return op_bn_bwd(dtype, g, gate, y, M, C, gamma, beta, mean, invstd, dgamma, dbeta, gy, coef_scratch, accum_scratch, accum_rows,
                   grad_unscale, stream);
}

extern "C" int mn_op_bn_relu_maxpool_h2(const float* y, const float* coef, void* out, unsigned char* idx, void* y16, int B, int H,
                                        int W, int C, void* stream) {
  begin_op();
  if (int e = check_bn_channels_h2(C)) return e;
  if (B < 1 || H < 1 || W < 1 || !y || !coef || !out) return fail("bn_relu_maxpool_h2: B, H, W >= 1, y, coef and out required");
  launch_bn_relu_maxpool_h2(y, coef, (half*)out, idx, B, H, W, C, (half*)y16, 0, (hipStream_t)stream);
  return check_launch("bn_relu_maxpool_h2");
}

extern "C" int mn_op_avgpool_fwd_h2(const void* in, float* out, int B, int HW, int C, void* stream) {
  begin_op();
  if (B < 1 || HW < 1 || C < 32 || C % 32 != 0 || !in || !out) return fail("avgpool_fwd_h2: B, HW >= 1, C a multiple of 32, in and out required");
  launch_avgpool_fwd_h2((const half*)in, out, B, HW, C, 0, (hipStream_t)stream);
  return check_launch("avgpool_fwd_h2");
}

extern "C" int mn_op_avgpool_bwd(int dtype, const float* gp, void* g, const void* gate, int B, int HW, int C, void* stream) {
  begin_op();
  if (dtype != MN_DTYPE_F16X2 && dtype != MN_DTYPE_F16X2M)
    return fail("avgpool_bwd: dtype must be MN_DTYPE_F16X2 (fp32 gradient) or MN_DTYPE_F16X2M (fp16 gradient); the gate is an h2 tensor");
  if (B < 1 || HW < 1 || C < 32 || C % 32 != 0 || !gp || !g) return fail("avgpool_bwd: B, HW >= 1, C a multiple of 32, gp and g required");
  if (dtype == MN_DTYPE_F16X2M)
    launch_avgpool_bwd<half>(gp, (half*)g, B, HW, C, (const half*)gate, 1, (hipStream_t)stream);
  else
    launch_avgpool_bwd_h2(gp, (float*)g, B, HW, C, (const half*)gate, (hipStream_t)stream);
  return check_launch("avgpool_bwd");
}

extern "C" int mn_op_widen_f16(const void* in, float* out, int64_t n, void* stream) {
  begin_op();
  if (n < 8 || n % 8 != 0 || !in || !out) return fail("widen_f16: n a positive multiple of 8, in and out required");
  launch_widen_f16((const half*)in, out, (long)n, (hipStream_t)stream);
  return check_launch("widen_f16");
}

extern "C" int mn_op_maxpool_fwd(int dtype, const void* in, void* out, unsigned char* idx, int B, int H, int W, int C,
                                 void* stream) {
  begin_op();
  if (dtype == MN_F16)
    launch_maxpool_fwd<half>((const half*)in, (half*)out, idx, B, H, W, C, (hipStream_t)stream);
  else
    launch_maxpool_fwd<float>((const float*)in, (float*)out, idx, B, H, W, C, (hipStream_t)stream);
  return check_launch("maxpool_fwd");
}

extern "C" int mn_op_maxpool_bwd(int dtype, const unsigned char* idx, const void* gout, void* gin, int B, int H, int W,
                                 int C, void* stream) {
  begin_op();
  if (dtype == MN_F16)
    launch_maxpool_bwd<half>(idx, (const half*)gout, (half*)gin, B, H, W, C, (hipStream_t)stream);
  else
    launch_maxpool_bwd<float>(idx, (const float*)gout, (float*)gin, B, H, W, C, (hipStream_t)stream);
  return check_launch("maxpool_bwd");
}

extern "C" int mn_op_occupy(int workgroups, int threads, float microseconds, const void* src, void* dst, int64_t bytes, int lds_kb,
                            void* stream) {
  begin_op();
  if (workgroups < 1 || workgroups > 4096 || threads < 64 || threads > 1024 || threads % 64 != 0)
    return fail("mn_op_occupy: 1..4096 workgroups of 64..1024 threads (a multiple of 64)");
  if (!(microseconds >= 0.f) || microseconds > 1e6f) return fail("mn_op_occupy: 0 <= microseconds <= 1e6");
  if (bytes < 0 || (bytes > 0 && (!src || !dst))) return fail("mn_op_occupy: bytes > 0 needs src and dst");
  if (lds_kb != 0 && lds_kb != 32 && lds_kb != 64) return fail("mn_op_occupy: lds_kb must be 0, 32 or 64");
  launch_occupy(workgroups, threads, microseconds, src, dst, (long)bytes, lds_kb, (hipStream_t)stream);
  return check_launch("occupy");
}

extern "C" int mn_op_color_jitter(const unsigned char* in, float* out, float* draws, float* work, int B, int H, int W,
                                  const float* ranges, uint64_t seed, uint32_t call, const float* mean, const float* std,
                                  void* stream) {
  begin_op();
  if (B < 1 || H < 1 || W < 1 || !in || !out || !draws || !work || !ranges || !mean || !std)
    return fail("mn_op_color_jitter: B, H, W >= 1 and every pointer required");
  InputNorm nm;
  for (int c = 0; c < 3; ++c) {
    if (!(std[c] > 0.f)) return fail("mn_op_color_jitter: std must be positive");
    nm.scale[c] = 1.f / std[c];
    nm.shift[c] = -mean[c] / std[c];
  }
  launch_u8_jitter<float>(in, out, B, H, W, H + 6, W + 6, nm, nullptr, jitter_params(ranges, seed, call), draws, work,
                          work + (long)B * kJitterChunks, (hipStream_t)stream);
  return check_launch("color_jitter");
}

// The tables of one mn_op_resize_u8 call travel through a pinned buffer of the calling thread (kept for the thread's life), so
// that the upload is ordered on the caller's stream like the kernel behind it; the next call waits for the previous upload only.
namespace {
struct ResizeStage {
  int* host = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool pending = false;
};
thread_local ResizeStage g_resize_stage;
}  // namespace

extern "C" int64_t mn_op_resize_work_bytes(int src_h, int src_w, int H, int W) {
  if (src_h < 1 || src_w < 1 || H < 1 || W < 1) {
    fail("mn_op_resize_work_bytes: source and output sizes must be positive");
    return -1;
  }
  return resize_table_bytes(src_h, src_w, H, W);
}

extern "C" int mn_op_resize_tile(int src_h, int src_w, int H, int W, int* tile_h, int* tile_w) {
  if (!tile_h || !tile_w) return fail("mn_op_resize_tile: tile_h and tile_w are required");
  const ResizePlan rp = resize_plan(1, src_h, src_w, H, W, nullptr);
  if (!rp.error.empty()) return fail("mn_op_resize_tile: " + rp.error);
  *tile_h = rp.g.th;
  *tile_w = rp.g.tw;
  return 0;
}

// both resize entries: index null = the plain operator
static int op_resize_u8(const char* name, const unsigned char* in, const int32_t* index, int64_t store_frames, unsigned char* out,
                        void* work, int B, int src_h, int src_w, int H, int W, float* bad_flag, void* stream) {
  const std::string who(name);
  if (!in || !out || !work) return fail(who + ": in, out and work are required");
  if (((uintptr_t)work & 3) != 0) return fail(who + ": work must be 4-byte aligned");
  const ResizePlan rp = resize_plan(B, src_h, src_w, H, W, (int*)work);
  if (!rp.error.empty()) return fail(who + ": " + rp.error);
  ResizeStage& st = g_resize_stage;
  const size_t bytes = rp.tables.size() * sizeof(int);
  if (!st.ev && hipEventCreateWithFlags(&st.ev, hipEventDisableTiming) != hipSuccess) return check_launch("resize_u8 (event)");
  if (st.pending) {
    (void)hipEventSynchronize(st.ev);
    st.pending = false;
  }
  if (st.cap < bytes) {
    if (st.host) (void)hipHostFree(st.host);
    st.host = nullptr;
    st.cap = 0;
    if (hipHostMalloc((void**)&st.host, bytes, 0) != hipSuccess) return check_launch("resize_u8 (pinned tables)");
    st.cap = bytes;
  }
  memcpy(st.host, rp.tables.data(), bytes);
  hipMemcpyAsync(work, st.host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
  hipEventRecord(st.ev, (hipStream_t)stream);
  st.pending = true;
  if (index && bad_flag) hipMemsetAsync(bad_flag, 0, sizeof(float), (hipStream_t)stream);
  launch_resize_u8(in, out, rp.g, (hipStream_t)stream, index, (long)store_frames, bad_flag);
  return check_launch("resize_u8");
}

extern "C" int mn_op_resize_u8(const unsigned char* in, unsigned char* out, void* work, int B, int src_h, int src_w, int H, int W,
                               void* stream) {
  begin_op();
  return op_resize_u8("mn_op_resize_u8", in, nullptr, 0, out, work, B, src_h, src_w, H, W, nullptr, stream);
}

extern "C" int mn_op_resize_u8_indexed(const unsigned char* store, const int32_t* index, int64_t store_frames, unsigned char* out,
                                       void* work, int B, int src_h, int src_w, int H, int W, float* bad_flag, void* stream) {
  begin_op();
  if (!index || ((uintptr_t)index & 3) != 0) return fail("mn_op_resize_u8_indexed: index (device int32 [B], 4-byte aligned) is required");
  if (store_frames < 1) return fail("mn_op_resize_u8_indexed: store_frames must be at least 1");
  return op_resize_u8("mn_op_resize_u8_indexed", store, index, store_frames, out, work, B, src_h, src_w, H, W, bad_flag, stream);
}

extern "C" int mn_op_gather_frames(const void* store, const int32_t* index, void* out, int64_t frame_bytes, int images,
                                   int64_t store_frames, float* bad_flag, void* stream) {
  begin_op();
  if (!store || !out) return fail("mn_op_gather_frames: store and out are required");
  if (!index || ((uintptr_t)index & 3) != 0) return fail("mn_op_gather_frames: index (device int32 [images], 4-byte aligned) is required");
  const std::string err = gather_frames_error((long)frame_bytes, images, (long)store_frames);
  if (!err.empty()) return fail("mn_op_gather_frames: " + err);
  if (bad_flag) hipMemsetAsync(bad_flag, 0, sizeof(float), (hipStream_t)stream);
  launch_gather_frames(store, index, out, (long)frame_bytes, images, (long)store_frames, bad_flag, (hipStream_t)stream);
  return check_launch("gather_frames");
}

extern "C" int64_t mn_op_frame_stats_work_bytes(int images, int H, int W, int blocks) {
  if (images < 1 || H < 1 || W < 1 || blocks < 0) {
    fail("mn_op_frame_stats_work_bytes: images, H and W must be positive and blocks >= 0");
    return -1;
  }
  return frame_stats_blocks(images, (long)H * W * 3, blocks, device_cus()) * 6 * (int64_t)sizeof(u64);
}

extern "C" int mn_op_frame_stats_u8(const unsigned char* frames, const int32_t* index, int64_t store_frames, int images, int H, int W,
                                    uint64_t* sums, int accumulate, int blocks, void* work, float* bad_flag, void* stream) {
  begin_op();
  if (!frames || !sums || !work) return fail("mn_op_frame_stats_u8: frames, sums and work are required");
  if (((uintptr_t)sums & 7) != 0 || ((uintptr_t)work & 7) != 0)
    return fail("mn_op_frame_stats_u8: sums (device uint64 [6]) and work must be 8-byte aligned");
  if (index && ((uintptr_t)index & 3) != 0) return fail("mn_op_frame_stats_u8: index (device int32 [images]) must be 4-byte aligned");
  if (images < 1 || H < 1 || W < 1) return fail("mn_op_frame_stats_u8: images, H and W must be positive");
  if (index && store_frames < 1) return fail("mn_op_frame_stats_u8: store_frames must be at least 1 with an index");
  if (blocks < 0) return fail("mn_op_frame_stats_u8: blocks must be >= 0 (0: the default grid)");
  const long L = (long)H * W * 3;
  const long nb = frame_stats_blocks(images, L, blocks, device_cus());
  if (index && bad_flag) hipMemsetAsync(bad_flag, 0, sizeof(float), (hipStream_t)stream);
  launch_frame_stats(frames, index, (long)store_frames, images, L, (u64*)sums, accumulate != 0, nb, (u64*)work, bad_flag,
                     (hipStream_t)stream);
  return check_launch("frame_stats_u8");
}

extern "C" int mn_op_stem_dgrad(int dtype, const void* gy, const void* w, float* gx, int B, int H, int W, float alpha, void* stream) {
  begin_op();
  if (dtype != MN_F32 && dtype != MN_F16) return fail("mn_op_stem_dgrad: dtype must be MN_DTYPE_F32 or MN_DTYPE_F16");
  if (B < 1 || H < 1 || W < 1 || !gy || !w || !gx) return fail("mn_op_stem_dgrad: B, H, W >= 1 and every pointer required");
  if ((long)B * H * cdiv(W, kSdTile) >= (1L << 31) - 4096) return fail("mn_op_stem_dgrad: too many output tiles; split the batch");
  if (dtype == MN_F16)
    launch_stem_dgrad<half>((const half*)gy, (const float*)w, gx, B, H, W, alpha, nullptr, (hipStream_t)stream);
  else
    launch_stem_dgrad<float>((const float*)gy, (const float*)w, gx, B, H, W, alpha, nullptr, (hipStream_t)stream);
  return check_launch("stem_dgrad");
}

extern "C" int mn_op_bn_eval_bwd(int dtype, const void* g, const void* gate, const float* scale, void* gy, int64_t M, int C,
                                 void* stream) {
  begin_op();
  if (dtype != MN_F32 && dtype != MN_F16) return fail("mn_op_bn_eval_bwd: dtype must be MN_DTYPE_F32 or MN_DTYPE_F16");
  const int vec = dtype == MN_F16 ? 8 : 4;
  if (M < 1 || C < vec || C % vec != 0 || !g || !scale || !gy)
    return fail("mn_op_bn_eval_bwd: M >= 1, C a multiple of the 16-byte piece (8 halves / 4 floats), g, scale and gy required");
  if (dtype == MN_F16)
    launch_bn_eval_bwd<half>((const half*)g, (const half*)gate, scale, nullptr, (half*)gy, (long)M, C, (hipStream_t)stream);
  else
    launch_bn_eval_bwd<float>((const float*)g, (const float*)gate, scale, nullptr, (float*)gy, (long)M, C, (hipStream_t)stream);
  return check_launch("bn_eval_bwd");
}

extern "C" int mn_op_saliency(const float* gx, const float* x, float* out, float* work, int B, int H, int W, void* stream) {
  begin_op();
  if (B < 1 || B > 65535 || H < 1 || W < 1 || !gx || !x || !out || !work)
    return fail("mn_op_saliency: 1 <= B <= 65535, H, W >= 1 and every pointer required");
  InputNorm nm{{1.f, 1.f, 1.f}, {0.f, 0.f, 0.f}};
  launch_saliency(gx, x, nullptr, nm, out, work, B, H, W, (hipStream_t)stream);
  return check_launch("saliency");
}
extern "C" int64_t mn_op_saliency_work_floats(int B) { return (int64_t)B * kSalChunks * 2; }
