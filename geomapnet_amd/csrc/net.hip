// MapNet / PoseNet training plan: the host-side schedule of one training step
// (/root/reference/common/train.py:322-363) as a fixed sequence of gfx950 kernel launches on
// caller-provided arenas.  See include/mapnet_hip.h for the ABI and DESIGN.md for the layout.
#include "../../include/mapnet_hip.h"

#include <cmath>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "criterion.h"
#include "elementwise.h"
#include "elementwise_h2.h"
#include "head.h"
#include "gather.h"
#include "jitter.h"
#include "resize.h"
#include "knobs.h"
#include "dense.h"
#include "igemm.h"
#include "dgrad.h"
#include "halo_pp.h"
#include "input_grad.h"
#include "layout.h"
#include "optim.h"
#include "pool.h"
#include "stem.h"
#include "stem_bwd.h"
#include "util.h"
#include "wgrad.h"

using namespace mn;

// ---- model layout entry points ------------------------------------------------------------------
static const Layout& layout_for(int feat_dim) {
  static thread_local std::unique_ptr<Layout> cache;
  if (!cache || cache->feat_dim != feat_dim) cache.reset(new Layout(feat_dim));
  return *cache;
}
extern "C" int mn_model_entries(int feat_dim) { return (int)layout_for(feat_dim).entries.size(); }
extern "C" int mn_model_entry(int feat_dim, int idx, mn_entry* out) {
  const Layout& L = layout_for(feat_dim);
  if (idx < 0 || idx >= (int)L.entries.size()) return fail("mn_model_entry: index out of range");
  *out = L.entries[idx];
  return 0;
}
extern "C" int64_t mn_model_param_floats(int feat_dim) { return layout_for(feat_dim).param_floats; }
extern "C" int64_t mn_model_buffer_bytes(int feat_dim) { return layout_for(feat_dim).buffer_bytes; }

// images per window: PoseNet 1, MapNet T, the online modes 2 T
static int frames_per_window(int mode, int T) { return mode == MN_MODE_POSENET ? 1 : (mode == MN_MODE_MAPNET ? T : 2 * T); }

namespace {

struct Bump {
  size_t cur = 0;
  size_t take(size_t bytes) {
    size_t o = cur;
    cur += (bytes + 255) & ~(size_t)255;
    return o;
  }
};

// event-pair timer for kernel classes (igemm, wgrad, whole step)
struct KernelTimer {
  bool enabled = false;
  struct Pair {
    hipEvent_t a, b;
    int cat;
  };
  std::deque<Pair> pool;  // stable addresses: callers hold Pair* across later begin() calls
  size_t used = 0;
  float ms[4] = {0, 0, 0, 0};
  int launches[4] = {0, 0, 0, 0};
  Pair* begin(int cat, hipStream_t s) {
    if (!enabled) return nullptr;
    if (used == pool.size()) {
      Pair p;
      hipEventCreate(&p.a);
      hipEventCreate(&p.b);
      pool.push_back(p);
    }
    Pair* p = &pool[used++];
    p->cat = cat;
    hipEventRecord(p->a, s);
    return p;
  }
  void end(Pair* p, hipStream_t s) {
    if (p) hipEventRecord(p->b, s);
  }
  void reset() { used = 0; }
  void collect() {  // caller has synchronised the stream
    for (int i = 0; i < 4; ++i) {
      ms[i] = 0;
      launches[i] = 0;
    }
    for (size_t i = 0; i < used; ++i) {
      float t = 0;
      hipEventSynchronize(pool[i].b);
      hipEventElapsedTime(&t, pool[i].a, pool[i].b);
      ms[pool[i].cat] += t;
      launches[pool[i].cat]++;
    }
  }
  ~KernelTimer() {
    for (auto& p : pool) {
      hipEventDestroy(p.a);
      hipEventDestroy(p.b);
    }
  }
};

struct PlanBase {
  virtual ~PlanBase() {
    for (hipEvent_t e : fork_events) hipEventDestroy(e);
    if (overflow_host) hipHostFree(overflow_host);
  }
  // (one process-wide side stream per device, never destroyed: plans come and go, the stream is reused)
  static hipStream_t shared_side_stream() {
    static hipStream_t streams[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    // (a side stream of lower or higher priority was measured: no gain.  A side stream restricted to n of the chip's CUs
    //  (hipExtStreamCreateWithCUMask), so that weight-gradient workgroups cannot take every CU away from the main stream's
    //  BatchNorm / data-gradient launches: measured and removed, profiles/r05 (cu mask))
    if (!streams[dev] && hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking) != hipSuccess) {
      streams[dev] = nullptr;
      (void)hipGetLastError();
    }
    return streams[dev];
  }
  // Weight-gradient launches do not feed the data-gradient chain, so they run on a second stream: their
  // workgroups fill the CUs the tail of each data-gradient launch leaves idle (layers 3-4 at B = 192 have
  // 1056 / 528 tiles for 512 resident slots).  fork: wstream waits for everything enqueued on s so far;
  // join: s waits for wstream.
  hipStream_t wstream = nullptr;
  std::vector<hipEvent_t> fork_events;
  size_t fork_next = 0;
  bool wgrad_pending = false;
  bool overlap_wgrad = knobs().wgrad_stream;
  hipEvent_t next_fork_event() {
    if (fork_events.size() < 64) {
      hipEvent_t e = nullptr;
      hipEventCreateWithFlags(&e, hipEventDisableTiming);
      fork_events.push_back(e);
      return e;
    }
    return fork_events[fork_next++ % fork_events.size()];
  }
  hipStream_t fork_wgrad(hipStream_t s) {
    if (!overlap_wgrad || s == nullptr || timer.enabled) return s;
    if (!wstream && !(wstream = shared_side_stream())) {
      overlap_wgrad = false;
      return s;
    }
    hipEvent_t e = next_fork_event();
    hipEventRecord(e, s);
    hipStreamWaitEvent(wstream, e, 0);
    wgrad_pending = true;
    if (head_wgrads_deferred) launch_head_wgrads(wstream);  // (head_backward: the first fork of the backward pass takes them along)
    return wstream;
  }
  bool head_wgrads_deferred = false;
  virtual void launch_head_wgrads(hipStream_t st) = 0;
  void join_wgrad(hipStream_t s) {
    if (!wgrad_pending) return;
    hipEvent_t e = next_fork_event();
    hipEventRecord(e, wstream);
    hipStreamWaitEvent(s, e, 0);
    wgrad_pending = false;
  }
  // Early loss read-back: the reference blocks on loss.item() (common/train.py:361) after the whole step; the value
  // exists as soon as the criterion has run, so it is copied to the caller's pinned host float right there and the
  // caller waits for THAT event only -- the host prepares the next step while backward and the optimiser still run.
  float* loss_host = nullptr;
  hipEvent_t loss_event = nullptr;
  bool loss_pending = false;
  void post_loss(const float* loss_dev_ptr, hipStream_t s) {
    if (!loss_host || s == nullptr) return;
    if (!loss_event && hipEventCreateWithFlags(&loss_event, hipEventDisableTiming) != hipSuccess) {
      loss_event = nullptr;
      (void)hipGetLastError();
      return;
    }
    hipMemcpyAsync(loss_host, loss_dev_ptr, sizeof(float), hipMemcpyDeviceToHost, s);
    hipEventRecord(loss_event, s);
    loss_pending = true;
  }
  // The step is enqueued DIRECTLY (~250 launches on two streams; the host needs ~1.5 ms per step and stays a full step
  // ahead of the device).  Capturing it into a hipGraph and replaying it was implemented and measured in rounds 1-2 and
  // removed in round 3: on ROCm 7.2 the replay was 2 % SLOWER than direct launches (19.57 vs 19.17 ms), forked branches
  // overlapped less inside a graph (early weight-gradient forks: +0.3 % in a graph, -2.4 % eager), and destroying a graph
  // exec that contains a fork/join crashed later graph launches in hip::Graph::UpdateStreams.
  virtual void after_optim_host() = 0;
  virtual int sync_step_to_device(hipStream_t s) = 0;
  virtual int64_t applied_steps() = 0;  // the device's count of optimiser steps that were applied (waits for the device)
  virtual size_t carve(char* base) = 0;  // lay the work arena out from `base` (null: only measure it); returns its bytes
  virtual int attach(float* params, float* opt_state, void* buffers, void* work, hipStream_t s) = 0;
  virtual void update_frozen(hipStream_t s) = 0;
  virtual int forward(const void* images, float* poses_out, int training, hipStream_t s) = 0;
  // dropout between the feature vector's ReLU and the pose heads (mn_set_dropout): probability, Philox key, calls so far
  float drop_p = 0.f;
  unsigned long long drop_seed = 0;
  unsigned drop_calls = 0;
  bool drop_this_step = false;  // the forward pass of the step being built applied a mask (the backward pass must, too)
  bool input_u8 = false;  // images are uint8 NHWC, normalised on the device (mn_set_input_u8)
  InputNorm input_norm{{1.f, 1.f, 1.f}, {0.f, 0.f, 0.f}};
  InputNorm jitter_norm{{1.f, 1.f, 1.f}, {0.f, 0.f, 0.f}};  // the same Normalize on x in [0, 1]: scale 1/std, shift -mean/std
  // ColorJitter on uint8 input (mn_set_color_jitter): ranges (brightness, contrast, saturation, hue), Philox key, jittered passes
  // so far; all ranges 0 = off, and the forward pass launches exactly what it launches without jitter
  float jit_range[4] = {0.f, 0.f, 0.f, 0.f};
  unsigned long long jit_seed = 0;
  unsigned jit_calls = 0;
  bool jitter_on() const { return jit_range[0] > 0.f || jit_range[1] > 0.f || jit_range[2] > 0.f || jit_range[3] > 0.f; }
  // Resize on uint8 input (mn_set_input_resize): `images` are source frames, resampled into the caller's buffer rs_frames at the
  // head of a pass; everything downstream reads rs_frames where it read `images`.  Off: nothing is launched for it
  bool resize_on = false;
  ResizeGeom rs_geom;
  unsigned char* rs_frames = nullptr;
  // Frames gathered from a device-resident store (mn_set_input_index): `images` is the store's base and image b of the batch is
  // frame in_index[b] of it -- read by the indexed resample where the resize is on, else gathered into the caller's buffer in_stage
  // at the head of a pass; everything downstream reads the gathered batch where it read `images`.  Off (null): nothing is launched
  const int32_t* in_index = nullptr;
  int64_t in_store_frames = 0;
  unsigned char* in_stage = nullptr;
  int64_t in_stage_bytes = 0;
  // Fused inference pass (mn_set_eval_fused): a training == 0 forward pass of an h2 plan finishes BatchNorm, residual and ReLU in
  // the epilogues of its convolutions.  Off: every pass launches exactly what it launched before the switch existed
  bool eval_fused = false;
  virtual std::string eval_fused_refusal() const = 0;  // empty: this plan can run the fused pass; else why mn_set_eval_fused fails
  virtual int input_grad(const void* images, const float* cot, float* gx_out, float* sal_out, float* poses_out, hipStream_t s) = 0;
  virtual int loss_only(const float* pred, const float* targ, float* loss_out, hipStream_t s) = 0;
  virtual int forward_loss(const void* images, const float* targets, float* loss_out, float* poses_out,
                           hipStream_t s) = 0;
  virtual int backward_stage(int stage, hipStream_t s) = 0;
  virtual int optim_step(float grad_mul, hipStream_t s) = 0;
  virtual int debug_tensor(const char* name, void** ptr, int64_t* numel, int32_t* dtype) = 0;
  virtual float* grad_arena() = 0;
  mn_config cfg;
  // fp16 loss scaling.  cur_scale multiplies d(pred) and is divided out where gradients enter the fp32 arena.  An
  // overflowed step is skipped on the device (optim.h, adam_prep_kernel); the count of skipped steps is copied to a
  // pinned host word after every optimiser step and read -- without waiting -- when the next step is enqueued: each
  // newly seen skip halves the scale, `scale_growth_interval` clean steps double it (0 = never grow).  The host reacts
  // one or two steps late; until then the device keeps skipping, so no non-finite value reaches weights or moments.
  float cur_scale = 1.f;
  bool scales_loss = false;  // gradients pass through fp16 (Plan: Mode::overflow_guard); other plans keep the scale at 1
  long long* overflow_host = nullptr;  // (only plans that guard against overflow allocate it) pinned: {last step skipped, skipped steps in total, last skipped attempt, last COMPLETED attempt}
  long long skipped_seen = 0;
  long long done_seen = 0;        // last completed attempt the host has accounted for (overflow_host[3])
  int64_t attempts = 0;           // optimiser steps enqueued on this plan (skipped ones included)
  int64_t scale_set_at = 0;       // `attempts` when the loss scale last changed: later attempts ran under cur_scale
  int64_t stuck_skips = 0;        // CONSECUTIVE skips seen while the scale already was 1 (nothing left to lower); an APPLIED
                                  // step, a scale growth or mn_set_loss_scale resets it
  long long clean_steps = 0;      // applied steps since the last skip the host has seen
  int scale_growth_interval = knobs().scale_growth;
  // The host reads the pinned words WITHOUT waiting for the device, so a poll that sees no new skip proves nothing by itself: the
  // host may simply be ahead (C-API callers that never read the loss, DataLoader jitter).  Progress is only what the device reports:
  // overflow_host[3], the index of the last attempt it completed.  (Round-4 ADVICE: the previous form reset `stuck_skips` and
  // advanced `clean_steps` on every poll without a new skip, so a run with permanently non-finite inputs whose polls interleave
  // with "nothing finished yet" could reset the counter forever and silently train nothing, and the loss scale grew on polls
  // that observed nothing.)
  void poll_overflow() {
    if (!overflow_host) return;
    const long long done = *(volatile long long*)(overflow_host + 3);   // read first: a copy landing in between can only make
    const long long seen = *(volatile long long*)(overflow_host + 1);   // `seen` newer than `done` (fewer clean steps counted)
    const long long last_bad = *(volatile long long*)(overflow_host + 2);
    const long long new_skips = seen > skipped_seen ? seen - skipped_seen : 0;
    const long long new_done = done > done_seen ? done - done_seen : 0;
    if (new_skips > 0) {
      // The host reads the count one or two steps late, and the steps enqueued meanwhile overflow under the OLD scale too:
      // a burst is ONE overflow event.  Halve once per burst -- i.e. only when a skipped step was enqueued after the
      // scale last changed.
      if (last_bad > scale_set_at) {
        if (cur_scale > 1.f) {
          cur_scale *= 0.5f;
          scale_set_at = attempts;
        } else {
          stuck_skips += new_skips;  // non-finite values that no loss scale can fix (inputs, forward pass)
        }
      }
      skipped_seen = seen;
      clean_steps = 0;
    }
    if (new_done > 0) {
      done_seen = done;
      // positive evidence of an applied step: the most recent completed attempt was not a skipped one
      if (last_bad < done) stuck_skips = 0;
      if (new_skips == 0) {
        clean_steps += new_done;
        if (scale_growth_interval > 0 && clean_steps >= scale_growth_interval) {
          clean_steps = 0;
          if (cur_scale < 65536.f) {
            cur_scale *= 2.f;
            scale_set_at = attempts;
          }
        }
      }
    }
  }
  Layout L{2048};
  float lr = 1e-4f, wd = 0.f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f, max_grad_norm = 0.f;
  int optim_method = 0, nesterov = 0;  // optim.h AdamArgs::method; beta1 / beta2 carry momentum / dampening | alpha
  int64_t step = 0;
  bool weights_dirty = true;
  int learn_beta = 0, learn_gamma = 0;
  // t_loss_fn / q_loss_fn of the criterion (mn_set_loss_fn; enum mn_loss_kind) and SmoothL1's beta / Huber's delta
  int t_kind = MN_LOSS_L1, q_kind = MN_LOSS_L1;
  float t_param = 0.f, q_param = 0.f;
  KernelTimer timer;
};

template <typename T>
struct Plan : PlanBase {
  static constexpr int VEC = ElemTraits<T>::VEC;
  static constexpr int DT = ElemTraits<T>::DTYPE;

  // ---- the mode ---------------------------------------------------------------------------------
  // What cfg.dtype (and MN_DETERMINISTIC) means for this plan, stated once: mode_of() fills it, carve, the launch helpers and
  // debug_tensor read it, and nothing else asks for the dtype.  A format is the MN_DTYPE_* code mn_debug_tensor reports.  The
  // arena is carved in elements of T whatever the format: an h2 / h2q element takes 4 bytes like fp32, and the plain fp16 tensors of
  // the fp16x2m backward pass sit in the buffers carved for fp32 -- the T* members below hold what `md` says, and the launches cast.
  static constexpr int FMT_F32 = MN_DTYPE_F32, FMT_F16 = MN_DTYPE_F16, FMT_H2 = MN_DTYPE_F16X2, FMT_H2Q = MN_DTYPE_F16X2Q;
  // the stem's backward pass: the two tile-walking fp16 kernels of stem_bwd.h on the stem's own tensors (fp16), the same kernels on
  // fp16 COPIES of the fp32 conv output and of the padded input (fp16x2m), or the chain BatchNorm backward -> weight gradient
  enum StemBwd { STEM_TILES, STEM_TILES_ON_COPIES, STEM_CHAIN };
  struct Mode {
    int act;     // activations a convolution consumes: block inputs / outputs, a1, the projection output, the pooled stem output
    int y;       // raw conv outputs (and everything of the stem but its pooled output): always T
    int gy;      // d(conv output)
    int gx;      // data gradients: ga1, gout, gp0
    int wf, wd;  // forward / data-gradient weight copies (wf = FMT_F32: no copy, the OHWI master is the operand)
    int mma_fwd, mma_bwd;  // contraction of the kernels that read fp32 tensors (common.h MMA_*)
    StemBwd stem_bwd;
    bool overflow_guard;  // gradients pass through fp16: scale the loss, skip overflowed steps (PlanBase::poll_overflow)
    bool pairs() const { return act == FMT_H2 || act == FMT_H2Q; }    // the h2 forward pass
    bool f16_bwd_on_pairs() const { return pairs() && gy == FMT_F16; }  // ... with the fp16 mode's backward kernels behind it
  };
  static Mode mode_of(int dtype, bool deterministic) {
    Mode m;
    m.act = m.y = m.gy = m.gx = m.wf = m.wd = DT;  // MN_DTYPE_F32, MN_DTYPE_F16 (which copies its weights: Plan<half> only)
    m.mma_fwd = m.mma_bwd = MMA_NATIVE;
    m.overflow_guard = DT == MN_F16;
    // (MN_DETERMINISTIC: the stem's backward goes through BatchNorm backward + the split-slice weight gradient instead)
    m.stem_bwd = DT == MN_F16 && !deterministic ? STEM_TILES : STEM_CHAIN;
    if (DT == MN_F16 || dtype == MN_DTYPE_F32) return m;
    // MN_DTYPE_F32X3 (Plan<float> only): fp32 tensors, contractions on the f16 / bf16 matrix pipe with split operands
    // (common.h MMA_*): forward f16x3, backward bf16x3; the fc / pose head stay on the exact fp32 MFMA
    m.mma_fwd = MMA_F16X3;  // (the h2 modes too: the stem's kernels and its fp32 tensors)
    m.mma_bwd = MMA_BF16X3;
    if (dtype == MN_DTYPE_F32X3) return m;
    // MN_DTYPE_F16X2 (Plan<float> only): every tensor a convolution consumes -- block inputs / outputs, a1, the projection
    // output, d(conv output), both weight copies -- is an h2 tensor (fp16 hi + lo halves, 4 bytes per element: the arena is
    // carved exactly as for fp32), written by the h2 element-wise kernels (elementwise_h2.h) and read by the h2 convolution
    // kernels through LDS-DMA; raw conv outputs, data gradients, statistics, head, criterion and optimiser are fp32.  The stem
    // (3 input channels: no 32-channel groups) stays on the fp32x3 kernels: fp32 xpad / stem.gy, f16x3 / bf16x3 contraction.
    // Gradients live in fp16 pairs, so the mode scales the loss and guards against overflow exactly as the fp16 mode does.
    m.act = m.gy = m.wf = m.wd = FMT_H2;
    m.overflow_guard = true;
    if (dtype == MN_DTYPE_F16X2) return m;
    // MN_DTYPE_F16X2M (round 5; Plan<float> only): the fp16x2 FORWARD pass, bit for bit -- loss and poses are that mode's -- and a
    // backward pass that contracts SINGLE fp16 operands, one MFMA per product, on the fp16 mode's kernels: d(conv output), data
    // gradients and the data-gradient weight copy are plain fp16 tensors (in the buffers the arena carves for fp32); the X operand of
    // a weight gradient and the ReLU gates are the HI halves of the h2 activations, read in place (round 5 read plain fp16 COPIES
    // written beside the h2 tensors; round 6: WgradArgs::x_h2, Epilogue::gate_h2 -- 2 bytes per activation element less written by
    // every BatchNorm apply, 2.5 GB less arena at 192 images).
    // What stays exact: every gate (sign of the forward value) and BatchNorm's backward statistics (fp32 conv output, fp64 sums).
    // What it costs the gradients: 1.1e-3 relative L2 overall / 1.6e-3 worst tensor (tools/mixed_budget.py: the oracle's own step
    // with fp16 conv operands in the backward pass) -- a fifth of the 4.9e-3 / 1.1e-2 by which two correct fp32 evaluations of this
    // network differ through ReLU gate flips.  The STEM is the exception to "statistics from the exact forward
    // values": by default (STEM_TILES_ON_COPIES) its two backward kernels (stem_bwd.h) read an fp16 copy of the fp32 conv output
    // (written by the stem's BatchNorm + max-pool pass) and an fp16 image of the input, so its BatchNorm-backward sums and xhat come
    // from fp16-rounded y; only its ReLU gate stays exact (the pooled gradient arrives already gated by layer1.0's data gradient:
    // StemBwdArgs::pre_gated).  MN_DETERMINISTIC=1 keeps the fp32 chain of fp16x2 for the stem.
    // Round 6: BatchNorm's backward pass reads a 2-byte RECORD of the forward pass (fp16 xhat + the ReLU's outcome in its lowest
    // bit, written by the forward apply) instead of the 4-byte conv output -- 2 bytes per element more in one forward pass, 2 fewer
    // in each of the two backward passes, and the gate stays exact (Unit::rec; profiles/r06/c4_batchnorm_backward_from_a_record.txt).
    m.gy = m.gx = m.wd = FMT_F16;
    if (!deterministic) m.stem_bwd = STEM_TILES_ON_COPIES;
    // MN_DTYPE_F16X2Q (round 5; Plan<float> only): fp16x2m whose FORWARD convolutions take both cross terms of a split-operand
    // product from fp8 copies on the block-scaled MFMA (common.h MMA_H2Q, h2q tensors): 2 instead of 3 MFMA-equivalents per forward
    // product, poses ~3e-4 from the fp32 reference instead of 1.6e-5 (bar 1e-3)
    if (dtype == MN_DTYPE_F16X2Q) m.act = m.wf = FMT_H2Q;
    return m;
  }
  // MN_DETERMINISTIC=1: bit-reproducible training steps -- every floating-point sum the step takes is added in an order
  // that does not depend on scheduling: BatchNorm sums through one accumulator row per producing workgroup (carve),
  // weight gradients through per-split workspace slices and an ordered reduction (conv_wgrad), the gradient norm through
  // per-workgroup partial sums (optim.h).  Costs ~x ms per step.
  const bool deterministic = knobs().deterministic;
  const Mode md;
  // ---- schedule knobs (knobs.h), copied at construction -------------------------------------------------------------
  // bit 0: BatchNorm+ReLU+max-pool in one forward pass (-0.15 ms/step); bit 1: max-pool gradient gathered inside the
  // BatchNorm backward passes instead of a maxpool_bwd launch (measured +0.05 ms/step: the gather runs twice) -- off
  const int fuse_stem_mask = knobs().fuse_stem;
  const bool fuse_stem = (fuse_stem_mask & 1) != 0;
  const bool fuse_stem_bwd = (fuse_stem_mask & 2) != 0;
  static constexpr bool parity_dgrad = true;  // stride-2 data gradients by parity class (dgrad.h: -1.6 % step time)
  // Weight-gradient schedule: the knobs, the per-mode defaults and their measurements are in knobs.h (resolve_wgrad_schedule)
  const WgradSchedule wgrad = resolve_wgrad_schedule(knobs(), md.overflow_guard, md.gy == FMT_F16);
  const int wgrad_tail = knobs().wgrad_tail;

  // ---- the network: units, blocks and their places in the arenas ---------------------------------------------------------
  struct Unit {  // conv + BatchNorm
    ConvP cp;
    BnP bp;
    int Hin, Win, Hout, Wout;
    long M;
    GatherGeom gf;
    DgradGeom dg;  // data-gradient launches (generic form + stride-2 parity classes), dgrad.h
    T* wf = nullptr;  // forward operand  [Cout][K], format md.wf
    T* wd = nullptr;  // data-gradient operand [Cin][R*S*Cout], format md.wd
    T* y = nullptr;   // raw conv output [M][Cout]
    T* gy = nullptr;  // its gradient, format md.gy
    half* rec = nullptr;  // fp16x2m: the BatchNorm's backward record [M][Cout] (elementwise_h2.h rec_pack), written by the forward apply
    float *mean, *invstd;
    float *coef_f, *coef_b;  // per-channel coefficients of the forward apply [2][C] / backward apply [4][C] (finalize kernels)
    double *accum_f, *accum_b;  // fp64 sums of the forward statistics / backward reductions, [rows_f | rows_b][2][C]
    int rows_f = 0, rows_b = 0; // accumulator rows (ACC_ROWS; MN_DETERMINISTIC: one row per producing workgroup)
    int ldw;           // row pitch of the master weight gradient
    const int* colmap = nullptr;
  };
  struct Block {  // activations in format md.act, their gradients in md.gx
    Unit u1, u2, ud;
    bool down;
    int stage;
    const T* x;   // block input
    T* gx;        // gradient w.r.t. block input (written by this block's backward)
    T* a1;        // relu(bn1(conv1 x))
    T* ga1;
    T* zd;        // bn_d(conv_d x) when down
    T* out;       // block output
    T* gout;      // gradient w.r.t. block output (written by the consumer)
  };

  float *params, *grads, *m1, *m2;
  char* buffers;
  char* work;
  int B, H, W, Hp, Wp;
  int frames;  // images per window
  T* xpad;
  Unit stem;
  T *a0, *ga0, *p0, *gp0;
  half* xpad16 = nullptr;   // fp16x2m: fp16 copy of the padded NHWC4 input (the stem's fp16 backward kernels, stem_bwd.h)
  int H0, W0, H1, W1;  // stem conv output, pooled output
  std::vector<Block> blocks;
  int Hl, Wl;  // last feature map
  float *pooled, *feat, *poses, *dposes, *dz, *dpooled, *fcT, *loss_dev, *dropmask;
  float *jit_draws, *jit_partials, *jit_mean;  // ColorJitter: [B][8] draws, [B][kJitterChunks] gray sums, [B] mean gray
  float *ig_flag, *sal_work;  // input_grad: {1 if the last call's gradient held a non-finite value}, [B][kSalChunks][2] (min, max)
  // mn_set_input_index: 1 if an index of the last indexed pass lay outside the store -- the second float of ig_flag's 256 bytes
  float* index_flag() const { return ig_flag + 1; }
  // BatchNorm sums are accumulated with fp64 atomics straight from the producing kernels (conv epilogue, backward
  // reduction) into ACC_ROWS rows per unit (row = producer block % ACC_ROWS, to spread same-address contention);
  // the consuming apply kernels add the rows in their prologue.  No separate partial-reduction launches.
  static constexpr int ACC_ROWS = 8;  // (32 rows measured equal: 14.73 vs 14.69 ms per step)
  double* acc_region = nullptr;
  size_t acc_bytes = 0;
  double* sqnorm;             // squared gradient norm: the first double of acc_region
  static constexpr int kSqPartials = 8192;
  double* sq_partials = nullptr;  // MN_DETERMINISTIC: per-workgroup sums of the gradient norm
  unsigned char* frozen;
  int* stem_colmap;
  RepackJob* repack_jobs;
  BnEvalJob* bn_eval_jobs = nullptr;  // every BatchNorm unit of the network: the fused inference pass's coefficient launch
  int bn_eval_njobs = 0;
  static constexpr int kBnEvalJobs = 40;  // stem + 16 blocks x 2 + 3 projections = 36
  int repack_njobs = 0, repack_blocks = 0, repack_head_jobs = -1, repack_head_blocks = 0;
  unsigned char* pool_idx;  // winning tap of every max-pool window
  float* wgf_ws = nullptr;  // partial tiles of the fused weight gradient (wgrad_fused.h), shared by its launches (one stream)
  long wgf_ws_floats = 0;
  void* zero_page;          // 256 zero bytes: source of out-of-image taps for the DMA conv pipeline
  long long* overflow_dev;  // {this step skipped, skipped steps in total, last skipped attempt, last completed attempt} (adam_prep_kernel)
  long long* step_dev;      // device-resident Adam step counter
  float* bc_dev;            // {1 - beta1^t, 1 - beta2^t}, derived on device from step_dev

  // ---- state of the step being enqueued ------------------------------------------------------------------------------
  int cur_training = 1;
  bool sqnorm_clean = false;  // zeroed by this step's fill and not yet accumulated into
  bool grads_zeroed = false;
  const float* cur_targets = nullptr;
  float* cur_loss = nullptr;
  struct PendingWgrad {
    Unit* u;
    const T* x;
  };
  std::vector<PendingWgrad> pending_wgrads;  // weight gradients held back until the next fork (flush_wgrads)

  // ---- construction -----------------------------------------------------------------------
  size_t carve(char* base) override {
    Bump b;
    auto A = [&](size_t bytes) { return base ? base + b.take(bytes) : (b.take(bytes), (char*)nullptr); };
    // all BatchNorm accumulators live in one region so a single memset per step clears them
    // MN_DETERMINISTIC: one row per producing workgroup: every (row, channel) slot then receives exactly ONE atomic add onto zero,
    // and the finalize kernels add the rows in a fixed order.  Forward producers: the stem kernel's persistent workgroups, the
    // layer1 kernel's persistent workgroups (halo_pp.h: at most one per 16x16-pixel tile), M-tiles of >= 128 rows elsewhere.
    auto set_rows = [&](Unit& u) {
      u.rows_f = u.rows_b = ACC_ROWS;
      if (!deterministic) return;
      u.rows_f = halo_path(u.gf) ? u.gf.B * cdiv(u.gf.P, kHaloTH) * cdiv(u.gf.Q, kHaloTW) : cdiv((int)u.M, 128);
      // (layer1's h2 convolutions on the persistent register-resident-weight kernel, halo_h2.h: one row per workgroup)
      if (md.act == FMT_H2 && u.cp.k == 3 && u.cp.stride == 1 && u.cp.cin == 64 && u.cp.cout == 64) {
        const int wgs = conv_halo_h2_grid(u.gf);
        if (u.rows_f < wgs) u.rows_f = wgs;
      }
      u.rows_b = 1024;  // >= the workgroups of a backward reduction (launch_bn_bwd: ~512)
    };
    stem.rows_f = stem.rows_b = ACC_ROWS;
    if (deterministic) {
      stem.rows_f = (DT == MN_F16 || md.mma_fwd == MMA_F16X3) ? 1024 : cdiv((int)stem.M, 128);
      stem.rows_b = 1024;
    }
    size_t acc_doubles = (size_t)(stem.rows_f + stem.rows_b) * 2 * 64;
    for (auto& blk : blocks) {
      set_rows(blk.u1);
      set_rows(blk.u2);
      if (blk.down) set_rows(blk.ud);
      acc_doubles += (size_t)(blk.u1.rows_f + blk.u1.rows_b + blk.u2.rows_f + blk.u2.rows_b) * 2 * blk.u1.cp.cout;
      if (blk.down) acc_doubles += (size_t)(blk.ud.rows_f + blk.ud.rows_b) * 2 * blk.ud.cp.cout;
    }
    // ... and the squared gradient norm rides at its head: ONE fill launch per step clears all of it (hipMemsetAsync's fill
    // kernel took ~110 us per call for these 2 MB, on the main stream at the head of every step; round-3 profile)
    acc_bytes = (acc_doubles + 2) * 8;
    acc_region = (double*)A(acc_bytes);
    sqnorm = acc_region;
    double* acc_cursor = acc_region ? acc_region + 2 : nullptr;
    auto unit_bufs = [&](Unit& u) {
      int C = u.cp.cout;
      u.y = (T*)A((size_t)u.M * C * sizeof(T));
      u.gy = (T*)A((size_t)u.M * C * sizeof(T));
      u.mean = (float*)A(C * 4);
      u.invstd = (float*)A(C * 4);
      u.coef_f = (float*)A(2 * C * 4);
      u.coef_b = (float*)A(4 * C * 4);
      u.accum_f = acc_cursor;
      u.accum_b = acc_cursor ? acc_cursor + (size_t)u.rows_f * 2 * C : nullptr;
      if (acc_cursor) acc_cursor += (size_t)(u.rows_f + u.rows_b) * 2 * C;
    };
    xpad = (T*)A((size_t)B * Hp * Wp * 4 * sizeof(T));
    // stem
    unit_bufs(stem);
    stem.wf = (T*)A((size_t)64 * 224 * sizeof(T));
    size_t n0 = (size_t)B * H0 * W0 * 64, n1 = (size_t)B * H1 * W1 * 64;
    a0 = (T*)A(n0 * sizeof(T));
    ga0 = (T*)A(n0 * sizeof(T));
    p0 = (T*)A(n1 * sizeof(T));
    gp0 = (T*)A(n1 * sizeof(T));
    pool_idx = (unsigned char*)A(n1);
    if (md.f16_bwd_on_pairs()) xpad16 = (half*)A((size_t)B * Hp * Wp * 4 * sizeof(half));
    const T* x = p0;
    T* gx = gp0;
    for (auto& blk : blocks) {
      blk.x = x;
      blk.gx = gx;
      Unit* us[3] = {&blk.u1, &blk.u2, blk.down ? &blk.ud : nullptr};
      for (Unit* u : us) {
        if (!u) continue;
        unit_bufs(*u);
        if (md.f16_bwd_on_pairs()) u->rec = (half*)A((size_t)u->M * u->cp.cout * sizeof(half));
        size_t wn = (size_t)u->cp.cout * u->cp.cin * u->cp.k * u->cp.k;
        if (md.wf != FMT_F32)
          u->wf = (T*)A(wn * sizeof(T));  // (h2: 4 bytes per element as well)
        else
          u->wf = base ? (T*)(params + u->cp.w) : nullptr;  // fp32: the OHWI master is the operand
        u->wd = (T*)A(wn * sizeof(T));
      }
      size_t no = (size_t)blk.u2.M * blk.u2.cp.cout;
      blk.a1 = (T*)A(no * sizeof(T));
      blk.ga1 = (T*)A(no * sizeof(T));
      blk.zd = blk.down ? (T*)A(no * sizeof(T)) : nullptr;
      blk.out = (T*)A(no * sizeof(T));
      blk.gout = (T*)A(no * sizeof(T));
      x = blk.out;
      gx = blk.gout;
    }
    int F = cfg.feat_dim;
    pooled = (float*)A((size_t)B * 512 * 4);
    feat = (float*)A((size_t)B * F * 4);
    poses = (float*)A((size_t)B * 6 * 4);
    dposes = (float*)A((size_t)B * 6 * 4);
    dz = (float*)A((size_t)B * F * 4);
    dropmask = (float*)A((size_t)B * F * 4);
    dpooled = (float*)A((size_t)B * 512 * 4);
    fcT = (float*)A((size_t)512 * F * 4);
    loss_dev = (float*)A(256);
    sq_partials = (double*)A((size_t)kSqPartials * 8);
    frozen = (unsigned char*)A(256);
    stem_colmap = (int*)A(224 * 4);
    repack_jobs = (RepackJob*)A(64 * sizeof(RepackJob));
    zero_page = (void*)A(256);
    wgf_ws_floats = (DT == MN_F16 || md.mma_bwd == MMA_BF16X3) ? wgrad_fused_ws_floats(WGF_BLOCKS) : 0;  // (all fused forms)
    if (deterministic && wgf_ws_floats < (16L << 20)) wgf_ws_floats = 16L << 20;  // split slices of the plain weight gradients
    wgf_ws = wgf_ws_floats ? (float*)A((size_t)wgf_ws_floats * 4) : nullptr;
    step_dev = (long long*)A(256);
    bc_dev = (float*)A(256);
    overflow_dev = (long long*)A(256);
    jit_draws = (float*)A((size_t)B * 8 * 4);  // (last: the buffers above keep their offsets)
    jit_partials = (float*)A((size_t)B * kJitterChunks * 4);
    jit_mean = (float*)A((size_t)B * 4);
    ig_flag = (float*)A(256);  // (input_grad: behind everything else, as above)
    sal_work = (float*)A((size_t)B * kSalChunks * 2 * 4);
    bn_eval_jobs = (BnEvalJob*)A(kBnEvalJobs * sizeof(BnEvalJob));  // (3 KB behind everything else, as above)
    return b.cur;
  }

  void init_unit(Unit& u, const ConvP& c, const BnP& b, int Hin, int Win) {
    u.cp = c;
    u.bp = b;
    u.Hin = Hin;
    u.Win = Win;
    u.Hout = (Hin + 2 * c.pad - c.k) / c.stride + 1;
    u.Wout = (Win + 2 * c.pad - c.k) / c.stride + 1;
    u.M = (long)B * u.Hout * u.Wout;
    u.gf = fwd_geom(B, Hin, Win, c.cin, c.cout, c.k, c.stride, c.pad, u.Hout, u.Wout);
    u.ldw = c.k * c.k * c.cin;
    u.dg = make_dgrad_geom(B, Hin, Win, c.cin, c.cout, c.k, c.stride, c.pad, u.Hout, u.Wout, VEC);
    u.gf.mma = md.mma_fwd;
    u.dg.full.mma = md.mma_bwd;
    for (int i = 0; i < u.dg.n_pc; ++i) u.dg.pc[i].g.mma = md.mma_bwd;
  }

  Plan(const mn_config& c) : md(mode_of(c.dtype, knobs().deterministic)) {
    cfg = c;
    cur_scale = c.loss_scale;
    scales_loss = md.overflow_guard;
    L = Layout(c.feat_dim);
    frames = frames_per_window(c.mode, c.T);
    B = c.windows * frames;
    H = c.H;
    W = c.W;
    Hp = H + 6;
    Wp = (W + 6 + 1 + 1) & ~1;  // even, >= W + 7
    // stem as a 7x4 conv over pixel pairs (C = 8), stride (2,1), no padding
    H0 = (H + 6 - 7) / 2 + 1;
    W0 = (W + 6 - 7) / 2 + 1;
    stem.cp = L.stem;
    stem.bp = L.stem_bn;
    stem.Hin = H; stem.Win = W; stem.Hout = H0; stem.Wout = W0;
    stem.M = (long)B * H0 * W0;
    GatherGeom g;
    g.B = B; g.Hi = Hp; g.Wi = Wp / 2; g.C = 8; g.P = H0; g.Q = W0; g.R = 7; g.S = 4;
    g.mul_p = 2; g.mul_q = 1; g.rsign = 1; g.ssign = 1; g.off_h = 0; g.off_w = 0; g.div = 1;
    g.M = B * H0 * W0; g.N = 64; g.K = 224;
    g.mma = md.mma_fwd;
    stem.gf = g;
    stem.ldw = 147;
    H1 = maxpool_out(H0);
    W1 = maxpool_out(W0);
    int h = H1, w = W1;
    for (const BlockP& bp : L.blocks) {
      Block blk;
      blk.down = bp.down;
      blk.stage = bp.stage;
      init_unit(blk.u1, bp.c1, bp.b1, h, w);
      init_unit(blk.u2, bp.c2, bp.b2, blk.u1.Hout, blk.u1.Wout);
      if (bp.down) init_unit(blk.ud, bp.cd, bp.bd, h, w);
      h = blk.u1.Hout;
      w = blk.u1.Wout;
      blocks.push_back(blk);
    }
    Hl = h;
    Wl = w;
  }

  int attach(float* params_, float* opt_state, void* buffers_, void* work_, hipStream_t s) override {
    params = params_;
    grads = opt_state;
    m1 = opt_state + L.param_floats;
    m2 = opt_state + 2 * L.param_floats;
    buffers = (char*)buffers_;
    work = (char*)work_;
    size_t total = carve(work);
    hipMemsetAsync(work, 0, total, s);
    // stem column map: compute column (r, s4, e) -> dense OHWI column (r, s', ch) or -1
    std::vector<int> cm(224);
    for (int r = 0; r < 7; ++r)
      for (int s4 = 0; s4 < 4; ++s4)
        for (int e = 0; e < 8; ++e) {
          int sp = 2 * s4 + (e >> 2), ch = e & 3;
          cm[(r * 4 + s4) * 8 + e] = (sp < 7 && ch < 3) ? (r * 7 + sp) * 3 + ch : -1;
        }
    hipMemcpyAsync(stem_colmap, cm.data(), 224 * 4, hipMemcpyHostToDevice, s);
    hipStreamSynchronize(s);  // cm is a host temporary
    stem.colmap = stem_colmap;
    if (md.overflow_guard && !overflow_host) {
      if (hipHostMalloc((void**)&overflow_host, 4 * sizeof(long long)) != hipSuccess) {
        overflow_host = nullptr;
        (void)hipGetLastError();
      } else {
        overflow_host[0] = overflow_host[1] = overflow_host[2] = overflow_host[3] = 0;
      }
    }
    build_repack_table(s);
    build_bn_eval_table(s);
    update_frozen(s);
    weights_dirty = true;
    return check_launch("attach");
  }

  void update_frozen(hipStream_t s) override {
    unsigned char f[4] = {(unsigned char)!learn_beta, (unsigned char)!learn_beta, (unsigned char)!learn_gamma,
                          (unsigned char)!learn_gamma};
    hipMemcpyAsync(frozen, f, 4, hipMemcpyHostToDevice, s);
    hipStreamSynchronize(s);
  }

  // ---- weights: fp32 master -> compute layouts ------------------------------------------------
  void build_repack_table(hipStream_t s) {
    std::vector<RepackJob> jobs;
    int blk = 0;
    auto add = [&](long src, void* a, void* b2, int O, int R, int S, int I, int mode) {
      RepackJob j;
      j.src_off = src; j.dst_a = a; j.dst_b = b2; j.O = O; j.R = R; j.S = S; j.I = I; j.mode = mode;
      long total = mode == 2 ? (long)O * R * 32 : (long)O * R * S * I;
      j.blk0 = blk;
      j.nblk = (int)((total + 4095) / 4096);
      blk += j.nblk;
      jobs.push_back(j);
    };
    add(stem.cp.w, stem.wf, nullptr, 64, 7, 7, 3, 2);
    repack_head_jobs = -1;
    for (auto& bk : blocks) {
      if (bk.stage >= 1 && repack_head_jobs < 0) {  // jobs before this one serve the stem and layer1
        repack_head_jobs = (int)jobs.size();
        repack_head_blocks = blk;
      }
      Unit* us[3] = {&bk.u1, &bk.u2, bk.down ? &bk.ud : nullptr};
      for (Unit* u : us) {
        if (!u) continue;
        const ConvP& c = u->cp;
        add(c.w, md.wf != FMT_F32 ? (void*)u->wf : nullptr, u->wd, c.cout, c.k, c.k, c.cin, 0);
      }
    }
    add(L.fc_w, fcT, nullptr, cfg.feat_dim, 1, 1, 512, 3);
    repack_njobs = (int)jobs.size();
    repack_blocks = blk;
    hipMemcpyAsync(repack_jobs, jobs.data(), jobs.size() * sizeof(RepackJob), hipMemcpyHostToDevice, s);
    hipStreamSynchronize(s);  // `jobs` is a host temporary
  }
  // the BatchNorm units of the network in pass order (bn_eval_coef_all_kernel, elementwise.h)
  void build_bn_eval_table(hipStream_t s) {
    std::vector<BnEvalJob> jobs;
    auto add = [&](const Unit& u) {
      BnEvalJob j;
      j.p = bn_params(u);
      j.coef = u.coef_f;
      j.C = u.cp.cout;
      jobs.push_back(j);
    };
    add(stem);
    for (auto& bk : blocks) {
      if (bk.down) add(bk.ud);
      add(bk.u1);
      add(bk.u2);
    }
    bn_eval_njobs = (int)jobs.size();
    if (bn_eval_njobs > kBnEvalJobs) bn_eval_njobs = 0;  // (cannot happen for this network; mn_set_eval_fused then refuses)
    hipMemcpyAsync(bn_eval_jobs, jobs.data(), (size_t)bn_eval_njobs * sizeof(BnEvalJob), hipMemcpyHostToDevice, s);
    hipStreamSynchronize(s);  // `jobs` is a host temporary
  }
  // head = stem + layer1 weights (needed first), tail = everything else; the tail can run on the side stream
  // while the stem and layer1 execute
  void repack_head(hipStream_t s) {
    const bool split = repack_head_jobs > 0;
    launch_repack<T>(repack_jobs, split ? repack_head_jobs : repack_njobs, params, 0, split ? repack_head_blocks : repack_blocks,
                     md.wf, md.wd, s);
  }
  void repack_tail(hipStream_t s) {
    const int hb = repack_head_jobs > 0 ? repack_head_blocks : repack_blocks;
    if (repack_blocks > hb) launch_repack<T>(repack_jobs, repack_njobs, params, hb, repack_blocks - hb, md.wf, md.wd, s);
    weights_dirty = false;
  }

  // ---- forward ------------------------------------------------------------------------------------
  BnParams bn_params(const Unit& u) {
    BnParams p;
    p.gamma = params + u.bp.gamma;
    p.beta = params + u.bp.beta;
    p.running_mean = (float*)buffers + u.bp.rm;
    p.running_var = (float*)buffers + u.bp.rv;
    p.num_batches_tracked = (long long*)(buffers + u.bp.nbt);
    p.mean = u.mean;
    p.invstd = u.invstd;
    p.eps = 1e-5f;
    p.momentum = 0.1f;
    return p;
  }
  Epilogue stats_epilogue(Unit& u, int training) {  // raw conv output + (training) its column sums for the BatchNorm
    Epilogue ep;
    ep.out = u.y;
    ep.ldc = u.cp.cout;
    if (training) {
      ep.stats_accum = u.accum_f;
      ep.stats_rows = u.rows_f;
    }
    return ep;
  }
  // the convolution of a block unit (the stem has its own: stem_conv)
  void conv_bn_stats(Unit& u, const T* x, int training, hipStream_t s) {
    const Epilogue ep = stats_epilogue(u, training);
    auto* tp = timer.begin(0, s);
    if (md.pairs())  // h2 activation and weights in, fp32 conv output + statistics out
      launch_igemm_h2(u.gf, (const half*)x, (const half*)u.wf, ep, s, (const half*)zero_page, md.act == FMT_H2Q);
    else if (halo_path(u.gf) && conv_halo_pp_applies(u.gf, ep))
      launch_conv_halo_pp(u.gf, (const half*)x, (const half*)u.wf, ep, s);
    else
      launch_igemm<T>(u.gf, x, u.wf, ep, s, (const T*)zero_page);
    timer.end(tp, s);
  }
  // Fused inference pass: out(h2) = [relu](conv(x; u) * scale + shift [+ res(h2)]) in ONE launch -- the kernel and tile shape
  // conv_bn_stats picks for this geometry, with the fused epilogue (igemm.h EV); u.y is not written.  u.coef_f holds this pass's
  // coefficients (bn_eval_coef_all_kernel at the head of the pass).
  std::string eval_fused_refusal() const override {
    static const char* const names[] = {"fp32", "fp16", "fp32x3", "fp16x2", "fp16x2m", "fp16x2q"};
    if (md.act != FMT_H2)
      return std::string("the fused inference pass needs h2 activations (fp16x2, fp16x2m); this plan computes in ") +
             (cfg.dtype >= 0 && cfg.dtype < 6 ? names[cfg.dtype] : "an unknown dtype");
    if (bn_eval_njobs <= 0) return "the coefficient job table does not hold this network's BatchNorm units";
    return "";
  }
  void conv_bn_eval(Unit& u, const T* x, const T* res, int relu, T* out, hipStream_t s) {
    const Epilogue ep = eval_epilogue(out, u.cp.cout, u.coef_f, res, relu);  // (what the dispatcher reads is the unfused launch's)
    auto* tp = timer.begin(0, s);
    launch_igemm_h2<true>(u.gf, (const half*)x, (const half*)u.wf, ep, s, (const half*)zero_page, false);
    timer.end(tp, s);
  }
  // the stem reads 3 channels (no 32-channel groups, no halo): its own kernels, or the generic implicit GEMM on exact fp32
  void stem_conv(int training, hipStream_t s) {
    double* const sums = training ? stem.accum_f : nullptr;
    auto* tp = timer.begin(0, s);
    if (DT == MN_F32 && md.mma_fwd == MMA_F16X3)  // the split-operand form of the stem kernel
      launch_stem_conv_x3((const float*)xpad, (const float*)stem.wf, (float*)stem.y, sums, stem.rows_f, B, H, W, Wp, s);
    else if (DT == MN_F16)  // weights in registers, input pairs read straight from LDS (stem.h)
      launch_stem_conv((const half*)xpad, (const half*)stem.wf, (half*)stem.y, sums, stem.rows_f, B, H, W, Wp, s);
    else
      launch_igemm<T>(stem.gf, xpad, stem.wf, stats_epilogue(stem, training), s, (const T*)zero_page);
    timer.end(tp, s);
  }
  // layer1's 64-channel 3x3 convolutions (forward and data gradient) run from an LDS-resident input halo in the
  // persistent two-group kernel of halo_pp.h; the shapes it does not cover go to the implicit-GEMM kernel
  bool halo_path(const GatherGeom& g) const { return md.act == FMT_F16 && conv_halo_applies(g); }
  void bn_finalize(Unit& u, hipStream_t s) {  // statistics -> (scale, shift), mean / invstd, running statistics
#ifdef MN_ABLATION_BUILD
    const int skip_c = knobs().abl_skip_finalize;  // (see launch_bn_bwd)
    static long calls = 0;
    if (u.cp.cout <= skip_c && ++calls > 400) return;
#endif
    launch_bn_finalize_fwd(u.accum_f, u.M, bn_params(u), cur_training, u.coef_f, u.cp.cout, u.rows_f, s);
  }
  void bn_act(Unit& u, const T* res, int relu, T* out, hipStream_t s) {
    bn_finalize(u, s);
    if (md.pairs())  // fp32 conv output in, h2 activation out (residual: an h2 activation)
      launch_bn_apply_h2((const float*)u.y, u.coef_f, (const half*)res, (half*)out, u.M, u.cp.cout, relu, md.act == FMT_H2Q ? 1 : 0,
                         cur_training ? u.rec : (half*)nullptr, u.mean, u.invstd, s);
    else
      launch_bn_apply<T>(u.y, u.coef_f, res, out, u.M, u.cp.cout, relu, s);
  }

  // ColorJitter + ToTensor + Normalize (jitter.h); every jittered pass advances jit_calls by one
  void launch_jitter_input(const unsigned char* images, half* x16, hipStream_t s) {
    launch_u8_jitter<T>(images, xpad, B, H, W, Hp, Wp, jitter_norm, x16, jitter_params(jit_range, jit_seed, jit_calls), jit_draws,
                        jit_partials, jit_mean, s);
    jit_calls += 1;
  }

  int forward(const void* images, float* poses_out, int training, hipStream_t s) override {
    return forward_impl(images, poses_out, training, false, s);
  }
  int forward_impl(const void* images, float* poses_out, int training, bool zero_grads, hipStream_t s) {
    if (jitter_on() && !input_u8)
      return fail("forward: ColorJitter (mn_set_color_jitter) needs uint8 input (mn_set_input_u8): fp32 frames arrive already "
                  "normalised, and ColorJitter must come before Normalize");
    if (resize_on && !input_u8)
      return fail("forward: Resize (mn_set_input_resize) needs uint8 input (mn_set_input_u8): fp32 frames arrive already "
                  "normalised, and Resize must come before Normalize");
    if ((resize_on || in_index) && !images) return fail("forward: images are required");
    const int64_t batch_bytes = (int64_t)B * H * W * 3 * (input_u8 ? 1 : 4);
    if (in_index && !resize_on && (!in_stage || in_stage_bytes < batch_bytes))
      return fail("forward: the staging buffer of mn_set_input_index holds " + std::to_string((long long)in_stage_bytes) +
                  " bytes, the gathered batch needs " + std::to_string((long long)batch_bytes) + " (mn_input_index_bytes)");
    // work the stem and layer1 do not depend on goes to the side stream: the repack of the later layers'
    // weights and optim.learner.zero_grad(); joined before layer2
    const bool dirty = weights_dirty;
    if (dirty) repack_head(s);
    grads_zeroed = zero_grads;
    cur_training = training;
    if (training) {  // forward statistics + backward reduction sums + the squared gradient norm
      launch_zero_fill(reinterpret_cast<float*>(acc_region), (long)(acc_bytes / 4), s);
      sqnorm_clean = true;
    }
    // (fp16x2m: the stem's fp16 backward kernels read an fp16 image of the input -- written by the same launch)
    half* const x16 = md.stem_bwd == STEM_TILES_ON_COPIES && training ? xpad16 : (half*)nullptr;
    if (in_index) {  // frames come from a store: the flag of an index outside it starts every pass at 0
      hipMemsetAsync(index_flag(), 0, sizeof(float), s);
      if (!resize_on) {
        launch_gather_frames(images, in_index, in_stage, batch_bytes / B, B, in_store_frames, index_flag(), s);
        images = in_stage;
      }
    }
    if (resize_on) {  // Resize first: the conversion below reads the resized frames
      launch_resize_u8((const unsigned char*)images, rs_frames, rs_geom, s, in_index, in_store_frames, index_flag());
      images = rs_frames;
    }
    if (input_u8 && jitter_on())
      launch_jitter_input((const unsigned char*)images, x16, s);
    else
      launch_input_to_padded_nhwc4<T>(images, input_u8, xpad, B, H, W, Hp, Wp, input_norm, x16, s);
    // forked AFTER the (HBM-bound) input conversion, so that the side stream's copies run beside the stem's MFMA-bound
    // convolution instead of competing with the conversion for bandwidth (step time: equal within noise)
    if (dirty || zero_grads) {
      hipStream_t side = fork_wgrad(s);
      if (dirty) repack_tail(side);
      if (zero_grads) launch_zero_fill(grads, L.param_floats, side);
    }
    // the fused inference pass: every unit's (scale, shift), mean and invstd from the running statistics in one launch, here at
    // the head of the pass -- after an optimiser step or a load_state_dict there is nothing to mark dirty
    const bool fused = eval_fused && !training;  // (mn_set_eval_fused turns it on only for a plan that can run it)
    if (fused) launch_bn_eval_coef_all(bn_eval_jobs, bn_eval_njobs, s);
    stem_conv(training, s);
    if (md.pairs()) {  // (always the fused form: fp32 conv output in, h2 pooled activation out)
      if (!fused) bn_finalize(stem, s);
      launch_bn_relu_maxpool_h2((const float*)stem.y, stem.coef_f, (half*)p0, pool_idx, B, H0, W0, 64,
                                training && md.stem_bwd == STEM_TILES_ON_COPIES ? (half*)a0 : (half*)nullptr,
                                md.act == FMT_H2Q ? 1 : 0, s);
    } else if (fuse_stem) {  // BatchNorm + ReLU + max-pool in one pass; the normalised stem activation is never stored
      bn_finalize(stem, s);
      launch_bn_relu_maxpool<T>(stem.y, stem.coef_f, p0, pool_idx, B, H0, W0, 64, s);
    } else {
      bn_act(stem, nullptr, 1, a0, s);
      launch_maxpool_fwd<T>(a0, p0, pool_idx, B, H0, W0, 64, s);
    }
    for (auto& blk : blocks) {
      if (blk.stage >= 1) join_wgrad(s);  // no-op once joined
      if (fused) {  // three launches per down block, two per other block; the fork and join of the projection path as below
        if (blk.down) conv_bn_eval(blk.ud, blk.x, nullptr, 0, blk.zd, fork_wgrad(s));
        conv_bn_eval(blk.u1, blk.x, nullptr, 1, blk.a1, s);
        if (blk.down) join_wgrad(s);
        conv_bn_eval(blk.u2, blk.a1, blk.down ? blk.zd : blk.x, 1, blk.out, s);
        continue;
      }
      // The projection path of a down block (1x1 stride-2 convolution, BatchNorm) depends on the block's input only: it runs on the
      // side stream -- idle in the forward pass -- beside conv1 -> bn1 -> conv2 and is joined before the residual add.  Three blocks,
      // ~0.25 ms of small launches: fp16x2m 18.18 -> 18.05 ms, four of four interleaved pairs (profiles/r06/c41_c42_*).
      if (blk.down) {
        hipStream_t ws = fork_wgrad(s);
        conv_bn_stats(blk.ud, blk.x, training, ws);
        bn_act(blk.ud, nullptr, 0, blk.zd, ws);
      }
      conv_bn_stats(blk.u1, blk.x, training, s);
      bn_act(blk.u1, nullptr, 1, blk.a1, s);
      conv_bn_stats(blk.u2, blk.a1, training, s);
      const T* res = blk.x;
      if (blk.down) {
        join_wgrad(s);
        res = blk.zd;
      }
      bn_act(blk.u2, res, 1, blk.out, s);
    }
    join_wgrad(s);
    const Block& last = blocks.back();
    int F = cfg.feat_dim;
    if (md.pairs())
      launch_avgpool_fwd_h2((const half*)last.out, pooled, B, Hl * Wl, 512, md.act == FMT_H2Q ? 1 : 0, s);
    else
      launch_avgpool_fwd<T>(last.out, pooled, B, Hl * Wl, 512, s);
    // fc 512 -> feat_dim, bias, ReLU (models/posenet.py:46,65-66); dropout is the identity under the
    // reference's pinned torch 0.4.1 (F.dropout default training=False)
    Epilogue ep;
    ep.out = feat;
    ep.ldc = F;
    ep.bias = params + L.fc_b;
    ep.relu = 1;
    DenseArgs da;
    da.A = pooled; da.W = params + L.fc_w; da.bias = params + L.fc_b; da.C = feat; da.M = B; da.N = F; da.K = 512; da.lda = 512;
    da.ldw = 512; da.ldc = F; da.relu = 1;
    if (dense_nt_applies(da))  // 32 x 32 tiles, K split over the workgroup's waves (dense.h)
      launch_dense_nt(da, s);
    else
      launch_igemm<float>(dense_geom(B, F, 512), (const float*)pooled, (const float*)(params + L.fc_w), ep, s, (const float*)zero_page);
    // F.dropout(x, p=droprate) (models/posenet.py:68-69), in training mode only (mn_set_dropout explains the reference's two
    // readings): a fresh Philox mask per training forward pass, kept for the backward pass
    drop_this_step = training && drop_p > 0.f;
    if (drop_this_step) {
      launch_dropout_fwd(feat, dropmask, (long)B * F, drop_p, drop_seed, drop_calls, s);
      drop_calls += 1;
    }
    launch_head_fwd(feat, params + L.xyz_w, params + L.xyz_b, params + L.wpqr_w, params + L.wpqr_b, poses, B, F, s);
    if (poses_out) hipMemcpyAsync(poses_out, poses, (size_t)B * 6 * 4, hipMemcpyDeviceToDevice, s);
    return check_launch("forward");
  }

  void run_criterion(const float* pred, const float* targ, float* loss, float* dpred, float* ds, hipStream_t s) {
    CriterionArgs a;
    a.mode = cfg.mode; a.N = cfg.windows; a.T = cfg.T; a.pred = pred; a.targ = targ; a.s = params + L.crit; a.loss = loss;
    a.dpred = dpred; a.ds = ds; a.vos_out = nullptr; a.grad_scale = cur_scale;
    a.t_kind = t_kind; a.t_param = t_param; a.q_kind = q_kind; a.q_param = q_param;
    launch_criterion(a, s);
  }
  int loss_only(const float* pred, const float* targ, float* loss_out, hipStream_t s) override {
    run_criterion(pred, targ, loss_out, nullptr, nullptr, s);
    return check_launch("loss");
  }
  int forward_loss(const void* images, const float* targets, float* loss_out, float* poses_out, hipStream_t s) override {
    if (int e = forward_impl(images, poses_out, 1, true, s)) return e;
    cur_targets = targets;
    cur_loss = loss_out ? loss_out : loss_dev;
    return 0;
  }

  // ---- backward -------------------------------------------------------------------------------------
  // BatchNorm backward of a block unit.  `g` arrives already gated (block_backward) unless self_gate: then it is the gradient
  // w.r.t. relu(bn_u(y)) -- a1 of the block -- and the gate is recomputed from y (or read from the record), never read from a1.
  // No other gate exists, so none can be passed: the h2 / fp16x2m apply kernels have no gate input
  void bn_bwd(Unit& u, const T* g, hipStream_t s, bool self_gate = false) {
    float* const gamma = params + u.bp.gamma;
    const float* const sg_beta = self_gate ? params + u.bp.beta : nullptr;
    if (md.f16_bwd_on_pairs())  // fp16 gradient and the forward pass's record in; plain fp16 d(conv output) out
      launch_bn_bwd_rec((const half*)g, (const half*)u.rec, u.M, u.cp.cout, gamma, u.mean, u.invstd, grads + u.bp.gamma,
                        grads + u.bp.beta, (half*)u.gy, u.accum_b, u.coef_b, 1.f / cur_scale, s, self_gate, u.rows_b);
    else if (md.gy == FMT_H2)  // fp32 gradient and conv output in, h2 d(conv output) out
      launch_bn_bwd_h2((const float*)g, (const float*)u.y, u.M, u.cp.cout, gamma, u.mean, u.invstd, grads + u.bp.gamma,
                       grads + u.bp.beta, (half*)u.gy, u.accum_b, u.coef_b, 1.f / cur_scale, s, sg_beta, u.rows_b);
    else
      launch_bn_bwd<T>(g, (const T*)nullptr, (const T*)u.y, u.M, u.cp.cout, gamma, u.mean, u.invstd, grads + u.bp.gamma,
                       grads + u.bp.beta, u.gy, u.accum_b, u.coef_b, 1.f / cur_scale, s, sg_beta, PoolGradSrc(), u.rows_b);
  }
  WgradArgs wgrad_args(Unit& u, const T* x) {
    WgradArgs a;
    a.g = u.gf; a.dY = u.gy; a.ldy = u.cp.cout; a.X = x; a.dW = grads + u.cp.w; a.ldw = u.ldw; a.colmap = u.colmap;
    a.g.mma = md.mma_bwd;
    a.alpha = 1.f / cur_scale; a.rows_per_split = 0;
    a.ws = wgf_ws; a.ws_floats = wgf_ws_floats;  // every weight-gradient launch of a step goes to the same stream (`ws`)
    a.det = deterministic;
    return a;
  }
  // reduction splits (measured, tools/conv_bench.py): one round of 2 workgroups per CU for the wide layers (half
  // the atomic traffic of 1024), more for layer1 and the stem whose pixel dimension is 4-16x longer
  static int wgrad_splits(const Unit& u) { return u.cp.cout >= 128 ? 512 : (u.M > 2000000 ? 2048 : 1024); }
  // weight gradient of a block unit; `ws`: the stream the launch goes to (the side stream after a fork, or the main stream)
  void conv_wgrad(Unit& u, const T* x, hipStream_t ws) {
    WgradArgs a = wgrad_args(u, x);
    auto* tp = timer.begin(1, ws);
    if (md.f16_bwd_on_pairs()) {  // plain fp16 d(conv output) against the HI halves of the h2 activation: the fp16 mode's kernels
      a.g.mma = MMA_NATIVE;
      a.x_h2 = true;
      launch_wgrad<half>(a, wgrad_splits(u), ws, zero_page);
    } else if (md.gy == FMT_H2) {  // h2 d(conv output) and activation
      a.g.mma = MMA_H2;
      launch_wgrad<half>(a, wgrad_splits(u), ws, zero_page);
    } else {
      launch_wgrad<T>(a, wgrad_splits(u), ws, zero_page);
    }
    timer.end(tp, ws);
  }
  // gx = data gradient of u (+ res), zeroed where out_gate <= 0
  void conv_dgrad(Unit& u, T* gx, const T* res, hipStream_t s, const T* out_gate = nullptr) {
    Epilogue ep;
    ep.out = gx;
    ep.ldc = u.cp.cin;
    ep.res = res;
    ep.out_gate = out_gate;
    auto* tp = timer.begin(0, s);
    if (md.gy == FMT_H2) {  // h2 d(conv output) and weights in, fp32 gradient out (+ fp32 residual, h2 gate of the block below)
      launch_conv_dgrad<half>(u.dg, (const half*)u.gy, (const half*)u.wd, ep, s, (const half*)zero_page, parity_dgrad, true);
    } else if (md.gy == FMT_F16) {  // the fp16 mode's launches: fp16 d(conv output), weights, gradient and residual
      ep.gate_h2 = md.pairs();      // (fp16x2m: the gate = hi halves of the h2 activation)
      if (conv_halo_applies(u.dg.full) && conv_halo_pp_applies(u.dg.full, ep))
        launch_conv_halo_pp(u.dg.full, (const half*)u.gy, (const half*)u.wd, ep, s);
      else
        launch_conv_dgrad<half>(u.dg, (const half*)u.gy, (const half*)u.wd, ep, s, (const half*)zero_page, parity_dgrad);
    } else {
      launch_conv_dgrad<T>(u.dg, (const T*)u.gy, (const T*)u.wd, ep, s, (const T*)zero_page, parity_dgrad);
    }
    timer.end(tp, s);
  }
  // the tail of a block's data gradient: gx = dgrad(u1) + the shortcut's gradient, gated by the ReLU `below` the block
  void block_input_dgrad(Block& blk, const T* below, hipStream_t s) {
    if (blk.down) {
      conv_dgrad(blk.u1, blk.gx, nullptr, s, below);  // gated here too: the projection launch below may only touch the even pixels
      conv_dgrad(blk.ud, blk.gx, blk.gx, s, below);   // accumulate the projection path in place, then gate
    } else {
      conv_dgrad(blk.u1, blk.gx, blk.gout, s, below);  // + identity path (already gated)
    }
  }
  void flush_wgrads(hipStream_t s) {
    if (pending_wgrads.empty()) return;
    hipStream_t ws = fork_wgrad(s);
    for (auto& p : pending_wgrads) conv_wgrad(*p.u, p.x, ws);
    pending_wgrads.clear();
  }
  // Every gradient w.r.t. a block OUTPUT is stored already multiplied by that block's ReLU gate (out > 0): its producer
  // -- the data gradient of the block above, or the average pool's backward for the last block -- applies the gate in
  // its epilogue (Epilogue::out_gate, reading its own input tensor), so bn2 / the projection's BatchNorm / the identity
  // path of this block use `gout` as it is and never read `out`.
  void block_backward(Block& blk, hipStream_t s) {
    // the gate of the block below = ReLU that produced this block's input (none below layer1.0: its input is the max-pool)
    // (fp16x2m: gates and the weight gradients' X operands are the HI halves of the h2 activations, read in place by the fp16
    //  kernels: conv_wgrad sets WgradArgs::x_h2, conv_dgrad Epilogue::gate_h2)
    const T* bx = blk.x;
    const T* ba1 = blk.a1;
    // (fp16x2m with the fp16 stem kernels: the gradient of the pooled stem activation leaves layer1.0 gated by that activation)
    const T* below = &blk == &blocks.front() ? (md.stem_bwd == STEM_TILES_ON_COPIES ? bx : nullptr) : bx;
    // (bn2 / the projection / the identity path take `gout` as stored: already gated)
    if (wgrad.sched == 2 || ((wgrad.defer_stages >> blk.stage) & 1)) {
      flush_wgrads(s);
      bn_bwd(blk.u2, blk.gout, s);
      conv_dgrad(blk.u2, blk.ga1, nullptr, s);
      pending_wgrads.push_back({&blk.u2, ba1});
      flush_wgrads(s);
      bn_bwd(blk.u1, blk.ga1, s, true);
      if (blk.down) bn_bwd(blk.ud, blk.gout, s);
      pending_wgrads.push_back({&blk.u1, bx});
      if (blk.down) pending_wgrads.push_back({&blk.ud, bx});
      block_input_dgrad(blk, below, s);
      return;
    }
    bn_bwd(blk.u2, blk.gout, s);
    // MN_WGRAD_TAIL = k: the weight gradients of the first k blocks of layer1 (the LAST k of the backward pass) are held back and
    // forked in front of the stem's backward kernels (backward_stage: flush_wgrads), which run alone on the step stream at the end of
    // the step and are VALU-bound -- the matrix pipe is idle under them.  Same stage, same gradient bucket.
    const bool tail = blk.stage == 0 && !blk.down && (int)(&blk - &blocks[0]) < wgrad_tail;
    const bool early = wgrad.sched == 1 && !tail && ((wgrad.early_stages >> blk.stage) & 1);
    if (early) conv_wgrad(blk.u2, ba1, fork_wgrad(s));
    conv_dgrad(blk.u2, blk.ga1, nullptr, s);
    bn_bwd(blk.u1, blk.ga1, s, true);
    if (blk.down) bn_bwd(blk.ud, blk.gout, s);
    if (tail) {
      pending_wgrads.push_back({&blk.u2, ba1});
      pending_wgrads.push_back({&blk.u1, bx});
    } else {
      hipStream_t ws = fork_wgrad(s);
      if (!early) conv_wgrad(blk.u2, ba1, ws);
      conv_wgrad(blk.u1, bx, ws);
      if (blk.down) conv_wgrad(blk.ud, bx, ws);
    }
    block_input_dgrad(blk, below, s);
  }
  void launch_head_wgrads(hipStream_t st) override {
    const int F = cfg.feat_dim;
    const float unscale = 1.f / cur_scale;
    launch_head_bwd_weight(dposes, feat, grads + L.xyz_w, grads + L.xyz_b, grads + L.wpqr_w, grads + L.wpqr_b, B, F, unscale,
                           cfg.filter_nans, st);
    // fc backward: weight + bias gradient in one launch of 32 x 32 tiles (dense.h)
    DenseWgradArgs dw;
    dw.dY = dz; dw.X = pooled; dw.dW = grads + L.fc_w; dw.db = grads + L.fc_b; dw.B = B; dw.F = F; dw.Cin = 512; dw.ldy = F;
    dw.ldx = 512; dw.ldw = 512; dw.alpha = unscale;
    launch_dense_wgrad(dw, st);
    head_wgrads_deferred = false;
  }
  // dpooled = dz * fc_w: 32 x 32 tiles with K split over the workgroup's waves (dense.h) where that form applies
  void fc_dgrad(hipStream_t s) {
    const int F = cfg.feat_dim;
    DenseArgs dd;
    dd.A = dz; dd.W = fcT; dd.bias = nullptr; dd.C = dpooled; dd.M = B; dd.N = 512; dd.K = F; dd.lda = F; dd.ldw = F; dd.ldc = 512;
    dd.relu = 0;
    Epilogue ep;
    ep.out = dpooled;
    ep.ldc = 512;
    if (dense_nt_applies(dd))
      launch_dense_nt(dd, s);
    else
      launch_igemm<float>(dense_geom(B, 512, F), (const float*)dz, (const float*)fcT, ep, s, (const float*)zero_page);
  }
  void head_backward(hipStream_t s) {
    const int F = cfg.feat_dim;
    if (!grads_zeroed) launch_zero_fill(grads, L.param_floats, s);  // optim.learner.zero_grad()
    grads_zeroed = false;
    run_criterion(poses, cur_targets, cur_loss, dposes, grads + L.crit, s);
    post_loss(cur_loss, s);
    launch_head_bwd_input(dposes, feat, params + L.xyz_w, params + L.wpqr_w, dz, B, F, cfg.filter_nans,
                          drop_this_step ? dropmask : nullptr, s);
    // The head's and the fc layer's WEIGHT gradients feed nothing downstream: with two streams they leave with the first fork of the
    // backward pass (fork_wgrad), off the chain criterion -> heads -> fc -> average pool -> layer4 (-0.02 ms, four of four
    // pairs, profiles/r06/c43_*)
    if (overlap_wgrad && s != nullptr && !timer.enabled)
      head_wgrads_deferred = true;
    else
      launch_head_wgrads(s);
    fc_dgrad(s);
    Block& last = blocks.back();
    if (md.f16_bwd_on_pairs())  // fp16 gradient out, gate = the hi halves of the last block's h2 output
      launch_avgpool_bwd<half>(dpooled, (half*)last.gout, B, Hl * Wl, 512, (const half*)last.out, 1, s);
    else if (md.pairs())
      launch_avgpool_bwd_h2(dpooled, (float*)last.gout, B, Hl * Wl, 512, (const half*)last.out, s);
    else
      launch_avgpool_bwd<T>(dpooled, last.gout, B, Hl * Wl, 512, last.out, 0, s);
  }
  void stem_backward(hipStream_t s) {
    float* const gamma = params + stem.bp.gamma;
    float* const beta = params + stem.bp.beta;
    if (md.stem_bwd != STEM_CHAIN) {
      const bool mx = md.stem_bwd == STEM_TILES_ON_COPIES;
      // two tile-walking launches (stem_bwd.h): BatchNorm sums, then the weight gradient with d(conv output) computed tile
      // by tile in LDS -- neither the max-pool's input gradient nor d(conv output) is stored
      StemBwdArgs a;
      a.y = mx ? (const half*)a0 : (const half*)stem.y; a.idx = pool_idx; a.gp = (const half*)gp0; a.gamma = gamma;
      a.beta = beta; a.coef = stem.coef_b; a.mean = stem.mean; a.invstd = stem.invstd; a.accum = stem.accum_b;
      a.accum_rows = stem.rows_b; a.xpad = mx ? (const half*)xpad16 : (const half*)xpad; a.dW = grads + stem.cp.w;
      a.colmap = stem_colmap; a.ldw = stem.ldw;
      a.alpha = 1.f / cur_scale;
      a.pre_gated = mx ? 1 : 0;
      launch_stem_bn_reduce(a, B, H, W, Wp, s);
      launch_bn_finalize_bwd(stem.accum_b, stem.M, gamma, stem.mean, stem.invstd, grads + stem.bp.gamma, grads + stem.bp.beta,
                             1.f / cur_scale, beta, stem.coef_b, 64, stem.rows_b, s);
      auto* tp = timer.begin(1, s);
      launch_stem_wgrad(a, B, H, W, Wp, s);
      timer.end(tp, s);
      return;
    }
    // the chain: BatchNorm backward with the stem's own ReLU gate recomputed from y, then the generic weight gradient
    const T* g = nullptr;
    PoolGradSrc pg;
    if (fuse_stem_bwd || md.pairs()) {  // (fp16x2: the stem's fp32 tensors make the materialised 1 GB gradient cost 0.5 ms per step)
      // the max-pool's input gradient is gathered from (argmax, pooled gradient) inside the BatchNorm backward
      // passes: neither the activation nor its gradient exists in memory
      pg.idx = pool_idx; pg.gout = gp0; pg.H = H0; pg.W = W0; pg.Po = H1; pg.Qo = W1;
      if (md.gx != md.y) {  // layer1.0's data gradient left gp0 in fp16: widened into ga0 (unused by the fused stem) for the fp32 chain
        launch_widen_f16((const half*)gp0, (float*)ga0, (long)B * H1 * W1 * 64, s);
        pg.gout = ga0;
      }
    } else {
      launch_maxpool_bwd<T>(pool_idx, gp0, ga0, B, H0, W0, 64, s);
      g = ga0;
    }
    launch_bn_bwd<T>(g, (const T*)nullptr, (const T*)stem.y, stem.M, 64, gamma, stem.mean, stem.invstd, grads + stem.bp.gamma,
                     grads + stem.bp.beta, stem.gy, stem.accum_b, stem.coef_b, 1.f / cur_scale, s, beta, pg, stem.rows_b);
    // The input gradient of the stem is not needed (nothing consumes it).  The weight gradient goes to the stream every
    // other weight gradient of the step runs on: they share the partial-tile / split-slice workspace (wgf_ws), and the
    // last layer1 launches forked a moment ago may still be using it (joined at the end of the stage).
    hipStream_t ws = fork_wgrad(s);
    auto* tp = timer.begin(1, ws);
    launch_wgrad<T>(wgrad_args(stem, xpad), wgrad_splits(stem), ws, zero_page);
    timer.end(tp, ws);
  }
  // ---- input gradient at inference (mn_input_grad) ---------------------------------------------------------------------
  // d(sum(cot * poses)) / d(images) in eval mode: the eval forward pass, then the data-gradient chain alone, on the step stream.
  // Against the training backward pass: BatchNorm is a per-channel scale (running statistics; bn_eval_bwd), there are no weight
  // gradients, no sums, no optimiser -- parameters, gradient arena, moments, buffers, counters, loss-scale state and acc_region
  // are not written -- and the chain ends in the stem's data gradient (stem_dgrad), which training never needs.
  void bn_eval_bwd(Unit& u, const T* g, const T* gate, bool recompute, hipStream_t s) {
    launch_bn_eval_bwd<T>(g, gate, (const float*)u.coef_f, recompute ? (const float*)(u.coef_f + u.cp.cout) : (const float*)nullptr,
                          u.gy, u.M, u.cp.cout, s);
  }
  int input_grad(const void* images, const float* cot, float* gx_out, float* sal_out, float* poses_out, hipStream_t s) override {
    if (md.pairs())
      return fail("mn_input_grad: supported dtypes are MN_DTYPE_F32, MN_DTYPE_F32X3 and MN_DTYPE_F16 (the fp16x2 / fp16x2m / fp16x2q "
                  "modes have no inference backward pass)");
    if (jitter_on())
      return fail("mn_input_grad: attention maps are taken on un-jittered frames; turn ColorJitter off (mn_set_color_jitter with all "
                  "ranges 0) for this call");
    if (!images || !gx_out) return fail("mn_input_grad: images and gx_out are required");
    if (int e = forward_impl(images, poses_out, 0, false, s)) return e;
    if (resize_on) images = rs_frames;  // the x of the saliency map: the frames the network saw
    else if (in_index) images = in_stage;
    const int F = cfg.feat_dim;
    hipMemsetAsync(ig_flag, 0, sizeof(float), s);
    launch_input_grad_seed(cot, dposes, B * 6, 1.f / (6.f * (float)B), cur_scale, s);
    launch_head_bwd_input(dposes, feat, params + L.xyz_w, params + L.wpqr_w, dz, B, F, cfg.filter_nans, nullptr, s);
    fc_dgrad(s);
    Block& last = blocks.back();
    launch_avgpool_bwd<T>(dpooled, last.gout, B, Hl * Wl, 512, last.out, 0, s);
    for (int i = (int)blocks.size() - 1; i >= 0; --i) {
      Block& blk = blocks[i];
      const T* below = i == 0 ? (const T*)nullptr : blk.x;  // (block_backward: the ReLU that produced this block's input)
      bn_eval_bwd(blk.u2, blk.gout, nullptr, false, s);
      conv_dgrad(blk.u2, blk.ga1, nullptr, s);
      bn_eval_bwd(blk.u1, blk.ga1, blk.a1, false, s);
      if (blk.down) bn_eval_bwd(blk.ud, blk.gout, nullptr, false, s);
      block_input_dgrad(blk, below, s);
    }
    launch_maxpool_bwd<T>(pool_idx, gp0, ga0, B, H0, W0, 64, s);
    // the fused BatchNorm + ReLU + max-pool pass never stored a0: the stem's gate is recomputed from y and coef_f
    if (fuse_stem)
      bn_eval_bwd(stem, ga0, stem.y, true, s);
    else
      bn_eval_bwd(stem, ga0, a0, false, s);
    launch_stem_dgrad<T>(stem.gy, (const float*)(params + stem.cp.w), gx_out, B, H, W, 1.f / cur_scale, ig_flag, s);
    if (sal_out)
      launch_saliency(gx_out, input_u8 ? (const float*)nullptr : (const float*)images,
                      input_u8 ? (const unsigned char*)images : (const unsigned char*)nullptr, input_norm, sal_out, sal_work, B, H, W,
                      s);
    return check_launch("input_grad");
  }

  int backward_stage(int stage, hipStream_t s) override {
    if (stage < 0 || stage > 3) return fail("backward_stage: stage must be 0..3");
    if (!cur_targets) return fail("backward_stage: call mn_train_forward_loss first");
    if (stage == 3) head_backward(s);
    for (int i = (int)blocks.size() - 1; i >= 0; --i)
      if (blocks[i].stage == stage) block_backward(blocks[i], s);
    if (stage == 0) {
      flush_wgrads(s);  // beside the stem's BatchNorm backward
      stem_backward(s);
    }
    flush_wgrads(s);
    if (head_wgrads_deferred) launch_head_wgrads(s);  // (no fork took them along)
    join_wgrad(s);  // the stage's gradient bucket is complete when this call's work on s is
    return check_launch("backward_stage");
  }

  float* grad_arena() override { return grads; }
  // ---- inspection (mn_debug_tensor): activations / gradients of the last step by name ---------------------------
  int debug_tensor(const char* name, void** ptr, int64_t* numel, int32_t* dtype) override {
    const std::string n(name);
    auto give = [&](const void* p, long count, int dt) {
      *ptr = const_cast<void*>(p);
      *numel = count;
      *dtype = dt;
      return 0;
    };
    const long n0 = (long)B * H0 * W0 * 64, n1 = (long)B * H1 * W1 * 64;
    const int AT = md.act, GT = md.gy, GD = md.gx;
    if (n == "xpad") return give(xpad, (long)B * Hp * Wp * 4, DT);
    if (n == "stem.y") return give(stem.y, n0, DT);
    if (n == "stem.gy") return give(stem.gy, n0, DT);
    if (n == "p0") return give(p0, n1, AT);
    if (n == "gp0") return give(gp0, n1, GD);
    if (n == "pooled") return give(pooled, (long)B * 512, MN_F32);
    if (n == "feat") return give(feat, (long)B * cfg.feat_dim, MN_F32);
    if (n == "poses") return give(poses, (long)B * 6, MN_F32);
    if (n == "dposes") return give(dposes, (long)B * 6, MN_F32);
    if (n == "dz") return give(dz, (long)B * cfg.feat_dim, MN_F32);
    if (n == "dpooled") return give(dpooled, (long)B * 512, MN_F32);
    if (n == "dropmask") return give(dropmask, (long)B * cfg.feat_dim, MN_F32);
    if (n == "jitter") return give(jit_draws, (long)B * 8, MN_F32);
    if (n == "input_grad_nonfinite") return give(ig_flag, 1, MN_F32);
    if (n == "input_index_bad") return give(index_flag(), 1, MN_F32);
    if (n.size() > 2 && n[0] == 'b') {  // "b<block>.<tensor>", blocks numbered 0..15 in network order
      const size_t dot = n.find('.');
      if (dot != std::string::npos) {
        const int bi = atoi(n.substr(1, dot - 1).c_str());
        const std::string t = n.substr(dot + 1);
        if (bi >= 0 && bi < (int)blocks.size()) {
          Block& k = blocks[bi];
          const long no = k.u2.M * k.u2.cp.cout;
          if (t == "y1") return give(k.u1.y, no, DT);
          if (t == "a1") return give(k.a1, no, AT);
          if (t == "y2") return give(k.u2.y, no, DT);
          if (t == "out") return give(k.out, no, AT);
          if (t == "gy1") return give(k.u1.gy, no, GT);
          if (t == "ga1") return give(k.ga1, no, GD);
          if (t == "gy2") return give(k.u2.gy, no, GT);
          if (t == "gout") return give(k.gout, no, GD);
          if (k.down && t == "yd") return give(k.ud.y, no, DT);
          if (k.down && t == "zd") return give(k.zd, no, AT);
          if (k.down && t == "gyd") return give(k.ud.gy, no, GT);
        }
      }
    }
    return fail("mn_debug_tensor: unknown tensor '" + n + "'");
  }

  // ---- optimiser -----------------------------------------------------------------------------------
  // host-side effects of an optimiser step
  void after_optim_host() override {
    step += 1;
    weights_dirty = true;
  }
  int sync_step_to_device(hipStream_t s) override {
    long long v = step;
    hipMemcpyAsync(step_dev, &v, sizeof(v), hipMemcpyHostToDevice, s);
    hipStreamSynchronize(s);
    return check_launch("sync_step");
  }
  int64_t applied_steps() override {
    long long v = 0;
    hipDeviceSynchronize();
    if (hipMemcpy(&v, step_dev, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
  }
  int optim_step(float grad_mul, hipStream_t s) override {
    // squared gradient norm: for clip_grad_norm, and (fp16) as the overflow detector of this step
    if (max_grad_norm > 0.f || md.overflow_guard) {
      // (MN_DETERMINISTIC: per-workgroup partial sums, folded in index order)
      double* const partials = deterministic && sqnorm_grid(L.model_floats) <= kSqPartials ? sq_partials : nullptr;
      if (!partials) {
        if (!sqnorm_clean) hipMemsetAsync(sqnorm, 0, sizeof(double), s);  // (a second optimiser step on one forward pass)
        sqnorm_clean = false;
      }
      launch_grad_sqnorm(grads, L.model_floats, sqnorm, partials, s);
    }
    attempts += 1;
    launch_adam_prep(step_dev, beta1, beta2, bc_dev, sqnorm, md.overflow_guard ? overflow_dev : nullptr, attempts, s);
    AdamArgs a;
    a.p = params; a.g = grads; a.m = m1; a.v = m2; a.n = L.param_floats; a.n_clip = L.model_floats; a.lr = lr; a.wd = wd;
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.bc1 = 1.f; a.bc2 = 1.f; a.bc_dev = bc_dev;
    a.grad_mul = grad_mul; a.max_norm = max_grad_norm; a.sqnorm = sqnorm; a.frozen = frozen; a.eps_mode = cfg.eps_mode;
    a.skip = md.overflow_guard ? overflow_dev : nullptr;
    a.method = optim_method; a.nesterov = nesterov;
    launch_adam(a, s);
    if (md.overflow_guard && overflow_host)
      hipMemcpyAsync(overflow_host, overflow_dev, 4 * sizeof(long long), hipMemcpyDeviceToHost, s);
    return check_launch("optim_step");
  }
};

// the storage type T is the only thing chosen here: what else a dtype means is Plan::mode_of's
std::unique_ptr<PlanBase> make_plan(const mn_config& cfg) {
  if (cfg.dtype == MN_DTYPE_F16) return std::unique_ptr<PlanBase>(new Plan<half>(cfg));
  return std::unique_ptr<PlanBase>(new Plan<float>(cfg));
}

}  // namespace

struct mn_handle {
  std::unique_ptr<PlanBase> plan;
};

static int validate(const mn_config* c) {
  if (!c) return fail("null config");
  if (c->mode < 0 || c->mode > 3) return fail("config: bad mode");
  if (c->dtype != MN_DTYPE_F32 && c->dtype != MN_DTYPE_F16 && c->dtype != MN_DTYPE_F32X3 && c->dtype != MN_DTYPE_F16X2 &&
      c->dtype != MN_DTYPE_F16X2M && c->dtype != MN_DTYPE_F16X2Q)
    return fail("config: bad dtype");
  if (c->windows < 1 || c->T < 1 || c->T > kMaxT) return fail("config: windows >= 1 and 1 <= T <= 8 required");
  if (c->mode == MN_MODE_POSENET && c->T != 1) return fail("config: PoseNet mode requires T = 1");
  if (c->mode >= MN_MODE_MAPNET && c->T < 2) return fail("config: MapNet modes require T >= 2");
  if (c->H < 32 || c->W < 32) return fail("config: image must be at least 32x32");
  if (c->feat_dim < 64 || c->feat_dim % 64 != 0) return fail("config: feat_dim must be a multiple of 64");
  if (!(c->loss_scale > 0.f)) return fail("config: loss_scale must be positive");
  {  // the largest activation (stem output, NHWC) must stay below the 4 GiB a 32-bit buffer offset spans
    const long frames = frames_per_window(c->mode, c->T);
    const long px = ((c->H - 1) / 2 + 1) * (long)((c->W - 1) / 2 + 1);
    if (c->windows * frames * px * 64 * (c->dtype == MN_DTYPE_F16 ? 2 : 4) >= 0xfffffff0l)
      return fail("config: batch too large (an activation tensor would exceed 4 GiB); split the batch");
  }
  return 0;
}

extern "C" int64_t mn_plan_bytes(const mn_config* cfg) {
  if (validate(cfg)) return -1;
  load_knobs();
  return (int64_t)make_plan(*cfg)->carve(nullptr);
}

extern "C" mn_handle* mn_create(const mn_config* cfg, float* params, float* opt_state, void* buffers, void* work,
                                void* stream) {
  if (validate(cfg)) return nullptr;
  if (!params || !opt_state || !buffers || !work) {
    fail("mn_create: null arena");
    return nullptr;
  }
  mn_handle* h = new mn_handle();
  begin_call();
  load_knobs();
  h->plan = make_plan(*cfg);
  if (h->plan->attach(params, opt_state, buffers, work, (hipStream_t)stream)) {
    delete h;
    return nullptr;
  }
  return h;
}
extern "C" void mn_destroy(mn_handle* h) { delete h; }

#define MN_H(h)                                       \
  if (!(h) || !(h)->plan) return fail("null handle"); \
  begin_call();                                       \
  PlanBase& P = *(h)->plan;

extern "C" int mn_set_learn_flags(mn_handle* h, int learn_beta, int learn_gamma) {
  MN_H(h);
  P.learn_beta = learn_beta;
  P.learn_gamma = learn_gamma;
  P.update_frozen(nullptr);
  return 0;
}
extern "C" int mn_set_loss_fn(mn_handle* h, int t_kind, float t_param, int q_kind, float q_param) {
  MN_H(h);
  if (const char* why = loss_fn_error(t_kind, t_param, q_kind, q_param)) return fail(std::string("mn_set_loss_fn: ") + why);
  P.t_kind = t_kind;
  P.t_param = t_param;
  P.q_kind = q_kind;
  P.q_param = q_param;
  return 0;
}
extern "C" int mn_set_optim(mn_handle* h, float lr, float weight_decay, float beta1, float beta2, float eps,
                            float max_grad_norm) {
  MN_H(h);
  P.lr = lr; P.wd = weight_decay; P.beta1 = beta1; P.beta2 = beta2; P.eps = eps; P.max_grad_norm = max_grad_norm;
  return 0;
}
extern "C" int mn_set_optim_method(mn_handle* h, int method, int nesterov) {
  MN_H(h);
  if (method < 0 || method > 2) return fail("set_optim_method: method must be 0 (adam), 1 (sgd) or 2 (rmsprop)");
  P.optim_method = method;
  P.nesterov = nesterov ? 1 : 0;
  return 0;
}
extern "C" int mn_set_step_count(mn_handle* h, int64_t step) {
  MN_H(h);
  // steps still in flight on the caller's (non-blocking) stream increment the device counter in adam_prep_kernel: let them
  // finish before the counter is overwritten through the NULL stream
  if (hipDeviceSynchronize() != hipSuccess) return check_launch("set_step_count");
  P.step = step;
  return P.sync_step_to_device(nullptr);
}
extern "C" int64_t mn_get_step_count(mn_handle* h) { return (h && h->plan) ? h->plan->applied_steps() : -1; }
extern "C" int mn_set_loss_host(mn_handle* h, float* pinned_host) {
  MN_H(h);
  P.loss_host = pinned_host;
  P.loss_pending = false;
  return 0;
}
extern "C" int mn_wait_loss(mn_handle* h) {
  if (!h || !h->plan) return -1;
  PlanBase& P = *h->plan;
  if (!P.loss_pending) return 1;  // nothing was posted (default stream): read the device scalar instead
  P.loss_pending = false;
  if (hipEventSynchronize(P.loss_event) != hipSuccess) {
    (void)hipGetLastError();
    return 1;
  }
  return 0;
}
extern "C" int mn_debug_tensor(mn_handle* h, const char* name, void** ptr, int64_t* numel, int32_t* dtype) {
  MN_H(h);
  if (!name || !ptr || !numel || !dtype) return fail("mn_debug_tensor: null argument");
  return P.debug_tensor(name, ptr, numel, dtype);
}
extern "C" int mn_get_loss_scale(mn_handle* h, float* scale, int64_t* skipped_steps) {
  MN_H(h);
  if (scale) *scale = P.cur_scale;
  if (skipped_steps) *skipped_steps = P.overflow_host ? (int64_t) * (volatile long long*)(P.overflow_host + 1) : 0;
  return 0;
}
extern "C" int64_t mn_stuck_overflow_steps(mn_handle* h) { return (h && h->plan) ? h->plan->stuck_skips : -1; }
extern "C" int mn_set_loss_scale(mn_handle* h, float scale, int growth_interval) {
  MN_H(h);
  if (!(scale > 0.f)) return fail("mn_set_loss_scale: scale must be positive");
  if (!P.scales_loss && scale != 1.f)
    return fail("mn_set_loss_scale: fp32 plans do not scale the loss");
  P.cur_scale = scale;
  P.scale_set_at = P.attempts;
  P.scale_growth_interval = growth_interval;
  P.clean_steps = 0;
  P.stuck_skips = 0;
  if (P.overflow_host) {  // skips of steps still in flight belong to the old scale: do not halve the new one for them
    hipDeviceSynchronize();
    P.skipped_seen = *(volatile long long*)(P.overflow_host + 1);
    P.done_seen = *(volatile long long*)(P.overflow_host + 3);
  }
  return 0;
}
extern "C" int mn_set_dropout(mn_handle* h, float p, uint64_t seed) {
  MN_H(h);
  if (!(p >= 0.f && p < 1.f)) return fail("mn_set_dropout: 0 <= p < 1 required");
  P.drop_p = p;
  P.drop_seed = seed;
  P.drop_calls = 0;
  return 0;
}
extern "C" int mn_set_dropout_calls(mn_handle* h, uint32_t calls) {
  MN_H(h);
  P.drop_calls = calls;
  return 0;
}
extern "C" int mn_set_input_u8(mn_handle* h, int enable, const float* mean, const float* std) {
  MN_H(h);
  if (enable && (!mean || !std)) return fail("mn_set_input_u8: mean and std (3 floats each, host memory) are required");
  if (enable)
    for (int c = 0; c < 3; ++c) {
      if (!(std[c] > 0.f)) return fail("mn_set_input_u8: std must be positive");
      P.input_norm.scale[c] = 1.f / (255.f * std[c]);
      P.input_norm.shift[c] = -mean[c] / std[c];
      P.jitter_norm.scale[c] = 1.f / std[c];
      P.jitter_norm.shift[c] = -mean[c] / std[c];
    }
  P.input_u8 = enable != 0;
  return 0;
}
extern "C" int mn_set_color_jitter(mn_handle* h, float brightness, float contrast, float saturation, float hue, uint64_t seed) {
  MN_H(h);
  const float v[4] = {brightness, contrast, saturation, hue};
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(v[k]) || !(v[k] >= 0.f))
      return fail("mn_set_color_jitter: brightness, contrast, saturation and hue must be finite and >= 0");
  if (!(hue <= 0.5f)) return fail("mn_set_color_jitter: 0 <= hue <= 0.5 required");
  for (int k = 0; k < 4; ++k) P.jit_range[k] = v[k];
  P.jit_seed = seed;
  P.jit_calls = 0;
  return 0;
}
static int resize_images(const mn_config* c) { return c->windows * frames_per_window(c->mode, c->T); }
extern "C" int64_t mn_input_resize_bytes(const mn_config* cfg, int src_h, int src_w) {
  if (validate(cfg)) return -1;
  if (src_h < 1 || src_w < 1) {
    fail("mn_input_resize_bytes: the source size must be positive");
    return -1;
  }
  return resize_frames_bytes(resize_images(cfg), cfg->H, cfg->W) + resize_table_bytes(src_h, src_w, cfg->H, cfg->W);
}
extern "C" int mn_set_input_resize(mn_handle* h, int src_h, int src_w, void* work, int64_t work_bytes) {
  MN_H(h);
  if (src_h == 0 && src_w == 0) {
    P.resize_on = false;
    P.rs_frames = nullptr;
    return 0;
  }
  if (src_h < 1 || src_w < 1) return fail("mn_set_input_resize: the source size must be positive (0, 0 turns the resize off)");
  if (!work) return fail("mn_set_input_resize: work (device memory of mn_input_resize_bytes) is required");
  if (((uintptr_t)work & 3) != 0) return fail("mn_set_input_resize: work must be 4-byte aligned");
  const int64_t frames = resize_frames_bytes(resize_images(&P.cfg), P.cfg.H, P.cfg.W);
  const int64_t need = frames + resize_table_bytes(src_h, src_w, P.cfg.H, P.cfg.W);
  if (work_bytes < need)
    return fail("mn_set_input_resize: work holds " + std::to_string((long long)work_bytes) + " bytes, mn_input_resize_bytes asks for " +
                std::to_string((long long)need));
  const ResizePlan rp = resize_plan(resize_images(&P.cfg), src_h, src_w, P.cfg.H, P.cfg.W, (int*)((unsigned char*)work + frames));
  if (!rp.error.empty()) return fail("mn_set_input_resize: " + rp.error);
  // passes in flight may still read the tables of an earlier setting in the same buffer
  if (hipDeviceSynchronize() != hipSuccess) return check_launch("set_input_resize");
  if (hipMemcpy((unsigned char*)work + frames, rp.tables.data(), rp.tables.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
    return check_launch("set_input_resize");
  P.rs_geom = rp.g;
  P.rs_frames = (unsigned char*)work;
  P.resize_on = true;
  return 0;
}
extern "C" int64_t mn_input_index_bytes(const mn_config* cfg, int input_u8) {
  if (validate(cfg)) return -1;
  return (int64_t)resize_images(cfg) * 3 * cfg->H * cfg->W * (input_u8 ? 1 : 4);
}
extern "C" int mn_set_input_index(mn_handle* h, const int32_t* index_dev, int64_t store_frames, void* work, int64_t work_bytes) {
  MN_H(h);
  if (!index_dev) {
    P.in_index = nullptr;
    P.in_store_frames = 0;
    P.in_stage = nullptr;
    P.in_stage_bytes = 0;
    return 0;
  }
  if (((uintptr_t)index_dev & 3) != 0) return fail("mn_set_input_index: index_dev must be 4-byte aligned (device int32 [images])");
  if (store_frames < 1) return fail("mn_set_input_index: store_frames must be at least 1");
  if (resize_images(&P.cfg) > 65535) return fail("mn_set_input_index: at most 65535 frames per pass (the gather's grid)");
  if (!P.resize_on) {  // (with the resize on the resample reads the store itself: no staging)
    const int64_t need = mn_input_index_bytes(&P.cfg, P.input_u8 ? 1 : 0);
    if (!work) return fail("mn_set_input_index: work (device memory of mn_input_index_bytes) is required");
    if (work_bytes < need)
      return fail("mn_set_input_index: work holds " + std::to_string((long long)work_bytes) + " bytes, mn_input_index_bytes asks for " +
                  std::to_string((long long)need));
  }
  P.in_index = index_dev;
  P.in_store_frames = store_frames;
  P.in_stage = P.resize_on ? nullptr : (unsigned char*)work;
  P.in_stage_bytes = P.resize_on ? 0 : work_bytes;
  return 0;
}
extern "C" int mn_set_color_jitter_calls(mn_handle* h, uint32_t calls) {
  MN_H(h);
  P.jit_calls = calls;
  return 0;
}
extern "C" int mn_set_eval_fused(mn_handle* h, int enable) {
  MN_H(h);
  if (enable) {
    const std::string why = P.eval_fused_refusal();
    if (!why.empty()) return fail("mn_set_eval_fused: " + why);
  }
  P.eval_fused = enable != 0;
  return 0;
}
extern "C" int mn_forward(mn_handle* h, const void* images, float* poses_out, int training, void* stream) {
  MN_H(h);
  return P.forward(images, poses_out, training, (hipStream_t)stream);
}
extern "C" int mn_input_grad(mn_handle* h, const void* images, const float* cot, float* gx_out, float* saliency_out, float* poses_out,
                             void* stream) {
  MN_H(h);
  return P.input_grad(images, cot, gx_out, saliency_out, poses_out, (hipStream_t)stream);
}
extern "C" int mn_loss(mn_handle* h, const float* pred, const float* targ, float* loss_out, void* stream) {
  MN_H(h);
  return P.loss_only(pred, targ, loss_out, (hipStream_t)stream);
}
extern "C" int mn_train_forward_loss(mn_handle* h, const void* images, const float* targets, float* loss_out,
                                     float* poses_out, void* stream) {
  MN_H(h);
  P.timer.reset();
  hipStream_t s = (hipStream_t)stream;
  P.weights_dirty = true;  // a training forward always follows an optimiser step or a parameter load
  P.poll_overflow();
  return P.forward_loss(images, targets, loss_out, poses_out, s);
}
extern "C" int mn_train_backward_stage(mn_handle* h, int stage, void* stream) {
  MN_H(h);
  if (stage < 0 || stage > 3) return fail("backward_stage: stage must be 0..3");
  hipStream_t s = (hipStream_t)stream;
  return P.backward_stage(stage, s);
}
extern "C" int mn_grad_bucket(mn_handle* h, int stage, int64_t* offset, int64_t* count) {
  MN_H(h);
  if (stage < 0 || stage > 3) return fail("mn_grad_bucket: stage must be 0..3");
  *offset = P.L.stage_begin[stage];
  *count = P.L.stage_end[stage] - P.L.stage_begin[stage];
  return 0;
}
extern "C" int mn_grad_bucket_pack_bf16(mn_handle* h, int stage, void* out_bf16, void* stream) {
  MN_H(h);
  if (stage < 0 || stage > 3 || !out_bf16) return fail("mn_grad_bucket_pack_bf16: stage 0..3 and an output buffer are required");
  const long off = P.L.stage_begin[stage], n = P.L.stage_end[stage] - off;
  launch_grad_pack_bf16(P.grad_arena() + off, (__bf16*)out_bf16, n, (hipStream_t)stream);
  return check_launch("grad_bucket_pack_bf16");
}
extern "C" int mn_grad_bucket_unpack_bf16(mn_handle* h, int stage, const void* in_bf16, void* stream) {
  MN_H(h);
  if (stage < 0 || stage > 3 || !in_bf16) return fail("mn_grad_bucket_unpack_bf16: stage 0..3 and an input buffer are required");
  const long off = P.L.stage_begin[stage], n = P.L.stage_end[stage] - off;
  launch_grad_unpack_bf16((const __bf16*)in_bf16, P.grad_arena() + off, n, (hipStream_t)stream);
  return check_launch("grad_bucket_unpack_bf16");
}
extern "C" int mn_optim_step(mn_handle* h, float grad_mul, void* stream) {
  MN_H(h);
  hipStream_t s = (hipStream_t)stream;
  int rc = P.optim_step(grad_mul, s);
  if (rc == 0) P.after_optim_host();
  return rc;
}
extern "C" int mn_train_step(mn_handle* h, const void* images, const float* targets, float* loss_out, float* poses_out,
                             void* stream) {
  MN_H(h);
  hipStream_t s = (hipStream_t)stream;
  P.timer.reset();
  P.weights_dirty = true;  // a training step always follows an optimiser step or a parameter load
  P.poll_overflow();
  auto* tp = P.timer.begin(3, s);
  int rc = P.forward_loss(images, targets, loss_out, poses_out, s);
  for (int st = 3; st >= 0 && rc == 0; --st) rc = P.backward_stage(st, s);
  if (rc == 0) rc = P.optim_step(1.f, s);
  P.timer.end(tp, s);
  if (rc == 0) P.after_optim_host();
  return rc;
}
extern "C" int mn_params_changed(mn_handle* h) {
  MN_H(h);
  P.weights_dirty = true;
  return 0;
}
extern "C" int mn_set_profiling(mn_handle* h, int enable) {
  MN_H(h);
  P.timer.enabled = enable != 0;
  P.timer.reset();
  return 0;
}
extern "C" int mn_last_kernel_ms(mn_handle* h, int which, float* ms, int* launches) {
  MN_H(h);
  if (which < 0 || which > 3) return fail("mn_last_kernel_ms: which must be 0..3");
  P.timer.collect();
  if (which == 0) {
    *ms = P.timer.ms[0] + P.timer.ms[1];
    *launches = P.timer.launches[0] + P.timer.launches[1];
  } else if (which == 1) {
    *ms = P.timer.ms[0];
    *launches = P.timer.launches[0];
  } else if (which == 2) {
    *ms = P.timer.ms[1];
    *launches = P.timer.launches[1];
  } else {
    *ms = P.timer.ms[3];
    *launches = P.timer.launches[3];
  }
  return 0;
}
