// Every MN_* environment variable the library reads, in one table.  This header is the only place in csrc/ that touches the
// environment; it is plain host C++ (the emulator build of tests/emu compiles it unchanged).
//
// Read rule: load_knobs() fills the table from the environment at plan creation (mn_plan_bytes, mn_create) and at the entry of every
// stand-alone mn_op_* call -- nowhere else.  A Plan copies the plan-level knobs it needs when it is constructed; launch helpers read
// the launch-level ones from knobs() at every launch.  mn_train_step / mn_forward / mn_train_backward_stage / mn_optim_step never
// touch the environment.  So a caller that sets a variable and then creates a plan or calls an operator gets that value, whatever
// ran earlier in the process.  The table is process-wide: creating a second plan under a changed environment also changes the
// launch-level knobs (the second block below) for plans that already exist.  load_knobs() is not synchronised; concurrent loads
// write the same values.
//
// Knobs whose A/B is finished and lost are not here: their defaults are constants at the use sites, with the measurement beside them.
#pragma once
#include <stdlib.h>

namespace mn {

constexpr int kKnobUnset = -0x7fffffff;  // an int knob whose default depends on the plan's mode (resolve_wgrad_schedule)

struct Knobs {
  // ---- plan level: copied by a Plan at construction -------------------------------------------------------------------------
  // MN_DETERMINISTIC=1: bit-reproducible training steps (every sum in a scheduling-independent order)
  bool deterministic = false;
  // MN_FUSE_STEM: bit 0 = BatchNorm + ReLU + max-pool in one forward pass (-0.15 ms/step); bit 1 = max-pool gradient gathered inside
  // the BatchNorm backward passes instead of a maxpool_bwd launch (+0.05 ms/step: the gather runs twice) -- off
  int fuse_stem = 1;
  // MN_WGRAD_STREAM=0: weight gradients on the main stream instead of the side stream (profiling tools: one stream to attribute)
  bool wgrad_stream = true;
  // MN_EARLY_FORK=0: weight-gradient schedule 0 whatever the mode (one fork per block)
  bool early_fork = true;
  // MN_WGRAD_SCHED: 0 = one fork per block, after its last BatchNorm backward; 1 = each weight gradient forked as soon as its dY
  // exists; 2 = deferred: queued and forked right before the NEXT BatchNorm-backward pass of the main stream.  Per-mode default and
  // its measurements: resolve_wgrad_schedule
  int wgrad_sched = kKnobUnset;
  // MN_WGRAD_EARLY_STAGES: bit k = schedule 1's early fork applies to stage k (else schedule 0's order there).  Per-mode default:
  // resolve_wgrad_schedule.  Kept: the best mask depends on which data-gradient shapes a batch size selects (profiles/r06/c35_to_c37_*)
  int wgrad_early_stages = kKnobUnset;
  // MN_WGRAD_DEFER_STAGES: bit k = stage k takes schedule 2's order whatever the plan's schedule is.  Per-mode default:
  // resolve_wgrad_schedule.  Kept for the same reason (profiles/r06/c38_to_c40_*)
  int wgrad_defer_stages = kKnobUnset;
  // MN_WGRAD_TAIL (block_backward): fp16x2m 0 -> 1: -0.04 ... -0.10 ms in six of six pairs (18.37 -> 18.31), 2: equal, 3: +0.06;
  // fp16 12.78 -> 12.73 (profiles/r06/c29_to_c32_*)
  int wgrad_tail = 1;
  // MN_SCALE_GROWTH: clean steps after which the fp16 loss scale doubles (0 = never); configuration, also mn_set_loss_scale
  int scale_growth = 2000;

  // ---- launch level: read by the launch helpers at every launch ----------------------------------------------------------------
  // MN_IGEMM_CONFIG=1|8|12 forces one tile configuration of igemm.h (0 = per shape); parity tests run the 12-wave tile with it
  int igemm_config = 0;
  // MN_IGEMM_HALO: 0 = the generic kernel for every shape, 1 = igemm_halo.h's 256-column shape (layer3), 2 = + its 128-column shapes
  // (layers 2 and 4).  Whole step 17.34 / 17.03 / 16.79 ms for 0 / 1 / 2 (round 2, same box); parity tests set 0 and 1
  int igemm_halo = 2;
  // MN_HALO384: igemm_halo.h's 8-wave 384-row tile: 0 never, 1 by tile count, 2 always (parity tests); profiles/r04/c28_*
  int halo384 = 1;
  // MN_HALO_A1: igemm_halo.h's 4-wave 192-row tile, two workgroups per CU: 0 off, 1 by tile count, 2 always (parity tests);
  // profiles/r04/c30_*
  int halo_a1 = 1;
  // MN_H2_HALO256=1: the 256-column h2 shape whatever the tile count (parity tests on small problems)
  bool h2_halo256 = false;
  // MN_WGRAD_FUSED=0: the plain-GEMM weight gradient for the shapes wgrad_fused.h covers (tests of the kernels it replaced)
  bool wgrad_fused = true;
  // MN_STEM_WGS: persistent workgroups of the stem kernels (stem.h, stem_bwd.h); 0 = each launch's own default (stem.h 512,
  // stem_bwd.h one or two per CU).  Tests set 3 so that every workgroup walks several tiles
  int stem_wgs = 0;
  // MN_HALO_PP_WGS / MN_HALO_H2_WGS: persistent workgroups of halo_pp.h / halo_h2.h: one per CU of the MI355X; configuration for a
  // part with another CU count
  int halo_pp_wgs = 256;
  int halo_h2_wgs = 256;

#ifdef MN_ABLATION_BUILD
  // ---- timing-experiment build only (make ablation; results are wrong by construction) -----------------------------------------
  int ablate = 0;              // MN_ABLATE: igemm.h kernels with parts of the main loop removed
  int wgf_ablate = 0;          // MN_WGF_ABLATE: wgrad_fused.h
  int halo_ablate = 0;         // MN_HALO_ABLATE: igemm_halo.h
  int halo_pp_ablate = 0;      // MN_HALO_PP_ABLATE: halo_pp.h
  int halo_h2_ablate = 0;      // MN_HALO_H2_ABLATE: halo_h2.h
  int abl_skip_finalize = 0;   // MN_ABL_SKIP_FINALIZE=c: no BatchNorm finalize launches for units of at most c channels after warm-up
  bool abl_skip_wgf = false;   // MN_ABL_SKIP_WGF (present): the step without the fused weight gradients
  bool wgf_skip_reduce = false;  // MN_WGF_SKIP_REDUCE (present): the step without their reduce launches
#endif
};

namespace knob_env {  // the three forms in use
inline int integer(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline bool on_unless_0(const char* name) { return integer(name, 1) != 0; }
inline bool present(const char* name) { return getenv(name) != nullptr; }
}  // namespace knob_env

inline Knobs& knobs_storage() {
  static Knobs k;
  return k;
}
inline const Knobs& knobs() { return knobs_storage(); }

inline void load_knobs() {
  using namespace knob_env;
  Knobs k;
  k.deterministic = integer("MN_DETERMINISTIC", 0) != 0;
  k.fuse_stem = integer("MN_FUSE_STEM", k.fuse_stem);
  k.wgrad_stream = on_unless_0("MN_WGRAD_STREAM");
  k.early_fork = on_unless_0("MN_EARLY_FORK");
  k.wgrad_sched = integer("MN_WGRAD_SCHED", kKnobUnset);
  k.wgrad_early_stages = integer("MN_WGRAD_EARLY_STAGES", kKnobUnset);
  k.wgrad_defer_stages = integer("MN_WGRAD_DEFER_STAGES", kKnobUnset);
  k.wgrad_tail = integer("MN_WGRAD_TAIL", k.wgrad_tail);
  k.scale_growth = integer("MN_SCALE_GROWTH", k.scale_growth);
  k.igemm_config = integer("MN_IGEMM_CONFIG", k.igemm_config);
  k.igemm_halo = integer("MN_IGEMM_HALO", k.igemm_halo);
  k.halo384 = integer("MN_HALO384", k.halo384);
  k.halo_a1 = integer("MN_HALO_A1", k.halo_a1);
  k.h2_halo256 = integer("MN_H2_HALO256", 0) != 0;
  k.wgrad_fused = on_unless_0("MN_WGRAD_FUSED");
  k.stem_wgs = integer("MN_STEM_WGS", k.stem_wgs);
  k.halo_pp_wgs = integer("MN_HALO_PP_WGS", k.halo_pp_wgs);
  k.halo_h2_wgs = integer("MN_HALO_H2_WGS", k.halo_h2_wgs);
#ifdef MN_ABLATION_BUILD
  k.ablate = integer("MN_ABLATE", 0);
  k.wgf_ablate = integer("MN_WGF_ABLATE", 0);
  k.halo_ablate = integer("MN_HALO_ABLATE", 0);
  k.halo_pp_ablate = integer("MN_HALO_PP_ABLATE", 0);
  k.halo_h2_ablate = integer("MN_HALO_H2_ABLATE", 0);
  k.abl_skip_finalize = integer("MN_ABL_SKIP_FINALIZE", 0);
  k.abl_skip_wgf = present("MN_ABL_SKIP_WGF");
  k.wgf_skip_reduce = present("MN_WGF_SKIP_REDUCE");
#endif
  knobs_storage() = k;
}

// The weight-gradient schedule of a plan: what the environment sets, else the measured default of the plan's mode.
//   mode                          sched   early stages   defer stages
//   fp16                            1          13              2        13.10 -> 13.00 ms, four of four pairs (profiles/r06/c52_to_c54_*)
//   fp16x2                          1          15              0        28.60 / 28.02 / 28.38 ms for 2 / 1 / 0 (profiles/r04/c43_*)
//   fp16x2m, fp16x2q                1          13              2        18.96 / 19.02 / 19.15 ms for 1 / 0 / 2 (profiles/r06/c6_*); stages:
//                                                                       18.61 -> 18.55 (early 13: every stage but layer2, whose data
//                                                                       gradients run in the 70 KB two-workgroup form) and 18.25 -> 18.20
//                                                                       ms (defer 2: layer2), six of six pairs each (c35_to_c40_*)
//   fp32, fp32x3                    2          15              0        round 2: 16.44 / 16.05 / 16.01 ms for 1 / 0 / 2; not re-measured
//   any mode, MN_EARLY_FORK=0       0
// Round 2's fused weight gradient (one 512-thread, 96 KB workgroup per CU) did not share a CU with a data-gradient workgroup and
// preferred 2; since its low-register forms (round 4: 134 / 150 registers, 64 KB of LDS) BatchNorm waves fit beside it and the
// fp16 family prefers the early fork.
struct WgradSchedule {
  int sched, early_stages, defer_stages;
};
// f16_family: fp16, fp16x2, fp16x2m, fp16x2q; per_stage: fp16, fp16x2m, fp16x2q
inline WgradSchedule resolve_wgrad_schedule(const Knobs& k, bool f16_family, bool per_stage) {
  WgradSchedule r;
  r.sched = k.wgrad_sched != kKnobUnset ? k.wgrad_sched : !k.early_fork ? 0 : f16_family ? 1 : 2;
  r.early_stages = k.wgrad_early_stages != kKnobUnset ? k.wgrad_early_stages : per_stage ? 13 : 15;
  r.defer_stages = k.wgrad_defer_stages != kKnobUnset ? k.wgrad_defer_stages : per_stage ? 2 : 0;
  return r;
}

}  // namespace mn
