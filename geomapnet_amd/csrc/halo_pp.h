// 3x3 stride-1 convolution of 64 -> 64 channel fp16 tensors (ResNet layer1, forward and data gradient) with the input tile
// staged ONCE in LDS, as a persistent "ping-pong" kernel.
//
//   out[b, y, x, n] = sum_{r, s, c} in[b, y + rsign*r + off_h, x + ssign*s + off_w, c] * Bw[n][(r*3 + s)*64 + c]
//
// (GatherGeom conventions of igemm.h: forward rsign = +1, off = -pad; data gradient rsign = -1, off = +pad.)
//
// Why not igemm.h: the implicit-GEMM kernel fetches every tap of every K-step through the LDS-DMA path -- for C = N = 64
// that is 221 KB per 128-pixel tile (nine shifted copies of the same 128 input rows + the 74 KB weight matrix) and the
// launch runs at the ~20 B/clk/CU that path sustains (159 us for 270 MB of tensors, MFMA pipe 21 % busy).  A workgroup
// that owns a 16x16-pixel output tile loads its 18x18-pixel input halo (41 KB) once and walks the nine taps as ADDRESS
// OFFSETS into that LDS image.  The first form of this idea (rounds 1-2, "halo.h", removed in round 3) ran one tile per
// 4-wave workgroup: halo DMA -> wait -> nine taps with a barrier each (the tap's weight slice streamed through a two-slot
// ring) -> epilogue through an LDS staging block.  Its ablations (profiles/r02) showed the three phases ADD: a CU held two
// such workgroups and they drifted into the same phase, so the matrix pipe idled through the DMA waits, nine barrier
// bubbles per tile and the epilogue (123 us for a launch whose MFMA time is 35 us and whose HBM floor -- 270 MB -- is
// ~55 us).  Here a workgroup is 8 waves in TWO groups of four, persistent over the tiles of the launch (one workgroup per
// CU), and the groups alternate by construction:
//
//   phase p:   group p & 1        computes tile p          (144 MFMAs per wave, NO barrier inside: all nine weight
//                                                           slices, 72 KB, are LDS-resident for the whole launch)
//              the other group    requests the halo of tile p + 1 into its own buffer, then stores tile p - 1
//   one s_barrier per phase.
//
// So the matrix pipe of each SIMD always has one wave in its MFMA loop while the other wave of that SIMD does the
// memory-side work of the neighbouring tiles.  LDS: weights 72 KB + two halo images 2 x 43 KB = 158 KB.  LDS image:
// pixel-major, 8 pieces of 16 bytes per pixel, piece slot XOR-swizzled by (pixel >> 1) & 7 on the source side of the DMA
// and in the fragment address.
//
// The epilogue uses NO LDS (a staging block would have to live in the halo buffer and delay the next halo's DMA behind
// the stores): the MFMA operands are swapped -- weights as the A operand, pixels as B -- so that the accumulator of a
// lane holds, for ONE pixel (lane & 31), channels 8q + 4(lane >> 5) + 0..3 of each 32-channel tile: four consecutive
// channels = one 8-byte store, the two half-waves completing 16 bytes, eight such stores covering the pixel's 128-byte
// line.  Residual / gate values are read in the same pattern.  BatchNorm column sums (forward) are per-lane partial
// sums held in registers across all tiles of the workgroup, folded across lanes once at the end; out-of-image pixels of
// ragged tiles (341 / 4 = 86 = 5*16 + 6 columns) are masked out of them.
#pragma once
#include "igemm.h"

namespace mn {

constexpr int kHaloTH = 16, kHaloTW = 16;  // output tile

// the shapes the kernel family covers: fp16, 3x3, stride 1, 64 input channels, same-size output
inline bool conv_halo_applies(const GatherGeom& g) {
  return g.R == 3 && g.S == 3 && g.C == 64 && g.mul_p == 1 && g.mul_q == 1 && g.div == 1 && g.P == g.Hi && g.Q == g.Wi &&
         g.K == 9 * 64 && g.N % 8 == 0 && !g.bt_on && (g.rsign == 1 || g.rsign == -1) && g.rsign == g.ssign &&
         (long)g.B * g.Hi * g.Wi * g.C * 2 < 0xfffffff0l;
}

constexpr int kPpWeightPieces = 9 * 512;  // nine 64 x 64 fp16 slices
// Tile: 16 x 16 pixels (TW = 16).  The template also builds 8 rows x 32 columns (TW = 32): there the 32 pixel lanes of an
// MFMA operand are 32 CONSECUTIVE pixels of one halo row, the conflict-free ds_read_b128 pattern of igemm.h, while with
// 16 x 16 tiles lanes 16-31 sit one halo row (18 pixels) below lanes 0-15 and collide with lanes 2-17
// (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.31 vs 0, profiles/r02/c27_sq_counters_layer1.txt, c28_*).  Measured EQUAL
// per launch and per step (c29_*): the bank conflicts are not what bounds the MFMA loop; only 16 x 16 is instantiated.
constexpr int pp_halo_passes(int TW) { return ((256 / TW + 2) * (TW + 2) * 8 + 63) / 64; }  // wave-wide DMAs per halo: 43 | 41

// ABL (timing experiments only, ablation build, results are wrong): bit 0 = halo DMA only for each group's first tile,
// bit 1 = no fragment reads, bit 2 = no stores / residual / gate loads, bit 3 = no MFMA.  PRIO: s_setprio of the MFMA loop.
// PD: K-sub-steps a fragment is read ahead of its MFMAs.  EARLY: residual / gate values of a tile are requested before its
// MFMA loop (64 registers held through it) instead of at the start of the store phase.
template <bool STATS, int ABL = 0, int PRIO = 0, int PD = 3, bool EARLY = false, int TW = 16>
static __global__ void __launch_bounds__(512, 1) conv_halo_pp_kernel(GatherGeom g, const half* __restrict__ A,
                                                                     const half* __restrict__ Bw, Epilogue ep, int tiles_x,
                                                                     int tiles_y, int ntiles) {
  constexpr int NP = 8;
  static_assert(TW == 16 || TW == 32, "tile width");
  constexpr int TH = 256 / TW, HW = TW + 2, HPIX = HW * (TH + 2);
  constexpr int RM = 32 / TW;  // tile rows per 32-pixel MFMA operand
  constexpr int kPpHaloPasses = pp_halo_passes(TW), kPpHaloBuf = kPpHaloPasses * 64;
  constexpr unsigned kOob = 0x80000000u;  // byte offset of a masked lane: beyond every tensor, no wrap when offsets are added
  static_assert((kPpWeightPieces + 2 * kPpHaloBuf) * 16 <= 160 * 1024 && kPpHaloBuf >= 256, "LDS");
  __shared__ piece_t smem[kPpWeightPieces + 2 * kPpHaloBuf];
  float* red = reinterpret_cast<float*>(&smem[kPpWeightPieces]);  // [8 waves][64][2]: the first halo buffer, after the last phase

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int grp = wave >> 2, wq = wave & 3;
  const int l31 = lane & 31, kh = lane >> 5;
  const int G = gridDim.x;
  const int wl = xcd_remap(blockIdx.x, G);
  const int nitems = wl < ntiles ? (ntiles - wl + G - 1) / G : 0;  // tiles wl, wl + G, ...
  piece_t* hbuf = &smem[kPpWeightPieces + grp * kPpHaloBuf];
  const bool flip = g.rsign < 0;
  // scalars out of the argument structs (lambdas below capture these, not the structs)
  const int gP = g.P, gQ = g.Q, gHi = g.Hi, gWi = g.Wi, gC = g.C, gN = g.N, gK = g.K, ldc = ep.ldc;
  const int off_h = flip ? g.off_h - 2 : g.off_h, off_w = flip ? g.off_w - 2 : g.off_w;
  const float alpha = ep.alpha;
  const bool relu = (ep.relu & 1) != 0;
  double* const stats_accum = ep.stats_accum;
  const int stats_rows = ep.stats_rows;

  const long tensor_bytes = (long)g.B * g.P * g.Q * ep.ldc * 2L;
  const __amdgpu_buffer_rsrc_t rsrc_a = make_rsrc(A, (long)g.B * g.Hi * g.Wi * g.C * 2L);
  const __amdgpu_buffer_rsrc_t rsrc_b = make_rsrc(Bw, (long)g.N * g.K * 2L);
  const __amdgpu_buffer_rsrc_t rsrc_out = make_rsrc(ep.out, tensor_bytes);
  // a null tensor has zero records: every load returns zeros, no branch
  const __amdgpu_buffer_rsrc_t rsrc_res = make_rsrc(ep.res, ep.res ? tensor_bytes : 0L);
  // (Epilogue::gate_h2: the gate is an h2 tensor of which the hi halves are read -- rows of 4 ldc bytes, 32-channel group j of a
  //  row at byte 128 j instead of 64 j)
  const int gmul = ep.gate_h2 ? 2 : 1;
  const __amdgpu_buffer_rsrc_t rsrc_gate = make_rsrc(ep.res_gate, ep.res_gate ? tensor_bytes * gmul : 0L);
  const __amdgpu_buffer_rsrc_t rsrc_ogate = make_rsrc(ep.out_gate, ep.out_gate ? tensor_bytes * gmul : 0L);
  const __amdgpu_buffer_rsrc_t rsrc_g1 = ep.res_gate ? rsrc_gate : rsrc_ogate;
  // the statistics form (forward) takes no residual / gates: 64 registers of column sums instead
  const bool has_res = !STATS && ep.res != nullptr, has_gate = !STATS && ep.res_gate != nullptr;
  const bool has_ogate = !STATS && ep.out_gate != nullptr;

  auto tile_coords = [&](int tile, int& b, int& y0, int& x0) __attribute__((always_inline)) {
    const int txi = tile % tiles_x;
    const int tmp = tile / tiles_x;
    const int tyi = tmp % tiles_y;
    b = tmp / tiles_y;
    y0 = tyi * TH;
    x0 = txi * TW;
  };
  // halo of a tile -> this group's buffer: 43 wave-wide DMA instructions dealt round-robin to the group's four waves
  auto issue_halo = [&](int tile) __attribute__((always_inline)) {
    int b, y0, x0;
    tile_coords(tile, b, y0, x0);
    const int oy = y0 + off_h, ox = x0 + off_w;
#pragma unroll
    for (int i = 0; i < (kPpHaloPasses + 3) / 4; ++i) {
      const int pass = i * 4 + wq;
      if (pass >= kPpHaloPasses) continue;  // wave-uniform
      const int q = pass * 64 + lane;
      const int hp = q >> 3, pc = q & 7;
      const int hy = hp / HW, hx = hp - hy * HW;
      const int iy = oy + hy, ix = ox + hx;
      const bool ok = hp < HPIX && (unsigned)iy < (unsigned)gHi && (unsigned)ix < (unsigned)gWi;
      const unsigned off = ok ? (unsigned)((((b * gHi + iy) * gWi + ix) * gC) * 2) + (unsigned)((pc ^ ((hp >> 1) & 7)) * 16) : ~0u;
      dma16(rsrc_a, off, 0u, hbuf + pass * 64);
    }
  };

  // ---- prologue: all nine weight slices (pass i = tap i: 64 rows x 8 pieces, swizzled on the source side), the first
  // tile of each group
  {
    const int br = t >> 3, pc = t & 7;
    const unsigned boff = br < gN ? (unsigned)(br * gK) * 2u + (unsigned)((pc ^ ((br >> 1) & 7)) * 16) : ~0u;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) dma16(rsrc_b, boff, (unsigned)(tap * gC * 2), &smem[tap * 512 + wave * 64]);
  }
  if (grp < nitems) issue_halo(wl + grp * G);

  // acc[i][j]: pixel tile i (32 pixels: tile row 2 wq + i for TW = 32, rows 4 wq + 2 i, + 1 for TW = 16) x channel tile j; register r =
  // channel 32 j + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  floatx16 acc[2][2];
  float st1[STATS ? 2 : 1][16], st2[STATS ? 2 : 1][16];  // per-lane column sums over this lane's pixels
  if constexpr (STATS) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) st1[j][r] = st2[j][r] = 0.f;
  }

  // residual and THE gate (res_gate or out_gate, never both: conv_halo_pp_applies) of a tile, in the store pattern
  Half4View rv[2][2][4], gv[2][2][4];
  auto pixel_offsets = [&](int tile, unsigned (&voff)[2], bool (&okp)[2], int rowmul = 1) __attribute__((always_inline)) {
    int b, y0, x0;
    tile_coords(tile, b, y0, x0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int y = y0 + (2 * wq + i) * RM + l31 / TW, x = x0 + l31 % TW;
      okp[i] = y < gP && x < gQ;
      voff[i] = okp[i] ? (unsigned)((((b * gP + y) * gQ + x) * ldc) * 2 * rowmul + kh * 8) : kOob;
    }
  };
  auto load_side = [&](int tile) __attribute__((always_inline)) {
    if ((ABL & 4) != 0 || !(has_res || has_gate || has_ogate)) return;
    unsigned voff[2], goff[2];
    bool okp[2];
    pixel_offsets(tile, voff, okp);
    pixel_offsets(tile, goff, okp, gmul);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          rv[i][j][q].p = __builtin_amdgcn_raw_buffer_load_b64(rsrc_res, (int)voff[i], j * 64 + q * 16, 0);
          gv[i][j][q].p = __builtin_amdgcn_raw_buffer_load_b64(rsrc_g1, (int)goff[i], j * 64 * gmul + q * 16, 0);
        }
  };

  const int prow = 2 * wq * RM + l31 / TW, pcol = l31 % TW;  // MFMA pixel tile i: RM tile rows further down
  auto compute = [&](int tile) __attribute__((always_inline)) {
    if constexpr (EARLY) load_side(tile);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // tap (r, s) reads halo pixel (prow + dy, pcol + dx), dy = r (forward) or 2 - r (data gradient)
    const int hpf = prow * HW + pcol + (flip ? 2 * HW + 2 : 0);
    const int sg = flip ? -1 : 1;
    // fragments of K-sub-step ks live in register slot ks; a sub-step's reads are issued two sub-steps (8 MFMAs, 256
    // matrix-pipe cycles) ahead of its MFMAs.  The tap loop is a real loop: fully unrolled, the 144 fragment addresses
    // get hoisted and spill.
    constexpr int SM = PD == 1 ? 1 : 3;  // fragments of sub-step ks live in register slot ks & SM
    static_assert(PD >= 1 && PD <= 3, "read-ahead");
    PieceView<half> fa[4][2], fb[4][2];
    auto load_frags = [&](int tap, int ks) __attribute__((always_inline)) {
      if constexpr ((ABL & 2) != 0) return;
      const int piece = ks * 2 + kh;
      const int hp0 = hpf + sg * ((tap / 3) * HW + tap % 3);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int hp = hp0 + i * RM * HW;
        fa[ks & SM][i].p = hbuf[hp * NP + (piece ^ ((hp >> 1) & 7))];
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = j * 32 + l31;
        fb[ks & SM][j].p = smem[tap * 512 + row * NP + (piece ^ ((row >> 1) & 7))];
      }
    };
    if constexpr ((ABL & 2) != 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[k][i].p = fb[k][i].p = zero_piece();
    }
    if constexpr (PRIO > 0) __builtin_amdgcn_s_setprio(PRIO);
#pragma unroll
    for (int k = 0; k < PD; ++k) load_frags(0, k);
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks + PD < 4)
          load_frags(tap, ks + PD);
        else if (tap + 1 < 9)
          load_frags(tap + 1, ks + PD - 4);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {  // weights = A operand (rows), pixels = B (columns)
            if constexpr ((ABL & 8) == 0) {
              mma_piece<half>(fb[ks & SM][j], fa[ks & SM][i], acc[i][j]);
            } else {
              asm volatile("" ::"v"(fa[ks & SM][i].p), "v"(fb[ks & SM][j].p));
            }
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (PRIO > 0) __builtin_amdgcn_s_setprio(0);
  };

  // memory-side phase of this group: the residual / gate values of the finished tile are requested first (loads return
  // in order: requested behind the halo they would wait for it), then the next tile's halo, then the tile is stored
  auto store_and_fetch = [&](int tile, int next_tile) __attribute__((always_inline)) {
    unsigned voff[2];
    bool okp[2];
    pixel_offsets(tile, voff, okp);
    if constexpr (!EARLY) load_side(tile);
    if ((ABL & 1) == 0 && next_tile >= 0) issue_halo(next_tile);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          Half4View o;
          const Half4View og = gv[i][j][q];  // (never both gates: conv_halo_pp_applies)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = q * 4 + e;
            float v = acc[i][j][r] * alpha;
            if (relu) v = fmaxf(v, 0.f);
            if constexpr (STATS) {
              const float vs = okp[i] ? v : 0.f;
              st1[j][r] += vs;
              st2[j][r] += vs * vs;
            }
            if (has_res) {
              float xr = (float)rv[i][j][q].e[e];
              if (has_gate && !((float)gv[i][j][q].e[e] > 0.f)) xr = 0.f;
              v += xr;
            }
            if (has_ogate && !((float)og.e[e] > 0.f)) v = 0.f;
            o.e[e] = (half)v;
          }
          if constexpr ((ABL & 4) == 0) {
            __builtin_amdgcn_raw_buffer_store_b64(o.p, rsrc_out, (int)voff[i], j * 64 + q * 16, 0);
          } else {
            asm volatile("" ::"v"(o.p));
          }
        }
  };

  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();  // weights and both first halos visible
  for (int p = 0; p <= nitems; ++p) {
    if ((p & 1) == grp) {
      if (p < nitems) compute(wl + p * G);
    } else if (p >= 1) {
      store_and_fetch(wl + (p - 1) * G, p + 1 < nitems ? wl + (p + 1) * G : -1);
    }
    wait_vmcnt<0>();               // this wave's halo DMAs (and stores)
    __builtin_amdgcn_s_barrier();  // the computing group is done reading its buffer; the other group's halo has landed
  }

  if constexpr (STATS) {
    if (stats_accum) {
      // fold the per-lane sums over the 32 pixels lanes of each half-wave; lanes 0 and 32 then hold the wave's sums.
      // Precision: a lane adds ~2 values per tile of its workgroup (36 at 192 images) in fp32, the 32 lanes and the 8 waves
      // are then combined as a tree, also fp32, and the result goes to the fp64 accumulators: at most 36 + 5 + 8 roundings
      // on any path (worst case 3e-6 relative to sum |x^2|, typically 3e-7) -- the same class as igemm.h's epilogue, whose
      // lanes add up to 96 rows of a tile sequentially before their tree.
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float a = st1[j][r], bsum = st2[j][r];
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) {
            a += __shfl_xor(a, o);
            bsum += __shfl_xor(bsum, o);
          }
          if (l31 == 0) {
            const int n = j * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            red[(wave * 64 + n) * 2 + 0] = a;
            red[(wave * 64 + n) * 2 + 1] = bsum;
          }
        }
      __syncthreads();
      if (t < 64) {
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
          sa += red[(w * 64 + t) * 2 + 0];
          sb += red[(w * 64 + t) * 2 + 1];
        }
        double* row = stats_accum + (long)((int)blockIdx.x % stats_rows) * 2 * gN;
        atomicAdd(row + t, (double)sa);
        atomicAdd(row + gN + t, (double)sb);
      }
    }
  }
}

// the shapes the persistent kernel covers: halo.h's with exactly 64 output channels in a dense [pixels][64] tensor,
// statistics (if any) through the fp64 accumulator rows and without residual / gates, at most one gate, no bias
inline bool conv_halo_pp_applies(const GatherGeom& g, const Epilogue& ep) {
  return conv_halo_applies(g) && g.N == 64 && ep.ldc == 64 && ep.stats == nullptr && ep.bias == nullptr && !ep.om_on &&
         (ep.stats_accum == nullptr || (ep.stats_rows > 0 && !ep.res && !ep.res_gate && !ep.out_gate)) &&
         !(ep.res_gate && ep.out_gate) &&
         (long)g.B * g.P * g.Q * ep.ldc * (ep.gate_h2 ? 4L : 2L) < 0x7ffffff0l;  // (masked lanes use offset 2^31)
}

// wgs: persistent workgroups (0 = knobs().halo_pp_wgs: one per CU)
inline void launch_conv_halo_pp(const GatherGeom& g, const half* A, const half* Bw, const Epilogue& ep, hipStream_t stream,
                                int wgs_arg = 0) {
  const int tx = cdiv(g.Q, kHaloTW), ty = cdiv(g.P, kHaloTH);
  const int ntiles = g.B * tx * ty;
  const int wgs = wgs_arg > 0 ? wgs_arg : knobs().halo_pp_wgs;
  const dim3 grid(ntiles < wgs ? ntiles : wgs);
#ifdef MN_ABLATION_BUILD
  const int abl = knobs().halo_pp_ablate;
#define PP_CASE(S, A_, P_) hipLaunchKernelGGL((conv_halo_pp_kernel<S, A_, P_>), grid, dim3(512), 0, stream, g, A, Bw, ep, tx, ty, ntiles); return
#define PP_VAR(S, PD_, E_) hipLaunchKernelGGL((conv_halo_pp_kernel<S, 0, 0, PD_, E_>), grid, dim3(512), 0, stream, g, A, Bw, ep, tx, ty, ntiles); return
  if (ep.stats_accum) {
    switch (abl) {
      case 200: case 201: PP_VAR(true, 2, false);
      case 210: case 211: PP_VAR(true, 3, false);
      default: break;
    }
  }
  if (!ep.stats_accum) {
    switch (abl) {
      case 1: PP_CASE(false, 1, 0);
      case 2: PP_CASE(false, 2, 0);
      case 4: PP_CASE(false, 4, 0);
      case 5: PP_CASE(false, 5, 0);
      case 8: PP_CASE(false, 8, 0);
      case 10: PP_CASE(false, 10, 0);
      case 13: PP_CASE(false, 13, 0);
      case 100: PP_CASE(false, 0, 1);  // not an ablation: MFMA loop at raised wave priority
      case 101: PP_CASE(false, 0, 3);
      case 200: PP_VAR(false, 2, false);  // not ablations: fragment read-ahead, early residual / gate requests
      case 201: PP_VAR(false, 2, true);
      case 210: PP_VAR(false, 3, false);
      case 211: PP_VAR(false, 3, true);
      default: break;
    }
  }
#undef PP_CASE
#undef PP_VAR
#endif
  if (ep.stats_accum)
    hipLaunchKernelGGL(conv_halo_pp_kernel<true>, grid, dim3(512), 0, stream, g, A, Bw, ep, tx, ty, ntiles);
  else
    hipLaunchKernelGGL(conv_halo_pp_kernel<false>, grid, dim3(512), 0, stream, g, A, Bw, ep, tx, ty, ntiles);
}

}  // namespace mn
