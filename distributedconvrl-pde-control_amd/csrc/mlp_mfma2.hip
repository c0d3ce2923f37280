// mlp_mfma2.hip -- fused fp32 MFMA path of the DDPG update for the reference-shaped 2-layer nets
// (`drop_middle_layer = true`, src/PDEagent.jl:30-41: actor Dense(ns,h,relu) -> Dense(h,1,tanh), critic
// Dense(ns+1,H,relu) -> Dense(H,1)) at large batches, e.g. the 2-D Keller-Segel case of BASELINE.json configs[3]:
// a 3x3 x 2 species x 2 steps window (ns = 36) over B*A = 100k columns, critic 37 -> 340 -> 1.  This is the
// "2-D conv as im2col-GEMM" contraction: [H x (ns+1)] x [(ns+1) x columns] on v_mfma_f32_16x16x4_f32.
// Restates src/PDEagent.jl:385-409 in the same two passes as mlp_mfma.hip, each followed by a finish launch (slab sum, and
// ADAM + Polyak when no all-reduce comes between), and the fused acting kernel.
// This file is the family's one translation unit and its host layer: shape constants and instantiation lists, visitors,
// predicates, grid2_of, the launches, the describers, fused2_family.  The kernels are templates instantiated from the lists
// below, in headers:
//   fused2_image.hpp   Net2, the flat layout (flat2_offsets), the LDS image (Lds2, carve2) and load_net2
//   fused2_layers.hpp  the first-layer products, the input rows and their staging, gemm_cols, the output row's gradient,
//                      Fused2Args, the slab's tile numbering
//   fused2_critic.hpp  ddpg2_critic_kernel, Critic2Lds          fused2_actor.hpp  ddpg2_actor_kernel, Actor2Lds
//   fused2_finish.hpp  finish2_kernel, apply2_kernel            fused2_act.hpp    policy_act2_kernel, Act2Lds
// Layout: one workgroup = 8 waves = 128 columns, a wave owns 16 columns.  The first-layer weights live in LDS as a
// padded image [HP][LDK]; the contraction index is blocked by 8 (k = 8 blk + 2 q + t, t = 0,1), so the A operand of
// two consecutive k-steps is ONE ds_read_b64 (row stride 8 KB + 4 floats = 2 x odd 8-byte slots: conflict-free over
// each 32-lane service group) and the B operand is the input row pair the lane loaded from HBM.  The output layer is
// a single row: its forward is a per-lane dot + two lane exchanges, its weight gradient a DPP row sum.  dW1 contracts
// over columns: dz1 and the inputs are transposed once through LDS and multiplied as MFMA tiles (mfma_blocks.hpp).
// The kernels read the FLAT parameter buffers (no padded copy to maintain).
#include "common.hpp"
#include "mlp.hpp"
// The family's shape constants are stated in this file (K2MAX and CPWMAX here, the instantiation lists and
// FUSED2_APPLY_MIN_BU below), where tests/fused_shape_cases.py reads them.  The two stand ahead of the headers because the
// layers and the critic pass are built on them.
#define K2MAX 6            // k-blocks of 8: the critic's ns + 1 inputs and the ones row of its staging image fit, ns + 2 <= 48
#define CPWMAX 4           // column chunks (of 128) one workgroup walks through: the weight images are loaded once per
                           // workgroup and the partial gradients of all its chunks share one slab
#include "fused2_critic.hpp"
#include "fused2_actor.hpp"
#include "fused2_finish.hpp"
#include "fused2_act.hpp"

namespace pdec {

// ------------------------------------------------------------------ host side
static int mt2_of(int H) { return (H + 1 + 15) / 16; }

// The instantiations of the two passes, X(critic tiles MT, actor tiles MTA) x Y(k-blocks KB): the ONE list behind the
// predicate (fused2_supported), the launches and the report of pdec_debug_batched_update_route.  The number of 8-row k-blocks
// is a compile-time constant (a smaller net runs the next larger variant on zero-padded rows: FUSED2_KBS ascends), so the
// MFMA chains carry no control flow.  The acting kernel: X(actor tiles MTA) x Y(k-blocks KB).
#define FUSED2_TILES(X) X(22, 2) X(22, 1) X(9, 2) X(9, 1)
#define FUSED2_ACT_TILES(X) X(2) X(1)
#define FUSED2_KBS(Y) Y(2) Y(5) Y(6)
static_assert(K2MAX == 6, "FUSED2_KBS ends at K2MAX");

// f(tile_c<KB>) of the first variant with kb <= KB k-blocks
template <class F>
static int visit2_kb(int kb, F&& f) {
#define Y(KB_) if (kb <= KB_) return f(tile_c<KB_>{});
  FUSED2_KBS(Y)
#undef Y
  set_error("fused 2-layer pass: no instantiation for %d k-blocks", kb);
  return PDEC_E_INVALID;
}
// f(tile_c<MT>, tile_c<MTA>, tile_c<KB>) of the pair's instantiation.  kb: the CRITIC's k-blocks decide KB in both passes (its
// input is the actor's rows and the action row) -- the launch (dispatch2) and the report (fused2_describe) both come through here
template <class F>
static int visit2(int kb, int mt, int mta, F&& f) {
  return visit2_kb(kb, [&](auto KB) {
#define X(MT_, MTA_) if (mt == MT_ && mta == MTA_) return f(tile_c<MT_>{}, tile_c<MTA_>{}, KB);
    FUSED2_TILES(X)
#undef X
    set_error("fused 2-layer pass: no instantiation for %d critic / %d actor tiles", mt, mta);
    return (int)PDEC_E_INVALID;
  });
}
template <class F>
static int visit2_act(int kb, int mta, F&& f) {
  return visit2_kb(kb, [&](auto KB) {
#define X(MTA_) if (mta == MTA_) return f(tile_c<MTA_>{}, KB);
    FUSED2_ACT_TILES(X)
#undef X
    set_error("fused 2-layer act: no instantiation for %d actor tiles", mta);
    return (int)PDEC_E_INVALID;
  });
}

static bool fused2_disabled() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("PDEC_DISABLE_FUSED");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}

static bool fused2_supported(const Mlp* A, const Mlp* C) {
  if (fused2_disabled()) return false;
  if (A->dtype != PDEC_F32 || C->dtype != PDEC_F32 || A->L != 2 || C->L != 2) return false;
  const int ns = A->dims[0];
  if (A->dims[2] != 1 || C->dims[0] != ns + 1 || C->dims[2] != 1 || ns + 2 > 8 * K2MAX) return false;
  if (A->acts[0] != PDEC_ACT_RELU || A->acts[1] != PDEC_ACT_TANH) return false;
  if (C->acts[0] != PDEC_ACT_RELU || C->acts[1] != PDEC_ACT_IDENTITY) return false;
  const int mt = mt2_of(C->dims[1]), mta = mt2_of(A->dims[1]);
  bool ok = false;
#define X(MT_, MTA_) ok = ok || (mt == MT_ && mta == MTA_);
  FUSED2_TILES(X)
#undef X
  return ok;
}

// Workgroups of a pass and wave tiles (16 columns) per workgroup.  Up to one 128-column chunk per CU: one chunk each.  Beyond
// that the tiles are dealt EVENLY over 256 workgroups (one per CU: a pass's LDS images leave room for one), each walking
// ceil(tpw / 8) <= CPWMAX chunks; more than CPWMAX chunks per CU: more workgroups.  (Dealing whole chunks strided over
// ceil(nchunk / cpw) workgroups made C4's 784 chunks 196 workgroups x 4.)
static int grid2_of(int Bu, int* tpw) {
  const int nt = (Bu + 15) / 16, nchunk = (nt + 7) / 8;
  if (nchunk <= 256) { *tpw = 8; return nchunk; }
  const int grid = std::max(256, (nchunk + CPWMAX - 1) / CPWMAX);
  *tpw = (nt + grid - 1) / grid;
  return (nt + *tpw - 1) / *tpw;
}

static Net2 net2_of(const Mlp* M) {
  Net2 n;
  n.p = M->params.as<float>();
  n.K0 = M->dims[0]; n.H = M->dims[1];
  n.kb = (n.K0 + 7) / 8;
  return n;
}

// dynamic LDS bytes of a pass on these arguments: the end of its layout, at the staging tiles of the net whose gradient it forms
template <int MT, int MTA, int KB>
static int lds2_checked(const Fused2Args& g, bool actor_pass, size_t* lds) {
  *lds = (size_t)(actor_pass ? Actor2Lds<MT, MTA, KB>::behind(0, 16 * nr_of(g.A.K0)).end : Critic2Lds<MT, MTA, KB>::behind(0, 16 * nr_of(g.C.K0)).end) * 4;
  PDEC_REQUIRE(*lds <= 160 * 1024, "fused 2-layer pass needs %zu B of LDS", *lds);
  return PDEC_OK;
}

template <int MT, int MTA, int KB>
static int launch2(Mlp* M, const Fused2Args& g, int grid, bool actor_pass) {
  size_t lds = 0;
  if (int rc = lds2_checked<MT, MTA, KB>(g, actor_pass, &lds)) return rc;
  const void* kern = actor_pass ? reinterpret_cast<const void*>(ddpg2_actor_kernel<MT, MTA, KB>)
                                : reinterpret_cast<const void*>(ddpg2_critic_kernel<MT, MTA, KB>);
  static size_t attr_lds[2] = {0, 0};          // per template instantiation and pass
  if (attr_lds[actor_pass] < lds) {
    PDEC_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_lds[actor_pass] = lds;
  }
  ProfScope ps(M, actor_pass ? "ddpg2_actor_fused" : "ddpg2_critic_fused", true);
  for (int rep = 0; rep < ps.reps; ++rep) {
    if (actor_pass) hipLaunchKernelGGL((ddpg2_actor_kernel<MT, MTA, KB>), dim3(grid), dim3(FTHREADS), lds, M->stream, g);
    else hipLaunchKernelGGL((ddpg2_critic_kernel<MT, MTA, KB>), dim3(grid), dim3(FTHREADS), lds, M->stream, g);
  }
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

static int dispatch2(Mlp* M, const Fused2Args& g, int grid, bool actor_pass, int mt, int mta) {
  return visit2(g.C.kb, mt, mta, [&](auto MT, auto MTA, auto KB) {
    return launch2<decltype(MT)::value, decltype(MTA)::value, decltype(KB)::value>(M, g, grid, actor_pass);
  });
}

// The ADAM / Polyak half of the finish arguments, for the finish launch that applies and for the apply launch.  Frozen
// targets (rho == 1, the reference as it runs) are not touched: *Mt becomes null (see launch_finish, mlp_mfma.hip).
static int apply2_args(Finish2Args& g, Mlp* M, Mlp** Mt, const AdamPolyak& ap) {
  g.apply = 1;
  if (int rc = bp_begin(M, ap.b1, ap.b2, &g.bp)) return rc;
  g.p = M->params.as<float>(); g.m = M->m.as<float>(); g.v = M->v.as<float>();
  g.eta = ap.eta; g.b1 = ap.b1; g.b2 = ap.b2; g.eps = ap.eps;
  if (*Mt && (float)ap.rho == 1.0f) *Mt = nullptr;
  if (*Mt) {
    g.pt = (*Mt)->params.as<float>();
    const float r = (float)ap.rho;
    g.rho = r; g.omr = 1.0f - r;
  }
  return PDEC_OK;
}
// behind the launch that applied
static void apply2_done(Mlp* M, Mlp* Mt) {
  bp_done(M);
  M->fw_dirty = true;
  if (Mt) Mt->fw_dirty = true;
}

static int launch_finish2(Mlp* M, Mlp* Mt, int nslab, int MT, int nR, double grad_scale, int mode, int Bu, int quirk,
                          void* loss_dev, const AdamPolyak* ap, const void* loss_add = nullptr) {
  Finish2Args g{};
  g.slabs = M->fslab.as<float>(); g.nslab = nslab; g.K0 = M->dims[0]; g.H = M->dims[1]; g.MT = MT; g.nR = nR;
  g.grads = M->grads.as<float>(); g.scale = (float)grad_scale; g.mode = mode; g.Bu = Bu; g.quirk = quirk;
  g.loss_out = (float*)loss_dev;
  g.loss_add = (const float*)loss_add;
  if (ap)
    if (int rc = apply2_args(g, M, &Mt, *ap)) return rc;
  {
    ProfScope ps(M, ap ? "fused2_finish" : "fused2_reduce");
    hipLaunchKernelGGL(finish2_kernel, dim3(stats2_chunk(MT, nR)), dim3(1024), 0, M->stream, g);   // one block per gradient chunk
  }
  PDEC_HIP(hipGetLastError());
  if (ap) apply2_done(M, Mt);
  return PDEC_OK;
}

// 2-layer fp32 actor [ns, h, 1] (relu, tanh | identity), h <= 31, ns <= 48, at least a few hundred columns
static bool fused2_act_supported(const Mlp* A, int cols) {
  if (fused2_disabled() || A->dtype != PDEC_F32 || A->L != 2 || A->dims[2] != 1 || cols < 256) return false;
  if (A->acts[0] != PDEC_ACT_RELU || (A->acts[1] != PDEC_ACT_TANH && A->acts[1] != PDEC_ACT_IDENTITY)) return false;
  return A->dims[0] <= 8 * K2MAX && mt2_of(A->dims[1]) <= 2;
}

static int fused2_policy_act(Mlp* A, const void* state, int cols, double act_noise, double act_limit, int learning, uint64_t seed,
                             uint64_t offset, void* actions_out, const uint64_t* ctr_cur, uint64_t* ctr_next, uint64_t ctr_inc) {
  const Net2 n = net2_of(A);
  const int mta = mt2_of(A->dims[1]), tanh_out = A->acts[1] == PDEC_ACT_TANH;
  const dim3 grid((cols + 63) / 64), block(256);
  ProfScope ps(A, "policy_act_fused");
  int rc = visit2_act(n.kb, mta, [&](auto MTA, auto KB) {
    constexpr int mta_ = decltype(MTA)::value, kb_ = decltype(KB)::value;
    const size_t lds = (size_t)Act2Lds<mta_, kb_>::end * 4;
    if (learning && A->noise_color)
      hipLaunchKernelGGL((policy_act2_kernel<mta_, kb_, NoiseColor>), grid, block, lds, A->stream, n, (const float*)state, cols,
                         noise_color_of(A, act_noise), (float)act_limit, learning, tanh_out, seed, offset, (float*)actions_out,
                         ctr_cur, ctr_next, ctr_inc);
    else if (A->noise_scale)
      hipLaunchKernelGGL((policy_act2_kernel<mta_, kb_, NoiseScale>), grid, block, lds, A->stream, n, (const float*)state, cols,
                         noise_scale_of(A), (float)act_limit, learning, tanh_out, seed, offset, (float*)actions_out, ctr_cur,
                         ctr_next, ctr_inc);
    else
      hipLaunchKernelGGL((policy_act2_kernel<mta_, kb_>), grid, block, lds, A->stream, n, (const float*)state, cols, (float)act_noise,
                         (float)act_limit, learning, tanh_out, seed, offset, (float*)actions_out, ctr_cur, ctr_next, ctr_inc);
    return (int)PDEC_OK;
  });
  if (rc) return rc;
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

static int fused2_act_describe(const Mlp* A, char* name, int name_len, int64_t* lds) {
  return visit2_act(net2_of(A).kb, mt2_of(A->dims[1]), [&](auto MTA, auto KB) {
    constexpr int mta_ = decltype(MTA)::value, kb_ = decltype(KB)::value;
    snprintf(name, name_len, "policy_act2_kernel<%d,%d>", mta_, kb_);
    *lds = (int64_t)Act2Lds<mta_, kb_>::end * 4;
    return (int)PDEC_OK;
  });
}

static bool fused2_net_supported(const Mlp* M) { return !fused2_disabled() && M->dtype == PDEC_F32 && M->L == 2; }

static int fused2_adam_polyak(Mlp* M, Mlp* Mt, const AdamPolyak& ap) {
  Finish2Args g{};
  g.grads = M->grads.as<float>();
  if (int rc = apply2_args(g, M, &Mt, ap)) return rc;
  {
    ProfScope ps(M, "fused2_apply");
    hipLaunchKernelGGL(apply2_kernel, dim3((M->nparams + 255) / 256), dim3(256), 0, M->stream, g, M->nparams);
  }
  PDEC_HIP(hipGetLastError());
  apply2_done(M, Mt);
  return PDEC_OK;
}

static int fused2_critic_grads(Mlp* A, Mlp* C, Mlp* At, Mlp* Ct, const void* s, const void* a, const void* r, const void* t,
                               const void* sn, int Bu, double gamma, int quirk, double grad_scale, void* loss_dev,
                               const AdamPolyak* apply, const void* loss_add) {
  const int mt = mt2_of(C->dims[1]), mta = mt2_of(A->dims[1]), nR = nr_of(C->dims[0]);
  int tpw = 8;
  const int grid = grid2_of(Bu, &tpw);
  const size_t need = slab2_floats(mt, nR, grid) * 4;
  if (C->fslab.bytes < need) PDEC_HIP(C->fslab.alloc(need));
  Fused2Args g{};
  g.C = net2_of(C); g.At = net2_of(At); g.Ct = net2_of(Ct);
  g.s = (const float*)s; g.a = (const float*)a; g.r = (const float*)r; g.t = (const float*)t; g.sn = (const float*)sn;
  g.Bu = Bu; g.ns = A->dims[0]; g.gamma = (float)gamma; g.quirk = quirk; g.tpw = tpw;
  g.slab = C->fslab.as<float>();
  if (quirk && C->rbar_ext) {          // reduced by the producer of r on its own stream (pdec_reward_mean)
    g.rbar = (const float*)C->rbar_ext;
  } else if (quirk) {
    float* rb = nullptr;
    int rcm = launch_rmean(C, (const float*)r, Bu, &rb);
    if (rcm) return rcm;
    g.rbar = rb;
  }
  C->rbar_ext = nullptr;
  int rc = dispatch2(C, g, grid, false, mt, mta);
  if (rc) return rc;
  return launch_finish2(C, apply ? Ct : nullptr, grid, mt, nR, grad_scale, 0, Bu, quirk, loss_dev, apply, loss_add);
}

static int fused2_actor_grads(Mlp* A, Mlp* C, Mlp* At, const void* s, int Bu, double grad_scale, void* loss_dev,
                              const AdamPolyak* apply) {
  const int mt = mt2_of(C->dims[1]), mta = mt2_of(A->dims[1]), nRa = nr_of(A->dims[0]);
  int tpw = 8;
  const int grid = grid2_of(Bu, &tpw);
  const size_t need = slab2_floats(mta, nRa, grid) * 4;
  if (A->fslab.bytes < need) PDEC_HIP(A->fslab.alloc(need));
  Fused2Args g{};
  g.C = net2_of(C); g.A = net2_of(A);
  g.s = (const float*)s; g.Bu = Bu; g.ns = A->dims[0]; g.tpw = tpw;
  g.slab = A->fslab.as<float>();
  int rc = dispatch2(C, g, grid, true, mt, mta);       // on the critic's stream object (shared stream, checked by the caller)
  if (rc) return rc;
  return launch_finish2(A, apply ? At : nullptr, grid, mta, nRa, grad_scale, 1, Bu, 0, loss_dev, apply);
}

// what fused2_critic_grads / fused2_actor_grads would launch for this pair (pdec_debug_batched_update_route): the networks go
// into the arguments as they do there, then the same visitor and the same LDS check as launch2
static int fused2_describe(const Mlp* A, const Mlp* C, bool actor_pass, char* name, int name_len, int64_t* lds) {
  Fused2Args g{};
  g.C = net2_of(C); g.A = net2_of(A);
  return visit2(g.C.kb, mt2_of(C->dims[1]), mt2_of(A->dims[1]), [&](auto MT, auto MTA, auto KB) {
    constexpr int mt_ = decltype(MT)::value, mta_ = decltype(MTA)::value, kb_ = decltype(KB)::value;
    size_t b = 0;
    if (int rc = lds2_checked<mt_, mta_, kb_>(g, actor_pass, &b)) return rc;
    snprintf(name, name_len, "%s<%d,%d,%d>", actor_pass ? "ddpg2_actor_kernel" : "ddpg2_critic_kernel", mt_, mta_, kb_);
    *lds = (int64_t)b;
    return (int)PDEC_OK;
  });
}

// below FUSED2_APPLY_MIN_BU columns the passes are the same kernels and ADAM / Polyak are launches of their own
#define FUSED2_APPLY_MIN_BU 64
#ifndef __HIP_DEVICE_COMPILE__        // (a host table: see fused3_family, mlp_mfma.hip)
const FusedFamily fused2_family = {fused2_supported,    fused2_net_supported, fused2_act_supported, FUSED2_APPLY_MIN_BU,
                                   fused2_critic_grads, fused2_actor_grads,   fused2_adam_polyak,   fused2_policy_act,
                                   fused2_describe,     fused2_act_describe};
#endif

}  // namespace pdec
