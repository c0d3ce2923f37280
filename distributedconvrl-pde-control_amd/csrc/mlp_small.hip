// mlp_small.hip -- the host side of the small DDPG update (pdec_ddpg_update_small / _rng, pdec_population_update): the ONE list of
// register-kernel instantiations with the shapes each serves, the plan that picks one and sizes its launch from the kernels' own
// LDS layouts, the launch, and the C entry points.  The kernels: small_generic.hpp (any depth), small2.hpp (2-layer nets, one
// thread per hidden unit), small2f.hpp (the same for frozen targets, two chains side by side); what they share: small_args.hpp,
// small2_blocks.hpp.
#include "small_generic.hpp"
#include "small2.hpp"
#include "small2f.hpp"

namespace pdec {

// 2-layer relu/tanh actor [ns, h, 1] + relu/identity critic [ns+1, H, 1], H and h <= 512, ns <= 15, Bu <= S2_BU
static bool small2_ok(const Mlp* A, const Mlp* C, int Bu) {
  if (getenv("PDEC_SMALL_GENERIC")) return false;
  if (A->L != 2 || C->L != 2 || Bu > S2_BU) return false;
  if (A->dims[2] != 1 || C->dims[2] != 1 || C->dims[0] != A->dims[0] + 1 || A->dims[0] > 15) return false;
  if (A->acts[0] != PDEC_ACT_RELU || A->acts[1] != PDEC_ACT_TANH || C->acts[0] != PDEC_ACT_RELU || C->acts[1] != PDEC_ACT_IDENTITY)
    return false;
  return A->dims[1] <= 512 && C->dims[1] <= 512;
}

static int fill_net(SmallNet& n, Mlp* M, Mlp* T) {
  PDEC_REQUIRE(M->L <= SM_MAXL, "small update: at most %d layers", SM_MAXL);
  n.p = M->params.as<float>(); n.g = M->grads.as<float>(); n.m = M->m.as<float>(); n.v = M->v.as<float>();
  n.pt = T->params.as<float>();
  n.L = M->L; n.nparams = M->nparams;
  for (int l = 0; l <= M->L; ++l) n.dims[l] = M->dims[l];
  for (int l = 0; l < M->L; ++l) { n.acts[l] = M->acts[l]; n.woff[l] = (int)M->w_off[l]; n.boff[l] = (int)M->b_off[l]; }
  return PDEC_OK;
}

}  // namespace pdec

using namespace pdec;

struct SmallSampling {     // != null: draw the slots in the kernel (pdec_ddpg_update_small_rng)
  uint64_t seed, offset;
  int64_t n_valid, n_rt, capacity;
  int stride;
};

// Every register-kernel instantiation pdec_ddpg_update_small(_rng) and pdec_population_update can launch,
// X(id, reported name, NS, BU, OS, EXACT, NWC, kernel): the ONE list behind SmallKernelId, the names
// pdec_debug_small_update_kernel reports, the rows small_plan() chooses from (the FIRST row that serves a shape, in this order)
// and the launch switch (small_launch).  The launch sites and the query both go through small_plan, so the query reports
// exactly what a call would launch.
// (tests/test_population_update_table.py reads the EXACT column by its position, as the literal true / false.)
//   NS, BU, EXACT  the kernel's KA and BUT: EXACT rows serve ns == NS and Bu == BU alone, the others ns <= NS and Bu <= BU; only
//                  EXACT kernels read a member's own hyper-parameters (small_serves_member_hyper; KC = NS + 1 everywhere)
//   OS             > 0: owner lanes for the actor's ADAM state (ddpg_small2_kernel's OS), for nA <= 64 and (ns + 2) nA <= 64 OS,
//                  unless PDEC_SMALL_OWN=0 -- the shipped moving-target shapes: Keller-Segel10_16 14 x 20 parameters, Fluid 11 x 18
//   NWC            > 0: the frozen-target two-chain kernel (ddpg_small2f_kernel) with NWC critic waves, for rho == 1,
//                  (ns + 2) nA + 1 <= 64 and 64 NWC - 63 <= nC <= 64 NWC, unless PDEC_SMALL_SPLIT=0.
//                  Only the exact KS instantiation (ns 1, batch 3, 129 - 192 critic units: KS22 / KS200 / KS500): there every
//                  guard folds at compile time and the backend fuses multiplies and adds the same way in both kernels, which is
//                  what makes them agree bit for bit; the bounded instantiations differ in the last place of the actor's gradient
//                  (a product fused into one kernel's sum and not the other's).
#define SMALL2_KERNELS(X)                                                                                        \
  X(S2F_2_1_3, "ddpg_small2f_kernel<2,1,3,1,3>", 1, 3, 0, true, 3, ddpg_small2f_kernel<2, 1, 3, true, 3>)         \
  X(S2_2_1_3, "ddpg_small2_kernel<2,1,3,1>", 1, 3, 0, true, 0, ddpg_small2_kernel<2, 1, 3, true>)                 \
  X(S2_13_12_3_OS5, "ddpg_small2_kernel<13,12,3,1,5>", 12, 3, 5, true, 0, ddpg_small2_kernel<13, 12, 3, true, 5>) \
  X(S2_10_9_3_OS4, "ddpg_small2_kernel<10,9,3,1,4>", 9, 3, 4, true, 0, ddpg_small2_kernel<10, 9, 3, true, 4>)     \
  X(S2_13_12_3, "ddpg_small2_kernel<13,12,3,1>", 12, 3, 0, true, 0, ddpg_small2_kernel<13, 12, 3, true>)          \
  X(S2_10_9_3, "ddpg_small2_kernel<10,9,3,1>", 9, 3, 0, true, 0, ddpg_small2_kernel<10, 9, 3, true>)              \
  X(S2_4_3_4, "ddpg_small2_kernel<4,3,4,0>", 3, S2_BU, 0, false, 0, ddpg_small2_kernel<4, 3, S2_BU, false>)       \
  X(S2_10_9_4, "ddpg_small2_kernel<10,9,4,0>", 9, S2_BU, 0, false, 0, ddpg_small2_kernel<10, 9, S2_BU, false>)    \
  X(S2_13_12_4, "ddpg_small2_kernel<13,12,4,0>", 12, S2_BU, 0, false, 0, ddpg_small2_kernel<13, 12, S2_BU, false>) \
  X(S2_16_15_4, "ddpg_small2_kernel<16,15,4,0>", 15, S2_BU, 0, false, 0, ddpg_small2_kernel<16, 15, S2_BU, false>)
static_assert(S2_BU == 4, "the reported names of the bounded instantiations spell S2_BU out");
enum SmallKernelId {
  SK_GENERIC,         // ddpg_small_kernel
#define X(ID, NAME, ...) SK_##ID,
  SMALL2_KERNELS(X)
#undef X
  SK_BATCHED,         // no kernel (not in the name table): reward groups that split the minibatch, served by the batched update
};
static const char* const small_kernel_names[] = {
    "ddpg_small_kernel",
#define X(ID, NAME, ...) NAME,
    SMALL2_KERNELS(X)
#undef X
};
struct Small2Row {
  SmallKernelId id;
  int ns, Bu, os;
  bool exact;
  int nwc;
};
static const Small2Row small2_rows[] = {
#define X(ID, NAME, NS, BU, OS, EXACT, NWC, ...) {SK_##ID, NS, BU, OS, EXACT, NWC},
    SMALL2_KERNELS(X)
#undef X
};

// does the row's kernel serve these shapes?  (its LDS is the caller's matter)
static bool small2_row_serves(const Small2Row& r, int ns, int Bu, int nA, int nC, float rho, bool own, bool split) {
  if (r.exact ? (ns != r.ns || Bu != r.Bu) : (ns > r.ns || Bu > r.Bu)) return false;
  if (r.os && !(own && nA <= 64 && (ns + 2) * nA <= 64 * r.os)) return false;
  if (r.nwc && !(split && rho == 1.0f && (ns + 2) * nA + 1 <= 64 && (nC + 63) / 64 == r.nwc)) return false;
  return true;
}

struct SmallPlan {
  SmallKernelId id;
  int threads;              // block size
  size_t lds;               // dynamic LDS bytes of the launch (slot table included)
  int smp_lds;              // float offset of the slot table
  int lds_params;           // generic kernel: the learner state staged in LDS
  int maxw;                 // generic kernel: widest layer
};

// the kernel a call launches, its block and its dynamic LDS -- or the error the call raises.  Reads the env switches
// PDEC_SMALL_GENERIC / PDEC_SMALL_OWN / PDEC_SMALL_SPLIT per call (the identity tests switch them).  A broadcast target
// (quirk) whose reward groups (pdec_ddpg_set_reward_groups) split the minibatch -- 2 <= g, g L < Bu -- has no small kernel:
// SK_BATCHED, which the call refuses (the caller updates through pdec_ddpg_update_async); g = 1 is the diagonal target and
// g L >= Bu the whole-minibatch broadcast, both served by the small kernels as they are.
static int small_plan(const Mlp* A, const Mlp* C, int loops, int Bu, float rho, bool sampling, int quirk, SmallPlan* pl) {
  PDEC_REQUIRE(loops >= 1 && Bu >= 1 && Bu <= 16, "pdec_ddpg_update_small: needs 1 <= Bu <= 16 (got %d)", Bu);
  if (quirk && C->rg_g >= 2 && (int64_t)C->rg_g * C->rg_L < Bu) {
    *pl = SmallPlan{};
    pl->id = SK_BATCHED;
    return PDEC_OK;
  }
  PDEC_REQUIRE(A->L <= SM_MAXL && C->L <= SM_MAXL, "small update: at most %d layers", SM_MAXL);
  const int ns = A->dims[0];
  int maxw = 1;
  for (int l = 0; l <= A->L; ++l) maxw = std::max(maxw, A->dims[l]);
  for (int l = 0; l <= C->L; ++l) maxw = std::max(maxw, C->dims[l]);
  pl->maxw = maxw;
  const SmallLds gen(A->L, C->L, maxw, Bu, A->nparams, C->nparams);
  PDEC_REQUIRE(gen.end_act * 4 <= 160 * 1024, "pdec_ddpg_update_small: layers too wide for the in-LDS activations (%zu B)",
               gen.end_act * 4);
  pl->lds_params = gen.end * 4 <= 150 * 1024;
  const size_t gen_floats = pl->lds_params ? gen.end : gen.end_act;
  const size_t tab_floats = sampling ? (size_t)3 * loops * Bu : 0;
  auto take = [&](SmallKernelId id, int threads, size_t floats) {      // the slot table sits behind the kernel's own LDS
    pl->id = id; pl->threads = threads; pl->smp_lds = (int)floats; pl->lds = (floats + tab_floats) * 4;
    return PDEC_OK;
  };
  if (small2_ok(A, C, Bu) && Small2Lds(loops, ns, Bu, 0).red * 4 <= 120 * 1024) {      // (red: behind the batches of all loops)
    const int nC = C->dims[1], nA = A->dims[1];
    const char* noown = getenv("PDEC_SMALL_OWN");
    const char* nosplit = getenv("PDEC_SMALL_SPLIT");
    const bool own = !(noown && noown[0] == '0'), split = !(nosplit && nosplit[0] == '0');
    for (const Small2Row& r : small2_rows) {
      if (!small2_row_serves(r, ns, Bu, nA, nC, rho, own, split)) continue;
      if (r.nwc) {     // frozen targets: the critic and the actor updates as two chains side by side, if they fit 150 KB
        const Small2fLds f(loops, ns, Bu, r.ns + 1, r.nwc);
        if ((f.end + tab_floats) * 4 <= 150 * 1024) return take(r.id, (r.nwc + 1) * 64, f.end);
        continue;
      }
      // the slot table sits behind the register kernel's LDS: it must fit in the workgroup's 160 KB, or the call takes the
      // generic kernel (which refuses cleanly when nothing fits) -- not a later row
      const Small2Lds l2(loops, ns, Bu, r.os);
      if ((l2.end + tab_floats) * 4 > 160 * 1024) break;
      return take(r.id, (std::max(nC, nA) + 63) / 64 * 64, l2.end);
    }
  }
  PDEC_REQUIRE((gen_floats + tab_floats) * 4 <= 160 * 1024,
               "pdec_ddpg_update_small: the slot table does not fit beside the learner state in LDS");
  return take(SK_GENERIC, SM_THREADS, gen_floats);
}

// do the kernels of this plan read a member's own gamma, rho and step sizes (sm_member_begin<HYPER>)?  All but the bounded
// instantiations of ddpg_small2_kernel: the rows that are not EXACT
static bool small_serves_member_hyper(const SmallPlan& pl) {
  for (const Small2Row& r : small2_rows)
    if (r.id == pl.id) return r.exact;
  return true;      // the generic kernel (and SK_BATCHED, which launches nothing)
}

// the shape checks of a small update on the four networks
static int small_nets(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, Mlp** pA, Mlp** pC, Mlp** pAt, Mlp** pCt) {
  Mlp* A = lookup_as<Mlp>(hA, Kind::Mlp);
  Mlp* C = lookup_as<Mlp>(hC, Kind::Mlp);
  Mlp* At = lookup_as<Mlp>(hAt, Kind::Mlp);
  Mlp* Ct = lookup_as<Mlp>(hCt, Kind::Mlp);
  if (!A || !C || !At || !Ct) { set_error("pdec_ddpg_update_small: bad network handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(A->dtype == PDEC_F32 && C->dtype == PDEC_F32 && At->dtype == PDEC_F32 && Ct->dtype == PDEC_F32,
               "pdec_ddpg_update_small: fp32 networks only (the reference's network dtype)");
  PDEC_REQUIRE(At->dims == A->dims && Ct->dims == C->dims, "ddpg: target networks must have the behaviour networks' shapes");
  const int ns = A->dims[0], na = A->dims[A->L];
  PDEC_REQUIRE(C->dims[0] == ns + na && C->dims[C->L] == 1, "ddpg: critic must map ns+na -> 1");
  PDEC_REQUIRE(A->stream == C->stream && At->stream == C->stream && Ct->stream == C->stream,
               "pdec_ddpg_update_small: the four networks must share one stream");
  *pA = A; *pC = C; *pAt = At; *pCt = Ct;
  return PDEC_OK;
}

// the fields of SmallArgs that a solo call and a population launch share; the caller adds its traces and slots, sampling
// bounds, beta-power slots and halt flag -- or the member table
static int small_args(SmallArgs& g, const SmallPlan& pl, Mlp* A, Mlp* C, Mlp* At, Mlp* Ct, int loops, int Bu, double gamma,
                      double rho, int quirk, double eta_actor, double eta_critic) {
  int rc;
  if ((rc = fill_net(g.A, A, At)) || (rc = fill_net(g.C, C, Ct))) return rc;
  g.maxw = pl.maxw;
  g.lds_params = pl.lds_params;
  g.loops = loops; g.Bu = Bu; g.ns = A->dims[0]; g.na = A->dims[A->L];
  g.quirk = quirk && C->rg_g == 1 ? 0 : quirk;     // groups of one column: the diagonal target
  g.gamma = (float)gamma; g.rho = (float)rho;      // Float32 in the reference (y = 0.99f0, p = 0.995f0)
  g.eta_a = eta_actor; g.eta_c = eta_critic; g.b1 = 0.9; g.b2 = 0.999; g.eps = 1e-8;
  g.smp_lds = pl.smp_lds;
  return PDEC_OK;
}

// the plan's kernel on `grid` workgroups; allows the launch's dynamic LDS once per kernel (the register kernels ask for up to
// 160 KB)
static int small_launch(const SmallPlan& pl, dim3 grid, hipStream_t stream, const SmallArgs& g, int nA, int nC) {
  static size_t attr[SK_BATCHED] = {};
  auto go = [&](auto kern, int threads, size_t lds_attr, const auto& args) -> int {
    if (attr[pl.id] < lds_attr) {
      PDEC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_attr));
      attr[pl.id] = lds_attr;
    }
    hipLaunchKernelGGL(kern, grid, dim3(threads), pl.lds, stream, args);
    PDEC_HIP(hipGetLastError());
    return PDEC_OK;
  };
  if (pl.id == SK_GENERIC) return go(ddpg_small_kernel, SM_THREADS, 160 * 1024, g);
  Small2Args a2{};
  a2.g = g;
  a2.g.lds_params = 0;
  a2.nC = nC; a2.nA = nA;
  switch (pl.id) {
#define X(ID, NAME, NS, BU, OS, EXACT, NWC, ...) case SK_##ID: return go(__VA_ARGS__, pl.threads, pl.lds, a2);
    SMALL2_KERNELS(X)
#undef X
    default: set_error("small update: no kernel for plan %d", (int)pl.id); return PDEC_E_INVALID;
  }
}

static int ddpg_update_small_impl(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* state_trace,
                                  const void* action_trace, const void* reward_trace, const void* terminal_trace,
                                  const int32_t* idx_s, const int32_t* idx_rt, const int32_t* idx_sn, int loops, int Bu,
                                  double gamma, double rho, int quirk, double eta_actor, double eta_critic,
                                  void* losses_dev, const SmallSampling* smp) {
  Mlp *A, *C, *At, *Ct;
  int rc;
  if ((rc = small_nets(hA, hC, hAt, hCt, &A, &C, &At, &Ct))) return rc;
  PDEC_REQUIRE(state_trace && action_trace && reward_trace && terminal_trace && (smp || (idx_s && idx_rt && idx_sn)),
               "pdec_ddpg_update_small: null argument");
  SmallPlan pl{};
  if ((rc = small_plan(A, C, loops, Bu, (float)rho, smp != nullptr, quirk, &pl))) return rc;
  PDEC_REQUIRE(pl.id != SK_BATCHED,
               "pdec_ddpg_update_small: reward groups g = %d, L = %d split the minibatch of %d; update through pdec_ddpg_update_async",
               C->rg_g, C->rg_L, Bu);
  SmallArgs g{};
  if ((rc = small_args(g, pl, A, C, At, Ct, loops, Bu, gamma, rho, quirk, eta_actor, eta_critic))) return rc;
  g.state = (const float*)state_trace; g.action = (const float*)action_trace;
  g.reward = (const float*)reward_trace; g.terminal = (const float*)terminal_trace;
  g.i_s = idx_s; g.i_rt = idx_rt; g.i_sn = idx_sn;
  if (smp) {
    const int64_t hi = smp->n_valid - smp->stride;           // inds in 1:length(t)-number_actuators (src/PDEagent.jl:318)
    PDEC_REQUIRE(hi >= 1 && hi < ((int64_t)1 << 32) && smp->capacity >= 1 && smp->stride >= 0,
                 "pdec_ddpg_update_small_rng: nothing to sample (valid %lld, stride %d)", (long long)smp->n_valid, smp->stride);
    g.smp_on = 1;
    g.smp_seed = smp->seed; g.smp_offset = smp->offset; g.smp_hi = (uint32_t)hi;
    g.smp_base = smp->n_rt > smp->capacity ? smp->n_rt - smp->capacity : 0;      // logical index of the oldest entry
    g.smp_cap = (int)smp->capacity; g.smp_cap1 = (int)(smp->capacity + smp->stride); g.smp_stride = smp->stride;
  }
  if ((rc = bp_begin(A, g.b1, g.b2, &g.bpA)) || (rc = bp_begin(C, g.b1, g.b2, &g.bpC))) return rc;
  g.losses = (float*)losses_dev;
  g.halt = C->halt;
  ProfScope ps(C, "ddpg_small");
  if ((rc = small_launch(pl, dim3(1), C->stream, g, A->dims[1], C->dims[1]))) return rc;
  bp_done(A);
  bp_done(C);
  A->fw_dirty = C->fw_dirty = At->fw_dirty = Ct->fw_dirty = true;
  return PDEC_OK;
}

// one launch of M workgroups: member m's small update with device-side sampling where its own trigger fires (sm_member_begin)
extern "C" int pdec_population_update(pdec_handle pop) {
  GET_POP(P, pop);
  Mlp *A = P->A[0], *C = P->C[0];
  SmallPlan pl{};
  int rc;
  if ((rc = small_plan(A, C, P->loops, P->Bu, (float)P->rho, true, P->quirk, &pl))) return rc;
  PDEC_REQUIRE(pl.id != SK_BATCHED, "pdec_population_update: reward groups that split the minibatch are not served");
  SmallArgs g{};
  if ((rc = small_args(g, pl, A, C, P->At[0], P->Ct[0], P->loops, P->Bu, P->gamma, P->rho, P->quirk, P->eta_a, P->eta_c))) return rc;
  g.smp_on = 1;
  g.smp_cap = (int)P->cap; g.smp_cap1 = (int)P->cap1; g.smp_stride = P->stride;
  g.pm = P->tab.as<PopMember>(); g.rows = P->rows;
  g.m_after = P->after; g.m_freq = P->freq; g.m_dsample = ((long long)P->loops * P->Bu + 3) / 4;
  PDEC_REQUIRE(!P->member_hyper || small_serves_member_hyper(pl),
               "pdec_population_update: %s does not serve per-member hyper-parameters (pdec_population_set_member_hyper)",
               small_kernel_names[pl.id]);
  g.m_hyper = P->member_hyper;
  ProfScope ps(P, "population_update");
  return small_launch(pl, dim3(P->M), P->stream, g, A->dims[1], C->dims[1]);
}

extern "C" int pdec_population_set_member_hyper(pdec_handle pop, int on) {
  GET_POP(P, pop);
  if (on) {
    SmallPlan pl{};
    int rc;
    if ((rc = small_plan(P->A[0], P->C[0], P->loops, P->Bu, (float)P->rho, true, P->quirk, &pl))) return rc;
    PDEC_REQUIRE(pl.id != SK_BATCHED && small_serves_member_hyper(pl),
                 "pdec_population_set_member_hyper: the update kernel of these networks (%s) takes one gamma, rho and pair of step "
                 "sizes for the whole launch: members of this shape cannot differ in them",
                 pl.id == SK_BATCHED ? "reward groups" : small_kernel_names[pl.id]);
  }
  P->member_hyper = on ? 1 : 0;
  return PDEC_OK;
}

extern "C" int pdec_debug_small_update_kernel(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, int loops, int Bu,
                                              double rho, int sampling, char* name, int name_len, int64_t* lds_bytes) {
  Mlp *A, *C, *At, *Ct;
  int rc;
  PDEC_REQUIRE(name && name_len > 0 && lds_bytes, "pdec_debug_small_update_kernel: null argument");
  if ((rc = small_nets(hA, hC, hAt, hCt, &A, &C, &At, &Ct))) return rc;
  SmallPlan pl{};
  if ((rc = small_plan(A, C, loops, Bu, (float)rho, sampling != 0, 1, &pl))) return rc;   // as a broadcast-target call would
  if (pl.id == SK_BATCHED) snprintf(name, name_len, "generic_path/reward_groups");
  else if (pl.id == SK_GENERIC) snprintf(name, name_len, "ddpg_small_kernel/lds_params=%d", pl.lds_params);
  else snprintf(name, name_len, "%s", small_kernel_names[pl.id]);
  *lds_bytes = (int64_t)pl.lds;
  return PDEC_OK;
}

extern "C" int pdec_ddpg_update_small(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* state_trace,
                                      const void* action_trace, const void* reward_trace, const void* terminal_trace,
                                      const int32_t* idx_s, const int32_t* idx_rt, const int32_t* idx_sn, int loops, int Bu,
                                      double gamma, double rho, int quirk, double eta_actor, double eta_critic,
                                      void* losses_dev) {
  return ddpg_update_small_impl(hA, hC, hAt, hCt, state_trace, action_trace, reward_trace, terminal_trace, idx_s, idx_rt, idx_sn,
                                loops, Bu, gamma, rho, quirk, eta_actor, eta_critic, losses_dev, nullptr);
}

extern "C" int pdec_ddpg_update_small_rng(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* state_trace,
                                          const void* action_trace, const void* reward_trace, const void* terminal_trace,
                                          int loops, int Bu, uint64_t seed, uint64_t offset, int64_t n_valid, int64_t n_rt,
                                          int64_t capacity, int stride, double gamma, double rho, int quirk, double eta_actor,
                                          double eta_critic, void* losses_dev) {
  SmallSampling smp{seed, offset, n_valid, n_rt, capacity, stride};
  return ddpg_update_small_impl(hA, hC, hAt, hCt, state_trace, action_trace, reward_trace, terminal_trace, nullptr, nullptr, nullptr,
                                loops, Bu, gamma, rho, quirk, eta_actor, eta_critic, losses_dev, &smp);
}
