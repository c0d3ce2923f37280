// mlp.hpp -- the MLP object shared by mlp.hip (generic path) and mlp_mfma.hip (fp32 MFMA path)
#pragma once
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "common.hpp"

namespace pdec {

struct Mlp : Object {
  int dtype = PDEC_F32, L = 0, max_cols = 0, nparams = 0;
  std::vector<int> dims, acts;
  std::vector<size_t> w_off, b_off;  // offsets into the flat buffers; W_l row-major [out][in], then b_l
  DevBuf params, grads, m, v;        // flat parameter / gradient / ADAM moment buffers
  // ADAM beta powers (Flux keeps Float64[beta1^t, beta2^t] beside the moments) are DEVICE resident and double-buffered:
  // every ADAM kernel reads slot `bp_sel` and ONE of its threads writes the advanced powers into the other slot, so
  // no launch argument depends on the step count and a captured HIP graph of the update replays unchanged (the
  // host only flips bp_sel, which returns to its captured value after an even number of steps).
  DevBuf bpd;                        // double [2][2]
  int bp_sel = 0;
  bool bp_init = false;
  hipEvent_t stop_event = nullptr;   // one-shot (pdec_mlp_set_stop_event): attached to the next reduction / update launch on this net
  hipEvent_t reduce_event = nullptr; // one-shot (pdec_mlp_set_reduce_event): attached to the next reduce-ONLY launch (flat gradient ready)
  const float* rpart_ext = nullptr;  // per-workgroup reward sums of the producer (pdec_ddpg_set_reward_partials), consumed likewise
  int rpart_n = 0;
  const void* rbar_ext = nullptr;    // batch-mean reward reduced elsewhere (pdec_ddpg_set_reward_mean), consumed by the next critic pass
  int rg_g = 0, rg_L = 1;            // reward groups of the broadcast target (pdec_ddpg_set_reward_groups; g = 0: off), sticky
  DevBuf rg_vals;                    // per-column group-mean reward [cols] + loss correction [1] (dtype of the net)
  DevBuf rg_work;                    // per-block partials of the correction (double) + the last-block counter (zero between launches)
  DevBuf noise_ctr;                  // uint64 [2]: double-buffered exploration-noise counter of pdec_policy_act_rng_dev
  int nc_sel = 0;
  int noise_rows = -1;   // pdec_mlp_set_noise_rows: exploration noise on the first rows of the output only (-1: all)
  std::vector<DevBuf> H;             // activations, feature-major [dims[l]][cols]
  DevBuf dz[2];                      // ping-pong dL/dz buffers [maxdim][cols]
  DevBuf dy;                         // dL/dy of the output layer [dims[L]][cols]
  DevBuf slabs;                      // split-K partial weight gradients
  DevBuf scratch;                    // loss statistics / device scalars
  int kchunk = 512, nsplit_max = 0, dx_index = 0;
  DevBuf fw, fslab;                  // fused-path padded weight image / per-workgroup gradient slabs
  DevBuf stamps;                     // diagnostic phase stamps (PDEC_STAMPS=1)
  bool stamps_armed = false;         // pdec_debug_critic_stamps: the next critic pass on this net records its stamps ...
  double stamps_last[13] = {0};      // ... here: 10 phase means, total cycles, shader clock (GHz), workgroups
  DevBuf noise;                      // internal exploration-noise buffer (pdec_policy_act_rng fallback)
  bool fw_dirty = true;
  DevBuf fw_pub[2];                  // published copies of the image for concurrent acting kernels
  int pub = 0;

  Mlp() : Object(Kind::Mlp) {}
  int init(int dtype, int L, const int32_t* dims, const int32_t* acts, int max_cols);
  template <class T>
  int pack(const void* s1, int n1, int l1, const void* s2, int n2, int l2, int cols);
  template <class T>
  int forward(int cols);
  template <class T>
  int backward(const void* dy, int ldy, int cols, bool want_dw, bool want_dx, double grad_scale);
  template <class T>
  T* dy_buf(int) { return dy.as<T>(); }
};

// ---- populations (pdec_population_create, population.py): M independent single-trajectory learners whose per-step launches
// are ONE launch of M workgroups each.  Workgroup m reads member m's pointers from a device table (PopMember) and its counters
// from row m of a device int64 table that the host writes once per episode and reads back once per episode.
#define POP_ROW 16
enum PopSlot {
  POP_USTEP = 0,    // policy.update_step
  POP_NSA,          // trajectory.n_sa
  POP_NRT,          // trajectory.n_rt
  POP_NOISE,        // policy._noise_off (Philox counters of the exploration noise)
  POP_SAMPLE,       // policy._sample_off (Philox counters of the minibatch draws)
  POP_HALT,         // the member's episode halt flag (low 32 bits; pdec_set_episode_halt's protocol)
  POP_ACTIVE,       // 1: the member runs this episode (0: its stop condition has fired)
  POP_BPA,          // slot of the actor's / critic's double-buffered ADAM beta powers (Mlp::bp_sel)
  POP_BPC,
  POP_NOISE_AMP,    // act_noise, act_limit (bit patterns of doubles)
  POP_LIMIT,
};
// a member's own hyper-parameters (bit patterns of doubles), read by the small update's prologue (sm_member_begin) when
// pdec_population_set_member_hyper is on; with it off the launch-wide values of pdec_population_create hold and the slots are
// not read.  Slot 15 stays free.
enum PopHyperSlot {
  POP_GAMMA = 11,   // policy.y
  POP_RHO,          // policy.rho_effective
  POP_ETA_A,        // behaviour actor's / critic's ADAM step size
  POP_ETA_C,
};
// ---- a member's book (pdec_population_episode_close, csrc/pop_book.hip): what its PDEhook and its stop condition hold between
// two episodes, so that the episode boundary needs no host.  A caller-owned device table int64 [M][POP_BOOK] beside the rows,
// doubles as bit patterns; population.py mirrors the names (tests/test_population_blocks_host.py compares them).
#define POP_BOOK 16
enum PopBookSlot {
  PBK_EP = 0,        // hook.ep: index of the episode that is running (the close increments it)
  PBK_MIN_BEST,      // hook.min_best_episode
  PBK_COLLECT_NNA,   // hook.collect_NNA (0 / 1)
  PBK_CMP_HAS,       // 1: rewards_compare is not empty
  PBK_CMP,           // Python's max(rewards_compare) (double): the first element unless a later one compared greater
  PBK_BESTREWARD,    // hook.bestreward (double)
  PBK_BESTEPISODE,   // hook.bestepisode
  PBK_STOP_KIND,     // 0: StopAfterEpisode, 1: StopAfterEpisodeWithMinSteps
  PBK_STOP_CUR,      // the stop object's cur
  PBK_STOP_LIMIT,    // its episode / step
  PBK_RANDOM_INIT,   // hook.use_random_init (0 / 1)
  PBK_INIT_SEED,     // hook.init_seed
  PBK_INIT_OFF,      // hook._init_off: Philox offset of the member's NEXT initial field
  PBK_INIT_INC,      // ceil(coefficients / 4): what one drawn field consumes
  PBK_FIRED,         // phase 0 -> phase 1 of one close: the stop condition fired in this episode
  PBK_SPARE,
};
// the episode log of a block, int64 [E][M][POP_ELOG]: one entry per member and episode
#define POP_ELOG 4
enum PopElogSlot {
  PEL_REWARD = 0,    // the episode reward (double)
  PEL_STEPS,         // executed control steps n (0: the member was idle)
  PEL_NEW_BEST,      // 1: the episode is the member's new best
  PEL_RAN,           // 1: the member ran this episode
};
struct PopMember {
  const void* actor_p;                         // behaviour actor parameters (acting)
  float *ts, *ta, *tr, *tt;                     // replay traces: state, action, reward, terminal
  uint64_t noise_seed, sample_seed;
  float *Ap, *Ag, *Am, *Av, *Apt, *Cp, *Cg, *Cm, *Cv, *Cpt;   // the small update's learner state
  double *bpA, *bpC;                            // [2][2] beta powers
  float* losses;                                // [2]
};
// one destination of pdec_population_clone: member `dst` takes over member `src`'s learner; bp*: the CURRENT beta-power slots
// (Mlp::bp_sel) of the two members' actors / critics, rows_*: the replay rows that go along (0: the destination keeps its replay)
struct PopClone {
  int src, dst, bpa_src, bpc_src, bpa_dst, bpc_dst;
  long long rows_sa, rows_rt;
};

// the activations of a Dense layer, as every forward pass of the library applies them (gemm_kernel's epilogue, the acting kernels)
template <class T>
__device__ __forceinline__ T apply_act(T z, int act) {
  if (act == PDEC_ACT_RELU) return z > 0 ? z : (T)0;
  if (act == PDEC_ACT_TANH) return (T)tanh((double)z);
  return z;
}
template <>
__device__ __forceinline__ float apply_act<float>(float z, int act) {
  if (act == PDEC_ACT_RELU) return z > 0 ? z : 0.0f;
  if (act == PDEC_ACT_TANH) return tanhf(z);
  return z;
}

// ---- acting for few columns (mlp.hip: small_act_kernel) and its member form (act_members.hip: act_members_kernel)
#define SMALL_ACT_MAXL 4                 // layers the two kernels take
#define SMALL_ACT_LDS (48 * 1024)        // bytes of LDS they allow themselves: two activation buffers [widest layer][columns]
int mlp_maxw(const Mlp* M);              // the widest layer, input included
// would pdec_policy_act_rng on `cols` states of M take a fused MFMA acting kernel (act_route: ACT_FUSED3 / ACT_FUSED2)?  Those sum
// in another order than small_act_kernel / gemm_kernel do.
bool act_route_is_fused(const Mlp* M, int cols);

// Philox4x32-10 counter-based generator (the exploration noise that replaces randn(rng), src/PDEagent.jl:201)
__device__ __forceinline__ void philox4x32(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// ---- the exploration-noise stream (seed, offset): Philox block `offset + (i >> 2)` holds the normals 4 (i >> 2) .. + 3, two
// Box-Muller pairs (cos, sin) from its halves.  Every acting path draws through these pieces, so that the step loop, the
// persistent rollouts and randn + act see the same numbers element for element.
__device__ __forceinline__ void noise_block(uint32_t (&ph)[4], uint64_t seed, uint64_t ctr) {
  ph[0] = (uint32_t)ctr; ph[1] = (uint32_t)(ctr >> 32); ph[2] = 0u; ph[3] = 0u;
  philox4x32(ph, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// Box-Muller radius and angle of half h (0 / 1) of a block
__device__ __forceinline__ void noise_polar(const uint32_t (&ph)[4], int h, double& rad, double& ang) {
  const double sc = 1.0 / 4294967296.0;
  const double u1 = ((double)ph[2 * h] + 0.5) * sc, u2 = ((double)ph[2 * h + 1] + 0.5) * sc;
  rad = sqrt(-2.0 * log(u1)); ang = 6.283185307179586 * u2;
}
// normal number i of the stream (I: the index type of the caller, kept so that its index arithmetic stays what it was)
template <class I>
__device__ __forceinline__ double noise_normal(uint64_t seed, uint64_t offset, I i) {
  uint32_t ph[4];
  noise_block(ph, seed, offset + (uint64_t)(i >> 2));
  double rad, ang;
  noise_polar(ph, (int)((i >> 1) & 1), rad, ang);
  return (i & 1) ? rad * sin(ang) : rad * cos(ang);
}

// kernel-side view of the beta powers: read `cur` (every thread that needs it), one thread of the grid writes `next`
struct BpArgs {
  const double* cur;
  double* next;
};
// slots for the next ADAM kernel on M (uploads {beta1, beta2} on the first step: Flux initialises the powers with the
// betas themselves); the caller flips M->bp_sel after enqueueing the kernel (bp_done)
int bp_begin(Mlp* M, double beta1, double beta2, BpArgs* out);
inline void bp_done(Mlp* M) { flip(M->bp_sel); }
__device__ __forceinline__ void bp_advance(const BpArgs& a, double b1, double b2, int times = 1) {
  double p0 = a.cur[0], p1 = a.cur[1];
  for (int i = 0; i < times; ++i) { p0 *= b1; p1 *= b2; }
  a.next[0] = p0;
  a.next[1] = p1;
}

// Reward groups (pdec_ddpg_set_reward_groups).  For a broadcast-target critic pass (quirk = 1) of Bu columns that the groups
// split (2 <= g, g L < Bu) this enqueues on C's stream the per-column group means rg and the loss correction
// mean_c (r_c - rg_c)^2, and returns the arguments of the pass that gives the grouped gradient: the diagonal target
// (quirk 0) on rg, the correction added to the loss.  g = 1 -> the diagonal pass on r; off, or g L >= Bu -> the arguments
// unchanged (whole-batch broadcast).  Refuses Bu % (g L) != 0.  Idempotent: a second call on its own output changes nothing.
struct CriticRoute {
  const void* r;
  int quirk;
  const void* loss_add;    // device scalar of the net's dtype added to the critic loss, or null
};
int reward_group_route(Mlp* C, const void* r, int Bu, int quirk, CriticRoute* out);

// a padded tile count as a type: the dispatch of the fused passes hands the instantiation it picked to a generic lambda, so the
// launch and the report of pdec_debug_batched_update_route go through one chain of comparisons
template <int N>
using tile_c = std::integral_constant<int, N>;

// mlp_mfma.hip: fused fp32 MFMA DDPG passes (3-layer actor/critic pairs)
struct AdamPolyak {
  double eta, b1, b2, eps, rho;
};
bool fused_supported(const Mlp* A, const Mlp* C);
bool fused_net_supported(const Mlp* M);
// apply != nullptr: the slab reduction also performs ADAM on the network, Polyak into its target and refreshes
// the padded weight images (single-GPU path: no all-reduce between gradient and update)
int fused_critic_grads(Mlp* A, Mlp* C, Mlp* At, Mlp* Ct, const void* s, const void* a, const void* r, const void* t,
                       const void* sn, int Bu, double gamma, int quirk, double grad_scale, void* loss_dev,
                       const AdamPolyak* apply, const void* loss_add = nullptr);
int fused_actor_grads(Mlp* A, Mlp* C, Mlp* At, const void* s, int Bu, double grad_scale, void* loss_dev,
                      const AdamPolyak* apply);
int fused_adam_polyak(Mlp* M, Mlp* Mt, const AdamPolyak& ap);
// flat parameters of the published image the next acting kernel reads (fw_pub[pub]), enqueued on `stream`
int fused_unpack_published(Mlp* A, float* flat_out, hipStream_t stream);
// ctr_cur != null: the noise offset is *ctr_cur (+ offset) and one thread writes *ctr_next = that + ctr_inc
int fused_policy_act(Mlp* A, const void* state, int cols, double act_noise, double act_limit, int learning,
                     uint64_t seed, uint64_t offset, void* actions_out, const uint64_t* ctr_cur = nullptr,
                     uint64_t* ctr_next = nullptr, uint64_t ctr_inc = 0);

// kernel name and dynamic LDS bytes of the pass / acting launch the functions above would make (nothing is launched)
int fused_describe(const Mlp* A, const Mlp* C, bool actor_pass, char* name, int name_len, int64_t* lds);
int fused_act_describe(const Mlp* A, char* name, int name_len, int64_t* lds);

// mlp_mfma2.hip: the same passes for the reference-shaped 2-layer nets [ns, h, 1] / [ns+1, H, 1] (flat parameters, no image)
// mean of r[0..n) in a fixed order, one block; *out = device scalar owned by C (mlp_mfma2.hip)
int launch_rmean(Mlp* C, const float* r, int n, float** out);
bool fused2_supported(const Mlp* A, const Mlp* C);
bool fused2_net_supported(const Mlp* M);
bool fused2_act_supported(const Mlp* A, int cols);
int fused2_policy_act(Mlp* A, const void* state, int cols, double act_noise, double act_limit, int learning, uint64_t seed,
                      uint64_t offset, void* actions_out, const uint64_t* ctr_cur = nullptr, uint64_t* ctr_next = nullptr,
                      uint64_t ctr_inc = 0);
int fused2_adam_polyak(Mlp* M, Mlp* Mt, const AdamPolyak& ap);
int fused2_critic_grads(Mlp* A, Mlp* C, Mlp* At, Mlp* Ct, const void* s, const void* a, const void* r, const void* t,
                        const void* sn, int Bu, double gamma, int quirk, double grad_scale, void* loss_dev,
                        const AdamPolyak* apply, const void* loss_add = nullptr);
int fused2_actor_grads(Mlp* A, Mlp* C, Mlp* At, const void* s, int Bu, double grad_scale, void* loss_dev,
                       const AdamPolyak* apply);

int fused2_describe(const Mlp* A, const Mlp* C, bool actor_pass, char* name, int name_len, int64_t* lds);
int fused2_act_describe(const Mlp* A, char* name, int name_len, int64_t* lds);

struct Population : Object {
  int M = 0, cols = 0, dtype = PDEC_F64;
  std::vector<Mlp*> A, C, At, Ct;
  DevBuf tab;                        // PopMember [M]
  DevBuf clones;                     // PopClone [M] (pdec_population_clone)
  DevBuf snap;                       // float* [M][2]: the hooks' best / current actor parameters (pdec_population_set_actor_copies)
  std::vector<Mlp*> snap_nets;       // (their objects: a copy makes their derived images stale)
  long long* rows = nullptr;         // [M][POP_ROW] (the caller's device buffer)
  long long cap = 0, cap1 = 0, after = 0, freq = 1, start_steps = 0;
  int stride = 0, loops = 1, Bu = 1, quirk = 0;
  double gamma = 0.99, rho = 1.0, eta_a = 0, eta_c = 0;   // member 0's at creation: they select the kernel, and hold for
  int member_hyper = 0;                                    // every member unless member_hyper (pdec_population_set_member_hyper)
  Population() : Object(Kind::Population) {}
};

}  // namespace pdec

// the population behind handle h at an entry point (the GET_MLP of populations; here because mlp.hip and mlp_small.hip
// both have population entry points)
#define GET_POP(P, h)                                                           \
  pdec::Population* P = pdec::lookup_as<pdec::Population>(h, pdec::Kind::Population); \
  if (!P) {                                                                     \
    pdec::set_error("%s: bad handle", __func__);                                \
    return PDEC_E_HANDLE;                                                       \
  }
