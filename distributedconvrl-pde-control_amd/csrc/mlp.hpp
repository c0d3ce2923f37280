// mlp.hpp -- the MLP object, what every acting path and every ADAM kernel share (activations, the exploration-noise stream, the
// beta powers) and the table of a fused DDPG kernel family.  For every file that holds an Mlp*: mlp.hip (generic path), ddpg.hip
// (DDPG passes and their routing), act.hip (acting), mlp_mfma.hip with fused3_*.hpp / mlp_mfma2.hip with fused2_*.hpp (the two fused families), and the rollout,
// replay, ledger, communicator and population files
#pragma once
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "common.hpp"

namespace pdec {

struct AdamPolyak {
  double eta, b1, b2, eps, rho;
};

// The finish launch of a fused 3-layer actor pass that has not been issued yet (pdec_ddpg_defer_actor_finish): what
// launch_finish needs to issue it later, alone (pdec_ddpg_flush_actor_finish) or as extra blocks of the next critic finish
struct PendingFinish {
  bool on = false;
  const float* slabs = nullptr;      // the actor's slab buffer as the pass left it
  int nslab = 0, mta = 0, Bu = 0;
  double scale = 1.0;
  void* loss = nullptr;
  AdamPolyak ap{};
  hipEvent_t stop = nullptr;         // the one-shot stop event that was set on the net when its pass was launched
};

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
  const double* noise_scale = nullptr;   // pdec_mlp_set_noise_scale: the caller's device array of amplitudes (null: the call's scalar)
  int64_t noise_scale_n = 0;             // its entries; an acting call then has noise_scale_n * noise_scale_cpe columns
  int noise_scale_cpe = 1;
  double* noise_color = nullptr;         // pdec_mlp_set_noise_color: the caller's device array of AR(1) states (null: white noise)
  const double* noise_color_ab = nullptr;  // its {a, b} per entry
  int64_t noise_color_n = 0;             // entries; an acting call then has noise_color_n * noise_color_cpe columns
  int noise_color_cpe = 1;
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
  bool defer_finish = false;         // pdec_ddpg_defer_actor_finish: armed (actor nets of the fused 3-layer family)
  PendingFinish pend;
  int n_paired = 0;                  // finish launches of this net that were blocks of a critic's finish launch (tests)

  Mlp() : Object(Kind::Mlp) {}
  int init(int dtype, int L, const int32_t* dims, const int32_t* acts, int max_cols);
  // in the net's dtype (mlp.hip)
  int pack(const void* s1, int n1, int l1, const void* s2, int n2, int l2, int cols);
  int forward(int cols);
  int backward(const void* dy, int ldy, int cols, bool want_dw, bool want_dx, double grad_scale);
  template <class T>
  T* dy_buf(int) { return dy.as<T>(); }
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

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- acting for few columns (act.hip: small_act_kernel) and its member form (act_members.hip: act_members_kernel)
#define SMALL_ACT_MAXL 4                 // layers the two kernels take
#define SMALL_ACT_LDS (48 * 1024)        // bytes of LDS they allow themselves: two activation buffers [widest layer][columns]
int mlp_maxw(const Mlp* M);              // the widest layer, input included
// what serves pdec_policy_act_rng for `cols` states where no fused family does (act.hip)
enum ActRoute { ACT_GENERIC = 0, ACT_SMALL };
ActRoute act_route(const Mlp* M, int cols);
// n normals of the stream (seed, offset) into dst on o's stream (mlp.hip: randn_kernel); ctr_cur != null: the device-resident
// counter of pdec_policy_act_rng_dev, see FusedFamily::policy_act
int launch_randn(Object* o, void* dst, size_t n, int dtype, uint64_t seed, uint64_t offset, const uint64_t* ctr_cur,
                 uint64_t* ctr_next, uint64_t ctr_inc);
// pdec_policy_act with the noise in `noise_dtype` (mlp.hip).  A state array set on M (pdec_mlp_set_noise_color) is advanced with
// noise[] as z, read as doubles: pdec_policy_act_rng draws them so, a caller's fp32 noise is converted first
int policy_act_noise(Mlp* M, const void* state, const void* noise, int noise_dtype, int cols, double act_noise,
                     double act_limit, void* actions_out, const char* who);

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

// ---- the exploration amplitude of a column as a kernel receives it: the launch scalar (the default instantiations, whose text
// and arguments are what they were before the array existed), or NoiseScale -- entry c / cols_per_entry of the device array of
// pdec_mlp_set_noise_scale, converted to the kernel's type as the scalar is ((T)act_noise: an array of equal values is the
// scalar call bit for bit)
struct NoiseScale {
  const double* scale;
  int cols_per_entry;
};
template <class T, class S, class I>
__device__ __forceinline__ T noise_amp(S a, I) { return (T)a; }
template <class T, class I>
__device__ __forceinline__ T noise_amp(NoiseScale s, I c) { return (T)s.scale[c / s.cols_per_entry]; }
inline NoiseScale noise_scale_of(const Mlp* M) { return NoiseScale{M->noise_scale, M->noise_scale_cpe}; }
// the number a kernel multiplies by the amplitude: the normal z of element i, converted to the kernel's type
template <class T, class S, class Z, class I, class J>
__device__ __forceinline__ T noise_draw(S, Z z, I, J) { return (T)z; }

// ---- temporally correlated noise (pdec_mlp_set_noise_color): the third carrier.  Element i = column * outputs + row keeps an
// AR(1) state x[i] in the caller's device array, a double whatever the kernel's type; a learning call advances it with the normal
// z the white call draws for that element, x = a_e x + b_e z (e = column / cols_per_entry), stores it, and adds (T)x times the
// amplitude -- entry e of the scale array where one is set too, the call's scalar otherwise (chosen at run time: ONE
// instantiation per kernel).  The lane that draws z owns x[i], so the load and the store need no synchronisation.  a = 0, b = 1
// gives x = z exactly, and such a call is the white call bit for bit.
struct NoiseColor {
  double* state;
  const double* ab;
  int cols_per_entry;
  const double* scale;
  double amp;
};
template <class T, class I>
__device__ __forceinline__ T noise_amp(const NoiseColor& k, I c) { return (T)(k.scale ? k.scale[c / k.cols_per_entry] : k.amp); }
template <class T, class Z, class I, class J>
__device__ __forceinline__ T noise_draw(const NoiseColor& k, Z z, I c, J i) {
  const double* ab = k.ab + 2 * (size_t)(c / k.cols_per_entry);
  const double x = ab[0] * k.state[i] + ab[1] * (double)z;
  k.state[i] = x;
  return (T)x;
}
// the element type of the noise[] an acting sequence hands to its last kernel: the kernel's own, or z as it is drawn
template <class T, class AN>
using noise_elem_t = std::conditional_t<std::is_same<AN, NoiseColor>::value, double, T>;
inline NoiseColor noise_color_of(const Mlp* M, double act_noise) {
  return NoiseColor{M->noise_color, M->noise_color_ab, M->noise_color_cpe, M->noise_scale, act_noise};
}
// is AN one of the carriers that hold an amplitude per column?
template <class AN>
inline constexpr bool noise_per_column = std::is_same<AN, NoiseScale>::value || std::is_same<AN, NoiseColor>::value;

// an acting call of `cols` columns against the arrays set on M (none set: fine)
#define PDEC_REQUIRE_NOISE_COLS(M, cols, who)                                                                                    \
  do {                                                                                                                           \
    PDEC_REQUIRE(!(M)->noise_scale || (long long)(cols) == (long long)(M)->noise_scale_n * (M)->noise_scale_cpe,                 \
                 "%s: %d columns, but the noise scale set on the actor serves %lld entries x %d columns = %lld", who, (int)(cols), \
                 (long long)(M)->noise_scale_n, (M)->noise_scale_cpe, (long long)(M)->noise_scale_n * (M)->noise_scale_cpe);     \
    PDEC_REQUIRE(!(M)->noise_color || (long long)(cols) == (long long)(M)->noise_color_n * (M)->noise_color_cpe,                 \
                 "%s: %d columns, but the noise color set on the actor serves %lld entries x %d columns = %lld", who, (int)(cols), \
                 (long long)(M)->noise_color_n, (M)->noise_color_cpe, (long long)(M)->noise_color_n * (M)->noise_color_cpe);     \
    PDEC_REQUIRE(!(M)->noise_color || !(M)->noise_scale || (M)->noise_color_cpe == (M)->noise_scale_cpe,                         \
                 "%s: the noise color set on the actor has %d columns per entry, its noise scale %d: they must be equal", who,   \
                 (M)->noise_color_cpe, (M)->noise_scale_cpe);                                                                    \
  } while (0)
// an entry that explores, or runs members, and has no AR(1) state to advance
#define PDEC_REFUSE_NOISE_COLOR(M, who, why)                                                                            \
  PDEC_REQUIRE(!(M)->noise_color, "%s: a noise color is set on the actor (pdec_mlp_set_noise_color); %s", who, why)

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

// ---- a fused DDPG kernel family: fp32 MFMA passes, apply and acting kernels for one class of actor / critic pairs.  Two exist:
// fused3_family (mlp_mfma.hip, kernels in fused3_*.hpp: 3-layer pairs on padded weight images) and fused2_family (mlp_mfma2.hip,
// kernels in fused2_*.hpp: the reference-shaped 2-layer nets [ns, h, 1] / [ns+1, H, 1] on the flat parameters).  ddpg.hip and act.hip pick one through the selectors below and
// call through the table; null = the generic path.
struct FusedFamily {
  bool (*pair_ok)(const Mlp* A, const Mlp* C);   // the passes serve this actor / critic pair
  bool (*net_ok)(const Mlp* M);                  // adam_polyak serves this net
  bool (*act_ok)(const Mlp* M, int cols);        // policy_act serves `cols` states of this actor
  int apply_min_bu;                              // pdec_ddpg_update_async applies ADAM + Polyak in the finish launch from this batch on
  // apply != nullptr: the slab reduction also performs ADAM on the network, Polyak into its target and refreshes
  // the padded weight images (single-GPU path: no all-reduce between gradient and update)
  int (*critic_grads)(Mlp* A, Mlp* C, Mlp* At, Mlp* Ct, const void* s, const void* a, const void* r, const void* t,
                      const void* sn, int Bu, double gamma, int quirk, double grad_scale, void* loss_dev,
                      const AdamPolyak* apply, const void* loss_add);
  int (*actor_grads)(Mlp* A, Mlp* C, Mlp* At, const void* s, int Bu, double grad_scale, void* loss_dev,
                     const AdamPolyak* apply);
  int (*adam_polyak)(Mlp* M, Mlp* Mt, const AdamPolyak& ap);
  // ctr_cur != null: the noise offset is *ctr_cur (+ offset) and one thread writes *ctr_next = that + ctr_inc.  With an array set
  // on A (pdec_mlp_set_noise_scale) the launch takes the kernel's NoiseScale instantiation and act_noise is not read; with a
  // state array set (pdec_mlp_set_noise_color) and learning != 0 its NoiseColor instantiation
  int (*policy_act)(Mlp* A, const void* state, int cols, double act_noise, double act_limit, int learning, uint64_t seed,
                    uint64_t offset, void* actions_out, const uint64_t* ctr_cur, uint64_t* ctr_next, uint64_t ctr_inc);
  // kernel name and dynamic LDS bytes of the pass / acting launch the functions above would make (nothing is launched)
  int (*describe)(const Mlp* A, const Mlp* C, bool actor_pass, char* name, int name_len, int64_t* lds);
  int (*act_describe)(const Mlp* A, char* name, int name_len, int64_t* lds);
};
extern const FusedFamily fused3_family, fused2_family;
// the family that serves a pair's passes / a net's apply / an acting call, asked in the order 3-layer, 2-layer (ddpg.hip)
const FusedFamily* fused_family_of_pair(const Mlp* A, const Mlp* C);
const FusedFamily* fused_family_of_net(const Mlp* M);
const FusedFamily* fused_family_of_act(const Mlp* M, int cols);
// would pdec_policy_act_rng on `cols` states of M take a fused MFMA acting kernel?  Those sum in another order than
// small_act_kernel / gemm_kernel do.
inline bool act_route_is_fused(const Mlp* M, int cols) { return fused_family_of_act(M, cols) != nullptr; }

// features of the 3-layer image, not of "a family" (mlp_mfma.hip, fused3_image.hpp): the net predicate (stop / reduce events, reward partials) and
// the flat parameters of the published image the next acting kernel reads (fw_pub[pub]), enqueued on `stream`
bool fused_net_supported(const Mlp* M);
int fused_unpack_published(Mlp* A, float* flat_out, hipStream_t stream);
// the pending finish of A as a launch of its own on A's stream (no-op when nothing is pending)
int fused_flush_pending(Mlp* A);
// an entry that reads what a pending finish has yet to write (the actor's image, its published copy, its parameters)
#define PDEC_REQUIRE_NO_PENDING(M, who)                                                                                     \
  PDEC_REQUIRE(!(M)->pend.on, "%s: the actor's finish launch is still pending (pdec_ddpg_defer_actor_finish): flush it first " \
                              "(pdec_ddpg_flush_actor_finish)", who)
// mean of r[0..n) in a fixed order, one block; *out = device scalar owned by C (ddpg.hip; both fused families call it)
int launch_rmean(Mlp* C, const float* r, int n, float** out);

}  // namespace pdec

// the network behind handle h at an entry point
#define GET_MLP(M, h)                                            \
  pdec::Mlp* M = pdec::lookup_as<pdec::Mlp>(h, pdec::Kind::Mlp); \
  if (!M) {                                                      \
    pdec::set_error("%s: not an mlp handle", __func__);          \
    return PDEC_E_HANDLE;                                        \
  }
