// roll_actor.hpp -- the in-kernel actor of the persistent rollouts (ks_rollout.hip: ks_rollout_kernel, kseg.hip:
// kseg_rollout_kernel) and the host plumbing their two launchers share
#pragma once
#include "env.hpp"
#include "mlp.hpp"

namespace pdec {

#define RO_W 32            // widest layer the in-kernel actor holds in registers
struct RollActor {
  const void* params;      // flat [W1 row-major [out][in], b1, W2, b2, ...] in the environment's dtype
  int L, nparams, rows;    // rows = widest layer: the height of an activation plane
  int dims[4], acts[3];
};
// member form (pdec_rollout_members): the batch is M blocks of K trajectories, block m driven by the actor whose flat
// parameters params[m] points to; all M actors have the shape of the RollActor argument.  Greedy (no exploration noise).
struct RollMembers {
  const void* const* params;   // device table [M]
  int K;                       // trajectories per member
  int f32;                     // the parameters are Float32 whatever the environment's dtype (promoted while the image is filled)
};
// AN: what carries the exploration amplitude -- the launch scalar, or NoiseScale (pdec_mlp_set_noise_scale)
template <class T, class AN = T>
struct RollArgs {
  int steps, learning;
  AN act_noise;
  T act_limit;
  uint64_t seed, offset;
  T *y, *state, *action;                   // in / out: [B][N], [B][A][ns], [B][A]
  T* reward_sum;                           // optional [B][A]: += every step's reward
  T *log_y, *log_p, *log_action, *log_reward;   // optional [steps][B][...]
  int32_t *done_any, *done_step;           // optional [B]
  int control_from;                        // pdec_env_set_control_from: steps t < control_from take the zero action, unrewarded
};

template <class T>
__device__ __forceinline__ T ro_act_fn(T z, int act) {
  if (act == PDEC_ACT_RELU) return z > (T)0 ? z : (T)0;
  if (act == PDEC_ACT_TANH) return (T)tanh((double)z);
  return z;
}
template <>
__device__ __forceinline__ float ro_act_fn<float>(float z, int act) {
  if (act == PDEC_ACT_RELU) return fmaxf(z, 0.f);
  if (act == PDEC_ACT_TANH) return tanhf(z);
  return z;
}

// LDS image of the actor: per layer Wt[din][RO_W] (transposed, outputs zero-padded to RO_W) followed by b[RO_W], so the
// RO_NB consecutive outputs a thread owns are contiguous (broadcast 128-bit reads).
#define RO_NB 16
__host__ __device__ inline int ro_image_elems(const int* dims, int L) {
  int n = 0;
  for (int l = 0; l < L; ++l) n += (dims[l] + 1) * RO_W;
  return n;
}
// S: the type of the flat parameters; S = float into T = double promotes exactly (what pdec_mlp_copy's cast would store)
template <class T, class S = T>
__device__ __forceinline__ void ro_load_image(const RollActor& A, const void* params, T* wl, int tid, int nt) {
  const S* src = static_cast<const S*>(params);
  int so = 0, dof = 0;
  for (int l = 0; l < A.L; ++l) {
    const int din = A.dims[l], dout = A.dims[l + 1];
    for (int i = tid; i < (din + 1) * RO_W; i += nt) {
      const int r = i / RO_W, o = i - r * RO_W;                    // r < din: weight row, r == din: bias
      wl[dof + i] = o < dout ? (T)(r < din ? src[so + o * din + r] : src[so + din * dout + o]) : (T)0;
    }
    so += din * dout + dout;
    dof += (din + 1) * RO_W;
  }
}

// actor forward for ONE PAIR of adjacent columns per thread (packed v_pk_fma_f32 for fp32): the activations of the pair
// sit in two LDS planes hb[plane][i][slot] private to the thread (bank = lane: conflict-free, no barrier between layers),
// the weights are broadcast 128-bit reads of the image; outputs in blocks of RO_NB accumulators, inputs four at a time so
// the LDS reads of four k-steps are in flight together; k-ordered accumulation like the oracle's W * x + b.
template <class T> struct RoPair {
  typedef T type __attribute__((ext_vector_type(2)));
  typedef T quad __attribute__((ext_vector_type(4), aligned(16)));
};
// NB outputs [ob, ob + NB) of one layer for the thread's column pair: acc = b + sum_i W[.][i] * in[i]
template <class T, int NB>
__device__ __forceinline__ void ro_block(const T* __restrict__ Wt, int din, int dout, int ob, int act,
                                         const typename RoPair<T>::type* pin, typename RoPair<T>::type* pout, int nslot) {
  using T2 = typename RoPair<T>::type;
  using T4 = typename RoPair<T>::quad;
  T2 acc[NB];
  T4 w[4][NB / 4];
#pragma unroll
  for (int v = 0; v < NB / 4; ++v) {
    const T4 b4 = *reinterpret_cast<const T4*>(Wt + din * RO_W + 4 * v);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[4 * v + r] = T2{b4[r], b4[r]};
  }
  int i = 0;
  for (; i + 4 <= din; i += 4) {
    T2 a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = pin[(size_t)(i + u) * nslot];
#pragma unroll
      for (int v = 0; v < NB / 4; ++v) w[u][v] = *reinterpret_cast<const T4*>(Wt + (i + u) * RO_W + 4 * v);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[j] += w[u][j >> 2][j & 3] * a[u];
  }
  for (; i < din; ++i) {
    const T2 a0 = pin[(size_t)i * nslot];
#pragma unroll
    for (int v = 0; v < NB / 4; ++v) w[0][v] = *reinterpret_cast<const T4*>(Wt + i * RO_W + 4 * v);
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] += w[0][j >> 2][j & 3] * a0;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j)
    if (ob + j < dout) pout[(size_t)(ob + j) * nslot] = T2{ro_act_fn<T>(acc[j].x, act), ro_act_fn<T>(acc[j].y, act)};
}
template <class T>
__device__ __forceinline__ typename RoPair<T>::type ro_actor_pair(const RollActor& A, const T* __restrict__ wl,
                                                                  typename RoPair<T>::type* hb, int slot, int nslot) {
  using T2 = typename RoPair<T>::type;
  T2* pin = hb + slot;
  T2* pout = hb + (size_t)A.rows * nslot + slot;
  int off = 0;
  for (int l = 0; l < A.L; ++l) {
    const int din = A.dims[l], dout = A.dims[l + 1], act = A.acts[l];
    int ob = 0;
    for (; dout - ob > 4; ob += RO_NB) ro_block<T, RO_NB>(wl + off + ob, din, dout, ob, act, pin, pout, nslot);
    if (ob < dout) ro_block<T, 4>(wl + off + ob, din, dout, ob, act, pin, pout, nslot);
    T2* tmp = pin; pin = pout; pout = tmp;
    off += (din + 1) * RO_W;
  }
  return pin[0];
}


// ------------------------------------------------------------------ host side of the two launchers
inline RollActor make_roll_actor(const Mlp& A) {
  RollActor ra{};
  ra.params = A.params.p; ra.L = A.L; ra.nparams = A.nparams;
  for (int l = 0; l <= A.L; ++l) { ra.dims[l] = A.dims[l]; ra.rows = std::max(ra.rows, A.dims[l]); }
  for (int l = 0; l < A.L; ++l) ra.acts[l] = A.acts[l];
  return ra;
}
template <class T, class AN = T>
RollArgs<T, AN> make_roll_args(const RollSpec& s, const RollPtrs& p) {
  AN amp;
  if constexpr (std::is_same<AN, NoiseScale>::value) amp = NoiseScale{s.noise_scale, s.noise_cpe};
  else amp = (T)s.act_noise;
  return RollArgs<T, AN>{s.steps, s.learning, amp, (T)s.act_limit, s.seed, s.offset, (T*)p.y, (T*)p.state, (T*)p.action,
                         (T*)p.reward_sum, (T*)p.log_y, (T*)p.log_p, (T*)p.log_action, (T*)p.log_reward, p.done_any, p.done_step,
                         s.control_from};
}
// does this launch take the kernels of the amplitude array?  (a learning solo launch with an array set on the actor)
inline bool roll_noise_tab(const RollSpec& s, const RollMembers* pm) { return !pm && s.learning && s.noise_scale; }
// dynamic LDS of a rollout workgroup: the step kernel's (E.lds_bytes) + state, rewards, the actor image and its activation
// planes (KS: [2][rows] column pairs per thread; Keller-Segel: [2][A][RO_W]).  noise_tab: a learning launch with the amplitude
// array of pdec_mlp_set_noise_scale keeps each of its columns' amplitude behind the planes (KS: [2][A]; Keller-Segel: [A]); a
// configuration that this pushes over the 64 KB bound takes the step loop.
inline size_t rollout_lds(const Env& E, const Mlp& A, bool ks, bool noise_tab = false) {
  const pdec_env_cfg& c = E.cfg;
  const size_t image = (ro_image_elems(A.dims.data(), A.L) + 3) & ~3;
  const size_t planes = ks ? (size_t)4 * *std::max_element(A.dims.begin(), A.dims.begin() + A.L + 1) * E.nthreads : (size_t)2 * c.A * RO_W;
  const size_t tab = noise_tab ? (ks ? 2 : 1) * (size_t)c.A : 0;
  return E.lds_bytes + ((size_t)2 * c.A * env_ns(c) + (ks ? 4 : 2) * (size_t)c.A + image + planes + tab) * dtype_size(c.dtype) + 16;
}
// does the persistent rollout of the KS (ks) or the 1-D Keller-Segel environment serve E with an actor of A's shape?
// (everything but the parameters' dtype: the member form reads Float32 parameters into an fp64 image)
inline bool rollout_shape_ok(const Env& E, const Mlp& A, bool ks, bool noise_tab = false) {
  const pdec_env_cfg& c = E.cfg;
  const char* off = getenv("PDEC_ROLLOUT_PERSISTENT");
  if (off && off[0] == '0') return false;
  if (c.pde_kind != (ks ? PDEC_PDE_KS_CNAB2 : PDEC_PDE_KSEG_RK4) || c.mono || c.check_max_value == 2) return false;
  if (ks && (c.temporal_steps != 1 || (E.nthreads & 1))) return false;   // KS only: no temporal stack, a column pair per thread
  if (A.L < 1 || A.L > 3 || A.dims[A.L] != 1 || A.dims[0] != env_ns(c)) return false;
  for (int l = 0; l <= A.L; ++l)
    if (A.dims[l] > RO_W) return false;
  return rollout_lds(E, A, ks, noise_tab) <= 64 * 1024;
}
}  // namespace pdec
