// act_members.hip -- agent(env) of M actors on ONE state matrix in one launch (pdec_policy_act_members).
//
// The 2-D environments have no persistent rollout: their control step is a launch sequence, and a greedy evaluation of M
// actors on K held-out fields each (population.py: evaluate_actors) used to be M such sequences at B = K.  With this kernel
// it is ONE sequence at B = M K: member m's block of C = K A state columns is driven by member m's actor, taken from the
// pointer table the environment owns (Env::roll_tab), and the env step that follows serves all M K trajectories at once.
//
// Arithmetic: small_act_body's (act.hip), which is gemm_kernel's -- per output element acc = 0, acc += (T)W[j][k] x[k] in
// ascending k, + (T)b[j], apply_act<T>, and after the last layer the clamp to +-act_limit -- so a member's actions are bit for
// bit those of pdec_policy_act_rng (greedy) on its block alone through either of those two routes.  Greedy only: the
// exploration noise of the solo call is numbered by global column, a member's stream is not defined.
#include "env.hpp"
#include "mlp.hpp"

namespace pdec {

struct ActMembersArgs {
  int L, cols, tc;                 // layers, columns per member, columns per tile (the LDS row stride)
  int dims[SMALL_ACT_MAXL + 1], acts[SMALL_ACT_MAXL], woff[SMALL_ACT_MAXL], boff[SMALL_ACT_MAXL];
  const void* const* tab;          // [M] the members' flat parameters (W_l row-major [out][in], then b_l)
  double lim;
};

// grid (tiles of one member, M), 256 threads: workgroup (tile, m) serves columns tile tc .. of member m's block -- nc <= tc of
// them, so the last tile of a member neither reads nor writes a neighbour's columns.  Activations [feature][column] in LDS,
// two buffers of maxw tc elements; consecutive lanes take consecutive columns (conflict-free LDS reads and writes).
template <class T, class TP>
__global__ __launch_bounds__(256) void act_members_kernel(ActMembersArgs g, const T* __restrict__ state, T* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char act_members_smem[];
  const int tid = threadIdx.x, tc = g.tc, m = blockIdx.y;
  const int c0 = blockIdx.x * tc;
  const int nc = min(tc, g.cols - c0);
  if (nc <= 0) return;
  int maxw = g.dims[0];
  for (int l = 1; l <= g.L; ++l) maxw = max(maxw, g.dims[l]);
  T* xin = reinterpret_cast<T*>(act_members_smem);
  T* xout = xin + (size_t)maxw * tc;
  const TP* p = static_cast<const TP*>(g.tab[m]);
  const size_t col0 = (size_t)m * g.cols + c0;       // first global column of the tile
  const int ns = g.dims[0];
  const T* s = state + col0 * ns;
  for (int i = tid; i < ns * nc; i += 256) {
    const int c = i / ns, k = i - c * ns;
    xin[k * tc + c] = s[i];
  }
  __syncthreads();
  for (int l = 0; l < g.L; ++l) {
    const int in = g.dims[l], on = g.dims[l + 1];
    const TP* W = p + g.woff[l];
    const TP* b = p + g.boff[l];
    for (int i = tid; i < on * nc; i += 256) {
      const int j = i / nc, c = i - j * nc;
      T acc = 0;
      for (int k = 0; k < in; ++k) acc += (T)W[j * in + k] * xin[k * tc + c];
      xout[j * tc + c] = apply_act<T>(acc + (T)b[j], g.acts[l]);
    }
    __syncthreads();
    T* t = xin; xin = xout; xout = t;
  }
  const int no = g.dims[g.L];
  const T lim = (T)g.lim;
  T* o = out + col0 * no;
  for (int i = tid; i < no * nc; i += 256) {         // i = column * outputs + row, as the solo kernels store
    const int c = i / no, f = i - c * no;
    T v = xin[f * tc + c];
    v = v < -lim ? -lim : (v > lim ? lim : v);
    o[i] = v;
  }
}

// tile_cols = the largest multiple of 64 whose two buffers fit SMALL_ACT_LDS, capped at cols_per_member rounded up to 64
// (population.py restates it: act_members_tiles)
ActMembersPlan act_members_plan(const Mlp& A, int state_dtype, int cols_per_member) {
  ActMembersPlan pl;
  const size_t per_col = (size_t)2 * mlp_maxw(&A) * dtype_size(state_dtype);
  int tc = (int)(SMALL_ACT_LDS / per_col) / 64 * 64;
  if (tc < 64 || cols_per_member < 1) return pl;
  tc = std::min(tc, (cols_per_member + 63) / 64 * 64);
  pl.tile_cols = tc;
  pl.tiles = (cols_per_member + tc - 1) / tc;
  pl.lds = per_col * tc;
  return pl;
}

bool act_members_served(int state_dtype, const std::vector<const Mlp*>& actors, int cols_per_member) {
  const Mlp& A = *actors[0];
  for (size_t m = 1; m < actors.size(); ++m)
    if (actors[m]->dims != A.dims || actors[m]->acts != A.acts || actors[m]->dtype != A.dtype) return false;
  if (A.dtype != PDEC_F32 && A.dtype != state_dtype) return false;
  if (A.L < 1 || A.L > SMALL_ACT_MAXL || actors.size() > 65535) return false;
  if (act_members_plan(A, state_dtype, cols_per_member).tile_cols == 0) return false;
  // the solo call acts through an actor of the states' dtype: an fp64 one never takes a fused MFMA route, an fp32 one is A itself
  if (state_dtype == PDEC_F32 && act_route_is_fused(&A, cols_per_member)) return false;
  return true;
}

int act_members_launch(Env& E, const std::vector<const Mlp*>& actors, const void* state, int cols_per_member, double act_limit,
                       void* actions_out) {
  const Mlp& A = *actors[0];
  const int dt = E.cfg.dtype;
  if (!act_members_served(dt, actors, cols_per_member)) { set_error("act_members_launch: configuration not covered"); return PDEC_E_INVALID; }
  const int rc = roll_tab_upload(E, actors);
  if (rc) return rc;
  const ActMembersPlan pl = act_members_plan(A, dt, cols_per_member);
  ActMembersArgs g{};
  g.L = A.L; g.cols = cols_per_member; g.tc = pl.tile_cols;
  for (int l = 0; l <= A.L; ++l) g.dims[l] = A.dims[l];
  for (int l = 0; l < A.L; ++l) { g.acts[l] = A.acts[l]; g.woff[l] = (int)A.w_off[l]; g.boff[l] = (int)A.b_off[l]; }
  g.tab = E.roll_tab.as<const void*>();
  g.lim = act_limit;
  const dim3 grid(pl.tiles, (unsigned)actors.size()), block(256);
  ProfScope ps(&E, "act_members");
  if (dt == PDEC_F64 && A.dtype == PDEC_F32)
    hipLaunchKernelGGL((act_members_kernel<double, float>), grid, block, pl.lds, E.stream, g, (const double*)state, (double*)actions_out);
  else if (dt == PDEC_F64)
    hipLaunchKernelGGL((act_members_kernel<double, double>), grid, block, pl.lds, E.stream, g, (const double*)state, (double*)actions_out);
  else
    hipLaunchKernelGGL((act_members_kernel<float, float>), grid, block, pl.lds, E.stream, g, (const float*)state, (float*)actions_out);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

}  // namespace pdec

using namespace pdec;

extern "C" int pdec_policy_act_members(pdec_handle henv, const pdec_handle* actors, int M, const void* state, int cols_per_member,
                                       double act_limit, void* actions_out, int* served) {
  Env* E = lookup_as<Env>(henv, Kind::Env);
  if (!E) { set_error("pdec_policy_act_members: bad handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(served, "pdec_policy_act_members: served is null");
  *served = 0;
  PDEC_REQUIRE(actors && M >= 1 && cols_per_member >= 1 && state && actions_out, "pdec_policy_act_members: null/empty argument");
  std::vector<const Mlp*> nets(M);
  for (int m = 0; m < M; ++m) {
    nets[m] = lookup_as<Mlp>(actors[m], Kind::Mlp);
    if (!nets[m]) { set_error("pdec_policy_act_members: bad actor handle (member %d)", m); return PDEC_E_HANDLE; }
    PDEC_REFUSE_NOISE_COLOR(nets[m], "pdec_policy_act_members", "the member forms do not serve it");
  }
  if (!act_members_served(E->cfg.dtype, nets, cols_per_member)) return PDEC_OK;
  const int rc = act_members_launch(*E, nets, state, cols_per_member, act_limit, actions_out);
  if (rc == PDEC_OK) *served = 1;
  return rc;
}

extern "C" int pdec_debug_act_members_plan(pdec_handle actor, int state_dtype, int cols_per_member, int* tile_cols, int* tiles,
                                           int64_t* lds_bytes) {
  const Mlp* A = lookup_as<Mlp>(actor, Kind::Mlp);
  if (!A) { set_error("pdec_debug_act_members_plan: not an mlp handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(tile_cols && tiles && lds_bytes && (state_dtype == PDEC_F32 || state_dtype == PDEC_F64),
               "pdec_debug_act_members_plan: null argument or bad dtype");
  const ActMembersPlan pl = act_members_plan(*A, state_dtype, cols_per_member);
  *tile_cols = pl.tile_cols; *tiles = pl.tiles; *lds_bytes = (int64_t)pl.lds;
  return PDEC_OK;
}
