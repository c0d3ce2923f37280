// fluid_sense.hip -- what the 2-D fluid environment does around its PDE step: sensing (featurize, reward_function,
// FluidSetup.jl:188-241), actuation (prepare_action, :243-261), the blow-up flag on the spectrum (src/PDEenv.jl:226-231), the
// episode initialisers ic(...) (src/fluid_rk4.jl:54-120) and error_detection (FluidSetup.jl:263-273), with the entry points that
// are nothing but these launches.  The n x n transforms they need are fluid_lds.hip's; fluid.hip has the design note.
#include "fluid.hpp"

namespace pdec {

// ------------------------------------------------------------------ sensing / actuation
// dots[b][s] = <y, gaussians[s]>: one wave per sensor over its BW x BH box   (FluidSetup.jl:196,216)
template <class T>
__global__ __launch_bounds__(256) void fluid_dots_kernel(int n, int S, int BH, int BW, const T* __restrict__ boxes,
                                                         const int* __restrict__ origin, const T* __restrict__ yreal,
                                                         T* __restrict__ dots) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + wv, b = blockIdx.y;
  if (s >= S) return;
  const int j0 = origin[2 * s], i0 = origin[2 * s + 1];
  const T* bx = boxes + (size_t)s * BH * BW;
  const T* y = yreal + (size_t)b * n * n;
  T acc = 0;
  for (int e = lane; e < BH * BW; e += 64) {
    const int dj = e / BH, di = e - dj * BH;
    int jj = j0 + dj, ii = i0 + di;
    if (jj >= n) jj -= n;
    if (ii >= n) ii -= n;
    acc += bx[e] * y[(size_t)jj * n + ii];
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) dots[(size_t)b * S + s] = acc;
}

template <class T>
struct FeatArgs {
  int S, A, spa, window, ns, check_max;
  int mem, na;      // action memory (cfg.memory_size): the last mem rows of a state column = rows 1.. of the action [A][na]
  T sensor_scale, r_in_scale, r_power, r_denom, a_pun, da_pun, max_value;
  const int* a2s;
};

// featurize (3x3 circular window of the spa x spa sensor grid, FluidSetup.jl:219-224) + reward (:188-202)
// term_out (pdec_env_set_terminal_out, the env step only): [B][A], 1 on every column of a trajectory whose flag of this step is
// set -- check_max 2: the flag reduced here in LDS, behind its barrier; 1: done[b] as fluid_maxabs_kernel left it; 0: zeros.
// Written on the reward path: the env step always has a reward_out (pdec_env_step refuses a null one).
template <class T>
__global__ __launch_bounds__(256) void fluid_feat_kernel(FeatArgs<T> g, const T* __restrict__ dots,
                                                         const T* __restrict__ action, const T* __restrict__ action_prev,
                                                         const T* __restrict__ state_prev, T* __restrict__ state_out,
                                                         T* __restrict__ reward_out, int32_t* __restrict__ done,
                                                         T* __restrict__ term_out) {
  __shared__ int flag;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const T* dt = dots + (size_t)b * g.S;
  if (tid == 0) flag = 0;
  __syncthreads();
  if (state_out) {
    const int w = g.window / 2, fresh = g.window * g.window;
    const T* prev = state_prev ? state_prev + (size_t)b * g.A * g.ns : nullptr;
    for (int idx = tid; idx < g.A * g.ns; idx += nt) {
      const int a = idx / g.ns, rr = idx - a * g.ns;
      T v;
      if (rr >= g.ns - g.mem) {          // FluidSetup.jl:236-241: env.action[end-(memory_size-1):end, :], zeros without env
        v = action ? action[((size_t)b * g.A + a) * g.na + 1 + (rr - (g.ns - g.mem))] : (T)0;
      } else if (rr < fresh || prev == nullptr) {
        const int r0 = rr % fresh, wi = r0 / g.window - w, wj = r0 % g.window - w;
        const int e = g.a2s[a];
        int row = (e / g.spa - wi) % g.spa, col = (e % g.spa - wj) % g.spa;
        if (row < 0) row += g.spa;
        if (col < 0) col += g.spa;
        v = dt[row * g.spa + col] * g.sensor_scale;
      } else {
        v = prev[a * g.ns + (rr - fresh)];
      }
      state_out[(size_t)b * g.A * g.ns + idx] = v;
    }
  }
  if (reward_out) {
    for (int a = tid; a < g.A; a += nt) {
      const T dd = fabs(g.r_in_scale * dt[g.a2s[a]]);
      const T pw = dd == 0 ? (T)0 : (T)pow((double)dd, (double)g.r_power);
      const T ac = action[((size_t)b * g.A + a) * g.na], da = ac - action_prev[((size_t)b * g.A + a) * g.na];   // row 1 (:200)
      const T r = -fabs(pw / g.r_denom) - g.a_pun * ac * ac - g.da_pun * da * da;
      reward_out[(size_t)b * g.A + a] = r;
      if (g.check_max == 2 && !(fabs(r) <= g.max_value)) atomicOr(&flag, 1);
    }
    __syncthreads();
    if (done && tid == 0 && g.check_max == 2) done[b] = flag;
    if (term_out) {
      const int f = g.check_max == 2 ? flag : (g.check_max == 1 ? done[b] : 0);
      const T tv = f ? (T)1 : (T)0;
      for (int a = tid; a < g.A; a += nt) term_out[(size_t)b * g.A + a] = tv;
    }
  }
}

// max|y| > max_value on the spectrum (check_max_value == "y", src/PDEenv.jl:226-231)
template <class T>
__global__ __launch_bounds__(256) void fluid_maxabs_kernel(int nn, T max_value, const C2<T>* __restrict__ y,
                                                           int32_t* __restrict__ done) {
  __shared__ int flag;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) flag = 0;
  __syncthreads();
  int f = 0;
  for (int i = threadIdx.x; i < nn; i += blockDim.x) {
    const C2<T> v = y[(size_t)b * nn + i];
    if (!(hypot(v.x, v.y) <= max_value)) f = 1;
  }
  if (f) atomicOr(&flag, 1);
  __syncthreads();
  if (threadIdx.x == 0) done[b] = flag;
}

// p = sum_a agent_power * action[a] * gaussians_actuators[a]   (FluidSetup.jl:254-258): one 16x16 block of
// cells per workgroup, candidates = the actuators whose box meets the block (CSR built at setup time)
template <class T>
__global__ __launch_bounds__(256) void fluid_actuate_kernel(int n, int A, int BH, int BW, int nb1,
                                                            const T* __restrict__ boxes, const int* __restrict__ origin,
                                                            const int* __restrict__ blk_ptr, const int* __restrict__ blk_idx,
                                                            const T* __restrict__ action, int na, T power, T* __restrict__ preal) {
  const int blk = blockIdx.x, b = blockIdx.y;
  const int bj = blk / nb1, bi = blk - bj * nb1;
  const int di = threadIdx.x & 15, dj = threadIdx.x >> 4;
  const int j = bj * 16 + dj, i = bi * 16 + di;
  if (j >= n || i >= n) return;
  T acc = 0;
  for (int q = blk_ptr[blk]; q < blk_ptr[blk + 1]; ++q) {
    const int a = blk_idx[q];
    int dj2 = j - origin[2 * a], di2 = i - origin[2 * a + 1];
    if (dj2 < 0) dj2 += n;
    if (di2 < 0) di2 += n;
    if (dj2 < BW && di2 < BH) acc += (power * action[((size_t)b * A + a) * na]) * boxes[((size_t)a * BW + dj2) * BH + di2];
  }
  preal[((size_t)b * n + j) * n + i] = acc;
}

// ------------------------------------------------------------------ initialisers and the error check
// Episode initialiser on the device: omega = sum over vortices of the 9 periodic images of a
// Taylor vortex U/a (2 - r^2/a^2) exp((1 - r^2/a^2)/2)   (src/fluid_rk4.jl:54-69, ic(...) :72-120).  One thread per
// cell, same summation order as the reference (vortex outer, image offsets i, j inner); vort [B][nv][4] = x0, y0, a, U.
template <class T>
__global__ void fluid_ic_kernel(int n, int nv, T Lx, T Ly, const T* __restrict__ vort, T* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char ic_smem[];
  T* sv = reinterpret_cast<T*>(ic_smem);
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < 4 * nv; i += blockDim.x) sv[i] = vort[(size_t)b * 4 * nv + i];
  __syncthreads();
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * n) return;
  const int jx = idx / n, iy = idx - jx * n;            // memory [nx][ny]: y is the fast axis
  const T x = (T)jx * (Lx / (T)n), y = (T)iy * (Ly / (T)n);
  T total = 0;
  for (int v = 0; v < nv; ++v) {
    const T x0 = sv[4 * v], y0 = sv[4 * v + 1], a0 = sv[4 * v + 2], U = sv[4 * v + 3];
    T omg = 0;
    for (int i = -1; i <= 1; ++i)
      for (int j = -1; j <= 1; ++j) {
        const T ddx = x - x0 - (T)i * Lx, ddy = y - y0 - (T)j * Ly;
        const T r2 = ddx * ddx + ddy * ddy;
        omg = omg + U / a0 * ((T)2 - r2 / (a0 * a0)) * exp((T)0.5 * ((T)1 - r2 / (a0 * a0)));
      }
    total = total + omg;
  }
  out[(size_t)b * n * n + idx] = total;
}

// the vortex table of an fp32 environment from the caller's doubles, on the device (pdec_fluid_ic_dev)
__global__ void fluid_round_kernel(const double* __restrict__ in, float* __restrict__ out, size_t cnt) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) out[i] = (float)in[i];
}

// The random draws of ic(3) / ic(4) (src/fluid_rk4.jl:72-120) from the library's Philox stream (seed, offset): one thread per
// (trajectory b, vortex v) = counter offset + b nv + v, its words w0..w3, u_i = (w_i + 0.5) 2^-32 (random_init_kernel's
// convention); row (x0, y0, a0, U) = (u0 Lx, u1 Ly, a0, 2 u3 - 1), a0 = a_base (case 3) or a_base (0.5 + u2) (case 4).
// tab: the environment's table [B][nv][4]; copy: the caller's, or null.
__global__ void fluid_vortex_draw_kernel(int total, int vary_a, double Lx, double Ly, double a_base, uint64_t seed, uint64_t offset,
                                         double* __restrict__ tab, double* __restrict__ copy) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint64_t ctr = offset + (uint64_t)i;
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  double u[4];
  for (int q = 0; q < 4; ++q) u[q] = ((double)c[q] + 0.5) * (1.0 / 4294967296.0);
  const double row[4] = {u[0] * Lx, u[1] * Ly, vary_a ? a_base * (0.5 + u[2]) : a_base, 2.0 * u[3] - 1.0};
  for (int q = 0; q < 4; ++q) {
    tab[(size_t)4 * i + q] = row[q];
    if (copy) copy[(size_t)4 * i + q] = row[q];
  }
}

// error_detection (scripts/Fluid/setup/FluidSetup.jl:263-273) on w = real(ifft2(y)) [B][n][n]: the largest |w[r][i] - w[r-1][i]|
// and |w[r][i] - w[r][i-1]|, periodic along both axes.  grid (ceil(n / FL_JUMP_ROWS), B): a workgroup walks its rows downwards,
// a thread keeps the row above in a register (one halo row per tile) and takes its left neighbour from the lane beside it
// (lane 0: one more load), so every row is read once, coalesced along the fast axis.  The maximum PROPAGATES NaN, as the host's
// torch max does; wave: shuffles, workgroup: LDS; then ONE integer OR per workgroup into bits[b]: 1 = above 10, 2 = NaN.
#define FL_JUMP_ROWS 16
#define FL_JUMP_NTH 256
template <class T>
__device__ __forceinline__ T nanmax(T a, T b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

template <class T>
__global__ __launch_bounds__(FL_JUMP_NTH) void fluid_jump_kernel(int n, const T* __restrict__ w, int32_t* __restrict__ bits) {
  __shared__ T part[FL_JUMP_NTH / 64];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
  const int r0 = blockIdx.x * FL_JUMP_ROWS, r1 = min(r0 + FL_JUMP_ROWS, n);
  const T* wb = w + (size_t)b * n * n;
  T m = 0;
  for (int i0 = 0; i0 < n; i0 += FL_JUMP_NTH) {        // (uniform trip count: the shuffle below is executed by whole waves)
    const int i = i0 + tid;
    const bool live = i < n;
    const int il = i == 0 ? n - 1 : i - 1;
    T up = live ? wb[(size_t)(r0 == 0 ? n - 1 : r0 - 1) * n + i] : (T)0;
    for (int r = r0; r < r1; ++r) {
      const T cur = live ? wb[(size_t)r * n + i] : (T)0;
      T left = __shfl_up(cur, 1);
      if (live && lane == 0) left = wb[(size_t)r * n + il];
      if (live) m = nanmax(m, nanmax(fabs(cur - up), fabs(cur - left)));
      up = cur;
    }
  }
  for (int off = 32; off > 0; off >>= 1) m = nanmax(m, __shfl_xor(m, off));
  if (lane == 0) part[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < FL_JUMP_NTH / 64; ++k) m = nanmax(m, part[k]);
    const int v = m != m ? 2 : (m > (T)10 ? 1 : 0);
    if (v) atomicOr(&bits[b], v);
  }
}

// errored[b] = the NaN-propagating maximum is above 10: some workgroup saw a jump and none saw a NaN
__global__ void fluid_jump_finish_kernel(int B, const int32_t* __restrict__ bits, int32_t* __restrict__ errored) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) errored[b] = bits[b] == 1 ? 1 : 0;
}

// ------------------------------------------------------------------ host side
int fluid_dots(FluidEnv& E, const void* y) {
  int rc = fluid_to_physical(E, y);
  if (rc) return rc;
  return fluid_by_dtype(E, [&](auto t) -> int {
    typedef decltype(t) T;
    const pdec_env_cfg& c = E.cfg;
    ProfScope ps(&E, "fluid_dots");
    hipLaunchKernelGGL(fluid_dots_kernel<T>, dim3((c.S + 3) / 4, c.B), dim3(256), 0, E.stream, E.n, c.S, E.BH, E.BW,
                       E.sbox.as<T>(), E.sorg.as<int>(), E.yreal.as<T>(), E.dots.as<T>());
    PDEC_HIP(hipGetLastError());
    return PDEC_OK;
  });
}

template <class T>
static FeatArgs<T> feat_args(const FluidEnv& E) {
  const pdec_env_cfg& c = E.cfg;
  FeatArgs<T> g;
  g.S = c.S; g.A = c.A; g.spa = c.sensors_per_axis; g.window = c.window;
  g.ns = env_ns(c); g.check_max = c.check_max_value;
  g.mem = c.memory_size; g.na = env_na(c);
  g.sensor_scale = (T)c.sensor_scale; g.r_in_scale = (T)c.reward_in_scale; g.r_power = (T)c.reward_power;
  g.r_denom = (T)c.reward_denom; g.a_pun = (T)c.action_punish; g.da_pun = (T)c.delta_action_punish; g.max_value = (T)c.max_value;
  g.a2s = E.a2s_d.as<int>();
  return g;
}

int fluid_feat_launch(FluidEnv& E, const void* action, const void* action_prev, const void* state_prev, void* state_out,
                      void* reward_out, int32_t* done, void* term_out) {
  return fluid_by_dtype(E, [&](auto t) -> int {
    typedef decltype(t) T;
    ProfScope ps(&E, "fluid_feat");
    hipLaunchKernelGGL(fluid_feat_kernel<T>, dim3(E.cfg.B), dim3(256), 0, E.stream, feat_args<T>(E), E.dots.as<T>(),
                       (const T*)action, (const T*)action_prev, (const T*)state_prev, (T*)state_out,
                       (T*)reward_out, done, (T*)term_out);
    PDEC_HIP(hipGetLastError());
    return PDEC_OK;
  });
}

int fluid_actuate(FluidEnv& E, const void* action, void* p_out) {
  return fluid_by_dtype(E, [&](auto t) -> int {
    typedef decltype(t) T;
    const pdec_env_cfg& c = E.cfg;
    ProfScope ps(&E, "fluid_actuate");
    hipLaunchKernelGGL(fluid_actuate_kernel<T>, dim3(E.nb1 * E.nb1, c.B), dim3(256), 0, E.stream, E.n, c.A, E.BH, E.BW,
                       E.nb1, E.abox.as<T>(), E.aorg.as<int>(), E.blkptr.as<int>(), E.blkidx.as<int>(),
                       (const T*)action, env_na(c), (T)c.agent_power, E.yreal.as<T>());
    (void)fluid_fft2_of_real(E, E.yreal.p, p_out);
    PDEC_HIP(hipGetLastError());
    return PDEC_OK;
  });
}

int fluid_done_y(FluidEnv& E, const void* y, int32_t* done) {
  return fluid_by_dtype(E, [&](auto t) -> int {
    typedef decltype(t) T;
    hipLaunchKernelGGL(fluid_maxabs_kernel<T>, dim3(E.cfg.B), dim3(256), 0, E.stream, E.n * E.n, (T)E.cfg.max_value,
                       (const C2<T>*)y, done);
    PDEC_HIP(hipGetLastError());
    return PDEC_OK;
  });
}

FluidEnv* fluid_handle(pdec_handle h, const char* who) {
  Env* E0 = lookup_as<Env>(h, Kind::Env);
  if (!E0 || E0->cfg.pde_kind != PDEC_PDE_FLUID_RK4) { set_error("%s: not a fluid env handle", who); return nullptr; }
  return static_cast<FluidEnv*>(E0);
}

}  // namespace pdec

using namespace pdec;

// the initialiser and the forward 2-D FFT on the environment's stream; vort: DEVICE [B][nv][4] in the environment's dtype
template <class T>
static int fluid_ic_launch(FluidEnv& E, const T* vort, int nv, void* y_out) {
  const pdec_env_cfg& c = E.cfg;
  ProfScope ps(&E, "fluid_ic");
  hipLaunchKernelGGL(fluid_ic_kernel<T>, dim3((E.n * E.n + 255) / 256, c.B), dim3(256), (size_t)nv * 4 * sizeof(T), E.stream,
                     E.n, nv, (T)c.Lx, (T)c.Lx, vort, E.yreal.as<T>());
  (void)fluid_fft2_of_real(E, E.yreal.p, y_out);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

// the vortex table in the environment's dtype (fp32: rounded once from the caller's doubles), the initialiser, the 2-D FFT
template <class T>
static int fluid_ic_t(FluidEnv& E, const double* vortices, int nv, void* y_out) {
  const size_t cnt = (size_t)E.cfg.B * nv * 4, vb = cnt * sizeof(T);
  std::vector<T> vt;
  const void* src = vortices;
  if (!std::is_same<T, double>::value) {
    vt.assign(vortices, vortices + cnt);
    src = vt.data();
  }
  if (E.icv.bytes < vb) PDEC_HIP(E.icv.alloc(vb));
  PDEC_HIP(hipMemcpyAsync(E.icv.p, src, vb, hipMemcpyHostToDevice, E.stream));
  int rc = fluid_ic_launch<T>(E, E.icv.as<T>(), nv, y_out);
  if (rc) return rc;
  PDEC_HIP(hipStreamSynchronize(E.stream));      // the host array (and vt) may be reused / freed once this returns
  return PDEC_OK;
}

// ic(caseno): spectrum of the sum of Taylor vortices (src/fluid_rk4.jl:72-120 with the random draws made by the
// caller).  vortices: HOST array [B][nv][4] of (x0, y0, a0, U_max); y_out: device [B][nx][ny][2].
extern "C" int pdec_fluid_ic(pdec_handle h, const double* vortices, int nv, void* y_out) {
  FluidEnv* Ep = fluid_handle(h, "pdec_fluid_ic");
  if (!Ep) return PDEC_E_HANDLE;
  PDEC_REQUIRE(vortices && y_out && nv >= 1 && nv <= 1024, "pdec_fluid_ic: bad arguments (1 <= nv <= 1024)");
  return fluid_by_dtype(*Ep, [&](auto t) -> int { return fluid_ic_t<decltype(t)>(*Ep, vortices, nv, y_out); });
}

// pdec_fluid_ic with the table already in device memory (doubles): the same launches, no host copy, no synchronisation.
// An fp32 environment rounds the table once, on the device, into its own icv (the rounding of the host path's cast).
static int fluid_ic_from_dev(FluidEnv& E, const double* vortices_dev, int nv, void* y_out) {
  if (E.cfg.dtype != PDEC_F32) return fluid_ic_launch<double>(E, vortices_dev, nv, y_out);
  const size_t cnt = (size_t)E.cfg.B * nv * 4;
  if (E.icv.bytes < cnt * sizeof(float)) PDEC_HIP(E.icv.alloc(cnt * sizeof(float)));
  hipLaunchKernelGGL(fluid_round_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, E.stream, vortices_dev, E.icv.as<float>(),
                     cnt);
  return fluid_ic_launch<float>(E, E.icv.as<float>(), nv, y_out);
}

extern "C" int pdec_fluid_ic_dev(pdec_handle h, const double* vortices_dev, int nv, void* y_out) {
  FluidEnv* Ep = fluid_handle(h, "pdec_fluid_ic_dev");
  if (!Ep) return PDEC_E_HANDLE;
  PDEC_REQUIRE(vortices_dev && y_out && nv >= 1 && nv <= 1024, "pdec_fluid_ic_dev: bad arguments (1 <= nv <= 1024)");
  return fluid_ic_from_dev(*Ep, vortices_dev, nv, y_out);
}

// ic(3) / ic(4) with the draws made on the device: fluid_vortex_draw_kernel into the environment's own table (allocated with the
// environment), then the launches of pdec_fluid_ic_dev on it; see include/pdeconv.h
extern "C" int pdec_fluid_ic_rng(pdec_handle h, uint64_t seed, uint64_t offset, int caseno, double* vortices_out, void* y_out) {
  FluidEnv* Ep = fluid_handle(h, "pdec_fluid_ic_rng");
  if (!Ep) return PDEC_E_HANDLE;
  PDEC_REQUIRE(caseno == 3 || caseno == 4, "pdec_fluid_ic_rng: caseno %d (3: 30 vortices, training; 4: 50, evaluation)", caseno);
  PDEC_REQUIRE(y_out, "pdec_fluid_ic_rng: null y_out");
  FluidEnv& E = *Ep;
  const int nv = caseno == 3 ? 30 : 50, total = E.cfg.B * nv;
  PDEC_REQUIRE(E.icd.bytes >= (size_t)total * 4 * sizeof(double), "pdec_fluid_ic_rng: internal: table too small");
  {
    ProfScope ps(&E, "fluid_vortex_draw");
    hipLaunchKernelGGL(fluid_vortex_draw_kernel, dim3((total + 255) / 256), dim3(256), 0, E.stream, total, caseno == 4 ? 1 : 0,
                       E.cfg.Lx, E.cfg.Lx, E.cfg.Lx / 20, seed, offset, E.icd.as<double>(), vortices_out);
    PDEC_HIP(hipGetLastError());
  }
  return fluid_ic_from_dev(E, E.icd.as<double>(), nv, y_out);
}

template <class T>
static int fluid_error_detection_t(FluidEnv& E, const void* y, int32_t* errored_out) {
  const int B = E.cfg.B;
  int rc = fluid_to_physical(E, y);
  if (rc) return rc;
  ProfScope ps(&E, "fluid_error_detection");
  PDEC_HIP(hipMemsetAsync(E.errbits.p, 0, sizeof(int32_t) * B, E.stream));
  hipLaunchKernelGGL(fluid_jump_kernel<T>, dim3((E.n + FL_JUMP_ROWS - 1) / FL_JUMP_ROWS, B), dim3(FL_JUMP_NTH), 0, E.stream, E.n,
                     E.yreal.as<T>(), E.errbits.as<int32_t>());
  hipLaunchKernelGGL(fluid_jump_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, E.stream, B, E.errbits.as<int32_t>(), errored_out);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

// error_detection of the fluid script (scripts/Fluid/setup/FluidSetup.jl:263-273) per trajectory; see include/pdeconv.h
extern "C" int pdec_fluid_error_detection(pdec_handle h, const void* y, int32_t* errored_out) {
  FluidEnv* Ep = fluid_handle(h, "pdec_fluid_error_detection");
  if (!Ep) return PDEC_E_HANDLE;
  PDEC_REQUIRE(y && errored_out, "pdec_fluid_error_detection: null argument");
  // (a batch stepped in parts: the parent environment has work arrays of the whole batch of its own, fluid_make)
  return fluid_by_dtype(*Ep, [&](auto t) -> int { return fluid_error_detection_t<decltype(t)>(*Ep, y, errored_out); });
}
