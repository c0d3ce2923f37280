// mlp.hip -- weight-shared ("convolutional") actor/critic MLPs on gfx950: forward,
// backward, Flux-ADAM, Polyak, policy act and the DDPG update.
//
// Restates (from scratch):
//   create_NNA / Chain(Dense...)            src/PDEagent.jl:14-56
//   CustomNeuralNetworkApproximator         src/custom_nna.jl:7-27
//   (policy::CustomDDPGPolicy)(env)         src/PDEagent.jl:175-209
//   RLBase.update!(policy, batch)           src/PDEagent.jl:363-418
//
// A Dense layer applied to the im2col state matrix [features, columns] is a 1-D/2-D
// convolution with circular padding expressed as a GEMM over columns.  Activations are
// kept feature-major H[f][col] (columns contiguous -> coalesced, one column per lane).
// This file holds the GENERIC path (any widths, fp32 and fp64): LDS-tiled VALU GEMMs with
// fused bias/activation and activation-derivative epilogues, split-K weight gradients with
// a deterministic slab reduction (so data-parallel replicas stay bit-identical), ADAM,
// Polyak, the counter-based normals and the generic acting sequence, with the Mlp methods and
// the pdec_mlp_* / pdec_adam_* / pdec_polyak / pdec_policy_act / pdec_randn entry points.
// The DDPG passes and their routing live in ddpg.hip, acting for few columns and the step glue
// in act.hip, the fp32 MFMA families in mlp_mfma.hip (+ fused3_*.hpp) / mlp_mfma2.hip (+ fused2_*.hpp).
#include "common.hpp"
#include "mlp.hpp"

namespace pdec {

// ------------------------------------------------------------------ tiled GEMM
#define GB_M 64
#define GB_N 64
#define GB_K 16

enum { EPI_STORE = 0, EPI_BIAS_ACT = 1, EPI_MUL_DACT = 2 };

template <class T>
struct GemmArgs {
  int M, N, K, kchunk;
  const T* A; long sam, sak;
  const T* B; long sbk, sbn;
  T* C; long scm, scn, scz;       // scz: slab stride for split-K (blockIdx.z)
  int epi, act;
  const T* bias;                  // EPI_BIAS_ACT: bias[m]
  const T* aux; long sauxm, sauxn;  // EPI_MUL_DACT: activation values at (m,n)
};

// (apply_act<T>: mlp.hpp -- csrc/act_members.hip applies the same activations)
// derivative expressed through the activation VALUE a = act(z)
template <class T>
__device__ __forceinline__ T dact_from_value(T a, int act) {
  if (act == PDEC_ACT_RELU) return a > 0 ? (T)1 : (T)0;
  if (act == PDEC_ACT_TANH) return (T)1 - a * a;
  return (T)1;
}

template <class T>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs<T> g) {
  __shared__ T As[GB_K][GB_M + 1];
  __shared__ T Bs[GB_K][GB_N + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * GB_M, n0 = blockIdx.x * GB_N;
  const int kbeg = blockIdx.z * g.kchunk;
  int kend = kbeg + g.kchunk;
  if (kend > g.K) kend = g.K;
  T acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0;
  for (int k0 = kbeg; k0 < kend; k0 += GB_K) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256;
      int m, k;
      if (g.sak == 1) { k = idx & 15; m = idx >> 4; } else { m = idx & 63; k = idx >> 6; }
      const int gm = m0 + m, gk = k0 + k;
      As[k][m] = (gm < g.M && gk < kend) ? g.A[gm * g.sam + gk * g.sak] : (T)0;
      int n, kb;
      if (g.sbn == 1) { n = idx & 63; kb = idx >> 6; } else { kb = idx & 15; n = idx >> 4; }
      const int gn = n0 + n, gkb = k0 + kb;
      Bs[kb][n] = (gn < g.N && gkb < kend) ? g.B[gkb * g.sbk + gn * g.sbn] : (T)0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < GB_K; ++k) {
      T a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[k][ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Bs[k][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
    }
    __syncthreads();
  }
  T* C = g.C + (size_t)blockIdx.z * g.scz;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 16 * i;
    if (m >= g.M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx + 16 * j;
      if (n >= g.N) continue;
      T v = acc[i][j];
      if (g.epi == EPI_BIAS_ACT) v = apply_act<T>(v + g.bias[m], g.act);
      else if (g.epi == EPI_MUL_DACT) v *= dact_from_value<T>(g.aux[m * g.sauxm + n * g.sauxn], g.act);
      C[m * g.scm + n * g.scn] = v;
    }
  }
}

// grad[i] = scale * sum_z slab[z][i]
template <class T>
__global__ void reduce_slabs_kernel(const T* __restrict__ slabs, T* __restrict__ grad, int n, int nz, size_t zstride,
                                    T scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T acc = 0;
  for (int z = 0; z < nz; ++z) acc += slabs[(size_t)z * zstride + i];
  grad[i] = acc * scale;
}

// db[m] = scale * sum_c dz[m][c]   (one block per row)
template <class T>
__global__ void rowsum_kernel(const T* __restrict__ dz, T* __restrict__ db, int cols, T scale) {
  __shared__ T red[256];
  const int m = blockIdx.x, tid = threadIdx.x;
  T acc = 0;
  for (int c = tid; c < cols; c += 256) acc += dz[(size_t)m * cols + c];
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) db[m] = red[0] * scale;
}

// X0[f][c] from up to two sources; layout flag 0: [cols][n] (Julia [n,cols]), 1: feature-major [n][cols]
template <class T>
__global__ void pack_kernel(T* __restrict__ X0, int cols, const T* __restrict__ s1, int n1, int l1,
                            const T* __restrict__ s2, int n2, int l2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  for (int f = 0; f < n1; ++f) X0[(size_t)f * cols + c] = l1 ? s1[(size_t)f * cols + c] : s1[(size_t)c * n1 + f];
  for (int f = 0; f < n2; ++f)
    X0[(size_t)(n1 + f) * cols + c] = l2 ? s2[(size_t)f * cols + c] : s2[(size_t)c * n2 + f];
}

// out[c][f] = H[f][c]
template <class T>
__global__ void unpack_kernel(const T* __restrict__ H, int cols, int n, T* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  for (int f = 0; f < n; ++f) out[(size_t)c * n + f] = H[(size_t)f * cols + c];
}

// dz[f][c] = dy(f,c) * act'(a[f][c]); dy layout flag as in pack
template <class T>
__global__ void dz_init_kernel(T* __restrict__ dz, const T* __restrict__ dy, int ldy, const T* __restrict__ a,
                               int n, int cols, int act) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  for (int f = 0; f < n; ++f) {
    const T d = ldy ? dy[(size_t)f * cols + c] : dy[(size_t)c * n + f];
    dz[(size_t)f * cols + c] = d * dact_from_value<T>(a[(size_t)f * cols + c], act);
  }
}

// Flux.Optimise.ADAM apply! + update!: arithmetic in Float64 (beta, eps, eta are Float64 in
// Flux, so the broadcast promotes), stored back in T.
template <class T>
__global__ void adam_kernel(T* __restrict__ p, const T* __restrict__ g, T* __restrict__ m, T* __restrict__ v, int n,
                            double eta, double b1, double b2, double eps, BpArgs bp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const double omb1p = 1.0 - bp.cur[0], omb2p = 1.0 - bp.cur[1];
  if (i == 0) bp_advance(bp, b1, b2);
  if (i >= n) return;
  const double gi = (double)g[i];
  const T mt = (T)(b1 * (double)m[i] + (1.0 - b1) * gi);
  const T vt = (T)(b2 * (double)v[i] + (1.0 - b2) * gi * gi);
  m[i] = mt;
  v[i] = vt;
  const T delta = (T)((double)mt / omb1p / (sqrt((double)vt / omb2p) + eps) * eta);
  p[i] = p[i] - delta;
}

template <class T>
__global__ void polyak_kernel(T* __restrict__ dst, const T* __restrict__ src, int n, T rho, T omr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = rho * dst[i] + omr * src[i];
}

template <class TD, class TS>
__global__ void cast_copy_kernel(TD* __restrict__ dst, const TS* __restrict__ src, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (TD)src[i];
}

// actions[c][f] = clamp(H[f][c] + noise[c][f]*act_noise, +-lim)
// (noise on the first nrows outputs only: the action-memory rows stay noise-free, src/PDEagent.jl:201)
// AN: what carries the amplitude -- the launch scalar, NoiseScale (pdec_mlp_set_noise_scale) or NoiseColor
// (pdec_mlp_set_noise_color: the kernel advances the state of element c n + f with z = noise[c n + f], and `noise` then points
// to DOUBLES whatever T is -- z as it is drawn; the parameter keeps its type so that the other instantiations keep their names)
template <class T, class AN = T>
__global__ void act_noise_clamp_kernel(const T* __restrict__ H, const T* __restrict__ noise, int cols, int n, int nrows,
                                       AN act_noise, T lim, T* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  const noise_elem_t<T, AN>* z = reinterpret_cast<const noise_elem_t<T, AN>*>(noise);
  for (int f = 0; f < n; ++f) {
    T v = H[(size_t)f * cols + c];
    if (noise && f < nrows) v += noise_draw<T>(act_noise, z[(size_t)c * n + f], c, (size_t)c * n + f) * noise_amp<T>(act_noise, c);
    v = v < -lim ? -lim : (v > lim ? lim : v);
    out[(size_t)c * n + f] = v;
  }
}

// ---- counter-based normals: Philox4x32-10 + Box-Muller (philox4x32 in mlp.hpp; replaces randn(rng), PDEagent.jl:201)
template <class T>
__global__ void randn_kernel(T* __restrict__ dst, size_t n, uint64_t seed, uint64_t offset, const uint64_t* ctr_cur = nullptr,
                             uint64_t* ctr_next = nullptr, uint64_t ctr_inc = 0) {
  const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;  // 4 normals per thread
  if (ctr_cur) {       // device-resident counter (pdec_policy_act_rng_dev)
    offset += *ctr_cur;
    if (q == 0) *ctr_next = offset + ctr_inc;
  }
  if (q * 4 >= n) return;
  uint32_t c[4];
  noise_block(c, seed, offset + q);
  for (int h = 0; h < 2; ++h) {
    double rad, ang;
    noise_polar(c, h, rad, ang);
    const size_t i = q * 4 + 2 * h;
    if (i < n) dst[i] = (T)(rad * cos(ang));
    if (i + 1 < n) dst[i + 1] = (T)(rad * sin(ang));
  }
}

// ------------------------------------------------------------------ Mlp methods
template <class T>
static int launch_gemm(Mlp& M, const char* label, GemmArgs<T> g, int nz) {
  dim3 grid(cdiv(g.N, GB_N), cdiv(g.M, GB_M), nz), block(256);
  ProfScope ps(&M, label);
  hipLaunchKernelGGL((gemm_kernel<T>), grid, block, 0, M.stream, g);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int Mlp::init(int dtype_, int L_, const int32_t* dims_, const int32_t* acts_, int max_cols_) {
  dtype = dtype_;
  L = L_;
  max_cols = max_cols_;
  dims.assign(dims_, dims_ + L + 1);
  acts.assign(acts_, acts_ + L);
  w_off.resize(L);
  b_off.resize(L);
  size_t off = 0, maxw = 0;
  int maxd = 0;
  for (int l = 0; l < L; ++l) {
    w_off[l] = off;
    off += (size_t)dims[l] * dims[l + 1];
    b_off[l] = off;
    off += dims[l + 1];
    maxw = std::max(maxw, (size_t)dims[l] * dims[l + 1]);
  }
  for (int l = 0; l <= L; ++l) maxd = std::max(maxd, dims[l]);
  nparams = (int)off;
  const size_t ts = dtype_size(dtype);
  PDEC_HIP(params.alloc(off * ts));
  PDEC_HIP(grads.alloc(off * ts));
  PDEC_HIP(m.alloc(off * ts));
  PDEC_HIP(v.alloc(off * ts));
  PDEC_HIP(hipMemset(params.p, 0, off * ts));
  PDEC_HIP(hipMemset(grads.p, 0, off * ts));
  PDEC_HIP(hipMemset(m.p, 0, off * ts));
  PDEC_HIP(hipMemset(v.p, 0, off * ts));
  PDEC_HIP(hipStreamSynchronize(nullptr));     // the memsets are queued on the null stream; later users run on non-blocking streams
  H.resize(L + 1);
  for (int l = 0; l <= L; ++l) PDEC_HIP(H[l].alloc((size_t)dims[l] * max_cols * ts));
  PDEC_HIP(dz[0].alloc((size_t)maxd * max_cols * ts));
  PDEC_HIP(dz[1].alloc((size_t)maxd * max_cols * ts));
  kchunk = 512;
  nsplit_max = cdiv(max_cols, kchunk);
  PDEC_HIP(slabs.alloc((size_t)nsplit_max * maxw * ts));
  PDEC_HIP(dy.alloc((size_t)dims[L] * max_cols * ts));
  PDEC_HIP(scratch.alloc(64 * 8));
  bp_init = false;       // beta powers initialised on the first adam step (Flux: Float64[beta1, beta2])
  return PDEC_OK;
}

template <class T>
static int pack_t(Mlp& M, const void* s1, int n1, int l1, const void* s2, int n2, int l2, int cols) {
  PDEC_REQUIRE(n1 + n2 == M.dims[0], "mlp: input rows %d+%d != %d", n1, n2, M.dims[0]);
  PDEC_REQUIRE(cols >= 1 && cols <= M.max_cols, "mlp: cols %d exceeds max_cols %d", cols, M.max_cols);
  ProfScope ps(&M, "mlp_pack");
  hipLaunchKernelGGL((pack_kernel<T>), dim3(cdiv(cols, 256)), dim3(256), 0, M.stream, M.H[0].as<T>(), cols, (const T*)s1, n1, l1,
                     (const T*)s2, n2, l2);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

template <class T>
static int forward_t(Mlp& M, int cols) {
  for (int l = 0; l < M.L; ++l) {
    GemmArgs<T> g{};
    g.M = M.dims[l + 1]; g.N = cols; g.K = M.dims[l]; g.kchunk = g.K;
    g.A = M.params.as<T>() + M.w_off[l]; g.sam = M.dims[l]; g.sak = 1;
    g.B = M.H[l].as<T>(); g.sbk = cols; g.sbn = 1;
    g.C = M.H[l + 1].as<T>(); g.scm = cols; g.scn = 1; g.scz = 0;
    g.epi = EPI_BIAS_ACT; g.act = M.acts[l]; g.bias = M.params.as<T>() + M.b_off[l];
    int rc = launch_gemm<T>(M, "mlp_fwd_gemm", g, 1);
    if (rc) return rc;
  }
  return PDEC_OK;
}

// dy: [out][cols] feature-major (ldy=1) or [cols][out] (ldy=0).  Leaves dX0 (w.r.t. the
// packed input, feature-major [in][cols]) in dz[dx_index] when want_dx.
template <class T>
static int backward_t(Mlp& M, const void* dy, int ldy, int cols, bool want_dw, bool want_dx, double grad_scale) {
  const int L = M.L;
  int cur = 0;
  {
    ProfScope ps(&M, "mlp_dz_init");
    hipLaunchKernelGGL((dz_init_kernel<T>), dim3(cdiv(cols, 256)), dim3(256), 0, M.stream, M.dz[cur].as<T>(), (const T*)dy, ldy,
                       M.H[L].as<T>(), M.dims[L], cols, M.acts[L - 1]);
    PDEC_HIP(hipGetLastError());
  }
  for (int l = L - 1; l >= 0; --l) {
    const int out = M.dims[l + 1], in = M.dims[l];
    if (want_dw) {
      const int nz = cdiv(cols, M.kchunk);
      GemmArgs<T> g{};
      g.M = out; g.N = in; g.K = cols; g.kchunk = M.kchunk;
      g.A = M.dz[cur].as<T>(); g.sam = cols; g.sak = 1;
      g.B = M.H[l].as<T>(); g.sbk = 1; g.sbn = cols;
      g.C = M.slabs.as<T>(); g.scm = in; g.scn = 1; g.scz = (long)out * in;
      g.epi = EPI_STORE;
      int rc = launch_gemm<T>(M, "mlp_dw_gemm", g, nz);
      if (rc) return rc;
      ProfScope ps(&M, "mlp_dw_reduce");
      hipLaunchKernelGGL((reduce_slabs_kernel<T>), dim3(cdiv(out * in, 256)), dim3(256), 0, M.stream, M.slabs.as<T>(),
                         M.grads.as<T>() + M.w_off[l], out * in, nz, (size_t)out * in, (T)grad_scale);
      hipLaunchKernelGGL((rowsum_kernel<T>), dim3(out), dim3(256), 0, M.stream, M.dz[cur].as<T>(), M.grads.as<T>() + M.b_off[l], cols,
                         (T)grad_scale);
      PDEC_HIP(hipGetLastError());
    }
    if (l > 0 || want_dx) {
      GemmArgs<T> g{};
      g.M = in; g.N = cols; g.K = out; g.kchunk = out;
      g.A = M.params.as<T>() + M.w_off[l]; g.sam = 1; g.sak = in;   // W^T
      g.B = M.dz[cur].as<T>(); g.sbk = cols; g.sbn = 1;
      g.C = M.dz[cur ^ 1].as<T>(); g.scm = cols; g.scn = 1; g.scz = 0;
      if (l > 0) {
        g.epi = EPI_MUL_DACT; g.act = M.acts[l - 1]; g.aux = M.H[l].as<T>(); g.sauxm = cols; g.sauxn = 1;
      } else {
        g.epi = EPI_STORE;
      }
      int rc = launch_gemm<T>(M, "mlp_dx_gemm", g, 1);
      if (rc) return rc;
      cur ^= 1;
    }
  }
  M.dx_index = cur;
  return PDEC_OK;
}

int Mlp::pack(const void* s1, int n1, int l1, const void* s2, int n2, int l2, int cols) {
  return dtype == PDEC_F64 ? pack_t<double>(*this, s1, n1, l1, s2, n2, l2, cols) : pack_t<float>(*this, s1, n1, l1, s2, n2, l2, cols);
}
int Mlp::forward(int cols) { return dtype == PDEC_F64 ? forward_t<double>(*this, cols) : forward_t<float>(*this, cols); }
int Mlp::backward(const void* dy, int ldy, int cols, bool want_dw, bool want_dx, double grad_scale) {
  return dtype == PDEC_F64 ? backward_t<double>(*this, dy, ldy, cols, want_dw, want_dx, grad_scale)
                           : backward_t<float>(*this, dy, ldy, cols, want_dw, want_dx, grad_scale);
}

int bp_begin(Mlp* M, double beta1, double beta2, BpArgs* out) {
  if (!M->bp_init) {
    if (!M->bpd.p) PDEC_HIP(M->bpd.alloc(4 * sizeof(double)));
    const double init[4] = {beta1, beta2, beta1, beta2};
    PDEC_HIP(hipMemcpy(M->bpd.p, init, sizeof(init), hipMemcpyHostToDevice));   // first step only (never inside a capture)
    M->bp_sel = 0;
    M->bp_init = true;
  }
  out->cur = M->bpd.as<double>() + 2 * M->bp_sel;
  out->next = M->bpd.as<double>() + 2 * (M->bp_sel ^ 1);
  return PDEC_OK;
}

int launch_randn(Object* o, void* dst, size_t n, int dtype, uint64_t seed, uint64_t offset, const uint64_t* ctr_cur,
                 uint64_t* ctr_next, uint64_t ctr_inc) {
  dim3 grid(cdiv((long)((n + 3) / 4), 256)), block(256);
  if (dtype == PDEC_F64)
    hipLaunchKernelGGL((randn_kernel<double>), grid, block, 0, o->stream, (double*)dst, n, seed, offset, ctr_cur, ctr_next, ctr_inc);
  else
    hipLaunchKernelGGL((randn_kernel<float>), grid, block, 0, o->stream, (float*)dst, n, seed, offset, ctr_cur, ctr_next, ctr_inc);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}
}  // namespace pdec

using namespace pdec;

// host conversion between the Julia layout (W column-major [out,in]) and the internal one
template <class T>
static void julia_to_internal(const Mlp& M, const T* src, T* dst) {
  size_t so = 0;
  for (int l = 0; l < M.L; ++l) {
    const int in = M.dims[l], out = M.dims[l + 1];
    for (int o = 0; o < out; ++o)
      for (int i = 0; i < in; ++i) dst[M.w_off[l] + (size_t)o * in + i] = src[so + (size_t)i * out + o];
    so += (size_t)in * out;
    for (int o = 0; o < out; ++o) dst[M.b_off[l] + o] = src[so + o];
    so += out;
  }
}
template <class T>
static void internal_to_julia(const Mlp& M, const T* src, T* dst) {
  size_t so = 0;
  for (int l = 0; l < M.L; ++l) {
    const int in = M.dims[l], out = M.dims[l + 1];
    for (int o = 0; o < out; ++o)
      for (int i = 0; i < in; ++i) dst[so + (size_t)i * out + o] = src[M.w_off[l] + (size_t)o * in + i];
    so += (size_t)in * out;
    for (int o = 0; o < out; ++o) dst[so + o] = src[M.b_off[l] + o];
    so += out;
  }
}

static int set_flat(Mlp* M, DevBuf& buf, const void* host) {
  const size_t ts = dtype_size(M->dtype), n = M->nparams;
  std::vector<unsigned char> tmp(n * ts);
  if (M->dtype == PDEC_F64) julia_to_internal<double>(*M, (const double*)host, (double*)tmp.data());
  else julia_to_internal<float>(*M, (const float*)host, (float*)tmp.data());
  PDEC_HIP(hipMemcpyAsync(buf.p, tmp.data(), n * ts, hipMemcpyHostToDevice, M->stream));
  PDEC_HIP(hipStreamSynchronize(M->stream));
  M->fw_dirty = true;
  return PDEC_OK;
}
static int get_flat(Mlp* M, const DevBuf& buf, void* host) {
  const size_t ts = dtype_size(M->dtype), n = M->nparams;
  std::vector<unsigned char> tmp(n * ts);
  PDEC_HIP(hipMemcpyAsync(tmp.data(), buf.p, n * ts, hipMemcpyDeviceToHost, M->stream));
  PDEC_HIP(hipStreamSynchronize(M->stream));
  if (M->dtype == PDEC_F64) internal_to_julia<double>(*M, (const double*)tmp.data(), (double*)host);
  else internal_to_julia<float>(*M, (const float*)tmp.data(), (float*)host);
  return PDEC_OK;
}

// pdec_policy_act, with the noise in `noise_dtype` (mlp.hpp)
int pdec::policy_act_noise(Mlp* M, const void* state, const void* noise, int noise_dtype, int cols, double act_noise,
                           double act_limit, void* actions_out, const char* who) {
  PDEC_REQUIRE(state && actions_out, "%s: null", who);
  if (noise) PDEC_REQUIRE_NOISE_COLS(M, cols, who);
  PDEC_REQUIRE(noise_dtype == M->dtype || (noise && M->noise_color && noise_dtype == PDEC_F64), "%s: noise of dtype %d", who, noise_dtype);
  if (noise && M->noise_color && noise_dtype != PDEC_F64) {   // a caller's fp32 noise: the recurrence reads z as doubles
    const size_t nz = (size_t)cols * M->dims[M->L];
    if (M->noise.bytes < nz * sizeof(double)) PDEC_HIP(M->noise.alloc(nz * sizeof(double)));
    hipLaunchKernelGGL((cast_copy_kernel<double, float>), dim3(cdiv((long)nz, 256)), dim3(256), 0, M->stream, M->noise.as<double>(),
                       (const float*)noise, (int)nz);
    noise = M->noise.p;
  }
  int rc = M->pack(state, M->dims[0], 0, nullptr, 0, 0, cols);
  if (rc) return rc;
  rc = M->forward(cols);
  if (rc) return rc;
  const int no = M->dims[M->L], nrows = M->noise_rows < 0 ? no : M->noise_rows;
  dim3 grid(cdiv(cols, 256)), block(256);
  ProfScope ps(M, "act_noise_clamp");
  if (noise && M->noise_color && M->dtype == PDEC_F64)
    hipLaunchKernelGGL((act_noise_clamp_kernel<double, NoiseColor>), grid, block, 0, M->stream, M->H[M->L].as<double>(),
                       (const double*)noise, cols, no, nrows, noise_color_of(M, act_noise), act_limit, (double*)actions_out);
  else if (noise && M->noise_color)
    hipLaunchKernelGGL((act_noise_clamp_kernel<float, NoiseColor>), grid, block, 0, M->stream, M->H[M->L].as<float>(),
                       (const float*)noise, cols, no, nrows, noise_color_of(M, act_noise), (float)act_limit, (float*)actions_out);
  else if (noise && M->noise_scale && M->dtype == PDEC_F64)
    hipLaunchKernelGGL((act_noise_clamp_kernel<double, NoiseScale>), grid, block, 0, M->stream, M->H[M->L].as<double>(),
                       (const double*)noise, cols, no, nrows, noise_scale_of(M), act_limit, (double*)actions_out);
  else if (noise && M->noise_scale)
    hipLaunchKernelGGL((act_noise_clamp_kernel<float, NoiseScale>), grid, block, 0, M->stream, M->H[M->L].as<float>(),
                       (const float*)noise, cols, no, nrows, noise_scale_of(M), (float)act_limit, (float*)actions_out);
  else if (M->dtype == PDEC_F64)
    hipLaunchKernelGGL((act_noise_clamp_kernel<double>), grid, block, 0, M->stream, M->H[M->L].as<double>(), (const double*)noise,
                       cols, no, nrows, act_noise, act_limit, (double*)actions_out);
  else
    hipLaunchKernelGGL((act_noise_clamp_kernel<float>), grid, block, 0, M->stream, M->H[M->L].as<float>(), (const float*)noise, cols,
                       no, nrows, (float)act_noise, (float)act_limit, (float*)actions_out);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

extern "C" {

int pdec_mlp_create(pdec_handle* h, int dtype, int n_layers, const int32_t* dims, const int32_t* acts,
                    const void* params_host, int max_cols) {
  PDEC_REQUIRE(h && dims && acts, "pdec_mlp_create: null");
  PDEC_REQUIRE(dtype == PDEC_F32 || dtype == PDEC_F64, "pdec_mlp_create: bad dtype");
  PDEC_REQUIRE(n_layers >= 1 && n_layers <= 8, "pdec_mlp_create: n_layers %d out of [1,8]", n_layers);
  PDEC_REQUIRE(max_cols >= 1, "pdec_mlp_create: max_cols must be >= 1");
  for (int l = 0; l <= n_layers; ++l) PDEC_REQUIRE(dims[l] >= 1 && dims[l] <= 4096, "pdec_mlp_create: dims[%d]=%d", l, dims[l]);
  for (int l = 0; l < n_layers; ++l) PDEC_REQUIRE(acts[l] >= 0 && acts[l] <= 2, "pdec_mlp_create: acts[%d]=%d", l, acts[l]);
  auto M = std::make_unique<Mlp>();
  int rc = M->init(dtype, n_layers, dims, acts, max_cols);
  if (rc) return rc;
  if (params_host && (rc = set_flat(M.get(), M->params, params_host))) return rc;
  *h = register_object(std::move(M));
  return PDEC_OK;
}

int pdec_mlp_num_params(pdec_handle h, int* n) {
  GET_MLP(M, h);
  PDEC_REQUIRE(n, "null");
  *n = M->nparams;
  return PDEC_OK;
}

int pdec_mlp_set_params(pdec_handle h, const void* params_host) {
  GET_MLP(M, h);
  PDEC_REQUIRE(params_host, "pdec_mlp_set_params: null");
  return set_flat(M, M->params, params_host);
}

int pdec_mlp_get_params(pdec_handle h, void* params_host) {
  GET_MLP(M, h);
  PDEC_REQUIRE(params_host, "pdec_mlp_get_params: null");
  return get_flat(M, M->params, params_host);
}

int pdec_mlp_copy(pdec_handle dst, pdec_handle src) {
  GET_MLP(D, dst);
  Mlp* S = lookup_as<Mlp>(src, Kind::Mlp);
  if (!S) { set_error("pdec_mlp_copy: bad src"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(D->dims == S->dims, "pdec_mlp_copy: shape mismatch");
  const int n = D->nparams;
  dim3 grid(cdiv(n, 256)), block(256);
  // order the copy after both handles' streams' prior work: use dst's stream after syncing src's
  if (S->stream != D->stream) PDEC_HIP(hipStreamSynchronize(S->stream));
  if (D->dtype == S->dtype) {
    PDEC_HIP(hipMemcpyAsync(D->params.p, S->params.p, n * dtype_size(D->dtype), hipMemcpyDeviceToDevice, D->stream));
  } else if (D->dtype == PDEC_F64) {
    hipLaunchKernelGGL((cast_copy_kernel<double, float>), grid, block, 0, D->stream, D->params.as<double>(), S->params.as<float>(), n);
  } else {
    hipLaunchKernelGGL((cast_copy_kernel<float, double>), grid, block, 0, D->stream, D->params.as<float>(), S->params.as<double>(), n);
  }
  PDEC_HIP(hipGetLastError());
  D->fw_dirty = true;
  return PDEC_OK;
}

int pdec_mlp_forward(pdec_handle h, const void* x, int cols, void* y_out) {
  GET_MLP(M, h);
  PDEC_REQUIRE(x && y_out, "pdec_mlp_forward: null");
  int rc = M->pack(x, M->dims[0], 0, nullptr, 0, 0, cols);
  if (rc) return rc;
  rc = M->forward(cols);
  if (rc) return rc;
  const int no = M->dims[M->L];
  dim3 grid(cdiv(cols, 256)), block(256);
  if (M->dtype == PDEC_F64)
    hipLaunchKernelGGL((unpack_kernel<double>), grid, block, 0, M->stream, M->H[M->L].as<double>(), cols, no, (double*)y_out);
  else
    hipLaunchKernelGGL((unpack_kernel<float>), grid, block, 0, M->stream, M->H[M->L].as<float>(), cols, no, (float*)y_out);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int pdec_mlp_backward(pdec_handle h, const void* x, const void* dy, int cols, void* dx_out, void* grads_out) {
  GET_MLP(M, h);
  PDEC_REQUIRE(x && dy, "pdec_mlp_backward: null");
  int rc = M->pack(x, M->dims[0], 0, nullptr, 0, 0, cols);
  if (rc) return rc;
  rc = M->forward(cols);
  if (rc) return rc;
  rc = M->backward(dy, 0, cols, true, dx_out != nullptr, 1.0);
  if (rc) return rc;
  dim3 grid(cdiv(cols, 256)), block(256);
  if (dx_out) {
    if (M->dtype == PDEC_F64)
      hipLaunchKernelGGL((unpack_kernel<double>), grid, block, 0, M->stream, M->dz[M->dx_index].as<double>(), cols, M->dims[0], (double*)dx_out);
    else
      hipLaunchKernelGGL((unpack_kernel<float>), grid, block, 0, M->stream, M->dz[M->dx_index].as<float>(), cols, M->dims[0], (float*)dx_out);
    PDEC_HIP(hipGetLastError());
  }
  if (grads_out) {
    // grads_out is a DEVICE buffer in the Julia layout: convert through the host (setup/test path)
    const size_t ts = dtype_size(M->dtype);
    std::vector<unsigned char> tmp((size_t)M->nparams * ts);
    rc = get_flat(M, M->grads, tmp.data());
    if (rc) return rc;
    PDEC_HIP(hipMemcpy(grads_out, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
  }
  return PDEC_OK;
}

int pdec_mlp_grad_buffer(pdec_handle h, void** dptr, int* n) {
  GET_MLP(M, h);
  PDEC_REQUIRE(dptr && n, "null");
  *dptr = M->grads.p;
  *n = M->nparams;
  return PDEC_OK;
}

int pdec_adam_step(pdec_handle h, double eta, double beta1, double beta2, double eps) {
  GET_MLP(M, h);
  BpArgs bp;
  int rc = bp_begin(M, beta1, beta2, &bp);
  if (rc) return rc;
  const int n = M->nparams;
  dim3 grid(cdiv(n, 256)), block(256);
  {
    ProfScope ps(M, "adam");
    if (M->dtype == PDEC_F64)
      hipLaunchKernelGGL((adam_kernel<double>), grid, block, 0, M->stream, M->params.as<double>(), M->grads.as<double>(),
                         M->m.as<double>(), M->v.as<double>(), n, eta, beta1, beta2, eps, bp);
    else
      hipLaunchKernelGGL((adam_kernel<float>), grid, block, 0, M->stream, M->params.as<float>(), M->grads.as<float>(),
                         M->m.as<float>(), M->v.as<float>(), n, eta, beta1, beta2, eps, bp);
  }
  PDEC_HIP(hipGetLastError());
  M->fw_dirty = true;
  bp_done(M);
  return PDEC_OK;
}

int pdec_adam_get_state(pdec_handle h, void* m_host, void* v_host, double* beta_pow2) {
  GET_MLP(M, h);
  int rc;
  if (m_host && (rc = get_flat(M, M->m, m_host))) return rc;
  if (v_host && (rc = get_flat(M, M->v, v_host))) return rc;
  if (beta_pow2) {
    beta_pow2[0] = beta_pow2[1] = -1.0;      // not initialised before the first ADAM step
    if (M->bp_init) {
      PDEC_HIP(hipStreamSynchronize(M->stream));
      PDEC_HIP(hipMemcpy(beta_pow2, M->bpd.as<double>() + 2 * M->bp_sel, 16, hipMemcpyDeviceToHost));
    }
  }
  return PDEC_OK;
}

int pdec_adam_set_state(pdec_handle h, const void* m_host, const void* v_host, const double* beta_pow2) {
  GET_MLP(M, h);
  int rc;
  if (m_host && (rc = set_flat(M, M->m, m_host))) return rc;
  if (v_host && (rc = set_flat(M, M->v, v_host))) return rc;
  if (beta_pow2) {
    if (beta_pow2[0] < 0) {
      M->bp_init = false;
    } else {
      if (!M->bpd.p) PDEC_HIP(M->bpd.alloc(4 * sizeof(double)));
      PDEC_HIP(hipStreamSynchronize(M->stream));
      PDEC_HIP(hipMemcpy(M->bpd.as<double>() + 2 * M->bp_sel, beta_pow2, 16, hipMemcpyHostToDevice));
      M->bp_init = true;
    }
  }
  return PDEC_OK;
}

int pdec_polyak(pdec_handle dst, pdec_handle src, double rho) {
  GET_MLP(D, dst);
  Mlp* S = lookup_as<Mlp>(src, Kind::Mlp);
  if (!S) { set_error("pdec_polyak: bad src"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(D->dims == S->dims && D->dtype == S->dtype, "pdec_polyak: shape/dtype mismatch");
  // rho == 1: dest = 1 * dest + 0 * src -- the reference as it runs (its loop body never executes, include/pdeconv.h at this
  // entry point): the target is left untouched, also where src holds an Inf / NaN that 0 * src would turn into NaN
  // (compared as Float32 for fp64 networks too: the kernels below receive r = (float)rho -- the reference holds p = 0.995f0 --, so a
  // rho that rounds to 1.0f IS the frozen case in their arithmetic: (double)r = 1, (double)(1.0f - r) = 0)
  if ((float)rho == 1.0f) return PDEC_OK;
  const int n = D->nparams;
  dim3 grid(cdiv(n, 256)), block(256);
  ProfScope ps(D, "polyak");
  const float r = (float)rho;  // the reference holds p = 0.995f0 and computes (1 - p) in Float32
  if (D->dtype == PDEC_F64) {
    hipLaunchKernelGGL((polyak_kernel<double>), grid, block, 0, D->stream, D->params.as<double>(), S->params.as<double>(), n,
                       (double)r, (double)(1.0f - r));
  } else {
    hipLaunchKernelGGL((polyak_kernel<float>), grid, block, 0, D->stream, D->params.as<float>(), S->params.as<float>(), n, r, 1.0f - r);
  }
  PDEC_HIP(hipGetLastError());
  D->fw_dirty = true;
  return PDEC_OK;
}

int pdec_policy_act(pdec_handle actor, const void* state, const void* noise, int cols, double act_noise,
                    double act_limit, void* actions_out) {
  GET_MLP(M, actor);
  return policy_act_noise(M, state, noise, M->dtype, cols, act_noise, act_limit, actions_out, "pdec_policy_act");
}

int pdec_randn(pdec_handle any_handle, void* dst, size_t n, int dtype, uint64_t seed, uint64_t offset) {
  Object* o = lookup(any_handle);
  if (!o) { set_error("pdec_randn: bad handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(dst, "pdec_randn: null");
  if (n == 0) return PDEC_OK;
  return launch_randn(o, dst, n, dtype, seed, offset, nullptr, nullptr, 0);
}

int pdec_mlp_acts_on_published_copy(pdec_handle actor, int* yes) {
  GET_MLP(M, actor);
  PDEC_REQUIRE(yes, "pdec_mlp_acts_on_published_copy: null");
  *yes = fused3_family.act_ok(M, 1) ? 1 : 0;      // the 3-layer family acts on the published image, at any number of columns
  return PDEC_OK;
}

}  // extern "C"
