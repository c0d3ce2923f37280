// random_init.hpp -- the episode initialiser of the 1-D setups as a device function, shared by random_init_kernel (replay.hip:
// pdec_env_random_init, pdec_env_random_init_members) and the episode clock's boundary launch (episode_clock.hip), which
// draws the new field of a trajectory whose episode has just ended.  Both launch 256 threads per trajectory: the KS rescale
// is a tree reduction over blockDim.x partial sums, so the drawn field depends on that size.
#pragma once
#include "env.hpp"
#include "mlp.hpp"      // philox4x32

namespace pdec {

#define RI_MAXC 64
#define RI_THREADS 256

// the constants of generate_random_init for an environment (replay.hip: random_init_kernel's comment)
struct RandomInitSpec {
  int N, nsp, nsin;
  double dx, fdiv, base, l2;
};
// false: not a 1-D setup (the 2-D Keller-Segel and the fluid have initialisers of their own)
inline bool random_init_spec(const pdec_env_cfg& c, RandomInitSpec* s) {
  const double two_pi = 6.283185307179586;
  if (c.pde_kind == PDEC_PDE_KS_CNAB2 || c.pde_kind == PDEC_PDE_KS_RK4_FD) {
    s->nsp = 1; s->nsin = 8; s->fdiv = two_pi; s->base = 0.0; s->l2 = 30.0;                                  // KSSetup.jl:288-298
  } else if (c.pde_kind == PDEC_PDE_KSEG_RK4) {
    s->nsp = 2; s->nsin = (int)ceil(c.Lx / 3.0); s->fdiv = two_pi * (c.Lx / 22.0); s->base = 1.0; s->l2 = 0.0;   // KellerSegelSetup.jl:373-384
  } else {
    return false;
  }
  s->N = c.N;
  s->dx = c.Lx / c.N;
  return true;
}

// trajectory b of y [B][N][nsp] from the Philox blocks (seed; ctr0 .. ctr0 + ceil(nc / 4) - 1).  Every thread of the
// workgroup calls it; a [RI_MAXC] and red [blockDim.x] are LDS.
template <class T>
__device__ __forceinline__ void random_init_row(T* __restrict__ y, int b, int N, int nsp, int nsin, double dx, double fdiv, double base,
                                                double l2_target, uint64_t seed, uint64_t ctr0, double* a, double* red) {
  const int tid = threadIdx.x, nc = nsp * nsin, nblk = (nc + 3) / 4;
  if (tid == 0) {
    double nrm = 0;
    for (int blk = 0; blk < nblk; ++blk) {
      const uint64_t ctr = ctr0 + blk;
      uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
      philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
      for (int i = 0; i < 4 && 4 * blk + i < nc; ++i) {
        const double v = 2.0 * (((double)c[i] + 0.5) * (1.0 / 4294967296.0)) - 1.0;
        a[4 * blk + i] = v;
        nrm += v * v;
      }
    }
    nrm = sqrt(nrm);
    for (int i = 0; i < nc; ++i) a[i] /= nrm;
  }
  __syncthreads();
  double scale = 1.0;
  if (l2_target > 0) {      // KS: rescale to |y0|_2 = 30 (one species)
    double acc = 0;
    for (int j = tid; j < N; j += blockDim.x) {
      const double x = (j + 1) * dx;
      double v = 0;
      for (int i = 1; i <= nsin; ++i) v += a[i - 1] * sin(i * x / fdiv);
      acc += v * v;
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    scale = l2_target / sqrt(red[0]);
  }
  for (int j = tid; j < N; j += blockDim.x) {
    const double x = (j + 1) * dx;
    for (int sp = 0; sp < nsp; ++sp) {
      double v = 0;
      for (int i = 1; i <= nsin; ++i) v += a[sp * nsin + i - 1] * sin(i * x / fdiv);
      y[((size_t)b * N + j) * nsp + sp] = (T)(base + v * scale);
    }
  }
}

}  // namespace pdec
