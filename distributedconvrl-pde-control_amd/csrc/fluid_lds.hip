// fluid_lds.hip -- the LDS-tile kernels of the 2-D fluid environment: transforms of a tile of lines out of LDS (any length
// that factors into 2, 3, 5), the three passes K1 / K2 / K3 of a right-hand side on them (advection, src/fluid_rk4.jl:145-190,
// with pad / chop :192-229 as index maps; rhs :134-143 and the rk4 stage update :122-132 in K3), and the plain 2-D transforms of
// the n x n grid that sensing and actuation use at every size (FluidSetup.jl:189,206,260).  fluid.hip has the design note.
#include "fluid.hpp"

namespace pdec {

// ------------------------------------------------------------------ tile FFT (nlines lines of one length in LDS)
template <int R, int SGN, class T>
__device__ __forceinline__ void tile_stage(const C2<T>* __restrict__ x, C2<T>* __restrict__ y,
                                           const C2<T>* __restrict__ tw, int N, int n, int s, int u0, int tpl) {
  const int m = n / R, nb = N / R;
  const bool pow2 = (s & (s - 1)) == 0;
  const int sh = 31 - __clz(s);
  for (int u = u0; u < nb; u += tpl) {
    int pp, q;
    if (pow2) { pp = u >> sh; q = u & (s - 1); }
    else { pp = u / s; q = u - pp * s; }
    C2<T> a[R];
#pragma unroll
    for (int j = 0; j < R; ++j) a[j] = x[q + s * (pp + m * j)];
    dft_small<R, SGN, T>(a);
    const int base = q + s * R * pp, ps = pp * s;
    y[base] = a[0];
    // one twiddle read per butterfly; w^2, w^3 by multiplication (the LDS, not the fp64 VALU, is the busy unit here)
    C2<T> w1 = tw[ps];
    if (SGN > 0) w1.y = -w1.y;
    C2<T> w = w1;
#pragma unroll
    for (int k = 1; k < R; ++k) {
      y[base + s * k] = cmul(a[k], w);
      if (k + 1 < R) w = cmul(w, w1);
    }
  }
}

// Transforms `nlines` (power of two <= FL_NTH) lines X[l*LS .. l*LS+N) -> returned buffer (X or Y).
// Issues a barrier before the first stage and after every stage.
template <int SGN, class T>
__device__ __forceinline__ C2<T>* tile_fft(C2<T>* X, C2<T>* Y, const C2<T>* tw, const FftPlan& pl, int LS,
                                           int nlines, int tid) {
  const int tpl = FL_NTH / nlines;
  const int line = tid / tpl, u0 = tid - line * tpl;
  int n = pl.N, s = 1;
  __syncthreads();
  for (int st = 0; st < pl.nstages; ++st) {
    const int r = pl.radix[st];
    const C2<T>* x = X + line * LS;
    C2<T>* y = Y + line * LS;
    if (r == 4) tile_stage<4, SGN, T>(x, y, tw, pl.N, n, s, u0, tpl);
    else if (r == 2) tile_stage<2, SGN, T>(x, y, tw, pl.N, n, s, u0, tpl);
    else if (r == 3) tile_stage<3, SGN, T>(x, y, tw, pl.N, n, s, u0, tpl);
    else tile_stage<5, SGN, T>(x, y, tw, pl.N, n, s, u0, tpl);
    __syncthreads();
    C2<T>* t = X; X = Y; Y = t;
    n /= r;
    s *= r;
  }
  return X;
}

// spectral velocities / vorticity gradients of one mode (src/fluid_rk4.jl:152-161)
template <class T>
__device__ __forceinline__ void fl_spec(C2<T> o, T kx, T ky, bool dc, C2<T>& u, C2<T>& v, C2<T>& wx, C2<T>& wy) {
  const T k2 = kx * kx + ky * ky;
  C2<T> psi = mk<T>(0, 0);
  if (!dc) psi = mk<T>(o.x / k2, o.y / k2);       // psihat = omghat ./ kx2ky2; psihat[1,1] = 0
  u = mk<T>(-ky * psi.y, ky * psi.x);             // uhat =  i ky psihat
  v = mk<T>(kx * psi.y, -kx * psi.x);             // vhat = -i kx psihat
  wx = mk<T>(-kx * o.y, kx * o.x);                // domgdx = i kx omghat
  wy = mk<T>(-ky * o.y, ky * o.x);                // domgdy = i ky omghat
}

// ------------------------------------------------------------------ K1: spectra + pad + Herm + inverse pass along y
// grid (ceil(nl/TL), B).  W[b][f][s][ip], f = 0: Z1, 1: Z2 (unnormalised inverse along y).
template <class T>
__global__ __launch_bounds__(FL_NTH) void fluid_k1_kernel(FluidDev<T> d, const C2<T>* __restrict__ omg,
                                                          C2<T>* __restrict__ W) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  C2<T>* X = reinterpret_cast<C2<T>*>(smem_raw);
  C2<T>* Y = X + d.TL * d.LS;
  C2<T>* tw = Y + d.TL * d.LS;
  const int tid = threadIdx.x, n = d.n, p = d.p, LS = d.LS;
  for (int k = tid; k < p; k += FL_NTH) tw[k] = d.twp[k];
  const int tpl = FL_NTH / d.TL, line = tid / tpl, u0 = tid - line * tpl;
  const int s = blockIdx.x * d.TL + line, b = blockIdx.y;
  const bool live = s < d.nl;
  int j = -1, jm = -1;
  if (live) {
    const int jp = fl_line_jp(s, n, p, d.nl);
    j = fl_unpad(jp, n, p);
    jm = fl_unpad((p - jp) % p, n, p);
  }
  const C2<T>* oj = omg + ((size_t)b * n + (j >= 0 ? j : 0)) * n;
  const C2<T>* om = omg + ((size_t)b * n + (jm >= 0 ? jm : 0)) * n;
  const T kj = j >= 0 ? d.k[j] : (T)0, kjm = jm >= 0 ? d.k[jm] : (T)0;
  C2<T> z2[FL_MAXE];
#pragma unroll
  for (int e = 0; e < FL_MAXE; ++e) {
    const int ip = u0 + tpl * e;
    z2[e] = mk<T>(0, 0);
    if (ip < p) {
      const int i = fl_unpad(ip, n, p), im = fl_unpad((p - ip) % p, n, p);
      C2<T> au = mk<T>(0, 0), av = au, ax = au, ay = au, mu = au, mv = au, mx = au, my = au;
      if (j >= 0 && i >= 0) fl_spec<T>(oj[i], kj, d.k[i], i == 0 && j == 0, au, av, ax, ay);
      if (jm >= 0 && im >= 0) fl_spec<T>(om[im], kjm, d.k[im], im == 0 && jm == 0, mu, mv, mx, my);
      // Herm(A) = (A(k) + conj(A(-k))) / 2
      const C2<T> hu = mk<T>((T)0.5 * (au.x + mu.x), (T)0.5 * (au.y - mu.y));
      const C2<T> hv = mk<T>((T)0.5 * (av.x + mv.x), (T)0.5 * (av.y - mv.y));
      const C2<T> hx = mk<T>((T)0.5 * (ax.x + mx.x), (T)0.5 * (ax.y - mx.y));
      const C2<T> hy = mk<T>((T)0.5 * (ay.x + my.x), (T)0.5 * (ay.y - my.y));
      X[line * LS + ip] = mk<T>(hu.x - hv.y, hu.y + hv.x);   // Z1 = Herm(u) + i Herm(v)
      z2[e] = mk<T>(hx.x - hy.y, hx.y + hy.x);               // Z2 = Herm(wx) + i Herm(wy)
    }
  }
  C2<T>* R = tile_fft<+1, T>(X, Y, tw, d.plp, LS, d.TL, tid);
  if (live) {
    C2<T>* w0 = W + (((size_t)b * 2 + 0) * d.nl + s) * p;
#pragma unroll
    for (int e = 0; e < FL_MAXE; ++e) {
      const int ip = u0 + tpl * e;
      if (ip < p) w0[ip] = R[line * LS + ip];
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < FL_MAXE; ++e) {
    const int ip = u0 + tpl * e;
    if (ip < p) X[line * LS + ip] = z2[e];
  }
  R = tile_fft<+1, T>(X, Y, tw, d.plp, LS, d.TL, tid);
  if (live) {
    C2<T>* w1 = W + (((size_t)b * 2 + 1) * d.nl + s) * p;
#pragma unroll
    for (int e = 0; e < FL_MAXE; ++e) {
      const int ip = u0 + tpl * e;
      if (ip < p) w1[ip] = R[line * LS + ip];
    }
  }
}

// ------------------------------------------------------------------ K2: inverse pass along x, product, forward pass along x
// grid (ceil(p/TL), B).  W2[b][j][ip] = chop_x( FFT_x( -(u wx + v wy) ) ), two columns per complex line.
template <class T>
__global__ __launch_bounds__(FL_NTH) void fluid_k2_kernel(FluidDev<T> d, const C2<T>* __restrict__ W,
                                                          C2<T>* __restrict__ W2) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  C2<T>* X = reinterpret_cast<C2<T>*>(smem_raw);
  C2<T>* Y = X + d.TL * d.LS;
  C2<T>* tw = Y + d.TL * d.LS;
  const int tid = threadIdx.x, n = d.n, p = d.p, LS = d.LS, TL = d.TL;
  for (int k = tid; k < p; k += FL_NTH) tw[k] = d.twp[k];
  const int tlsh = 31 - __clz(TL);
  const int tpl = FL_NTH / TL, line = tid / tpl, u0 = tid - line * tpl;
  const int ip0 = blockIdx.x * TL, b = blockIdx.y;
  C2<T> r0[FL_MAXE];
  T wre[FL_MAXE];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    if (f) __syncthreads();
    const C2<T>* Wf = W + (((size_t)b * 2 + f) * d.nl) * p;
    for (int idx = tid; idx < TL * p; idx += FL_NTH) {       // transposed load, zero fill = pad() along x
      const int t = idx & (TL - 1), jp = idx >> tlsh;
      const int s = fl_line_of(jp, n, p, d.nl), ip = ip0 + t;
      C2<T> v = mk<T>(0, 0);
      if (s >= 0 && ip < p) v = Wf[(size_t)s * p + ip];
      X[t * LS + jp] = v;
    }
    C2<T>* R = tile_fft<+1, T>(X, Y, tw, d.plp, LS, TL, tid);
#pragma unroll
    for (int e = 0; e < FL_MAXE; ++e) {
      const int jp = u0 + tpl * e;
      if (jp < p) {
        const C2<T> v = R[line * LS + jp];
        if (f == 0) r0[e] = v;
        else wre[e] = -(r0[e].x * v.x + r0[e].y * v.y) * d.inv2;   // -(u wx + v wy), both ifft scalings
      }
    }
  }
  __syncthreads();
  const int half = TL / 2;
#pragma unroll
  for (int e = 0; e < FL_MAXE; ++e) {
    const int jp = u0 + tpl * e;
    if (jp < p) {
      T* dst = reinterpret_cast<T*>(&X[(line & (half - 1)) * LS + jp]);
      dst[line >= half ? 1 : 0] = wre[e];
    }
  }
  C2<T>* R = tile_fft<-1, T>(X, Y, tw, d.plp, LS, half, tid);
  for (int idx = tid; idx < TL * n; idx += FL_NTH) {
    const int t = idx & (TL - 1), jj = idx >> tlsh;
    const int ip = ip0 + t;
    if (ip >= p) continue;
    const int jp = fl_pad(jj, n, p), jq = (p - jp) % p, tt = t & (half - 1);
    const C2<T> y = R[tt * LS + jp], ym = R[tt * LS + jq];
    C2<T> o;
    if (t < half) o = mk<T>((T)0.5 * (y.x + ym.x), (T)0.5 * (y.y - ym.y));     // (Y + conj(Ym)) / 2
    else o = mk<T>((T)0.5 * (y.y + ym.y), (T)-0.5 * (y.x - ym.x));              // (Y - conj(Ym)) / (2i)
    W2[((size_t)b * n + jj) * p + ip] = o;
  }
}

// ------------------------------------------------------------------ K3: forward pass along y, chop, rhs, RK4 stage
// grid (ceil(n/TL), B).  mode 0: out = rhs;  1: out = f0 + ca k, acc = f0 + cb k;  2: out = f0 + ca k, acc += cb k;
// 4: out = acc + cb k.
template <class T>
__global__ __launch_bounds__(FL_NTH) void fluid_k3_kernel(FluidDev<T> d, const C2<T>* __restrict__ W2,
                                                          const C2<T>* omg_s, const C2<T>* __restrict__ phat,
                                                          const C2<T>* f0, C2<T>* acc, C2<T>* out, int mode, T ca, T cb) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  C2<T>* X = reinterpret_cast<C2<T>*>(smem_raw);
  C2<T>* Y = X + d.TL * d.LS;
  C2<T>* tw = Y + d.TL * d.LS;
  const int tid = threadIdx.x, n = d.n, p = d.p, LS = d.LS;
  for (int k = tid; k < p; k += FL_NTH) tw[k] = d.twp[k];
  const int tpl = FL_NTH / d.TL, line = tid / tpl, u0 = tid - line * tpl;
  const int j = blockIdx.x * d.TL + line, b = blockIdx.y;
  const bool live = j < n;
  const C2<T>* w2 = W2 + ((size_t)b * n + (live ? j : 0)) * p;
#pragma unroll
  for (int e = 0; e < FL_MAXE; ++e) {
    const int ip = u0 + tpl * e;
    if (ip < p) X[line * LS + ip] = live ? w2[ip] : mk<T>(0, 0);
  }
  C2<T>* R = tile_fft<-1, T>(X, Y, tw, d.plp, LS, d.TL, tid);
  if (!live) return;
  const T kj = d.k[j];
#pragma unroll
  for (int e = 0; e < FL_MAXE; ++e) {
    const int ip = u0 + tpl * e;
    if (ip >= p) continue;
    const int i = fl_unpad(ip, n, p);
    if (i < 0) continue;
    const size_t off = ((size_t)b * n + j) * n + i;
    const T ki = d.k[i], lin = -d.nu * (kj * kj + ki * ki);
    const C2<T> o = omg_s[off], nl = R[line * LS + ip], ph = phat[off];
    const C2<T> k = mk<T>(lin * o.x + d.scale_out * nl.x + ph.x, lin * o.y + d.scale_out * nl.y + ph.y);
    if (mode == 0) {
      out[off] = k;
    } else if (mode == 4) {
      const C2<T> a = acc[off];
      out[off] = mk<T>(a.x + cb * k.x, a.y + cb * k.y);
    } else {
      const C2<T> f = f0[off];
      out[off] = mk<T>(f.x + ca * k.x, f.y + ca * k.y);
      if (mode == 1) acc[off] = mk<T>(f.x + cb * k.x, f.y + cb * k.y);
      else {
        const C2<T> a = acc[off];
        acc[off] = mk<T>(a.x + cb * k.x, a.y + cb * k.y);
      }
    }
  }
}

// ------------------------------------------------------------------ plain 2-D FFT passes of the n x n grid
// (sensing: y = real(ifft(env.y)), FluidSetup.jl:189,206; actuation: fft(p), :260)
template <class T, int SGN, bool REAL_IN>
__global__ __launch_bounds__(FL_NTH) void fluid_fft_fast_kernel(FluidDev<T> d, const void* __restrict__ in,
                                                                C2<T>* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  C2<T>* X = reinterpret_cast<C2<T>*>(smem_raw);
  C2<T>* Y = X + d.TLn * d.LSn;
  C2<T>* tw = Y + d.TLn * d.LSn;
  const int tid = threadIdx.x, n = d.n, LS = d.LSn;
  for (int k = tid; k < n; k += FL_NTH) tw[k] = d.twn[k];
  const int tpl = FL_NTH / d.TLn, line = tid / tpl, u0 = tid - line * tpl;
  const int j = blockIdx.x * d.TLn + line, b = blockIdx.y;
  const bool live = j < n;
  const size_t base = ((size_t)b * n + (live ? j : 0)) * n;
#pragma unroll
  for (int e = 0; e < FL_MAXE; ++e) {
    const int i = u0 + tpl * e;
    if (i < n) {
      C2<T> v = mk<T>(0, 0);
      if (live) v = REAL_IN ? mk<T>(static_cast<const T*>(in)[base + i], 0) : static_cast<const C2<T>*>(in)[base + i];
      X[line * LS + i] = v;
    }
  }
  C2<T>* R = tile_fft<SGN, T>(X, Y, tw, d.pln, LS, d.TLn, tid);
  if (!live) return;
#pragma unroll
  for (int e = 0; e < FL_MAXE; ++e) {
    const int i = u0 + tpl * e;
    if (i < n) out[base + i] = R[line * LS + i];
  }
}

template <class T, int SGN, bool REAL_OUT>
__global__ __launch_bounds__(FL_NTH) void fluid_fft_slow_kernel(FluidDev<T> d, const C2<T>* __restrict__ in,
                                                                void* __restrict__ out, T scale) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  C2<T>* X = reinterpret_cast<C2<T>*>(smem_raw);
  C2<T>* Y = X + d.TLn * d.LSn;
  C2<T>* tw = Y + d.TLn * d.LSn;
  const int tid = threadIdx.x, n = d.n, LS = d.LSn, TL = d.TLn;
  for (int k = tid; k < n; k += FL_NTH) tw[k] = d.twn[k];
  const int tlsh = 31 - __clz(TL);
  const int i0 = blockIdx.x * TL, b = blockIdx.y;
  for (int idx = tid; idx < TL * n; idx += FL_NTH) {
    const int t = idx & (TL - 1), j = idx >> tlsh, i = i0 + t;
    X[t * LS + j] = i < n ? in[((size_t)b * n + j) * n + i] : mk<T>(0, 0);
  }
  C2<T>* R = tile_fft<SGN, T>(X, Y, tw, d.pln, LS, TL, tid);
  for (int idx = tid; idx < TL * n; idx += FL_NTH) {
    const int t = idx & (TL - 1), j = idx >> tlsh, i = i0 + t;
    if (i >= n) continue;
    const C2<T> v = R[t * LS + j];
    const size_t off = ((size_t)b * n + j) * n + i;
    if (REAL_OUT) static_cast<T*>(out)[off] = v.x * scale;
    else static_cast<C2<T>*>(out)[off] = mk<T>(v.x * scale, v.y * scale);
  }
}

// ------------------------------------------------------------------ host side
int pick_tile(int len) {
  int t = 16;
  while (t > 1 && t * len > FL_NTH * FL_MAXE) t >>= 1;
  return t;
}

template <class K>
static int set_lds(K kern, size_t bytes) {
  PDEC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return PDEC_OK;
}

int fluid_set_attrs(const FluidEnv& E) {
  return fluid_by_dtype(E, [&](auto t) -> int {
    typedef decltype(t) T;
    int rc;
    if ((rc = set_lds(fluid_k1_kernel<T>, E.lds_p))) return rc;
    if ((rc = set_lds(fluid_k2_kernel<T>, E.lds_p))) return rc;
    if ((rc = set_lds(fluid_k3_kernel<T>, E.lds_p))) return rc;
    if ((rc = set_lds(fluid_fft_fast_kernel<T, +1, false>, E.lds_n))) return rc;
    if ((rc = set_lds(fluid_fft_fast_kernel<T, -1, true>, E.lds_n))) return rc;
    if ((rc = set_lds(fluid_fft_slow_kernel<T, +1, true>, E.lds_n))) return rc;
    if ((rc = set_lds(fluid_fft_slow_kernel<T, -1, false>, E.lds_n))) return rc;
    return PDEC_OK;
  });
}

template <class T>
static int fluid_rhs_launch_lds_t(FluidEnv& E, const void* omg_s, const void* phat, const void* f0, void* acc, void* out,
                                  int mode, double ca, double cb) {
  typedef C2<T> Z;
  const FluidDev<T> d = fluid_dev<T>(E);
  const int B = E.cfg.B;
  {
    ProfScope ps(&E, "fluid_k1", true);
    for (int r = 0; r < ps.reps; ++r)
      hipLaunchKernelGGL(fluid_k1_kernel<T>, dim3((E.nl + E.TL - 1) / E.TL, B), dim3(FL_NTH), E.lds_p, E.stream, d,
                         (const Z*)omg_s, E.W.as<Z>());
  }
  {
    ProfScope ps(&E, "fluid_k2", true);
    for (int r = 0; r < ps.reps; ++r)
      hipLaunchKernelGGL(fluid_k2_kernel<T>, dim3((E.p + E.TL - 1) / E.TL, B), dim3(FL_NTH), E.lds_p, E.stream, d,
                         E.W.as<Z>(), E.W2.as<Z>());
  }
  {
    ProfScope ps(&E, "fluid_k3", mode == 0);
    for (int r = 0; r < ps.reps; ++r)
      hipLaunchKernelGGL(fluid_k3_kernel<T>, dim3((E.n + E.TL - 1) / E.TL, B), dim3(FL_NTH), E.lds_p, E.stream, d,
                         E.W2.as<Z>(), (const Z*)omg_s, (const Z*)phat, (const Z*)f0, (Z*)acc, (Z*)out, mode, (T)ca, (T)cb);
  }
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int fluid_rhs_launch_lds(FluidEnv& E, const void* omg_s, const void* phat, const void* f0, void* acc, void* out, int mode, double ca,
                         double cb) {
  return fluid_by_dtype(E, [&](auto t) -> int {
    return fluid_rhs_launch_lds_t<decltype(t)>(E, omg_s, phat, f0, acc, out, mode, ca, cb);
  });
}

// ---- the n x n transform pair through E.tmpc, each direction written once
// spec = fft2(real), un-scaled (actuation, FluidSetup.jl:260; the initialisers); launches only: the caller checks for errors
int fluid_fft2_of_real(FluidEnv& E, const void* real, void* spec) {
  return fluid_by_dtype(E, [&](auto t) -> int {
    typedef decltype(t) T;
    typedef C2<T> Z;
    const FluidDev<T> d = fluid_dev<T>(E);
    const dim3 grid((E.n + E.TLn - 1) / E.TLn, E.cfg.B);
    hipLaunchKernelGGL((fluid_fft_fast_kernel<T, -1, true>), grid, dim3(FL_NTH), E.lds_n, E.stream, d, real, E.tmpc.as<Z>());
    hipLaunchKernelGGL((fluid_fft_slow_kernel<T, -1, false>), grid, dim3(FL_NTH), E.lds_n, E.stream, d, E.tmpc.as<Z>(), spec, (T)1);
    return PDEC_OK;
  });
}

// yreal = real(ifft(y))   (sensing, FluidSetup.jl:189,206; error_detection)
int fluid_to_physical(FluidEnv& E, const void* y) {
  return fluid_by_dtype(E, [&](auto t) -> int {
    typedef decltype(t) T;
    typedef C2<T> Z;
    const FluidDev<T> d = fluid_dev<T>(E);
    const dim3 grid((E.n + E.TLn - 1) / E.TLn, E.cfg.B);
    ProfScope ps(&E, "fluid_ifft2");
    hipLaunchKernelGGL((fluid_fft_fast_kernel<T, +1, false>), grid, dim3(FL_NTH), E.lds_n, E.stream, d, y, E.tmpc.as<Z>());
    hipLaunchKernelGGL((fluid_fft_slow_kernel<T, +1, true>), grid, dim3(FL_NTH), E.lds_n, E.stream, d, E.tmpc.as<Z>(), E.yreal.p,
                       d.invn2);
    PDEC_HIP(hipGetLastError());
    return PDEC_OK;
  });
}

}  // namespace pdec
