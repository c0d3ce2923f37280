// fluid_wave.hip -- the one-line-per-wave kernels of the 2-D fluid environment and the table of WaveFft plans that serve them:
// K1w / K2w / K2p / K3w are the three passes of a right-hand side (advection, src/fluid_rk4.jl:145-190, with pad / chop :192-229
// as index maps; rhs :134-143 and the rk4 stage update :122-132 in K3w), K31w is K3w of one stage fused with K1w of the next
// right-hand side; their launchers, the fused integrator of do_step (FluidSetup.jl:163-172), and the unit-test entries of the
// register transforms and of the table.  fluid.hip has the design note.
#include "fluid.hpp"

namespace pdec {

// ------------------------------------------------------------------ wave-FFT variants of K1 / K2 / K3
// Same three passes, but every line transform runs in the registers of ONE wave (wave_fft.hpp): no LDS stage
// round trips, no barriers inside a transform.  LDS is only used to turn coalesced global accesses into the
// permuted (digit-reversed) element order the transforms consume / produce, and for K2's column transposition.
// Used when the padded length p has a row in fluid_wave_table below (otherwise the LDS-tile kernels of fluid_lds.hip); 64 and
// 192 run two lines per wave (half-wave transforms).

// the spectral part of K1w for one work item: from the two spectrum lines in LDS (Lj: line j0, Lm: its mirror j1) the
// packed inverse transforms of the carried line t and -- nhalf = 2 -- of its mirror line s_mirror
template <class T, int E, int Q, int LB>
__device__ __forceinline__ void fluid_k1w_body(const FluidDev<T>& d, const C2<T>* Lj, const C2<T>* Lm, int j0, int j1,
                                               int t, int s_mirror, int nhalf, C2<T>* __restrict__ W, int b,
                                               WaveFft<T, E, Q, LB>& f, int l, const T* __restrict__ kt) {
  typedef WaveFft<T, E, Q, LB> F;
  typedef C2<T> Z;
  const int n = d.n, p = d.p;
  const Z zero = mk<T>(0, 0);
#pragma unroll 1
  for (int half = 0; half < nhalf; ++half) {
    const Z* La = half ? Lm : Lj;     // the line's own spectrum / its mirror's
    const Z* Lb = half ? Lj : Lm;
    const int j = half ? j1 : j0, jm = half ? j0 : j1, s = half ? s_mirror : t;
    const T kj = j >= 0 ? kt[j] : (T)0, kjm = jm >= 0 ? kt[jm] : (T)0;
#pragma unroll 1
    for (int fld = 0; fld < 2; ++fld) {
      Z a[F::R];
#pragma unroll
      for (int jj = 0; jj < F::R; ++jj) {
        const int ip = f.mode_index(jj);
        const int i = fl_unpad(ip, n, p), im = fl_unpad((p - ip) % p, n, p);
        // fl_spec() of the mode and of its mirror, but only the two spectra this field needs (the velocities need
        // psihat = omghat ./ k^2, the vorticity gradients do not)
        const bool va = j >= 0 && i >= 0, vm = jm >= 0 && im >= 0;
        Z oa = zero, om_ = zero;
        T ki = 0, kim = 0;
        if (va) { oa = La[i]; ki = kt[i]; }
        if (vm) { om_ = Lb[im]; kim = kt[im]; }
        if (fld == 0) {   // Z1 = Herm(u) + i Herm(v),  u = i ky psi, v = -i kx psi
          // one reciprocal serves the four quotients of the pair (k^2 of a mode and of its mirror are the same number;
          // omghat * (1 / k^2) instead of omghat / k^2: <= 1 ulp from the reference's quotient)
          const T k2 = va ? kj * kj + ki * ki : kjm * kjm + kim * kim;
          const T r = (T)1 / k2;
          const Z pa = (va && !(i == 0 && j == 0)) ? mk<T>(oa.x * r, oa.y * r) : zero;
          const Z pm = (vm && !(im == 0 && jm == 0)) ? mk<T>(om_.x * r, om_.y * r) : zero;
          const Z au = mk<T>(-ki * pa.y, ki * pa.x), av = mk<T>(kj * pa.y, -kj * pa.x);
          const Z mu = mk<T>(-kim * pm.y, kim * pm.x), mv = mk<T>(kjm * pm.y, -kjm * pm.x);
          const Z hu = mk<T>((T)0.5 * (au.x + mu.x), (T)0.5 * (au.y - mu.y)), hv = mk<T>((T)0.5 * (av.x + mv.x), (T)0.5 * (av.y - mv.y));
          a[jj] = mk<T>(hu.x - hv.y, hu.y + hv.x);
        } else {          // Z2 = Herm(wx) + i Herm(wy),  wx = i kx omg, wy = i ky omg
          const Z ax = mk<T>(-kj * oa.y, kj * oa.x), ay = mk<T>(-ki * oa.y, ki * oa.x);
          const Z mx = mk<T>(-kjm * om_.y, kjm * om_.x), my = mk<T>(-kim * om_.y, kim * om_.x);
          const Z hx = mk<T>((T)0.5 * (ax.x + mx.x), (T)0.5 * (ax.y - mx.y)), hy = mk<T>((T)0.5 * (ay.x + my.x), (T)0.5 * (ay.y - my.y));
          a[jj] = mk<T>(hx.x - hy.y, hx.y + hy.x);
        }
      }
      f.inverse(a);
      if (d.wtile) {
        // tile-major: element x of line s goes to tile x / 8, row s, column x % 8 -- 128-byte pieces that are CONTIGUOUS over
        // the lines of a tile (consecutive waves of a workgroup write consecutive rows), so that the x-pass reads whole tiles
        Z* w = W + ((size_t)b * 2 + fld) * d.nl * p + (size_t)s * 8;
#pragma unroll
        for (int jj = 0; jj < F::R; ++jj) {
          const int x = l + F::LANES * jj;
          w[(size_t)(x >> 3) * d.nl * 8 + (x & 7)] = a[jj];
        }
      } else {
        Z* w = W + (((size_t)b * 2 + fld) * d.nl + s) * p;
#pragma unroll
        for (int jj = 0; jj < F::R; ++jj) w[l + F::LANES * jj] = a[jj];
      }
    }
  }
}

// K1w: one wave per PAIR of carried lines (a line and its mirror, see below).  LDS: per wave the two spectrum lines j and mirror(j) (2 n complex).
template <class T, int E, int Q, int LB>
__global__ __launch_bounds__(256) void fluid_k1w_kernel(FluidDev<T> d, const C2<T>* __restrict__ omg,
                                                        C2<T>* __restrict__ W, int pair) {
  typedef WaveFft<T, E, Q, LB> F;
  typedef C2<T> Z;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  // a "line slot" is a wave (LB = 6) or a half wave (LB = 5: two lines per wave); l = position inside the line
  const int lane = threadIdx.x & 63, l = lane & (F::LANES - 1), slot = (threadIdx.x >> 6) * F::LPW + (lane >> LB);
  const int n = d.n, p = d.p;
  Z* Lj = reinterpret_cast<Z*>(smem_raw) + (size_t)slot * 2 * n;
  Z* Lm = Lj + n;
  // the wavenumber table in LDS (round 4): the spectral part reads k of every mode and of its mirror -- 48 dependent global
  // loads per wave item, each with its own wait, in the middle of the fp64 arithmetic
  T* kt = reinterpret_cast<T*>(smem_raw + (size_t)4 * F::LPW * 2 * n * sizeof(Z));
  for (int i = threadIdx.x; i < n; i += 256) kt[i] = d.k[i];
  __syncthreads();
  // work item t = carried line t (jp = t <= n/2) TOGETHER WITH its mirror line (jp' = p - t): both need exactly the
  // spectrum lines j and mirror(j) -- with the roles swapped -- so one load of the two lines serves two output lines
  // (half the reads of omg and half the exposed load latency per transform); line 0 is its own mirror
  // (pair = 0: one carried line per slot, every line loads its two spectrum lines itself -- more, shorter waves: better
  // for the small grids, n = 128: 12.8 vs 15.2 us)
  const int t = blockIdx.x * 4 * F::LPW + slot, b = blockIdx.y;
  if (t >= (pair ? n / 2 + 1 : d.nl)) return;             // whole line slot; no workgroup barrier below this point
  const int jp = fl_line_jp(t, n, p, d.nl), jpm = (p - jp) % p;
  const int s_mirror = fl_line_of(jpm, n, p, d.nl);
  const int j0 = fl_unpad(jp, n, p), j1 = fl_unpad(jpm, n, p);
  // (a literal zero, not a named one: the named object was given a stack slot -- a dead scratch store per wave)
  for (int i = l; i < n; i += F::LANES) {
    Lj[i] = j0 >= 0 ? omg[((size_t)b * n + j0) * n + i] : mk<T>(0, 0);
    Lm[i] = j1 >= 0 ? omg[((size_t)b * n + j1) * n + i] : mk<T>(0, 0);
  }
  __builtin_amdgcn_wave_barrier();
  F f;
  f.init(d.twp, lane);
  const int nhalf = (pair && s_mirror >= 0 && s_mirror != t) ? 2 : 1;
  fluid_k1w_body<T, E, Q, LB>(d, Lj, Lm, j0, j1, t, s_mirror, nhalf, W, b, f, l, kt);
}

// K2w: TC columns per workgroup, one wave per column.  LDS: the [TC][p] column tile (transposition + permuted access).
// TC = 4 keeps the tile at 48 KB so that several workgroups share a CU and one's global loads / stores overlap the
// others' transforms (with TC = 8 a CU holds a single workgroup and load -> transform -> store serialise).
template <class T, int E, int Q, int TC, int LB>
__global__ __launch_bounds__(64 * TC >> (6 - LB)) void fluid_k2w_kernel(FluidDev<T> d, const C2<T>* __restrict__ W,
                                                            C2<T>* __restrict__ W2) {
  typedef WaveFft<T, E, Q, LB> F;
  typedef C2<T> Z;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  Z* tile = reinterpret_cast<Z*>(smem_raw);
  constexpr int NT = 64 * TC / F::LPW;                      // one line slot (wave or half wave) per column
  const int tid = threadIdx.x, lane = tid & 63, wv = (tid >> 6) * F::LPW + (lane >> LB), n = d.n, p = d.p, LS = p + 1;
  const int ip0 = blockIdx.x * TC, b = blockIdx.y;
  F f;
  f.init(d.twp, lane);
  Z r0[F::R], a[F::R];
  // tile element (t, jp) of a field: W[fld][s(jp)][ip0 + t] or 0 (pad() along x); thread-strided over the TC x p tile
  constexpr int NPF = (TC * F::N + NT - 1) / NT;            // tile elements per thread
  auto tile_src = [&](int fld, int idx) -> Z {
    const int t = idx % TC, jp = idx / TC;
    const int s = fl_line_of(jp, n, p, d.nl), ip = ip0 + t;
    if (s >= 0 && ip < p) return W[(((size_t)b * 2 + fld) * d.nl + s) * p + ip];
    return mk<T>(0, 0);
  };
  for (int idx = tid; idx < TC * p; idx += NT) tile[(idx % TC) * LS + idx / TC] = tile_src(0, idx);
  Z pre[NPF];                                               // field 1 is fetched while field 0 is transformed
#pragma unroll
  for (int u = 0; u < NPF; ++u) {
    const int idx = tid + u * NT;
    pre[u] = idx < TC * p ? tile_src(1, idx) : mk<T>(0, 0);
  }
  __syncthreads();
#pragma unroll
  for (int jj = 0; jj < F::R; ++jj) r0[jj] = tile[wv * LS + f.mode_index(jj)];
  f.inverse(r0);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NPF; ++u) {
    const int idx = tid + u * NT;
    if (idx < TC * p) tile[(idx % TC) * LS + idx / TC] = pre[u];
  }
  __syncthreads();
#pragma unroll
  for (int jj = 0; jj < F::R; ++jj) a[jj] = tile[wv * LS + f.mode_index(jj)];
  f.inverse(a);
  // -(u wx + v wy), both ifft scalings; forward transform of the real product (one column per wave)
#pragma unroll
  for (int jj = 0; jj < F::R; ++jj) a[jj] = mk<T>(-(r0[jj].x * a[jj].x + r0[jj].y * a[jj].y) * d.inv2, (T)0);
  f.forward(a);
  __syncthreads();
#pragma unroll
  for (int jj = 0; jj < F::R; ++jj) tile[wv * LS + f.mode_index(jj)] = a[jj];
  __syncthreads();
  for (int idx = tid; idx < TC * n; idx += NT) {        // chop() along x + coalesced store
    const int t = idx % TC, jj = idx / TC, ip = ip0 + t;
    if (ip < p) W2[((size_t)b * n + jj) * p + ip] = tile[t * LS + fl_pad(jj, n, p)];
  }
}

// K2p (round 4): the same x-pass as a PERSISTENT, software-pipelined kernel -- one 8-wave workgroup per CU walks its share of
// the (trajectory, 8-column) tiles; the field tile needed NEXT streams into LDS by LDS-DMA (no VGPR staging) while the waves
// run the line transforms of the current one out of registers.
//   * a tile is TC = 8 columns wide: every global access of W and W2 is a whole 128-byte line (8 complex fp64) -- K2w's TC = 4
//     moves 64-byte half lines -- and only the nl non-zero lines of a column are ever fetched or kept in LDS (pad() is an index map);
//   * LDS: one field region R, [nl rounded up to 8][8] complex (65 KiB at n = 512), an output staging region S, [n][8] (64 KiB), and
//     the radix-Q twiddle table (8 KiB).  A DMA piece (1 KiB per wave instruction) is 8 lines x 8 columns, lane l fetching line
//     8c + (l >> 3), column (l & 7) ^ ((line >> 2) & 7): the column swizzle spreads the 16-byte reads of one wave (lines a
//     multiple of 4 apart in the digit-reversed order the transforms consume) over the banks; S is swizzled the same way;
//   * per tile:  [f0 landed] read column | barrier | DMA f1 -> R | inverse -> r0 | [f1 landed] read column | barrier |
//     DMA f0 of the NEXT tile -> R | inverse -> a | product, forward | column -> S | barrier | 128-byte-line stores of S.
//     f1 has one transform (~5 us) to land, the next f0 two.  Vector-memory operations retire in issue order on vmcnt (loads
//     and stores alike): "f0(next) has landed" = at most the 8 store instructions issued behind its DMA are outstanding; the
//     barriers are raw (s_waitcnt lgkmcnt(0); s_barrier) -- __syncthreads() would drain the prefetch.
//     (First cut: two field regions, outputs stored straight from the transform's registers -- 16-byte pieces of 64 different
//     lines per instruction: 9.4 M partial-line writes per launch cost 23-34 us that no amount of overlap hid.)
// Same arithmetic per column as K2w, in the same order.  W2 is bit-identical to K2w's where the compiler contracts the two kernels'
// multiply-adds alike: measured so in fp64 at n = 256 and 512 and in fp32 at n = 256; NOT in fp32 at n = 512
// (<float,4,3,..>: 392 fused multiply-add lanes in K2w, 398 in K2p), where the right-hand sides differ by 1.6e-7 of max |rhs|
// (2.6 units of 2^-24; tests/test_gpu_fluid_geometry.py holds both to the oracle and the difference to 16 units).
__device__ __forceinline__ void k2p_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int N>
__device__ __forceinline__ void k2p_wait_but() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// K2p's tile geometry for an element of ZB bytes (16: complex double, 8: complex float), in ONE place.  A tile is TC = 8
// columns (one wave per column); a DMA piece is what one 16-byte-per-lane wave instruction moves, 1 KiB: LPL lanes per tile line,
// EPL elements per lane, LPP lines.  fp64: 8 lanes x 1 element, 8 lines; fp32: 4 lanes x 2 adjacent columns, 16 lines.
// The column swizzle acts on the lane slot (a column pair in fp32): slot ^ ((line >> 2) & (LPL - 1)).
template <int ZB>
struct K2pGeom {
  static constexpr int TC = 8, EPL = 16 / ZB, LPL = TC / EPL, LPL_SH = EPL == 1 ? 3 : 2, LPP = 64 / LPL, PIECE = 64 * EPL;   // PIECE: elements
  static __host__ __device__ int npieces(int nl) { return (nl + LPP - 1) / LPP; }
  static __host__ __device__ int npw(int nl) { return (npieces(nl) + 7) / 8; }                    // DMA pieces per wave and field
  static __host__ __device__ int nsu(int n) { return n * TC / 512; }                             // output elements per thread
  // LDS element of (line sl, column col) in the field region
  static __device__ __forceinline__ int at(int sl, int col) {
    return sl * TC + EPL * ((col / EPL) ^ ((sl >> 2) & (LPL - 1))) + col % EPL;
  }
  // vmcnt waits: behind the DMA of the next tile's field 0 a thread issues exactly its NSU output stores (one store instruction
  // per element: the elements of a thread lie 64 rows apart, nothing to merge); nothing is issued behind field 1's DMA
  template <int NSU>
  static constexpr int wait_f0_next() { return NSU; }
};

// NPW: DMA pieces per wave and field (K2pGeom::npw); NSU: output elements per thread (K2pGeom::nsu)
template <class T, int E, int Q, int NPW, int NSU>
__global__ __launch_bounds__(512) void fluid_k2p_kernel(FluidDev<T> d, const C2<T>* __restrict__ W,
                                                        C2<T>* __restrict__ W2, int ntiles) {
  typedef WaveFft<T, E, Q, 6, true> F;    // radix-Q twiddles from an LDS table: the kernel sits near the 256-VGPR limit of 2 waves / SIMD
  typedef C2<T> Z;
  typedef K2pGeom<(int)sizeof(Z)> G;
  constexpr int TC = G::TC;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = d.n, p = d.p, nl = d.nl;
  const int npieces = G::npieces(nl);
  Z* R = reinterpret_cast<Z*>(smem_raw);
  Z* S = R + (size_t)npieces * G::PIECE;  // [n][8]
  Z* WQ = S + (size_t)n * TC;             // [(Q - 1) E][64]
  const int tiles_per_b = p / TC;
  F f;
  f.init(d.twp, lane, WQ, wv == 0);
  __syncthreads();
  // LDS element of (line of the mode in slot jj, my column) or -1 (a pad() zero); recomputed where used (a few integer
  // operations per slot against a 768-point transform) instead of held in registers
  auto src_of = [&](int jj) -> int {
    const int sl = fl_line_of(f.mode_index(jj), n, p, nl);
    return sl >= 0 ? G::at(sl, wv) : -1;
  };
  // the transform's twiddles are ordinary global loads: they must have landed BEFORE the first DMA is issued -- the compiler
  // waits vmcnt(0) at the first use of a global load, which would drain every prefetch in flight behind it
  f.touch();
  auto dma_tile = [&](int fld, int tile) {
    int lv = lane;
    asm volatile("" : "+v"(lv));                         // opaque per call: the offsets below are not hoisted (and spilled)
    const int b = tile / tiles_per_b, ip0 = (tile - b * tiles_per_b) * TC;
    // (W is tile-major for this kernel, FluidDev::wtile: tile ip0 / 8 of a field is the contiguous block [nl][8])
    const char* base = reinterpret_cast<const char*>(W + ((size_t)b * 2 + fld) * nl * p + (size_t)(ip0 >> 3) * nl * 8);      // wave-uniform
#pragma unroll
    for (int j = 0; j < NPW; ++j) {
      // piece c: lines LPP c .. LPP c + LPP - 1; this lane's 16 bytes (recomputed per issue: kept in registers the offsets spill,
      // and a scratch reload is a vector-memory load whose wait drains the DMA queue).  LDS receives the lanes in order, so lane
      // slot s of a line holds the columns of slot s ^ swizzle -- what G::at() reads back.
      int c = wv + 8 * j;
      c = c < npieces ? c : npieces - 1;
      int sl = c * G::LPP + (lv >> G::LPL_SH);
      sl = sl < nl ? sl : nl - 1;                        // rows past nl - 1 of the last piece: never read
      const unsigned off = (unsigned)(sl * TC + G::EPL * ((lv & (G::LPL - 1)) ^ ((sl >> 2) & (G::LPL - 1)))) * (unsigned)sizeof(Z);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + off),
                                       (__attribute__((address_space(3))) void*)(R + (size_t)c * G::PIECE), 16, 0, 0);
    }
  };
  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  dma_tile(0, tile);
  // the pad() zero: a named object in fp64 (the form built and measured there); in fp32 the named one was given a stack slot,
  // and a scratch access is a vector-memory operation whose wait would drain the DMA queue -- a literal there
  [[maybe_unused]] const Z zero = mk<T>(0, 0);
  bool first = true;
  for (; tile < ntiles; tile += gridDim.x) {
    const int next = tile + gridDim.x;
    const bool more = next < ntiles;
    Z r0[F::R], a[F::R];
    // ---- field 0 has landed: behind its DMA only the NSU stores of the previous tile were issued
    if (first) k2p_wait_but<0>(); else k2p_wait_but<G::template wait_f0_next<NSU>()>();
    first = false;
    k2p_lds_barrier();
#pragma unroll
    for (int jj = 0; jj < F::R; ++jj) {
      const int si = src_of(jj);
      if constexpr (sizeof(T) == 8) r0[jj] = si >= 0 ? R[si] : zero;
      else r0[jj] = si >= 0 ? R[si] : mk<T>(0, 0);
    }
    k2p_lds_barrier();                                   // every wave has read field 0
    dma_tile(1, tile);
    f.inverse(r0);
    // ---- field 1 (nothing younger than its DMA is in flight; the stores of the previous tile are older and retire first)
    k2p_wait_but<0>();
    k2p_lds_barrier();
#pragma unroll
    for (int jj = 0; jj < F::R; ++jj) {
      const int si = src_of(jj);
      if constexpr (sizeof(T) == 8) a[jj] = si >= 0 ? R[si] : zero;
      else a[jj] = si >= 0 ? R[si] : mk<T>(0, 0);
    }
    k2p_lds_barrier();                                   // every wave has read field 1
    if (more) dma_tile(0, next);
    f.inverse(a);
    // ---- -(u wx + v wy), both ifft scalings; forward transform of the real product (one column per wave)
#pragma unroll
    for (int jj = 0; jj < F::R; ++jj) a[jj] = mk<T>(-(r0[jj].x * a[jj].x + r0[jj].y * a[jj].y) * d.inv2, (T)0);
    f.forward(a);
    // ---- chop() along x: kept modes of my column into S (S was last read two barriers ago), then whole-line stores.
    // (Round 6, measured: the stores issued in the middle of the NEXT tile by all waves, or at its start by waves 4 - 7 only while
    // their SIMD partners transform, make the launch 7 - 14 us LONGER -- HISTORY.md 6.5.)
#pragma unroll
    for (int jj = 0; jj < F::R; ++jj) {
      const int kk = fl_unpad(f.mode_index(jj), n, p);
      if (kk >= 0) S[kk * TC + (wv ^ ((kk >> 2) & 7))] = a[jj];
    }
    k2p_lds_barrier();
    const int b = tile / tiles_per_b, ip0 = (tile - b * tiles_per_b) * TC;
    Z* out = W2 + (size_t)b * n * p + ip0;
#pragma unroll
    for (int u = 0; u < NSU; ++u) {
      const int idx = tid + 512 * u, kk = idx >> 3, col = idx & 7;
      out[(size_t)kk * p + col] = S[kk * TC + (col ^ ((kk >> 2) & 7))];
    }
  }
}

// K3w: one wave per kept line j.  LDS: per wave one n-complex line (digit-reversed -> natural for coalesced global access).
template <class T, int E, int Q, int LB>
__global__ __launch_bounds__(256) void fluid_k3w_kernel(FluidDev<T> d, const C2<T>* __restrict__ W2,
                                                        const C2<T>* omg_s, const C2<T>* __restrict__ phat,
                                                        const C2<T>* f0, C2<T>* acc, C2<T>* out, int mode,
                                                        T ca, T cb) {
  typedef WaveFft<T, E, Q, LB> F;
  typedef C2<T> Z;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63, l = lane & (F::LANES - 1), slot = (threadIdx.x >> 6) * F::LPW + (lane >> LB);
  const int n = d.n, p = d.p;
  Z* Ln = reinterpret_cast<Z*>(smem_raw) + (size_t)slot * n;
  const int j = blockIdx.x * 4 * F::LPW + slot, b = blockIdx.y;
  if (j >= n) return;
  F f;
  f.init(d.twp, lane);
  Z a[F::R];
  const Z* w2 = W2 + ((size_t)b * n + j) * p;
#pragma unroll
  for (int jj = 0; jj < F::R; ++jj) a[jj] = w2[l + F::LANES * jj];
  f.forward(a);
#pragma unroll
  for (int jj = 0; jj < F::R; ++jj) {
    const int i = fl_unpad(f.mode_index(jj), n, p);          // chop() along y
    if (i >= 0) Ln[i] = a[jj];
  }
  __builtin_amdgcn_wave_barrier();
  const T kj = d.k[j];
  for (int i = l; i < n; i += F::LANES) {
    const size_t off = ((size_t)b * n + j) * n + i;
    const T ki = d.k[i], lin = -d.nu * (kj * kj + ki * ki);
    const Z o = omg_s[off], nlv = Ln[i], ph = phat[off];
    const Z k = mk<T>(lin * o.x + d.scale_out * nlv.x + ph.x, lin * o.y + d.scale_out * nlv.y + ph.y);
    if (mode == 0) {
      out[off] = k;
    } else if (mode == 4) {
      const Z ac = acc[off];
      out[off] = mk<T>(ac.x + cb * k.x, ac.y + cb * k.y);
    } else {
      const Z fv = f0[off];
      out[off] = mk<T>(fv.x + ca * k.x, fv.y + ca * k.y);
      if (mode == 1) acc[off] = mk<T>(fv.x + cb * k.x, fv.y + cb * k.y);
      else {
        const Z ac = acc[off];
        acc[off] = mk<T>(ac.x + cb * k.x, ac.y + cb * k.y);
      }
    }
  }
}

// K31w = K3w of one RK4 stage fused with K1w of the NEXT right-hand side (src/fluid_rk4.jl:122-190 inside rk4, :192-229):
// the stage value K3 writes for a kept line j is exactly the spectrum line K1 reads next, and K1 of a line pair (t, mirror)
// needs only the lines j0, j1 of that pair -- so a wave finishes the stage for its two lines (forward transform along y of
// W2, chop, linear term + forcing, stage update; `out` / `acc` to HBM as K3w does), keeps the two new spectrum lines in
// LDS and runs the K1w body from there.  Saves the re-read of the stage value (4 MB per trajectory and RHS at n = 512)
// and one launch per RHS.  mode 1 / 2 / 4 as in K3w (mode 0, the bare RHS, has no successor).  Pair items only (n >= 256).
template <class T, int E, int Q, int LB>
__global__ __launch_bounds__(256) void fluid_k31w_kernel(FluidDev<T> d, const C2<T>* __restrict__ W2,
                                                         const C2<T>* omg_s, const C2<T>* __restrict__ phat,
                                                         const C2<T>* f0, C2<T>* acc, C2<T>* out, int mode,
                                                         T ca, T cb, C2<T>* __restrict__ W) {
  typedef WaveFft<T, E, Q, LB> F;
  typedef C2<T> Z;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63, l = lane & (F::LANES - 1), slot = (threadIdx.x >> 6) * F::LPW + (lane >> LB);
  const int n = d.n, p = d.p;
  Z* Lj = reinterpret_cast<Z*>(smem_raw) + (size_t)slot * 2 * n;
  Z* Lm = Lj + n;
  const int t = blockIdx.x * 4 * F::LPW + slot, b = blockIdx.y;
  if (t > n / 2) return;
  const int jp = fl_line_jp(t, n, p, d.nl), jpm = (p - jp) % p;
  const int s_mirror = fl_line_of(jpm, n, p, d.nl);
  const int j0 = fl_unpad(jp, n, p), j1 = fl_unpad(jpm, n, p);
  const Z zero = mk<T>(0, 0);
  F f;
  f.init(d.twp, lane);
  // ---- K3 for the kept lines j0 and (if it is another line) j1
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    const int j = h ? j1 : j0;
    Z* Ln = h ? Lm : Lj;
    if (h && (j1 < 0 || j1 == j0)) {
      if (j1 < 0)                                   // the mirror of the Nyquist line lies in the padding: zero spectrum
        for (int i = l; i < n; i += F::LANES) Ln[i] = zero;
      break;
    }
    Z a[F::R];
    const Z* w2 = W2 + ((size_t)b * n + j) * p;
#pragma unroll
    for (int jj = 0; jj < F::R; ++jj) a[jj] = w2[l + F::LANES * jj];
    f.forward(a);
#pragma unroll
    for (int jj = 0; jj < F::R; ++jj) {
      const int i = fl_unpad(f.mode_index(jj), n, p);          // chop() along y
      if (i >= 0) Ln[i] = a[jj];
    }
    __builtin_amdgcn_wave_barrier();
    const T kj = d.k[j];
    for (int i = l; i < n; i += F::LANES) {
      const size_t off = ((size_t)b * n + j) * n + i;
      const T ki = d.k[i], lin = -d.nu * (kj * kj + ki * ki);
      const Z o = omg_s[off], nlv = Ln[i], ph = phat[off];
      const Z k = mk<T>(lin * o.x + d.scale_out * nlv.x + ph.x, lin * o.y + d.scale_out * nlv.y + ph.y);
      Z nv;
      if (mode == 4) {
        const Z ac = acc[off];
        nv = mk<T>(ac.x + cb * k.x, ac.y + cb * k.y);
      } else {
        const Z fv = f0[off];
        nv = mk<T>(fv.x + ca * k.x, fv.y + ca * k.y);
        if (mode == 1) acc[off] = mk<T>(fv.x + cb * k.x, fv.y + cb * k.y);
        else {
          const Z ac = acc[off];
          acc[off] = mk<T>(ac.x + cb * k.x, ac.y + cb * k.y);
        }
      }
      out[off] = nv;
      Ln[i] = nv;                                   // the spectrum line of the next right-hand side
    }
  }
  __builtin_amdgcn_wave_barrier();
  // ---- K1 of the next right-hand side from the two lines
  const Z* Lmm = (j1 == j0) ? Lj : Lm;              // line 0 is its own mirror
  const int nhalf = (s_mirror >= 0 && s_mirror != t) ? 2 : 1;
  fluid_k1w_body<T, E, Q, LB>(d, Lj, Lmm, j0, j1, t, s_mirror, nhalf, W, b, f, l, d.k);
}

// ------------------------------------------------------------------ wave FFT unit-test entry (pdec_debug_wave_fft)
template <class T, int E, int Q, int LB>
__global__ __launch_bounds__(256) void wave_fft_debug_kernel(const C2<T>* __restrict__ in, C2<T>* __restrict__ out,
                                                            const C2<T>* __restrict__ tw, int nlines, int sgn) {
  typedef WaveFft<T, E, Q, LB> F;
  const int lane = threadIdx.x & 63, l = lane & (F::LANES - 1);
  const int line = (blockIdx.x * 4 + (threadIdx.x >> 6)) * F::LPW + (lane >> LB);
  if (line >= nlines) return;
  F f;
  f.init(tw, lane);
  C2<T> a[F::R];
  const C2<T>* x = in + (size_t)line * F::N;
  C2<T>* y = out + (size_t)line * F::N;
  if (sgn < 0) {
#pragma unroll
    for (int j = 0; j < F::R; ++j) a[j] = x[l + F::LANES * j];
    f.forward(a);
#pragma unroll
    for (int j = 0; j < F::R; ++j) y[f.mode_index(j)] = a[j];
  } else {
#pragma unroll
    for (int j = 0; j < F::R; ++j) a[j] = x[f.mode_index(j)];
    f.inverse(a);
#pragma unroll
    for (int j = 0; j < F::R; ++j) y[l + F::LANES * j] = a[j];
  }
}

// ------------------------------------------------------------------ host side
template <class K>
static int wave_lds_limit(K kern) {
  PDEC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return PDEC_OK;
}

// the dynamic-LDS limit of the three kernels of an un-fused right-hand side: once per instantiation, for the rhs launcher and
// the fused integrator alike (K2p and K31w set theirs where they alone are launched)
template <class T, int E, int Q, int LB>
static int fluid_wave_attrs() {
  static bool attr = false;
  if (attr) return PDEC_OK;
  int rc;
  if ((rc = wave_lds_limit(fluid_k1w_kernel<T, E, Q, LB>))) return rc;
  if ((rc = wave_lds_limit(fluid_k2w_kernel<T, E, Q, FL_K2_TC, LB>))) return rc;
  if ((rc = wave_lds_limit(fluid_k3w_kernel<T, E, Q, LB>))) return rc;
  attr = true;
  return PDEC_OK;
}

// the persistent x-pass as one instantiation builds it: NPW DMA pieces per wave, NSU output elements per thread
#ifndef FL_K2P_WPC32
#define FL_K2P_WPC32 2      // fp32 K2p: at most this many workgroups per CU, where registers and LDS allow (fp64: one, 134 KB of LDS)
#endif
template <class T, int E, int Q, int NPW, int NSU>
static int fluid_k2p_launch(FluidEnv& Ev, const FluidDev<T>& d) {
  typedef C2<T> Z;
  typedef K2pGeom<(int)sizeof(Z)> G;
  const int ntiles = Ev.cfg.B * (Ev.p / 8);
  const size_t lds = ((size_t)G::npieces(Ev.nl) * G::PIECE + (size_t)Ev.n * G::TC + (size_t)(Q > 1 ? (Q - 1) * E : 1) * 64) * sizeof(Z);
  static bool attr = false;
  static int ncu = 256, wpc = 1;
  if (!attr) {
    int dev = 0, rc;
    hipDeviceProp_t pr;
    PDEC_HIP(hipGetDevice(&dev));
    PDEC_HIP(hipGetDeviceProperties(&pr, dev));
    if (pr.multiProcessorCount > 0) ncu = pr.multiProcessorCount;
    if ((rc = wave_lds_limit(fluid_k2p_kernel<T, E, Q, NPW, NSU>))) return rc;
    if (!std::is_same<T, double>::value) {   // fp32: as many resident workgroups per CU as registers and LDS allow, <= 2
      int nb = 1;
      PDEC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fluid_k2p_kernel<T, E, Q, NPW, NSU>, 512, lds));
      wpc = nb < 1 ? 1 : (nb < FL_K2P_WPC32 ? nb : FL_K2P_WPC32);
    }
    attr = true;
  }
  const int grid = ntiles < ncu * wpc ? ntiles : ncu * wpc;
  hipLaunchKernelGGL((fluid_k2p_kernel<T, E, Q, NPW, NSU>), dim3(grid), dim3(512), lds, Ev.stream, d, Ev.W.as<Z>(), Ev.W2.as<Z>(),
                     ntiles);
  return PDEC_OK;
}

// K2 of the wave path: the persistent pipelined form (fluid_k2p_kernel) where k2p_eligible found it in the environment's row of
// the plan table -- then K1 wrote W tile-major, d.wtile -- else the tile form.  PDEC_FLUID_K2P=0 / 1 forces the choice.
template <class T, int E, int Q, int LB>
static int fluid_k2_launch(FluidEnv& Ev, const FluidDev<T>& d) {
  typedef C2<T> Z;
  const int B = Ev.cfg.B, p = Ev.p;
  constexpr int LPW = 64 >> LB, TC = FL_K2_TC;   // (fp32 too: measured 8 columns, 131 -> 4 columns, 152-156 env-steps/s at C5's shape)
  if (d.wtile) return Ev.wave->fns<T>().k2p(Ev, d);
  hipLaunchKernelGGL((fluid_k2w_kernel<T, E, Q, TC, LB>), dim3((p + TC - 1) / TC, B), dim3(64 * TC / LPW),
                     (size_t)TC * (p + 1) * sizeof(Z), Ev.stream, d, Ev.W.as<Z>(), Ev.W2.as<Z>());
  return PDEC_OK;
}

// one rhs evaluation fused with an RK4 stage update (mode as in fluid_k3_kernel)
template <class T, int E, int Q, int LB>
static int fluid_rhs_launch_wave(FluidEnv& Ev, const FluidDev<T>& d, const void* omg_s, const void* phat, const void* f0,
                                 void* acc, void* out, int mode, double ca, double cb) {
  typedef C2<T> Z;
  const int B = Ev.cfg.B, n = Ev.n;
  constexpr int LPW = 64 >> LB, LPB = 4 * LPW;               // line slots per wave / per 256-thread workgroup
  int rc;
  if ((rc = fluid_wave_attrs<T, E, Q, LB>())) return rc;
  const int pair = n >= 256 ? 1 : 0;      // a line and its mirror per wave (K1w) once there are enough lines to fill the chip
  {
    ProfScope ps(&Ev, "fluid_k1", true);
    for (int r = 0; r < ps.reps; ++r)
      hipLaunchKernelGGL((fluid_k1w_kernel<T, E, Q, LB>), dim3(((pair ? n / 2 + 1 : Ev.nl) + LPB - 1) / LPB, B), dim3(256),
                         (size_t)LPB * 2 * n * sizeof(Z) + (size_t)n * sizeof(T), Ev.stream, d, (const Z*)omg_s, Ev.W.as<Z>(), pair);
  }
  {
    ProfScope ps(&Ev, "fluid_k2", true);
    for (int r = 0; r < ps.reps; ++r)
      if ((rc = fluid_k2_launch<T, E, Q, LB>(Ev, d))) return rc;
  }
  {
    ProfScope ps(&Ev, "fluid_k3", mode == 0);
    for (int r = 0; r < ps.reps; ++r)
      hipLaunchKernelGGL((fluid_k3w_kernel<T, E, Q, LB>), dim3((n + LPB - 1) / LPB, B), dim3(256), (size_t)LPB * n * sizeof(Z), Ev.stream, d,
                         Ev.W2.as<Z>(), (const Z*)omg_s, (const Z*)phat, (const Z*)f0, (Z*)acc, (Z*)out, mode, (T)ca, (T)cb);
  }
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

// do_step (FluidSetup.jl:163-172): K sub-steps of rk4 (src/fluid_rk4.jl:122-132), in place on f
// RK4 sub-steps with K3 of every stage fused with K1 of the next right-hand side (fluid_k31w_kernel): K1 once, then
// K2 + K31 per stage, a plain K3 at the very end.  Wave-transform path with line pairs (n >= 256).
template <class T, int E, int Q, int LB>
static int fluid_integrate_wave(FluidEnv& Ev, const FluidDev<T>& d, void* f, const void* phat) {
  typedef C2<T> Z;
  const int B = Ev.cfg.B, n = Ev.n;
  constexpr int LPW = 64 >> LB, LPB = 4 * LPW;
  static bool attr = false;
  if (!attr) {
    int rc;
    if ((rc = fluid_wave_attrs<T, E, Q, LB>())) return rc;
    if ((rc = wave_lds_limit(fluid_k31w_kernel<T, E, Q, LB>))) return rc;
    attr = true;
  }
  const double h = Ev.cfg.dt / Ev.cfg.K;
  Z *fs = Ev.fs.as<Z>(), *acc = Ev.acc.as<Z>(), *fz = (Z*)f;
  const dim3 gpair((n / 2 + 1 + LPB - 1) / LPB, B);
  const size_t lds2 = (size_t)LPB * 2 * n * sizeof(Z);
  auto k2 = [&]() {
    ProfScope ps(&Ev, "fluid_k2");
    (void)fluid_k2_launch<T, E, Q, LB>(Ev, d);
  };
  auto k31 = [&](const Z* omg_s, Z* out, int mode, double ca, double cb) {
    ProfScope ps(&Ev, "fluid_k31");
    hipLaunchKernelGGL((fluid_k31w_kernel<T, E, Q, LB>), gpair, dim3(256), lds2, Ev.stream, d, Ev.W2.as<Z>(), omg_s, (const Z*)phat,
                       (const Z*)fz, acc, out, mode, (T)ca, (T)cb, Ev.W.as<Z>());
  };
  {
    ProfScope ps(&Ev, "fluid_k1");
    hipLaunchKernelGGL((fluid_k1w_kernel<T, E, Q, LB>), gpair, dim3(256), lds2 + (size_t)n * sizeof(T), Ev.stream, d, (const Z*)fz, Ev.W.as<Z>(), 1);
  }
  for (int it = 0; it < Ev.cfg.K; ++it) {
    k2(); k31(fz, fs, 1, 0.5 * h, h / 6.0);
    k2(); k31(fs, fs, 2, 0.5 * h, h / 3.0);
    k2(); k31(fs, fs, 2, h, h / 3.0);
    k2();
    if (it + 1 < Ev.cfg.K) {
      k31(fs, fz, 4, 0.0, h / 6.0);
    } else {
      ProfScope ps(&Ev, "fluid_k3");
      hipLaunchKernelGGL((fluid_k3w_kernel<T, E, Q, LB>), dim3((n + LPB - 1) / LPB, B), dim3(256), (size_t)LPB * n * sizeof(Z), Ev.stream, d,
                         Ev.W2.as<Z>(), (const Z*)fs, (const Z*)phat, (const Z*)fz, acc, fz, 4, (T)0, (T)(h / 6.0));
    }
  }
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

template <class T, int E, int Q, int LB>
static void wave_fft_debug_launch(const void* in, void* out, const void* tw, int nlines, int sgn) {
  constexpr int LPB = 4 * (64 >> LB);
  hipLaunchKernelGGL((wave_fft_debug_kernel<T, E, Q, LB>), dim3((nlines + LPB - 1) / LPB), dim3(256), 0, 0, (const C2<T>*)in,
                     (C2<T>*)out, (const C2<T>*)tw, nlines, sgn);
}

// ------------------------------------------------------------------ the table of wave plans
// The only place that names an (E, Q, LB) triple: one row per padded length, and what a row does not name is not built.
//  * the un-fused right-hand side, K2w and the debug kernel: every row;
//  * the fused integrator with K31w: the one-line-per-wave rows from p = 256 -- it works on line pairs, n >= 256, and p >= n;
//  * the persistent x-pass: needs ifpad, so p = 3 n / 2 with n a multiple of 64 -- n = 512 and n = 256 --, each with the one
//    (NPW, NSU) pair per dtype that K2pGeom gives for it (nl = n + 1; k2p_eligible compares).
// A host table: nothing on the device reads it, and only the host pass emits it.
template <class T, int E, int Q, int LB, int NPW, int NSU>
constexpr FluidWaveFns<T> wave_fns() {
  constexpr int p = WaveFft<T, E, Q, LB>::N;
  FluidWaveFns<T> f{};
  f.rhs = fluid_rhs_launch_wave<T, E, Q, LB>;
  if constexpr (LB == 6 && p >= 256) f.integrate = fluid_integrate_wave<T, E, Q, LB>;
  if constexpr (NPW != 0) {
    static_assert(LB == 6 && p % 8 == 0, "fluid_k2p_kernel: one line per wave, 8-column tiles");
    f.k2p = fluid_k2p_launch<T, E, Q, NPW, NSU>;
    f.k2p_npw = NPW;
    f.k2p_nsu = NSU;
  }
  f.debug = wave_fft_debug_launch<T, E, Q, LB>;
  return f;
}
template <int P, int E, int Q, int LB, int NPW64 = 0, int NPW32 = 0, int NSU = 0>
constexpr FluidWavePlan wave_row() {
  static_assert(WaveFft<double, E, Q, LB>::N == P && WaveFft<float, E, Q, LB>::N == P, "the plan transforms lines of another length");
  return {P, E, Q, LB, wave_fns<double, E, Q, LB, NPW64, NSU>(), wave_fns<float, E, Q, LB, NPW32, NSU>()};
}
static const FluidWavePlan fluid_wave_table[] = {
    //        p  E  Q  LB  K2p: NPW fp64, fp32, NSU
    wave_row<768, 4, 3, 6, 9, 5, 8>(),
    wave_row<512, 4, 2, 6>(),
    wave_row<256, 4, 1, 6>(),
    wave_row<384, 2, 3, 6, 5, 3, 4>(),
    wave_row<128, 2, 1, 6>(),
    wave_row<192, 2, 3, 5>(),      // the reference's 128^2 training grid, padded
    wave_row<64, 2, 1, 5>(),
};

const FluidWavePlan* fluid_wave_plan(int p) {
  for (const FluidWavePlan& r : fluid_wave_table)
    if (r.p == p) return &r;
  return nullptr;
}

// does the persistent x-pass (fluid_k2p_kernel) serve this environment?  Decided once: K1 writes W in the layout K2 reads.
bool k2p_eligible(const FluidEnv& E) {
  static const char* env = getenv("PDEC_FLUID_K2P");
  const bool want = env ? env[0] == '1' : E.n >= 256;
  if (!(want && E.wave && E.p % 8 == 0 && E.cfg.ifpad && E.n * 8 % 512 == 0)) return false;
  // built: the row has the instantiation of this geometry's DMA pieces per wave and output elements per thread
  return fluid_by_dtype(E, [&](auto t) {
    typedef decltype(t) T;
    typedef K2pGeom<(int)sizeof(C2<T>)> G;
    const FluidWaveFns<T>& f = E.wave->fns<T>();
    return f.k2p && f.k2p_npw == G::npw(E.nl) && f.k2p_nsu == G::nsu(E.n);
  });
}

}  // namespace pdec

using namespace pdec;

// Unit-test entries for the register-resident wave FFT (wave_fft.hpp): nlines lines of `len` complex doubles
// (pdec_debug_wave_fft) or complex floats (pdec_debug_wave_fft_f32), natural order in and out, unnormalised forward (sgn < 0)
// or inverse (sgn > 0).  len: a padded length of fluid_wave_table.  Twiddles computed in fp64, rounded once.
template <class T>
static int debug_wave_fft(const char* name, const void* in_dev, void* out_dev, int len, int nlines, int sgn) {
  PDEC_REQUIRE(in_dev && out_dev && nlines >= 1, "%s: null/empty", name);
  const FluidWavePlan* plan = fluid_wave_plan(len);
  if (!plan) { set_error("%s: unsupported length %d", name, len); return PDEC_E_INVALID; }
  std::vector<double> tw(2 * (size_t)len);
  for (int m = 0; m < len; ++m) { tw[2 * m] = cos(2 * M_PI * m / len); tw[2 * m + 1] = -sin(2 * M_PI * m / len); }
  DevBuf d;
  int rc = upload_converted(d, tw.data(), tw.size(), std::is_same<T, float>::value ? PDEC_F32 : PDEC_F64);
  if (rc) return rc;
  plan->fns<T>().debug(in_dev, out_dev, d.p, nlines, sgn);
  PDEC_HIP(hipGetLastError());
  PDEC_HIP(hipDeviceSynchronize());
  return PDEC_OK;
}
extern "C" int pdec_debug_wave_fft(const void* in_dev, void* out_dev, int len, int nlines, int sgn) {
  return debug_wave_fft<double>("pdec_debug_wave_fft", in_dev, out_dev, len, nlines, sgn);
}
extern "C" int pdec_debug_wave_fft_f32(const void* in_dev, void* out_dev, int len, int nlines, int sgn) {
  return debug_wave_fft<float>("pdec_debug_wave_fft_f32", in_dev, out_dev, len, nlines, sgn);
}

// Unit-test entry: the plan table as the host code reads it (no device, no handle); see include/pdeconv_debug.h
extern "C" int pdec_debug_fluid_wave_table(int32_t* out, int cap, int* nrows) {
  PDEC_REQUIRE(nrows, "pdec_debug_fluid_wave_table: null nrows");
  constexpr int NR = (int)(sizeof(fluid_wave_table) / sizeof(fluid_wave_table[0])), PER = 14;
  *nrows = NR;
  PDEC_REQUIRE(out && cap >= NR * PER, "pdec_debug_fluid_wave_table: out holds %d numbers, the table has %d", out ? cap : 0, NR * PER);
  for (const FluidWavePlan& r : fluid_wave_table) {
    const int32_t row[PER] = {r.p, r.E, r.Q, r.LB,
                              r.f64.rhs != nullptr, r.f64.integrate != nullptr, r.f64.k2p != nullptr, r.f64.k2p_npw, r.f64.k2p_nsu,
                              r.f32.rhs != nullptr, r.f32.integrate != nullptr, r.f32.k2p != nullptr, r.f32.k2p_npw, r.f32.k2p_nsu};
    for (int i = 0; i < PER; ++i) *out++ = row[i];
  }
  return PDEC_OK;
}
