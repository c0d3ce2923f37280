// ks_engines.hpp -- the FFT engines of the spectral KS kernels (ks_step.hip, ks_rollout.hip) and the ONE list of them
// (with_ks_engine): a kernel takes its engine as a template parameter, the host picks it by Env::engine
#pragma once
#include "env.hpp"

namespace pdec {

// ------------------------------------------------------------------ KS CNAB2 kernel
#define KS_MPT 4  // modes / cells owned per thread: k = tid + j*nt

// FFT engines: transform the 4 values a thread owns (indices tid + j*nt) in place.
// Generic engine: mixed-radix Stockham through LDS (any N = 2^a 3^b 5^c).
template <class T>
struct FftGeneric {
  static constexpr int kThreads = 1024;     // largest workgroup the host launches this engine with
  C2<T>*X, *Y;
  const C2<T>* tw;
  FftPlan pl;
  int N, tid, nt;
  __device__ __forceinline__ void init(unsigned char* smem, const EnvDev<T>& e, int tid_, int nt_) {
    N = e.N; tid = tid_; nt = nt_; pl = e.fft;
    X = reinterpret_cast<C2<T>*>(smem);
    Y = X + N;
    C2<T>* t = Y + N;
    for (int k = tid; k < N; k += nt) t[k] = e.tw[k];
    tw = t;
  }
  static __host__ __device__ size_t lds_complex(int N) { return 3 * (size_t)N; }
  // wave-space mode held in slot j after a forward transform (natural order for this engine)
  __device__ __forceinline__ int mode_index(int j) const { return tid + j * nt; }
  // cell held in slot j in physical space
  __device__ __forceinline__ int phys_index(int j) const { return tid + j * nt; }
  template <int SGN>
  __device__ __forceinline__ void run(C2<T> (&a)[KS_MPT]) {
#pragma unroll
    for (int j = 0; j < KS_MPT; ++j) {
      const int k = tid + j * nt;
      if (k < N) X[k] = a[j];
    }
    C2<T>* R = fft_lds<SGN, T>(X, Y, tw, pl, tid, nt);
#pragma unroll
    for (int j = 0; j < KS_MPT; ++j) {
      const int k = tid + j * nt;
      if (k < N) a[j] = R[k];
    }
    __syncthreads();
  }
  // natural-order complex image of the last result for the sensing stage
  __device__ __forceinline__ C2<T>* publish(const C2<T> (&a)[KS_MPT]) {
#pragma unroll
    for (int j = 0; j < KS_MPT; ++j) {
      const int k = tid + j * nt;
      if (k < N) X[k] = a[j];
    }
    __syncthreads();
    return X;
  }
};

// Radix-4 engine for N = 4^L with nt = N/4 threads: in the Stockham DIF form every stage of
// thread t reads x[t + (N/4) j] -- its own registers for the first stage and conflict-free LDS
// rows afterwards -- and the last stage lands back on the owned indices, so a transform costs
// L-1 LDS round trips and L-1 barriers; all twiddles are per-thread constants held in registers.
template <class T, int L>
struct FftR4 {
  C2<T>* buf[2];
  C2<T> w[L - 1][3];
  int tid, par;
  static constexpr int N = 1 << (2 * L), NT = N / 4;
  static constexpr int kThreads = (NT + 63) / 64 * 64;
  __device__ __forceinline__ void init(unsigned char* smem, const EnvDev<T>& e, int tid_, int) {
    tid = tid_; par = 0;
    buf[0] = reinterpret_cast<C2<T>*>(smem);
    buf[1] = buf[0] + N;
#pragma unroll
    for (int st = 0; st < L - 1; ++st) {
      const int s = 1 << (2 * st);
      const int base = tid & ~(s - 1);          // p*s
#pragma unroll
      for (int k = 1; k < 4; ++k) w[st][k - 1] = e.tw[base * k];
    }
  }
  static __host__ __device__ size_t lds_complex(int) { return 2 * (size_t)N; }
  __device__ __forceinline__ int mode_index(int j) const { return tid + j * NT; }
  __device__ __forceinline__ int phys_index(int j) const { return tid + j * NT; }
  template <int SGN>
  __device__ __forceinline__ void run(C2<T> (&a)[KS_MPT]) {
#pragma unroll
    for (int st = 0; st < L; ++st) {
      if (st > 0) {
        const C2<T>* in = buf[par ^ ((st - 1) & 1)];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = in[tid + NT * j];
      }
      dft_small<4, SGN, T>(a);
      if (st < L - 1) {
        const int s = 1 << (2 * st);
        const int q = tid & (s - 1);
        const int ob = q + 4 * (tid - q);       // q + 4 s p
        C2<T>* out = buf[par ^ (st & 1)];
        out[ob] = a[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
          C2<T> tw = w[st][k - 1];
          if (SGN > 0) tw.y = -tw.y;
          out[ob + s * k] = cmul(a[k], tw);
        }
        __syncthreads();
      }
    }
    if ((L - 1) & 1) par ^= 1;                  // next transform starts on the buffer not read last
  }
  __device__ __forceinline__ C2<T>* publish(const C2<T> (&a)[KS_MPT]) {
    __syncthreads();
    C2<T>* X = buf[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) X[tid + NT * j] = a[j];
    __syncthreads();
    return X;
  }
};

// ---- register-resident single-wave engine for N = 256 (64 lanes x 4 points): NO LDS traffic.
// In-place radix-4 decimation in frequency: stage st transforms the index digit that currently lives in
// the register index, then that digit is exchanged with one 2-bit digit of the lane id -- lane bits 5:4 by
// v_permlane32_swap / v_permlane16_swap, bits 3:2 by bank-masked DPP row shifts, bits 1:0 by DPP quad
// permutes -- so the next stage again works on the 4 registers of a lane.  The forward transform leaves mode
// k = (lane>>4) + 4((lane>>2)&3) + 16(lane&3) + 64 j in slot j (digit-reversed); the inverse runs the same
// steps backwards and returns to the natural order n = lane + 64 j.  The CNAB2 update is pointwise in wave
// space, so the permuted order only changes which per-mode constants a lane loads (mode_index).
// Besides being shorter, the transform does not queue behind other kernels' LDS traffic when the PDE step
// shares CUs with the MFMA update passes (measured: the LDS engine slowed 46 -> 140 us there).
__device__ __forceinline__ void lane_swap32(unsigned& a, unsigned& b) {   // a[lanes 32-63] <-> b[lanes 0-31]
  auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = r[0]; b = r[1];
}
__device__ __forceinline__ void lane_swap16(unsigned& a, unsigned& b) {   // odd 16-lane rows of a <-> even rows of b
  auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
  a = r[0]; b = r[1];
}
#define PDEC_DPP(old, src, ctrl, bank) (unsigned)__builtin_amdgcn_update_dpp((int)(old), (int)(src), ctrl, 0xF, bank, false)
// exchange the register index (0..3) with lane bits 5:4
__device__ __forceinline__ void xch_rows(unsigned (&v)[4]) {
  lane_swap32(v[0], v[2]); lane_swap32(v[1], v[3]);
  lane_swap16(v[0], v[1]); lane_swap16(v[2], v[3]);
}
// ... with lane bits 3:2 (row_ror:8 = lane^8; row_shr:4 / row_shl:4 = lane-4 / lane+4 inside a 16-lane row)
__device__ __forceinline__ void xch_mid(unsigned (&v)[4]) {
  unsigned t;
  t = v[0]; v[0] = PDEC_DPP(v[0], v[2], 0x128, 0xC); v[2] = PDEC_DPP(v[2], t, 0x128, 0x3);
  t = v[1]; v[1] = PDEC_DPP(v[1], v[3], 0x128, 0xC); v[3] = PDEC_DPP(v[3], t, 0x128, 0x3);
  t = v[0]; v[0] = PDEC_DPP(v[0], v[1], 0x114, 0xA); v[1] = PDEC_DPP(v[1], t, 0x104, 0x5);
  t = v[2]; v[2] = PDEC_DPP(v[2], v[3], 0x114, 0xA); v[3] = PDEC_DPP(v[3], t, 0x104, 0x5);
}
// ... with lane bits 1:0 (quad_perm [2,3,0,1] = lane^2, [1,0,3,2] = lane^1)
__device__ __forceinline__ void xch_low(unsigned (&v)[4], bool b1, bool b0) {
  unsigned s, t;
  s = PDEC_DPP(0, v[2], 0x4E, 0xF); t = PDEC_DPP(0, v[0], 0x4E, 0xF); v[0] = b1 ? s : v[0]; v[2] = b1 ? v[2] : t;
  s = PDEC_DPP(0, v[3], 0x4E, 0xF); t = PDEC_DPP(0, v[1], 0x4E, 0xF); v[1] = b1 ? s : v[1]; v[3] = b1 ? v[3] : t;
  s = PDEC_DPP(0, v[1], 0xB1, 0xF); t = PDEC_DPP(0, v[0], 0xB1, 0xF); v[0] = b0 ? s : v[0]; v[1] = b0 ? v[1] : t;
  s = PDEC_DPP(0, v[3], 0xB1, 0xF); t = PDEC_DPP(0, v[2], 0xB1, 0xF); v[2] = b0 ? s : v[2]; v[3] = b0 ? v[3] : t;
}
// apply an exchange to every 32-bit word of the 4 complex values a lane holds
template <int WHICH, class T>
__device__ __forceinline__ void xch_complex(C2<T> (&a)[4], bool b1, bool b0) {
  constexpr int W = sizeof(T) / 4;      // words per real
  unsigned w[2 * W][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned tmp[2 * W];
    __builtin_memcpy(tmp, &a[j], sizeof(C2<T>));
#pragma unroll
    for (int c = 0; c < 2 * W; ++c) w[c][j] = tmp[c];
  }
#pragma unroll
  for (int c = 0; c < 2 * W; ++c) {
    if (WHICH == 2) xch_rows(w[c]);
    else if (WHICH == 1) xch_mid(w[c]);
    else xch_low(w[c], b1, b0);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned tmp[2 * W];
#pragma unroll
    for (int c = 0; c < 2 * W; ++c) tmp[c] = w[c][j];
    __builtin_memcpy(&a[j], tmp, sizeof(C2<T>));
  }
}

// ---- fp32 fast path: the same exchanges written in place (inline asm), one instruction per moved word.
// One binary step of a digit exchange on register pairs (P_k, Q_k), k = 0..3 (two components x two pairs):
//   newQ = bit ? Q : perm(P),  newP = bit ? perm(Q) : P        (bit = the lane-id bit being exchanged)
// as v_cndmask_b32_dpp (DPP permutes src0; VCC = lane mask of the bit, then its complement).  The builtin form
// above costs ~2.5x the instructions in register copies and separate selects.
#define PDEC_XSTEP(CA, CB, MASK, P0, Q0, P1, Q1, P2, Q2, P3, Q3)                                           \
  {                                                                                                        \
    float n0_, n1_, n2_, n3_;                                                                              \
    asm("s_nop 1\n\t"                                                                                      \
        "s_mov_b64 vcc, %12\n\t"                                                                           \
        "v_cndmask_b32_dpp %8, %0, %1, vcc " CA " row_mask:0xf bank_mask:0xf\n\t"                           \
        "v_cndmask_b32_dpp %9, %2, %3, vcc " CA " row_mask:0xf bank_mask:0xf\n\t"                           \
        "v_cndmask_b32_dpp %10, %4, %5, vcc " CA " row_mask:0xf bank_mask:0xf\n\t"                          \
        "v_cndmask_b32_dpp %11, %6, %7, vcc " CA " row_mask:0xf bank_mask:0xf\n\t"                          \
        "s_mov_b64 vcc, %13\n\t"                                                                           \
        "v_cndmask_b32_dpp %0, %1, %0, vcc " CB " row_mask:0xf bank_mask:0xf\n\t"                           \
        "v_cndmask_b32_dpp %2, %3, %2, vcc " CB " row_mask:0xf bank_mask:0xf\n\t"                           \
        "v_cndmask_b32_dpp %4, %5, %4, vcc " CB " row_mask:0xf bank_mask:0xf\n\t"                           \
        "v_cndmask_b32_dpp %6, %7, %6, vcc " CB " row_mask:0xf bank_mask:0xf"                                \
        : "+v"(P0), "+v"(Q0), "+v"(P1), "+v"(Q1), "+v"(P2), "+v"(Q2), "+v"(P3), "+v"(Q3), "=&v"(n0_), "=&v"(n1_), \
          "=&v"(n2_), "=&v"(n3_)                                                                           \
        : "s"(MASK), "s"(~(MASK))                                                                          \
        : "vcc");                                                                                          \
    Q0 = n0_; Q1 = n1_; Q2 = n2_; Q3 = n3_;                                                                \
  }
// digit = lane bits 3:2 (WHICH 1) or 1:0 (WHICH 0); bits 5:4 (WHICH 2) use the permlane swaps
template <int WHICH>
__device__ __forceinline__ void xch_complex_f32(C2<float> (&a)[4]) {
  if (WHICH == 2) {
    asm("s_nop 1\n\t"
        "v_permlane32_swap_b32 %0, %2\n\t"
        "v_permlane32_swap_b32 %4, %6\n\t"
        "v_permlane32_swap_b32 %1, %3\n\t"
        "v_permlane32_swap_b32 %5, %7\n\t"
        "s_nop 1\n\t"
        "v_permlane16_swap_b32 %0, %1\n\t"
        "v_permlane16_swap_b32 %4, %5\n\t"
        "v_permlane16_swap_b32 %2, %3\n\t"
        "v_permlane16_swap_b32 %6, %7"
        : "+v"(a[0].x), "+v"(a[1].x), "+v"(a[2].x), "+v"(a[3].x), "+v"(a[0].y), "+v"(a[1].y), "+v"(a[2].y), "+v"(a[3].y));
  } else if (WHICH == 1) {
    // bit 3 (lane ^ 8 = row_ror:8), register pairs (0,2), (1,3)
    PDEC_XSTEP("row_ror:8", "row_ror:8", 0xFF00FF00FF00FF00ull, a[0].x, a[2].x, a[1].x, a[3].x, a[0].y, a[2].y, a[1].y, a[3].y)
    // bit 2: lanes with the bit clear read lane + 4 (row_ror:12), lanes with it set read lane - 4 (row_ror:4); pairs (0,1), (2,3)
    PDEC_XSTEP("row_ror:12", "row_ror:4", 0xF0F0F0F0F0F0F0F0ull, a[0].x, a[1].x, a[2].x, a[3].x, a[0].y, a[1].y, a[2].y, a[3].y)
  } else {
    PDEC_XSTEP("quad_perm:[2,3,0,1]", "quad_perm:[2,3,0,1]", 0xCCCCCCCCCCCCCCCCull, a[0].x, a[2].x, a[1].x, a[3].x, a[0].y, a[2].y,
               a[1].y, a[3].y)
    PDEC_XSTEP("quad_perm:[1,0,3,2]", "quad_perm:[1,0,3,2]", 0xAAAAAAAAAAAAAAAAull, a[0].x, a[1].x, a[2].x, a[3].x, a[0].y, a[1].y,
               a[2].y, a[3].y)
  }
}

// ---- fp32 packed-math butterflies: VOP3P op_sel / neg modifiers give the multiplication by +-i and the complex
// product without any register shuffling (the compiler scalarises these and adds ~60 moves per transform).
typedef float pkf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pkf2 pk_add_mi(pkf2 a, pkf2 b) {   // a + (-i) b = (a.x + b.y, a.y - b.x)
  pkf2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ pkf2 pk_add_pi(pkf2 a, pkf2 b) {   // a + i b = (a.x - b.y, a.y + b.x)
  pkf2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
template <int SGN>   // a * w (SGN < 0) or a * conj(w) (SGN > 0)
__device__ __forceinline__ pkf2 pk_cmul(pkf2 a, pkf2 w) {
  pkf2 t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "v"(w));                 // (a.x w.x, a.y w.x)
  if (SGN < 0)   // (t.x - a.y w.y, t.y + a.x w.y)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(a), "v"(w), "v"(t));
  else           // (t.x + a.y w.y, t.y - a.x w.y)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[0,1,0]" : "=v"(r) : "v"(a), "v"(w), "v"(t));
  return r;
}
template <int SGN>
__device__ __forceinline__ void pk_dft4(C2<float> (&a)[4]) {
  pkf2 v0 = __builtin_bit_cast(pkf2, a[0]), v1 = __builtin_bit_cast(pkf2, a[1]), v2 = __builtin_bit_cast(pkf2, a[2]),
       v3 = __builtin_bit_cast(pkf2, a[3]);
  const pkf2 s02 = v0 + v2, d02 = v0 - v2, s13 = v1 + v3, d13 = v1 - v3;
  v0 = s02 + s13;
  v2 = s02 - s13;
  v1 = SGN < 0 ? pk_add_mi(d02, d13) : pk_add_pi(d02, d13);   // d02 + (-+i) d13
  v3 = SGN < 0 ? pk_add_pi(d02, d13) : pk_add_mi(d02, d13);   // d02 - (-+i) d13
  a[0] = __builtin_bit_cast(C2<float>, v0); a[1] = __builtin_bit_cast(C2<float>, v1);
  a[2] = __builtin_bit_cast(C2<float>, v2); a[3] = __builtin_bit_cast(C2<float>, v3);
}

template <class T>
struct FftWave256 {
  static constexpr int kThreads = 64;
  C2<T>* buf;
  C2<T> w[3][3];       // twiddles of the three inner stages, per lane
  int tid;
  bool b1, b0;
  static constexpr int N = 256, NT = 64;
  __device__ __forceinline__ void init(unsigned char* smem, const EnvDev<T>& e, int tid_, int) {
    tid = tid_;
    b1 = (tid & 2) != 0; b0 = (tid & 1) != 0;
    buf = reinterpret_cast<C2<T>*>(smem);
    const int low[3] = {tid, 4 * (tid & 15), 16 * (tid & 3)};   // k * (index formed by the digits still to transform)
#pragma unroll
    for (int st = 0; st < 3; ++st)
#pragma unroll
      for (int k = 1; k < 4; ++k) w[st][k - 1] = e.tw[(k * low[st]) & 255];
  }
  static __host__ __device__ size_t lds_complex(int) { return (size_t)N; }   // only for publish()
  __device__ __forceinline__ int mode_index(int j) const {
    return (tid >> 4) + 4 * ((tid >> 2) & 3) + 16 * (tid & 3) + 64 * j;
  }
  __device__ __forceinline__ int phys_index(int j) const { return tid + NT * j; }
  template <int ST>
  __device__ __forceinline__ void exchange(C2<T> (&a)[4]) {
    if constexpr (sizeof(T) == 4) {
      xch_complex_f32<2 - ST>(reinterpret_cast<C2<float>(&)[4]>(a));
    } else {
      if (ST == 0) xch_complex<2, T>(a, b1, b0);
      else if (ST == 1) xch_complex<1, T>(a, b1, b0);
      else xch_complex<0, T>(a, b1, b0);
    }
  }
  template <int ST, int SGN>
  __device__ __forceinline__ void twiddle(C2<T> (&a)[4]) {
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if constexpr (sizeof(T) == 4) {
        a[k] = __builtin_bit_cast(C2<T>, pk_cmul<SGN>(__builtin_bit_cast(pkf2, a[k]), __builtin_bit_cast(pkf2, w[ST][k - 1])));
      } else {
        C2<T> tw = w[ST][k - 1];
        if (SGN > 0) tw.y = -tw.y;
        a[k] = cmul(a[k], tw);
      }
    }
  }
  template <int SGN>
  __device__ __forceinline__ void dft4(C2<T> (&a)[4]) {
    if constexpr (sizeof(T) == 4) pk_dft4<SGN>(reinterpret_cast<C2<float>(&)[4]>(a));
    else dft_small<4, SGN, T>(a);
  }
  template <int SGN>
  __device__ __forceinline__ void run(C2<T> (&a)[KS_MPT]) {
    if (SGN < 0) {   // forward: natural -> digit-reversed
      dft4<-1>(a); twiddle<0, -1>(a); exchange<0>(a);
      dft4<-1>(a); twiddle<1, -1>(a); exchange<1>(a);
      dft4<-1>(a); twiddle<2, -1>(a); exchange<2>(a);
      dft4<-1>(a);
    } else {         // inverse: digit-reversed -> natural (unnormalised)
      dft4<+1>(a);
      exchange<2>(a); twiddle<2, +1>(a); dft4<+1>(a);
      exchange<1>(a); twiddle<1, +1>(a); dft4<+1>(a);
      exchange<0>(a); twiddle<0, +1>(a); dft4<+1>(a);
    }
  }
  __device__ __forceinline__ C2<T>* publish(const C2<T> (&a)[KS_MPT]) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) buf[tid + NT * j] = a[j];
    __syncthreads();
    return buf;
  }
};

// ---- N = 256 over TWO waves (fp32; the fused step beside the update passes, pdec_env_set_two_wave_step): 128 lanes x 2 points,
// bit for bit the one-wave engine on 0.6 of its vector instructions per wave.  Every radix-4 DIF butterfly of FftWave256 is
// run as its two radix-2 levels -- level 1 over the high bit of the digit (s02, d02 | s13, d13), level 2 over the low bit with
// the inner -+i as a swap and a negation of d13 in the lanes that hold the d pair -- and the twiddles multiply where they
// multiply there, so every element sees the same floating-point operations in the same order.  Between two levels the ONE
// register bit is exchanged with one bit of the thread id: bits 5 and 4 by v_permlane32/16_swap, bits 3..0 by the DPP select
// steps of PDEC_XSTEP on one register pair, the wave bit through LDS (1 KB per exchange, two halves alternating, one raw
// barrier).  Index bits, forward: thread tid owns n = tid + 128 r (r: register); at the end wave = k0 & 1, lane bits
// 5..0 = k0 >> 1, k1 & 1, k1 >> 1, k2 & 1, k2 >> 1, k3 & 1 and r = k3 >> 1 of mode k0 + 4 k1 + 16 k2 + 64 k3.
__device__ __forceinline__ void wave_pair_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#define PDEC_XSTEP2(CA, CB, MASK, P0, Q0, P1, Q1)                                                          \
  {                                                                                                        \
    float n0_, n1_;                                                                                        \
    asm("s_nop 1\n\t"                                                                                      \
        "s_mov_b64 vcc, %6\n\t"                                                                            \
        "v_cndmask_b32_dpp %4, %0, %1, vcc " CA " row_mask:0xf bank_mask:0xf\n\t"                           \
        "v_cndmask_b32_dpp %5, %2, %3, vcc " CA " row_mask:0xf bank_mask:0xf\n\t"                           \
        "s_mov_b64 vcc, %7\n\t"                                                                            \
        "v_cndmask_b32_dpp %0, %1, %0, vcc " CB " row_mask:0xf bank_mask:0xf\n\t"                           \
        "v_cndmask_b32_dpp %2, %3, %2, vcc " CB " row_mask:0xf bank_mask:0xf"                                \
        : "+v"(P0), "+v"(Q0), "+v"(P1), "+v"(Q1), "=&v"(n0_), "=&v"(n1_)                                   \
        : "s"(MASK), "s"(~(MASK))                                                                          \
        : "vcc");                                                                                          \
    Q0 = n0_; Q1 = n1_;                                                                                    \
  }
// a * w (SGN < 0) or a * conj(w) (SGN > 0) in the lanes of `mask`, a in the others: pk_cmul's two instructions under EXEC
template <int SGN>
__device__ __forceinline__ pkf2 pk_cmul_lanes(pkf2 a, pkf2 w, unsigned long long mask) {
  pkf2 t;
  unsigned long long sv;
  if (SGN < 0)
    asm("s_and_saveexec_b64 %2, %4\n\t"
        "v_pk_mul_f32 %1, %0, %3 op_sel_hi:[1,0]\n\t"
        "v_pk_fma_f32 %0, %0, %3, %1 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]\n\t"
        "s_mov_b64 exec, %2"
        : "+v"(a), "=&v"(t), "=&s"(sv) : "v"(w), "s"(mask) : "scc");
  else
    asm("s_and_saveexec_b64 %2, %4\n\t"
        "v_pk_mul_f32 %1, %0, %3 op_sel_hi:[1,0]\n\t"
        "v_pk_fma_f32 %0, %0, %3, %1 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[0,1,0]\n\t"
        "s_mov_b64 exec, %2"
        : "+v"(a), "=&v"(t), "=&s"(sv) : "v"(w), "s"(mask) : "scc");
  return a;
}

struct FftWave256x2 {
  static constexpr int kThreads = 128;
  static constexpr int kMpt = 2;            // points per lane (the kernels' KS_MPT for this engine)
  static constexpr int kSumThreads = 64;    // the step's sums (sensor dots, reward partial) keep the one-wave engine's tree: wave 0 does them
  static constexpr int N = 256, NT = 128;
  C2<float>* buf;      // [2][128]: the halves of the cross-wave exchange; [256]: publish()
  pkf2 w0[3], w1[3];   // twiddles of the three inner stages for register 0 (digit k = kl; unused where kl = 0) and 1 (k = kl + 2)
  int tid, lane, wv, par;
  __device__ __forceinline__ void init(unsigned char* smem, const EnvDev<float>& e, int tid_, int) {
    tid = tid_; lane = tid & 63; par = 0;
    wv = __builtin_amdgcn_readfirstlane(tid >> 6);     // uniform: the wave's own branches are scalar
    buf = reinterpret_cast<C2<float>*>(smem);
    const int kl[3] = {wv, (lane >> 4) & 1, (lane >> 2) & 1};               // low bit of the stage's output digit
    const int low[3] = {lane, 4 * (lane & 15), 16 * (lane & 3)};            // as in FftWave256
#pragma unroll
    for (int st = 0; st < 3; ++st) {
      w0[st] = __builtin_bit_cast(pkf2, e.tw[(kl[st] * low[st]) & 255]);
      w1[st] = __builtin_bit_cast(pkf2, e.tw[((kl[st] + 2) * low[st]) & 255]);
    }
  }
  static __host__ __device__ size_t lds_complex(int) { return (size_t)N; }
  __device__ __forceinline__ int mode_index(int j) const {
    const int k0 = wv + 2 * (lane >> 5), k1 = ((lane >> 4) & 1) + 2 * ((lane >> 3) & 1);
    const int k2 = ((lane >> 2) & 1) + 2 * ((lane >> 1) & 1), k3 = (lane & 1) + 2 * j;
    return k0 + 4 * k1 + 16 * k2 + 64 * k3;
  }
  __device__ __forceinline__ int phys_index(int j) const { return tid + NT * j; }

  // level 1 of a radix-4 butterfly: (v0, v2) -> (s02, d02) or (v1, v3) -> (s13, d13)
  static __device__ __forceinline__ void level1(C2<float> (&a)[2]) {
    const pkf2 p = __builtin_bit_cast(pkf2, a[0]), q = __builtin_bit_cast(pkf2, a[1]);
    a[0] = __builtin_bit_cast(C2<float>, p + q);
    a[1] = __builtin_bit_cast(C2<float>, p - q);
  }
  // level 2 in lanes: (s02, s13) -> (v0, v2) where d is clear, (d02, d13) -> (v1, v3) = d02 +- (-+i) d13 where it is set
  template <int SGN>
  static __device__ __forceinline__ void level2(C2<float> (&a)[2], bool d) {
    const C2<float> b = a[1];
    pkf2 r;
    if (SGN < 0) { r.x = d ? b.y : b.x; r.y = d ? -b.x : b.y; }      // -i b = (b.y, -b.x)
    else { r.x = d ? -b.y : b.x; r.y = d ? b.x : b.y; }              // +i b = (-b.y, b.x)
    const pkf2 p = __builtin_bit_cast(pkf2, a[0]);
    a[0] = __builtin_bit_cast(C2<float>, p + r);
    a[1] = __builtin_bit_cast(C2<float>, p - r);
  }
  // level 2 where the wave bit says which pair a wave holds (wave 1: the d pair)
  template <int SGN>
  __device__ __forceinline__ void level2_wave(C2<float> (&a)[2]) const {
    const pkf2 p = __builtin_bit_cast(pkf2, a[0]), q = __builtin_bit_cast(pkf2, a[1]);
    if (wv) {
      a[0] = __builtin_bit_cast(C2<float>, SGN < 0 ? pk_add_mi(p, q) : pk_add_pi(p, q));
      a[1] = __builtin_bit_cast(C2<float>, SGN < 0 ? pk_add_pi(p, q) : pk_add_mi(p, q));
    } else {
      a[0] = __builtin_bit_cast(C2<float>, p + q);
      a[1] = __builtin_bit_cast(C2<float>, p - q);
    }
  }
  // twiddles of stage ST: register 1 always (digit 2 or 3), register 0 where the digit's low bit is set (digit 1)
  template <int ST, int SGN>
  __device__ __forceinline__ void twiddle(C2<float> (&a)[2]) const {
    a[1] = __builtin_bit_cast(C2<float>, pk_cmul<SGN>(__builtin_bit_cast(pkf2, a[1]), w1[ST]));
    if (ST == 0) {
      if (wv) a[0] = __builtin_bit_cast(C2<float>, pk_cmul<SGN>(__builtin_bit_cast(pkf2, a[0]), w0[0]));
    } else {
      a[0] = __builtin_bit_cast(C2<float>, pk_cmul_lanes<SGN>(__builtin_bit_cast(pkf2, a[0]), w0[ST],
                                                              ST == 1 ? 0xFFFF0000FFFF0000ull : 0xF0F0F0F0F0F0F0F0ull));
    }
  }
  // exchange the register bit with lane bit BIT
  template <int BIT>
  static __device__ __forceinline__ void xch(C2<float> (&a)[2]) {
    if (BIT == 5) {
      asm("s_nop 1\n\t"
          "v_permlane32_swap_b32 %0, %2\n\t"
          "v_permlane32_swap_b32 %1, %3"
          : "+v"(a[0].x), "+v"(a[0].y), "+v"(a[1].x), "+v"(a[1].y));
    } else if (BIT == 4) {
      asm("s_nop 1\n\t"
          "v_permlane16_swap_b32 %0, %2\n\t"
          "v_permlane16_swap_b32 %1, %3"
          : "+v"(a[0].x), "+v"(a[0].y), "+v"(a[1].x), "+v"(a[1].y));
    } else if (BIT == 3) {
      PDEC_XSTEP2("row_ror:8", "row_ror:8", 0xFF00FF00FF00FF00ull, a[0].x, a[1].x, a[0].y, a[1].y)
    } else if (BIT == 2) {
      PDEC_XSTEP2("row_ror:12", "row_ror:4", 0xF0F0F0F0F0F0F0F0ull, a[0].x, a[1].x, a[0].y, a[1].y)
    } else if (BIT == 1) {
      PDEC_XSTEP2("quad_perm:[2,3,0,1]", "quad_perm:[2,3,0,1]", 0xCCCCCCCCCCCCCCCCull, a[0].x, a[1].x, a[0].y, a[1].y)
    } else {
      PDEC_XSTEP2("quad_perm:[1,0,3,2]", "quad_perm:[1,0,3,2]", 0xAAAAAAAAAAAAAAAAull, a[0].x, a[1].x, a[0].y, a[1].y)
    }
  }
  // ... with the wave bit: wave 0 hands its register 1 to wave 1's register 0 and takes that one.  The halves alternate, so
  // the writes of the next exchange need no second barrier (the one after it lies behind this one's reads)
  __device__ __forceinline__ void xch_wave(C2<float> (&a)[2]) {
    C2<float>* X = buf + 128 * par;
    par ^= 1;
    if (wv) X[tid] = a[0]; else X[tid] = a[1];
    wave_pair_barrier();
    if (wv) a[0] = X[tid ^ 64]; else a[1] = X[tid ^ 64];
  }
  template <int SGN>
  __device__ __forceinline__ void run(C2<float> (&a)[2]) {
    const bool d4 = (lane & 16) != 0, d2 = (lane & 4) != 0, d0 = (lane & 1) != 0;
    if (SGN < 0) {   // forward: natural -> digit-reversed
      level1(a); xch_wave(a); level2_wave<-1>(a); twiddle<0, -1>(a);
      xch<5>(a); level1(a); xch<4>(a); level2<-1>(a, d4); twiddle<1, -1>(a);
      xch<3>(a); level1(a); xch<2>(a); level2<-1>(a, d2); twiddle<2, -1>(a);
      xch<1>(a); level1(a); xch<0>(a); level2<-1>(a, d0);
    } else {         // inverse: digit-reversed -> natural (unnormalised)
      level1(a); xch<0>(a); level2<+1>(a, d0);
      xch<1>(a); twiddle<2, +1>(a); level1(a); xch<2>(a); level2<+1>(a, d2);
      xch<3>(a); twiddle<1, +1>(a); level1(a); xch<4>(a); level2<+1>(a, d4);
      xch<5>(a); twiddle<0, +1>(a); level1(a); xch_wave(a); level2_wave<+1>(a);
    }
  }
  __device__ __forceinline__ C2<float>* publish(const C2<float> (&a)[2]) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) buf[tid + NT * j] = a[j];
    __syncthreads();
    return buf;
  }
};

// ---- N = 1024 (BASELINE configs[2]) on four waves: ONE cross-wave radix-4 stage + the single-wave 256-point engine (round 4).
// Thread tid of 256 owns x[tid + 256 j], j = 0..3 -- exactly the inputs of the first radix-4 DIF butterfly.  After that
// butterfly and its twiddle W_1024^(tid k2), slot k2 holds element n1 = tid of the length-256 sub-sequence k2; one LDS round
// trip hands sub-sequence w to wave w as element lane + 64 j in slot j, and the wave transforms it in registers (FftWave256:
// lane-digit exchanges by permlane swaps / DPP, no LDS, no barrier).  A transform therefore costs ONE LDS round trip and ONE
// workgroup barrier where the Stockham engine FftR4<5> needs four of each; the two buffers alternate so the next
// transform's writes need no second barrier.  Forward leaves mode k = w + 4 (perm(lane) + 64 j) in slot j of wave w (the CNAB2
// update is pointwise in wave space: only the per-mode constant loads are permuted); the inverse runs the steps backwards
// and returns to the natural order.
template <class T>
struct FftWave1024 {
  static constexpr int kThreads = 256;
  static constexpr int N = 1024, NT = 256;
  FftWave256<T> core;
  C2<T>* buf[2];
  C2<T> wx[3];          // W_1024^(tid k), k = 1..3
  int tid, lane, wv, par;
  __device__ __forceinline__ void init(unsigned char* smem, const EnvDev<T>& e, int tid_, int) {
    tid = tid_; lane = tid & 63; wv = tid >> 6; par = 0;
    buf[0] = reinterpret_cast<C2<T>*>(smem);
    buf[1] = buf[0] + N;
    core.tid = lane;
    core.b1 = (lane & 2) != 0; core.b0 = (lane & 1) != 0;
    core.buf = buf[0];
    const int low[3] = {lane, 4 * (lane & 15), 16 * (lane & 3)};
#pragma unroll
    for (int st = 0; st < 3; ++st)
#pragma unroll
      for (int k = 1; k < 4; ++k) core.w[st][k - 1] = e.tw[(4 * k * low[st]) & 1023];      // W_256^x = W_1024^(4x)
#pragma unroll
    for (int k = 1; k < 4; ++k) wx[k - 1] = e.tw[(k * tid) & 1023];
  }
  static __host__ __device__ size_t lds_complex(int) { return 2 * (size_t)N; }
  __device__ __forceinline__ int mode_index(int j) const {
    return wv + 4 * ((lane >> 4) + 4 * ((lane >> 2) & 3) + 16 * (lane & 3) + 64 * j);
  }
  __device__ __forceinline__ int phys_index(int j) const { return tid + NT * j; }
  template <int SGN>
  __device__ __forceinline__ void run(C2<T> (&a)[KS_MPT]) {
    C2<T>* X = buf[par];
    par ^= 1;
    if (SGN < 0) {   // forward: natural -> (wave, digit-reversed)
      core.template dft4<-1>(a);
#pragma unroll
      for (int k = 1; k < 4; ++k) a[k] = cmul(a[k], wx[k - 1]);
#pragma unroll
      for (int k = 0; k < 4; ++k) X[k * 256 + tid] = a[k];
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = X[wv * 256 + lane + 64 * j];
      core.template run<-1>(a);
    } else {         // inverse (unnormalised)
      core.template run<+1>(a);
#pragma unroll
      for (int j = 0; j < 4; ++j) X[wv * 256 + lane + 64 * j] = a[j];
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = X[k * 256 + tid];
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        C2<T> tw = wx[k - 1];
        tw.y = -tw.y;
        a[k] = cmul(a[k], tw);
      }
      core.template dft4<+1>(a);
    }
  }
  __device__ __forceinline__ C2<T>* publish(const C2<T> (&a)[KS_MPT]) {
    __syncthreads();
    C2<T>* X = buf[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) X[tid + NT * j] = a[j];
    __syncthreads();
    return X;
  }
};

// Compile-time mixed-radix engine for the reference's own grid sizes (KS22: 192 = 4.4.3.4, KS200: 240 = 4.5.3.4,
// KS500: 600 = 4.5.5.2.3).  Stockham stages like FftGeneric, but (i) every radix, stride and index split is a template
// constant (no runtime plan walk, divisions by constants, fully unrolled), and (ii) the plan has radices <= 4 at both
// ends: in PHYSICAL space thread t owns the cells t + (N/R_first) j -- exactly the inputs of its first-stage butterfly
// -- and in WAVE space the modes t + (N/R_last) k -- the outputs of its last-stage butterfly; the inverse runs the plan
// backwards, so it consumes the wave-space layout and lands on the physical one.  A transform therefore costs L-1 LDS
// round trips (the generic engine: L+2) and one butterfly per thread and stage.  A single wave per trajectory pair has
// nothing to hide latency behind, so dependent round trips and instruction count ARE the step time at these sizes.
template <class T, int N_, int L_, int R0, int R1, int R2, int R3, int R4>
struct FftFixed {
  static constexpr int N = N_, L = L_;
  C2<T>* buf[2];
  const C2<T>* tw;
  int tid;
  static constexpr int rad(int i) { return i == 0 ? R0 : (i == 1 ? R1 : (i == 2 ? R2 : (i == 3 ? R3 : R4))); }
  static constexpr int M0 = N / R0, ML = N / rad(L - 1);
  static constexpr int max_m(int i) { return i >= L ? 0 : (N / rad(i) > max_m(i + 1) ? N / rad(i) : max_m(i + 1)); }
  static constexpr int kThreads = (max_m(0) + 63) / 64 * 64;
  __device__ __forceinline__ void init(unsigned char* smem, const EnvDev<T>& e, int tid_, int nt) {
    tid = tid_;
    buf[0] = reinterpret_cast<C2<T>*>(smem);
    buf[1] = buf[0] + N;
    C2<T>* t = buf[1] + N;
    for (int k = tid; k < N; k += nt) t[k] = e.tw[k];
    tw = t;
  }
  static __host__ __device__ size_t lds_complex(int) { return 3 * (size_t)N; }
  __device__ __forceinline__ int mode_index(int j) const { return (tid < ML && j < rad(L - 1)) ? tid + j * ML : N; }
  __device__ __forceinline__ int phys_index(int j) const { return (tid < M0 && j < R0) ? tid + j * M0 : N; }

  // one Stockham stage of radix R on sub-length NN with stride S; FIRST: inputs are the caller's registers,
  // LAST: outputs stay in registers
  template <int R, int SGN, bool FIRST, bool LAST, int NN, int S>
  __device__ __forceinline__ void stage(C2<T> (&a)[KS_MPT], const C2<T>* __restrict__ X, C2<T>* __restrict__ Y) {
    constexpr int m = NN / R, nb = N / R;
    if (tid < nb) {
      const int p = tid / S, q = tid - p * S;
      C2<T> b[R];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        if (FIRST) b[j] = a[j < KS_MPT ? j : 0];
        else b[j] = X[q + S * (p + m * j)];
      }
      C2<T> w[R];
      const int ps = p * S;
      if (!LAST) {
#pragma unroll
        for (int k = 1; k < R; ++k) w[k] = tw[ps * k];
      }
      dft_small<R, SGN, T>(b);
      const int base = q + S * R * p;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        C2<T> v = b[k];
        if (!LAST && k > 0) {
          C2<T> ww = w[k];
          if (SGN > 0) ww.y = -ww.y;
          v = cmul(v, ww);
        }
        if (LAST) a[k < KS_MPT ? k : 0] = v;
        else Y[base + S * k] = v;
      }
    }
  }
  // stage I of the (forward or reversed) plan, sub-length and stride accumulated at compile time
  template <int SGN, int I, int NN, int S>
  __device__ __forceinline__ void walk(C2<T> (&a)[KS_MPT]) {
    if constexpr (I < L) {
      constexpr int R = rad(SGN < 0 ? I : L - 1 - I);
      constexpr bool FIRST = I == 0, LAST = I == L - 1;
      // stage I reads what stage I-1 wrote: buffers alternate, stage 0 writes buf[0]
      stage<R, SGN, FIRST, LAST, NN, S>(a, buf[(I + 1) & 1], buf[I & 1]);
      if (!LAST) __syncthreads();
      walk<SGN, I + 1, NN / R, S * R>(a);
    }
  }
  template <int SGN>
  __device__ __forceinline__ void run(C2<T> (&a)[KS_MPT]) {
    walk<SGN, 0, N, 1>(a);
    __syncthreads();      // the last stage's readers are done before the next transform writes buf[0] again
  }
  __device__ __forceinline__ C2<T>* publish(const C2<T> (&a)[KS_MPT]) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KS_MPT; ++j) {
      const int k = phys_index(j);
      if (k < N) buf[0][k] = a[j];
    }
    __syncthreads();
    return buf[0];
  }
};
template <class T> using FftFixed192 = FftFixed<T, 192, 4, 4, 4, 3, 4, 1>;
template <class T> using FftFixed240 = FftFixed<T, 240, 4, 4, 5, 3, 4, 1>;
template <class T> using FftFixed600 = FftFixed<T, 600, 5, 4, 5, 5, 2, 3>;

// modes / cells per thread of an engine (KS_MPT unless it says otherwise) and the threads that do the step's sums (0: all)
template <class ENG, class = void> struct KsMpt { static constexpr int value = KS_MPT; };
template <class ENG> struct KsMpt<ENG, std::void_t<decltype(ENG::kMpt)>> { static constexpr int value = ENG::kMpt; };
template <class ENG, class = void> struct KsSumThreads { static constexpr int value = 0; };
template <class ENG> struct KsSumThreads<ENG, std::void_t<decltype(ENG::kSumThreads)>> { static constexpr int value = ENG::kSumThreads; };

// ---- the list of engines: calls f with a tag that names the engine type of `k` at precision T (tag.kind: the enumerator,
// decltype(tag)::type: the engine).  Every launch ladder, the LDS footprint (ENG::lds_complex) and the workgroup sizes
// (ENG::kThreads) go through here; guard with `if constexpr` on the tag where only some engines have an instantiation.
// STEP: the list of ks_step.hip, which alone has the two-wave form of the N = 256 step (fp32)
template <KsEngine K, class ENG> struct KsEngineTag { static constexpr KsEngine kind = K; using type = ENG; };
template <class T, bool STEP = false, class F>
auto with_ks_engine(KsEngine k, F&& f) {
  if constexpr (STEP && sizeof(T) == 4)
    if (k == KsEngine::Wave256x2) return f(KsEngineTag<KsEngine::Wave256x2, FftWave256x2>{});
  switch (k) {
    case KsEngine::Wave256: return f(KsEngineTag<KsEngine::Wave256, FftWave256<T>>{});
    case KsEngine::Wave1024: return f(KsEngineTag<KsEngine::Wave1024, FftWave1024<T>>{});
    case KsEngine::LdsR4_256: return f(KsEngineTag<KsEngine::LdsR4_256, FftR4<T, 4>>{});
    case KsEngine::LdsR4_1024: return f(KsEngineTag<KsEngine::LdsR4_1024, FftR4<T, 5>>{});
    case KsEngine::Fixed192: return f(KsEngineTag<KsEngine::Fixed192, FftFixed192<T>>{});
    case KsEngine::Fixed240: return f(KsEngineTag<KsEngine::Fixed240, FftFixed240<T>>{});
    case KsEngine::Fixed600: return f(KsEngineTag<KsEngine::Fixed600, FftFixed600<T>>{});
    default: return f(KsEngineTag<KsEngine::Generic, FftGeneric<T>>{});
  }
}

}  // namespace pdec
