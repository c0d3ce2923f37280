// small2.hpp -- the small DDPG update for 2-layer nets (the reference's `drop_middle_layer = true` shape, src/PDEagent.jl:30-41):
// one THREAD per hidden unit.
// A thread keeps its unit's weights (first-layer row, bias, output weight), their ADAM moments and the target copies in
// REGISTERS for all `loops` updates; forward, backward, ADAM and Polyak of a unit are thread-local, and only the
// output-layer sums cross threads (DPP inside a wave, one LDS exchange + one barrier across waves).  Three barriers
// per update instead of ~35, no weight traffic at all between the first load and the final write-back.
#pragma once
#include "small2_blocks.hpp"

namespace pdec {

// EXACT: ns == KA and Bu == BUT are compile-time constants (the shipped experiments: (1,3) KS, (12,3) Keller-Segel,
// (9,3) fluid), so every column / input-row guard folds away; otherwise KA / BUT are upper bounds checked at run time
// OS > 0: the ADAM state of the actor's per-unit parameters lives ONE PARAMETER PER (lane, slot) of wave 0 -- flat parameter f in
// lane f % 64, slot f / 64, OS slots -- instead of ns + 2 parameters per unit thread: the actor's update is then OS fp64 ADAM chains
// per update (5 for the Keller-Segel actor's 280 parameters) where the 20 unit threads ran 14 one after the other while every other
// wave waited.  Gradients reach their owners and the new weights (and targets) their units through LDS, inside the wave (LDS
// operations of one wave execute in order: no barrier).  Same arithmetic per parameter.  Needs nA <= 64, (ns + 2) nA <= 64 OS.
template <int KC, int KA, int BUT, bool EXACT, int OS = 0>
__global__ __launch_bounds__(512) void ddpg_small2_kernel(Small2Args a_m) {
  Small2Args a_in = a_m;
  if (a_in.g.pm && !sm_member_begin<EXACT>(a_in.g)) return;
  const SmallArgs& g = a_in.g;
  extern __shared__ __align__(16) float sm[];
  const int tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
  if (sm_halted(g, tid)) return;
  const int Bu = EXACT ? BUT : g.Bu, ns = EXACT ? KA : g.ns, K0 = ns + 1, nC = a_in.nC, nA = a_in.nA;
  const bool isC = tid < nC, isA = tid < nA;
  const Small2Lds lay(g.loops, ns, Bu, OS);
  const int bstride = lay.bstride;
  float* batch = sm + lay.batch;
  float* red = sm + lay.red;
  float* xg = sm + lay.xg;
  // three exchanges per update, two buffers: the parity flips from one update to the next, so an exchange never reuses
  // the buffer of the exchange right before it (a fast wave cannot overwrite partials a slow wave is still summing)
  int rp = 0;
  s2_stage_batches(g, sm_slots(g, sm, tid, nt), batch, bstride, ns, Bu, tid, nt);
  // ---- this thread's unit: parameters p, moments m/v, target pt
  float cw1[KC], cw1m[KC], cw1v[KC], cw1t[KC], cb1 = 0, cb1m = 0, cb1v = 0, cb1t = 0, cw2 = 0, cw2m = 0, cw2v = 0, cw2t = 0;
  float aw1[KA], aw1m[KA], aw1v[KA], aw1t[KA], ab1 = 0, ab1m = 0, ab1v = 0, ab1t = 0, aw2 = 0, aw2m = 0, aw2v = 0, aw2t = 0;
  // output biases: replicated in every thread (identical arithmetic), written back by thread 0
  const int cob1 = nC * K0, cow2 = cob1 + nC, cob2 = cow2 + nC;
  const int aob1 = nA * ns, aow2 = aob1 + nA, aob2 = aow2 + nA;
  float cb2 = g.C.p[cob2], cb2m = g.C.m[cob2], cb2v = g.C.v[cob2], cb2t = g.C.pt[cob2];
  float ab2 = g.A.p[aob2], ab2m = g.A.m[aob2], ab2v = g.A.v[aob2], ab2t = g.A.pt[aob2];
  s2_load_critic_unit(g.C, isC, tid, K0, cob1, cow2, cw1, cw1m, cw1v, cw1t, cb1, cb1m, cb1v, cb1t, cw2, cw2m, cw2v, cw2t);
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    const bool ok = isA && k < ns;
    aw1[k] = ok ? g.A.p[tid * ns + k] : 0.f; aw1m[k] = ok ? g.A.m[tid * ns + k] : 0.f;
    aw1v[k] = ok ? g.A.v[tid * ns + k] : 0.f; aw1t[k] = ok ? g.A.pt[tid * ns + k] : 0.f;
  }
  if (isA) {
    ab1 = g.A.p[aob1 + tid]; ab1m = g.A.m[aob1 + tid]; ab1v = g.A.v[aob1 + tid]; ab1t = g.A.pt[aob1 + tid];
    aw2 = g.A.p[aow2 + tid]; aw2m = g.A.m[aow2 + tid]; aw2v = g.A.v[aow2 + tid]; aw2t = g.A.pt[aow2 + tid];
  }
  constexpr int OSN = OS > 0 ? OS : 1;
  float op[OSN], om[OSN], ov[OSN], opt[OSN];
  const int nown = (ns + 2) * nA;                    // the actor's per-unit parameters = flat indices [0, nown)
  if constexpr (OS > 0) {
#pragma unroll
    for (int j = 0; j < OS; ++j) {
      const int f = j * 64 + tid;
      const bool own = tid < 64 && f < nown;
      op[j] = own ? g.A.p[f] : 0.f; om[j] = own ? g.A.m[f] : 0.f; ov[j] = own ? g.A.v[f] : 0.f; opt[j] = own ? g.A.pt[f] : 0.f;
    }
  }
  double bpa0 = g.bpA.cur[0], bpa1 = g.bpA.cur[1], bpc0 = g.bpC.cur[0], bpc1 = g.bpC.cur[1];
  const float omr = 1.0f - g.rho, invB = 1.f / (float)Bu;
  const bool frz = g.rho == 1.0f;
  float closs = 0.f, aloss = 0.f;
  for (int it = 0; it < g.loops; ++it) {
    const float* bsn = batch + it * bstride;
    const float* bs = bsn + ns * Bu;
    const float* ba = bs + ns * Bu;
    const float* br = ba + Bu;
    const float* bt = br + Bu;
    if (it == 0) __syncthreads();          // the batches are staged
    float v[2 * BUT];
    // Three exchanges per update: {a' = At(s'), A(s)} -> {qt = Ct([s'; a']), q = C([s; a])} -> critic update ->
    // {q of the updated critic on [s; A(s)], da}.  The behaviour actor's forward does not depend on the critic update, so
    // it shares the first exchange with the target actor's (src/PDEagent.jl:385 and :403).
    float ha[BUT];
#pragma unroll
    for (int c = 0; c < BUT; ++c) {
      float zt = ab1t, z = ab1;
#pragma unroll
      for (int k = 0; k < KA; ++k)
        if (k < ns) {
          zt += aw1t[k] * bsn[k * Bu + (c < Bu ? c : 0)];
          z += aw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
        }
      const bool on = isA && c < Bu;
      ha[c] = on ? fmaxf(z, 0.f) : 0.f;
      v[c] = on ? aw2t * fmaxf(zt, 0.f) : 0.f;
      v[BUT + c] = aw2 * ha[c];
    }
    s2_reduce2<2 * BUT>(v, Bu, red + rp * (S2_NW * S2_ROW), nw, tid);
    rp ^= 1;
    float an[BUT], ao[BUT];
#pragma unroll
    for (int c = 0; c < BUT; ++c) { an[c] = tanhf(v[c] + ab2t); ao[c] = tanhf(v[BUT + c] + ab2); }
    // ---- qt = Ct([s'; a'])  :386   and   q = C([s; a])  :392
    float h[BUT];
#pragma unroll
    for (int c = 0; c < BUT; ++c) {
      float zt = cb1t, z = cb1;
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (k < ns) {
          zt += cw1t[k] * bsn[k * Bu + (c < Bu ? c : 0)];
          z += cw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
        } else if (k == ns) {
          zt += cw1t[k] * an[c];
          z += cw1[k] * ba[c < Bu ? c : 0];
        }
      const bool on = isC && c < Bu;
      h[c] = on ? fmaxf(z, 0.f) : 0.f;
      v[c] = on ? cw2t * fmaxf(zt, 0.f) : 0.f;
      v[BUT + c] = cw2 * h[c];
    }
    s2_reduce2<2 * BUT>(v, Bu, red + rp * (S2_NW * S2_ROW), nw, tid);
    rp ^= 1;
    float qt[BUT];
#pragma unroll
    for (int c = 0; c < BUT; ++c) { qt[c] = v[c] + cb2t; v[c] = v[BUT + c]; }     // v[c] = q partial sum (without b2)
    float dq[BUT];
    {
      float rbar = 0.f;
      for (int c = 0; c < Bu; ++c) rbar += br[c];
      rbar *= invB;
      float loss = 0.f, gb2 = 0.f;
#pragma unroll
      for (int c = 0; c < BUT; ++c) {
        dq[c] = 0.f;
        if (c < Bu) {
          const float cc = g.gamma * (1.f - bt[c]) * qt[c] - (v[c] + cb2);
          if (g.quirk) {
            for (int j = 0; j < Bu; ++j) loss += (br[j] + cc) * (br[j] + cc);
          } else {
            loss += (br[c] + cc) * (br[c] + cc);
          }
          dq[c] = -(2.f * invB) * ((g.quirk ? rbar : br[c]) + cc);
          gb2 += dq[c];
        }
      }
      closs = g.quirk ? loss / (float)(Bu * Bu) : loss * invB;
      const double o1 = 1.0 / (1.0 - bpc0), o2 = 1.0 / (1.0 - bpc1);
      // thread-local backward of unit `tid`: dW2 = sum_c dq h, dz1 = relu'(h) w2 dq, db1 = sum_c dz1, dW1[k] = sum_c dz1 x[k]
      float gw2 = 0.f, gb1 = 0.f, gw1[KC];
#pragma unroll
      for (int k = 0; k < KC; ++k) gw1[k] = 0.f;
#pragma unroll
      for (int c = 0; c < BUT; ++c)
        if (c < Bu) {
          gw2 = fmaf(dq[c], h[c], gw2);
          const float dz = h[c] > 0.f ? cw2 * dq[c] : 0.f;
          gb1 += dz;
#pragma unroll
          for (int k = 0; k < KC; ++k)
            if (k < ns) gw1[k] = fmaf(dz, bs[k * Bu + c], gw1[k]);
            else if (k == ns) gw1[k] = fmaf(dz, ba[c], gw1[k]);
        }
      if (isC) {
#pragma unroll
        for (int k = 0; k < KC; ++k)
          if (k < K0) s2_adam(cw1[k], cw1m[k], cw1v[k], cw1t[k], gw1[k], g.eta_c, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
        s2_adam(cb1, cb1m, cb1v, cb1t, gb1, g.eta_c, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
        s2_adam(cw2, cw2m, cw2v, cw2t, gw2, g.eta_c, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
      }
      s2_adam(cb2, cb2m, cb2v, cb2t, gb2, g.eta_c, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
      bpc0 *= g.b1;
      bpc1 *= g.b2;
    }
    // ---- actor: -mean(C([s; A(s)])) with the updated critic                     :402-412
    // critic forward on [s; A(s)]: q for the reported loss and da[c] = sum_f W1c[f][ns] relu'(h) w2 (-1/Bu) in ONE exchange
#pragma unroll
    for (int c = 0; c < BUT; ++c) {
      float z = cb1;
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (k < ns) z += cw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
        else if (k == ns) z += cw1[k] * ao[c];
      const bool on = isC && c < Bu;
      v[c] = on ? cw2 * fmaxf(z, 0.f) : 0.f;
      float wns = 0.f;
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (k == ns) wns = cw1[k];
      v[BUT + c] = (on && z > 0.f) ? wns * cw2 * (-invB) : 0.f;
    }
    s2_reduce2<2 * BUT>(v, Bu, red + rp * (S2_NW * S2_ROW), nw, tid);
    rp ^= 1;
    {
      float s = 0.f;
      for (int c = 0; c < Bu; ++c) s += v[c] + cb2;
      aloss = -s * invB;
      const double o1 = 1.0 / (1.0 - bpa0), o2 = 1.0 / (1.0 - bpa1);
      const S2ActorGrad<KA> ag = s2_actor_grad<KA, BUT>(v + BUT, ao, ha, aw2, bs, Bu, ns);
      if constexpr (OS > 0) {
        if (tid < 64) {                    // wave 0: units -> owners -> units through LDS, in program order
          float* gA = xg;
          float* pA = xg + 64 * OS;
          float* ptA = pA + 64 * OS;
          if (isA) {
#pragma unroll
            for (int k = 0; k < KA; ++k)
              if (k < ns) gA[tid * ns + k] = ag.gw1[k];
            gA[aob1 + tid] = ag.gb1;
            gA[aow2 + tid] = ag.gw2;
          }
#pragma unroll
          for (int j = 0; j < OS; ++j) {
            const int f = j * 64 + tid;
            if (f < nown) {
              s2_adam(op[j], om[j], ov[j], opt[j], gA[f], g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
              pA[f] = op[j];
              if (!frz) ptA[f] = opt[j];
            }
          }
          if (isA) {
#pragma unroll
            for (int k = 0; k < KA; ++k)
              if (k < ns) {
                aw1[k] = pA[tid * ns + k];
                if (!frz) aw1t[k] = ptA[tid * ns + k];
              }
            ab1 = pA[aob1 + tid]; aw2 = pA[aow2 + tid];
            if (!frz) { ab1t = ptA[aob1 + tid]; aw2t = ptA[aow2 + tid]; }
          }
        }
      } else if (isA) {
#pragma unroll
        for (int k = 0; k < KA; ++k)
          if (k < ns) s2_adam(aw1[k], aw1m[k], aw1v[k], aw1t[k], ag.gw1[k], g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
        s2_adam(ab1, ab1m, ab1v, ab1t, ag.gb1, g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
        s2_adam(aw2, aw2m, aw2v, aw2t, ag.gw2, g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
      }
      s2_adam(ab2, ab2m, ab2v, ab2t, ag.gb2, g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
      bpa0 *= g.b1;
      bpa1 *= g.b2;
    }
  }
  // ---- write the learner state back
  if (isC) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k < K0) {
        g.C.p[tid * K0 + k] = cw1[k]; g.C.m[tid * K0 + k] = cw1m[k]; g.C.v[tid * K0 + k] = cw1v[k];
        if (!frz) g.C.pt[tid * K0 + k] = cw1t[k];
      }
    g.C.p[cob1 + tid] = cb1; g.C.m[cob1 + tid] = cb1m; g.C.v[cob1 + tid] = cb1v;
    if (!frz) g.C.pt[cob1 + tid] = cb1t;
    g.C.p[cow2 + tid] = cw2; g.C.m[cow2 + tid] = cw2m; g.C.v[cow2 + tid] = cw2v;
    if (!frz) g.C.pt[cow2 + tid] = cw2t;
  }
  if constexpr (OS > 0) {
#pragma unroll
    for (int j = 0; j < OS; ++j) {
      const int f = j * 64 + tid;
      if (tid < 64 && f < nown) {
        g.A.p[f] = op[j]; g.A.m[f] = om[j]; g.A.v[f] = ov[j];
        if (!frz) g.A.pt[f] = opt[j];
      }
    }
  } else if (isA) {
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (k < ns) {
        g.A.p[tid * ns + k] = aw1[k]; g.A.m[tid * ns + k] = aw1m[k]; g.A.v[tid * ns + k] = aw1v[k];
        if (!frz) g.A.pt[tid * ns + k] = aw1t[k];
      }
    g.A.p[aob1 + tid] = ab1; g.A.m[aob1 + tid] = ab1m; g.A.v[aob1 + tid] = ab1v;
    if (!frz) g.A.pt[aob1 + tid] = ab1t;
    g.A.p[aow2 + tid] = aw2; g.A.m[aow2 + tid] = aw2m; g.A.v[aow2 + tid] = aw2v;
    if (!frz) g.A.pt[aow2 + tid] = aw2t;
  }
  if (tid == 0) {
    g.C.p[cob2] = cb2; g.C.m[cob2] = cb2m; g.C.v[cob2] = cb2v;
    if (!frz) g.C.pt[cob2] = cb2t;
    g.A.p[aob2] = ab2; g.A.m[aob2] = ab2m; g.A.v[aob2] = ab2v;
    if (!frz) g.A.pt[aob2] = ab2t;
    if (g.losses) { g.losses[0] = closs; g.losses[1] = aloss; }
    g.bpA.next[0] = bpa0; g.bpA.next[1] = bpa1;
    g.bpC.next[0] = bpc0; g.bpC.next[1] = bpc1;
  }
}

}  // namespace pdec
