// small2f.hpp -- the update of small2.hpp for the reference's FROZEN target networks (rho == 1: the Polyak loop of
// src/PDEagent.jl:414-417 runs over an empty parameter list) -- the KS experiments' regime -- as TWO CHAINS SIDE BY
// SIDE.  With targets that never move
//   * the TD targets gamma (1 - t) Ct([s'; At(s')]) of all `loops` minibatches depend on nothing the launch changes: they are
//     computed once, up front, all columns at a time (one tanhf stream for all of them instead of three per update);
//   * a critic update reads the critic alone; an actor update reads the actor and the critic AFTER the critic update of the same
//     loop.  So the critic waves (one thread per critic unit, as in ddpg_small2_kernel) run critic update i while ONE more wave, on
//     the SIMD that kernel leaves idle, runs actor update i - 1 against the critic weights update i - 1 published in LDS (double
//     buffered): a lane of that wave holds the actor's unit `lane` and walks the critic's units lane, 64 + lane, ... for the
//     forward through the updated critic.  Two workgroup barriers per iteration (the critic's exchange, the hand-over), loops + 1
//     iterations; per iteration each wave issues about a third of what an update costs it there.
// Bit-identical to ddpg_small2_kernel at rho == 1: every sum is taken over the same lanes in the same order (the actor wave sums
// critic units r * 64 + lane by the wave tree and adds the rows r in order, which is what the cross-wave exchange there does), the
// expressions are the ones there (test_split_small_update_is_bit_identical).  Needs (KA + 2) nA + 1 <= 64 and nC <= 448; launched for the exact
// KS instantiation only (see small_plan).
#pragma once
#include "small2_blocks.hpp"

namespace pdec {

// NWC: the number of critic waves, a compile-time constant (3 for the KS nets' 140 critic units): the row loop of the actor wave
// unrolls and its 18 wave sums interleave
template <int KC, int KA, int BUT, bool EXACT, int NWC>
__global__ __launch_bounds__(512) void ddpg_small2f_kernel(Small2Args a_m) {
  Small2Args a_in = a_m;
  if (a_in.g.pm && !sm_member_begin(a_in.g)) return;
  const SmallArgs& g = a_in.g;
  extern __shared__ __align__(16) float sm[];
  const int tid = threadIdx.x, nt = blockDim.x, nwc = NWC, wv = tid >> 6, lane = tid & 63;
  if (sm_halted(g, tid)) return;
  const int Bu = EXACT ? BUT : g.Bu, ns = EXACT ? KA : g.ns, K0 = ns + 1, nC = a_in.nC, nA = a_in.nA;
  const bool actor_wave = wv == nwc;
  const bool isC = !actor_wave && tid < nC, isA = actor_wave && lane < nA;
  const Small2fLds lay(g.loops, ns, Bu, KC, nwc);
  const int bstride = lay.bstride, ncol = lay.ncol, PUBN = lay.pubn, PUBS = lay.pubs;
  float* batch = sm + lay.batch;
  float* red = sm + lay.red;
  float* tq = sm + lay.tq;
  float* tan_ = sm + lay.tan_;
  float* tpart = sm + lay.tpart;
  float* pub = sm + lay.pub;
  s2_stage_batches(g, sm_slots(g, sm, tid, nt), batch, bstride, ns, Bu, tid, nt);
  // ---- this thread's unit (critic waves: critic unit tid; actor wave: actor unit lane)
  float cw1[KC], cw1m[KC], cw1v[KC], cw1t[KC], cb1 = 0, cb1m = 0, cb1v = 0, cb1t = 0, cw2 = 0, cw2m = 0, cw2v = 0, cw2t = 0;
  float aw1[KA], aw1t[KA], ab1 = 0, ab1t = 0, aw2 = 0, aw2t = 0;        // (the actor's moments: with their owner lanes, below)
  const int cob1 = nC * K0, cow2 = cob1 + nC, cob2 = cow2 + nC;
  const int aob1 = nA * ns, aow2 = aob1 + nA, aob2 = aow2 + nA;
  float cb2 = g.C.p[cob2], cb2m = g.C.m[cob2], cb2v = g.C.v[cob2], cb2t = g.C.pt[cob2];
  float ab2 = g.A.p[aob2], ab2t = g.A.pt[aob2];
  s2_load_critic_unit(g.C, isC, tid, K0, cob1, cow2, cw1, cw1m, cw1v, cw1t, cb1, cb1m, cb1v, cb1t, cw2, cw2m, cw2v, cw2t);
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    const bool ok = isA && k < ns;
    aw1[k] = ok ? g.A.p[lane * ns + k] : 0.f;
    aw1t[k] = ok ? g.A.pt[lane * ns + k] : 0.f;
  }
  if (isA) {
    ab1 = g.A.p[aob1 + lane]; ab1t = g.A.pt[aob1 + lane];
    aw2 = g.A.p[aow2 + lane]; aw2t = g.A.pt[aow2 + lane];
  }
  // The actor's ADAM state lives ONE PARAMETER PER LANE of the actor wave: lane kind * nA + unit owns parameter `kind` (first-layer
  // weights 0 .. KA-1, then b1, then w2) of unit `unit`, lane (KA + 2) nA owns b2 -- (KA + 2) nA + 1 <= 64 lanes, one ADAM chain per
  // update instead of KA + 3 one after the other on nA lanes (the actor wave is the long pole of an iteration and ~45 % of its work
  // was these chains).  Gradients reach their owner and the new weights their unit by ds_bpermute; same arithmetic per parameter.
  constexpr int NP = KA + 2;
  const int okind = actor_wave ? lane / nA : 0, ounit = lane - okind * nA;
  const bool ownP = actor_wave && lane < NP * nA, ownB2 = actor_wave && lane == NP * nA;
  const int oidx = ownB2 ? aob2 : (okind < KA ? ounit * ns + okind : (okind == KA ? aob1 + ounit : aow2 + ounit));
  float op = 0.f, om = 0.f, ov = 0.f, opt_unused = 0.f;
  if ((ownP && (okind >= KA || okind < ns)) || ownB2) { op = g.A.p[oidx]; om = g.A.m[oidx]; ov = g.A.v[oidx]; }
  double bpa0 = g.bpA.cur[0], bpa1 = g.bpA.cur[1], bpc0 = g.bpC.cur[0], bpc1 = g.bpC.cur[1];
  const float invB = 1.f / (float)Bu;
  float closs = 0.f, aloss = 0.f;
  __syncthreads();                         // the batches are staged
  // ---- TD targets of every minibatch column, once.  a' = tanh(At(s')): actor wave, one tanhf stream over the columns.
  // Columns go four at a time: their wave sums are independent dependency chains (six DPP adds with hazard waits each) that
  // the scheduler interleaves inside one block -- one column per trip cost 15 us of the launch, a quarter of it.
  constexpr int PG = 4;
  if (actor_wave && nA <= 16) {
    // The actor's units fit one ROW of 16 lanes: a DPP chain then sums FOUR columns, one per row (unit lane & 15 of column ... + row;
    // the row totals at lanes 15 / 31 / 47 / 63 are formed exactly like the single row total of s2_wave_sum, whose two broadcast
    // steps only add the zeros of the empty rows) -- 16 columns per trip of four chains.
    const int ru = lane & 15, rr = lane >> 4;
    const bool isAr = ru < nA;
    float rw1[KA], rb1 = isAr ? g.A.pt[aob1 + ru] : 0.f, rw2 = isAr ? g.A.pt[aow2 + ru] : 0.f;
#pragma unroll
    for (int k = 0; k < KA; ++k) rw1[k] = (isAr && k < ns) ? g.A.pt[ru * ns + k] : 0.f;
    for (int col0 = 0; col0 < ncol; col0 += 64) {
      float mine = 0.f;
      const int nc = min(64, ncol - col0);
      for (int cc0 = 0; cc0 < nc; cc0 += 4 * PG) {
        float S[PG];
#pragma unroll
        for (int u = 0; u < PG; ++u) {
          const int col = min(col0 + cc0 + 4 * u + rr, ncol - 1), it = col / Bu, c = col - it * Bu;
          const float* bsn = batch + it * bstride;
          float zt = rb1;
#pragma unroll
          for (int k = 0; k < KA; ++k)
            if (k < ns) zt += rw1[k] * bsn[k * Bu + c];
          S[u] = s2_row_sum(isAr ? rw2 * fmaxf(zt, 0.f) : 0.f);
        }
#pragma unroll
        for (int u = 0; u < PG; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float T = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, S[u]), 16 * r + 15));
            if (lane == cc0 + 4 * u + r) mine = T;
          }
      }
      if (lane < nc) tan_[col0 + lane] = tanhf((0.f + mine) + ab2t);
    }
  } else if (actor_wave) {
    for (int col0 = 0; col0 < ncol; col0 += 64) {
      float mine = 0.f;
      const int nc = min(64, ncol - col0);
      for (int cc0 = 0; cc0 < nc; cc0 += PG) {
        float S[PG];
#pragma unroll
        for (int u = 0; u < PG; ++u) {
          const int col = min(col0 + cc0 + u, ncol - 1), it = col / Bu, c = col - it * Bu;
          const float* bsn = batch + it * bstride;
          float zt = ab1t;
#pragma unroll
          for (int k = 0; k < KA; ++k)
            if (k < ns) zt += aw1t[k] * bsn[k * Bu + c];
          S[u] = s2_wave_sum(isA ? aw2t * fmaxf(zt, 0.f) : 0.f);
        }
#pragma unroll
        for (int u = 0; u < PG; ++u)
          if (lane == cc0 + u) mine = S[u];
      }
      if (lane < nc) tan_[col0 + lane] = tanhf((0.f + mine) + ab2t);
    }
  }
  __syncthreads();
  // qt = Ct([s'; a']): critic waves (their threads hold the target critic's units), wave sums by column
  if (!actor_wave) {
    for (int col0 = 0; col0 < ncol; col0 += PG) {
      float S[PG];
#pragma unroll
      for (int u = 0; u < PG; ++u) {
        const int col = min(col0 + u, ncol - 1), it = col / Bu, c = col - it * Bu;
        const float* bsn = batch + it * bstride;
        const float an = tan_[col];
        float zt = cb1t;
#pragma unroll
        for (int k = 0; k < KC; ++k)
          if (k < ns) zt += cw1t[k] * bsn[k * Bu + c];
          else if (k == ns) zt += cw1t[k] * an;
        S[u] = s2_wave_sum(isC ? cw2t * fmaxf(zt, 0.f) : 0.f);
      }
      if (lane == 0)
#pragma unroll
        for (int u = 0; u < PG; ++u)
          if (col0 + u < ncol) tpart[wv * ncol + col0 + u] = S[u];
    }
  }
  __syncthreads();
  for (int col = tid; col < ncol; col += nt) {
    float a = 0.f;
    for (int w = 0; w < nwc; ++w) a += tpart[w * ncol + col];
    tq[col] = a + cb2t;
  }
  // (the first barrier of the loop below orders tq before its first reader)
  // ---- iteration i: critic update i (critic waves) beside actor update i - 1 (actor wave)
  for (int i = 0; i <= g.loops; ++i) {
    float* rb = red + (i & 1) * (S2_NW * S2_ROW);
    float* pw = pub + (i & 1) * PUBS;                 // the critic publishes update i here
    const float* pr = pub + ((i + 1) & 1) * PUBS;     // update i - 1, read by the actor wave
    if (!actor_wave) {
      if (i < g.loops) {
        const float* bs = batch + i * bstride + ns * Bu;
        const float* ba = bs + ns * Bu;
        const float* br = ba + Bu;
        const float* bt = br + Bu;
        // ---- q = C([s; a])  (src/PDEagent.jl:392)
        float h[BUT], v[BUT];
#pragma unroll
        for (int c = 0; c < BUT; ++c) {
          float z = cb1;
#pragma unroll
          for (int k = 0; k < KC; ++k)
            if (k < ns) z += cw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
            else if (k == ns) z += cw1[k] * ba[c < Bu ? c : 0];
          const bool on = isC && c < Bu;
          h[c] = on ? fmaxf(z, 0.f) : 0.f;
          v[c] = cw2 * h[c];
        }
#pragma unroll
        for (int c = 0; c < BUT; ++c)
          if (c < Bu) v[c] = s2_wave_sum(v[c]);
        if (lane == 0)
#pragma unroll
          for (int c = 0; c < BUT; ++c) rb[wv * S2_ROW + c] = v[c];
        __syncthreads();                                 // barrier 1
        float part[S2_NW][BUT];
#pragma unroll
        for (int w = 0; w < S2_NW; ++w)
#pragma unroll
          for (int c = 0; c < BUT; ++c) part[w][c] = rb[w * S2_ROW + c];
#pragma unroll
        for (int c = 0; c < BUT; ++c) v[c] = 0.f;
#pragma unroll
        for (int w = 0; w < S2_NW; ++w)
          if (w < nwc) {
#pragma unroll
            for (int c = 0; c < BUT; ++c) v[c] += part[w][c];
          }
        float qt[BUT], dq[BUT];
#pragma unroll
        for (int c = 0; c < BUT; ++c) qt[c] = c < Bu ? tq[i * Bu + c] : 0.f;
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
            if (k < K0) s2_adam(cw1[k], cw1m[k], cw1v[k], cw1t[k], gw1[k], g.eta_c, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
          s2_adam(cb1, cb1m, cb1v, cb1t, gb1, g.eta_c, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
          s2_adam(cw2, cw2m, cw2v, cw2t, gw2, g.eta_c, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
        }
        s2_adam(cb2, cb2m, cb2v, cb2t, gb2, g.eta_c, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
        bpc0 *= g.b1;
        bpc1 *= g.b2;
        // publish the updated critic for the actor wave
#pragma unroll
        for (int k = 0; k < KC; ++k) pw[k * PUBN + tid] = cw1[k];
        pw[KC * PUBN + tid] = cb1;
        pw[(KC + 1) * PUBN + tid] = cw2;
        if (tid == 0) pw[(KC + 2) * PUBN] = cb2;
      } else {
        __syncthreads();                                 // barrier 1 of the last iteration (the actor wave's partner)
      }
    } else {
      __syncthreads();                                   // barrier 1: the critic's exchange
      if (i >= 1) {
        const int j = i - 1;
        const float* bs = batch + j * bstride + ns * Bu;
        // ---- A(s)  (src/PDEagent.jl:403)
        float ha[BUT], ao[BUT];
        float mine = 0.f;
#pragma unroll
        for (int c = 0; c < BUT; ++c) {
          float z = ab1;
#pragma unroll
          for (int k = 0; k < KA; ++k)
            if (k < ns) z += aw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
          const bool on = isA && c < Bu;
          ha[c] = on ? fmaxf(z, 0.f) : 0.f;
          const float S = s2_wave_sum(aw2 * ha[c]);
          if (lane == c) mine = S;
        }
        {
          const float t = tanhf((0.f + mine) + ab2);      // lane c: tanh of column c -- one stream for the Bu columns
#pragma unroll
          for (int c = 0; c < BUT; ++c) ao[c] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t), c));
        }
        // ---- forward through the critic AFTER its update j: q on [s; A(s)] and da, rows r = units r * 64 + lane in order
        const float pcb2 = pr[(KC + 2) * PUBN];
        float vq[BUT], vd[BUT];
#pragma unroll
        for (int c = 0; c < BUT; ++c) vq[c] = vd[c] = 0.f;
#pragma unroll
        for (int r = 0; r < NWC; ++r) {
          const int u = r * 64 + lane;
          float w1[KC];
#pragma unroll
          for (int k = 0; k < KC; ++k) w1[k] = pr[k * PUBN + u];
          const float b1 = pr[KC * PUBN + u], w2 = pr[(KC + 1) * PUBN + u];
#pragma unroll
          for (int c = 0; c < BUT; ++c)
            if (c < Bu) {
              float z = b1;
#pragma unroll
              for (int k = 0; k < KC; ++k)
                if (k < ns) z += w1[k] * bs[k * Bu + c];
                else if (k == ns) z += w1[k] * ao[c];
              const bool on = u < nC;
              float wns = 0.f;
#pragma unroll
              for (int k = 0; k < KC; ++k)
                if (k == ns) wns = w1[k];
              vq[c] += s2_wave_sum(on ? w2 * fmaxf(z, 0.f) : 0.f);
              vd[c] += s2_wave_sum((on && z > 0.f) ? wns * w2 * (-invB) : 0.f);
            }
        }
        float sacc = 0.f;
        for (int c = 0; c < Bu; ++c) sacc += vq[c] + pcb2;
        aloss = -sacc * invB;
        const double o1 = 1.0 / (1.0 - bpa0), o2 = 1.0 / (1.0 - bpa1);
        const S2ActorGrad<KA> ag = s2_actor_grad<KA, BUT>(vd, ao, ha, aw2, bs, Bu, ns);
        {
          // gradients to their owner lanes (unit lanes hold gw1[k], gb1, gw2 of their unit; gb2 is the same in every lane)
          auto pull = [&](float x, int from) {
            return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(from * 4, __builtin_bit_cast(int, x)));
          };
          float gown = ag.gb2;
#pragma unroll
          for (int k = 0; k < KA; ++k) {
            const float t = pull(ag.gw1[k], ounit);
            if (ownP && okind == k) gown = t;
          }
          {
            const float t1 = pull(ag.gb1, ounit), t2 = pull(ag.gw2, ounit);
            if (ownP && okind == KA) gown = t1;
            if (ownP && okind == KA + 1) gown = t2;
          }
          if ((ownP && (okind >= KA || okind < ns)) || ownB2)
            s2_adam(op, om, ov, opt_unused, gown, g.eta_a, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
          // the new weights back to their units
#pragma unroll
          for (int k = 0; k < KA; ++k) {
            const float t = pull(op, lane + k * nA);
            if (isA && k < ns) aw1[k] = t;
          }
          const float t1 = pull(op, lane + KA * nA), t2 = pull(op, lane + (KA + 1) * nA);
          if (isA) { ab1 = t1; aw2 = t2; }
          ab2 = pull(op, NP * nA);
        }
        bpa0 *= g.b1;
        bpa1 *= g.b2;
      }
    }
    __syncthreads();                                     // barrier 2: update i is published, update i - 1 has been read
  }
  // ---- write the learner state back (the targets keep their bits)
  if (isC) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k < K0) { g.C.p[tid * K0 + k] = cw1[k]; g.C.m[tid * K0 + k] = cw1m[k]; g.C.v[tid * K0 + k] = cw1v[k]; }
    g.C.p[cob1 + tid] = cb1; g.C.m[cob1 + tid] = cb1m; g.C.v[cob1 + tid] = cb1v;
    g.C.p[cow2 + tid] = cw2; g.C.m[cow2 + tid] = cw2m; g.C.v[cow2 + tid] = cw2v;
  }
  if ((ownP && (okind >= KA || okind < ns)) || ownB2) { g.A.p[oidx] = op; g.A.m[oidx] = om; g.A.v[oidx] = ov; }
  if (tid == 0) {
    g.C.p[cob2] = cb2; g.C.m[cob2] = cb2m; g.C.v[cob2] = cb2v;
    if (g.losses) g.losses[0] = closs;
    g.bpC.next[0] = bpc0; g.bpC.next[1] = bpc1;
  }
  if (actor_wave && lane == 0) {
    if (g.losses) g.losses[1] = aloss;
    g.bpA.next[0] = bpa0; g.bpA.next[1] = bpa1;
  }
}

}  // namespace pdec
