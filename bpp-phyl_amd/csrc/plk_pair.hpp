// plk_pair.hpp -- pairwise maximum-likelihood distances: the sufficient statistics of every
// pair of tips in one pass over the tip codes, then a Newton ascent per pair on that table.
//
// The reference runs one TwoTreeLikelihood per pair (Distance/DistanceEstimation.cpp:647-687),
// each paying O(patterns) per trial length.  The likelihood of two sequences joined by one
// branch depends on a pattern only through its two codes (a, b), so with
//     N[a][b]  = sum_p w_p [code_a(p) = a][code_b(p) = b]                  (pair_count_kernel)
//     alpha[a][k] = sum_x pi_x init[a][x] V[x][k],  beta[k][b] = sum_y Vinv[k][y] init[b][y],
//     delta[a][b] = sum_x pi_x init[a][x] init[b][x]                       (pair_basis_kernel)
//     l_ab(t)  = sum_k alpha[a][k] beta[k][b] sum_c p_c exp(lambda_k r_c t)
// the log-likelihood is F(t) = sum_ab N_ab log l_ab(t) (TwoTreeLikelihood::computeTreeLikelihood
// :474-521 on codes instead of patterns) and pair_newton_kernel never sees a pattern.
//
// Counts.  A workgroup takes one 4096-pattern block and a group of kPairGroup pairs.  Its four
// waves share the block's patterns, four per lane (one 32-bit load per code row), and add the
// weights to bins in LDS with ds_add_f64: with U codes in use a lane's target is one of U^2
// addresses, so lanes collide and the add has to be atomic.  Up to 32 codes every wave has bins
// of its own (4 U^2 doubles <= 32 KB), beyond that the waves share one set; up to 64 codes the
// block's weights are staged in LDS once per workgroup (32 KB) and serve all pairs of the group,
// beyond that (U^2 doubles alone pass 32 KB) they are read through L2.  LDS stays within 64 KB,
// which bounds U at kPairMaxCodes = 90.  The bins are summed over the wave sets in set order
// and stored per (block, pair); pair_sum_kernel adds the blocks in block order and scatters the
// compact table into the caller's code numbering.  The order in which colliding lanes reach a
// bin is the hardware's: for integer weights with a sum below 2^53 every partial sum is exact
// and the table does not depend on any order; other weights agree to rounding.
// (Lane-private register bins for U <= 4 -- 16 compare-and-adds per pattern -- and a Gram
// product of one-hot rows on the matrix pipe -- U times the useful work -- were weighed against
// this and not built: DESIGN 4.8.)
//
// Newton.  One workgroup per pair runs the whole ascent; the rule is plk_nni_scores' (plk.h).
// Per evaluation the S sums over the rate classes
//     G0[k] = sum_c p_c e(mu t), G1 = sum_c p_c mu exp(mu t), G2 = sum_c p_c mu^2 exp(mu t),
//     GA[k] = sum_c p_c e(mu t_acc), GX[k] = sum_c p_c exp(mu t_acc) expm1(mu (t - t_acc)),
// mu = lambda_k r_c, are formed once in LDS (e = expm1 while t max|mu| <= 1, the short-length
// form of plk_nni.hpp: l = delta + sum alpha beta G0, else exp), and every entry with N > 0 is
// S fused multiply-adds per sum.  Sums over entries: per lane in entry order, lanes by
// butterfly, waves in wave order -- fixed, so a pair's result does not depend on its place in
// the list or on the chunking.
#pragma once

#include "plk_nni.hpp"

namespace plk {

constexpr int kPairThreads = 256;
constexpr int kPairBlock = 4096;    // patterns per workgroup of pair_count_kernel (= kRootBlock)
constexpr int kPairGroup = 8;       // pairs per workgroup
constexpr int kPairMaxCodes = 90;   // codes in use: U^2 doubles within 64 KB of LDS
constexpr int kPairOwnBins = 32;    // up to here one set of bins per wave
constexpr int kPairStageW = 64;     // up to here the weights are staged in LDS

struct PairCountArgs {
  const uint8_t* codes;     // compact codes [tip][n_pad]
  const double* weights;    // [n_pad]
  const int32_t* tip_a;     // [n_pairs]
  const int32_t* tip_b;
  double* part;             // [block][pair][U^2]
  int64_t n_pad;
  int64_t n_patterns;
  int32_t U;
  int32_t n_pairs;
};

__global__ __launch_bounds__(kPairThreads) void pair_count_kernel(PairCountArgs a) {
  extern __shared__ double lds[];  // weights [kPairBlock] when staged, then bins [sets][U^2]
  const int U = a.U, U2 = U * U;
  const bool stage = U <= kPairStageW;
  const int sets = U <= kPairOwnBins ? kPairThreads / 64 : 1;
  double* wl = lds;
  double* bins = lds + (stage ? kPairBlock : 0);
  const int64_t p0 = (int64_t)blockIdx.x * kPairBlock;
  if (stage)
    for (int i = threadIdx.x; i < kPairBlock; i += kPairThreads) wl[i] = p0 + i < a.n_patterns ? a.weights[p0 + i] : 0.0;
  for (int i = threadIdx.x; i < sets * U2; i += kPairThreads) bins[i] = 0.0;
  __syncthreads();
  double* mine = bins + ((threadIdx.x >> 6) % sets) * U2;
  const int pr1 = min((int)(blockIdx.y + 1) * kPairGroup, a.n_pairs);
  for (int pr = blockIdx.y * kPairGroup; pr < pr1; ++pr) {
    const uint8_t* __restrict__ ra = a.codes + (int64_t)a.tip_a[pr] * a.n_pad;
    const uint8_t* __restrict__ rb = a.codes + (int64_t)a.tip_b[pr] * a.n_pad;
#pragma unroll
    for (int it = 0; it < kPairBlock / (4 * kPairThreads); ++it) {
      const int i = (it * kPairThreads + threadIdx.x) * 4;
      const int64_t p = p0 + i;
      // p is a multiple of 4 and so is n_pad >= n_patterns: the four bytes lie inside the row
      if (p < a.n_patterns) {
        const uint32_t ca = *reinterpret_cast<const uint32_t*>(ra + p);
        const uint32_t cb = *reinterpret_cast<const uint32_t*>(rb + p);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (p + j < a.n_patterns) {  // padding patterns add nothing
            const double w = stage ? wl[i + j] : a.weights[p + j];
            atomicAdd(&mine[((ca >> (8 * j)) & 255u) * U + ((cb >> (8 * j)) & 255u)], w);
          }
      }
    }
    __syncthreads();
    double* __restrict__ out = a.part + ((int64_t)blockIdx.x * a.n_pairs + pr) * U2;
    for (int i = threadIdx.x; i < U2; i += kPairThreads) {
      double s = 0.0;
      for (int q = 0; q < sets; ++q) {  // fixed order
        s += bins[q * U2 + i];
        bins[q * U2 + i] = 0.0;
      }
      out[i] = s;
    }
    __syncthreads();
  }
}

// The blocks in block order, into the caller's code numbering (full is zero on entry).
__global__ __launch_bounds__(256) void pair_sum_kernel(const double* __restrict__ part, double* __restrict__ full,
                                                       const int32_t* __restrict__ orig, int n_blk, int n_pairs, int U,
                                                       int Ut) {
  const int U2 = U * U;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)n_pairs * U2) return;
  const int pr = (int)(id / U2), i = (int)(id - (int64_t)pr * U2);
  double s = 0.0;
  for (int b = 0; b < n_blk; ++b) s += part[((int64_t)b * n_pairs + pr) * U2 + i];
  full[(int64_t)pr * Ut * Ut + (int64_t)orig[i / U] * Ut + orig[i % U]] = s;
}

struct PairBasisArgs {
  const double* table;   // the caller's code table [Ut][S]
  const double* V;       // of the model
  const double* Vinv;
  const double* pi;
  double* alpha;         // [Ut][S]
  double* beta;          // [S][Ut]
  double* delta;         // [Ut][Ut]
  int32_t* res;          // [Ut] the state of a resolved code (one non-zero entry), else -1
  int32_t S, Ut;
};

__global__ __launch_bounds__(256) void pair_basis_kernel(PairBasisArgs a) {
  const int S = a.S, Ut = a.Ut;
  const int n = gridDim.x * 256, id = blockIdx.x * 256 + threadIdx.x;
  for (int e = id; e < Ut * S; e += n) {
    const int c = e / S, k = e - c * S;
    double s = 0.0;
    for (int x = 0; x < S; ++x) s = fma(a.pi[x] * a.table[c * S + x], a.V[x * S + k], s);
    a.alpha[e] = s;
  }
  for (int e = id; e < S * Ut; e += n) {
    const int k = e / Ut, c = e - k * Ut;
    double s = 0.0;
    for (int y = 0; y < S; ++y) s = fma(a.Vinv[k * S + y], a.table[c * S + y], s);
    a.beta[e] = s;
  }
  for (int e = id; e < Ut * Ut; e += n) {
    const int c = e / Ut, d = e - c * Ut;
    double s = 0.0;
    for (int x = 0; x < S; ++x) s = fma(a.pi[x] * a.table[c * S + x], a.table[d * S + x], s);
    a.delta[e] = s;
  }
  for (int c = id; c < Ut; c += n) {
    int cnt = 0, st = -1;
    for (int x = 0; x < S; ++x)
      if (a.table[c * S + x] != 0.0) ++cnt, st = x;
    a.res[c] = cnt == 1 ? st : -1;
  }
}

struct PairNewtonArgs {
  const double* full;     // [pair][Ut][Ut]
  const double* alpha;
  const double* beta;
  const double* delta;
  const int32_t* res;
  const double* lambda;   // [S] of the model
  const double* rates;
  const double* probs;
  const double* t0;       // [pair], or null: the start from the table
  double* out;            // [pair][4]: t_opt, lnl, d1, d2
  int32_t* status;        // [pair]
  int32_t* passes;        // [pair]
  double t_min, t_max, tol;
  int32_t S, C, Ut, max_iter;
};

__global__ __launch_bounds__(kPairThreads) void pair_newton_kernel(PairNewtonArgs a) {
  extern __shared__ double lds[];  // G [5][S], then the wave sums [4][waves]
  constexpr int NW = kPairThreads / 64;
  const int S = a.S, C = a.C, Ut = a.Ut, UU = a.Ut * a.Ut;
  double* G = lds;
  double* red = lds + 5 * S;
  const double* __restrict__ N = a.full + (int64_t)blockIdx.x * UU;
  // v[] over the workgroup, every thread gets the sums (uniform decisions below)
  auto reduce = [&](double (&v)[4]) {
    __syncthreads();  // red's readers of the previous round are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double r = v[i];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
      if ((threadIdx.x & 63) == 0) red[i * NW + (threadIdx.x >> 6)] = r;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double s = 0.0;
      for (int q = 0; q < NW; ++q) s += red[i * NW + q];  // fixed order
      v[i] = s;
    }
  };
  double lmax = 0.0, rmax = 0.0;
  for (int k = 0; k < S; ++k) lmax = fmax(lmax, fabs(a.lambda[k]));
  for (int c = 0; c < C; ++c) rmax = fmax(rmax, fabs(a.rates[c]));
  // F, d1, d2 at t and F(t) - F(ta)
  auto eval = [&](double t, double ta, double (&v)[4]) {
    const bool small = t * lmax * rmax <= 1.0, small_a = ta * lmax * rmax <= 1.0;
    __syncthreads();  // G's readers of the previous evaluation are done
    for (int k = threadIdx.x; k < S; k += kPairThreads) {
      double g0 = 0.0, g1 = 0.0, g2 = 0.0, ga = 0.0, gx = 0.0;
      for (int c = 0; c < C; ++c) {
        const double mu = a.lambda[k] * a.rates[c], pc = a.probs[c];
        const double e = exp(mu * t), ea = exp(mu * ta);
        g0 = fma(pc, small ? expm1(mu * t) : e, g0);
        g1 = fma(pc * mu, e, g1);
        g2 = fma(pc * mu * mu, e, g2);
        ga = fma(pc, small_a ? expm1(mu * ta) : ea, ga);
        gx = fma(pc * ea, expm1(mu * (t - ta)), gx);
      }
      G[k] = g0, G[S + k] = g1, G[2 * S + k] = g2, G[3 * S + k] = ga, G[4 * S + k] = gx;
    }
    __syncthreads();
    v[0] = v[1] = v[2] = v[3] = 0.0;
    for (int e = threadIdx.x; e < UU; e += kPairThreads) {
      const double n = N[e];
      if (!(n > 0.0)) continue;
      const int ca = e / Ut, cb = e - ca * Ut;
      double l0 = 0.0, l1 = 0.0, l2 = 0.0, la = 0.0, dx = 0.0;
      for (int k = 0; k < S; ++k) {
        const double ab = a.alpha[ca * S + k] * a.beta[k * Ut + cb];
        l0 = fma(ab, G[k], l0);
        l1 = fma(ab, G[S + k], l1);
        l2 = fma(ab, G[2 * S + k], l2);
        la = fma(ab, G[3 * S + k], la);
        dx = fma(ab, G[4 * S + k], dx);
      }
      const double d = a.delta[e];
      if (small) l0 += d;
      if (small_a) la += d;
      const bool ok = post_ok(l0), ok_a = ok && post_ok(la);
      if (ok) {
        const double g1 = l1 / l0, g2 = l2 / l0;
        v[0] = fma(n, log(l0), v[0]);
        v[1] = fma(n, g1, v[1]);
        v[2] = fma(n, g2 - g1 * g1, v[2]);
      }
      if (ok_a) {
        const double q = dx / la;
        // (a ratio far from 1 has nothing to cancel: the plain quotient there)
        v[3] = fma(n, q > -0.5 ? log1p(q) : log(l0 / la), v[3]);
      }
    }
    reduce(v);
  };
  double v[4];
  double t;
  if (a.t0) {
    t = a.t0[blockIdx.x];
  } else {
    // d / g: the weight of the entries with both codes resolved, and of those that differ
    v[0] = v[1] = v[2] = v[3] = 0.0;
    for (int e = threadIdx.x; e < UU; e += kPairThreads) {
      const double n = N[e];
      const int ra = a.res[e / Ut], rb = a.res[e % Ut];
      if (n > 0.0 && ra >= 0 && rb >= 0) {
        v[0] += n;
        if (ra != rb) v[1] += n;
      }
    }
    reduce(v);
    t = v[0] > 0.0 ? fmin(fmax(v[1] / v[0], a.t_min), a.t_max) : a.t_min;
  }
  eval(t, t, v);
  double F = v[0], D1 = v[1], D2 = v[2], trial = 0.0;
  bool half = false;
  int st = 0, it = 0;
  while (a.max_iter > 0) {
    double tp = half ? 0.5 * (t + trial) : D2 < 0.0 ? t - D1 / D2 : D1 > 0.0 ? 2.0 * t : 0.5 * t;
    tp = tp != tp ? t : fmin(fmax(tp, a.t_min), a.t_max);
    if (fabs(tp - t) <= a.tol * fmax(t, a.t_min)) break;  // converged
    if (it == a.max_iter) {
      st = 1;
      break;
    }
    trial = tp;
    eval(tp, t, v);
    ++it;
    if (v[3] >= 0.0) {
      t = tp, F += v[3], D1 = v[1], D2 = v[2];
      half = false;
    } else {
      half = true;
    }
  }
  if (threadIdx.x == 0) {
    double* o = a.out + (int64_t)blockIdx.x * 4;
    o[0] = t, o[1] = F, o[2] = D1, o[3] = D2;
    a.status[blockIdx.x] = st;
    a.passes[blockIdx.x] = 1 + it;
  }
}

}  // namespace plk
