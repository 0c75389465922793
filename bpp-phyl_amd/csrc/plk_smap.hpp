// plk_smap.hpp -- stochastic mapping (plk_smap_sample): histories of substitutions on every branch,
// drawn from their posterior given the tips (Nielsen 2002).  The reference samples one site at a
// time and a branch by rejection (Mapping/StochasticMapping.cpp:591-641: simulate forward until the
// path ends in the son's state, 10 000 tries); here the same distribution is drawn without
// rejection:
//   1. ancestral states down the tree from the stored lower partials L: the class with weights
//      p_c sum_x pi_x L_root[c][x], the root state with pi_x L_root[c][x], node v under father state f
//      with P_v[c][f][y] L_v[c][y] (tips included: an ambiguous tip gets a sampled state);
//   2. per branch an endpoint-conditioned path by uniformisation (Hobolth & Stone 2009): with
//      mu = max_x -Q[x][x], R = I + Q / mu and lambda = mu r_c t_v, the number of jumps n has weights
//      Pois(n; lambda) R^n[a][b] (their sum is P_v[c][a][b]), the chain x_1 .. x_{n-1} has weights
//      R[x_{i-1}][y] R^{n-i}[y][b], and the n + 1 segment lengths are t_v times normalised
//      exponentials (the spacings of n uniform points).  A jump with x_i = x_{i-1} is virtual.
// Every draw is the weighted draw of include/plk.h on a uniform of plk_simulate's generator
// (plk_sim.hpp) with its fourth counter word telling the streams apart: 1 the ancestral draws,
// 2 + v the path of branch v.  Weights that are products are rounded before they are added
// (__dmul_rn, __dadd_rn: a fused multiply-add would change draws), so tests/smap_rule.py restates
// every integer result exactly.
//
// smap_table_kernel builds R and R^n (one workgroup per model and row: row x of R^n is row x of
// R^{n-1} times R, so the rows are independent) and the Poisson terms per (branch, class).
// smap_sample_kernel runs one lane per site over the call's replicates: the dwell sums are added
// in replicate order and the integer sums need no atomics, since a lane owns its site's entries.
// The (node, father) list is uniform over the lanes; L is read from the tiled layout, coalesced
// over patterns; P rows and the R / R^n tables are gathers on the lane's own (c, f, b), R^n stored
// [n][b][y] so that the column the chain draw walks is contiguous.  For 4 states the tables of
// every model are staged in LDS where they fit.  The jump scan and the chain have data-dependent
// trip counts: their bodies are short and nothing is done to make them wave-uniform.
#pragma once

#include "plk_sim.hpp"

namespace plk {

constexpr int kSmapMaxJumps = 128;            // PLK_SMAP_MAX_JUMPS
constexpr int kSmapN1 = kSmapMaxJumps + 1;    // table entries n = 0 .. 128
constexpr int kSmapThreads = 256;
constexpr size_t kSmapLdsMax = 64 * 1024;     // 4-state tables of every model at most, to be staged
constexpr double kSmapMaxLambda = 32.0;       // the Poisson tail beyond 128 is below 1e-30

struct SmapEntry {
  int32_t node;      // branch = child node index v
  int32_t father;
  int32_t model;
  int32_t is_tip;
  int32_t child;     // tip index or internal slot of v
  int32_t pad_;
  double t;
};

struct SmapArgs {
  // tables
  const double* Q;        // [model][S][S]
  double* R;              // [model][S][S]
  double* RpowT;          // [model][N + 1][b][y] = (R^n)[y][b]
  double* pois;           // [node][C][N + 1]
  const double* rates;
  const SmapEntry* list;  // fathers first
  int32_t n_list;
  int32_t S, C, T, n_models;
  int32_t rpow_blocks;    // leading workgroups of the table kernel that build R and R^n (0: current)
  // sampling
  const double* partials;
  const uint8_t* codes;       // compact codes [tip][n_pad]
  const double* code_table;   // compact table [n_codes][S]
  const double* pmats;
  const double* pi;
  const double* probs;
  const uint8_t* type_of;     // [S][S]
  int64_t slot_stride, n_pad, n_patterns;
  int32_t root, root_slot, n_nodes;
  int32_t n_rep, keep;
  uint64_t seed, replicate0, site0;
  uint8_t* states;        // [keep ? n_rep : 1][n_nodes + 1][n_pad]; row n_nodes holds the classes
  uint16_t* jumps;        // [n_rep][n_nodes][n_pad], kept rows only
  uint16_t* counts;       // [n_rep][n_nodes][T][n_pad], kept rows only
  double* dwell;          // [n_rep][n_nodes][S][n_pad] kept, else one scratch row [S][n_pad]
  uint32_t* count_sum;    // [n_nodes][T][n_pad]
  double* dwell_sum;      // [n_nodes][S][n_pad]
  uint32_t* state_tally;  // [n_nodes][S][n_pad]
  uint32_t* class_tally;  // [C][n_pad]
  unsigned long long* n_bad;
};

__device__ __forceinline__ double smap_mu(const double* __restrict__ Q, int S) {
  double mu = 0.0;
  for (int x = 0; x < S; ++x) mu = fmax(mu, -Q[x * S + x]);
  return mu;
}

// Workgroups [0, rpow_blocks): model m = id / S, row x = id % S of R and of every R^n.
// The others: one thread per (list entry, class) writes its Poisson terms.
__global__ void __launch_bounds__(64) smap_table_kernel(SmapArgs a) {
  __shared__ double sR[64 * 64];
  __shared__ double row[2][64];
  const int S = a.S, SS = a.S * a.S;
  if ((int)blockIdx.x < a.rpow_blocks) {
    const int m = blockIdx.x / S, x = blockIdx.x - m * S;
    const double* Q = a.Q + (size_t)m * SS;
    const double mu = smap_mu(Q, S);
    for (int e = threadIdx.x; e < SS; e += 64) {
      const int z = e / S, y = e - z * S;
      const double q = Q[e] / mu;
      sR[e] = z == y ? 1.0 + q : q;
    }
    __syncthreads();
    const int y = threadIdx.x;
    double* T = a.RpowT + (size_t)m * kSmapN1 * SS;
    if (y < S) {
      a.R[(size_t)m * SS + x * S + y] = sR[x * S + y];
      const double v = x == y ? 1.0 : 0.0;
      row[0][y] = v;
      T[y * S + x] = v;
    }
    __syncthreads();
    for (int n = 1; n <= kSmapMaxJumps; ++n) {
      const int cur = n & 1;
      if (y < S) {
        double s = 0.0;
        for (int z = 0; z < S; ++z) s = fma(row[cur ^ 1][z], sR[z * S + y], s);
        row[cur][y] = s;
        T[(size_t)n * SS + y * S + x] = s;
      }
      __syncthreads();
    }
  } else {
    const int id = ((int)blockIdx.x - a.rpow_blocks) * 64 + threadIdx.x;
    if (id >= a.n_list * a.C) return;
    const int e = id / a.C, c = id - e * a.C;
    const SmapEntry en = a.list[e];
    const double lam = smap_mu(a.Q + (size_t)en.model * SS, S) * a.rates[c] * en.t;
    double* out = a.pois + ((size_t)en.node * a.C + c) * kSmapN1;
    double p = exp(-lam);
    out[0] = p;
    for (int n = 1; n <= kSmapMaxJumps; ++n) {
      p = p * lam / (double)n;
      out[n] = p;
    }
  }
}

// A lane's uniforms of one stream (fourth counter word c3): the block of the last draw index is kept.
struct SmapGen {
  uint64_t site, replicate, seed, c3;
  uint64_t blk;
  SimBlock w;

  __device__ __forceinline__ void stream(uint64_t c3_) {
    c3 = c3_;
    blk = ~(uint64_t)0;
  }
  __device__ __forceinline__ double uniform(uint32_t k) {
    const uint64_t b = k >> 2;
    if (b != blk) {
      w = sim_philox(site, b, replicate, c3, seed, 0);
      blk = b;
    }
    const uint32_t j = k & 3u;
    const uint64_t x = j == 0 ? w.w0 : j == 1 ? w.w1 : j == 2 ? w.w2 : w.w3;
    return (double)(x >> 11) * 0x1.0p-53;
  }
};

// The weighted draw over w(0) .. w(n - 1): weights not > 0 count as 0, cum is the sequential sum,
// thr = u cum[n - 1]; the first y with thr < cum[y], else the largest y of positive weight (0: none).
template <class W>
__device__ __forceinline__ int smap_draw(int n, double u, W w) {
  double tot = 0.0;
  int last = 0;
  for (int y = 0; y < n; ++y) {
    const double v = w(y);
    if (v > 0.0) {
      tot = __dadd_rn(tot, v);
      last = y;
    }
  }
  const double thr = __dmul_rn(u, tot);
  double cum = 0.0;
  for (int y = 0; y < n; ++y) {
    const double v = w(y);
    if (v > 0.0) {
      cum = __dadd_rn(cum, v);
      if (thr < cum) return y;
    }
  }
  return last;
}

// One lane per site, looping over the call's replicates.  S_ > 0: the state count at compile time.
// LDS_: R and R^n of every model are first copied into LDS (4 states).
template <int S_, bool LDS_>
__global__ void __launch_bounds__(kSmapThreads) smap_sample_kernel(SmapArgs a) {
  extern __shared__ double smap_lds[];
  const int S = S_ ? S_ : a.S, SS = S * S;
  const int C = a.C, CS = C * S, T = a.T;
  const double* Rt = a.R;
  const double* Tt = a.RpowT;
  if (LDS_) {
    const int n_tab = a.n_models * kSmapN1 * SS, n_r = a.n_models * SS;
    for (int i = threadIdx.x; i < n_tab; i += kSmapThreads) smap_lds[i] = a.RpowT[i];
    for (int i = threadIdx.x; i < n_r; i += kSmapThreads) smap_lds[n_tab + i] = a.R[i];
    __syncthreads();
    Tt = smap_lds;
    Rt = smap_lds + n_tab;
  }
  const int64_t p = (int64_t)blockIdx.x * kSmapThreads + threadIdx.x;
  if (p >= a.n_patterns) return;  // padding sites draw and write nothing
  const int64_t np = a.n_pad;
  const int64_t tb = (p >> 7) * CS * kTile + (p & (kTile - 1));
  const int nn = a.n_nodes;
  // L_v[c][y] of the lane's pattern
  auto L = [&](int is_tip, int child, int c, int y) -> double {
    if (is_tip) return a.code_table[(size_t)a.codes[(size_t)child * np + p] * S + y];
    return a.partials[(int64_t)child * a.slot_stride + tb + ((int64_t)c * S + y) * kTile];
  };
  // class weights: the same for every replicate
  double wc[16];
  double ctot = 0.0;
  int clast = 0;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    wc[c] = 0.0;
    if (c < C) {
      double s = 0.0;
      for (int x = 0; x < S; ++x) s = __dadd_rn(s, __dmul_rn(a.pi[x], L(0, a.root_slot, c, x)));
      const double v = __dmul_rn(a.probs[c], s);
      if (v > 0.0) {
        wc[c] = v;
        ctot = __dadd_rn(ctot, v);
        clast = c;
      }
    }
  }
  const bool bad = !(ctot > 0.0 && ctot < __builtin_huge_val());
  unsigned long long n_bad = 0;
  SmapGen g, ge, go;  // ancestral draws; a path's even and odd draw indices
  g.site = ge.site = go.site = a.site0 + (uint64_t)p;
  g.seed = ge.seed = go.seed = a.seed;
  for (int r = 0; r < a.n_rep; ++r) {
    const int64_t kr = a.keep ? r : 0;
    uint8_t* st = a.states + kr * (nn + 1) * np + p;
    if (bad) {
      // states 255, counts and dwelling times 0; the sums are left alone
      st[(int64_t)nn * np] = 255;
      st[(int64_t)a.root * np] = 255;
      for (int i = 0; i < a.n_list; ++i) {
        const int v = a.list[i].node;
        st[(int64_t)v * np] = 255;
        if (a.keep) {
          const int64_t rb = kr * nn + v;
          a.jumps[rb * np + p] = 0;
          for (int k = 0; k < T; ++k) a.counts[(rb * T + k) * np + p] = 0;
          for (int s = 0; s < S; ++s) a.dwell[(rb * S + s) * np + p] = 0.0;
        }
      }
      ++n_bad;
      continue;
    }
    g.replicate = ge.replicate = go.replicate = a.replicate0 + (uint64_t)r;
    g.stream(1);
    int cls = clast;
    {
      const double thr = __dmul_rn(g.uniform(0), ctot);
      double cum = 0.0;
      bool found = false;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c < C && !found && wc[c] > 0.0) {
          cum = __dadd_rn(cum, wc[c]);
          if (thr < cum) {
            cls = c;
            found = true;
          }
        }
    }
    st[(int64_t)nn * np] = (uint8_t)cls;
    a.class_tally[(int64_t)cls * np + p] += 1;
    const int xr = smap_draw(S, g.uniform(1), [&](int y) { return __dmul_rn(a.pi[y], L(0, a.root_slot, cls, y)); });
    st[(int64_t)a.root * np] = (uint8_t)xr;
    a.state_tally[((int64_t)a.root * S + xr) * np + p] += 1;
    for (int i = 0; i < a.n_list; ++i) {
      const SmapEntry e = a.list[i];
      const int v = e.node;
      const int xa = st[(int64_t)e.father * np];
      const double* Prow = a.pmats + (((int64_t)v * C + cls) * S + xa) * S;
      const int xb = smap_draw(S, g.uniform(2u + (uint32_t)v),
                               [&](int y) { return __dmul_rn(Prow[y], L(e.is_tip, e.child, cls, y)); });
      st[(int64_t)v * np] = (uint8_t)xb;
      a.state_tally[((int64_t)v * S + xb) * np + p] += 1;
      // the path a -> b on branch v
      const int64_t rb = kr * nn + v;
      double* dw = a.dwell + (a.keep ? rb * S : 0) * np + p;
      uint16_t* cnt = a.keep ? a.counts + rb * T * np + p : nullptr;
      uint32_t* csum = a.count_sum + (int64_t)v * T * np + p;
      for (int s = 0; s < S; ++s) dw[(int64_t)s * np] = 0.0;
      if (cnt)
        for (int k = 0; k < T; ++k) cnt[(int64_t)k * np] = 0;
      ge.stream(2u + (uint64_t)v);
      go.stream(2u + (uint64_t)v);
      const double* Tm = Tt + (size_t)e.model * kSmapN1 * SS;
      const double* Rm = Rt + (size_t)e.model * SS;
      const double* po = a.pois + ((size_t)v * C + cls) * kSmapN1;
      int n = -1;
      {
        const double thr = __dmul_rn(ge.uniform(0), Prow[xb]);
        double cum = 0.0;
        int last = -1;
        for (int j = 0; j <= kSmapMaxJumps; ++j) {
          const double w = __dmul_rn(po[j], Tm[(size_t)j * SS + xb * S + xa]);
          if (w > 0.0) {
            cum = __dadd_rn(cum, w);
            last = j;
            if (thr < cum) {
              n = j;
              break;
            }
          }
        }
        if (n < 0) n = last;
        if (n < 0) {  // no positive term: stay, or the direct jump
          n = xa == xb ? 0 : 1;
          if (xa != xb) ++n_bad;
        }
      }
      if (a.keep) a.jumps[rb * np + p] = (uint16_t)n;
      if (n == 0) {
        dw[(int64_t)xa * np] = e.t;
      } else {
        double se = 0.0;
        for (int j = 0; j <= n; ++j) se = __dadd_rn(se, -log(1.0 - ge.uniform(2u * j + 2u)));
        int x = xa;
        for (int j = 0; j <= n; ++j) {
          if (j > 0) {
            int xn = xb;
            if (j < n) {
              const double* Rrow = Rm + x * S;
              const double* Tcol = Tm + (size_t)(n - j) * SS + xb * S;
              xn = smap_draw(S, go.uniform(2u * j - 1u), [&](int y) { return __dmul_rn(Rrow[y], Tcol[y]); });
            }
            if (xn != x) {
              const int ty = a.type_of[x * S + xn];
              if (ty) {
                csum[(int64_t)(ty - 1) * np] += 1;
                if (cnt) cnt[(int64_t)(ty - 1) * np] += 1;
              }
            }
            x = xn;
          }
          const double ej = -log(1.0 - ge.uniform(2u * j + 2u));
          const double d = __ddiv_rn(__dmul_rn(e.t, ej), se);
          dw[(int64_t)x * np] = __dadd_rn(dw[(int64_t)x * np], d);
        }
      }
      double* ds = a.dwell_sum + (int64_t)v * S * np + p;
      for (int s = 0; s < S; ++s) ds[(int64_t)s * np] = __dadd_rn(ds[(int64_t)s * np], dw[(int64_t)s * np]);
    }
  }
  if (n_bad) atomicAdd(a.n_bad, n_bad);
}

// Weighted totals of the count sums: one workgroup per (listed branch, type k, root block of
// kRootBlock patterns), all on grid.x; row = node * T + k.  Summed in fixed order, so the host's sum
// over blocks does not depend on the sharding.
__global__ void __launch_bounds__(256) smap_totals_kernel(const uint32_t* __restrict__ count_sum,
                                                          const double* __restrict__ weights, double* __restrict__ blk,
                                                          const SmapEntry* __restrict__ list, int T, int64_t n_pad,
                                                          int64_t n_patterns, int n_blocks) {
  __shared__ double red[4];
  const int64_t r = blockIdx.x / n_blocks, B = blockIdx.x - r * n_blocks;
  const int64_t row = (int64_t)list[r / T].node * T + r % T;
  double s = 0.0;
  for (int j = 0; j < kRootBlock / 256; ++j) {
    const int64_t p = B * kRootBlock + (int64_t)j * 256 + threadIdx.x;
    if (p < n_patterns) s += weights[p] * (double)count_sum[row * n_pad + p];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) blk[row * n_blocks + B] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace plk
