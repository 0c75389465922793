// plk_sim.hpp -- simulation of alignments (plk_simulate): the reference's
// NonHomogeneousSequenceSimulator (Simulation/NonHomogeneousSequenceSimulator.cpp: the per-site
// walk :306-353, the inverse-CDF draw :433-483, the cumulative tables of its constructor :110-160)
// with a counter-based generator in the place of the sequential RandomTools stream.
//
// A draw is a pure function of (seed, replicate, global site, draw index k): word k & 3 of
// Philox4x64-10 (Salmon et al. 2011) at counter (site, k >> 2, replicate, 0) and key (seed, 0), its
// upper 53 bits times 2^-53.  k = 0 draws the site's rate class, 1 the root state, 2 + v the state
// of node v.  So no result depends on the launch geometry, on sharding or on the order of the list.
//
// sim_cdf_kernel turns the handle's P[node][c][x][.] (and the class probabilities and pi) into
// cumulative rows, summed sequentially in fp64, with the fallback index of each row: the largest y
// with p[y] > 0, taken where no cumulative value exceeds u (rounding, rows that do not sum to 1).
// sim_walk_kernel runs the whole tree, one lane per site: the list of (node, father) is the same for
// every lane (uniform addresses: scalar loads), a lane reads back only the states it wrote itself
// (one byte per site and node, coalesced over sites), and finds the first y with u < cum[y] by a
// binary search over the monotone row -- the answer of the definition's linear scan.  For 4 states
// a workgroup of 1024 lanes first copies the tables into LDS where two copies fit a CU (64 taxa
// and 4 classes: 73 KB) and searches there.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace plk {

constexpr int kSimThreads = 256;
constexpr int kSimLdsThreads = 1024;         // lanes of a workgroup that stages the tables in LDS
constexpr size_t kSimLdsMax = 80 * 1024;     // its table bytes at most: two workgroups per CU

struct SimArgs {
  const double* pmats;   // [node][C][S][S]
  const double* probs;   // [C]
  const double* pi;      // [S]
  double* cdf;           // [node][C][S][S] cumulative rows
  int32_t* fb;           // [node][C][S] fallback index of each row
  double* cdf_cls;       // [C], then its fallback as a double
  double* cdf_root;      // [S], then its fallback as a double
  const int2* list;      // (node, father) in preorder, fathers first
  int32_t n_list;
  int32_t S, C;
  int32_t root, n_tips;
  uint8_t* states;       // [n_nodes + 1][n_pad]; row n_nodes holds the classes
  int32_t n_nodes;
  uint8_t* codes;        // [n_tips][n_pad] compact tip codes, or null: tips are not written
  const uint8_t* code_of_state;  // [S] compact code of each state
  int64_t n_pad, n_patterns;
  uint64_t seed, replicate, site0;
};

// cum[y] = cum[y - 1] + p[y]; returns the largest y with p[y] > 0 (0: none)
__device__ __forceinline__ int sim_cum_row(const double* __restrict__ p, double* __restrict__ cum, int n) {
  double s = 0.0;
  int last = 0;
  for (int y = 0; y < n; ++y) {
    const double v = p[y];
    s = y == 0 ? v : s + v;
    cum[y] = s;
    if (v > 0.0) last = y;
  }
  return last;
}

// One thread per row (list entry, class, father's state); two more for the class and root rows.
__global__ void __launch_bounds__(kSimThreads) sim_cdf_kernel(SimArgs a) {
  const int rows = a.n_list * a.C * a.S;
  const int t = blockIdx.x * kSimThreads + threadIdx.x;
  if (t < rows) {
    const int e = t / (a.C * a.S), r = t - e * (a.C * a.S);
    const int64_t row = (int64_t)a.list[e].x * a.C * a.S + r;
    a.fb[row] = sim_cum_row(a.pmats + row * a.S, a.cdf + row * a.S, a.S);
  } else if (t == rows) {
    a.cdf_cls[a.C] = (double)sim_cum_row(a.probs, a.cdf_cls, a.C);
  } else if (t == rows + 1) {
    a.cdf_root[a.S] = (double)sim_cum_row(a.pi, a.cdf_root, a.S);
  }
}

struct SimBlock {
  uint64_t w0, w1, w2, w3;
};

__device__ __forceinline__ SimBlock sim_philox(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0, uint64_t k1) {
  constexpr uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
  constexpr uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t hi0 = __umul64hi(M0, c0), lo0 = M0 * c0;
    const uint64_t hi1 = __umul64hi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return SimBlock{c0, c1, c2, c3};
}

// The lane's generator: the block of the last draw index is kept, so the draws k of one block
// (k >> 2 equal) cost one evaluation.  k is the same in every lane: the branch is uniform.
struct SimLane {
  uint64_t site, replicate, seed;
  uint64_t blk;
  SimBlock w;

  __device__ __forceinline__ double uniform(uint32_t k) {
    const uint64_t b = k >> 2;
    if (b != blk) {
      w = sim_philox(site, b, replicate, 0, seed, 0);
      blk = b;
    }
    const uint32_t j = k & 3u;
    const uint64_t x = j == 0 ? w.w0 : j == 1 ? w.w1 : j == 2 ? w.w2 : w.w3;
    return (double)(x >> 11) * 0x1.0p-53;
  }
};

// first y in [0, n) with u < cum[y]; fb where there is none
__device__ __forceinline__ int sim_search(const double* __restrict__ cum, int n, double u, int fb) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (u < cum[mid])
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo < n ? lo : fb;
}

// One lane per site.  S_ > 0: the state count at compile time (4, 20, 64); 0: read from the args.
// LDS_: the workgroup (kSimLdsThreads lanes) first copies the cumulative rows and fallback indices
// of every node into LDS and searches there; the host takes it where two workgroups' tables fit
// a CU (kSimLdsMax bytes each), so the occupancy stays what the plain kernel has.
template <int S_, bool LDS_>
__global__ void __launch_bounds__(LDS_ ? kSimLdsThreads : kSimThreads) sim_walk_kernel(SimArgs a) {
  extern __shared__ double sim_lds[];
  const int S = S_ ? S_ : a.S;
  const int C = a.C;
  const double* cdf = a.cdf;
  const int32_t* fbt = a.fb;
  if (LDS_) {
    const int n_fb = a.n_nodes * C * S, n_tab = n_fb * S;
    int32_t* lfb = reinterpret_cast<int32_t*>(sim_lds + n_tab);
    for (int i = threadIdx.x; i < n_tab; i += kSimLdsThreads) sim_lds[i] = a.cdf[i];
    for (int i = threadIdx.x; i < n_fb; i += kSimLdsThreads) lfb[i] = a.fb[i];
    __syncthreads();
    cdf = sim_lds;
    fbt = lfb;
  }
  const int64_t p = (int64_t)blockIdx.x * (LDS_ ? kSimLdsThreads : kSimThreads) + threadIdx.x;
  if (p >= a.n_patterns) return;  // padding sites draw and write nothing
  SimLane g;
  g.site = a.site0 + (uint64_t)p;
  g.replicate = a.replicate;
  g.seed = a.seed;
  g.blk = ~(uint64_t)0;
  const int c = sim_search(a.cdf_cls, C, g.uniform(0), (int)a.cdf_cls[C]);
  a.states[(int64_t)a.n_nodes * a.n_pad + p] = (uint8_t)c;
  const int xr = sim_search(a.cdf_root, S, g.uniform(1), (int)a.cdf_root[S]);
  a.states[(int64_t)a.root * a.n_pad + p] = (uint8_t)xr;
  for (int i = 0; i < a.n_list; ++i) {
    const int2 e = a.list[i];
    const int v = e.x;
    const int xf = a.states[(int64_t)e.y * a.n_pad + p];
    const int64_t row = ((int64_t)v * C + c) * S + xf;
    const int x = sim_search(cdf + row * S, S, g.uniform(2u + (uint32_t)v), fbt[row]);
    a.states[(int64_t)v * a.n_pad + p] = (uint8_t)x;
    if (a.codes && v < a.n_tips) a.codes[(int64_t)v * a.n_pad + p] = a.code_of_state[x];
  }
}

}  // namespace plk
