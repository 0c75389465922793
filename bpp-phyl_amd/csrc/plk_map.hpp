// plk_map.hpp -- probabilistic substitution mapping: the posterior expected number of
// substitutions of each type, on each branch, at each pattern.
//
// The reference forms them on the host (SubstitutionMappingTools::computeSubstitutionVectors,
// Mapping/SubstitutionMappingTools.cpp:63-372, over DecompositionSubstitutionCount /
// DecompositionMethods, Mapping/DecompositionMethods.cpp:88-165) as a six-deep loop
// node x site x class x x x y x type.  Here a type k of a model is a matrix B_k (B_k[x][y] =
// Q[x][y] where x -> y belongs to the type, 0 elsewhere and on the diagonal) and, with
// tau = r_c t_v and the model's real eigen system (V, Vinv, lambda),
//     G_k       = Vinv B_k V                                            (once per model and type)
//     J[i][j]   = int_0^tau exp(lambda_i s) exp(lambda_j (tau - s)) ds
//     W^k_{v,c} = V (J o G_k) Vinv = int_0^tau e^{Qs} B_k e^{Q(tau-s)} ds
// so W^k[x][y] = E[count of type k, end state y | start state x] (the reference's
// getAllNumbersOfSubstitutions(tau, k)[x][y] * P(tau)[x][y]).  After the preorder pass of
// plk_dr.hpp HBM holds L_v and U_v of every branch, and per branch, pattern and type
//     l   = sum_c p_c sum_xy u[c][x] P_v[c][x][y]   L_v[c][y]
//     n_k = sum_c p_c sum_xy u[c][x] W^k_{v,c}[x][y] L_v[c][y],      count = n_k / l,
// u = U_v (x pi at the root's sons where U_v leaves pi out): the bilinear form of the
// derivative reduction with a count matrix in the place of dP, read out per pattern.  The
// scale counts of U_v and L_v multiply n_k and l alike and are never read.  A pattern whose
// l is not a positive finite number gets counts 0.
//
// J is formed as tau exp(max(lambda_i, lambda_j) tau) phi(-|lambda_i - lambda_j| tau) with
// phi(z) = expm1(z) / z, phi(0) = 1 (J is symmetric in i, j): no cancellation for nearly equal
// eigenvalues and no overflow, where the reference's (e_i - e_j) / (lambda_i - lambda_j) with
// an exact == 0 test loses every digit for eigenvalues an ulp apart.  An entry of W that
// rounding leaves below 0 is stored as 0.
#pragma once

#include "plk_post.hpp"

namespace plk {

constexpr int kMapMaxTypes = 16;

struct CountMatArgs {
  const double* t;         // [n_req]
  const int32_t* branch;   // [n_req]
  const int32_t* model;    // [n_req] or null (model 0)
  const double* rates;
  const double* V;
  const double* Vinv;
  const double* lambda;
  const double* G;         // [model][T][S][S]
  double* W;               // [node][T][C][S][S]
  int32_t S, C, T, n_req;
};

__device__ __forceinline__ double map_J(double li, double lj, double tau) {
  const double z = -fabs(li - lj) * tau;
  const double phi = z == 0.0 ? 1.0 : expm1(z) / z;
  return tau * exp(fmax(li, lj) * tau) * phi;
}

// Any state count: one workgroup per (branch, class).  J (the same for every type) and the
// inner product (J o G_k) Vinv sit in LDS, 2 S^2 doubles (64 KiB at 64 states, so V, Vinv and
// G_k are read through the caches instead of being staged beside them).
__global__ __launch_bounds__(256) void count_matrix_kernel(CountMatArgs a) {
  extern __shared__ double lds[];
  const int S = a.S, SS = a.S * a.S;
  double* sJ = lds;
  double* sT = lds + SS;
  const int i0 = blockIdx.x, c = blockIdx.y;
  const int b = a.branch[i0], m = a.model ? a.model[i0] : 0;
  const double tau = a.t[i0] * a.rates[c];
  const double* lam = a.lambda + (size_t)m * S;
  const double* V = a.V + (size_t)m * SS;
  const double* Vi = a.Vinv + (size_t)m * SS;
  for (int e = threadIdx.x; e < SS; e += blockDim.x) {
    const int i = e / S, j = e - i * S;
    sJ[e] = map_J(lam[i], lam[j], tau);
  }
  __syncthreads();
  for (int k = 0; k < a.T; ++k) {
    const double* G = a.G + ((size_t)m * a.T + k) * SS;
    for (int e = threadIdx.x; e < SS; e += blockDim.x) {
      const int i = e / S, y = e - i * S;
      double s = 0.0;
      for (int j = 0; j < S; ++j) s = fma(sJ[i * S + j] * G[i * S + j], Vi[j * S + y], s);
      sT[e] = s;
    }
    __syncthreads();
    double* W = a.W + (((size_t)b * a.T + k) * a.C + c) * SS;
    for (int e = threadIdx.x; e < SS; e += blockDim.x) {
      const int x = e / S, y = e - x * S;
      double s = 0.0;
      for (int i = 0; i < S; ++i) s = fma(V[x * S + i], sT[i * S + y], s);
      W[e] = fmax(s, 0.0);
    }
    __syncthreads();  // sT is rewritten by the next type
  }
}

// S <= 4 in the style of pmat4_kernel: one thread per output row (request, class, x), J and
// the row's products in registers, no LDS and no barrier.
template <int S>
__global__ __launch_bounds__(64) void count_matrix4_kernel(CountMatArgs a) {
  const int id = blockIdx.x * 64 + threadIdx.x;
  if (id >= a.n_req * a.C * S) return;
  const int x = id % S, c = (id / S) % a.C, i0 = id / (S * a.C);
  const int b = a.branch[i0], m = a.model ? a.model[i0] : 0;
  const double tau = a.t[i0] * a.rates[c];
  const double* lam = a.lambda + (size_t)m * S;
  const double* V = a.V + (size_t)m * S * S;
  const double* Vi = a.Vinv + (size_t)m * S * S;
  double J[S][S], vx[S], vi[S][S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    vx[i] = V[x * S + i];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      J[i][j] = j < i ? J[j][i] : map_J(lam[i], lam[j], tau);
      vi[i][j] = Vi[i * S + j];
    }
  }
  for (int k = 0; k < a.T; ++k) {
    const double* G = a.G + ((size_t)m * a.T + k) * S * S;
    double* W = a.W + ((((size_t)b * a.T + k) * a.C + c) * S + x) * S;
    double r[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < S; ++j) s = fma(vx[j] * J[j][i], G[j * S + i], s);  // (v_x (J o G_k))[i]
      r[i] = s;
    }
#pragma unroll
    for (int y = 0; y < S; ++y) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < S; ++i) s = fma(r[i], vi[i][y], s);
      W[y] = fmax(s, 0.0);
    }
  }
}

struct MapBranch {    // (field order is read as 8 int32 by map_s4_kernel)
  int32_t node;       // branch = child node index (P and W index)
  int32_t is_tip;     // L_v from the tip's codes
  int32_t child;      // tip index or internal slot of v
  int32_t uslot;      // slot of U_v
  int32_t use_pi;     // U_v leaves pi out
  int32_t pad_[3];
};

struct MapArgs {
  const double* partials;
  const uint8_t* codes;       // compact codes [tip][n_pad]
  const double* code_table;   // compact table [n_codes][S]
  const double* pmats;
  const double* wmats;        // [node][T][C][S][S]
  const double* pi;
  const double* probs;
  const double* weights;
  double* counts;             // [branch][T][n_pad] or null
  double* blk;                // [branch][T][n_blk] sums of w count per workgroup pass, or null
  int64_t slot_stride;
  int64_t n_pad;
  int64_t n_patterns;
  int32_t C;
  int32_t T;
  int32_t n_blk;              // 256-pattern (map_s4_kernel) or 64-pattern (map_mfma_kernel) blocks
  int32_t G;                  // matrices staged in LDS at a time (map_mfma_kernel)
};

constexpr int kMapThreads = 256;

// S <= 4: one lane = one pattern, P_v[c] and W^k_v[c] through the constant address space
// (scalar loads, as post_s4_kernel).  Types run in the outer loop, so a pattern holds one
// accumulator at a time whatever T is.  CT > 0: the class count is a compile-time constant and
// L, u of every class stay in registers over the types; CT = 0 reads them again per type.
template <int S, int CT>
__global__ __launch_bounds__(kMapThreads) void map_s4_kernel(const MapBranch* __restrict__ branches, MapArgs a) {
  typedef __attribute__((address_space(4))) const int32_t* MapCI;
  __shared__ double red[kMapMaxTypes][kMapThreads / 64];
  const MapCI w = (MapCI)(branches + blockIdx.y);
  const int node = w[0], is_tip = w[1], child = w[2], uslot = w[3], use_pi = w[4];
  const int C = CT ? CT : a.C;
  const int CS = C * S;
  constexpr int NC = CT ? CT : 1;
  const int64_t p = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
  const bool live = p < a.n_patterns;
  const int64_t tb = (p >> 7) * CS * kTile + (p & (kTile - 1));
  const double* __restrict__ Lb = a.partials + (int64_t)(is_tip ? 0 : child) * a.slot_stride + tb;
  const double* __restrict__ Ub = a.partials + (int64_t)uslot * a.slot_stride + tb;
  const double* __restrict__ row = a.code_table + (size_t)(is_tip ? a.codes[(size_t)child * a.n_pad + p] : 0) * S;
  auto load = [&](int c, double (&L)[S], double (&u)[S]) {
#pragma unroll
    for (int y = 0; y < S; ++y) L[y] = is_tip ? row[y] : Lb[((int64_t)c * S + y) * kTile];
#pragma unroll
    for (int x = 0; x < S; ++x) {
      const double v = Ub[((int64_t)c * S + x) * kTile];
      u[x] = use_pi ? v * ((DrCPd)a.pi)[x] : v;
    }
  };
  // p_c u^T M L for one class
  auto form = [&](const double* Mg, int c, const double (&L)[S], const double (&u)[S]) {
    const DrCPd M = (DrCPd)(Mg + (int64_t)c * S * S);
    double s = 0.0;
#pragma unroll
    for (int x = 0; x < S; ++x) {
      double z = 0.0;
#pragma unroll
      for (int y = 0; y < S; ++y) z = fma(M[x * S + y], L[y], z);
      s = fma(u[x], z, s);
    }
    return ((DrCPd)a.probs)[c] * s;
  };
  double L[NC][S], u[NC][S];
  if constexpr (CT > 0) {
#pragma unroll
    for (int c = 0; c < CT; ++c) load(c, L[c], u[c]);
  }
  auto all_classes = [&](const double* Mg) {
    double s = 0.0;
    if constexpr (CT > 0) {
#pragma unroll
      for (int c = 0; c < CT; ++c) s += form(Mg, c, L[c], u[c]);
    } else {
      for (int c = 0; c < C; ++c) {
        load(c, L[0], u[0]);
        s += form(Mg, c, L[0], u[0]);
      }
    }
    return s;
  };
  const double l = all_classes(a.pmats + (int64_t)node * C * S * S);
  const bool ok = live && post_ok(l);
  const double wt = live ? a.weights[p] : 0.0;
  for (int k = 0; k < a.T; ++k) {
    const double n = all_classes(a.wmats + ((int64_t)node * a.T + k) * C * S * S);
    const double cnt = ok ? fmax(n, 0.0) / l : 0.0;
    if (a.counts) a.counts[((int64_t)blockIdx.y * a.T + k) * a.n_pad + p] = cnt;
    if (a.blk) {
      double r = ok ? wt * cnt : 0.0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
      if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = r;
    }
  }
  if (a.blk) {
    __syncthreads();
    if (threadIdx.x < a.T) {
      double t = 0.0;
      for (int i = 0; i < kMapThreads / 64; ++i) t += red[threadIdx.x][i];  // fixed order
      a.blk[((int64_t)blockIdx.y * a.T + threadIdx.x) * a.n_blk + blockIdx.x] = t;
    }
  }
}

// S = 20 / 64 on v_mfma_f64_16x16x4f64 in the layout of dr_branch_mfma_kernel: L_v of the
// wave's 16 patterns is the B operand, z = M L comes out of matvec_m lane by lane beside u, and
// u . z closes with the two cross-lane adds over the four lane rows.  The matrices of a branch
// are numbered m = c (T + 1) + kk with kk = 0 for P_v and kk = k + 1 for W^k_v; they are staged
// transposed in LDS G at a time, once per workgroup when all of them fit the launch's LDS (a
// workgroup loops over the branch's 64-pattern blocks), else again per block.  Classes run in
// the outer loop, so L and u of a class are read once and stay in registers over P and every
// type; l and the n_k of a pattern accumulate in LDS (one slot per pattern and kk, written and
// read by the pattern's first lane row only -- a register array indexed by kk would go to
// scratch).  First form: types outside, L and u read again per type -- cfg3 32.8 ms, cfg4
// 6.96 ms at T = 1 against the figures of DESIGN 5.
template <int S>
__global__ __launch_bounds__(kMapThreads) __attribute__((amdgpu_waves_per_eu(2))) void map_mfma_kernel(const MapBranch* __restrict__ branches, MapArgs a) {
  constexpr int XT = MShape<S>::XT;
  extern __shared__ double lds[];
  __shared__ double red[kMapMaxTypes][kMapThreads / 64];
  __shared__ double acc[kMapMaxTypes + 1][64];  // l and n_k of the workgroup's 64 patterns
  const MapBranch b = branches[blockIdx.y];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int lr = lane >> 4, lc = lane & 15;
  const int C = a.C, CS = a.C * S, NM = (a.T + 1) * a.C;
  bool staged = false;
  for (int64_t blk = blockIdx.x; blk < a.n_blk; blk += gridDim.x) {
    const int64_t p = blk * 64 + 16 * g + lc;
    const bool live = p < a.n_patterns;
    const int64_t tb = (p >> 7) * CS * kTile + (p & (kTile - 1));
    const double* Lb = a.partials + (int64_t)(b.is_tip ? 0 : b.child) * a.slot_stride + tb;
    const double* Ub = a.partials + (int64_t)b.uslot * a.slot_stride + tb;
    const double* row = a.code_table + (size_t)(b.is_tip ? a.codes[(size_t)b.child * a.n_pad + p] : 0) * S;
    const double wt = live ? a.weights[p] : 0.0;
    const int pl = 16 * g + lc;
    if (lr == 0)
      for (int kk = 0; kk <= a.T; ++kk) acc[kk][pl] = 0.0;
    for (int c = 0; c < C; ++c) {
      MAcc<S> src;
      double uu[XT][4];
#pragma unroll
      for (int xt = 0; xt < XT; ++xt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int y = 16 * xt + lr + 4 * r;
          const bool v = m_valid<S>(xt, r, lr);
          src[xt][r] = !v ? 0.0 : b.is_tip ? row[y] : Lb[(int64_t)(c * S + y) * kTile];
          const double u = v ? Ub[(int64_t)(c * S + y) * kTile] : 0.0;
          uu[xt][r] = v && b.use_pi ? u * a.pi[y] : u;
        }
      const double pc = a.probs[c];
      for (int kk = 0; kk <= a.T; ++kk) {
        const int m = c * (a.T + 1) + kk, mm = m % a.G;
        if (mm == 0 && !(staged && a.G == NM)) {
          const int cnt = min(a.G, NM - m);
          staged = true;
          __syncthreads();  // the previous group's readers are done
          for (int i = threadIdx.x; i < cnt * S * S; i += kMapThreads) {
            const int j = (m + i / (S * S)), e = i % (S * S);
            const int jc = j / (a.T + 1), jk = j - jc * (a.T + 1);
            const double* from = jk == 0 ? a.pmats + ((size_t)b.node * C + jc) * S * S
                                         : a.wmats + (((size_t)b.node * a.T + jk - 1) * C + jc) * S * S;
            const int x = e / S, y = e - x * S;  // source [x][y] -> LDS [y][x]
            lds[(size_t)(i / (S * S)) * S * S + y * S + x] = from[e];
          }
          __syncthreads();
        }
        f64x4m z[XT];
        matvec_m<S>(z, src, lds + (size_t)mm * S * S, lr, lc);
        double s = 0.0;
#pragma unroll
        for (int xt = 0; xt < XT; ++xt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (m_valid<S>(xt, r, lr)) s = fma(uu[xt][r], z[xt][r], s);
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (lr == 0) acc[kk][pl] = fma(pc, s, acc[kk][pl]);
      }
    }
    const double l = lr == 0 ? acc[0][pl] : 0.0;
    const bool ok = live && lr == 0 && post_ok(l);
    for (int k = 0; k < a.T; ++k) {
      const double cnt = ok ? fmax(acc[k + 1][pl], 0.0) / l : 0.0;
      if (a.counts && lr == 0) a.counts[((int64_t)blockIdx.y * a.T + k) * a.n_pad + p] = cnt;
      if (a.blk) {
        double r = ok ? wt * cnt : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
        if (lane == 0) red[k][g] = r;
      }
    }
    if (a.blk) {
      __syncthreads();
      if (threadIdx.x < a.T) {
        double t = 0.0;
        for (int i = 0; i < kMapThreads / 64; ++i) t += red[threadIdx.x][i];  // fixed order
        a.blk[((int64_t)blockIdx.y * a.T + threadIdx.x) * a.n_blk + blk] = t;
      }
      __syncthreads();  // red[] is rewritten by the next block
    }
  }
}

// Workgroup sums -> sums per root block (kRootBlock patterns, `per` workgroup sums each), in
// fixed order: out[row][B] for row = branch * T + k.
__global__ __launch_bounds__(256) void map_blocks_kernel(const double* __restrict__ blk, double* __restrict__ out,
                                                         int n_rows, int n_blk, int per, int n_out) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= n_rows * n_out) return;
  const int r = id / n_out, B = id - r * n_out;
  double t = 0.0;
  for (int i = B * per; i < min((B + 1) * per, n_blk); ++i) t += blk[(size_t)r * n_blk + i];
  out[id] = t;
}

}  // namespace plk
