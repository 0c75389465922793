// plk_post.hpp -- marginal posteriors of internal nodes: ancestral states and rate classes.
//
// The reference forms them on the host from the double-recursive arrays
// (MarginalAncestralStateReconstruction::getAncestralStatesForNode,
// DRTreeLikelihoodTools::getPosteriorProbabilitiesForEachStateForEachRate,
// AbstractDiscreteRatesAcrossSitesTreeLikelihood::getPosteriorProbabilitiesOfEachRate).
// After the preorder pass of plk_dr.hpp HBM holds, for every internal node v, the lower
// partial L_v and the upper vector U_v (conditional on the state y at v's father), so per
// pattern
//     up_v[c][x] = sum_y u[c][y] P_v[c][y][x],   u = U_v (x pi_y where U_v leaves pi out),
//     J_v[c][x]  = p_c up_v[c][x] L_v[c][x]      (root: J_r[c][x] = p_c pi_x L_r[c][x]),
//     l          = sum_c sum_x J_v[c][x]         (the site likelihood, at every node),
// and the outputs are J / l, its two marginals and the argmax of the state marginal.  The
// power-of-two scale counts of L_v and U_v are per node and pattern, so they cancel in
// J / l and are never read.  A pattern whose l is not a positive finite number gets zeros
// and best_state 255.  Every output is a probability: a J that rounding of P(t) left a few
// ulps below 0 counts as 0, and a marginal that its sum left a few ulps above 1 as 1.
//
// One launch serves a chunk of nodes: grid = (pattern blocks, nodes).  Lanes run along
// patterns (every (class, state) row read is one contiguous KiB per wave) and the outputs
// are staged row-wise, [node][row][n_pad], so every store is coalesced as well; the host
// turns the rows into the caller's [pattern][...] order.
#pragma once

#include "plk_dr.hpp"

namespace plk {

struct PostNode {     // (field order is read as 8 int32 by post_s4_kernel)
  int32_t node;       // P index of the branch above v
  int32_t lslot;      // slot of L_v
  int32_t uslot;      // slot of U_v (the root: lslot, never read)
  int32_t use_pi;     // U_v leaves pi out (sons of the root after the levelwise preorder)
  int32_t is_root;
  int32_t pad_[3];
};

struct PostArgs {
  const double* partials;
  const double* pmats;
  const double* pi;
  const double* probs;
  double* joint;      // [node][C S][n_pad] or null
  double* spost;      // [node][S][n_pad] or null
  double* cpost;      // [node][C][n_pad] or null
  uint8_t* best;      // [node][n_pad] or null
  int64_t slot_stride;
  int64_t n_pad;
  int32_t C;
  int32_t n_blk;      // 64-pattern blocks (the MFMA kernel's loop bound)
  int32_t G;          // classes staged in LDS at a time (MFMA kernel)
};

constexpr int kPostThreads = 256;

__device__ __forceinline__ bool post_ok(double l) { return l > 0.0 && l <= 1.79769313486231570815e308; }

// S <= 4: one lane = one pattern, P_v[c] through the constant address space (scalar loads,
// as dr_pre_s4_kernel).  CT > 0: the class count is a compile-time constant -- the loads of
// all classes are issued before the arithmetic and J stays in registers, so every output
// comes from one pass.  CT = 0 (any other class count): a first pass over the classes forms
// l and the state sums, a second one (only when joint or class_post is asked for) forms J
// again and writes J / l.
template <int S, int CT>
__global__ __launch_bounds__(kPostThreads) void post_s4_kernel(const PostNode* __restrict__ nodes, PostArgs a) {
  typedef __attribute__((address_space(4))) const int32_t* PostCI;
  const PostCI w = (PostCI)(nodes + blockIdx.y);
  const int node = w[0], lslot = w[1], uslot = w[2], use_pi = w[3], is_root = w[4];
  const int C = CT ? CT : a.C;
  const int CS = C * S;
  const int64_t p = (int64_t)blockIdx.x * kPostThreads + threadIdx.x;
  const int64_t tb = (p >> 7) * CS * kTile + (p & (kTile - 1));
  const double* __restrict__ Lb = a.partials + (int64_t)lslot * a.slot_stride + tb;
  const double* __restrict__ Ub = a.partials + (int64_t)uslot * a.slot_stride + tb;
  double pi[S];
#pragma unroll
  for (int x = 0; x < S; ++x) pi[x] = ((DrCPd)a.pi)[x];
  // J of one class from its L and U rows
  auto term = [&](int c, const double (&L)[S], const double (&U)[S], double (&J)[S]) {
    const double pc = ((DrCPd)a.probs)[c];
    if (is_root) {
#pragma unroll
      for (int x = 0; x < S; ++x) J[x] = fmax(pc * pi[x] * L[x], 0.0);
    } else {
      const DrCPd P = (DrCPd)(a.pmats + ((int64_t)node * C + c) * S * S);
      double u[S];
#pragma unroll
      for (int y = 0; y < S; ++y) u[y] = use_pi ? U[y] * pi[y] : U[y];
#pragma unroll
      for (int x = 0; x < S; ++x) {
        double t = 0.0;
#pragma unroll
        for (int y = 0; y < S; ++y) t = fma(u[y], P[y * S + x], t);
        J[x] = fmax(pc * t * L[x], 0.0);
      }
    }
  };
  auto load = [&](int c, double (&L)[S], double (&U)[S]) {
#pragma unroll
    for (int x = 0; x < S; ++x) L[x] = Lb[((int64_t)c * S + x) * kTile];
    if (!is_root)
#pragma unroll
      for (int y = 0; y < S; ++y) U[y] = Ub[((int64_t)c * S + y) * kTile];
  };
  const int64_t nb = (int64_t)blockIdx.y * a.n_pad + p;
  double sp[S];
#pragma unroll
  for (int x = 0; x < S; ++x) sp[x] = 0.0;
  bool ok;
  if constexpr (CT > 0) {
    double L[CT][S], U[CT][S], J[CT][S];
#pragma unroll
    for (int c = 0; c < CT; ++c) load(c, L[c], U[c]);
    double l = 0.0;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      term(c, L[c], U[c], J[c]);
#pragma unroll
      for (int x = 0; x < S; ++x) l += J[c][x];
    }
    ok = post_ok(l);
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      double cs = 0.0;
#pragma unroll
      for (int x = 0; x < S; ++x) {
        const double r = ok ? J[c][x] / l : 0.0;
        sp[x] += r;
        cs += r;
        if (a.joint) a.joint[((int64_t)blockIdx.y * CS + c * S + x) * a.n_pad + p] = r;
      }
      if (a.cpost) a.cpost[((int64_t)blockIdx.y * C + c) * a.n_pad + p] = fmin(cs, 1.0);
    }
#pragma unroll
    for (int x = 0; x < S; ++x) sp[x] = fmin(sp[x], 1.0);
  } else {
    double l = 0.0;
    for (int c = 0; c < C; ++c) {
      double L[S], U[S], J[S];
      load(c, L, U);
      term(c, L, U, J);
#pragma unroll
      for (int x = 0; x < S; ++x) {
        sp[x] += J[x];
        l += J[x];
      }
    }
    ok = post_ok(l);
#pragma unroll
    for (int x = 0; x < S; ++x) sp[x] = ok ? fmin(sp[x] / l, 1.0) : 0.0;
    if (a.joint || a.cpost)
      for (int c = 0; c < C; ++c) {
        double L[S], U[S], J[S];
        load(c, L, U);
        term(c, L, U, J);
        double cs = 0.0;
#pragma unroll
        for (int x = 0; x < S; ++x) {
          const double r = ok ? J[x] / l : 0.0;
          cs += r;
          if (a.joint) a.joint[((int64_t)blockIdx.y * CS + c * S + x) * a.n_pad + p] = r;
        }
        if (a.cpost) a.cpost[((int64_t)blockIdx.y * C + c) * a.n_pad + p] = fmin(cs, 1.0);
      }
  }
  if (a.spost)
#pragma unroll
    for (int x = 0; x < S; ++x) a.spost[((int64_t)blockIdx.y * S + x) * a.n_pad + p] = sp[x];
  if (a.best) {
    int bi = 0;
    double bv = sp[0];
#pragma unroll
    for (int x = 1; x < S; ++x)
      if (sp[x] > bv) {  // (strict: the lowest index among the maxima)
        bv = sp[x];
        bi = x;
      }
    a.best[nb] = ok ? (uint8_t)bi : (uint8_t)255;
  }
}

// S = 20 / 64 on v_mfma_f64_16x16x4f64, the contraction of dr_branch_mfma_kernel turned
// round: up = P_v^T u is matvec_m with P_v as stored in the place of a child's P^T, so u is
// the B operand in treeM's layout (lane l holds states 16 xt + (l >> 4) + 4 r of pattern
// l & 15) and up comes out in the same layout, where it meets L_v lane by lane.  A wave
// owns 16 patterns, a workgroup 64; workgroups loop over a node's 64-pattern blocks and
// stage P_v once when all classes fit the launch's LDS.  Two passes over the classes as in
// the CT = 0 form above (the second only for joint / class_post).  Held to two waves per SIMD:
// left alone the 64-state build takes 302 registers (one wave) and ran cfg4 in 2.63 ms against
// 1.83 ms (246 VGPRs, no spill).
template <int S>
__global__ __launch_bounds__(kPostThreads) __attribute__((amdgpu_waves_per_eu(2))) void post_mfma_kernel(const PostNode* __restrict__ nodes, PostArgs a) {
  constexpr int XT = MShape<S>::XT;
  extern __shared__ double lds[];
  const PostNode nd = nodes[blockIdx.y];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int lr = lane >> 4, lc = lane & 15;
  const int C = a.C, CS = a.C * S;
  const bool two = a.joint || a.cpost;
  bool staged = false;
  for (int64_t blk = blockIdx.x; blk < a.n_blk; blk += gridDim.x) {
    const int64_t p = blk * 64 + 16 * g + lc;
    const int64_t tb = (p >> 7) * CS * kTile + (p & (kTile - 1));
    const double* Lb = a.partials + (int64_t)nd.lslot * a.slot_stride + tb;
    const double* Ub = a.partials + (int64_t)nd.uslot * a.slot_stride + tb;
    f64x4m sp[XT];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) sp[xt] = (f64x4m){0.0, 0.0, 0.0, 0.0};
    double l = 0.0;
    bool ok = false;
    for (int pass = 0; pass < (two ? 2 : 1); ++pass) {
      for (int c = 0; c < C; ++c) {
        const int cc = c % a.G;
        if (!nd.is_root && cc == 0 && !(staged && a.G == C)) {
          const int n = min(a.G, C - c) * S * S;
          staged = true;
          __syncthreads();  // the previous group's readers are done
          const double* src = a.pmats + ((size_t)nd.node * C + c) * S * S;
          for (int i = threadIdx.x; i < n; i += kPostThreads) lds[i] = src[i];
          __syncthreads();
        }
        const double pc = a.probs[c];
        f64x4m J[XT];
        if (nd.is_root) {
#pragma unroll
          for (int xt = 0; xt < XT; ++xt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int x = 16 * xt + lr + 4 * r;
              J[xt][r] = m_valid<S>(xt, r, lr) ? fmax(pc * a.pi[x] * Lb[(int64_t)(c * S + x) * kTile], 0.0) : 0.0;
            }
        } else {
          MAcc<S> u;
#pragma unroll
          for (int xt = 0; xt < XT; ++xt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int y = 16 * xt + lr + 4 * r;
              double v = m_valid<S>(xt, r, lr) ? Ub[(int64_t)(c * S + y) * kTile] : 0.0;
              if (nd.use_pi && m_valid<S>(xt, r, lr)) v *= a.pi[y];
              u[xt][r] = v;
            }
          f64x4m up[XT];
          matvec_m<S>(up, u, lds + cc * S * S, lr, lc);
#pragma unroll
          for (int xt = 0; xt < XT; ++xt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int x = 16 * xt + lr + 4 * r;
              J[xt][r] = m_valid<S>(xt, r, lr) ? fmax(pc * up[xt][r] * Lb[(int64_t)(c * S + x) * kTile], 0.0) : 0.0;
            }
        }
        if (pass == 0) {
#pragma unroll
          for (int xt = 0; xt < XT; ++xt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              sp[xt][r] += J[xt][r];
              l += J[xt][r];
            }
        } else {
          double cs = 0.0;
#pragma unroll
          for (int xt = 0; xt < XT; ++xt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (m_valid<S>(xt, r, lr)) {
                const double v = ok ? J[xt][r] / l : 0.0;
                cs += v;
                if (a.joint)
                  a.joint[((int64_t)blockIdx.y * CS + c * S + 16 * xt + lr + 4 * r) * a.n_pad + p] = v;
              }
          cs += __shfl_xor(cs, 16, 64);
          cs += __shfl_xor(cs, 32, 64);
          if (a.cpost && lr == 0) a.cpost[((int64_t)blockIdx.y * C + c) * a.n_pad + p] = fmin(cs, 1.0);
        }
      }
      if (pass == 0) {
        // a pattern's states are spread over the 4 lane rows (lr)
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        ok = post_ok(l);
        int bi = 255;
        double bv = -1.0;
#pragma unroll
        for (int xt = 0; xt < XT; ++xt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (m_valid<S>(xt, r, lr)) {
              const int x = 16 * xt + lr + 4 * r;
              const double v = ok ? fmin(sp[xt][r] / l, 1.0) : 0.0;
              if (a.spost) a.spost[((int64_t)blockIdx.y * S + x) * a.n_pad + p] = v;
              if (v > bv || (v == bv && x < bi)) {
                bv = v;
                bi = x;
              }
            }
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
          const double ov = __shfl_xor(bv, off, 64);
          const int oi = __shfl_xor(bi, off, 64);
          if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
          }
        }
        if (a.best && lr == 0) a.best[(int64_t)blockIdx.y * a.n_pad + p] = ok ? (uint8_t)bi : (uint8_t)255;
      }
    }
    // (G < C: the staged matrices are restaged by the next block, behind its own barrier)
  }
}

// The same pass for S = 20 / 64 on the VALU (PLK_TUNE POST_VALU=1; the A/B partner of
// post_mfma_kernel): one lane = one pattern, 256 patterns per workgroup, P_v of one
// class staged in LDS and read as wave-wide broadcasts (every lane the same address), u and the
// state sums in registers, four states' dot products in flight.
template <int S>
__global__ __launch_bounds__(kPostThreads) void post_valu_kernel(const PostNode* __restrict__ nodes, PostArgs a) {
  extern __shared__ double lds[];  // P_v[c], [y][x]
  const PostNode nd = nodes[blockIdx.y];
  const int C = a.C, CS = a.C * S;
  const int64_t p = (int64_t)blockIdx.x * kPostThreads + threadIdx.x;
  const int64_t tb = (p >> 7) * CS * kTile + (p & (kTile - 1));
  const double* Lb = a.partials + (int64_t)nd.lslot * a.slot_stride + tb;
  const double* Ub = a.partials + (int64_t)nd.uslot * a.slot_stride + tb;
  const bool two = a.joint || a.cpost;
  double sp[S];
#pragma unroll
  for (int x = 0; x < S; ++x) sp[x] = 0.0;
  double l = 0.0;
  bool ok = false;
  for (int pass = 0; pass < (two ? 2 : 1); ++pass) {
    for (int c = 0; c < C; ++c) {
      if (!nd.is_root) {
        __syncthreads();  // the previous class's readers are done
        const double* src = a.pmats + ((size_t)nd.node * C + c) * S * S;
        for (int i = threadIdx.x; i < S * S; i += kPostThreads) lds[i] = src[i];
        __syncthreads();
      }
      const double pc = a.probs[c];
      double u[S];
      if (!nd.is_root)
#pragma unroll
        for (int y = 0; y < S; ++y) u[y] = nd.use_pi ? Ub[(int64_t)(c * S + y) * kTile] * a.pi[y] : Ub[(int64_t)(c * S + y) * kTile];
      double cs = 0.0;
#pragma unroll
      for (int x0 = 0; x0 < S; x0 += 4) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (nd.is_root) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = a.pi[x0 + k];
        } else {
#pragma unroll
          for (int y = 0; y < S; ++y)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fma(u[y], lds[y * S + x0 + k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double J = fmax(pc * acc[k] * Lb[(int64_t)(c * S + x0 + k) * kTile], 0.0);
          if (pass == 0) {
            sp[x0 + k] += J;
            l += J;
          } else {
            const double v = ok ? J / l : 0.0;
            cs += v;
            if (a.joint) a.joint[((int64_t)blockIdx.y * CS + c * S + x0 + k) * a.n_pad + p] = v;
          }
        }
      }
      if (pass == 1 && a.cpost) a.cpost[((int64_t)blockIdx.y * C + c) * a.n_pad + p] = fmin(cs, 1.0);
    }
    if (pass == 0) {
      ok = post_ok(l);
      int bi = 0;
      double bv = -1.0;
#pragma unroll
      for (int x = 0; x < S; ++x) {
        const double v = ok ? fmin(sp[x] / l, 1.0) : 0.0;
        if (a.spost) a.spost[((int64_t)blockIdx.y * S + x) * a.n_pad + p] = v;
        if (v > bv) {
          bv = v;
          bi = x;
        }
      }
      if (a.best) a.best[(int64_t)blockIdx.y * a.n_pad + p] = ok ? (uint8_t)bi : (uint8_t)255;
    }
  }
}

}  // namespace plk
