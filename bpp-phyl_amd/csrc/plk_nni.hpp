// plk_nni.hpp -- nearest-neighbour interchanges scored on the device, the length of the
// move's branch re-estimated.
//
// The reference scores one move at a time on the host (NNIHomogeneousTreeLikelihood::testNNI,
// Likelihood/NNIHomogeneousTreeLikelihood.cpp:205-309: two conditional arrays per site, class
// and state, then Brent over BranchLikelihood, :93-120) and NNITopologySearch calls it for every
// eligible node of every round.  A move is (son s, uncle u): p is the father of s, g the father
// of p, u another son of g; s and u change places and the length t of branch p is estimated
// again.  With q_v = P_v L_v (a tip: P_v times its code row) and, per pattern and class,
//     up_g = pi at the root, else sum_y u_g[y] P_g[y][x],  u_g = U_g (x pi where U_g leaves it out),
//     A1 = up_g q_s prod_{o son of g, o not p, u} q_o        (at g, swapped tree)
//     A2 = q_u prod_{o son of p, o not s} q_o                (at p, swapped tree)
//     B1 = up_g q_u prod_{o}  q_o,   B2 = q_s prod_{o} q_o   (the same for the current tree)
//     l_cur = sum_c p_c B1^T P_p B2,
// the real eigen system (V, Vinv, lambda) of the model of branch p gives
//     gamma[c][k] = p_c (sum_x A1[x] V[x][k]) (sum_y Vinv[k][y] A2[y])
//     rho(t)      = (1 / l_cur) sum_c sum_k gamma[c][k] exp(lambda_k r_c t)
// and Delta(t) = sum_patterns w log rho(t) = lnL(swapped tree, t) - lnL(current tree).  l_cur and
// gamma are built from the same stored vectors, so their power-of-two scale factors cancel and
// the scale counts are never read (the rule of plk_dr.hpp, plk_post.hpp, plk_map.hpp).
//
// That holds while the product of the stored vectors is a normal double.  Under PLK_FLAG_SCALING
// each stored vector has its joint maximum anywhere in [2^-256, 1) (lower after a three-son op
// of small sons: one factor 2^256 per op), and l_cur multiplies four of them on a binary tree
// (U_g, L_s, L_u, the other son of p) and six at trifurcations: the product reached 0 and the
// pattern was dropped without a word (1 / l_cur = 0: it added 0 to every sum, and its site row
// was 0.0).  So the build first takes an exact power of two out of each vector -- 2^-e, e the
// exponent of its joint maximum over classes and states (nni_pow2) -- which puts every maximum
// in [1, 2).  l_cur, gamma and d share the factor, 1 / l_cur carries its inverse, and powers of
// two are exact: wherever nothing underflowed before, every result is bitwise what it was.
//
// nni_coef_* pay the matrix-vector products once per move and store the rows
// [move][c S + k][n_pad] of gamma plus two rows: 1 / l_cur (0 where l_cur is not a positive
// finite number) -- l_cur needs every class before any gamma can be divided, and the extra row
// keeps the build at one pass over the classes with a handful of live registers for any class
// count -- and d = sum_c p_c A1 . A2 = sum_ck gamma[c][k], a sum of non-negative terms.
// nni_eval_kernel then streams the rows once per trial length: rho, rho', rho'' and the
// workgroup sums of w log rho, w rho'/rho, w (rho''/rho - (rho'/rho)^2), and a fourth sum, the
// change of w log rho against the move's accepted point, formed per pattern from
// rho(t) - rho(t_acc) (see nni_eval_kernel).  A pattern whose rho is not a positive finite
// number adds 0 to all of them.
//
// Short lengths.  Where the two sides of the move disagree rho(t) is small against the gamma it
// is summed from (rho(0) = d), and sum gamma exp(.) loses what d, formed without a
// subtraction, keeps: on 20 states at t = 1e-6 the plain sum left 6e-9 per unit weight in d1.
// So while t max|lambda_k r_c| <= 1 a move is evaluated as rho = d + sum gamma expm1(lambda r t)
// (the same number in exact arithmetic); longer lengths, where exp(.) has damped the terms that
// cancel, keep the plain sum.  The switch depends on the move's t alone.
#pragma once

#include "plk_map.hpp"

namespace plk {

struct NniKid {       // a subtree hanging off g or p
  int32_t kind;       // 0: internal, 1: tip (L from the codes), 2: absent
  int32_t child;      // tip index or internal slot
  int32_t node;       // P index
};

struct NniMove {      // (read as 24 int32 by nni_coef_s4_kernel)
  NniKid k[5];        // s, u, the third son of g, the other sons of p (one or two)
  int32_t g_node;     // P index of the branch above g
  int32_t g_uslot;    // slot of U_g
  int32_t g_root;     // g is the root: up_g = pi
  int32_t g_pi;       // U_g leaves pi out
  int32_t p_node;     // P index of branch p
  int32_t model;      // eigen system of branch p
  int32_t pad_[3];
};

struct NniArgs {
  const double* partials;
  const uint8_t* codes;       // compact codes [tip][n_pad]
  const double* code_table;   // compact table [n_codes][S]
  const double* pmats;
  const double* pmatsT;       // (MFMA kernel)
  const double* V;            // [model][S][S]
  const double* Vinv;         // [model][S][S]; the MFMA kernel gets the transposed copy
  const double* pi;
  const double* probs;
  double* coef;               // [move][C S + kNniExtra][n_pad]
  int64_t slot_stride;
  int64_t n_pad;
  int32_t C;
  int32_t n_blk;              // 64-pattern blocks (the MFMA kernel's loop bound)
};

constexpr int kNniThreads = 256;
constexpr int kNniExtra = 2;  // rows after gamma: 1 / l_cur, d

// 2^-e for a joint maximum m in [2^e, 2^(e+1)); 1 for a vector of zeros (or anything not finite)
__device__ __forceinline__ double nni_pow2(double m) {
  if (!(m > 0.0 && m <= 1.79769313486231570815e308)) return 1.0;
  const int e = ilogb(m);
  return ldexp(1.0, e < -1000 ? 1000 : -e);
}

// S <= 4: one lane = one pattern, the move record and every matrix through the constant
// address space (scalar loads, as map_s4_kernel).  CT > 0: the class count is a compile-time
// constant and the class loop is unrolled, so the loads of all classes are in flight together.
template <int S, int CT>
__global__ __launch_bounds__(kNniThreads) void nni_coef_s4_kernel(const NniMove* __restrict__ moves, NniArgs a) {
  typedef __attribute__((address_space(4))) const int32_t* NniCI;
  const NniCI w = (NniCI)(moves + blockIdx.y);
  const int g_node = w[15], g_uslot = w[16], g_root = w[17], g_pi = w[18], p_node = w[19], model = w[20];
  const int C = CT ? CT : a.C;
  const int CS = C * S;
  const int64_t p = (int64_t)blockIdx.x * kNniThreads + threadIdx.x;
  const int64_t tb = (p >> 7) * CS * kTile + (p & (kTile - 1));
  const DrCPd V = (DrCPd)(a.V + (int64_t)model * S * S);
  const DrCPd Vi = (DrCPd)(a.Vinv + (int64_t)model * S * S);
  // the power of two taken out of each vector: sc[j] for subtree j, sc[5] for U_g
  double sc[6];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int kind = w[3 * j], child = w[3 * j + 1];
    double m = 0.0;
    if (kind == 1) {
      const double* __restrict__ row = a.code_table + (size_t)a.codes[(size_t)child * a.n_pad + p] * S;
#pragma unroll
      for (int y = 0; y < S; ++y) m = fmax(m, row[y]);
    } else if (kind == 0) {
      const double* __restrict__ Lb = a.partials + (int64_t)child * a.slot_stride + tb;
      for (int e = 0; e < CS; ++e) m = fmax(m, Lb[(int64_t)e * kTile]);
    }
    sc[j] = nni_pow2(m);
  }
  {
    double m = 0.0;
    if (!g_root) {
      const double* __restrict__ Ub = a.partials + (int64_t)g_uslot * a.slot_stride + tb;
      for (int e = 0; e < CS; ++e) m = fmax(m, Ub[(int64_t)e * kTile]);
    }
    sc[5] = nni_pow2(m);
  }
  // q = P_v L_v of subtree j for class c
  auto q = [&](int j, int c, double (&r)[S]) {
    const int kind = w[3 * j], child = w[3 * j + 1], node = w[3 * j + 2];
    double L[S];
    if (kind == 1) {
      const double* __restrict__ row = a.code_table + (size_t)a.codes[(size_t)child * a.n_pad + p] * S;
#pragma unroll
      for (int y = 0; y < S; ++y) L[y] = row[y] * sc[j];
    } else {
      const double* __restrict__ Lb = a.partials + (int64_t)child * a.slot_stride + tb;
#pragma unroll
      for (int y = 0; y < S; ++y) L[y] = Lb[((int64_t)c * S + y) * kTile] * sc[j];
    }
    const DrCPd P = (DrCPd)(a.pmats + ((int64_t)node * C + c) * S * S);
#pragma unroll
    for (int x = 0; x < S; ++x) {
      double z = 0.0;
#pragma unroll
      for (int y = 0; y < S; ++y) z = fma(P[x * S + y], L[y], z);
      r[x] = z;
    }
  };
  double* __restrict__ out = a.coef + (int64_t)blockIdx.y * (CS + kNniExtra) * a.n_pad + p;
  double l = 0.0, d = 0.0;
  auto one_class = [&](int c) {
    double up[S], qs[S], qu[S], b2[S], t[S];
    if (g_root) {
#pragma unroll
      for (int x = 0; x < S; ++x) up[x] = ((DrCPd)a.pi)[x];
    } else {
      const double* __restrict__ Ub = a.partials + (int64_t)g_uslot * a.slot_stride + tb;
      const DrCPd Pg = (DrCPd)(a.pmats + ((int64_t)g_node * C + c) * S * S);
      double u[S];
#pragma unroll
      for (int y = 0; y < S; ++y) {
        const double v = Ub[((int64_t)c * S + y) * kTile] * sc[5];
        u[y] = g_pi ? v * ((DrCPd)a.pi)[y] : v;
      }
#pragma unroll
      for (int x = 0; x < S; ++x) {
        double z = 0.0;
#pragma unroll
        for (int y = 0; y < S; ++y) z = fma(u[y], Pg[y * S + x], z);
        up[x] = z;
      }
    }
    if (w[6] != 2) {
      q(2, c, t);
#pragma unroll
      for (int x = 0; x < S; ++x) up[x] *= t[x];
    }
    q(0, c, qs);
    q(1, c, qu);
    q(3, c, b2);
    if (w[12] != 2) {
      q(4, c, t);
#pragma unroll
      for (int x = 0; x < S; ++x) b2[x] *= t[x];
    }
    const double pc = ((DrCPd)a.probs)[c];
    // l_cur: B1^T P_p B2
    const DrCPd Pp = (DrCPd)(a.pmats + ((int64_t)p_node * C + c) * S * S);
    double s = 0.0;
#pragma unroll
    for (int x = 0; x < S; ++x) {
      double z = 0.0;
#pragma unroll
      for (int y = 0; y < S; ++y) z = fma(Pp[x * S + y], qs[y] * b2[y], z);
      s = fma(up[x] * qu[x], z, s);
    }
    l = fma(pc, s, l);
    double dd = 0.0;
#pragma unroll
    for (int x = 0; x < S; ++x) dd = fma(up[x] * qs[x], qu[x] * b2[x], dd);
    d = fma(pc, dd, d);
#pragma unroll
    for (int k = 0; k < S; ++k) {
      double a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int x = 0; x < S; ++x) {
        a1 = fma(up[x] * qs[x], V[x * S + k], a1);
        a2 = fma(Vi[k * S + x], qu[x] * b2[x], a2);
      }
      out[((int64_t)c * S + k) * a.n_pad] = pc * a1 * a2;
    }
  };
  if constexpr (CT > 0) {
#pragma unroll
    for (int c = 0; c < CT; ++c) one_class(c);
  } else {
    for (int c = 0; c < C; ++c) one_class(c);
  }
  out[(int64_t)CS * a.n_pad] = post_ok(l) ? 1.0 / l : 0.0;
  out[(int64_t)(CS + 1) * a.n_pad] = d;
}

// S = 20 / 64 on v_mfma_f64_16x16x4f64 in the layout of dr_branch_mfma_kernel / map_mfma_kernel:
// a lane (lr, lc) holds the states 16 xt + lr + 4 r of the wave's pattern lc, matvec_m maps that
// layout onto itself, so the products chain without a shuffle.  Sixteen patterns per wave,
// classes in the outer loop, a workgroup loops over the move's 64-pattern blocks.  Every
// matrix is staged in LDS for its product, one at a time (P^T from the transposed copy; P_g
// itself and V are the "transposed" operands of up_g = P_g^T u and a1 = V^T A1; Vinv comes in
// transposed): read straight from global memory the 64-state build clustered the operand
// loads of a whole product and spilled 1.6 KB per lane.
template <int S>
__global__ __launch_bounds__(kNniThreads) __attribute__((amdgpu_waves_per_eu(S == 64 ? 1 : 2))) void nni_coef_mfma_kernel(const NniMove* __restrict__ moves, NniArgs a) {
  constexpr int XT = MShape<S>::XT;
  extern __shared__ double lds[];
  const NniMove mv = moves[blockIdx.y];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int lr = lane >> 4, lc = lane & 15;
  const int C = a.C, CS = a.C * S;
  const double* V = a.V + (size_t)mv.model * S * S;
  const double* ViT = a.Vinv + (size_t)mv.model * S * S;
  // d = M^T-staged matvec: the matrix goes through LDS, one at a time (every branch around a
  // call is uniform over the workgroup: the move, the block loop and the class loop are)
  auto mvs = [&](f64x4m (&d)[XT], const MAcc<S>& src, const double* M) {
    __syncthreads();  // the previous matrix's readers are done
    for (int i = threadIdx.x; i < S * S; i += kNniThreads) lds[i] = M[i];
    __syncthreads();
    matvec_m<S>(d, src, lds, lr, lc);
  };
  for (int64_t blk = blockIdx.x; blk < a.n_blk; blk += gridDim.x) {
    const int64_t p = blk * 64 + 16 * g + lc;
    const int64_t tb = (p >> 7) * CS * kTile + (p & (kTile - 1));
    // the power of two taken out of each vector (see the head of this file): sc[j] for subtree
    // j, sc[5] for U_g; the joint maximum of a pattern is spread over its four lanes
    double sc[6];
    for (int j = 0; j < 6; ++j) {
      const int kind = j < 5 ? mv.k[j].kind : mv.g_root ? 2 : 0;
      const double* row = a.code_table + (size_t)(kind == 1 ? a.codes[(size_t)mv.k[j].child * a.n_pad + p] : 0) * S;
      const double* Lb = a.partials + (int64_t)(kind == 1 ? 0 : j < 5 ? mv.k[j].child : mv.g_uslot) * a.slot_stride + tb;
      double m = 0.0;
      if (kind != 2)
        for (int c = 0; c < (kind == 1 ? 1 : C); ++c)
#pragma unroll
          for (int xt = 0; xt < XT; ++xt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int y = 16 * xt + lr + 4 * r;
              if (m_valid<S>(xt, r, lr)) m = fmax(m, kind == 1 ? row[y] : Lb[(int64_t)(c * S + y) * kTile]);
            }
      m = fmax(m, __shfl_xor(m, 16, 64));
      m = fmax(m, __shfl_xor(m, 32, 64));
      sc[j] = nni_pow2(m);
    }
    // q = P_v L_v of subtree j for class c
    auto q = [&](int j, int c, f64x4m (&d)[XT]) {
      const NniKid kd = mv.k[j];
      MAcc<S> src;
      const double* row = a.code_table + (size_t)(kd.kind == 1 ? a.codes[(size_t)kd.child * a.n_pad + p] : 0) * S;
      const double* Lb = a.partials + (int64_t)(kd.kind == 1 ? 0 : kd.child) * a.slot_stride + tb;
#pragma unroll
      for (int xt = 0; xt < XT; ++xt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int y = 16 * xt + lr + 4 * r;
          src[xt][r] = !m_valid<S>(xt, r, lr) ? 0.0 : (kd.kind == 1 ? row[y] : Lb[(int64_t)(c * S + y) * kTile]) * sc[j];
        }
      mvs(d, src, a.pmatsT + ((size_t)kd.node * C + c) * S * S);
    };
    double l = 0.0, d = 0.0;
    double* out = a.coef + (int64_t)blockIdx.y * (CS + kNniExtra) * a.n_pad + p;
    for (int c = 0; c < C; ++c) {
      // (the order keeps at most six state vectors of the pattern alive, the operand of a
      // product included: 64 states hold 32 registers each)
      f64x4m up[XT], b2[XT], w1[XT], w2[XT], z[XT];
      if (mv.g_root) {
#pragma unroll
        for (int xt = 0; xt < XT; ++xt)
#pragma unroll
          for (int r = 0; r < 4; ++r) up[xt][r] = m_valid<S>(xt, r, lr) ? a.pi[16 * xt + lr + 4 * r] : 0.0;
      } else {
        const double* Ub = a.partials + (int64_t)mv.g_uslot * a.slot_stride + tb;
#pragma unroll
        for (int xt = 0; xt < XT; ++xt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int y = 16 * xt + lr + 4 * r;
            const bool v = m_valid<S>(xt, r, lr);
            const double u = v ? Ub[(int64_t)(c * S + y) * kTile] * sc[5] : 0.0;
            w1[xt][r] = v && mv.g_pi ? u * a.pi[y] : u;
          }
        mvs(up, w1, a.pmats + ((size_t)mv.g_node * C + c) * S * S);
      }
      if (mv.k[2].kind != 2) {
        q(2, c, w1);
#pragma unroll
        for (int xt = 0; xt < XT; ++xt) up[xt] *= w1[xt];
      }
      q(3, c, b2);
      if (mv.k[4].kind != 2) {
        q(4, c, w1);
#pragma unroll
        for (int xt = 0; xt < XT; ++xt) b2[xt] *= w1[xt];
      }
      const double pc = a.probs[c];
      q(0, c, w1);  // q_s
#pragma unroll
      for (int xt = 0; xt < XT; ++xt) w2[xt] = w1[xt] * b2[xt];  // B2
      mvs(z, w2, a.pmatsT + ((size_t)mv.p_node * C + c) * S * S);
#pragma unroll
      for (int xt = 0; xt < XT; ++xt) {
        z[xt] *= up[xt];   // up_g (*) (P_p B2): B1^T (P_p B2) = q_u . z
        w1[xt] *= up[xt];  // A1
        w2[xt] *= up[xt];  // up_g (*) B2: A1 . A2 = q_u . w2
      }
      mvs(up, w1, V);  // a1 (up_g itself is done)
      q(1, c, w1);     // q_u
      double s = 0.0, dd = 0.0;
#pragma unroll
      for (int xt = 0; xt < XT; ++xt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (m_valid<S>(xt, r, lr)) {
            s = fma(w1[xt][r], z[xt][r], s);
            dd = fma(w1[xt][r], w2[xt][r], dd);
          }
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      dd += __shfl_xor(dd, 16, 64);
      dd += __shfl_xor(dd, 32, 64);
      l = fma(pc, s, l);
      d = fma(pc, dd, d);
#pragma unroll
      for (int xt = 0; xt < XT; ++xt) w1[xt] *= b2[xt];  // A2
      mvs(z, w1, ViT);  // a2
#pragma unroll
      for (int xt = 0; xt < XT; ++xt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (m_valid<S>(xt, r, lr)) out[((int64_t)c * S + 16 * xt + lr + 4 * r) * a.n_pad] = pc * up[xt][r] * z[xt][r];
    }
    if (lr == 0) {
      out[(int64_t)CS * a.n_pad] = post_ok(l) ? 1.0 / l : 0.0;
      out[(int64_t)(CS + 1) * a.n_pad] = d;
    }
  }
}

// Vinv^T of every model, for the MFMA build
__global__ __launch_bounds__(256) void nni_transpose_kernel(const double* __restrict__ in, double* __restrict__ out, int S) {
  const double* src = in + (size_t)blockIdx.x * S * S;
  double* dst = out + (size_t)blockIdx.x * S * S;
  for (int e = threadIdx.x; e < S * S; e += 256) dst[(e % S) * S + e / S] = src[e];
}

struct NniEvalArgs {
  const double* coef;         // [move][CS + kNniExtra][n_pad]
  const double* weights;
  const int32_t* idx;         // [n_act] move of the chunk
  const int32_t* model;       // [n_act]
  const double* t;            // [n_act] trial lengths, then [n_act] the lengths of the accepted points
  const double* rates;
  const double* lambda;       // [model][S]
  double* ex;                 // [n_act][4 CS + 2]: E_j, lambda_k r_c, A_j, X_j, f, fa (nni_expo_kernel)
  double* blk;                // [n_act][kNniSums][n_blk] workgroup sums
  int64_t n_pad;
  int64_t n_patterns;
  int32_t S, C;
  int32_t n_blk;              // kNniThreads-pattern blocks
  int32_t n_act;
};

constexpr int kNniSums = 4;  // w log rho, w rho'/rho, w (rho''/rho - (rho'/rho)^2), w log(rho(t) / rho(t_acc))

// The exponentials and lambda_k r_c per active move: wave-uniform in nni_eval_kernel.  With
// mu = lambda_k r_c: exp(mu t) = E + f, where f = 1 and E = expm1(.) while t max|mu| <= 1 (the
// short-length form), else f = 0; exp(mu t_acc) = A + fa in the same way for the accepted
// point; X = expm1(mu (t - t_acc)).
__global__ __launch_bounds__(64) void nni_expo_kernel(NniEvalArgs a) {
  const int CS = a.C * a.S;
  const int id = blockIdx.x * 64 + threadIdx.x;
  if (id >= a.n_act * CS) return;
  const int i = id / CS, j = id - i * CS;
  const int c = j / a.S, k = j - c * a.S;
  const double* lam = a.lambda + (size_t)a.model[i] * a.S;
  double lmax = 0.0, rmax = 0.0;
  for (int q = 0; q < a.S; ++q) lmax = fmax(lmax, fabs(lam[q]));
  for (int q = 0; q < a.C; ++q) rmax = fmax(rmax, fabs(a.rates[q]));
  const double t = a.t[i], ta = a.t[a.n_act + i];
  const bool small = t * lmax * rmax <= 1.0, small_a = ta * lmax * rmax <= 1.0;
  const double mu = lam[k] * a.rates[c];
  double* ex = a.ex + (size_t)i * (4 * CS + 2);
  ex[j] = small ? expm1(mu * t) : exp(mu * t);
  ex[CS + j] = mu;
  ex[2 * CS + j] = small_a ? expm1(mu * ta) : exp(mu * ta);
  ex[3 * CS + j] = expm1(mu * (t - ta));
  if (j == 0) {
    ex[4 * CS] = small ? 1.0 : 0.0;
    ex[4 * CS + 1] = small_a ? 1.0 : 0.0;
  }
}

// Grid = (pattern blocks, active moves), one lane = one pattern: one pass over the move's rows
// gives rho, rho', rho'' at the trial length and, from the same rows, rho at the accepted
// point and rho(t) - rho(t_acc) = sum gamma exp(mu t_acc) expm1(mu (t - t_acc)).  The fourth
// sum, w log1p((rho(t) - rho(t_acc)) / rho(t_acc)), is F(t) - F(t_acc) without the
// cancellation of two sums of logs: near the optimum a Newton step changes F by less than
// the rounding of F itself, and whether the step is accepted is decided on this sum.
__global__ __launch_bounds__(kNniThreads) void nni_eval_kernel(NniEvalArgs a) {
  __shared__ double red[kNniSums][kNniThreads / 64];
  const int CS = a.C * a.S;
  const int mv = ((__attribute__((address_space(4))) const int32_t*)a.idx)[blockIdx.y];
  const DrCPd ex = (DrCPd)(a.ex + (size_t)blockIdx.y * (4 * CS + 2));
  const double f = ex[4 * CS], fa = ex[4 * CS + 1];
  const int64_t p = (int64_t)blockIdx.x * kNniThreads + threadIdx.x;
  const bool live = p < a.n_patterns;
  const double* __restrict__ row = a.coef + (int64_t)mv * (CS + kNniExtra) * a.n_pad + p;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, ra = 0.0, dr = 0.0;
  for (int j = 0; j < CS; ++j) {
    const double mu = ex[CS + j], g = row[(int64_t)j * a.n_pad];
    const double ge = g * (ex[j] + f);
    r0 = fma(g, ex[j], r0);
    r1 = fma(ge, mu, r1);
    r2 = fma(ge * mu, mu, r2);
    ra = fma(g, ex[2 * CS + j], ra);
    dr = fma(g * (ex[2 * CS + j] + fa), ex[3 * CS + j], dr);
  }
  const double d = row[(int64_t)(CS + 1) * a.n_pad], inv_l = row[(int64_t)CS * a.n_pad];
  r0 = fma(f, d, r0);
  ra = fma(fa, d, ra);
  const double rho = r0 * inv_l;
  const bool ok = live && post_ok(rho);
  const bool ok_a = ok && post_ok(ra * inv_l);
  const double wt = live ? a.weights[p] : 0.0;
  const double g1 = ok ? r1 / r0 : 0.0, g2 = ok ? r2 / r0 : 0.0;
  const double q = ok_a ? dr / ra : 0.0;
  // (a ratio far from 1 has nothing to cancel: the plain quotient there)
  const double dl = !ok_a ? 0.0 : q > -0.5 ? log1p(q) : log(r0 / ra);
  double v[kNniSums] = {ok ? wt * log(rho) : 0.0, wt * g1, wt * (g2 - g1 * g1), wt * dl};
#pragma unroll
  for (int i = 0; i < kNniSums; ++i) {
    double r = v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
    if ((threadIdx.x & 63) == 0) red[i][threadIdx.x >> 6] = r;
  }
  __syncthreads();
  if (threadIdx.x < kNniSums) {
    double t = 0.0;
    for (int i = 0; i < kNniThreads / 64; ++i) t += red[threadIdx.x][i];  // fixed order
    a.blk[((int64_t)blockIdx.y * kNniSums + threadIdx.x) * a.n_blk + blockIdx.x] = t;
  }
}

}  // namespace plk
