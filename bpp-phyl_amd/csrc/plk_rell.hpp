// plk_rell.hpp -- RELL resampling (resampling of estimated log-likelihoods): site rows kept on
// the device, replicate weights, and their product on fp64 matrix cores.
//
// The reference (PairedSiteLikelihoods::computeExpectedLikelihoodWeights,
// Likelihood/PairedSiteLikelihoods.cpp:124-176) runs a triple host loop: for every replicate and
// every model, Y += lnL[model][site] * count[site] over all sites.  That is G = W . L^T with
// K = sites.  Here a site row is a device vector of n_pad doubles (padding 0.0), the weights are
// [replicate][n_pad] (padding 0.0), and
//     G[r][m] = sum_p W[r][p] row[m][p],   Gabs[r][m] = sum_p |W[r][p]| |row[m][p]|.
//
// Summation rule (no element's bits depend on sharding, chunking, or the place of a replicate or
// row in the call):
//   1. per plk_block_size() = 4096 patterns a partial starts from +0.0 and takes the block's
//      patterns by fused multiply-add in this order: the block's 32-pattern segments ascending;
//      inside a segment q = 0..7; inside q the patterns 32 seg + 8 k + q for k = 0, 1, 2, 3 (the
//      K slots of one v_mfma_f64_16x16x4f64: lane (k, i) holds the 8 consecutive patterns
//      32 seg + 8 k .. + 7 of its replicate / row, one 64-byte run, and feeds element q to the
//      q-th MFMA of the segment).  Padding patterns are part of the chain (they add +0.0).
//   2. the partials of an element are added in global block order, one chain from +0.0.
//
// rell_partial_kernel is the split-K GEMM of step 1: a workgroup of four waves owns a tile of
// 64 replicates x 64 rows of one block, wave (wr, wm) the 32 x 32 quarter -- two A fragments
// (W), two B fragments (rows), four accumulator tiles.  Every fragment is loaded straight from
// global memory, 4 x 16 bytes per lane and segment, the next segment's loads issued before the
// 32 MFMAs of the current one.  Rows past the chunk's replicates / rows are zero fragments and
// are never read.  rell_chain_kernel is step 2, seeded (a later shard continues the chain of the
// one before it).
#pragma once

#include "plk_nni.hpp"

namespace plk {

constexpr int kRellThreads = 256;
constexpr int kRellTile = 64;   // replicates and rows of a workgroup's tile
constexpr int kRellSeg = 32;    // patterns of a segment: 8 MFMAs of K = 4

struct RellArgs {
  const double* W;      // first replicate of the chunk, [Rc][n_pad]
  const double* rows;   // first row of the chunk, [Mc][n_pad]
  double* part;         // [n_blk][Rc][Mc]
  double* part_abs;     // the same of the absolute values (ABS)
  int64_t n_pad;
  int32_t Rc, Mc;
};

typedef double rell_f64x2 __attribute__((ext_vector_type(2)));

// eight consecutive doubles of a lane's run (src == nullptr: a zero fragment)
__device__ __forceinline__ void rell_load(double (&d)[8], const double* __restrict__ src) {
  if (src) {
    const rell_f64x2* s = reinterpret_cast<const rell_f64x2*>(src);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const rell_f64x2 v = s[i];
      d[2 * i] = v[0];
      d[2 * i + 1] = v[1];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = 0.0;
  }
}

template <bool ABS>
__global__ __launch_bounds__(kRellThreads) void rell_partial_kernel(RellArgs a) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane >> 4, lc = lane & 15;
  const int rep0 = blockIdx.y * kRellTile + 32 * (w >> 1);
  const int row0 = blockIdx.x * kRellTile + 32 * (w & 1);
  const int64_t p0 = (int64_t)blockIdx.z * kRootBlock;
  const int n_seg = (int)(min((int64_t)kRootBlock, a.n_pad - p0) / kRellSeg);
  // the lane's run of segment 0 in its two replicates and two rows (null: past the chunk)
  const double* pa[2];
  const double* pb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rep = rep0 + 16 * i + lc, row = row0 + 16 * i + lc;
    pa[i] = rep < a.Rc ? a.W + (int64_t)rep * a.n_pad + p0 + 8 * lr : nullptr;
    pb[i] = row < a.Mc ? a.rows + (int64_t)row * a.n_pad + p0 + 8 * lr : nullptr;
  }
  f64x4m acc[2][2], abs_acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      acc[i][j] = (f64x4m){0.0, 0.0, 0.0, 0.0};
      abs_acc[i][j] = (f64x4m){0.0, 0.0, 0.0, 0.0};
    }
  double fa[2][8], fb[2][8], na[2][8], nb[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    rell_load(fa[i], pa[i]);
    rell_load(fb[i], pb[i]);
  }
  for (int seg = 0; seg < n_seg; ++seg) {
    const bool more = seg + 1 < n_seg;  // uniform: never a read past the block
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rell_load(na[i], more && pa[i] ? pa[i] + (int64_t)(seg + 1) * kRellSeg : nullptr);
      rell_load(nb[i], more && pb[i] ? pb[i] + (int64_t)(seg + 1) * kRellSeg : nullptr);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i][q], fb[j][q], acc[i][j], 0, 0, 0);
          if (ABS)
            abs_acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fabs(fa[i][q]), fabs(fb[j][q]), abs_acc[i][j], 0, 0, 0);
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        fa[i][q] = na[i][q];
        fb[i][q] = nb[i][q];
      }
  }
  // D[replicate lr + 4 r][row lc] of every accumulator tile
  const int64_t base = (int64_t)blockIdx.z * a.Rc * a.Mc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rep = rep0 + 16 * i + lr + 4 * r, row = row0 + 16 * j + lc;
        if (rep < a.Rc && row < a.Mc) {
          a.part[base + (int64_t)rep * a.Mc + row] = acc[i][j][r];
          if (ABS) a.part_abs[base + (int64_t)rep * a.Mc + row] = abs_acc[i][j][r];
        }
      }
}

// out[e] = seed[e] (null: +0.0) + part[0][e] + part[1][e] + ..., one thread per element
__global__ __launch_bounds__(256) void rell_chain_kernel(const double* __restrict__ part, const double* __restrict__ seed,
                                                         double* __restrict__ out, int64_t n_elem, int n_blk) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_elem) return;
  double s = seed ? seed[e] : 0.0;
  for (int b = 0; b < n_blk; ++b) s += part[(int64_t)b * n_elem + e];
  out[e] = s;
}

// row[p] = site[p] where it is finite, else 0.0 (padding: 0.0); the non-finite values of every
// workgroup are counted into bad[workgroup]
__global__ __launch_bounds__(256) void rell_row_from_site_kernel(const double* __restrict__ site, double* __restrict__ row,
                                                                 int32_t* __restrict__ bad, int64_t n_patterns) {
  __shared__ int32_t cnt[4];
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < n_patterns;
  const double v = live ? site[p] : 0.0;
  const bool ok = fabs(v) <= 1.79769313486231570815e308;  // false for NaN and +-inf
  row[p] = ok ? v : 0.0;
  const unsigned long long m = __ballot(live && !ok);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) bad[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// The sibling of nni_eval_kernel that stores: row[first + blockIdx.y][p] = log rho(t) of the
// move idx[blockIdx.y], formed exactly as nni_eval_kernel forms the term it weights and sums
// (the same fma chain over the same exponentials of nni_expo_kernel, the short-length form under
// the same condition); 0.0 where rho is not a positive finite number, and in the padding.
__global__ __launch_bounds__(kNniThreads) void nni_rows_kernel(NniEvalArgs a, double* __restrict__ rows) {
  const int CS = a.C * a.S;
  const int mv = ((__attribute__((address_space(4))) const int32_t*)a.idx)[blockIdx.y];
  const DrCPd ex = (DrCPd)(a.ex + (size_t)blockIdx.y * (4 * CS + 2));
  const double f = ex[4 * CS];
  const int64_t p = (int64_t)blockIdx.x * kNniThreads + threadIdx.x;
  const bool live = p < a.n_patterns;
  const double* __restrict__ row = a.coef + (int64_t)mv * (CS + kNniExtra) * a.n_pad + p;
  double r0 = 0.0;
  for (int j = 0; j < CS; ++j) r0 = fma(row[(int64_t)j * a.n_pad], ex[j], r0);
  const double d = row[(int64_t)(CS + 1) * a.n_pad], inv_l = row[(int64_t)CS * a.n_pad];
  r0 = fma(f, d, r0);
  const double rho = r0 * inv_l;
  rows[(int64_t)blockIdx.y * a.n_pad + p] = live && post_ok(rho) ? log(rho) : 0.0;
}

}  // namespace plk
