// plk_pars.hpp -- Fitch parsimony (plk_pars_*): the reference's DRTreeParsimonyScore
// (Parsimony/DRTreeParsimonyScore.cpp) as integer kernels.  A pair is (set, score): the set a bit
// mask over the parsimony states, the score the changes counted below (or around) the edge.  The
// only operation is the reference's sequential fold (:276-311): add the scores, intersect the
// sets, and where the intersection is empty take the union and count one change.
//
// Storage: 2 * n_internal arrays over n_pad patterns, array `slot` the lower pair of internal node
// n_tips + slot and array n_internal + slot its upper pair; sets of 1, 4 or 8 bytes (by state
// count), scores of 16 bits (a score is at most the number of folds, so trees of more than 65535
// nodes are rejected).  Tip sets are not stored: the code byte indexes the mask table in LDS.
//
// pars_update_kernel runs the whole tree in one launch: a lane owns its patterns from the first op
// to the last and reads back only what it wrote itself, so the ops need no barrier between them.
// The op program is the same for every lane (uniform addresses: scalar loads).  With 1-byte sets a
// lane takes four consecutive patterns as one dword of sets and one 8-byte load of scores.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace plk {

constexpr int kParsThreads = 256;
constexpr int kParsMaxIn = 8;  // inputs of one fold of a move

// An input or output of a fold: kind in the top bits, index below.
enum { kParsTip = 0, kParsArr = 1, kParsGf = 3 };
constexpr int kParsKindShift = 28;
constexpr int32_t kParsIdxMask = (1 << kParsKindShift) - 1;
__host__ __device__ inline int32_t pars_ref(int kind, int idx) { return (int32_t)(kind << kParsKindShift) | idx; }

// The op program is a stream of int32: per op [output array, n inputs, input refs ...].

// A move with its inputs resolved: gf = F(gf[0 .. n_gf)), pp = F(pp[0 .. n_pp)) where the ref of
// kind kParsGf stands for gf.
struct ParsMove {
  int32_t n_gf, n_pp;
  int32_t gf[kParsMaxIn];
  int32_t pp[kParsMaxIn];
};

struct ParsBufs {
  const uint8_t* codes;   // [n_tips][n_pad] compact codes
  const double* weights;  // [n_pad]
  void* sets;             // [2 n_internal][n_pad] of set_t
  uint16_t* scores;       // [2 n_internal][n_pad]
  int64_t n_pad, n_patterns;
};

// One pattern per lane, sets of type T (32 or 64 bits).
template <class T>
struct ParsLane1 {
  typedef T set_t;
  static constexpr int kVec = 1;
  T set;
  uint32_t sc;

  static __device__ __forceinline__ ParsLane1 load(const ParsBufs& b, int32_t ref, int64_t p, const T* mask) {
    const int idx = ref & kParsIdxMask;
    ParsLane1 x;
    if ((ref >> kParsKindShift) == kParsTip) {
      x.set = mask[b.codes[(int64_t)idx * b.n_pad + p]];
      x.sc = 0;
    } else {
      const int64_t o = (int64_t)idx * b.n_pad + p;
      x.set = static_cast<const T*>(b.sets)[o];
      x.sc = b.scores[o];
    }
    return x;
  }
  static __device__ __forceinline__ void store(const ParsBufs& b, int arr, int64_t p, const ParsLane1& x) {
    const int64_t o = (int64_t)arr * b.n_pad + p;
    static_cast<T*>(b.sets)[o] = x.set;
    b.scores[o] = (uint16_t)x.sc;
  }
  static __device__ __forceinline__ ParsLane1 fold(const ParsLane1& a, const ParsLane1& c) {
    ParsLane1 x;
    const T i = a.set & c.set;
    const bool empty = i == 0;
    x.set = empty ? (T)(a.set | c.set) : i;
    x.sc = a.sc + c.sc + (empty ? 1u : 0u);
    return x;
  }
  static __device__ __forceinline__ unsigned long long weighted(const ParsBufs& b, const ParsLane1& x, int64_t p) {
    if (p >= b.n_patterns) return 0;
    return (unsigned long long)b.weights[p] * x.sc;
  }
};

// Four consecutive patterns per lane, sets of one byte each in a dword, scores of 16 bits each in
// two dwords.  A score never passes 65535, so the packed adds carry nothing across the halves.
struct ParsLane4 {
  typedef uint8_t set_t;
  static constexpr int kVec = 4;
  uint32_t set, s01, s23;

  static __device__ __forceinline__ ParsLane4 load(const ParsBufs& b, int32_t ref, int64_t p, const uint8_t* mask) {
    const int idx = ref & kParsIdxMask;
    ParsLane4 x;
    if ((ref >> kParsKindShift) == kParsTip) {
      const uint32_t c = *reinterpret_cast<const uint32_t*>(b.codes + (int64_t)idx * b.n_pad + p);
      x.set = (uint32_t)mask[c & 255u] | ((uint32_t)mask[(c >> 8) & 255u] << 8) | ((uint32_t)mask[(c >> 16) & 255u] << 16) |
              ((uint32_t)mask[c >> 24] << 24);
      x.s01 = x.s23 = 0;
    } else {
      const int64_t o = (int64_t)idx * b.n_pad + p;
      x.set = *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(b.sets) + o);
      const uint2 s = *reinterpret_cast<const uint2*>(b.scores + o);
      x.s01 = s.x;
      x.s23 = s.y;
    }
    return x;
  }
  static __device__ __forceinline__ void store(const ParsBufs& b, int arr, int64_t p, const ParsLane4& x) {
    const int64_t o = (int64_t)arr * b.n_pad + p;
    *reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(b.sets) + o) = x.set;
    *reinterpret_cast<uint2*>(b.scores + o) = make_uint2(x.s01, x.s23);
  }
  static __device__ __forceinline__ ParsLane4 fold(const ParsLane4& a, const ParsLane4& c) {
    ParsLane4 x;
    const uint32_t i = a.set & c.set;
    // 0x80 in every byte of i that is zero, exact per byte: the add of the low seven bits stays
    // below 0x100, so nothing crosses a byte boundary
    const uint32_t z = ~(((i & 0x7f7f7f7fu) + 0x7f7f7f7fu) | i | 0x7f7f7f7fu);
    const uint32_t m = (z >> 7) * 0xffu;  // 0xff in those bytes
    x.set = i | ((a.set | c.set) & m);
    x.s01 = a.s01 + c.s01 + (((z >> 7) & 1u) | ((z >> 15) & 1u) << 16);
    x.s23 = a.s23 + c.s23 + (((z >> 23) & 1u) | ((z >> 31) & 1u) << 16);
    return x;
  }
  static __device__ __forceinline__ unsigned long long weighted(const ParsBufs& b, const ParsLane4& x, int64_t p) {
    const uint32_t sc[4] = {x.s01 & 0xffffu, x.s01 >> 16, x.s23 & 0xffffu, x.s23 >> 16};
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (p + k < b.n_patterns) s += (unsigned long long)b.weights[p + k] * sc[k];
    return s;
  }
};

// Sum of v over the workgroup: in the wave first, then over the waves; valid in thread 0.
__device__ __forceinline__ unsigned long long pars_block_sum(unsigned long long v, unsigned long long* wsum) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = __shfl_down((uint32_t)v, d, 64), hi = __shfl_down((uint32_t)(v >> 32), d, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kParsThreads / 64; ++w) s += wsum[w];
  return s;
}

template <class L>
__device__ __forceinline__ L pars_fold_inputs(const ParsBufs& b, const int32_t* in, int n, int64_t p,
                                              const typename L::set_t* mask) {
  L x = L::load(b, in[0], p, mask);
  for (int k = 1; k < n; ++k) x = L::fold(x, L::load(b, in[k], p, mask));
  return x;
}

// Lower ops in postorder, upper ops in preorder, the root's op last: its scores, weighted, are
// summed per workgroup and added to *total (integer adds: the order is free).
template <class L>
__global__ void __launch_bounds__(kParsThreads)
    pars_update_kernel(ParsBufs b, const uint64_t* __restrict__ masks, const int32_t* __restrict__ prog, int n_ops,
                       unsigned long long* total) {
  __shared__ typename L::set_t mask[256];
  __shared__ unsigned long long wsum[kParsThreads / 64];
  mask[threadIdx.x] = (typename L::set_t)masks[threadIdx.x];
  __syncthreads();
  const int64_t p = ((int64_t)blockIdx.x * kParsThreads + threadIdx.x) * L::kVec;
  unsigned long long part = 0;
  if (p < b.n_pad) {
    const int32_t* pc = prog;
    L x;
    for (int i = 0; i < n_ops; ++i) {
      const int32_t out = pc[0], n = pc[1];
      x = pars_fold_inputs<L>(b, pc + 2, n, p, mask);
      L::store(b, out, p, x);
      pc += 2 + n;
    }
    part = L::weighted(b, x, p);
  }
  const unsigned long long s = pars_block_sum(part, wsum);
  if (threadIdx.x == 0 && s) atomicAdd(total, s);
}

// Workgroup (move, pattern block): the two folds of the move per pattern, pp's score weighted,
// one integer add per workgroup into sums[move].
template <class L>
__global__ void __launch_bounds__(kParsThreads)
    pars_nni_kernel(ParsBufs b, const uint64_t* __restrict__ masks, const ParsMove* __restrict__ moves, int n_blk,
                    unsigned long long* sums) {
  __shared__ typename L::set_t mask[256];
  __shared__ unsigned long long wsum[kParsThreads / 64];
  mask[threadIdx.x] = (typename L::set_t)masks[threadIdx.x];
  __syncthreads();
  const int mv = blockIdx.x / n_blk, blk = blockIdx.x - mv * n_blk;
  const ParsMove& m = moves[mv];
  const int64_t p = ((int64_t)blk * kParsThreads + threadIdx.x) * L::kVec;
  unsigned long long part = 0;
  if (p < b.n_pad) {
    const L gf = pars_fold_inputs<L>(b, m.gf, m.n_gf, p, mask);
    L x = (m.pp[0] >> kParsKindShift) == kParsGf ? gf : L::load(b, m.pp[0], p, mask);
    for (int k = 1; k < m.n_pp; ++k)
      x = L::fold(x, (m.pp[k] >> kParsKindShift) == kParsGf ? gf : L::load(b, m.pp[k], p, mask));
    part = L::weighted(b, x, p);
  }
  const unsigned long long s = pars_block_sum(part, wsum);
  if (threadIdx.x == 0 && s) atomicAdd(&sums[mv], s);
}

}  // namespace plk
