// Neighbor joining (Saitou & Nei 1987) with the Studier & Keppler (1988) criterion: among r
// clusters join the pair minimising Q_ij = (r - 2) d_ij - S_i - S_j, S_i = sum_k d_ik; the
// branches get b_i = d_ij / 2 + (S_i - S_j) / (2 (r - 2)) and b_j = d_ij - b_i; the join u has
// d_uk = (d_ik + d_jk - d_ij) / 2.  Ties go to the first pair in row order.  Exact on an
// additive matrix.
#ifndef BPP_AMD_NEIGHBORJOINING_H
#define BPP_AMD_NEIGHBORJOINING_H

#include "AbstractAgglomerativeDistanceMethod.h"

namespace bpp {

class NeighborJoining : public AbstractAgglomerativeDistanceMethod {
 protected:
  std::vector<double> sums_;  // S per row of matrix_

 public:
  NeighborJoining(bool rooted = false, bool positiveLengths = false, bool verbose = true)
      : AbstractAgglomerativeDistanceMethod(verbose, rooted) {
    positiveLengths_ = positiveLengths;
  }
  NeighborJoining(const DistanceMatrix& matrix, bool rooted = false, bool positiveLengths = false, bool verbose = true)
      : AbstractAgglomerativeDistanceMethod(matrix, verbose, rooted) {
    positiveLengths_ = positiveLengths;
    computeTree();
  }
  NeighborJoining* clone() const { return new NeighborJoining(*this); }
  std::string getName() const override { return "NJ"; }

 protected:
  std::pair<size_t, size_t> bestPair() override;
  std::pair<double, double> branchLengths(size_t i, size_t j) override;
  void reduce(size_t i, size_t j, double bi, double bj) override;
};

}  // namespace bpp

#endif
