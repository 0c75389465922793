// What the agglomerative methods share: the matrix, the flags, the tree built by computeTree()
// and the joining loop itself.  A method supplies the pair to join, the two branch lengths and
// the distances of the new cluster (NeighborJoining.h, BioNJ.h).  PGMA and hierarchical
// clustering are not part of the mirror.
#ifndef BPP_AMD_ABSTRACTAGGLOMERATIVEDISTANCEMETHOD_H
#define BPP_AMD_ABSTRACTAGGLOMERATIVEDISTANCEMETHOD_H

#include <memory>
#include <vector>

#include "DistanceMethod.h"

namespace bpp {

class AbstractAgglomerativeDistanceMethod : public AgglomerativeDistanceMethod {
 protected:
  DistanceMatrix matrix_;                       // working copy: rows of joined clusters are reused
  std::unique_ptr<TreeTemplate<Node> > tree_;
  bool verbose_;
  bool rootTree_;
  bool positiveLengths_ = false;

 public:
  AbstractAgglomerativeDistanceMethod(bool verbose = true, bool rootTree = false)
      : matrix_(0), verbose_(verbose), rootTree_(rootTree) {}
  AbstractAgglomerativeDistanceMethod(const DistanceMatrix& matrix, bool verbose = true, bool rootTree = false)
      : matrix_(matrix), verbose_(verbose), rootTree_(rootTree) {}
  AbstractAgglomerativeDistanceMethod(const AbstractAgglomerativeDistanceMethod& a)
      : matrix_(a.matrix_), tree_(a.tree_ ? a.tree_->clone() : nullptr), verbose_(a.verbose_), rootTree_(a.rootTree_),
        positiveLengths_(a.positiveLengths_) {}
  AbstractAgglomerativeDistanceMethod& operator=(const AbstractAgglomerativeDistanceMethod& a) {
    matrix_ = a.matrix_;
    tree_.reset(a.tree_ ? a.tree_->clone() : nullptr);
    verbose_ = a.verbose_, rootTree_ = a.rootTree_, positiveLengths_ = a.positiveLengths_;
    return *this;
  }

  void setDistanceMatrix(const DistanceMatrix& matrix) override;
  // a new tree (the caller's), leaves named from the matrix; null before computeTree()
  TreeTemplate<Node>* getTree() const override { return tree_ ? new TreeTemplate<Node>(*tree_) : nullptr; }
  // Joins clusters until three are left (an unrooted tree ends in a three-son root) or, for a
  // rooted tree, two (the root sits in the middle of the last branch).
  void computeTree() override;
  void setVerbose(bool yn) override { verbose_ = yn; }
  bool isVerbose() const override { return verbose_; }
  void outputPositiveLengths(bool yn) { positiveLengths_ = yn; }

 protected:
  // The state of the joining loop: the active clusters' rows in matrix_, in increasing order.
  std::vector<size_t> active_;
  // (i, j), positions in active_, i < j
  virtual std::pair<size_t, size_t> bestPair() = 0;
  // the lengths of the branches from clusters i and j to their join
  virtual std::pair<double, double> branchLengths(size_t i, size_t j) = 0;
  // Row active_[i] becomes the join of (i, j): its distance to every other cluster.  Called
  // before j leaves active_.
  virtual void reduce(size_t i, size_t j, double bi, double bj) = 0;
  virtual void start() {}
};

}  // namespace bpp

#endif
