// Likelihood/NNIHomogeneousTreeLikelihood.h: a double-recursive homogeneous likelihood whose
// tree NNITopologySearch can rearrange.  The reference's testNNI builds two conditional arrays
// on the host and Brent-optimises one branch length, one node at a time
// (NNIHomogeneousTreeLikelihood.cpp:205-309).  Here the first testNNI after a parameter or
// topology change scores every eligible node with one plk_nni_scores call -- from the partials
// and upper vectors the engine holds -- and caches the answers, so a round of a search costs
// one call.  Deviation: a safeguarded Newton ascent to 1e-8 replaces Brent at tolerance 0.1, so
// the remembered length is closer to the optimum and the improvement at least as large.
#ifndef BPP_AMD_NNIHOMOGENEOUSTREELIKELIHOOD_H
#define BPP_AMD_NNIHOMOGENEOUSTREELIKELIHOOD_H

#include <map>

#include "../NNISearchable.h"
#include "TreeLikelihood.h"

namespace bpp {

class NNIHomogeneousTreeLikelihood : public DRHomogeneousTreeLikelihood, public virtual NNISearchable {
  struct Score {
    double delta, length;
  };
  mutable std::map<int, Score> scores_;  // per node id, of the current tree and parameters
  mutable bool scoresValid_ = false;
  mutable size_t scoreCalls_ = 0;        // plk_nni_scores calls so far

  // the uncle testNNI / doNNI give the node: the reference's choice by the father's position
  static const Node* uncleOf(const Node* son);
  void scoreAllNodes() const;
  void rebuildOps();

 public:
  NNIHomogeneousTreeLikelihood(const Tree& tree, SubstitutionModel* model, DiscreteDistribution* rDist,
                               bool checkRooted = true, bool verbose = true);
  NNIHomogeneousTreeLikelihood(const Tree& tree, const SiteContainer& data, SubstitutionModel* model,
                               DiscreteDistribution* rDist, bool checkRooted = true, bool verbose = true);
  void fireParameterChanged(const ParameterList& params) override;

  // -(lnL of the tree with the node and its uncle exchanged and the father's branch re-estimated
  //   - current lnL): negative for an improvement.  0 for a node whose father or grandfather has
  // more than three sons (the engine does not score those).
  double testNNI(int nodeId) const override;
  // the length testNNI found best for the father's branch
  double getBestBranchLength(int nodeId) const;
  // exchange the two subtrees, give the father's branch the remembered length (its BrLen
  // parameter follows), rebuild the engine's op list and evaluate
  void doNNI(int nodeId) override;
  const Tree& getTopology() const override { return getTree(); }
  double getTopologyValue() const override { return getValue(); }
  // (a test changes nothing: the cached scores of the round stay)
  void topologyChangeTested(const TopologyChangeEvent&) override {}
  void topologyChangeSuccessful(const TopologyChangeEvent&) override { scoresValid_ = false; }
  void topologyChangePerformed(const TopologyChangeEvent&) override { scoresValid_ = false; }
  size_t getNumberOfScoreCalls() const { return scoreCalls_; }

  // Local bootstrap proportions (RELL over the three NNI configurations around a branch, the
  // "LBP" of MOLPHY), keyed by the id of the lower node of every internal branch p whose father
  // g and itself have at most three sons.  The rivals of p are the interchanges (s, uncle) for
  // every son s of p, each at the length testNNI re-estimated (the cached plk_nni_scores
  // answers).  One plk_nni_site_rows call writes log rho per pattern of every rival, the
  // weights are bootstrap(nSites) counts per replicate mapped to patterns, and one
  // plk_replicate_sums call returns the resampled differences to the current tree, whose own is
  // 0.  Changes no parameter, no cached score and no later getValue().  The rows and weights stay
  // on the engine until the next call or plk_site_rows_reserve(engine, 0): plk_replicate_sums
  // over rows 0 .. (the sum of getLocalBootstrapRivals()) returns the same sums again.
  std::map<int, double> computeLocalBootstrap(size_t nReplicates) const;
  // frees those rows and weights (replicates x patterns doubles and one row per rival)
  void releaseLocalBootstrap() const;
  // the branches of the last computeLocalBootstrap in row order and the rivals of each
  const std::vector<int>& getLocalBootstrapNodeIds() const { return lbpIds_; }
  const std::vector<size_t>& getLocalBootstrapRivals() const { return lbpRivals_; }
  // The share of replicates in which no rival beats the current configuration: G is
  // replicates x (sum of rivals), replicate-major, the rivals of a branch side by side.  A
  // replicate counts 0 when a rival's sum is positive, else 1 / k with k = 1 + the rivals whose
  // sum is exactly 0 (tied at the top with the current configuration).
  static std::vector<double> localBootstrapFromSums(const std::vector<double>& G, size_t replicates,
                                                    const std::vector<size_t>& rivals);

 private:
  mutable std::vector<int> lbpIds_;
  mutable std::vector<size_t> lbpRivals_;
};

}  // namespace bpp

#endif
