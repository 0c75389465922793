// NNITopologySearch.h: hill climbing over nearest-neighbour interchanges.  FAST applies the
// first improving interchange of a round, BETTER tests every node and applies the best one; both
// repeat until a round finds none.  Over an NNIHomogeneousTreeLikelihood every round of either is
// served by one plk_nni_scores call (the first testNNI after a change scores every node).  The
// reference's PHYML algorithm needs clone() of the likelihood, which this mirror does not have.
#ifndef BPP_AMD_NNITOPOLOGYSEARCH_H
#define BPP_AMD_NNITOPOLOGYSEARCH_H

#include <string>
#include <vector>

#include "NNISearchable.h"

namespace bpp {

class NNITopologySearch : public virtual TopologySearch {
  NNISearchable* searchableTree_;  // not owned
  std::string algorithm_;
  unsigned int verbose_;
  std::vector<TopologyListener*> topoListeners_;
  std::vector<double> accepted_;   // testNNI value of every interchange applied
  size_t rounds_ = 0;

  std::vector<int> candidateNodes() const;
  void notifyAllPerformed(const TopologyChangeEvent& event);
  void notifyAllTested(const TopologyChangeEvent& event);
  void notifyAllSuccessful(const TopologyChangeEvent& event);
  void searchFast();
  void searchBetter();

 public:
  static const std::string FAST;
  static const std::string BETTER;

  NNITopologySearch(NNISearchable& tree, const std::string& algorithm = FAST, unsigned int verbose = 2)
      : searchableTree_(&tree), algorithm_(algorithm), verbose_(verbose) {}
  void search() override;
  void addTopologyListener(TopologyListener* listener) override { topoListeners_.push_back(listener); }
  const Tree& getTopology() const { return searchableTree_->getTopology(); }
  NNISearchable* getSearchableObject() { return searchableTree_; }
  const NNISearchable* getSearchableObject() const { return searchableTree_; }
  // the testNNI values of the interchanges the last search() applied, in order, and its rounds
  const std::vector<double>& getAcceptedImprovements() const { return accepted_; }
  size_t getNumberOfRounds() const { return rounds_; }
};

}  // namespace bpp

#endif
