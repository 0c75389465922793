// Parsimony/DRTreeParsimonyScore.h: double-recursive Fitch parsimony on the engine's plk_pars_*
// calls.  The reference keeps, per node, one (bitset, score) array per neighbour and folds them on
// the host; here the sites are compressed to patterns with integer weights, plk_pars_update forms
// every lower and upper pair of the tree in one launch, and the first testNNI after a change
// scores every eligible node with one plk_pars_nni_scores call (later tests read the cache), so a
// round of NNITopologySearch costs one call.
#ifndef BPP_AMD_DRTREEPARSIMONYSCORE_H
#define BPP_AMD_DRTREEPARSIMONYSCORE_H

#include <map>

#include "../../Seq/Container/VectorSiteContainer.h"
#include "../../Text/TextTools.h"
#include "../NNISearchable.h"
#include "AbstractTreeParsimonyScore.h"

struct plk_handle_s;

namespace bpp {

class DRTreeParsimonyScore : public AbstractTreeParsimonyScore, public virtual NNISearchable {
  plk_handle_s* engine_ = nullptr;
  size_t nbDistinctSites_ = 0;
  std::vector<size_t> patternOfSite_;
  std::map<const Node*, int> engineIndex_;  // leaves first (in the tree's order), then internal nodes in postorder
  int nTips_ = 0;
  mutable bool current_ = false;          // the engine's pairs are those of tree_
  mutable unsigned int score_ = 0;
  mutable std::vector<unsigned int> patternScores_;
  mutable std::map<int, double> nniScores_;  // per node id, of the current tree
  mutable bool nniValid_ = false;
  mutable size_t nniCalls_ = 0, updateCalls_ = 0;
  std::map<int, int> nodeStates_;         // computeSolution()

  void init_(bool verbose);
  void check(int rc, const char* what) const;
  void update_() const;                   // plk_pars_update on the tree as it stands
  void scoreAllNodes_() const;
  static const Node* uncleOf(const Node* son);

 public:
  DRTreeParsimonyScore(const Tree& tree, const SiteContainer& data, bool verbose = true, bool includeGaps = false);
  DRTreeParsimonyScore(const DRTreeParsimonyScore& tp);
  DRTreeParsimonyScore& operator=(const DRTreeParsimonyScore&) = delete;
  ~DRTreeParsimonyScore() override;
  DRTreeParsimonyScore* clone() const override { return new DRTreeParsimonyScore(*this); }

  unsigned int getScore() const override;
  unsigned int getScoreForSite(size_t site) const override;
  size_t getNumberOfDistinctSites() const { return nbDistinctSites_; }

  // The score of the tree with the node and its uncle exchanged minus the current score.  The
  // uncle is the grandfather's son next to the father: the one before it when the father is the
  // third son or a later one, else the other of the first two.
  double testNNI(int nodeId) const override;
  // Exchange the two; each is appended to its new father's sons.
  void doNNI(int nodeId) override;
  const Tree& getTopology() const override { return getTree(); }
  double getTopologyValue() const override { return getScore(); }
  // after an interchange the pairs are formed again (plk_pars_update); a test alone changes nothing
  void topologyChangeTested(const TopologyChangeEvent&) override { getScore(); }
  void topologyChangeSuccessful(const TopologyChangeEvent&) override {}
  void topologyChangePerformed(const TopologyChangeEvent&) override { getScore(); }
  size_t getNumberOfScoreCalls() const { return nniCalls_; }    // plk_pars_nni_scores calls so far
  size_t getNumberOfUpdateCalls() const { return updateCalls_; }  // plk_pars_update calls so far

  // One most parsimonious assignment of the first distinct site: a node whose set (a leaf's
  // states, an internal node's lower set, the root's set as its first internal son sees it) holds
  // one state takes it, any other takes its father's state, and an ambiguous root picks at random.
  void computeSolution();
  int getNodeState(const Node* node) const;
};

}  // namespace bpp

#endif
