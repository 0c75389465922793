// Host mirror: NNI topology search over plk_nni_scores (NNIHomogeneousTreeLikelihood,
// NNITopologySearch).  Clean-room; see the headers for what the reference does instead.
#include <algorithm>
#include <cmath>

#include "Bpp/App/ApplicationTools.h"
#include "Bpp/Phyl/Likelihood/NNIHomogeneousTreeLikelihood.h"
#include "Bpp/Phyl/NNITopologySearch.h"
#include "Bpp/Text/TextTools.h"
#include "plk.h"

namespace bpp {

// ---------------------------------------------------------------------------
// NNIHomogeneousTreeLikelihood
// ---------------------------------------------------------------------------

NNIHomogeneousTreeLikelihood::NNIHomogeneousTreeLikelihood(const Tree& tree, SubstitutionModel* model,
                                                           DiscreteDistribution* rDist, bool checkRooted, bool verbose)
    : DRHomogeneousTreeLikelihood(tree, model, rDist, checkRooted, verbose) {}

NNIHomogeneousTreeLikelihood::NNIHomogeneousTreeLikelihood(const Tree& tree, const SiteContainer& data,
                                                           SubstitutionModel* model, DiscreteDistribution* rDist,
                                                           bool checkRooted, bool verbose)
    : DRHomogeneousTreeLikelihood(tree, data, model, rDist, checkRooted, verbose) {}

void NNIHomogeneousTreeLikelihood::fireParameterChanged(const ParameterList& params) {
  scoresValid_ = false;
  DRHomogeneousTreeLikelihood::fireParameterChanged(params);
}

// The father's position among the grandfather's sons decides: the first son when the father
// is the third or a later one, else the other of the first two.
const Node* NNIHomogeneousTreeLikelihood::uncleOf(const Node* son) {
  const Node* parent = son->getFather();
  const Node* grand = parent->getFather();
  size_t pos = 0;
  while (grand->getSon(pos) != parent) pos++;
  return grand->getSon(pos > 1 ? 0 : 1 - pos);
}

void NNIHomogeneousTreeLikelihood::scoreAllNodes() const {
  scores_.clear();
  std::vector<int> ids;
  std::vector<int32_t> son, uncle;
  std::vector<double> t0;
  for (const Node* n : nodes_) {
    if (!n->hasFather() || !n->getFather()->hasFather()) continue;
    const Node* parent = n->getFather();
    const Node* grand = parent->getFather();
    if (parent->getNumberOfSons() > 3 || grand->getNumberOfSons() > 3) continue;
    ids.push_back(n->getId());
    son.push_back(engineIndex_.at(n));
    uncle.push_back(engineIndex_.at(uncleOf(n)));
    t0.push_back(std::min(std::max(parent->getDistanceToFather(), minimumBrLen_), maximumBrLen_));
  }
  scoresValid_ = true;
  if (ids.empty()) return;
  refreshDerivativeMatrices();  // the preorder pass reads dP / d2P of every branch
  std::vector<double> length(ids.size()), delta(ids.size());
  scoreCalls_++;
  check(plk_nni_scores(engine_, (int)ids.size(), son.data(), uncle.data(), nullptr, t0.data(), minimumBrLen_,
                       maximumBrLen_, 1e-8, 40, length.data(), delta.data(), nullptr, nullptr, nullptr),
        "plk_nni_scores");
  for (size_t i = 0; i < ids.size(); i++) scores_[ids[i]] = Score{delta[i], length[i]};
}

double NNIHomogeneousTreeLikelihood::testNNI(int nodeId) const {
  if (!initialized_) throw Exception("NNIHomogeneousTreeLikelihood::testNNI(). Object not initialized.");
  const Node* n = tree_->getNode(nodeId);
  if (!n->hasFather()) throw Exception("NNIHomogeneousTreeLikelihood::testNNI(). Node 'son' must not be the root node.");
  if (!n->getFather()->hasFather())
    throw Exception("NNIHomogeneousTreeLikelihood::testNNI(). Node 'parent' must not be the root node.");
  if (!scoresValid_) scoreAllNodes();
  const auto it = scores_.find(nodeId);
  if (it == scores_.end()) return 0.;
  // A change below the engine's accuracy on delta (1e-10 of |lnL|) is no improvement: two
  // topologies around a branch at its lower bound score alike, and a search that took their
  // rounding for a gain would swap them for ever.
  const double delta = it->second.delta;
  return std::fabs(delta) <= 1e-10 * std::fabs(minusLogLik_) ? 0. : -delta;
}

double NNIHomogeneousTreeLikelihood::getBestBranchLength(int nodeId) const {
  testNNI(nodeId);
  const auto it = scores_.find(nodeId);
  if (it == scores_.end()) throw Exception("NNIHomogeneousTreeLikelihood::getBestBranchLength(). Node was not scored.");
  return it->second.length;
}

// the op list again from the rearranged tree, in postorder; engine indices stay with their nodes
void NNIHomogeneousTreeLikelihood::rebuildOps() {
  opParent_.clear();
  opChildren_.clear();
  opFlags_.clear();
  maxSons_ = 0;
  for (Node* n : tree_->getNodes()) {
    if (n->isLeaf()) continue;
    maxSons_ = std::max(maxSons_, n->getNumberOfSons());
    for (size_t k = 0; k < n->getNumberOfSons(); k += 3) {
      std::vector<int> ch;
      for (size_t j = k; j < std::min(k + 3, n->getNumberOfSons()); j++) ch.push_back(engineIndex_.at(n->getSon(j)));
      opParent_.push_back(engineIndex_.at(n));
      opChildren_.push_back(ch);
      opFlags_.push_back(k == 0 ? 0 : PLK_OP_ACCUMULATE);
    }
  }
}

void NNIHomogeneousTreeLikelihood::doNNI(int nodeId) {
  const double length = getBestBranchLength(nodeId);
  Node* son = tree_->getNode(nodeId);
  Node* parent = son->getFather();
  Node* grand = parent->getFather();
  Node* uncle = const_cast<Node*>(uncleOf(son));
  std::vector<Node*>&ps = parent->sons(), &gs = grand->sons();
  *std::find(ps.begin(), ps.end(), son) = uncle;
  *std::find(gs.begin(), gs.end(), uncle) = son;
  son->setFather(grand);
  uncle->setFather(parent);
  // the father's branch: the node, its BrLen parameter and the list handed to optimisers
  parent->setDistanceToFather(length);
  const size_t i = (size_t)(std::find(nodes_.begin(), nodes_.end(), parent) - nodes_.begin());
  const std::string name = "BrLen" + TextTools::toString(i);
  if (parameters_.hasParameter(name)) parameters_.setParameterValue(name, length);
  if (brLenParameters_.hasParameter(name)) brLenParameters_.setParameterValue(name, length);
  rebuildOps();
  scoresValid_ = false;
  evaluateTree(std::vector<const Node*>(1, parent), false);
}

// ---------------------------------------------------------------------------
// NNITopologySearch
// ---------------------------------------------------------------------------

const std::string NNITopologySearch::FAST = "Fast";
const std::string NNITopologySearch::BETTER = "Better";

void NNITopologySearch::notifyAllPerformed(const TopologyChangeEvent& event) {
  searchableTree_->topologyChangePerformed(event);
  for (TopologyListener* l : topoListeners_) l->topologyChangePerformed(event);
}

void NNITopologySearch::notifyAllTested(const TopologyChangeEvent& event) {
  searchableTree_->topologyChangeTested(event);
  for (TopologyListener* l : topoListeners_) l->topologyChangeTested(event);
}

void NNITopologySearch::notifyAllSuccessful(const TopologyChangeEvent& event) {
  searchableTree_->topologyChangeSuccessful(event);
  for (TopologyListener* l : topoListeners_) l->topologyChangeSuccessful(event);
}

// every node but the root and its sons, in the tree's postorder
std::vector<int> NNITopologySearch::candidateNodes() const {
  const TreeTemplate<Node> tree(searchableTree_->getTopology());
  std::vector<int> ids;
  for (const Node* n : tree.getNodes())
    if (n->hasFather() && n->getFather()->hasFather()) ids.push_back(n->getId());
  return ids;
}

void NNITopologySearch::search() {
  accepted_.clear();
  rounds_ = 0;
  if (algorithm_ == FAST)
    searchFast();
  else if (algorithm_ == BETTER)
    searchBetter();
  else
    throw Exception("Unknown NNI algorithm: " + algorithm_ + " (this mirror has Fast and Better).");
}

void NNITopologySearch::searchFast() {
  bool found = true;
  while (found) {
    found = false;
    rounds_++;
    for (int id : candidateNodes()) {
      const double diff = searchableTree_->testNNI(id);
      notifyAllTested(TopologyChangeEvent(*this));
      if (verbose_ >= 3) ApplicationTools::displayResult("   Testing node " + TextTools::toString(id), TextTools::toString(diff));
      if (diff < 0.) {
        searchableTree_->doNNI(id);
        accepted_.push_back(diff);
        notifyAllPerformed(TopologyChangeEvent(*this));
        if (verbose_ >= 1)
          ApplicationTools::displayResult("   Current value", TextTools::toString(searchableTree_->getTopologyValue(), 10));
        found = true;
        break;
      }
    }
  }
}

void NNITopologySearch::searchBetter() {
  bool found = true;
  while (found) {
    rounds_++;
    int best = 0;
    double bestDiff = 0.;
    found = false;
    for (int id : candidateNodes()) {
      const double diff = searchableTree_->testNNI(id);
      notifyAllTested(TopologyChangeEvent(*this));
      if (verbose_ >= 3) ApplicationTools::displayResult("   Testing node " + TextTools::toString(id), TextTools::toString(diff));
      if (diff < bestDiff) {
        best = id;
        bestDiff = diff;
        found = true;
      }
    }
    if (found) {
      searchableTree_->doNNI(best);
      accepted_.push_back(bestDiff);
      notifyAllPerformed(TopologyChangeEvent(*this));
      if (verbose_ >= 1)
        ApplicationTools::displayResult("   Current value", TextTools::toString(searchableTree_->getTopologyValue(), 10));
    }
  }
}

}  // namespace bpp
