// Host mirror: Fitch parsimony over the engine's plk_pars_* calls (AbstractTreeParsimonyScore,
// DRTreeParsimonyScore).  Clean-room; see the headers for what the reference does instead.
#include <algorithm>
#include <cstdlib>

#include "Bpp/App/ApplicationTools.h"
#include "Bpp/Numeric/Random/RandomTools.h"
#include "Bpp/Phyl/Parsimony/DRTreeParsimonyScore.h"
#include "Bpp/Text/TextTools.h"
#include "plk.h"

namespace bpp {

// ---------------------------------------------------------------------------
// AbstractTreeParsimonyScore
// ---------------------------------------------------------------------------

AbstractTreeParsimonyScore::AbstractTreeParsimonyScore(const Tree& tree, const SiteContainer& data, bool verbose,
                                                       bool includeGaps)
    : tree_(new TreeTemplate<Node>(tree)),
      data_(data.clone()),
      alphabet_(data.getAlphabet()),
      includeGaps_(includeGaps),
      nbStates_((size_t)data.getAlphabet()->getSize() + (includeGaps ? 1 : 0)) {
  for (const std::string& name : tree_->getLeavesNames())
    if (!data_->hasSequence(name)) throw SequenceNotFoundException("AbstractTreeParsimonyScore: no sequence for leaf", name);
  (void)verbose;
}

std::vector<unsigned int> AbstractTreeParsimonyScore::getScoreForEachSite() const {
  std::vector<unsigned int> scores(data_->getNumberOfSites());
  for (size_t i = 0; i < scores.size(); i++) scores[i] = getScoreForSite(i);
  return scores;
}

// ---------------------------------------------------------------------------
// DRTreeParsimonyScore
// ---------------------------------------------------------------------------

DRTreeParsimonyScore::DRTreeParsimonyScore(const Tree& tree, const SiteContainer& data, bool verbose, bool includeGaps)
    : AbstractTreeParsimonyScore(tree, data, verbose, includeGaps) {
  init_(verbose);
}

DRTreeParsimonyScore::DRTreeParsimonyScore(const DRTreeParsimonyScore& tp)
    : AbstractTreeParsimonyScore(*tp.tree_, *tp.data_, false, tp.includeGaps_), nodeStates_(tp.nodeStates_) {
  init_(false);
}

DRTreeParsimonyScore::~DRTreeParsimonyScore() {
  if (engine_) plk_destroy(engine_);
}

void DRTreeParsimonyScore::check(int rc, const char* what) const {
  if (rc != PLK_OK) throw DeviceException(rc, std::string(what) + ": " + plk_last_error(engine_));
}

void DRTreeParsimonyScore::init_(bool verbose) {
  const std::vector<const Node*> leaves = getTreeP_()->getLeaves();
  nTips_ = (int)leaves.size();
  int nInternal = 0;
  for (const Node* n : getTreeP_()->getNodes())
    if (n->isLeaf())
      engineIndex_[n] = (int)(std::find(leaves.begin(), leaves.end(), n) - leaves.begin());
    else
      engineIndex_[n] = nTips_ + nInternal++;
  if (nInternal == 0) throw Exception("DRTreeParsimonyScore: the tree has no internal node");

  // tip codes: the alphabet's codes; a gap is the unknown code, or with includeGaps a code of its own
  const int nAlpha = alphabet_->getNumberOfCodes(), S = alphabet_->getSize();
  const int gapCode = includeGaps_ ? nAlpha : alphabet_->getUnknownCharacterCode();
  const int nCodes = nAlpha + (includeGaps_ ? 1 : 0);
  if (nCodes > 256) throw Exception("DRTreeParsimonyScore: more than 256 character codes");
  const size_t nSites = data_->getNumberOfSites();
  std::vector<std::vector<uint8_t> > rows((size_t)nTips_, std::vector<uint8_t>(nSites));
  for (int t = 0; t < nTips_; t++) {
    const Sequence& seq = data_->getSequence(leaves[(size_t)t]->getName());
    for (size_t i = 0; i < nSites; i++) {
      const int v = seq.getValue(i);
      if (v < -1 || v >= nAlpha) throw BadIntException(v, "DRTreeParsimonyScore: state outside the alphabet");
      rows[(size_t)t][i] = (uint8_t)(v < 0 ? gapCode : v);
    }
  }
  // distinct columns in the order of their first site, with integer weights
  std::map<std::vector<uint8_t>, size_t> seen;
  std::vector<std::vector<uint8_t> > patterns((size_t)nTips_);
  std::vector<double> weights;
  patternOfSite_.resize(nSites);
  std::vector<uint8_t> column((size_t)nTips_);
  for (size_t i = 0; i < nSites; i++) {
    for (int t = 0; t < nTips_; t++) column[(size_t)t] = rows[(size_t)t][i];
    auto it = seen.find(column);
    if (it == seen.end()) {
      it = seen.emplace(column, weights.size()).first;
      for (int t = 0; t < nTips_; t++) patterns[(size_t)t].push_back(column[(size_t)t]);
      weights.push_back(0.);
    }
    patternOfSite_[i] = it->second;
    weights[it->second] += 1.;
  }
  nbDistinctSites_ = weights.size();
  if (nbDistinctSites_ == 0) throw Exception("DRTreeParsimonyScore: the alignment has no site");
  if (verbose) ApplicationTools::displayResult("Number of distinct sites", TextTools::toString(nbDistinctSites_));

  const char* dev = std::getenv("BPP_AMD_DEVICE");
  const int Se = std::max(S, 2);
  plk_handle h = nullptr;
  const int rc = plk_create(dev ? std::atoi(dev) : 0, Se, 1, (int64_t)nbDistinctSites_, nTips_, nInternal, 1, 0, &h);
  if (rc != PLK_OK) throw DeviceException(rc, std::string("plk_create: ") + plk_last_error(nullptr));
  engine_ = h;
  std::vector<double> table((size_t)nCodes * Se, 0.);
  std::vector<uint64_t> masks((size_t)nCodes, 0);
  for (int c = 0; c < nAlpha; c++)
    for (int s : alphabet_->getAlias(c)) {
      table[(size_t)c * Se + s] = 1.;
      masks[(size_t)c] |= (uint64_t)1 << s;
    }
  if (includeGaps_) {
    std::fill(table.begin() + (size_t)nAlpha * Se, table.end(), 1.);
    if (S < 64) masks[(size_t)nAlpha] = (uint64_t)1 << S;
  }
  check(plk_set_code_table(engine_, nCodes, table.data()), "plk_set_code_table");
  check(plk_pars_set_code_masks(engine_, (int)nbStates_, nCodes, masks.data()), "plk_pars_set_code_masks");
  for (int t = 0; t < nTips_; t++) check(plk_set_tip_codes(engine_, t, patterns[(size_t)t].data()), "plk_set_tip_codes");
  check(plk_set_pattern_weights(engine_, weights.data()), "plk_set_pattern_weights");
  current_ = false;
}

void DRTreeParsimonyScore::update_() const {
  std::vector<plk_op> ops;
  for (const Node* n : getTreeP_()->getNodes()) {
    if (n->isLeaf()) continue;
    for (size_t k = 0; k < n->getNumberOfSons(); k += 3) {
      plk_op op;
      op.parent = engineIndex_.at(n);
      op.n_children = 0;
      op.flags = k == 0 ? 0 : PLK_OP_ACCUMULATE;
      for (size_t j = k; j < std::min(k + 3, n->getNumberOfSons()); j++) op.child[op.n_children++] = engineIndex_.at(n->getSon(j));
      for (int j = op.n_children; j < 3; j++) op.child[j] = 0;
      ops.push_back(op);
    }
  }
  updateCalls_++;
  check(plk_pars_update(engine_, ops.data(), (int)ops.size()), "plk_pars_update");
  uint64_t score = 0;
  std::vector<uint32_t> sites(nbDistinctSites_);
  check(plk_pars_score(engine_, &score, sites.data()), "plk_pars_score");
  score_ = (unsigned int)score;
  patternScores_.assign(sites.begin(), sites.end());
  current_ = true;
  nniValid_ = false;
}

unsigned int DRTreeParsimonyScore::getScore() const {
  if (!current_) update_();
  return score_;
}

unsigned int DRTreeParsimonyScore::getScoreForSite(size_t site) const {
  if (!current_) update_();
  return patternScores_.at(patternOfSite_.at(site));
}

const Node* DRTreeParsimonyScore::uncleOf(const Node* son) {
  const Node* parent = son->getFather();
  const Node* grand = parent->getFather();
  size_t pos = 0;
  while (grand->getSon(pos) != parent) pos++;
  return grand->getSon(pos > 1 ? pos - 1 : 1 - pos);
}

void DRTreeParsimonyScore::scoreAllNodes_() const {
  if (!current_) update_();
  nniScores_.clear();
  std::vector<int> ids;
  std::vector<int32_t> son, uncle;
  for (const Node* n : getTreeP_()->getNodes()) {
    if (!n->hasFather() || !n->getFather()->hasFather()) continue;
    ids.push_back(n->getId());
    son.push_back(engineIndex_.at(n));
    uncle.push_back(engineIndex_.at(uncleOf(n)));
  }
  nniValid_ = true;
  if (ids.empty()) return;
  std::vector<int64_t> delta(ids.size());
  nniCalls_++;
  check(plk_pars_nni_scores(engine_, (int)ids.size(), son.data(), uncle.data(), delta.data()), "plk_pars_nni_scores");
  for (size_t i = 0; i < ids.size(); i++) nniScores_[ids[i]] = (double)delta[i];
}

double DRTreeParsimonyScore::testNNI(int nodeId) const {
  const Node* son = getTreeP_()->getNode(nodeId);
  if (!son->hasFather()) throw Exception("DRTreeParsimonyScore::testNNI(). Node 'son' must not be the root node.");
  if (!son->getFather()->hasFather()) throw Exception("DRTreeParsimonyScore::testNNI(). Node 'parent' must not be the root node.");
  if (!current_ || !nniValid_) scoreAllNodes_();
  return nniScores_.at(nodeId);
}

void DRTreeParsimonyScore::doNNI(int nodeId) {
  Node* son = getTreeP_()->getNode(nodeId);
  if (!son->hasFather()) throw Exception("DRTreeParsimonyScore::doNNI(). Node 'son' must not be the root node.");
  Node* parent = son->getFather();
  if (!parent->hasFather()) throw Exception("DRTreeParsimonyScore::doNNI(). Node 'parent' must not be the root node.");
  Node* grand = parent->getFather();
  Node* uncle = const_cast<Node*>(uncleOf(son));
  std::vector<Node*>&ps = parent->sons(), &gs = grand->sons();
  ps.erase(std::find(ps.begin(), ps.end(), son));
  gs.erase(std::find(gs.begin(), gs.end(), uncle));
  parent->addSon(uncle);
  grand->addSon(son);
  current_ = false;
  nniValid_ = false;
}

void DRTreeParsimonyScore::computeSolution() {
  if (!current_) update_();
  const TreeTemplate<Node>* tree = getTreeP_();
  const Node* root = tree->getRootNode();
  std::map<int, std::vector<unsigned int> > possible;
  uint64_t set = 0;
  std::vector<uint64_t> sets(nbDistinctSites_);
  for (const Node* n : tree->getNodes()) {
    if (n->hasFather()) {
      check(plk_pars_get_edge(engine_, engineIndex_.at(n), 0, sets.data(), nullptr), "plk_pars_get_edge");
    } else {
      // the root's states as its first internal son sees them: that son's upper pair
      const Node* neighbor = nullptr;
      for (size_t k = 0; k < n->getNumberOfSons() && !neighbor; k++)
        if (!n->getSon(k)->isLeaf()) neighbor = n->getSon(k);
      if (!neighbor) throw Exception("DRTreeParsimonyScore::computeSolution(). The root has no internal son.");
      check(plk_pars_get_edge(engine_, engineIndex_.at(neighbor), 1, sets.data(), nullptr), "plk_pars_get_edge");
    }
    set = sets[0];  // the first distinct site
    std::vector<unsigned int>& states = possible[n->getId()];
    for (unsigned int s = 0; s < nbStates_; s++)
      if (set >> s & 1) states.push_back(s);
  }
  nodeStates_.clear();
  std::vector<const Node*> stack(1, root);  // preorder: a father before its sons
  while (!stack.empty()) {
    const Node* n = stack.back();
    stack.pop_back();
    std::vector<unsigned int> states = possible[n->getId()];
    int state;
    if (states.size() == 1)
      state = (int)states[0];
    else if (n->hasFather())
      state = nodeStates_.at(n->getFather()->getId());
    else
      state = (int)RandomTools::pickOne(states);
    nodeStates_[n->getId()] = state;
    for (size_t k = n->getNumberOfSons(); k-- > 0;) stack.push_back(n->getSon(k));
  }
}

int DRTreeParsimonyScore::getNodeState(const Node* node) const {
  const auto it = nodeStates_.find(node->getId());
  if (it == nodeStates_.end()) throw Exception("DRTreeParsimonyScore::getNodeState(). No state: call computeSolution() first.");
  return it->second;
}

}  // namespace bpp
