// Host mirror: marginal ancestral states and posterior rate classes over plk_node_posteriors
// (MarginalAncestralStateReconstruction, DRTreeLikelihoodTools and the posterior-rate queries
// of AbstractDiscreteRatesAcrossSitesTreeLikelihood).  The device forms J = p_c (P_v^T U_v) L_v
// and its marginals next to the partials; the host keeps what the reference keeps there --
// leaves, sampling, the pattern -> site expansion.
#include "Bpp/Numeric/Random/RandomTools.h"
#include "Bpp/Phyl/Likelihood/DRTreeLikelihoodTools.h"
#include "Bpp/Phyl/Likelihood/MarginalAncestralStateReconstruction.h"
#include "Bpp/Text/TextTools.h"
#include "plk.h"

namespace bpp {

AbstractPlkTreeLikelihood::NodePosteriors AbstractPlkTreeLikelihood::computeNodePosteriors(
    const std::vector<int>& nodeIds, bool joint, bool states, bool classes, bool best) const {
  if (!initialized_) throw Exception("computeNodePosteriors: instance is not initialized.");
  std::vector<int32_t> eng;
  bool rootOnly = true;
  for (int id : nodeIds) {
    const Node* n = tree_->getNode(id);
    if (n->isLeaf()) throw Exception("computeNodePosteriors: node " + TextTools::toString(id) + " is a leaf");
    eng.push_back(engineIndex_.at(n));
    if (eng.back() != rootEngine_) rootOnly = false;
  }
  if (!rootOnly) refreshDerivativeMatrices();  // the preorder pass reads dP / d2P of every branch
  NodePosteriors out;
  const size_t n = eng.size() * nbDistinctSites_;
  if (joint) out.joint.resize(n * nbClasses_ * nbStates_);
  if (states) out.statePost.resize(n * nbStates_);
  if (classes) out.classPost.resize(n * nbClasses_);
  if (best) out.best.resize(n);
  check(plk_node_posteriors(engine_, (int)eng.size(), eng.data(), joint ? out.joint.data() : nullptr,
                            states ? out.statePost.data() : nullptr, classes ? out.classPost.data() : nullptr,
                            best ? out.best.data() : nullptr),
        "plk_node_posteriors");
  return out;
}

std::vector<int> AbstractPlkTreeLikelihood::getInnerNodesId() const {
  std::vector<int> ids;
  for (const Node* n : tree_->getNodes())
    if (!n->isLeaf()) ids.push_back(n->getId());
  return ids;
}

const std::vector<int>& AbstractPlkTreeLikelihood::getLeafPatternStates(int nodeId) const {
  const Node* n = tree_->getNode(nodeId);
  if (!n->isLeaf()) throw Exception("getLeafPatternStates: node " + TextTools::toString(nodeId) + " is not a leaf");
  return patternStates_.at((size_t)engineIndex_.at(n));
}

VVdouble AbstractPlkTreeLikelihood::getLeafLikelihoods(int nodeId) const {
  const std::vector<int>& st = getLeafPatternStates(nodeId);
  const SubstitutionModel* m = getModelForNode(nodeId);
  VVdouble out(nbDistinctSites_, Vdouble(nbStates_));
  for (size_t i = 0; i < nbDistinctSites_; i++)
    for (size_t x = 0; x < nbStates_; x++) out[i][x] = m->getInitValue(x, st[i]);
  return out;
}

VVdouble AbstractPlkTreeLikelihood::getPosteriorProbabilitiesOfEachRate() const {
  const NodePosteriors p =
      computeNodePosteriors(std::vector<int>(1, tree_->getRootNode()->getId()), false, false, true, false);
  VVdouble out(nbSites_, Vdouble(nbClasses_));
  for (size_t i = 0; i < nbSites_; i++)
    for (size_t c = 0; c < nbClasses_; c++) out[i][c] = p.classPost[rootPatternLinks_[i] * nbClasses_ + c];
  return out;
}

Vdouble AbstractPlkTreeLikelihood::getPosteriorRateOfEachSite() const {
  const VVdouble post = getPosteriorProbabilitiesOfEachRate();
  const Vdouble& rates = rateDistribution_->getCategories();
  Vdouble out(nbSites_, 0.);
  for (size_t i = 0; i < nbSites_; i++)
    for (size_t c = 0; c < nbClasses_; c++) out[i] += rates[c] * post[i][c];
  return out;
}

std::vector<size_t> AbstractPlkTreeLikelihood::getRateClassWithMaxPostProbOfEachSite() const {
  const VVdouble post = getPosteriorProbabilitiesOfEachRate();
  std::vector<size_t> out(nbSites_);
  for (size_t i = 0; i < nbSites_; i++) out[i] = VectorTools::whichMax(post[i]);
  return out;
}

// ---------------------------------------------------------------------------

VVVdouble DRTreeLikelihoodTools::getPosteriorProbabilitiesForEachStateForEachRate(const DRTreeLikelihood& drl,
                                                                                 int nodeId) {
  const size_t nSites = drl.getNumberOfDistinctSites(), nC = drl.getNumberOfClasses(), nS = drl.getNumberOfStates();
  VVVdouble post(nSites, VVdouble(nC, Vdouble(nS, 0.)));
  if (drl.isLeafNode(nodeId)) {
    // the leaf's init values, normalised over the states, times the class probability
    const VVdouble leaf = drl.getLeafLikelihoods(nodeId);
    const Vdouble& pc = drl.getRateDistribution()->getProbabilities();
    for (size_t i = 0; i < nSites; i++) {
      const double sum = VectorTools::sum(leaf[i]);
      for (size_t c = 0; c < nC; c++)
        for (size_t x = 0; x < nS; x++) post[i][c][x] = leaf[i][x] * pc[c] / sum;
    }
    return post;
  }
  const AbstractPlkTreeLikelihood::NodePosteriors p =
      drl.computeNodePosteriors(std::vector<int>(1, nodeId), true, false, false, false);
  for (size_t i = 0; i < nSites; i++)
    for (size_t c = 0; c < nC; c++)
      for (size_t x = 0; x < nS; x++) post[i][c][x] = p.joint[(i * nC + c) * nS + x];
  return post;
}

Vdouble DRTreeLikelihoodTools::getPosteriorStateFrequencies(const DRTreeLikelihood& drl, int nodeId) {
  const VVVdouble probs = getPosteriorProbabilitiesForEachStateForEachRate(drl, nodeId);
  const std::vector<unsigned int>& w = drl.getWeights();
  Vdouble freqs(drl.getNumberOfStates(), 0.);
  double sumw = 0.;
  for (size_t i = 0; i < probs.size(); i++) {
    sumw += w[i];
    for (size_t c = 0; c < probs[i].size(); c++)
      for (size_t x = 0; x < freqs.size(); x++) freqs[x] += probs[i][c][x] * w[i];
  }
  for (double& f : freqs) f /= sumw;
  return freqs;
}

// ---------------------------------------------------------------------------

MarginalAncestralStateReconstruction::MarginalAncestralStateReconstruction(const AbstractPlkTreeLikelihood* drl)
    : likelihood_(drl) {
  if (!drl) throw NullPointerException("MarginalAncestralStateReconstruction: null likelihood");
  if (!drl->isInitialized()) throw Exception("MarginalAncestralStateReconstruction: likelihood is not initialized.");
}

std::vector<size_t> MarginalAncestralStateReconstruction::getAncestralStatesForNode(int nodeId, VVdouble& probs,
                                                                                     bool sample) const {
  const size_t nSites = likelihood_->getNumberOfDistinctSites(), nS = likelihood_->getNumberOfStates();
  std::vector<size_t> anc(nSites, 0);
  probs.assign(nSites, Vdouble(nS, 0.));
  if (likelihood_->isLeafNode(nodeId)) {
    const VVdouble leaf = likelihood_->getLeafLikelihoods(nodeId);
    for (size_t i = 0; i < nSites; i++) anc[i] = ancestral::oneHot(leaf[i], probs[i]);
    return anc;
  }
  const AbstractPlkTreeLikelihood::NodePosteriors p =
      likelihood_->computeNodePosteriors(std::vector<int>(1, nodeId), false, true, false, !sample);
  for (size_t i = 0; i < nSites; i++) {
    std::copy(p.statePost.begin() + i * nS, p.statePost.begin() + (i + 1) * nS, probs[i].begin());
    anc[i] = sample ? ancestral::sampleState(probs[i], RandomTools::giveRandomNumberBetweenZeroAndEntry(1.))
                    : (size_t)p.best[i];
  }
  return anc;
}

std::vector<size_t> MarginalAncestralStateReconstruction::getAncestralStatesForNode(int nodeId) const {
  if (likelihood_->isLeafNode(nodeId)) {
    VVdouble probs;
    return getAncestralStatesForNode(nodeId, probs, false);
  }
  const AbstractPlkTreeLikelihood::NodePosteriors p =
      likelihood_->computeNodePosteriors(std::vector<int>(1, nodeId), false, false, false, true);
  return std::vector<size_t>(p.best.begin(), p.best.end());
}

std::map<int, std::vector<size_t> > MarginalAncestralStateReconstruction::getAllAncestralStates() const {
  std::map<int, std::vector<size_t> > anc;
  const size_t nSites = likelihood_->getNumberOfDistinctSites();
  const std::vector<int> inner = likelihood_->getInnerNodesId();
  const AbstractPlkTreeLikelihood::NodePosteriors p = likelihood_->computeNodePosteriors(inner, false, false, false, true);
  for (size_t k = 0; k < inner.size(); k++)
    anc[inner[k]].assign(p.best.begin() + k * nSites, p.best.begin() + (k + 1) * nSites);
  // leaves: their observed sequences (an ambiguous state: the first model state it allows)
  for (int id : likelihood_->getTree().getNodesId()) {
    if (!likelihood_->isLeafNode(id)) continue;
    VVdouble probs;
    anc[id] = getAncestralStatesForNode(id, probs, false);
  }
  return anc;
}

Sequence* MarginalAncestralStateReconstruction::getAncestralSequenceForNode(int nodeId, VVdouble* probs,
                                                                            bool sample) const {
  VVdouble patterned;
  const std::vector<size_t> states = getAncestralStatesForNode(nodeId, patterned, sample);
  const std::vector<size_t>& links = likelihood_->getRootArrayPositions();
  const SubstitutionModel* model = likelihood_->getModelForNode(nodeId);
  const std::vector<size_t> perSite = ancestral::expandPatterns(states, links);
  std::vector<int> all(perSite.size());
  for (size_t i = 0; i < perSite.size(); i++) all[i] = model->getAlphabetStateAsInt(perSite[i]);
  if (probs) *probs = ancestral::expandPatterns(patterned, links);
  return new BasicSequence(TextTools::toString(nodeId), all, likelihood_->getAlphabet());
}

}  // namespace bpp
