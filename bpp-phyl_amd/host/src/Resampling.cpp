// Host mirror: RELL resampling over plk_replicate_sums -- PairedSiteLikelihoods (expected
// likelihood weights) and the local bootstrap of NNIHomogeneousTreeLikelihood.  Clean-room; see
// the headers for what the reference does instead.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>

#include "Bpp/Numeric/Random/RandomTools.h"
#include "Bpp/Phyl/Likelihood/NNIHomogeneousTreeLikelihood.h"
#include "Bpp/Phyl/Likelihood/PairedSiteLikelihoods.h"
#include "plk.h"

namespace bpp {

// ---------------------------------------------------------------------------
// PairedSiteLikelihoods
// ---------------------------------------------------------------------------

namespace {
// every record of a container covers the same sites: `got` values where `want` are held
void requireSites(const char* who, std::size_t got, std::size_t want) {
  if (got != want)
    throw Exception(std::string("PairedSiteLikelihoods::") + who + ": a record of " + std::to_string(got) +
                    " site log-likelihoods cannot join records of " + std::to_string(want) + " sites.");
}
}  // namespace

// The records go in one by one through appendModel, which checks their lengths; names are
// optional as a whole (none given: every model gets an empty name).
PairedSiteLikelihoods::PairedSiteLikelihoods(const std::vector<std::vector<double> >& siteLogLikelihoods,
                                             const std::vector<std::string>& modelNames) {
  const bool named = !modelNames.empty();
  if (named && modelNames.size() != siteLogLikelihoods.size())
    throw Exception("PairedSiteLikelihoods: " + std::to_string(modelNames.size()) + " names were given for " +
                    std::to_string(siteLogLikelihoods.size()) + " models.");
  for (std::size_t m = 0; m < siteLogLikelihoods.size(); m++)
    appendModel(siteLogLikelihoods[m], named ? modelNames[m] : std::string());
}

void PairedSiteLikelihoods::appendModel(const std::vector<double>& siteLogLikelihoods, const std::string& modelName) {
  if (!logLikelihoods_.empty()) requireSites("appendModel", siteLogLikelihoods.size(), getNumberOfSites());
  logLikelihoods_.push_back(siteLogLikelihoods);
  modelNames_.push_back(modelName);
}

void PairedSiteLikelihoods::appendModel(const TreeLikelihood& treeLikelihood, const std::string& modelName) {
  appendModel(treeLikelihood.getLogLikelihoodForEachSite(), modelName);
}

void PairedSiteLikelihoods::appendModels(const PairedSiteLikelihoods& psl) {
  // (an empty container on either side has no site count to disagree with)
  if (!logLikelihoods_.empty() && !psl.logLikelihoods_.empty())
    requireSites("appendModels", psl.getNumberOfSites(), getNumberOfSites());
  for (std::size_t m = 0; m < psl.getNumberOfModels(); m++) {
    logLikelihoods_.push_back(psl.logLikelihoods_[m]);
    modelNames_.push_back(psl.modelNames_[m]);
  }
}

void PairedSiteLikelihoods::setNames(const std::vector<std::string>& names) {
  if (names.size() != getNumberOfModels())
    throw Exception("PairedSiteLikelihoods::setNames: " + std::to_string(names.size()) + " names for " +
                    std::to_string(getNumberOfModels()) + " models.");
  modelNames_ = names;
}

// A pseudoreplicate as site counts: round(length * scaling) sites drawn with replacement, each
// draw one RandomTools integer below `length` (so a seed fixes the replicate).
std::vector<int> PairedSiteLikelihoods::bootstrap(std::size_t length, double scaling) {
  std::vector<int> counts(length, 0);
  std::size_t left = static_cast<std::size_t>(std::floor(static_cast<double>(length) * scaling + 0.5));
  while (left-- > 0) counts[RandomTools::giveIntRandomNumberBetweenZeroAndEntry<std::size_t>(length)]++;
  return counts;
}

std::vector<double> PairedSiteLikelihoods::expectedLikelihoodWeightsFromSums(const std::vector<double>& G,
                                                                             std::size_t replicates, std::size_t models) {
  if (G.size() != replicates * models) throw Exception("PairedSiteLikelihoods: the sums are not replicates x models.");
  std::vector<double> weights(models, 0.), e(models);
  for (std::size_t r = 0; r < replicates; r++) {
    const double* y = G.data() + r * models;
    const double ymax = *std::max_element(y, y + models);
    for (std::size_t m = 0; m < models; m++) e[m] = std::exp(y[m] - ymax);
    const double sum = std::accumulate(e.begin(), e.end(), 0.0);
    for (std::size_t m = 0; m < models; m++) weights[m] += e[m] / sum;
  }
  for (double& w : weights) w /= static_cast<double>(replicates);
  return weights;
}

namespace {
void checkPlk(plk_handle h, int rc, const char* what) {
  if (rc != PLK_OK) {
    const std::string msg = std::string(what) + ": " + plk_last_error(h);
    if (h) plk_destroy(h);
    throw Exception(msg);
  }
}
}  // namespace

std::pair<std::vector<std::string>, std::vector<double> > PairedSiteLikelihoods::computeExpectedLikelihoodWeights(
    int replicates, int device) const {
  const std::size_t M = getNumberOfModels(), n = getNumberOfSites(), R = replicates > 0 ? (std::size_t)replicates : 0;
  if (M == 0 || n == 0 || R == 0) return std::make_pair(modelNames_, std::vector<double>(M, 0.));
  // every replicate's counts first, in the reference's order of draws
  std::vector<double> W(R * n);
  for (std::size_t r = 0; r < R; r++) {
    const std::vector<int> c = bootstrap(n);
    std::copy(c.begin(), c.end(), W.begin() + r * n);
  }
  // a scratch handle of the smallest legal shape whose patterns are the sites
  plk_handle h = nullptr;
  checkPlk(nullptr, plk_create(device, 2, 1, (int64_t)n, 0, 1, 1, 0, &h), "plk_create");
  checkPlk(h, plk_site_rows_reserve(h, (int)M), "plk_site_rows_reserve");
  for (std::size_t m = 0; m < M; m++) checkPlk(h, plk_site_row_set(h, (int)m, logLikelihoods_[m].data()), "plk_site_row_set");
  checkPlk(h, plk_set_replicate_weights(h, (int)R, W.data()), "plk_set_replicate_weights");
  std::vector<double> G(R * M);
  checkPlk(h, plk_replicate_sums(h, 0, (int)M, G.data(), nullptr), "plk_replicate_sums");
  plk_destroy(h);
  return std::make_pair(modelNames_, expectedLikelihoodWeightsFromSums(G, R, M));
}

// ---------------------------------------------------------------------------
// NNIHomogeneousTreeLikelihood: local bootstrap
// ---------------------------------------------------------------------------

std::vector<double> NNIHomogeneousTreeLikelihood::localBootstrapFromSums(const std::vector<double>& G, size_t replicates,
                                                                         const std::vector<size_t>& rivals) {
  const size_t n = std::accumulate(rivals.begin(), rivals.end(), (size_t)0);
  if (G.size() != replicates * n) throw Exception("localBootstrapFromSums: the sums are not replicates x rivals.");
  std::vector<double> lbp(rivals.size(), 0.);
  for (size_t r = 0; r < replicates; r++) {
    const double* g = G.data() + r * n;
    for (size_t b = 0; b < rivals.size(); g += rivals[b], b++) {
      size_t tied = 1;
      bool beaten = false;
      for (size_t k = 0; k < rivals[b]; k++) {
        beaten = beaten || g[k] > 0.;
        tied += g[k] == 0. ? 1 : 0;
      }
      if (!beaten) lbp[b] += 1. / static_cast<double>(tied);
    }
  }
  if (replicates > 0)
    for (double& v : lbp) v /= static_cast<double>(replicates);
  return lbp;
}

std::map<int, double> NNIHomogeneousTreeLikelihood::computeLocalBootstrap(size_t nReplicates) const {
  if (!initialized_) throw Exception("NNIHomogeneousTreeLikelihood::computeLocalBootstrap(). Object not initialized.");
  lbpIds_.clear();
  lbpRivals_.clear();
  std::vector<int32_t> son, uncle;
  std::vector<double> t;
  for (const Node* p : nodes_) {
    if (p->isLeaf() || !p->hasFather()) continue;
    const Node* g = p->getFather();
    if (p->getNumberOfSons() > 3 || g->getNumberOfSons() > 3 || p->getNumberOfSons() < 2) continue;
    lbpIds_.push_back(p->getId());
    lbpRivals_.push_back(p->getNumberOfSons());
    for (size_t k = 0; k < p->getNumberOfSons(); k++) {
      const Node* s = p->getSon(k);
      son.push_back(engineIndex_.at(s));
      uncle.push_back(engineIndex_.at(uncleOf(s)));
      t.push_back(getBestBranchLength(s->getId()));  // the cached scores; one call if there are none
    }
  }
  std::map<int, double> out;
  if (lbpIds_.empty() || nReplicates == 0) return out;
  const size_t n = son.size(), P = nbDistinctSites_;
  // the replicates' counts per site, added up per pattern
  std::vector<double> W(nReplicates * P, 0.);
  for (size_t r = 0; r < nReplicates; r++) {
    const std::vector<int> c = PairedSiteLikelihoods::bootstrap(nbSites_);
    double* w = W.data() + r * P;
    for (size_t i = 0; i < nbSites_; i++) w[rootPatternLinks_[i]] += c[i];
  }
  refreshDerivativeMatrices();  // the preorder pass reads dP / d2P of every branch
  check(plk_site_rows_reserve(engine_, (int)n), "plk_site_rows_reserve");
  check(plk_nni_site_rows(engine_, (int)n, son.data(), uncle.data(), nullptr, t.data(), 0), "plk_nni_site_rows");
  check(plk_set_replicate_weights(engine_, (int)nReplicates, W.data()), "plk_set_replicate_weights");
  std::vector<double> G(nReplicates * n);
  check(plk_replicate_sums(engine_, 0, (int)n, G.data(), nullptr), "plk_replicate_sums");
  const std::vector<double> lbp = localBootstrapFromSums(G, nReplicates, lbpRivals_);
  for (size_t b = 0; b < lbpIds_.size(); b++) out[lbpIds_[b]] = lbp[b];
  return out;
}

void NNIHomogeneousTreeLikelihood::releaseLocalBootstrap() const {
  if (!engine_) return;
  check(plk_set_replicate_weights(engine_, 0, nullptr), "plk_set_replicate_weights");
  check(plk_site_rows_reserve(engine_, 0), "plk_site_rows_reserve");
}

}  // namespace bpp
