// Likelihood/PairedSiteLikelihoods.h: per-site log-likelihoods of several models (or trees) on
// the same sites, and RELL resampling over them.  The reference's
// computeExpectedLikelihoodWeights (Likelihood/PairedSiteLikelihoods.cpp:124-176) draws one count
// vector per replicate and sums lnL[model][site] * count[site] in a triple host loop.  Here all
// count vectors are drawn first (the same draws in the same order), the sums of all replicates
// and models come from one plk_replicate_sums call on a scratch handle whose patterns are the
// sites, and the reference's per-replicate softmax average runs on those sums.  Deviations: the
// mirror's trees carry no name, so appendModel(const TreeLikelihood&) takes the name to record;
// getNumberOfSites() of a container without models is 0, where the reference throws;
// computeExpectedLikelihoodWeights takes the device of its scratch handle.
#ifndef BPP_AMD_PAIREDSITELIKELIHOODS_H
#define BPP_AMD_PAIREDSITELIKELIHOODS_H

#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "TreeLikelihood.h"

namespace bpp {

class PairedSiteLikelihoods {
  std::vector<std::vector<double> > logLikelihoods_;
  std::vector<std::string> modelNames_;

 public:
  PairedSiteLikelihoods() {}
  PairedSiteLikelihoods(const std::vector<std::vector<double> >& siteLogLikelihoods,
                        const std::vector<std::string>& modelNames = std::vector<std::string>());

  void appendModel(const std::vector<double>& siteLogLikelihoods, const std::string& modelName = "");
  void appendModel(const TreeLikelihood& treeLikelihood, const std::string& modelName = "");
  void appendModels(const PairedSiteLikelihoods& psl);

  const std::vector<double>& getLogLikelihoods(std::size_t model) const { return logLikelihoods_.at(model); }
  const std::vector<std::vector<double> >& getLogLikelihoods() const { return logLikelihoods_; }
  const std::string& getModelName(std::size_t model) const { return modelNames_.at(model); }
  const std::vector<std::string>& getModelNames() const { return modelNames_; }
  void setName(std::size_t model, const std::string& name) { modelNames_.at(model) = name; }
  void setNames(const std::vector<std::string>& names);
  std::size_t getNumberOfSites() const { return logLikelihoods_.empty() ? 0 : logLikelihoods_[0].size(); }
  std::size_t getNumberOfModels() const { return logLikelihoods_.size(); }

  // counts of floor(length * scaling + 0.5) draws over `length` sites (RandomTools)
  static std::vector<int> bootstrap(std::size_t length, double scaling = 1);

  // (names, weights): the mean over the replicates of exp(Y_m - max Y) / sum_m exp(Y_m - max Y),
  // Y_m the replicate's resampled log-likelihood of model m.  One engine call, on a scratch
  // handle created on `device` and destroyed before the call returns.
  std::pair<std::vector<std::string>, std::vector<double> > computeExpectedLikelihoodWeights(int replicates = 10000,
                                                                                             int device = 0) const;

  // the arithmetic after the sums: G is replicates x models, replicate-major
  static std::vector<double> expectedLikelihoodWeightsFromSums(const std::vector<double>& G, std::size_t replicates,
                                                               std::size_t models);
};

}  // namespace bpp

#endif
