// Pairwise maximum-likelihood distances (Distance/DistanceEstimation.h of the reference).
//
// The reference optimises one TwoTreeLikelihood per pair of sequences on the host
// (DistanceEstimation.cpp:647-687).  Here computeMatrix() uploads the alignment's site patterns
// once and makes ONE plk_pair_distances call for all pairs: the device forms every pair's table
// of code-pair weights in one pass and runs a Newton ascent per pair on it (include/plk.h).
// Out of scope, throwing Exception: setOptimizer and a non-empty setAdditionalParameters (joint
// optimisation of model parameters with the distances), and the public TwoTreeLikelihood class.
#ifndef BPP_AMD_DISTANCEESTIMATION_H
#define BPP_AMD_DISTANCEESTIMATION_H

#include <memory>

#include "../../Numeric/Parameter.h"
#include "../../Numeric/Prob/DiscreteDistribution.h"
#include "../../Seq/Container/SiteContainer.h"
#include "../../Seq/DistanceMatrix.h"
#include "../Model/SubstitutionModel.h"

namespace bpp {

class Optimizer;

class DistanceEstimation {
  std::unique_ptr<TransitionModel> model_;
  std::unique_ptr<DiscreteDistribution> rateDist_;
  const SiteContainer* sites_ = nullptr;
  std::unique_ptr<DistanceMatrix> dist_;
  size_t verbose_ = 1;
  std::vector<double> lnl_;   // [pair] two-sequence log-likelihoods of the last computeMatrix()
  long long passes_ = 0;

 public:
  // (the model and the rate distribution become the object's, as in the reference)
  DistanceEstimation(TransitionModel* model, DiscreteDistribution* rateDist, size_t verbose = 1)
      : model_(model), rateDist_(rateDist), verbose_(verbose) {}
  DistanceEstimation(TransitionModel* model, DiscreteDistribution* rateDist, const SiteContainer* sites,
                     size_t verbose = 1, bool computeMat = true)
      : model_(model), rateDist_(rateDist), sites_(sites), verbose_(verbose) {
    if (computeMat) computeMatrix();
  }
  DistanceEstimation(const DistanceEstimation& d)
      : model_(d.model_ ? d.model_->clone() : nullptr), rateDist_(d.rateDist_ ? d.rateDist_->clone() : nullptr),
        sites_(d.sites_), dist_(d.dist_ ? d.dist_->clone() : nullptr), verbose_(d.verbose_), lnl_(d.lnl_),
        passes_(d.passes_) {}
  DistanceEstimation& operator=(const DistanceEstimation& d) {
    if (this != &d) {
      DistanceEstimation c(d);
      std::swap(model_, c.model_), std::swap(rateDist_, c.rateDist_), std::swap(dist_, c.dist_);
      sites_ = c.sites_, verbose_ = c.verbose_, lnl_ = c.lnl_, passes_ = c.passes_;
    }
    return *this;
  }
  virtual ~DistanceEstimation() {}
  DistanceEstimation* clone() const { return new DistanceEstimation(*this); }

  // t_min = 1e-6 (the reference's minimumBrLen_), t_max = 10000, Newton to 1e-8 in at most 40
  // passes after the first, every pair started from its share of differing resolved characters.
  void computeMatrix();
  // a new copy, null before computeMatrix()
  DistanceMatrix* getMatrix() const { return dist_ ? new DistanceMatrix(*dist_) : nullptr; }

  bool hasModel() const { return (bool)model_; }
  const TransitionModel& getModel() const {
    if (!model_) throw Exception("DistanceEstimation::getModel(). No model associated to this instance.");
    return *model_;
  }
  void resetSubstitutionModel(TransitionModel* model = nullptr) { model_.reset(model); }
  bool hasRateDistribution() const { return (bool)rateDist_; }
  const DiscreteDistribution& getRateDistribution() const {
    if (!rateDist_) throw Exception("DistanceEstimation::getRateDistribution(). No rate distribution associated to this instance.");
    return *rateDist_;
  }
  void resetRateDistribution(DiscreteDistribution* rateDist = nullptr) { rateDist_.reset(rateDist); }

  void setData(const SiteContainer* sites) { sites_ = sites; }
  const SiteContainer* getData() const { return sites_; }
  void resetData() { sites_ = nullptr; }

  void setOptimizer(const Optimizer*) { throw Exception("DistanceEstimation::setOptimizer: the distances are optimised on the device"); }
  void setAdditionalParameters(const ParameterList& parameters) {
    if (parameters.size() > 0)
      throw Exception("DistanceEstimation::setAdditionalParameters: joint optimisation of model parameters is not supported");
  }
  void resetAdditionalParameters() {}

  void setVerbose(size_t verbose) { verbose_ = verbose; }
  size_t getVerbose() const { return verbose_; }

  // Of the last computeMatrix(): the log-likelihood of the pair (i, j), i != j, at its distance,
  // and the evaluation passes the slowest pair took.
  double getPairLogLikelihood(size_t i, size_t j) const;
  long long getNumberOfPasses() const { return passes_; }
};

}  // namespace bpp

#endif
