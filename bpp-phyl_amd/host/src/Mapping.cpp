// Host mirror: probabilistic substitution mapping over plk_branch_counts
// (SubstitutionMappingTools::computeSubstitutionVectors, DecompositionSubstitutionCount).  The
// device forms the count matrices W^k_v and, from the double-recursive arrays, the counts
// n_k / l per branch, pattern and type; the host keeps the registers, the count classes'
// own formulas (API parity, and the matrices of counts the device does not form) and the
// pattern -> site expansion.
#include <cmath>
#include <map>
#include <mutex>

#include "Bpp/Phyl/Mapping/DecompositionSubstitutionCount.h"
#include "Bpp/Phyl/Mapping/SubstitutionMappingTools.h"
#include "Bpp/Text/TextTools.h"
#include "plk.h"

namespace bpp {

namespace {
std::mutex& countTypesMutex() {
  static std::mutex* m = new std::mutex;  // (never destroyed: likelihoods may outlive static destruction)
  return *m;
}
std::map<const plk_handle_s*, size_t>& countTypesTable() {
  static std::map<const plk_handle_s*, size_t>* t = new std::map<const plk_handle_s*, size_t>;
  return *t;
}
}  // namespace

size_t& engineCountTypes(const plk_handle_s* engine) {
  std::lock_guard<std::mutex> lock(countTypesMutex());
  return countTypesTable()[engine];  // (references into a std::map stay valid)
}

void forgetEngineCountTypes(const plk_handle_s* engine) {
  std::lock_guard<std::mutex> lock(countTypesMutex());
  countTypesTable().erase(engine);
}

std::string TotalSubstitutionRegister::getTypeName(size_t type) const {
  if (type == 0) return "nonsubstitution";
  if (type == 1) return "substitution";
  throw Exception("TotalSubstitutionRegister::getTypeName: bad substitution type " + TextTools::toString(type));
}

std::string ComprehensiveSubstitutionRegister::getTypeName(size_t type) const {
  if (type == 0) return "nonsubstitution";
  if (type > getNumberOfSubstitutionTypes())
    throw Exception("ComprehensiveSubstitutionRegister::getTypeName: bad substitution type " + TextTools::toString(type));
  const size_t s = model_->getNumberOfStates(), x = (type - 1) / (s - 1), r = (type - 1) % (s - 1);
  return TextTools::toString(x) + "->" + TextTools::toString(r < x ? r : r + 1);
}

// ---------------------------------------------------------------------------

DecompositionSubstitutionCount::DecompositionSubstitutionCount(const SubstitutionModel* model, SubstitutionRegister* reg)
    : AbstractSubstitutionCount(model, reg) {
  if (!model) throw NullPointerException("DecompositionSubstitutionCount: null model");
  if (!reg) throw NullPointerException("DecompositionSubstitutionCount: null register");
}

std::vector<double> DecompositionSubstitutionCount::getBMatrices() const {
  const size_t S = model_->getNumberOfStates(), T = getNumberOfSubstitutionTypes();
  std::vector<double> B(T * S * S, 0.);
  const RowMatrix<double>& Q = model_->getGenerator();
  for (size_t x = 0; x < S; x++)
    for (size_t y = 0; y < S; y++) {
      const size_t k = x == y ? 0 : register_->getType(x, y);
      if (k > 0) B[((k - 1) * S + x) * S + y] = Q(x, y) * model_->getRate();
    }
  return B;
}

RowMatrix<double> DecompositionSubstitutionCount::getCountsTimesP(double length, size_t type) const {
  const size_t S = model_->getNumberOfStates();
  if (type < 1 || type > getNumberOfSubstitutionTypes())
    throw Exception("DecompositionSubstitutionCount: bad substitution type " + TextTools::toString(type));
  for (double b : model_->getIEigenValues())
    if (b != 0.) throw Exception("DecompositionSubstitutionCount: complex eigen systems are not supported");
  const RowMatrix<double>& V = model_->getColumnRightEigenVectors();
  const RowMatrix<double>& Vi = model_->getRowLeftEigenVectors();
  const std::vector<double> Ball = getBMatrices();
  const double* B = Ball.data() + (type - 1) * S * S;
  // A = J o (V^-1 B V)
  RowMatrix<double> tmp(S, S), A(S, S), W(S, S);
  for (size_t i = 0; i < S; i++)
    for (size_t y = 0; y < S; y++) {
      double s = 0.;
      for (size_t x = 0; x < S; x++) s += Vi(i, x) * B[x * S + y];
      tmp(i, y) = s;
    }
  for (size_t i = 0; i < S; i++)
    for (size_t j = 0; j < S; j++) {
      double g = 0.;
      for (size_t y = 0; y < S; y++) g += tmp(i, y) * V(y, j);
      const double li = model_->getEigenValues()[i] * model_->getRate(), lj = model_->getEigenValues()[j] * model_->getRate();
      const double z = -std::fabs(li - lj) * length;
      const double phi = z == 0. ? 1. : std::expm1(z) / z;
      A(i, j) = g * length * std::exp(std::max(li, lj) * length) * phi;
    }
  for (size_t i = 0; i < S; i++)
    for (size_t y = 0; y < S; y++) {
      double s = 0.;
      for (size_t j = 0; j < S; j++) s += A(i, j) * Vi(j, y);
      tmp(i, y) = s;
    }
  for (size_t x = 0; x < S; x++)
    for (size_t y = 0; y < S; y++) {
      double s = 0.;
      for (size_t i = 0; i < S; i++) s += V(x, i) * tmp(i, y);
      W(x, y) = s > 0. ? s : 0.;
    }
  return W;
}

RowMatrix<double>* DecompositionSubstitutionCount::getAllNumbersOfSubstitutions(double length, size_t type) const {
  if (length < 0) throw Exception("DecompositionSubstitutionCount::getAllNumbersOfSubstitutions: negative branch length");
  const size_t S = model_->getNumberOfStates();
  const RowMatrix<double> W = getCountsTimesP(length, type);
  const RowMatrix<double>& P = model_->getPij_t(length);
  RowMatrix<double>* N = new RowMatrix<double>(S, S);
  for (size_t x = 0; x < S; x++)
    for (size_t y = 0; y < S; y++) {
      const double q = W(x, y) / P(x, y);
      (*N)(x, y) = std::isfinite(q) && q > 0. ? q : 0.;
    }
  return N;
}

double DecompositionSubstitutionCount::getNumberOfSubstitutions(size_t initialState, size_t finalState, double length,
                                                                size_t type) const {
  std::unique_ptr<RowMatrix<double> > N(getAllNumbersOfSubstitutions(length, type));
  return (*N)(initialState, finalState);
}

// ---------------------------------------------------------------------------

std::vector<double> AbstractPlkTreeLikelihood::computeBranchCounts(const std::vector<int>& nodeIds,
                                                                   SubstitutionCount& count) const {
  if (!initialized_) throw Exception("computeBranchCounts: instance is not initialized.");
  if (!(extraFlags_ & PLK_FLAG_DOUBLE_RECURSIVE))
    throw Exception("computeBranchCounts: substitution mapping needs a double-recursive likelihood.");
  if (!count.hasSubstitutionRegister()) throw Exception("computeBranchCounts: the count has no substitution register.");
  const size_t T = count.getNumberOfSubstitutionTypes(), S = nbStates_, C = nbClasses_;
  if (T < 1 || T > 16)
    throw Exception("computeBranchCounts: " + TextTools::toString(T) + " substitution types (the engine takes 1 to 16)");
  size_t& fixedTypes = engineCountTypes(engine_);
  if (fixedTypes && T > fixedTypes)
    throw Exception("computeBranchCounts: this likelihood's engine is fixed to " + TextTools::toString(fixedTypes) +
                    " substitution types; map the larger register first or on another likelihood object");
  const size_t Te = fixedTypes ? fixedTypes : T;  // (types T .. Te - 1 stay empty)
  std::vector<const Node*> nodes;
  std::vector<int32_t> eng, mod;
  std::vector<double> len;
  for (int id : nodeIds) {
    const Node* n = tree_->getNode(id);
    if (!n->hasFather()) throw Exception("computeBranchCounts: node " + TextTools::toString(id) + " is the root");
    nodes.push_back(n);
    eng.push_back(engineIndex_.at(n));
    mod.push_back(modelIndexForNode(n));
    len.push_back(n->getDistanceToFather());
  }
  if (eng.empty()) return std::vector<double>();
  refreshDerivativeMatrices();  // the preorder pass reads dP / d2P of every branch
  // the device forms W from the eigen system it holds: that of this likelihood's own model
  const DecompositionSubstitutionCount* dec = dynamic_cast<const DecompositionSubstitutionCount*>(&count);
  bool device = dec != nullptr;
  for (size_t i = 0; device && i < nodes.size(); i++) {
    const SubstitutionModel* m = modelForIndex(mod[i]);
    device = m == count.getSubstitutionModel() && !m->needsHostPij();
  }
  if (device) {
    std::vector<double> B = dec->getBMatrices();
    B.resize(Te * S * S, 0.);
    std::vector<char> sent(engineModels_, 0);
    for (int m : mod)
      if (!sent[(size_t)m]) {
        check(plk_set_count_types(engine_, m, (int)Te, B.data()), "plk_set_count_types");
        sent[(size_t)m] = 1;
      }
    fixedTypes = Te;
    check(plk_update_count_matrices(engine_, (int)eng.size(), eng.data(), mod.data(), len.data()),
          "plk_update_count_matrices");
  } else {
    const SubstitutionModel* m = count.getSubstitutionModel();
    if (!m || m->getNumberOfStates() != S) throw Exception("computeBranchCounts: the count's model does not fit the likelihood.");
    const Vdouble& rates = rateDistribution_->getCategories();
    std::vector<double> W(Te * C * S * S);
    for (size_t i = 0; i < eng.size(); i++) {
      std::fill(W.begin(), W.end(), 0.);
      for (size_t c = 0; c < C; c++) {
        const double tau = len[i] * rates[c];
        const RowMatrix<double> P = m->getPij_t(tau);
        for (size_t k = 0; k < T; k++) {
          std::unique_ptr<RowMatrix<double> > N(count.getAllNumbersOfSubstitutions(tau, k + 1));
          for (size_t x = 0; x < S; x++)
            for (size_t y = 0; y < S; y++) W[((k * C + c) * S + x) * S + y] = (*N)(x, y) * P(x, y);
        }
      }
      check(plk_set_count_matrix(engine_, eng[i], (int)Te, W.data()), "plk_set_count_matrix");
      fixedTypes = Te;
    }
  }
  std::vector<double> all(eng.size() * nbDistinctSites_ * Te);
  check(plk_branch_counts(engine_, (int)eng.size(), eng.data(), all.data(), nullptr), "plk_branch_counts");
  if (Te == T) return all;
  std::vector<double> out(eng.size() * nbDistinctSites_ * T);
  for (size_t r = 0; r < eng.size() * nbDistinctSites_; r++)
    std::copy(all.begin() + r * Te, all.begin() + r * Te + T, out.begin() + r * T);
  return out;
}

ProbabilisticSubstitutionMapping* SubstitutionMappingTools::computeSubstitutionVectors(
    const DRTreeLikelihood& drtl, const std::vector<int>& nodeIds, SubstitutionCount& substitutionCount, bool verbose) {
  if (!drtl.isInitialized()) throw Exception("SubstitutionMappingTools::computeSubstitutionVectors: likelihood is not initialized.");
  std::vector<int> ids = nodeIds;
  if (ids.empty()) {
    ids = drtl.getTree().getNodesId();  // postorder: the root comes last
    ids.pop_back();
  }
  const size_t nSites = drtl.getNumberOfSites(), nPat = drtl.getNumberOfDistinctSites();
  const size_t T = substitutionCount.getNumberOfSubstitutionTypes();
  if (verbose) ApplicationTools::displayTask("Compute joint node-pairs likelihood", true);
  const std::vector<double> counts = drtl.computeBranchCounts(ids, substitutionCount);
  ProbabilisticSubstitutionMapping* map = new ProbabilisticSubstitutionMapping(ids, nSites, T);
  const std::vector<size_t>& links = drtl.getRootArrayPositions();
  for (size_t b = 0; b < ids.size(); b++)
    for (size_t i = 0; i < nSites; i++)
      for (size_t k = 0; k < T; k++) (*map)(b, i, k) = counts[(b * nPat + links[i]) * T + k];
  if (verbose) ApplicationTools::displayTaskDone();
  return map;
}

}  // namespace bpp
