// Probabilistic substitution mapping through the Bio++ API mirror on the MI355X:
// SubstitutionMappingTools::computeSubstitutionVectors over a DecompositionSubstitutionCount
// with the total and the comprehensive register, on 20000 simulated sites of the tree
// ((A:0.1,B:0.2):0.15,C:0.1,D:0.3) under the reference test's GTR, with a constant rate and
// with Gamma(4).  Checks: per (branch, site) the comprehensive types sum to the total count
// (1e-10); per branch the summed total count is within 10 % of nSites * t_v (the posterior
// expectation's relative sd is at most 1 / sqrt(nSites * t_v), about 2.2 % on the shortest
// branch, so the reference test's own 10 % margin is more than four sd); a user-defined
// SubstitutionCount goes through the host-matrix path (plk_set_count_matrix) and agrees
// with the device's own count matrices to 1e-9.  Prints PASSED and exits 0 on success.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Likelihood/DRHomogeneousTreeLikelihood.h>
#include <Bpp/Phyl/Mapping/DecompositionSubstitutionCount.h>
#include <Bpp/Phyl/Mapping/ProbabilisticSubstitutionMapping.h>
#include <Bpp/Phyl/Mapping/SubstitutionMappingTools.h>
#include <Bpp/Phyl/Mapping/SubstitutionRegister.h>
#include <Bpp/Phyl/Model/Nucleotide/GTR.h>
#include <Bpp/Phyl/Model/RateDistribution/ConstantRateDistribution.h>
#include <Bpp/Phyl/Model/RateDistribution/GammaDiscreteRateDistribution.h>
#include <Bpp/Phyl/Simulation/HomogeneousSequenceSimulator.h>
#include <Bpp/Phyl/TreeTemplate.h>
#include <Bpp/Seq/Alphabet/AlphabetTools.h>

#include <cmath>
#include <iomanip>
#include <iostream>
#include <memory>

using namespace bpp;

static int failures = 0;

static void expect(const std::string& what, bool ok) {
  std::cout << what << (ok ? " ok" : " FAIL") << std::endl;
  if (!ok) failures++;
}

static void expectNear(const std::string& what, double got, double want, double tol) {
  const bool ok = std::fabs(got - want) <= tol;
  std::cout << std::setprecision(12) << what << " = " << got << " (expected " << want << ", tol " << tol << ") "
            << (ok ? "ok" : "FAIL") << std::endl;
  if (!ok) failures++;
}

// A count the mirror knows nothing about: the decomposition's host matrices behind the plain
// SubstitutionCount interface, so the mapping takes the plk_set_count_matrix path.
class UserCount : public AbstractSubstitutionCount {
  DecompositionSubstitutionCount inner_;

 public:
  UserCount(const SubstitutionModel* model, SubstitutionRegister* reg)
      : AbstractSubstitutionCount(model, reg), inner_(model, reg->clone()) {}
  UserCount* clone() const override { return new UserCount(*this); }
  double getNumberOfSubstitutions(size_t i, size_t j, double length, size_t type = 1) const override {
    return inner_.getNumberOfSubstitutions(i, j, length, type);
  }
  RowMatrix<double>* getAllNumbersOfSubstitutions(double length, size_t type = 1) const override {
    return inner_.getAllNumbersOfSubstitutions(length, type);
  }
};

static void run(const std::string& label, DiscreteDistribution* rdist) {
  std::unique_ptr<TreeTemplate<Node> > tree(TreeTemplateTools::parenthesisToTree("((A:0.1,B:0.2):0.15,C:0.1,D:0.3);"));
  const NucleicAlphabet* dna = &AlphabetTools::DNA_ALPHABET;
  GTR model(dna, 1, 0.2, 0.3, 0.4, 0.4, 0.1, 0.35, 0.35, 0.2);
  const size_t n = 20000;
  RandomTools::setSeed(20261019);
  HomogeneousSequenceSimulator simulator(&model, rdist, tree.get());
  std::unique_ptr<SiteContainer> sites(simulator.simulate(n));
  DRHomogeneousTreeLikelihood tl(*tree, *sites, &model, rdist, true, false);
  tl.initialize();
  const double lnl0 = tl.getValue();
  std::cout << label << ": -lnL = " << std::setprecision(12) << lnl0 << ", " << tl.getNumberOfDistinctSites()
            << " patterns" << std::endl;

  // registers: total and comprehensive; the host count functions first (API parity)
  DecompositionSubstitutionCount countDet(&model, new ComprehensiveSubstitutionRegister(&model));
  DecompositionSubstitutionCount countTot(&model, new TotalSubstitutionRegister(&model));
  expect(label + ": register sizes", countTot.getNumberOfSubstitutionTypes() == 1 && countDet.getNumberOfSubstitutionTypes() == 12);
  {
    // the expected total number of substitutions at stationarity is the branch length
    std::unique_ptr<RowMatrix<double> > N(countTot.getAllNumbersOfSubstitutions(0.3, 1));
    const RowMatrix<double>& P = model.getPij_t(0.3);
    double mean = 0., detSum = 0.;
    for (size_t x = 0; x < 4; x++)
      for (size_t y = 0; y < 4; y++) mean += model.freq(x) * P(x, y) * (*N)(x, y);
    expectNear(label + ": E[total count] over a branch of length 0.3", mean, 0.3, 1e-12);
    for (size_t k = 1; k <= 12; k++) detSum += countDet.getNumberOfSubstitutions(0, 2, 0.3, k);
    expectNear(label + ": comprehensive types sum to the total (host, A -> G)", detSum,
               countTot.getNumberOfSubstitutions(0, 2, 0.3, 1), 1e-12);
    const ComprehensiveSubstitutionRegister reg(&model);
    expect(label + ": comprehensive register numbering",
           reg.getType(0, 0) == 0 && reg.getType(0, 1) == 1 && reg.getType(1, 0) == 4 && reg.getType(3, 2) == 12);
  }

  std::vector<int> ids = tl.getTree().getNodesId();
  ids.pop_back();  // the root
  std::unique_ptr<ProbabilisticSubstitutionMapping> mapDet(SubstitutionMappingTools::computeSubstitutionVectors(tl, ids, countDet, false));
  std::unique_ptr<ProbabilisticSubstitutionMapping> mapTot(SubstitutionMappingTools::computeSubstitutionVectors(tl, ids, countTot, false));
  expect(label + ": mapping sizes", mapDet->getNumberOfSites() == n && mapDet->getNumberOfBranches() == ids.size() &&
                                        mapDet->getNumberOfSubstitutionTypes() == 12 &&
                                        mapTot->getNumberOfSubstitutionTypes() == 1 && mapTot->getNumberOfSites() == n);
  const TreeTemplate<Node>& ltt = dynamic_cast<const TreeTemplate<Node>&>(tl.getTree());
  double worstSum = 0.;
  bool nonneg = true, forms = true;
  for (size_t j = 0; j < ids.size(); j++) {
    double total = 0.;
    for (size_t i = 0; i < n; i++) {
      const std::vector<double> det = mapDet->getNumberOfSubstitutions(ids[j], i);
      const double tot = mapTot->getNumberOfSubstitutions(ids[j], i, 0);
      double s = 0.;
      for (double v : det) {
        s += v;
        nonneg = nonneg && v >= 0.;
      }
      worstSum = std::max(worstSum, std::fabs(s - tot));
      forms = forms && (*mapTot)(mapTot->getNodeIndex(ids[j]), i, 0) == tot && det[5] == mapDet->getNumberOfSubstitutions(ids[j], i, 5);
      total += tot;
    }
    const double t = ltt.getNode(ids[j])->getDistanceToFather();
    std::cout << label << ": branch above node " << ids[j] << " (t = " << t << "): summed total count " << total
              << ", nSites * t = " << n * t << std::endl;
    expect(label + ": summed total count within 10 % of nSites * t", std::fabs(total - n * t) / (n * t) <= 0.1);
  }
  expectNear(label + ": comprehensive sum vs total per (branch, site), max abs", worstSum, 0., 1e-10);
  expect(label + ": counts are non-negative", nonneg);
  expect(label + ": accessor forms agree", forms);

  // every branch in one call with the default node list
  {
    std::unique_ptr<ProbabilisticSubstitutionMapping> all(SubstitutionMappingTools::computeSubstitutionVectors(tl, countTot, false));
    bool same = all->getNumberOfBranches() == ids.size();
    for (size_t j = 0; same && j < ids.size(); j++)
      for (size_t i = 0; same && i < n; i += 97)
        same = all->getNumberOfSubstitutions(ids[j], i, 0) == mapTot->getNumberOfSubstitutions(ids[j], i, 0);
    expect(label + ": the default node list is every branch", same);
  }

  // a user-defined count: host matrices through plk_set_count_matrix
  {
    UserCount user(&model, new ComprehensiveSubstitutionRegister(&model));
    std::unique_ptr<ProbabilisticSubstitutionMapping> mapUser(SubstitutionMappingTools::computeSubstitutionVectors(tl, ids, user, false));
    double worst = 0.;
    for (size_t j = 0; j < ids.size(); j++)
      for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < 12; k++)
          worst = std::max(worst, std::fabs(mapUser->getNumberOfSubstitutions(ids[j], i, k) -
                                            mapDet->getNumberOfSubstitutions(ids[j], i, k)));
    expectNear(label + ": host-matrix path vs device path, max abs", worst, 0., 1e-9);
  }
  expectNear(label + ": -lnL after the mappings", tl.getValue(), lnl0, 0.);

  // the root has no branch; a plain likelihood has no upper vectors
  bool threw = false;
  try {
    std::vector<int> bad(1, tl.getTree().getNodesId().back());
    std::unique_ptr<ProbabilisticSubstitutionMapping> m(SubstitutionMappingTools::computeSubstitutionVectors(tl, bad, countTot, false));
  } catch (Exception&) {
    threw = true;
  }
  expect(label + ": the root is refused", threw);
}

int main() {
  ConstantRateDistribution constant;
  run("constant rate", &constant);
  GammaDiscreteRateDistribution gamma(4, 0.5);
  run("Gamma(4)", &gamma);
  if (failures) {
    std::cout << failures << " FAILURES" << std::endl;
    return 1;
  }
  std::cout << "PASSED" << std::endl;
  return 0;
}
