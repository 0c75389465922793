// NNI topology search through the Bio++ API mirror on the MI355X: NNITopologySearch (BETTER and
// FAST) over an NNIHomogeneousTreeLikelihood, on 2000 sites simulated on a 10-taxon tree under
// GTR + Gamma(4).  The topology is perturbed by three interchanges, then searched.  Checks: the
// perturbation lowered lnL; the final lnL is not below the true tree's on the same data minus
// 1e-6; every accepted testNNI value equals the change of getValue() that doNNI produced (1e-8
// relative); every round of either algorithm cost one plk_nni_scores call; the listener hooks
// fire once per applied interchange; testNNI of an unchanged object is served from the cache.
// Prints PASSED and exits 0 on success.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Likelihood/NNIHomogeneousTreeLikelihood.h>
#include <Bpp/Phyl/Model/Nucleotide/GTR.h>
#include <Bpp/Phyl/Model/RateDistribution/GammaDiscreteRateDistribution.h>
#include <Bpp/Phyl/NNITopologySearch.h>
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

// records the likelihood's value after every applied interchange
class ValueRecorder : public TopologyListener {
  const NNIHomogeneousTreeLikelihood* tl_;

 public:
  std::vector<double> values;
  size_t tested = 0;
  explicit ValueRecorder(const NNIHomogeneousTreeLikelihood* tl) : tl_(tl) {}
  void topologyChangeTested(const TopologyChangeEvent&) override { tested++; }
  void topologyChangePerformed(const TopologyChangeEvent&) override { values.push_back(tl_->getValue()); }
};

static std::vector<int> candidates(const Tree& t) {
  const TreeTemplate<Node> tree(t);
  std::vector<int> ids;
  for (const Node* n : tree.getNodes())
    if (n->hasFather() && n->getFather()->hasFather()) ids.push_back(n->getId());
  return ids;
}

static void run(const std::string& algorithm, const TreeTemplate<Node>& tree, const SiteContainer& sites,
                SubstitutionModel* model, DiscreteDistribution* rdist) {
  NNIHomogeneousTreeLikelihood tl(tree, sites, model, rdist, true, false);
  tl.initialize();
  const double trueValue = tl.getValue();
  std::cout << algorithm << ": true tree -lnL = " << std::setprecision(14) << trueValue << ", "
            << tl.getNumberOfDistinctSites() << " patterns" << std::endl;

  // the cache: a second test of an unchanged object is no engine call, and every node is scored
  const std::vector<int> ids0 = candidates(tl.getTopology());
  expect(algorithm + ": 2 (n - 3) = 14 nodes to test", ids0.size() == 14);
  const double first = tl.testNNI(ids0[0]);
  for (int id : ids0) tl.testNNI(id);
  expect(algorithm + ": one plk_nni_scores call scores every node", tl.getNumberOfScoreCalls() == 1);
  expect(algorithm + ": cached value is returned again", tl.testNNI(ids0[0]) == first);

  // three perturbing interchanges, each checked against the value it produces
  double value = trueValue;
  for (int k = 0; k < 3; k++) {
    const std::vector<int> ids = candidates(tl.getTopology());
    const int id = ids[(size_t)(3 + 4 * k) % ids.size()];
    const double diff = tl.testNNI(id);
    tl.doNNI(id);
    const double now = tl.getValue();
    expect(algorithm + ": perturbing interchange " + std::to_string(k) + " changes -lnL by its testNNI value",
           std::fabs((now - value) - diff) <= 1e-8 * std::max(1., std::fabs(diff)));
    value = now;
  }
  std::cout << algorithm << ": perturbed -lnL = " << value << std::endl;
  expect(algorithm + ": the perturbation lowered lnL", value > trueValue + 1.);

  const size_t callsBefore = tl.getNumberOfScoreCalls();
  NNITopologySearch search(tl, algorithm, 0);
  ValueRecorder rec(&tl);
  search.addTopologyListener(&rec);
  search.search();
  const std::vector<double>& acc = search.getAcceptedImprovements();
  const double final = tl.getValue();
  std::cout << algorithm << ": " << search.getNumberOfRounds() << " rounds, " << acc.size()
            << " interchanges, final -lnL = " << final << std::endl;
  expect(algorithm + ": interchanges were applied", !acc.empty());
  expect(algorithm + ": the listener saw every applied interchange", rec.values.size() == acc.size());
  expect(algorithm + ": the listener saw the tests", rec.tested >= acc.size());
  expect(algorithm + ": final lnL is not below the true tree's", -final >= -trueValue - 1e-6);
  bool agree = true;
  double prev = value, worst = 0.;
  for (size_t i = 0; i < acc.size() && i < rec.values.size(); i++) {
    const double change = rec.values[i] - prev;
    const double err = std::fabs(change - acc[i]) / std::max(1., std::fabs(change));
    worst = std::max(worst, err);
    agree = agree && acc[i] < 0. && err <= 1e-8;
    prev = rec.values[i];
  }
  std::cout << algorithm << ": worst |testNNI - change of getValue()| = " << worst << " (relative)" << std::endl;
  expect(algorithm + ": every accepted testNNI value is the change of getValue()", agree);
  expect(algorithm + ": getTopologyValue() is the value", tl.getTopologyValue() == final);
  expect(algorithm + ": one plk_nni_scores call per round",
         tl.getNumberOfScoreCalls() - callsBefore == search.getNumberOfRounds());
  // the optimisers still see the re-estimated lengths
  const ParameterList bl = tl.getBranchLengthsParameters();
  tl.setParameters(bl);
  expect(algorithm + ": the BrLen parameters carry the tree's lengths",
         std::fabs(tl.getValue() - final) <= 1e-9 * std::fabs(final));
}

int main() {
  try {
    std::unique_ptr<TreeTemplate<Node> > tree(TreeTemplateTools::parenthesisToTree(
        "(((A:0.12,B:0.2):0.08,(C:0.1,D:0.25):0.07):0.06,((E:0.15,F:0.1):0.09,G:0.2):0.07,"
        "((H:0.18,I:0.12):0.08,J:0.22):0.1);"));
    const NucleicAlphabet* dna = &AlphabetTools::DNA_ALPHABET;
    GTR model(dna, 1, 0.2, 0.3, 0.4, 0.4, 0.1, 0.35, 0.35, 0.2);
    GammaDiscreteRateDistribution rdist(4, 0.6);
    RandomTools::setSeed(20261020);
    HomogeneousSequenceSimulator simulator(&model, &rdist, tree.get());
    std::unique_ptr<SiteContainer> sites(simulator.simulate(2000));
    run(NNITopologySearch::BETTER, *tree, *sites, &model, &rdist);
    run(NNITopologySearch::FAST, *tree, *sites, &model, &rdist);
  } catch (std::exception& e) {
    std::cout << "exception: " << e.what() << std::endl;
    return 1;
  }
  if (failures) {
    std::cout << failures << " check(s) FAILED" << std::endl;
    return 1;
  }
  std::cout << "PASSED" << std::endl;
  return 0;
}
