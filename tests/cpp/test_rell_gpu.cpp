// RELL resampling through the Bio++ API mirror on the MI355X.  2000 sites are simulated under
// GTR + Gamma(4) on a 12-taxon tree with one internal branch of length 1e-3 (the rest >= 0.1);
// NNITopologySearch runs, then NNIHomogeneousTreeLikelihood::computeLocalBootstrap(1000).  Checks:
// every branch but the short one gets a proportion >= 0.95 and the short one stays below it; the
// proportions equal localBootstrapFromSums applied to the sums fetched through plk_replicate_sums
// from the rows and weights the call left on the engine; getValue() and the number of
// plk_nni_scores calls are unchanged by it; getLogLikelihoodForEachSite() sums to the lnL; and
// PairedSiteLikelihoods::computeExpectedLikelihoodWeights on three hand-made site-lnL vectors
// equals a plain host loop over the same drawn counts to 1e-12 per weight.
// `test_rell_gpu dump` prints the tree and the alignment and touches no device.
// Prints PASSED and exits 0 on success.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Likelihood/NNIHomogeneousTreeLikelihood.h>
#include <Bpp/Phyl/Likelihood/PairedSiteLikelihoods.h>
#include <Bpp/Phyl/Model/Nucleotide/GTR.h>
#include <Bpp/Phyl/Model/RateDistribution/GammaDiscreteRateDistribution.h>
#include <Bpp/Phyl/NNITopologySearch.h>
#include <Bpp/Phyl/Simulation/HomogeneousSequenceSimulator.h>
#include <Bpp/Phyl/TreeTemplate.h>
#include <Bpp/Seq/Alphabet/AlphabetTools.h>

#include <cmath>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <memory>
#include <numeric>

#include "plk.h"

using namespace bpp;

static int failures = 0;

static void expect(const std::string& what, bool ok) {
  std::cout << what << (ok ? " ok" : " FAIL") << std::endl;
  if (!ok) failures++;
}

static const char* NEWICK =
    "(((A:0.12,B:0.2):0.1,(C:0.1,D:0.25):0.001):0.1,((E:0.15,F:0.1):0.1,G:0.2):0.12,"
    "(((H:0.18,I:0.12):0.1,J:0.22):0.1,(K:0.15,L:0.2):0.11):0.1);";
static const size_t SITES = 2000, REPLICATES = 1000;
static const uint64_t SEED = 20261020;

static void localBootstrap(const TreeTemplate<Node>& tree, const SiteContainer& sites, SubstitutionModel* model,
                           DiscreteDistribution* rdist) {
  NNIHomogeneousTreeLikelihood tl(tree, sites, model, rdist, true, false);
  tl.initialize();
  NNITopologySearch search(tl, NNITopologySearch::BETTER, 0);
  search.search();
  const double value = tl.getValue();
  const size_t calls = tl.getNumberOfScoreCalls();
  std::cout << "search: " << search.getNumberOfRounds() << " rounds, " << search.getAcceptedImprovements().size()
            << " interchanges, -lnL = " << std::setprecision(14) << value << std::endl;

  const std::vector<double> each = tl.getLogLikelihoodForEachSite();
  expect("getLogLikelihoodForEachSite: one value per site, summing to lnL",
         each.size() == SITES && std::fabs(std::accumulate(each.begin(), each.end(), 0.) + value) <= 1e-9 * std::fabs(value));
  expect("getLogLikelihoodForEachSite follows getLogLikelihoodForASite", each[17] == tl.getLogLikelihoodForASite(17));

  RandomTools::setSeed(SEED + 1);
  const std::map<int, double> lbp = tl.computeLocalBootstrap(REPLICATES);
  expect("computeLocalBootstrap leaves getValue() alone", tl.getValue() == value);
  expect("computeLocalBootstrap makes no plk_nni_scores call after a search", tl.getNumberOfScoreCalls() == calls);
  expect("one proportion per internal branch (n - 3 = 9)", lbp.size() == 9);

  // the same numbers from the sums, fetched through the C ABI
  const std::vector<int>& ids = tl.getLocalBootstrapNodeIds();
  const std::vector<size_t>& rivals = tl.getLocalBootstrapRivals();
  const size_t rows = std::accumulate(rivals.begin(), rivals.end(), (size_t)0);
  std::vector<double> G(REPLICATES * rows), Gabs(G.size());
  const int rc = plk_replicate_sums(tl.getEngine(), 0, (int)rows, G.data(), Gabs.data());
  expect("plk_replicate_sums over the rows the call left", rc == PLK_OK && rows == 18);
  const std::vector<double> again = NNIHomogeneousTreeLikelihood::localBootstrapFromSums(G, REPLICATES, rivals);
  bool same = ids.size() == lbp.size();
  for (size_t b = 0; same && b < ids.size(); b++) same = lbp.at(ids[b]) == again[b];
  expect("the proportions are localBootstrapFromSums of those sums", same);
  // a replicate's sum over a row is the resampled difference to the current tree: bounded by its Gabs
  bool bounded = true;
  for (size_t i = 0; i < G.size(); i++) bounded = bounded && std::fabs(G[i]) <= Gabs[i];
  expect("|G| <= Gabs", bounded);

  // support: the branch of length 1e-3 (or whatever the search left of it) against the rest
  const TreeTemplate<Node> now(tl.getTree());
  size_t nShort = 0;
  bool shortBelow = false, restAbove = true;
  for (const auto& kv : lbp) {
    const double len = now.getNode(kv.first)->getDistanceToFather();
    std::cout << "  node " << kv.first << ": length " << len << ", local bootstrap " << kv.second << std::endl;
    if (len < 0.01) {
      nShort++;
      shortBelow = kv.second < 0.95;
    } else {
      restAbove = restAbove && kv.second >= 0.95;
    }
  }
  expect("one short internal branch", nShort == 1);
  expect("the short branch stays below 0.95", shortBelow);
  expect("every other branch gets at least 0.95", restAbove);

  // a second call draws other counts but is the same computation; the scores stay cached
  RandomTools::setSeed(SEED + 1);
  expect("the same seed gives the same proportions", tl.computeLocalBootstrap(REPLICATES) == lbp);
  expect("still no plk_nni_scores call", tl.getNumberOfScoreCalls() == calls && tl.getValue() == value);
  tl.releaseLocalBootstrap();
  expect("releaseLocalBootstrap frees the rows and weights",
         plk_replicate_sums(tl.getEngine(), 0, (int)rows, G.data(), nullptr) == PLK_ERR_STATE && tl.getValue() == value);
}

static void expectedLikelihoodWeights() {
  const size_t n = 500, R = 200;
  std::vector<std::vector<double> > l(3, std::vector<double>(n));
  for (size_t i = 0; i < n; i++) {
    l[0][i] = -3. - 2. * std::fabs(std::sin(0.37 * (double)i));
    l[1][i] = l[0][i] + 0.02 * std::cos(1.3 * (double)i);
    l[2][i] = l[0][i] - 0.004 + 0.03 * std::sin(0.11 * (double)i);
  }
  PairedSiteLikelihoods psl(l, {"m0", "m1", "m2"});
  RandomTools::setSeed(7);
  const std::pair<std::vector<std::string>, std::vector<double> > elw = psl.computeExpectedLikelihoodWeights((int)R);
  // the reference's loop over the same draws
  RandomTools::setSeed(7);
  std::vector<double> want(3, 0.);
  for (size_t r = 0; r < R; r++) {
    const std::vector<int> c = PairedSiteLikelihoods::bootstrap(n);
    double y[3], e[3];
    for (int m = 0; m < 3; m++) {
      y[m] = 0.;
      for (size_t s = 0; s < n; s++) y[m] += l[(size_t)m][s] * c[s];
    }
    const double ymax = std::max(y[0], std::max(y[1], y[2]));
    for (int m = 0; m < 3; m++) e[m] = std::exp(y[m] - ymax);
    for (int m = 0; m < 3; m++) want[(size_t)m] += e[m] / (e[0] + e[1] + e[2]);
  }
  double worst = 0.;
  for (int m = 0; m < 3; m++) worst = std::max(worst, std::fabs(elw.second[(size_t)m] - want[(size_t)m] / (double)R));
  std::cout << "expected likelihood weights " << elw.second[0] << " " << elw.second[1] << " " << elw.second[2]
            << ", worst difference to the host loop " << worst << std::endl;
  expect("expected likelihood weights equal the host loop to 1e-12", worst <= 1e-12 && elw.first[2] == "m2");
  expect("no model takes everything", elw.second[0] > 0.01 && elw.second[1] > 0.01 && elw.second[2] > 0.01);
}

int main(int argc, char** argv) {
  try {
    std::unique_ptr<TreeTemplate<Node> > tree(TreeTemplateTools::parenthesisToTree(NEWICK));
    const NucleicAlphabet* dna = &AlphabetTools::DNA_ALPHABET;
    GTR model(dna, 1, 0.2, 0.3, 0.4, 0.4, 0.1, 0.35, 0.35, 0.2);
    GammaDiscreteRateDistribution rdist(4, 0.6);
    RandomTools::setSeed(SEED);
    HomogeneousSequenceSimulator simulator(&model, &rdist, tree.get());
    std::unique_ptr<SiteContainer> sites(simulator.simulate(SITES));
    if (argc > 1 && !std::strcmp(argv[1], "dump")) {
      std::cout << "NEWICK " << NEWICK << std::endl;
      for (size_t i = 0; i < sites->getNumberOfSequences(); i++) {
        std::cout << "SEQ " << sites->getSequencesNames()[i] << " ";
        for (size_t s = 0; s < SITES; s++) std::cout << sites->getState(i, s);
        std::cout << std::endl;
      }
      return 0;
    }
    localBootstrap(*tree, *sites, &model, &rdist);
    expectedLikelihoodWeights();
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
