// RELL resampling of the Bio++ mirror without a device: the arithmetic that follows the engine's
// replicate sums -- NNIHomogeneousTreeLikelihood::localBootstrapFromSums and
// PairedSiteLikelihoods::expectedLikelihoodWeightsFromSums on hand-made sums, ties included --
// the bootstrap counts, and the container's bookkeeping.  Prints PASSED and exits 0 on success.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Likelihood/NNIHomogeneousTreeLikelihood.h>
#include <Bpp/Phyl/Likelihood/PairedSiteLikelihoods.h>

#include <cmath>
#include <iostream>
#include <numeric>

using namespace bpp;

static int failures = 0;

static void expect(const std::string& what, bool ok) {
  std::cout << what << (ok ? " ok" : " FAIL") << std::endl;
  if (!ok) failures++;
}

static bool close(double a, double b, double tol = 1e-15) { return std::fabs(a - b) <= tol; }

int main() {
  try {
    // bootstrap(n, s): floor(n s + 0.5) draws over n sites
    RandomTools::setSeed(11);
    const std::pair<size_t, double> shapes[] = {{10, 1.}, {7, 0.5}, {1000, 2.5}, {3, 0.5}, {1, 1.}, {5, 0.}};
    for (const auto& sh : shapes) {
      const std::vector<int> c = PairedSiteLikelihoods::bootstrap(sh.first, sh.second);
      const long want = (long)std::floor((double)sh.first * sh.second + 0.5);
      bool nonneg = true;
      for (int v : c) nonneg = nonneg && v >= 0;
      expect("bootstrap(" + std::to_string(sh.first) + ", " + std::to_string(sh.second) + ") sums to " + std::to_string(want),
             c.size() == sh.first && nonneg && std::accumulate(c.begin(), c.end(), 0L) == want);
    }
    const std::vector<int> big = PairedSiteLikelihoods::bootstrap(50);
    expect("bootstrap draws differ between sites", *std::max_element(big.begin(), big.end()) >= 2);

    // local bootstrap: two branches of two rivals each, four replicates
    //   replicate 0: (-1, -2) -> 1        (0.5, -1) -> 0
    //   replicate 1: (0, -1)  -> 1/2      (0, 0)    -> 1/3
    //   replicate 2: (1, 0)   -> 0        (-3, -0.) -> 1/2   (-0. is 0: a tie)
    //   replicate 3: (-1e-300, -5) -> 1   (-1, -1)  -> 1
    const std::vector<double> G = {-1, -2, 0.5, -1, 0, -1, 0, 0, 1, 0, -3, -0., -1e-300, -5, -1, -1};
    const std::vector<double> lbp = NNIHomogeneousTreeLikelihood::localBootstrapFromSums(G, 4, {2, 2});
    expect("local bootstrap of branch 0 = 2.5 / 4", lbp.size() == 2 && close(lbp[0], 2.5 / 4));
    expect("local bootstrap of branch 1 = (1/3 + 1/2 + 1) / 4", close(lbp[1], (1. / 3 + 0.5 + 1.) / 4));
    // one branch of three rivals (a trifurcation below it) next to one of two
    const std::vector<double> G3 = {0, 0, 0, -1, -1, -1, -2, -3, 4, 0, -1, -1, 0, 0, 1e-300};
    const std::vector<double> l3 = NNIHomogeneousTreeLikelihood::localBootstrapFromSums(G3, 3, {3, 2});
    //   (0, 0, 0) -> 1/4, (-1, -1) -> 1;  (-1, -2, -3) -> 1, (4, 0) -> 0;  (-1, -1, 0) -> 1/2, (0, 1e-300) -> 0
    expect("three rivals: (1/4 + 1 + 1/2) / 3", close(l3[0], (0.25 + 1. + 0.5) / 3));
    expect("two rivals beside them: (1 + 0 + 0) / 3", close(l3[1], 1. / 3));
    bool threw = false;
    try {
      NNIHomogeneousTreeLikelihood::localBootstrapFromSums(G3, 3, {3, 3});
    } catch (Exception&) {
      threw = true;
    }
    expect("a wrong shape throws", threw);
    expect("no replicates: zeros", NNIHomogeneousTreeLikelihood::localBootstrapFromSums({}, 0, {2})[0] == 0.);

    // expected likelihood weights: two replicates, three models
    //   (-10, -10 + ln 3, -10)  -> (1/5, 3/5, 1/5);   (-5, -1000, -5) -> (1/2, 0, 1/2)
    const std::vector<double> Y = {-10., -10. + std::log(3.), -10., -5., -1000., -5.};
    const std::vector<double> w = PairedSiteLikelihoods::expectedLikelihoodWeightsFromSums(Y, 2, 3);
    expect("expected likelihood weights (0.35, 0.3, 0.35)",
           w.size() == 3 && close(w[0], 0.35, 1e-12) && close(w[1], 0.3, 1e-12) && close(w[2], 0.35, 1e-12));
    expect("the weights sum to 1", close(w[0] + w[1] + w[2], 1., 1e-12));
    const std::vector<double> tie = PairedSiteLikelihoods::expectedLikelihoodWeightsFromSums({-3., -3., 7., 7.}, 2, 2);
    expect("tied models share the weight", close(tie[0], 0.5) && close(tie[1], 0.5));

    // the container
    PairedSiteLikelihoods psl;
    psl.appendModel({-1., -2., -3.}, "a");
    psl.appendModel({-1.5, -2.5, -3.5}, "b");
    threw = false;
    try {
      psl.appendModel({-1., -2.}, "short");
    } catch (Exception&) {
      threw = true;
    }
    expect("a record of another length is refused", threw);
    threw = false;
    try {
      PairedSiteLikelihoods bad({{-1., -2.}, {-1.}});
    } catch (Exception&) {
      threw = true;
    }
    expect("records of different lengths are refused by the constructor", threw);
    threw = false;
    try {
      PairedSiteLikelihoods bad({{-1., -2.}, {-1., -3.}}, {"only one"});
    } catch (Exception&) {
      threw = true;
    }
    expect("a name list of another length is refused", threw);
    expect("without names every model has an empty one",
           PairedSiteLikelihoods({{-1., -2.}, {-1., -3.}}).getModelNames() == std::vector<std::string>(2));
    expect("an empty container has no sites", PairedSiteLikelihoods().getNumberOfSites() == 0);
    PairedSiteLikelihoods both({{-4., -5., -6.}}, {"c"});
    both.appendModels(psl);
    expect("appendModels keeps order and names",
           both.getNumberOfModels() == 3 && both.getNumberOfSites() == 3 && both.getModelName(0) == "c" &&
               both.getModelNames()[2] == "b" && both.getLogLikelihoods(1)[2] == -3.);
    expect("no replicates, no engine call", both.computeExpectedLikelihoodWeights(0).second == std::vector<double>(3, 0.));
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
