// From an alignment to an NNI-refined tree through the Bio++ API mirror on the MI355X:
// DistanceEstimation -> BioNJ -> NNITopologySearch, on sites simulated by
// HomogeneousSequenceSimulator on a fixed 12-taxon tree under GTR + Gamma(4), seeded.
//
// The tree and the site count are a condition, not a measurement: 3000 sites and inner branches
// of 0.05 or more were chosen on the CPU so that the numpy restatement's ML distances
// (tests/test_pair_cpu.py) and the numpy BioNJ (tests/test_distance_host.py) recover the true
// bipartitions from this very alignment; tests/test_distance_host.py keeps checking that from
// the alignment `test_distance_gpu dump` prints (the dump touches no device).
//
// Checks: the matrix of DistanceEstimation equals a direct plk_pair_distances call over the
// uncompressed sites bit for bit (the pair tables are the same integers), is symmetric with a
// zero diagonal, and every pair converged; BioNJ on it returns the true tree's bipartitions;
// NNITopologySearch (BETTER) from the BioNJ tree makes no move.  Prints PASSED and exits 0.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Distance/BioNJ.h>
#include <Bpp/Phyl/Distance/DistanceEstimation.h>
#include <Bpp/Phyl/Likelihood/NNIHomogeneousTreeLikelihood.h>
#include <Bpp/Phyl/Model/Nucleotide/GTR.h>
#include <Bpp/Phyl/Model/RateDistribution/GammaDiscreteRateDistribution.h>
#include <Bpp/Phyl/NNITopologySearch.h>
#include <Bpp/Phyl/Simulation/HomogeneousSequenceSimulator.h>
#include <Bpp/Phyl/TreeTemplate.h>
#include <Bpp/Seq/Alphabet/AlphabetTools.h>

#include <algorithm>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <memory>
#include <set>

#include "plk.h"

using namespace bpp;

static int failures = 0;

static void expect(const std::string& what, bool ok) {
  std::cout << what << (ok ? " ok" : " FAIL") << std::endl;
  if (!ok) failures++;
}

// the side without the first leaf name of every inner branch
static std::set<std::set<std::string> > bipartitions(const TreeTemplate<Node>& tree) {
  std::vector<std::string> names = tree.getLeavesNames();
  std::sort(names.begin(), names.end());
  std::set<std::set<std::string> > out;
  for (const Node* n : tree.getNodes()) {
    if (!n->hasFather() || n->isLeaf()) continue;
    std::set<std::string> side;
    for (const Node* l : TreeTemplateTools::getLeaves(*n)) side.insert(l->getName());
    if (side.count(names[0])) {
      std::set<std::string> other;
      for (const std::string& s : names)
        if (!side.count(s)) other.insert(s);
      side.swap(other);
    }
    if (side.size() > 1 && side.size() < names.size() - 1) out.insert(side);
  }
  return out;
}

static void check(plk_handle h, int rc, const char* what) {
  if (rc != PLK_OK) throw Exception(std::string(what) + ": " + plk_last_error(h));
}

int main(int argc, char** argv) {
  try {
    const char* newick =
        "(((A:0.12,B:0.2):0.08,(C:0.1,D:0.25):0.07):0.06,((E:0.15,F:0.1):0.09,(G:0.2,K:0.14):0.06):0.07,"
        "((H:0.18,I:0.12):0.08,(J:0.22,L:0.09):0.05):0.1);";
    const size_t nSites = 3000;
    std::unique_ptr<TreeTemplate<Node> > tree(TreeTemplateTools::parenthesisToTree(newick));
    const NucleicAlphabet* dna = &AlphabetTools::DNA_ALPHABET;
    GTR model(dna, 1, 0.2, 0.3, 0.4, 0.4, 0.1, 0.35, 0.35, 0.2);
    GammaDiscreteRateDistribution rdist(4, 0.6);
    RandomTools::setSeed(20261021);
    HomogeneousSequenceSimulator simulator(&model, &rdist, tree.get());
    std::unique_ptr<SiteContainer> sites(simulator.simulate(nSites));
    const std::vector<std::string> names = sites->getSequencesNames();
    const size_t n = names.size();
    if (argc > 1 && std::strcmp(argv[1], "dump") == 0) {
      std::cout << "NEWICK " << newick << std::endl;
      for (size_t t = 0; t < n; t++) {
        std::cout << "SEQ " << names[t] << " ";
        for (size_t i = 0; i < nSites; i++) std::cout << sites->getState(t, i);
        std::cout << std::endl;
      }
      return 0;
    }

    DistanceEstimation est(model.clone(), rdist.clone(), sites.get(), 0, true);
    std::unique_ptr<DistanceMatrix> D(est.getMatrix());
    expect("the matrix has a row per sequence, named", D->size() == n && D->getNames() == names);
    bool sym = true;
    for (size_t i = 0; i < n; i++)
      for (size_t j = 0; j < n; j++) sym = sym && (*D)(i, j) == (*D)(j, i) && (i != j || (*D)(i, j) == 0.);
    expect("symmetric with a zero diagonal", sym);
    std::cout << "passes of the slowest pair: " << est.getNumberOfPasses() << std::endl;

    // the direct call: every site a pattern of weight 1
    {
      plk_handle h = nullptr;
      check(nullptr, plk_create(0, 4, 4, (int64_t)nSites, (int)n, 1, 1, 0, &h), "plk_create");
      const int nc = dna->getNumberOfCodes();
      std::vector<double> table((size_t)nc * 4);
      for (int c = 0; c < nc; c++)
        for (size_t s = 0; s < 4; s++) table[(size_t)c * 4 + s] = model.getInitValue(s, c);
      check(h, plk_set_code_table(h, nc, table.data()), "plk_set_code_table");
      std::vector<uint8_t> codes(nSites);
      for (size_t t = 0; t < n; t++) {
        for (size_t i = 0; i < nSites; i++) codes[i] = (uint8_t)sites->getState(t, i);
        check(h, plk_set_tip_codes(h, (int)t, codes.data()), "plk_set_tip_codes");
      }
      check(h, plk_set_category_rates(h, rdist.getCategories().data(), rdist.getProbabilities().data()), "rates");
      check(h, plk_set_root_frequencies(h, model.getFrequencies().data()), "pi");
      std::vector<double> lam(4);
      for (size_t k = 0; k < 4; k++) lam[k] = model.getEigenValues()[k] * model.getRate();
      check(h, plk_set_eigen(h, 0, model.getColumnRightEigenVectors().data(), model.getRowLeftEigenVectors().data(), lam.data()),
            "plk_set_eigen");
      std::vector<int32_t> a, b;
      for (size_t i = 0; i < n; i++)
        for (size_t j = i + 1; j < n; j++) a.push_back((int32_t)i), b.push_back((int32_t)j);
      std::vector<double> t(a.size()), lnl(a.size());
      std::vector<int32_t> status(a.size());
      check(h, plk_pair_distances(h, (int)a.size(), a.data(), b.data(), 0, nullptr, 1e-6, 10000., 1e-8, 40, t.data(), lnl.data(),
                                  nullptr, nullptr, status.data()),
            "plk_pair_distances");
      bool equal = true, converged = true, lnlEqual = true;
      for (size_t k = 0; k < a.size(); k++) {
        equal = equal && t[k] == (*D)((size_t)a[k], (size_t)b[k]);
        lnlEqual = lnlEqual && lnl[k] == est.getPairLogLikelihood((size_t)a[k], (size_t)b[k]);
        converged = converged && status[k] == 0;
      }
      expect("DistanceEstimation equals the direct plk_pair_distances call", equal && lnlEqual);
      expect("every pair converged", converged);
      plk_destroy(h);
    }

    BioNJ bionj(*D, false, true, false);
    std::unique_ptr<TreeTemplate<Node> > start(bionj.getTree());
    std::cout << "BioNJ: " << TreeTemplateTools::treeToParenthesis(*start) << std::endl;
    expect("BioNJ returns the true tree's bipartitions", bipartitions(*start) == bipartitions(*tree));
    expect("nine inner branches", bipartitions(*tree).size() == 9);

    NNIHomogeneousTreeLikelihood tl(*start, *sites, &model, &rdist, true, false);
    tl.initialize();
    const double before = tl.getValue();
    NNITopologySearch search(tl, NNITopologySearch::BETTER, 0);
    search.search();
    std::cout << std::setprecision(14) << "BioNJ tree -lnL = " << before << ", after " << search.getNumberOfRounds()
              << " round(s) " << tl.getValue() << std::endl;
    expect("NNITopologySearch (BETTER) makes no move from the BioNJ tree", search.getAcceptedImprovements().empty());
    const TreeTemplate<Node> final(tl.getTopology());
    expect("and keeps its bipartitions", bipartitions(final) == bipartitions(*tree));
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
