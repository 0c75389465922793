// DeviceSequenceSimulator through the Bio++ API mirror on the MI355X (plk_simulate underneath).
//   1. The non-homogeneous test's tree and model set (T92 per branch, GC root frequencies,
//      Gamma(4, 1)) and a homogeneous GTR + Gamma(4) tree, 20 000 sites each: the container equals,
//      character by character, what plk_simulate + plk_sim_get_states give on a handle set up by
//      hand here with the same seed and replicate.
//   2. Internal sequences appear only when asked for; a second simulate() differs from the first
//      and uses the next replicate number.
//   3. Under the stationary homogeneous model each tip's state frequencies lie within 5 binomial
//      standard deviations, 5 sqrt(pi_x (1 - pi_x) / N), of pi_x.
//   4. RHomogeneousTreeLikelihood on the simulated container gives a higher lnL at the generating
//      branch lengths than with every length doubled.
// Prints PASSED and exits 0 on success.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Likelihood/RHomogeneousTreeLikelihood.h>
#include <Bpp/Phyl/Model/FrequencySet/NucleotideFrequencySet.h>
#include <Bpp/Phyl/Model/Nucleotide/GTR.h>
#include <Bpp/Phyl/Model/Nucleotide/T92.h>
#include <Bpp/Phyl/Model/RateDistribution/GammaDiscreteRateDistribution.h>
#include <Bpp/Phyl/Model/SubstitutionModelSetTools.h>
#include <Bpp/Phyl/Simulation/DeviceSequenceSimulator.h>
#include <Bpp/Phyl/TreeTemplate.h>
#include <Bpp/Seq/Alphabet/AlphabetTools.h>
#include <Bpp/Seq/Container/VectorSiteContainer.h>

#include <cmath>
#include <iostream>
#include <map>
#include <memory>

#include "plk.h"

using namespace bpp;

static int failures = 0;

static void expect(const std::string& what, bool ok, const std::string& detail = "") {
  std::cout << what << (detail.empty() ? "" : ": " + detail) << (ok ? " ok" : " FAIL") << std::endl;
  if (!ok) failures++;
}

static void must(int rc, const char* what, plk_handle h) {
  if (rc != PLK_OK) {
    std::cout << what << " failed: " << plk_last_error(h) << std::endl;
    std::exit(1);
  }
}

// states per node name (leaves) or id (internal nodes) from a handle set up by hand
static std::map<std::string, std::vector<uint8_t> > byHand(const SubstitutionModelSet& ms, const DiscreteDistribution& rd,
                                                           const TreeTemplate<Node>& tree, size_t n, uint64_t seed,
                                                           uint64_t replicate) {
  const std::vector<const Node*> all = [&] {
    std::vector<const Node*> v;
    for (const Node* x : tree.getNodes()) v.push_back(x);
    return v;
  }();
  std::map<const Node*, int> idx;
  int nt = 0, ni = 0;
  for (const Node* x : all)
    if (x->isLeaf()) idx[x] = nt++;
  for (const Node* x : all)
    if (!x->isLeaf()) idx[x] = nt + ni++;
  const int S = (int)ms.getNumberOfStates(), C = (int)rd.getNumberOfCategories(), M = (int)ms.getNumberOfModels();
  plk_handle h = nullptr;
  must(plk_create(0, S, C, (int64_t)n, nt, ni, M, 0u, &h), "plk_create", nullptr);
  must(plk_set_category_rates(h, rd.getCategories().data(), rd.getProbabilities().data()), "rates", h);
  const Vdouble pi = ms.getRootFrequencies();
  must(plk_set_root_frequencies(h, pi.data()), "pi", h);
  for (int m = 0; m < M; m++) {
    const SubstitutionModel& model = *ms.getModel((size_t)m);
    std::vector<double> lam((size_t)S);
    for (int k = 0; k < S; k++) lam[(size_t)k] = model.getEigenValues()[(size_t)k] * model.getRate();
    must(plk_set_eigen(h, m, model.getColumnRightEigenVectors().data(), model.getRowLeftEigenVectors().data(), lam.data()),
         "eigen", h);
  }
  std::vector<int32_t> br, mod;
  std::vector<double> t;
  std::vector<plk_op> ops;
  for (const Node* x : all) {
    if (x->hasFather()) {
      br.push_back(idx[x]);
      mod.push_back((int32_t)ms.getModelIndexForNode(x->getId()));
      t.push_back(x->getDistanceToFather());
    }
    for (size_t k = 0; k < x->getNumberOfSons(); k += 3) {
      plk_op o = {idx[x], 0, {0, 0, 0}, k == 0 ? 0 : PLK_OP_ACCUMULATE};
      for (size_t j = k; j < std::min(k + 3, x->getNumberOfSons()); j++) o.child[o.n_children++] = idx[x->getSon(j)];
      ops.push_back(o);
    }
  }
  must(plk_update_pmatrices(h, (int)br.size(), br.data(), mod.data(), t.data(), PLK_DERIV_P), "P(t)", h);
  must(plk_simulate(h, ops.data(), (int)ops.size(), idx[tree.getRootNode()], seed, replicate, 0, nullptr, 0u), "plk_simulate", h);
  std::map<std::string, std::vector<uint8_t> > out;
  for (const Node* x : all) {
    std::vector<uint8_t>& s = out[x->isLeaf() ? x->getName() : std::to_string(x->getId())];
    s.resize(n);
    must(plk_sim_get_states(h, idx[x], s.data()), "plk_sim_get_states", h);
  }
  plk_destroy(h);
  return out;
}

static bool sameCharacters(const SiteContainer& sites, const std::map<std::string, std::vector<uint8_t> >& want) {
  for (const std::string& name : sites.getSequencesNames()) {
    const Sequence& s = sites.getSequence(name);
    const std::vector<uint8_t>& w = want.at(name);
    if (s.size() != w.size()) return false;
    for (size_t i = 0; i < w.size(); i++)
      if (s.getValue(i) != (int)w[i]) return false;
  }
  return true;
}

static size_t differing(const SiteContainer& a, const SiteContainer& b) {
  size_t d = 0;
  for (const std::string& name : a.getSequencesNames()) {
    const Sequence &x = a.getSequence(name), &y = b.getSequence(name);
    for (size_t i = 0; i < x.size(); i++) d += x.getValue(i) != y.getValue(i);
  }
  return d;
}

static void common(DeviceSequenceSimulator& sim, const TreeTemplate<Node>& tree, const DiscreteDistribution& rd,
                   const std::string& tag, uint64_t seed) {
  const size_t n = 20000, nLeaves = tree.getNumberOfLeaves(), nNodes = tree.getNodes().size();
  sim.setSeed(seed);
  expect(tag + ": replicate 0 first", sim.getReplicate() == 0);
  std::unique_ptr<SiteContainer> first(sim.simulate(n));
  expect(tag + ": leaves only by default",
         first->getNumberOfSequences() == nLeaves && first->getNumberOfSites() == n &&
             first->getSequencesNames() == tree.getLeavesNames() && sim.getSequencesNames() == tree.getLeavesNames());
  expect(tag + ": equals plk_simulate on a handle set up by hand",
         sameCharacters(*first, byHand(*sim.getSubstitutionModelSet(), rd, tree, n, seed, 0)));
  expect(tag + ": replicate 1 next", sim.getReplicate() == 1);
  std::unique_ptr<SiteContainer> second(sim.simulate(n));
  const size_t d = differing(*first, *second);
  expect(tag + ": a second simulate differs", d > n * nLeaves / 4, std::to_string(d) + " characters");
  expect(tag + ": and is replicate 1 by hand",
         sameCharacters(*second, byHand(*sim.getSubstitutionModelSet(), rd, tree, n, seed, 1)));
  sim.outputInternalSequences(true);
  std::unique_ptr<SiteContainer> withInternal(sim.simulate(n));
  expect(tag + ": internal sequences when asked for",
         withInternal->getNumberOfSequences() == nNodes && sim.getSequencesNames().size() == nNodes);
  expect(tag + ": every node equals replicate 2 by hand",
         sameCharacters(*withInternal, byHand(*sim.getSubstitutionModelSet(), rd, tree, n, seed, 2)));
  sim.outputInternalSequences(false);
  // another site count: the handle is recreated, the stream goes on
  std::unique_ptr<SiteContainer> fewer(sim.simulate(777));
  expect(tag + ": another site count",
         fewer->getNumberOfSites() == 777 && fewer->getNumberOfSequences() == nLeaves &&
             sameCharacters(*fewer, byHand(*sim.getSubstitutionModelSet(), rd, tree, 777, seed, 3)));
  sim.setSeed(seed);
  std::unique_ptr<SiteContainer> again(sim.simulate(n));
  expect(tag + ": the same seed gives the same alignment", differing(*first, *again) == 0);
}

static void nonHomogeneous() {
  std::unique_ptr<TreeTemplate<Node> > tree(
      TreeTemplateTools::parenthesisToTree("(((A:0.1, B:0.2):0.3,C:0.1):0.2,(D:0.3,(E:0.2,F:0.05):0.1):0.1);"));
  const NucleicAlphabet* alphabet = &AlphabetTools::DNA_ALPHABET;
  FrequencySet* rootFreqs = new GCFrequencySet(alphabet);
  SubstitutionModel* model = new T92(alphabet, 3.);
  std::map<std::string, std::vector<Vint> > globalParameterNames;
  globalParameterNames["T92.kappa"] = {};
  std::map<std::string, std::string> alias;
  std::unique_ptr<SubstitutionModelSet> modelSet(
      SubstitutionModelSetTools::createNonHomogeneousModelSet(model, rootFreqs, tree.get(), alias, globalParameterNames));
  for (size_t i = 0; i < modelSet->getNumberOfModels(); ++i)
    modelSet->setParameterValue("T92.theta_" + std::to_string(i + 1), 0.1 + 0.8 * (double)i / (double)modelSet->getNumberOfModels());
  GammaDiscreteRateDistribution rdist(4, 1.0);
  DeviceSequenceSimulator sim(modelSet.get(), &rdist, tree.get());
  expect("NH: queries", sim.getAlphabet() == alphabet && sim.getSubstitutionModelSet() == modelSet.get());
  common(sim, *tree, rdist, "NH", 42);
}

static void homogeneous() {
  std::unique_ptr<TreeTemplate<Node> > tree(TreeTemplateTools::parenthesisToTree(
      "((A:0.12,B:0.2):0.08,(C:0.15,(D:0.1,E:0.25):0.06):0.1,(F:0.3,G:0.05):0.14);"));
  const NucleicAlphabet* alphabet = &AlphabetTools::DNA_ALPHABET;
  GTR model(alphabet, 1.2, 0.4, 0.6, 0.8, 0.5, 0.30, 0.20, 0.25, 0.25);
  GammaDiscreteRateDistribution rdist(4, 0.6);
  DeviceSequenceSimulator sim(&model, &rdist, tree.get());
  common(sim, *tree, rdist, "GTR+G4", 7);

  const size_t n = 20000;
  sim.setSeed(7);
  std::unique_ptr<SiteContainer> sites(sim.simulate(n));
  const Vdouble pi = model.getFrequencies();
  bool within = true;
  double worst = 0.;
  for (const std::string& name : sites->getSequencesNames()) {
    std::vector<size_t> count(4, 0);
    const Sequence& s = sites->getSequence(name);
    for (size_t i = 0; i < n; i++) count[(size_t)s.getValue(i)]++;
    for (size_t x = 0; x < 4; x++) {
      const double z = std::fabs((double)count[x] / (double)n - pi[x]) / std::sqrt(pi[x] * (1. - pi[x]) / (double)n);
      worst = std::max(worst, z);
      if (z > 5.) within = false;
    }
  }
  expect("GTR+G4: tip frequencies within 5 binomial standard deviations of pi", within, "worst " + std::to_string(worst));

  RHomogeneousTreeLikelihood tl(*tree, *sites, &model, &rdist, true, false);
  tl.initialize();
  const double lnl = tl.getLogLikelihood();
  TreeTemplate<Node> doubled(*tree);
  for (Node* x : doubled.getNodes())
    if (x->hasFather()) x->setDistanceToFather(2. * x->getDistanceToFather());
  RHomogeneousTreeLikelihood tl2(doubled, *sites, &model, &rdist, true, false);
  tl2.initialize();
  const double lnl2 = tl2.getLogLikelihood();
  expect("GTR+G4: lnL at the generating lengths above lnL at doubled lengths", lnl > lnl2 && std::isfinite(lnl),
         std::to_string(lnl) + " vs " + std::to_string(lnl2));
}

int main() {
  try {
    nonHomogeneous();
    homogeneous();
  } catch (std::exception& e) {
    std::cout << "exception: " << e.what() << std::endl;
    return 1;
  }
  if (failures) {
    std::cout << failures << " FAILED" << std::endl;
    return 1;
  }
  std::cout << "PASSED" << std::endl;
  return 0;
}
