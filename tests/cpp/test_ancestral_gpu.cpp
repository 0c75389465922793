// Marginal ancestral states and posterior rate classes through the Bio++ API mirror on the
// MI355X: MarginalAncestralStateReconstruction, DRTreeLikelihoodTools and the posterior-rate
// queries, on the 4-taxon tree and sequences of the smoke run with T92 + Gamma(4), against a
// brute-force sum over the two ancestors' states and the rate classes formed here from the
// mirror's own getPij_t (tolerance 1e-10).  Prints PASSED and exits 0 on success.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Likelihood/DRHomogeneousTreeLikelihood.h>
#include <Bpp/Phyl/Likelihood/DRTreeLikelihoodTools.h>
#include <Bpp/Phyl/Likelihood/MarginalAncestralStateReconstruction.h>
#include <Bpp/Phyl/Likelihood/RHomogeneousTreeLikelihood.h>
#include <Bpp/Phyl/Model/Nucleotide/T92.h>
#include <Bpp/Phyl/Model/RateDistribution/GammaDiscreteRateDistribution.h>
#include <Bpp/Phyl/TreeTemplate.h>
#include <Bpp/Seq/Alphabet/AlphabetTools.h>
#include <Bpp/Seq/Container/VectorSiteContainer.h>

#include <cmath>
#include <iomanip>
#include <iostream>
#include <memory>
#include <string>

#include "plk.h"

using namespace bpp;

static int failures = 0;

static void expect(const char* what, bool ok) {
  std::cout << what << (ok ? " ok" : " FAIL") << std::endl;
  if (!ok) failures++;
}

static void expectNear(const char* what, double got, double want, double tol) {
  const bool ok = std::fabs(got - want) <= tol;
  std::cout << std::setprecision(17) << what << " = " << got << " (expected " << want << ", tol " << tol << ") "
            << (ok ? "ok" : "FAIL") << std::endl;
  if (!ok) failures++;
}

// Brute force for the tree ((A, B)n1, C, D)r at one site: W[c][x][y], the joint of class c,
// state x at the root and state y at n1, normalised.
struct Brute {
  double root[4][4], n1[4][4], rate;  // [class][state]; posterior mean rate
};

static Brute brute(const SubstitutionModel& m, const DiscreteDistribution& rd, const double t[5], const int st[4]) {
  // t: A, B, n1, C, D
  Brute b;
  double W[4][4][4], total = 0.;
  for (size_t c = 0; c < 4; c++) {
    RowMatrix<double> P[5];
    for (int k = 0; k < 5; k++) P[k] = m.getPij_t(t[k] * rd.getCategory(c));
    auto tip = [&](int k, size_t from, int state) {
      double s = 0.;
      for (size_t z = 0; z < 4; z++) s += P[k](from, z) * m.getInitValue(z, state);
      return s;
    };
    for (size_t x = 0; x < 4; x++)
      for (size_t y = 0; y < 4; y++) {
        W[c][x][y] = rd.getProbability(c) * m.freq(x) * P[2](x, y) * tip(0, y, st[0]) * tip(1, y, st[1]) *
                     tip(3, x, st[2]) * tip(4, x, st[3]);
        total += W[c][x][y];
      }
  }
  b.rate = 0.;
  for (size_t c = 0; c < 4; c++)
    for (size_t s = 0; s < 4; s++) {
      b.root[c][s] = b.n1[c][s] = 0.;
      for (size_t o = 0; o < 4; o++) {
        b.root[c][s] += W[c][s][o] / total;
        b.n1[c][s] += W[c][o][s] / total;
      }
      b.rate += rd.getCategory(c) * b.root[c][s];
    }
  return b;
}

int main() {
  std::unique_ptr<TreeTemplate<Node> > tree(
      TreeTemplateTools::parenthesisToTree("((A:0.01, B:0.02):0.03,C:0.01,D:0.1);"));
  const NucleicAlphabet* dna = &AlphabetTools::DNA_ALPHABET;
  VectorSiteContainer aln(dna);
  const char* names[] = {"A", "B", "C", "D"};
  const char* seqs[] = {"AAATGGCTGTGCACGTC", "GACTGGATCTGCACGTC", "CTCTGGATGTGCACGTG", "AAATGGCGGTGCGCCTA"};
  for (int i = 0; i < 4; i++) aln.addSequence(BasicSequence(names[i], seqs[i], dna));
  T92 model(dna, 3.);
  GammaDiscreteRateDistribution rdist(4, 1.0);
  DRHomogeneousTreeLikelihood tl(*tree, aln, &model, &rdist, true, false);
  tl.initialize();
  const double lnl0 = tl.getValue();
  expectNear("T92+G4 -lnL (DR)", lnl0, 85.030942031997312824, 1e-9);
  const auto stats0 = tl.getEvaluationStats();

  // the tree as the likelihood holds it: the root and its internal son, branch lengths by name
  const Tree& lt = tl.getTree();
  const TreeTemplate<Node>& ltt = dynamic_cast<const TreeTemplate<Node>&>(lt);
  const Node* root = ltt.getRootNode();
  const Node* n1 = nullptr;
  std::map<std::string, const Node*> leaf;
  for (const Node* n : ltt.getNodes()) {
    if (n->isLeaf()) leaf[n->getName()] = n;
    else if (n != root) n1 = n;
  }
  expect("one internal node below the root", n1 != nullptr && n1->getFather() == root);
  const double t[5] = {leaf["A"]->getDistanceToFather(), leaf["B"]->getDistanceToFather(), n1->getDistanceToFather(),
                       leaf["C"]->getDistanceToFather(), leaf["D"]->getDistanceToFather()};

  const size_t nSites = tl.getNumberOfSites(), nPat = tl.getNumberOfDistinctSites();
  const std::vector<size_t>& links = tl.getRootArrayPositions();
  // one site of each pattern
  std::vector<size_t> siteOf(nPat, 0);
  for (size_t i = nSites; i-- > 0;) siteOf[links[i]] = i;
  std::vector<Brute> bf(nPat);
  for (size_t p = 0; p < nPat; p++) {
    int st[4];
    for (int k = 0; k < 4; k++) st[k] = aln.getSequence(names[k]).getValue(siteOf[p]);
    bf[p] = brute(model, rdist, t, st);
  }

  MarginalAncestralStateReconstruction asr(&tl);
  double worstJoint = 0., worstState = 0.;
  for (const Node* v : {root, n1}) {
    const VVVdouble joint = DRTreeLikelihoodTools::getPosteriorProbabilitiesForEachStateForEachRate(tl, v->getId());
    VVdouble probs;
    const std::vector<size_t> states = asr.getAncestralStatesForNode(v->getId(), probs, false);
    const std::vector<size_t> states1 = asr.getAncestralStatesForNode(v->getId());
    expect("one- and three-argument forms agree", states == states1);
    Vdouble freqs(4, 0.);
    double sumw = 0.;
    for (size_t p = 0; p < nPat; p++) {
      const double(*ref)[4] = v == root ? bf[p].root : bf[p].n1;
      Vdouble sp(4, 0.);
      for (size_t c = 0; c < 4; c++)
        for (size_t x = 0; x < 4; x++) {
          worstJoint = std::max(worstJoint, std::fabs(joint[p][c][x] - ref[c][x]));
          sp[x] += ref[c][x];
        }
      for (size_t x = 0; x < 4; x++) {
        worstState = std::max(worstState, std::fabs(probs[p][x] - sp[x]));
        freqs[x] += sp[x] * tl.getWeights()[p];
      }
      sumw += tl.getWeights()[p];
      if (states[p] != VectorTools::whichMax(sp)) {
        std::cout << "pattern " << p << ": state " << states[p] << " vs " << VectorTools::whichMax(sp) << std::endl;
        failures++;
      }
    }
    const Vdouble f = DRTreeLikelihoodTools::getPosteriorStateFrequencies(tl, v->getId());
    for (size_t x = 0; x < 4; x++) expectNear("posterior state frequency", f[x], freqs[x] / sumw, 1e-10);
    // sampled states have a non-zero posterior
    RandomTools::setSeed(7);
    VVdouble sprobs;
    const std::vector<size_t> drawn = asr.getAncestralStatesForNode(v->getId(), sprobs, true);
    bool possible = true;
    for (size_t p = 0; p < nPat; p++) possible = possible && drawn[p] < 4 && sprobs[p][drawn[p]] > 0.;
    expect("sampled states have a non-zero posterior", possible);
    // per-site sequence and probabilities follow the pattern links
    VVdouble siteProbs;
    std::unique_ptr<Sequence> seq(asr.getAncestralSequenceForNode(v->getId(), &siteProbs, false));
    bool linked = seq->size() == nSites && siteProbs.size() == nSites;
    for (size_t i = 0; linked && i < nSites; i++)
      linked = seq->getValue(i) == (int)states[links[i]] && siteProbs[i] == probs[links[i]];
    expect("ancestral sequence follows the pattern links", linked);
  }
  expectNear("joint posterior vs brute force (max abs)", worstJoint, 0., 1e-10);
  expectNear("state posterior vs brute force (max abs)", worstState, 0., 1e-10);

  // leaves: one-hot on the observed state; DRTreeLikelihoodTools' leaf formula
  for (int k = 0; k < 4; k++) {
    VVdouble probs;
    const std::vector<size_t> st = asr.getAncestralStatesForNode(leaf[names[k]]->getId(), probs, false);
    const VVVdouble lj = DRTreeLikelihoodTools::getPosteriorProbabilitiesForEachStateForEachRate(tl, leaf[names[k]]->getId());
    bool ok = true;
    for (size_t p = 0; p < nPat; p++) {
      const int obs = aln.getSequence(names[k]).getValue(siteOf[p]);
      double sum = 0.;
      for (size_t x = 0; x < 4; x++) {
        sum += probs[p][x];
        ok = ok && probs[p][x] == ((int)x == obs ? 1. : 0.);
        for (size_t c = 0; c < 4; c++)
          ok = ok && std::fabs(lj[p][c][x] - ((int)x == obs ? rdist.getProbability(c) : 0.)) <= 1e-15;
      }
      ok = ok && sum == 1. && (int)st[p] == obs;
    }
    expect("leaf is one-hot", ok);
  }

  // all nodes in one call equal the per-node calls
  {
    const std::map<int, std::vector<size_t> > all = asr.getAllAncestralStates();
    bool same = all.size() == lt.getNodesId().size();
    for (int id : lt.getNodesId()) same = same && all.count(id) && all.at(id) == asr.getAncestralStatesForNode(id);
    expect("getAllAncestralStates equals the per-node calls", same);
  }

  // posterior rates, on the DR likelihood and on a plain R likelihood
  RHomogeneousTreeLikelihood rl(*tree, aln, &model, &rdist, true, false);
  rl.initialize();
  const double rl0 = rl.getValue();
  const std::string path0 = plk_kernel_path(rl.getEngine());
  for (const AbstractPlkTreeLikelihood* l : {(const AbstractPlkTreeLikelihood*)&tl, (const AbstractPlkTreeLikelihood*)&rl}) {
    const Vdouble rate = l->getPosteriorRateOfEachSite();
    const VVdouble post = l->getPosteriorProbabilitiesOfEachRate();
    const std::vector<size_t> cls = l->getRateClassWithMaxPostProbOfEachSite();
    double worst = 0.;
    bool argmax = rate.size() == nSites && post.size() == nSites && cls.size() == nSites;
    for (size_t i = 0; argmax && i < nSites; i++) {
      const Brute& b = bf[links[i]];
      worst = std::max(worst, std::fabs(rate[i] - b.rate));
      Vdouble cp(4, 0.);
      for (size_t c = 0; c < 4; c++) {
        for (size_t x = 0; x < 4; x++) cp[c] += b.root[c][x];
        worst = std::max(worst, std::fabs(post[i][c] - cp[c]));
      }
      argmax = cls[i] == VectorTools::whichMax(cp);
    }
    expectNear("posterior rates vs brute force (max abs)", worst, 0., 1e-10);
    expect("rate class with the largest posterior", argmax);
  }
  // the queries left the likelihoods as they were
  expectNear("DR -lnL after the queries", tl.getValue(), lnl0, 0.);
  expectNear("R -lnL after the queries", rl.getValue(), rl0, 0.);
  expect("R kernel path after the queries", path0 == plk_kernel_path(rl.getEngine()));
  double s = 0.;
  for (size_t i = 0; i < nSites; i++) s += rl.getLogLikelihoodForASite(i);
  expectNear("R sum of site lnL after the queries", s, rl.getLogLikelihood(), 1e-10);
  const auto stats1 = tl.getEvaluationStats();
  expect("evaluation stats unchanged", stats1.evaluations == stats0.evaluations &&
                                           stats1.pmatBranches == stats0.pmatBranches &&
                                           stats1.fullTraversals == stats0.fullTraversals &&
                                           stats1.scaledFallbacks == stats0.scaledFallbacks &&
                                           stats1.eigenUploads == stats0.eigenUploads);
  // and a parameter change is followed: the root's posterior after a longer branch differs
  {
    ParameterList one = tl.getParameters().createSubList(std::vector<std::string>(1, "BrLen0"));
    const VVVdouble before = DRTreeLikelihoodTools::getPosteriorProbabilitiesForEachStateForEachRate(tl, n1->getId());
    const double v = one[0].getValue();
    one[0].setValue(v * 3. + 0.05);
    tl.f(one);
    const VVVdouble after = DRTreeLikelihoodTools::getPosteriorProbabilitiesForEachStateForEachRate(tl, n1->getId());
    one[0].setValue(v);
    tl.f(one);
    const VVVdouble back = DRTreeLikelihoodTools::getPosteriorProbabilitiesForEachStateForEachRate(tl, n1->getId());
    double moved = 0., restored = 0.;
    for (size_t p = 0; p < nPat; p++)
      for (size_t c = 0; c < 4; c++)
        for (size_t x = 0; x < 4; x++) {
          moved = std::max(moved, std::fabs(after[p][c][x] - before[p][c][x]));
          restored = std::max(restored, std::fabs(back[p][c][x] - before[p][c][x]));
        }
    expect("posteriors follow a branch-length change", moved > 1e-6);
    expectNear("posteriors after restoring the length", restored, 0., 1e-12);
  }
  if (failures) {
    std::cout << failures << " FAILURES" << std::endl;
    return 1;
  }
  std::cout << "PASSED" << std::endl;
  return 0;
}
