// Stochastic mapping through the Bio++ API mirror on the MI355X: DeviceStochasticMapping on 300
// simulated sites of the tree ((A:0.1,B:0.2):0.15,C:0.1,D:0.3) under the reference test's GTR with
// Gamma(4).  Checks:
//   1. the mirror's means are the sums of plk_smap_sample on a handle set up by hand with the same
//      node numbers, seed and replicates, divided by the number of replicates (==), with the
//      comprehensive register;
//   2. state frequencies of the internal nodes, pooled over the distinct patterns, within 6 binomial
//      standard errors (variance R sum_p q (1 - q)) of MarginalAncestralStateReconstruction;
//   3. the total register's mean counts per branch, pooled over the distinct patterns, within 6
//      standard errors (the kept replicates' own) of SubstitutionMappingTools::
//      computeSubstitutionVectors;
//   4. kept replicates: resolved leaves keep their state, dwelling times sum to the branch length
//      (1e-12), the means are the means of the kept rows.
// Prints PASSED and exits 0 on success.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Likelihood/DRHomogeneousTreeLikelihood.h>
#include <Bpp/Phyl/Likelihood/MarginalAncestralStateReconstruction.h>
#include <Bpp/Phyl/Mapping/DecompositionSubstitutionCount.h>
#include <Bpp/Phyl/Mapping/DeviceStochasticMapping.h>
#include <Bpp/Phyl/Mapping/ProbabilisticSubstitutionMapping.h>
#include <Bpp/Phyl/Mapping/SubstitutionMappingTools.h>
#include <Bpp/Phyl/Mapping/SubstitutionRegister.h>
#include <Bpp/Phyl/Model/Nucleotide/GTR.h>
#include <Bpp/Phyl/Model/RateDistribution/GammaDiscreteRateDistribution.h>
#include <Bpp/Phyl/Simulation/HomogeneousSequenceSimulator.h>
#include <Bpp/Phyl/TreeTemplate.h>
#include <Bpp/Seq/Alphabet/AlphabetTools.h>

#include <cmath>
#include <iomanip>
#include <iostream>
#include <memory>

#include "plk.h"

using namespace bpp;

static int failures = 0;

static void expect(const std::string& what, bool ok) {
  std::cout << what << (ok ? " ok" : " FAIL") << std::endl;
  if (!ok) failures++;
}

static void expectBelow(const std::string& what, double got, double bound) {
  const bool ok = got <= bound;
  std::cout << std::setprecision(6) << what << " = " << got << " (bound " << bound << ") " << (ok ? "ok" : "FAIL") << std::endl;
  if (!ok) failures++;
}

static void ok(plk_handle h, int rc, const char* what) {
  if (rc != PLK_OK) {
    std::cout << what << ": " << plk_last_error(h) << std::endl;
    std::exit(2);
  }
}

int main() {
  std::unique_ptr<TreeTemplate<Node> > tree(TreeTemplateTools::parenthesisToTree("((A:0.1,B:0.2):0.15,C:0.1,D:0.3);"));
  const NucleicAlphabet* dna = &AlphabetTools::DNA_ALPHABET;
  GTR model(dna, 1, 0.2, 0.3, 0.4, 0.4, 0.1, 0.35, 0.35, 0.2);
  GammaDiscreteRateDistribution gamma(4, 0.5);
  const size_t n = 300, S = 4, C = 4;
  RandomTools::setSeed(20261021);
  HomogeneousSequenceSimulator simulator(&model, &gamma, tree.get());
  std::unique_ptr<SiteContainer> sites(simulator.simulate(n));
  DRHomogeneousTreeLikelihood tl(*tree, *sites, &model, &gamma, true, false);
  tl.initialize();
  const double lnl0 = tl.getValue();
  const size_t nPat = tl.getNumberOfDistinctSites();
  std::cout << "-lnL = " << std::setprecision(12) << lnl0 << ", " << nPat << " patterns" << std::endl;
  // one site of every distinct pattern
  std::vector<size_t> siteOf(nPat, n);
  for (size_t i = 0; i < n; i++)
    if (siteOf[tl.getRootArrayPosition(i)] == n) siteOf[tl.getRootArrayPosition(i)] = i;
  const TreeTemplate<Node>& ltt = dynamic_cast<const TreeTemplate<Node>&>(tl.getTree());
  std::vector<int> ids = ltt.getNodesId();
  const int rootId = ids.back();
  ids.pop_back();

  // 1. against a handle set up by hand
  {
    const uint64_t seed = 77;
    const size_t R = 16, T = 12;
    ComprehensiveSubstitutionRegister reg(&model);
    DeviceStochasticMapping sm(tl, reg);
    sm.sample(seed, R);
    expect("sizes", sm.getNumberOfReplicates() == R && sm.getNumberOfSubstitutionTypes() == T && sm.getNumberOfSites() == n &&
                        sm.getBranchIds().size() == ids.size());
    const std::vector<const Node*> all = ltt.getNodes();
    int nTips = 0, nInternal = 0;
    for (const Node* v : all) (v->isLeaf() ? nTips : nInternal)++;
    plk_handle h = nullptr;
    ok(nullptr, plk_create(0, (int)S, (int)C, (int64_t)nPat, nTips, nInternal, 1, PLK_FLAG_SCALING | PLK_FLAG_NONNEG_GUARD, &h),
       "plk_create");
    const int nc = (int)dna->getNumberOfCodes();
    std::vector<double> table((size_t)nc * S);
    for (int c = 0; c < nc; c++)
      for (size_t s = 0; s < S; s++) table[(size_t)c * S + s] = model.getInitValue(s, c);
    ok(h, plk_set_code_table(h, nc, table.data()), "plk_set_code_table");
    for (const Node* v : all)
      if (v->isLeaf()) {
        const std::vector<int>& st = tl.getLeafPatternStates(v->getId());
        std::vector<uint8_t> codes(st.begin(), st.end());
        ok(h, plk_set_tip_codes(h, sm.getEngineIndex(v->getId()), codes.data()), "plk_set_tip_codes");
      }
    std::vector<double> w(tl.getWeights().begin(), tl.getWeights().end());
    ok(h, plk_set_pattern_weights(h, w.data()), "plk_set_pattern_weights");
    ok(h, plk_set_category_rates(h, gamma.getCategories().data(), gamma.getProbabilities().data()), "plk_set_category_rates");
    ok(h, plk_set_root_frequencies(h, model.getFrequencies().data()), "plk_set_root_frequencies");
    std::vector<double> lam(S), Q(S * S);
    for (size_t k = 0; k < S; k++) lam[k] = model.getEigenValues()[k] * model.getRate();
    ok(h, plk_set_eigen(h, 0, model.getColumnRightEigenVectors().data(), model.getRowLeftEigenVectors().data(), lam.data()),
       "plk_set_eigen");
    std::vector<uint8_t> typeOf(S * S, 0);
    for (size_t x = 0; x < S; x++)
      for (size_t y = 0; y < S; y++) {
        Q[x * S + y] = model.getGenerator()(x, y) * model.getRate();
        if (x != y) typeOf[x * S + y] = (uint8_t)reg.getType(x, y);
      }
    ok(h, plk_smap_set_generator(h, 0, Q.data()), "plk_smap_set_generator");
    ok(h, plk_smap_set_types(h, (int)T, typeOf.data()), "plk_smap_set_types");
    std::vector<int32_t> br;
    std::vector<double> len;
    for (int id : ids) {
      br.push_back(sm.getEngineIndex(id));
      len.push_back(ltt.getNode(id)->getDistanceToFather());
    }
    ok(h, plk_update_pmatrices(h, (int)br.size(), br.data(), nullptr, len.data(), PLK_DERIV_P), "plk_update_pmatrices");
    std::vector<plk_op> ops;
    for (const Node* v : all) {  // postorder
      if (v->isLeaf()) continue;
      for (size_t k = 0; k < v->getNumberOfSons(); k += 3) {
        plk_op o;
        o.parent = sm.getEngineIndex(v->getId());
        o.n_children = 0;
        for (size_t j = 0; j < 3; j++) {
          o.child[j] = -1;
          if (k + j < v->getNumberOfSons()) o.child[o.n_children++] = sm.getEngineIndex(v->getSon(k + j)->getId());
        }
        o.flags = k == 0 ? 0 : PLK_OP_ACCUMULATE;
        ops.push_back(o);
      }
    }
    ok(h, plk_update_partials(h, ops.data(), (int)ops.size()), "plk_update_partials");
    ok(h, plk_smap_sample(h, sm.getEngineIndex(rootId), (int)br.size(), br.data(), nullptr, len.data(), seed, 0, (int)R, 0, 0u),
       "plk_smap_sample");
    std::vector<uint32_t> cs(br.size() * nPat * T), tal(br.size() * nPat * S);
    std::vector<double> ds(br.size() * nPat * S);
    ok(h, plk_smap_get_sums(h, (int)br.size(), br.data(), cs.data(), ds.data()), "plk_smap_get_sums");
    ok(h, plk_smap_get_tallies(h, (int)br.size(), br.data(), tal.data(), nullptr), "plk_smap_get_tallies");
    bool same = true;
    uint64_t events = 0;
    for (size_t b = 0; b < ids.size(); b++)
      for (size_t i = 0; i < n; i++) {
        const size_t p = tl.getRootArrayPosition(i);
        const std::vector<double> mc = sm.getMeanCounts(ids[b], i), md = sm.getMeanDwellingTimes(ids[b], i),
                                  sf = sm.getStateFrequencies(ids[b], i);
        for (size_t k = 0; k < T; k++) {
          same = same && mc[k] == (double)cs[(b * nPat + p) * T + k] / (double)R;
          events += cs[(b * nPat + p) * T + k];
        }
        for (size_t x = 0; x < S; x++)
          same = same && md[x] == ds[(b * nPat + p) * S + x] / (double)R && sf[x] == (double)tal[(b * nPat + p) * S + x] / (double)R;
      }
    expect("the mirror's means are the hand-built handle's sums / R", same);
    expect("events were sampled", events > 0);
    plk_destroy(h);
  }

  // 2., 3., 4. with the total register and kept replicates
  const size_t R = 1024;
  TotalSubstitutionRegister total(&model);
  DeviceStochasticMapping sm(tl, total, true);
  sm.sample(20261021, R);
  {
    MarginalAncestralStateReconstruction asr(&tl);
    double worst = 0.;
    for (int id : tl.getInnerNodesId()) {
      VVdouble probs;
      asr.getAncestralStatesForNode(id, probs, false);
      for (size_t x = 0; x < S; x++) {
        double obs = 0., want = 0., var = 0.;
        for (size_t p = 0; p < nPat; p++) {
          obs += sm.getStateFrequencies(id, siteOf[p])[x] * (double)R;
          want += probs[p][x] * (double)R;
          var += probs[p][x] * (1. - probs[p][x]) * (double)R;
        }
        worst = std::max(worst, std::fabs(obs - want) / std::sqrt(var));
      }
    }
    expectBelow("state frequencies vs MarginalAncestralStateReconstruction, largest |z|", worst, 6.);
  }
  {
    DecompositionSubstitutionCount countTot(&model, new TotalSubstitutionRegister(&model));
    std::unique_ptr<ProbabilisticSubstitutionMapping> map(SubstitutionMappingTools::computeSubstitutionVectors(tl, ids, countTot, false));
    double worst = 0., worstMean = 0., worstDwell = 0.;
    bool tipsKept = true;
    for (int id : ids) {
      const double t = ltt.getNode(id)->getDistanceToFather();
      double want = 0., sum = 0., sum2 = 0., fromMeans = 0.;
      for (size_t p = 0; p < nPat; p++) {
        want += map->getNumberOfSubstitutions(id, siteOf[p], 0);
        fromMeans += sm.getMeanCounts(id, siteOf[p])[0];
      }
      for (size_t r = 0; r < R; r++) {
        double x = 0.;
        for (size_t p = 0; p < nPat; p++) {
          x += sm.getCounts(r, id, siteOf[p])[0];
          if (r % 64 == 0) {
            const std::vector<double> d = sm.getDwellingTimes(r, id, siteOf[p]);
            worstDwell = std::max(worstDwell, std::fabs(d[0] + d[1] + d[2] + d[3] - t) / t);
            if (ltt.getNode(id)->isLeaf()) {
              const int obs = tl.getLeafPatternStates(id)[p];
              if (obs >= 0 && obs < 4) tipsKept = tipsKept && sm.getNodeState(r, id, siteOf[p]) == (size_t)obs;
            }
          }
        }
        sum += x;
        sum2 += x * x;
      }
      const double mean = sum / R, se = std::sqrt((sum2 - R * mean * mean) / (R - 1.) / R);
      std::cout << "branch above node " << id << ": sampled mean " << mean << ", expected " << want << ", se " << se << std::endl;
      worst = std::max(worst, std::fabs(mean - want) / se);
      worstMean = std::max(worstMean, std::fabs(mean - fromMeans) / std::max(1., mean));
    }
    expectBelow("total counts vs computeSubstitutionVectors, largest |z|", worst, 6.);
    expectBelow("means vs kept rows, relative", worstMean, 1e-12);
    expectBelow("dwelling times sum to the branch length, relative", worstDwell, 1e-12);
    expect("resolved leaves keep their state", tipsKept);
  }
  bool threw = false;
  try {
    sm.getMeanCounts(rootId, 0);
  } catch (Exception&) {
    threw = true;
  }
  expect("the root has no branch", threw);
  expect("-lnL after the mappings unchanged", tl.getValue() == lnl0);
  if (failures) {
    std::cout << failures << " FAILURES" << std::endl;
    return 1;
  }
  std::cout << "PASSED" << std::endl;
  return 0;
}
