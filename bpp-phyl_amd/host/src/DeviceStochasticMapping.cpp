// Host mirror: DeviceStochasticMapping (see the header) over plk_smap_sample, and the second
// engine handle a likelihood hands it.
#include "Bpp/Phyl/Mapping/DeviceStochasticMapping.h"

#include <cstdlib>

#include "Bpp/Exceptions.h"
#include "Bpp/Text/TextTools.h"
#include "plk.h"

namespace bpp {

// Everything the likelihood's own engine was given, on a handle that keeps every partial:
// code table, tip codes and weights (uploadData), eigen systems, rates and root frequencies
// (uploadModels), P(t) of every branch (updatePmatrices: host P(t) for a model without a usable
// eigen system), the generators for plk_smap_sample, then one full traversal.
AbstractPlkTreeLikelihood::MappingEngine AbstractPlkTreeLikelihood::createMappingEngine() const {
  if (!initialized_) throw Exception("createMappingEngine: instance is not initialized.");
  const size_t S = nbStates_, C = nbClasses_;
  const char* dev = std::getenv("BPP_AMD_DEVICE");
  const unsigned flags = (unsigned)PLK_FLAG_SCALING | (engineGuard_ ? (unsigned)PLK_FLAG_NONNEG_GUARD : 0u);
  plk_handle h = nullptr;
  int rc = plk_create(dev ? std::atoi(dev) : 0, (int)S, (int)C, (int64_t)nbDistinctSites_, nTips_, nInternal_,
                      (int)engineModels_, flags, &h);
  if (rc != PLK_OK) throw DeviceException(rc, std::string("plk_create: ") + plk_last_error(nullptr));
  MappingEngine out;
  out.handle = h;
  out.root = rootEngine_;
  auto ok = [&](int r, const char* what) {
    if (r == PLK_OK) return;
    const std::string msg = std::string(what) + ": " + plk_last_error(h);
    plk_destroy(h);
    throw DeviceException(r, msg);
  };
  const SubstitutionModel* m0 = modelForIndex(0);
  const int nc = (int)data_->getAlphabet()->getNumberOfCodes();
  std::vector<double> table((size_t)nc * S);
  for (int c = 0; c < nc; c++)
    for (size_t s = 0; s < S; s++) table[(size_t)c * S + s] = m0->getInitValue(s, c);
  ok(plk_set_code_table(h, nc, table.data()), "plk_set_code_table");
  std::vector<uint8_t> codes(nbDistinctSites_);
  for (int t = 0; t < nTips_; t++) {
    for (size_t p = 0; p < nbDistinctSites_; p++) codes[p] = (uint8_t)patternStates_[(size_t)t][p];
    ok(plk_set_tip_codes(h, t, codes.data()), "plk_set_tip_codes");
  }
  const std::vector<double> w(rootWeights_.begin(), rootWeights_.end());
  ok(plk_set_pattern_weights(h, w.data()), "plk_set_pattern_weights");
  const Vdouble& rates = rateDistribution_->getCategories();
  ok(plk_set_category_rates(h, rates.data(), rateDistribution_->getProbabilities().data()), "plk_set_category_rates");
  ok(plk_set_root_frequencies(h, rootFreqs_.data()), "plk_set_root_frequencies");
  std::vector<double> lam(S), Q(S * S);
  for (size_t m = 0; m < engineModels_; m++) {
    const SubstitutionModel* model = modelForIndex((int)m);
    if (!model) continue;
    const RowMatrix<double>& G = model->getGenerator();
    for (size_t x = 0; x < S; x++)
      for (size_t y = 0; y < S; y++) Q[x * S + y] = G(x, y) * model->getRate();
    ok(plk_smap_set_generator(h, (int)m, Q.data()), "plk_smap_set_generator");
    if (model->needsHostPij()) continue;
    for (size_t k = 0; k < S; k++) lam[k] = model->getEigenValues()[k] * model->getRate();
    ok(plk_set_eigen(h, (int)m, model->getColumnRightEigenVectors().data(), model->getRowLeftEigenVectors().data(),
                     lam.data()),
       "plk_set_eigen");
  }
  std::vector<int32_t> br, mod;
  std::vector<double> t, P(C * S * S);
  for (const Node* n : nodes_) {
    const int e = engineIndex_.at(n), mi = modelIndexForNode(n);
    const double d = n->getDistanceToFather();
    out.branchIds.push_back(n->getId());
    out.branch.push_back(e);
    out.model.push_back(mi);
    out.length.push_back(d);
    const SubstitutionModel* model = modelForIndex(mi);
    if (model && model->needsHostPij()) {
      for (size_t c = 0; c < C; c++) {
        const RowMatrix<double>& Pc = model->getPij_t(d * rates[c]);
        std::copy(Pc.data(), Pc.data() + S * S, P.begin() + c * S * S);
      }
      ok(plk_set_pmatrix(h, e, P.data()), "plk_set_pmatrix");
    } else {
      br.push_back(e);
      mod.push_back(mi);
      t.push_back(d);
    }
  }
  if (!br.empty())
    ok(plk_update_pmatrices(h, (int)br.size(), br.data(), mod.data(), t.data(), PLK_DERIV_P), "plk_update_pmatrices");
  for (const auto& kv : engineIndex_) out.engineOfId[kv.first->getId()] = kv.second;
  std::vector<plk_op> ops(opParent_.size());
  for (size_t i = 0; i < ops.size(); i++) {
    ops[i].parent = opParent_[i];
    ops[i].n_children = (int32_t)opChildren_[i].size();
    for (size_t k = 0; k < 3; k++) ops[i].child[k] = k < opChildren_[i].size() ? opChildren_[i][k] : -1;
    ops[i].flags = opFlags_[i];
  }
  ok(plk_update_partials(h, ops.data(), (int)ops.size()), "plk_update_partials");
  return out;
}

// ---------------------------------------------------------------------------

DeviceStochasticMapping::DeviceStochasticMapping(const DRTreeLikelihood& drtl, const SubstitutionRegister& reg, bool keep)
    : keep_(keep) {
  if (!drtl.isInitialized()) throw Exception("DeviceStochasticMapping: likelihood is not initialized.");
  nbStates_ = drtl.getNumberOfStates();
  nbTypes_ = reg.getNumberOfSubstitutionTypes();
  if (nbTypes_ < 1 || nbTypes_ > 16)
    throw Exception("DeviceStochasticMapping: " + TextTools::toString(nbTypes_) + " substitution types (the engine takes 1 to 16)");
  nbSites_ = drtl.getNumberOfSites();
  nbPatterns_ = drtl.getNumberOfDistinctSites();
  links_ = drtl.getRootArrayPositions();
  eng_ = drtl.createMappingEngine();
  try {
    std::vector<uint8_t> typeOf(nbStates_ * nbStates_, 0);
    for (size_t x = 0; x < nbStates_; x++)
      for (size_t y = 0; y < nbStates_; y++)
        if (x != y) typeOf[x * nbStates_ + y] = (uint8_t)reg.getType(x, y);
    check(plk_smap_set_types(eng_.handle, (int)nbTypes_, typeOf.data()), "plk_smap_set_types");
  } catch (...) {
    plk_destroy(eng_.handle);
    throw;
  }
  for (size_t i = 0; i < eng_.branchIds.size(); i++) branchRow_[eng_.branchIds[i]] = i;
  for (const auto& kv : eng_.engineOfId) {
    nodeRow_[kv.first] = nodeIds_.size();
    nodeIds_.push_back(kv.first);
  }
}

DeviceStochasticMapping::~DeviceStochasticMapping() {
  if (eng_.handle) plk_destroy(eng_.handle);
}

void DeviceStochasticMapping::check(int rc, const char* what) const {
  if (rc != PLK_OK) throw DeviceException(rc, std::string(what) + ": " + plk_last_error(eng_.handle));
}

void DeviceStochasticMapping::sample(uint64_t seed, size_t nReplicates) {
  if (nReplicates == 0) throw Exception("DeviceStochasticMapping::sample: no replicate requested");
  nbReplicates_ = 0;
  keyStates_ = keyCounts_ = keyDwell_ = -1;
  check(plk_smap_sample(eng_.handle, eng_.root, (int)eng_.branch.size(), eng_.branch.data(), eng_.model.data(),
                        eng_.length.data(), seed, 0, (int)nReplicates, 0, keep_ ? PLK_SMAP_KEEP : 0u),
        "plk_smap_sample");
  const size_t nb = eng_.branch.size(), nn = nodeIds_.size();
  countSum_.resize(nb * nbPatterns_ * nbTypes_);
  dwellSum_.resize(nb * nbPatterns_ * nbStates_);
  stateTally_.resize(nn * nbPatterns_ * nbStates_);
  check(plk_smap_get_sums(eng_.handle, (int)nb, eng_.branch.data(), countSum_.data(), dwellSum_.data()), "plk_smap_get_sums");
  std::vector<int32_t> nodes;
  for (int id : nodeIds_) nodes.push_back(eng_.engineOfId.at(id));
  check(plk_smap_get_tallies(eng_.handle, (int)nn, nodes.data(), stateTally_.data(), nullptr), "plk_smap_get_tallies");
  seed_ = seed;
  nbReplicates_ = nReplicates;
}

size_t DeviceStochasticMapping::branchRow(int nodeId) const {
  const auto it = branchRow_.find(nodeId);
  if (it == branchRow_.end())
    throw Exception("DeviceStochasticMapping: node " + TextTools::toString(nodeId) + " has no branch (the root, or no node)");
  return it->second;
}

size_t DeviceStochasticMapping::pattern(size_t site) const {
  if (site >= nbSites_) throw Exception("DeviceStochasticMapping: site " + TextTools::toString(site) + " out of range");
  return links_[site];
}

void DeviceStochasticMapping::needSample(bool kept, size_t replicate) const {
  if (!nbReplicates_) throw Exception("DeviceStochasticMapping: no sample yet.");
  if (kept && !keep_) throw Exception("DeviceStochasticMapping: replicates are kept only with keep = true.");
  if (kept && replicate >= nbReplicates_)
    throw Exception("DeviceStochasticMapping: replicate " + TextTools::toString(replicate) + " out of range");
}

std::vector<double> DeviceStochasticMapping::getMeanCounts(int nodeId, size_t site) const {
  needSample(false, 0);
  const uint32_t* s = countSum_.data() + (branchRow(nodeId) * nbPatterns_ + pattern(site)) * nbTypes_;
  std::vector<double> out(nbTypes_);
  for (size_t k = 0; k < nbTypes_; k++) out[k] = (double)s[k] / (double)nbReplicates_;
  return out;
}

std::vector<double> DeviceStochasticMapping::getMeanDwellingTimes(int nodeId, size_t site) const {
  needSample(false, 0);
  const double* s = dwellSum_.data() + (branchRow(nodeId) * nbPatterns_ + pattern(site)) * nbStates_;
  std::vector<double> out(nbStates_);
  for (size_t x = 0; x < nbStates_; x++) out[x] = s[x] / (double)nbReplicates_;
  return out;
}

std::vector<double> DeviceStochasticMapping::getStateFrequencies(int nodeId, size_t site) const {
  needSample(false, 0);
  const auto it = nodeRow_.find(nodeId);
  if (it == nodeRow_.end()) throw Exception("DeviceStochasticMapping: no node " + TextTools::toString(nodeId));
  const uint32_t* s = stateTally_.data() + (it->second * nbPatterns_ + pattern(site)) * nbStates_;
  std::vector<double> out(nbStates_);
  for (size_t x = 0; x < nbStates_; x++) out[x] = (double)s[x] / (double)nbReplicates_;
  return out;
}

size_t DeviceStochasticMapping::getNodeState(size_t replicate, int nodeId, size_t site) const {
  needSample(true, replicate);
  const size_t p = pattern(site);
  const int e = getEngineIndex(nodeId);
  const int64_t key = (int64_t)replicate * (int64_t)nodeIds_.size() + e;
  if (key != keyStates_) {
    rowStates_.resize(nbPatterns_);
    keyStates_ = -1;
    check(plk_smap_get_states(eng_.handle, replicate, e, rowStates_.data()), "plk_smap_get_states");
    keyStates_ = key;
  }
  return rowStates_[p];
}

std::vector<unsigned int> DeviceStochasticMapping::getCounts(size_t replicate, int nodeId, size_t site) const {
  needSample(true, replicate);
  const size_t p = pattern(site);
  const int e = eng_.branch[branchRow(nodeId)];
  const int64_t key = (int64_t)replicate * (int64_t)nodeIds_.size() + e;
  if (key != keyCounts_) {
    rowCounts_.resize(nbPatterns_ * nbTypes_);
    keyCounts_ = -1;
    check(plk_smap_get_counts(eng_.handle, replicate, e, rowCounts_.data()), "plk_smap_get_counts");
    keyCounts_ = key;
  }
  return std::vector<unsigned int>(rowCounts_.begin() + p * nbTypes_, rowCounts_.begin() + (p + 1) * nbTypes_);
}

std::vector<double> DeviceStochasticMapping::getDwellingTimes(size_t replicate, int nodeId, size_t site) const {
  needSample(true, replicate);
  const size_t p = pattern(site);
  const int e = eng_.branch[branchRow(nodeId)];
  const int64_t key = (int64_t)replicate * (int64_t)nodeIds_.size() + e;
  if (key != keyDwell_) {
    rowDwell_.resize(nbPatterns_ * nbStates_);
    keyDwell_ = -1;
    check(plk_smap_get_dwell(eng_.handle, replicate, e, rowDwell_.data()), "plk_smap_get_dwell");
    keyDwell_ = key;
  }
  return std::vector<double>(rowDwell_.begin() + p * nbStates_, rowDwell_.begin() + (p + 1) * nbStates_);
}

}  // namespace bpp
