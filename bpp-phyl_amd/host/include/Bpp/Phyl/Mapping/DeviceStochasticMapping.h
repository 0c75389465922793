// Stochastic mapping on the MI355X: histories of substitutions on every branch, sampled from their
// posterior given the data (what Mapping/StochasticMapping.{h,cpp} samples one site at a time and
// by rejection), over plk_smap_sample (include/plk.h).  Built from a double-recursive likelihood
// and a SubstitutionRegister, as SubstitutionMappingTools::computeSubstitutionVectors is: the
// generator comes from the likelihood's model(s), the event types from the register.
//
// The object owns an engine handle of its own (AbstractPlkTreeLikelihood::createMappingEngine): the
// likelihood's engine keeps its partials in registers for the common shapes, and the sampler
// reads them from memory.  It holds the parameters the likelihood had at construction.
//
// sample(seed, n) draws replicates 0 .. n - 1 of that seed (a result depends on seed, replicate,
// site pattern and node only) and replaces the results of an earlier call.  Means are over the
// replicates; sites are expanded from the likelihood's distinct patterns.  With keep = true the
// per-replicate rows stay on the device and getNodeState, getCounts and getDwellingTimes read one
// replicate.  Not provided: the reference's StochasticMapping class with its Tree* per mapping,
// generateExpectedMapping, event lists with times.
#ifndef BPP_AMD_DEVICESTOCHASTICMAPPING_H
#define BPP_AMD_DEVICESTOCHASTICMAPPING_H

#include <cstdint>
#include <map>
#include <vector>

#include "../Likelihood/DRTreeLikelihoodTools.h"
#include "SubstitutionRegister.h"

struct plk_handle_s;  // include/plk.h

namespace bpp {

class DeviceStochasticMapping {
  AbstractPlkTreeLikelihood::MappingEngine eng_;
  std::vector<size_t> links_;  // site -> pattern
  size_t nbSites_ = 0, nbPatterns_ = 0, nbStates_ = 0, nbTypes_ = 0, nbReplicates_ = 0;
  bool keep_;
  uint64_t seed_ = 0;
  std::map<int, size_t> branchRow_;   // node id -> row of the branch arrays
  std::vector<int> nodeIds_;          // every node, in the order of the tallies
  std::map<int, size_t> nodeRow_;
  std::vector<uint32_t> countSum_;    // [branch][pattern][type]
  std::vector<double> dwellSum_;      // [branch][pattern][state]
  std::vector<uint32_t> stateTally_;  // [node][pattern][state]
  // the last kept row read of each kind (a caller walks the sites of one replicate and node)
  mutable std::vector<uint8_t> rowStates_;
  mutable std::vector<uint16_t> rowCounts_;
  mutable std::vector<double> rowDwell_;
  mutable int64_t keyStates_ = -1, keyCounts_ = -1, keyDwell_ = -1;

  void check(int rc, const char* what) const;
  size_t branchRow(int nodeId) const;
  size_t pattern(size_t site) const;
  void needSample(bool kept, size_t replicate) const;

 public:
  DeviceStochasticMapping(const DRTreeLikelihood& drtl, const SubstitutionRegister& reg, bool keep = false);
  ~DeviceStochasticMapping();
  DeviceStochasticMapping(const DeviceStochasticMapping&) = delete;
  DeviceStochasticMapping& operator=(const DeviceStochasticMapping&) = delete;

  void sample(uint64_t seed, size_t nReplicates);
  size_t getNumberOfReplicates() const { return nbReplicates_; }
  size_t getNumberOfSubstitutionTypes() const { return nbTypes_; }
  size_t getNumberOfSites() const { return nbSites_; }
  // the branches (node ids, the root left out) in the order of the handle's list
  const std::vector<int>& getBranchIds() const { return eng_.branchIds; }
  // means over the replicates at a site: counts per type and dwelling times per state of the
  // branch above nodeId, how often nodeId took each state
  std::vector<double> getMeanCounts(int nodeId, size_t site) const;
  std::vector<double> getMeanDwellingTimes(int nodeId, size_t site) const;
  std::vector<double> getStateFrequencies(int nodeId, size_t site) const;
  // one kept replicate
  size_t getNodeState(size_t replicate, int nodeId, size_t site) const;
  std::vector<unsigned int> getCounts(size_t replicate, int nodeId, size_t site) const;
  std::vector<double> getDwellingTimes(size_t replicate, int nodeId, size_t site) const;
  // the handle and a node's index in it (tests compare with a handle set up by hand)
  plk_handle_s* getEngine() const { return eng_.handle; }
  int getEngineIndex(int nodeId) const { return eng_.engineOfId.at(nodeId); }
};

}  // namespace bpp

#endif
