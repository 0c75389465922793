// Mapping/ProbabilisticSubstitutionMapping.h: per branch, site and substitution type, the
// posterior expected number of substitutions (the result of
// SubstitutionMappingTools::computeSubstitutionVectors).
#ifndef BPP_AMD_PROBABILISTICSUBSTITUTIONMAPPING_H
#define BPP_AMD_PROBABILISTICSUBSTITUTIONMAPPING_H

#include <map>
#include <vector>

#include "../../Exceptions.h"
#include "../../Text/TextTools.h"

namespace bpp {

class ProbabilisticSubstitutionMapping {
  std::vector<int> nodeIds_;            // the branches, by the id of the node below
  std::map<int, size_t> index_;
  size_t nbSites_ = 0, nbTypes_ = 0;
  std::vector<double> counts_;          // [branch][site][type]

 public:
  ProbabilisticSubstitutionMapping() {}
  ProbabilisticSubstitutionMapping(const std::vector<int>& nodeIds, size_t nbSites, size_t nbTypes)
      : nodeIds_(nodeIds), nbSites_(nbSites), nbTypes_(nbTypes), counts_(nodeIds.size() * nbSites * nbTypes, 0.) {
    for (size_t i = 0; i < nodeIds_.size(); i++) index_[nodeIds_[i]] = i;
  }
  size_t getNumberOfSites() const { return nbSites_; }
  size_t getNumberOfBranches() const { return nodeIds_.size(); }
  size_t getNumberOfSubstitutionTypes() const { return nbTypes_; }
  const std::vector<int>& getNodesId() const { return nodeIds_; }
  size_t getNodeIndex(int nodeId) const {
    auto it = index_.find(nodeId);
    if (it == index_.end())
      throw Exception("ProbabilisticSubstitutionMapping: no branch above node " + TextTools::toString(nodeId));
    return it->second;
  }
  // type from 0
  double getNumberOfSubstitutions(int nodeId, size_t siteIndex, size_t type) const {
    return (*this)(getNodeIndex(nodeId), siteIndex, type);
  }
  std::vector<double> getNumberOfSubstitutions(int nodeId, size_t siteIndex) const {
    const double* p = &(*this)(getNodeIndex(nodeId), siteIndex, 0);
    return std::vector<double>(p, p + nbTypes_);
  }
  double& operator()(size_t branchIndex, size_t siteIndex, size_t type) {
    return counts_[(branchIndex * nbSites_ + siteIndex) * nbTypes_ + type];
  }
  const double& operator()(size_t branchIndex, size_t siteIndex, size_t type) const {
    return counts_[(branchIndex * nbSites_ + siteIndex) * nbTypes_ + type];
  }
};

}  // namespace bpp

#endif
