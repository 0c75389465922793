// Mapping/SubstitutionMappingTools.h: probabilistic substitution mapping from a
// double-recursive likelihood.  The reference's six-deep host loop (node x site x class x x x
// y x type) is one device call here (plk_branch_counts, AbstractPlkTreeLikelihood::
// computeBranchCounts); the host expands the engine's patterns to sites.
#ifndef BPP_AMD_SUBSTITUTIONMAPPINGTOOLS_H
#define BPP_AMD_SUBSTITUTIONMAPPINGTOOLS_H

#include <vector>

#include "../Likelihood/DRTreeLikelihoodTools.h"
#include "ProbabilisticSubstitutionMapping.h"
#include "SubstitutionCount.h"

namespace bpp {

struct SubstitutionMappingTools {
  // nodeIds: the nodes whose branches are counted on; empty: every node but the root.  The
  // caller owns the result.
  static ProbabilisticSubstitutionMapping* computeSubstitutionVectors(const DRTreeLikelihood& drtl,
                                                                      const std::vector<int>& nodeIds,
                                                                      SubstitutionCount& substitutionCount,
                                                                      bool verbose = true);
  static ProbabilisticSubstitutionMapping* computeSubstitutionVectors(const DRTreeLikelihood& drtl,
                                                                      SubstitutionCount& substitutionCount,
                                                                      bool verbose = true) {
    return computeSubstitutionVectors(drtl, std::vector<int>(), substitutionCount, verbose);
  }
};

}  // namespace bpp

#endif
