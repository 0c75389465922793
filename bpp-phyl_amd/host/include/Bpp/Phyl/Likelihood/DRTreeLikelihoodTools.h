// Likelihood/DRTreeLikelihoodTools.h: posterior probabilities of the states at a node from a
// double-recursive likelihood.  Internal nodes are served by the device
// (plk_node_posteriors); the class probabilities are part of the joint, which is the
// reference's value whenever they are equal.
#ifndef BPP_AMD_DRTREELIKELIHOODTOOLS_H
#define BPP_AMD_DRTREELIKELIHOODTOOLS_H

#include "TreeLikelihood.h"

namespace bpp {

typedef AbstractPlkTreeLikelihood DRTreeLikelihood;

struct DRTreeLikelihoodTools {
  // [distinct site pattern][rate class][state]
  static VVVdouble getPosteriorProbabilitiesForEachStateForEachRate(const DRTreeLikelihood& drl, int nodeId);
  // mean of the state posteriors over the patterns, weighted by the pattern weights
  static Vdouble getPosteriorStateFrequencies(const DRTreeLikelihood& drl, int nodeId);
};

}  // namespace bpp

#endif
