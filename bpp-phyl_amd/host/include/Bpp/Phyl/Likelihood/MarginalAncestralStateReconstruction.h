// Likelihood/MarginalAncestralStateReconstruction.h: marginal reconstruction of ancestral
// states from a double-recursive likelihood (DRHomogeneousTreeLikelihood or
// DRNonHomogeneousTreeLikelihood).  The posteriors of internal nodes are formed on the device
// (plk_node_posteriors); only the state probabilities, or one byte per node and pattern,
// come back.
#ifndef BPP_AMD_MARGINALANCESTRALSTATERECONSTRUCTION_H
#define BPP_AMD_MARGINALANCESTRALSTATERECONSTRUCTION_H

#include "AncestralStateReconstruction.h"
#include "TreeLikelihood.h"

namespace bpp {

class MarginalAncestralStateReconstruction : public AncestralStateReconstruction {
  const AbstractPlkTreeLikelihood* likelihood_;  // not owned

 public:
  explicit MarginalAncestralStateReconstruction(const AbstractPlkTreeLikelihood* drl);
  // States per distinct pattern and their posterior probabilities [pattern][state].  A leaf is
  // one-hot on the first maximum of its init values.  sample: states drawn from the posterior
  // (RandomTools) instead of the most probable ones.
  std::vector<size_t> getAncestralStatesForNode(int nodeId, VVdouble& probs, bool sample) const;
  std::vector<size_t> getAncestralStatesForNode(int nodeId) const override;
  // one engine call for the most probable states of all internal nodes
  std::map<int, std::vector<size_t> > getAllAncestralStates() const override;
  // per site; probs (may be null) receives the per-site posterior probabilities
  Sequence* getAncestralSequenceForNode(int nodeId, VVdouble* probs, bool sample) const;
  Sequence* getAncestralSequenceForNode(int nodeId) const override {
    return getAncestralSequenceForNode(nodeId, nullptr, false);
  }
};

}  // namespace bpp

#endif
