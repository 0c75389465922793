// Likelihood/AncestralStateReconstruction.h: the interface of the ancestral state
// reconstruction methods, and the host-only helpers of the mirror's implementation
// (namespace ancestral: no engine, no likelihood object -- usable and testable on their own).
#ifndef BPP_AMD_ANCESTRALSTATERECONSTRUCTION_H
#define BPP_AMD_ANCESTRALSTATERECONSTRUCTION_H

#include <cstddef>
#include <map>
#include <vector>

#include "../../Numeric/VectorTools.h"
#include "../../Seq/Sequence.h"

namespace bpp {

namespace ancestral {

// One-hot row on the first of the largest entries of `row` (a leaf's init values).
inline size_t oneHot(const std::vector<double>& row, std::vector<double>& probs) {
  const size_t j = VectorTools::whichMax(row);
  probs.assign(row.size(), 0.);
  if (!row.empty()) probs[j] = 1.;
  return j;
}

// The state drawn from `probs` by the uniform number r in [0, 1): the first state whose
// cumulated probability reaches r.  Rounding can leave the total a few ulps below r; the draw
// then falls on the last state with a non-zero probability, never on an impossible one.
inline size_t sampleState(const std::vector<double>& probs, double r) {
  double cum = 0.;
  size_t last = 0;
  for (size_t j = 0; j < probs.size(); j++) {
    if (!(probs[j] > 0.)) continue;
    cum += probs[j];
    last = j;
    if (r <= cum) return j;
  }
  return last;
}

// Per-pattern values to per-site values through the site -> pattern links.
template <class T>
std::vector<T> expandPatterns(const std::vector<T>& perPattern, const std::vector<size_t>& links) {
  std::vector<T> out(links.size());
  for (size_t i = 0; i < links.size(); i++) out[i] = perPattern.at(links[i]);
  return out;
}

}  // namespace ancestral

class AncestralStateReconstruction {
 public:
  virtual ~AncestralStateReconstruction() {}
  // the ancestral states of one node, per distinct site pattern
  virtual std::vector<size_t> getAncestralStatesForNode(int nodeId) const = 0;
  // every node's states (leaves: their observed states), by node id
  virtual std::map<int, std::vector<size_t> > getAllAncestralStates() const = 0;
  // the ancestral sequence of one node, per site (the caller owns it)
  virtual Sequence* getAncestralSequenceForNode(int nodeId) const = 0;
};

}  // namespace bpp

#endif
