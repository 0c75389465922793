// NNISearchable.h: what NNITopologySearch needs of an object whose tree it rearranges.
#ifndef BPP_AMD_NNISEARCHABLE_H
#define BPP_AMD_NNISEARCHABLE_H

#include "TopologySearch.h"
#include "TreeTemplate.h"

namespace bpp {

class NNISearchable : public TopologyListener {
 public:
  // The change of the score if the node changed places with its uncle: negative for an
  // improvement.  nodeId is neither the root nor a son of the root.
  virtual double testNNI(int nodeId) const = 0;
  // Apply that interchange.
  virtual void doNNI(int nodeId) = 0;
  virtual const Tree& getTopology() const = 0;
  // The current score (lower is better).
  virtual double getTopologyValue() const = 0;
};

}  // namespace bpp

#endif
