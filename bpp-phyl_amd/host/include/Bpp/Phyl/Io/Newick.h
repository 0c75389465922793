// Io/Newick.h: reads the first tree of a Newick file (the description may span lines).
#ifndef BPP_AMD_NEWICK_H
#define BPP_AMD_NEWICK_H

#include <string>

#include "../TreeTemplate.h"

namespace bpp {

class Newick {
 public:
  Newick() {}
  // the caller owns the tree; ids are the postorder index
  TreeTemplate<Node>* readTree(const std::string& path) const;
  TreeTemplate<Node>* read(const std::string& path) const { return readTree(path); }
};

}  // namespace bpp

#endif
