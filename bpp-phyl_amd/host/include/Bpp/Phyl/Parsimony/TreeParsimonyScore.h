// Parsimony/TreeParsimonyScore.h: what a parsimony score of an alignment on a tree offers.
#ifndef BPP_AMD_TREEPARSIMONYSCORE_H
#define BPP_AMD_TREEPARSIMONYSCORE_H

#include <vector>

#include "../TreeTemplate.h"

namespace bpp {

class TreeParsimonyScore {
 public:
  virtual ~TreeParsimonyScore() {}
  virtual TreeParsimonyScore* clone() const = 0;
  // the number of changes over all sites
  virtual unsigned int getScore() const = 0;
  virtual unsigned int getScoreForSite(size_t site) const = 0;
  virtual std::vector<unsigned int> getScoreForEachSite() const = 0;
  virtual const Tree& getTree() const = 0;
};

}  // namespace bpp

#endif
