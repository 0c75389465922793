// Parsimony/AbstractTreeParsimonyScore.h: the tree (a copy, kept as given: not unrooted), the
// data and the state count of a parsimony score.  With includeGaps the gap is one more state.
#ifndef BPP_AMD_ABSTRACTTREEPARSIMONYSCORE_H
#define BPP_AMD_ABSTRACTTREEPARSIMONYSCORE_H

#include <memory>

#include "../../Seq/Container/SiteContainer.h"
#include "TreeParsimonyScore.h"

namespace bpp {

class AbstractTreeParsimonyScore : public virtual TreeParsimonyScore {
 protected:
  std::unique_ptr<TreeTemplate<Node> > tree_;
  std::unique_ptr<SiteContainer> data_;
  const Alphabet* alphabet_;
  bool includeGaps_;
  size_t nbStates_;

  TreeTemplate<Node>* getTreeP_() { return tree_.get(); }
  const TreeTemplate<Node>* getTreeP_() const { return tree_.get(); }

 public:
  AbstractTreeParsimonyScore(const Tree& tree, const SiteContainer& data, bool verbose, bool includeGaps);
  const Tree& getTree() const override { return *tree_; }
  std::vector<unsigned int> getScoreForEachSite() const override;
  size_t getNumberOfStates() const { return nbStates_; }
};

}  // namespace bpp

#endif
