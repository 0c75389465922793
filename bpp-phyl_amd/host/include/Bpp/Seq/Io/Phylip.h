// Seq/Io/Phylip.h: reads a Phylip alignment.  The first line holds the number of sequences and of
// sites.  Classic format (extended = false): a name is the first 10 characters of its line;
// extended: the name ends at the first run of two blanks (or a tab).  Sequential: a sequence runs
// over as many lines as it needs before the next name; interleaved: blocks of one line per
// sequence, names in the first block only.  Blanks inside a sequence are dropped.
#ifndef BPP_AMD_PHYLIP_H
#define BPP_AMD_PHYLIP_H

#include <string>

#include "../Container/SiteContainer.h"

namespace bpp {

class Phylip {
  bool extended_, sequential_;

 public:
  explicit Phylip(bool extended = true, bool sequential = true) : extended_(extended), sequential_(sequential) {}
  // the caller owns the container
  VectorSiteContainer* readAlignment(const std::string& path, const Alphabet* alphabet) const;
};

}  // namespace bpp

#endif
