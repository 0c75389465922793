// The mirror's file readers on the two parsimony fixtures (no device): prints what Newick::readTree
// and Phylip::readAlignment return, for tests/test_readers_host.py to compare with its own reading
// of the files.  argv[1]: the directory of example1.ph and example1.mp.dnd.
#include <Bpp/Phyl/Io/Newick.h>
#include <Bpp/Seq/Alphabet/AlphabetTools.h>
#include <Bpp/Seq/Io/Phylip.h>

#include <iomanip>
#include <iostream>
#include <memory>

using namespace bpp;

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "tests/golden";
  try {
    Newick treeReader;
    std::unique_ptr<TreeTemplate<Node> > tree(treeReader.readTree(dir + "/example1.mp.dnd"));
    std::cout << std::setprecision(17);
    for (const Node* n : const_cast<const TreeTemplate<Node>&>(*tree).getNodes()) {
      std::cout << "NODE " << n->getId() << " " << (n->hasName() ? n->getName() : "-") << " "
                << (n->hasFather() ? n->getFather()->getId() : -1) << " " << n->getNumberOfSons() << " ";
      if (n->hasDistanceToFather())
        std::cout << n->getDistanceToFather();
      else
        std::cout << "none";
      std::cout << std::endl;
    }
    std::cout << "NEWICK " << TreeTemplateTools::treeToParenthesis(*tree) << std::endl;
    Phylip alnReader(false, false);
    std::unique_ptr<SiteContainer> sites(alnReader.readAlignment(dir + "/example1.ph", &AlphabetTools::DNA_ALPHABET));
    std::cout << "ALN " << sites->getNumberOfSequences() << " " << sites->getNumberOfSites() << std::endl;
    for (size_t i = 0; i < sites->getNumberOfSequences(); i++) {
      const Sequence& s = sites->getSequence(i);
      std::cout << "SEQ " << s.getName() << " " << s.toString();
      for (size_t k = 0; k < s.size(); k++) std::cout << " " << s.getValue(k);
      std::cout << std::endl;
    }
    // the same alignment through the sequential reader: one line per sequence is both layouts
    Phylip sequential(false, true);
    std::unique_ptr<SiteContainer> again(sequential.readAlignment(dir + "/example1.ph", &AlphabetTools::DNA_ALPHABET));
    bool same = again->getNumberOfSequences() == sites->getNumberOfSequences();
    for (size_t i = 0; same && i < sites->getNumberOfSequences(); i++)
      same = again->getSequence(i).getName() == sites->getSequence(i).getName() &&
             again->getSequence(i).getContent() == sites->getSequence(i).getContent();
    if (!same) {
      std::cout << "sequential and interleaved readings differ" << std::endl;
      return 1;
    }
    bool threw = false;
    try {
      treeReader.readTree(dir + "/no_such_file.dnd");
    } catch (Exception&) {
      threw = true;
    }
    if (!threw) {
      std::cout << "a missing file raised nothing" << std::endl;
      return 1;
    }
  } catch (std::exception& e) {
    std::cout << "exception: " << e.what() << std::endl;
    return 1;
  }
  std::cout << "PASSED" << std::endl;
  return 0;
}
