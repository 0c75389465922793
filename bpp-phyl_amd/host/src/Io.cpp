// Host mirror: file readers (Newick trees, Phylip alignments).  Clean-room, from the formats'
// descriptions; only what the parsimony and distance programs read.
#include <cctype>
#include <fstream>
#include <sstream>

#include "Bpp/Phyl/Io/Newick.h"
#include "Bpp/Seq/Io/Phylip.h"

namespace bpp {

TreeTemplate<Node>* Newick::readTree(const std::string& path) const {
  std::ifstream in(path.c_str());
  if (!in) throw Exception("Newick::readTree: cannot open " + path);
  std::string description, line;
  while (std::getline(in, line)) {
    for (char c : line)
      if (c != '\r' && c != '\n') description += c;
    if (description.find(';') != std::string::npos) break;
  }
  const size_t end = description.find(';');
  if (end == std::string::npos) throw Exception("Newick::readTree: no ';' in " + path);
  return TreeTemplateTools::parenthesisToTree(description.substr(0, end + 1));
}

namespace {
std::string withoutBlanks(const std::string& s) {
  std::string out;
  for (char c : s)
    if (!std::isspace((unsigned char)c)) out += c;
  return out;
}
}  // namespace

VectorSiteContainer* Phylip::readAlignment(const std::string& path, const Alphabet* alphabet) const {
  std::ifstream in(path.c_str());
  if (!in) throw Exception("Phylip::readAlignment: cannot open " + path);
  std::string line;
  size_t nSeq = 0, nSites = 0;
  while (std::getline(in, line))
    if (!withoutBlanks(line).empty()) break;
  {
    std::istringstream head(line);
    if (!(head >> nSeq >> nSites) || nSeq == 0 || nSites == 0)
      throw Exception("Phylip::readAlignment: the first line of " + path + " must hold the two sizes");
  }
  // a name and what follows it on its line
  auto splitName = [&](const std::string& l, std::string& name, std::string& rest) {
    size_t cut;
    if (!extended_) {
      cut = std::min<size_t>(10, l.size());
    } else {
      cut = l.find('\t');
      const size_t two = l.find("  ");
      if (two != std::string::npos && (cut == std::string::npos || two < cut)) cut = two;
      if (cut == std::string::npos) cut = l.size();
    }
    name = l.substr(0, cut);
    while (!name.empty() && std::isspace((unsigned char)name.back())) name.pop_back();
    size_t b = 0;
    while (b < name.size() && std::isspace((unsigned char)name[b])) b++;
    name = name.substr(b);
    rest = withoutBlanks(l.substr(cut));
  };
  std::vector<std::string> names, seqs;
  const size_t w = alphabet->getStateCodingSize();
  const size_t want = nSites * w;
  while (std::getline(in, line)) {
    if (withoutBlanks(line).empty()) continue;
    if (sequential_) {
      if (names.size() == seqs.size() && (seqs.empty() || seqs.back().size() >= want)) {
        if (names.size() == nSeq) break;
        names.emplace_back();
        seqs.emplace_back();
        splitName(line, names.back(), seqs.back());
      } else {
        seqs.back() += withoutBlanks(line);
      }
    } else if (names.size() < nSeq) {
      names.emplace_back();
      seqs.emplace_back();
      splitName(line, names.back(), seqs.back());
    } else {
      // a later block: lines in the order of the first
      size_t k = 0;
      while (k < nSeq && seqs[k].size() >= want) k++;
      size_t shortest = 0;
      for (size_t j = 1; j < nSeq; j++)
        if (seqs[j].size() < seqs[shortest].size()) shortest = j;
      if (k == nSeq) break;
      seqs[shortest] += withoutBlanks(line);
    }
  }
  if (names.size() != nSeq) throw Exception("Phylip::readAlignment: " + path + " holds fewer sequences than its first line says");
  VectorSiteContainer* sites = new VectorSiteContainer(alphabet);
  try {
    for (size_t i = 0; i < nSeq; i++) {
      if (seqs[i].size() != want)
        throw Exception("Phylip::readAlignment: sequence '" + names[i] + "' has " + std::to_string(seqs[i].size() / w) + " sites, not " +
                        std::to_string(nSites));
      sites->addSequence(BasicSequence(names[i], seqs[i], alphabet));
    }
  } catch (...) {
    delete sites;
    throw;
  }
  return sites;
}

}  // namespace bpp
