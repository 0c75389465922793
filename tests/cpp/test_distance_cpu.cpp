// NeighborJoining and BioNJ of the Bio++ API mirror, no GPU.  On the additive matrix of a fixed
// 9-leaf tree both methods must return that tree: its bipartitions and every branch length to
// 1e-12, unrooted (a three-son root) and rooted (the root on the last branch; its two branches
// add up to the split's length).  For that matrix plus the symmetric perturbation
// 0.01 sin(3 i + 5 j), i < j, and for a 5-taxon matrix that yields a negative length (with and
// without positiveLengths), the trees are printed as "TREE <case> <method> <shape> <newick>" for
// tests/test_distance_host.py, which compares them with its own numpy NJ and BioNJ.
// Prints PASSED and exits 0 on success.
#include <Bpp/Phyl/Distance/BioNJ.h>
#include <Bpp/Phyl/Distance/NeighborJoining.h>
#include <Bpp/Phyl/TreeTemplate.h>

#include <algorithm>
#include <cmath>
#include <iostream>
#include <map>
#include <memory>
#include <set>

using namespace bpp;

static int failures = 0;

static void expect(const std::string& what, bool ok) {
  std::cout << what << (ok ? " ok" : " FAIL") << std::endl;
  if (!ok) failures++;
}

typedef std::map<std::set<std::string>, double> Splits;

// the side without the first leaf name -> branch length (the two branches of a two-son root add up)
static Splits splitsOf(const TreeTemplate<Node>& tree) {
  std::vector<std::string> names = tree.getLeavesNames();
  std::sort(names.begin(), names.end());
  const std::set<std::string> all(names.begin(), names.end());
  Splits out;
  for (const Node* n : tree.getNodes()) {
    if (!n->hasFather()) continue;
    std::set<std::string> side;
    for (const Node* l : TreeTemplateTools::getLeaves(*n)) side.insert(l->getName());
    if (side.count(names[0])) {
      std::set<std::string> other;
      for (const std::string& s : all)
        if (!side.count(s)) other.insert(s);
      side.swap(other);
    }
    out[side] += n->getDistanceToFather();
  }
  return out;
}

static bool same(const Splits& a, const Splits& b, double tol) {
  if (a.size() != b.size()) return false;
  for (const auto& kv : a) {
    auto it = b.find(kv.first);
    if (it == b.end() || std::fabs(it->second - kv.second) > tol) return false;
  }
  return true;
}

static DistanceMatrix additiveMatrix(const TreeTemplate<Node>& tree) {
  std::vector<const Node*> leaves = tree.getLeaves();
  std::sort(leaves.begin(), leaves.end(), [](const Node* a, const Node* b) { return a->getName() < b->getName(); });
  std::vector<std::string> names;
  for (const Node* l : leaves) names.push_back(l->getName());
  DistanceMatrix D(names);
  for (size_t i = 0; i < leaves.size(); i++) {
    std::map<const Node*, double> up;
    double acc = 0.;
    for (const Node* n = leaves[i]; n; n = n->getFather()) {
      up[n] = acc;
      if (n->hasFather()) acc += n->getDistanceToFather();
    }
    for (size_t j = 0; j < leaves.size(); j++) {
      if (i == j) continue;
      acc = 0.;
      for (const Node* n = leaves[j]; n; n = n->getFather()) {
        if (up.count(n)) {
          D(i, j) = acc + up[n];
          break;
        }
        acc += n->getDistanceToFather();
      }
    }
  }
  return D;
}

template <class Method>
static void runCase(const std::string& label, const DistanceMatrix& D, bool positive, const Splits* want) {
  for (int rooted = 0; rooted < 2; rooted++) {
    Method m(D, rooted != 0, positive, false);
    std::unique_ptr<TreeTemplate<Node> > t(m.getTree());
    const std::string what = label + " " + m.getName() + (rooted ? " rooted" : " unrooted");
    expect(what + ": root has " + (rooted ? "two" : "three") + " sons",
           t->getRootNode()->getNumberOfSons() == (rooted ? 2u : 3u));
    expect(what + ": leaves are named from the matrix", t->getNumberOfLeaves() == D.size());
    if (want) expect(what + ": the tree's bipartitions and lengths to 1e-12", same(splitsOf(*t), *want, 1e-12));
    // the setter path gives the same tree as the constructor
    Method m2(rooted != 0, positive, false);
    m2.setDistanceMatrix(D);
    m2.computeTree();
    std::unique_ptr<TreeTemplate<Node> > t2(m2.getTree());
    expect(what + ": setDistanceMatrix + computeTree", same(splitsOf(*t2), splitsOf(*t), 0.));
    std::cout << "TREE " << label << " " << m.getName() << " " << (rooted ? "rooted" : "unrooted") << " "
              << TreeTemplateTools::treeToParenthesis(*t) << std::endl;
  }
}

int main() {
  try {
    std::unique_ptr<TreeTemplate<Node> > tree(TreeTemplateTools::parenthesisToTree(
        "(((A:0.11,B:0.23):0.07,(C:0.31,D:0.05):0.13):0.09,((E:0.17,F:0.19):0.21,G:0.29):0.03,"
        "(H:0.37,I:0.02):0.15);"));
    const DistanceMatrix D = additiveMatrix(*tree);
    const Splits want = splitsOf(*tree);
    expect("the fixed tree has 15 branches", want.size() == 15);
    runCase<NeighborJoining>("additive", D, false, &want);
    runCase<BioNJ>("additive", D, false, &want);

    DistanceMatrix P(D);
    for (size_t i = 0; i < P.size(); i++)
      for (size_t j = i + 1; j < P.size(); j++) P(i, j) = P(j, i) = D(i, j) + 0.01 * std::sin(3. * (double)i + 5. * (double)j);
    runCase<NeighborJoining>("perturbed", P, false, nullptr);
    runCase<BioNJ>("perturbed", P, false, nullptr);

    const double neg[5][5] = {{0.0, 0.1, 5.0, 5.2, 4.9}, {0.1, 0.0, 1.0, 1.3, 0.8}, {5.0, 1.0, 0.0, 0.6, 1.1},
                              {5.2, 1.3, 0.6, 0.0, 1.2}, {4.9, 0.8, 1.1, 1.2, 0.0}};
    DistanceMatrix N(std::vector<std::string>{"A", "B", "C", "D", "E"});
    for (size_t i = 0; i < 5; i++)
      for (size_t j = 0; j < 5; j++) N(i, j) = neg[i][j];
    runCase<NeighborJoining>("negative", N, false, nullptr);
    runCase<BioNJ>("negative", N, false, nullptr);
    runCase<NeighborJoining>("positive", N, true, nullptr);
    runCase<BioNJ>("positive", N, true, nullptr);
    {
      NeighborJoining a(N, false, false, false), b(N, false, true, false);
      std::unique_ptr<TreeTemplate<Node> > ta(a.getTree()), tb(b.getTree());
      double lo = 0., lob = 1.;
      for (const auto& kv : splitsOf(*ta)) lo = std::min(lo, kv.second);
      for (const auto& kv : splitsOf(*tb)) lob = std::min(lob, kv.second);
      expect("the 5-taxon matrix yields a negative length", lo < -0.1);
      expect("positiveLengths clamps it to 0", lob == 0.);
    }
    NeighborJoining nj;
    BioNJ bio;
    expect("names", nj.getName() == "NJ" && bio.getName() == "BioNJ");
    expect("no tree before computeTree", nj.getTree() == nullptr);
    nj.setVerbose(false);
    expect("setVerbose", !nj.isVerbose());
  } catch (std::exception& e) {
    std::cout << "exception: " << e.what() << std::endl;
    return 1;
  }
  if (failures) {
    std::cout << failures << " check(s) FAILED" << std::endl;
    return 1;
  }
  std::cout << "PASSED" << std::endl;
  return 0;
}
