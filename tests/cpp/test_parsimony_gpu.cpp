// Fitch parsimony through the Bio++ API mirror on the MI355X (DRTreeParsimonyScore over the
// plk_pars_* calls).  argv[1]: the directory of example1.ph and example1.mp.dnd.
//   1. The reference's golden: score 9 on that alignment and tree with the gap as a state.
//   2. Its second golden: score 3 on an 8-taxon caterpillar of binary characters, and the node
//      states computeSolution() assigns.
//   3. NNITopologySearch (BETTER and FAST) over DRTreeParsimonyScore on 2000 sites simulated on a
//      10-taxon tree perturbed by three interchanges: the final score is at most the true tree's,
//      equals a plain Fitch recount of the final tree written here, every applied interchange
//      changed getScore() by exactly its testNNI value, and every round cost one
//      plk_pars_nni_scores call.
// Prints PASSED and exits 0 on success.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Io/Newick.h>
#include <Bpp/Phyl/Model/Nucleotide/GTR.h>
#include <Bpp/Phyl/Model/RateDistribution/GammaDiscreteRateDistribution.h>
#include <Bpp/Phyl/NNITopologySearch.h>
#include <Bpp/Phyl/Parsimony/DRTreeParsimonyScore.h>
#include <Bpp/Phyl/Simulation/HomogeneousSequenceSimulator.h>
#include <Bpp/Phyl/TreeTemplate.h>
#include <Bpp/Seq/Alphabet/AlphabetTools.h>
#include <Bpp/Seq/Alphabet/BinaryAlphabet.h>
#include <Bpp/Seq/Container/VectorSiteContainer.h>
#include <Bpp/Seq/Io/Phylip.h>

#include <iostream>
#include <map>
#include <memory>

using namespace bpp;

static int failures = 0;

static void expect(const std::string& what, bool ok) {
  std::cout << what << (ok ? " ok" : " FAIL") << std::endl;
  if (!ok) failures++;
}

// ---- a plain Fitch count on the host: per site, sets folded son by son ----
static unsigned int fitchSite(const Node* n, const SiteContainer& sites, size_t site, unsigned long& set) {
  if (n->isLeaf()) {
    set = 0;
    const int v = sites.getSequence(n->getName()).getValue(site);
    const Alphabet* a = sites.getAlphabet();
    for (int s : a->getAlias(v < 0 ? a->getUnknownCharacterCode() : v)) set |= 1ul << s;
    return 0;
  }
  unsigned int changes = 0;
  for (size_t k = 0; k < n->getNumberOfSons(); k++) {
    unsigned long sonSet = 0;
    changes += fitchSite(n->getSon(k), sites, site, sonSet);
    if (k == 0)
      set = sonSet;
    else if (set & sonSet)
      set &= sonSet;
    else {
      set |= sonSet;
      changes++;
    }
  }
  return changes;
}

static unsigned int fitch(const Tree& tree, const SiteContainer& sites) {
  const TreeTemplate<Node> t(tree);
  unsigned int total = 0;
  for (size_t i = 0; i < sites.getNumberOfSites(); i++) {
    unsigned long set = 0;
    total += fitchSite(t.getRootNode(), sites, i, set);
  }
  return total;
}

class ScoreRecorder : public TopologyListener {
  const DRTreeParsimonyScore* pars_;

 public:
  std::vector<unsigned int> scores;
  explicit ScoreRecorder(const DRTreeParsimonyScore* pars) : pars_(pars) {}
  void topologyChangePerformed(const TopologyChangeEvent&) override { scores.push_back(pars_->getScore()); }
};

static std::vector<int> candidates(const Tree& t) {
  const TreeTemplate<Node> tree(t);
  std::vector<int> ids;
  for (const Node* n : tree.getNodes())
    if (n->hasFather() && n->getFather()->hasFather()) ids.push_back(n->getId());
  return ids;
}

static void golden(const std::string& dir) {
  Newick treeReader;
  std::unique_ptr<Tree> tree(treeReader.readTree(dir + "/example1.mp.dnd"));
  Phylip alnReader(false, false);
  std::unique_ptr<SiteContainer> sites(alnReader.readAlignment(dir + "/example1.ph", &AlphabetTools::DNA_ALPHABET));
  DRTreeParsimonyScore pars(*tree, *sites, false, true);
  std::cout << "golden: score " << pars.getScore() << ", " << pars.getNumberOfDistinctSites() << " distinct sites" << std::endl;
  expect("golden: score 9 with the gap as a state", pars.getScore() == 9);
  unsigned int sum = 0;
  for (unsigned int s : pars.getScoreForEachSite()) sum += s;
  expect("golden: the site scores sum to the score", sum == 9 && pars.getScoreForEachSite().size() == 10);
  expect("golden: the gap column costs one change", pars.getScoreForSite(4) == 1);
  DRTreeParsimonyScore noGaps(*tree, *sites, false, false);
  expect("golden: score 8 without it, the host recount's", noGaps.getScore() == 8 && fitch(*tree, *sites) == 8);
  std::unique_ptr<DRTreeParsimonyScore> copy(pars.clone());
  expect("golden: a clone scores alike", copy->getScore() == 9);
}

static void solution() {
  std::unique_ptr<TreeTemplate<Node> > tree(
      TreeTemplateTools::parenthesisToTree("(((((((S1:1,S2:1):1,S3:2):1,S4:3):1,S5:4):1,S6:5):1,S7:6):1,S8:7);"));
  const BinaryAlphabet alphabet;
  VectorSiteContainer sites(&alphabet);
  const char* chars[8] = {"0", "1", "0", "1", "1", "1", "0", "0"};
  for (int i = 0; i < 8; i++) sites.addSequence(BasicSequence("S" + std::to_string(i + 1), chars[i], &alphabet));
  DRTreeParsimonyScore pars(*tree, sites, false);
  expect("solution: score 3", pars.getScore() == 3);
  pars.computeSolution();
  // (((((((S1{0},S2{1})N2{0},S3{0})N4{0},S4{1})N6{1},S5{1})N8{1},S6{1})N10{1},S7{0})N12{0},S8{0})N14{0}
  std::map<std::string, int> want = {{"S1", 0}, {"S2", 1}, {"N2", 0}, {"S3", 0}, {"N4", 0},  {"S4", 1},  {"N6", 1}, {"S5", 1},
                                     {"N8", 1}, {"S6", 1}, {"N10", 1}, {"S7", 0}, {"N12", 0}, {"S8", 0}, {"N14", 0}};
  const TreeTemplate<Node> t(pars.getTree());
  bool all = true;
  size_t n = 0;
  for (const Node* node : t.getNodes()) {
    const std::string name = node->hasName() ? node->getName() : "N" + std::to_string(node->getId());
    const int state = pars.getNodeState(node);
    if (!want.count(name) || want[name] != state) {
      std::cout << "solution: node " << name << " has state " << state << std::endl;
      all = false;
    }
    n++;
  }
  expect("solution: the 15 node states", all && n == 15);
}

static void search(const std::string& algorithm, const TreeTemplate<Node>& tree, const SiteContainer& sites) {
  DRTreeParsimonyScore pars(tree, sites, false);
  const unsigned int trueScore = pars.getScore();
  std::cout << algorithm << ": true tree scores " << trueScore << ", " << pars.getNumberOfDistinctSites() << " patterns" << std::endl;
  expect(algorithm + ": the true tree's score is the host recount", trueScore == fitch(tree, sites));

  const std::vector<int> ids0 = candidates(pars.getTopology());
  expect(algorithm + ": 14 nodes to test", ids0.size() == 14);
  const double first = pars.testNNI(ids0[0]);
  for (int id : ids0) pars.testNNI(id);
  expect(algorithm + ": one plk_pars_nni_scores call scores every node", pars.getNumberOfScoreCalls() == 1);
  expect(algorithm + ": the cached value is returned again", pars.testNNI(ids0[0]) == first);

  unsigned int score = trueScore;
  for (int k = 0; k < 3; k++) {
    const std::vector<int> ids = candidates(pars.getTopology());
    const int id = ids[(size_t)(3 + 4 * k) % ids.size()];
    const double diff = pars.testNNI(id);
    pars.doNNI(id);
    const unsigned int now = pars.getScore();
    expect(algorithm + ": perturbing interchange " + std::to_string(k) + " changes the score by its testNNI value",
           (double)now - (double)score == diff);
    score = now;
  }
  std::cout << algorithm << ": perturbed tree scores " << score << std::endl;
  expect(algorithm + ": the perturbation raised the score", score > trueScore);
  expect(algorithm + ": the perturbed score is the host recount", score == fitch(pars.getTree(), sites));

  const size_t callsBefore = pars.getNumberOfScoreCalls();
  NNITopologySearch nni(pars, algorithm, 0);
  ScoreRecorder rec(&pars);
  nni.addTopologyListener(&rec);
  nni.search();
  const std::vector<double>& acc = nni.getAcceptedImprovements();
  const unsigned int final = pars.getScore();
  std::cout << algorithm << ": " << nni.getNumberOfRounds() << " rounds, " << acc.size() << " interchanges, final score " << final
            << std::endl;
  expect(algorithm + ": interchanges were applied", !acc.empty() && rec.scores.size() == acc.size());
  expect(algorithm + ": the final score is at most the true tree's", final <= trueScore);
  expect(algorithm + ": the final score is the host recount of the final tree", final == fitch(pars.getTree(), sites));
  bool exact = true;
  unsigned int prev = score;
  for (size_t i = 0; i < acc.size() && i < rec.scores.size(); i++) {
    exact = exact && acc[i] < 0. && (double)rec.scores[i] - (double)prev == acc[i];
    prev = rec.scores[i];
  }
  expect(algorithm + ": every applied interchange lowered getScore() by exactly its testNNI value", exact);
  expect(algorithm + ": getTopologyValue() is the score", pars.getTopologyValue() == (double)final);
  expect(algorithm + ": one plk_pars_nni_scores call per round", pars.getNumberOfScoreCalls() - callsBefore == nni.getNumberOfRounds());
}

int main(int argc, char** argv) {
  try {
    golden(argc > 1 ? argv[1] : "tests/golden");
    solution();
    std::unique_ptr<TreeTemplate<Node> > tree(TreeTemplateTools::parenthesisToTree(
        "(((A:0.12,B:0.2):0.08,(C:0.1,D:0.25):0.07):0.06,((E:0.15,F:0.1):0.09,G:0.2):0.07,"
        "((H:0.18,I:0.12):0.08,J:0.22):0.1);"));
    const NucleicAlphabet* dna = &AlphabetTools::DNA_ALPHABET;
    GTR model(dna, 1, 0.2, 0.3, 0.4, 0.4, 0.1, 0.35, 0.35, 0.2);
    GammaDiscreteRateDistribution rdist(4, 0.6);
    RandomTools::setSeed(20261020);
    HomogeneousSequenceSimulator simulator(&model, &rdist, tree.get());
    std::unique_ptr<SiteContainer> sites(simulator.simulate(2000));
    search(NNITopologySearch::BETTER, *tree, *sites);
    search(NNITopologySearch::FAST, *tree, *sites);
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
