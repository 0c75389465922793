// Host mirror: pairwise ML distances over libplk (one plk_pair_distances call for all pairs of
// an alignment) and the agglomerative tree builders that turn the matrix into a starting tree.
// NJ and BioNJ are host code: O(n^3) on an n x n matrix, nothing next to the likelihood work.
#include <cstdlib>
#include <cstring>
#include <limits>
#include <unordered_map>

#include "Bpp/App/ApplicationTools.h"
#include "Bpp/Phyl/Distance/BioNJ.h"
#include "Bpp/Phyl/Distance/DistanceEstimation.h"
#include "plk.h"

namespace bpp {

namespace {
// BPP_AMD_DEVICES=0,1,...: shard the patterns over these devices; else BPP_AMD_DEVICE (default 0)
std::vector<int> devicesFromEnv() {
  std::vector<int> d;
  if (const char* e = std::getenv("BPP_AMD_DEVICES")) {
    const std::string s(e);
    for (size_t i = 0; i < s.size();) {
      size_t j = s.find(',', i);
      if (j == std::string::npos) j = s.size();
      if (j > i) d.push_back(std::atoi(s.substr(i, j - i).c_str()));
      i = j + 1;
    }
  }
  return d;
}

struct Handle {
  plk_handle h = nullptr;
  ~Handle() {
    if (h) plk_destroy(h);
  }
  void check(int rc, const char* what) const {
    if (rc != PLK_OK) throw DeviceException(rc, std::string(what) + ": " + plk_last_error(h));
  }
};
}  // namespace

void DistanceEstimation::computeMatrix() {
  if (!model_) throw Exception("DistanceEstimation::computeMatrix: no model");
  if (!rateDist_) throw Exception("DistanceEstimation::computeMatrix: no rate distribution");
  if (!sites_) throw Exception("DistanceEstimation::computeMatrix: no data");
  const size_t n = sites_->getNumberOfSequences(), nSites = sites_->getNumberOfSites();
  if (n < 2) throw Exception("DistanceEstimation::computeMatrix: at least two sequences are needed");
  const Alphabet* alphabet = model_->getAlphabet();
  if (sites_->getAlphabet()->getAlphabetType() != alphabet->getAlphabetType())
    throw AlphabetMismatchException("Data and model must have the same alphabet type.");
  const size_t S = model_->getNumberOfStates(), C = rateDist_->getNumberOfCategories();
  const int nc = alphabet->getNumberOfCodes();
  // states the model does not allow (gaps among them) throw as in the likelihood classes
  for (size_t t = 0; t < n; t++)
    for (size_t i = 0; i < nSites; i++) {
      const int s = sites_->getState(t, i);
      if (s < 0 || !alphabet->isIntInAlphabet(s)) model_->getInitValue(0, s);
    }
  // the alignment's distinct columns and their weights, as the likelihood classes compress them
  std::unordered_map<std::string, size_t> seen;
  std::vector<double> weights;
  std::vector<size_t> repr;
  std::string key(n * sizeof(int), '\0');
  for (size_t i = 0; i < nSites; i++) {
    for (size_t t = 0; t < n; t++) {
      const int s = sites_->getState(t, i);
      std::memcpy(&key[t * sizeof(int)], &s, sizeof(int));
    }
    auto it = seen.find(key);
    if (it == seen.end()) {
      it = seen.emplace(key, weights.size()).first;
      weights.push_back(0.);
      repr.push_back(i);
    }
    weights[it->second] += 1.;
  }
  const size_t nPat = weights.size();
  if (nPat == 0) throw Exception("DistanceEstimation::computeMatrix: no site");
  if (verbose_ > 1) ApplicationTools::displayResult("Number of distinct sites", nPat);

  Handle e;
  const std::vector<int> devs = devicesFromEnv();
  const char* dev = std::getenv("BPP_AMD_DEVICE");
  const int rc = devs.empty() ? plk_create(dev ? std::atoi(dev) : 0, (int)S, (int)C, (int64_t)nPat, (int)n, 1, 1, 0, &e.h)
                              : plk_create_multi(devs.data(), (int)devs.size(), (int)S, (int)C, (int64_t)nPat, (int)n, 1, 1, 0, &e.h);
  if (rc != PLK_OK) throw DeviceException(rc, std::string("plk_create: ") + plk_last_error(nullptr));
  std::vector<double> table((size_t)nc * S);
  for (int c = 0; c < nc; c++)
    for (size_t s = 0; s < S; s++) table[(size_t)c * S + s] = model_->getInitValue(s, c);
  e.check(plk_set_code_table(e.h, nc, table.data()), "plk_set_code_table");
  std::vector<uint8_t> codes(nPat);
  for (size_t t = 0; t < n; t++) {
    for (size_t p = 0; p < nPat; p++) codes[p] = (uint8_t)sites_->getState(t, repr[p]);
    e.check(plk_set_tip_codes(e.h, (int)t, codes.data()), "plk_set_tip_codes");
  }
  e.check(plk_set_pattern_weights(e.h, weights.data()), "plk_set_pattern_weights");
  e.check(plk_set_category_rates(e.h, rateDist_->getCategories().data(), rateDist_->getProbabilities().data()),
          "plk_set_category_rates");
  e.check(plk_set_root_frequencies(e.h, model_->getFrequencies().data()), "plk_set_root_frequencies");
  std::vector<double> lam(S);
  for (size_t k = 0; k < S; k++) lam[k] = model_->getEigenValues()[k] * model_->getRate();
  e.check(plk_set_eigen(e.h, 0, model_->getColumnRightEigenVectors().data(), model_->getRowLeftEigenVectors().data(), lam.data()),
          "plk_set_eigen");

  std::vector<int32_t> a, b;
  for (size_t i = 0; i < n; i++)
    for (size_t j = i + 1; j < n; j++) a.push_back((int32_t)i), b.push_back((int32_t)j);
  std::vector<double> t(a.size());
  std::vector<int32_t> status(a.size());
  lnl_.assign(a.size(), 0.);
  e.check(plk_pair_distances(e.h, (int)a.size(), a.data(), b.data(), 0, nullptr, 1e-6, 10000., 1e-8, 40, t.data(), lnl_.data(),
                             nullptr, nullptr, status.data()),
          "plk_pair_distances");
  int64_t passes = 0;
  e.check(plk_pair_passes(e.h, &passes), "plk_pair_passes");
  passes_ = passes;
  dist_.reset(new DistanceMatrix(sites_->getSequencesNames()));
  for (size_t k = 0; k < a.size(); k++) {
    (*dist_)((size_t)a[k], (size_t)b[k]) = (*dist_)((size_t)b[k], (size_t)a[k]) = t[k];
    if (status[k] != 0 && verbose_ > 0)
      ApplicationTools::displayWarning("DistanceEstimation: pair (" + dist_->getName((size_t)a[k]) + ", " +
                                       dist_->getName((size_t)b[k]) + ") spent its 40 passes");
  }
}

double DistanceEstimation::getPairLogLikelihood(size_t i, size_t j) const {
  if (!dist_) throw Exception("DistanceEstimation::getPairLogLikelihood: no matrix yet");
  const size_t n = dist_->size();
  if (i == j || i >= n || j >= n) throw IndexOutOfBoundsException("DistanceEstimation::getPairLogLikelihood", i == j ? j : std::max(i, j), 0, n);
  if (i > j) std::swap(i, j);
  return lnl_[i * n - i * (i + 1) / 2 + (j - i - 1)];
}

// ---------------------------------------------------------------------------
// The joining loop
// ---------------------------------------------------------------------------
void AbstractAgglomerativeDistanceMethod::setDistanceMatrix(const DistanceMatrix& matrix) {
  matrix_ = matrix;
  tree_.reset();
}

void AbstractAgglomerativeDistanceMethod::computeTree() {
  const size_t n = matrix_.size();
  if (n < 2) throw Exception("AbstractAgglomerativeDistanceMethod::computeTree: at least two taxa are needed");
  const DistanceMatrix input(matrix_);  // the rows of matrix_ are overwritten by the joins
  auto len = [&](double l) { return positiveLengths_ && l < 0. ? 0. : l; };
  std::vector<Node*> node(n);
  for (size_t i = 0; i < n; i++) node[i] = new Node((int)i, matrix_.getName(i));
  active_.resize(n);
  for (size_t i = 0; i < n; i++) active_[i] = i;
  start();
  int id = (int)n;
  const size_t stop = rootTree_ ? 2 : 3;
  while (active_.size() > stop) {
    const std::pair<size_t, size_t> p = bestPair();
    const std::pair<double, double> bl = branchLengths(p.first, p.second);
    reduce(p.first, p.second, bl.first, bl.second);
    Node* u = new Node(id++);
    Node *si = node[active_[p.first]], *sj = node[active_[p.second]];
    si->setDistanceToFather(len(bl.first));
    sj->setDistanceToFather(len(bl.second));
    u->addSon(si);
    u->addSon(sj);
    node[active_[p.first]] = u;
    active_.erase(active_.begin() + (std::ptrdiff_t)p.second);
  }
  Node* root = new Node(id);
  if (active_.size() == 3) {
    const size_t a = active_[0], b = active_[1], c = active_[2];
    const double ab = matrix_(a, b), ac = matrix_(a, c), bc = matrix_(b, c);
    node[a]->setDistanceToFather(len(0.5 * (ab + ac - bc)));
    node[b]->setDistanceToFather(len(0.5 * (ab + bc - ac)));
    node[c]->setDistanceToFather(len(0.5 * (ac + bc - ab)));
    for (size_t k : {a, b, c}) root->addSon(node[k]);
  } else {
    const size_t a = active_[0], b = active_[1];
    node[a]->setDistanceToFather(len(0.5 * matrix_(a, b)));
    node[b]->setDistanceToFather(len(0.5 * matrix_(a, b)));
    root->addSon(node[a]);
    root->addSon(node[b]);
  }
  tree_.reset(new TreeTemplate<Node>(root));
  matrix_ = input;
}

// ---------------------------------------------------------------------------
// Neighbor joining
// ---------------------------------------------------------------------------
std::pair<size_t, size_t> NeighborJoining::bestPair() {
  const size_t r = active_.size();
  sums_.assign(matrix_.size(), 0.);
  for (size_t a : active_)
    for (size_t b : active_)
      if (a != b) sums_[a] += matrix_(a, b);
  std::pair<size_t, size_t> best(0, 1);
  double qBest = std::numeric_limits<double>::infinity();
  for (size_t i = 0; i < r; i++)
    for (size_t j = i + 1; j < r; j++) {
      const size_t a = active_[i], b = active_[j];
      const double q = (double)(r - 2) * matrix_(a, b) - sums_[a] - sums_[b];
      if (q < qBest) qBest = q, best = std::make_pair(i, j);
    }
  return best;
}

std::pair<double, double> NeighborJoining::branchLengths(size_t i, size_t j) {
  const size_t a = active_[i], b = active_[j];
  const double d = matrix_(a, b);
  const double bi = 0.5 * d + (sums_[a] - sums_[b]) / (2. * (double)(active_.size() - 2));
  return std::make_pair(bi, d - bi);
}

void NeighborJoining::reduce(size_t i, size_t j, double, double) {
  const size_t a = active_[i], b = active_[j];
  const double d = matrix_(a, b);
  for (size_t k : active_)
    if (k != a && k != b) matrix_(a, k) = matrix_(k, a) = 0.5 * (matrix_(a, k) + matrix_(b, k) - d);
}

// ---------------------------------------------------------------------------
// BIONJ
// ---------------------------------------------------------------------------
void BioNJ::start() {
  const size_t n = matrix_.size();
  variance_.resize(n * n);
  for (size_t a = 0; a < n; a++)
    for (size_t b = 0; b < n; b++) variance_[a * n + b] = matrix_(a, b);
}

void BioNJ::reduce(size_t i, size_t j, double bi, double bj) {
  const size_t n = matrix_.size(), r = active_.size();
  const size_t a = active_[i], b = active_[j];
  const double vab = variance_[a * n + b];
  double lambda = 0.5;
  if (vab != 0. && r > 2) {
    double s = 0.;
    for (size_t k : active_)
      if (k != a && k != b) s += variance_[b * n + k] - variance_[a * n + k];
    lambda = 0.5 + s / (2. * (double)(r - 2) * vab);
    lambda = lambda < 0. ? 0. : lambda > 1. ? 1. : lambda;
  }
  for (size_t k : active_)
    if (k != a && k != b) {
      matrix_(a, k) = matrix_(k, a) = lambda * (matrix_(a, k) - bi) + (1. - lambda) * (matrix_(b, k) - bj);
      variance_[a * n + k] = variance_[k * n + a] =
          lambda * variance_[a * n + k] + (1. - lambda) * variance_[b * n + k] - lambda * (1. - lambda) * vab;
    }
}

}  // namespace bpp
