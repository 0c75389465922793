// Host mirror: DeviceSequenceSimulator (see the header) over plk_simulate.
#include "Bpp/Phyl/Simulation/DeviceSequenceSimulator.h"

#include <cstdlib>

#include "Bpp/Exceptions.h"
#include "Bpp/Phyl/Model/SubstitutionModelSet.h"
#include "Bpp/Phyl/Model/SubstitutionModelSetTools.h"
#include "Bpp/Seq/Container/VectorSiteContainer.h"
#include "plk.h"

namespace bpp {

namespace {
int deviceFromEnv() {
  const char* e = std::getenv("BPP_AMD_DEVICE");
  return e ? std::atoi(e) : 0;
}
}  // namespace

DeviceSequenceSimulator::DeviceSequenceSimulator(const SubstitutionModelSet* modelSet, const DiscreteDistribution* rate,
                                                 const Tree* tree)
    : modelSet_(modelSet), alphabet_(modelSet ? modelSet->getAlphabet() : nullptr), rate_(rate) {
  if (!modelSet || !rate || !tree) throw NullPointerException("DeviceSequenceSimulator: null argument");
  const TreeTemplate<Node>* tt = dynamic_cast<const TreeTemplate<Node>*>(tree);
  if (!tt) throw Exception("DeviceSequenceSimulator: unsupported tree implementation");
  if (!modelSet->isFullySetUpFor(*tree))
    throw Exception("DeviceSequenceSimulator(constructor). Model set is not fully specified.");
  tree_.reset(new TreeTemplate<Node>(*tt));
  init();
}

DeviceSequenceSimulator::DeviceSequenceSimulator(const SubstitutionModel* model, const DiscreteDistribution* rate,
                                                 const Tree* tree)
    : modelSet_(nullptr), alphabet_(model ? model->getAlphabet() : nullptr), rate_(rate) {
  if (!model || !rate || !tree) throw NullPointerException("DeviceSequenceSimulator: null argument");
  const TreeTemplate<Node>* tt = dynamic_cast<const TreeTemplate<Node>*>(tree);
  if (!tt) throw Exception("DeviceSequenceSimulator: unsupported tree implementation");
  FixedFrequencySet* f = new FixedFrequencySet(model->getAlphabet(), model->getFrequencies());
  f->setNamespace("anc.");
  ownModelSet_.reset(SubstitutionModelSetTools::createHomogeneousModelSet(model->clone(), f, tt));
  modelSet_ = ownModelSet_.get();
  tree_.reset(new TreeTemplate<Node>(*tt));
  init();
}

DeviceSequenceSimulator::~DeviceSequenceSimulator() {
  if (engine_) plk_destroy(engine_);
}

void DeviceSequenceSimulator::check(int rc, const char* what) const {
  if (rc != PLK_OK) throw DeviceException(rc, std::string(what) + ": " + plk_last_error(engine_));
}

void DeviceSequenceSimulator::init() {
  nbClasses_ = rate_->getNumberOfCategories();
  nbStates_ = modelSet_->getNumberOfStates();
  const std::vector<Node*> all = tree_->getNodes();
  leaves_.clear();
  engineIndex_.clear();
  nTips_ = nInternal_ = 0;
  for (const Node* n : all)
    if (n->isLeaf()) {
      leaves_.push_back(n);
      engineIndex_[n] = nTips_++;
    }
  for (const Node* n : all)
    if (!n->isLeaf()) engineIndex_[n] = nTips_ + nInternal_++;
  if (nInternal_ < 1) throw Exception("DeviceSequenceSimulator: the tree has no internal node");
  rootEngine_ = engineIndex_[tree_->getRootNode()];
  opParent_.clear();
  opChildren_.clear();
  opFlags_.clear();
  for (const Node* n : all) {  // postorder: the root's ops come last
    if (n->isLeaf()) continue;
    for (size_t k = 0; k < n->getNumberOfSons(); k += 3) {
      std::vector<int> ch;
      for (size_t j = k; j < std::min(k + 3, n->getNumberOfSons()); j++) ch.push_back(engineIndex_[n->getSon(j)]);
      opParent_.push_back(engineIndex_[n]);
      opChildren_.push_back(ch);
      opFlags_.push_back(k == 0 ? 0 : PLK_OP_ACCUMULATE);
    }
  }
  outputInternalSequences(outputInternalSequences_);
}

void DeviceSequenceSimulator::outputInternalSequences(bool yn) {
  outputInternalSequences_ = yn;
  seqNames_.clear();
  if (yn) {
    for (const Node* n : tree_->getNodes())
      seqNames_.push_back(n->isLeaf() ? n->getName() : std::to_string(n->getId()));
  } else {
    for (const Node* n : leaves_) seqNames_.push_back(n->getName());
  }
}

// A handle for this number of sites with the models, the rates, the root frequencies and every
// branch's P(t): eigen systems go to the device (AbstractPlkTreeLikelihood::uploadEigen), a model
// whose eigen system failed its check sends host P(t . r_c) (its updatePmatrices).
void DeviceSequenceSimulator::ensureEngine(size_t numberOfSites) const {
  if (engine_ && engineSites_ == numberOfSites) return;
  if (engine_) {
    plk_destroy(engine_);
    engine_ = nullptr;
  }
  const size_t S = nbStates_, C = nbClasses_, nModels = modelSet_->getNumberOfModels();
  plk_handle h = nullptr;
  const int rc = plk_create(deviceFromEnv(), (int)S, (int)C, (int64_t)numberOfSites, nTips_, nInternal_, (int)nModels, 0u, &h);
  if (rc != PLK_OK) throw DeviceException(rc, std::string("plk_create: ") + plk_last_error(nullptr));
  engine_ = h;
  engineSites_ = numberOfSites;
  const Vdouble& rates = rate_->getCategories();
  check(plk_set_category_rates(engine_, rates.data(), rate_->getProbabilities().data()), "plk_set_category_rates");
  const Vdouble pi = modelSet_->getRootFrequencies();
  check(plk_set_root_frequencies(engine_, pi.data()), "plk_set_root_frequencies");
  for (size_t m = 0; m < nModels; m++) {
    const SubstitutionModel& model = *modelSet_->getModel(m);
    if (model.needsHostPij()) continue;
    std::vector<double> lam(S);
    for (size_t k = 0; k < S; k++) lam[k] = model.getEigenValues()[k] * model.getRate();
    check(plk_set_eigen(engine_, (int)m, model.getColumnRightEigenVectors().data(),
                        model.getRowLeftEigenVectors().data(), lam.data()),
          "plk_set_eigen");
  }
  std::vector<int32_t> br, mod;
  std::vector<double> t, P(C * S * S);
  for (const Node* n : tree_->getNodes()) {
    if (n == tree_->getRootNode()) continue;
    const size_t m = modelSet_->getModelIndexForNode(n->getId());
    const SubstitutionModel* model = modelSet_->getModel(m);
    const double d = n->getDistanceToFather();
    if (model->needsHostPij()) {
      for (size_t c = 0; c < C; c++) {
        const RowMatrix<double>& Pc = model->getPij_t(d * rates[c]);
        std::copy(Pc.data(), Pc.data() + S * S, P.begin() + c * S * S);
      }
      check(plk_set_pmatrix(engine_, engineIndex_.at(n), P.data()), "plk_set_pmatrix");
    } else {
      br.push_back(engineIndex_.at(n));
      mod.push_back((int32_t)m);
      t.push_back(d);
    }
  }
  if (!br.empty())
    check(plk_update_pmatrices(engine_, (int)br.size(), br.data(), mod.data(), t.data(), PLK_DERIV_P),
          "plk_update_pmatrices");
}

SiteContainer* DeviceSequenceSimulator::simulate(size_t numberOfSites) const {
  if (numberOfSites == 0) throw Exception("DeviceSequenceSimulator::simulate: no site requested");
  ensureEngine(numberOfSites);
  std::vector<plk_op> ops(opParent_.size());
  for (size_t i = 0; i < ops.size(); i++) {
    ops[i].parent = opParent_[i];
    ops[i].n_children = (int32_t)opChildren_[i].size();
    for (int k = 0; k < 3; k++) ops[i].child[k] = k < ops[i].n_children ? opChildren_[i][(size_t)k] : 0;
    ops[i].flags = opFlags_[i];
  }
  check(plk_simulate(engine_, ops.data(), (int)ops.size(), rootEngine_, seed_, replicate_, 0, nullptr, 0u), "plk_simulate");
  replicate_++;
  std::vector<const Node*> out;
  if (outputInternalSequences_) {
    for (const Node* n : tree_->getNodes()) out.push_back(n);
  } else {
    out = leaves_;
  }
  std::unique_ptr<VectorSiteContainer> sites(new VectorSiteContainer(alphabet_));
  std::vector<uint8_t> s(numberOfSites);
  for (size_t i = 0; i < out.size(); i++) {
    check(plk_sim_get_states(engine_, engineIndex_.at(out[i]), s.data()), "plk_sim_get_states");
    std::vector<int> content(s.begin(), s.end());
    sites->addSequence(BasicSequence(seqNames_[i], content, alphabet_));
  }
  return sites.release();
}

}  // namespace bpp
