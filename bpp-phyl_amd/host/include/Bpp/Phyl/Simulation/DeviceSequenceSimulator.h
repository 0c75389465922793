// Site simulation along a tree on the MI355X: the surface of NonHomogeneousSequenceSimulator
// (Simulation/NonHomogeneousSequenceSimulator.cpp:110-160 init, 306-353 simulate, 433-483 evolve)
// over plk_simulate.  The simulator owns an engine handle for the requested number of sites
// (recreated when that number changes), uploads eigen systems, rates, root frequencies and P(t)
// the way the likelihood classes do -- a model without a usable eigen system sends its host
// P(t . r_c) through plk_set_pmatrix -- and each simulate() is one plk_simulate call followed by
// one plk_sim_get_states per output sequence.
//
// The random numbers are the engine's counter-based draws (include/plk.h), not RandomTools': a
// result depends on (seed, replicate, site, node) only.  Every simulate() uses the next replicate
// number, starting at 0; setSeed() starts a new stream at replicate 0.  Deviation from the host
// simulator: the rate class is drawn from the distribution's probabilities, which is the
// reference's uniform draw whenever the classes are equiprobable.
#ifndef BPP_AMD_DEVICESEQUENCESIMULATOR_H
#define BPP_AMD_DEVICESEQUENCESIMULATOR_H

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../Numeric/Prob/DiscreteDistribution.h"
#include "../../Seq/Container/SiteContainer.h"
#include "../Model/SubstitutionModelSet.h"
#include "../TreeTemplate.h"

struct plk_handle_s;  // include/plk.h

namespace bpp {

class DeviceSequenceSimulator {
  const SubstitutionModelSet* modelSet_;
  std::unique_ptr<SubstitutionModelSet> ownModelSet_;
  const Alphabet* alphabet_;
  const DiscreteDistribution* rate_;
  std::unique_ptr<TreeTemplate<Node> > tree_;
  std::vector<const Node*> leaves_;
  std::vector<std::string> seqNames_;
  size_t nbClasses_ = 0, nbStates_ = 0;
  bool outputInternalSequences_ = false;
  // engine layout, that of the likelihood classes: tips first, then internal nodes, each in the
  // tree's node order; one op per three sons
  std::map<const Node*, int> engineIndex_;
  int nTips_ = 0, nInternal_ = 0, rootEngine_ = -1;
  std::vector<int> opParent_, opFlags_;
  std::vector<std::vector<int> > opChildren_;
  mutable plk_handle_s* engine_ = nullptr;
  mutable size_t engineSites_ = 0;
  mutable uint64_t seed_ = 0, replicate_ = 0;

  void init();
  void check(int rc, const char* what) const;
  void ensureEngine(size_t numberOfSites) const;

 public:
  DeviceSequenceSimulator(const SubstitutionModelSet* modelSet, const DiscreteDistribution* rate, const Tree* tree);
  // homogeneous case: the model on every branch, its equilibrium frequencies at the root
  DeviceSequenceSimulator(const SubstitutionModel* model, const DiscreteDistribution* rate, const Tree* tree);
  virtual ~DeviceSequenceSimulator();
  DeviceSequenceSimulator(const DeviceSequenceSimulator&) = delete;
  DeviceSequenceSimulator& operator=(const DeviceSequenceSimulator&) = delete;

  SiteContainer* simulate(size_t numberOfSites) const;
  std::vector<std::string> getSequencesNames() const { return seqNames_; }
  const Alphabet* getAlphabet() const { return alphabet_; }
  const SubstitutionModelSet* getSubstitutionModelSet() const { return modelSet_; }
  void outputInternalSequences(bool yn);
  void setSeed(uint64_t seed) {
    seed_ = seed;
    replicate_ = 0;
  }
  uint64_t getSeed() const { return seed_; }
  // the replicate number the next simulate() will use (the calls since the last setSeed)
  uint64_t getReplicate() const { return replicate_; }
};

}  // namespace bpp

#endif
