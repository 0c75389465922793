// Mapping/SubstitutionCount.h: the expected number of substitutions of each type of a register
// along a branch of a given length, conditional on the states at its two ends.
#ifndef BPP_AMD_SUBSTITUTIONCOUNT_H
#define BPP_AMD_SUBSTITUTIONCOUNT_H

#include <memory>
#include <vector>

#include "SubstitutionRegister.h"

namespace bpp {

class SubstitutionCount {
 public:
  virtual ~SubstitutionCount() {}
  virtual SubstitutionCount* clone() const = 0;
  virtual bool hasSubstitutionRegister() const = 0;
  virtual const SubstitutionRegister* getSubstitutionRegister() const = 0;
  virtual void setSubstitutionRegister(SubstitutionRegister* reg) = 0;  // takes ownership
  virtual size_t getNumberOfSubstitutionTypes() const { return getSubstitutionRegister()->getNumberOfSubstitutionTypes(); }
  virtual const SubstitutionModel* getSubstitutionModel() const = 0;
  virtual void setSubstitutionModel(const SubstitutionModel* model) = 0;
  // E[count of type `type` (1..T) | start state, end state, length]
  virtual double getNumberOfSubstitutions(size_t initialState, size_t finalState, double length,
                                          size_t type = 1) const = 0;
  // the same for every pair of states, [start][end]; the caller owns the matrix
  virtual RowMatrix<double>* getAllNumbersOfSubstitutions(double length, size_t type = 1) const = 0;
  virtual std::vector<double> getNumberOfSubstitutionsForEachType(size_t initialState, size_t finalState,
                                                                  double length) const {
    std::vector<double> v(getNumberOfSubstitutionTypes());
    for (size_t k = 0; k < v.size(); k++) v[k] = getNumberOfSubstitutions(initialState, finalState, length, k + 1);
    return v;
  }
};

// register ownership and the model pointer
class AbstractSubstitutionCount : public virtual SubstitutionCount {
 protected:
  std::shared_ptr<SubstitutionRegister> register_;
  const SubstitutionModel* model_;

 public:
  AbstractSubstitutionCount(const SubstitutionModel* model, SubstitutionRegister* reg) : register_(reg), model_(model) {}
  bool hasSubstitutionRegister() const override { return register_ != nullptr; }
  const SubstitutionRegister* getSubstitutionRegister() const override { return register_.get(); }
  void setSubstitutionRegister(SubstitutionRegister* reg) override { register_.reset(reg); }
  const SubstitutionModel* getSubstitutionModel() const override { return model_; }
  void setSubstitutionModel(const SubstitutionModel* model) override { model_ = model; }
};

}  // namespace bpp

#endif
