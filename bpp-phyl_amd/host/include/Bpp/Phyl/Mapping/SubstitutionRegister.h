// Mapping/SubstitutionRegister.h: which substitution type a change x -> y belongs to.  Types
// are numbered from 1; 0 means "not counted" (the reference's convention).  The two registers
// the engine's tests and tools use: every change in one type, and one type per ordered pair.
#ifndef BPP_AMD_SUBSTITUTIONREGISTER_H
#define BPP_AMD_SUBSTITUTIONREGISTER_H

#include <string>

#include "../Model/SubstitutionModel.h"

namespace bpp {

class SubstitutionRegister {
 public:
  virtual ~SubstitutionRegister() {}
  virtual SubstitutionRegister* clone() const = 0;
  virtual const Alphabet* getAlphabet() const = 0;
  virtual const SubstitutionModel* getSubstitutionModel() const = 0;
  virtual size_t getNumberOfSubstitutionTypes() const = 0;
  virtual const std::string& getName() const = 0;
  // 0 if the change is not counted (x == y included), else the type in 1..T
  virtual size_t getType(size_t fromState, size_t toState) const = 0;
  virtual std::string getTypeName(size_t type) const = 0;
};

class AbstractSubstitutionRegister : public virtual SubstitutionRegister {
 protected:
  const SubstitutionModel* model_;
  std::string name_;

 public:
  AbstractSubstitutionRegister(const SubstitutionModel* model, const std::string& name) : model_(model), name_(name) {}
  const SubstitutionModel* getSubstitutionModel() const override { return model_; }
  const Alphabet* getAlphabet() const override { return model_->getAlphabet(); }
  const std::string& getName() const override { return name_; }
};

// every change x != y is of type 1
class TotalSubstitutionRegister : public AbstractSubstitutionRegister {
 public:
  explicit TotalSubstitutionRegister(const SubstitutionModel* model) : AbstractSubstitutionRegister(model, "Total") {}
  TotalSubstitutionRegister* clone() const override { return new TotalSubstitutionRegister(*this); }
  size_t getNumberOfSubstitutionTypes() const override { return 1; }
  size_t getType(size_t fromState, size_t toState) const override { return fromState == toState ? 0 : 1; }
  std::string getTypeName(size_t type) const override;
};

// one type per ordered pair x != y, numbered row by row: S (S - 1) types
class ComprehensiveSubstitutionRegister : public AbstractSubstitutionRegister {
 public:
  explicit ComprehensiveSubstitutionRegister(const SubstitutionModel* model)
      : AbstractSubstitutionRegister(model, "Comprehensive") {}
  ComprehensiveSubstitutionRegister* clone() const override { return new ComprehensiveSubstitutionRegister(*this); }
  size_t getNumberOfSubstitutionTypes() const override {
    const size_t s = model_->getNumberOfStates();
    return s * (s - 1);
  }
  size_t getType(size_t fromState, size_t toState) const override {
    if (fromState == toState) return 0;
    const size_t s = model_->getNumberOfStates();
    return fromState * (s - 1) + (toState < fromState ? toState : toState - 1) + 1;
  }
  std::string getTypeName(size_t type) const override;
};

}  // namespace bpp

#endif
