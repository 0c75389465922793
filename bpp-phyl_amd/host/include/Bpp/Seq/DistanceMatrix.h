// A square matrix of distances with a name per row (bpp-seq DistanceMatrix subset).
#ifndef BPP_AMD_DISTANCEMATRIX_H
#define BPP_AMD_DISTANCEMATRIX_H

#include <string>
#include <vector>

#include "../Exceptions.h"

namespace bpp {

class DistanceMatrix {
  std::vector<std::string> names_;
  std::vector<double> d_;

 public:
  explicit DistanceMatrix(const std::vector<std::string>& names) : names_(names), d_(names.size() * names.size(), 0.) {}
  explicit DistanceMatrix(size_t n) : names_(n), d_(n * n, 0.) {
    for (size_t i = 0; i < n; i++) names_[i] = "Taxon " + std::to_string(i);
  }
  DistanceMatrix* clone() const { return new DistanceMatrix(*this); }

  size_t size() const { return names_.size(); }
  size_t getNumberOfRows() const { return names_.size(); }
  size_t getNumberOfColumns() const { return names_.size(); }
  void reset() { d_.assign(d_.size(), 0.); }

  const std::vector<std::string>& getNames() const { return names_; }
  const std::string& getName(size_t i) const {
    if (i >= names_.size()) throw IndexOutOfBoundsException("DistanceMatrix::getName", i, 0, names_.size());
    return names_[i];
  }
  void setName(size_t i, const std::string& name) {
    if (i >= names_.size()) throw IndexOutOfBoundsException("DistanceMatrix::setName", i, 0, names_.size());
    names_[i] = name;
  }
  void setNames(const std::vector<std::string>& names) {
    if (names.size() != names_.size()) throw Exception("DistanceMatrix::setNames: " + std::to_string(names.size()) + " names for " + std::to_string(names_.size()) + " rows");
    names_ = names;
  }
  size_t getNameIndex(const std::string& name) const {
    for (size_t i = 0; i < names_.size(); i++)
      if (names_[i] == name) return i;
    throw Exception("DistanceMatrix::getNameIndex: name not found: " + name);
  }

  double& operator()(size_t i, size_t j) { return d_[i * names_.size() + j]; }
  const double& operator()(size_t i, size_t j) const { return d_[i * names_.size() + j]; }
  double& operator()(const std::string& a, const std::string& b) { return (*this)(getNameIndex(a), getNameIndex(b)); }
  const double& operator()(const std::string& a, const std::string& b) const {
    return (*this)(getNameIndex(a), getNameIndex(b));
  }
};

}  // namespace bpp

#endif
