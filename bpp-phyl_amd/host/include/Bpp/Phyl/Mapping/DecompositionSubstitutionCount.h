// Mapping/DecompositionSubstitutionCount.h: analytic counts from the model's eigen system
// (the reference's DecompositionSubstitutionCount / DecompositionMethods).  In a substitution
// mapping on this count's own model the count matrices are formed on the device
// (plk_set_count_types + plk_update_count_matrices); the two functions below form them on the
// host, by the same formulas, for API parity:
//   W^k(t) = V (J o (V^-1 B_k V)) V^-1,  J[i][j] = t e^{max(l_i, l_j) t} phi(-|l_i - l_j| t),
//   N^k(t)[x][y] = W^k[x][y] / P(t)[x][y]   (0 where the quotient is negative or not finite).
// Real eigen systems only.
#ifndef BPP_AMD_DECOMPOSITIONSUBSTITUTIONCOUNT_H
#define BPP_AMD_DECOMPOSITIONSUBSTITUTIONCOUNT_H

#include "SubstitutionCount.h"

namespace bpp {

class DecompositionSubstitutionCount : public AbstractSubstitutionCount {
 public:
  // takes ownership of the register
  DecompositionSubstitutionCount(const SubstitutionModel* model, SubstitutionRegister* reg);
  DecompositionSubstitutionCount* clone() const override { return new DecompositionSubstitutionCount(*this); }
  double getNumberOfSubstitutions(size_t initialState, size_t finalState, double length, size_t type = 1) const override;
  RowMatrix<double>* getAllNumbersOfSubstitutions(double length, size_t type = 1) const override;
  // B_k of every type, flat [T][S][S]: (rate x) Q[x][y] where the register puts x -> y in type k + 1
  std::vector<double> getBMatrices() const;
  // W^k(length) = N^k o P, [S][S] (what plk_update_count_matrices forms on the device)
  RowMatrix<double> getCountsTimesP(double length, size_t type) const;
};

}  // namespace bpp

#endif
