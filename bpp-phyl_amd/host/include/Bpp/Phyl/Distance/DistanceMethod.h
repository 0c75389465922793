// Tree reconstruction from a distance matrix: the interface (Distance/DistanceMethod.h).
#ifndef BPP_AMD_DISTANCEMETHOD_H
#define BPP_AMD_DISTANCEMETHOD_H

#include <string>

#include "../../Seq/DistanceMatrix.h"
#include "../TreeTemplate.h"

namespace bpp {

class DistanceMethod {
 public:
  virtual ~DistanceMethod() {}
  virtual void setDistanceMatrix(const DistanceMatrix& matrix) = 0;
  virtual void computeTree() = 0;
  virtual Tree* getTree() const = 0;
  virtual std::string getName() const = 0;
  virtual void setVerbose(bool yn) = 0;
  virtual bool isVerbose() const = 0;
};

class AgglomerativeDistanceMethod : public DistanceMethod {};

}  // namespace bpp

#endif
