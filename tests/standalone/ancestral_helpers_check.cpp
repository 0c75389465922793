// Stand-alone check of the mirror's host-only ancestral helpers (namespace bpp::ancestral and
// VectorTools::whichMax): argmax with ties, one-hot leaves, sampling, pattern -> site
// expansion.  Header-only code, no engine and no library: tests/test_posteriors_cpu.py builds
// this once plainly and once with -fsanitize=address,undefined and runs both.
#include <Bpp/Numeric/Random/RandomTools.h>
#include <Bpp/Phyl/Likelihood/AncestralStateReconstruction.h>

#include <cstdio>
#include <vector>

using namespace bpp;

static int failures = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAIL line %d: %s\n", __LINE__, #c);       \
      failures++;                                            \
    }                                                        \
  } while (0)

int main() {
  typedef std::vector<double> V;
  // whichMax: the first of the largest entries
  CHECK(VectorTools::whichMax(V{0.1, 0.4, 0.4, 0.1}) == 1);
  CHECK(VectorTools::whichMax(V{0.25, 0.25, 0.25, 0.25}) == 0);
  CHECK(VectorTools::whichMax(V{0., 0., 0., 1.}) == 3);
  CHECK(VectorTools::whichMax(V{0.7}) == 0);
  CHECK(VectorTools::whichMax(V{}) == 0);
  // one-hot leaves: an unambiguous state, an ambiguity code (several 1s), a gap (all 1s)
  V probs;
  CHECK(ancestral::oneHot(V{0., 0., 1., 0.}, probs) == 2 && probs == (V{0., 0., 1., 0.}));
  CHECK(ancestral::oneHot(V{0., 1., 0., 1.}, probs) == 1 && probs == (V{0., 1., 0., 0.}));
  CHECK(ancestral::oneHot(V{1., 1., 1., 1.}, probs) == 0 && probs == (V{1., 0., 0., 0.}));
  CHECK(ancestral::oneHot(V{}, probs) == 0 && probs.empty());
  // sampling: thresholds, zero-probability states never drawn, totals short of r
  const V p{0.2, 0., 0.5, 0.3};
  CHECK(ancestral::sampleState(p, 0.0) == 0);
  CHECK(ancestral::sampleState(p, 0.2) == 0);
  CHECK(ancestral::sampleState(p, 0.2000001) == 2);
  CHECK(ancestral::sampleState(p, 0.7) == 2);
  CHECK(ancestral::sampleState(p, 0.99) == 3);
  CHECK(ancestral::sampleState(V{0.5, 0.4999999999999999, 0.}, 0.9999999999999999) == 1);  // never state 2
  CHECK(ancestral::sampleState(V{0., 0., 0.}, 0.5) == 0);                                   // an underflowed pattern
  RandomTools::setSeed(11);
  size_t count[4] = {0, 0, 0, 0};
  for (int i = 0; i < 20000; i++) count[ancestral::sampleState(p, RandomTools::giveRandomNumberBetweenZeroAndEntry(1.))]++;
  CHECK(count[1] == 0);
  CHECK(count[0] > 3600 && count[0] < 4400 && count[2] > 9500 && count[2] < 10500 && count[3] > 5500 && count[3] < 6500);
  // pattern -> site expansion
  const std::vector<size_t> links{0, 1, 0, 2, 1, 0};
  const std::vector<size_t> st = ancestral::expandPatterns(std::vector<size_t>{3, 1, 2}, links);
  CHECK((st == std::vector<size_t>{3, 1, 3, 2, 1, 3}));
  const std::vector<V> pr = ancestral::expandPatterns(std::vector<V>{V{1., 0.}, V{0.5, 0.5}, V{0., 1.}}, links);
  CHECK(pr.size() == 6 && pr[3] == (V{0., 1.}) && pr[4] == (V{0.5, 0.5}) && pr[5] == (V{1., 0.}));
  CHECK(ancestral::expandPatterns(std::vector<size_t>{}, std::vector<size_t>{}).empty());
  bool threw = false;
  try {
    ancestral::expandPatterns(std::vector<size_t>{1}, std::vector<size_t>{0, 1});  // a link past the patterns
  } catch (const std::out_of_range&) {
    threw = true;
  }
  CHECK(threw);
  if (failures) return 1;
  std::printf("PASSED\n");
  return 0;
}
