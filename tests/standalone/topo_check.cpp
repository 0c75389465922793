// Stand-alone check of csrc/plk_topo.hpp (host only, no HIP): the tree view and the KOp lists
// of the path, root-pair and preorder passes against arrays written out by hand from the
// loops these builders replaced.  Lists are compared with memcmp over whole records, so the
// zeroed tail of a short op, the order of the ops and their grouping into launches all count.
#include <cstdio>
#include <cstring>
#include <vector>

#include "plk_topo.hpp"

using namespace plk;

static int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static const int ACC = PLK_OP_ACCUMULATE, SG = kOpSigned;

static bool same_ops(const std::vector<KOp>& got, const std::vector<KOp>& want) {
  if (got.size() != want.size()) {
    std::printf("  %zu ops, expected %zu\n", got.size(), want.size());
    return false;
  }
  for (size_t i = 0; i < got.size(); ++i)
    if (std::memcmp(&got[i], &want[i], sizeof(KOp)) != 0) {
      const KOp &g = got[i], &w = want[i];
      std::printf("  op %zu: parent %d n %d child %d %d %d branch %d %d %d tip %d %d %d flags %d\n", i, g.parent, g.n,
                  g.child[0], g.child[1], g.child[2], g.branch[0], g.branch[1], g.branch[2], g.is_tip[0], g.is_tip[1],
                  g.is_tip[2], g.flags);
      std::printf("  expected parent %d n %d child %d %d %d branch %d %d %d tip %d %d %d flags %d\n", w.parent, w.n,
                  w.child[0], w.child[1], w.child[2], w.branch[0], w.branch[1], w.branch[2], w.is_tip[0], w.is_tip[1],
                  w.is_tip[2], w.flags);
      return false;
    }
  return true;
}

static bool same_launches(const std::vector<OpLaunch>& got, const std::vector<OpLaunch>& want) {
  if (got.size() != want.size()) return false;
  for (size_t i = 0; i < got.size(); ++i)
    if (got[i].first != want[i].first || got[i].count != want[i].count) return false;
  return true;
}

// (a) ((a,b),c) in a handle of 4 tips and 3 internal nodes: 4 = (0,1), 5 = (4,2) the root;
// node 6 still lists tip 3 from an earlier tree and hangs nowhere.
static void check_view() {
  std::vector<std::vector<int> > kids(7);
  kids[4] = {0, 1};
  kids[5] = {4, 2};
  kids[6] = {3};
  const TopoView from_root(kids, 5), from_branch(kids, 0), from_son(kids, 2), stale(kids, 3);
  CHECK((from_root.parent == std::vector<int>{4, 4, 5, 6, 5, -1, -1}));
  CHECK(from_branch.parent == from_root.parent);
  CHECK(&from_root.kids == &kids);  // read in place, no copy
  CHECK(from_root.root == 5);
  CHECK(from_branch.root == 5);
  CHECK(from_son.root == 5);
  CHECK(stale.root == 6);           // climbing from the stale side ends at its own top
  CHECK(TopoView(kids, 6).root == 6);
  CHECK((from_root.in_tree() == std::vector<char>{1, 1, 1, 0, 1, 1, 0}));
  CHECK((from_root.levels() == std::vector<std::vector<int> >{{5}, {4, 2}, {0, 1}}));
  CHECK((from_root.path_sons(0) == std::vector<int>{0, 1, 4, 2}));
  CHECK((from_root.path_sons(4) == std::vector<int>{4, 2}));
  CHECK(from_root.path_sons(5).empty());
}

// (b) 1, 3, 4 and 5 factors into slot 7: 1, 1, 2 and 2 ops
static void check_product_ops() {
  std::vector<OpKid> k;
  for (int i = 0; i < 5; ++i) k.push_back(OpKid{i & 1, 10 + i, 20 + i});
  auto first = [&](int n) { return std::vector<OpKid>(k.begin(), k.begin() + n); };
  std::vector<KOp> ops;
  CHECK(append_product_ops(ops, 7, first(1), 0) == 1);
  CHECK(same_ops(ops, {KOp{7, 1, {10, 0, 0}, {20, 0, 0}, {0, 0, 0}, 0}}));
  ops.clear();
  CHECK(append_product_ops(ops, 7, first(3), 0) == 1);
  CHECK(same_ops(ops, {KOp{7, 3, {10, 11, 12}, {20, 21, 22}, {0, 1, 0}, 0}}));
  ops.clear();
  CHECK(append_product_ops(ops, 7, first(4), SG) == 2);
  CHECK(same_ops(ops, {KOp{7, 3, {10, 11, 12}, {20, 21, 22}, {0, 1, 0}, SG},
                       KOp{7, 1, {13, 0, 0}, {23, 0, 0}, {1, 0, 0}, ACC | SG}}));
  // appended behind what is there
  CHECK(append_product_ops(ops, 8, first(5), 0) == 2);
  CHECK(same_ops(ops, {KOp{7, 3, {10, 11, 12}, {20, 21, 22}, {0, 1, 0}, SG},
                       KOp{7, 1, {13, 0, 0}, {23, 0, 0}, {1, 0, 0}, ACC | SG},
                       KOp{8, 3, {10, 11, 12}, {20, 21, 22}, {0, 1, 0}, 0},
                       KOp{8, 2, {13, 14, 0}, {23, 24, 0}, {1, 0, 0}, ACC}}));
  ops.clear();
  CHECK(append_product_ops(ops, 7, first(0), 0) == 0);
  CHECK(ops.empty());
}

// The tree of (c), (d) and (e): 5 tips, the cherry 5 = (3,4) and the root 6 = (0,1,5,2).
// As in a handle of these sizes: scratch matrices from 7 (= nodes), scratch tip rows from 5
// (= tips), scratch slots from 2 (= internal nodes).
static std::vector<std::vector<int> > four_son_tree() {
  std::vector<std::vector<int> > kids(7);
  kids[5] = {3, 4};
  kids[6] = {0, 1, 5, 2};
  return kids;
}

// (c) path ops
static void check_path_ops() {
  const std::vector<std::vector<int> > kids = four_son_tree();
  const int tip_row[2] = {5, 6}, mat[2] = {7, 8};
  {  // tip branch 3 at depth 2: two steps, the passes ping-pong 2 -> 3 and 4 -> 5
    const TopoView t(kids, 3);
    CHECK(t.root == 6);
    std::vector<KOp> flat;
    std::vector<OpLaunch> launches;
    CHECK(path_ops(t, 3, 5, tip_row, mat, 2, flat, launches) == 2);
    CHECK(same_ops(flat, {KOp{2, 2, {5, 4, 0}, {7, 4, 0}, {1, 1, 0}, SG},          // step 0, dP: scratch row 5, matrix 7
                          KOp{4, 2, {6, 4, 0}, {8, 4, 0}, {1, 1, 0}, SG},          // step 0, d2P: scratch row 6, matrix 8
                          KOp{3, 3, {0, 1, 2}, {0, 1, 5}, {1, 1, 0}, SG},          // step 1, chunk 0: reads slot 2
                          KOp{5, 3, {0, 1, 4}, {0, 1, 5}, {1, 1, 0}, SG},          //                  reads slot 4
                          KOp{3, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC | SG},    // step 1, chunk 1
                          KOp{5, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC | SG}}));
    CHECK(same_launches(launches, {{0, 2}, {2, 2}, {4, 2}}));
  }
  {  // internal branch 5 at depth 1: one step, its own slot with the scratch matrix
    const TopoView t(kids, 5);
    std::vector<KOp> flat;
    std::vector<OpLaunch> launches;
    CHECK(path_ops(t, 5, 5, tip_row, mat, 2, flat, launches) == 1);
    CHECK(same_ops(flat, {KOp{2, 3, {0, 1, 0}, {0, 1, 7}, {1, 1, 0}, SG},
                          KOp{4, 3, {0, 1, 0}, {0, 1, 8}, {1, 1, 0}, SG},
                          KOp{2, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC | SG},
                          KOp{4, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC | SG}}));
    CHECK(same_launches(launches, {{0, 2}, {2, 2}}));
  }
}

// (d) root-pair ops with a = tip 1 and b = internal node 5: ten ops, chunk-major
static void check_root_pair_ops() {
  const std::vector<std::vector<int> > kids = four_son_tree();
  const TopoView t(kids, 1);
  CHECK(t.parent[1] == 6 && t.parent[5] == 6 && t.parent[6] < 0);
  std::vector<KOp> flat;
  std::vector<OpLaunch> launches;
  root_pair_ops(t, 6, 1, 5, 5, 7, 2, flat, launches);
  CHECK(same_ops(flat, {KOp{2, 3, {0, 5, 0}, {0, 7, 5}, {1, 1, 0}, SG},    // dP_a: row 5, matrix 7
                        KOp{3, 3, {0, 1, 0}, {0, 1, 9}, {1, 1, 0}, SG},    // dP_b: matrix 9
                        KOp{4, 3, {0, 6, 0}, {0, 8, 5}, {1, 1, 0}, SG},    // d2P_a: row 6, matrix 8
                        KOp{5, 3, {0, 1, 0}, {0, 1, 10}, {1, 1, 0}, SG},   // d2P_b: matrix 10
                        KOp{6, 3, {0, 5, 0}, {0, 7, 9}, {1, 1, 0}, SG},    // dP_a and dP_b
                        KOp{2, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC | SG},
                        KOp{3, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC | SG},
                        KOp{4, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC | SG},
                        KOp{5, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC | SG},
                        KOp{6, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC | SG}}));
  CHECK(same_launches(launches, {{0, 5}, {5, 5}}));
}

// (e) upper ops, U slots from 10 (slot 10 + v), M_f in matrix 20 + f
static void check_upper_ops() {
  {
    const std::vector<std::vector<int> > kids = four_son_tree();
    const TopoView t(kids, 6);
    CHECK((t.levels() == std::vector<std::vector<int> >{{6}, {0, 1, 5, 2}, {3, 4}}));
    std::vector<KOp> flat;
    std::vector<OpLaunch> launches;
    upper_ops(t, {0}, 5, 10, 20, flat, launches);     // a tip under the root: no U_f term
    upper_ops(t, {3, 4}, 5, 10, 20, flat, launches);  // the next level behind it: U_f first
    CHECK(same_ops(flat, {KOp{10, 3, {1, 0, 2}, {1, 5, 2}, {1, 0, 1}, 0},
                          KOp{13, 2, {15, 4, 0}, {25, 4, 0}, {0, 1, 0}, 0},
                          KOp{14, 2, {15, 3, 0}, {25, 3, 0}, {0, 1, 0}, 0}}));
    CHECK(same_launches(launches, {{0, 1}, {1, 2}}));
    upper_ops(t, {}, 5, 10, 20, flat, launches);      // an empty level launches nothing
    CHECK(flat.size() == 3 && launches.size() == 2);
  }
  {
    // 6 tips; 6 = (3,4), 7 = (0,1,2,6) a father of four sons below the root 8 = (7,5)
    std::vector<std::vector<int> > kids(9);
    kids[6] = {3, 4};
    kids[7] = {0, 1, 2, 6};
    kids[8] = {7, 5};
    const TopoView t(kids, 8);
    std::vector<KOp> flat;
    std::vector<OpLaunch> launches;
    upper_ops(t, {0, 1, 2, 6}, 6, 10, 20, flat, launches);
    CHECK(same_ops(flat, {KOp{10, 3, {17, 1, 2}, {27, 1, 2}, {0, 1, 1}, 0},   // chunk 0 of the four sons
                          KOp{11, 3, {17, 0, 2}, {27, 0, 2}, {0, 1, 1}, 0},
                          KOp{12, 3, {17, 0, 1}, {27, 0, 1}, {0, 1, 1}, 0},
                          KOp{16, 3, {17, 0, 1}, {27, 0, 1}, {0, 1, 1}, 0},
                          KOp{10, 1, {0, 0, 0}, {6, 0, 0}, {0, 0, 0}, ACC},   // chunk 1: the second launch
                          KOp{11, 1, {0, 0, 0}, {6, 0, 0}, {0, 0, 0}, ACC},
                          KOp{12, 1, {0, 0, 0}, {6, 0, 0}, {0, 0, 0}, ACC},
                          KOp{16, 1, {2, 0, 0}, {2, 0, 0}, {1, 0, 0}, ACC}}));
    CHECK(same_launches(launches, {{0, 4}, {4, 4}}));
    // nodes with one and with two chunks: the second launch holds only the longer one's
    flat.clear();
    launches.clear();
    upper_ops(t, {5, 0}, 6, 10, 20, flat, launches);
    CHECK(same_ops(flat, {KOp{15, 1, {1, 0, 0}, {7, 0, 0}, {0, 0, 0}, 0},
                          KOp{10, 3, {17, 1, 2}, {27, 1, 2}, {0, 1, 1}, 0},
                          KOp{10, 1, {0, 0, 0}, {6, 0, 0}, {0, 0, 0}, ACC}}));
    CHECK(same_launches(launches, {{0, 2}, {2, 1}}));
  }
}

int main() {
  static_assert(sizeof(KOp) == 12 * sizeof(int32_t), "KOp has no padding: memcmp compares fields only");
  check_view();
  check_product_ops();
  check_path_ops();
  check_root_pair_ops();
  check_upper_ops();
  if (failures) {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("PASSED\n");
  return 0;
}
