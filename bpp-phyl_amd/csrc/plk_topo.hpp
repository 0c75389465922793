// plk_topo.hpp -- host-only: the tree the handle has merged from its op lists, seen from one
// start node, and the KOp lists of the derivative and preorder passes built from it.  No HIP
// in here: tests/standalone/topo_check.cpp compiles it with the host compiler and pins every
// list below, op for op.  The order of the ops in a flat list and their grouping into
// launches are behaviour (a launch runs its ops side by side; an ACCUMULATE op needs the
// launch before it), and this file owns both.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/plk.h"

namespace plk {

// Device-side description of one partial update (children already resolved
// into tip indices or internal slots).
struct KOp {
  int32_t parent;    // internal slot
  int32_t n;         // number of children (1..3)
  int32_t child[3];  // tip index (is_tip) or internal slot
  int32_t branch[3]; // node index of the child = transition-matrix index
  int32_t is_tip[3];
  int32_t flags;     // PLK_OP_ACCUMULATE | kOpSigned
};
// Internal op flag: the vector being formed may have either sign (dP / d2P substituted on a
// branch: the path and root-pair derivative vectors), so the rescale decision takes the largest
// magnitude.  By the largest value a vector whose entries are all negative is never rescaled --
// and a path vector stays all negative from there to the root (P and the siblings' products are
// positive) until it leaves the double range.  Likelihood vectors keep the largest value: the
// decision the oracle restates.
constexpr int kOpSigned = 2;

// The merged tree of every traversal so far (an incremental call lists only the ancestors of
// the changed branches), read in place from the handle's topo_kids.  A node that an earlier
// tree left behind keeps its sons' list, so parent[] takes the last writer in node order and
// in_tree() tells which nodes hang below the root.  The root is where climbing from `start`
// ends: start at the last op's parent for the current traversal's root, at a branch for the
// root above that branch (the branch itself when nothing lists it as a son).
struct TopoView {
  const std::vector<std::vector<int> >& kids;
  std::vector<int> parent;
  int root;

  TopoView(const std::vector<std::vector<int> >& topo_kids, int start) : kids(topo_kids), parent(topo_kids.size(), -1) {
    for (size_t n = 0; n < kids.size(); ++n)
      for (int c : kids[n]) parent[c] = (int)n;
    root = start;
    while (parent[root] >= 0) root = parent[root];
  }

  std::vector<char> in_tree() const {
    std::vector<char> in(kids.size(), 0);
    std::vector<int> st(1, root);
    while (!st.empty()) {
      const int n = st.back();
      st.pop_back();
      in[n] = 1;
      for (int c : kids[n]) st.push_back(c);
    }
    return in;
  }

  // every son of every node from the father of `branch` up to the root: what a pass along
  // that path reads
  std::vector<int> path_sons(int branch) const {
    std::vector<int> sons;
    for (int n = parent[branch]; n >= 0; n = parent[n]) sons.insert(sons.end(), kids[n].begin(), kids[n].end());
    return sons;
  }

  // preorder levels: depth 0 = the root, depth 1 = its sons, ... (sons in list order)
  std::vector<std::vector<int> > levels() const {
    std::vector<std::vector<int> > depth(1, std::vector<int>(1, root));
    while (true) {
      std::vector<int> next;
      for (int n : depth.back())
        for (int c : kids[n]) next.push_back(c);
      if (next.empty()) break;
      depth.push_back(next);
    }
    return depth;
  }
};

// One factor of a product op, as KOp stores it.
struct OpKid {
  int32_t is_tip, child, branch;
};
// node c with its own P: a tip's row or an internal node's slot
inline OpKid own_kid(int c, int nt) { return OpKid{c < nt, c < nt ? c : c - nt, c}; }

// The product ops of one output slot: at most three factors per op, the second op on
// accumulates into what the first wrote.  Returns the number of ops appended.
inline int append_product_ops(std::vector<KOp>& ops, int out, const std::vector<OpKid>& kids, int flags) {
  int n_chunks = 0;
  for (size_t k0 = 0; k0 < kids.size(); k0 += 3, ++n_chunks) {
    KOp op;
    std::memset(&op, 0, sizeof(op));
    op.parent = out;
    op.flags = (k0 == 0 ? 0 : PLK_OP_ACCUMULATE) | flags;
    for (size_t k = k0; k < kids.size() && k < k0 + 3; ++k) {
      const int j = op.n++;
      op.is_tip[j] = kids[k].is_tip;
      op.child[j] = kids[k].child;
      op.branch[j] = kids[k].branch;
    }
    ops.push_back(op);
  }
  return n_chunks;
}

// `count` ops of the flat list from `first` on, run in one launch
struct OpLaunch {
  size_t first;
  int count;
};

// Chunk-major merge of the op lists of several outputs: op j of every list that has one, lists
// in order, makes one launch.
inline void append_chunk_major(const std::vector<std::vector<KOp> >& per_out, std::vector<KOp>& flat,
                               std::vector<OpLaunch>& launches) {
  for (size_t j = 0;; ++j) {
    const size_t first = flat.size();
    for (const std::vector<KOp>& l : per_out)
      if (j < l.size()) flat.push_back(l[j]);
    if (flat.size() == first) return;
    launches.push_back(OpLaunch{first, (int)(flat.size() - first)});
  }
}

// Path ops of a branch: the traversal from the branch's father to the root with the branch's
// P replaced by scratch matrix mat[x] (for a tip branch: scratch tip row tip_row[x]) in pass
// x = 0, 1, every other son read from its own partial.  The path vector of pass x ping-pongs
// between the slots slot0 + 2x and slot0 + 2x + 1.  One launch per (path node, chunk) holds the
// two passes side by side.  Returns the number of path nodes; the last one wrote slot
// slot0 + 2x + ((steps - 1) & 1).
inline int path_ops(const TopoView& t, int branch, int nt, const int tip_row[2], const int mat[2], int slot0,
                    std::vector<KOp>& flat, std::vector<OpLaunch>& launches) {
  int path = branch, cur = 0;
  for (int n = t.parent[branch]; n >= 0; path = n, n = t.parent[n], ++cur) {
    std::vector<std::vector<KOp> > pass(2);
    for (int x = 0; x < 2; ++x) {
      const int out = slot0 + 2 * x + (cur & 1), in = slot0 + 2 * x + ((cur + 1) & 1);
      std::vector<OpKid> ks;
      for (int c : t.kids[n])
        if (c != path)
          ks.push_back(own_kid(c, nt));
        else if (path == branch)  // the differentiated branch
          ks.push_back(OpKid{c < nt, c < nt ? tip_row[x] : c - nt, mat[x]});
        else                      // the path vector from the step below
          ks.push_back(OpKid{0, in, c});
      append_product_ops(pass[x], out, ks, kOpSigned);  // dL, d2L: either sign
    }
    append_chunk_major(pass, flat, launches);
  }
  return cur;
}

// Root-pair ops: the root's product in five variants, variant v into slot0 + v, with scratch
// matrix nn + x (for a tip son: scratch tip row nt + x) substituted on the sons a and b:
// x = 0 dP_a, 1 d2P_a, 2 dP_b, 3 d2P_b.  Chunk-major: five variants per launch.
inline void root_pair_ops(const TopoView& t, int root, int a, int b, int nt, int nn, int slot0, std::vector<KOp>& flat,
                          std::vector<OpLaunch>& launches) {
  // variant v: scratch index substituted on a and on b (-1 = the son's own P)
  static const int sub[5][2] = {{0, -1}, {-1, 2}, {1, -1}, {-1, 3}, {0, 2}};
  std::vector<std::vector<KOp> > variant(5);
  for (int v = 0; v < 5; ++v) {
    std::vector<OpKid> ks;
    for (int c : t.kids[root]) {
      const int x = c == a ? sub[v][0] : c == b ? sub[v][1] : -1;
      ks.push_back(OpKid{c < nt, c < nt ? (x >= 0 ? nt + x : c) : c - nt, x >= 0 ? nn + x : c});
    }
    append_product_ops(variant[v], slot0 + v, ks, kOpSigned);  // substituted products: either sign
  }
  append_chunk_major(variant, flat, launches);
}

// Upper ops: U_v = (M_f U_f) (*) prod_{siblings s} (P_s L_s) into slot dr_slot0 + v for every
// v of `nodes` (f the father of v; M_f is matrix mat_base + f; no U_f term under the root).
// Chunk j of all nodes in one launch; the caller passes one preorder level at a time.
inline void upper_ops(const TopoView& t, const std::vector<int>& nodes, int nt, int dr_slot0, int mat_base,
                      std::vector<KOp>& flat, std::vector<OpLaunch>& launches) {
  std::vector<std::vector<KOp> > per_node(nodes.size());
  for (size_t i = 0; i < nodes.size(); ++i) {
    const int v = nodes[i], f = t.parent[v];
    std::vector<OpKid> ks;
    if (f != t.root) ks.push_back(OpKid{0, dr_slot0 + f, mat_base + f});
    for (int s : t.kids[f])
      if (s != v) ks.push_back(own_kid(s, nt));
    append_product_ops(per_node[i], dr_slot0 + v, ks, 0);
  }
  append_chunk_major(per_node, flat, launches);
}

}  // namespace plk
