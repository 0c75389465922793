// Emit the hiprtc source of the one-class-per-workgroup program with a table image
// (plk_jit.hpp: JitShape::img) for tests/test_jit_table_image.py: the traversal (plk_jit_tree4c,
// whose prologue is one copy of the image) and the builder kernels (plk_jit_tabs4c, _l) in one
// module.
//   jit_emit_img <wp 0|1> [img 0|1] > kernel.hip
// The program is the 7-tip tree of jit_emit_wp.cpp (tree4q): root 11 = (Q 10 = ((t0, t1)8,
// (t2, t3)9), (t4, t5)7, t6) -- a quad, a cherry and a tip -- in the same shape (C = 4, two
// patterns per lane, direct codes, wave tasks), so that its resources compare with that test's.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plk_jit.hpp"

using namespace plk;

int main(int argc, char** argv) {
  const bool wp = argc > 1 && std::atoi(argv[1]) != 0;
  const bool img = argc > 2 ? std::atoi(argv[2]) != 0 : true;
  std::vector<TInstr> prog;
  auto add = [&](int op, int d, int a, int b) { prog.push_back(TInstr{op, d, a, b}); };
  add(T_DESCEND, 1, 0, 0);
  add(T_DESCEND, 2, 0, 0);
  add(T_TIP, 2, 0, 0);
  add(T_TIP, 2, 1, 1);
  add(T_ASCEND, 2, -1, 8);
  add(T_DESCEND, 2, 0, 0);
  add(T_TIP, 2, 2, 2);
  add(T_TIP, 2, 3, 3);
  add(T_ASCEND, 2, -1, 9);
  add(T_ASCEND, 1, -1, 10);
  add(T_DESCEND, 1, 0, 0);
  add(T_TIP, 1, 4, 4);
  add(T_TIP, 1, 5, 5);
  add(T_ASCEND, 1, -1, 7);
  add(T_TIP, 0, 6, 6);
  add(T_ROOT, 0, -1, 1);
  const std::vector<int32_t> starts = {0};
  JitShape sh;
  sh.C = 4;
  sh.cls = true;
  sh.CW = 1;
  sh.U = 4;
  sh.scale = false;
  const JitPlan plan = jit_plan(prog, starts, sh.C, sh.U, 136 * 1024 / 8, false, true, 136 * 1024 / 8);
  sh.NT = plan.NU;
  sh.TD = plan.tab_doubles;
  sh.QT = plan.quad_tmp;
  sh.soa = true;
  sh.dc = true;
  sh.dcw = 1;
  sh.G = 4;
  sh.PW = 2;
  sh.L = 3;
  sh.ppipe = true;
  sh.wt = true;
  sh.wp = wp;
  sh.img = img;
  const std::string src = jit_tree4_source(plan, sh);
  if (src.empty()) return 1;
  std::fwrite(src.data(), 1, src.size(), stdout);
  return 0;
}
