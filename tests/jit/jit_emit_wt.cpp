// Emit the hiprtc source of the two direct-code programs whose waves share nothing in the loop
// (plk_jit.hpp: JitShape::wt_ok), with the wave-task schedule on or off, so that
// tests/test_jit_wave_tasks.py can cross-compile both for gfx950 and compare the code objects.
//   jit_emit_wt <tree4q|ciw> <wt 0|1> > kernel.hip
//   tree4q: one class per workgroup with a quad unit (plk_jit_tree4c), C = 4, two patterns per lane
//   ciw:    every class in the wave with rescaling and stored fragment roots (plk_jit_tree4), C = 4,
//           two 16-byte code words per pattern
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plk_jit.hpp"

using namespace plk;

int main(int argc, char** argv) {
  const std::string kind = argc > 1 ? argv[1] : "tree4q";
  const bool wt = argc > 2 && std::atoi(argv[2]) != 0;
  std::vector<TInstr> prog;
  auto add = [&](int op, int d, int a, int b) { prog.push_back(TInstr{op, d, a, b}); };
  std::vector<int32_t> starts;
  if (kind == "tree4q") {
    // one fragment, root 11 = (Q 10 = ((t0, t1)8, (t2, t3)9), (t4, t5)7, t6): a quad, a cherry, a tip
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
    starts = {0};
  } else {
    // 7 tips (0..6), internal nodes 7..11.  Fragment 0: node 10 = ((t0, t1)8, (t2, t3)9),
    // stored in slot 0.  Fragment 1 (root 11): (t4, t5)7 unstored, t6, slot 0 via branch 10.
    add(T_DESCEND, 1, 0, 0);
    add(T_TIP, 1, 0, 0);
    add(T_TIP, 1, 1, 1);
    add(T_ASCEND, 1, -1, 8);
    add(T_DESCEND, 1, 0, 0);
    add(T_TIP, 1, 2, 2);
    add(T_TIP, 1, 3, 3);
    add(T_ASCEND, 1, -1, 9);
    add(T_ROOT, 0, 0, 0);
    const int start1 = (int)prog.size();
    add(T_DESCEND, 1, 0, 0);
    add(T_TIP, 1, 4, 4);
    add(T_TIP, 1, 5, 5);
    add(T_ASCEND, 1, -1, 7);
    add(T_TIP, 0, 6, 6);
    add(T_DESCEND, 1, 0, 0);
    add(T_LOAD, 1, 0, 10);
    add(T_ASCEND, 1, 1, 11);
    add(T_ROOT, 0, -1, 1);
    starts = {0, start1};
  }
  JitShape sh;
  sh.C = 4;
  sh.cls = kind == "tree4q";
  sh.CW = sh.cls ? 1 : sh.C;
  sh.U = sh.cls ? 4 : 16;
  sh.scale = !sh.cls;
  const JitPlan plan = sh.cls ? jit_plan(prog, starts, sh.C, sh.U, 136 * 1024 / 8, false, true, 136 * 1024 / 8)
                              : jit_plan(prog, starts, sh.C, sh.U, 64 * 1024 / 8, true);
  sh.NT = plan.NU;
  sh.TD = plan.tab_doubles;
  sh.QT = plan.quad_tmp;
  sh.soa = sh.cls;
  sh.dc = true;
  sh.dcw = sh.cls ? 1 : 2;
  sh.G = sh.cls ? 4 : 2;
  sh.PW = sh.cls ? 2 : 1;
  sh.L = sh.CW > 1 ? 2 : 3;
  sh.ppipe = true;
  sh.wt = wt;
  if (!sh.wt_ok()) {
    std::fprintf(stderr, "shape is not eligible for wave tasks\n");
    return 1;
  }
  const std::string src = jit_tree4_source(plan, sh);
  if (src.empty()) return 1;
  std::fwrite(src.data(), 1, src.size(), stdout);
  return 0;
}
