// Emit the hiprtc source of the two direct-code wave-task programs (plk_jit.hpp: JitShape::wt)
// with the workgroup task pool (JitShape::wp) on or off, so that tests/test_jit_task_pool.py can
// cross-compile both for gfx950 and compare the code objects; and check the pool's ticket -> task
// map (jit_pool_task, whose expression the generated kernel carries as POOL_TASK_) on the host.
//   jit_emit_wp <tree4q|ciw> <wp 0|1> > kernel.hip
//   jit_emit_wp map            (prints "ok"; exit status 1 and a line per violation otherwise)
//   tree4q: one class per workgroup with a quad unit (plk_jit_tree4c), C = 4, two patterns per lane
//   ciw:    every class in the wave with rescaling and stored fragment roots (plk_jit_tree4), C = 4,
//           two 16-byte code words per pattern
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plk_jit.hpp"

using namespace plk;

// Every task of [0, n_tasks) exactly once over the workgroups' tickets, per-workgroup counts
// within one of each other, and a workgroup's first ticket past its end (and the 16 behind it,
// one per wave that may still draw) past the end.
static int check_map() {
  int bad = 0;
  for (int gx : {1, 2, 3, 64})
    for (int n : {0, 1, 3, 17, 157, 7813}) {
      std::vector<int> seen((size_t)n, 0);
      int lo = n + 1, hi = -1;
      for (int x = 0; x < gx; ++x) {
        int cnt = 0;
        while (jit_pool_task(x, gx, cnt) < n) ++seen[(size_t)jit_pool_task(x, gx, cnt++)];
        for (int j = cnt; j <= cnt + 16; ++j)
          if (jit_pool_task(x, gx, j) < n) {
            std::printf("gx %d n %d: workgroup %d ticket %d comes back inside\n", gx, n, x, j);
            ++bad;
          }
        lo = std::min(lo, cnt);
        hi = std::max(hi, cnt);
      }
      for (int t = 0; t < n; ++t)
        if (seen[(size_t)t] != 1) {
          std::printf("gx %d n %d: task %d taken %d times\n", gx, n, t, seen[(size_t)t]);
          ++bad;
        }
      if (hi - lo > 1 || lo != n / gx || hi != (n + gx - 1) / gx) {
        std::printf("gx %d n %d: workgroups own %d .. %d tasks\n", gx, n, lo, hi);
        ++bad;
      }
    }
  if (!bad) std::printf("ok\n");
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  const std::string kind = argc > 1 ? argv[1] : "tree4q";
  if (kind == "map") return check_map();
  const bool wp = argc > 2 && std::atoi(argv[2]) != 0;
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
  sh.wt = true;
  sh.wp = wp;
  if (!sh.wt_ok()) {
    std::fprintf(stderr, "shape is not eligible for wave tasks\n");
    return 1;
  }
  const std::string src = jit_tree4_source(plan, sh);
  if (src.empty()) return 1;
  std::fwrite(src.data(), 1, src.size(), stdout);
  return 0;
}
