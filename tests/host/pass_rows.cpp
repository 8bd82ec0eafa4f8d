// pass_rows.cpp -- TEST INFRASTRUCTURE (host): the row plan of the wavefront's certified pass (csrc/amwg_pass.h pass_rows / pass_part_slot / pass_part_row, the
// helpers norm_sq_pass_wave itself walks by).  For every n from 1 to argv[1] and B in {8, 16}, following the kernel's own order -- the full blocks, then the parts
// B/2, B/4, .., 1 of the remainder, then the partly filled row --: every observation is covered exactly once, a lane meets its observations in increasing order, the
// remainder's slots do not overlap, and at most one block is shorter than B rows.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "amwg_pass.h"
using namespace amwg;
int main(int argc, char **argv) {
  const int n_max = argc > 1 ? atoi(argv[1]) : 4 * 1024 + 65;
  long bad = 0, checked = 0;
  auto fail = [&](const char *what, int n, int B) { if (bad++ < 10) printf("FAIL n=%d B=%d: %s\n", n, B, what); };
  for (int B : {8, 16}) {
    for (int n = 1; n <= n_max; ++n) {
      ++checked;
      const PassRows pr = pass_rows(n, B);
      std::vector<int> seen(n, 0), last(64, -1);
      std::vector<int> slot_used(B, 0);
      auto visit = [&](int i, int lane) {
        if (i < 0 || i >= n) { fail("an index outside the data", n, B); return; }
        ++seen[i];
        if (i <= last[lane]) fail("a lane's observations out of order", n, B);
        last[lane] = i;
      };
      if (pr.full < 0 || pr.full >= B || pr.blocks < 0 || (pr.masked != 0 && pr.masked != 1)) fail("plan out of range", n, B);
      int short_blocks = 0;
      for (int k = 0; k < pr.blocks; ++k)
        for (int b = 0; b < B; ++b)
          for (int lane = 0; lane < 64; ++lane) visit((k * B + b) * 64 + lane, lane);
      const int rows_left = pr.full + pr.masked;
      if (rows_left > 0 && rows_left < B) ++short_blocks;
      if (rows_left > B) fail("a remainder longer than a block", n, B);
      for (int p = B / 2; p >= 1; p /= 2) {
        if (!(pr.full & p)) continue;
        for (int b = 0; b < p; ++b) {
          const int slot = pass_part_slot(B, p) + b, row = pass_part_row(pr.full, p) + b;
          if (slot < 0 || slot >= B - 1) { fail("a part's slot outside the set (or on the partly filled row's)", n, B); continue; }
          if (slot_used[slot]++) fail("two rows in one slot", n, B);
          if (row < 0 || row >= pr.full) fail("a part's row outside the remainder", n, B);
          for (int lane = 0; lane < 64; ++lane) visit(pr.blocks * B * 64 + row * 64 + lane, lane);
        }
      }
      if (pr.masked)
        for (int lane = 0; lane < 64; ++lane) {
          const int i = pr.blocks * B * 64 + pr.full * 64 + lane;
          if (i < n) visit(i, lane);      // (the kernel's `has`)
        }
      for (int i = 0; i < n; ++i)
        if (seen[i] != 1) { fail("an observation not covered exactly once", n, B); break; }
      if (short_blocks > 1) fail("more than one block shorter than B", n, B);
    }
  }
  printf("checked=%ld failures=%ld\n", checked, bad);
  return bad ? 1 : 0;
}
