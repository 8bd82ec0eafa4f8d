// twoval_eval_host.cpp -- TEST INFRASTRUCTURE: csrc/amwg_twoval.h (the same source the kernels compile) built for the HOST and evaluated for arrays of lanes:
// lane j sums the n observations of the caller's six tables (w, pre, om1, po1, om0, po0 back to back, n / 32 + 2 words each) from acc0[j] with the addends
// l1[j] (observation = 1) and l0[j] (tests/twoval_cases.py, tests/test_twoval_host.py).
//   g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -fPIC -shared -I bayes.js_amd/csrc tests/host/twoval_eval_host.cpp -o twoval_eval_host.so
#include "amwg_twoval.h"

using namespace amwg;

extern "C" int twoval_eval(const uint32_t *tab, int n, long m, const double *acc0, const double *l1, const double *l0, double *out) {
  if (!tab || n < 0 || m < 0) return -1;
  const size_t W = two_valued_words(n);
  const BitData B{tab, tab + W, tab + 2 * W, tab + 3 * W, tab + 4 * W, tab + 5 * W, n};
  for (long j = 0; j < m; ++j) out[j] = two_valued_sum(acc0[j], l1[j], l0[j], B);
  return 0;
}
