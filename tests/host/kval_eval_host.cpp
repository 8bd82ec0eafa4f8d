// kval_eval_host.cpp -- TEST INFRASTRUCTURE: csrc/amwg_kval.h (the same source the kernels compile) built for the HOST and evaluated for arrays of lanes:
// lane j sums the value indices idx[n] from acc0[j] with the addends c[j * K + k] on the caller's tables (tests/kval_cases.py, tests/test_kval_host.py).
//   g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -fPIC -shared -I bayes.js_amd/csrc tests/host/kval_eval_host.cpp -o kval_eval_host.so
#include "amwg_kval.h"

using namespace amwg;

template <int K>
static void lanes(const uint8_t *idx, int n, const uint32_t *tab, long m, const double *acc0, const double *c, double *out) {
  const KValData B{tab, idx, n};
  for (long j = 0; j < m; ++j) {
    double cs[K];
    for (int k = 0; k < K; ++k) cs[k] = c[j * K + k];
    out[j] = k_valued_sum<K>(acc0[j], cs, B);
  }
}

extern "C" int kval_eval(int K, const uint8_t *idx, int n, const uint32_t *tab, long m, const double *acc0, const double *c, double *out) {
  switch (K) {
    case 1: lanes<1>(idx, n, tab, m, acc0, c, out); return 0;
    case 2: lanes<2>(idx, n, tab, m, acc0, c, out); return 0;
    case 3: lanes<3>(idx, n, tab, m, acc0, c, out); return 0;
    case 5: lanes<5>(idx, n, tab, m, acc0, c, out); return 0;
    case 8: lanes<8>(idx, n, tab, m, acc0, c, out); return 0;
    case 13: lanes<13>(idx, n, tab, m, acc0, c, out); return 0;
    case 16: lanes<16>(idx, n, tab, m, acc0, c, out); return 0;
  }
  return -1;
}
