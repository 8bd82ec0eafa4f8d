// csrc/amwg_cdf.h compiled for the host (tests/test_cdf_host.py): the functions the predictive kernels call, on arrays.
#include "amwg_ld.h"
#include "amwg_cdf.h"

extern "C" void cdf_erfc(long n, const double *x, double *out) {
  for (long i = 0; i < n; ++i) out[i] = amwg::erfc_amwg(x[i]);
}
// lfact and lg as the library hands them over: lfactorial_js(y) (the packed array of the Poisson family), log_v8(lam).  out[i] = F, Fm, Q
extern "C" void cdf_poisson(long n, const double *y, const double *lam, double *out) {
  for (long i = 0; i < n; ++i)
    amwg::poisson_cdf_pair(y[i], y[i] < 0 ? amwg::kInf : amwg::lfactorial_js(y[i]), lam[i], amwg::log_v8(lam[i]), out[3 * i], out[3 * i + 1], out[3 * i + 2]);
}
