// pointwise_eval_host.cpp -- TEST INFRASTRUCTURE: evaluates the pointwise terms of a translated closure (the generated `amwg::UserTerms`, the same text hiprtc
// compiles for the GPU behind the closure's source) on the host: make_draw once per state, then term for every observation.
//   g++ -std=c++17 -O2 -ffp-contract=off -I bayes.js_amd/csrc -DAMWG_USER_SOURCE='"<file.hip>"' -DAMWG_TERMS_SOURCE='"<file.terms.hip>"' -shared -fPIC ...
#include "amwg_user.h"
#include AMWG_USER_SOURCE
#include AMWG_TERMS_SOURCE

extern "C" int pointwise_n_obs() { return amwg::UserTerms::kTermN; }
extern "C" int pointwise_state_n() { return amwg::UserTerms::kStateN; }
extern "C" int pointwise_draw_bytes() { return (int)sizeof(amwg::UserTerms::Draw); }

// state[kStateN] (component p at state[p]: a stored draw with one column); arrays[j]: device-typed storage (f64 / u8 / i32 as the translator chose); out[kTermN]
extern "C" void pointwise_terms(const double *state, const void *const *arrays, int n_arrays, double *out) {
  amwg::DataRef d{};
  for (int j = 0; j < n_arrays && j < amwg::kInlineUserArrays; ++j) d.arr[j] = arrays[j];
  d.arr_ext = n_arrays > amwg::kInlineUserArrays ? arrays + amwg::kInlineUserArrays : nullptr;
  amwg::UserTerms::Draw w = amwg::UserTerms::make_draw(state, 1, d);
  amwg::UserTerms::set_base(w, 0);
  for (int i = 0; i < amwg::UserTerms::kTermN; ++i) out[i] = amwg::UserTerms::term(w, d, amwg::UserTerms::kTermStart + i, state, 1);
}
