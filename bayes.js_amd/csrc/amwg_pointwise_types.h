// amwg_pointwise_types.h -- the two plain structs the WAIC / LOO kernels (amwg_pointwise.h) and their host launchers (amwg_waic.h, amwg_loo.h) exchange.  No device
// code: the host units take these without the kernel templates; hiprtc takes them with amwg_pointwise.h.
#pragma once
#include "amwg_stdint.h"
#include "amwg_types.h"

// one dataset's size and the places of its copies inside the family's arrays (DatasetConsts, amwg_dataset.h: what the step kernels read); a closure: n_obs = kTermN
struct WaicDataset {
  int32_t n_obs, data_mid_range;
  int64_t off_x, off_y, off_lfact, off_xb;
};

namespace amwg {
// the model argument of a translated closure: its DataRef; a dataset sampler's table of pointers [n_datasets][row_stride] (amwg_user_dataset.h), nullptr otherwise
struct UserTermsArg {
  DataRef d;
  const void *const *table;
  int32_t row_stride, reserved;
};
}  // namespace amwg
