// MFMA weight-gradient, exact-f32 instantiations.
#include "wgrad_impl.h"
namespace segmi {
int wgrad_mfma_f32(const WgradParams& p, const WgradPlan& pl, int ksize, int stride, hipStream_t st) {
  return launch_wgrad_mfma<float>(p, pl, ksize, stride, st);
}
}  // namespace segmi
