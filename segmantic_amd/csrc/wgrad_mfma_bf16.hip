// MFMA weight-gradient, bf16 instantiations (ds_read_b64_tr_b16 + v_mfma_f32_16x16x32_bf16).
#include "wgrad_mfma_h16.h"
namespace segmi {
int wgrad_mfma_bf16(const WgradParams& p, const WgradPlan& pl, int ksize, int stride, hipStream_t st) {
  return wgrad_mfma_h16<bf16_t>(p, pl, ksize, stride, st);
}
}  // namespace segmi
