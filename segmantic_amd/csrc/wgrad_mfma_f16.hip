// MFMA weight-gradient, fp16 instantiations (ds_read_b64_tr_b16 + v_mfma_f32_16x16x32_f16).
#include "wgrad_mfma_h16.h"
namespace segmi {
int wgrad_mfma_f16(const WgradParams& p, int ksize, int stride, int ct, int gx, hipStream_t st) {
  return wgrad_mfma_h16<f16_t>(p, ksize, stride, ct, gx, st);
}
}  // namespace segmi
