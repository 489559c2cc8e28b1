// MFMA conv / transposed-conv forward, bf16 instantiations (v_mfma_f32_16x16x32_bf16).
#include "conv_mfma_h16.h"
namespace segmi {
int conv_mfma_bf16(const ConvParams& p, const ConvPlan& pl, int ksize, int stride, hipStream_t st) {
  return conv_mfma_h16<bf16_t>(p, pl, ksize, stride, st);
}
int conv_s2_bnbwd_bf16(const ConvBnBwdParams& p, hipStream_t st) { return conv_s2_bnbwd_h16<bf16_t>(p, st); }
int convt_mfma_bf16(const ConvTParams& p, const ConvTPlan& pl, hipStream_t st) { return convt_mfma_h16<bf16_t>(p, pl, st); }
}  // namespace segmi
