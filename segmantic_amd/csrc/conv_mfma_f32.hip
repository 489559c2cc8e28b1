// MFMA conv / transposed-conv forward, exact-f32 instantiations (v_mfma_f32_16x16x4_f32).
#include "conv_fwd_impl.h"
#include "conv_ks_impl.h"
#include "convt_ps_impl.h"
namespace segmi {
int conv_mfma_f32(const ConvParams& p, const ConvPlan& pl, int ksize, int stride, hipStream_t st) {
  if (pl.family == kConvKSplit) return launch_conv_ks<float, 16>(p, pl, st);
  return launch_conv_tile<float>(p, pl, ksize, stride, st);
}
int convt_mfma_f32(const ConvTParams& p, const ConvTPlan& pl, hipStream_t st) {
  return pl.family == kConvTPersistent ? launch_convt_ps<float>(p, pl, st) : launch_convt_tile<float>(p, pl, st);
}
}  // namespace segmi
