// MFMA conv / transposed-conv forward for the 16-bit storage formats: one body, instantiated once per format
// (conv_mfma_bf16.hip: v_mfma_f32_16x16x32_bf16, conv_mfma_f16.hip: v_mfma_f32_16x16x32_f16).  Both formats pick
// the same kernel family for every layer (conv_plan.h).
#pragma once
#include "conv_fwd_impl.h"
#include "conv_ring2_impl.h"
#include "conv_ring3_impl.h"
#include "conv_ks_impl.h"
#include "convt_ps_impl.h"
#include "conv_bnbwd_impl.h"
namespace segmi {
template <typename T>
static int conv_mfma_h16(const ConvParams& p, const ConvPlan& pl, int ksize, int stride, hipStream_t st) {
  switch (pl.family) {
    case kConvRing3: return launch_conv_ring3<T>(p, pl, st);
    case kConvRing2: return launch_conv_ring2<T>(p, pl, st);
    case kConvKSplit: return launch_conv_ks<T, 32>(p, pl, st);
    case kConvTile: return launch_conv_tile<T>(p, pl, ksize, stride, st);
  }
  SEGMI_UNSUPPORTED("conv3d: kernel family %d is not an MFMA family", pl.family);
}
template <typename T>
static int conv_s2_bnbwd_h16(const ConvBnBwdParams& p, hipStream_t st) {
  switch (p.Cout / 16) {
    case 1: return launch_conv_s2_bnbwd<T, 1>(p, st);
    case 2: return launch_conv_s2_bnbwd<T, 2>(p, st);
    case 4: return launch_conv_s2_bnbwd<T, 4>(p, st);
  }
  SEGMI_UNSUPPORTED("bn_act_bwd_apply_conv: %d output channels", p.Cout);
}
template <typename T>
static int convt_mfma_h16(const ConvTParams& p, const ConvTPlan& pl, hipStream_t st) {
  return pl.family == kConvTPersistent ? launch_convt_ps<T>(p, pl, st) : launch_convt_tile<T>(p, pl, st);
}
}  // namespace segmi
