// MFMA conv / transposed-conv forward for the 16-bit storage formats: one body, instantiated once per format
// (conv_mfma_bf16.hip: v_mfma_f32_16x16x32_bf16, conv_mfma_f16.hip: v_mfma_f32_16x16x32_f16).  Both formats pick
// the same kernel family for every layer.
#pragma once
#include "conv_fwd_impl.h"
#include "conv_ring2_impl.h"
#include "conv_ring3_impl.h"
#include "conv_ks_impl.h"
#include "convt_ps_impl.h"
#include "conv_bnbwd_impl.h"
namespace segmi {
template <typename T>
static int conv_mfma_h16(const ConvParams& p, int ksize, int stride, hipStream_t st) {
  constexpr int dt = DtypeOf<T>::value;
  if (conv_ring_zsplit(dt, p.Cin, ksize, stride, p.N, p.Do, p.Ho, p.Wo) > 0)
    return conv_ring3_ok(p) ? launch_conv_ring3<T>(p, st) : launch_conv_ring2<T>(p, st);
  if (conv_ks_ok(dt, p.Cin, ksize, stride)) return launch_conv_ks_t<T, 32>(p, st);
  return launch_conv_mfma_t<T>(p, ksize, stride, st);
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
static int convt_mfma_h16(const ConvTParams& p, hipStream_t st) {
  if (convt_ps_ok(DtypeOf<T>::value, p.Cin, p.Cout, p.Wi)) return launch_convt_ps_t<T>(p, st);
  return launch_convt_mfma_t<T>(p, st);
}
}  // namespace segmi
