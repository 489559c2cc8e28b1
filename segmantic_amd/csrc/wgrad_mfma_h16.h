// MFMA weight-gradient for the 16-bit storage formats (ds_read_b64_tr_b16 + v_mfma_f32_16x16x32_{bf16,f16}): one
// body, instantiated by wgrad_mfma_bf16.hip and wgrad_mfma_f16.hip.
#pragma once
#include "wgrad_impl.h"
#include "wgrad_ws_impl.h"
namespace segmi {

// the wave-specialised kernel's instantiation of a plan: stride, channel blocking, dY tile
template <typename T>
static int launch_wgrad_ws(const WgradParams& p, const WgradPlan& pl, int stride, hipStream_t st) {
  switch (wgrad_key(3, stride, pl.ct, Tile3{pl.td, pl.th, pl.tw})) {
    WG_PLANNED(launch_wgrad_ws_cfg, 3, 1, 1, 1) WG_PLANNED(launch_wgrad_ws_cfg, 3, 1, 2, 1)
    WG_PLANNED(launch_wgrad_ws_cfg, 3, 2, 1, 1) WG_PLANNED(launch_wgrad_ws_cfg, 3, 2, 2, 1)
  }
  SEGMI_UNSUPPORTED("conv3d_wgrad: no wave-specialised kernel for s%d, channel blocking %d", stride, pl.ct);
}

template <typename T>
static int wgrad_mfma_h16(const WgradParams& p, const WgradPlan& pl, int ksize, int stride, hipStream_t st) {
  if (pl.path == kWgradWaveSpecialised) return launch_wgrad_ws<T>(p, pl, stride, st);
  return launch_wgrad_mfma<T>(p, pl, ksize, stride, st);
}
}  // namespace segmi
