// conv_ring_impl.h -- geometry of the persistent "z-marching" MFMA Conv3d forward for the
// full-resolution layers (k3, stride 1, Cin = one chunk); the kernel itself is conv_ring2_impl.h, the plan (z-split, ring3 or ring2) conv_plan.h.
// (The first formulation -- one output plane x 8 rows per wave, described below -- needed one 1-KiB
// LDS fragment per MFMA and spilled in its f32 and 32-channel variants; bf16 layers run ring2, f32
// layers the K-split / tile kernels, which are 6 % faster there than the spilling ring was.)
//
// A workgroup owns a column of output tiles (fixed n, y-tile, x-tile) and marches along z in
// steps of TD = 4 planes.  The input halo lives in a ring of R = 10 LDS planes of (8+2)x(16+2)
// voxel rows: step i computes from ring slots 4i..4i+5 (mod 10) while the 4 NEW planes of step
// i+1 -- fetched from HBM before the compute phase -- are written to slots 4i+6..4i+9, which
// nobody reads during step i.  So, compared with the tile-at-a-time kernel:
//   * every input plane is read once per column instead of 1.5x (z halo re-reads are gone),
//   * the global-load latency hides under 112 MFMAs per wave (one s_barrier per step),
//   * weight fragments stay in registers for the whole column, residual rows are prefetched,
//   * BN statistics are reduced once per column (rows = columns, 32x fewer than tiles).
// Wave w computes plane z = 4i + w of the step (8 voxel tiles = 8 y-rows of 16 x), so the kd
// part of every LDS address is wave-uniform.
#pragma once
#include "conv_fwd_impl.h"

namespace segmi {

template <typename T, int CK>
struct RingGeom {
  static constexpr int KG = Elem<T>::KG;
  static constexpr int SPT = CK / KG;
  static constexpr int TD = 4, TH = 8, TW = 16;
  static constexpr int HH = TH + 2, HW = TW + 2;
  static constexpr int R = 10;
  static constexpr int NSLOT = 27 * SPT;
  static constexpr int NSTEP = (NSLOT + 3) / 4;
  static constexpr int RAWB = CK * (int)sizeof(T);
  static constexpr int ROWB = RAWB == 32 ? 32 : RAWB + 16;
  static constexpr int CPR = RAWB / 16;
  static constexpr int PLANE_ROWS = HH * HW;
  static constexpr int PLANE_B = PLANE_ROWS * ROWB;
  static constexpr int LDS_BYTES = R * PLANE_B;
  static constexpr int PLANE_CHUNKS = PLANE_ROWS * CPR;        // 16-byte chunks per plane
  static constexpr int NLD = (TD * PLANE_CHUNKS + 255) / 256;   // loads per thread per step
  static constexpr int NLD0 = (2 * PLANE_CHUNKS + 255) / 256;   // extra loads of the prologue
};

// 4 channels of one voxel in storage format
template <typename T> struct Raw4;
template <> struct Raw4<float> {
  typedef f32x4 type;
  __device__ static type ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  __device__ static f32x4 cvt(type v) { return v; }
};
template <> struct Raw4<bf16_t> {
  typedef u32x2 type;
  __device__ static type ld(const bf16_t* p) { return *reinterpret_cast<const u32x2*>(p); }
  __device__ static f32x4 cvt(type o) {
    return f32x4{__uint_as_float(o[0] << 16), __uint_as_float(o[0] & 0xffff0000u),
                 __uint_as_float(o[1] << 16), __uint_as_float(o[1] & 0xffff0000u)};
  }
};
template <> struct Raw4<f16_t> {
  typedef u32x2 type;
  __device__ static type ld(const f16_t* p) { return *reinterpret_cast<const u32x2*>(p); }
  __device__ static f32x4 cvt(type o) {
    return f32x4{H16<f16_t>::lo(o[0]), H16<f16_t>::hi(o[0]), H16<f16_t>::lo(o[1]), H16<f16_t>::hi(o[1])};
  }
};


}  // namespace segmi
