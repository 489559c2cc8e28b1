// wgrad_impl.h -- MFMA weight gradient of Conv3d k3 (stride 1 or 2).
//
//   dW[co][ci][tap] = sum_{n,vox} dY[n,vox,co] * X[n, vox*S + tap - 1, ci]
//
// GEMM with the huge voxel axis as K: D[co][ci] += A[co][k=vox] * B[k=vox][ci].  Both operands
// need "8 voxels of one channel" per lane, i.e. the transpose of the NDHWC rows staged in LDS:
//   bf16 -> ds_read_b64_tr_b16 (gfx950 transposing LDS read; 2 reads = one 16x16x32 operand)
//   f32  -> ds_read_b32 gathers (one 16x16x4 operand each)
// The k -> voxel assignment is free as long as A and B agree; we use voxel = 16h + 4g + q
// (h = which tr-read, g = lane>>4, q = row the lane addresses) so that every 32-lane LDS
// group touches 256 contiguous bytes (conflict-free for stride-1 convs).
//
// Work split: workgroup = (voxel-tile range) x (16*CT out-channels) x (16*CT in-channels);
// its 4 waves own taps {w, w+4, ...} (7/7/7/6) so no cross-wave reduction is needed, and keep
// their 7*CT*CT accumulators in registers across all tiles of the range (persistent loop).
// Per-workgroup partial slabs are reduced in fixed order by wgrad_reduce_kernel: bitwise
// reproducible, no atomics.
//
// Time split, measured with timing probes since removed, on the 128^3 x 8, 16 x 16 layer (cold caches,
// us): all 444, no global loads 316, no LDS-read / MFMA loop 254, neither 137 -- the three phases of a
// tile barely overlap at 2 workgroups per CU; the MFMA-loop phase sits at the LDS instruction
// rate (2 ds_read_b64_tr_b16 per operand, ~2.4 clk each, 2.3 per MFMA).
#pragma once
#include "common.h"
#include "conv_plan.h"

namespace segmi {

struct WgradParams {
  const void* x;
  const void* dy;
  float* partials;
  int N, Dx, Hx, Wx, Dy, Hy, Wy, Cin, Cout, ldx, ldy;
  int tz, ty, tx;
  int ntiles;
  int zs, zper;   // wave-specialised kernel: z-segments per column, z-tiles per segment
  unsigned x_bytes, y_bytes;   // ... and the byte extents of the two tensors (buffer num_records)
  int ci_chunks;
  // optional input transform of X (segmi_in_affine): the BatchNorm-apply + PReLU that produced the
  // forward input is applied while the X tile is committed to LDS (bf16 only)
  const float* in_scale;
  const float* in_shift;
  const float* in_alpha;
};

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) float lds_f32;

template <typename T, int KS_, int S, int CTO, int CTI, int TD, int TH, int TW>
struct WgradGeom {
  static constexpr int KS = KS_, PAD = (KS_ - 1) / 2, NTAPS = KS_ * KS_ * KS_;
  static constexpr int NTW = (NTAPS + 3) / 4;  // taps per wave
  static constexpr int NV = TD * TH * TW;
  static constexpr int NL = NV / 16;  // 16-voxel lines
  static constexpr int HD = (TD - 1) * S + KS, HH = (TH - 1) * S + KS, HW = (TW - 1) * S + KS;
  static constexpr int YROWB = 16 * CTO * (int)sizeof(T), XROWB = 16 * CTI * (int)sizeof(T);
  static constexpr int YCPR = YROWB / 16, XCPR = XROWB / 16;
  static constexpr int YBYTES = NV * YROWB;
  static constexpr int XROWS = HD * HH * HW;
  static constexpr int LDS_BYTES = YBYTES + XROWS * XROWB;
  static constexpr int LPG = sizeof(T) == 2 ? 2 : 1;  // lines per mma16
  static_assert(NL % LPG == 0, "tile must hold whole k-steps");
  static_assert(TW == 8 || TW == 16, "tile width");
};

// row (in X halo rows) of voxel `v` (0..15) of line `line`, before the tap offset
template <int S, int TH, int TW, int HH, int HW>
__device__ __forceinline__ constexpr int wg_line_row(int line) {
  // a line is 16 consecutive voxel indices: TW=16 -> one x-row, TW=8 -> two x-rows
  const int first = line * 16;
  const int y = (first / TW) % TH, z = first / (TW * TH);
  return (z * S * HH + y * S) * HW;
}

template <typename T, int KS, int S, int CTO, int CTI, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void wgrad_mfma_kernel(WgradParams p) {
  using G = WgradGeom<T, KS, S, CTO, CTI, TD, TH, TW>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ysm = smem;
  char* xsm = smem + G::YBYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i16 = lane & 15;

  const int cochunk = blockIdx.y / p.ci_chunks, cichunk = blockIdx.y % p.ci_chunks;
  const int co0 = cochunk * 16 * CTO, ci0 = cichunk * 16 * CTI;

  f32x4 acc[G::NTW][CTO][CTI];
#pragma unroll
  for (int a = 0; a < G::NTW; ++a)
#pragma unroll
    for (int b = 0; b < CTO; ++b)
#pragma unroll
      for (int c = 0; c < CTI; ++c) acc[a][b][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // wave-uniform tap offsets (bytes into the X tile)
  int tapoff[G::NTW];
#pragma unroll
  for (int ti = 0; ti < G::NTW; ++ti) {
    int tap = wave + 4 * ti;
    if (tap > G::NTAPS - 1) tap = G::NTAPS - 1;
    const int kd = tap / (KS * KS), kh = (tap / KS) % KS, kw = tap % KS;
    tapoff[ti] = ((kd * G::HH + kh) * G::HW + kw) * G::XROWB;
  }

  // per-lane address parts
  int ylane, xlane;
  if constexpr (sizeof(T) == 2) {
    const int q = i16 >> 2, pp = i16 & 3;
    const int v = 4 * g + q;  // voxel within the line
    ylane = v * G::YROWB + 8 * pp;
    xlane = ((v / TW) * S * G::HW + (v % TW) * S) * G::XROWB + 8 * pp;
  } else {
    ylane = g * G::YROWB + 4 * i16;   // + 4u rows per sub-step
    xlane = g * S * G::XROWB + 4 * i16;
  }

  const char* xb = (const char*)p.x;
  const char* yb = (const char*)p.dy;
  // Register-staged software pipeline: the global loads of tile t+1 are issued before the MFMA
  // phase of tile t and land in LDS after it (global latency hides under compute).
  constexpr int NLY = (G::NV * G::YCPR + 255) / 256, NLX = (G::XROWS * G::XCPR + 255) / 256;
  static_assert(NLX <= 32, "one validity bit per staged X chunk");
  frag_t ry[NLY], rx[NLX];
  // Step-invariant per-lane descriptors: 32-bit byte offset inside a tile and packed tile-local
  // coordinates.  Per tile only a wave-uniform base pointer and uniform limits change, so a load
  // costs ~6 VALU ops of bounds checking instead of a 64-bit voxel-address multiply chain.
  int y_goff[NLY], x_goff[NLX];
  unsigned y_pk[NLY], x_pk[NLX];
#pragma unroll
  for (int k = 0; k < NLY; ++k) {
    const int i = tid + 256 * k;
    const int v = i / G::YCPR, ch = i % G::YCPR;
    const int vz = v / (TW * TH), vy = (v / TW) % TH, vx = v % TW;
    y_goff[k] = ((vz * p.Hy + vy) * p.Wy + vx) * p.ldy * (int)sizeof(T) + ch * 16;
    y_pk[k] = i < G::NV * G::YCPR ? (unsigned)(vz | (vy << 8) | (vx << 16)) : 0xffffffffu;
  }
#pragma unroll
  for (int k = 0; k < NLX; ++k) {
    const int i = tid + 256 * k;
    const int v = i / G::XCPR, ch = i % G::XCPR;
    const int hx = v % G::HW, hy = (v / G::HW) % G::HH, hz = v / (G::HW * G::HH);
    x_goff[k] = ((hz * p.Hx + hy) * p.Wx + hx) * p.ldx * (int)sizeof(T) + ch * 16;
    x_pk[k] = i < G::XROWS * G::XCPR ? (unsigned)(hz | (hy << 8) | (hx << 16)) : 0xffffffffu;
  }
  // input transform: this thread's X chunks all sit at channel offset (tid % XCPR) * 8 of the block
  const bool in_tf = sizeof(T) == 2 && p.in_scale != nullptr;
  const bool in_act = in_tf && p.in_alpha != nullptr;
  float tsc[8], tsh[8];
  float in_alpha = in_act ? *p.in_alpha : 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ch = ci0 + (tid % G::XCPR) * 8 + e;
    tsc[e] = in_tf ? p.in_scale[ch] : 1.f;
    tsh[e] = in_tf ? p.in_shift[ch] : 0.f;
  }
  unsigned xin = 0u;   // bit k: rx[k] of the pending tile lies inside the volume (zero padding stays 0)
  auto fetch = [&](int tile) {
    int t = tile;
    const int txi = t % p.tx; t /= p.tx;
    const int tyi = t % p.ty; t /= p.ty;
    const int tzi = t % p.tz;
    const int n = t / p.tz;
    const int oz0 = tzi * TD, oy0 = tyi * TH, ox0 = txi * TW;
    const int iz0 = oz0 * S - G::PAD, iy0 = oy0 * S - G::PAD, ix0 = ox0 * S - G::PAD;
    const char* ybase = yb + (((((int64_t)n * p.Dy + oz0) * p.Hy + oy0) * p.Wy + ox0) * p.ldy + co0) *
                                 (int64_t)sizeof(T);
    const char* xbase = xb + (((((int64_t)n * p.Dx + iz0) * p.Hx + iy0) * p.Wx + ix0) * p.ldx + ci0) *
                                 (int64_t)sizeof(T);
    const unsigned lz = p.Dy - oz0, ly = p.Hy - oy0, lx = p.Wy - ox0;
#pragma unroll
    for (int k = 0; k < NLY; ++k) {        // dY tile [NV][16*CTO]
      const unsigned pk = y_pk[k];
      ry[k] = frag_t{0u, 0u, 0u, 0u};
      if ((pk & 255u) < lz && ((pk >> 8) & 255u) < ly && (pk >> 16) < lx)
        ry[k] = *reinterpret_cast<const frag_t*>(ybase + (unsigned)y_goff[k]);
    }
#pragma unroll
    for (int k = 0; k < NLX; ++k) {        // X halo tile [HD*HH*HW][16*CTI]
      const unsigned pk = x_pk[k];
      rx[k] = frag_t{0u, 0u, 0u, 0u};
      const bool inside = pk != 0xffffffffu && (unsigned)((int)(pk & 255u) + iz0) < (unsigned)p.Dx &&
          (unsigned)((int)((pk >> 8) & 255u) + iy0) < (unsigned)p.Hx &&
          (unsigned)((int)(pk >> 16) + ix0) < (unsigned)p.Wx;
      if (inside) rx[k] = *reinterpret_cast<const frag_t*>(xbase + (unsigned)x_goff[k]);
      if (in_tf) xin = inside ? (xin | (1u << k)) : (xin & ~(1u << k));
    }
  };
  // (the X loop exists in three copies behind wave-uniform branches: no transform / affine /
  // affine + PReLU -- no per-element selects on the two runtime flags)
  auto commit_with = [&](auto tf) {
#pragma unroll
    for (int k = 0; k < NLY; ++k) {
      const int i = tid + 256 * k;
      if (i < G::NV * G::YCPR)
        *reinterpret_cast<frag_t*>(ysm + (i / G::YCPR) * G::YROWB + (i % G::YCPR) * 16) = ry[k];
    }
#pragma unroll
    for (int k = 0; k < NLX; ++k) {
      const int i = tid + 256 * k;
      if (i < G::XROWS * G::XCPR) {
        frag_t val = rx[k];
        if ((xin >> k) & 1u) val = tf(val);
        *reinterpret_cast<frag_t*>(xsm + (i / G::XCPR) * G::XROWB + (i % G::XCPR) * 16) = val;
      }
    }
  };
  auto commit = [&]() {
    if constexpr (sizeof(T) == 2) {
      if (in_act && in_alpha >= 0.f && in_alpha <= 1.f) {
        commit_with([&](frag_t v) { return bn_prelu01_h8<T>(v, tsc, tsh, in_alpha); });
        return;
      }
      if (in_act) { commit_with([&](frag_t v) { return bn_prelu_h8<T>(v, tsc, tsh, in_alpha, true); }); return; }
      if (in_tf) { commit_with([&](frag_t v) { return bn_prelu_h8<T>(v, tsc, tsh, 0.f, false); }); return; }
    }
    commit_with([](frag_t v) { return v; });
  };
  if ((int)blockIdx.x < p.ntiles) fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    __syncthreads();   // every wave is done reading the previous tile
    commit();
    __syncthreads();
    if (tile + (int)gridDim.x < p.ntiles) fetch(tile + gridDim.x);

#pragma unroll
    for (int lg = 0; lg < G::NL / G::LPG; ++lg) {
      frag_t af[CTO];
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int ct = 0; ct < CTO; ++ct) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (lds_s16x4*)(ysm + ylane + (2 * lg) * 16 * G::YROWB + ct * 32));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (lds_s16x4*)(ysm + ylane + (2 * lg + 1) * 16 * G::YROWB + ct * 32));
          const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
          af[ct] = frag_t{l2[0], l2[1], h2[0], h2[1]};
        }
      } else {
#pragma unroll
        for (int ct = 0; ct < CTO; ++ct) {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            af[ct][u] = __float_as_uint(*(lds_f32*)(ysm + ylane + (lg * 16 + 4 * u) * G::YROWB + ct * 64));
        }
      }
#pragma unroll
      for (int ti = 0; ti < G::NTW; ++ti) {
        if (KS == 1 && wave != 0) break;  // k1: a single tap, owned by wave 0
        frag_t bf[CTI];
        if constexpr (sizeof(T) == 2) {
          const int r0 = wg_line_row<S, TH, TW, G::HH, G::HW>(2 * lg) * G::XROWB;
          const int r1 = wg_line_row<S, TH, TW, G::HH, G::HW>(2 * lg + 1) * G::XROWB;
#pragma unroll
          for (int it = 0; it < CTI; ++it) {
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (lds_s16x4*)(xsm + xlane + tapoff[ti] + r0 + it * 32));
            const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (lds_s16x4*)(xsm + xlane + tapoff[ti] + r1 + it * 32));
            const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
            bf[it] = frag_t{l2[0], l2[1], h2[0], h2[1]};
          }
        } else {
          const int r0 = wg_line_row<S, TH, TW, G::HH, G::HW>(lg) * G::XROWB;
#pragma unroll
          for (int it = 0; it < CTI; ++it) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              // voxel 4u+g of the line: TW=16 -> same x-row; TW=8 -> rows u>>1
              const int vo = TW == 16 ? 4 * u * S : ((u >> 1) * S * G::HW + 4 * (u & 1) * S);
              bf[it][u] = __float_as_uint(
                  *(lds_f32*)(xsm + xlane + tapoff[ti] + r0 + vo * G::XROWB + it * 64));
            }
          }
        }
#pragma unroll
        for (int ct = 0; ct < CTO; ++ct)
#pragma unroll
          for (int it = 0; it < CTI; ++it) acc[ti][ct][it] = mma16<T>(af[ct], bf[it], acc[ti][ct][it]);
      }
    }
  }

  // partial slab [block][Cout][Cin][27]
  float* slab = p.partials + (int64_t)blockIdx.x * p.Cout * p.Cin * G::NTAPS;
#pragma unroll
  for (int ti = 0; ti < G::NTW; ++ti) {
    const int tap = wave + 4 * ti;
    if (tap < G::NTAPS) {
#pragma unroll
      for (int ct = 0; ct < CTO; ++ct)
#pragma unroll
        for (int it = 0; it < CTI; ++it)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int co = co0 + ct * 16 + 4 * g + e, ci = ci0 + it * 16 + i16;
            slab[((int64_t)co * p.Cin + ci) * G::NTAPS + tap] = acc[ti][ct][it][e];
          }
    }
  }
}

template <typename T, int KS, int S, int CTO, int CTI, int TD, int TH, int TW>
static int launch_wgrad_cfg(WgradParams p, int gx_hint, hipStream_t st) {
  using G = WgradGeom<T, KS, S, CTO, CTI, TD, TH, TW>;
  p.tz = cdiv(p.Dy, TD);
  p.ty = cdiv(p.Hy, TH);
  p.tx = cdiv(p.Wy, TW);
  p.ntiles = p.N * p.tz * p.ty * p.tx;
  // 32-bit byte offsets inside one staged tile
  SEGMI_CHECK_ARG((int64_t)G::HD * p.Hx * p.Wx * p.ldx * (int64_t)sizeof(T) < (1ll << 31) &&
                      (int64_t)TD * p.Hy * p.Wy * p.ldy * (int64_t)sizeof(T) < (1ll << 31),
                  "conv3d_wgrad: plane too large for the MFMA kernel's 32-bit tile offsets");
  p.ci_chunks = p.Cin / (16 * CTI);
  const int co_chunks = p.Cout / (16 * CTO);
  dim3 grid((unsigned)gx_hint, (unsigned)(co_chunks * p.ci_chunks));
  auto kern = wgrad_mfma_kernel<T, KS, S, CTO, CTI, TD, TH, TW>;
  static bool attr_done = false;
  if (!attr_done && G::LDS_BYTES > 64 * 1024) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                              hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES);
    attr_done = true;
  }
  hipLaunchKernelGGL(kern, grid, 256, G::LDS_BYTES, st, p);
  SEGMI_LAUNCH_CHECK("conv3d_wgrad(mfma)");
  return SEGMI_OK;
}

// the MFMA kernel's instantiation of a plan: (k, s), channel blocking, dY tile (wgrad_tile_shape)
constexpr int wgrad_key(int ks, int s, int ct, Tile3 t) { return ((((ks * 4 + s) * 32 + ct) * 8 + t.td) * 16 + t.th) * 32 + t.tw; }
#define WG_CASE(LAUNCH, KS, S, CTO, CTI, TD, TH, TW) \
  case wgrad_key(KS, S, 10 * CTO + CTI, Tile3{TD, TH, TW}): return LAUNCH<T, KS, S, CTO, CTI, TD, TH, TW>(p, pl.gx, st);
#define WG_W(LAUNCH, KS, S, CTO, CTI, WIDE)                                     \
  WG_CASE(LAUNCH, KS, S, CTO, CTI, wgrad_tile_shape(KS, S, 10 * CTO + CTI, WIDE).td, \
          wgrad_tile_shape(KS, S, 10 * CTO + CTI, WIDE).th, wgrad_tile_shape(KS, S, 10 * CTO + CTI, WIDE).tw)
#define WG_PLANNED(LAUNCH, KS, S, CTO, CTI) WG_W(LAUNCH, KS, S, CTO, CTI, true) WG_W(LAUNCH, KS, S, CTO, CTI, false)
// Shapes no plan picks (the stride-2 tiles on a stride-1 block, the 2-plane tile on the k3 16 x 16 block).  The library
// has carried these instantiations since before the plan existed; they are listed so that its kernels stay what they were.
#define WG_UNPLANNED_S1(KS, CTO, CTI) \
  WG_CASE(launch_wgrad_cfg, KS, 1, CTO, CTI, 2, 4, 16) WG_CASE(launch_wgrad_cfg, KS, 1, CTO, CTI, 2, 8, 8)

template <typename T>
static int launch_wgrad_mfma(const WgradParams& p, const WgradPlan& pl, int ksize, int stride, hipStream_t st) {
  const int key = wgrad_key(ksize, stride, pl.ct, Tile3{pl.td, pl.th, pl.tw});
  if constexpr (sizeof(T) == 2) {
    switch (key) {
      WG_PLANNED(launch_wgrad_cfg, 1, 1, 2, 1) WG_PLANNED(launch_wgrad_cfg, 3, 1, 2, 1) WG_PLANNED(launch_wgrad_cfg, 3, 2, 2, 1)
      WG_UNPLANNED_S1(1, 2, 1) WG_UNPLANNED_S1(3, 2, 1)
    }
  }
  switch (key) {
    WG_PLANNED(launch_wgrad_cfg, 1, 1, 1, 1) WG_PLANNED(launch_wgrad_cfg, 3, 1, 1, 1) WG_PLANNED(launch_wgrad_cfg, 3, 2, 1, 1)
    WG_UNPLANNED_S1(1, 1, 1) WG_CASE(launch_wgrad_cfg, 3, 1, 1, 1, 2, 8, 16)
  }
  SEGMI_UNSUPPORTED("conv3d_wgrad: no MFMA kernel for k%d s%d, channel blocking %d", ksize, stride, pl.ct);
}

}  // namespace segmi
