// conv_ks_impl.h -- K-split variant of the MFMA Conv3d forward for the deep layers (many input
// channels, few voxels: 8^3 .. 32^3 per sample).
//
// conv_fwd_impl.h gives every wave 2 voxel tiles and ALL k-steps: each of the 4 waves streams
// the same weight fragments from L2/L1 (4x redundant, 64 B/clk L1) and gets only 2 MFMAs per
// fragment to hide the next fragment's latency -- with one workgroup per CU (16^3 x 128, 8^3 x 256)
// that latency chain is the run time (45-180 TFLOP/s measured).  Here every wave owns ALL 8 voxel
// tiles of the workgroup and a quarter of the k-steps (taps w, w+4, ...): a weight fragment is
// fetched once per workgroup and feeds 8*NT MFMAs, so a one-step-ahead prefetch covers the L2
// latency.  The 4 partial accumulators are summed through LDS in fixed wave order (deterministic),
// then wave w runs the usual epilogue on voxel tiles 2w, 2w+1.
#pragma once
#include "conv_fwd_impl.h"

namespace segmi {

// Residency (workgroups per CU = waves per SIMD).  LDS: max(halo image, 24 KB * NT of exchange area), so 48 KB
// at NT = 2 and the halo image (28 - 34 KB) at NT = 1.  Registers: left to itself under __launch_bounds__(256)
// the allocator spends them freely and lands on 2 waves (1 for the several-chunk forms at NT = 2), so it is
// held to a wave count.  One chunk: 3 at NT = 2 (acc 64 + weights 56 + staging 28 leave no room for a fourth),
// 4 at NT = 1.  Several chunks (a second weight set): 2.  The narrow tile at NT = 2 with several chunks spills
// 29 registers under that budget and is left alone (298 registers, 1 wave; the parent form had 250): no
// layer of the UNet engine takes it.
constexpr int conv_ks_waves(bool one, int nt, int tw) {
  return one ? (nt == 2 ? 3 : 4) : (nt == 2 && tw == 8 ? 1 : 2);
}
template <int W> struct KsWave { static constexpr int value = W; };

template <typename T, int CK, int KS, int S, int NT, int TD, int TH, int TW, bool ONE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(conv_ks_waves(ONE, NT, TW))))
void conv_fwd_ks_kernel(ConvParams p) {
  using G = ConvGeom<T, CK, KS, S, TD, TH, TW>;
  static_assert(G::SPT == 4, "k-split kernel: one k-step per tap");
  static_assert(G::NVT == 8, "k-split kernel: 8 voxel tiles per workgroup");
  constexpr int NSW = (G::NSTEP + 3) / 4;   // k-steps per wave per chunk
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r = lane & 15;

  int t = blockIdx.x;
  const int txi = t % p.tx; t /= p.tx;
  const int tyi = t % p.ty; t /= p.ty;
  const int tzi = t % p.tz;
  const int n = t / p.tz;
  const int oz0 = tzi * TD, oy0 = tyi * TH, ox0 = txi * TW;
  const int iz0 = oz0 * S - G::PAD, iy0 = oy0 * S - G::PAD, ix0 = ox0 * S - G::PAD;
  const int nt0 = blockIdx.y * NT;

  f32x4 acc[8][NT];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int vaddr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = i * 16 + r;
    const int x = idx % TW, y = (idx / TW) % TH, z = idx / (TW * TH);
    vaddr[i] = ((z * S * G::HH + y * S) * G::HW + x * S) * G::ROWB + g * 16;
  }
  // LDS offsets of this wave's taps
  int tapoff[NSW];
#pragma unroll
  for (int si = 0; si < NSW; ++si) {
    int tap = wave + 4 * si;
    if (tap > G::NTAPS - 1) tap = G::NTAPS - 1;
    tapoff[si] = (((tap / (KS * KS)) * G::HH + (tap / KS) % KS) * G::HW + tap % KS) * G::ROWB;
  }

  constexpr int NCH = G::HD * G::HH * G::HW * G::CPR;
  constexpr int NLD = (NCH + 255) / 256;
  const char* inb = (const char*)p.in;
  frag_t stg[NLD];
  auto fetch = [&](int c) {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int i = tid + 256 * k;
      const int v = i / G::CPR, ch = i % G::CPR;
      const int hx = v % G::HW, hy = (v / G::HW) % G::HH, hz = v / (G::HW * G::HH);
      const int z = iz0 + hz, y = iy0 + hy, x = ix0 + hx;
      stg[k] = frag_t{0u, 0u, 0u, 0u};
      if (i < NCH && (unsigned)z < (unsigned)p.Di && (unsigned)y < (unsigned)p.Hi &&
          (unsigned)x < (unsigned)p.Wi) {
        const int64_t e = ((((int64_t)n * p.Di + z) * p.Hi + y) * p.Wi + x) * p.ldi + c * CK;
        stg[k] = *reinterpret_cast<const frag_t*>(inb + e * (int64_t)sizeof(T) + ch * 16);
      }
    }
  };
  // the staged halo image -> LDS rows
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int i = tid + 256 * k;
      if (i < NCH) *reinterpret_cast<frag_t*>(smem + (i / G::CPR) * G::ROWB + (i % G::CPR) * 16) = stg[k];
    }
  };
  // this wave's weight fragments of a chunk (k-steps wave, wave+4, ...): all fetched at once, one
  // chunk ahead, so a cold L2 costs one exposed latency per kernel instead of one per k-step
  const char* wb0 = (const char*)p.wfrag + (int64_t)nt0 * 1024 + lane * 16;
  frag_t wcur[NSW][NT];
  auto fetch_w = [&](int c, auto& dst) {
#pragma unroll
    for (int si = 0; si < NSW; ++si) {
      int s = wave + 4 * si;
      if (s > G::NSTEP - 1) s = G::NSTEP - 1;
#pragma unroll
      for (int j = 0; j < NT; ++j)
        dst[si][j] = *reinterpret_cast<const frag_t*>(
            wb0 + (((int64_t)c * G::NSTEP + s) * p.ntiles_total + j) * 1024);
    }
  };
  // k-step si of this wave on the halo image
  auto kstep = [&](int si) {
    const int s = wave + 4 * si;
    if (s < G::NSTEP) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const frag_t a = *reinterpret_cast<const frag_t*>(smem + vaddr[i] + tapoff[si]);
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = mma16<T>(wcur[si][j], a, acc[i][j]);
      }
    }
  };
  fetch(0);
  fetch_w(0, wcur);
  if constexpr (ONE) {
    // one channel chunk: no next-chunk registers, no chunk loop
    commit();
    __syncthreads();
#pragma unroll
    for (int si = 0; si < NSW; ++si) kstep(si);
    __syncthreads();   // the exchange below overwrites the halo image
  } else {
    // one halo image, two barriers per chunk, the next chunk's halo and weights fetched behind the
    // second one.  (Two halo images with one barrier per chunk and the loads issued a chunk earlier
    // were built and measured: not faster on any layer, see DESIGN.md.)
    frag_t wnxt[NSW][NT];
    for (int c = 0; c < p.nchunks; ++c) {
      if (c > 0) __syncthreads();
      commit();
      __syncthreads();
      if (c + 1 < p.nchunks) {
        fetch(c + 1);
        fetch_w(c + 1, wnxt);
      }
#pragma unroll
      for (int si = 0; si < NSW; ++si) kstep(si);
#pragma unroll
      for (int si = 0; si < NSW; ++si)
#pragma unroll
        for (int j = 0; j < NT; ++j) wcur[si][j] = wnxt[si][j];
    }
    __syncthreads();   // the exchange below overwrites the halo image
  }

  // ---- fixed-order sum of the 4 waves' partial accumulators.  Wave w finishes voxel tiles 2w, 2w+1:
  // it keeps its own partial sums of those in registers and passes the other six tiles through LDS,
  // red[owner][k][tile of the owner][NT][lane] with k the writer's rank among the owner's 3 foreign
  // waves.  The area starts at smem: the halo image is dead behind the barrier above.  `wave` is
  // uniform, so each phase branches once to the copy written for that wave: every register index
  // and LDS slot is a constant (a select over the 8 tiles costs 16 more live registers).
  f32x4* red = reinterpret_cast<f32x4*>(smem);
  f32x4 fin[2][NT];
  auto put = [&](auto wc) {
    constexpr int w = decltype(wc)::value;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (d == w) continue;
      const int k = w < d ? w : w - 1;
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < NT; ++j) red[(((d * 3 + k) * 2 + ii) * NT + j) * 64 + lane] = acc[2 * d + ii][j];
    }
  };
  auto get = [&](auto wc) {
    constexpr int w = decltype(wc)::value;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        // wave order 0 + 1 + 2 + 3, the own partial at position w
        f32x4 part[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
          part[s] = s == w ? acc[2 * w + ii][j]
                           : red[(((w * 3 + (s < w ? s : s - 1)) * 2 + ii) * NT + j) * 64 + lane];
        f32x4 v = part[0];
        v += part[1];
        v += part[2];
        v += part[3];
        fin[ii][j] = v;
      }
  };
  switch (wave) {
    case 0: put(KsWave<0>{}); break;
    case 1: put(KsWave<1>{}); break;
    case 2: put(KsWave<2>{}); break;
    default: put(KsWave<3>{});
  }
  __syncthreads();
  switch (wave) {
    case 0: get(KsWave<0>{}); break;
    case 1: get(KsWave<1>{}); break;
    case 2: get(KsWave<2>{}); break;
    default: get(KsWave<3>{});
  }

  // ---- epilogue (as conv_fwd_impl.h): wave w owns voxel tiles 2w, 2w+1
  f32x4 bias4[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    bias4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p.bias) bias4[j] = *reinterpret_cast<const f32x4*>(p.bias + (nt0 + j) * 16 + 4 * g);
  }
  const bool has_alpha = p.alpha != nullptr;
  const float alpha = has_alpha ? *p.alpha : 0.f;
  f32x4 ssum[NT], ssq[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    ssum[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    ssq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  T* outp = (T*)p.out;
  const T* resp = (const T*)p.res;
  f32x4 resv[2][NT];
  if (resp) {
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const int idx = (wave * 2 + ii) * 16 + r;
      const int oz = oz0 + idx / (TW * TH), oy = oy0 + (idx / TW) % TH, ox = ox0 + idx % TW;
      const bool valid = oz < p.Do && oy < p.Ho && ox < p.Wo;
      const int64_t vox = (((int64_t)n * p.Do + oz) * p.Ho + oy) * p.Wo + ox;
#pragma unroll
      for (int j = 0; j < NT; ++j)
        resv[ii][j] = valid ? load4<T>(resp + vox * p.ldr + (nt0 + j) * 16 + 4 * g)
                            : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < NT; ++j) touch_v(resv[ii][j]);
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) touch_v(bias4[j]);
#pragma unroll
  for (int k = 0; k < NLD; ++k) touch_v(stg[k]);
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    const int idx = (wave * 2 + ii) * 16 + r;
    const int oz = oz0 + idx / (TW * TH), oy = oy0 + (idx / TW) % TH, ox = ox0 + idx % TW;
    const bool valid = oz < p.Do && oy < p.Ho && ox < p.Wo;
    const int64_t vox = (((int64_t)n * p.Do + oz) * p.Ho + oy) * p.Wo + ox;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      f32x4 v = fin[ii][j] + bias4[j];
      if (valid) {
        if (p.stats) {
          ssum[j] += v;
          ssq[j] += v * v;
        }
        if (has_alpha) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : alpha * v[e];
        }
        const int co = (nt0 + j) * 16 + 4 * g;
        if (resp) v += resv[ii][j];
        store4<T>(outp + vox * p.ldo + co, v);
      }
    }
  }
  if (p.stats) {
    __syncthreads();  // everyone is done with the partial sums
    float* rs = reinterpret_cast<float*>(smem);  // [wave][2][NT*16]
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = row16_sum(ssum[j][e]);
        const float b = row16_sum(ssq[j][e]);
        if (r == 0) {
          rs[(wave * 2 + 0) * NT * 16 + j * 16 + 4 * g + e] = a;
          rs[(wave * 2 + 1) * NT * 16 + j * 16 + 4 * g + e] = b;
        }
      }
    __syncthreads();
    if (tid < 2 * NT * 16) {
      const int which = tid / (NT * 16), ch = tid % (NT * 16);
      float sacc = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) sacc += rs[(w * 2 + which) * NT * 16 + ch];
      fin_store(&p.stats[((int64_t)blockIdx.x * 2 + which) * p.Cout + nt0 * 16 + ch], sacc);
    }
    fin_tail_run<BnFin, 256, offsetof(ConvParams, ft), offsetof(ConvParams, bfin)>(p.stats, smem);
  }
}

template <typename T, int CK, int KS, int S, int NT, int TD, int TH, int TW, bool ONE>
static int launch_conv_ks_one(ConvParams p, const ConvPlan& pl, hipStream_t st) {
  using G = ConvGeom<T, CK, KS, S, TD, TH, TW>;
  p.tz = pl.tz; p.ty = pl.ty; p.tx = pl.tx;
  SEGMI_CHECK_ARG(TD == pl.td && TH == pl.th && TW == pl.tw && pl.grid_x > 0 && (int64_t)p.N * p.tz * p.ty * p.tx == pl.grid_x,
                  "conv3d: too many tiles, or the k-split kernel's grid is not the planned one");
  dim3 grid((unsigned)pl.grid_x, (unsigned)(p.Cout / (16 * NT)));
  constexpr int red = 4 * 3 * 2 * NT * 64 * 16;                 // 6 foreign tiles per wave
  constexpr int lds0 = G::LDS_BYTES > red ? G::LDS_BYTES : red;
  p.fin_on = p.fin_on && p.stats;
  const size_t lds = fin_tail_arm(p, grid, 256, 2 * p.Cout, lds0);
  return launch_wg256<conv_fwd_ks_kernel<T, CK, KS, S, NT, TD, TH, TW, ONE>>(grid, lds, lds > 64 * 1024, st,
                                                                            "conv3d_fwd(mfma, k-split)", p);
}

// a layer of one channel chunk takes the form without next-chunk registers and chunk loop
template <typename T, int CK, int KS, int S, int NT, int TD, int TH, int TW>
static int launch_conv_ks_cfg(const ConvParams& p, const ConvPlan& pl, hipStream_t st) {
  return p.nchunks == 1 ? launch_conv_ks_one<T, CK, KS, S, NT, TD, TH, TW, true>(p, pl, st)
                        : launch_conv_ks_one<T, CK, KS, S, NT, TD, TH, TW, false>(p, pl, st);
}

// the k-split kernel's instantiation of a plan: output tiles per workgroup x tile width (conv_ks_tile_shape)
template <typename T, int CK>
static int launch_conv_ks(const ConvParams& p, const ConvPlan& pl, hipStream_t st) {
#define KS_CASE(NT, WIDE)                                                          \
  case NT * 32 + conv_ks_tile_shape(WIDE).tw: {                                    \
    constexpr Tile3 t = conv_ks_tile_shape(WIDE);                                  \
    return launch_conv_ks_cfg<T, CK, 3, 1, NT, t.td, t.th, t.tw>(p, pl, st);       \
  }
  switch (pl.nt * 32 + pl.tw) { KS_CASE(2, true) KS_CASE(2, false) KS_CASE(1, true) KS_CASE(1, false) }
#undef KS_CASE
  SEGMI_UNSUPPORTED("conv3d: no k-split kernel of %d output tiles per workgroup", pl.nt);
}

}  // namespace segmi
