// degrade.hip -- the `augment_degrade` training augmentation (not in the reference):
// additive Gaussian noise, Gaussian blur, a brightness multiplier and simulated low resolution on the
// sampler's dense f32 NDHWC patches [count][rd][rh][rw][c], in that order, one draw per patch shared by
// its channels.
//   * blur and lowres are the only out-of-place steps (patches <-> workspace);
//   * noise is a pure function of (seed, element index) and is added where the first step loads a value
//     (a blur halo or a lowres tap recomputes it), brightness multiplies where the last step stores;
//   * a patch with neither blur nor lowres takes one in-place elementwise pass.
// A patch therefore costs at most two read + write passes; only selected patches are touched.
#include "common.h"

#include <math.h>

namespace segmi {

constexpr int kMaxPatches = 16;
constexpr int kMaxRadius = 8;        // R = floor(4 sigma + 0.5) <= 8, i.e. sigma <= 2.0

// ---- the noise field: Box-Muller over a counter hash, k = 2 e + j in uint32 arithmetic
__device__ __forceinline__ uint32_t degrade_hash(uint32_t k, uint32_t seed) {
  uint32_t h = k * 0x9E3779B1u ^ seed;
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ float degrade_gauss(uint32_t seed, uint32_t e) {
  const uint32_t h0 = degrade_hash(2u * e, seed), h1 = degrade_hash(2u * e + 1u, seed);
  const float u1 = (float)((h0 >> 8) + 1u) * 0x1p-24f;      // (0, 1]
  const float u2 = (float)(h1 >> 8) * 0x1p-24f;             // [0, 1): 2 u2 is exact
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// what the first step adds at its loads and the last step multiplies at its stores, per slot; a slot is
// one selected patch of the launch (`patch` = its index in the call)
struct DegradeSlots {
  int n;
  unsigned char patch[kMaxPatches];
  unsigned char noise[kMaxPatches], bright[kMaxPatches];
  uint32_t seed[kMaxPatches];
  float sd[kMaxPatches];      // sqrt(variance)
  float mult[kMaxPatches];
};

// ---- neither blur nor lowres: x = (x + sd g) * mult in place, four consecutive elements per thread; VEC: as one
// 16-byte access (every patch base 16-byte aligned and the patch a multiple of four elements long)
template <bool VEC>
__global__ __launch_bounds__(256) void degrade_pointwise_kernel(float* __restrict__ x, int64_t per, DegradeSlots s) {
  const int slot = blockIdx.y;
  const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= per) return;
  float* q = x + (int64_t)s.patch[slot] * per + e0;
  const bool noise = s.noise[slot], bright = s.bright[slot];
  const uint32_t seed = s.seed[slot];
  const float sd = s.sd[slot], mult = s.mult[slot];
  const int n = VEC ? 4 : (per - e0 < 4 ? (int)(per - e0) : 4);
  f32x4 v;
  if constexpr (VEC) {
    v = *reinterpret_cast<const f32x4*>(q);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < n ? q[k] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (noise) v[k] += sd * degrade_gauss(seed, (uint32_t)(e0 + k));
    if (bright) v[k] *= mult;
  }
  if constexpr (VEC) {
    *reinterpret_cast<f32x4*>(q) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) q[k] = v[k];
  }
}

// ---- workspace -> patches for the patches that took one out-of-place step only
template <bool VEC>
__global__ __launch_bounds__(256) void degrade_copy_back_kernel(const float* __restrict__ ws, float* __restrict__ x,
                                                                int64_t per, DegradeSlots s) {
  const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= per) return;
  const int64_t at = (int64_t)s.patch[blockIdx.y] * per + e0;
  if constexpr (VEC) {
    *reinterpret_cast<f32x4*>(x + at) = *reinterpret_cast<const f32x4*>(ws + at);
  } else {
    for (int k = 0; k < 4 && e0 + k < per; ++k) x[at + k] = ws[at + k];
  }
}

// ---- blur: separable Gaussian, scipy's `reflect` border, one tile plus its halo staged in LDS
struct BlurSlots {
  DegradeSlots s;
  float w[kMaxPatches][2 * kMaxRadius + 1];     // w[k + R], k = -R..R, normalised
};

// scipy.ndimage "reflect" (d c b a | a b c d | d c b a) for any integer i
__device__ __forceinline__ int reflect_index(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

// The tile of one workgroup by radius: with its halo and the z-pass buffer it fits 64 KB of LDS (60 KB at R = 4 and
// at R = 8).  FLAT = a patch of depth 1 (a 2-D network): no z halo and no z pass.
template <int R, bool FLAT> struct BlurShape {
  static constexpr int TZ = FLAT ? 1 : (R <= 4 ? 8 : 4), TY = FLAT ? 16 : (R <= 4 ? 8 : 4),
                       TX = FLAT ? 64 : (R <= 4 ? 32 : 16);
  static constexpr int RZ = FLAT ? 0 : R;
  static constexpr int LZ = TZ + 2 * RZ, LY = TY + 2 * R, LX = TX + 2 * R, PLANE = LY * LX;
  static constexpr int NA = LZ * PLANE, NB = TZ * PLANE;    // floats of the two LDS buffers
};

// One workgroup = one tile of one channel of one patch; the radius is a template parameter (one launch per radius
// that occurs in a call), so the weights sit in registers and every pass is unrolled.  A holds the tile with its
// halo.  z pass: a thread owns a (y, x) column of A, reads it once and writes its TZ sums to B.  y pass: a thread
// owns a (z, x) column of B and writes TY sums back into A.  x pass: a thread owns an output voxel.  Lanes run along
// x in every pass.  An in-plane axis of extent 1 is not special-cased: reflect maps every tap to its one voxel, and
// the weights sum to 1 within an f32 rounding.
template <int R, bool FLAT>
__global__ __launch_bounds__(256) void degrade_blur_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           int rd, int rh, int rw, int c, int ntx, int nty,
                                                           BlurSlots p) {
  using S = BlurShape<R, FLAT>;
  constexpr int TZ = S::TZ, TY = S::TY, TX = S::TX, RZ = S::RZ, LZ = S::LZ, LY = S::LY, LX = S::LX, PLANE = S::PLANE;
  constexpr int NP = (PLANE + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  float* A = reinterpret_cast<float*>(dsm);
  float* B = A + S::NA;
  const int slot = blockIdx.y, ch = blockIdx.z, tid = threadIdx.x;
  // a patch holds fewer than 2^31 elements: element indices fit 32 bits
  const int64_t per = (int64_t)rd * rh * rw * c;
  const float* in = src + (int64_t)p.s.patch[slot] * per;
  float* out = dst + (int64_t)p.s.patch[slot] * per;
  int tile = blockIdx.x;
  const int x0 = (tile % ntx) * TX; tile /= ntx;
  const int y0 = (tile % nty) * TY;
  const int z0 = (tile / nty) * TZ;
  float w[2 * R + 1];
#pragma unroll
  for (int k = 0; k <= 2 * R; ++k) w[k] = p.w[slot][k];
  const bool noise = p.s.noise[slot];
  const uint32_t seed = p.s.seed[slot];
  const float sd = p.s.sd[slot];

  // load: thread tid owns the plane positions tid, tid + 256, ...; their in-plane source offsets are fixed
  int off[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int q = tid + 256 * j;
    const int ly = q / LX, lx = q % LX;
    off[j] = (reflect_index(y0 + ly - R, rh) * rw + reflect_index(x0 + lx - R, rw)) * c + ch;
  }
  const int zstride = rh * rw * c;
  for (int lz = 0; lz < LZ; ++lz) {
    const int base = reflect_index(z0 + lz - RZ, rd) * zstride;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int q = tid + 256 * j;
      if (q < PLANE) {
        const int e = base + off[j];
        float v = in[e];
        if (noise) v += sd * degrade_gauss(seed, (uint32_t)e);
        A[lz * PLANE + q] = v;
      }
    }
  }
  __syncthreads();
  // z: A [LZ][LY][LX] -> B [TZ][LY][LX]
  if constexpr (RZ > 0) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int q = tid + 256 * j;
      if (q < PLANE) {
        float acc[TZ];
#pragma unroll
        for (int z = 0; z < TZ; ++z) acc[z] = 0.f;
#pragma unroll
        for (int kk = 0; kk < LZ; ++kk) {
          const float a = A[kk * PLANE + q];
#pragma unroll
          for (int z = 0; z < TZ; ++z)
            if (kk - z >= 0 && kk - z <= 2 * R) acc[z] += w[kk - z] * a;
        }
#pragma unroll
        for (int z = 0; z < TZ; ++z) B[z * PLANE + q] = acc[z];
      }
    }
    __syncthreads();
  }
  // y: [TZ][LY][LX] -> [TZ][TY][LX]; from B into A behind a z pass, else from A into B
  const float* ysrc = RZ > 0 ? B : A;
  float* ydst = RZ > 0 ? A : B;
  constexpr int NC = TZ * LX;
#pragma unroll
  for (int j = 0; j < (NC + 255) / 256; ++j) {
    const int q = tid + 256 * j;
    if (q < NC) {
      const int z = q / LX, lx = q % LX;
      float acc[TY];
#pragma unroll
      for (int y = 0; y < TY; ++y) acc[y] = 0.f;
#pragma unroll
      for (int kk = 0; kk < LY; ++kk) {
        const float a = ysrc[z * PLANE + kk * LX + lx];
#pragma unroll
        for (int y = 0; y < TY; ++y)
          if (kk - y >= 0 && kk - y <= 2 * R) acc[y] += w[kk - y] * a;
      }
#pragma unroll
      for (int y = 0; y < TY; ++y) ydst[(z * TY + y) * LX + lx] = acc[y];
    }
  }
  __syncthreads();
  // x: [TZ][TY][LX] -> the tile's voxels inside the patch
  const bool bright = p.s.bright[slot];
  const float mult = p.s.mult[slot];
  constexpr int NO = TZ * TY * TX;
#pragma unroll
  for (int j = 0; j < (NO + 255) / 256; ++j) {
    const int o = tid + 256 * j;
    const int x = o % TX, y = (o / TX) % TY, z = o / (TX * TY);
    const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
    if (o >= NO || gz >= rd || gy >= rh || gx >= rw) continue;
    const float* a = ydst + (z * TY + y) * LX + x;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) acc += w[k] * a[k];
    if (bright) acc *= mult;
    out[((gz * rh + gy) * rw + gx) * c + ch] = acc;
  }
}

template <int R>
static void launch_blur(const float* src, float* dst, int rd, int rh, int rw, int c, const BlurSlots& bs,
                        hipStream_t st) {
  if (rd == 1) {
    using S = BlurShape<R, true>;
    const int nty = cdiv(rh, S::TY), ntx = cdiv(rw, S::TX);
    hipLaunchKernelGGL((degrade_blur_kernel<R, true>), dim3((unsigned)(nty * ntx), bs.s.n, c), 256,
                       (size_t)(S::NA + S::NB) * sizeof(float), st, src, dst, rd, rh, rw, c, ntx, nty, bs);
  } else {
    using S = BlurShape<R, false>;
    const int ntz = cdiv(rd, S::TZ), nty = cdiv(rh, S::TY), ntx = cdiv(rw, S::TX);
    hipLaunchKernelGGL((degrade_blur_kernel<R, false>), dim3((unsigned)(ntz * nty * ntx), bs.s.n, c), 256,
                       (size_t)(S::NA + S::NB) * sizeof(float), st, src, dst, rd, rh, rw, c, ntx, nty, bs);
  }
}

// ---- lowres: nearest down onto a coarse grid, linear back up, as one gather of at most 8 taps
struct LowresSlots {
  DegradeSlots s;
  unsigned char from_ws[kMaxPatches];   // the blur ran first: read the workspace, write the patches
  int m[kMaxPatches][3];                // coarse extents (z, y, x)
};
constexpr int kLowresChunk = 4096;       // elements per workgroup

__device__ __forceinline__ float lowres_mix(float a, float b, float f) { return f == 0.f ? a : a + f * (b - a); }

// Per axis and fine index i the two source voxels and the fraction are tabulated in LDS by every workgroup:
// with N = (2 i + 1) m - n clamped to [0, 2 n (m - 1)], t = N / 2n, j0 = min(N div 2n, max(m - 2, 0)),
// f = (N - 2n j0) / 2n in integers until the last division; src(j) = ((2 j + 1) n) div (2 m).  An axis
// with m == n passes through (one tap, f = 0).
__global__ __launch_bounds__(256) void degrade_lowres_kernel(float* __restrict__ patches, float* __restrict__ ws,
                                                             int rd, int rh, int rw, int c, LowresSlots p) {
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  const int ntab = rd + rh + rw;
  int* s0 = reinterpret_cast<int*>(dsm);
  int* s1 = s0 + ntab;
  float* fr = reinterpret_cast<float*>(s1 + ntab);
  const int slot = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < ntab; i += 256) {
    const int a = i < rd ? 0 : (i < rd + rh ? 1 : 2);
    const int idx = a == 0 ? i : (a == 1 ? i - rd : i - rd - rh);
    const int64_t n = a == 0 ? rd : (a == 1 ? rh : rw), m = p.m[slot][a];
    int v0 = idx, v1 = idx;
    float f = 0.f;
    if (m != n) {
      int64_t N = (2 * (int64_t)idx + 1) * m - n;
      const int64_t hi = 2 * n * (m - 1);
      N = N < 0 ? 0 : (N > hi ? hi : N);
      int64_t j0 = N / (2 * n);
      const int64_t cap = m >= 2 ? m - 2 : 0;
      if (j0 > cap) j0 = cap;
      const int64_t j1 = j0 + 1 < m ? j0 + 1 : m - 1;
      f = (float)(N - 2 * n * j0) / (float)(2 * n);
      v0 = (int)(((2 * j0 + 1) * n) / (2 * m));
      v1 = (int)(((2 * j1 + 1) * n) / (2 * m));
    }
    s0[i] = v0; s1[i] = v1; fr[i] = f;
  }
  __syncthreads();
  const int64_t per = (int64_t)rd * rh * rw * c;
  const int64_t base = (int64_t)p.s.patch[slot] * per;
  const float* in = (p.from_ws[slot] ? ws : patches) + base;
  float* out = (p.from_ws[slot] ? patches : ws) + base;
  const bool noise = p.s.noise[slot], bright = p.s.bright[slot];
  const uint32_t seed = p.s.seed[slot];
  const float sd = p.s.sd[slot], mult = p.s.mult[slot];
  for (int k = 0; k < kLowresChunk / 256; ++k) {
    const int64_t e = (int64_t)blockIdx.x * kLowresChunk + k * 256 + tid;
    if (e >= per) break;
    const int ch = (int)(e % c);
    int64_t v = e / c;
    const int x = (int)(v % rw); v /= rw;
    const int y = (int)(v % rh);
    const int z = (int)(v / rh);
    const int zs[2] = {s0[z], s1[z]}, ys[2] = {s0[rd + y], s1[rd + y]}, xs[2] = {s0[rd + rh + x], s1[rd + rh + x]};
    const float fz = fr[z], fy = fr[rd + y], fx = fr[rd + rh + x];
    auto tap = [&](int zz, int yy, int xx) {
      const int64_t ee = (((int64_t)zz * rh + yy) * rw + xx) * c + ch;
      float val = in[ee];
      if (noise) val += sd * degrade_gauss(seed, (uint32_t)ee);
      return val;
    };
    float vz[2] = {0.f, 0.f};
#pragma unroll
    for (int bz = 0; bz < 2; ++bz) {
      if (bz == 1 && fz == 0.f) continue;
      float vy[2] = {0.f, 0.f};
#pragma unroll
      for (int by = 0; by < 2; ++by) {
        if (by == 1 && fy == 0.f) continue;
        float a = tap(zs[bz], ys[by], xs[0]);
        if (fx != 0.f) a = lowres_mix(a, tap(zs[bz], ys[by], xs[1]), fx);
        vy[by] = a;
      }
      vz[bz] = lowres_mix(vy[0], vy[1], fy);
    }
    float r = lowres_mix(vz[0], vz[1], fz);
    if (bright) r *= mult;
    out[e] = r;
  }
}

static inline bool any_on(const uint8_t* on, int count) {
  if (!on) return false;
  for (int i = 0; i < count; ++i) if (on[i]) return true;
  return false;
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int64_t segmi_degrade_workspace(int count, int rd, int rh, int rw, int c) {
  if (count <= 0 || rd <= 0 || rh <= 0 || rw <= 0 || c <= 0) return 0;
  return (int64_t)count * rd * rh * rw * c * 4;
}

int segmi_degrade_augment(float* patches, int count, int rd, int rh, int rw, int c,
                          const uint8_t* noise_on_host, const float* variance_host, const uint32_t* seed_host,
                          const uint8_t* blur_on_host, const float* sigma_host,
                          const uint8_t* bright_on_host, const float* multiplier_host,
                          const uint8_t* lowres_on_host, const int32_t* coarse_host, void* workspace,
                          void* stream) {
  SEGMI_CHECK_ARG(patches && count > 0 && count <= kMaxPatches && rd > 0 && rh > 0 && rw > 0 && c > 0,
                  "degrade_augment: bad arguments (1..%d patches)", kMaxPatches);
  // the noise counter k = 2 e + j is 32 bits wide
  SEGMI_CHECK_ARG((double)rd * rh * rw * c < 2147483648.0 && c <= 65535,
                  "degrade_augment: a patch holds fewer than 2^31 elements and at most 65535 channels");
  SEGMI_CHECK_ARG((!noise_on_host || (variance_host && seed_host)) && (!blur_on_host || sigma_host) &&
                      (!bright_on_host || multiplier_host) && (!lowres_on_host || coarse_host),
                  "degrade_augment: missing parameter array");
  const int ext[3] = {rd, rh, rw};
  // per patch: what fires.  A lowres whose coarse grid is the fine grid on every axis is the identity: off.
  bool noise[kMaxPatches], blur[kMaxPatches], bright[kMaxPatches], lowres[kMaxPatches];
  int radius[kMaxPatches] = {0};
  bool any_oop = false, any = false;
  for (int i = 0; i < count; ++i) {
    noise[i] = noise_on_host && noise_on_host[i];
    blur[i] = blur_on_host && blur_on_host[i];
    bright[i] = bright_on_host && bright_on_host[i];
    lowres[i] = lowres_on_host && lowres_on_host[i];
    if (noise[i])
      SEGMI_CHECK_ARG(variance_host[i] >= 0.f && isfinite(variance_host[i]),
                      "degrade_augment: noise variance %g of patch %d (finite and >= 0)", (double)variance_host[i], i);
    if (bright[i])
      SEGMI_CHECK_ARG(isfinite(multiplier_host[i]), "degrade_augment: brightness multiplier of patch %d is not finite", i);
    if (blur[i]) {
      const double sg = (double)sigma_host[i];
      SEGMI_CHECK_ARG(sg > 0.0 && isfinite(sg) && floor(4.0 * sg + 0.5) <= (double)kMaxRadius,
                      "degrade_augment: blur sigma %g of patch %d (0 < sigma, radius floor(4 sigma + 0.5) <= %d)",
                      sg, i, kMaxRadius);
      radius[i] = (int)floor(4.0 * sg + 0.5);
      if (radius[i] == 0) blur[i] = false;       // sigma < 0.125: the one weight is 1, the identity
    }
    if (lowres[i]) {
      bool same = true;
      for (int a = 0; a < 3; ++a) {
        const int m = coarse_host[3 * i + a];
        SEGMI_CHECK_ARG(m >= 1 && m <= ext[a], "degrade_augment: lowres coarse extent %d of patch %d, axis %d "
                        "(1..%d)", m, i, a, ext[a]);
        same = same && m == ext[a];
      }
      if (same) lowres[i] = false;
    }
    any_oop = any_oop || blur[i] || lowres[i];
    any = any || noise[i] || blur[i] || bright[i] || lowres[i];
  }
  if (!any) return SEGMI_OK;
  SEGMI_CHECK_ARG(!any_oop || workspace, "degrade_augment: blur and lowres need the workspace "
                  "(segmi_degrade_workspace bytes)");
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = (int64_t)rd * rh * rw * c;
  float* ws = (float*)workspace;
  auto fill = [&](DegradeSlots& s, int i, bool with_noise, bool with_bright) {
    const int k = s.n++;
    s.patch[k] = (unsigned char)i;
    s.noise[k] = with_noise && noise[i];
    s.bright[k] = with_bright && bright[i];
    s.seed[k] = noise[i] ? seed_host[i] : 0u;
    s.sd[k] = noise[i] ? (float)sqrt((double)variance_host[i]) : 0.f;
    s.mult[k] = bright[i] ? multiplier_host[i] : 1.f;
    return k;
  };
  const unsigned gx = (unsigned)cdiv64(per, 1024);
  // 16-byte accesses in the pointwise and copy kernels: every patch of both buffers starts 16-byte aligned
  const bool vec = per % 4 == 0 && (uintptr_t)patches % 16 == 0 && (uintptr_t)workspace % 16 == 0;

  // 1. blur: patches -> workspace, the noise added at the loads; the brightness at the stores unless lowres follows.
  // One launch per radius that occurs.
  for (int R = 1; R <= kMaxRadius; ++R) {
    BlurSlots bs{};
    for (int i = 0; i < count; ++i) {
      if (!blur[i] || radius[i] != R) continue;
      const int k = fill(bs.s, i, true, !lowres[i]);
      const double sg = (double)sigma_host[i];
      double w[2 * kMaxRadius + 1], sum = 0.0;
      for (int j = -R; j <= R; ++j) sum += (w[j + R] = exp(-(double)(j * j) / (2.0 * sg * sg)));
      for (int j = 0; j <= 2 * R; ++j) bs.w[k][j] = (float)(w[j] / sum);
    }
    if (!bs.s.n) continue;
    switch (R) {
      case 1: launch_blur<1>(patches, ws, rd, rh, rw, c, bs, st); break;
      case 2: launch_blur<2>(patches, ws, rd, rh, rw, c, bs, st); break;
      case 3: launch_blur<3>(patches, ws, rd, rh, rw, c, bs, st); break;
      case 4: launch_blur<4>(patches, ws, rd, rh, rw, c, bs, st); break;
      case 5: launch_blur<5>(patches, ws, rd, rh, rw, c, bs, st); break;
      case 6: launch_blur<6>(patches, ws, rd, rh, rw, c, bs, st); break;
      case 7: launch_blur<7>(patches, ws, rd, rh, rw, c, bs, st); break;
      default: launch_blur<8>(patches, ws, rd, rh, rw, c, bs, st); break;
    }
  }

  // 2. lowres: workspace -> patches behind a blur, else patches -> workspace with the noise added at the taps
  LowresSlots ls{};
  for (int i = 0; i < count; ++i) {
    if (!lowres[i]) continue;
    const int k = fill(ls.s, i, !blur[i], true);
    ls.from_ws[k] = blur[i];
    for (int a = 0; a < 3; ++a) ls.m[k][a] = coarse_host[3 * i + a];
  }
  if (ls.s.n) {
    const size_t lds = (size_t)(rd + rh + rw) * 12;
    SEGMI_CHECK_ARG(lds <= 48 * 1024, "degrade_augment: lowres takes patch extents that sum to at most 4096");
    hipLaunchKernelGGL(degrade_lowres_kernel, dim3((unsigned)cdiv64(per, kLowresChunk), ls.s.n), 256, lds, st, patches,
                       ws, rd, rh, rw, c, ls);
  }

  // 3. one out-of-place step only: the result is in the workspace
  DegradeSlots cs{};
  for (int i = 0; i < count; ++i)
    if (blur[i] != lowres[i]) fill(cs, i, false, false);
  if (cs.n) {
    if (vec) hipLaunchKernelGGL(degrade_copy_back_kernel<true>, dim3(gx, cs.n), 256, 0, st, ws, patches, per, cs);
    else hipLaunchKernelGGL(degrade_copy_back_kernel<false>, dim3(gx, cs.n), 256, 0, st, ws, patches, per, cs);
  }

  // 4. neither: noise and brightness in one in-place pass
  DegradeSlots ps{};
  for (int i = 0; i < count; ++i)
    if (!blur[i] && !lowres[i] && (noise[i] || bright[i])) fill(ps, i, true, true);
  if (ps.n) {
    if (vec) hipLaunchKernelGGL(degrade_pointwise_kernel<true>, dim3(gx, ps.n), 256, 0, st, patches, per, ps);
    else hipLaunchKernelGGL(degrade_pointwise_kernel<false>, dim3(gx, ps.n), 256, 0, st, patches, per, ps);
  }
  SEGMI_LAUNCH_CHECK("degrade_augment");
  return SEGMI_OK;
}

}  // extern "C"
