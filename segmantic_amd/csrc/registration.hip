// registration.hip -- the kernels of rigid / affine registration by mutual information:
// the block-mean pyramid level, the fixed image's bin volume, and the joint intensity histogram of a fixed
// volume and a moving volume interpolated under up to 32 candidate transforms in one launch.  Every sum that
// crosses lanes is an integer (sample weights are fixed point, unit 2^16), so a table does not depend on launch
// shape or arrival order.  Built with -ffp-contract=off: index map, trilinear weights and the bin coordinate are
// specified operation by operation in float64.
//
// segmi_joint_histogram: grid (x = voxel blocks under SEGMI_JOINT_HIST_GRID_CAP, y = candidate groups).  A
// workgroup keeps ONE table of 32-bit counters per candidate of its group in LDS (kJointHistLdsCounters in all)
// and strides over the fixed voxels; a voxel's bin is loaded once and serves every candidate of the group.  One
// trip of the stride loop adds at most 256 samples * 2^16 = 2^24 to a counter, so the table is flushed into the
// global int64 table (device-scope integer atomics) every kJointHistFlushTrips = 128 trips (<= 2^31 per counter)
// and at the end.  No wave-private copies: LDS executes one wave's atomic instruction at a time, so copies
// remove no same-cell serialisation inside a wave (where a smooth image puts it) and would cut the group to a
// quarter, i.e. four times the passes over the fixed bins and the index arithmetic.
#include "common.h"

namespace segmi {

constexpr int kJointHistMaxCandidates = 32;
constexpr int kJointHistLdsCounters = 8192;   // 32 KB of u32: 32 / 8 / 2 candidates at 16 / 32 / 64 bins
constexpr int kJointHistFlushTrips = 128;     // 128 trips * 256 lanes * 2^16 = 2^31 < 2^32
constexpr int kBinShrinkGridCap = SEGMI_BIN_SHRINK_GRID_CAP;
constexpr int kJointHistGridCap = SEGMI_JOINT_HIST_GRID_CAP;

typedef unsigned long long u64;

static inline int joint_hist_group(int bins) {
  if (bins != 16 && bins != 32 && bins != 64) return 0;
  const int g = kJointHistLdsCounters / (bins * bins);
  return g > kJointHistMaxCandidates ? kJointHistMaxCandidates : g;
}

// ------------------------------------------------------------------ pyramid level
struct ShrinkParams {
  const void* src;
  float* dst;
  int sx, sy, sz, dx, dy, dz, fx, fy, fz;
};

template <typename P>
__global__ __launch_bounds__(256) void bin_shrink_kernel(ShrinkParams p) {
  const P* __restrict__ src = (const P*)p.src;
  const int64_t total = (int64_t)p.dx * p.dy * p.dz;
  const double count = (double)(p.fx * p.fy * p.fz);
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int ox = e % p.dx;
    const int oy = (e / p.dx) % p.dy;
    const int oz = e / ((int64_t)p.dx * p.dy);
    double s = 0.0;
    for (int z = 0; z < p.fz; ++z)
      for (int y = 0; y < p.fy; ++y) {
        const P* row = src + ((int64_t)(oz * p.fz + z) * p.sy + (oy * p.fy + y)) * p.sx + (int64_t)ox * p.fx;
        for (int x = 0; x < p.fx; ++x) s = s + (double)row[x];
      }
    p.dst[e] = (float)(s / count);
  }
}

// ------------------------------------------------------------------ fixed bins
__global__ __launch_bounds__(256) void fixed_bins_kernel(const float* __restrict__ img, const float* __restrict__ mask,
                                                          int64_t n, double lo, double scale, int bins,
                                                          uint8_t* __restrict__ out) {
  const double top = (double)(bins - 1);
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    double b = floor(((double)img[e] - lo) * scale + 0.5);
    b = b > 0.0 ? b : 0.0;          // a NaN voxel lands in bin 0
    b = b < top ? b : top;
    uint8_t v = (uint8_t)(int)b;
    if (mask && mask[e] < 0.5f) v = 255;
    out[e] = v;
  }
}

// ------------------------------------------------------------------ joint histogram
struct JointHistParams {
  const uint8_t* fbin;
  const void* mov;
  u64* out;
  int fx, fy, fz, mx, my, mz;
  int T, bins, group;
  double mlo, mscale;
  double m[kJointHistMaxCandidates][12];   // fixed index (x,y,z,1) -> continuous moving index (x,y,z)
};

// table [group][B][B] of the workgroup added into the global one and cleared; every lane calls it
__device__ __forceinline__ void joint_hist_flush(unsigned* lds, u64* __restrict__ out, int entries) {
  __syncthreads();
  for (int e = threadIdx.x; e < entries; e += 256) {
    const unsigned v = lds[e];
    if (v) {
      atomicAdd(&out[e], (u64)v);
      lds[e] = 0;
    }
  }
  __syncthreads();
}

template <typename P>
__global__ __launch_bounds__(256) void joint_hist_kernel(JointHistParams p) {
  __shared__ unsigned lds[kJointHistLdsCounters];
  const P* __restrict__ mov = (const P*)p.mov;
  const int B = p.bins, BB = B * B;
  const int t0 = blockIdx.y * p.group;
  const int gcount = p.T - t0 < p.group ? p.T - t0 : p.group;
  const int entries = gcount * BB;                       // <= kJointHistLdsCounters by the choice of group
  u64* __restrict__ out = p.out + (int64_t)t0 * BB;
  for (int e = threadIdx.x; e < entries; e += 256) lds[e] = 0;
  __syncthreads();

  const int64_t total = (int64_t)p.fx * p.fy * p.fz;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t trips = (total + stride - 1) / stride;   // the same for every lane: the flushes hold barriers
  const double hx = (double)(p.mx - 1), hy = (double)(p.my - 1), hz = (double)(p.mz - 1);
  const double top = (double)(B - 1);
  int since = 0;
  for (int64_t trip = 0; trip < trips; ++trip) {
    const int64_t e = trip * stride + blockIdx.x * 256ll + threadIdx.x;
    int fb = 255;
    if (e < total) fb = p.fbin[e];
    if (fb < B) {                                        // 255 = ignore; B .. 254 never index the table
      const double x = (double)(int)(e % p.fx);
      const double y = (double)(int)((e / p.fx) % p.fy);
      const double z = (double)(int)(e / ((int64_t)p.fx * p.fy));
      for (int g = 0; g < gcount; ++g) {
        const double* m = p.m[t0 + g];
        const double cx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
        const double cy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
        const double cz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        if (!(cx >= 0.0 && cx <= hx && cy >= 0.0 && cy <= hy && cz >= 0.0 && cz <= hz)) continue;
        const double fx0 = floor(cx), fy0 = floor(cy), fz0 = floor(cz);
        const int x0 = (int)fx0, y0 = (int)fy0, z0 = (int)fz0;
        const double fx = cx - fx0, fy = cy - fy0, fz = cz - fz0;
        const int x1 = x0 + 1 > p.mx - 1 ? p.mx - 1 : x0 + 1;
        const int y1 = y0 + 1 > p.my - 1 ? p.my - 1 : y0 + 1;
        const int z1 = z0 + 1 > p.mz - 1 ? p.mz - 1 : z0 + 1;
        // corner order, weights and accumulation as resample_kernel (image.hip): bit d of the corner = dim d
        double val = 0.0;
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
          const int xi = (corner & 1) ? x1 : x0, yi = (corner & 2) ? y1 : y0, zi = (corner & 4) ? z1 : z0;
          double w = (corner & 1) ? fx : 1.0 - fx;
          w = __dmul_rn(w, (corner & 2) ? fy : 1.0 - fy);
          w = __dmul_rn(w, (corner & 4) ? fz : 1.0 - fz);
          val = __dadd_rn(val, __dmul_rn(w, (double)mov[((int64_t)zi * p.my + yi) * p.mx + xi]));
        }
        double b = (val - p.mlo) * p.mscale;
        b = b > 0.0 ? b : 0.0;                           // NaN -> 0: the cell index stays inside the table
        b = b < top ? b : top;
        int i = (int)floor(b);
        i = i < B - 2 ? i : B - 2;
        const double t = b - (double)i;
        const unsigned q = (unsigned)(int)floor(t * 65536.0 + 0.5);
        unsigned* cell = lds + g * BB + fb * B + i;
        if (q != 65536u) atomicAdd(cell, 65536u - q);
        if (q) atomicAdd(cell + 1, q);
      }
    }
    if (++since == kJointHistFlushTrips) {
      joint_hist_flush(lds, out, entries);
      since = 0;
    }
  }
  joint_hist_flush(lds, out, entries);
}

}  // namespace segmi

using namespace segmi;

#define SEGMI_BY_PIXEL(pixel, F, what)                                   \
  switch (pixel) {                                                       \
    case 0: F(float); break;                                             \
    case 1: F(uint8_t); break;                                           \
    case 2: F(int16_t); break;                                           \
    case 3: F(int32_t); break;                                           \
    case 4: F(uint16_t); break;                                          \
    default: SEGMI_CHECK_ARG(false, what ": unknown pixel type %d", pixel); \
  }

extern "C" {

int segmi_bin_shrink(int pixel, const void* src, int sx, int sy, int sz, int fx, int fy, int fz, float* dst,
                     void* stream) {
  SEGMI_CHECK_ARG(src && dst, "bin_shrink: null pointer");
  SEGMI_CHECK_ARG(sx > 0 && sy > 0 && sz > 0, "bin_shrink: empty image");
  SEGMI_CHECK_ARG(fx >= 1 && fy >= 1 && fz >= 1 && fx <= 8 && fy <= 8 && fz <= 8 && fx <= sx && fy <= sy && fz <= sz,
                  "bin_shrink: factors must lie in 1 .. 8 and within the extent, got %d %d %d for %d x %d x %d", fx, fy,
                  fz, sx, sy, sz);
  ShrinkParams p{src, dst, sx, sy, sz, sx / fx, sy / fy, sz / fz, fx, fy, fz};
  const int grid = grid_1d((int64_t)p.dx * p.dy * p.dz, kBinShrinkGridCap);
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH(P) hipLaunchKernelGGL(bin_shrink_kernel<P>, grid, 256, 0, st, p)
  SEGMI_BY_PIXEL(pixel, LAUNCH, "bin_shrink")
#undef LAUNCH
  SEGMI_LAUNCH_CHECK("bin_shrink");
  return SEGMI_OK;
}

int segmi_fixed_bins(const float* image, const float* mask_mean, int64_t n, double lo, double hi, int bins,
                     uint8_t* out, void* stream) {
  SEGMI_CHECK_ARG(image && out && n > 0, "fixed_bins: bad arguments");
  SEGMI_CHECK_ARG(joint_hist_group(bins) > 0, "fixed_bins: bins must be 16, 32 or 64, got %d", bins);
  SEGMI_CHECK_ARG(hi > lo && hi - lo < 1e300, "fixed_bins: the image is constant (lo = hi = %g) or not finite", lo);
  const double scale = (double)(bins - 1) / (hi - lo);
  hipLaunchKernelGGL(fixed_bins_kernel, grid_1d(n, kBinShrinkGridCap), 256, 0, (hipStream_t)stream, image, mask_mean,
                     n, lo, scale, bins, out);
  SEGMI_LAUNCH_CHECK("fixed_bins");
  return SEGMI_OK;
}

int segmi_joint_histogram_group(int bins) { return joint_hist_group(bins); }

int segmi_joint_histogram(const uint8_t* fixed_bins, int fx, int fy, int fz, int pixel, const void* moving, int mx,
                          int my, int mz, const double* index_maps_host, int candidates, int bins, double mlo,
                          double mscale, int64_t* out, void* stream) {
  SEGMI_CHECK_ARG(fixed_bins && moving && index_maps_host && out, "joint_histogram: null pointer");
  SEGMI_CHECK_ARG(fx > 0 && fy > 0 && fz > 0 && mx > 0 && my > 0 && mz > 0, "joint_histogram: empty image");
  SEGMI_CHECK_ARG(candidates >= 1 && candidates <= kJointHistMaxCandidates,
                  "joint_histogram: 1 .. %d candidates per call, got %d", kJointHistMaxCandidates, candidates);
  const int group = joint_hist_group(bins);
  SEGMI_CHECK_ARG(group > 0, "joint_histogram: bins must be 16, 32 or 64, got %d", bins);
  SEGMI_CHECK_ARG(mlo == mlo && mscale == mscale, "joint_histogram: mlo / mscale is NaN");
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = sizeof(int64_t) * (size_t)candidates * bins * bins;
  if (hipMemsetAsync(out, 0, bytes, st) != hipSuccess) {
    set_error("joint_histogram: clearing the table failed");
    return SEGMI_ELAUNCH;
  }
  JointHistParams p{};
  p.fbin = fixed_bins; p.mov = moving; p.out = (u64*)out;
  p.fx = fx; p.fy = fy; p.fz = fz; p.mx = mx; p.my = my; p.mz = mz;
  p.T = candidates; p.bins = bins; p.group = group; p.mlo = mlo; p.mscale = mscale;
  for (int t = 0; t < candidates; ++t)
    for (int k = 0; k < 12; ++k) p.m[t][k] = index_maps_host[t * 12 + k];
  const dim3 grid(grid_1d((int64_t)fx * fy * fz, kJointHistGridCap), cdiv(candidates, group));
#define LAUNCH(P) hipLaunchKernelGGL(joint_hist_kernel<P>, grid, 256, 0, st, p)
  SEGMI_BY_PIXEL(pixel, LAUNCH, "joint_histogram")
#undef LAUNCH
  SEGMI_LAUNCH_CHECK("joint_histogram");
  return SEGMI_OK;
}

}  // extern "C"
