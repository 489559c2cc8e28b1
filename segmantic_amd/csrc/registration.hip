// registration.hip -- the kernels of rigid / affine registration by mutual information:
// the block-mean pyramid level, the fixed image's bin volume, and the joint intensity histogram of a fixed
// volume and a moving volume interpolated under up to 32 candidate transforms in one launch (the table in LDS, its
// flush bound and the sampling: mi_sampling.h).  Built with -ffp-contract=off: index map, trilinear weights and the
// bin coordinate are specified operation by operation in float64.
#include "mi_sampling.h"

namespace segmi {

constexpr int kJointHistMaxCandidates = SEGMI_JOINT_HIST_MAX_CANDIDATES;
constexpr int kBinShrinkGridCap = SEGMI_BIN_SHRINK_GRID_CAP;
constexpr int kJointHistGridCap = SEGMI_JOINT_HIST_GRID_CAP;

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
  HistParams h;
  double m[kJointHistMaxCandidates][12];   // fixed index (x,y,z,1) -> continuous moving index (x,y,z)
};

// coordinate policy of joint_hist_body: candidate t is the affine index map m[t]
struct AffineCoord {
  const double (&m)[kJointHistMaxCandidates][12];
  struct Voxel { double x, y, z; };
  __device__ __forceinline__ void voxel(int ix, int iy, int iz, Voxel& v) const {
    v.x = (double)ix; v.y = (double)iy; v.z = (double)iz;
  }
  __device__ __forceinline__ void at(const Voxel& v, int t, double& cx, double& cy, double& cz) const {
    const double* a = m[t];
    cx = ((a[0] * v.x + a[1] * v.y) + a[2] * v.z) + a[3];
    cy = ((a[4] * v.x + a[5] * v.y) + a[6] * v.z) + a[7];
    cz = ((a[8] * v.x + a[9] * v.y) + a[10] * v.z) + a[11];
  }
};

template <typename P>
__global__ __launch_bounds__(256) void joint_hist_kernel(JointHistParams p) {
  joint_hist_body<P>(p.h, AffineCoord{p.m});
}

}  // namespace segmi

using namespace segmi;

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
  SEGMI_CHECK_ARG(hist_group(bins, kJointHistMaxCandidates) > 0, "fixed_bins: bins must be 16, 32 or 64, got %d", bins);
  SEGMI_CHECK_ARG(hi > lo && hi - lo < 1e300, "fixed_bins: the image is constant (lo = hi = %g) or not finite", lo);
  const double scale = (double)(bins - 1) / (hi - lo);
  hipLaunchKernelGGL(fixed_bins_kernel, grid_1d(n, kBinShrinkGridCap), 256, 0, (hipStream_t)stream, image, mask_mean,
                     n, lo, scale, bins, out);
  SEGMI_LAUNCH_CHECK("fixed_bins");
  return SEGMI_OK;
}

int segmi_joint_histogram_group(int bins) { return hist_group(bins, kJointHistMaxCandidates); }

int segmi_joint_histogram(const uint8_t* fixed_bins, int fx, int fy, int fz, int pixel, const void* moving, int mx,
                          int my, int mz, const double* index_maps_host, int candidates, int bins, double mlo,
                          double mscale, int64_t* out, void* stream) {
  SEGMI_CHECK_ARG(fixed_bins && moving && index_maps_host && out, "joint_histogram: null pointer");
  SEGMI_CHECK_ARG(fx > 0 && fy > 0 && fz > 0 && mx > 0 && my > 0 && mz > 0, "joint_histogram: empty image");
  SEGMI_CHECK_ARG(candidates >= 1 && candidates <= kJointHistMaxCandidates,
                  "joint_histogram: 1 .. %d candidates per call, got %d", kJointHistMaxCandidates, candidates);
  const int group = hist_group(bins, kJointHistMaxCandidates);
  SEGMI_CHECK_ARG(group > 0, "joint_histogram: bins must be 16, 32 or 64, got %d", bins);
  SEGMI_CHECK_ARG(mlo == mlo && mscale == mscale, "joint_histogram: mlo / mscale is NaN");
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = sizeof(int64_t) * (size_t)candidates * bins * bins;
  if (hipMemsetAsync(out, 0, bytes, st) != hipSuccess) {
    set_error("joint_histogram: clearing the table failed");
    return SEGMI_ELAUNCH;
  }
  JointHistParams p{};
  p.h = HistParams{fixed_bins, moving, (u64*)out, fx, fy, fz, mx, my, mz, candidates, bins, group, mlo, mscale};
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
