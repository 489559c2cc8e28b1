// image.hip -- ITK-semantics 3-D resample (trilinear / nearest) and channel-wise intensity
// normalisation.  Replaces the SimpleITK CPU path of src/segmantic/image/processing.py:49-120
// and MONAI NormalizeIntensityd (monai_unet.py:164).  HBM-bound; index math in f64 as ITK does.
#include "common.h"
#include "pixel_traits.h"

namespace segmi {

struct ResampleParams {
  const void* src;
  void* dst;
  int sx, sy, sz, dx, dy, dz;
  double m[12];  // out index (x,y,z,1) -> continuous in index (x,y,z)
  int interp;
  double defval;
};

template <typename P>
__global__ void resample_kernel(ResampleParams p) {
  const P* src = (const P*)p.src;
  P* dst = (P*)p.dst;
  const int64_t total = (int64_t)p.dx * p.dy * p.dz;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int ox = e % p.dx;
    const int oy = (e / p.dx) % p.dy;
    const int oz = e / ((int64_t)p.dx * p.dy);
    double cx = p.m[0] * ox + p.m[1] * oy + p.m[2] * oz + p.m[3];
    double cy = p.m[4] * ox + p.m[5] * oy + p.m[6] * oz + p.m[7];
    double cz = p.m[8] * ox + p.m[9] * oy + p.m[10] * oz + p.m[11];
    if (p.interp & 2) {  // border padding (MONAI Spacing / grid_sample "border"): clamp the coordinate
      cx = cx < 0.0 ? 0.0 : (cx > p.sx - 1.0 ? p.sx - 1.0 : cx);
      cy = cy < 0.0 ? 0.0 : (cy > p.sy - 1.0 ? p.sy - 1.0 : cy);
      cz = cz < 0.0 ? 0.0 : (cz > p.sz - 1.0 ? p.sz - 1.0 : cz);
    }
    dst[e] = resample_tap(src, p.sx, p.sy, p.sz, cx, cy, cz, p.interp, p.defval);
  }
}

constexpr int kNormChunk = 1 << 16;

__global__ __launch_bounds__(256) void norm_reduce_kernel(const float* __restrict__ x, int64_t nvox,
                                                          int chunks, double* __restrict__ part) {
  __shared__ double red[2][4];
  const int c = blockIdx.y, chunk = blockIdx.x;
  const float* xc = x + (int64_t)c * nvox;
  const int64_t v0 = (int64_t)chunk * kNormChunk;
  const int64_t v1 = v0 + kNormChunk < nvox ? v0 + kNormChunk : nvox;
  double s = 0.0, q = 0.0;
  for (int64_t v = v0 + threadIdx.x; v < v1; v += 256) {
    const double a = (double)xc[v];
    s += a; q += a * a;
  }
  s = wave_sum(s); q = wave_sum(q);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = s; red[1][wave] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[((int64_t)c * chunks + chunk) * 2 + 0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    part[((int64_t)c * chunks + chunk) * 2 + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

__global__ void norm_finalize_kernel(const double* __restrict__ part, int c, int chunks,
                                     int64_t nvox, float* __restrict__ ms) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  double s = 0.0, q = 0.0;
  for (int k = 0; k < chunks; ++k) { s += part[((int64_t)i * chunks + k) * 2]; q += part[((int64_t)i * chunks + k) * 2 + 1]; }
  const double m = s / (double)nvox;
  double var = q / (double)nvox - m * m;
  if (var < 0.0) var = 0.0;
  float sd = (float)sqrt(var);
  if (sd == 0.f) sd = 1.f;
  ms[2 * i] = (float)m;
  ms[2 * i + 1] = sd;
}

__global__ void norm_apply_kernel(float* __restrict__ x, int64_t nvox, const float* __restrict__ ms) {
  const int c = blockIdx.y;
  const float m = ms[2 * c], sd = ms[2 * c + 1];
  float* xc = x + (int64_t)c * nvox;
  for (int64_t v = blockIdx.x * 256ll + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256)
    xc[v] = (xc[v] - m) / sd;
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int segmi_resample3d(int pixel, const void* src, int sx, int sy, int sz, void* dst, int dx,
                     int dy, int dz, const double* index_map_host, int interp,
                     double default_value, void* stream) {
  SEGMI_CHECK_ARG(src && dst && index_map_host, "resample3d: null pointer");
  SEGMI_CHECK_ARG(sx > 0 && sy > 0 && sz > 0 && dx > 0 && dy > 0 && dz > 0, "resample3d: empty image");
  SEGMI_CHECK_ARG(interp >= 0 && interp <= 7 && (!(interp & 4) || (interp & 1)),
                  "resample3d: interp must be 0 (linear) or 1 (nearest), +2 for border padding, +4 (nearest only) to round half to even");
  ResampleParams p{};
  p.src = src; p.dst = dst; p.sx = sx; p.sy = sy; p.sz = sz; p.dx = dx; p.dy = dy; p.dz = dz;
  for (int i = 0; i < 12; ++i) p.m[i] = index_map_host[i];
  p.interp = interp; p.defval = default_value;
  const int64_t total = (int64_t)dx * dy * dz;
  const int grid = (int)(cdiv64(total, 256) > 8192 ? 8192 : cdiv64(total, 256));
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH(P) hipLaunchKernelGGL(resample_kernel<P>, grid, 256, 0, st, p)
  SEGMI_BY_PIXEL(pixel, LAUNCH, "resample3d")
#undef LAUNCH
  SEGMI_LAUNCH_CHECK("resample3d");
  return SEGMI_OK;
}

int64_t segmi_normalize_workspace(int c, int64_t nvox) {
  const int64_t chunks = cdiv64(nvox, kNormChunk);
  return c * chunks * 2 * 8 + (int64_t)c * 2 * 4 + 256;
}

int segmi_normalize_intensity(float* x, int c, int64_t nvox, void* workspace, void* stream) {
  SEGMI_CHECK_ARG(x && workspace && c > 0 && nvox > 0, "normalize_intensity: bad arguments");
  const int chunks = (int)cdiv64(nvox, kNormChunk);
  double* part = (double*)workspace;
  float* ms = (float*)((char*)workspace + ((int64_t)c * chunks * 2 * 8 + 255) / 256 * 256);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(norm_reduce_kernel, dim3(chunks, c), 256, 0, st, (const float*)x, nvox, chunks, part);
  hipLaunchKernelGGL(norm_finalize_kernel, cdiv(c, 64), 64, 0, st, (const double*)part, c, chunks, nvox, ms);
  const int gx = (int)(cdiv64(nvox, 256) > 2048 ? 2048 : cdiv64(nvox, 256));
  hipLaunchKernelGGL(norm_apply_kernel, dim3(gx, c), 256, 0, st, x, nvox, (const float*)ms);
  SEGMI_LAUNCH_CHECK("normalize_intensity");
  return SEGMI_OK;
}

}  // extern "C"
