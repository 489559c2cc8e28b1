// resample_hq.hip -- the two high-quality interpolators of the ITK-semantics resampler:
// cubic B-spline (a recursive prefilter into float64 coefficients, then a 64-tap gather) and label-Gaussian (a
// windowed per-label vote in exact integer arithmetic).  Conventions as segmi_resample3d (image.hip): arrays
// [z][y][x], the 3x4 index map, f64 coordinates, the inside test -0.5 <= c < n - 0.5, the border clamp and the
// saturate-then-truncate cast.  Built with -ffp-contract=off: every product below is rounded before it is added.
// All three kernels are bound by memory and cache traffic, not arithmetic; no MFMA.
#include "common.h"
#include "pixel_traits.h"

#include <math.h>

namespace segmi {

// ------------------------------------------------------------------ cubic B-spline: prefilter
// |z|^k < 2^-106 from k = 56 on (|z|^28 < 2^-53): on lines longer than this the causal sum stops there
constexpr int kHorizon = 56;
constexpr double kGain = 6.0;  // (1 - z)(1 - 1/z)

__device__ __forceinline__ double ipow(double z, int k) {
  double r = 1.0, b = z;
  while (k) {
    if (k & 1) r *= b;
    b *= b;
    k >>= 1;
  }
  return r;
}

// x pass: one wave per row, lane = x within a 64-sample chunk, so loads and stores are coalesced.  The first-order
// recursion v[k] = s[k] + z v[k-1] runs inside a chunk as a 6-step scan over the lanes (v += z^(2^i) * v[lane - 2^i])
// and between chunks through the last lane's value.  Reads native pixels, applies the gain, writes float64.
template <typename P>
__global__ __launch_bounds__(256) void bspline_x_kernel(const P* __restrict__ src, double* coef, int n, int64_t rows,
                                                        double z) {
  const int lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x * 4ll + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const P* s = src + row * n;
  double* c = coef + row * n;
  if (n == 1) {
    if (lane == 0) c[0] = (double)s[0];
    return;
  }
  double zp[6];
  zp[0] = z;
#pragma unroll
  for (int i = 1; i < 6; ++i) zp[i] = zp[i - 1] * zp[i - 1];
  const double zup = ipow(z, lane + 1);   // weight of the previous chunk's last value
  const double zdn = ipow(z, 64 - lane);  // weight of the next chunk's first value
  // causal initial value: the mirror sum over the whole line, or its first kHorizon terms on a long line
  double c0;
  {
    const int k = 1 + lane;
    double part = 0.0;
    if (n - 1 <= kHorizon) {
      const double zn1 = ipow(z, n - 1);
      if (k <= n - 2) part = zup * (kGain * (double)s[k] + zn1 * (kGain * (double)s[n - 1 - k]));
      part = wave_sum(part);
      c0 = (kGain * (double)s[0] + zn1 * (kGain * (double)s[n - 1]) + part) / (1.0 - zn1 * zn1);
    } else {
      if (k <= kHorizon) part = zup * (kGain * (double)s[k]);
      c0 = kGain * (double)s[0] + wave_sum(part);
    }
  }
  const int chunks = (n + 63) >> 6;
  const int li = (n - 1) & 63;
  double carry = 0.0, cl = 0.0, cm = 0.0;  // cl = c+[n-1], cm = c+[n-2]
  for (int ch = 0; ch < chunks; ++ch) {
    const int k = ch * 64 + lane;
    double v = k < n ? kGain * (double)s[k] : 0.0;
    if (k == 0) v = c0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double t = __shfl_up(v, 1 << i);
      if (lane >= (1 << i)) v += zp[i] * t;
    }
    v += zup * carry;
    if (ch == chunks - 1) {
      cl = __shfl(v, li);
      cm = li > 0 ? __shfl(v, li - 1) : carry;
    }
    carry = __shfl(v, 63);
    if (k < n) c[k] = v;
  }
  const double cinit = z / (z * z - 1.0) * (z * cm + cl);
  carry = 0.0;
  for (int ch = chunks - 1; ch >= 0; --ch) {
    const int k = ch * 64 + lane;
    double v = 0.0;
    if (k < n) v = k == n - 1 ? cinit : -z * c[k];  // each lane re-reads what it stored itself
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double t = __shfl_down(v, 1 << i);
      if (lane + (1 << i) < 64) v += zp[i] * t;
    }
    v += zdn * carry;
    carry = __shfl(v, 0);
    if (k < n) c[k] = v;
  }
}

// y and z passes, in place: one thread per line, consecutive threads on consecutive x, so every step of the
// recursion is one coalesced 512-byte access per wave.  line id -> first element (id / inner) * outer + id % inner.
__global__ __launch_bounds__(256) void bspline_line_kernel(double* coef, int n, int64_t stride, int64_t inner,
                                                           int64_t outer, int64_t lines, double z) {
  const int64_t id = blockIdx.x * 256ll + threadIdx.x;
  if (id >= lines) return;
  double* c = coef + (id / inner) * outer + id % inner;
  double sum = kGain * c[0];
  double zk = z;
  if (n - 1 <= kHorizon) {
    const double zn1 = ipow(z, n - 1);
    sum += zn1 * (kGain * c[(n - 1) * stride]);
    for (int k = 1; k < n - 1; ++k) {
      sum += zk * (kGain * c[k * stride] + zn1 * (kGain * c[(n - 1 - k) * stride]));
      zk *= z;
    }
    sum /= 1.0 - zn1 * zn1;
  } else {
    for (int k = 1; k <= kHorizon; ++k) {
      sum += zk * (kGain * c[k * stride]);
      zk *= z;
    }
  }
  double prev = sum, cm = sum;
  c[0] = prev;
#pragma unroll 4
  for (int k = 1; k < n; ++k) {
    cm = prev;
    prev = kGain * c[k * stride] + z * prev;
    c[k * stride] = prev;
  }
  double cur = z / (z * z - 1.0) * (z * cm + prev);
  c[(n - 1) * stride] = cur;
#pragma unroll 4
  for (int k = n - 2; k >= 0; --k) {
    cur = z * (cur - c[k * stride]);
    c[k * stride] = cur;
  }
}

// ------------------------------------------------------------------ shared: output voxel -> continuous index
struct HqParams {
  const void* src;  // B-spline: the float64 coefficients; label-Gaussian: the native pixels
  void* dst;
  int sx, sy, sz, dx, dy, dz;
  double m[12];
  int border;
  double defval;
  double inv[3];  // label-Gaussian: 1 / (sigma sqrt 2) per axis (x, y, z)
  int r[3];       // label-Gaussian: window radius per axis
  int taps;       // label-Gaussian: 2 max(r) + 1, the row length of the weight table
};

__device__ __forceinline__ bool hq_coords(const HqParams& p, int64_t e, double& cx, double& cy, double& cz) {
  const int ox = e % p.dx;
  const int oy = (e / p.dx) % p.dy;
  const int oz = e / ((int64_t)p.dx * p.dy);
  cx = p.m[0] * ox + p.m[1] * oy + p.m[2] * oz + p.m[3];
  cy = p.m[4] * ox + p.m[5] * oy + p.m[6] * oz + p.m[7];
  cz = p.m[8] * ox + p.m[9] * oy + p.m[10] * oz + p.m[11];
  if (p.border) {
    cx = cx < 0.0 ? 0.0 : (cx > p.sx - 1.0 ? p.sx - 1.0 : cx);
    cy = cy < 0.0 ? 0.0 : (cy > p.sy - 1.0 ? p.sy - 1.0 : cy);
    cz = cz < 0.0 ? 0.0 : (cz > p.sz - 1.0 ? p.sz - 1.0 : cz);
  }
  return cx >= -0.5 && cx < p.sx - 0.5 && cy >= -0.5 && cy < p.sy - 0.5 && cz >= -0.5 && cz < p.sz - 0.5;
}

// ------------------------------------------------------------------ cubic B-spline: evaluate
// whole-sample mirror of a tap index: period 2(n-1), everything -> 0 on an axis of extent 1
__device__ __forceinline__ int mirror_fold(int i, int n) {
  if (i >= 0 && i < n) return i;  // all but the taps next to a face
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  i %= period;
  if (i < 0) i += period;
  return i > n - 1 ? period - i : i;
}

__device__ __forceinline__ void bspline_taps(double c, int n, double (&w)[4], int (&idx)[4]) {
  const double f = floor(c);
  const double t = c - f;
  const double u = 1.0 - t;
  const double t2 = t * t, t3 = t2 * t;
  // times the float64 nearest 1/6, not a division: twelve f64 divisions per voxel would cost more than the 64 taps
  constexpr double sixth = 1.0 / 6.0;
  w[0] = u * u * u * sixth;
  w[1] = (3.0 * t3 - 6.0 * t2 + 4.0) * sixth;
  w[2] = (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) * sixth;
  w[3] = t3 * sixth;
  const int b = (int)f - 1;
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = mirror_fold(b + j, n);
}

// One thread per output voxel, consecutive lanes on consecutive output x: the 64 taps of neighbouring voxels
// overlap (all of them when upsampling), so the gather is served by L1 / L2 and each coefficient leaves HBM once.
template <typename P>
__global__ __launch_bounds__(256) void bspline_eval_kernel(HqParams p) {
  const double* __restrict__ coef = (const double*)p.src;
  P* dst = (P*)p.dst;
  const int64_t total = (int64_t)p.dx * p.dy * p.dz;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    double cx, cy, cz;
    double val = p.defval;
    if (hq_coords(p, e, cx, cy, cz)) {
      double wx[4], wy[4], wz[4];
      int ix[4], iy[4], iz[4];
      bspline_taps(cx, p.sx, wx, ix);
      bspline_taps(cy, p.sy, wy, iy);
      bspline_taps(cz, p.sz, wz, iz);
      val = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        double plane = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double* row = coef + ((int64_t)iz[a] * p.sy + iy[b]) * p.sx;
          double r = 0.0;
#pragma unroll
          for (int c = 0; c < 4; ++c) r += wx[c] * row[ix[c]];
          plane += wy[b] * r;
        }
        val += wz[a] * plane;
      }
    }
    dst[e] = PixelTraits<P>::cast(val);
  }
}

// ------------------------------------------------------------------ label-Gaussian
constexpr int kLabelTable = 8;      // distinct labels a thread tallies in registers
constexpr int kLabelMaxRadius = 8;  // window radius limit per axis
constexpr double kLabelScale = 262144.0;  // 2^18

// The part lo .. hi of the window [i0 - r, i0 + r] that lies inside the buffer, i0 = floor(c + 0.5).
__device__ __forceinline__ void label_axis_window(double c, int n, int r, int& lo, int& hi) {
  const int i0 = (int)floor(c + 0.5);
  lo = i0 - r < 0 ? 0 : i0 - r;
  hi = i0 + r > n - 1 ? n - 1 : i0 + r;
}

// Per-axis integer weights of one voxel into the thread's own column of the LDS table (entry stride 256): tap t
// stands for input index lo + t.  Neighbouring taps share an edge, (i + 0.5) - c being the same float64 as
// ((i + 1) - 0.5) - c, so each erf is taken once.
__device__ __forceinline__ void label_axis_weights(double c, double inv, int lo, int hi, int* q) {
  double below = erf((((double)lo - 0.5) - c) * inv);
  for (int i = lo; i <= hi; ++i) {
    const double above = erf((((double)i + 0.5) - c) * inv);
    const double w = 0.5 * (above - below);
    q[(i - lo) * 256] = (int)(int64_t)floor(w * kLabelScale + 0.5);
    below = above;
  }
}

// One thread per output voxel.  A window holding a single label (the interior of every structure) is answered
// after one comparison sweep, before any weight is computed.  Otherwise the thread tallies up to kLabelTable labels in registers; a window with
// more distinct labels takes the slow path: for each first occurrence of a label, rescan the window.
template <typename P>
__global__ __launch_bounds__(256) void label_gaussian_kernel(HqParams p) {
  extern __shared__ int qtab[];  // [axis][tap][thread]
  const P* __restrict__ src = (const P*)p.src;
  P* dst = (P*)p.dst;
  int* qx = qtab + threadIdx.x;
  int* qy = qx + p.taps * 256;
  int* qz = qy + p.taps * 256;
  const int64_t total = (int64_t)p.dx * p.dy * p.dz;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    double cx, cy, cz;
    if (!hq_coords(p, e, cx, cy, cz)) {
      dst[e] = PixelTraits<P>::cast(p.defval);
      continue;
    }
    int x0, x1, y0, y1, z0, z1;
    label_axis_window(cx, p.sx, p.r[0], x0, x1);
    label_axis_window(cy, p.sy, p.r[1], y0, y1);
    label_axis_window(cz, p.sz, p.r[2], z0, z1);
    const P first = src[((int64_t)z0 * p.sy + y0) * p.sx + x0];
    bool uniform = true;
    for (int z = z0; z <= z1 && uniform; ++z)
      for (int y = y0; y <= y1 && uniform; ++y) {
        const P* row = src + ((int64_t)z * p.sy + y) * p.sx;
        for (int x = x0; x <= x1; ++x) uniform = uniform && row[x] == first;
      }
    if (uniform) {
      dst[e] = first;
      continue;
    }
    label_axis_weights(cx, p.inv[0], x0, x1, qx);
    label_axis_weights(cy, p.inv[1], y0, y1, qy);
    label_axis_weights(cz, p.inv[2], z0, z1, qz);
    P lab[kLabelTable];
    int64_t score[kLabelTable];
#pragma unroll
    for (int t = 0; t < kLabelTable; ++t) { lab[t] = first; score[t] = 0; }
    int count = 0;
    bool overflow = false;
    for (int z = z0; z <= z1 && !overflow; ++z)
      for (int y = y0; y <= y1 && !overflow; ++y) {
        const P* row = src + ((int64_t)z * p.sy + y) * p.sx;
        const int64_t wzy = (int64_t)qz[(z - z0) * 256] * qy[(y - y0) * 256];
        for (int x = x0; x <= x1; ++x) {
          const P v = row[x];
          const int64_t w = wzy * qx[(x - x0) * 256];
          bool found = false;
#pragma unroll
          for (int t = 0; t < kLabelTable; ++t) {
            const bool hit = t < count && lab[t] == v;
            score[t] += hit ? w : 0;
            found = found || hit;
          }
          if (!found) {
            if (count == kLabelTable) { overflow = true; break; }
#pragma unroll
            for (int t = 0; t < kLabelTable; ++t)
              if (t == count) { lab[t] = v; score[t] = w; }
            ++count;
          }
        }
      }
    P best = first;
    int64_t best_score = -1;
    if (!overflow) {
#pragma unroll
      for (int t = 0; t < kLabelTable; ++t)
        if (t < count && (score[t] > best_score || (score[t] == best_score && lab[t] < best))) {
          best = lab[t];
          best_score = score[t];
        }
    } else {
      const int nx = x1 - x0 + 1, ny = y1 - y0 + 1, nz = z1 - z0 + 1;
      const int nwin = nx * ny * nz;
      for (int a = 0; a < nwin; ++a) {
        const int ax = a % nx, ay = (a / nx) % ny, az = a / (nx * ny);
        const P v = src[((int64_t)(z0 + az) * p.sy + (y0 + ay)) * p.sx + (x0 + ax)];
        int64_t s = 0;
        bool seen = false;  // v at an earlier tap: already scored
        for (int b = 0; b < nwin; ++b) {
          const int bx = b % nx, by = (b / nx) % ny, bz = b / (nx * ny);
          if (src[((int64_t)(z0 + bz) * p.sy + (y0 + by)) * p.sx + (x0 + bx)] != v) continue;
          if (b < a) { seen = true; break; }
          s += (int64_t)qz[bz * 256] * qy[by * 256] * qx[bx * 256];
        }
        if (!seen && (s > best_score || (s == best_score && v < best))) {
          best = v;
          best_score = s;
        }
      }
    }
    dst[e] = best;
  }
}

}  // namespace segmi

using namespace segmi;

namespace {

bool hq_shape_ok(int sx, int sy, int sz) { return sx > 0 && sy > 0 && sz > 0; }

void hq_fill(HqParams& p, const void* src, int sx, int sy, int sz, void* dst, int dx, int dy, int dz,
             const double* index_map_host, int border, double default_value) {
  p.src = src; p.dst = dst; p.sx = sx; p.sy = sy; p.sz = sz; p.dx = dx; p.dy = dy; p.dz = dz;
  for (int i = 0; i < 12; ++i) p.m[i] = index_map_host[i];
  p.border = border; p.defval = default_value;
}

}  // namespace

extern "C" {

int64_t segmi_bspline_workspace(int sx, int sy, int sz) {
  if (!hq_shape_ok(sx, sy, sz)) return 0;
  return (int64_t)sx * sy * sz * 8;
}

int segmi_bspline_prefilter(int pixel, const void* src, int sx, int sy, int sz, double* coef, void* stream) {
  SEGMI_CHECK_ARG(src && coef, "bspline_prefilter: null pointer");
  SEGMI_CHECK_ARG(hq_shape_ok(sx, sy, sz), "bspline_prefilter: empty image");
  const int64_t rows = (int64_t)sy * sz, plane = (int64_t)sx * sy, nvox = plane * sz;
  SEGMI_CHECK_ARG(cdiv64(rows, 4) < (1ll << 31) && cdiv64(nvox, 256) < (1ll << 31), "bspline_prefilter: image too large");
  hipStream_t st = (hipStream_t)stream;
  const double z = sqrt(3.0) - 2.0;
  const int gx = (int)cdiv64(rows, 4);
#define LAUNCH(P) hipLaunchKernelGGL(bspline_x_kernel<P>, gx, 256, 0, st, (const P*)src, coef, sx, rows, z)
  SEGMI_BY_PIXEL(pixel, LAUNCH, "bspline_prefilter")
#undef LAUNCH
  if (sy > 1) {  // lines along y: one per (z, x)
    const int64_t lines = (int64_t)sx * sz;
    hipLaunchKernelGGL(bspline_line_kernel, (int)cdiv64(lines, 256), 256, 0, st, coef, sy, (int64_t)sx, (int64_t)sx,
                       plane, lines, z);
  }
  if (sz > 1)  // lines along z: one per (y, x)
    hipLaunchKernelGGL(bspline_line_kernel, (int)cdiv64(plane, 256), 256, 0, st, coef, sz, plane, plane, (int64_t)0,
                       plane, z);
  SEGMI_LAUNCH_CHECK("bspline_prefilter");
  return SEGMI_OK;
}

int segmi_resample3d_bspline(const double* coef, int sx, int sy, int sz, int pixel, void* dst, int dx, int dy, int dz,
                             const double* index_map_host, int border, double default_value, void* stream) {
  SEGMI_CHECK_ARG(coef && dst && index_map_host, "resample3d_bspline: null pointer");
  SEGMI_CHECK_ARG(hq_shape_ok(sx, sy, sz) && hq_shape_ok(dx, dy, dz), "resample3d_bspline: empty image");
  SEGMI_CHECK_ARG(border == 0 || border == 1, "resample3d_bspline: border must be 0 or 1");
  HqParams p{};
  hq_fill(p, coef, sx, sy, sz, dst, dx, dy, dz, index_map_host, border, default_value);
  const int grid = grid_1d((int64_t)dx * dy * dz, SEGMI_RESAMPLE_HQ_GRID_CAP);
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH(P) hipLaunchKernelGGL(bspline_eval_kernel<P>, grid, 256, 0, st, p)
  SEGMI_BY_PIXEL(pixel, LAUNCH, "resample3d_bspline")
#undef LAUNCH
  SEGMI_LAUNCH_CHECK("resample3d_bspline");
  return SEGMI_OK;
}

int segmi_resample3d_label_gaussian(int pixel, const void* src, int sx, int sy, int sz, void* dst, int dx, int dy,
                                    int dz, const double* index_map_host, const double* sigma_xyz_host, double alpha,
                                    int border, double default_value, void* stream) {
  SEGMI_CHECK_ARG(src && dst && index_map_host && sigma_xyz_host, "resample3d_label_gaussian: null pointer");
  SEGMI_CHECK_ARG(hq_shape_ok(sx, sy, sz) && hq_shape_ok(dx, dy, dz), "resample3d_label_gaussian: empty image");
  SEGMI_CHECK_ARG(border == 0 || border == 1, "resample3d_label_gaussian: border must be 0 or 1");
  SEGMI_CHECK_ARG(alpha > 0.0 && alpha <= 1e6, "resample3d_label_gaussian: alpha must be positive, got %g", alpha);
  HqParams p{};
  hq_fill(p, src, sx, sy, sz, dst, dx, dy, dz, index_map_host, border, default_value);
  int rmax = 0;
  for (int a = 0; a < 3; ++a) {
    const double s = sigma_xyz_host[a];
    SEGMI_CHECK_ARG(s > 0.0 && s <= 1e6, "resample3d_label_gaussian: sigma must be positive, got %g", s);
    const double r = ceil(alpha * s);
    SEGMI_CHECK_ARG(r <= kLabelMaxRadius, "resample3d_label_gaussian: radius ceil(alpha * sigma) = %g exceeds %d voxels",
                    r, kLabelMaxRadius);
    p.r[a] = (int)r;
    p.inv[a] = 1.0 / (s * sqrt(2.0));
    rmax = p.r[a] > rmax ? p.r[a] : rmax;
  }
  p.taps = 2 * rmax + 1;
  const size_t lds = (size_t)3 * p.taps * 256 * sizeof(int);
  const int grid = grid_1d((int64_t)dx * dy * dz, SEGMI_RESAMPLE_HQ_GRID_CAP);
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH(P) hipLaunchKernelGGL(label_gaussian_kernel<P>, grid, 256, lds, st, p)
  SEGMI_BY_PIXEL(pixel, LAUNCH, "resample3d_label_gaussian")
#undef LAUNCH
  SEGMI_LAUNCH_CHECK("resample3d_label_gaussian");
  return SEGMI_OK;
}

}  // extern "C"
