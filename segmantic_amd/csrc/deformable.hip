// deformable.hip -- the kernels of B-spline free-form deformable registration by mutual information (DESIGN.md
// section 24): the joint histogram of a fixed bin volume and a moving volume under up to 8 candidate control grids
// in one launch, the integer gradient of the metric scattered onto the control grid, the fold count / Jacobian
// determinant of a grid, and the resampling of the moving image through the transform.  As in registration.hip
// every sum that crosses lanes is an integer and everything else is float64 with every operation rounded on its own
// (built with -ffp-contract=off), so a table, a gradient and a warped image are bit-equal to the numpy restatement.
// The histogram's table, the trilinear sample and the bin scatter are those of registration.hip (mi_sampling.h); the
// warp ends in the resampler's tap (pixel_traits.h).
#include "mi_sampling.h"
#include "pixel_traits.h"

namespace segmi {

constexpr int kFfdMaxCandidates = SEGMI_FFD_MAX_CANDIDATES;
constexpr int kFfdMaxPoints = SEGMI_FFD_MAX_CONTROL_POINTS;
constexpr int64_t kFfdMaxSupport = (int64_t)SEGMI_FFD_GRADIENT_MAX_SUPPORT;

// ------------------------------------------------------------------ the B-spline, axis by axis
// span index k and fraction f of level voxel j: i = j F + 0.5 (F - 1), t = (i (n - 3)) / (dim - 1),
// k = min(floor(t), n - 4), f = t - k.  An axis of extent 1 has t = 0.  j F + F - 1 <= dim - 1 (checked on the
// host), so 0 <= t <= n - 3 and the four taps k .. k + 3 lie inside the grid.
__device__ __forceinline__ void ffd_span(int j, int F, int dim, int n, int& k, double& f) {
  if (dim == 1) { k = 0; f = 0.0; return; }
  const double i = (double)j * (double)F + 0.5 * (double)(F - 1);
  const double t = (i * (double)(n - 3)) / (double)(dim - 1);
  double kf = floor(t);
  const double top = (double)(n - 4);
  kf = kf < top ? kf : top;
  kf = kf > 0.0 ? kf : 0.0;
  k = (int)kf;
  f = t - kf;
}

// the "/ 6" of the cubic weights is a multiplication by the float64 nearest to 1 / 6: twelve float64 divisions per
// voxel would be a third of a kernel's arithmetic
__device__ __forceinline__ void ffd_weights(double f, double* w) {
  constexpr double sixth = 1.0 / 6.0;
  const double g = 1.0 - f, f2 = f * f, f3 = f2 * f;
  w[0] = ((g * g) * g) * sixth;
  w[1] = ((3.0 * f3 - 6.0 * f2) + 4.0) * sixth;
  w[2] = (((3.0 * f2 - 3.0 * f3) + 3.0 * f) + 1.0) * sixth;
  w[3] = f3 * sixth;
}

// d w / d f
__device__ __forceinline__ void ffd_dweights(double f, double* w) {
  const double g = 1.0 - f, f2 = f * f;
  w[0] = (g * g) * -0.5;
  w[1] = 1.5 * f2 - 2.0 * f;
  w[2] = ((f - 1.5 * f2)) + 0.5;
  w[3] = f2 * 0.5;
}

struct FfdGrid {
  int lx, ly, lz, dx, dy, dz, fx, fy, fz, nx, ny, nz;
};

// u (mm along the fixed array axes x, y, z) of one control grid [3][nz][ny][nx] at the taps kx.., ky.., kz..:
// per component the 64 terms ((wz wy) wx) * phi added from 0 with z taps outermost and x taps innermost, ascending.
// base points at tap (kz, ky, kx) of component x; sy, sz, sc: strides of a row, a plane and a component.
template <typename PhiPtr>
__device__ __forceinline__ void ffd_displacement(PhiPtr base, int64_t sy, int64_t sz, int64_t sc, const double* wx,
                                                 const double* wy, const double* wz, const FfdGrid& g, double* u) {
  double u0 = 0.0, u1 = 0.0, u2 = 0.0;
  // the z loop stays rolled: unrolled, the 192 loads of a candidate are hoisted together and the kernels spill
#pragma unroll 1
  for (int c = 0; c < 4; ++c) {
    const double wzc = c == 0 ? wz[0] : (c == 1 ? wz[1] : (c == 2 ? wz[2] : wz[3]));
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const double wzy = wzc * wy[b];
      PhiPtr row = base + c * sz + b * sy;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double w = wzy * wx[a];
        u0 = u0 + w * row[a];
        u1 = u1 + w * row[sc + a];
        u2 = u2 + w * row[2 * sc + a];
      }
    }
  }
  u[0] = g.dx == 1 ? 0.0 : u0;          // an axis of extent 1 carries no displacement
  u[1] = g.dy == 1 ? 0.0 : u1;
  u[2] = g.dz == 1 ? 0.0 : u2;
}

// continuous moving index: c_r = (((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3]) + ((R[r][0] u_x + R[r][1] u_y) + R[r][2] u_z)
__device__ __forceinline__ double ffd_coord(const double* m, const double* r, double x, double y, double z,
                                            const double* u) {
  return (((m[0] * x + m[1] * y) + m[2] * z) + m[3]) + ((r[0] * u[0] + r[1] * u[1]) + r[2] * u[2]);
}

// ------------------------------------------------------------------ joint histogram under candidate grids
struct FfdHistParams {
  HistParams h;                           // the fixed extent is the level grid g.lx x g.ly x g.lz
  const double* phi;                      // [T][3][nz][ny][nx]
  FfdGrid g;
  double m[12], r[9];
};

// coordinate policy of joint_hist_body: spans and weights once per voxel, the displacement under control grid t
struct BsplineCoord {
  const FfdHistParams& p;
  struct Voxel {
    double x, y, z, wx[4], wy[4], wz[4];
    int64_t tap;                          // of the first support point in a component
  };
  __device__ __forceinline__ void voxel(int ix, int iy, int iz, Voxel& v) const {
    const FfdGrid& g = p.g;
    int kx, ky, kz;
    double f;
    v.x = (double)ix; v.y = (double)iy; v.z = (double)iz;
    ffd_span(ix, g.fx, g.dx, g.nx, kx, f); ffd_weights(f, v.wx);
    ffd_span(iy, g.fy, g.dy, g.ny, ky, f); ffd_weights(f, v.wy);
    ffd_span(iz, g.fz, g.dz, g.nz, kz, f); ffd_weights(f, v.wz);
    v.tap = ((int64_t)kz * g.ny + ky) * g.nx + kx;
  }
  __device__ __forceinline__ void at(const Voxel& v, int t, double& cx, double& cy, double& cz) const {
    const FfdGrid& g = p.g;
    const int64_t np = (int64_t)g.nx * g.ny * g.nz;
    double u[3];
    ffd_displacement(p.phi + (int64_t)t * 3 * np + v.tap, (int64_t)g.nx, (int64_t)g.nx * g.ny, np, v.wx, v.wy, v.wz, g, u);
    cx = ffd_coord(p.m, p.r, v.x, v.y, v.z, u);
    cy = ffd_coord(p.m + 4, p.r + 3, v.x, v.y, v.z, u);
    cz = ffd_coord(p.m + 8, p.r + 6, v.x, v.y, v.z, u);
  }
};

template <typename P>
__global__ __launch_bounds__(256) void ffd_joint_hist_kernel(FfdHistParams p) {
  joint_hist_body<P>(p.h, BsplineCoord{p});
}

// ------------------------------------------------------------------ gradient onto the control grid
struct FfdGradParams {
  const uint8_t* fbin;
  const void* mov;
  const double* phi;                      // [3][nz][ny][nx]
  const int* qd;                          // [bins][bins - 1]
  long long* out;                         // [3][nz][ny][nx]
  FfdGrid g;
  int mx, my, mz, bins;
  double mlo, mscale, gscale;
  double m[12], r[9];
};

// first level voxel j of an axis whose span index is >= k (ldim when there is none): an estimate from the inverse
// of ffd_span, corrected with ffd_span itself, which is monotone in j
__device__ int ffd_cell_start(int k, int F, int dim, int n, int ldim) {
  if (k <= 0) return 0;
  if (dim == 1 || k > n - 4) return ldim;
  const double est = (((double)k * (double)(dim - 1)) / (double)(n - 3) - 0.5 * (double)(F - 1)) / (double)F;
  int j = (int)ceil(est);
  j = j < 0 ? 0 : (j > ldim ? ldim : j);
  int kk;
  double f;
  while (j > 0) {
    ffd_span(j - 1, F, dim, n, kk, f);
    if (kk < k) break;
    --j;
  }
  while (j < ldim) {
    ffd_span(j, F, dim, n, kk, f);
    if (kk >= k) break;
    ++j;
  }
  return j;
}

// One workgroup works inside ONE control cell (grid x), on every gridDim.y-th batch of 256 of its voxels (grid y):
// all its samples share one 4 x 4 x 4 support.  A batch is produced sample per lane (the integers E_a = Qd * G_a and
// the twelve axis weights go to LDS) and consumed point per lane: lane l of wave w owns support point l and adds
// E_a * Wq of the samples 64 w .. 64 w + 63 to three 64-bit registers.  At the end the four waves' sums meet in LDS
// and each non-zero (point, component) costs one global 64-bit atomic.  Integer sums: any order is exact.
template <typename P>
__global__ __launch_bounds__(256) void ffd_gradient_kernel(FfdGradParams p) {
  __shared__ double sphi[3][64];
  __shared__ double sw[256][12];
  __shared__ int se[256][3];
  __shared__ long long sacc[4][192];
  const P* __restrict__ mov = (const P*)p.mov;
  const FfdGrid g = p.g;
  const int B = p.bins;
  const int spx = g.nx - 3, spy = g.ny - 3;
  const int kx = blockIdx.x % spx, ky = (blockIdx.x / spx) % spy, kz = blockIdx.x / (spx * spy);
  const int x_lo = ffd_cell_start(kx, g.fx, g.dx, g.nx, g.lx), x_hi = ffd_cell_start(kx + 1, g.fx, g.dx, g.nx, g.lx);
  const int y_lo = ffd_cell_start(ky, g.fy, g.dy, g.ny, g.ly), y_hi = ffd_cell_start(ky + 1, g.fy, g.dy, g.ny, g.ly);
  const int z_lo = ffd_cell_start(kz, g.fz, g.dz, g.nz, g.lz), z_hi = ffd_cell_start(kz + 1, g.fz, g.dz, g.nz, g.lz);
  const int ex = x_hi - x_lo, ey = y_hi - y_lo, ez = z_hi - z_lo;
  if (ex <= 0 || ey <= 0 || ez <= 0) return;            // a cell no level voxel falls into (uniform over the workgroup)
  const int64_t count = (int64_t)ex * ey * ez;
  const int64_t batches = (count + 255) / 256;
  const int64_t np = (int64_t)g.nx * g.ny * g.nz;
  const int tid = threadIdx.x;
  if (tid < 192) {
    const int comp = tid >> 6, pt = tid & 63;
    sphi[comp][pt] = p.phi[comp * np + ((int64_t)(kz + (pt >> 4)) * g.ny + (ky + ((pt >> 2) & 3))) * g.nx + kx + (pt & 3)];
  }
  __syncthreads();
  const double top = (double)(B - 1);
  const int wave = tid >> 6, lane = tid & 63;
  const int pc = lane >> 4, pb = (lane >> 2) & 3, pa = lane & 3;
  long long acc0 = 0, acc1 = 0, acc2 = 0;
  for (int64_t batch = blockIdx.y; batch < batches; batch += gridDim.y) {
    // ---- produce: one sample per lane
    const int64_t e = batch * 256 + tid;
    int e0 = 0, e1 = 0, e2 = 0;
    double wx[4] = {0.0, 0.0, 0.0, 0.0}, wy[4] = {0.0, 0.0, 0.0, 0.0}, wz[4] = {0.0, 0.0, 0.0, 0.0};
    if (e < count) {
      const int ix = x_lo + (int)(e % ex), iy = y_lo + (int)((e / ex) % ey), iz = z_lo + (int)(e / ((int64_t)ex * ey));
      const int fb = p.fbin[((int64_t)iz * g.ly + iy) * g.lx + ix];
      if (fb < B) {
        const double x = (double)ix, y = (double)iy, z = (double)iz;
        int k_;
        double f;
        ffd_span(ix, g.fx, g.dx, g.nx, k_, f); ffd_weights(f, wx);
        ffd_span(iy, g.fy, g.dy, g.ny, k_, f); ffd_weights(f, wy);
        ffd_span(iz, g.fz, g.dz, g.nz, k_, f); ffd_weights(f, wz);
        double u[3];
        ffd_displacement(&sphi[0][0], (int64_t)4, (int64_t)16, (int64_t)64, wx, wy, wz, g, u);
        const double cx = ffd_coord(p.m, p.r, x, y, z, u);
        const double cy = ffd_coord(p.m + 4, p.r + 3, x, y, z, u);
        const double cz = ffd_coord(p.m + 8, p.r + 6, x, y, z, u);
        if (mi_inside(p.mx, p.my, p.mz, cx, cy, cz)) {
          double gc[3];                                   // the derivatives of the value by c_x, c_y, c_z
          const double val = mi_sample<P, true>(mov, p.mx, p.my, p.mz, cx, cy, cz, gc);
          const double b = (val - p.mlo) * p.mscale;
          if (b > 0.0 && b < top) {                       // a clamped bin coordinate has no derivative
            const int i = (int)floor(b);                  // 0 .. B - 2
            const int qd = p.qd[fb * (B - 1) + i];
            const double* r = p.r;
            double d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              double s = ((gc[0] * r[a] + gc[1] * r[3 + a]) + gc[2] * r[6 + a]) * p.gscale;
              s = s > -1.0 ? s : -1.0;                    // NaN -> -1: stays a finite integer
              s = s < 1.0 ? s : 1.0;
              d[a] = rint(s * 32768.0);
            }
            e0 = g.dx == 1 ? 0 : qd * (int)d[0];
            e1 = g.dy == 1 ? 0 : qd * (int)d[1];
            e2 = g.dz == 1 ? 0 : qd * (int)d[2];
          }
        }
      }
    }
    se[tid][0] = e0; se[tid][1] = e1; se[tid][2] = e2;
#pragma unroll
    for (int a = 0; a < 4; ++a) { sw[tid][a] = wx[a]; sw[tid][4 + a] = wy[a]; sw[tid][8 + a] = wz[a]; }
    __syncthreads();
    // ---- consume: one support point per lane, a quarter of the batch per wave
    for (int s = wave * 64; s < wave * 64 + 64; ++s) {
      const int q0 = se[s][0], q1 = se[s][1], q2 = se[s][2];
      if (!(q0 | q1 | q2)) continue;                      // uniform over the wave
      const long long wq = (long long)rint(((sw[s][8 + pc] * sw[s][4 + pb]) * sw[s][pa]) * 4096.0);
      acc0 += (long long)q0 * wq;
      acc1 += (long long)q1 * wq;
      acc2 += (long long)q2 * wq;
    }
    __syncthreads();
  }
  sacc[wave][lane] = acc0; sacc[wave][64 + lane] = acc1; sacc[wave][128 + lane] = acc2;
  __syncthreads();
  if (tid < 192) {
    const long long v = ((sacc[0][tid] + sacc[1][tid]) + sacc[2][tid]) + sacc[3][tid];
    if (v) {
      const int comp = tid >> 6, pt = tid & 63;
      const int64_t at = comp * np + ((int64_t)(kz + (pt >> 4)) * g.ny + (ky + ((pt >> 2) & 3))) * g.nx + kx + (pt & 3);
      atomicAdd((u64*)p.out + at, (u64)v);
    }
  }
}

// ------------------------------------------------------------------ fold count and Jacobian determinant
struct FfdJacParams {
  const double* phi;
  long long* folded;
  long long* min_key;                     // the minimum as an order-preserving integer; ffd_jac_finish decodes it
  float* map;
  FfdGrid g;
  double invh[3];                         // 1 / control spacing in mm per axis (0 on an axis of extent 1)
};

__device__ __forceinline__ long long ffd_key(double v) {
  const long long b = __double_as_longlong(v);
  return b >= 0 ? b : b ^ 0x7fffffffffffffffll;
}

__global__ void ffd_jac_init(long long* folded, long long* min_key) {
  *folded = 0;
  *min_key = 0x7ff0000000000000ll;        // +inf
}

__global__ void ffd_jac_finish(long long* min_key) {
  const long long k = *min_key;
  *min_key = k >= 0 ? k : k ^ 0x7fffffffffffffffll;   // the bits of the double again
}

__global__ __launch_bounds__(256) void ffd_jacobian_kernel(FfdJacParams p) {
  __shared__ unsigned long long scount;
  __shared__ long long smin;
  const FfdGrid g = p.g;
  if (threadIdx.x == 0) { scount = 0; smin = 0x7ff0000000000000ll; }
  __syncthreads();
  const int64_t np = (int64_t)g.nx * g.ny * g.nz;
  const int64_t total = (int64_t)g.lx * g.ly * g.lz;
  unsigned long long bad = 0;
  double lowest = __longlong_as_double(0x7ff0000000000000ll);
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int ix = (int)(e % g.lx), iy = (int)((e / g.lx) % g.ly), iz = (int)(e / ((int64_t)g.lx * g.ly));
    int kx, ky, kz;
    double f, wx[4], wy[4], wz[4], vx[4], vy[4], vz[4];
    ffd_span(ix, g.fx, g.dx, g.nx, kx, f); ffd_weights(f, wx); ffd_dweights(f, vx);
    ffd_span(iy, g.fy, g.dy, g.ny, ky, f); ffd_weights(f, wy); ffd_dweights(f, vy);
    ffd_span(iz, g.fz, g.dz, g.nz, kz, f); ffd_weights(f, wz); ffd_dweights(f, vz);
    const double* base = p.phi + ((int64_t)kz * g.ny + ky) * g.nx + kx;
    // s[a][b] = sum over the 64 taps (z outermost, x innermost) of (derivative weights along b) * phi_a
    double s[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {                          // rolled, as in ffd_displacement
      const double wzc = c == 0 ? wz[0] : (c == 1 ? wz[1] : (c == 2 ? wz[2] : wz[3]));
      const double vzc = c == 0 ? vz[0] : (c == 1 ? vz[1] : (c == 2 ? vz[2] : vz[3]));
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const double w_zy = wzc * wy[b], w_zdy = wzc * vy[b], w_dzy = vzc * wy[b];
        const double* row = base + ((int64_t)c * g.ny + b) * g.nx;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const double w0 = w_zy * vx[a], w1 = w_zdy * wx[a], w2 = w_dzy * wx[a];
#pragma unroll
          for (int comp = 0; comp < 3; ++comp) {
            const double v = row[comp * np + a];
            s[comp][0] = s[comp][0] + w0 * v;
            s[comp][1] = s[comp][1] + w1 * v;
            s[comp][2] = s[comp][2] + w2 * v;
          }
        }
      }
    }
    const bool flat[3] = {g.dx == 1, g.dy == 1, g.dz == 1};
    double j[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) j[a][b] = (a == b ? 1.0 : 0.0) + (flat[a] ? 0.0 : s[a][b] * p.invh[b]);
    const double det = (j[0][0] * (j[1][1] * j[2][2] - j[1][2] * j[2][1]) - j[0][1] * (j[1][0] * j[2][2] - j[1][2] * j[2][0])) +
                       j[0][2] * (j[1][0] * j[2][1] - j[1][1] * j[2][0]);
    if (det <= 0.0) ++bad;
    lowest = det < lowest ? det : lowest;
    if (p.map) p.map[e] = (float)det;
  }
  if (bad) atomicAdd(&scount, bad);
  atomicMin(&smin, ffd_key(lowest));
  __syncthreads();
  if (threadIdx.x == 0) {
    if (scount) atomicAdd((u64*)p.folded, (u64)scount);
    atomicMin(p.min_key, smin);
  }
}

// ------------------------------------------------------------------ warp
struct FfdWarpParams {
  const double* phi;
  const void* src;
  void* dst;                              // nullable
  float* disp;                            // nullable, [3][z][y][x] mm along the physical axes
  FfdGrid g;
  int mx, my, mz, nearest;
  double defval;
  double m[12], r[9], dir[9];
};

template <typename P>
__global__ __launch_bounds__(256) void ffd_warp_kernel(FfdWarpParams p) {
  const P* __restrict__ src = (const P*)p.src;
  P* __restrict__ dst = (P*)p.dst;
  const FfdGrid g = p.g;
  const int64_t np = (int64_t)g.nx * g.ny * g.nz;
  const int64_t total = (int64_t)g.lx * g.ly * g.lz;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int ix = (int)(e % g.lx), iy = (int)((e / g.lx) % g.ly), iz = (int)(e / ((int64_t)g.lx * g.ly));
    const double x = (double)ix, y = (double)iy, z = (double)iz;
    int kx, ky, kz;
    double f, wx[4], wy[4], wz[4], u[3];
    ffd_span(ix, g.fx, g.dx, g.nx, kx, f); ffd_weights(f, wx);
    ffd_span(iy, g.fy, g.dy, g.ny, ky, f); ffd_weights(f, wy);
    ffd_span(iz, g.fz, g.dz, g.nz, kz, f); ffd_weights(f, wz);
    ffd_displacement(p.phi + ((int64_t)kz * g.ny + ky) * g.nx + kx, (int64_t)g.nx, (int64_t)g.nx * g.ny, np, wx, wy, wz, g,
                     u);
    if (p.disp) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
        p.disp[r * total + e] = (float)((p.dir[3 * r] * u[0] + p.dir[3 * r + 1] * u[1]) + p.dir[3 * r + 2] * u[2]);
    }
    if (!dst) continue;
    const double cx = ffd_coord(p.m, p.r, x, y, z, u);
    const double cy = ffd_coord(p.m + 4, p.r + 3, x, y, z, u);
    const double cz = ffd_coord(p.m + 8, p.r + 6, x, y, z, u);
    dst[e] = resample_tap(src, p.mx, p.my, p.mz, cx, cy, cz, p.nearest ? 1 : 0, p.defval);
  }
}

static int ffd_grid_check(const char* what, const segmi_ffd_grid* s, FfdGrid& g) {
  SEGMI_CHECK_ARG(s, "%s: null grid description", what);
  g = FfdGrid{s->lx, s->ly, s->lz, s->dx, s->dy, s->dz, s->fx, s->fy, s->fz, s->nx, s->ny, s->nz};
  SEGMI_CHECK_ARG(g.lx > 0 && g.ly > 0 && g.lz > 0 && g.dx > 0 && g.dy > 0 && g.dz > 0, "%s: empty image", what);
  SEGMI_CHECK_ARG(g.fx >= 1 && g.fy >= 1 && g.fz >= 1 && g.fx <= 8 && g.fy <= 8 && g.fz <= 8, "%s: level factors must lie in 1 .. 8, got %d %d %d",
                  what, g.fx, g.fy, g.fz);
  SEGMI_CHECK_ARG((int64_t)g.lx * g.fx <= g.dx && (int64_t)g.ly * g.fy <= g.dy && (int64_t)g.lz * g.fz <= g.dz,
                  "%s: the level grid %d x %d x %d times its factors %d %d %d exceeds the image %d x %d x %d", what,
                  g.lx, g.ly, g.lz, g.fx, g.fy, g.fz, g.dx, g.dy, g.dz);
  SEGMI_CHECK_ARG(g.nx >= 4 && g.ny >= 4 && g.nz >= 4, "%s: a control grid has at least 4 points per axis, got %d x %d x %d (x, y, z)",
                  what, g.nx, g.ny, g.nz);
  SEGMI_CHECK_ARG((int64_t)g.nx * g.ny * g.nz <= kFfdMaxPoints, "%s: %lld control points, at most %d", what,
                  (long long)g.nx * g.ny * g.nz, kFfdMaxPoints);
  return SEGMI_OK;
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int segmi_ffd_joint_histogram(const uint8_t* fixed_bins, const segmi_ffd_grid* grid, const double* control,
                              int candidates, int pixel, const void* moving, int mx, int my, int mz,
                              const double* index_map_host, const double* r_host, int bins, double mlo, double mscale,
                              int64_t* out, void* stream) {
  SEGMI_CHECK_ARG(fixed_bins && control && moving && index_map_host && r_host && out, "ffd_joint_histogram: null pointer");
  FfdGrid g;
  if (int rc = ffd_grid_check("ffd_joint_histogram", grid, g)) return rc;
  SEGMI_CHECK_ARG(mx > 0 && my > 0 && mz > 0, "ffd_joint_histogram: empty moving image");
  SEGMI_CHECK_ARG(candidates >= 1 && candidates <= kFfdMaxCandidates, "ffd_joint_histogram: 1 .. %d candidate grids per call, got %d",
                  kFfdMaxCandidates, candidates);
  const int group = hist_group(bins, kFfdMaxCandidates);
  SEGMI_CHECK_ARG(group > 0, "ffd_joint_histogram: bins must be 16, 32 or 64, got %d", bins);
  SEGMI_CHECK_ARG(pixel >= 0 && pixel <= 4, "ffd_joint_histogram: unknown pixel type %d", pixel);
  SEGMI_CHECK_ARG(mlo == mlo && mscale == mscale, "ffd_joint_histogram: mlo / mscale is NaN");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, sizeof(int64_t) * (size_t)candidates * bins * bins, st) != hipSuccess) {
    set_error("ffd_joint_histogram: clearing the table failed");
    return SEGMI_ELAUNCH;
  }
  FfdHistParams p{};
  p.h = HistParams{fixed_bins, moving, (u64*)out, g.lx, g.ly, g.lz, mx, my, mz, candidates, bins, group, mlo, mscale};
  p.phi = control; p.g = g;
  for (int k = 0; k < 12; ++k) p.m[k] = index_map_host[k];
  for (int k = 0; k < 9; ++k) p.r[k] = r_host[k];
  const dim3 blocks(grid_1d((int64_t)g.lx * g.ly * g.lz, SEGMI_FFD_HIST_GRID_CAP), cdiv(candidates, group));
#define LAUNCH(P) hipLaunchKernelGGL(ffd_joint_hist_kernel<P>, blocks, 256, 0, st, p)
  SEGMI_BY_PIXEL(pixel, LAUNCH, "ffd_joint_histogram")
#undef LAUNCH
  SEGMI_LAUNCH_CHECK("ffd_joint_histogram");
  return SEGMI_OK;
}

int segmi_ffd_gradient(const uint8_t* fixed_bins, const segmi_ffd_grid* grid, const double* control, int pixel,
                       const void* moving, int mx, int my, int mz, const double* index_map_host, const double* r_host,
                       int bins, double mlo, double mscale, double gscale, const int32_t* qd, int64_t* out,
                       void* stream) {
  SEGMI_CHECK_ARG(fixed_bins && control && moving && index_map_host && r_host && qd && out, "ffd_gradient: null pointer");
  FfdGrid g;
  if (int rc = ffd_grid_check("ffd_gradient", grid, g)) return rc;
  SEGMI_CHECK_ARG(mx > 0 && my > 0 && mz > 0, "ffd_gradient: empty moving image");
  SEGMI_CHECK_ARG(hist_group(bins, kFfdMaxCandidates) > 0, "ffd_gradient: bins must be 16, 32 or 64, got %d", bins);
  SEGMI_CHECK_ARG(pixel >= 0 && pixel <= 4, "ffd_gradient: unknown pixel type %d", pixel);
  SEGMI_CHECK_ARG(mlo == mlo && mscale == mscale && gscale == gscale, "ffd_gradient: mlo / mscale / gscale is NaN");
  // a control point's support is four spans per axis: at most ceil(4 l / spans) + 1 level voxels, and never more than l
  int64_t support = 1;
  const int l[3] = {g.lx, g.ly, g.lz}, n[3] = {g.nx, g.ny, g.nz};
  for (int a = 0; a < 3; ++a) {
    int64_t s = cdiv64(4ll * l[a], n[a] - 3) + 1;
    support *= s < l[a] ? s : l[a];
  }
  SEGMI_CHECK_ARG(support <= kFfdMaxSupport,
                  "ffd_gradient: %lld samples under one control point's support, at most %lld (2^42 per sample in an int64 sum): "
                  "use more control points", (long long)support, (long long)kFfdMaxSupport);
  hipStream_t st = (hipStream_t)stream;
  const int64_t np = (int64_t)g.nx * g.ny * g.nz;
  if (hipMemsetAsync(out, 0, sizeof(int64_t) * 3 * (size_t)np, st) != hipSuccess) {
    set_error("ffd_gradient: clearing the table failed");
    return SEGMI_ELAUNCH;
  }
  FfdGradParams p{};
  p.fbin = fixed_bins; p.mov = moving; p.phi = control; p.qd = qd; p.out = (long long*)out; p.g = g;
  p.mx = mx; p.my = my; p.mz = mz; p.bins = bins; p.mlo = mlo; p.mscale = mscale; p.gscale = gscale;
  for (int k = 0; k < 12; ++k) p.m[k] = index_map_host[k];
  for (int k = 0; k < 9; ++k) p.r[k] = r_host[k];
  // the largest cell: ceil(l / spans) + 1 level voxels per axis
  int64_t cell = 1;
  for (int a = 0; a < 3; ++a) {
    int64_t s = cdiv64(l[a], n[a] - 3) + 1;
    cell *= s < l[a] ? s : l[a];
  }
  const int64_t chunks = cdiv64(cell, 256);
  const dim3 blocks((unsigned)((g.nx - 3) * (g.ny - 3) * (g.nz - 3)),
                    (unsigned)(chunks > SEGMI_FFD_GRADIENT_GRID_CAP ? SEGMI_FFD_GRADIENT_GRID_CAP : chunks));
#define LAUNCH(P) hipLaunchKernelGGL(ffd_gradient_kernel<P>, blocks, 256, 0, st, p)
  SEGMI_BY_PIXEL(pixel, LAUNCH, "ffd_gradient")
#undef LAUNCH
  SEGMI_LAUNCH_CHECK("ffd_gradient");
  return SEGMI_OK;
}

int segmi_ffd_jacobian(const segmi_ffd_grid* grid, const double* control, const double* inv_spacing_host,
                       int64_t* folded, double* min_jacobian, float* det_map, void* stream) {
  SEGMI_CHECK_ARG(control && inv_spacing_host && folded && min_jacobian, "ffd_jacobian: null pointer");
  FfdGrid g;
  if (int rc = ffd_grid_check("ffd_jacobian", grid, g)) return rc;
  FfdJacParams p{};
  p.phi = control; p.folded = (long long*)folded; p.min_key = (long long*)min_jacobian; p.map = det_map; p.g = g;
  for (int a = 0; a < 3; ++a) {
    SEGMI_CHECK_ARG(inv_spacing_host[a] == inv_spacing_host[a], "ffd_jacobian: inverse control spacing is NaN");
    p.invh[a] = inv_spacing_host[a];
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ffd_jac_init, 1, 1, 0, st, p.folded, p.min_key);
  hipLaunchKernelGGL(ffd_jacobian_kernel, grid_1d((int64_t)g.lx * g.ly * g.lz, SEGMI_FFD_JACOBIAN_GRID_CAP), 256, 0, st, p);
  hipLaunchKernelGGL(ffd_jac_finish, 1, 1, 0, st, p.min_key);
  SEGMI_LAUNCH_CHECK("ffd_jacobian");
  return SEGMI_OK;
}

int segmi_ffd_warp(const segmi_ffd_grid* grid, const double* control, int pixel, const void* moving, int mx, int my,
                   int mz, const double* index_map_host, const double* r_host, int nearest, double default_value,
                   void* dst, const double* direction_host, float* displacement, void* stream) {
  SEGMI_CHECK_ARG(control && index_map_host && r_host, "ffd_warp: null pointer");
  SEGMI_CHECK_ARG(dst || displacement, "ffd_warp: neither an output image nor a displacement field was asked for");
  SEGMI_CHECK_ARG(!dst || moving, "ffd_warp: null moving image");
  SEGMI_CHECK_ARG(!displacement || direction_host, "ffd_warp: a displacement field needs the fixed direction matrix");
  FfdGrid g;
  if (int rc = ffd_grid_check("ffd_warp", grid, g)) return rc;
  SEGMI_CHECK_ARG(g.fx == 1 && g.fy == 1 && g.fz == 1 && g.lx == g.dx && g.ly == g.dy && g.lz == g.dz,
                  "ffd_warp: the output grid is the full-resolution fixed grid (factors 1)");
  SEGMI_CHECK_ARG(!dst || (mx > 0 && my > 0 && mz > 0), "ffd_warp: empty moving image");
  SEGMI_CHECK_ARG(pixel >= 0 && pixel <= 4, "ffd_warp: unknown pixel type %d", pixel);
  SEGMI_CHECK_ARG(nearest == 0 || nearest == 1, "ffd_warp: nearest must be 0 (linear) or 1, got %d", nearest);
  FfdWarpParams p{};
  p.phi = control; p.src = moving; p.dst = dst; p.disp = displacement; p.g = g;
  p.mx = mx; p.my = my; p.mz = mz; p.nearest = nearest; p.defval = default_value;
  for (int k = 0; k < 12; ++k) p.m[k] = index_map_host[k];
  for (int k = 0; k < 9; ++k) {
    p.r[k] = r_host[k];
    p.dir[k] = direction_host ? direction_host[k] : 0.0;
  }
  hipStream_t st = (hipStream_t)stream;
  const int blocks = grid_1d((int64_t)g.lx * g.ly * g.lz, SEGMI_FFD_WARP_GRID_CAP);
#define LAUNCH(P) hipLaunchKernelGGL(ffd_warp_kernel<P>, blocks, 256, 0, st, p)
  SEGMI_BY_PIXEL(pixel, LAUNCH, "ffd_warp")
#undef LAUNCH
  SEGMI_LAUNCH_CHECK("ffd_warp");
  return SEGMI_OK;
}

}  // extern "C"
