// n4.hip -- MRI / CT preprocessing of src/segmantic/image/modality.py on the GPU:
//   Otsu threshold      : min/max pass, 200-bin exact count histogram, one-thread pick of the threshold;
//   shrink              : one gather of the image, its mask (given, or the Otsu threshold applied) and the
//                         log values of the fit set;
//   N4                  : the whole iteration on the device (histogram of U, Wiener sharpening by direct
//                         512-point circular convolutions in f64, B-spline BA fit by per-tile partials
//                         folded in a fixed order, field re-evaluation, CV sums); one 8-byte read per iteration;
//   full-resolution     : B-spline evaluation fused with the division, separable per row;
//   scale_clamp_ct      : 27-voxel median (forgetful selection), clamp and scale.
// Every sum is exact (integer) or runs in a fixed order, so repeated calls are bit-identical.
#include "labelvol.h"

// the clamp / scale expression and the Otsu / sharpening arithmetic are rounded operation by operation
// (the Makefile also gives this file -ffp-contract=off)
#pragma clang fp contract(off)

namespace segmi {

constexpr int kN4Threads = 256;
constexpr int kN4RedBlocks = 1024;       // fixed grid of the reduction kernels: fixed summation order
constexpr int kN4MaxBins = 512;         // padded sharpening size P <= 1024: 40 KB of LDS
constexpr int kSharpThreads = 512;
constexpr int kBaMaxT = 16;              // tile points per axis
constexpr size_t kBaLdsBudget = 48 * 1024;
constexpr double kHistFix = 4294967296.0;  // 2^32: histogram weights as exact u64 fixed point


// ------------------------------------------------------------------ per-axis B-spline geometry
// lat == 1: an axis without spline dimension (weight 1); else m = lat - 3 spans, u = i / (n - 1) * m.
__host__ __device__ __forceinline__ int axis_span(int i, int n, int lat) {
  if (lat == 1) return 0;
  const int m = lat - 3;
  const double u = n > 1 ? (double)i / (double)(n - 1) * (double)m : 0.0;
  int s = (int)floor(u);
  return s < m - 1 ? s : m - 1;
}

__host__ __device__ __forceinline__ int axis_taps(int lat) { return lat == 1 ? 1 : 4; }

__device__ __forceinline__ int axis_weights(int i, int n, int lat, double w[4]) {
  const bool spline = lat > 1;
  const int m = spline ? lat - 3 : 1;
  const double u = (spline && n > 1) ? (double)i / (double)(n - 1) * (double)m : 0.0;
  int s = (int)floor(u);
  s = s < m - 1 ? s : m - 1;
  const double t = u - s;
  const double t2 = t * t, t3 = t2 * t;
  // selects on values, not two branches that store into w: keeps w in registers
  w[0] = spline ? (1.0 - t) * (1.0 - t) * (1.0 - t) / 6.0 : 1.0;
  w[1] = spline ? (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0 : 0.0;
  w[2] = spline ? (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0 : 0.0;
  w[3] = spline ? t3 / 6.0 : 0.0;
  return s;
}

struct Grid3 {
  int n[3];    // z, y, x voxels
  int lat[3];  // control points per axis
};

__device__ __forceinline__ unsigned f2key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ------------------------------------------------------------------ Otsu
// ws: u32 keys[2] (min, max of the finite values)
template <bool VEC>
__global__ __launch_bounds__(kN4Threads) void otsu_minmax_kernel(const float* __restrict__ x, int64_t n,
                                                                 unsigned* keys) {
  unsigned kmin = 0xffffffffu, kmax = 0u;
  auto take = [&](float v) {
    if (isfinite(v)) {
      const unsigned k = f2key(v);
      kmin = min(kmin, k);
      kmax = max(kmax, k);
    }
  };
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, parts = (int64_t)gridDim.x * blockDim.x;
  int64_t tail = 0;
  if (VEC) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (int64_t i = t; i < n / 4; i += parts) {
      const float4 v = x4[i];
      take(v.x); take(v.y); take(v.z); take(v.w);
    }
    tail = n / 4 * 4;
  }
  for (int64_t i = tail + t; i < n; i += parts) take(x[i]);
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o));
    kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&keys[0], kmin);
    atomicMax(&keys[1], kmax);
  }
}

// one LDS count per wave when every active lane hits the same bin (b < 0: no bin)
__device__ __forceinline__ void wave_count(unsigned* h, int b) {
  const int b0 = __builtin_amdgcn_readfirstlane(b);
  const unsigned long long act = __ballot(1);
  const unsigned long long same = __ballot(b == b0);
  if (same == act) {
    if (b0 >= 0 && (int)__lane_id() == __ffsll((long long)act) - 1) atomicAdd(&h[b0], (unsigned)__popcll(act));
  } else if (b >= 0) {
    atomicAdd(&h[b], 1u);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kN4Threads) void otsu_hist_kernel(const float* __restrict__ x, int64_t n,
                                                               const unsigned* keys, int bins,
                                                               unsigned long long* counts) {
  __shared__ unsigned h[kN4MaxBins];
  for (int i = threadIdx.x; i < bins; i += blockDim.x) h[i] = 0;
  __syncthreads();
  const unsigned k0 = keys[0], k1 = keys[1];
  const double lo = k0 <= k1 ? (double)key2f(k0) : 0.0;
  const double hi = k0 <= k1 ? (double)key2f(k1) : 0.0;
  const double w = (hi - lo) / (double)bins;
  auto bin = [&](float v) -> int {
    if (!isfinite(v)) return -1;
    if (!(w > 0.0)) return 0;
    const double c = floor(((double)v - lo) / w);
    return c < (double)(bins - 1) ? (int)c : bins - 1;
  };
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, parts = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = VEC ? n / 4 : 0;
  // every lane runs the same trip count per wave so that wave_count's ballots see whole waves
  const int64_t span = (int64_t)gridDim.x * blockDim.x;
  const int64_t base = (int64_t)blockIdx.x * blockDim.x;
  for (int64_t i0 = base; i0 < nv; i0 += span) {
    const int64_t i = i0 + threadIdx.x;
    float4 v = make_float4(NAN, NAN, NAN, NAN);
    if (i < nv) v = reinterpret_cast<const float4*>(x)[i];
    wave_count(h, bin(v.x)); wave_count(h, bin(v.y)); wave_count(h, bin(v.z)); wave_count(h, bin(v.w));
  }
  for (int64_t i0 = nv * 4 + base; i0 < n; i0 += span) {
    const int64_t i = i0 + threadIdx.x;
    wave_count(h, i < n ? bin(x[i]) : -1);
  }
  (void)t; (void)parts;
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += blockDim.x)
    if (h[i]) atomicAdd(&counts[i], (unsigned long long)h[i]);
}

__global__ void otsu_init_kernel(unsigned* keys, unsigned long long* counts, int bins) {
  if (threadIdx.x == 0) { keys[0] = 0xffffffffu; keys[1] = 0u; }
  for (int i = threadIdx.x; i < bins; i += blockDim.x) counts[i] = 0ull;
}

// stats: [0] lo, [1] width, [2] threshold, [3] finite count (as double); one thread, bin order
__global__ void otsu_pick_kernel(const unsigned* keys, const unsigned long long* counts, int bins, double* stats,
                                 int64_t* counts_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned k0 = keys[0], k1 = keys[1];
  const double lo = k0 <= k1 ? (double)key2f(k0) : 0.0;
  const double hi = k0 <= k1 ? (double)key2f(k1) : 0.0;
  const double w = (hi - lo) / (double)bins;
  double n_tot = 0.0, s_all = 0.0;
  for (int i = 0; i < bins; ++i) {
    const double c = (double)counts[i];
    n_tot += c;
    s_all += c * (lo + (i + 0.5) * w);
    if (counts_out) counts_out[i] = (int64_t)counts[i];
  }
  double best = -1.0, w0 = 0.0, s0 = 0.0;
  int kb = 0;
  for (int k = 0; k < bins; ++k) {
    const double c = (double)counts[k];
    w0 += c;
    s0 += c * (lo + (k + 0.5) * w);
    const double w1 = n_tot - w0;
    double var = 0.0;
    if (w0 > 0.0 && w1 > 0.0) {
      const double d = s0 / w0 - (s_all - s0) / w1;
      var = w0 * w1 * (d * d);
    }
    if (var > best) { best = var; kb = k; }
  }
  stats[0] = lo;
  stats[1] = w;
  stats[2] = lo + (kb + 1) * w;
  stats[3] = n_tot;
}

// ------------------------------------------------------------------ shrink / mask / log gather
// out voxel (jz, jy, jx) <- input (jz fz + oz, jy fy + oy, jx fx + ox); mask: given (== 1 is the label) or
// outside where v > threshold (stats[2]), inside elsewhere; log = log(v) on the fit set, NaN elsewhere.
struct ShrinkParams {
  const float* x;
  const uint8_t* mask;
  const double* stats;
  float* out_img;
  uint8_t* out_mask;
  double* out_log;
  int64_t sy, sz;        // input strides (x stride 1)
  int ns[3], f[3], o[3]; // z, y, x
  int inside, outside;
};

__global__ __launch_bounds__(kN4Threads) void n4_shrink_kernel(ShrinkParams p) {
  const int64_t total = (int64_t)p.ns[0] * p.ns[1] * p.ns[2];
  const double thr = p.stats ? p.stats[2] : 0.0;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
    const int jx = (int)(j % p.ns[2]);
    const int64_t r = j / p.ns[2];
    const int jy = (int)(r % p.ns[1]);
    const int jz = (int)(r / p.ns[1]);
    const int64_t src = (int64_t)(jz * p.f[0] + p.o[0]) * p.sz + (int64_t)(jy * p.f[1] + p.o[1]) * p.sy +
                        (int64_t)(jx * p.f[2] + p.o[2]);
    const float v = p.x[src];
    int m = 1;
    if (p.mask) m = p.mask[src];
    else if (p.stats) m = (double)v > thr ? p.outside : p.inside;
    if (p.out_img) p.out_img[j] = v;
    if (p.out_mask) p.out_mask[j] = (uint8_t)m;
    if (p.out_log) p.out_log[j] = (m == 1 && isfinite(v) && v > 0.0f) ? log((double)v) : (double)NAN;
  }
}

// ------------------------------------------------------------------ N4 state
struct N4State {
  double umin, umax;   // U = L - field over the fit set
  double slope;        // of the last sharpening
  double cv;
  double count;
  double pad[3];
};

// partial of one reduction block: s1 = sum (e - 1), s2 = sum (e - 1)^2, count, umin, umax
struct N4Part {
  double s1, s2, cnt, umin, umax, pad;
};

// the four taps of every axis run unconditionally (registers, no scratch); an axis without spline
// dimension has weights {1, 0, 0, 0} and its tap index is clamped to 0
__device__ __forceinline__ double grid_value(const double* lat, const Grid3& g, int z, int y, int x) {
  double wz[4], wy[4], wx[4];
  const int sz = axis_weights(z, g.n[0], g.lat[0], wz);
  const int sy = axis_weights(y, g.n[1], g.lat[1], wy);
  const int sx = axis_weights(x, g.n[2], g.lat[2], wx);
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int iz = min(sz + a, g.lat[0] - 1), iy = min(sy + b, g.lat[1] - 1);
      const double* row = lat + ((int64_t)iz * g.lat[1] + iy) * g.lat[2];
      double racc = 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) racc += wx[c] * row[min(sx + c, g.lat[2] - 1)];
      acc += wz[a] * wy[b] * racc;
    }
  return acc;
}

__device__ __forceinline__ void block_reduce_part(N4Part& v, N4Part* out) {
  __shared__ N4Part s[kN4Threads];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = kN4Threads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      N4Part& a = s[threadIdx.x];
      const N4Part& b = s[threadIdx.x + o];
      a.s1 += b.s1; a.s2 += b.s2; a.cnt += b.cnt;
      a.umin = fmin(a.umin, b.umin); a.umax = fmax(a.umax, b.umax);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = s[0];
}

// field <- the lattice's field on the grid (lat null: 0); with cv, the sums of e = exp(old - new) over the
// fit set; always min / max of U = L - field_new and the fit-set count.  Fixed grid (kN4RedBlocks).
__global__ __launch_bounds__(kN4Threads) void n4_eval_kernel(const double* __restrict__ L, double* field,
                                                             const double* lat, Grid3 g, int cv, N4Part* parts) {
  const int64_t total = (int64_t)g.n[0] * g.n[1] * g.n[2];
  N4Part v{0.0, 0.0, 0.0, INFINITY, -INFINITY, 0.0};
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(j % g.n[2]);
    const int64_t r = j / g.n[2];
    const int y = (int)(r % g.n[1]);
    const int z = (int)(r / g.n[1]);
    const double nf = lat ? grid_value(lat, g, z, y, x) : 0.0;
    const double l = L[j];
    if (isfinite(l)) {
      if (cv) {
        const double e = exp(field[j] - nf) - 1.0;
        v.s1 += e;
        v.s2 += e * e;
      }
      const double u = l - nf;
      v.cnt += 1.0;
      v.umin = fmin(v.umin, u);
      v.umax = fmax(v.umax, u);
    }
    field[j] = nf;
  }
  block_reduce_part(v, parts + blockIdx.x);
}

__global__ __launch_bounds__(kN4Threads) void n4_finalise_kernel(const N4Part* parts, int nparts, N4State* st) {
  N4Part v{0.0, 0.0, 0.0, INFINITY, -INFINITY, 0.0};
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    const N4Part b = parts[i];
    v.s1 += b.s1; v.s2 += b.s2; v.cnt += b.cnt;
    v.umin = fmin(v.umin, b.umin); v.umax = fmax(v.umax, b.umax);
  }
  __shared__ N4Part tot;
  block_reduce_part(v, &tot);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = tot.cnt;
    const double mean = 1.0 + tot.s1 / n;
    double var = (tot.s2 - tot.s1 * tot.s1 / n) / (n - 1.0);
    var = var > 0.0 ? var : 0.0;
    st->cv = sqrt(var) / mean;
    st->umin = tot.umin;
    st->umax = tot.umax;
    st->count = n;
  }
}

// histogram of U by linear splatting, weights as exact u64 fixed point (2^-32)
__global__ __launch_bounds__(kN4Threads) void n4_hist_kernel(const double* __restrict__ L,
                                                             const double* __restrict__ field, int64_t total,
                                                             const N4State* st, int bins,
                                                             unsigned long long* hist) {
  __shared__ unsigned long long h[kN4MaxBins];
  for (int i = threadIdx.x; i < bins; i += blockDim.x) h[i] = 0ull;
  __syncthreads();
  const double lo = st->umin;
  const double slope = (st->umax - st->umin) / (double)(bins - 1);
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
    const double l = L[j];
    if (!isfinite(l)) continue;
    const double u = field ? l - field[j] : l;
    double c = slope > 0.0 ? (u - lo) / slope : 0.0;
    c = c > 0.0 ? c : 0.0;
    double fi = floor(c);
    int i = fi < (double)(bins - 1) ? (int)fi : bins - 1;
    const double fr = c - (double)i;
    const double f1 = fr < 1.0 ? fr : 1.0;
    atomicAdd(&h[i], (unsigned long long)llrint((1.0 - f1) * kHistFix));
    if (i + 1 < bins) atomicAdd(&h[i + 1], (unsigned long long)llrint(f1 * kHistFix));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += blockDim.x)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

// Wiener sharpening of the histogram (one workgroup).  With F real and even, IDFT(DFT(a) F^) is the
// circular convolution a (*) F, and IDFT(DFT(V) G) is V (*) g with g = IDFT(G): the transforms of the
// contract become direct f64 sums over P points.  Writes E [bins] and st->slope, then clears hist.
__global__ __launch_bounds__(kSharpThreads) void n4_sharpen_kernel(unsigned long long* hist, N4State* st, int bins,
                                                                   int P, double fwhm, double noise, double* E) {
  extern __shared__ double sm[];
  double* cs = sm;           // cos(2 pi j / P)
  double* F = sm + P;        // Gaussian
  double* V = sm + 2 * P;    // padded histogram, later x * Ut
  double* G = sm + 3 * P;    // Wiener filter, later Ut
  double* g = sm + 4 * P;    // IDFT(G)
  const int off = (P - bins) / 2;
  const double lo = st->umin;
  const double slope = (st->umax - st->umin) / (double)(bins - 1);
  const double fw = fwhm / slope;
  const double ex = 4.0 * log(2.0) / (fw * fw);
  const double sc = 2.0 * sqrt(log(2.0) / M_PI) / fw;
  for (int j = threadIdx.x; j < P; j += blockDim.x) {
    cs[j] = cospi(2.0 * (double)j / (double)P);
    const int nn = j <= P / 2 ? j : P - j;
    F[j] = sc * exp(-ex * (double)nn * (double)nn);
    V[j] = (j >= off && j < off + bins) ? (double)hist[j - off] / kHistFix : 0.0;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < bins; j += blockDim.x) hist[j] = 0ull;  // ready for the next iteration
  const int mask = P - 1;
  for (int k = threadIdx.x; k < P; k += blockDim.x) {
    double fh = 0.0;
    for (int n = 0; n < P; ++n) fh += F[n] * cs[(n * k) & mask];
    G[k] = fh / (fh * fh + noise);
  }
  __syncthreads();
  for (int n = threadIdx.x; n < P; n += blockDim.x) {
    double a = 0.0;
    for (int k = 0; k < P; ++k) a += G[k] * cs[(n * k) & mask];
    g[n] = a / (double)P;
  }
  __syncthreads();
  double ut[(2 * kN4MaxBins + kSharpThreads - 1) / kSharpThreads];
  int q = 0;
  for (int n = threadIdx.x; n < P; n += blockDim.x, ++q) {
    double a = 0.0;
    for (int m = off; m < off + bins; ++m) a += V[m] * g[(n - m) & mask];
    ut[q] = a > 0.0 ? a : 0.0;
  }
  __syncthreads();  // every read of V and G is done
  q = 0;
  for (int n = threadIdx.x; n < P; n += blockDim.x, ++q) {
    G[n] = ut[q];
    V[n] = (lo + (double)(n - off) * slope) * ut[q];
  }
  __syncthreads();
  for (int n = off + threadIdx.x; n < off + bins; n += blockDim.x) {
    double num = 0.0, den = 0.0;
    for (int m = 0; m < P; ++m) {
      const double f = F[(n - m) & mask];
      num += V[m] * f;
      den += G[m] * f;
    }
    E[n - off] = den != 0.0 ? num / den : 0.0;
  }
  if (threadIdx.x == 0) st->slope = slope;
}

__device__ __forceinline__ double sharpened(double u, double lo, double slope, const double* E, int bins) {
  double c = slope > 0.0 ? (u - lo) / slope : 0.0;
  c = c > 0.0 ? c : 0.0;
  const double fi = floor(c);
  if (fi >= (double)(bins - 1)) return E[bins - 1];
  const int i = (int)fi;
  return E[i] + (E[i + 1] - E[i]) * (c - fi);
}

__global__ __launch_bounds__(kN4Threads) void n4_sharpened_kernel(const double* __restrict__ L, int64_t total,
                                                                  const N4State* st, const double* E, int bins,
                                                                  double* out) {
  const double lo = st->umin, slope = st->slope;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
    const double l = L[j];
    out[j] = isfinite(l) ? sharpened(l, lo, slope, E, bins) : (double)NAN;
  }
}

// ------------------------------------------------------------------ BA fit by tiles
// A tile of T[0] x T[1] x T[2] grid points touches only a window of the lattice; its num / den over that
// window are separable contractions (w_k = wz wy wx, sum w^2 = Sz Sy Sx), done in three LDS stages in f64
// and written as the tile's partial.  n4_fold_kernel then sums each control point over the tiles that
// cover it, in tile order.
struct BaPlan {
  int T[3], tiles[3], W[3];
  int64_t ntiles;
  size_t lds, part_doubles;
};

static void ba_windows(const Grid3& g, const int T[3], int W[3], int tiles[3]) {
  for (int a = 0; a < 3; ++a) {
    tiles[a] = (g.n[a] + T[a] - 1) / T[a];
    W[a] = 1;
    for (int t = 0; t < tiles[a]; ++t) {
      const int s = t * T[a], e = std::min(s + T[a], g.n[a]) - 1;
      const int w = axis_span(e, g.n[a], g.lat[a]) - axis_span(s, g.n[a], g.lat[a]) + axis_taps(g.lat[a]);
      W[a] = std::max(W[a], w);
    }
  }
}

static size_t ba_lds(const int T[3], const int W[3]) {
  const size_t pts = (size_t)T[0] * T[1] * T[2];
  const size_t a1 = (size_t)T[0] * T[1] * W[2], a2 = (size_t)T[0] * W[1] * W[2];
  return 2 * 8 * (pts + a1 + a2);
}

static BaPlan ba_plan(const Grid3& g) {
  BaPlan p{};
  for (int a = 0; a < 3; ++a) p.T[a] = g.n[a] == 1 ? 1 : (g.n[0] == 1 ? kBaMaxT : 8);
  for (;;) {
    ba_windows(g, p.T, p.W, p.tiles);
    p.lds = ba_lds(p.T, p.W);
    if (p.lds <= kBaLdsBudget) break;
    int a = -1;  // halve the tile along the axis of the widest window that can still shrink
    for (int b = 0; b < 3; ++b)
      if (p.T[b] > 1 && (a < 0 || p.W[b] > p.W[a])) a = b;
    if (a < 0) break;  // one point per tile: windows of 4, far inside the budget
    p.T[a] /= 2;
  }
  p.ntiles = (int64_t)p.tiles[0] * p.tiles[1] * p.tiles[2];
  p.part_doubles = (size_t)p.ntiles * 2 * p.W[0] * p.W[1] * p.W[2];
  return p;
}

struct BaParams {
  const double* L;       // log values (NaN: not in the fit set), or the residual itself when E is null
  const double* field;   // nullable
  const double* E;       // nullable: r = U - sharpened(U)
  const N4State* st;
  double* part;          // [tile][2][W0 W1 W2]
  Grid3 g;
  int T[3], tiles[3], W[3];
  int bins;
};

__global__ __launch_bounds__(kN4Threads) void n4_ba_kernel(BaParams p) {
  extern __shared__ double sm[];
  __shared__ double tw[3][kBaMaxT][4];
  __shared__ double ts2[3][kBaMaxT];
  __shared__ int toff[3][kBaMaxT];
  __shared__ int tlo[3], tcnt[3], twin[3];
  const int64_t tile = blockIdx.x;
  int tix[3];
  tix[2] = (int)(tile % p.tiles[2]);
  tix[1] = (int)((tile / p.tiles[2]) % p.tiles[1]);
  tix[0] = (int)(tile / ((int64_t)p.tiles[2] * p.tiles[1]));
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    const int s = tix[a] * p.T[a];
    const int c = min(p.T[a], p.g.n[a] - s);
    tcnt[a] = c;
    tlo[a] = axis_span(s, p.g.n[a], p.g.lat[a]);
    twin[a] = axis_span(s + c - 1, p.g.n[a], p.g.lat[a]) - tlo[a] + axis_taps(p.g.lat[a]);
  }
  __syncthreads();
  if (threadIdx.x < 3 * kBaMaxT) {
    const int a = threadIdx.x / kBaMaxT, i = threadIdx.x % kBaMaxT;
    if (i < tcnt[a]) {
      double w[4];
      const int s = axis_weights(tix[a] * p.T[a] + i, p.g.n[a], p.g.lat[a], w);
      toff[a][i] = s - tlo[a];
      double s2 = 0.0;
      for (int k = 0; k < 4; ++k) { tw[a][i][k] = w[k]; s2 += w[k] * w[k]; }
      ts2[a][i] = s2;
    }
  }
  __syncthreads();
  const int cz = tcnt[0], cy = tcnt[1], cx = tcnt[2];
  const int wz = twin[0], wy = twin[1], wx = twin[2];
  const int kz = axis_taps(p.g.lat[0]), ky = axis_taps(p.g.lat[1]), kx = axis_taps(p.g.lat[2]);
  const int npts = p.T[0] * p.T[1] * p.T[2];
  double* an = sm;                                  // alpha (num) [cz][cy][cx]
  double* ad = an + npts;                           // fit-set indicator (den)
  double* b1n = ad + npts;                          // [cz][cy][wx]
  double* b1d = b1n + (size_t)p.T[0] * p.T[1] * p.W[2];
  double* b2n = b1d + (size_t)p.T[0] * p.T[1] * p.W[2];  // [cz][wy][wx]
  double* b2d = b2n + (size_t)p.T[0] * p.W[1] * p.W[2];
  double lo = 0.0, slope = 0.0;
  if (p.E) { lo = p.st->umin; slope = p.st->slope; }
  for (int q = threadIdx.x; q < cz * cy * cx; q += blockDim.x) {
    const int ix = q % cx, iy = (q / cx) % cy, iz = q / (cx * cy);
    const int64_t j = ((int64_t)(tix[0] * p.T[0] + iz) * p.g.n[1] + (tix[1] * p.T[1] + iy)) * p.g.n[2] +
                      (tix[2] * p.T[2] + ix);
    const double l = p.L[j];
    double alpha = 0.0, ind = 0.0;
    if (isfinite(l)) {
      const double u = p.field ? l - p.field[j] : l;
      const double r = p.E ? u - sharpened(u, lo, slope, p.E, p.bins) : u;
      alpha = r / (ts2[0][iz] * ts2[1][iy] * ts2[2][ix]);
      ind = 1.0;
    }
    an[q] = alpha;
    ad[q] = ind;
  }
  __syncthreads();
  // stage 1: contract x
  for (int q = threadIdx.x; q < cz * cy * wx; q += blockDim.x) {
    const int c = q % wx, zy = q / wx;
    double sn = 0.0, sd = 0.0;
    for (int ix = 0; ix < cx; ++ix) {
      const int k = c - toff[2][ix];
      if (k < 0 || k >= kx) continue;
      const double w = tw[2][ix][k], w2 = w * w;
      sn += an[zy * cx + ix] * (w2 * w);
      sd += ad[zy * cx + ix] * w2;
    }
    b1n[q] = sn;
    b1d[q] = sd;
  }
  __syncthreads();
  // stage 2: contract y
  for (int q = threadIdx.x; q < cz * wy * wx; q += blockDim.x) {
    const int c = q % wx, b = (q / wx) % wy, iz = q / (wx * wy);
    double sn = 0.0, sd = 0.0;
    for (int iy = 0; iy < cy; ++iy) {
      const int k = b - toff[1][iy];
      if (k < 0 || k >= ky) continue;
      const double w = tw[1][iy][k], w2 = w * w;
      sn += b1n[(iz * cy + iy) * wx + c] * (w2 * w);
      sd += b1d[(iz * cy + iy) * wx + c] * w2;
    }
    b2n[q] = sn;
    b2d[q] = sd;
  }
  __syncthreads();
  // stage 3: contract z, write the partial
  const int64_t pw = (int64_t)p.W[0] * p.W[1] * p.W[2];
  double* out = p.part + tile * 2 * pw;
  for (int q = threadIdx.x; q < wz * wy * wx; q += blockDim.x) {
    const int c = q % wx, b = (q / wx) % wy, a = q / (wx * wy);
    double sn = 0.0, sd = 0.0;
    for (int iz = 0; iz < cz; ++iz) {
      const int k = a - toff[0][iz];
      if (k < 0 || k >= kz) continue;
      const double w = tw[0][iz][k], w2 = w * w;
      sn += b2n[(iz * wy + b) * wx + c] * (w2 * w);
      sd += b2d[(iz * wy + b) * wx + c] * w2;
    }
    const int64_t o = ((int64_t)a * p.W[1] + b) * p.W[2] + c;
    out[o] = sn;
    out[pw + o] = sd;
  }
}

// lattice[k] += num / den (0 where den is 0).  One workgroup per control point: thread t sums the covering
// tiles t, t + 256, ... (in tile order), then a fixed tree adds the threads' sums.  At level 0 each of the
// 64 control points is covered by every tile, so the tiles are what must be spread over threads.
__global__ __launch_bounds__(kN4Threads) void n4_fold_kernel(BaParams p, double* lattice) {
  __shared__ int s_t0[3], s_t1[3];
  __shared__ double s_num[kN4Threads], s_den[kN4Threads];
  const int64_t k = blockIdx.x;
  int kk[3];
  kk[2] = (int)(k % p.g.lat[2]);
  kk[1] = (int)((k / p.g.lat[2]) % p.g.lat[1]);
  kk[0] = (int)(k / ((int64_t)p.g.lat[2] * p.g.lat[1]));
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    const int ka = a == 0 ? kk[0] : (a == 1 ? kk[1] : kk[2]);
    int t0 = p.tiles[a], t1 = -1;
    for (int t = 0; t < p.tiles[a]; ++t) {
      const int s = t * p.T[a], e = min(s + p.T[a], p.g.n[a]) - 1;
      const int lo = axis_span(s, p.g.n[a], p.g.lat[a]);
      const int hi = axis_span(e, p.g.n[a], p.g.lat[a]) + axis_taps(p.g.lat[a]) - 1;
      if (lo <= ka && ka <= hi) {
        t0 = min(t0, t);
        t1 = t;
      }
    }
    s_t0[a] = t0;
    s_t1[a] = t1;
  }
  __syncthreads();
  const int cz = max(0, s_t1[0] - s_t0[0] + 1), cy = max(0, s_t1[1] - s_t0[1] + 1), cx = max(0, s_t1[2] - s_t0[2] + 1);
  const int64_t pw = (int64_t)p.W[0] * p.W[1] * p.W[2];
  double num = 0.0, den = 0.0;
  for (int i = threadIdx.x; i < cz * cy * cx; i += blockDim.x) {
    const int tx = s_t0[2] + i % cx, ty = s_t0[1] + (i / cx) % cy, tz = s_t0[0] + i / (cx * cy);
    const int oz = kk[0] - axis_span(tz * p.T[0], p.g.n[0], p.g.lat[0]);
    const int oy = kk[1] - axis_span(ty * p.T[1], p.g.n[1], p.g.lat[1]);
    const int ox = kk[2] - axis_span(tx * p.T[2], p.g.n[2], p.g.lat[2]);
    const int64_t tile = ((int64_t)tz * p.tiles[1] + ty) * p.tiles[2] + tx;
    const double* part = p.part + tile * 2 * pw + ((int64_t)oz * p.W[1] + oy) * p.W[2] + ox;
    num += part[0];
    den += part[pw];
  }
  s_num[threadIdx.x] = num;
  s_den[threadIdx.x] = den;
  __syncthreads();
  for (int o = kN4Threads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s_num[threadIdx.x] += s_num[threadIdx.x + o];
      s_den[threadIdx.x] += s_den[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) lattice[k] += s_den[0] > 0.0 ? s_num[0] / s_den[0] : 0.0;
}

// exact cubic subdivision per axis (lat == 1 stays 1)
__global__ __launch_bounds__(kN4Threads) void n4_refine_kernel(const double* __restrict__ c, int lz, int ly, int lx,
                                                               double* __restrict__ f) {
  const int L[3] = {lz, ly, lx};
  int Fd[3];
  for (int a = 0; a < 3; ++a) Fd[a] = L[a] == 1 ? 1 : 2 * (L[a] - 3) + 3;
  const int64_t nf = (int64_t)Fd[0] * Fd[1] * Fd[2];
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nf) return;
  int j[3];
  j[2] = (int)(k % Fd[2]);
  j[1] = (int)((k / Fd[2]) % Fd[1]);
  j[0] = (int)(k / ((int64_t)Fd[2] * Fd[1]));
  int idx[3][3];
  double cf[3][3];
  int nt[3];
  for (int a = 0; a < 3; ++a) {
    if (L[a] == 1) {
      nt[a] = 1; idx[a][0] = 0; cf[a][0] = 1.0;
    } else if (j[a] % 2 == 0) {
      nt[a] = 2; idx[a][0] = j[a] / 2; idx[a][1] = j[a] / 2 + 1; cf[a][0] = cf[a][1] = 0.5;
    } else {
      const int i = (j[a] + 1) / 2;
      nt[a] = 3; idx[a][0] = i - 1; idx[a][1] = i; idx[a][2] = i + 1;
      cf[a][0] = 0.125; cf[a][1] = 0.75; cf[a][2] = 0.125;
    }
  }
  double acc = 0.0;
  for (int a = 0; a < nt[0]; ++a)
    for (int b = 0; b < nt[1]; ++b) {
      double r = 0.0;
      for (int e = 0; e < nt[2]; ++e) r += cf[2][e] * c[((int64_t)idx[0][a] * ly + idx[1][b]) * lx + idx[2][e]];
      acc += cf[0][a] * cf[1][b] * r;
    }
  f[k] = acc;
}

// ------------------------------------------------------------------ full-resolution evaluation
// A block owns R consecutive rows.  Per row, the z / y weights fold the lattice into one row of Lx
// coefficients in f64 (Q, kept as f32 in LDS); each voxel then needs four x taps.  out = x / exp(field)
// when x is given, else the field.  float4 accesses when a row is a whole number of float4.
template <bool VEC>
__global__ __launch_bounds__(kN4Threads) void n4_full_kernel(const double* __restrict__ lat, Grid3 g,
                                                             const float* __restrict__ x, float* __restrict__ out,
                                                             int R) {
  extern __shared__ float q[];  // [R][Lx]
  const int Lx = g.lat[2];
  const int64_t rows = (int64_t)g.n[0] * g.n[1];
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int nr = (int)min((int64_t)R, rows - r0);
  for (int i = threadIdx.x; i < nr * Lx; i += blockDim.x) {
    const int rl = i / Lx, c = i % Lx;
    const int64_t row = r0 + rl;
    const int z = (int)(row / g.n[1]), y = (int)(row % g.n[1]);
    double wz[4], wy[4];
    const int sz = axis_weights(z, g.n[0], g.lat[0], wz);
    const int sy = axis_weights(y, g.n[1], g.lat[1], wy);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int iz = min(sz + a, g.lat[0] - 1), iy = min(sy + b, g.lat[1] - 1);
        acc += wz[a] * wy[b] * lat[((int64_t)iz * g.lat[1] + iy) * Lx + c];
      }
    q[i] = (float)acc;
  }
  __syncthreads();
  const int nx = g.n[2];
  const bool spline = Lx > 1;
  const int m = Lx - 3;
  const float scale = nx > 1 ? (float)((double)m / (double)(nx - 1)) : 0.0f;
  auto field_at = [&](int rl, int xi) -> float {
    const float* qr = q + rl * Lx;
    if (!spline) return qr[0];
    const float u = (float)xi * scale;
    int s = (int)floorf(u);
    s = s < m - 1 ? s : m - 1;
    const float t = u - (float)s;
    const float t2 = t * t, t3 = t2 * t;
    const float w0 = (1.0f - t) * (1.0f - t) * (1.0f - t) / 6.0f;
    const float w1 = (3.0f * t3 - 6.0f * t2 + 4.0f) / 6.0f;
    const float w2 = (-3.0f * t3 + 3.0f * t2 + 3.0f * t + 1.0f) / 6.0f;
    const float w3 = t3 / 6.0f;
    return w0 * qr[s] + w1 * qr[s + 1] + w2 * qr[s + 2] + w3 * qr[s + 3];
  };
  const int64_t base = r0 * nx;
  const int cnt = nr * nx;
  if (VEC) {
    const float4* x4 = reinterpret_cast<const float4*>(x ? x + base : nullptr);
    float4* o4 = reinterpret_cast<float4*>(out + base);
    for (int e4 = threadIdx.x; e4 < cnt / 4; e4 += blockDim.x) {
      const int e = e4 * 4, rl = e / nx, x0 = e - rl * nx;
      float4 f = make_float4(field_at(rl, x0), field_at(rl, x0 + 1), field_at(rl, x0 + 2), field_at(rl, x0 + 3));
      if (x) {
        const float4 v = x4[e4];
        f = make_float4(v.x / expf(f.x), v.y / expf(f.y), v.z / expf(f.z), v.w / expf(f.w));
      }
      o4[e4] = f;
    }
  } else {
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
      const int rl = e / nx, xi = e - rl * nx;
      const float f = field_at(rl, xi);
      out[base + e] = x ? x[base + e] / expf(f) : f;
    }
  }
}

// ------------------------------------------------------------------ CT: median, clamp, scale
__device__ __forceinline__ void cx(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// exact median of 27 values by forgetful selection: keep 15, drop min and max, add one, repeat
__device__ __forceinline__ float median27(const float v[27]) {
  float a[15];
#pragma unroll
  for (int i = 0; i < 15; ++i) a[i] = v[i];
#pragma unroll
  for (int r = 0; r < 13; ++r) {
    const int n = 15 - r;
#pragma unroll
    for (int i = 1; i < n; ++i) cx(a[0], a[i]);
#pragma unroll
    for (int i = 1; i < n - 1; ++i) cx(a[i], a[n - 1]);
    if (r < 12) a[0] = v[15 + r];  // the active set is now a[0 .. n-2]
  }
  return a[1];
}

__global__ __launch_bounds__(kN4Threads) void ct_scale_kernel(const float* __restrict__ x, int nz, int ny, int nx,
                                                              float* __restrict__ out) {
  const int64_t total = (int64_t)nz * ny * nx;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
    const int xi = (int)(j % nx);
    const int64_t r = j / nx;
    const int yi = (int)(r % ny), zi = (int)(r / ny);
    float v[27];
#pragma unroll
    for (int dz = 0; dz < 3; ++dz) {
      const int zz = min(max(zi + dz - 1, 0), nz - 1);
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int yy = min(max(yi + dy - 1, 0), ny - 1);
        const float* row = x + ((int64_t)zz * ny + yy) * nx;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) v[(dz * 3 + dy) * 3 + dx] = row[min(max(xi + dx - 1, 0), nx - 1)];
      }
    }
    float m = median27(v);
    m = fminf(fmaxf(m, -1100.0f), 3100.0f);
    // (v + 1100) * 255 / 4200 as (v + 1100) * fl(255 / 4200): within 1 ulp of the f64 value
    const float t = m + 1100.0f;
    out[j] = t * (float)(255.0 / 4200.0);
  }
}

// ------------------------------------------------------------------ host side
static int red_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(kN4RedBlocks, (n + kN4Threads - 1) / kN4Threads)); }

static int padded_bins(int bins) {
  int p = 1;
  while (p < bins) p *= 2;
  return 2 * p;
}

struct N4Layout {
  size_t state, hist, E, parts, field, lat0, lat1, part, total;
};

static Grid3 level_grid(int nz, int ny, int nx, int spans) {
  Grid3 g{{nz, ny, nx}, {1, 1, 1}};
  for (int a = 0; a < 3; ++a) g.lat[a] = g.n[a] == 1 ? 1 : spans + 3;
  return g;
}

static N4Layout n4_layout(int nz, int ny, int nx, int control_points, int levels, int bins) {
  N4Layout l{};
  const int64_t n = (int64_t)nz * ny * nx;
  size_t maxpart = 0, maxlat = 1;
  for (int lev = 0; lev < levels; ++lev) {
    const Grid3 g = level_grid(nz, ny, nx, (control_points - 3) << lev);
    maxpart = std::max(maxpart, ba_plan(g).part_doubles);
    maxlat = std::max(maxlat, (size_t)g.lat[0] * g.lat[1] * g.lat[2]);
  }
  l.state = 0;
  l.hist = lv_align256(sizeof(N4State));
  l.E = l.hist + lv_align256((size_t)bins * 8);
  l.parts = l.E + lv_align256((size_t)bins * 8);
  l.field = l.parts + lv_align256((size_t)kN4RedBlocks * sizeof(N4Part));
  l.lat0 = l.field + lv_align256((size_t)n * 8);
  l.lat1 = l.lat0 + lv_align256(maxlat * 8);
  l.part = l.lat1 + lv_align256(maxlat * 8);
  l.total = l.part + lv_align256(maxpart * 8);
  return l;
}

static bool n4_dims_ok(int nz, int ny, int nx) {
  return nz >= 1 && ny >= 1 && nx >= 1 && (int64_t)nz * ny * nx < ((int64_t)1 << 40);
}

static int launch_ba(const Grid3& g, const double* L, const double* field, const double* E, const N4State* st,
                     double* part, double* lattice, int bins, hipStream_t s) {
  const BaPlan pl = ba_plan(g);
  if (pl.lds > kBaLdsBudget) {
    set_error("n4: no B-spline tile fits the LDS budget (lattice %d x %d x %d)", g.lat[0], g.lat[1], g.lat[2]);
    return SEGMI_EUNSUPPORTED;
  }
  BaParams p{};
  p.L = L; p.field = field; p.E = E; p.st = st; p.part = part; p.g = g; p.bins = bins;
  for (int a = 0; a < 3; ++a) { p.T[a] = pl.T[a]; p.tiles[a] = pl.tiles[a]; p.W[a] = pl.W[a]; }
  hipLaunchKernelGGL(n4_ba_kernel, dim3((unsigned)pl.ntiles), dim3(kN4Threads), pl.lds, s, p);
  const int64_t nl = (int64_t)g.lat[0] * g.lat[1] * g.lat[2];
  hipLaunchKernelGGL(n4_fold_kernel, dim3((unsigned)nl), dim3(kN4Threads), 0, s, p, lattice);
  SEGMI_LAUNCH_CHECK("n4 B-spline fit");
  return 0;
}

static void launch_sharpen(unsigned long long* hist, N4State* st, int bins, double fwhm, double noise, double* E,
                           hipStream_t s) {
  const int P = padded_bins(bins);
  hipLaunchKernelGGL(n4_sharpen_kernel, dim3(1), dim3(kSharpThreads), (size_t)5 * P * 8, s, hist, st, bins, P, fwhm,
                     noise, E);
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int64_t segmi_otsu_workspace_bytes(int bins) {
  if (bins < 2 || bins > kN4MaxBins) return 0;
  return (int64_t)(256 + lv_align256((size_t)bins * 8));
}

int segmi_otsu(const float* x, int64_t n, int bins, int64_t* counts, double* stats, void* ws, size_t ws_bytes,
               void* stream) {
  SEGMI_CHECK_ARG(x && stats && ws, "otsu: null pointer");
  SEGMI_CHECK_ARG(n > 0 && bins >= 2 && bins <= kN4MaxBins, "otsu: n > 0, 2 <= bins <= %d", kN4MaxBins);
  SEGMI_CHECK_ARG(ws_bytes >= (size_t)segmi_otsu_workspace_bytes(bins), "otsu: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned* keys = (unsigned*)ws;
  unsigned long long* h = (unsigned long long*)((char*)ws + 256);
  hipLaunchKernelGGL(otsu_init_kernel, dim3(1), dim3(kN4Threads), 0, s, keys, h, bins);
  const bool vec = ((uintptr_t)x & 15) == 0;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n / 4 + kN4Threads - 1) / kN4Threads));
  if (vec) {
    hipLaunchKernelGGL(otsu_minmax_kernel<true>, dim3(grid), dim3(kN4Threads), 0, s, x, n, keys);
    hipLaunchKernelGGL(otsu_hist_kernel<true>, dim3(grid), dim3(kN4Threads), 0, s, x, n, keys, bins, h);
  } else {
    hipLaunchKernelGGL(otsu_minmax_kernel<false>, dim3(grid), dim3(kN4Threads), 0, s, x, n, keys);
    hipLaunchKernelGGL(otsu_hist_kernel<false>, dim3(grid), dim3(kN4Threads), 0, s, x, n, keys, bins, h);
  }
  hipLaunchKernelGGL(otsu_pick_kernel, dim3(1), dim3(64), 0, s, keys, h, bins, stats, counts);
  SEGMI_LAUNCH_CHECK("otsu");
  return 0;
}

int segmi_n4_shrink(const float* x, int nz, int ny, int nx, int fz, int fy, int fx, const uint8_t* mask,
                    const double* otsu_stats, int inside, int outside, float* out_img, uint8_t* out_mask,
                    double* out_log, void* stream) {
  SEGMI_CHECK_ARG(x, "n4_shrink: null input");
  SEGMI_CHECK_ARG(n4_dims_ok(nz, ny, nx) && fz >= 1 && fy >= 1 && fx >= 1, "n4_shrink: bad sizes or factors");
  ShrinkParams p{};
  p.x = x; p.mask = mask; p.stats = otsu_stats; p.out_img = out_img; p.out_mask = out_mask; p.out_log = out_log;
  p.sy = nx; p.sz = (int64_t)ny * nx;
  const int n[3] = {nz, ny, nx}, f[3] = {fz, fy, fx};
  for (int a = 0; a < 3; ++a) {
    p.f[a] = f[a];
    p.ns[a] = std::max(1, n[a] / f[a]);
    p.o[a] = (int)floor(((double)(n[a] - 1) - (double)(p.ns[a] - 1) * f[a]) / 2.0 + 0.5);
    // the last gathered index (ns - 1) f + o must lie inside the axis
    SEGMI_CHECK_ARG(p.o[a] >= 0 && (int64_t)(p.ns[a] - 1) * f[a] + p.o[a] < n[a], "n4_shrink: offset out of range");
  }
  p.inside = inside; p.outside = outside;
  const int64_t total = (int64_t)p.ns[0] * p.ns[1] * p.ns[2];
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(65536, (total + kN4Threads - 1) / kN4Threads));
  hipLaunchKernelGGL(n4_shrink_kernel, dim3(grid), dim3(kN4Threads), 0, (hipStream_t)stream, p);
  SEGMI_LAUNCH_CHECK("n4_shrink");
  return 0;
}

int64_t segmi_n4_workspace_bytes(int nz, int ny, int nx, int control_points, int levels, int bins) {
  if (!n4_dims_ok(nz, ny, nx) || control_points < 4 || levels < 1 || levels > 12 || bins < 2 || bins > kN4MaxBins)
    return 0;
  if ((int64_t)(control_points - 3) << (levels - 1) > 4096) return 0;
  return (int64_t)n4_layout(nz, ny, nx, control_points, levels, bins).total;
}

int segmi_n4_fit(const double* logimg, int nz, int ny, int nx, const int* iterations_host, int levels,
                 int control_points, int bins, double fwhm, double noise, double threshold, double* lattice,
                 double* field, int* elapsed_host, double* cv_host, void* ws, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(logimg && iterations_host && lattice && elapsed_host && cv_host && ws, "n4_fit: null pointer");
  const int64_t need = segmi_n4_workspace_bytes(nz, ny, nx, control_points, levels, bins);
  SEGMI_CHECK_ARG(need > 0, "n4_fit: unsupported sizes / levels / control points / bins");
  SEGMI_CHECK_ARG(ws_bytes >= (size_t)need, "n4_fit: workspace of %zu bytes, %lld needed", ws_bytes, (long long)need);
  SEGMI_CHECK_ARG(fwhm > 0.0 && noise >= 0.0, "n4_fit: fwhm > 0 and noise >= 0");
  hipStream_t s = (hipStream_t)stream;
  const N4Layout l = n4_layout(nz, ny, nx, control_points, levels, bins);
  char* w = (char*)ws;
  N4State* st = (N4State*)(w + l.state);
  unsigned long long* hist = (unsigned long long*)(w + l.hist);
  double* E = (double*)(w + l.E);
  N4Part* parts = (N4Part*)(w + l.parts);
  double* fld = (double*)(w + l.field);
  double* lat[2] = {(double*)(w + l.lat0), (double*)(w + l.lat1)};
  double* part = (double*)(w + l.part);
  const int64_t n = (int64_t)nz * ny * nx;
  const int rb = red_blocks(n);
  int spans = control_points - 3;
  Grid3 g = level_grid(nz, ny, nx, spans);
  const size_t nl0 = (size_t)g.lat[0] * g.lat[1] * g.lat[2];
  if (hipMemsetAsync(hist, 0, (size_t)bins * 8, s) != hipSuccess ||
      hipMemsetAsync(lat[0], 0, nl0 * 8, s) != hipSuccess) {
    set_error("n4_fit: workspace initialisation failed");
    return SEGMI_ELAUNCH;
  }
  hipLaunchKernelGGL(n4_eval_kernel, dim3(rb), dim3(kN4Threads), 0, s, logimg, fld, (const double*)nullptr, g, 0,
                     parts);
  hipLaunchKernelGGL(n4_finalise_kernel, dim3(1), dim3(kN4Threads), 0, s, parts, rb, st);
  SEGMI_LAUNCH_CHECK("n4_fit init");
  N4State h{};
  if (hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    set_error("n4_fit: reading the fit-set statistics failed");
    return SEGMI_ELAUNCH;
  }
  if (h.count < 2.0) {
    set_error("n4: the fit set (mask == 1, input > 0, finite) has %.0f voxels; at least 2 are needed", h.count);
    return SEGMI_EDATA;
  }
  if (!(h.umax > h.umin)) {
    set_error("n4: every log value of the fit set is equal (%g); the histogram has no range", h.umin);
    return SEGMI_EDATA;
  }
  int cur = 0;
  double cv = INFINITY;
  for (int lev = 0; lev < levels; ++lev) {
    if (lev > 0) {
      const int64_t nf = (int64_t)(g.lat[0] == 1 ? 1 : 2 * spans + 3) * (g.lat[1] == 1 ? 1 : 2 * spans + 3) *
                         (g.lat[2] == 1 ? 1 : 2 * spans + 3);
      hipLaunchKernelGGL(n4_refine_kernel, dim3((unsigned)((nf + kN4Threads - 1) / kN4Threads)), dim3(kN4Threads), 0, s,
                         lat[cur], g.lat[0], g.lat[1], g.lat[2], lat[1 - cur]);
      cur = 1 - cur;
      spans *= 2;
      g = level_grid(nz, ny, nx, spans);
    }
    int it = 0;
    cv = INFINITY;
    while (it < iterations_host[lev] && cv > threshold) {
      hipLaunchKernelGGL(n4_hist_kernel, dim3(rb), dim3(kN4Threads), 0, s, logimg, (const double*)fld, n,
                         (const N4State*)st, bins, hist);
      launch_sharpen(hist, st, bins, fwhm, noise, E, s);
      const int rc = launch_ba(g, logimg, fld, E, st, part, lat[cur], bins, s);
      if (rc) return rc;
      hipLaunchKernelGGL(n4_eval_kernel, dim3(rb), dim3(kN4Threads), 0, s, logimg, fld, (const double*)lat[cur], g, 1,
                         parts);
      hipLaunchKernelGGL(n4_finalise_kernel, dim3(1), dim3(kN4Threads), 0, s, parts, rb, st);
      SEGMI_LAUNCH_CHECK("n4_fit iteration");
      if (hipMemcpyAsync(&cv, &st->cv, sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess) {
        set_error("n4_fit: reading the convergence value failed");
        return SEGMI_ELAUNCH;
      }
      ++it;
    }
    elapsed_host[lev] = it;
  }
  *cv_host = cv;
  const size_t nl = (size_t)g.lat[0] * g.lat[1] * g.lat[2];
  if (hipMemcpyAsync(lattice, lat[cur], nl * 8, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      (field && hipMemcpyAsync(field, fld, (size_t)n * 8, hipMemcpyDeviceToDevice, s) != hipSuccess)) {
    set_error("n4_fit: copying the results failed");
    return SEGMI_ELAUNCH;
  }
  return 0;
}

int segmi_n4_sharpen(const double* u, int nz, int ny, int nx, int bins, double fwhm, double noise, double* E,
                     double* sharp, void* ws, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(u && E && sharp && ws, "n4_sharpen: null pointer");
  const int64_t need = segmi_n4_workspace_bytes(nz, ny, nx, 4, 1, bins);
  SEGMI_CHECK_ARG(need > 0 && ws_bytes >= (size_t)need, "n4_sharpen: bad sizes or workspace too small");
  SEGMI_CHECK_ARG(fwhm > 0.0 && noise >= 0.0, "n4_sharpen: fwhm > 0 and noise >= 0");
  hipStream_t s = (hipStream_t)stream;
  const N4Layout l = n4_layout(nz, ny, nx, 4, 1, bins);
  char* w = (char*)ws;
  N4State* st = (N4State*)(w + l.state);
  unsigned long long* hist = (unsigned long long*)(w + l.hist);
  N4Part* parts = (N4Part*)(w + l.parts);
  double* fld = (double*)(w + l.field);
  const int64_t n = (int64_t)nz * ny * nx;
  const int rb = red_blocks(n);
  const Grid3 g = level_grid(nz, ny, nx, 1);
  if (hipMemsetAsync(hist, 0, (size_t)bins * 8, s) != hipSuccess) {
    set_error("n4_sharpen: memset failed");
    return SEGMI_ELAUNCH;
  }
  hipLaunchKernelGGL(n4_eval_kernel, dim3(rb), dim3(kN4Threads), 0, s, u, fld, (const double*)nullptr, g, 0, parts);
  hipLaunchKernelGGL(n4_finalise_kernel, dim3(1), dim3(kN4Threads), 0, s, parts, rb, st);
  hipLaunchKernelGGL(n4_hist_kernel, dim3(rb), dim3(kN4Threads), 0, s, u, (const double*)nullptr, n,
                     (const N4State*)st, bins, hist);
  launch_sharpen(hist, st, bins, fwhm, noise, E, s);
  hipLaunchKernelGGL(n4_sharpened_kernel, dim3(rb), dim3(kN4Threads), 0, s, u, n, (const N4State*)st, (const double*)E,
                     bins, sharp);
  SEGMI_LAUNCH_CHECK("n4_sharpen");
  return 0;
}

int segmi_n4_bspline_fit(const double* r, int nz, int ny, int nx, int spans, double* lattice, void* ws,
                         size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(r && lattice && ws, "n4_bspline_fit: null pointer");
  const int64_t need = segmi_n4_workspace_bytes(nz, ny, nx, spans + 3, 1, 2);
  SEGMI_CHECK_ARG(spans >= 1 && need > 0 && ws_bytes >= (size_t)need, "n4_bspline_fit: bad sizes or workspace");
  hipStream_t s = (hipStream_t)stream;
  const N4Layout l = n4_layout(nz, ny, nx, spans + 3, 1, 2);
  const Grid3 g = level_grid(nz, ny, nx, spans);
  const size_t nl = (size_t)g.lat[0] * g.lat[1] * g.lat[2];
  if (hipMemsetAsync(lattice, 0, nl * 8, s) != hipSuccess) {
    set_error("n4_bspline_fit: memset failed");
    return SEGMI_ELAUNCH;
  }
  return launch_ba(g, r, nullptr, nullptr, nullptr, (double*)((char*)ws + l.part), lattice, 2, s);
}

int segmi_n4_refine(const double* coarse, int lz, int ly, int lx, double* fine, void* stream) {
  SEGMI_CHECK_ARG(coarse && fine, "n4_refine: null pointer");
  const int L[3] = {lz, ly, lx};
  int64_t nf = 1;
  for (int a = 0; a < 3; ++a) {
    SEGMI_CHECK_ARG(L[a] == 1 || (L[a] >= 4 && L[a] <= 8192), "n4_refine: lattice sizes are 1 or >= 4");
    nf *= L[a] == 1 ? 1 : 2 * (L[a] - 3) + 3;
  }
  hipLaunchKernelGGL(n4_refine_kernel, dim3((unsigned)((nf + kN4Threads - 1) / kN4Threads)), dim3(kN4Threads), 0,
                     (hipStream_t)stream, coarse, lz, ly, lx, fine);
  SEGMI_LAUNCH_CHECK("n4_refine");
  return 0;
}

int segmi_n4_evaluate(const double* lattice, int lz, int ly, int lx, const float* x, float* out, int nz, int ny,
                      int nx, void* stream) {
  SEGMI_CHECK_ARG(lattice && out, "n4_evaluate: null pointer");
  SEGMI_CHECK_ARG(n4_dims_ok(nz, ny, nx), "n4_evaluate: bad sizes");
  const int L[3] = {lz, ly, lx};
  for (int a = 0; a < 3; ++a)
    SEGMI_CHECK_ARG(L[a] == 1 || (L[a] >= 4 && L[a] <= 8192), "n4_evaluate: lattice sizes are 1 or >= 4");
  const Grid3 g{{nz, ny, nx}, {lz, ly, lx}};
  int R = std::max(1, 16384 / nx);  // 8 float4 per thread at nx = 512: amortises the per-row prologue
  R = std::max(1, std::min(R, 8192 / lx));
  const int64_t rows = (int64_t)nz * ny;
  const int64_t grid = (rows + R - 1) / R;
  SEGMI_CHECK_ARG(grid < ((int64_t)1 << 31), "n4_evaluate: too many rows");
  const bool vec = nx % 4 == 0 && ((uintptr_t)out & 15) == 0 && (!x || ((uintptr_t)x & 15) == 0);
  const size_t lds = (size_t)R * lx * sizeof(float);
  if (vec)
    hipLaunchKernelGGL(n4_full_kernel<true>, dim3((unsigned)grid), dim3(kN4Threads), lds, (hipStream_t)stream, lattice,
                       g, x, out, R);
  else
    hipLaunchKernelGGL(n4_full_kernel<false>, dim3((unsigned)grid), dim3(kN4Threads), lds, (hipStream_t)stream, lattice,
                       g, x, out, R);
  SEGMI_LAUNCH_CHECK("n4_evaluate");
  return 0;
}

int segmi_ct_scale(const float* x, int nz, int ny, int nx, float* out, void* stream) {
  SEGMI_CHECK_ARG(x && out && x != out, "ct_scale: null or aliased pointers");
  SEGMI_CHECK_ARG(n4_dims_ok(nz, ny, nx), "ct_scale: bad sizes");
  const int64_t total = (int64_t)nz * ny * nx;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(65536, (total + kN4Threads - 1) / kN4Threads));
  hipLaunchKernelGGL(ct_scale_kernel, dim3(grid), dim3(kN4Threads), 0, (hipStream_t)stream, x, nz, ny, nx, out);
  SEGMI_LAUNCH_CHECK("ct_scale");
  return 0;
}

}  // extern "C"
