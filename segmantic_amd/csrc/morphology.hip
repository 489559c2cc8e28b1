// morphology.hip -- exact Euclidean feature transform (the index of the nearest feature voxel of every
// voxel) and the element-wise kernels that turn it into label morphology by a physical radius
// (seg/morphology.py; DESIGN.md section 15 defines the results).
//
// Feature transform over a box of bd x bh x bw voxels, one i32 per voxel, every pass in place on `index`:
//   P1 along x : one wave per (z, y) row, lanes over x.  Two sweeps of ballots give the nearest feature
//                column at or left of x and right of x; the nearer one is kept, the left one on a tie.
//                index[z][y][x] = x' (box coordinates), -1 when the row holds no feature.
//   P2 along y : lanes over the (z, x) lines.  Lower envelope (Felzenszwalb-Huttenlocher) of the parabolas
//                (sy (y - q))^2 + (sx (x - x'_q))^2 with the stack [depth][line] in the workspace; the stack
//                keeps (q, x'_q), the heights are recomputed.  index[z][y][x] = y' * bw + x'.
//   P3 along z : lanes over the (y, x) lines, the same envelope over (z', y' * bw + x'); writes the linear
//                index of the winner in the full volume and, optionally, its distance.
// Tie rule: among equally near features the smallest raster index (z, then y, then x) wins.  Each pass
// prefers the smaller coordinate among equal candidates (P1: left; P2 / P3: the fill advances to the next
// parabola only when it is strictly lower) and the outermost pass runs along z, so z dominates y dominates x.
// Arithmetic: with one spacing for all axes every comparison is i64 arithmetic on voxel counts (exact);
// otherwise candidates are compared as the f64 value ((sz dz)^2 + (sy dy)^2) + (sx dx)^2, formed in that
// order with no contraction, so candidates at mirrored offsets compare bit-equal.  P2 alone stays in i64
// whenever sy == sx (thick slices): within a plane the voxel counts order the candidates exactly.
#include "labelvol.h"

namespace segmi {

constexpr int kFtMaxExtent = 1 << 20;   // keeps the i64 products of the exact envelope test below 2^63
constexpr float kMorphInf = __builtin_inff();

enum { kFtNonZero = 0, kFtZero = 1, kFtEqual = 2, kFtNotEqual = 3, kFtTable = 4 };

struct FtParams {
  const void* lab;
  const uint8_t* table;      // mode kFtTable: 65536 bytes, non-zero = feature
  int d, h, w, mode, label;
  int z0, y0, x0, bd, bh, bw;
  int exact;                 // one spacing for all axes: count in voxels, scale by s2 at the end
  double sz, sy, sx, s2;
  int32_t* index;            // [bd][bh][bw]
  float* dist;               // nullable, [bd][bh][bw]
  int dist_sqrt;
  int32_t* sv;               // stack positions [depth][line]
  int32_t* sp;               // stack payloads  [depth][line]
};

__device__ __forceinline__ bool ft_feature(int v, int mode, int label, const uint8_t* table) {
  switch (mode) {
    case kFtNonZero: return v != 0;
    case kFtZero: return v == 0;
    case kFtEqual: return v == label;
    case kFtNotEqual: return v != label;
    default: return (unsigned)v < 65536u && table[v] != 0;
  }
}

// squared physical distance of the offset (dz, dy, dx): the one formula every kernel and the oracle share
__device__ __forceinline__ double ft_dist_sq(int dz, int dy, int dx, int exact, double s2, double sz, double sy,
                                             double sx) {
  if (exact) return (double)((int64_t)dz * dz + (int64_t)dy * dy + (int64_t)dx * dx) * s2;
  const double a = sz * (double)dz, b = sy * (double)dy, c = sx * (double)dx;
  return (a * a + b * b) + c * c;
}

// ------------------------------------------------------------------ P1
template <typename T>
__global__ __launch_bounds__(256) void ft_p1_kernel(FtParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t rows = (int64_t)p.bd * p.bh;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const T* lab = (const T*)p.lab;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nwaves) {
    const int z = (int)(r / p.bh), y = (int)(r % p.bh);
    const T* row = lab + ((int64_t)(p.z0 + z) * p.h + (p.y0 + y)) * p.w + p.x0;
    int32_t* o = p.index + r * p.bw;
    int last = -1;
    for (int c = 0; c < p.bw; c += 64) {
      const int x = c + lane;
      const bool f = x < p.bw && ft_feature((int)row[x], p.mode, p.label, p.table);
      const unsigned long long m = __ballot(f);
      const unsigned long long below = m & ((2ull << lane) - 1ull);     // lanes <= lane (lane 63: all)
      if (x < p.bw) o[x] = below ? c + 63 - __clzll((long long)below) : last;
      if (m) last = c + 63 - __clzll((long long)m);
    }
    int next = -1;
    for (int c = (p.bw - 1) / 64 * 64; c >= 0; c -= 64) {
      const int x = c + lane;
      const bool f = x < p.bw && ft_feature((int)row[x], p.mode, p.label, p.table);
      const unsigned long long m = __ballot(f);
      const unsigned long long above = m >> lane;                       // lanes >= lane
      if (x < p.bw) {
        const int left = o[x];
        const int right = above ? x + __ffsll((long long)above) - 1 : next;
        // the left candidate wins a tie: smaller x
        if (right >= 0 && (left < 0 || right - x < x - left)) o[x] = right;
      }
      if (m) next = c + __ffsll((long long)m) - 1;
    }
  }
}

// ------------------------------------------------------------------ P2 / P3
template <bool EXACT> struct FtH { using type = double; };
template <> struct FtH<true> { using type = int64_t; };

// what a line of P2 (PASS 2: fixed z, x) or P3 (PASS 3: fixed y, x) knows about itself
struct FtLine {
  int y, x, bw;
  double sa, sy, sx;       // spacing along the line, and of the axes the payload spans
};

// the two height terms of the payload found at one position of the line: (sy dy)^2 and (sx dx)^2
// (voxel counts when EXACT).  PASS 2 payloads are x', PASS 3 payloads y' * bw + x'.
template <bool EXACT, int PASS>
__device__ __forceinline__ void ft_heights(const FtLine& l, int pl, typename FtH<EXACT>::type& hy,
                                           typename FtH<EXACT>::type& hx) {
  int dy = 0, dx;
  if (PASS == 2) {
    dx = l.x - pl;
  } else {
    const int py = (int)((unsigned)pl / (unsigned)l.bw);
    dy = l.y - py;
    dx = l.x - (pl - py * l.bw);
  }
  if constexpr (EXACT) {
    hy = (typename FtH<EXACT>::type)((int64_t)dy * dy);
    hx = (typename FtH<EXACT>::type)((int64_t)dx * dx);
  } else {
    const double b = l.sy * (double)dy, c = l.sx * (double)dx;
    hy = (typename FtH<EXACT>::type)(b * b);
    hx = (typename FtH<EXACT>::type)(c * c);
  }
}

// value at sample t of the candidate at position q: ((sa (t - q))^2 + hy) + hx, in that order
template <bool EXACT>
__device__ __forceinline__ typename FtH<EXACT>::type ft_value(const FtLine& l, int t, int q,
                                                              typename FtH<EXACT>::type hy,
                                                              typename FtH<EXACT>::type hx) {
  if constexpr (EXACT) return (typename FtH<EXACT>::type)((int64_t)(t - q) * (t - q)) + hy + hx;
  const double a = l.sa * (double)(t - q);
  return (typename FtH<EXACT>::type)((a * a + (double)hy) + (double)hx);
}

// One line of n samples, in place on io[i * stride]: candidates are the samples with a payload >= 0.
// The first loop builds the lower envelope (b is dropped when the newcomer q takes over no later than b
// itself takes over from a: b is then lowest at one point at most, where a is as low and has the smaller
// coordinate); the second walks it and moves on only to a strictly lower parabola.
template <bool EXACT, int PASS>
__device__ __forceinline__ void ft_envelope_line(const FtParams& p, const FtLine& l, int32_t* io, int64_t stride,
                                                 float* dist, int n, int32_t* sv, int32_t* sp, int64_t nl) {
  using H = typename FtH<EXACT>::type;
  const double w2 = l.sa * l.sa;
  int top = -1;
  int va = 0, vb = 0;        // positions of the two topmost parabolas (a below b)
  H ga = 0, gb = 0;          // their heights
  for (int q = 0; q < n; ++q) {
    const int pl = io[q * stride];
    if (pl < 0) continue;
    H hy, hx;
    ft_heights<EXACT, PASS>(l, pl, hy, hx);
    const H gq = hy + hx;
    while (top >= 1) {
      bool pop;
      const int64_t qb = (int64_t)q * q - (int64_t)vb * vb, ba = (int64_t)vb * vb - (int64_t)va * va;
      if constexpr (EXACT) {
        pop = ((int64_t)(gq - gb) + qb) * (int64_t)(vb - va) <= ((int64_t)(gb - ga) + ba) * (int64_t)(q - vb);
      } else {
        pop = ((double)(gq - gb) + w2 * (double)qb) * (double)(vb - va) <=
              ((double)(gb - ga) + w2 * (double)ba) * (double)(q - vb);
      }
      if (!pop) break;
      --top;
      vb = va; gb = ga;
      if (top >= 1) {
        va = sv[(top - 1) * nl];
        H ay, ax;
        ft_heights<EXACT, PASS>(l, sp[(top - 1) * nl], ay, ax);
        ga = ay + ax;
      }
    }
    ++top;
    sv[top * nl] = q;
    sp[top * nl] = pl;
    va = vb; ga = gb;
    vb = q; gb = gq;
  }
  if (top < 0) {
    for (int t = 0; t < n; ++t) {
      io[t * stride] = -1;
      if (PASS == 3 && dist) dist[t * stride] = kMorphInf;
    }
    return;
  }
  int k = 0;
  int v0 = sv[0], p0 = sp[0], v1 = 0, p1 = 0;
  H hy0, hx0, hy1 = 0, hx1 = 0;
  ft_heights<EXACT, PASS>(l, p0, hy0, hx0);
  if (top >= 1) { v1 = sv[nl]; p1 = sp[nl]; ft_heights<EXACT, PASS>(l, p1, hy1, hx1); }
  for (int t = 0; t < n; ++t) {
    H c0 = ft_value<EXACT>(l, t, v0, hy0, hx0);
    while (k < top) {
      const H c1 = ft_value<EXACT>(l, t, v1, hy1, hx1);
      if (!(c1 < c0)) break;
      ++k; v0 = v1; p0 = p1; hy0 = hy1; hx0 = hx1; c0 = c1;
      if (k < top) { v1 = sv[(k + 1) * nl]; p1 = sp[(k + 1) * nl]; ft_heights<EXACT, PASS>(l, p1, hy1, hx1); }
    }
    if (PASS == 2) {
      io[t * stride] = v0 * p.bw + p0;
    } else {
      const int py = (int)((unsigned)p0 / (unsigned)p.bw), px = p0 - py * p.bw;
      io[t * stride] = (int32_t)(((int64_t)(p.z0 + v0) * p.h + (p.y0 + py)) * p.w + (p.x0 + px));
      if (dist) {
        const double d2 = EXACT ? (double)c0 * p.s2 : (double)c0;
        dist[t * stride] = p.dist_sqrt ? (float)sqrt(d2) : (float)d2;
      }
    }
  }
}

// P2: lanes over the bd*bw (z, x) lines, samples bw apart
template <bool EXACT>
__global__ __launch_bounds__(256) void ft_p2_kernel(FtParams p) {
  const int64_t nl = (int64_t)p.bd * p.bw;
  const int64_t line = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (line >= nl) return;
  const int64_t z = line / p.bw;
  FtLine l;
  l.x = (int)(line % p.bw); l.y = 0; l.bw = p.bw;
  l.sa = p.sy; l.sy = p.sy; l.sx = p.sx;
  ft_envelope_line<EXACT, 2>(p, l, p.index + z * p.bh * p.bw + l.x, p.bw, nullptr, p.bh, p.sv + line, p.sp + line, nl);
}

// P3: lanes over the bh*bw (y, x) lines, samples one plane apart
template <bool EXACT>
__global__ __launch_bounds__(256) void ft_p3_kernel(FtParams p) {
  const int64_t nl = (int64_t)p.bh * p.bw;
  const int64_t line = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (line >= nl) return;
  FtLine l;
  l.y = (int)(line / p.bw); l.x = (int)(line % p.bw); l.bw = p.bw;
  l.sa = p.sz; l.sy = p.sy; l.sx = p.sx;
  ft_envelope_line<EXACT, 3>(p, l, p.index + line, nl, p.dist ? p.dist + line : nullptr, p.bd, p.sv + line,
                             p.sp + line, nl);
}

// ------------------------------------------------------------------ element-wise companions
struct MorphParams {
  const void* lab;
  const int32_t* index;
  int d, h, w, label;
  int z0, y0, x0, bd, bh, bw;
  int exact;
  double sz, sy, sx, s2, r2;
  const void* keep;         // erode select: nullable, voxels with keep != 0 are left alone
  void* out;
  int32_t* planes;
  int ndim;
};

// squared distance from voxel (z, y, x) to the voxel of linear index i
__device__ __forceinline__ double morph_dist_sq(const MorphParams& p, int z, int y, int x, int i) {
  const int hw = p.h * p.w;
  const int iz = i / hw, rem = i - iz * hw, iy = rem / p.w, ix = rem - iy * p.w;
  return ft_dist_sq(z - iz, y - iy, x - ix, p.exact, p.s2, p.sz, p.sy, p.sx);
}

// out[v] = labels[index[v]] for a zero voxel whose nearest feature lies within the radius, else labels[v]
template <typename T>
__global__ __launch_bounds__(256) void morph_gather_kernel(MorphParams p) {
  const int64_t n = (int64_t)p.d * p.h * p.w;
  const T* lab = (const T*)p.lab;
  T* out = (T*)p.out;
  const int hw = p.h * p.w;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    T val = lab[v];
    if (val == 0) {
      const int i = p.index[v];
      if (i >= 0) {
        const int z = (int)(v / hw), rem = (int)(v - (int64_t)z * hw), y = rem / p.w, x = rem - y * p.w;
        if (morph_dist_sq(p, z, y, x, i) <= p.r2) val = lab[i];
      }
    }
    out[v] = val;
  }
}

// out[v] = 0 for the voxels of `label` inside the box whose nearest feature lies within the radius;
// index is the box-shaped result of the feature transform, out holds a copy of the labels; voxels with
// keep[v] != 0 are skipped (closing: the voxels labelled before the dilation never change)
template <typename T>
__global__ __launch_bounds__(256) void morph_erode_kernel(MorphParams p) {
  const int64_t n = (int64_t)p.bd * p.bh * p.bw;
  const T* lab = (const T*)p.lab;
  T* out = (T*)p.out;
  const int bhw = p.bh * p.bw;
  for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < n; b += (int64_t)gridDim.x * 256) {
    const int bz = (int)(b / bhw), rem = (int)(b - (int64_t)bz * bhw), by = rem / p.bw, bx = rem - by * p.bw;
    const int z = p.z0 + bz, y = p.y0 + by, x = p.x0 + bx;
    const int64_t v = ((int64_t)z * p.h + y) * p.w + x;
    if ((int)lab[v] != p.label || (p.keep && ((const T*)p.keep)[v] != 0)) continue;
    const int i = p.index[b];
    if (i >= 0 && morph_dist_sq(p, z, y, x, i) <= p.r2) out[v] = 0;
  }
}

// planes[a][v] = coordinate a of the voxel index[v] (z, y, x; y, x for a 2-D input), -1 where index is -1
__global__ __launch_bounds__(256) void morph_planes_kernel(MorphParams p) {
  const int64_t n = (int64_t)p.d * p.h * p.w;
  const int hw = p.h * p.w;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    const int i = p.index[v];
    int iz = -1, iy = -1, ix = -1;
    if (i >= 0) {
      iz = i / hw;
      const int rem = i - iz * hw;
      iy = rem / p.w;
      ix = rem - iy * p.w;
    }
    if (p.ndim == 3) {
      p.planes[v] = iz; p.planes[n + v] = iy; p.planes[2 * n + v] = ix;
    } else {
      p.planes[v] = iy; p.planes[n + v] = ix;
    }
  }
}

// ------------------------------------------------------------------ host helpers
// the two halves of the feature-transform workspace: the value and the payload of the running envelope
struct FtLayout { size_t sv, sp, total; };
static inline FtLayout ft_layout(int bd, int bh, int bw) {
  LvCarver c;
  FtLayout l;
  l.sv = c.take((size_t)bd * bh * bw * 4);
  l.sp = c.take((size_t)bd * bh * bw * 4);
  l.total = c.off;
  return l;
}

// exact = one spacing for every axis the input has
static inline int morph_exact(const double* s, int sd) { return s[1] == s[2] && (sd == 2 || s[0] == s[1]); }

}  // namespace segmi

using namespace segmi;

#define MORPH_CHECK_VOLUME(what, lb, d, h, w, sd) \
  LV_CHECK_LABEL_BYTES(what, lb);                   \
  LV_CHECK_SPATIAL_DIMS(what, sd, d);               \
  LV_CHECK_VOXELS(what, d, h, w)

extern "C" {

int64_t segmi_feature_transform_workspace_bytes(int bd, int bh, int bw) {
  if (bd <= 0 || bh <= 0 || bw <= 0) return 0;
  return (int64_t)ft_layout(bd, bh, bw).total;
}

int segmi_feature_transform(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int mode,
                            int label, const uint8_t* table, const int32_t* box, const double* spacing_zyx,
                            int32_t* index, float* dist, int dist_sqrt, void* workspace, size_t ws_bytes,
                            void* stream) {
  SEGMI_CHECK_ARG(labels && spacing_zyx && index && workspace, "feature_transform: null pointer");
  MORPH_CHECK_VOLUME("feature_transform", label_bytes, d, h, w, spatial_dims);
  SEGMI_CHECK_ARG(mode >= kFtNonZero && mode <= kFtTable, "feature_transform: mode must be 0 .. 4");
  SEGMI_CHECK_ARG(mode != kFtTable || table, "feature_transform: mode 4 needs the table");
  LV_CHECK_SPACING("feature_transform", spacing_zyx);
  const int32_t whole[6] = {0, d, 0, h, 0, w};
  const int32_t* b = box ? box : whole;
  LV_CHECK_BOX("feature_transform", b, d, h, w);
  FtParams p{};
  p.lab = labels; p.table = table; p.d = d; p.h = h; p.w = w; p.mode = mode; p.label = label;
  p.z0 = b[0]; p.y0 = b[2]; p.x0 = b[4];
  p.bd = b[1] - b[0]; p.bh = b[3] - b[2]; p.bw = b[5] - b[4];
  SEGMI_CHECK_ARG(p.bd <= kFtMaxExtent && p.bh <= kFtMaxExtent && p.bw <= kFtMaxExtent,
                  "feature_transform: an extent above %d", kFtMaxExtent);
  const FtLayout l = ft_layout(p.bd, p.bh, p.bw);
  SEGMI_CHECK_ARG(ws_bytes >= l.total, "feature_transform: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
  p.sz = spacing_zyx[0]; p.sy = spacing_zyx[1]; p.sx = spacing_zyx[2];
  p.exact = morph_exact(spacing_zyx, spatial_dims);
  p.s2 = p.sx * p.sx;
  p.index = index; p.dist = dist; p.dist_sqrt = dist_sqrt;
  p.sv = (int32_t*)((char*)workspace + l.sv);
  p.sp = (int32_t*)((char*)workspace + l.sp);
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)p.bd * p.bh;
  const int g1 = lv_grid(rows, 4, 1 << 20);
#define P1(T) hipLaunchKernelGGL(ft_p1_kernel<T>, g1, 256, 0, st, p)
  LV_BY_LABEL(label_bytes, P1);
#undef P1
  const int g2 = (int)cdiv64((int64_t)p.bd * p.bw, 256), g3 = (int)cdiv64((int64_t)p.bh * p.bw, 256);
  // P2 only orders candidates of one plane: with sy == sx that order is the one of the voxel counts
  // dy^2 + dx^2, whatever sz is.  In f64 the sums (sy dy)^2 + (sx dx)^2 of two offsets that are equally far
  // (3, 4 against 5, 0) can differ in the last bit, and P2 would drop the candidate with the smaller raster
  // index although the full distances P3 compares are bit-equal.
  if (p.exact || p.sy == p.sx)
    hipLaunchKernelGGL(ft_p2_kernel<true>, g2, 256, 0, st, p);
  else
    hipLaunchKernelGGL(ft_p2_kernel<false>, g2, 256, 0, st, p);
  if (p.exact)
    hipLaunchKernelGGL(ft_p3_kernel<true>, g3, 256, 0, st, p);
  else
    hipLaunchKernelGGL(ft_p3_kernel<false>, g3, 256, 0, st, p);
  SEGMI_LAUNCH_CHECK("feature_transform");
  return SEGMI_OK;
}

static int morph_params(MorphParams& p, const char* what, const void* labels, int d, int h, int w, int spatial_dims,
                        const int32_t* index, const double* spacing_zyx, double radius) {
  SEGMI_CHECK_ARG(lv_spacing_ok(spacing_zyx), "%s: spacing must be positive and finite", what);
  if (!(radius >= 0.0)) {
    set_error("%s: the radius must be >= 0 (infinity: no limit)", what);
    return SEGMI_EINVAL;
  }
  p.lab = labels; p.index = index; p.d = d; p.h = h; p.w = w;
  p.sz = spacing_zyx[0]; p.sy = spacing_zyx[1]; p.sx = spacing_zyx[2];
  p.exact = morph_exact(spacing_zyx, spatial_dims);
  p.s2 = p.sx * p.sx;
  p.r2 = radius * radius;
  return SEGMI_OK;
}

int segmi_morph_gather(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims,
                       const int32_t* index, const double* spacing_zyx, double radius, void* out, void* stream) {
  SEGMI_CHECK_ARG(labels && index && spacing_zyx && out, "morph_gather: null pointer");
  MORPH_CHECK_VOLUME("morph_gather", label_bytes, d, h, w, spatial_dims);
  MorphParams p{};
  const int rc = morph_params(p, "morph_gather", labels, d, h, w, spatial_dims, index, spacing_zyx, radius);
  if (rc != SEGMI_OK) return rc;
  p.out = out;
  hipStream_t st = (hipStream_t)stream;
  const int grid = lv_grid((int64_t)d * h * w, 256, 1 << 20);
#define GATHER(T) hipLaunchKernelGGL(morph_gather_kernel<T>, grid, 256, 0, st, p)
  LV_BY_LABEL(label_bytes, GATHER);
#undef GATHER
  SEGMI_LAUNCH_CHECK("morph_gather");
  return SEGMI_OK;
}

int segmi_morph_erode_select(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int label,
                             const int32_t* box, const int32_t* index, const double* spacing_zyx, double radius,
                             const void* keep, void* out, void* stream) {
  SEGMI_CHECK_ARG(labels && index && spacing_zyx && out, "morph_erode_select: null pointer");
  MORPH_CHECK_VOLUME("morph_erode_select", label_bytes, d, h, w, spatial_dims);
  const int32_t whole[6] = {0, d, 0, h, 0, w};
  const int32_t* b = box ? box : whole;
  LV_CHECK_BOX("morph_erode_select", b, d, h, w);
  MorphParams p{};
  const int rc = morph_params(p, "morph_erode_select", labels, d, h, w, spatial_dims, index, spacing_zyx, radius);
  if (rc != SEGMI_OK) return rc;
  p.label = label; p.out = out; p.keep = keep;
  p.z0 = b[0]; p.y0 = b[2]; p.x0 = b[4];
  p.bd = b[1] - b[0]; p.bh = b[3] - b[2]; p.bw = b[5] - b[4];
  hipStream_t st = (hipStream_t)stream;
  const int grid = lv_grid((int64_t)p.bd * p.bh * p.bw, 256, 1 << 20);
#define ERODE(T) hipLaunchKernelGGL(morph_erode_kernel<T>, grid, 256, 0, st, p)
  LV_BY_LABEL(label_bytes, ERODE);
#undef ERODE
  SEGMI_LAUNCH_CHECK("morph_erode_select");
  return SEGMI_OK;
}

int segmi_morph_index_planes(const int32_t* index, int d, int h, int w, int spatial_dims, int32_t* planes,
                             void* stream) {
  SEGMI_CHECK_ARG(index && planes, "morph_index_planes: null pointer");
  MORPH_CHECK_VOLUME("morph_index_planes", 4, d, h, w, spatial_dims);
  MorphParams p{};
  p.index = index; p.d = d; p.h = h; p.w = w; p.planes = planes; p.ndim = spatial_dims;
  hipLaunchKernelGGL(morph_planes_kernel, lv_grid((int64_t)d * h * w, 256, 1 << 20), 256, 0, (hipStream_t)stream, p);
  SEGMI_LAUNCH_CHECK("morph_index_planes");
  return SEGMI_OK;
}

}  // extern "C"
