// landmarks.hip -- vertebra-landmark transforms on the GPU: per-label centroid sums of a label volume,
// the closed-form Gaussian heatmap written from them, the per-channel max and first argmax of a heatmap,
// and the bounding box of the positive voxels.
// Replaces the per-label torch.where / GaussianSmooth / ScaleIntensity loop, the numpy max + np.where and
// generate_spatial_bounding_box of src/segmantic/detect/transforms.py.
//
// Arrays are [C][D][H][W] = [C][z][y][x]; every kernel is a row walker: one wave per row (c, z, y), lanes
// along x, so z and y are known per row and no kernel divides per voxel.  All four passes are bound by
// HBM bandwidth; none of the entry points synchronises with the host.
#include "labelvol.h"

namespace segmi {

constexpr int kLmMaxLabels = 255;      // label values 0 .. K, K <= 255
constexpr int kHmTailOff = 4;          // heatmap parameter buffer, in 32-bit words: K, S, gamma, 0,
constexpr int kHmTabOff = 4 + 256;     // tails[256] (by label), then f32 tables [K + 1][S]
constexpr int kLmMaxWgs = 4096;

template <typename T> struct Vec4Of;
template <> struct Vec4Of<uint8_t> { typedef uint32_t type; };
template <> struct Vec4Of<int16_t> { typedef uint2 type; };
template <> struct Vec4Of<int32_t> { typedef uint4 type; };
template <> struct Vec4Of<float> { typedef uint4 type; };

// four consecutive elements by one 4-, 8- or 16-byte load
template <typename T>
__device__ __forceinline__ void load4(const T* p, T (&v)[4]) {
  const typename Vec4Of<T>::type raw = *reinterpret_cast<const typename Vec4Of<T>::type*>(p);
  __builtin_memcpy(v, &raw, sizeof(raw));
}

// sum of the bit positions set in m
__device__ __forceinline__ unsigned bitpos_sum(unsigned long long m) {
  return __popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2u * __popcll(m & 0xCCCCCCCCCCCCCCCCull) +
         4u * __popcll(m & 0xF0F0F0F0F0F0F0F0ull) + 8u * __popcll(m & 0xFF00FF00FF00FF00ull) +
         16u * __popcll(m & 0xFFFF0000FFFF0000ull) + 32u * __popcll(m & 0xFFFFFFFF00000000ull);
}

// ------------------------------------------------------------------ centroid sums
// sums u64 [K + 1][4] = (count, sum x, sum y, sum z) per label; a label outside [0, K] sets *flag.
// Each lane holds V consecutive x (V = 4 when W % 4 == 0, else 1).  Per chunk of 64 V voxels the wave
// walks the distinct labels with ballots (vertebrae are contiguous, so one or two per chunk); for label c
// and sub-element j the ballot mask m_j gives count = popc(m_j) and sum x = popc(m_j) (x0 + j) + V *
// bitpos_sum(m_j).  One lane folds that into the workgroup's LDS table, and each workgroup adds its table
// to the global one with one u64 atomic per (label, field) it touched.  Integer sums: deterministic.
template <typename T, int V>
__global__ __launch_bounds__(256) void centroid_kernel(const T* __restrict__ lab, int d, int h, int w, int k,
                                                       unsigned long long* sums, int* flag) {
  __shared__ unsigned long long s_tab[(kLmMaxLabels + 1) * 4];
  for (int i = threadIdx.x; i < (k + 1) * 4; i += 256) s_tab[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int rows = d * h;
  bool bad = false;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
    const int z = r / h, y = r - z * h;
    const T* row = lab + (int64_t)r * w;
    for (int x0 = 0; x0 < w; x0 += 64 * V) {
      const int x = x0 + lane * V;
      int v[V];
      if (x < w) {
        if constexpr (V == 4) {
          T t[4];
          load4(row + x, t);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = (int)t[j];
        } else {
          v[0] = (int)row[x];
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = 0;
      }
      unsigned pend = 0;   // sub-elements of this lane still to fold in
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const bool ok = x < w && v[j] >= 0 && v[j] <= k;
        bad |= x < w && !ok;
        pend |= (unsigned)ok << j;
      }
      unsigned long long todo = __ballot(pend != 0);
      while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        int mine = -1;   // this lane's first pending label (a select chain: no indexed register array)
#pragma unroll
        for (int j = V - 1; j >= 0; --j) mine = ((pend >> j) & 1u) ? v[j] : mine;
        const int c = __shfl(mine, lead);
        unsigned cnt = 0;
        unsigned long long sx = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const bool hit = ((pend >> j) & 1u) && v[j] == c;
          const unsigned long long m = __ballot(hit);
          pend &= ~((unsigned)hit << j);
          const unsigned n = __popcll(m);
          cnt += n;
          sx += (unsigned long long)n * (unsigned)(x0 + j) + (unsigned long long)V * bitpos_sum(m);
        }
        todo = __ballot(pend != 0);
        if (lane == lead) {
          unsigned long long* e = s_tab + c * 4;
          atomicAdd(e + 0, (unsigned long long)cnt);
          atomicAdd(e + 1, sx);
          atomicAdd(e + 2, (unsigned long long)cnt * (unsigned)y);
          atomicAdd(e + 3, (unsigned long long)cnt * (unsigned)z);
        }
      }
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(flag, 1);
  __syncthreads();
  for (int c = threadIdx.x; c <= k; c += 256) {
    const unsigned long long* e = s_tab + c * 4;
    if (e[0] == 0) continue;
#pragma unroll
    for (int f = 0; f < 4; ++f) atomicAdd(sums + c * 4 + f, e[f]);
  }
}

// ------------------------------------------------------------------ heatmap
// Channel c's closed form, set up once per thread from the centroid sums: centre = floor(mean index),
// support = centre +- tail clipped to the volume (x: the centre slice only unless smooth_3d), P = kz * ky
// * kx (kx = 1 off the smoothed form), H = (P - min P) / (max P - min P) * gamma with min / max P over the
// whole channel taken from the clipped kernel ranges (min P = 0 unless the support covers the volume).
struct HmChan {
  bool on;
  int lo[3], hi[3], ctr[3];
  const float* tab[3];   // tab[a][i - ctr[a]] for i in [lo[a], hi[a]]
  float mn, den, gamma;
};

__device__ __forceinline__ float hm_k(const HmChan& ch, int a, int i) {
  return ch.tab[a] ? ch.tab[a][i - ch.ctr[a]] : 1.0f;
}

__device__ HmChan hm_setup(const int* prm, const unsigned long long* sums, const int* flag, int c, int d, int h,
                           int w, bool smooth3d) {
  HmChan ch;
  ch.on = false;
  const int k = prm[0], s = prm[1];
  const unsigned long long n = sums[c * 4];
  if (c == 0 || c > k || n == 0 || *flag != 0) return ch;
  const int t = prm[kHmTailOff + c];
  const float* tab = reinterpret_cast<const float*>(prm + kHmTabOff) + (size_t)c * s + t;  // tab[0] = peak
  const int ext[3] = {w, h, d};
  float mx = 1.0f, mn = 1.0f;
  bool covers = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int ctr = (int)(sums[c * 4 + 1 + a] / n);
    const int ta = (a == 0 && !smooth3d) ? 0 : t;
    ch.ctr[a] = ctr;
    ch.lo[a] = max(ctr - ta, 0);
    ch.hi[a] = min(ctr + ta, ext[a] - 1);
    ch.tab[a] = (a == 0 && !smooth3d) ? nullptr : tab;
    covers = covers && ch.lo[a] == 0 && ch.hi[a] == ext[a] - 1;
  }
  // the same product order as the voxel values (built with -ffp-contract=off: no product is fused into the
  // subtraction), so the centre maps to exactly gamma and the minimum to exactly 0
  float amx[3], amn[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    amx[a] = 0.0f; amn[a] = __builtin_inff();
    for (int i = ch.lo[a]; i <= ch.hi[a]; ++i) {
      const float v = hm_k(ch, a, i);
      amx[a] = fmaxf(amx[a], v); amn[a] = fminf(amn[a], v);
    }
  }
  mx = amx[2] * amx[1] * amx[0];
  mn = covers ? amn[2] * amn[1] * amn[0] : 0.0f;
  ch.mn = mn;
  ch.den = mx - mn;
  ch.gamma = __int_as_float(prm[2]);
  ch.on = ch.den != 0.0f;   // a constant channel scales to 0
  return ch;
}

__device__ __forceinline__ float hm_value(const HmChan& ch, int z, int y, int x) {
  if (x < ch.lo[0] || x > ch.hi[0]) return 0.0f;
  const float p = hm_k(ch, 2, z) * hm_k(ch, 1, y) * hm_k(ch, 0, x);
  return (p - ch.mn) / ch.den * ch.gamma;
}

// out f32 [K + 1][D][H][W]; blockIdx.y = channel, waves over rows (z, y), lanes over x (a float4 each
// when W % 4 == 0).  Rows outside the channel's support box are stored as zeros with no arithmetic.
template <bool V4>
__global__ __launch_bounds__(256) void heatmap_kernel(const int* __restrict__ prm,
                                                      const unsigned long long* __restrict__ sums,
                                                      const int* __restrict__ flag, int d, int h, int w,
                                                      int smooth3d, float* __restrict__ out) {
  const int c = blockIdx.y;
  const HmChan ch = hm_setup(prm, sums, flag, c, d, h, w, smooth3d != 0);
  const int lane = threadIdx.x & 63;
  const int rows = d * h;
  float* base = out + (size_t)c * rows * w;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
    const int z = r / h, y = r - z * h;
    float* row = base + (size_t)r * w;
    const bool live = ch.on && z >= ch.lo[2] && z <= ch.hi[2] && y >= ch.lo[1] && y <= ch.hi[1];
    if (V4) {
      for (int x = lane * 4; x < w; x += 256) {
        f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = hm_value(ch, z, y, x + j);
        }
        *reinterpret_cast<f32x4*>(row + x) = o;
      }
    } else {
      for (int x = lane; x < w; x += 64) row[x] = live ? hm_value(ch, z, y, x) : 0.0f;
    }
  }
}

// ------------------------------------------------------------------ max and first argmax
// key = orderable(value) << 32 | (0xFFFFFFFF - lexkey), lexkey = (x H + y) D + z: the u64 max is the
// channel max and, among equal values, the lexicographically smallest (x, y, z).  -0.0 is read as +0.0,
// NaN is left out of the max and sets nan[c].
__device__ __forceinline__ unsigned orderable(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool V4>
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ x_, int d, int h, int w,
                                                     unsigned long long* keys, int* nan) {
  __shared__ unsigned long long s_best[4];
  const int c = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = d * h;
  const unsigned hd = (unsigned)h * (unsigned)d;
  const float* base = x_ + (size_t)c * rows * w;
  unsigned long long best = 0;
  bool saw_nan = false;
  for (int r = blockIdx.x * 4 + wave; r < rows; r += gridDim.x * 4) {
    const int z = r / h, y = r - z * h;
    const float* row = base + (size_t)r * w;
    const unsigned lex_row = (unsigned)y * (unsigned)d + (unsigned)z;
    constexpr int V = V4 ? 4 : 1;
    for (int x = lane * V; x < w; x += 64 * V) {
      float v[V];
      if constexpr (V4) load4(row + x, v);
      else v[0] = row[x];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float f = v[j] + 0.0f;   // -0.0 + 0.0 = +0.0
        saw_nan |= f != f;
        const unsigned lex = (unsigned)(x + j) * hd + lex_row;
        const unsigned long long key = ((unsigned long long)orderable(f) << 32) | (0xFFFFFFFFu - lex);
        best = (f == f && key > best) ? key : best;
      }
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long b = __shfl_xor(best, o);
    best = b > best ? b : best;
  }
  if (__ballot(saw_nan) && lane == 0) atomicOr(nan + c, 1);
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b = s_best[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) b = s_best[i] > b ? s_best[i] : b;
    if (b) atomicMax(keys + c, b);
  }
}

// ------------------------------------------------------------------ positive bounding box
// box i32[6]: accumulated as (min x, min y, min z, max x, max y, max z) inclusive, finalised half-open as
// (x0, y0, z0, x1, y1, z1); an image without a positive voxel gives six zeros.
__global__ void pbox_init_kernel(int32_t* box) {
  if (threadIdx.x < 6) box[threadIdx.x] = threadIdx.x < 3 ? 0x7fffffff : -1;
}

__global__ void pbox_fin_kernel(int32_t* box) {
  if (threadIdx.x != 0) return;
  const bool empty = box[3] < 0;
  for (int a = 0; a < 6; ++a) box[a] = empty ? 0 : (a < 3 ? box[a] : box[a] + 1);
}

template <typename T>
__device__ __forceinline__ bool positive(T v) { return v > T(0); }   // NaN and -0.0 are not

// rows (c, z, y) over all channels; each lane keeps its own extremes, reduced over the wave and the
// workgroup before six global atomics.
template <typename T, int V>
__global__ __launch_bounds__(256) void pbox_kernel(const T* __restrict__ x_, int rows, int d, int h, int w,
                                                   int32_t* box) {
  __shared__ int s_e[4][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int e[6] = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1};
  for (int r = blockIdx.x * 4 + wave; r < rows; r += gridDim.x * 4) {
    const int zy = r % (d * h);
    const int z = zy / h, y = zy - z * h;
    const T* row = x_ + (int64_t)r * w;
    int xmin = 0x7fffffff, xmax = -1;
    for (int x = lane * V; x < w; x += 64 * V) {
      T v[V];
      if constexpr (V == 4) load4(row + x, v);
      else v[0] = row[x];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (positive(v[j])) { xmin = min(xmin, x + j); xmax = max(xmax, x + j); }
      }
    }
    if (xmax >= 0) {
      e[0] = min(e[0], xmin); e[3] = max(e[3], xmax);
      e[1] = min(e[1], y); e[4] = max(e[4], y);
      e[2] = min(e[2], z); e[5] = max(e[5], z);
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      e[a] = min(e[a], __shfl_xor(e[a], o));
      e[a + 3] = max(e[a + 3], __shfl_xor(e[a + 3], o));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) s_e[wave][a] = e[a];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    int v = s_e[0][a];
#pragma unroll
    for (int i = 1; i < 4; ++i) v = a < 3 ? min(v, s_e[i][a]) : max(v, s_e[i][a]);
    if (s_e[0][3] >= 0 || s_e[1][3] >= 0 || s_e[2][3] >= 0 || s_e[3][3] >= 0) {
      if (a < 3) atomicMin(box + a, v);
      else atomicMax(box + a, v);
    }
  }
}

static inline int lm_grid(int rows, int channels) {
  int g = cdiv(rows, 4);
  const int cap = kLmMaxWgs / (channels > 0 ? channels : 1);
  if (g > cap) g = cap > 0 ? cap : 1;
  return g;
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int segmi_label_centroids(const void* labels, int label_bytes, int d, int h, int w, int k, int64_t* sums,
                          int32_t* flag, void* stream) {
  SEGMI_CHECK_ARG(labels && sums && flag, "label_centroids: null pointer");
  LV_CHECK_LABEL_BYTES("label_centroids", label_bytes);
  SEGMI_CHECK_ARG(d > 0 && h > 0 && w > 0 && (int64_t)d * h < (1ll << 31), "label_centroids: bad extents");
  SEGMI_CHECK_ARG(k >= 0 && k <= kLmMaxLabels, "label_centroids: 0 <= k <= %d", kLmMaxLabels);
  hipStream_t st = (hipStream_t)stream;
  hipMemsetAsync(sums, 0, sizeof(int64_t) * 4 * (k + 1), st);
  hipMemsetAsync(flag, 0, sizeof(int32_t), st);
  const int grid = lm_grid(d * h, 1);
  unsigned long long* s = (unsigned long long*)sums;
  const bool v4 = w % 4 == 0 && ((uintptr_t)labels % (4 * label_bytes)) == 0;
#define CENT(T)                                                                                          \
  do {                                                                                                   \
    if (v4) hipLaunchKernelGGL((centroid_kernel<T, 4>), grid, 256, 0, st, (const T*)labels, d, h, w, k, s, flag); \
    else hipLaunchKernelGGL((centroid_kernel<T, 1>), grid, 256, 0, st, (const T*)labels, d, h, w, k, s, flag); \
  } while (0)
  LV_BY_LABEL(label_bytes, CENT);
#undef CENT
  SEGMI_LAUNCH_CHECK("label_centroids");
  return SEGMI_OK;
}

int segmi_vert_heatmap(const int32_t* params, int k, const int64_t* sums, const int32_t* flag, int d, int h,
                       int w, int smooth_3d, float* out, void* stream) {
  SEGMI_CHECK_ARG(params && sums && flag && out, "vert_heatmap: null pointer");
  SEGMI_CHECK_ARG(d > 0 && h > 0 && w > 0 && (int64_t)d * h < (1ll << 31), "vert_heatmap: bad extents");
  SEGMI_CHECK_ARG(k >= 0 && k <= kLmMaxLabels, "vert_heatmap: 0 <= k <= %d", kLmMaxLabels);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(lm_grid(d * h, k + 1), k + 1);
  const bool v4 = w % 4 == 0 && ((uintptr_t)out % 16) == 0;
  if (v4) hipLaunchKernelGGL(heatmap_kernel<true>, grid, 256, 0, st, params, (const unsigned long long*)sums,
                             flag, d, h, w, smooth_3d, out);
  else hipLaunchKernelGGL(heatmap_kernel<false>, grid, 256, 0, st, params, (const unsigned long long*)sums,
                          flag, d, h, w, smooth_3d, out);
  SEGMI_LAUNCH_CHECK("vert_heatmap");
  return SEGMI_OK;
}

int segmi_channel_argmax(const float* x, int c, int d, int h, int w, uint64_t* keys, int32_t* nan,
                         void* stream) {
  SEGMI_CHECK_ARG(x && keys && nan, "channel_argmax: null pointer");
  SEGMI_CHECK_ARG(c > 0 && c <= 65535, "channel_argmax: 1 <= channels <= 65535");
  SEGMI_CHECK_ARG(d > 0 && h > 0 && w > 0 && (int64_t)d * h < (1ll << 31), "channel_argmax: bad extents");
  SEGMI_CHECK_ARG((int64_t)d * h * w < (1ll << 32), "channel_argmax: a channel holds 2^32 voxels or more");
  hipStream_t st = (hipStream_t)stream;
  hipMemsetAsync(keys, 0, sizeof(uint64_t) * c, st);
  hipMemsetAsync(nan, 0, sizeof(int32_t) * c, st);
  const dim3 grid(lm_grid(d * h, c), c);
  const bool v4 = w % 4 == 0 && ((uintptr_t)x % 16) == 0;
  if (v4) hipLaunchKernelGGL(argmax_kernel<true>, grid, 256, 0, st, x, d, h, w, (unsigned long long*)keys, nan);
  else hipLaunchKernelGGL(argmax_kernel<false>, grid, 256, 0, st, x, d, h, w, (unsigned long long*)keys, nan);
  SEGMI_LAUNCH_CHECK("channel_argmax");
  return SEGMI_OK;
}

int segmi_positive_bbox(const void* x, int dtype_bytes, int is_float, int c, int d, int h, int w, int32_t* box,
                        void* stream) {
  SEGMI_CHECK_ARG(x && box, "positive_bbox: null pointer");
  SEGMI_CHECK_ARG(dtype_bytes == 1 || dtype_bytes == 2 || dtype_bytes == 4, "positive_bbox: 1, 2 or 4 bytes");
  SEGMI_CHECK_ARG(!is_float || dtype_bytes == 4, "positive_bbox: float data is f32");
  SEGMI_CHECK_ARG(c > 0 && d > 0 && h > 0 && w > 0 && (int64_t)c * d * h < (1ll << 31),
                  "positive_bbox: bad extents");
  hipStream_t st = (hipStream_t)stream;
  const int rows = c * d * h;
  const int grid = lm_grid(rows, 1);
  hipLaunchKernelGGL(pbox_init_kernel, 1, 64, 0, st, box);
  const bool v4 = w % 4 == 0 && ((uintptr_t)x % (4 * dtype_bytes)) == 0;
#define PBOX(T)                                                                                          \
  do {                                                                                                   \
    if (v4) hipLaunchKernelGGL((pbox_kernel<T, 4>), grid, 256, 0, st, (const T*)x, rows, d, h, w, box);  \
    else hipLaunchKernelGGL((pbox_kernel<T, 1>), grid, 256, 0, st, (const T*)x, rows, d, h, w, box);     \
  } while (0)
  if (is_float) PBOX(float);
  else LV_BY_LABEL(dtype_bytes, PBOX);
#undef PBOX
  hipLaunchKernelGGL(pbox_fin_kernel, 1, 64, 0, st, box);
  SEGMI_LAUNCH_CHECK("positive_bbox");
  return SEGMI_OK;
}

}  // extern "C"
