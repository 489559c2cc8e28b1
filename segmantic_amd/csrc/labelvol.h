// labelvol.h -- the foundation shared by the label-volume translation units (distance, components,
// morphology, surfaces, decimate; landmarks, n4 and nyul take the pieces that apply): workspace carving,
// the host argument checks, the capped grid size, the host-table uploader and the
// workgroup scan.  Everything here is integer arithmetic or a bare comparison, so the header means the same
// in the units compiled with -ffp-contract=off and in those compiled without it.
#pragma once
#include "common.h"

namespace segmi {

// ------------------------------------------------------------------ workspaces
static inline size_t lv_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Carves a workspace into consecutive regions, each rounded up to 256 bytes.  A file describes its layout
// once, as a sequence of take() calls; the *_workspace_bytes function and the launches read the same offsets.
struct LvCarver {
  size_t off = 0;                                // bytes carved so far: the total after the last take()
  size_t take(size_t bytes) { const size_t at = off; off += lv_align256(bytes); return at; }
};

// ------------------------------------------------------------------ host argument checks
static inline bool lv_voxels_ok(int d, int h, int w) {
  return d > 0 && h > 0 && w > 0 && (int64_t)d * h * w < (1ll << 31);
}
// the surface-net lattice has one cell more than voxels along every axis
static inline bool lv_cells_ok(int d, int h, int w) {
  return d > 0 && h > 0 && w > 0 && ((int64_t)d + 1) * ((int64_t)h + 1) * ((int64_t)w + 1) < (1ll << 31);
}
// half-open z0 z1 y0 y1 x0 x1, not empty, inside the volume
static inline bool lv_box_ok(const int32_t* b, int d, int h, int w) {
  return b[0] >= 0 && b[0] < b[1] && b[1] <= d && b[2] >= 0 && b[2] < b[3] && b[3] <= h && b[4] >= 0 &&
         b[4] < b[5] && b[5] <= w;
}
// comparisons only: NaN fails the first, infinity the second
template <typename F>
static inline bool lv_spacing_ok(const F* s) {
  for (int a = 0; a < 3; ++a)
    if (!(s[a] > (F)0) || !(s[a] < (F)__builtin_inf())) return false;
  return true;
}

#define LV_CHECK_LABEL_BYTES(what, lb) \
  SEGMI_CHECK_ARG((lb) == 1 || (lb) == 2 || (lb) == 4, what ": label_bytes must be 1, 2 or 4")
#define LV_CHECK_SPATIAL_DIMS(what, sd, d) \
  SEGMI_CHECK_ARG((sd) == 3 || ((sd) == 2 && (d) == 1), what ": spatial_dims must be 3, or 2 with d == 1")
#define LV_CHECK_VOXELS(what, d, h, w) \
  SEGMI_CHECK_ARG(lv_voxels_ok(d, h, w), what ": extents must be positive with d*h*w < 2^31")
#define LV_CHECK_CELLS(what, d, h, w) \
  SEGMI_CHECK_ARG(lv_cells_ok(d, h, w), what ": extents must be positive with (d+1)(h+1)(w+1) < 2^31")
#define LV_CHECK_BOX(what, b, d, h, w) \
  SEGMI_CHECK_ARG((d) > 0 && (h) > 0 && (w) > 0 && lv_box_ok(b, d, h, w), what ": box outside the volume or empty")
#define LV_CHECK_SPACING(what, s) \
  SEGMI_CHECK_ARG(lv_spacing_ok(s), what ": spacing must be positive and finite")

// ------------------------------------------------------------------ launches
// workgroups for n items at `per` items each, at most `cap` (the kernels stride over the rest), at least 1
static inline int lv_grid(int64_t n, int per, int cap) { return grid_1d(cdiv64(n, per) * 256, cap); }

// A host table reaches the device through kernel arguments, N entries per launch: no staging buffer, no
// copy that would have to outlive the call.  sink(i, e) receives entry i of the table.
template <typename E, int N> struct LvTableChunk { int first, n; E e[N]; };
template <typename E> struct LvStore {
  E* table;
  __device__ void operator()(int i, const E& e) const { table[i] = e; }
};
template <typename E, int N, typename Sink>
__global__ void lv_table_kernel(Sink sink, LvTableChunk<E, N> c) {
  if ((int)threadIdx.x < c.n) sink(c.first + (int)threadIdx.x, c.e[threadIdx.x]);
}
template <int N, typename E, typename Sink>
static void lv_upload_table(const E* host, int n, Sink sink, hipStream_t st) {
  for (int i = 0; i < n; i += N) {
    LvTableChunk<E, N> c{};
    c.first = i;
    c.n = n - i < N ? n - i : N;
    for (int j = 0; j < c.n; ++j) c.e[j] = host[i + j];
    hipLaunchKernelGGL((lv_table_kernel<E, N, Sink>), 1, N, 0, st, sink, c);
  }
}

// ------------------------------------------------------------------ scans
// Exclusive prefix of v over the BLOCK threads of the workgroup, in thread order (Hillis-Steele in LDS).
// T is an integer or an integer vector; s holds BLOCK words and ends with the inclusive prefixes, so
// s[BLOCK - 1] is the workgroup's sum.  Every thread of the workgroup calls it.
template <int BLOCK, typename T>
__device__ __forceinline__ T lv_block_scan(T v, T* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int o = 1; o < BLOCK; o <<= 1) {
    const T add = t >= o ? s[t - o] : T{};
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  return s[t] - v;
}

// Exclusive scan, in place and by one workgroup of 1024, of nb rows of COLS interleaved 32-bit block sums
// (two's complement: int32 and uint32 alike).  Sums are formed in 64 bits.  Row nb receives the totals;
// `copy` (nullable) receives them too.  With `overflow` (nullable, one word) a total above 2^31 - 1 sets
// the word to 1 and all totals to 0; it is 0 otherwise.
template <int COLS>
__global__ __launch_bounds__(1024) void lv_scan_partials_kernel(uint32_t* partials, int64_t nb, uint32_t* copy,
                                                                uint32_t* overflow) {
  typedef unsigned long long Acc __attribute__((ext_vector_type(COLS)));
  __shared__ Acc sums[1024];
  const int64_t per = (nb + 1023) / 1024, b0 = threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
  Acc s{};
  for (int64_t b = b0; b < b1; ++b)
    for (int c = 0; c < COLS; ++c) s[c] += partials[COLS * b + c];
  Acc run = lv_block_scan<1024>(s, sums);
  for (int64_t b = b0; b < b1; ++b)
    for (int c = 0; c < COLS; ++c) {
      const uint32_t cnt = partials[COLS * b + c];
      partials[COLS * b + c] = (uint32_t)run[c];
      run[c] += cnt;
    }
  if (threadIdx.x == 1023) {
    bool over = false;
    for (int c = 0; c < COLS; ++c) over |= overflow && sums[1023][c] > 0x7fffffffull;
    for (int c = 0; c < COLS; ++c) {
      const uint32_t total = over ? 0u : (uint32_t)sums[1023][c];
      partials[COLS * nb + c] = total;
      if (copy) copy[c] = total;
    }
    if (overflow) *overflow = over ? 1u : 0u;
  }
}

}  // namespace segmi
