// conv_shared.h -- what the kernels of the MFMA convolution family have in common at their end: the hand-off
// of a workgroup's per-channel sums to its row of a partial table (BatchNorm statistics, BatchNorm-backward
// sums), and the host-side launch of a 256-thread kernel with dynamic LDS.  The hand-off is used where it leaves
// the kernels' resource tables (-Rpass-analysis=kernel-resource-usage) as they were: the tile transposed kernel,
// the small-Cin kernel and the three-row form of ring3.  The other kernels carry it as their own text (DESIGN.md
// section 4).  The helper's shape (the stated wave range, c4, two functions) exists only to keep those tables:
// after ANY change to it, or a compiler update, compare the tables of every kernel that calls it again.
#pragma once
#include "common.h"
#include "fin_tail.h"

namespace segmi {

// Per-lane channel sums -> the workgroup's row of a [grid.x][ROWS][width] partial table, in two steps that
// every kernel calls back to back from all 256 threads: wg_chan_rows_sum (the lanes' sums -> LDS, closed by a
// barrier) and wg_chan_rows_put (LDS -> the table; fin_tail_run may follow).  They are two functions so that
// the arguments of the second -- table pointer and row width, read from the kernel's parameter block -- are
// evaluated behind the barrier, where the kernels have always read them.
// The lane layout is the MFMA accumulator's: lane (g = lane / 16, r = lane % 16) holds, in row k, the sum
// over its voxels of channel j * 16 + 4 * g + e as sums_k[j][e] (an f32x4[NT], or one f32x4 when NT == 1).
// The order is fixed, so the rows are reproducible bit for bit: row16_sum over the 16 lanes of a group, LDS
// red[wave][ROWS][NT * 16], then the first ROWS * NT * 16 threads add the four waves in the order 0..3.
__device__ __forceinline__ const f32x4& lane_sums(const f32x4& s, int) { return s; }
template <int NT>
__device__ __forceinline__ const f32x4& lane_sums(const f32x4 (&s)[NT], int j) { return s[j]; }

template <int NT, class... S>
__device__ __forceinline__ void wg_chan_rows_sum(int wave, int c4, int r, float* red, const S&... sums) {
  constexpr int ROWS = (int)sizeof...(S);
  __builtin_assume(wave >= 0 && wave < 4);   // (known where the kernels compute it; this is compiled on its own first)
  float* slot = red + c4;                    // of the lane's 4 channels (c4 = 4 * g), inside red[wave][row][NT * 16]
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a[ROWS] = {row16_sum(lane_sums(sums, j)[e])...};
      if (r == 0) {
#pragma unroll
        for (int k = 0; k < ROWS; ++k) slot[(wave * ROWS + k) * NT * 16 + j * 16 + e] = a[k];
      }
    }
  __syncthreads();
}
//   ch0    channel offset of the workgroup's NT * 16 channels inside a row of `width` channels
//   FROW   row FROW is multiplied by factor[channel of the workgroup] before it is written (-1: none)
template <int ROWS, int NT, int FROW = -1>
__device__ __forceinline__ void wg_chan_rows_put(const float* red, float* part, int width, int ch0,
                                                 const float* factor = nullptr) {
  const int tid = threadIdx.x;
  if (tid < ROWS * NT * 16) {
    const int which = tid / (NT * 16), ch = tid % (NT * 16);
    float sacc = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) sacc += red[(w * ROWS + which) * NT * 16 + ch];
    if constexpr (FROW >= 0) {
      if (which == FROW) sacc *= factor[ch];
    }
    fin_store(&part[((int64_t)blockIdx.x * ROWS + which) * width + ch0 + ch], sacc);
  }
}

// Launch of KERN with 256-thread workgroups and `lds` bytes of dynamic LDS; a failed launch is reported
// under `name`.  A kernel gets more than the default 64 KiB of LDS only after its limit has been raised to
// `lds`: that happens here once per instantiation (KERN is a template argument, so `attr_done` is the
// kernel's own), in the first launch for which the caller's rule `raise` holds.
template <auto KERN, class... A>
static int launch_wg256(dim3 grid, size_t lds, bool raise, hipStream_t st, const char* name, const A&... args) {
  static bool attr_done = false;
  if (!attr_done && raise) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    attr_done = true;
  }
  hipLaunchKernelGGL(KERN, grid, 256, lds, st, args...);
  SEGMI_LAUNCH_CHECK(name);
  return SEGMI_OK;
}

}  // namespace segmi
