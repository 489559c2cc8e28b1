// mi_sampling.h -- the sampling core of registration by mutual information, shared by registration.hip (affine
// candidates) and deformable.hip (B-spline candidates): the workgroup's table of counters in LDS and its flush, the
// trilinear value (and gradient) of the moving image at a continuous index, the two fixed-point atomics of a sample,
// and the body of the joint-histogram kernel over a coordinate policy.  Both files are built with -ffp-contract=off:
// everything here is float64 with every operation rounded on its own, in the order written.
//
// The joint histogram: grid (x = voxel blocks under the caller's grid cap, y = candidate groups).  A workgroup keeps
// ONE table of 32-bit counters per candidate of its group in LDS (kHistLdsCounters in all) and strides over the fixed
// voxels; a voxel's bin is loaded once and serves every candidate of the group.  One trip of the stride loop adds at
// most 256 samples * 2^16 = 2^24 to a counter, so the table is flushed into the global int64 table (device-scope
// integer atomics) every kHistFlushTrips = 128 trips (<= 2^31 per counter) and at the end.  Every sum that crosses
// lanes is an integer (sample weights are fixed point, unit 2^16), so a table does not depend on launch shape or
// arrival order.  No wave-private copies: LDS executes one wave's atomic instruction at a time, so copies remove no
// same-cell serialisation inside a wave (where a smooth image puts it) and would cut the group to a quarter, i.e.
// four times the passes over the fixed bins and the index arithmetic.
#pragma once
#include "common.h"

namespace segmi {

typedef unsigned long long u64;

constexpr int kHistLdsCounters = 8192;   // 32 KB of u32: 32 / 8 / 2 candidates at 16 / 32 / 64 bins
constexpr int kHistFlushTrips = 128;     // 128 trips * 256 lanes * 2^16 = 2^31 < 2^32

// candidates per workgroup (0: bins is not 16, 32 or 64), never more than the entry point's cap per launch
static inline int hist_group(int bins, int max_candidates) {
  if (bins != 16 && bins != 32 && bins != 64) return 0;
  const int g = kHistLdsCounters / (bins * bins);
  return g > max_candidates ? max_candidates : g;
}

// table [group][B][B] of the workgroup added into the global one and cleared; every lane calls it
__device__ __forceinline__ void hist_flush(unsigned* lds, u64* __restrict__ out, int entries) {
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

// the histogram's inside domain: 0 <= c <= dim - 1 on every axis; no default value, no border clamp
__device__ __forceinline__ bool mi_inside(int mx, int my, int mz, double cx, double cy, double cz) {
  const double hx = (double)(mx - 1), hy = (double)(my - 1), hz = (double)(mz - 1);
  return cx >= 0.0 && cx <= hx && cy >= 0.0 && cy <= hy && cz >= 0.0 && cz <= hz;
}

// Trilinear value of mov [mz][my][mx] at a continuous index inside (mi_inside); the upper tap of the last voxel is
// clamped onto it, with weight 0.  Corner order as resample_tap (pixel_traits.h): bit d of the corner = dim d, added
// from 0 ascending.  GRAD: also d value / d c into grad[3], corner by corner in the same order.
template <typename P, bool GRAD>
__device__ __forceinline__ double mi_sample(const P* __restrict__ mov, int mx, int my, int mz, double cx, double cy,
                                            double cz, double* grad) {
  const double fx0 = floor(cx), fy0 = floor(cy), fz0 = floor(cz);
  const int x0 = (int)fx0, y0 = (int)fy0, z0 = (int)fz0;
  const double fx = cx - fx0, fy = cy - fy0, fz = cz - fz0;
  const int x1 = x0 + 1 > mx - 1 ? mx - 1 : x0 + 1;
  const int y1 = y0 + 1 > my - 1 ? my - 1 : y0 + 1;
  const int z1 = z0 + 1 > mz - 1 ? mz - 1 : z0 + 1;
  double v = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
#pragma unroll
  for (int corner = 0; corner < 8; ++corner) {
    const int xi = (corner & 1) ? x1 : x0, yi = (corner & 2) ? y1 : y0, zi = (corner & 4) ? z1 : z0;
    const double s = (double)mov[((int64_t)zi * my + yi) * mx + xi];
    const double ax = (corner & 1) ? fx : 1.0 - fx;
    const double ay = (corner & 2) ? fy : 1.0 - fy;
    const double az = (corner & 4) ? fz : 1.0 - fz;
    if constexpr (GRAD) {
      v = v + ((ax * ay) * az) * s;
      const double tx = (ay * az) * s, ty = (ax * az) * s, tz = (ax * ay) * s;
      gx = (corner & 1) ? gx + tx : gx - tx;
      gy = (corner & 2) ? gy + ty : gy - ty;
      gz = (corner & 4) ? gz + tz : gz - tz;
    } else {
      double w = ax;
      w = w * ay;
      w = w * az;
      v = v + w * s;
    }
  }
  if constexpr (GRAD) { grad[0] = gx; grad[1] = gy; grad[2] = gz; }
  return v;
}

// One sample of moving value `val` into row [B] of a table in LDS (the row of its fixed bin): the bin coordinate
// b = clamp((val - mlo) * mscale, 0, B - 1), i = min(floor(b), B - 2), t = b - i, and the sample's 2^16 split as
// q = floor(t * 2^16 + 0.5) to cell i + 1 and the rest to cell i.  A zero weight adds nothing.
__device__ __forceinline__ void hist_scatter(unsigned* row, int B, double val, double mlo, double mscale) {
  const double top = (double)(B - 1);
  double b = (val - mlo) * mscale;
  b = b > 0.0 ? b : 0.0;                                   // NaN -> 0: the cell index stays inside the table
  b = b < top ? b : top;
  int i = (int)floor(b);
  i = i < B - 2 ? i : B - 2;
  const double t = b - (double)i;
  const unsigned q = (unsigned)(int)floor(t * 65536.0 + 0.5);
  if (q != 65536u) atomicAdd(row + i, 65536u - q);
  if (q) atomicAdd(row + i + 1, q);
}

// what the two joint-histogram kernels have in common of their parameters
struct HistParams {
  const uint8_t* fbin;                     // [fz][fy][fx], 255 = ignore
  const void* mov;                         // [mz][my][mx]
  u64* out;                                // [T][bins][bins]
  int fx, fy, fz, mx, my, mz;
  int T, bins, group;
  double mlo, mscale;
};

// The body of a joint-histogram kernel (256 lanes).  Coord gives the continuous moving index of (voxel, candidate):
//   typename Coord::Voxel                       what is computed once per fixed voxel
//   void voxel(ix, iy, iz, Voxel&) const        ... from its level index
//   void at(const Voxel&, t, cx, cy, cz) const  the index under candidate t of the launch
template <typename P, typename Coord>
__device__ __forceinline__ void joint_hist_body(const HistParams& p, const Coord& coord) {
  __shared__ unsigned lds[kHistLdsCounters];
  const P* __restrict__ mov = (const P*)p.mov;
  const int B = p.bins, BB = B * B;
  const int t0 = blockIdx.y * p.group;
  const int gcount = p.T - t0 < p.group ? p.T - t0 : p.group;
  const int entries = gcount * BB;                       // <= kHistLdsCounters by the choice of group
  u64* __restrict__ out = p.out + (int64_t)t0 * BB;
  for (int e = threadIdx.x; e < entries; e += 256) lds[e] = 0;
  __syncthreads();

  const int64_t total = (int64_t)p.fx * p.fy * p.fz;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t trips = (total + stride - 1) / stride;   // the same for every lane: the flushes hold barriers
  int since = 0;
  for (int64_t trip = 0; trip < trips; ++trip) {
    const int64_t e = trip * stride + blockIdx.x * 256ll + threadIdx.x;
    int fb = 255;
    if (e < total) fb = p.fbin[e];
    if (fb < B) {                                        // 255 = ignore; B .. 254 never index the table
      typename Coord::Voxel v;
      coord.voxel((int)(e % p.fx), (int)((e / p.fx) % p.fy), (int)(e / ((int64_t)p.fx * p.fy)), v);
      for (int g = 0; g < gcount; ++g) {
        double cx, cy, cz;
        coord.at(v, t0 + g, cx, cy, cz);
        if (!mi_inside(p.mx, p.my, p.mz, cx, cy, cz)) continue;
        hist_scatter(lds + g * BB + fb * B, B, mi_sample<P, false>(mov, p.mx, p.my, p.mz, cx, cy, cz, nullptr), p.mlo,
                     p.mscale);
      }
    }
    if (++since == kHistFlushTrips) {
      hist_flush(lds, out, entries);
      since = 0;
    }
  }
  hist_flush(lds, out, entries);
}

}  // namespace segmi
