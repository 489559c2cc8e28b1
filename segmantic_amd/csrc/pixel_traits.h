// pixel_traits.h -- the resamplers' output cast (ITK's): saturate to the pixel type's range, then truncate; and the
// trilinear / nearest tap of resample_kernel (image.hip) and ffd_warp_kernel (deformable.hip).
#pragma once
#include <stdint.h>

namespace segmi {

template <typename P> struct PixelTraits;
template <> struct PixelTraits<float> { static __device__ float cast(double v) { return (float)v; } };
template <> struct PixelTraits<uint8_t> { static __device__ uint8_t cast(double v) { v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v); return (uint8_t)v; } };
template <> struct PixelTraits<uint16_t> { static __device__ uint16_t cast(double v) { v = v < 0.0 ? 0.0 : (v > 65535.0 ? 65535.0 : v); return (uint16_t)v; } };
template <> struct PixelTraits<int16_t> { static __device__ int16_t cast(double v) { v = v < -32768.0 ? -32768.0 : (v > 32767.0 ? 32767.0 : v); return (int16_t)v; } };
template <> struct PixelTraits<int32_t> { static __device__ int32_t cast(double v) { v = v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v); return (int32_t)v; } };

// The output value at the continuous source index (cx, cy, cz) of src [sz][sy][sx]: `defval` unless
// -0.5 <= c < dim - 0.5 on every axis; else, with interp & 1, the nearest voxel (ITK rounds half up; interp & 4 =
// round half to even: torch grid_sample "nearest" = nearbyint, what MONAI's Spacing(mode="nearest") ends in); else
// the 8-corner sum with the taps clamped into the image.  Corner order and accumulation as oracle/resample_ref.py
// (bit d of the corner = dim d).  The products and sums are the explicit round-to-nearest intrinsics, so the result
// is the same bits as the numpy oracle whether or not the including file is built with FMA contraction.
template <typename P>
__device__ __forceinline__ P resample_tap(const P* src, int sx, int sy, int sz, double cx, double cy, double cz,
                                          int interp, double defval) {
  double val = defval;
  const bool inside = cx >= -0.5 && cx < sx - 0.5 && cy >= -0.5 && cy < sy - 0.5 &&
                      cz >= -0.5 && cz < sz - 0.5;
  if (inside) {
    if (interp & 1) {
      int ix, iy, iz;
      if (interp & 4) { ix = (int)rint(cx); iy = (int)rint(cy); iz = (int)rint(cz); }
      else { ix = (int)floor(cx + 0.5); iy = (int)floor(cy + 0.5); iz = (int)floor(cz + 0.5); }
      ix = ix < 0 ? 0 : (ix > sx - 1 ? sx - 1 : ix);
      iy = iy < 0 ? 0 : (iy > sy - 1 ? sy - 1 : iy);
      iz = iz < 0 ? 0 : (iz > sz - 1 ? sz - 1 : iz);
      val = (double)src[((int64_t)iz * sy + iy) * sx + ix];
    } else {
      const double fx0 = floor(cx), fy0 = floor(cy), fz0 = floor(cz);
      int bx = (int)fx0, by = (int)fy0, bz = (int)fz0;
      double fx = cx - fx0, fy = cy - fy0, fz = cz - fz0;
      if (bx < 0) fx = 0.0;
      if (by < 0) fy = 0.0;
      if (bz < 0) fz = 0.0;
      const int x0 = bx < 0 ? 0 : bx, y0 = by < 0 ? 0 : by, z0 = bz < 0 ? 0 : bz;
      const int x1 = bx + 1 > sx - 1 ? sx - 1 : (bx + 1 < 0 ? 0 : bx + 1);
      const int y1 = by + 1 > sy - 1 ? sy - 1 : (by + 1 < 0 ? 0 : by + 1);
      const int z1 = bz + 1 > sz - 1 ? sz - 1 : (bz + 1 < 0 ? 0 : bz + 1);
      val = 0.0;
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) {
        const int xi = (corner & 1) ? x1 : x0, yi = (corner & 2) ? y1 : y0, zi = (corner & 4) ? z1 : z0;
        double w = (corner & 1) ? fx : 1.0 - fx;
        w = __dmul_rn(w, (corner & 2) ? fy : 1.0 - fy);
        w = __dmul_rn(w, (corner & 4) ? fz : 1.0 - fz);
        val = __dadd_rn(val, __dmul_rn(w, (double)src[((int64_t)zi * sy + yi) * sx + xi]));
      }
    }
  }
  return PixelTraits<P>::cast(val);
}

}  // namespace segmi
