// pixel_traits.h -- the resamplers' output cast (ITK's): saturate to the pixel type's range, then truncate.
#pragma once
#include <stdint.h>

namespace segmi {

template <typename P> struct PixelTraits;
template <> struct PixelTraits<float> { static __device__ float cast(double v) { return (float)v; } };
template <> struct PixelTraits<uint8_t> { static __device__ uint8_t cast(double v) { v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v); return (uint8_t)v; } };
template <> struct PixelTraits<uint16_t> { static __device__ uint16_t cast(double v) { v = v < 0.0 ? 0.0 : (v > 65535.0 ? 65535.0 : v); return (uint16_t)v; } };
template <> struct PixelTraits<int16_t> { static __device__ int16_t cast(double v) { v = v < -32768.0 ? -32768.0 : (v > 32767.0 ? 32767.0 : v); return (int16_t)v; } };
template <> struct PixelTraits<int32_t> { static __device__ int32_t cast(double v) { v = v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v); return (int32_t)v; } };

}  // namespace segmi
