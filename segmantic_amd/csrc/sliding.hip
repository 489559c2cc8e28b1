// sliding.hip -- sliding-window inference data movement (gather / ordered blend / finalise),
// channel argmax and label overlap counts.  All HBM-bound.  (The training sampler's patch cropper lives
// with the other sampler gathers in augment.hip.)
#include <type_traits>

#include "common.h"

namespace segmi {

constexpr int kMaxWin = 16;
constexpr int kSwGrid = 8192;   // workgroup cap of the strided 1-D kernels

struct WinList {
  int n;
  int z[kMaxWin], y[kMaxWin], x[kMaxWin];
};

template <typename TS, typename TD>
__global__ void sw_gather_kernel(const TS* __restrict__ img, TD* __restrict__ win, WinList wl,
                                 int D, int H, int W, int C, int ldi, int rd, int rh, int rw,
                                 int ldw) {
  const int64_t per = (int64_t)rd * rh * rw * C;
  const int64_t total = per * wl.n;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = e % C;
    int64_t t = e / C;
    const int x = t % rw; t /= rw;
    const int y = t % rh; t /= rh;
    const int z = t % rd;
    const int w = t / rd;
    const int gz = wl.z[w] + z, gy = wl.y[w] + y, gx = wl.x[w] + x;
    float v = 0.f;
    if ((unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
      v = Elem<TS>::ld(img + (((int64_t)gz * H + gy) * W + gx) * ldi + c);
    Elem<TD>::st(win + ((((int64_t)w * rd + z) * rh + y) * rw + x) * ldw + c, v);
  }
}

// single-channel images (the usual case): one thread gathers 4 consecutive x of a window row and
// stores them with one 16-byte (f32) / 8-byte (bf16) write
template <typename TS, typename TD>
__global__ void sw_gather4_kernel(const TS* __restrict__ img, TD* __restrict__ win, WinList wl,
                                  int D, int H, int W, int ldi, int rd, int rh, int rw) {
  const int rw4 = rw / 4;
  const int64_t per = (int64_t)rd * rh * rw4;
  const int64_t total = per * wl.n;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    int64_t t = e;
    const int x = (int)(t % rw4) * 4; t /= rw4;
    const int y = (int)(t % rh); t /= rh;
    const int z = (int)(t % rd);
    const int w = (int)(t / rd);
    const int gz = wl.z[w] + z, gy = wl.y[w] + y, gx = wl.x[w] + x;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if ((unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H) {
      const TS* row = img + (((int64_t)gz * H + gy) * W) * ldi;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((unsigned)(gx + j) < (unsigned)W) v[j] = Elem<TS>::ld(row + (int64_t)(gx + j) * ldi);
    }
    store4<TD>(win + ((((int64_t)w * rd + z) * rh + y) * rw + x), v);
  }
}

// one thread per (voxel of the windows' bounding box, channel); windows applied IN ORDER so the
// f32 accumulation order equals the reference's sequential `out[slice] += w * pred`.
template <typename T>
__global__ void sw_scatter_kernel(const T* __restrict__ pred, WinList wl, const float* __restrict__ imp,
                                  float* __restrict__ acc, float* __restrict__ cnt, int D, int H,
                                  int W, int K, int lda, int rd, int rh, int rw, int ldp, int bz0,
                                  int by0, int bx0, int bd, int bh, int bw) {
  const int64_t total = (int64_t)bd * bh * bw * K;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int k = e % K;
    int64_t t = e / K;
    const int x = bx0 + t % bw; t /= bw;
    const int y = by0 + t % bh; t /= bh;
    const int z = bz0 + (int)t;
    const int64_t vox = ((int64_t)z * H + y) * W + x;
    float a = acc[vox * lda + k];
    float c = (cnt && k == 0) ? cnt[vox] : 0.f;
    bool touched = false;
    for (int w = 0; w < wl.n; ++w) {
      const int lz = z - wl.z[w], ly = y - wl.y[w], lx = x - wl.x[w];
      if ((unsigned)lz < (unsigned)rd && (unsigned)ly < (unsigned)rh && (unsigned)lx < (unsigned)rw) {
        const int64_t lv = ((int64_t)lz * rh + ly) * rw + lx;
        const float wt = imp ? imp[lv] : 1.f;
        const float pv = Elem<T>::ld(pred + (((int64_t)w * rd * rh * rw) + lv) * ldp + k);
        a += wt * pv;
        c += wt;
        touched = true;
      }
    }
    if (touched) {
      acc[vox * lda + k] = a;
      if (cnt && k == 0) cnt[vox] = c;
    }
  }
}

// 4-channel vector variant of sw_scatter_kernel (K % 4 == 0, 16-byte aligned rows): one thread
// per (voxel, 4 channels): f32x4 read-modify-write of the accumulator, 8/16-byte prediction loads
template <typename T>
__global__ void sw_scatter4_kernel(const T* __restrict__ pred, WinList wl, const float* __restrict__ imp,
                                   float* __restrict__ acc, float* __restrict__ cnt, int D, int H,
                                   int W, int K, int lda, int rd, int rh, int rw, int ldp, int bz0,
                                   int by0, int bx0, int bd, int bh, int bw) {
  const int kg = K / 4;
  const int64_t total = (int64_t)bd * bh * bw * kg;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int k = (int)(e % kg) * 4;
    int64_t t = e / kg;
    const int x = bx0 + (int)(t % bw); t /= bw;
    const int y = by0 + (int)(t % bh); t /= bh;
    const int z = bz0 + (int)t;
    const int64_t vox = ((int64_t)z * H + y) * W + x;
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
    float c = 0.f;
    bool touched = false;
    for (int w = 0; w < wl.n; ++w) {
      const int lz = z - wl.z[w], ly = y - wl.y[w], lx = x - wl.x[w];
      if ((unsigned)lz < (unsigned)rd && (unsigned)ly < (unsigned)rh && (unsigned)lx < (unsigned)rw) {
        const int64_t lv = ((int64_t)lz * rh + ly) * rw + lx;
        const float wt = imp ? imp[lv] : 1.f;
        const f32x4 pv = load4<T>(pred + (((int64_t)w * rd * rh * rw) + lv) * ldp + k);
        if (!touched) {   // first contributing window: fetch the running sums (same add order
          a = *reinterpret_cast<const f32x4*>(acc + vox * lda + k);   // as the scalar kernel)
          c = (cnt && k == 0) ? cnt[vox] : 0.f;
          touched = true;
        }
        a += wt * pv;
        c += wt;
      }
    }
    if (touched) {
      *reinterpret_cast<f32x4*>(acc + vox * lda + k) = a;
      if (cnt && k == 0) cnt[vox] = c;
    }
  }
}

// argmax with K/4 lanes per voxel (K in {4,8,16,32,64,128,256}): 16-byte loads, lane-group
// butterfly keeping torch.argmax semantics (first maximal index; first NaN wins)
__device__ __forceinline__ bool am_better(float av, int ai, float bv, int bi) {
  // true when (bv, bi) should replace (av, ai)
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return bn && (!an || bi < ai);
  return bv > av || (bv == av && bi < ai);
}
template <typename T, typename L>
__global__ void argmax4_kernel(const T* __restrict__ lg, const float* __restrict__ cnt,
                               float* __restrict__ wb, L* __restrict__ labels, int64_t nvox, int K,
                               int ld) {
  const int tpv = K / 4;                       // lanes per voxel (power of two <= 64)
  const int64_t total = nvox * tpv;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e0 = blockIdx.x * 256ll; e0 < total; e0 += stride) {   // whole wave iterates together
    const int64_t e = e0 + threadIdx.x;
    const bool live = e < total;
    const int64_t v = live ? e / tpv : 0;
    const int k = (int)(e % tpv) * 4;
    f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {
      x = load4<T>(lg + v * ld + k);
      if (cnt) {
        const float c = cnt[v];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = x[j] / c;
      }
      if (wb) *reinterpret_cast<f32x4*>(wb + v * ld + k) = x;
    }
    float bv = x[0];
    int bi = k;
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (am_better(bv, bi, x[j], k + j)) { bv = x[j]; bi = k + j; }
    for (int o = 1; o < tpv; o <<= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (am_better(bv, bi, ov, oi)) { bv = ov; bi = oi; }
    }
    if (live && k == 0) labels[v] = (L)bi;
  }
}

template <typename T, typename L>
__global__ void argmax_kernel(const T* __restrict__ lg, const float* __restrict__ cnt,
                              float* __restrict__ wb, L* __restrict__ labels, int64_t nvox, int K,
                              int ld) {
  for (int64_t v = blockIdx.x * 256ll + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * 256) {
    const T* p = lg + v * ld;
    const float c = cnt ? cnt[v] : 1.f;
    float best = 0.f;
    int bi = 0;
    for (int k = 0; k < K; ++k) {
      float x = Elem<T>::ld(p + k);
      if (cnt) x = x / c;
      if (wb) wb[v * ld + k] = x;
      // torch.argmax: first maximal index; a NaN counts as maximal and the first one wins
      if (k == 0) { best = x; }
      else if (best == best && (x != x || x > best)) { best = x; bi = k; }
    }
    labels[v] = (L)bi;
  }
}

// ---------------------------------------------------------------- deferred ordered blend
// Every window prediction of the dense schedule is kept (`cache` slot = window index - lo); one
// pass then sums, per output voxel, the covering windows in ascending window index -- the same
// f32 addition sequence as the reference's sequential `out[slice] += w * pred` -- divides by the
// count and takes the argmax.  Each prediction element is read exactly once and no f32
// accumulator is read-modified-written per window group (5.4x less HBM traffic than the
// streaming blend at overlap 0.5).
constexpr int kMaxStarts = 64;
struct BlendSched {
  int n[3];
  int start[3][kMaxStarts];   // per-dimension window origins, ascending (first dim slowest)
};

// G = channels per lane (16 bytes of T); K / G lanes cooperate on one voxel
template <typename T, typename L, int G>
__global__ __launch_bounds__(256) void sw_blend_kernel(
    const T* __restrict__ cache, BlendSched sc, int lo, int hi, const float* __restrict__ imp,
    float* __restrict__ out, float* __restrict__ cnt_out, L* __restrict__ labels, int D, int H,
    int W, int K, int ldo, int rd, int rh, int rw, int ldp, int normalize) {
  // A workgroup takes 256-lane segments of one output row (z, y): z, y and with them the covering
  // windows of those two dimensions are wave-uniform (scalar loops), only x is per lane, and no
  // lane does a 64-bit division (the flat-index form spent more time dividing than loading).
  const int tpv = K / G;
  const int lanes_row = W * tpv;
  const int segs = (lanes_row + 255) / 256;
  const int nseg = D * H * segs;
  for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
    const int seg = s % segs, row = s / segs;
    const int y = row % H, z = row / H;
    const int e = seg * 256 + (int)threadIdx.x;
    const bool live = e < lanes_row;
    const int x = live ? e / tpv : 0;
    const int k = live ? (e % tpv) * G : 0;
    const int64_t v = (int64_t)row * W + x;
    float a[G];
#pragma unroll
    for (int j = 0; j < G; ++j) a[j] = 0.f;
    float c = 0.f;
    if (live) {
      for (int kz = 0; kz < sc.n[0]; ++kz) {
        const int lz = z - sc.start[0][kz];
        if ((unsigned)lz >= (unsigned)rd) continue;
        for (int ky = 0; ky < sc.n[1]; ++ky) {
          const int ly = y - sc.start[1][ky];
          if ((unsigned)ly >= (unsigned)rh) continue;
          for (int kx = 0; kx < sc.n[2]; ++kx) {
            const int lx = x - sc.start[2][kx];
            if ((unsigned)lx >= (unsigned)rw) continue;
            const int w = (kz * sc.n[1] + ky) * sc.n[2] + kx;
            if (w < lo || w >= hi) continue;
            const int64_t lv = ((int64_t)lz * rh + ly) * rw + lx;
            const float wt = imp ? imp[lv] : 1.f;
            const T* pp = cache + ((int64_t)(w - lo) * rd * rh * rw + lv) * ldp + k;
            if constexpr (G == 8) {
              f32x4 p0, p1;
              const u32x4 o = *reinterpret_cast<const u32x4*>(pp);
              p0[0] = H16<T>::lo(o[0]); p0[1] = H16<T>::hi(o[0]);
              p0[2] = H16<T>::lo(o[1]); p0[3] = H16<T>::hi(o[1]);
              p1[0] = H16<T>::lo(o[2]); p1[1] = H16<T>::hi(o[2]);
              p1[2] = H16<T>::lo(o[3]); p1[3] = H16<T>::hi(o[3]);
#pragma unroll
              for (int j = 0; j < 4; ++j) { a[j] += wt * p0[j]; a[4 + j] += wt * p1[j]; }
            } else if constexpr (G == 4) {
              const f32x4 p0 = load4<T>(pp);
#pragma unroll
              for (int j = 0; j < 4; ++j) a[j] += wt * p0[j];
            } else {
              a[0] += wt * Elem<T>::ld(pp);
            }
            c += wt;
          }
        }
      }
      if (normalize) {
#pragma unroll
        for (int j = 0; j < G; ++j) a[j] = a[j] / c;
      }
      if (out) {
        if constexpr (G >= 4) {
#pragma unroll
          for (int j = 0; j < G; j += 4)
            *reinterpret_cast<f32x4*>(out + v * ldo + k + j) = f32x4{a[j], a[j + 1], a[j + 2], a[j + 3]};
        } else {
          out[v * ldo + k] = a[0];
        }
      }
      if (cnt_out && k == 0) cnt_out[v] = c;
    }
    if (labels) {
      float bv = a[0];
      int bi = k;
#pragma unroll
      for (int j = 1; j < G; ++j)
        if (am_better(bv, bi, a[j], k + j)) { bv = a[j]; bi = k + j; }
      if (tpv <= 64 && (tpv & (tpv - 1)) == 0) {
        for (int o = 1; o < tpv; o <<= 1) {
          const float ov = __shfl_xor(bv, o);
          const int oi = __shfl_xor(bi, o);
          if (am_better(bv, bi, ov, oi)) { bv = ov; bi = oi; }
        }
        if (live && k == 0) labels[v] = (L)bi;
      }
    }
  }
}

__global__ void label_counts_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ truth,
                                    int64_t n, int K, unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned int hist[];  // [K][3]
  for (int i = threadIdx.x; i < 3 * K; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int a = pred[i], b = truth[i];
    if ((unsigned)a < (unsigned)K) atomicAdd(&hist[a * 3 + 1], 1u);
    if ((unsigned)b < (unsigned)K) atomicAdd(&hist[b * 3 + 2], 1u);
    if (a == b && (unsigned)a < (unsigned)K) atomicAdd(&hist[a * 3 + 0], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * K; i += blockDim.x)
    if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
}


// The same blend for schedules in which at most TWO windows cover a coordinate in every dimension (overlap <= 0.5:
// BASELINE config 3 and the reference's defaults): the <= 8 covering windows of a voxel are located first (z, y:
// wave-uniform; x: per lane), all their loads are issued back to back with a non-temporal hint (each of the 23 GB of
// predictions is read exactly once), then summed in ascending window order -- the same f32 sequence as
// sw_blend_kernel, bit for bit.  sw_blend_kernel finds and loads its windows inside three nested loops with
// per-lane conditions: hipcc keeps ONE 16-byte load per wave in flight, 32 KB per CU, and the pass streamed at
// 2.9 TB/s (round 3: 8 ms of a 43 ms volume).
template <typename T, typename L, int G>
__global__ __launch_bounds__(256) void sw_blend2_kernel(
    const T* __restrict__ cache, BlendSched sc, int lo, int hi, const float* __restrict__ imp,
    float* __restrict__ out, float* __restrict__ cnt_out, L* __restrict__ labels, int D, int H,
    int W, int K, int ldo, int rd, int rh, int rw, int ldp, int normalize) {
  typedef typename std::conditional<G == 8, u32x4, f32x4>::type vec_t;
  const int tpv = K / G;
  const int lanes_row = W * tpv;
  const int segs = (lanes_row + 255) / 256;
  const int nseg = D * H * segs;
  const int64_t wvox = (int64_t)rd * rh * rw;
  for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
    const int seg = s % segs, row = s / segs;
    const int y = row % H, z = row / H;
    const int e = seg * 256 + (int)threadIdx.x;
    const bool live = e < lanes_row;
    const int x = live ? e / tpv : 0;
    const int k = live ? (e % tpv) * G : 0;
    const int64_t v = (int64_t)row * W + x;
    // first covering window and how many cover (1 or 2), per dimension
    int kz0 = 0, ky0 = 0;
    while (kz0 + 1 < sc.n[0] && sc.start[0][kz0] + rd <= z) ++kz0;
    while (ky0 + 1 < sc.n[1] && sc.start[1][ky0] + rh <= y) ++ky0;
    const int nzc = kz0 + 1 < sc.n[0] && sc.start[0][kz0 + 1] <= z ? 2 : 1;
    const int nyc = ky0 + 1 < sc.n[1] && sc.start[1][ky0 + 1] <= y ? 2 : 1;
    int kx0 = 0, sx0 = sc.start[2][0], sx1 = sc.start[2][0];
    bool two_x = false;
    for (int kx = 1; kx < sc.n[2]; ++kx) {
      const int st = sc.start[2][kx];
      const bool past = sx0 + rw <= x;              // the current first window ends before x: move on
      if (past) { kx0 = kx; sx0 = st; }
      else if (!two_x && kx == kx0 + 1 && st <= x) { two_x = true; sx1 = st; }
    }
    const int lz0 = z - sc.start[0][kz0], ly0 = y - sc.start[1][ky0];
    const int lz1 = nzc == 2 ? z - sc.start[0][kz0 + 1] : 0, ly1 = nyc == 2 ? y - sc.start[1][ky0 + 1] : 0;
    vec_t pv[8];
    float wt[8];
    bool ok[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int iz = c >> 2, iy = (c >> 1) & 1, ix = c & 1;
      const int w = ((kz0 + iz) * sc.n[1] + ky0 + iy) * sc.n[2] + kx0 + ix;
      ok[c] = live && iz < nzc && iy < nyc && (ix == 0 || two_x) && w >= lo && w < hi;
      const int lz = iz ? lz1 : lz0, ly = iy ? ly1 : ly0, lx = x - (ix ? sx1 : sx0);
      const int64_t lv = ok[c] ? ((int64_t)lz * rh + ly) * rw + lx : 0;
      const int64_t slot = ok[c] ? (int64_t)(w - lo) : 0;
      pv[c] = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(cache + (slot * wvox + lv) * ldp + k));
      wt[c] = imp ? imp[lv] : 1.f;
    }
    float a[G];
#pragma unroll
    for (int j = 0; j < G; ++j) a[j] = 0.f;
    float cacc = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (ok[c]) {
        if constexpr (G == 8) {
          const u32x4 o = pv[c];
          a[0] += wt[c] * H16<T>::lo(o[0]); a[1] += wt[c] * H16<T>::hi(o[0]);
          a[2] += wt[c] * H16<T>::lo(o[1]); a[3] += wt[c] * H16<T>::hi(o[1]);
          a[4] += wt[c] * H16<T>::lo(o[2]); a[5] += wt[c] * H16<T>::hi(o[2]);
          a[6] += wt[c] * H16<T>::lo(o[3]); a[7] += wt[c] * H16<T>::hi(o[3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] += wt[c] * pv[c][j];
        }
        cacc += wt[c];
      }
    }
    if (live) {
      if (normalize) {
#pragma unroll
        for (int j = 0; j < G; ++j) a[j] = a[j] / cacc;
      }
      if (out) {
#pragma unroll
        for (int j = 0; j < G; j += 4)
          *reinterpret_cast<f32x4*>(out + v * ldo + k + j) = f32x4{a[j], a[j + 1], a[j + 2], a[j + 3]};
      }
      if (cnt_out && k == 0) cnt_out[v] = cacc;
    }
    if (labels) {
      float bv = a[0];
      int bi = k;
#pragma unroll
      for (int j = 1; j < G; ++j)
        if (am_better(bv, bi, a[j], k + j)) { bv = a[j]; bi = k + j; }
      for (int o = 1; o < tpv; o <<= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (am_better(bv, bi, ov, oi)) { bv = ov; bi = oi; }
      }
      if (live && k == 0) labels[v] = (L)bi;
    }
  }
}

// which blend kernel a call takes: `vec` = G (16 bytes of T) channels per lane, K / G a power of two <= 64, aligned rows;
// `two` = at most two windows cover any coordinate in every dimension (start[i + 2] >= start[i] + roi) of an ascending,
// gap-free schedule: the variant that issues all covering loads up front (41.8 vs 42.9 ms per volume with the generic
// kernel).  segmi_sw_blend launches by this choice and segmi_sw_blend_kernel_name reports it.
struct BlendChoice {
  bool vec, two;
  int g;            // channels per lane
};
static BlendChoice blend_choice(int dtype, const void* cache, int k, int ldp, const int32_t* const starts[3],
                                const int nn[3], const int rr[3], const float* out_logits, int ldo) {
  BlendChoice bc{};
  const int gfull = 16 / dtype_size(dtype);
  bc.vec = k % gfull == 0 && ldp % gfull == 0 && ((uintptr_t)cache % 16) == 0 &&
           (!out_logits || (ldo % 4 == 0 && ((uintptr_t)out_logits % 16) == 0)) &&
           (k / gfull) <= 64 && ((k / gfull) & (k / gfull - 1)) == 0;
  bc.g = bc.vec ? gfull : 1;
  bool two = bc.vec;            // the scalar lanes always run the generic kernel
  for (int dd = 0; dd < 3 && two; ++dd)
    for (int i = 0; i + 2 < nn[dd]; ++i)
      if (starts[dd][i + 2] < starts[dd][i] + rr[dd]) { two = false; break; }
  for (int dd = 0; dd < 3 && two; ++dd)          // ascending, gap-free coverage (MONAI's dense schedule)
    for (int i = 0; i + 1 < nn[dd]; ++i)
      if (starts[dd][i + 1] <= starts[dd][i] || starts[dd][i + 1] > starts[dd][i] + rr[dd]) { two = false; break; }
  bc.two = two;
  return bc;
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int segmi_sw_gather(int dtype_src, const segmi_act* image, int img_index,
                    const int32_t* starts_host, int nwin, int dst_dtype,
                    const segmi_act* windows, void* stream) {
  SEGMI_CHECK_ARG(act_ok(image) && act_ok(windows) && starts_host, "sw_gather: bad arguments");
  SEGMI_CHECK_ARG(nwin > 0 && nwin <= kMaxWin && windows->n >= nwin, "sw_gather: 1..%d windows per call", kMaxWin);
  SEGMI_CHECK_ARG(img_index >= 0 && img_index < image->n && image->c == windows->c, "sw_gather: image index / channels");
  SEGMI_CHECK_ARG(dtype_pair_ok(dtype_src, dst_dtype), "sw_gather: bad dtypes");
  WinList wl{};
  wl.n = nwin;
  for (int i = 0; i < nwin; ++i) { wl.z[i] = starts_host[3 * i]; wl.y[i] = starts_host[3 * i + 1]; wl.x[i] = starts_host[3 * i + 2]; }
  const int es = dtype_size(dtype_src);
  const char* base = (const char*)image->data + (int64_t)img_index * image->d * image->h * image->w * image->ld * es;
  const int64_t total = (int64_t)nwin * windows->d * windows->h * windows->w * windows->c;
  hipStream_t st = (hipStream_t)stream;
  if (image->c == 1 && windows->ld == 1 && windows->w % 4 == 0 &&
      ((uintptr_t)windows->data % (4 * dtype_size(dst_dtype))) == 0) {
    const int g4 = grid_1d(total / 4, kSwGrid);
#define GATHER4(TS, TD)                                                                                      \
  hipLaunchKernelGGL((sw_gather4_kernel<TS, TD>), g4, 256, 0, st, (const TS*)base, (TD*)windows->data, wl, \
                     image->d, image->h, image->w, image->ld, windows->d, windows->h, windows->w)
    SEGMI_BY_DTYPE_PAIR(dtype_src, dst_dtype, GATHER4);
#undef GATHER4
  } else {
    const int grid = grid_1d(total, kSwGrid);
#define GATHER(TS, TD)                                                                                       \
  hipLaunchKernelGGL((sw_gather_kernel<TS, TD>), grid, 256, 0, st, (const TS*)base, (TD*)windows->data, wl, \
                     image->d, image->h, image->w, image->c, image->ld, windows->d, windows->h, windows->w, \
                     windows->ld)
    SEGMI_BY_DTYPE_PAIR(dtype_src, dst_dtype, GATHER);
#undef GATHER
  }
  SEGMI_LAUNCH_CHECK("sw_gather");
  return SEGMI_OK;
}

int segmi_sw_scatter_add(int dtype, const segmi_act* pred, const int32_t* starts_host,
                         int nwin, const float* importance, const segmi_act* acc, float* cnt,
                         void* stream) {
  SEGMI_CHECK_ARG(dtype_ok(dtype), "sw_scatter_add: bad dtype");
  SEGMI_CHECK_ARG(act_ok(pred) && act_ok(acc) && starts_host && acc->n == 1, "sw_scatter_add: bad arguments");
  SEGMI_CHECK_ARG(nwin > 0 && nwin <= kMaxWin && pred->n >= nwin && pred->c == acc->c, "sw_scatter_add: windows / channels");
  WinList wl{};
  wl.n = nwin;
  int z0 = 1 << 30, y0 = 1 << 30, x0 = 1 << 30, z1 = -(1 << 30), y1 = -(1 << 30), x1 = -(1 << 30);
  for (int i = 0; i < nwin; ++i) {
    wl.z[i] = starts_host[3 * i]; wl.y[i] = starts_host[3 * i + 1]; wl.x[i] = starts_host[3 * i + 2];
    z0 = wl.z[i] < z0 ? wl.z[i] : z0; y0 = wl.y[i] < y0 ? wl.y[i] : y0; x0 = wl.x[i] < x0 ? wl.x[i] : x0;
    z1 = wl.z[i] + pred->d > z1 ? wl.z[i] + pred->d : z1;
    y1 = wl.y[i] + pred->h > y1 ? wl.y[i] + pred->h : y1;
    x1 = wl.x[i] + pred->w > x1 ? wl.x[i] + pred->w : x1;
  }
  z0 = z0 < 0 ? 0 : z0; y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0;
  z1 = z1 > acc->d ? acc->d : z1; y1 = y1 > acc->h ? acc->h : y1; x1 = x1 > acc->w ? acc->w : x1;
  if (z1 <= z0 || y1 <= y0 || x1 <= x0) return SEGMI_OK;
  const int bd = z1 - z0, bh = y1 - y0, bw = x1 - x0;
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = acc->c % 4 == 0 && acc->ld % 4 == 0 && pred->ld % 4 == 0 && ((uintptr_t)acc->data % 16) == 0 &&
                  ((uintptr_t)pred->data % (4 * dtype_size(dtype))) == 0;
  const int grid = grid_1d((int64_t)bd * bh * bw * (v4 ? acc->c / 4 : acc->c), kSwGrid);
#define SCATTER(T, KERN)                                                                                      \
  hipLaunchKernelGGL(KERN<T>, grid, 256, 0, st, (const T*)pred->data, wl, importance, (float*)acc->data, cnt, \
                     acc->d, acc->h, acc->w, acc->c, acc->ld, pred->d, pred->h, pred->w, pred->ld, z0, y0, x0, \
                     bd, bh, bw)
  if (v4) SEGMI_BY_DTYPE(dtype, SCATTER, sw_scatter4_kernel);
  else SEGMI_BY_DTYPE(dtype, SCATTER, sw_scatter_kernel);
#undef SCATTER
  SEGMI_LAUNCH_CHECK("sw_scatter_add");
  return SEGMI_OK;
}

static int argmax_launch(int dtype, const segmi_act* lg, const float* cnt, int write_back,
                         void* labels, int label_bytes, hipStream_t st) {
  const int64_t nvox = act_voxels(lg);
  float* wb = write_back ? (float*)lg->data : nullptr;
  const int tpv = lg->c / 4;
  const bool v4 = lg->c % 4 == 0 && tpv >= 1 && tpv <= 64 && (tpv & (tpv - 1)) == 0 && lg->ld % 4 == 0 &&
                  ((uintptr_t)lg->data % (4 * dtype_size(dtype))) == 0;
  const int grid = grid_1d(v4 ? nvox * tpv : nvox, kSwGrid);
#define ARGMAX(L, T, KERN)                                                                                   \
  hipLaunchKernelGGL((KERN<T, L>), grid, 256, 0, st, (const T*)lg->data, cnt, wb, (L*)labels, nvox, lg->c, lg->ld)
#define ARGMAX_T(T, KERN) LV_BY_LABEL(label_bytes, ARGMAX, T, KERN)
  if (v4) SEGMI_BY_DTYPE(dtype, ARGMAX_T, argmax4_kernel);
  else SEGMI_BY_DTYPE(dtype, ARGMAX_T, argmax_kernel);
#undef ARGMAX_T
#undef ARGMAX
  SEGMI_LAUNCH_CHECK("argmax");
  return SEGMI_OK;
}

int segmi_sw_finalize(const segmi_act* acc, const float* cnt, int write_logits, void* labels,
                      int label_bytes, void* stream) {
  SEGMI_CHECK_ARG(act_ok(acc) && cnt && labels, "sw_finalize: bad arguments");
  SEGMI_CHECK_ARG(label_bytes == 1 || label_bytes == 2 || label_bytes == 4, "sw_finalize: label_bytes");
  SEGMI_CHECK_ARG(label_bytes > 1 || acc->c <= 256, "sw_finalize: uint8 labels hold at most 256 classes");
  return argmax_launch(SEGMI_F32, acc, cnt, write_logits, labels, label_bytes, (hipStream_t)stream);
}

int segmi_argmax(int dtype, const segmi_act* logits, void* labels, int label_bytes, void* stream) {
  SEGMI_CHECK_ARG(dtype_ok(dtype), "argmax: bad dtype");
  SEGMI_CHECK_ARG(act_ok(logits) && labels, "argmax: bad arguments");
  SEGMI_CHECK_ARG(label_bytes == 1 || label_bytes == 2 || label_bytes == 4, "argmax: label_bytes");
  return argmax_launch(dtype, logits, nullptr, 0, labels, label_bytes, (hipStream_t)stream);
}

int segmi_sw_blend(int dtype, const void* cache, int k, int ldp, const int32_t* starts_z, int nz,
                   const int32_t* starts_y, int ny, const int32_t* starts_x, int nx, int win_lo,
                   int win_hi, int rd, int rh, int rw, const float* importance, int d, int h, int w,
                   float* out_logits, int ldo, float* out_count, void* labels, int label_bytes,
                   int normalize, void* stream) {
  SEGMI_CHECK_ARG(dtype_ok(dtype), "sw_blend: bad dtype");
  SEGMI_CHECK_ARG(cache && starts_z && starts_y && starts_x && k > 0 && ldp >= k && rd > 0 &&
                      rh > 0 && rw > 0 && d > 0 && h > 0 && w > 0,
                  "sw_blend: bad arguments");
  SEGMI_CHECK_ARG(out_logits || labels, "sw_blend: nothing to write");
  SEGMI_CHECK_ARG(!out_logits || ldo >= k, "sw_blend: bad logits row stride");
  if (nz > kMaxStarts || ny > kMaxStarts || nx > kMaxStarts || nz < 1 || ny < 1 || nx < 1)
    SEGMI_UNSUPPORTED("sw_blend: at most %d window origins per dimension", kMaxStarts);
  SEGMI_CHECK_ARG(0 <= win_lo && win_lo < win_hi && (int64_t)win_hi <= (int64_t)nz * ny * nx,
                  "sw_blend: window range [%d, %d) outside the schedule", win_lo, win_hi);
  SEGMI_CHECK_ARG(!labels || normalize, "sw_blend: labels need the normalised blend");
  SEGMI_CHECK_ARG(!labels || label_bytes == 1 || label_bytes == 2 || label_bytes == 4,
                  "sw_blend: label_bytes");
  SEGMI_CHECK_ARG(!labels || label_bytes > 1 || k <= 256, "sw_blend: uint8 labels hold at most 256 classes");
  BlendSched sc{};
  sc.n[0] = nz; sc.n[1] = ny; sc.n[2] = nx;
  for (int i = 0; i < nz; ++i) sc.start[0][i] = starts_z[i];
  for (int i = 0; i < ny; ++i) sc.start[1][i] = starts_y[i];
  for (int i = 0; i < nx; ++i) sc.start[2][i] = starts_x[i];
  const int32_t* const starts[3] = {starts_z, starts_y, starts_x};
  const int nn[3] = {nz, ny, nx}, rr[3] = {rd, rh, rw};
  const BlendChoice bc = blend_choice(dtype, cache, k, ldp, starts, nn, rr, out_logits, ldo);
  const bool vec = bc.vec, two = bc.two;
  hipStream_t st = (hipStream_t)stream;
  const int64_t row_segs = (int64_t)d * h * (((int64_t)w * (k / bc.g) + 255) / 256);
  SEGMI_CHECK_ARG(row_segs < (1ll << 31) && (int64_t)w * k < (1ll << 30), "sw_blend: volume too large");
  const int grid = (int)(row_segs < 16384 ? row_segs : 16384);
  // labels come from the vector kernels only: the scalar lanes (one channel each) write the logits, and the
  // labels (if wanted) come from a second pass over them
  SEGMI_CHECK_ARG(vec || !labels || out_logits, "sw_blend: the scalar path labels from the written logits");
#define BLEND(L, T, KERN, G)                                                                                  \
  hipLaunchKernelGGL((KERN<T, L, G>), grid, 256, 0, st, (const T*)cache, sc, win_lo, win_hi, importance,      \
                     out_logits, out_count, vec ? (L*)labels : nullptr, d, h, w, k, ldo, rd, rh, rw, ldp, normalize)
#define BLEND_L(T, KERN) SEGMI_BY_LABEL_AS(lb, uint8_t, uint16_t, int32_t, BLEND, T, KERN, (int)(16 / sizeof(T)))
#define BLEND_T(T)                                                \
  do {                                                            \
    if (!vec) BLEND(int32_t, T, sw_blend_kernel, 1);              \
    else if (two) BLEND_L(T, sw_blend2_kernel);                   \
    else BLEND_L(T, sw_blend_kernel);                             \
  } while (0)
  const int lb = labels ? label_bytes : 4;   // without labels the width is not checked and does not matter
  SEGMI_BY_DTYPE(dtype, BLEND_T);
#undef BLEND_T
#undef BLEND_L
#undef BLEND
  SEGMI_LAUNCH_CHECK("sw_blend");
  if (!vec && labels) {
    segmi_act lg{out_logits, 1, d, h, w, k, ldo};
    return argmax_launch(SEGMI_F32, &lg, nullptr, 0, labels, label_bytes, st);
  }
  return SEGMI_OK;
}

const char* segmi_sw_blend_kernel_name(int dtype, const void* cache, int k, int ldp, const int32_t* starts_z, int nz,
                                       const int32_t* starts_y, int ny, const int32_t* starts_x, int nx, int rd,
                                       int rh, int rw, const float* out_logits, int ldo) {
  static thread_local char buf[64];
  if (!dtype_ok(dtype) || !cache || !starts_z || !starts_y || !starts_x || k <= 0 || ldp < k || rd <= 0 || rh <= 0 ||
      rw <= 0 || nz < 1 || ny < 1 || nx < 1 || nz > kMaxStarts || ny > kMaxStarts || nx > kMaxStarts)
    return "invalid";
  const int32_t* const starts[3] = {starts_z, starts_y, starts_x};
  const int nn[3] = {nz, ny, nx}, rr[3] = {rd, rh, rw};
  const BlendChoice bc = blend_choice(dtype, cache, k, ldp, starts, nn, rr, out_logits, ldo);
  snprintf(buf, sizeof buf, "sw_%s_kernel<%s, G=%d>", !bc.vec ? "blend_scalar" : bc.two ? "blend2" : "blend", dtype_name(dtype), bc.g);
  return buf;
}

int segmi_label_counts(const int32_t* pred, const int32_t* truth, int64_t n, int k,
                       int64_t* counts, void* stream) {
  SEGMI_CHECK_ARG(pred && truth && counts && n > 0 && k > 0 && k <= 4096, "label_counts: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)k * 3 * 8, st) != hipSuccess) {
    set_error("label_counts: memset failed");
    return SEGMI_ELAUNCH;
  }
  const int grid = grid_1d(n, 1024);
  hipLaunchKernelGGL(label_counts_kernel, grid, 256, (size_t)k * 3 * 4, st, pred, truth, n, k,
                     (unsigned long long*)counts);
  SEGMI_LAUNCH_CHECK("label_counts");
  return SEGMI_OK;
}

}  // extern "C"
