// distance.hip -- segmentation evaluation on the GPU: per-label bounding boxes, the exact Euclidean
// distance transform (EDT) over a label's box, the distance sampler with in-launch f64 finalisation,
// an exact radix select for order statistics, and confusion counts.
// Replaces the SimpleITK CPU path of src/segmantic/seg/evaluation.py:5-125 (BinaryContour +
// SignedMaurerDistanceMap + numpy statistics) and of scripts/evaluate_segmentations.py.
//
// EDT layout (crop extents bd x bh x bw, squared physical distances in f32):
//   P1 along z : lanes over (y, x) lines, two register sweeps (nearest feature forward / backward),
//                the feature test (mask or 6/4-face contour) read from the full label volume;
//                writes f1[z][y][x].
//   P2 along y : lanes over (z, x) lines, lower envelope of parabolas (Felzenszwalb-Huttenlocher)
//                with the stack in scratch laid out [depth][line]; writes out[z][x][y].
//   P3 along x : lanes over (z, y) lines on that transposed layout, in place (the stack keeps the
//                parabola heights, so the fill pass reads nothing it has overwritten).
// The contour transform is signed as SignedMaurerDistanceMap(insideIsPositive=False) is: a voxel of the
// label carries the sign bit (P1 sets it, P2 and P3 copy it from the position they overwrite).  So one
// map per volume serves both query kinds: |d| is the distance to the contour (surface distances), and
// for a query point outside the label the distance to the label equals the distance to its contour (a
// nearest label voxel always has a background face neighbour that lies closer to the query point), so
// clamping d <= 0 to 0 gives the distance to the label (point-wise distances).
// With unit spacing the envelope arithmetic is exact integer arithmetic (i64 products), so the result
// is bit-exact against brute force while squared distances stay below 2^24.
#include "labelvol.h"
#include "reduce_fin.h"

namespace segmi {

constexpr float kInf = __builtin_inff();
constexpr int kBoxMaxLabels = 1024;
constexpr int kSampleWgs = 1024;      // sampler grid cap: the partial table has at most this many rows
constexpr int kSelectWgs = 512;
constexpr int kSelectBins = 2048;     // 11-bit digits: passes over bits 31..21, 20..10, 9..0
constexpr int kSelectMaxRanks = 4;


template <typename T>
__device__ __forceinline__ int lab_at(const T* lab, int64_t o) { return (int)lab[o]; }

// voxel (z, y, x) of the full volume is in the feature / query set of label c.
// contour: a voxel of c with at least one face neighbour that is not c (outside the volume = background);
// a 2-D input (sd == 2, d == 1) never looks along z.
template <typename T, bool CONTOUR>
__device__ __forceinline__ bool in_set(const T* lab, int d, int h, int w, int sd, int c, int z, int y, int x) {
  const int64_t hw = (int64_t)h * w;
  const int64_t o = (int64_t)z * hw + (int64_t)y * w + x;
  if (lab_at(lab, o) != c) return false;
  if (!CONTOUR) return true;
  if (x == 0 || lab_at(lab, o - 1) != c) return true;
  if (x == w - 1 || lab_at(lab, o + 1) != c) return true;
  if (y == 0 || lab_at(lab, o - w) != c) return true;
  if (y == h - 1 || lab_at(lab, o + w) != c) return true;
  if (sd == 3) {
    if (z == 0 || lab_at(lab, o - hw) != c) return true;
    if (z == d - 1 || lab_at(lab, o + hw) != c) return true;
  }
  return false;
}

// ------------------------------------------------------------------ label boxes
// boxes i32[k][6] accumulate inclusive (min z, max z, min y, max y, min x, max x); counts u64[k][2].
__global__ void boxes_init_kernel(int32_t* boxes, unsigned long long* counts, int k) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= k) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) { boxes[c * 6 + 2 * a] = 0x7fffffff; boxes[c * 6 + 2 * a + 1] = -1; }
  counts[2 * c] = 0; counts[2 * c + 1] = 0;
}

// One wave per row (z, y), lanes over x.  Per 64-voxel chunk the distinct labels are walked with
// ballots (a chunk rarely holds more than two): the ballot mask gives the x extent and the count, and
// one lane folds them into the workgroup's LDS table; each workgroup then adds its table to the global
// one with one atomic per (label, field) it touched.  No per-voxel atomics.
template <typename T>
__global__ __launch_bounds__(256) void boxes_kernel(const T* __restrict__ pred, const T* __restrict__ truth,
                                                    int d, int h, int w, int k, int32_t* boxes,
                                                    unsigned long long* counts) {
  extern __shared__ int s_tab[];   // [k][8]: 6 box fields, 2 counts
  for (int i = threadIdx.x; i < k; i += 256) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { s_tab[i * 8 + 2 * a] = 0x7fffffff; s_tab[i * 8 + 2 * a + 1] = -1; }
    s_tab[i * 8 + 6] = 0; s_tab[i * 8 + 7] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int rows = d * h;
  const int nwaves = gridDim.x * 4;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nwaves) {
    const int z = r / h, y = r % h;
    const int64_t base = (int64_t)r * w;
    for (int x0 = 0; x0 < w; x0 += 64) {
      const int x = x0 + lane;
      const int vp = x < w ? (int)pred[base + x] : -1;
      const int vt = x < w ? (int)truth[base + x] : -1;
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        const int v = which ? vt : vp;
        unsigned long long todo = __ballot(v >= 0 && v < k);
        while (todo) {
          const int lead = __ffsll((long long)todo) - 1;
          const int c = __shfl(v, lead);
          const unsigned long long m = __ballot(v == c);
          todo &= ~m;
          if (lane == lead) {
            int* e = s_tab + c * 8;
            atomicMin(e + 0, z); atomicMax(e + 1, z);
            atomicMin(e + 2, y); atomicMax(e + 3, y);
            atomicMin(e + 4, x0 + __ffsll((long long)m) - 1);
            atomicMax(e + 5, x0 + 63 - __clzll((long long)m));
            atomicAdd(e + 6 + which, __popcll(m));
          }
        }
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < k; c += 256) {
    const int* e = s_tab + c * 8;
    if (e[6] == 0 && e[7] == 0) continue;
    atomicMin(boxes + c * 6 + 0, e[0]); atomicMax(boxes + c * 6 + 1, e[1]);
    atomicMin(boxes + c * 6 + 2, e[2]); atomicMax(boxes + c * 6 + 3, e[3]);
    atomicMin(boxes + c * 6 + 4, e[4]); atomicMax(boxes + c * 6 + 5, e[5]);
    if (e[6]) atomicAdd(counts + 2 * c, (unsigned long long)e[6]);
    if (e[7]) atomicAdd(counts + 2 * c + 1, (unsigned long long)e[7]);
  }
}

// inclusive maxima -> half-open; a label present in neither volume gets the empty box 0 0 0 0 0 0
__global__ void boxes_fin_kernel(int32_t* boxes, const unsigned long long* counts, int k) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= k) return;
  const bool empty = counts[2 * c] == 0 && counts[2 * c + 1] == 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    boxes[c * 6 + 2 * a] = empty ? 0 : boxes[c * 6 + 2 * a];
    boxes[c * 6 + 2 * a + 1] = empty ? 0 : boxes[c * 6 + 2 * a + 1] + 1;
  }
}

// ------------------------------------------------------------------ EDT
struct EdtParams {
  const void* lab;
  int d, h, w, sd, label;
  int z0, y0, x0, bd, bh, bw;
  float sz, sy, sx;          // spacing per array axis
  float* f1;                 // [bd][bh][bw] after P1
  float* out;                // [bd][bw][bh] after P2 / P3
  int32_t* sv;               // stack positions  [depth][line]
  float* sg;                 // stack heights    [depth][line]
};

// P1: lanes over the bh*bw (y, x) lines of the crop; the forward sweep leaves the distance (in voxels)
// to the previous feature in f1, the backward sweep turns it into the squared physical distance.
template <typename T, bool CONTOUR>
__global__ __launch_bounds__(256) void edt_p1_kernel(EdtParams p) {
  const int nl = p.bh * p.bw;
  const int line = blockIdx.x * 256 + threadIdx.x;
  if (line >= nl) return;
  const int y = line / p.bw, x = line % p.bw;
  const T* lab = (const T*)p.lab;
  float* f = p.f1 + line;
  const int64_t st = nl;
  const int kNone = -(1 << 30);
  int last = kNone;
  for (int z = 0; z < p.bd; ++z) {
    if (in_set<T, CONTOUR>(lab, p.d, p.h, p.w, p.sd, p.label, p.z0 + z, p.y0 + y, p.x0 + x)) last = z;
    f[z * st] = last == kNone ? kInf : (float)(z - last);
  }
  int next = kNone;
  const double sz = p.sz;
  for (int z = p.bd - 1; z >= 0; --z) {
    const float fv = f[z * st];
    if (fv == 0.f) next = z;   // (the forward sweep stores no sign)
    int dist = fv < kInf ? (int)fv : 0x7fffffff;
    if (next != kNone && next - z < dist) dist = next - z;
    float o = kInf;
    if (dist != 0x7fffffff) {
      const double dz = (double)dist * sz;
      o = (float)(dz * dz);
    }
    if (CONTOUR && in_set<T, false>(lab, p.d, p.h, p.w, p.sd, p.label, p.z0 + z, p.y0 + y, p.x0 + x)) o = -o;
    f[z * st] = o;
  }
}

// Lower envelope of the parabolas g(q) + w2 (t - q)^2 over one line of n samples (in[i * stride]),
// written to out[i * ostride].  EXACT: unit spacing and integer heights, every comparison in i64.
// SIGNED: heights are |in|, and out[t] takes the sign of in[t] (read just before out[t] is written, so
// in == out works).
template <bool EXACT, bool SIGNED>
__device__ __forceinline__ void envelope_line(const float* in, int64_t stride, float* outp, int64_t ostride, int n,
                                              double w2, int32_t* sv, float* sg, int64_t nl) {
  int top = -1;
  int va = 0, vb = 0;        // positions of the two topmost parabolas (a below b)
  float ga = 0.f, gb = 0.f;
  for (int q = 0; q < n; ++q) {
    const float gq = SIGNED ? fabsf(in[q * stride]) : in[q * stride];
    if (!(gq < kInf)) continue;
    // pop b while the new parabola q takes over before b's own region starts
    while (top >= 1) {
      bool pop;
      if (EXACT) {
        const int64_t Fa = (int64_t)ga + (int64_t)va * va, Fb = (int64_t)gb + (int64_t)vb * vb;
        const int64_t Fq = (int64_t)gq + (int64_t)q * q;
        pop = (Fq - Fb) * (int64_t)(vb - va) <= (Fb - Fa) * (int64_t)(q - vb);
      } else {
        const double Fa = (double)ga + w2 * (double)va * va, Fb = (double)gb + w2 * (double)vb * vb;
        const double Fq = (double)gq + w2 * (double)q * q;
        pop = (Fq - Fb) * (double)(vb - va) <= (Fb - Fa) * (double)(q - vb);
      }
      if (!pop) break;
      --top;
      vb = va; gb = ga;
      if (top >= 1) { va = sv[(top - 1) * nl]; ga = sg[(top - 1) * nl]; }
    }
    ++top;
    sv[top * nl] = q;
    sg[top * nl] = gq;
    va = vb; ga = gb;
    vb = q; gb = gq;
  }
  if (top < 0) {
    for (int t = 0; t < n; ++t) outp[t * ostride] = SIGNED ? copysignf(kInf, in[t * stride]) : kInf;
    return;
  }
  int k = 0;
  int v0 = sv[0], v1 = 0;
  float g0 = sg[0], g1 = 0.f;
  if (top >= 1) { v1 = sv[nl]; g1 = sg[nl]; }
  for (int t = 0; t < n; ++t) {
    if (EXACT) {
      int64_t c0 = (int64_t)g0 + (int64_t)(t - v0) * (t - v0);
      while (k < top) {
        const int64_t c1 = (int64_t)g1 + (int64_t)(t - v1) * (t - v1);
        if (c1 > c0) break;
        ++k; v0 = v1; g0 = g1; c0 = c1;
        if (k < top) { v1 = sv[(k + 1) * nl]; g1 = sg[(k + 1) * nl]; }
      }
      outp[t * ostride] = SIGNED ? copysignf((float)c0, in[t * stride]) : (float)c0;
    } else {
      double c0 = (double)g0 + w2 * (double)(t - v0) * (t - v0);
      while (k < top) {
        const double c1 = (double)g1 + w2 * (double)(t - v1) * (t - v1);
        if (c1 > c0) break;
        ++k; v0 = v1; g0 = g1; c0 = c1;
        if (k < top) { v1 = sv[(k + 1) * nl]; g1 = sg[(k + 1) * nl]; }
      }
      outp[t * ostride] = SIGNED ? copysignf((float)c0, in[t * stride]) : (float)c0;
    }
  }
}

// P2: lanes over the bd*bw (z, x) lines; f1[z][y][x] -> out[z][x][y]
template <bool EXACT, bool SIGNED>
__global__ __launch_bounds__(256) void edt_p2_kernel(EdtParams p) {
  const int64_t nl = (int64_t)p.bd * p.bw;
  const int64_t line = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (line >= nl) return;
  const int64_t z = line / p.bw, x = line % p.bw;
  envelope_line<EXACT, SIGNED>(p.f1 + z * p.bh * p.bw + x, p.bw, p.out + line * p.bh, 1, p.bh,
                       (double)p.sy * p.sy, p.sv + line, p.sg + line, nl);
}

// P3: lanes over the bd*bh (z, y) lines of out[z][x][y], in place
template <bool EXACT, bool SIGNED>
__global__ __launch_bounds__(256) void edt_p3_kernel(EdtParams p) {
  const int64_t nl = (int64_t)p.bd * p.bh;
  const int64_t line = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (line >= nl) return;
  const int64_t z = line / p.bh, y = line % p.bh;
  float* base = p.out + z * p.bw * p.bh + y;
  envelope_line<EXACT, SIGNED>(base, p.bh, base, p.bh, p.bw, (double)p.sx * p.sx, p.sv + line, p.sg + line, nl);
}

// ------------------------------------------------------------------ sampler
struct SampleParams {
  const float* dist;          // [bd][bw][bh]
  const void* lab;
  int d, h, w, sd, label;
  int z0, y0, x0, bd, bh, bw;
  double* stats;              // count, sum, sum of squares, max
  float* values;              // nullable: squared distances of the query voxels, compacted
  unsigned long long* n_values;
  double* partials;           // [gridDim.x][4]
  unsigned ticket;
};

__device__ __forceinline__ void st_relaxed(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_relaxed(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wave per crop row (z, y), lanes over x: the query test reads the label volume coalesced, the
// distance is read only for query voxels.  Per-thread f64 sums in a fixed order, a fixed-order
// workgroup reduction into row blockIdx.x of the partial table, and the workgroup that draws the last
// ticket folds the table in a fixed order (fin_tail.h protocol, f64 rows): repeated calls are
// bit-identical whichever workgroup finishes last.
template <typename T, bool CONTOUR>
__global__ __launch_bounds__(256) void sample_kernel(SampleParams p) {
  __shared__ double s_red[4][256];
  __shared__ int s_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* lab = (const T*)p.lab;
  const int rows = p.bd * p.bh;
  const int nwaves = gridDim.x * 4;
  double cnt = 0.0, sum = 0.0, sq = 0.0, mx = 0.0;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int r = blockIdx.x * 4 + wave; r < rows; r += nwaves) {
    const int z = r / p.bh, y = r % p.bh;
    for (int x0 = 0; x0 < p.bw; x0 += 64) {
      const int x = x0 + lane;
      const bool q = x < p.bw && in_set<T, CONTOUR>(lab, p.d, p.h, p.w, p.sd, p.label, p.z0 + z, p.y0 + y, p.x0 + x);
      float d2 = 0.f;
      if (q) {
        // contour queries: |d| (surface distance); foreground queries: d <= 0 (inside the target) -> 0
        d2 = p.dist[((int64_t)z * p.bw + x) * p.bh + y];
        d2 = CONTOUR ? fabsf(d2) : (d2 <= 0.f ? 0.f : d2);
        const double dd = sqrt((double)d2);
        cnt += 1.0; sum += dd; sq += (double)d2; mx = dd > mx ? dd : mx;
      }
      if (p.values) {
        const unsigned long long m = __ballot(q);
        if (m) {
          const int lead = __ffsll((long long)m) - 1;
          unsigned long long b = 0;
          if (lane == lead) b = atomicAdd(p.n_values, (unsigned long long)__popcll(m));
          b = __shfl(b, lead);
          if (q) p.values[b + __popcll(m & lt)] = d2;
        }
      }
    }
  }
  cnt = wave_sum(cnt); sum = wave_sum(sum); sq = wave_sum(sq);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_xor(mx, o); mx = t > mx ? t : mx; }
  if (lane == 0) { s_red[0][wave] = cnt; s_red[1][wave] = sum; s_red[2][wave] = sq; s_red[3][wave] = mx; }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int f = threadIdx.x;
    double v = s_red[f][0];
    for (int i = 1; i < 4; ++i) v = f == 3 ? (s_red[f][i] > v ? s_red[f][i] : v) : v + s_red[f][i];
    st_relaxed(p.partials + (int64_t)blockIdx.x * 4 + f, v);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(&g_fin_tickets[p.ticket], 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
    if (s_last) __hip_atomic_store(&g_fin_tickets[p.ticket], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  const int tid = threadIdx.x;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = tid; b < (int)gridDim.x; b += 256) {
#pragma unroll
    for (int f = 0; f < 3; ++f) a[f] += ld_relaxed(p.partials + (int64_t)b * 4 + f);
    const double m = ld_relaxed(p.partials + (int64_t)b * 4 + 3);
    a[3] = m > a[3] ? m : a[3];
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) s_red[f][tid] = a[f];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int f = 0; f < 3; ++f) s_red[f][tid] += s_red[f][tid + o];
      s_red[3][tid] = s_red[3][tid + o] > s_red[3][tid] ? s_red[3][tid + o] : s_red[3][tid];
    }
    __syncthreads();
  }
  if (tid < 4) p.stats[tid] = s_red[tid][0];
}

// ------------------------------------------------------------------ radix select
// State in the workspace: i64 [kSelectMaxRanks][2] = (prefix of the bit pattern found so far, rank
// still to skip inside that prefix; -1 = no values), then u32 hist[n_ranks][2048].  The passes hand
// their state over on the device: no host round trip between passes.
struct SelectParams {
  const float* values;
  const int64_t* n;
  const int64_t* ranks;
  int n_ranks;
  float* out;
  int64_t* state;
  unsigned* hist;
};

__global__ void select_init_kernel(SelectParams p) {
  const int64_t n = *p.n;
  if (threadIdx.x < p.n_ranks) {
    int64_t r = p.ranks[threadIdx.x];
    r = r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
    p.state[2 * threadIdx.x] = 0;
    p.state[2 * threadIdx.x + 1] = n > 0 ? r : -1;
  }
  for (int i = threadIdx.x; i < p.n_ranks * kSelectBins; i += 256) p.hist[i] = 0;
}

template <int PASS>
__global__ __launch_bounds__(256) void select_hist_kernel(SelectParams p) {
  constexpr int shift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
  constexpr unsigned mask = PASS == 2 ? 1023u : 2047u;
  constexpr int hi = PASS == 0 ? 32 : (PASS == 1 ? 21 : 10);
  __shared__ unsigned s_hist[kSelectMaxRanks * kSelectBins];
  const int64_t n = *p.n;
  if ((int64_t)blockIdx.x * 256 >= n) return;
  unsigned pre[kSelectMaxRanks];
  bool on[kSelectMaxRanks];
#pragma unroll
  for (int r = 0; r < kSelectMaxRanks; ++r) {
    on[r] = r < p.n_ranks && p.state[2 * r + 1] >= 0;
    pre[r] = on[r] ? (unsigned)p.state[2 * r] : 0u;
  }
  for (int i = threadIdx.x; i < p.n_ranks * kSelectBins; i += 256) s_hist[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned u = __float_as_uint(p.values[i]);
#pragma unroll
    for (int r = 0; r < kSelectMaxRanks; ++r)
      if (on[r] && (hi == 32 || (u >> hi) == (pre[r] >> hi))) atomicAdd(&s_hist[r * kSelectBins + ((u >> shift) & mask)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < p.n_ranks * kSelectBins; i += 256)
    if (s_hist[i]) atomicAdd(p.hist + i, s_hist[i]);
}

// one workgroup per rank: find the digit whose cumulative count passes the remaining rank
template <int PASS>
__global__ __launch_bounds__(256) void select_scan_kernel(SelectParams p) {
  constexpr int shift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
  __shared__ int64_t s_scan[256];
  const int r = blockIdx.x, tid = threadIdx.x;
  unsigned* h = p.hist + r * kSelectBins;
  const int64_t rem = p.state[2 * r + 1];
  int64_t loc[8], tot = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { loc[j] = h[tid * 8 + j]; tot += loc[j]; }
  const int64_t before = lv_block_scan<256>(tot, s_scan);
#pragma unroll
  for (int j = 0; j < 8; ++j) h[tid * 8 + j] = 0;      // ready for the next pass
  if (rem >= 0 && rem >= before && rem < before + tot) {
    int64_t c = before;
    int j = 0;
    for (; j < 8; ++j) {
      if (rem < c + loc[j]) break;
      c += loc[j];
    }
    const unsigned pre = (unsigned)p.state[2 * r] | ((unsigned)(tid * 8 + j) << shift);
    p.state[2 * r] = pre;
    p.state[2 * r + 1] = rem - c;
    if (PASS == 2) p.out[r] = __uint_as_float(pre);
  }
  if (PASS == 2 && rem < 0 && tid == 0) p.out[r] = __builtin_nanf("");
}

// ------------------------------------------------------------------ confusion counts
template <typename T>
__global__ __launch_bounds__(256) void confusion_lds_kernel(const T* __restrict__ pred, const T* __restrict__ truth,
                                                            int64_t n, int k, unsigned long long* cm) {
  __shared__ unsigned s_cm[64 * 64];
  for (int i = threadIdx.x; i < k * k; i += 256) s_cm[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int t = (int)truth[i], q = (int)pred[i];
    if (t >= 0 && t < k && q >= 0 && q < k) atomicAdd(&s_cm[t * k + q], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k * k; i += 256)
    if (s_cm[i]) atomicAdd(cm + i, (unsigned long long)s_cm[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void confusion_global_kernel(const T* __restrict__ pred, const T* __restrict__ truth,
                                                               int64_t n, int k, unsigned long long* cm) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int t = (int)truth[i], q = (int)pred[i];
    if (t >= 0 && t < k && q >= 0 && q < k) atomicAdd(cm + (int64_t)t * k + q, 1ull);
  }
}

// ------------------------------------------------------------------ host helpers
struct EdtLayout {
  int64_t nvox;
  size_t f1, sv, sg, partials, total;
};
static inline EdtLayout edt_layout(int bd, int bh, int bw) {
  LvCarver c;
  EdtLayout l;
  l.nvox = (int64_t)bd * bh * bw;
  l.f1 = c.take((size_t)l.nvox * 4);
  l.sv = c.take((size_t)l.nvox * 4);
  l.sg = c.take((size_t)l.nvox * 4);
  l.partials = c.take((size_t)kSampleWgs * 4 * sizeof(double));
  l.total = c.off;
  return l;
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int segmi_label_boxes(const void* pred, const void* truth, int label_bytes, int d, int h, int w, int k,
                      int32_t* boxes, int64_t* counts, void* stream) {
  SEGMI_CHECK_ARG(pred && truth && boxes && counts, "label_boxes: null pointer");
  LV_CHECK_LABEL_BYTES("label_boxes", label_bytes);
  SEGMI_CHECK_ARG(d > 0 && h > 0 && w > 0 && (int64_t)d * h < (1ll << 31), "label_boxes: bad extents");
  SEGMI_CHECK_ARG(k > 0 && k <= kBoxMaxLabels, "label_boxes: 1 <= k <= %d", kBoxMaxLabels);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* cnt = (unsigned long long*)counts;
  hipLaunchKernelGGL(boxes_init_kernel, cdiv(k, 256), 256, 0, st, boxes, cnt, k);
  const int rows = d * h;
  const int grid = lv_grid(rows, 4, 1024);
  const size_t lds = (size_t)k * 8 * sizeof(int);
#define BOXES(T) hipLaunchKernelGGL(boxes_kernel<T>, grid, 256, lds, st, (const T*)pred, (const T*)truth, d, h, w, k, boxes, cnt)
  LV_BY_LABEL(label_bytes, BOXES);
#undef BOXES
  hipLaunchKernelGGL(boxes_fin_kernel, cdiv(k, 256), 256, 0, st, boxes, (const unsigned long long*)cnt, k);
  SEGMI_LAUNCH_CHECK("label_boxes");
  return SEGMI_OK;
}

int64_t segmi_edt_workspace_bytes(int bd, int bh, int bw) {
  if (bd <= 0 || bh <= 0 || bw <= 0) return 0;
  return (int64_t)edt_layout(bd, bh, bw).total;
}

int segmi_edt_sq(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int label,
                 int feature, const int32_t* box, const float* spacing_zyx, float* dist_sq, void* workspace,
                 size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(labels && box && spacing_zyx && dist_sq && workspace, "edt_sq: null pointer");
  LV_CHECK_LABEL_BYTES("edt_sq", label_bytes);
  LV_CHECK_SPATIAL_DIMS("edt_sq", spatial_dims, d);
  SEGMI_CHECK_ARG(feature == 0 || feature == 1, "edt_sq: feature must be 0 (foreground) or 1 (contour)");
  LV_CHECK_BOX("edt_sq", box, d, h, w);
  LV_CHECK_SPACING("edt_sq", spacing_zyx);
  EdtParams p{};
  p.lab = labels; p.d = d; p.h = h; p.w = w; p.sd = spatial_dims; p.label = label;
  p.z0 = box[0]; p.y0 = box[2]; p.x0 = box[4];
  p.bd = box[1] - box[0]; p.bh = box[3] - box[2]; p.bw = box[5] - box[4];
  SEGMI_CHECK_ARG((int64_t)p.bh * p.bw < (1ll << 31) && (int64_t)p.bd * p.bh < (1ll << 31) &&
                  (int64_t)p.bd * p.bw < (1ll << 31), "edt_sq: crop too large");
  const EdtLayout l = edt_layout(p.bd, p.bh, p.bw);
  SEGMI_CHECK_ARG(ws_bytes >= l.total, "edt_sq: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
  char* ws = (char*)workspace;
  p.f1 = (float*)(ws + l.f1); p.sv = (int32_t*)(ws + l.sv); p.sg = (float*)(ws + l.sg);
  p.out = dist_sq;
  p.sz = spacing_zyx[0]; p.sy = spacing_zyx[1]; p.sx = spacing_zyx[2];
  const bool exact = p.sz == 1.f && p.sy == 1.f && p.sx == 1.f;
  hipStream_t st = (hipStream_t)stream;
  const int g1 = (int)cdiv64((int64_t)p.bh * p.bw, 256);
#define P1(T, CT) hipLaunchKernelGGL((edt_p1_kernel<T, CT>), g1, 256, 0, st, p)
  if (feature) LV_BY_LABEL(label_bytes, P1, true);
  else LV_BY_LABEL(label_bytes, P1, false);
#undef P1
  const int g2 = (int)cdiv64((int64_t)p.bd * p.bw, 256), g3 = (int)cdiv64((int64_t)p.bd * p.bh, 256);
#define P23(E, S)                                                  \
  do {                                                             \
    hipLaunchKernelGGL((edt_p2_kernel<E, S>), g2, 256, 0, st, p); \
    hipLaunchKernelGGL((edt_p3_kernel<E, S>), g3, 256, 0, st, p); \
  } while (0)
  if (exact) { if (feature) P23(true, true); else P23(true, false); }
  else { if (feature) P23(false, true); else P23(false, false); }
#undef P23
  SEGMI_LAUNCH_CHECK("edt_sq");
  return SEGMI_OK;
}

int segmi_edt_sample(const float* dist_sq, const void* labels, int label_bytes, int d, int h, int w,
                     int spatial_dims, int label, int query, const int32_t* box, double* stats, float* values,
                     int64_t* n_values, void* workspace, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(dist_sq && labels && box && stats && workspace, "edt_sample: null pointer");
  SEGMI_CHECK_ARG(!values || n_values, "edt_sample: values need the n_values counter");
  LV_CHECK_LABEL_BYTES("edt_sample", label_bytes);
  LV_CHECK_SPATIAL_DIMS("edt_sample", spatial_dims, d);
  SEGMI_CHECK_ARG(query == 0 || query == 1, "edt_sample: query must be 0 (foreground) or 1 (contour)");
  LV_CHECK_BOX("edt_sample", box, d, h, w);
  SampleParams p{};
  p.dist = dist_sq; p.lab = labels; p.d = d; p.h = h; p.w = w; p.sd = spatial_dims; p.label = label;
  p.z0 = box[0]; p.y0 = box[2]; p.x0 = box[4];
  p.bd = box[1] - box[0]; p.bh = box[3] - box[2]; p.bw = box[5] - box[4];
  SEGMI_CHECK_ARG((int64_t)p.bd * p.bh < (1ll << 31), "edt_sample: crop too large");
  const EdtLayout l = edt_layout(p.bd, p.bh, p.bw);
  SEGMI_CHECK_ARG(ws_bytes >= l.total, "edt_sample: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
  p.stats = stats; p.values = values; p.n_values = (unsigned long long*)n_values;
  p.partials = (double*)((char*)workspace + l.partials);
  p.ticket = g_fin_next.fetch_add(1) % kFinTickets;
  const int rows = p.bd * p.bh;
  const int grid = lv_grid(rows, 4, kSampleWgs);
  hipStream_t st = (hipStream_t)stream;
#define SAMPLE(T, CT) hipLaunchKernelGGL((sample_kernel<T, CT>), grid, 256, 0, st, p)
  if (query) LV_BY_LABEL(label_bytes, SAMPLE, true);
  else LV_BY_LABEL(label_bytes, SAMPLE, false);
#undef SAMPLE
  SEGMI_LAUNCH_CHECK("edt_sample");
  return SEGMI_OK;
}

int64_t segmi_select_workspace_bytes(int n_ranks) {
  if (n_ranks <= 0 || n_ranks > kSelectMaxRanks) return 0;
  return 256 + (int64_t)n_ranks * kSelectBins * (int64_t)sizeof(unsigned);
}

int segmi_select_f32(const float* values, const int64_t* n, const int64_t* ranks, int n_ranks, float* out,
                     void* workspace, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(values && n && ranks && out && workspace, "select_f32: null pointer");
  SEGMI_CHECK_ARG(n_ranks > 0 && n_ranks <= kSelectMaxRanks, "select_f32: 1 <= n_ranks <= %d", kSelectMaxRanks);
  SEGMI_CHECK_ARG(ws_bytes >= (size_t)segmi_select_workspace_bytes(n_ranks), "select_f32: workspace too small");
  SelectParams p{};
  p.values = values; p.n = n; p.ranks = ranks; p.n_ranks = n_ranks; p.out = out;
  p.state = (int64_t*)workspace;
  p.hist = (unsigned*)((char*)workspace + 256);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(select_init_kernel, 1, 256, 0, st, p);
  hipLaunchKernelGGL(select_hist_kernel<0>, kSelectWgs, 256, 0, st, p);
  hipLaunchKernelGGL(select_scan_kernel<0>, n_ranks, 256, 0, st, p);
  hipLaunchKernelGGL(select_hist_kernel<1>, kSelectWgs, 256, 0, st, p);
  hipLaunchKernelGGL(select_scan_kernel<1>, n_ranks, 256, 0, st, p);
  hipLaunchKernelGGL(select_hist_kernel<2>, kSelectWgs, 256, 0, st, p);
  hipLaunchKernelGGL(select_scan_kernel<2>, n_ranks, 256, 0, st, p);
  SEGMI_LAUNCH_CHECK("select_f32");
  return SEGMI_OK;
}

int segmi_confusion_counts(const void* pred, const void* truth, int label_bytes, int64_t n, int k, int64_t* cm,
                           void* stream) {
  SEGMI_CHECK_ARG(pred && truth && cm && n > 0, "confusion_counts: bad arguments");
  LV_CHECK_LABEL_BYTES("confusion_counts", label_bytes);
  SEGMI_CHECK_ARG(k > 0 && k <= 4096, "confusion_counts: 1 <= k <= 4096");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(cm, 0, (size_t)k * k * 8, st) != hipSuccess) {
    set_error("confusion_counts: memset failed");
    return SEGMI_ELAUNCH;
  }
  const int grid = lv_grid(n, 256, 1024);
  unsigned long long* c = (unsigned long long*)cm;
#define CM(T)                                                                                            \
  do {                                                                                                      \
    if (k <= 64) hipLaunchKernelGGL(confusion_lds_kernel<T>, grid, 256, 0, st, (const T*)pred, (const T*)truth, n, k, c); \
    else hipLaunchKernelGGL(confusion_global_kernel<T>, grid, 256, 0, st, (const T*)pred, (const T*)truth, n, k, c);      \
  } while (0)
  LV_BY_LABEL(label_bytes, CM);
#undef CM
  SEGMI_LAUNCH_CHECK("confusion_counts");
  return SEGMI_OK;
}

}  // extern "C"
