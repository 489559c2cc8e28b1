// nyul.hip -- Nyul-Udupa histogram standardisation: exact quantile landmarks of each segment (a channel,
// or the whole tensor) by a segmented, masked, multi-rank radix select, then the piecewise-linear map.
// Replaces src/segmantic/seg/nyul_normalize.py:46-70 (torch.quantile / np.quantile + interp1d).
//
// Keys: f32 bits mapped to an order-preserving u32 (negatives: all bits flipped; non-negatives: sign bit
// set), so signed intensities order correctly (-0.0 and +0.0 are adjacent keys of equal value).  NaN is
// counted, never histogrammed.  Digits: bits 31..21 (pass A), 20..10 (pass B), 9..0 (pass C).
//   pass A : per segment, masked count, NaN count and the 2048-bin histogram of the top digit.
//   ranks  : from n, the two ranks of each landmark (torch's f32 rule for n <= 2^24, numpy's f64 rule
//            above), each rank's top digit, and the distinct active prefixes ("slots", sorted).
//   pass B/C: only elements whose prefix is a slot are histogrammed, into that slot's bins.  The slots of
//            a pass are disjoint, so an element adds to at most one bin; a 2048-entry LDS table (top digit ->
//            first slot) rejects the others with one LDS read.  A workgroup holds kSlotsLds slots' bins in
//            LDS; more slots are covered by further slot groups (grid.z), each re-reading the segment.
//   finalise: lerp of the two order statistics per landmark.
// All state lives in the workspace; no host round trip between passes.  Same-bin runs (a constant
// background) are aggregated per wave before the LDS atomic.
#include "labelvol.h"

// Built with -ffp-contract=off (Makefile): the HIP headers' __fmul_rn & co. are plain operators that
// would otherwise be fused with their neighbours; the two fused lerps are explicit __fmaf_rn calls.
#pragma clang fp contract(off)

namespace segmi {

constexpr int kNyulMaxLandmarks = 64;
constexpr int kNyulMaxRanks = 2 * kNyulMaxLandmarks;
constexpr int kNyulBins = 2048;
constexpr int kSlotsLds = 16;             // 16 slots x 2048 u32 = 128 KiB of LDS in pass B
constexpr int kHistThreads = 1024;
constexpr int kExactRankLimit = 1 << 24;  // torch.quantile's largest input


// per-segment workspace record (then the histograms)
struct NyulSeg {
  unsigned long long n;         // masked, non-NaN values
  unsigned long long nan;       // masked NaN values
  int nslot;                    // distinct active prefixes of the current pass (0: nothing to select)
  int pad;
  unsigned prefix[kNyulMaxRanks];
  long long rem[kNyulMaxRanks]; // rank still to skip inside the prefix
  int slotof[kNyulMaxRanks];
  unsigned slotpre[kNyulMaxRanks];
};

struct NyulLayout {
  size_t seg, hist0, hist1, hist2, total;  // per-segment strides are derived from n_ranks
};

static NyulLayout nyul_layout(int segments, int n_ranks) {
  NyulLayout l{};
  l.seg = 0;
  l.hist0 = lv_align256((size_t)segments * sizeof(NyulSeg));
  l.hist1 = l.hist0 + lv_align256((size_t)segments * kNyulBins * 8);
  l.hist2 = l.hist1 + lv_align256((size_t)segments * n_ranks * kNyulBins * 8);
  l.total = l.hist2 + lv_align256((size_t)segments * n_ranks * (kNyulBins / 2) * 8);
  return l;
}

struct NyulParams {
  const float* x;
  int64_t seg_len;
  int segments;
  int nonzero;
  int nq;                       // landmarks L; ranks = 2L
  NyulSeg* seg;
  unsigned long long* hist0;    // [S][2048]
  unsigned long long* hist1;    // [S][2L][2048]
  unsigned long long* hist2;    // [S][2L][1024]
  float* landmarks;             // [S][L]
  int64_t* counts;              // [S]
  double q[kNyulMaxLandmarks];
};

__device__ __forceinline__ unsigned f2key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// one LDS count per wave when every active lane hits the same bin (b < 0: no bin)
__device__ __forceinline__ void wave_add(unsigned* h, int b) {
  const int b0 = __builtin_amdgcn_readfirstlane(b);
  const unsigned long long act = __ballot(1);
  const unsigned long long same = __ballot(b == b0);
  if (same == act) {
    if (b0 >= 0 && (int)__lane_id() == __ffsll((long long)act) - 1) atomicAdd(&h[b0], (unsigned)__popcll(act));
  } else if (b >= 0) {
    atomicAdd(&h[b], 1u);
  }
}

// f(v) for every element of one segment, float4 loads when VEC; this thread's share of `parts`
template <bool VEC, typename F>
__device__ __forceinline__ void for_segment(const float* p, int64_t len, int64_t t, int64_t parts, F f) {
  if (VEC) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (int64_t i = t; i < len / 4; i += parts) {
      const float4 v = p4[i];
      f(v.x); f(v.y); f(v.z); f(v.w);
    }
  } else {
    for (int64_t i = t; i < len; i += parts) f(p[i]);
  }
}

// ------------------------------------------------------------------ pass A
template <bool VEC>
__global__ __launch_bounds__(kHistThreads) void nyul_pass_a_kernel(NyulParams p) {
  __shared__ unsigned s_hist[kNyulBins];
  __shared__ unsigned long long s_cnt[2];
  const int s = blockIdx.y;
  for (int i = threadIdx.x; i < kNyulBins; i += kHistThreads) s_hist[i] = 0;
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  unsigned n = 0, nan = 0;
  const bool nz = p.nonzero;
  for_segment<VEC>(p.x + (int64_t)s * p.seg_len, p.seg_len, (int64_t)blockIdx.x * kHistThreads + threadIdx.x,
                   (int64_t)gridDim.x * kHistThreads, [&](float v) {
    int b = -1;
    if (!nz || v != 0.0f) {
      if (v != v) ++nan;
      else { ++n; b = (int)(f2key(v) >> 21); }
    }
    wave_add(s_hist, b);
  });
  atomicAdd(&s_cnt[0], (unsigned long long)n);
  atomicAdd(&s_cnt[1], (unsigned long long)nan);
  __syncthreads();
  unsigned long long* h = p.hist0 + (size_t)s * kNyulBins;
  for (int i = threadIdx.x; i < kNyulBins; i += kHistThreads)
    if (s_hist[i]) atomicAdd(h + i, (unsigned long long)s_hist[i]);
  if (threadIdx.x == 0) {
    if (s_cnt[0]) atomicAdd(&p.seg[s].n, s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&p.seg[s].nan, s_cnt[1]);
  }
}

// rank r of landmark r/2 (lo for even r, hi for odd) and its weight, by the regime of n
struct RankW { long long lo, hi; double w; };
__device__ __forceinline__ RankW landmark_rank(double q, long long n) {
  RankW r;
  if (n <= kExactRankLimit) {  // torch.quantile: ranks = f32(q) * (n - 1) in f32
    const float rank = __fmul_rn((float)q, (float)(n - 1));
    r.lo = (long long)truncf(rank);
    r.hi = (long long)ceilf(rank);
    r.w = (double)__fsub_rn(rank, (float)r.lo);
  } else {                     // numpy.quantile 'linear': virtual index in f64
    const double vi = __dmul_rn(q, (double)(n - 1));
    const double fl = floor(vi);
    r.lo = (long long)fl;
    r.hi = vi >= (double)(n - 1) ? r.lo : r.lo + 1;
    r.w = __dsub_rn(vi, fl);
  }
  return r;
}

// distinct prefixes of the segment's ranks, sorted: seg.nslot, seg.slotpre, seg.slotof.  R <= 128 threads.
__device__ void nyul_dedup(NyulSeg& g, int R, unsigned* s_pre, int* s_first) {
  const int r = threadIdx.x;
  if (r < R) s_pre[r] = g.prefix[r];
  __syncthreads();
  if (r < R) {
    int first = 1;
    for (int k = 0; k < r; ++k) first &= s_pre[k] != s_pre[r];
    s_first[r] = first;
  }
  __syncthreads();
  if (r < R) {
    int below = 0;
    for (int k = 0; k < R; ++k) below += s_first[k] && s_pre[k] < s_pre[r];
    g.slotof[r] = below;
    if (s_first[r]) g.slotpre[below] = s_pre[r];
  }
  if (r == 0) {
    int c = 0;
    for (int k = 0; k < R; ++k) c += s_first[k];
    g.nslot = c;
  }
}

// exclusive scan of BINS u64 counts in s_cum[0..BINS] by 256 threads; returns this thread's first bin
template <int BINS>
__device__ void scan_bins(const unsigned long long* h, unsigned long long* s_cum, unsigned long long* s_part) {
  constexpr int per = BINS / 256;
  const int tid = threadIdx.x;
  unsigned long long loc[per], tot = 0;
#pragma unroll
  for (int j = 0; j < per; ++j) { loc[j] = h[tid * per + j]; tot += loc[j]; }
  s_part[tid] = tot;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned long long v = tid >= o ? s_part[tid - o] : 0;
    __syncthreads();
    s_part[tid] += v;
    __syncthreads();
  }
  unsigned long long c = s_part[tid] - tot;
#pragma unroll
  for (int j = 0; j < per; ++j) { s_cum[tid * per + j] = c; c += loc[j]; }
  if (tid == 255) s_cum[BINS] = c;
  __syncthreads();
}

// first bin b with cum[b] <= r < cum[b + 1]
template <int BINS>
__device__ __forceinline__ int find_bin(const unsigned long long* cum, unsigned long long r) {
  int lo = 0, hi = BINS - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cum[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one workgroup (256 threads) per segment: ranks, their top digits, slots of pass B
__global__ __launch_bounds__(256) void nyul_ranks_kernel(NyulParams p) {
  __shared__ unsigned long long s_cum[kNyulBins + 1];
  __shared__ unsigned long long s_part[256];
  __shared__ unsigned s_pre[kNyulMaxRanks];
  __shared__ int s_first[kNyulMaxRanks];
  const int s = blockIdx.x, R = 2 * p.nq, tid = threadIdx.x;
  NyulSeg& g = p.seg[s];
  const unsigned long long n = g.n;
  scan_bins<kNyulBins>(p.hist0 + (size_t)s * kNyulBins, s_cum, s_part);
  if (n == 0 || g.nan) {  // nothing to select: empty or NaN segment
    if (tid == 0) g.nslot = 0;
    return;
  }
  if (tid < R) {
    const RankW rw = landmark_rank(p.q[tid >> 1], (long long)n);
    const unsigned long long r = (unsigned long long)((tid & 1) ? rw.hi : rw.lo);
    const int b = find_bin<kNyulBins>(s_cum, r);
    g.prefix[tid] = (unsigned)b << 21;
    g.rem[tid] = (long long)(r - s_cum[b]);
  }
  __syncthreads();
  nyul_dedup(g, R, s_pre, s_first);
}

// ------------------------------------------------------------------ passes B and C
// PASS 1: prefix = top 11 bits, digit = bits 20..10; PASS 2: prefix = top 22 bits, digit = bits 9..0
template <int PASS, bool VEC>
__global__ __launch_bounds__(kHistThreads) void nyul_pass_bc_kernel(NyulParams p) {
  constexpr int BINS = PASS == 1 ? kNyulBins : kNyulBins / 2;
  constexpr int shift = PASS == 1 ? 10 : 0;
  constexpr unsigned pmask = PASS == 1 ? 0xffe00000u : 0xfffffc00u;
  __shared__ unsigned s_hist[kSlotsLds * BINS];
  __shared__ short s_table[kNyulBins];
  __shared__ unsigned s_sp[kNyulMaxRanks];
  const int s = blockIdx.y, g0 = blockIdx.z * kSlotsLds;
  const NyulSeg& g = p.seg[s];
  const int nsl = g.nslot;
  if (g0 >= nsl) return;
  const int nloc = nsl - g0 < kSlotsLds ? nsl - g0 : kSlotsLds;
  for (int i = threadIdx.x; i < kNyulBins; i += kHistThreads) s_table[i] = -1;
  for (int i = threadIdx.x; i < nloc * BINS; i += kHistThreads) s_hist[i] = 0;
  if (threadIdx.x < nsl) s_sp[threadIdx.x] = g.slotpre[threadIdx.x];
  __syncthreads();
  if (threadIdx.x < nsl) {
    const unsigned top = s_sp[threadIdx.x] >> 21;
    if (threadIdx.x == 0 || (s_sp[threadIdx.x - 1] >> 21) != top) s_table[top] = (short)threadIdx.x;
  }
  __syncthreads();
  const bool nz = p.nonzero;
  for_segment<VEC>(p.x + (int64_t)s * p.seg_len, p.seg_len, (int64_t)blockIdx.x * kHistThreads + threadIdx.x,
                   (int64_t)gridDim.x * kHistThreads, [&](float v) {
    int b = -1;
    if ((!nz || v != 0.0f) && v == v) {
      const unsigned k = f2key(v);
      int j = s_table[k >> 21];
      if (j >= 0) {
        if (PASS == 2)
          while (j < nsl && s_sp[j] != (k & pmask) && (s_sp[j] >> 21) == (k >> 21)) ++j;
        if (j < nsl && s_sp[j] == (k & pmask) && j >= g0 && j < g0 + nloc)
          b = (j - g0) * BINS + (int)((k >> shift) & (BINS - 1));
      }
    }
    wave_add(s_hist, b);
  });
  __syncthreads();
  unsigned long long* h = (PASS == 1 ? p.hist1 : p.hist2) + ((size_t)s * 2 * p.nq + g0) * BINS;
  for (int i = threadIdx.x; i < nloc * BINS; i += kHistThreads)
    if (s_hist[i]) atomicAdd(h + i, (unsigned long long)s_hist[i]);
}

// grid (slot, segment): resolve the digit of every rank in the slot
template <int PASS>
__global__ __launch_bounds__(256) void nyul_scan_kernel(NyulParams p) {
  constexpr int BINS = PASS == 1 ? kNyulBins : kNyulBins / 2;
  constexpr int shift = PASS == 1 ? 10 : 0;
  __shared__ unsigned long long s_cum[BINS + 1];
  __shared__ unsigned long long s_part[256];
  const int j = blockIdx.x, s = blockIdx.y, R = 2 * p.nq;
  NyulSeg& g = p.seg[s];
  if (j >= g.nslot) return;
  scan_bins<BINS>((PASS == 1 ? p.hist1 : p.hist2) + ((size_t)s * R + j) * BINS, s_cum, s_part);
  if ((int)threadIdx.x < R && g.slotof[threadIdx.x] == j) {
    const int r = threadIdx.x;
    const unsigned long long rem = (unsigned long long)g.rem[r];
    const int b = find_bin<BINS>(s_cum, rem);
    g.prefix[r] |= (unsigned)b << shift;
    g.rem[r] = (long long)(rem - s_cum[b]);
  }
}

// after pass B: the slots of pass C
__global__ __launch_bounds__(256) void nyul_reslot_kernel(NyulParams p) {
  __shared__ unsigned s_pre[kNyulMaxRanks];
  __shared__ int s_first[kNyulMaxRanks];
  NyulSeg& g = p.seg[blockIdx.x];
  if (g.nslot == 0) return;
  nyul_dedup(g, 2 * p.nq, s_pre, s_first);
}

// lerp of the order statistics: a + w(b-a) for |w| < 0.5, else b - (b-a)(1-w).  For n <= 2^24 in f32 with
// the product fused into the add, as torch's lerp kernels compute it (bit-equal to torch.quantile); above,
// in f64 with every operation rounded, as numpy's _lerp does, then rounded to f32.
__global__ __launch_bounds__(64) void nyul_finalize_kernel(NyulParams p) {
  const int s = blockIdx.x, j = threadIdx.x;
  const NyulSeg& g = p.seg[s];
  if (j == 0) p.counts[s] = (int64_t)(g.n + g.nan);
  if (j >= p.nq) return;
  float out;
  if (g.n == 0 || g.nan) {
    out = __builtin_nanf("");
  } else {
    const float a = key2f(g.prefix[2 * j]), b = key2f(g.prefix[2 * j + 1]);
    const RankW rw = landmark_rank(p.q[j], (long long)g.n);
    if (g.n <= (unsigned long long)kExactRankLimit) {
      const float w = (float)rw.w, d = __fsub_rn(b, a);
      out = fabsf(w) < 0.5f ? __fmaf_rn(w, d, a) : __fmaf_rn(-d, __fsub_rn(1.0f, w), b);
    } else {
      const double w = rw.w, da = a, d = __dsub_rn((double)b, da);
      out = (float)(w < 0.5 ? __dadd_rn(da, __dmul_rn(w, d)) : __dsub_rn((double)b, __dmul_rn(d, __dsub_rn(1.0, w))));
    }
  }
  p.landmarks[(size_t)s * p.nq + j] = out;
}

// ------------------------------------------------------------------ map
struct NyulMapParams {
  float* x;
  int64_t seg_len;
  int nonzero;
  int nq;
  const float* landmarks;
  const int64_t* counts;
  float scale[kNyulMaxLandmarks];
};

template <bool VEC>
__global__ __launch_bounds__(256) void nyul_map_kernel(NyulMapParams p) {
  __shared__ float s_xp[kNyulMaxLandmarks], s_m[kNyulMaxLandmarks], s_b[kNyulMaxLandmarks];
  const int s = blockIdx.y, L = p.nq;
  if (p.counts && p.counts[s] == 0) return;  // empty mask: bit-untouched
  if (threadIdx.x < L) s_xp[threadIdx.x] = p.landmarks[(size_t)s * L + threadIdx.x];
  __syncthreads();
  if (threadIdx.x < L - 1) {
    const int i = threadIdx.x;
    const float m = __fdiv_rn(__fsub_rn(p.scale[i + 1], p.scale[i]), __fsub_rn(s_xp[i + 1], s_xp[i]));
    s_m[i] = m;
    s_b[i] = __fsub_rn(p.scale[i], __fmul_rn(m, s_xp[i]));
  }
  __syncthreads();
  const bool nz = p.nonzero;
  auto f = [&](float v) -> float {
    if (nz && v == 0.0f) return v;
    int lo = 0, hi = L;  // torch.searchsorted (left): first xp not below v
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (!(s_xp[mid] >= v)) lo = mid + 1; else hi = mid;
    }
    const int i = lo - 1 < 0 ? 0 : (lo - 1 > L - 2 ? L - 2 : lo - 1);
    return __fadd_rn(__fmul_rn(s_m[i], v), s_b[i]);
  };
  float* base = p.x + (int64_t)s * p.seg_len;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, parts = (int64_t)gridDim.x * 256;
  if (VEC) {
    float4* p4 = reinterpret_cast<float4*>(base);
    for (int64_t i = t; i < p.seg_len / 4; i += parts) {
      float4 v = p4[i];
      v.x = f(v.x); v.y = f(v.y); v.z = f(v.z); v.w = f(v.w);
      p4[i] = v;
    }
  } else {
    for (int64_t i = t; i < p.seg_len; i += parts) base[i] = f(base[i]);
  }
}

static int chunks_per_segment(int64_t seg_len, int segments, int per_chip, int threads) {
  int64_t c = cdiv64(per_chip, segments);
  const int64_t need = cdiv64(seg_len, (int64_t)threads * 4);
  if (c > need) c = need;
  return c < 1 ? 1 : (int)c;
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int64_t segmi_nyul_workspace_bytes(int segments, int n_quantiles) {
  if (segments <= 0 || segments > 65535 || n_quantiles < 2 || n_quantiles > kNyulMaxLandmarks) return 0;
  return (int64_t)nyul_layout(segments, 2 * n_quantiles).total;
}

int segmi_nyul_landmarks(const float* x, int segments, int64_t seg_len, int nonzero, const double* quantiles_host,
                         int n_quantiles, float* landmarks, int64_t* counts, void* workspace, size_t ws_bytes,
                         void* stream) {
  SEGMI_CHECK_ARG(x && quantiles_host && landmarks && counts && workspace, "nyul_landmarks: null pointer");
  SEGMI_CHECK_ARG(segments > 0 && segments <= 65535 && seg_len > 0, "nyul_landmarks: bad segments / seg_len");
  SEGMI_CHECK_ARG(n_quantiles >= 2 && n_quantiles <= kNyulMaxLandmarks, "nyul_landmarks: 2 <= n_quantiles <= %d",
                  kNyulMaxLandmarks);
  const NyulLayout l = nyul_layout(segments, 2 * n_quantiles);
  SEGMI_CHECK_ARG(ws_bytes >= l.total, "nyul_landmarks: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
  NyulParams p{};
  p.x = x; p.seg_len = seg_len; p.segments = segments; p.nonzero = nonzero ? 1 : 0; p.nq = n_quantiles;
  for (int i = 0; i < n_quantiles; ++i) {
    SEGMI_CHECK_ARG(quantiles_host[i] >= 0.0 && quantiles_host[i] <= 1.0 &&
                    (i == 0 || quantiles_host[i] >= quantiles_host[i - 1]),
                    "nyul_landmarks: quantiles must be sorted and in [0, 1]");
    p.q[i] = quantiles_host[i];
  }
  char* ws = (char*)workspace;
  p.seg = (NyulSeg*)(ws + l.seg);
  p.hist0 = (unsigned long long*)(ws + l.hist0);
  p.hist1 = (unsigned long long*)(ws + l.hist1);
  p.hist2 = (unsigned long long*)(ws + l.hist2);
  p.landmarks = landmarks; p.counts = counts;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, l.total, st) != hipSuccess) {
    set_error("nyul_landmarks: memset failed");
    return SEGMI_ELAUNCH;
  }
  const bool vec = seg_len % 4 == 0 && ((uintptr_t)x & 15) == 0;
  const int R = 2 * n_quantiles;
  const dim3 ga(chunks_per_segment(seg_len, segments, 512, kHistThreads), segments);
  const dim3 gbc(chunks_per_segment(seg_len, segments, 256, kHistThreads), segments, cdiv(R, kSlotsLds));
  if (vec) hipLaunchKernelGGL(nyul_pass_a_kernel<true>, ga, kHistThreads, 0, st, p);
  else hipLaunchKernelGGL(nyul_pass_a_kernel<false>, ga, kHistThreads, 0, st, p);
  hipLaunchKernelGGL(nyul_ranks_kernel, segments, 256, 0, st, p);
  if (vec) hipLaunchKernelGGL((nyul_pass_bc_kernel<1, true>), gbc, kHistThreads, 0, st, p);
  else hipLaunchKernelGGL((nyul_pass_bc_kernel<1, false>), gbc, kHistThreads, 0, st, p);
  hipLaunchKernelGGL(nyul_scan_kernel<1>, dim3(R, segments), 256, 0, st, p);
  hipLaunchKernelGGL(nyul_reslot_kernel, segments, 256, 0, st, p);
  if (vec) hipLaunchKernelGGL((nyul_pass_bc_kernel<2, true>), gbc, kHistThreads, 0, st, p);
  else hipLaunchKernelGGL((nyul_pass_bc_kernel<2, false>), gbc, kHistThreads, 0, st, p);
  hipLaunchKernelGGL(nyul_scan_kernel<2>, dim3(R, segments), 256, 0, st, p);
  hipLaunchKernelGGL(nyul_finalize_kernel, segments, 64, 0, st, p);
  SEGMI_LAUNCH_CHECK("nyul_landmarks");
  return SEGMI_OK;
}

int segmi_nyul_apply(float* x, int segments, int64_t seg_len, int nonzero, const float* landmarks,
                     const int64_t* counts, const float* standard_scale_host, int n_quantiles, void* stream) {
  SEGMI_CHECK_ARG(x && landmarks && standard_scale_host, "nyul_apply: null pointer");
  SEGMI_CHECK_ARG(segments > 0 && segments <= 65535 && seg_len > 0, "nyul_apply: bad segments / seg_len");
  SEGMI_CHECK_ARG(n_quantiles >= 2 && n_quantiles <= kNyulMaxLandmarks, "nyul_apply: 2 <= n_quantiles <= %d",
                  kNyulMaxLandmarks);
  NyulMapParams p{};
  p.x = x; p.seg_len = seg_len; p.nonzero = nonzero ? 1 : 0; p.nq = n_quantiles;
  p.landmarks = landmarks; p.counts = counts;
  for (int i = 0; i < n_quantiles; ++i) p.scale[i] = standard_scale_host[i];
  const bool vec = seg_len % 4 == 0 && ((uintptr_t)x & 15) == 0;
  const dim3 grid(chunks_per_segment(seg_len, segments, 2048, 256), segments);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(nyul_map_kernel<true>, grid, 256, 0, st, p);
  else hipLaunchKernelGGL(nyul_map_kernel<false>, grid, 256, 0, st, p);
  SEGMI_LAUNCH_CHECK("nyul_apply");
  return SEGMI_OK;
}

}  // extern "C"
