// tta.hip -- mirror test-time augmentation: per-pass softmax accumulated at the un-mirrored voxel, the
// finalisation of the accumulated scores (label, confidence, normalised entropy, probabilities) and the
// per-label means of a voxel map.  All streaming, HBM-bound; every result is specified operation by
// operation, so the file is built without contraction into FMAs.
//
// Three lane layouts, picked per call (tta_layout):
//   vec    K in {4, 8, 16, 32}, 16-byte aligned rows: K / 4 lanes share a voxel, 16 bytes per lane, a
//          wave-instruction moves 1 KiB of consecutive bytes.  Channel maxima go through a butterfly,
//          the ascending-channel sums through a lane-to-lane chain (chain_sum).
//   scalar every other K <= 32 (and unaligned views): one lane per voxel, the channels in registers.
//   wave   K > 32: a wave shares a voxel, lane l holds channels l, l + 64, ...
// vec and scalar lanes are dealt over segments of an output row (z, y); a mirrored x reverses the order
// of the voxels inside the segment a workgroup takes, so a wave still reads one consecutive span.
#include <mutex>

#include "fin_tail.h"

namespace segmi {

constexpr int kTtaMaxK = 512;
constexpr int kTtaMaxGrid = 8192;      // workgroups of 256 threads, the cap sliding.hip uses too
constexpr int kTtaScalarK = 32;        // channels a lane of the scalar layout keeps in registers

// first maximal index wins (the rule of segmi_argmax; scores are finite, no NaN handling needed)
__device__ __forceinline__ bool tta_better(float av, int ai, float bv, int bi) {
  return bv > av || (bv == av && bi < ai);
}

// Sum of the tpv * G values a lane group holds, in ascending channel order: lane `sub` owns channels
// [sub * G, sub * G + G).  Lane q takes the running sum of lane q - 1 and adds its own values one by
// one; the total is then broadcast.  Every lane of the wave must call it (tpv is wave-uniform).
template <int G>
__device__ __forceinline__ float chain_sum(const float (&v)[G], int sub, int tpv) {
  float r = 0.f;
  for (int q = 0; q < tpv; ++q) {
    const float prev = __shfl_up(r, 1, tpv);
    if (sub == q) {
      r = q == 0 ? v[0] : prev + v[0];
#pragma unroll
      for (int j = 1; j < G; ++j) r += v[j];
    }
  }
  return __shfl(r, tpv - 1, tpv);
}

// The same over the channels a wave holds as e[j] = channel j * 64 + lane: a scalar walk over the lanes.
template <int NJ>
__device__ __forceinline__ float wave_chain_sum(const float (&e)[NJ], int K) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = K - j * 64 < 64 ? K - j * 64 : 64;
    for (int l = 0; l < n; ++l) {
      const float t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e[j]), l));
      s = (j == 0 && l == 0) ? t : s + t;
    }
  }
  return s;
}

// Lanes over row segments: `lanes_row` lanes cover one row (z, y); a workgroup takes 256 consecutive
// lanes of a long row or 256 / lanes_row whole short rows.  32-bit index math only.
struct RowMap {
  int D, H, W, tpv, lanes_row, segs, rpw, nunits;
};
static inline bool row_map_make(RowMap& m, int D, int H, int W, int tpv) {
  if ((int64_t)W * tpv >= (1ll << 30) || (int64_t)D * H >= (1ll << 30)) return false;
  m.D = D; m.H = H; m.W = W; m.tpv = tpv;
  m.lanes_row = W * tpv;
  m.segs = (m.lanes_row + 255) / 256;
  m.rpw = m.lanes_row < 256 ? 256 / m.lanes_row : 1;
  const int64_t units = (((int64_t)D * H + m.rpw - 1) / m.rpw) * m.segs;
  if (units >= (1ll << 31)) return false;
  m.nunits = (int)units;
  return true;
}
struct RowLane {
  bool live;
  int z, y, x, sub;
};
__device__ __forceinline__ RowLane row_lane(const RowMap& m, int unit) {
  const int seg = unit % m.segs, grp = unit / m.segs;
  const int tid = (int)threadIdx.x;
  const int rl = m.rpw > 1 ? tid / m.lanes_row : 0;
  const int e = m.rpw > 1 ? tid - rl * m.lanes_row : seg * 256 + tid;
  const int row = grp * m.rpw + rl;
  RowLane r;
  r.live = rl < m.rpw && row < m.D * m.H && e < m.lanes_row;
  r.z = r.live ? row / m.H : 0;
  r.y = r.live ? row - r.z * m.H : 0;
  r.x = r.live ? e / m.tpv : 0;
  r.sub = e % m.tpv;
  return r;
}

// ------------------------------------------------------------------ accumulate
struct AccParams {
  const float* lg;      // [D][H][W] voxels of `ldl` floats
  float* acc;           // dense [D][H][W][K]
  RowMap m;
  int K, ldl, flip, first;
};

__device__ __forceinline__ int64_t mirrored_voxel(const AccParams& p, int z, int y, int x) {
  const int sz = (p.flip & 1) ? p.m.D - 1 - z : z;
  const int sy = (p.flip & 2) ? p.m.H - 1 - y : y;
  const int sx = (p.flip & 4) ? p.m.W - 1 - x : x;
  return ((int64_t)sz * p.m.H + sy) * p.m.W + sx;
}

__global__ __launch_bounds__(256) void tta_accumulate_vec_kernel(AccParams p) {
  const int tpv = p.m.tpv;
  for (int u = blockIdx.x; u < p.m.nunits; u += gridDim.x) {
    const RowLane r = row_lane(p.m, u);
    const int64_t v = ((int64_t)r.z * p.m.H + r.y) * p.m.W + r.x;
    float* ap = p.acc + v * p.K + r.sub * 4;
    f32x4 l = f32x4{0.f, 0.f, 0.f, 0.f}, a = l;
    if (r.live) {
      l = __builtin_nontemporal_load(
          reinterpret_cast<const f32x4*>(p.lg + mirrored_voxel(p, r.z, r.y, r.x) * p.ldl + r.sub * 4));
      if (!p.first) a = *reinterpret_cast<const f32x4*>(ap);
    }
    float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
    for (int o = 1; o < tpv; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = expf(l[j] - mx);
    const float s = chain_sum<4>(e, r.sub, tpv);
    if (r.live) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = p.first ? e[j] / s : a[j] + e[j] / s;
      *reinterpret_cast<f32x4*>(ap) = o;
    }
  }
}

__global__ __launch_bounds__(256) void tta_accumulate_scalar_kernel(AccParams p) {
  const int K = p.K;
  for (int u = blockIdx.x; u < p.m.nunits; u += gridDim.x) {
    const RowLane r = row_lane(p.m, u);
    if (!r.live) continue;
    const float* lp = p.lg + mirrored_voxel(p, r.z, r.y, r.x) * p.ldl;
    float* ap = p.acc + (((int64_t)r.z * p.m.H + r.y) * p.m.W + r.x) * K;
    float e[kTtaScalarK];
#pragma unroll
    for (int c = 0; c < kTtaScalarK; ++c) e[c] = c < K ? lp[c] : 0.f;
    float mx = e[0];
#pragma unroll
    for (int c = 1; c < kTtaScalarK; ++c)
      if (c < K) mx = fmaxf(mx, e[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < kTtaScalarK; ++c)
      if (c < K) {
        e[c] = expf(e[c] - mx);
        s = c == 0 ? e[0] : s + e[c];
      }
#pragma unroll
    for (int c = 0; c < kTtaScalarK; ++c)
      if (c < K) ap[c] = p.first ? e[c] / s : ap[c] + e[c] / s;
  }
}

// K > 32: one wave per output row (z, y) at a time, the lanes over the channels of one voxel
template <int NJ>
__global__ __launch_bounds__(256) void tta_accumulate_wave_kernel(AccParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = p.K, rows = p.m.D * p.m.H;
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const int z = row / p.m.H, y = row - z * p.m.H;
    for (int x = 0; x < p.m.W; ++x) {
      const float* lp = p.lg + mirrored_voxel(p, z, y, x) * p.ldl;
      float* ap = p.acc + ((int64_t)row * p.m.W + x) * K;
      float e[NJ], a[NJ];
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = j * 64 + lane;
        e[j] = c < K ? __builtin_nontemporal_load(lp + c) : -INFINITY;
        a[j] = (c < K && !p.first) ? ap[c] : 0.f;
        mx = fmaxf(mx, e[j]);
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
#pragma unroll
      for (int j = 0; j < NJ; ++j) e[j] = expf(e[j] - mx);      // dead lanes: exp(-inf) = 0, never summed
      const float s = wave_chain_sum<NJ>(e, K);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = j * 64 + lane;
        if (c < K) ap[c] = p.first ? e[j] / s : a[j] + e[j] / s;
      }
    }
  }
}

// ------------------------------------------------------------------ finalize
struct FinParams {
  const float* sc;     // voxels of `lds_` floats
  float* probs;        // nullable; may alias sc (same stride)
  void* labels;
  float* conf;         // nullable
  float* ent;          // nullable
  RowMap m;            // D = 1, H = rows of 2^16 voxels at most: the voxels are a flat list here
  int64_t nvox;
  int K, ld, ldp;
};

// q log q with 0 log 0 = 0
__device__ __forceinline__ float plogp(float q) { return q > 0.f ? q * logf(q) : 0.f; }
__device__ __forceinline__ float norm_entropy(float h, int K) {
  const float t = -h / logf((float)K);
  return t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
}

template <typename L>
__global__ __launch_bounds__(256) void tta_finalize_vec_kernel(FinParams p) {
  const int tpv = p.m.tpv;
  L* labels = (L*)p.labels;
  for (int u = blockIdx.x; u < p.m.nunits; u += gridDim.x) {
    const RowLane r = row_lane(p.m, u);
    const int64_t v = (int64_t)r.y * p.m.W + r.x;
    const bool live = r.live && v < p.nvox;
    float q[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p.sc + v * p.ld + r.sub * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = t[j];
    }
    const float s = chain_sum<4>(q, r.sub, tpv);
    const bool empty = s == 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = empty ? ((r.sub == 0 && j == 0) ? 1.f : 0.f) : q[j] / s;
    float bv = q[0];
    int bi = r.sub * 4;
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (tta_better(bv, bi, q[j], r.sub * 4 + j)) { bv = q[j]; bi = r.sub * 4 + j; }
    for (int o = 1; o < tpv; o <<= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (tta_better(bv, bi, ov, oi)) { bv = ov; bi = oi; }
    }
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = plogp(q[j]);
    const float h = chain_sum<4>(t, r.sub, tpv);
    if (live) {
      if (p.probs) *reinterpret_cast<f32x4*>(p.probs + v * p.ldp + r.sub * 4) = f32x4{q[0], q[1], q[2], q[3]};
      if (r.sub == 0) {
        labels[v] = (L)bi;
        if (p.conf) p.conf[v] = bv;
        if (p.ent) p.ent[v] = norm_entropy(h, p.K);
      }
    }
  }
}

template <typename L>
__global__ __launch_bounds__(256) void tta_finalize_scalar_kernel(FinParams p) {
  const int K = p.K;
  L* labels = (L*)p.labels;
  for (int64_t v = blockIdx.x * 256ll + threadIdx.x; v < p.nvox; v += (int64_t)gridDim.x * 256) {
    const float* sp = p.sc + v * p.ld;
    float q[kTtaScalarK];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < kTtaScalarK; ++c) {
      q[c] = c < K ? sp[c] : 0.f;
      if (c < K) s = c == 0 ? q[0] : s + q[c];
    }
    const bool empty = s == 0.f;
    float bv = 0.f, h = 0.f;
    int bi = 0;
#pragma unroll
    for (int c = 0; c < kTtaScalarK; ++c)
      if (c < K) {
        q[c] = empty ? (c == 0 ? 1.f : 0.f) : q[c] / s;
        if (c == 0) bv = q[0];
        else if (q[c] > bv) { bv = q[c]; bi = c; }
        const float t = plogp(q[c]);
        h = c == 0 ? t : h + t;
        if (p.probs) p.probs[v * p.ldp + c] = q[c];
      }
    labels[v] = (L)bi;
    if (p.conf) p.conf[v] = bv;
    if (p.ent) p.ent[v] = norm_entropy(h, K);
  }
}

template <typename L, int NJ>
__global__ __launch_bounds__(256) void tta_finalize_wave_kernel(FinParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = p.K;
  L* labels = (L*)p.labels;
  for (int64_t v = blockIdx.x * 4ll + wave; v < p.nvox; v += (int64_t)gridDim.x * 4) {
    const float* sp = p.sc + v * p.ld;
    float q[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = j * 64 + lane;
      q[j] = c < K ? sp[c] : 0.f;
    }
    const float s = wave_chain_sum<NJ>(q, K);
    const bool empty = s == 0.f;
    float bv = -1.f;
    int bi = 0x7fffffff;
    float t[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = j * 64 + lane;
      q[j] = empty ? (c == 0 ? 1.f : 0.f) : q[j] / s;
      if (c < K && tta_better(bv, bi, q[j], c)) { bv = q[j]; bi = c; }
      t[j] = c < K ? plogp(q[j]) : 0.f;
      if (p.probs && c < K) p.probs[v * p.ldp + c] = q[j];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (tta_better(bv, bi, ov, oi)) { bv = ov; bi = oi; }
    }
    const float h = wave_chain_sum<NJ>(t, K);
    if (lane == 0) {
      labels[v] = (L)bi;
      if (p.conf) p.conf[v] = bv;
      if (p.ent) p.ent[v] = norm_entropy(h, K);
    }
  }
}

// ------------------------------------------------------------------ per-label means
constexpr int kLmSlots = 4;                 // partial tables in flight (handed out round-robin with the tickets)
constexpr int kLmCells = 65536;             // rows * k of one partial table
constexpr int kLmMaxRows = 512;
constexpr int kLmMaxDevices = 16;

struct LmParams {
  const void* lab;
  const float* val;
  int64_t n;
  int k;
  double* sums;
  long long* counts;
  double* psum;                 // [gridDim.x][k]
  unsigned long long* pcnt;     // [gridDim.x][k]
  unsigned ticket;
};

// A wave takes 64 consecutive voxels at a time, chunk after chunk in a fixed order.  Per chunk it walks
// the distinct labels present (by first lane), sums the values of each with a fixed-shape butterfly and
// adds the sum to its own LDS bin.  The workgroup folds its four waves in wave order into row blockIdx.x
// of the partial table; the workgroup that draws the last ticket folds the rows in ascending order
// (fin_tail.h protocol on f64 rows, as distance.hip's sampler).  Nothing depends on arrival order.
template <typename T>
__global__ __launch_bounds__(256) void label_means_kernel(LmParams p) {
  extern __shared__ double lm_lds[];                      // [4][k] sums, then [4][k] counts
  __shared__ int s_last;
  const int k = p.k;
  double* bsum = lm_lds;
  unsigned long long* bcnt = reinterpret_cast<unsigned long long*>(lm_lds + 4 * k);
  for (int i = threadIdx.x; i < 4 * k; i += 256) { bsum[i] = 0.0; bcnt[i] = 0ull; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* lab = (const T*)p.lab;
  const int64_t nchunks = (p.n + 63) / 64;
  for (int64_t ch = blockIdx.x * 4ll + wave; ch < nchunks; ch += (int64_t)gridDim.x * 4) {
    const int64_t i = ch * 64 + lane;
    int l = -1;
    float x = 0.f;
    if (i < p.n) {
      l = (int)lab[i];
      x = p.val[i];
    }
    const bool todo = (unsigned)l < (unsigned)k;
    unsigned long long m = __ballot(todo);
    while (m) {
      const int lead = __ffsll((long long)m) - 1;
      const int cur = __shfl(l, lead);
      const bool mine = todo && l == cur;
      const unsigned long long pm = __ballot(mine);
      const double t = wave_sum(mine ? (double)x : 0.0);
      if (lane == 0) {
        bsum[wave * k + cur] += t;
        bcnt[wave * k + cur] += (unsigned long long)__popcll(pm);
      }
      m &= ~pm;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < k; c += 256) {
    const double s = ((bsum[c] + bsum[k + c]) + bsum[2 * k + c]) + bsum[3 * k + c];
    const unsigned long long q = bcnt[c] + bcnt[k + c] + bcnt[2 * k + c] + bcnt[3 * k + c];
    __hip_atomic_store(p.psum + (int64_t)blockIdx.x * k + c, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p.pcnt + (int64_t)blockIdx.x * k + c, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  fin_drain_stores();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(&g_fin_tickets[p.ticket], 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
    if (s_last) __hip_atomic_store(&g_fin_tickets[p.ticket], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  const int rows = (int)gridDim.x;
  for (int c = threadIdx.x; c < k; c += 256) {
    double s = 0.0;
    unsigned long long q = 0ull;
    int b = 0;
    for (; b + 8 <= rows; b += 8) {                       // 8 rows in flight, added in ascending order
      double ts[8];
      unsigned long long tq[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ts[j] = __hip_atomic_load(p.psum + (int64_t)(b + j) * k + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tq[j] = __hip_atomic_load(p.pcnt + (int64_t)(b + j) * k + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) { s += ts[j]; q += tq[j]; }
    }
    for (; b < rows; ++b) {
      s += __hip_atomic_load(p.psum + (int64_t)b * k + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      q += __hip_atomic_load(p.pcnt + (int64_t)b * k + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    p.sums[c] = s;
    p.counts[c] = (long long)q;
  }
}

// the partial tables: kLmSlots per device, allocated on first use and kept for the life of the process
static void* lm_workspace(unsigned slot) {
  static std::mutex mu;
  static void* ws[kLmMaxDevices][kLmSlots] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kLmMaxDevices) return nullptr;
  std::lock_guard<std::mutex> g(mu);
  if (!ws[dev][slot] && hipMalloc(&ws[dev][slot], (size_t)kLmCells * 16) != hipSuccess) {
    (void)hipGetLastError();
    ws[dev][slot] = nullptr;
  }
  return ws[dev][slot];
}

enum { kLayoutVec = 0, kLayoutScalar = 1, kLayoutWave = 2 };
static int tta_layout(int k, const void* a, int lda, const void* b, int ldb) {
  if (k > kTtaScalarK) return kLayoutWave;
  const int tpv = k / 4;
  const bool vec = k % 4 == 0 && (tpv & (tpv - 1)) == 0 && lda % 4 == 0 && ((uintptr_t)a % 16) == 0 &&
                   (!b || (ldb % 4 == 0 && ((uintptr_t)b % 16) == 0));
  return vec ? kLayoutVec : kLayoutScalar;
}
static inline int tta_grid(int64_t units) {
  return (int)(units > kTtaMaxGrid ? kTtaMaxGrid : (units < 1 ? 1 : units));
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int segmi_tta_accumulate(const segmi_act* logits, int flip_mask, float* acc, int first, void* stream) {
  SEGMI_CHECK_ARG(act_ok(logits) && acc && logits->n == 1, "tta_accumulate: bad arguments");
  SEGMI_CHECK_ARG(logits->c >= 2 && logits->c <= kTtaMaxK, "tta_accumulate: 2 <= K <= %d", kTtaMaxK);
  SEGMI_CHECK_ARG(flip_mask >= 0 && flip_mask < 8, "tta_accumulate: flip_mask has bits 0 (d), 1 (h), 2 (w) only");
  SEGMI_CHECK_ARG((const void*)logits->data != (const void*)acc, "tta_accumulate: acc must not alias the logits");
  AccParams p{};
  p.lg = (const float*)logits->data; p.acc = acc;
  p.K = logits->c; p.ldl = logits->ld; p.flip = flip_mask; p.first = first ? 1 : 0;
  const int layout = tta_layout(p.K, p.lg, p.ldl, acc, p.K);
  SEGMI_CHECK_ARG(row_map_make(p.m, logits->d, logits->h, logits->w, layout == kLayoutVec ? p.K / 4 : 1),
                  "tta_accumulate: volume too large");
  hipStream_t st = (hipStream_t)stream;
  if (layout == kLayoutVec) {
    hipLaunchKernelGGL(tta_accumulate_vec_kernel, tta_grid(p.m.nunits), 256, 0, st, p);
  } else if (layout == kLayoutScalar) {
    hipLaunchKernelGGL(tta_accumulate_scalar_kernel, tta_grid(p.m.nunits), 256, 0, st, p);
  } else {
    const int grid = tta_grid(((int64_t)p.m.D * p.m.H + 3) / 4);
    const int nj = (p.K + 63) / 64;
    if (nj <= 1) hipLaunchKernelGGL(tta_accumulate_wave_kernel<1>, grid, 256, 0, st, p);
    else if (nj <= 2) hipLaunchKernelGGL(tta_accumulate_wave_kernel<2>, grid, 256, 0, st, p);
    else if (nj <= 4) hipLaunchKernelGGL(tta_accumulate_wave_kernel<4>, grid, 256, 0, st, p);
    else hipLaunchKernelGGL(tta_accumulate_wave_kernel<8>, grid, 256, 0, st, p);
  }
  SEGMI_LAUNCH_CHECK("tta_accumulate");
  return SEGMI_OK;
}

int segmi_tta_finalize(const segmi_act* scores, int k, void* labels, int label_bytes, float* confidence,
                       float* entropy, const segmi_act* probs_out, void* stream) {
  SEGMI_CHECK_ARG(act_ok(scores) && labels, "tta_finalize: bad arguments");
  SEGMI_CHECK_ARG(k == scores->c && k >= 2 && k <= kTtaMaxK, "tta_finalize: k = channels of scores, 2 <= k <= %d", kTtaMaxK);
  SEGMI_CHECK_ARG(label_bytes == 1 || label_bytes == 4, "tta_finalize: label_bytes 1 or 4");
  SEGMI_CHECK_ARG(label_bytes > 1 || k <= 256, "tta_finalize: uint8 labels hold at most 256 classes");
  if (probs_out) {
    SEGMI_CHECK_ARG(act_ok(probs_out) && probs_out->c == k && act_voxels(probs_out) == act_voxels(scores),
                    "tta_finalize: probs_out must have the voxels and channels of scores");
    // in place is fine (a voxel is read whole before it is written); a shifted overlap is not
    SEGMI_CHECK_ARG(probs_out->data != scores->data || probs_out->ld == scores->ld,
                    "tta_finalize: probs_out aliasing scores needs the same voxel stride");
  }
  FinParams p{};
  p.sc = (const float*)scores->data;
  p.probs = probs_out ? (float*)probs_out->data : nullptr;
  p.labels = labels; p.conf = confidence; p.ent = entropy;
  p.nvox = act_voxels(scores);
  p.K = k; p.ld = scores->ld; p.ldp = probs_out ? probs_out->ld : 0;
  const int layout = tta_layout(k, p.sc, p.ld, p.probs, p.ldp);
  hipStream_t st = (hipStream_t)stream;
#define FIN(L, KERNEL, GRID, ...) hipLaunchKernelGGL((KERNEL<L, ##__VA_ARGS__>), GRID, 256, 0, st, p)
#define FIN_BY_LABEL(KERNEL, GRID, ...) SEGMI_BY_LABEL_14(label_bytes, FIN, KERNEL, GRID, ##__VA_ARGS__)
  if (layout == kLayoutVec) {
    // the flat voxel list as rows of 2^16 voxels: the lanes of a voxel stay together, no 64-bit division
    const int64_t roww = p.nvox < 65536 ? p.nvox : 65536;
    const int64_t nrows = (p.nvox + roww - 1) / roww;
    SEGMI_CHECK_ARG(nrows < (1ll << 30) && row_map_make(p.m, 1, (int)nrows, (int)roww, k / 4),
                    "tta_finalize: volume too large");
    FIN_BY_LABEL(tta_finalize_vec_kernel, tta_grid(p.m.nunits));
  } else if (layout == kLayoutScalar) {
    FIN_BY_LABEL(tta_finalize_scalar_kernel, tta_grid((p.nvox + 255) / 256));
  } else {
    const int grid = tta_grid((p.nvox + 3) / 4);
    const int nj = (k + 63) / 64;
    if (nj <= 1) FIN_BY_LABEL(tta_finalize_wave_kernel, grid, 1);
    else if (nj <= 2) FIN_BY_LABEL(tta_finalize_wave_kernel, grid, 2);
    else if (nj <= 4) FIN_BY_LABEL(tta_finalize_wave_kernel, grid, 4);
    else FIN_BY_LABEL(tta_finalize_wave_kernel, grid, 8);
  }
#undef FIN_BY_LABEL
#undef FIN
  SEGMI_LAUNCH_CHECK("tta_finalize");
  return SEGMI_OK;
}

int segmi_label_means(const void* labels, int label_bytes, const float* values, int64_t n, int k, double* sums,
                      int64_t* counts, void* stream) {
  SEGMI_CHECK_ARG(labels && values && sums && counts && n > 0, "label_means: bad arguments");
  SEGMI_CHECK_ARG(label_bytes == 1 || label_bytes == 4, "label_means: label_bytes 1 or 4");
  SEGMI_CHECK_ARG(k >= 1 && k <= kTtaMaxK, "label_means: 1 <= k <= %d", kTtaMaxK);
  LmParams p{};
  p.lab = labels; p.val = values; p.n = n; p.k = k; p.sums = sums; p.counts = (long long*)counts;
  const unsigned draw = g_fin_next.fetch_add(1);
  p.ticket = draw % kFinTickets;
  char* ws = (char*)lm_workspace(draw % kLmSlots);
  if (!ws) {
    set_error("label_means: no memory for the partial tables");
    return SEGMI_ELAUNCH;
  }
  int rows = kLmCells / k;
  rows = rows > kLmMaxRows ? kLmMaxRows : rows;
  const int64_t want = (n + 64 * 4 * 8 - 1) / (64 * 4 * 8);       // >= 8 chunks per wave before another workgroup
  const int grid = (int)(want < 1 ? 1 : (want > rows ? rows : want));
  p.psum = (double*)ws;
  p.pcnt = (unsigned long long*)(ws + (size_t)kLmCells * 8);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)k * 4 * 16;
#define LABEL_MEANS(L) hipLaunchKernelGGL(label_means_kernel<L>, grid, 256, lds, st, p)
  SEGMI_BY_LABEL_14(label_bytes, LABEL_MEANS);
#undef LABEL_MEANS
  SEGMI_LAUNCH_CHECK("label_means");
  return SEGMI_OK;
}

}  // extern "C"
