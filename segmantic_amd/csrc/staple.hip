// staple.hip -- multi-label STAPLE fusion of R label volumes (Warfield et al. 2004 in the multi-label form of
// ITK's MultiLabelSTAPLEImageFilter), DESIGN.md section 22.  Posteriors are fixed point (Q = 2^24) and every
// sum is an integer, so the result does not depend on launch shape or arrival order.  Built with
// -ffp-contract=off: the E-step is specified operation by operation in float64.
//
// Launches of one call:
//   staple_count_kernel   prior counts, agreed-voxel counts per label, start M-step of the one-hot vote
//   staple_table_kernel   (start)  prior, theta_0
//   per iteration:
//   staple_em_kernel      E-step of the disputed voxels, their q added into S (LDS table, or global atomics)
//   staple_table_kernel   agreed voxels added as count[l] * q_cons[l][.], theta, delta, the stop flag
//   staple_final_kernel   E-step with the theta of the last E-step: labels and (on request) the posterior
// The stop flag lives on the device: passes launched after the stop return at once, and the host reads the
// state back once every kStapleChunk iterations.
#include "labelvol.h"

namespace segmi {

constexpr int kStapleMaxRaters = 16;
constexpr int kStapleMaxLabels = 64;
constexpr int kStapleGridCap = 4096;       // workgroups of 256: one pass of the grid covers 1 048 576 voxels
constexpr int kStapleLdsEntries = 6144;    // R * L * L int64 entries (48 KB) that the workgroup table holds
constexpr int kStapleChunk = 16;           // iterations enqueued between two read-backs of the state
constexpr double kStapleQ = 16777216.0;    // 2^24
constexpr long long kStapleQi = 1ll << 24;

typedef unsigned long long u64;

struct StapleState {
  int32_t it, converged, done, cur;        // cur: which of the two theta buffers the next E-step reads
  u64 bad;                                 // ~(voxel << 4 | rater) of the first label outside 0 .. L-1, 0 = none
  double delta;
};

struct StaplePtrs {
  const void* p[kStapleMaxRaters];
};
struct StaplePrior {
  int given;
  double v[kStapleMaxLabels];
};

struct StapleWs {
  StapleState* state;
  u64* cnt;        // [L]       label counts over all raters
  u64* agree;      // [L]       voxels on which every rater says l
  u64* acc;        // [R][L][L] sums of the disputed voxels of the pass in flight
  double* theta;   // [2][R][L][L]
  double* prior;   // [L]
};

struct StapleLayout {
  size_t state, cnt, agree, acc, theta, prior, total, zeroed;
};
static inline StapleLayout staple_layout(int r, int l) {
  StapleLayout o;
  LvCarver c;
  const size_t e = (size_t)r * l * l;
  o.state = c.take(sizeof(StapleState));
  o.cnt = c.take(sizeof(u64) * l);
  o.agree = c.take(sizeof(u64) * l);
  o.acc = c.take(sizeof(u64) * e);
  o.zeroed = c.off;                        // everything up to here starts at zero
  o.theta = c.take(sizeof(double) * 2 * e);
  o.prior = c.take(sizeof(double) * l);
  o.total = c.off;
  return o;
}
static inline StapleWs staple_carve(void* ws, const StapleLayout& o) {
  char* b = (char*)ws;
  return StapleWs{(StapleState*)(b + o.state), (u64*)(b + o.cnt), (u64*)(b + o.agree), (u64*)(b + o.acc),
                  (double*)(b + o.theta), (double*)(b + o.prior)};
}
// the one place that decides between the workgroup table in LDS and global atomics
static inline bool staple_lds_table(int r, int l) { return (int64_t)r * l * l <= kStapleLdsEntries; }

// labels of voxel i; false (and the flag raised) when one lies outside 0 .. L-1
template <typename T>
__device__ __forceinline__ bool staple_load(const StaplePtrs& ptrs, int R, int L, int64_t i, int (&lab)[kStapleMaxRaters],
                                            StapleState* state) {
  bool ok = true;
#pragma unroll
  for (int r = 0; r < kStapleMaxRaters; ++r) {
    lab[r] = 0;
    if (r < R) {
      const long long v = (long long)((const T*)ptrs.p[r])[i];
      if (v < 0 || v >= L) {
        if (state) atomicMax(&state->bad, ~((u64)i << 4 | (u64)r));
        ok = false;
      } else {
        lab[r] = (int)v;
      }
    }
  }
  return ok;
}

__device__ __forceinline__ bool staple_agreed(const int (&lab)[kStapleMaxRaters], int R) {
  bool same = true;
#pragma unroll
  for (int r = 1; r < kStapleMaxRaters; ++r)
    if (r < R) same &= lab[r] == lab[0];
  return same;
}

// p[s] = prior[s] * theta_0[D_0][s] * theta_1[D_1][s] * ... in this order, every product rounded
__device__ __forceinline__ double staple_product(const double* __restrict__ prior, const double* __restrict__ theta,
                                                 const int (&lab)[kStapleMaxRaters], int R, int L, int s) {
  double p = prior[s];
#pragma unroll
  for (int r = 0; r < kStapleMaxRaters; ++r)
    if (r < R) p = p * theta[((size_t)r * L + lab[r]) * L + s];
  return p;
}
__device__ __forceinline__ double staple_total(const double* __restrict__ prior, const double* __restrict__ theta,
                                               const int (&lab)[kStapleMaxRaters], int R, int L) {
  double tot = staple_product(prior, theta, lab, R, L, 0);
  for (int s = 1; s < L; ++s) tot = tot + staple_product(prior, theta, lab, R, L, s);
  return tot;
}
__device__ __forceinline__ long long staple_q(double p, double tot) {
  const double w = p / tot;
  return (long long)floor(w * kStapleQ + 0.5);
}

// S[r][D_r][s] += q for every rater: into the workgroup table, or straight into the global one
__device__ __forceinline__ void staple_add(u64* table, const int (&lab)[kStapleMaxRaters], int R, int L, int s, long long q) {
#pragma unroll
  for (int r = 0; r < kStapleMaxRaters; ++r)
    if (r < R) atomicAdd(&table[((size_t)r * L + lab[r]) * L + s], (u64)q);
}

template <bool LDS>
__device__ __forceinline__ u64* staple_table_begin(u64* lds, u64* global, int entries) {
  if (!LDS) return global;
  for (int e = threadIdx.x; e < entries; e += 256) lds[e] = 0;
  __syncthreads();
  return lds;
}
template <bool LDS>
__device__ __forceinline__ void staple_table_end(const u64* lds, u64* global, int entries) {
  if (!LDS) return;
  __syncthreads();
  for (int e = threadIdx.x; e < entries; e += 256)
    if (lds[e]) atomicAdd(&global[e], lds[e]);
}

// prior counts, agreed counts, and the M-step of the one-hot vote (ties: the smallest label) for disputed voxels
template <typename T, bool LDS>
__global__ __launch_bounds__(256) void staple_count_kernel(StaplePtrs ptrs, int R, int L, int64_t n, StapleWs ws) {
  __shared__ u64 s_tab[LDS ? kStapleLdsEntries : 1];
  __shared__ u64 s_cnt[kStapleMaxLabels], s_agree[kStapleMaxLabels];
  if (threadIdx.x < kStapleMaxLabels) s_cnt[threadIdx.x] = s_agree[threadIdx.x] = 0;
  u64* tab = staple_table_begin<LDS>(s_tab, ws.acc, R * L * L);
  __syncthreads();
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int lab[kStapleMaxRaters];
    if (!staple_load<T>(ptrs, R, L, i, lab, ws.state)) continue;
#pragma unroll
    for (int r = 0; r < kStapleMaxRaters; ++r)
      if (r < R) atomicAdd(&s_cnt[lab[r]], 1ull);
    if (staple_agreed(lab, R)) {
      atomicAdd(&s_agree[lab[0]], 1ull);
      continue;
    }
    int best = lab[0], bestc = 0;
#pragma unroll
    for (int a = 0; a < kStapleMaxRaters; ++a)
      if (a < R) {
        int c = 0;
#pragma unroll
        for (int b = 0; b < kStapleMaxRaters; ++b)
          if (b < R) c += lab[b] == lab[a];
        if (c > bestc || (c == bestc && lab[a] < best)) { best = lab[a]; bestc = c; }
      }
    staple_add(tab, lab, R, L, best, kStapleQi);
  }
  staple_table_end<LDS>(s_tab, ws.acc, R * L * L);
  __syncthreads();
  if (threadIdx.x < L) {
    if (s_cnt[threadIdx.x]) atomicAdd(&ws.cnt[threadIdx.x], s_cnt[threadIdx.x]);
    if (s_agree[threadIdx.x]) atomicAdd(&ws.agree[threadIdx.x], s_agree[threadIdx.x]);
  }
}

// one E-step + M-step over the disputed voxels
template <typename T, bool LDS>
__global__ __launch_bounds__(256) void staple_em_kernel(StaplePtrs ptrs, int R, int L, int64_t n, StapleWs ws) {
  __shared__ u64 s_tab[LDS ? kStapleLdsEntries : 1];
  if (ws.state->done) return;                       // uniform over the grid: the flag changes between launches only
  const double* theta = ws.theta + (size_t)ws.state->cur * R * L * L;
  u64* tab = staple_table_begin<LDS>(s_tab, ws.acc, R * L * L);
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int lab[kStapleMaxRaters];
    if (!staple_load<T>(ptrs, R, L, i, lab, nullptr)) continue;
    if (staple_agreed(lab, R)) continue;
    const double tot = staple_total(ws.prior, theta, lab, R, L);
    if (!(tot > 0.0)) continue;                     // q = 0: only a given prior of tiny size gets here
    for (int s = 0; s < L; ++s) {
      const long long q = staple_q(staple_product(ws.prior, theta, lab, R, L, s), tot);
      if (q) staple_add(tab, lab, R, L, s, q);
    }
  }
  staple_table_end<LDS>(s_tab, ws.acc, R * L * L);
}

// One workgroup of 1024.  start: prior and theta_0 from the one-hot vote.  Otherwise: the M-step of the pass just
// run (agreed voxels added as count[l] * q_cons[l][s]), theta, delta and the stop decision.  sums: S of this M-step.
__global__ __launch_bounds__(1024) void staple_table_kernel(int R, int L, int64_t n, int start, StaplePrior given,
                                                            int max_iterations, double tolerance, StapleWs ws,
                                                            long long* __restrict__ sums, double* __restrict__ prior_out) {
  __shared__ long long s_qcons[kStapleMaxLabels * kStapleMaxLabels];
  __shared__ long long s_t[kStapleMaxLabels];
  __shared__ double s_red[1024];
  StapleState* st = ws.state;
  if (st->done) return;
  const int t = threadIdx.x, entries = R * L * L;
  const int cur = st->cur;
  const double* theta_cur = ws.theta + (size_t)cur * entries;
  double* theta_new = ws.theta + (size_t)(start ? cur : 1 - cur) * entries;
  if (start) {
    if (t < L) {
      const double p = given.given ? given.v[t] : (double)ws.cnt[t] / (double)((long long)R * n);
      ws.prior[t] = p;
      prior_out[t] = p;
    }
    for (int e = t; e < L * L; e += 1024) s_qcons[e] = (e / L == e % L) ? kStapleQi : 0;
  } else {
    for (int e = t; e < L * L; e += 1024) s_qcons[e] = 0;
    __syncthreads();
    if (t < L && ws.agree[t]) {                     // the E-step of the tuple (t, t, ..., t)
      int lab[kStapleMaxRaters];
#pragma unroll
      for (int r = 0; r < kStapleMaxRaters; ++r) lab[r] = t;
      const double tot = staple_total(ws.prior, theta_cur, lab, R, L);
      if (tot > 0.0)
        for (int s = 0; s < L; ++s) s_qcons[t * L + s] = staple_q(staple_product(ws.prior, theta_cur, lab, R, L, s), tot);
    }
  }
  __syncthreads();
  for (int e = t; e < entries; e += 1024) {
    const int l = (e / L) % L, s = e % L;
    sums[e] = (long long)ws.acc[e] + (long long)ws.agree[l] * s_qcons[l * L + s];
    ws.acc[e] = 0;
  }
  __syncthreads();
  if (t < L) {
    long long sum = 0;
    for (int l = 0; l < L; ++l) sum += sums[l * L + t];
    s_t[t] = sum;
  }
  __syncthreads();
  double dmax = 0.0;
  for (int e = t; e < entries; e += 1024) {
    const long long ts = s_t[e % L];
    const double v = ts == 0 ? 0.0 : (double)sums[e] / (double)ts;
    if (!start) {
      const double d = fabs(v - theta_cur[e]);
      dmax = d > dmax ? d : dmax;
    }
    theta_new[e] = v;
  }
  if (start) {
    if (t == 0 && st->bad) st->done = 1;            // an input label outside the range: nothing more runs
    return;
  }
  s_red[t] = dmax;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (t < o) s_red[t] = s_red[t + o] > s_red[t] ? s_red[t + o] : s_red[t];
    __syncthreads();
  }
  if (t == 0) {
    const double delta = s_red[0];
    st->delta = delta;
    st->it += 1;
    st->cur = 1 - cur;
    if (delta < tolerance) { st->converged = 1; st->done = 1; }
    else if (st->it == max_iterations) st->done = 1;
  }
}

// the last E-step again, with the theta it used: labels (first maximum) and the posterior q / Q
template <typename T>
__global__ __launch_bounds__(256) void staple_final_kernel(StaplePtrs ptrs, int R, int L, int64_t n, StapleWs ws,
                                                           T* __restrict__ out, float* __restrict__ posterior) {
  const double* theta = ws.theta + (size_t)(1 - ws.state->cur) * R * L * L;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int lab[kStapleMaxRaters];
    if (!staple_load<T>(ptrs, R, L, i, lab, nullptr)) continue;
    const double tot = staple_total(ws.prior, theta, lab, R, L);
    long long bestq = -1;
    int best = 0;
    for (int s = 0; s < L; ++s) {
      const long long q = tot > 0.0 ? staple_q(staple_product(ws.prior, theta, lab, R, L, s), tot) : 0;
      if (q > bestq) { bestq = q; best = s; }
      if (posterior) posterior[(size_t)s * n + i] = (float)q * (1.0f / 16777216.0f);
    }
    out[i] = (T)best;
  }
}

static bool staple_shape_ok(int raters, int num_classes, int64_t n) {
  return raters >= 1 && raters <= kStapleMaxRaters && num_classes >= 2 && num_classes <= kStapleMaxLabels && n > 0 &&
         n < (1ll << 31);
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int64_t segmi_staple_workspace_bytes(int raters, int num_classes) {
  if (!staple_shape_ok(raters, num_classes, 1)) return 0;
  return (int64_t)staple_layout(raters, num_classes).total;
}

const char* segmi_staple_table_name(int raters, int num_classes) {
  if (!staple_shape_ok(raters, num_classes, 1)) return "";
  return staple_lds_table(raters, num_classes) ? "lds" : "global";
}

int segmi_staple(const void* const* labels_host, int raters, int label_bytes, int64_t n, int num_classes,
                 const double* prior_host, int max_iterations, double tolerance, void* out, int64_t* sums,
                 double* prior, float* posterior, int32_t* info_host, void* ws, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(labels_host && out && sums && prior && info_host && ws, "staple: null pointer");
  LV_CHECK_LABEL_BYTES("staple", label_bytes);
  SEGMI_CHECK_ARG(staple_shape_ok(raters, num_classes, n), "staple: 1 .. %d raters, 2 .. %d classes, 0 < n < 2^31",
                  kStapleMaxRaters, kStapleMaxLabels);
  SEGMI_CHECK_ARG(max_iterations >= 1, "staple: max_iterations must be >= 1");
  SEGMI_CHECK_ARG(tolerance >= 0.0 && tolerance < __builtin_inf(), "staple: tolerance must be finite and >= 0");
  const StapleLayout lay = staple_layout(raters, num_classes);
  SEGMI_CHECK_ARG(ws_bytes >= lay.total, "staple: workspace of %zu bytes, %zu needed", ws_bytes, lay.total);
  StaplePtrs ptrs{};
  for (int r = 0; r < raters; ++r) {
    SEGMI_CHECK_ARG(labels_host[r], "staple: null label volume");
    ptrs.p[r] = labels_host[r];
  }
  StaplePrior given{};
  if (prior_host) {
    given.given = 1;
    for (int s = 0; s < num_classes; ++s) {
      SEGMI_CHECK_ARG(prior_host[s] > 0.0 && prior_host[s] < __builtin_inf(), "staple: prior must be positive and finite");
      given.v[s] = prior_host[s];
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const StapleWs w = staple_carve(ws, lay);
  const int R = raters, L = num_classes;
  const bool lds = staple_lds_table(R, L);
  const int grid = lv_grid(n, 256, kStapleGridCap);
  info_host[0] = info_host[1] = 0;
  info_host[2] = -1;
  info_host[3] = 0;
  if (hipMemsetAsync(ws, 0, lay.zeroed, st) != hipSuccess) {
    set_error("staple: memset failed");
    return SEGMI_ELAUNCH;
  }
#define COUNT(T)                                                                                          \
  do {                                                                                                    \
    if (lds) hipLaunchKernelGGL((staple_count_kernel<T, true>), grid, 256, 0, st, ptrs, R, L, n, w);      \
    else hipLaunchKernelGGL((staple_count_kernel<T, false>), grid, 256, 0, st, ptrs, R, L, n, w);         \
  } while (0)
  LV_BY_LABEL(label_bytes, COUNT);
#undef COUNT
  hipLaunchKernelGGL(staple_table_kernel, 1, 1024, 0, st, R, L, n, 1, given, max_iterations, tolerance, w,
                     (long long*)sums, prior);
  SEGMI_LAUNCH_CHECK("staple");
  StapleState host{};
  for (int first = 0; first < max_iterations && !host.done; first += kStapleChunk) {
    const int last = first + kStapleChunk < max_iterations ? first + kStapleChunk : max_iterations;
    for (int it = first; it < last; ++it) {
#define EM(T)                                                                                             \
  do {                                                                                                    \
    if (lds) hipLaunchKernelGGL((staple_em_kernel<T, true>), grid, 256, 0, st, ptrs, R, L, n, w);         \
    else hipLaunchKernelGGL((staple_em_kernel<T, false>), grid, 256, 0, st, ptrs, R, L, n, w);            \
  } while (0)
      LV_BY_LABEL(label_bytes, EM);
#undef EM
      hipLaunchKernelGGL(staple_table_kernel, 1, 1024, 0, st, R, L, n, 0, given, max_iterations, tolerance, w,
                         (long long*)sums, prior);
    }
    SEGMI_LAUNCH_CHECK("staple");
    if (hipMemcpyAsync(&host, w.state, sizeof(host), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      set_error("staple: reading the state back failed");
      return SEGMI_ELAUNCH;
    }
  }
  if (host.bad) {                                   // report the rater and the value; nothing was written to out
    const int r = (int)(~host.bad & 15);
    const int64_t i = (int64_t)(~host.bad >> 4);
    int32_t v4 = 0;
    int16_t v2 = 0;
    uint8_t v1 = 0;
    void* dst = label_bytes == 4 ? (void*)&v4 : label_bytes == 2 ? (void*)&v2 : (void*)&v1;
    if (hipMemcpyAsync(dst, (const char*)labels_host[r] + (size_t)i * label_bytes, label_bytes, hipMemcpyDeviceToHost,
                       st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      set_error("staple: reading the offending label back failed");
      return SEGMI_ELAUNCH;
    }
    info_host[2] = r;
    info_host[3] = label_bytes == 4 ? v4 : label_bytes == 2 ? (int32_t)v2 : (int32_t)v1;
    return SEGMI_OK;
  }
  info_host[0] = host.it;
  info_host[1] = host.converged;
#define FINAL(T) hipLaunchKernelGGL(staple_final_kernel<T>, grid, 256, 0, st, ptrs, R, L, n, w, (T*)out, posterior)
  LV_BY_LABEL(label_bytes, FINAL);
#undef FINAL
  SEGMI_LAUNCH_CHECK("staple");
  return SEGMI_OK;
}

}  // extern "C"
