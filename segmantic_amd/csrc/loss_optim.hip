// loss_optim.hip -- fused softmax + one-hot + Dice loss (forward / backward), its Dice + cross-entropy
// extension (LossMode kDiceCE: same passes, one more partial / coefficient row), the Tversky and Dice + focal
// losses on the same passes (kTversky, kFocal: DESIGN.md section 21), and the
// flat-arena optimisers (Adam, SGD, AdaBelief).  HBM-bound: logits are read once per pass in
// 16-byte vectors along the class axis (NDHWC keeps the K classes of a voxel contiguous), the
// softmax lives in registers, reductions are two-stage and deterministic.
#include "common.h"
#include "fin_tail.h"
#include <type_traits>

namespace segmi {

constexpr int kDiceVox = 8192;  // voxels per workgroup


// one block: per (n,k) sums of the collapsed rows (f64), loss + backward coefficients
struct DiceFin {
  int n, k;
  float smooth_nr, smooth_dr;
  float *coef, *loss;
  // sums: [n][3][k] = {intersection, sum p, sum t}
  __device__ void operator()(const double* sums, double* red) const {
    const int tid = threadIdx.x;
    double local = 0.0;
    const double nk = (double)n * k;
    for (int o = tid; o < n * k; o += 256) {
      const int b = o / k, j = o % k;
      const double* q = sums + ((int64_t)b * 3) * k + j;
      const double I = q[0], P = q[k], Tt = q[2 * k];
      // f32 arithmetic as the reference does on the reduced sums
      const float If = (float)I, Df = (float)Tt + (float)P;
      const float f = 1.0f - (2.0f * If + smooth_nr) / (Df + smooth_dr);
      local += (double)f;
      const double den = (double)Df + (double)smooth_dr;
      coef[((int64_t)b * 2 + 0) * k + j] = (float)(-2.0 / den / nk);
      coef[((int64_t)b * 2 + 1) * k + j] = (float)((2.0 * (double)If + (double)smooth_nr) / (den * den) / nk);
    }
    red[tid] = local;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) *loss = (float)(red[0] / nk);
  }
};

// Dice + cross-entropy: loss = lambda_dice * Dice + lambda_ce * CE.
//   Dice: the term above; without the background class 0 is dropped and the mean runs over n * (k - 1).
//   CE:   sum_v w[y_v] * (-log p_{v,y_v}) / W,  W = sum_v w[y_v] over the whole batch (torch's weighted mean);
//         voxels whose label is outside [0, k) are in neither sum (they are in no row of the table).
// sums: [n][4][k] = {intersection, sum p, sum t, sum of -log p_y over the voxels with y = k}
// coef: [n][3][k] = {lambda_dice * Dice pair (0 for an excluded background), c_k = lambda_ce * w_k / W}
struct DiceCEFin {
  int n, k;
  float smooth_nr, smooth_dr;
  float lambda_dice, lambda_ce;
  int include_background;
  const float* weight;   // nullable: ones
  float *coef, *loss;
  __device__ void operator()(const double* sums, double* red) const {
    const int tid = threadIdx.x;
    double local = 0.0, num = 0.0, wsum = 0.0;
    const int k0 = include_background ? 0 : 1;
    const double nk = (double)n * (k - k0);
    const double ld = (double)lambda_dice;
    for (int o = tid; o < n * k; o += 256) {
      const int b = o / k, j = o % k;
      const double* q = sums + ((int64_t)b * 4) * k + j;
      const double I = q[0], P = q[k], Tt = q[2 * k];
      const double w = weight ? (double)weight[j] : 1.0;
      num += w * q[3 * k];
      wsum += w * Tt;
      float* c = coef + ((int64_t)b * 3) * k + j;
      if (j < k0) {
        c[0] = 0.f;
        c[k] = 0.f;
        continue;
      }
      // f32 arithmetic as the reference does on the reduced sums
      const float If = (float)I, Df = (float)Tt + (float)P;
      const float f = 1.0f - (2.0f * If + smooth_nr) / (Df + smooth_dr);
      local += (double)f;
      const double den = (double)Df + (double)smooth_dr;
      c[0] = (float)(ld * (-2.0 / den / nk));
      c[k] = (float)(ld * ((2.0 * (double)If + (double)smooth_nr) / (den * den) / nk));
    }
    red[tid] = local;
    red[256 + tid] = num;
    red[512 + tid] = wsum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) {
        red[tid] += red[tid + o];
        red[256 + tid] += red[256 + tid + o];
        red[512 + tid] += red[512 + tid + o];
      }
      __syncthreads();
    }
    // lambda_ce = 0 switches the term off altogether: a batch without any weighted voxel (W = 0, CE = NaN
    // by torch's rule) must not turn a pure Dice loss into NaN
    const bool ce_on = lambda_ce != 0.f;
    const double W = red[512];
    for (int o = tid; o < n * k; o += 256) {
      const int j = o % k;
      const double w = weight ? (double)weight[j] : 1.0;
      coef[((int64_t)(o / k) * 3 + 2) * k + j] = ce_on ? (float)((double)lambda_ce * w / W) : 0.f;
    }
    if (tid == 0) {
      double total = ld * (red[0] / nk);
      if (ce_on) total += (double)lambda_ce * (red[256] / W);
      *loss = (float)total;
    }
  }
};

// Tversky / focal Tversky: per (n, k), all in f64 on the reduced sums,
//   TI = (I + smooth_nr) / (I + alpha (P - I) + beta (T - I) + smooth_dr),  loss = mean of (1 - TI)^exponent
// over the included (n, k); where 1 - TI <= 0 the term and its coefficients are 0.
// sums: [n][3][k] as DiceFin; coef: [n][2][k] = {d loss / d I, d loss / d P} (0 for an excluded background), the
// pair dice_bwd_kernel applies: d loss / d p_{v,k} = coef[0][k] [y_v = k] + coef[1][k]
struct TverskyFin {
  int n, k;
  float smooth_nr, smooth_dr;
  float alpha, beta, exponent;
  int include_background;
  float *coef, *loss;
  __device__ void operator()(const double* sums, double* red) const {
    const int tid = threadIdx.x;
    double local = 0.0;
    const int k0 = include_background ? 0 : 1;
    const double nk = (double)n * (k - k0);
    const double a = (double)alpha, bt = (double)beta, e = (double)exponent;
    for (int o = tid; o < n * k; o += 256) {
      const int b = o / k, j = o % k;
      const double* q = sums + ((int64_t)b * 3) * k + j;
      const double I = q[0], P = q[k], Tt = q[2 * k];
      float* c = coef + ((int64_t)b * 2) * k + j;
      double cI = 0.0, cP = 0.0;
      if (j >= k0) {
        const double num = I + (double)smooth_nr;
        const double den = I + a * (P - I) + bt * (Tt - I) + (double)smooth_dr;
        const double u = 1.0 - num / den;
        if (u > 0.0) {
          // d (u^e) / d TI = -e u^(e - 1);  d TI / d I = (den - num (1 - alpha - beta)) / den^2,  d TI / d P = -alpha num / den^2
          const double dt = exponent == 1.f ? -1.0 : -e * pow(u, e - 1.0);
          local += exponent == 1.f ? u : pow(u, e);
          cI = dt * (den - num * (1.0 - a - bt)) / (den * den) / nk;
          cP = dt * (-a * num) / (den * den) / nk;
        }
      }
      c[0] = (float)cI;
      c[k] = (float)cP;
    }
    red[tid] = local;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) *loss = (float)(red[0] / nk);
  }
};

struct ChanSumFin {   // sums: [k] channel sums
  int k;
  float* db;
  __device__ void operator()(const double* sums, double*) const {
    for (int ch = threadIdx.x; ch < k; ch += 256) db[ch] = (float)sums[ch];
  }
};

struct DiceParams {
  const void* logits;
  const float* labels;
  float* partials;   // [chunks][n][3][k]; Dice + CE: [chunks][n][4][k]
  const float* coef; // [n][2][k]; Dice + CE: [n][3][k]
  void* dlogits;
  int n, k, ld, ldd;
  int64_t vox;       // voxels per batch item
  int chunks;
  float grad_scale;
  const float* amp;  // nullable: {scale, found_inf} in device memory; scale replaces grad_scale
  float* bias_part;  // [n * chunks][k] per-workgroup channel sums of the written gradient (nullable)
  // finalisation by the last workgroup of the launch (fin_tail.h): forward -> DiceFin (Dice + CE: DiceCEFin)
  // over `partials`, backward -> ChanSumFin over `bias_part`
  FinTail ft;
  DiceFin dfin;
  ChanSumFin cfin;
  DiceCEFin cefin;
  float gamma;       // kFocal: the focusing exponent, in [1, 5] (0 runs the kDiceCE kernels)
  TverskyFin tfin;
};

// which loss a kernel instantiation computes.  kDice and kDiceCE are the kernels as they were before the other two
// existed: everything the later modes add sits behind `if constexpr`
enum LossMode : int {
  kDice = 0,     // 3 partial rows, DiceFin, 2 coefficient rows
  kDiceCE = 1,   // + a fourth partial row (sum of -log p_y) and DiceCEFin, 3 coefficient rows
  kTversky = 2,  // the kDice forward with TverskyFin; its backward IS the kDice backward
  kFocal = 3,    // kDiceCE with q^gamma * -log p_y in the fourth row and the focal factor on the backward's c_y
};

// VECLD: the caller has checked ONCE per workgroup (logits_vec_ok) that every voxel's class row is
// 16-byte aligned -- a per-voxel alignment test is a divergent branch around every load and keeps the
// loads of an unrolled trip from being issued together
template <typename T>
__device__ __forceinline__ bool logits_vec_ok(const T* base, int k, int ld) {
  constexpr int VEC = 16 / sizeof(T);
  return k % VEC == 0 && ld % VEC == 0 && ((uintptr_t)base % 16) == 0;
}
template <typename T, int KMAX, bool VECLD>
__device__ __forceinline__ void load_logits(const T* p, int k, float (&v)[KMAX]) {
  constexpr int VEC = 16 / sizeof(T);
  if constexpr (VECLD) {
#pragma unroll
    for (int j = 0; j < KMAX; j += VEC) {
      if (j < k) {
        const frag_t f = *reinterpret_cast<const frag_t*>(p + j);
        if constexpr (sizeof(T) == 4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (j + e < KMAX) v[j + e] = __uint_as_float(f[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (j + 2 * e < KMAX) v[j + 2 * e] = H16<T>::lo(f[e]);
            if (j + 2 * e + 1 < KMAX) v[j + 2 * e + 1] = H16<T>::hi(f[e]);
          }
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) if (j < k) v[j] = Elem<T>::ld(p + j);
  }
}

// FAST: hardware exp2 (v_exp_f32, ~1 ulp in exp2 but ~2e-7 relative after the log2(e) scaling)
// for the bf16 path, where the logits carry 8 bits anyway; the f32 parity path keeps the
// correctly-rounded libm expf.
template <int KMAX, bool FAST>
__device__ __forceinline__ void softmax_inplace(int k, float (&v)[KMAX]) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) if (j < k) m = fmaxf(m, v[j]);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) if (j < k) {
    v[j] = FAST ? __builtin_amdgcn_exp2f((v[j] - m) * 1.4426950408889634f) : expf(v[j] - m);
    s += v[j];
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) if (j < k) v[j] *= inv;
}

// softmax_inplace (the same operations in the same order: the probabilities keep their bits) that also returns
// -log p_lab = log sum_j exp(x_j - m) - (x_lab - m), from the sum and the shifted logit and never from the stored
// probability: a true class 200 below the maximum gives 200, not -log(0).  The sum lies in [1, k], so the hardware
// log2 (v_log_f32) of the 16-bit path needs no denormal care; f32 keeps libm logf like its expf.  A label
// outside [0, k) returns a value no caller uses.
template <int KMAX, bool FAST>
__device__ __forceinline__ float softmax_nll_inplace(int k, float (&v)[KMAX], int lab) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) if (j < k) m = fmaxf(m, v[j]);
  float s = 0.f, xl = 0.f;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) if (j < k) {
    if (j == lab) xl = v[j] - m;
    v[j] = FAST ? __builtin_amdgcn_exp2f((v[j] - m) * 1.4426950408889634f) : expf(v[j] - m);
    s += v[j];
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) if (j < k) v[j] *= inv;
  return (FAST ? __builtin_amdgcn_logf(s) * 0.6931471805599453f : logf(s)) - xl;
}

// x^g for x >= 0 and g > 0 (0 at x = 0): libm powf for f32; the 16-bit paths use v_log_f32 / v_exp_f32 like the rest
// of their softmax (log2(0) = -inf, g * -inf = -inf, exp2(-inf) = 0)
template <bool FAST>
__device__ __forceinline__ float pow_pos(float x, float g) {
  return FAST ? __builtin_amdgcn_exp2f(g * __builtin_amdgcn_logf(x)) : powf(x, g);
}

// q^gamma with q = 1 - p_lab formed as the sum of the other probabilities (1 - p cancels when the voxel is classified
// well; q = 0 gives 0).  A label outside [0, k) returns a value no caller uses.
template <int KMAX, bool FULL, bool FAST>
__device__ __forceinline__ float focal_q_pow(int k, const float (&pr)[KMAX], int lab, float gamma) {
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
    if ((FULL || j < k) && j != lab) q += pr[j];
  return pow_pos<FAST>(q, gamma);
}

// FULL: k == KMAX (16 / 32 / 64 labels): every per-channel predicate folds away at compile time
// CE: Dice + cross-entropy -- a fourth partial row (sum of -log p_y over the voxels with y = k) and DiceCEFin;
// CE = false is the Dice-only kernel, unchanged
// kFocal: the fourth row receives q^gamma * -log p_y, q = the sum of the other probabilities (as the backward's `rest`)
template <typename T, int KMAX, bool FULL, int MODE>
__global__ __launch_bounds__(256) void dice_fwd_kernel(DiceParams p) {
  constexpr bool CE = MODE == kDiceCE || MODE == kFocal;
  constexpr bool FOCAL = MODE == kFocal;
  constexpr int ROWS = CE ? 4 : 3;
  __shared__ float red[4][ROWS * KMAX];
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t v0 = (int64_t)chunk * kDiceVox;
  const int64_t v1 = v0 + kDiceVox < p.vox ? v0 + kDiceVox : p.vox;
  const T* lg = (const T*)p.logits + (int64_t)n * p.vox * p.ld;
  const float* lb = p.labels + (int64_t)n * p.vox;
  float si[KMAX], sp[KMAX], stt[KMAX];
  float snl[CE ? KMAX : 1];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) si[j] = sp[j] = stt[j] = 0.f;
  if constexpr (CE) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) snl[j] = 0.f;
  }
  // U voxels per trip with every load issued before the first softmax (one voxel per trip behind a
  // per-voxel alignment branch left the 32-byte loads exposed: 3.4 TB/s); the sums keep their voxel
  // order, so the partials keep their bits
  auto sweep = [&](auto vec_tag) {
    constexpr bool VL = decltype(vec_tag)::value;
    constexpr int U = KMAX <= 16 ? 4 : (KMAX <= 32 ? 2 : 1);
    int64_t v = v0 + tid;
    for (; v + 256 * (U - 1) < v1; v += 256 * U) {
      float x[U][KMAX], lf[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        load_logits<T, KMAX, VL>(lg + (v + 256 * u) * p.ld, FULL ? KMAX : p.k, x[u]);
        lf[u] = __builtin_nontemporal_load(lb + v + 256 * u);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int lab = (int)lf[u];
        float nll = 0.f;
        if constexpr (CE) nll = softmax_nll_inplace<KMAX, sizeof(T) == 2>(FULL ? KMAX : p.k, x[u], lab);
        else softmax_inplace<KMAX, sizeof(T) == 2>(FULL ? KMAX : p.k, x[u]);
        if constexpr (FOCAL) nll *= focal_q_pow<KMAX, FULL, sizeof(T) == 2>(p.k, x[u], lab, p.gamma);
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
          if (FULL || j < p.k) {
            sp[j] += x[u][j];
            if (j == lab) {
              si[j] += x[u][j];
              stt[j] += 1.f;
              if constexpr (CE) snl[j] += nll;
            }
          }
        }
      }
    }
    for (; v < v1; v += 256) {
      float x[KMAX];
      load_logits<T, KMAX, VL>(lg + v * p.ld, FULL ? KMAX : p.k, x);
      const int lab = (int)lb[v];
      float nll = 0.f;
      if constexpr (CE) nll = softmax_nll_inplace<KMAX, sizeof(T) == 2>(FULL ? KMAX : p.k, x, lab);
      else softmax_inplace<KMAX, sizeof(T) == 2>(FULL ? KMAX : p.k, x);
      if constexpr (FOCAL) nll *= focal_q_pow<KMAX, FULL, sizeof(T) == 2>(p.k, x, lab, p.gamma);
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        if (FULL || j < p.k) {
          sp[j] += x[j];
          if (j == lab) {
            si[j] += x[j];
            stt[j] += 1.f;
            if constexpr (CE) snl[j] += nll;
          }
        }
      }
    }
  };
  if (logits_vec_ok<T>(lg, p.k, p.ld)) sweep(std::true_type{});
  else sweep(std::false_type{});
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (FULL || j < p.k) {
      const float a = wave_sum(si[j]), b = wave_sum(sp[j]), c = wave_sum(stt[j]);
      if (lane == 0) { red[wave][j] = a; red[wave][KMAX + j] = b; red[wave][2 * KMAX + j] = c; }
      if constexpr (CE) {
        const float d = wave_sum(snl[j]);
        if (lane == 0) red[wave][3 * KMAX + j] = d;
      }
    }
  }
  __syncthreads();
  if (tid < ROWS * p.k) {
    const int which = tid / p.k, j = tid % p.k;
    const float s = red[0][which * KMAX + j] + red[1][which * KMAX + j] +
                    red[2][which * KMAX + j] + red[3][which * KMAX + j];
    fin_store(&p.partials[(((int64_t)chunk * p.n + n) * ROWS + which) * p.k + j], s);   // [chunk][n][ROWS][k]
  }
  {
    extern __shared__ double dice_tail_lds[];
    if constexpr (CE)
      fin_tail_run<DiceCEFin, 256, offsetof(DiceParams, ft), offsetof(DiceParams, cefin)>(p.partials, dice_tail_lds);
    else if constexpr (MODE == kTversky)
      fin_tail_run<TverskyFin, 256, offsetof(DiceParams, ft), offsetof(DiceParams, tfin)>(p.partials, dice_tail_lds);
    else
      fin_tail_run<DiceFin, 256, offsetof(DiceParams, ft), offsetof(DiceParams, dfin)>(p.partials, dice_tail_lds);
  }
}

// CE: the third coefficient row c_k = lambda_ce * w_k / W adds c_y * (p_j - [j = y]) per class.  For j = y the
// bracket is formed as -(sum of the other probabilities): p_y - 1 cancels when the voxel is classified well.
// kFocal: d Focal_v / d x_j = g_v * c_y * (p_j - [j = y]) with g_v = q^gamma + gamma q^(gamma - 1) nll p_y: the CE term
// with cy multiplied by g_v; nll is recomputed as the forward formed it (softmax_nll_inplace keeps the probabilities' bits)
template <typename T, int KMAX, bool FULL, int MODE>
__global__ __launch_bounds__(256) void dice_bwd_kernel(DiceParams p) {
  static_assert(MODE != kTversky, "the Tversky backward is the kDice kernel");
  constexpr bool CE = MODE == kDiceCE || MODE == kFocal;
  constexpr bool FOCAL = MODE == kFocal;
  constexpr int ROWS = CE ? 3 : 2;
  __shared__ float cf[ROWS * KMAX];
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < ROWS * p.k) cf[(tid / p.k) * KMAX + tid % p.k] = p.coef[(int64_t)n * ROWS * p.k + tid];
  __syncthreads();
  const int64_t v0 = (int64_t)chunk * kDiceVox;
  const int64_t v1 = v0 + kDiceVox < p.vox ? v0 + kDiceVox : p.vox;
  const T* lg = (const T*)p.logits + (int64_t)n * p.vox * p.ld;
  T* dl = (T*)p.dlogits + (int64_t)n * p.vox * p.ldd;
  const float* lb = p.labels + (int64_t)n * p.vox;
  float gsum[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) gsum[j] = 0.f;
  const bool vec_in = logits_vec_ok<T>(lg, p.k, p.ld);
  const bool vec_out = (FULL || p.k % 4 == 0) && p.ldd % 4 == 0 && ((uintptr_t)dl % (4 * sizeof(T))) == 0;
  const float grad_scale = p.amp ? p.amp[0] : p.grad_scale;
  for (int64_t v = v0 + tid; v < v1; v += 256) {
    float x[KMAX];
    if (vec_in) load_logits<T, KMAX, true>(lg + v * p.ld, FULL ? KMAX : p.k, x);
    else load_logits<T, KMAX, false>(lg + v * p.ld, FULL ? KMAX : p.k, x);
    float nll = 0.f;
    if constexpr (FOCAL) nll = softmax_nll_inplace<KMAX, sizeof(T) == 2>(FULL ? KMAX : p.k, x, (int)lb[v]);
    else softmax_inplace<KMAX, sizeof(T) == 2>(FULL ? KMAX : p.k, x);
    const int lab = (int)lb[v];
    float fg = 0.f, fq = 0.f;        // kFocal: g_v and q_v, formed here so that only two scalars live through the Dice part
    if constexpr (FOCAL) {
      float py = 0.f, q = 0.f;       // q: the sum the CE term calls `rest`
#pragma unroll
      for (int j = 0; j < KMAX; ++j)
        if (FULL || j < p.k) {
          if (j == lab) py = x[j];
          else q += x[j];
        }
      // q^(gamma - 1) is 1 for gamma = 1 whatever q is (0 * log2(0) would be NaN)
      const float qg1 = p.gamma == 1.f ? 1.f : pow_pos<sizeof(T) == 2>(q, p.gamma - 1.f);
      fg = fmaf(p.gamma * qg1, nll * py, qg1 * q);
      fq = q;
      // keep the scheduler from spreading this block over the Dice part: the ragged 64-class instantiations sit at
      // the register limit, and fp16 spilled without it
      __builtin_amdgcn_sched_barrier(0);
    }
    float dot = 0.f;
    float dp[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (FULL || j < p.k) {
        dp[j] = cf[KMAX + j] + (j == lab ? cf[j] : 0.f);
        dot = fmaf(x[j], dp[j], dot);
      }
    }
    float cy = 0.f, rest = 0.f;    // CE term: cy * (p_j - [j = y]), cy = grad_scale * c_y (0 for a label outside [0, k))
    if constexpr (CE) {
      const bool in = (unsigned)lab < (unsigned)(FULL ? KMAX : p.k);
      cy = in ? grad_scale * cf[2 * KMAX + (in ? lab : 0)] : 0.f;
      if constexpr (FOCAL) {
        rest = fq;
        cy *= fg;
      } else {
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
          if ((FULL || j < p.k) && j != lab) rest += x[j];
      }
    }
    T* o = dl + v * p.ldd;
    if (vec_out) {
#pragma unroll
      for (int j = 0; j < KMAX; j += 4) {
        if (FULL || j < p.k) {
          f32x4 g4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            g4[e] = (j + e < KMAX) ? grad_scale * x[j + e] * (dp[j + e] - dot) : 0.f;
            if constexpr (CE) if (j + e < KMAX) g4[e] += cy * (j + e == lab ? -rest : x[j + e]);
          }
          store4<T>(o + j, g4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j + e < KMAX) gsum[j + e] += g4[e];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < KMAX; ++j)
        if (FULL || j < p.k) {
          float gv = grad_scale * x[j] * (dp[j] - dot);
          if constexpr (CE) gv += cy * (j == lab ? -rest : x[j]);
          Elem<T>::st(o + j, gv);
          gsum[j] += gv;
        }
    }
  }
  // bias gradient of the layer that produced the logits = channel sums of dlogits: folded here so
  // the 537 MB tensor is not read once more for it (fixed-order: wave butterfly, then 4 waves)
  if (p.bias_part) {
    __shared__ float bsum[4][KMAX];
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      const float s = wave_sum(gsum[j]);
      if (lane == 0) bsum[wave][j] = s;
    }
    __syncthreads();
    if (tid < p.k)
      fin_store(&p.bias_part[((int64_t)n * p.chunks + chunk) * p.k + tid],
                (bsum[0][tid] + bsum[1][tid]) + (bsum[2][tid] + bsum[3][tid]));
    {
      extern __shared__ double dice_tail_lds[];
      fin_tail_run<ChanSumFin, 256, offsetof(DiceParams, ft), offsetof(DiceParams, cfin)>(p.bias_part, dice_tail_lds);
    }
  }
}

// ---------------------------------------------------------------- optimisers
// one element of each update, shared by the plain kernels and the loss-scaled (_amp) ones
__device__ __forceinline__ void adam_elem(int64_t i, float* __restrict__ p, const float* __restrict__ g,
                                          float* __restrict__ m, float* __restrict__ v, float* __restrict__ vmax,
                                          float omb1, float beta2, float omb2, float eps, float wd,
                                          float step_size, float bc2_sqrt, float grad_scale) {
  float gi = g[i] * grad_scale;
  const float pi = p[i];
  if (wd != 0.f) gi = fmaf(wd, pi, gi);
  float mi = m[i];
  mi = mi + omb1 * (gi - mi);                   // exp_avg.lerp_(grad, 1 - beta1)
  float vi = v[i] * beta2;
  vi = fmaf(omb2 * gi, gi, vi);                 // mul_(beta2).addcmul_(g, g, 1 - beta2)
  m[i] = mi;
  v[i] = vi;
  float vv = vi;
  if (vmax) { vv = fmaxf(vmax[i], vi); vmax[i] = vv; }
  const float denom = sqrtf(vv) / bc2_sqrt + eps;
  p[i] = pi - step_size * (mi / denom);
}

__device__ __forceinline__ void sgd_elem(int64_t i, float* __restrict__ p, const float* __restrict__ g,
                                         float* __restrict__ buf, float lr, float momentum, float wd, int first,
                                         float grad_scale) {
  float gi = g[i] * grad_scale;
  const float pi = p[i];
  if (wd != 0.f) gi = fmaf(wd, pi, gi);
  if (momentum != 0.f) {
    const float b = first ? gi : fmaf(buf[i], momentum, gi);
    buf[i] = b;
    gi = b;
  }
  p[i] = pi - lr * gi;
}

__device__ __forceinline__ void adabelief_elem(int64_t i, float* __restrict__ p, const float* __restrict__ g,
                                               float* __restrict__ m, float* __restrict__ s, float decay,
                                               float beta1, float omb1, float beta2, float omb2, float eps,
                                               float wd, int decouple, float step_size, float bc2_sqrt,
                                               float grad_scale) {
  float gi = g[i] * grad_scale;
  float pi = p[i];
  if (wd != 0.f) {
    if (decouple) pi *= decay;             // p.mul_(1 - lr * weight_decay)
    else gi = fmaf(wd, pi, gi);
  }
  const float mi = fmaf(omb1, gi, m[i] * beta1);     // mul_(beta1).add_(g, alpha=1 - beta1)
  const float r = gi - mi;
  float si = fmaf(omb2 * r, r, s[i] * beta2);        // mul_(beta2).addcmul_(r, r, value=1 - beta2)
  si += eps;  // exp_avg_var.add_(eps) is in place in adabelief_pytorch
  m[i] = mi;
  s[i] = si;
  const float denom = sqrtf(si) / bc2_sqrt + eps;
  p[i] = pi - step_size * (mi / denom);
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            float* __restrict__ vmax, int64_t n, float omb1, float beta2,
                            float omb2, float eps, float wd, float step_size, float bc2_sqrt,
                            float grad_scale) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    adam_elem(i, p, g, m, v, vmax, omb1, beta2, omb2, eps, wd, step_size, bc2_sqrt, grad_scale);
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                           float* __restrict__ buf, int64_t n, float lr, float momentum,
                           float wd, int first, float grad_scale) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    sgd_elem(i, p, g, buf, lr, momentum, wd, first, grad_scale);
}

__global__ void adabelief_kernel(float* __restrict__ p, const float* __restrict__ g,
                                 float* __restrict__ m, float* __restrict__ s, int64_t n,
                                 float decay, float beta1, float omb1, float beta2,
                                 float omb2, float eps, float wd, int decouple,
                                 float step_size, float bc2_sqrt, float grad_scale) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    adabelief_elem(i, p, g, m, s, decay, beta1, omb1, beta2, omb2, eps, wd, decouple, step_size, bc2_sqrt,
                   grad_scale);
}

// ---------------------------------------------------------------- dynamic loss scaling
// amp = {scale, found_inf, skipped steps} in device memory (segmi.h).  The gated updates read found_inf and the optimiser's
// count of applied steps there: a step with a non-finite gradient leaves every parameter and moment untouched
// (torch's GradScaler skips optimizer.step()); otherwise the gradient is unscaled by 1/scale (formed in double and
// rounded to f32 once, as GradScaler's inv_scale) on top of grad_scale, and the bias corrections use step + 1.
__device__ __forceinline__ float amp_inv_scale(const float* amp) { return (float)(1.0 / (double)amp[0]); }

__global__ void adam_amp_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, float* __restrict__ vmax, int64_t n, double lr,
                                double beta1, double beta2, float eps, float wd, const float* __restrict__ amp,
                                const int64_t* __restrict__ step, float grad_scale) {
  if (amp[1] != 0.f) return;
  const double t = (double)(*step + 1);
  const float step_size = (float)(lr / (1.0 - pow(beta1, t)));
  const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, t));
  const float gs = grad_scale * amp_inv_scale(amp);
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    adam_elem(i, p, g, m, v, vmax, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, wd, step_size,
              bc2_sqrt, gs);
}

__global__ void sgd_amp_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                               int64_t n, float lr, float momentum, float wd, const float* __restrict__ amp,
                               const int64_t* __restrict__ step, float grad_scale) {
  if (amp[1] != 0.f) return;
  const int first = *step == 0;
  const float gs = grad_scale * amp_inv_scale(amp);
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    sgd_elem(i, p, g, buf, lr, momentum, wd, first, gs);
}

__global__ void adabelief_amp_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                     float* __restrict__ s, int64_t n, double lr, double beta1, double beta2,
                                     float eps, double wd, int decouple, const float* __restrict__ amp,
                                     const int64_t* __restrict__ step, float grad_scale) {
  if (amp[1] != 0.f) return;
  const double t = (double)(*step + 1);
  const float step_size = (float)(lr / (1.0 - pow(beta1, t)));
  const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, t));
  const float gs = grad_scale * amp_inv_scale(amp);
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    adabelief_elem(i, p, g, m, s, (float)(1.0 - lr * wd), (float)beta1, (float)(1.0 - beta1), (float)beta2,
                   (float)(1.0 - beta2), eps, (float)wd, decouple, step_size, bc2_sqrt, gs);
}

// found_inf |= any non-finite element of g (never cleared here: segmi_amp_update_scale clears it)
__global__ __launch_bounds__(256) void amp_check_kernel(const float* __restrict__ g, int64_t n, float* amp) {
  bool bad = false;
  const int64_t n4 = ((uintptr_t)g % 16) == 0 ? n / 4 : 0;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) bad |= (__float_as_uint(v[e]) & 0x7f800000u) == 0x7f800000u;
  }
  for (int64_t i = 4 * n4 + blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    bad |= (__float_as_uint(g[i]) & 0x7f800000u) == 0x7f800000u;
  if (__syncthreads_or(bad) && threadIdx.x == 0) amp[1] = 1.f;
}

// torch._amp_update_scale_ on {scale, found_inf} + growth tracker; a skipped step is counted in amp[2]; when the step
// was applied, the optimiser's step count advances; found_inf is cleared for the next step
__global__ void amp_update_kernel(float* amp, int32_t* tracker, int64_t* step, float growth, float backoff,
                                  int interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float scale = amp[0];
  if (amp[1] != 0.f) {
    amp[0] = scale * backoff;
    *tracker = 0;
    amp[2] += 1.f;
  } else {
    const int successful = *tracker + 1;
    if (successful >= interval) {
      const float grown = scale * growth;
      if (__builtin_isfinite(grown)) amp[0] = grown;
      *tracker = 0;
    } else {
      *tracker = successful;
    }
    if (step) *step += 1;
  }
  amp[1] = 0.f;
}

constexpr int kOptCap = 2048;   // workgroups of an optimiser step

template <typename T, int MODE>
static int dice_dispatch(bool fwd, const DiceParams& p, hipStream_t st) {
  constexpr int BMODE = MODE == kTversky ? (int)kDice : MODE;   // backward instantiation
  dim3 grid(p.chunks, p.n);
  const size_t lds = p.ft.on ? fin_tail_lds(p.ft.width, 256) : 0;
#define DICE_K(KM)                                                                       \
  do {                                                                                   \
    if (p.k == KM) {                                                                     \
      if (fwd) hipLaunchKernelGGL((dice_fwd_kernel<T, KM, true, MODE>), grid, 256, lds, st, p);  \
      else hipLaunchKernelGGL((dice_bwd_kernel<T, KM, true, BMODE>), grid, 256, lds, st, p);      \
    } else {                                                                             \
      if (fwd) hipLaunchKernelGGL((dice_fwd_kernel<T, KM, false, MODE>), grid, 256, lds, st, p); \
      else hipLaunchKernelGGL((dice_bwd_kernel<T, KM, false, BMODE>), grid, 256, lds, st, p);     \
    }                                                                                    \
  } while (0)
  if (p.k <= 4) DICE_K(4);
  else if (p.k <= 16) DICE_K(16);
  else if (p.k <= 32) DICE_K(32);
  else if (p.k <= 64) DICE_K(64);
  else SEGMI_UNSUPPORTED("softmax_dice: at most 64 classes (got %d)", p.k);
#undef DICE_K
  SEGMI_LAUNCH_CHECK("softmax_dice");
  return SEGMI_OK;
}
template <int MODE>
static int dice_dispatch_dt(int dtype, bool fwd, const DiceParams& p, hipStream_t st) {
#define DICE_T(T) return dice_dispatch<T, MODE>(fwd, p, st)
  SEGMI_BY_DTYPE(dtype, DICE_T);
#undef DICE_T
}

}  // namespace segmi

using namespace segmi;

static inline int dice_real_chunks(const segmi_act* logits) {
  return (int)cdiv64((int64_t)logits->d * logits->h * logits->w, kDiceVox);
}

// ---- the one path of the four losses (LossMode): shared checks, DiceParams, launch
// per LossMode: the partial rows its forward writes, and the rows its finalisation's LDS bound is computed from
// (kTversky writes 3 rows and is held to the 4-row bound, so that one batch / class bound holds for every
// configurable loss)
struct DiceModeRows { int partial, lds; };
static constexpr DiceModeRows kDiceModeRows[] = {{3, 3}, {4, 4}, {3, 4}, {4, 4}};

static bool focal_gamma_ok(float gamma) { return gamma == 0.f || (gamma >= 1.f && gamma <= 5.f); }

// the checks every entry point shares, the storage type first.  dlogits: the backward's (null in a forward);
// ptrs: the entry point's other mandatory pointers are all there
static int dice_check(const char* name, int dtype, const segmi_act* logits, const segmi_act* dlogits, bool ptrs) {
  SEGMI_CHECK_ARG(dtype_ok(dtype), "%s: bad dtype", name);
  SEGMI_CHECK_ARG(act_ok(logits) && ptrs, "%s: bad arguments", name);
  SEGMI_CHECK_ARG(!dlogits || (act_ok(dlogits) && logits->n == dlogits->n && logits->d == dlogits->d &&
                               logits->h == dlogits->h && logits->w == dlogits->w && logits->c == dlogits->c),
                  "%s: bad arguments", name);
  return SEGMI_OK;
}

static DiceParams dice_params(const segmi_act* logits, const float* labels) {
  DiceParams p{};
  p.logits = logits->data; p.labels = labels;
  p.n = logits->n; p.k = logits->c; p.ld = logits->ld;
  p.vox = (int64_t)logits->d * logits->h * logits->w;
  p.chunks = dice_real_chunks(logits);
  return p;
}

// kFocal with gamma = 0 IS Dice + cross-entropy and runs its kernels
static int dice_launch(int mode, float gamma, int dtype, bool fwd, const DiceParams& p, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (mode == kFocal && gamma == 0.f) mode = kDiceCE;
  switch (mode) {
    case kDice: return dice_dispatch_dt<kDice>(dtype, fwd, p, st);
    case kFocal: return dice_dispatch_dt<kFocal>(dtype, fwd, p, st);
    case kDiceCE: return dice_dispatch_dt<kDiceCE>(dtype, fwd, p, st);
    default: return dice_dispatch_dt<kTversky>(dtype, fwd, p, st);
  }
}

static void dice_set_fin(DiceParams& p, const DiceFin& f) { p.dfin = f; }
static void dice_set_fin(DiceParams& p, const DiceCEFin& f) { p.cefin = f; }
static void dice_set_fin(DiceParams& p, const TverskyFin& f) { p.tfin = f; }

// the forward of `mode` after the entry point's own checks: the loss and the backward coefficients are written by
// the last workgroup of the launch itself (fin_tail.h) -- rows = chunks, one row = [n][partial rows][k], folded in f64
// and handed to `fin`
template <class Fin>
static int dice_fwd(const char* name, int mode, int dtype, const segmi_act* logits, const float* labels,
                    float* partials, int include_background, float gamma, const Fin& fin, void* stream) {
  SEGMI_CHECK_ARG(include_background || logits->c > 1, "%s: include_background = 0 needs more than one class", name);
  DiceParams p = dice_params(logits, labels);
  p.partials = partials;
  p.gamma = gamma;
  // the finalising workgroup holds one row of doubles in LDS (fin_tail_lds): 64 KB per workgroup
  const DiceModeRows rows = kDiceModeRows[mode];
  const size_t lds = fin_tail_lds(p.n * rows.lds * p.k, 256);
  SEGMI_CHECK_ARG(lds <= 64 * 1024,
                  "%s: batch %d x %d classes needs %zu bytes of LDS for the finalisation, the limit is 65536 "
                  "(n * k <= %d)", name, p.n, p.k, lds, (int)((64 * 1024 / sizeof(double) - 4 * 256) / rows.lds));
  p.ft = fin_tail_make(p.chunks, p.n * rows.partial * p.k, (unsigned)p.chunks * (unsigned)p.n);
  dice_set_fin(p, fin);
  return dice_launch(mode, gamma, dtype, true, p, stream);
}

// amp: the _amp entry points' loss scale on the device (it replaces grad_scale), null in the others
static int dice_bwd(const char* name, int mode, int dtype, const segmi_act* logits, const float* labels,
                    const float* coef, float gamma, float grad_scale, const float* amp, const segmi_act* dlogits,
                    float* scratch, float* bias_grad, void* stream) {
  if (int rc = dice_check(name, dtype, logits, dlogits, labels && coef && dlogits)) return rc;
  SEGMI_CHECK_ARG(focal_gamma_ok(gamma), "%s: gamma must be 0 or lie in [1, 5] (got %g)", name, (double)gamma);
  SEGMI_CHECK_ARG(!bias_grad || scratch, "%s: bias_grad needs the scratch buffer", name);
  DiceParams p = dice_params(logits, labels);
  p.coef = coef; p.dlogits = dlogits->data; p.ldd = dlogits->ld;
  p.grad_scale = grad_scale;
  p.amp = amp;
  p.gamma = gamma;
  if (bias_grad) {   // channel sums of the written gradient, folded by the last workgroup of the launch
    p.bias_part = scratch;
    p.ft = fin_tail_make(p.n * p.chunks, p.k, (unsigned)p.chunks * (unsigned)p.n);
    p.cfin = ChanSumFin{p.k, bias_grad};
  }
  // the Tversky backward is the Dice backward on its coefficient pair
  return dice_launch(mode == kTversky ? (int)kDice : mode, gamma, dtype, false, p, stream);
}

// the _amp entry points: the scale comes from amp[0]
static int dice_bwd_amp(const char* name, int mode, int dtype, const segmi_act* logits, const float* labels,
                        const float* coef, float gamma, const float* amp, const segmi_act* dlogits, float* scratch,
                        float* bias_grad, void* stream) {
  SEGMI_CHECK_ARG(amp, "%s: amp state missing", name);
  return dice_bwd(name, mode, dtype, logits, labels, coef, gamma, 1.f, amp, dlogits, scratch, bias_grad, stream);
}

// ---- Dice + cross-entropy and Dice + focal: 4-row partials, 3-row coefficients, DiceCEFin.  kFocal: the fourth row
// holds the focal sums and `lambda2` (named `lambda2_name` in messages) is lambda_focal
static int dice_ce_fwd(const char* name, const char* lambda2_name, int mode, int dtype, const segmi_act* logits,
                       const float* labels, float* partials, float* coef, float* loss, float smooth_nr,
                       float smooth_dr, float lambda_dice, float lambda2, float gamma, int include_background,
                       const float* class_weight, void* stream) {
  if (int rc = dice_check(name, dtype, logits, nullptr, labels && partials && coef && loss)) return rc;
  SEGMI_CHECK_ARG(focal_gamma_ok(gamma), "%s: gamma must be 0 or lie in [1, 5] (got %g)", name, (double)gamma);
  SEGMI_CHECK_ARG(lambda_dice >= 0.f && lambda2 >= 0.f && __builtin_isfinite(lambda_dice) &&
                      __builtin_isfinite(lambda2),
                  "%s: lambda_dice / %s must be finite and >= 0 (got %g, %g)", name, lambda2_name,
                  (double)lambda_dice, (double)lambda2);
  return dice_fwd(name, mode, dtype, logits, labels, partials, include_background, gamma,
                  DiceCEFin{logits->n, logits->c, smooth_nr, smooth_dr, lambda_dice, lambda2, include_background != 0,
                            class_weight, coef, loss}, stream);
}

extern "C" {

// chunks the caller must allocate: the real ones + a tail of 2 * kFinScratchRows + 1 rows.  The tail held the f64
// stage-1 reduction of reduce_fin.h; since the FinTail hand-off nothing reads or writes it.  It stays in the count
// only so that the buffers existing callers size by it remain large enough.
int segmi_dice_chunks(const segmi_act* logits) {
  if (!logits) return 0;
  return dice_real_chunks(logits) + 2 * kFinScratchRows + 1;
}

// chunks of every other forward: the real ones
int segmi_dice_ce_chunks(const segmi_act* logits) {
  if (!logits) return 0;
  return dice_real_chunks(logits);
}

// ---- Dice: 3-row partials, 2-row coefficients
int segmi_softmax_dice_fwd(int dtype, const segmi_act* logits, const float* labels,
                           float* partials, float* coef, float* loss, float smooth_nr,
                           float smooth_dr, void* stream) {
  const char* name = "softmax_dice_fwd";
  if (int rc = dice_check(name, dtype, logits, nullptr, labels && partials && coef && loss)) return rc;
  return dice_fwd(name, kDice, dtype, logits, labels, partials, 1, 0.f,
                  DiceFin{logits->n, logits->c, smooth_nr, smooth_dr, coef, loss}, stream);
}

int segmi_softmax_dice_bwd(int dtype, const segmi_act* logits, const float* labels,
                           const float* coef, float grad_scale, const segmi_act* dlogits,
                           float* scratch, float* bias_grad, void* stream) {
  return dice_bwd("softmax_dice_bwd", kDice, dtype, logits, labels, coef, 0.f, grad_scale, nullptr, dlogits, scratch,
                  bias_grad, stream);
}

int segmi_softmax_dice_bwd_amp(int dtype, const segmi_act* logits, const float* labels,
                               const float* coef, const float* amp, const segmi_act* dlogits,
                               float* scratch, float* bias_grad, void* stream) {
  return dice_bwd_amp("softmax_dice_bwd_amp", kDice, dtype, logits, labels, coef, 0.f, amp, dlogits, scratch,
                      bias_grad, stream);
}

// ---- Dice + cross-entropy: 4-row partials, 3-row coefficients
int segmi_softmax_dice_ce_fwd(int dtype, const segmi_act* logits, const float* labels, float* partials,
                              float* coef, float* loss, float smooth_nr, float smooth_dr, float lambda_dice,
                              float lambda_ce, int include_background, const float* class_weight, void* stream) {
  return dice_ce_fwd("softmax_dice_ce_fwd", "lambda_ce", kDiceCE, dtype, logits, labels, partials, coef, loss,
                     smooth_nr, smooth_dr, lambda_dice, lambda_ce, 0.f, include_background, class_weight, stream);
}

int segmi_softmax_dice_ce_bwd(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                              float grad_scale, const segmi_act* dlogits, float* scratch, float* bias_grad,
                              void* stream) {
  return dice_bwd("softmax_dice_ce_bwd", kDiceCE, dtype, logits, labels, coef, 0.f, grad_scale, nullptr, dlogits,
                  scratch, bias_grad, stream);
}

int segmi_softmax_dice_ce_bwd_amp(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                                  const float* amp, const segmi_act* dlogits, float* scratch, float* bias_grad,
                                  void* stream) {
  return dice_bwd_amp("softmax_dice_ce_bwd_amp", kDiceCE, dtype, logits, labels, coef, 0.f, amp, dlogits, scratch,
                      bias_grad, stream);
}

// ---- Tversky: the Dice forward with TverskyFin; the backward is the Dice backward on its coefficient pair
int segmi_softmax_tversky_fwd(int dtype, const segmi_act* logits, const float* labels, float* partials, float* coef,
                              float* loss, float smooth_nr, float smooth_dr, float alpha, float beta, float exponent,
                              int include_background, void* stream) {
  const char* name = "softmax_tversky_fwd";
  if (int rc = dice_check(name, dtype, logits, nullptr, labels && partials && coef && loss)) return rc;
  SEGMI_CHECK_ARG(alpha >= 0.f && beta >= 0.f && __builtin_isfinite(alpha) && __builtin_isfinite(beta) &&
                      alpha + beta > 0.f,
                  "%s: alpha / beta must be finite and >= 0 with alpha + beta > 0 (got %g, %g)", name,
                  (double)alpha, (double)beta);
  SEGMI_CHECK_ARG(exponent > 0.f && exponent <= 3.f, "%s: exponent must lie in (0, 3] (got %g)", name,
                  (double)exponent);
  return dice_fwd(name, kTversky, dtype, logits, labels, partials, include_background, 0.f,
                  TverskyFin{logits->n, logits->c, smooth_nr, smooth_dr, alpha, beta, exponent,
                             include_background != 0, coef, loss}, stream);
}

int segmi_softmax_tversky_bwd(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                              float grad_scale, const segmi_act* dlogits, float* scratch, float* bias_grad,
                              void* stream) {
  return dice_bwd("softmax_tversky_bwd", kTversky, dtype, logits, labels, coef, 0.f, grad_scale, nullptr, dlogits,
                  scratch, bias_grad, stream);
}

int segmi_softmax_tversky_bwd_amp(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                                  const float* amp, const segmi_act* dlogits, float* scratch, float* bias_grad,
                                  void* stream) {
  return dice_bwd_amp("softmax_tversky_bwd_amp", kTversky, dtype, logits, labels, coef, 0.f, amp, dlogits, scratch,
                      bias_grad, stream);
}

// ---- Dice + focal: the Dice + cross-entropy passes with the focal factor
int segmi_softmax_dice_focal_fwd(int dtype, const segmi_act* logits, const float* labels, float* partials,
                                 float* coef, float* loss, float smooth_nr, float smooth_dr, float lambda_dice,
                                 float lambda_focal, float gamma, int include_background, const float* class_weight,
                                 void* stream) {
  return dice_ce_fwd("softmax_dice_focal_fwd", "lambda_focal", kFocal, dtype, logits, labels, partials, coef, loss,
                     smooth_nr, smooth_dr, lambda_dice, lambda_focal, gamma, include_background, class_weight, stream);
}

int segmi_softmax_dice_focal_bwd(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                                 float gamma, float grad_scale, const segmi_act* dlogits, float* scratch,
                                 float* bias_grad, void* stream) {
  return dice_bwd("softmax_dice_focal_bwd", kFocal, dtype, logits, labels, coef, gamma, grad_scale, nullptr, dlogits,
                  scratch, bias_grad, stream);
}

int segmi_softmax_dice_focal_bwd_amp(int dtype, const segmi_act* logits, const float* labels, const float* coef,
                                     float gamma, const float* amp, const segmi_act* dlogits, float* scratch,
                                     float* bias_grad, void* stream) {
  return dice_bwd_amp("softmax_dice_focal_bwd_amp", kFocal, dtype, logits, labels, coef, gamma, amp, dlogits,
                      scratch, bias_grad, stream);
}

int segmi_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    float* max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                    double eps, double weight_decay, int64_t step, float grad_scale,
                    void* stream) {
  SEGMI_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n > 0 && step > 0, "adam: bad arguments");
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const float step_size = (float)(lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  hipLaunchKernelGGL(adam_kernel, grid_1d(n, kOptCap), 256, 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, max_exp_avg_sq, n, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps, (float)weight_decay, step_size, bc2_sqrt,
                     grad_scale);
  SEGMI_LAUNCH_CHECK("adam");
  return SEGMI_OK;
}

int segmi_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, double lr,
                   double momentum, double weight_decay, int first_step, float grad_scale,
                   void* stream) {
  SEGMI_CHECK_ARG(param && grad && n > 0 && (momentum == 0.0 || momentum_buf), "sgd: bad arguments");
  hipLaunchKernelGGL(sgd_kernel, grid_1d(n, kOptCap), 256, 0, (hipStream_t)stream, param, grad,
                     momentum_buf, n, (float)lr, (float)momentum, (float)weight_decay, first_step,
                     grad_scale);
  SEGMI_LAUNCH_CHECK("sgd");
  return SEGMI_OK;
}

int segmi_adabelief_step(float* param, const float* grad, float* exp_avg, float* exp_avg_var,
                         int64_t n, double lr, double beta1, double beta2, double eps,
                         double weight_decay, int weight_decouple, int64_t step,
                         float grad_scale, void* stream) {
  SEGMI_CHECK_ARG(param && grad && exp_avg && exp_avg_var && n > 0 && step > 0, "adabelief: bad arguments");
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  hipLaunchKernelGGL(adabelief_kernel, grid_1d(n, kOptCap), 256, 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_var, n, (float)(1.0 - lr * weight_decay), (float)beta1,
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                     (float)weight_decay, weight_decouple, (float)(lr / bc1), (float)sqrt(bc2),
                     grad_scale);
  SEGMI_LAUNCH_CHECK("adabelief");
  return SEGMI_OK;
}

int segmi_amp_check_finite(const float* grad, int64_t n, float* amp, void* stream) {
  SEGMI_CHECK_ARG(grad && amp && n > 0, "amp_check_finite: bad arguments");
  hipLaunchKernelGGL(amp_check_kernel, grid_1d(n, kOptCap), 256, 0, (hipStream_t)stream, grad, n, amp);
  SEGMI_LAUNCH_CHECK("amp_check_finite");
  return SEGMI_OK;
}

int segmi_amp_update_scale(float* amp, int32_t* growth_tracker, int64_t* step, double growth_factor,
                           double backoff_factor, int growth_interval, void* stream) {
  SEGMI_CHECK_ARG(amp && growth_tracker && growth_interval > 0, "amp_update_scale: bad arguments");
  hipLaunchKernelGGL(amp_update_kernel, 1, 64, 0, (hipStream_t)stream, amp, growth_tracker, step,
                     (float)growth_factor, (float)backoff_factor, growth_interval);
  SEGMI_LAUNCH_CHECK("amp_update_scale");
  return SEGMI_OK;
}

int segmi_adam_step_amp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        float* max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                        double eps, double weight_decay, const float* amp, const int64_t* step,
                        float grad_scale, void* stream) {
  SEGMI_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n > 0 && amp && step, "adam_amp: bad arguments");
  hipLaunchKernelGGL(adam_amp_kernel, grid_1d(n, kOptCap), 256, 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, max_exp_avg_sq, n, lr, beta1, beta2, (float)eps, (float)weight_decay, amp, step,
                     grad_scale);
  SEGMI_LAUNCH_CHECK("adam_amp");
  return SEGMI_OK;
}

int segmi_sgd_step_amp(float* param, const float* grad, float* momentum_buf, int64_t n, double lr,
                       double momentum, double weight_decay, const float* amp, const int64_t* step,
                       float grad_scale, void* stream) {
  SEGMI_CHECK_ARG(param && grad && n > 0 && (momentum == 0.0 || momentum_buf) && amp && step,
                  "sgd_amp: bad arguments");
  hipLaunchKernelGGL(sgd_amp_kernel, grid_1d(n, kOptCap), 256, 0, (hipStream_t)stream, param, grad, momentum_buf, n,
                     (float)lr, (float)momentum, (float)weight_decay, amp, step, grad_scale);
  SEGMI_LAUNCH_CHECK("sgd_amp");
  return SEGMI_OK;
}

int segmi_adabelief_step_amp(float* param, const float* grad, float* exp_avg, float* exp_avg_var,
                             int64_t n, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int weight_decouple, const float* amp,
                             const int64_t* step, float grad_scale, void* stream) {
  SEGMI_CHECK_ARG(param && grad && exp_avg && exp_avg_var && n > 0 && amp && step, "adabelief_amp: bad arguments");
  hipLaunchKernelGGL(adabelief_amp_kernel, grid_1d(n, kOptCap), 256, 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_var, n, lr, beta1, beta2, (float)eps, weight_decay, weight_decouple, amp, step,
                     grad_scale);
  SEGMI_LAUNCH_CHECK("adabelief_amp");
  return SEGMI_OK;
}

}  // extern "C"
