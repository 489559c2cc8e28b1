// patch_fusion.hip -- patch-based label fusion of A atlases onto a target (locally weighted voting and the
// non-local fusion of Coupe et al. 2011 on quantised intensities), DESIGN.md section 25.  Intensities are 8-bit,
// distances and votes are integers and the weight is a table lookup, so the result does not depend on launch
// shape or summation order.  Built with -ffp-contract=off: the quantiser is specified operation by operation.
//
// Launches of one call:
//   pf_check_kernel   labels outside 0 .. K-1 raise the device flag (first voxel, then first atlas)
//   pf_fuse_kernel    one workgroup per tile of target voxels; returns at once when the flag is raised
// One workgroup stages the target tile (halo rp) and the weight table once, then per atlas the image tile (halo
// rp + rs) and the label tile (halo rs) as bytes, and walks the search offsets from LDS.  Per offset the patch
// distance of every voxel of the tile comes from three separable box sums: along x straight from the staged
// bytes (s_xs), along y (s_ys), along z into registers.  The adaptive bandwidth needs the smallest distance of a
// voxel before any weight, so that mode walks the candidates twice (first sweep: the minimum; second sweep: the
// weights) and recomputes the distances: A * (2rs+1)^3 distances per voxel fit neither registers nor LDS.
// Scores live in LDS as [label][voxel], each voxel owned by one thread, so no atomics are needed; the tile is
// 8 x 8 x 8 while that table fits next to the staged tiles (K <= 18) and 2 x 8 x 8 above.  LDS is sized per call
// from the radii and the classes (pf_lds), so the usual radii leave room for three workgroups per CU.  The patch
// radii are template arguments where all three agree (or z is 0, a 2-D image), so that the box-sum loops unroll and
// their LDS reads issue together; other radii take the instantiation with run-time loop bounds.
#include "labelvol.h"

namespace segmi {

constexpr int kPfMaxAtlases = 16;
constexpr int kPfMaxLabels = 64;
constexpr int kPfMaxRadius = 3;
constexpr int kPfMaxH2 = 65025;              // 255^2: den = npatch * h2 stays below 2^24.5
constexpr int kPfTableEntries = 1024;
constexpr unsigned kPfMaxWeight = 65536;
constexpr int kPfThreads = 256;
constexpr int kPfTileX = 8;
constexpr int kPfTileY = 8;
constexpr int kPfTileZSmall = 8;             // tile depth while the score table of the classes fits (small-K form)
constexpr int kPfTileZLarge = 2;             // tile depth of the large-K form
constexpr int kPfSmallMaxLabels = 18;        // most classes of the small-K form: 18 * 512 scores = 36 KB
constexpr int kPfCheckGridCap = 4096;        // workgroups of 256: one pass of the grid covers 1 048 576 voxels
constexpr int kPfQuantGridCap = 4096;
constexpr uint8_t kPfOutside = 0xff;         // staged label of a position outside the volume: no candidate

typedef unsigned long long u64;

struct PfState {
  u64 bad;                                   // ~(voxel << 4 | atlas) of the first label outside 0 .. K-1, 0 = none
};

struct PfWs {
  PfState* state;
  u64* ptrs;                                 // [2][kPfMaxAtlases]: device addresses of the images, then of the label maps
};
struct PfLayout {
  size_t state, ptrs, total;
};
static inline PfLayout pf_layout() {
  PfLayout o;
  LvCarver c;
  o.state = c.take(sizeof(PfState));
  o.ptrs = c.take(sizeof(u64) * 2 * kPfMaxAtlases);
  o.total = c.off;
  return o;
}
static inline PfWs pf_carve(void* ws, const PfLayout& o) {
  char* b = (char*)ws;
  return PfWs{(PfState*)(b + o.state), (u64*)(b + o.ptrs)};
}

struct PfGeom {
  int d, h, w;
  int rpz, rpy, rpx;                         // patch radius
  int rsz, rsy, rsx;                         // search radius
  int atlases, classes;
  int adaptive;                              // 1: den = max(min D, den0); 0: den = den0
  unsigned den0;                             // npatch * min_h2 (adaptive) or npatch * h2 (fixed)
  int tiles_y, tiles_x;
};

static inline bool pf_small(int num_classes) { return num_classes <= kPfSmallMaxLabels; }

// ------------------------------------------------------------------ quantiser
// q = clamp(floor((v - lo) * scale + 0.5), 0, 255) in float32, every operation rounded on its own; NaN gives 0
__global__ __launch_bounds__(256) void pf_quantise_kernel(const float* __restrict__ src, int64_t n, float lo, float scale,
                                                          uint8_t* __restrict__ dst) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float t = (src[i] - lo) * scale;
    const float q = floorf(t + 0.5f);
    dst[i] = !(q > 0.f) ? (uint8_t)0 : q > 255.f ? (uint8_t)255 : (uint8_t)q;
  }
}

// ------------------------------------------------------------------ range check
template <typename T>
__global__ __launch_bounds__(256) void pf_check_kernel(const u64* __restrict__ ptrs, int A, int K, int64_t n, PfState* state) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    for (int a = 0; a < A; ++a) {
      const long long v = (long long)((const T*)ptrs[kPfMaxAtlases + a])[i];
      if (v < 0 || v >= K) atomicMax(&state->bad, ~((u64)i << 4 | (u64)a));
    }
}

__device__ __forceinline__ int pf_clamp(int v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }

// k = min(floor(64 D / den), 1023) without a divide per candidate.  magic = floor((2^32 - 1) / den), n = 64 D < 2^31,
// 1 <= den < 2^31.  q' = floor(n * magic / 2^32) is q = floor(n / den) or q - 1:
//   magic * den <= 2^32 - 1          so  n * magic / 2^32 <  n / den                       and q' <= q;
//   magic * den >  2^32 - 1 - den    so  n * magic / 2^32 >  n / den - n / (den 2^32) - n / 2^32 > n / den - 1
//                                    (each of the two terms is below 1/2 because n < 2^31), and q' >= q - 1.
// q' * den <= n, so the remainder n - q' * den does not wrap, lies in 0 .. 2 den - 1, and one comparison corrects q'.
__device__ __forceinline__ unsigned pf_bin(unsigned D, unsigned den, unsigned magic) {
  const unsigned n = 64u * D;
  unsigned q = __umulhi(n, magic);
  if (n - q * den >= den) ++q;
  return q < (unsigned)(kPfTableEntries - 1) ? q : (unsigned)(kPfTableEntries - 1);
}

// The LDS of one workgroup, in 32-bit words then bytes; the launch and the kernel read the same offsets.
struct PfLds {
  int w, sc, xs, ys, t, i, l, total;         // byte offsets: table, scores, x sums, xy sums, target, image, labels
};
__host__ __device__ inline PfLds pf_lds(const PfGeom& g, int TZ) {
  const int tez = TZ + 2 * g.rpz, tey = kPfTileY + 2 * g.rpy, tex = kPfTileX + 2 * g.rpx;
  PfLds o;
  int at = 0;
  auto take = [&at](int bytes) { const int was = at; at += (bytes + 15) & ~15; return was; };
  o.w = take(4 * kPfTableEntries);
  o.sc = take(4 * g.classes * TZ * kPfTileY * kPfTileX);
  o.xs = take(4 * tez * tey * kPfTileX);
  o.ys = take(4 * tez * kPfTileY * kPfTileX);
  o.t = take(tez * tey * tex);
  o.i = take((tez + 2 * g.rsz) * (tey + 2 * g.rsy) * (tex + 2 * g.rsx));
  o.l = take((TZ + 2 * g.rsz) * (kPfTileY + 2 * g.rsy) * (kPfTileX + 2 * g.rsx));
  o.total = at;
  return o;
}
// the most a call can ask for: the small-K form at its class limit and the largest radii
static_assert(4 * kPfTableEntries + 4 * kPfSmallMaxLabels * 512 + 4 * 14 * 14 * 8 + 4 * 14 * 64 + 2 * 2744 + 8000 + 7 * 16 <= 65536,
              "the LDS of a workgroup stays within 64 KB");

// ------------------------------------------------------------------ fusion
// RPZ, RPYX: the patch radius along z and along y and x when the call's radii have that form, -1: read from g
template <typename T, int TZ, int RPZ, int RPYX>
__global__ __launch_bounds__(kPfThreads) void pf_fuse_kernel(PfGeom g, PfWs ws, const uint8_t* __restrict__ tq,
                                                             const uint32_t* __restrict__ table, T* __restrict__ out,
                                                             uint32_t* __restrict__ best, uint32_t* __restrict__ total,
                                                             uint32_t* __restrict__ scores) {
  constexpr int R = kPfMaxRadius, TY = kPfTileY, TX = kPfTileX, NT = kPfThreads;
  constexpr int NV = TZ * TY * TX;                                   // voxels of a tile
  constexpr int VPT = (NV + NT - 1) / NT;                            // voxels a thread owns
  constexpr int EZ = TZ + 2 * (RPZ >= 0 ? RPZ : R), EY = TY + 2 * (RPYX >= 0 ? RPYX : R);   // tile with the patch halo
  constexpr int XQ = 4;                                              // consecutive x-pass sums that share their taps
  constexpr int XI = (EZ * EY * (TX / XQ) + NT - 1) / NT;            // groups of XQ x-pass sums a thread forms
  constexpr int YI = (EZ * TY * TX + NT - 1) / NT;                   // y-pass sums a thread forms
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
  if (ws.state->bad) return;                                         // uniform over the grid: set by the launch before
  const PfLds lds = pf_lds(g, TZ);
  uint32_t* const s_w = (uint32_t*)(s_mem + lds.w);
  uint32_t* const s_sc = (uint32_t*)(s_mem + lds.sc);                // [label][voxel]
  uint32_t* const s_xs = (uint32_t*)(s_mem + lds.xs);                // [z'][y'][x]: sums along x
  uint32_t* const s_ys = (uint32_t*)(s_mem + lds.ys);                // [z'][y][x]: sums along x and y
  uint8_t* const s_t = s_mem + lds.t;                                // target, halo rp
  uint8_t* const s_i = s_mem + lds.i;                                // atlas image, halo rp + rs
  uint8_t* const s_l = s_mem + lds.l;                                // atlas labels, halo rs
  const int tid = threadIdx.x;
  const int d = g.d, h = g.h, w = g.w, K = g.classes;
  const int rpz = RPZ >= 0 ? RPZ : g.rpz, rpy = RPYX >= 0 ? RPYX : g.rpy, rpx = RPYX >= 0 ? RPYX : g.rpx;
  const int rsz = g.rsz, rsy = g.rsy, rsx = g.rsx;
  int b = blockIdx.x;
  const int x0 = (b % g.tiles_x) * TX;
  b /= g.tiles_x;
  const int y0 = (b % g.tiles_y) * TY;
  const int z0 = (b / g.tiles_y) * TZ;
  const int tz = d - z0 < TZ ? d - z0 : TZ;                          // planes of this tile inside the volume
  // extents of the staged tiles (y and x always over the whole tile: reads are clamped, stores are guarded)
  const int tez = tz + 2 * rpz, tey = TY + 2 * rpy, tex = TX + 2 * rpx;
  const int iez = tez + 2 * rsz, iey = tey + 2 * rsy, iex = tex + 2 * rsx;
  const int lez = tz + 2 * rsz, ley = TY + 2 * rsy, lex = TX + 2 * rsx;

  for (int i = tid; i < tez * tey * tex; i += NT) {
    const int xx = i % tex, r = i / tex, yy = r % tey, zz = r / tey;
    s_t[i] = tq[((size_t)pf_clamp(z0 - rpz + zz, d) * h + pf_clamp(y0 - rpy + yy, h)) * w + pf_clamp(x0 - rpx + xx, w)];
  }
  for (int i = tid; i < kPfTableEntries; i += NT) s_w[i] = table[i] < kPfMaxWeight ? table[i] : kPfMaxWeight;
  for (int i = tid; i < K * NV; i += NT) s_sc[i] = 0;

  // what a thread sums in each pass, as offsets into the staged tiles: fixed for the whole kernel
  int xt[XI], xi[XI];
#pragma unroll
  for (int j = 0; j < XI; ++j) {
    const int i = tid + NT * j;
    const int x = (i % (TX / XQ)) * XQ, r = i / (TX / XQ), yy = r % tey, zz = r / tey;
    xt[j] = i < tez * tey * (TX / XQ) ? (zz * tey + yy) * tex + x : -1;
    xi[j] = ((zz + rsz) * iey + yy + rsy) * iex + x + rsx;
  }
  int yx[YI];
#pragma unroll
  for (int j = 0; j < YI; ++j) {
    const int i = tid + NT * j;
    const int x = i % TX, y = (i / TX) % TY, zz = i / (TX * TY);
    yx[j] = i < tez * TY * TX ? (zz * tey + y) * TX + x : -1;
  }
  int vl[VPT];                                                       // owned voxel -> its place in the label tile, -1: none
  int64_t vg[VPT];                                                   // ... and in the volume
  unsigned dmin[VPT], den[VPT], magic[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int v = tid + NT * j;
    const int x = v % TX, y = (v / TX) % TY, z = v / (TX * TY);
    const bool in = z < tz && y0 + y < h && x0 + x < w;
    vl[j] = in ? ((z + rsz) * ley + y + rsy) * lex + x + rsx : -1;
    vg[j] = ((int64_t)(z0 + z) * h + y0 + y) * w + x0 + x;
    dmin[j] = 0xffffffffu;
    den[j] = g.den0;
    magic[j] = 0xffffffffu / g.den0;
  }

  for (int sweep = g.adaptive ? 0 : 1; sweep < 2; ++sweep) {
    for (int a = 0; a < g.atlases; ++a) {
      const uint8_t* __restrict__ img = (const uint8_t*)ws.ptrs[a];
      const T* __restrict__ lab = (const T*)ws.ptrs[kPfMaxAtlases + a];
      __syncthreads();                                               // the passes over the atlas before are done
      for (int i = tid; i < iez * iey * iex; i += NT) {
        const int xx = i % iex, r = i / iex, yy = r % iey, zz = r / iey;
        s_i[i] = img[((size_t)pf_clamp(z0 - rpz - rsz + zz, d) * h + pf_clamp(y0 - rpy - rsy + yy, h)) * w +
                     pf_clamp(x0 - rpx - rsx + xx, w)];
      }
      for (int i = tid; i < lez * ley * lex; i += NT) {
        const int xx = i % lex, r = i / lex, yy = r % ley, zz = r / ley;
        const int gz = z0 - rsz + zz, gy = y0 - rsy + yy, gx = x0 - rsx + xx;
        const bool in = gz >= 0 && gz < d && gy >= 0 && gy < h && gx >= 0 && gx < w;
        s_l[i] = in ? (uint8_t)lab[((size_t)gz * h + gy) * w + gx] : kPfOutside;
      }
      __syncthreads();
      for (int oz = -rsz; oz <= rsz; ++oz)
        for (int oy = -rsy; oy <= rsy; ++oy)
          for (int ox = -rsx; ox <= rsx; ++ox) {
            const int io = (oz * iey + oy) * iex + ox, lo = (oz * ley + oy) * lex + ox;
            // along x, from the bytes: s_xs[z'][y'][x] = sum over px of (T[x + px] - I[x + px + o])^2, XQ
            // consecutive x per thread: they share all but XQ - 1 of their squared differences
#pragma unroll
            for (int j = 0; j < XI; ++j)
              if (xt[j] >= 0) {
                const uint8_t* pt = s_t + xt[j];
                const uint8_t* pi = s_i + xi[j] + io;
                u32x4 sum;
                if constexpr (RPYX >= 0) {
                  unsigned e[2 * RPYX + XQ];
#pragma unroll
                  for (int k = 0; k < 2 * RPYX + XQ; ++k) {
                    const int df = (int)pt[k] - (int)pi[k];
                    e[k] = (unsigned)(df * df);
                  }
                  unsigned s = 0;
#pragma unroll
                  for (int k = 0; k <= 2 * RPYX; ++k) s += e[k];
                  sum[0] = s;
#pragma unroll
                  for (int q = 1; q < XQ; ++q) {
                    s += e[2 * RPYX + q] - e[q - 1];
                    sum[q] = s;
                  }
                } else {
#pragma unroll
                  for (int q = 0; q < XQ; ++q) {
                    unsigned s = 0;
                    for (int px = 0; px <= 2 * rpx; ++px) {
                      const int df = (int)pt[q + px] - (int)pi[q + px];
                      s += (unsigned)(df * df);
                    }
                    sum[q] = s;
                  }
                }
                *(u32x4*)&s_xs[XQ * (tid + NT * j)] = sum;
              }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < YI; ++j)
              if (yx[j] >= 0) {
                unsigned s = 0;
#pragma unroll
                for (int py = 0; py <= 2 * rpy; ++py) s += s_xs[yx[j] + py * TX];
                s_ys[tid + NT * j] = s;
              }
            __syncthreads();
            // along z into registers; the next offset's x-pass may begin meanwhile (it writes s_xs only)
#pragma unroll
            for (int j = 0; j < VPT; ++j)
              if (vl[j] >= 0) {
                const unsigned l = s_l[vl[j] + lo];
                if (l != kPfOutside) {
                  unsigned D = 0;
#pragma unroll
                  for (int pz = 0; pz <= 2 * rpz; ++pz) D += s_ys[tid + NT * j + pz * TY * TX];
                  if (sweep == 0) dmin[j] = D < dmin[j] ? D : dmin[j];
                  else s_sc[l * NV + tid + NT * j] += s_w[pf_bin(D, den[j], magic[j])];
                }
              }
          }
    }
    if (sweep == 0) {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        den[j] = dmin[j] != 0xffffffffu && dmin[j] > g.den0 ? dmin[j] : g.den0;
        magic[j] = 0xffffffffu / den[j];                             // one divide per voxel
      }
    }
  }

  // every score of a voxel was added by the thread that owns it: no barrier before they are read
#pragma unroll
  for (int j = 0; j < VPT; ++j)
    if (vl[j] >= 0) {
      uint32_t* sc = s_sc + tid + NT * j;
      unsigned sum = 0;
      for (int l = 0; l < K; ++l) sum += sc[l * NV];
      if (sum == 0) {                                                // no weight at all: the unweighted vote at o = 0
        for (int a = 0; a < g.atlases; ++a) sc[(int)((const T*)ws.ptrs[kPfMaxAtlases + a])[vg[j]] * NV] += 1;
        sum = g.atlases;
      }
      unsigned top = 0;
      int arg = 0;
      for (int l = 0; l < K; ++l) {
        const unsigned s = sc[l * NV];
        if (s > top) { top = s; arg = l; }                           // first maximum: the smallest label among equals
        if (scores) scores[(size_t)l * d * h * w + vg[j]] = s;
      }
      out[vg[j]] = (T)arg;
      if (best) best[vg[j]] = top;
      if (total) total[vg[j]] = sum;
    }
}

static bool pf_radii_ok(const int32_t* r) {
  return r && r[0] >= 0 && r[0] <= kPfMaxRadius && r[1] >= 0 && r[1] <= kPfMaxRadius && r[2] >= 0 && r[2] <= kPfMaxRadius;
}
static bool pf_shape_ok(int atlases, int num_classes) {
  return atlases >= 1 && atlases <= kPfMaxAtlases && num_classes >= 2 && num_classes <= kPfMaxLabels;
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int segmi_quantise_u8(const float* src, int64_t n, double lo, double hi, uint8_t* dst, void* stream) {
  SEGMI_CHECK_ARG(src && dst, "quantise_u8: null pointer");
  SEGMI_CHECK_ARG(n > 0 && n < (1ll << 31), "quantise_u8: 0 < n < 2^31");
  SEGMI_CHECK_ARG(lo > -__builtin_inf() && hi < __builtin_inf() && hi > lo, "quantise_u8: lo < hi, both finite");
  const float scale = (float)(255.0 / (hi - lo));
  SEGMI_CHECK_ARG(scale < (float)__builtin_inf(), "quantise_u8: the range hi - lo is too narrow for float32");
  hipLaunchKernelGGL(pf_quantise_kernel, lv_grid(n, 256, kPfQuantGridCap), 256, 0, (hipStream_t)stream, src, n, (float)lo,
                     scale, dst);
  SEGMI_LAUNCH_CHECK("quantise_u8");
  return SEGMI_OK;
}

int64_t segmi_patch_fusion_workspace_bytes(int atlases, int num_classes) {
  if (!pf_shape_ok(atlases, num_classes)) return 0;
  return (int64_t)pf_layout().total;
}

const char* segmi_patch_fusion_variant_name(int num_classes, const int32_t* patch_radius, const int32_t* search_radius) {
  if (!pf_shape_ok(1, num_classes) || !pf_radii_ok(patch_radius) || !pf_radii_ok(search_radius)) return "";
  return pf_small(num_classes) ? "lds_scores_tile_8x8x8" : "lds_scores_tile_2x8x8";
}

int segmi_patch_fusion(const uint8_t* target_q, const void* const* atlas_q_host, const void* const* atlas_labels_host,
                       int atlases, int label_bytes, int d, int h, int w, int num_classes, const int32_t* patch_radius,
                       const int32_t* search_radius, int adaptive, int h2, const uint32_t* table, void* out, uint32_t* best,
                       uint32_t* total, uint32_t* scores, int32_t* info_host, void* ws, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(target_q && atlas_q_host && atlas_labels_host && table && out && info_host && ws, "patch_fusion: null pointer");
  LV_CHECK_LABEL_BYTES("patch_fusion", label_bytes);
  LV_CHECK_VOXELS("patch_fusion", d, h, w);
  SEGMI_CHECK_ARG(pf_shape_ok(atlases, num_classes), "patch_fusion: 1 .. %d atlases, 2 .. %d classes", kPfMaxAtlases,
                  kPfMaxLabels);
  SEGMI_CHECK_ARG(pf_radii_ok(patch_radius) && pf_radii_ok(search_radius), "patch_fusion: radii (z, y, x) in 0 .. %d",
                  kPfMaxRadius);
  SEGMI_CHECK_ARG(adaptive == 0 || adaptive == 1, "patch_fusion: adaptive must be 0 or 1");
  SEGMI_CHECK_ARG(h2 >= 1 && h2 <= kPfMaxH2, "patch_fusion: h2 / min_h2 in 1 .. %d", kPfMaxH2);
  const PfLayout lay = pf_layout();
  SEGMI_CHECK_ARG(ws_bytes >= lay.total, "patch_fusion: workspace of %zu bytes, %zu needed", ws_bytes, lay.total);
  u64 ptrs[2 * kPfMaxAtlases] = {};
  for (int a = 0; a < atlases; ++a) {
    SEGMI_CHECK_ARG(atlas_q_host[a] && atlas_labels_host[a], "patch_fusion: null atlas volume");
    ptrs[a] = (u64)(uintptr_t)atlas_q_host[a];
    ptrs[kPfMaxAtlases + a] = (u64)(uintptr_t)atlas_labels_host[a];
  }
  const int ext[3] = {d, h, w};
  int rp[3], rs[3];
  for (int a = 0; a < 3; ++a) {                       // an axis of extent 1 has no neighbours: both radii are 0 there
    rp[a] = ext[a] == 1 ? 0 : patch_radius[a];
    rs[a] = ext[a] == 1 ? 0 : search_radius[a];
  }
  const int tzs = pf_small(num_classes) ? kPfTileZSmall : kPfTileZLarge;
  PfGeom g{};
  g.d = d; g.h = h; g.w = w;
  g.rpz = rp[0]; g.rpy = rp[1]; g.rpx = rp[2];
  g.rsz = rs[0]; g.rsy = rs[1]; g.rsx = rs[2];
  g.atlases = atlases;
  g.classes = num_classes;
  g.adaptive = adaptive;
  g.den0 = (unsigned)((2 * rp[0] + 1) * (2 * rp[1] + 1) * (2 * rp[2] + 1)) * (unsigned)h2;
  g.tiles_y = cdiv(h, kPfTileY);
  g.tiles_x = cdiv(w, kPfTileX);
  const int64_t tiles = (int64_t)cdiv(d, tzs) * g.tiles_y * g.tiles_x;   // below 2^31 / 8: a grid takes them all
  const int64_t n = (int64_t)d * h * w;
  hipStream_t st = (hipStream_t)stream;
  const PfWs wsp = pf_carve(ws, lay);
  info_host[0] = -1;
  info_host[1] = 0;
  if (hipMemsetAsync(wsp.state, 0, sizeof(PfState), st) != hipSuccess) {
    set_error("patch_fusion: memset failed");
    return SEGMI_ELAUNCH;
  }
  lv_upload_table<2 * kPfMaxAtlases>(ptrs, 2 * kPfMaxAtlases, LvStore<u64>{wsp.ptrs}, st);
#define CHECK(T) \
  hipLaunchKernelGGL(pf_check_kernel<T>, lv_grid(n, 256, kPfCheckGridCap), 256, 0, st, wsp.ptrs, atlases, num_classes, n, wsp.state)
  LV_BY_LABEL(label_bytes, CHECK);
#undef CHECK
  const unsigned lds = (unsigned)pf_lds(g, tzs).total;
  const int ryx = rp[1] == rp[2] ? rp[1] : -1;        // the compile-time radii: (r, r, r) or (0, r, r), else none
  const int rz = ryx >= 0 && (rp[0] == ryx || rp[0] == 0) ? rp[0] : -1;
#define FUSE_AS(T, TZ, RZ, RYX)                                                                                      \
  hipLaunchKernelGGL((pf_fuse_kernel<T, TZ, RZ, RYX>), (unsigned)tiles, kPfThreads, lds, st, g, wsp, target_q, table, (T*)out, \
                     best, total, scores)
#define FUSE_TILE(T, TZ)                                              \
  do {                                                                \
    if (rz < 0) FUSE_AS(T, TZ, -1, -1);                               \
    else if (ryx == 0) FUSE_AS(T, TZ, 0, 0);                          \
    else if (ryx == 1 && rz == 1) FUSE_AS(T, TZ, 1, 1);               \
    else if (ryx == 2 && rz == 2) FUSE_AS(T, TZ, 2, 2);               \
    else if (ryx == 3 && rz == 3) FUSE_AS(T, TZ, 3, 3);               \
    else if (ryx == 1) FUSE_AS(T, TZ, 0, 1);                          \
    else if (ryx == 2) FUSE_AS(T, TZ, 0, 2);                          \
    else FUSE_AS(T, TZ, 0, 3);                                        \
  } while (0)
#define FUSE(T)                                                       \
  do {                                                                \
    if (tzs == kPfTileZSmall) FUSE_TILE(T, kPfTileZSmall);            \
    else FUSE_TILE(T, kPfTileZLarge);                                 \
  } while (0)
  LV_BY_LABEL(label_bytes, FUSE);
#undef FUSE
#undef FUSE_TILE
#undef FUSE_AS
  SEGMI_LAUNCH_CHECK("patch_fusion");
  PfState host{};
  if (hipMemcpyAsync(&host, wsp.state, sizeof(host), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    set_error("patch_fusion: reading the state back failed");
    return SEGMI_ELAUNCH;
  }
  if (host.bad) {                                     // report the atlas and the value; nothing was written
    const int a = (int)(~host.bad & 15);
    const int64_t i = (int64_t)(~host.bad >> 4);
    int32_t v4 = 0;
    int16_t v2 = 0;
    uint8_t v1 = 0;
    void* dst = label_bytes == 4 ? (void*)&v4 : label_bytes == 2 ? (void*)&v2 : (void*)&v1;
    if (hipMemcpyAsync(dst, (const char*)atlas_labels_host[a] + (size_t)i * label_bytes, label_bytes, hipMemcpyDeviceToHost,
                       st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      set_error("patch_fusion: reading the offending label back failed");
      return SEGMI_ELAUNCH;
    }
    info_host[0] = a;
    info_host[1] = label_bytes == 4 ? v4 : label_bytes == 2 ? (int32_t)v2 : (int32_t)v1;
  }
  return SEGMI_OK;
}

}  // extern "C"
