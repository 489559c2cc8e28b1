// components.hip -- multi-label connected-component labelling (2-D / 3-D, connectivity 1..ndim) by
// union-find, and the label-map clean-up kernels built on it: component sizes, canonical 1..n
// numbering, keep-largest (per-class top-k), remove-small, fill-holes, and the MapLabels LUT pass
// (reference src/segmantic/seg/transforms.py:91-127).  Everything is integer arithmetic with one
// canonical result; DESIGN.md section 13 holds the definitions.
//
// Union-find INVARIANT (every loop below terminates because of it):
//   parent[v] <= v at all times, and every atomic only ever LOWERS a parent.
// Hence a find chain strictly descends (at most v steps) and every round of a union loop strictly
// lowers its larger operand: all loops end on any input, whatever the other workgroups do.  There is
// no cooperative launch, no grid barrier and no spin-wait; the phases are separate launches.  Linking
// towards the smaller linear index makes a component's root its first voxel in raster order, so the
// result does not depend on scheduling.  Inside the launches that lower parents, parents are read
// with relaxed agent-scope atomic loads only (never through a cached plain load).
//
// Passes of segmi_cc_label (the output array `root` is the parent array):
//   1. tile  : one workgroup per 64 x 8 x 8 tile.  A wave reads 64 consecutive x voxels; ballots give
//              every voxel the start of its equal-value run as first parent; the unions inside the
//              tile run on LDS atomics; the tile is flattened in LDS and written as linear indices.
//   2. seam  : unions of the neighbour pairs that cross a tile face / edge / corner, lock-free on
//              global atomics.
//   3. flatten: root[v] = find(v).
// A pair of facing runs needs one union only, so both passes skip the pairs another pair implies:
//   straight pair (v, n = v + (dz, dy, 0)): skipped when v-1 ~ v and n-1 ~ n (the pair (v-1, n-1) does it);
//   diagonal pair (v, n = v + (dz, dy, +-1)): skipped when v ~ v + (dz, dy, 0) (that straight pair and
//   n's x-run do it) or when v's x-neighbour on n's side has v's value (its straight pair does it).
// The straight pair has fewer non-zero offsets than the diagonal one, so connectivity always admits it.
#include "labelvol.h"

namespace segmi {

constexpr int kTX = 64, kTY = 8, kTZ = 8, kTile = kTX * kTY * kTZ;
constexpr int kScanItems = 4096;       // voxels per workgroup of the compaction passes (4 waves x 16 x 64)
constexpr int kClassTable = 65536;     // classes of the keep-largest table (256 are used for uint8)
constexpr int kMaxKeep = 8;
constexpr int kAppliedChunk = 64;

// compact needs the regions before `keys`, keep-largest those before `lo`, fill-holes all of them.  lo and hi
// are the int32 words per voxel that ops.CC_FILL_WORDS counts: keep the two in step
struct CcLayout { size_t partials, keys, winners, applied, lo, hi, total; };
static CcLayout cc_layout(int64_t n) {
  LvCarver c;
  CcLayout l{};
  l.partials = c.take((size_t)(cdiv64(n, kScanItems) + 1) * sizeof(int32_t));
  l.keys = c.take((size_t)kClassTable * sizeof(unsigned long long));
  l.winners = c.take((size_t)kMaxKeep * kClassTable * sizeof(int32_t));
  l.applied = c.take((size_t)kClassTable / 8);
  l.lo = c.take((size_t)n * sizeof(int32_t));
  l.hi = c.take((size_t)n * sizeof(int32_t));
  l.total = c.off;
  return l;
}

struct CcParams {
  const void* lab;
  int d, h, w, conn, with_bg;
  int32_t* parent;
};

#define CC_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CC_LOAD_WG(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)

// chain of strictly descending parents: ends after at most v steps
__device__ __forceinline__ int cc_find(int32_t* parent, int v) {
  int nxt;
  while ((nxt = CC_LOAD(parent + v)) != v) v = nxt;
  return v;
}
// every round lowers max(a, b): ends without any other workgroup's help
__device__ __forceinline__ void cc_union(int32_t* parent, int a, int b) {
  a = cc_find(parent, a);
  b = cc_find(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) break;
    a = old;
  }
}
__device__ __forceinline__ int cc_find_lds(int* par, int v) {
  int nxt;
  while ((nxt = CC_LOAD_WG(par + v)) != v) v = nxt;
  return v;
}
__device__ __forceinline__ void cc_union_lds(int* par, int a, int b) {
  a = cc_find_lds(par, a);
  b = cc_find_lds(par, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);
    if (old == a) break;
    a = old;
  }
}

__device__ __forceinline__ int nnz3(int a, int b, int c) { return (a != 0) + (b != 0) + (c != 0); }

// ---- pass 1: tile-local labelling in LDS
template <typename T>
__global__ __launch_bounds__(256) void cc_tile_kernel(CcParams p, int tiles_x, int tiles_y) {
  __shared__ int lab[kTile];
  __shared__ int par[kTile];   // local index of the parent, -1 for voxels outside every component
  const T* __restrict__ src = (const T*)p.lab;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, tz = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = tx * kTX, y0 = ty * kTY, z0 = tz * kTZ;

  for (int row = wave; row < kTY * kTZ; row += 4) {
    const int z = z0 + row / kTY, y = y0 + row % kTY, x = x0 + lane;
    const bool inb = z < p.d && y < p.h && x < p.w;
    const int val = inb ? (int)src[((int64_t)z * p.h + y) * p.w + x] : 0;
    const bool active = inb && (p.with_bg || val != 0);
    const int pv = __shfl_up(val, 1);
    const int pa = __shfl_up((int)active, 1);
    const bool head = active && (lane == 0 || !pa || pv != val);
    const unsigned long long heads = __ballot(head);
    const int start = 63 - __clzll(heads & ((2ull << lane) - 1ull));   // own run's head: set for every active lane
    lab[row * kTX + lane] = val;
    par[row * kTX + lane] = active ? row * kTX + start : -1;
  }
  __syncthreads();

  // whether tile voxels i and j (both inside the tile) are voxels of components and carry one value
#define EQ(i, j) (CC_LOAD_WG(par + (i)) >= 0 && CC_LOAD_WG(par + (j)) >= 0 && lab[i] == lab[j])
  for (int row = wave; row < kTY * kTZ; row += 4) {
    const int lz = row / kTY, ly = row % kTY, lx = lane, li = row * kTX + lane;
    if (CC_LOAD_WG(par + li) < 0) continue;
    for (int dz = -1; dz <= 0; ++dz)
      for (int dy = -1; dy <= (dz ? 1 : -1); ++dy) {
        const int nz = lz + dz, ny = ly + dy;
        if (nz < 0 || ny < 0 || ny >= kTY || nnz3(dz, dy, 0) > p.conn) continue;
        const int ri = (nz * kTY + ny) * kTX + lx;   // the straight neighbour
        const bool straight = EQ(li, ri);
        // a neighbour outside the tile counts as different: that can only add a redundant union
        if (straight && !(lx > 0 && EQ(li, li - 1) && EQ(ri, ri - 1))) cc_union_lds(par, li, ri);
        if (straight || nnz3(dz, dy, 1) > p.conn) continue;
        if (lx > 0 && EQ(li, ri - 1) && !EQ(li, li - 1)) cc_union_lds(par, li, ri - 1);
        if (lx < kTX - 1 && EQ(li, ri + 1) && !EQ(li, li + 1)) cc_union_lds(par, li, ri + 1);
      }
  }
#undef EQ
  __syncthreads();

  for (int row = wave; row < kTY * kTZ; row += 4) {
    const int z = z0 + row / kTY, y = y0 + row % kTY, x = x0 + lane;
    if (!(z < p.d && y < p.h && x < p.w)) continue;
    const int li = row * kTX + lane;
    int g = -1;
    if (par[li] >= 0) {
      const int r = cc_find_lds(par, li);   // local raster order is global raster order: r is the tile's first voxel
      const int rrow = r / kTX;
      g = (int)(((int64_t)(z0 + rrow / kTY) * p.h + (y0 + rrow % kTY)) * p.w + x0 + r % kTX);
    }
    p.parent[((int64_t)z * p.h + y) * p.w + x] = g;
  }
}

// ---- pass 2: unions across tile seams, one wave per 64 consecutive x voxels of a row
template <typename T>
__global__ __launch_bounds__(256) void cc_seam_kernel(CcParams p, int chunks, int64_t waves) {
  const T* __restrict__ src = (const T*)p.lab;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= waves) return;
  const int lane = threadIdx.x & 63;
  const int64_t rowi = wid / chunks;
  const int x = (int)(wid % chunks) * kTX + lane, y = (int)(rowi % p.h), z = (int)(rowi / p.h);
  const int lz = z % kTZ, ly = y % kTY;
  if (x >= p.w) return;
  // only voxels on a tile face have a neighbour pair that leaves the tile
  if (lz != 0 && ly != 0 && ly != kTY - 1 && lane != 0 && lane != kTX - 1) return;
  const int64_t v = ((int64_t)z * p.h + y) * p.w + x;
  const int a = (int)src[v];
  if (!p.with_bg && a == 0) return;
  // same value (v's own is `a`, a voxel of a component): zeros match only when the background is labelled
#define SAME(i) ((int)src[i] == a)
  if (lane == 0 && x > 0 && SAME(v - 1)) cc_union(p.parent, (int)v, (int)v - 1);
  for (int dz = -1; dz <= 0; ++dz)
    for (int dy = -1; dy <= (dz ? 1 : -1); ++dy) {
      const int nz = z + dz, ny = y + dy;
      if (nz < 0 || ny < 0 || ny >= p.h || nnz3(dz, dy, 0) > p.conn) continue;
      const bool row_out = (lz + dz < 0) || (ly + dy < 0) || (ly + dy >= kTY);   // the row lies in another tile
      if (!row_out && lane != 0 && lane != kTX - 1) continue;
      const int64_t r = ((int64_t)nz * p.h + ny) * p.w + x;
      const bool straight = SAME(r);
      if (straight) {
        if (row_out && !(x > 0 && SAME(v - 1) && SAME(r - 1))) cc_union(p.parent, (int)v, (int)r);
        continue;
      }
      if (nnz3(dz, dy, 1) > p.conn) continue;
      if (x > 0 && (row_out || lane == 0) && SAME(r - 1) && !SAME(v - 1)) cc_union(p.parent, (int)v, (int)(r - 1));
      if (x + 1 < p.w && (row_out || lane == kTX - 1) && SAME(r + 1) && !SAME(v + 1))
        cc_union(p.parent, (int)v, (int)(r + 1));
    }
#undef SAME
}

// ---- pass 3: root[v] = find(v); the store lowers parent[v] (path compression), so it is atomic too
__global__ __launch_bounds__(256) void cc_flatten_kernel(int32_t* parent, int64_t n) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int q = CC_LOAD(parent + v);
  if (q < 0 || q == (int)v) return;
  const int r = cc_find(parent, q);
  if (r != q) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- sizes: one atomic per (wave, run of lanes that share a root)
__global__ __launch_bounds__(256) void cc_sizes_kernel(const int32_t* __restrict__ root, int64_t n,
                                                       int32_t* __restrict__ size) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int r = v < n ? root[v] : -2;
  const int prev = __shfl_up(r, 1);
  const bool edge = lane == 0 || prev != r;
  const unsigned long long edges = __ballot(edge);
  if (edge && r >= 0) {
    const unsigned long long above = lane == 63 ? 0ull : edges & ~((2ull << lane) - 1ull);
    const int end = above ? __ffsll((long long)above) - 1 : 64;
    atomicAdd(size + r, end - lane);
  }
}

// ---- canonical numbering: prefix count over root flags (count / scan of partials / apply / gather)
__device__ __forceinline__ int64_t scan_index(int64_t block, int wave, int j, int lane) {
  return block * kScanItems + wave * (kScanItems / 4) + j * 64 + lane;
}
__global__ __launch_bounds__(256) void cc_count_kernel(const int32_t* __restrict__ root, int64_t n,
                                                       int32_t* __restrict__ partials) {
  __shared__ int tot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int c = 0;
  for (int j = 0; j < 16; ++j) {
    const int64_t v = scan_index(blockIdx.x, wave, j, lane);
    c += __popcll(__ballot(v < n && root[v] == (int)v));
  }
  if (lane == 0) tot[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = tot[0] + tot[1] + tot[2] + tot[3];
}
__global__ __launch_bounds__(256) void cc_number_kernel(const int32_t* __restrict__ root, int64_t n,
                                                        const int32_t* __restrict__ partials,
                                                        int32_t* __restrict__ comp) {
  __shared__ int tot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int c = 0;
  for (int j = 0; j < 16; ++j) {
    const int64_t v = scan_index(blockIdx.x, wave, j, lane);
    c += __popcll(__ballot(v < n && root[v] == (int)v));
  }
  if (lane == 0) tot[wave] = c;
  __syncthreads();
  int run = partials[blockIdx.x];
  for (int k = 0; k < wave; ++k) run += tot[k];
  for (int j = 0; j < 16; ++j) {
    const int64_t v = scan_index(blockIdx.x, wave, j, lane);
    const bool is_root = v < n && root[v] == (int)v;
    const unsigned long long m = __ballot(is_root);
    if (is_root) comp[v] = run + __popcll(m & ((1ull << lane) - 1ull)) + 1;
    run += __popcll(m);
  }
}
__global__ __launch_bounds__(256) void cc_gather_kernel(const int32_t* __restrict__ root, int64_t n,
                                                        int32_t* comp) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int r = root[v];
  if (r == (int)v) return;            // numbered by cc_number_kernel; no other thread writes a root's entry
  comp[v] = r < 0 ? 0 : comp[r];
}

// ---- the set of applied labels as a bit table
struct CcAppliedBits {
  unsigned* bits;
  __device__ void operator()(int, int32_t v) const {
    if (v >= 0 && v < kClassTable) atomicOr(bits + (v >> 5), 1u << (v & 31));
  }
};
__device__ __forceinline__ bool cc_applied(const unsigned* bits, int c) {
  return c >= 0 && c < kClassTable && ((bits[c >> 5] >> (c & 31)) & 1u);
}

// ---- keep-largest: num_components rounds of a 64-bit atomicMax over the roots of each class
struct KeepParams {
  const void* lab;
  const int32_t* root;
  const int32_t* size;
  const unsigned* applied;
  unsigned long long* keys;
  int32_t* winners;     // [kMaxKeep][kClassTable], -1 = none
  int64_t n;
  int classes, independent, rounds;
  void* out;
};
// class slot of a root; -1 when the voxel takes no part
template <typename T>
__device__ __forceinline__ int keep_slot(const KeepParams& p, int64_t v) {
  if (!p.independent) return 0;     // the roots come from the union mask of the applied classes
  const int c = (int)((const T*)p.lab)[v];
  return (c > 0 && c < p.classes && cc_applied(p.applied, c)) ? c : -1;
}
template <typename T>
__global__ __launch_bounds__(256) void cc_keep_round_kernel(KeepParams p, int round) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= p.n || p.root[v] != (int)v) return;
  const int c = keep_slot<T>(p, v);
  if (c < 0) return;
  for (int j = 0; j < round; ++j)
    if (p.winners[j * kClassTable + c] == (int)v) return;
  // larger size first, then the smaller first voxel
  atomicMax(p.keys + c, ((unsigned long long)(unsigned)p.size[v] << 32) | (unsigned)~(unsigned)v);
}
__global__ void cc_keep_pick_kernel(KeepParams p, int round) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= p.classes) return;
  const unsigned long long k = p.keys[c];
  p.winners[round * kClassTable + c] = k ? (int)~(unsigned)(k & 0xffffffffull) : -1;
  p.keys[c] = 0ull;
}
template <typename T>
__global__ __launch_bounds__(256) void cc_keep_apply_kernel(KeepParams p) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= p.n) return;
  const T val = ((const T*)p.lab)[v];
  const int r = p.root[v];
  T o = val;
  if (r >= 0) {
    const int c = keep_slot<T>(p, v);
    if (c >= 0) {
      bool keep = false;
      for (int j = 0; j < p.rounds; ++j) keep |= p.winners[j * kClassTable + c] == r;
      if (!keep) o = (T)0;
    }
  }
  ((T*)p.out)[v] = o;
}

template <typename T>
__global__ __launch_bounds__(256) void cc_remove_small_kernel(const T* __restrict__ lab, const int32_t* __restrict__ root,
                                                              const int32_t* __restrict__ size, int64_t n,
                                                              int min_size, T* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int r = root[v];
  out[v] = (r >= 0 && size[r] < min_size) ? (T)0 : lab[v];
}

// ---- fill-holes: (min, max) of the neighbouring non-zero values at the root of every 0-component;
// a voxel on the array border forces min != max
struct FillParams {
  const void* lab;
  const int32_t* root;
  const unsigned* applied;
  int32_t* lo;
  int32_t* hi;
  int d, h, w, sd, conn, all;
  void* out;
};
template <typename T>
__global__ __launch_bounds__(256) void cc_fill_init_kernel(FillParams p, int64_t n) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n || p.root[v] != (int)v || ((const T*)p.lab)[v] != (T)0) return;
  p.lo[v] = INT32_MAX;
  p.hi[v] = INT32_MIN;
}
template <typename T>
__global__ __launch_bounds__(256) void cc_fill_scan_kernel(FillParams p, int64_t n) {
  const T* __restrict__ src = (const T*)p.lab;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n || src[v] != (T)0) return;
  const int x = (int)(v % p.w), y = (int)((v / p.w) % p.h), z = (int)(v / ((int64_t)p.w * p.h));
  int lo = INT32_MAX, hi = INT32_MIN;
  if (x == 0 || x == p.w - 1 || y == 0 || y == p.h - 1 || (p.sd == 3 && (z == 0 || z == p.d - 1))) {
    lo = INT32_MIN;
    hi = INT32_MAX;
  } else {
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int nz = z + dz;
          if (nz < 0 || nz >= p.d || nnz3(dz, dy, dx) > p.conn || nnz3(dz, dy, dx) == 0) continue;
          const int c = (int)src[((int64_t)nz * p.h + (y + dy)) * p.w + (x + dx)];   // y, x are interior
          if (c != 0) { lo = c < lo ? c : lo; hi = c > hi ? c : hi; }
        }
    if (lo > hi) return;            // no labelled neighbour
  }
  const int r = p.root[v];
  if (r < 0) return;              // root was labelled without the background: nothing to fill
  // both words only ever move outwards: skip the atomic that would change nothing
  if (lo < CC_LOAD(p.lo + r)) atomicMin(p.lo + r, lo);
  if (hi > CC_LOAD(p.hi + r)) atomicMax(p.hi + r, hi);
}
template <typename T>
__global__ __launch_bounds__(256) void cc_fill_apply_kernel(FillParams p, int64_t n) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  T o = ((const T*)p.lab)[v];
  if (o == (T)0) {
    const int r = p.root[v];
    if (r >= 0) {
      const int lo = p.lo[r], hi = p.hi[r];
      if (lo == hi && (p.all || cc_applied(p.applied, lo))) o = (T)lo;
    }
  }
  ((T*)p.out)[v] = o;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void map_labels_kernel(const TI* __restrict__ in, int64_t n,
                                                         const int64_t* __restrict__ lut, int lut_len,
                                                         TO* __restrict__ out) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t k = (int64_t)in[i];
    // the caller has checked the range; a stray index must still never leave the table
    out[i] = (k >= 0 && k < lut_len) ? (TO)lut[k] : (TO)0;
  }
}

static int cc_set_applied(unsigned* bits, const int32_t* applied_host, int n_applied, hipStream_t st) {
  if (hipMemsetAsync(bits, n_applied ? 0 : 0xff, kClassTable / 8, st) != hipSuccess) return 1;
  lv_upload_table<kAppliedChunk>(applied_host, n_applied, CcAppliedBits{bits}, st);
  return 0;
}

}  // namespace segmi

using namespace segmi;

extern "C" {

int64_t segmi_cc_workspace_bytes(int d, int h, int w) {
  if (!lv_voxels_ok(d, h, w)) return 0;
  return (int64_t)cc_layout((int64_t)d * h * w).total;
}

int segmi_cc_label(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int connectivity,
                   int with_background, int32_t* root, void* ws, size_t ws_bytes, void* stream) {
  (void)ws; (void)ws_bytes;   // the parent array is `root` itself; labelling needs no scratch
  SEGMI_CHECK_ARG(labels && root, "cc_label: null pointer");
  LV_CHECK_LABEL_BYTES("cc_label", label_bytes);
  LV_CHECK_SPATIAL_DIMS("cc_label", spatial_dims, d);
  LV_CHECK_VOXELS("cc_label", d, h, w);
  SEGMI_CHECK_ARG(connectivity >= 1 && connectivity <= spatial_dims, "cc_label: connectivity must be 1 .. %d", spatial_dims);
  hipStream_t st = (hipStream_t)stream;
  CcParams p{labels, d, h, w, connectivity, with_background ? 1 : 0, root};
  const int64_t n = (int64_t)d * h * w;
  const int tx = cdiv(w, kTX), ty = cdiv(h, kTY), tz = cdiv(d, kTZ);
  const int64_t tiles = (int64_t)tx * ty * tz;
  const int64_t waves = (int64_t)d * h * tx;
  SEGMI_CHECK_ARG(tiles < (1ll << 31) && cdiv64(waves, 4) < (1ll << 31), "cc_label: too many rows for one launch");
#define TILE(T) hipLaunchKernelGGL(cc_tile_kernel<T>, (unsigned)tiles, 256, 0, st, p, tx, ty)
  LV_BY_LABEL(label_bytes, TILE);
#undef TILE
#define SEAM(T) hipLaunchKernelGGL(cc_seam_kernel<T>, (unsigned)cdiv64(waves, 4), 256, 0, st, p, tx, waves)
  LV_BY_LABEL(label_bytes, SEAM);
#undef SEAM
  hipLaunchKernelGGL(cc_flatten_kernel, (unsigned)cdiv64(n, 256), 256, 0, st, root, n);
  SEGMI_LAUNCH_CHECK("cc_label");
  return SEGMI_OK;
}

int segmi_cc_sizes(const int32_t* root, int64_t n, int32_t* size, void* stream) {
  SEGMI_CHECK_ARG(root && size, "cc_sizes: null pointer");
  SEGMI_CHECK_ARG(n > 0 && n < (1ll << 31), "cc_sizes: 0 < n < 2^31");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(size, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess) {
    set_error("cc_sizes: memset failed");
    return SEGMI_ELAUNCH;
  }
  hipLaunchKernelGGL(cc_sizes_kernel, (unsigned)cdiv64(n, 256), 256, 0, st, root, n, size);
  SEGMI_LAUNCH_CHECK("cc_sizes");
  return SEGMI_OK;
}

int segmi_cc_compact(const int32_t* root, int64_t n, int32_t* comp, int32_t* n_comp, void* ws, size_t ws_bytes,
                     void* stream) {
  SEGMI_CHECK_ARG(root && comp && n_comp && ws, "cc_compact: null pointer");
  SEGMI_CHECK_ARG(n > 0 && n < (1ll << 31), "cc_compact: 0 < n < 2^31");
  const CcLayout l = cc_layout(n);
  SEGMI_CHECK_ARG(ws_bytes >= l.keys, "cc_compact: workspace of %zu bytes, %zu needed", ws_bytes, l.keys);
  hipStream_t st = (hipStream_t)stream;
  int32_t* partials = (int32_t*)((char*)ws + l.partials);
  const int64_t nb = cdiv64(n, kScanItems);
  hipLaunchKernelGGL(cc_count_kernel, (unsigned)nb, 256, 0, st, root, n, partials);
  hipLaunchKernelGGL(lv_scan_partials_kernel<1>, 1, 1024, 0, st, (uint32_t*)partials, nb, (uint32_t*)n_comp, (uint32_t*)nullptr);
  hipLaunchKernelGGL(cc_number_kernel, (unsigned)nb, 256, 0, st, root, n, (const int32_t*)partials, comp);
  hipLaunchKernelGGL(cc_gather_kernel, (unsigned)cdiv64(n, 256), 256, 0, st, root, n, comp);
  SEGMI_LAUNCH_CHECK("cc_compact");
  return SEGMI_OK;
}

int segmi_cc_keep_largest(const void* labels, int label_bytes, int64_t n, const int32_t* root, const int32_t* size,
                          const int32_t* applied_host, int n_applied, int independent, int num_components,
                          void* out, void* ws, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(labels && root && size && out && ws, "cc_keep_largest: null pointer");
  LV_CHECK_LABEL_BYTES("cc_keep_largest", label_bytes);
  SEGMI_CHECK_ARG(n > 0 && n < (1ll << 31), "cc_keep_largest: 0 < n < 2^31");
  SEGMI_CHECK_ARG(n_applied >= 0 && (n_applied == 0 || applied_host), "cc_keep_largest: bad applied labels");
  SEGMI_CHECK_ARG(num_components >= 1 && num_components <= kMaxKeep, "cc_keep_largest: num_components must be 1 .. %d", kMaxKeep);
  const CcLayout l = cc_layout(n);
  SEGMI_CHECK_ARG(ws_bytes >= l.lo, "cc_keep_largest: workspace of %zu bytes, %zu needed", ws_bytes, l.lo);
  hipStream_t st = (hipStream_t)stream;
  char* w8 = (char*)ws;
  KeepParams p{};
  p.lab = labels; p.root = root; p.size = size; p.n = n; p.out = out;
  p.applied = (const unsigned*)(w8 + l.applied);
  p.keys = (unsigned long long*)(w8 + l.keys);
  p.winners = (int32_t*)(w8 + l.winners);
  p.classes = independent ? (label_bytes == 1 ? 256 : kClassTable) : 1;
  p.independent = independent ? 1 : 0;
  p.rounds = num_components;
  if (cc_set_applied((unsigned*)(w8 + l.applied), applied_host, n_applied, st) ||
      hipMemsetAsync(p.keys, 0, (size_t)kClassTable * sizeof(unsigned long long), st) != hipSuccess) {
    set_error("cc_keep_largest: memset failed");
    return SEGMI_ELAUNCH;
  }
  const unsigned grid = (unsigned)cdiv64(n, 256);
  for (int r = 0; r < num_components; ++r) {
#define ROUND(T) hipLaunchKernelGGL(cc_keep_round_kernel<T>, grid, 256, 0, st, p, r)
    LV_BY_LABEL(label_bytes, ROUND);
#undef ROUND
    hipLaunchKernelGGL(cc_keep_pick_kernel, cdiv(p.classes, 256), 256, 0, st, p, r);
  }
#define APPLY(T) hipLaunchKernelGGL(cc_keep_apply_kernel<T>, grid, 256, 0, st, p)
  LV_BY_LABEL(label_bytes, APPLY);
#undef APPLY
  SEGMI_LAUNCH_CHECK("cc_keep_largest");
  return SEGMI_OK;
}

int segmi_cc_remove_small(const void* labels, int label_bytes, int64_t n, const int32_t* root, const int32_t* size,
                          int min_size, void* out, void* stream) {
  SEGMI_CHECK_ARG(labels && root && size && out, "cc_remove_small: null pointer");
  LV_CHECK_LABEL_BYTES("cc_remove_small", label_bytes);
  SEGMI_CHECK_ARG(n > 0 && n < (1ll << 31), "cc_remove_small: 0 < n < 2^31");
  SEGMI_CHECK_ARG(min_size >= 0, "cc_remove_small: min_size must be >= 0");
  hipStream_t st = (hipStream_t)stream;
#define SMALL(T) hipLaunchKernelGGL(cc_remove_small_kernel<T>, (unsigned)cdiv64(n, 256), 256, 0, st, (const T*)labels, root, size, n, min_size, (T*)out)
  LV_BY_LABEL(label_bytes, SMALL);
#undef SMALL
  SEGMI_LAUNCH_CHECK("cc_remove_small");
  return SEGMI_OK;
}

int segmi_cc_fill_holes(const void* labels, int label_bytes, int d, int h, int w, int spatial_dims, int connectivity,
                        const int32_t* root, const int32_t* applied_host, int n_applied, void* out, void* ws,
                        size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(labels && root && out && ws, "cc_fill_holes: null pointer");
  LV_CHECK_LABEL_BYTES("cc_fill_holes", label_bytes);
  LV_CHECK_SPATIAL_DIMS("cc_fill_holes", spatial_dims, d);
  LV_CHECK_VOXELS("cc_fill_holes", d, h, w);
  SEGMI_CHECK_ARG(connectivity >= 1 && connectivity <= spatial_dims, "cc_fill_holes: connectivity must be 1 .. %d", spatial_dims);
  SEGMI_CHECK_ARG(n_applied >= 0 && (n_applied == 0 || applied_host), "cc_fill_holes: bad applied labels");
  const int64_t n = (int64_t)d * h * w;
  const CcLayout l = cc_layout(n);
  SEGMI_CHECK_ARG(ws_bytes >= l.total, "cc_fill_holes: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
  hipStream_t st = (hipStream_t)stream;
  char* w8 = (char*)ws;
  FillParams p{};
  p.lab = labels; p.root = root; p.out = out;
  p.applied = (const unsigned*)(w8 + l.applied);
  p.lo = (int32_t*)(w8 + l.lo); p.hi = (int32_t*)(w8 + l.hi);
  p.d = d; p.h = h; p.w = w; p.sd = spatial_dims; p.conn = connectivity; p.all = n_applied == 0;
  if (cc_set_applied((unsigned*)(w8 + l.applied), applied_host, n_applied, st)) {
    set_error("cc_fill_holes: memset failed");
    return SEGMI_ELAUNCH;
  }
  const unsigned grid = (unsigned)cdiv64(n, 256);
#define FILL(T)                                                            \
  do {                                                                        \
    hipLaunchKernelGGL(cc_fill_init_kernel<T>, grid, 256, 0, st, p, n);       \
    hipLaunchKernelGGL(cc_fill_scan_kernel<T>, grid, 256, 0, st, p, n);       \
    hipLaunchKernelGGL(cc_fill_apply_kernel<T>, grid, 256, 0, st, p, n);      \
  } while (0)
  LV_BY_LABEL(label_bytes, FILL);
#undef FILL
  SEGMI_LAUNCH_CHECK("cc_fill_holes");
  return SEGMI_OK;
}

int segmi_map_labels(const void* in, int in_bytes, int64_t n, const int64_t* lut, int lut_len, void* out,
                     int out_bytes, void* stream) {
  SEGMI_CHECK_ARG(in && lut && out, "map_labels: null pointer");
  SEGMI_CHECK_ARG(in_bytes == 1 || in_bytes == 2 || in_bytes == 4 || in_bytes == 8, "map_labels: in_bytes must be 1, 2, 4 or 8");
  SEGMI_CHECK_ARG(out_bytes == 1 || out_bytes == 2 || out_bytes == 4 || out_bytes == 8, "map_labels: out_bytes must be 1, 2, 4 or 8");
  SEGMI_CHECK_ARG(n > 0 && lut_len > 0, "map_labels: empty input or table");
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)lv_grid(n, 256, 65536);
#define MAP(TI, TO) hipLaunchKernelGGL((map_labels_kernel<TI, TO>), grid, 256, 0, st, (const TI*)in, n, lut, lut_len, (TO*)out)
#define MAP_OUT(TI)                                \
  do {                                             \
    if (out_bytes == 1) MAP(TI, uint8_t);          \
    else if (out_bytes == 2) MAP(TI, int16_t);     \
    else if (out_bytes == 4) MAP(TI, int32_t);     \
    else MAP(TI, int64_t);                         \
  } while (0)
  if (in_bytes == 1) MAP_OUT(uint8_t);
  else if (in_bytes == 2) MAP_OUT(int16_t);
  else if (in_bytes == 4) MAP_OUT(int32_t);
  else MAP_OUT(int64_t);
#undef MAP_OUT
#undef MAP
  SEGMI_LAUNCH_CHECK("map_labels");
  return SEGMI_OK;
}

}  // extern "C"
