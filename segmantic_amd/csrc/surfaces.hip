// surfaces.hip -- label-surface extraction by discrete surface nets (reference
// scripts/visualize_label_surfaces.py, which hands the job to VTK's flying edges).  DESIGN.md section 14 holds
// the definitions; segmantic_amd/image/surfaces.py repeats them.  In short, for one label c:
//   P      = (L == c) padded by one layer of false; lattice point (k, j, i) is voxel (k-1, j-1, i-1).
//   cell   (k, j, i), 0 <= k <= d etc.: the 2x2x2 block P[k..k+1, j..j+1, i..i+1]; ACTIVE when mixed.
//   vertex one per active cell, numbered in raster order of the cells, at the mean of the midpoints of the
//          cell's crossing edges (offset o = s / 2n in [0,1]^3; index coordinate = (cell - 1) + o).
//   faces  one quad (two triangles) per crossing lattice edge, owned by the cell whose lowest corner is the
//          edge's lower end, in the order x-, y-, z-edge; normal from c to not-c.
//
// Work is restricted to each label's bounding box grown by one cell, cut into CHUNKS of 64 consecutive cells
// along x (chunk columns are aligned to multiples of 64 cells, so a neighbour cell's chunk is found by
// arithmetic).  All selected labels share every launch: a wave handles one chunk and finds its label by a
// binary search over the labels' first chunk numbers.
//   count   : corner tests from 2x2 rows of labels (the x-1 column comes from the lane below), ballots give
//             the chunk's 64-bit activity mask and its face count: {mask u64, vertices u32, faces u32} per
//             chunk, a quarter byte per cell, no per-cell index volume.
//   scan    : block sums / one workgroup over the partials / block-local scan, over both counts.
//   emit    : recomputes the corners; a cell's vertex number is its chunk's prefix plus the popcount of the
//             mask below its lane, the neighbour cells' numbers come the same way from their chunks.
//   relax   : Jacobi sweeps over the cell-local offsets through the [V][6] neighbour table emit wrote.
//   finish  : index coordinate -> physical coordinate in f64, rounded once.
//   measure : area and signed volume per label, f64 per-thread sums in a fixed order, a fixed-order workgroup
//             tree, and the workgroup that draws the last ticket folds the table (fin_tail.h protocol).
// Phases are separate launches: no grid-wide wait, no spin loop, no cooperative launch.  The file is compiled
// with -ffp-contract=off: positions are specified operation by operation.
#include "labelvol.h"
#include "reduce_fin.h"

namespace segmi {

constexpr int kSurfScan = 1024;        // chunks per workgroup of the scan passes (256 threads x 4)
constexpr int kSurfTableChunk = 32;    // label-table entries per upload launch
constexpr int kSurfMeasureWgs = 32;    // workgroups per label of the measure pass
constexpr int kSurfMaxLabels = 65535;

// cells z0 .. z0+nz-1, y0 .. y0+ny-1, chunk columns cx0 .. cx0+ncx-1 (cells 64*cx .. 64*cx+63)
struct SurfLabel { int c, z0, y0, cx0, nz, ny, ncx, base; };

struct SurfLayout { size_t table, mask, vpre, fpre, partials, total; int64_t chunks; };

// per-label boxes (host, half-open voxel boxes z0 z1 y0 y1 x0 x1; empty when z1 <= z0) -> table + layout
static int surf_layout(const int32_t* sel, const int32_t* boxes, int n_sel, int d, int h, int w, SurfLabel* table,
                       SurfLayout* out) {
  int64_t chunks = 0;
  for (int l = 0; l < n_sel; ++l) {
    const int32_t* b = boxes + 6 * l;
    SurfLabel e{};
    e.c = sel[l];
    if (e.c < 1 || e.c > 65535 || (l > 0 && sel[l] <= sel[l - 1])) return 1;
    if (chunks >= (1ll << 31)) return 2;
    e.base = (int)chunks;
    if (b[1] > b[0]) {
      if (b[0] < 0 || b[1] > d || b[2] < 0 || b[3] > h || b[3] <= b[2] || b[4] < 0 || b[5] > w || b[5] <= b[4]) return 1;
      e.z0 = b[0]; e.nz = b[1] - b[0] + 1;
      e.y0 = b[2]; e.ny = b[3] - b[2] + 1;
      e.cx0 = b[4] / 64; e.ncx = b[5] / 64 - e.cx0 + 1;
      chunks += (int64_t)e.nz * e.ny * e.ncx;
    }
    if (table) table[l] = e;
  }
  if (chunks >= (1ll << 31)) return 2;
  SurfLayout y{};
  LvCarver c;
  y.chunks = chunks;
  y.table = c.take((size_t)(n_sel + 1) * sizeof(SurfLabel));
  y.mask = c.take((size_t)(chunks + 1) * sizeof(unsigned long long));
  y.vpre = c.take((size_t)(chunks + 1) * sizeof(uint32_t));
  y.fpre = c.take((size_t)(chunks + 1) * sizeof(uint32_t));
  // the block sums of the scan, then the three words of its totals
  y.partials = c.take((size_t)(cdiv64(chunks, kSurfScan) + 2) * 2 * sizeof(uint32_t));
  y.total = c.off;
  *out = y;
  return 0;
}

struct SurfParams {
  const void* lab;
  int d, h, w, n_sel;
  int64_t chunks;
  const SurfLabel* table;
  unsigned long long* mask;
  uint32_t* vpre;     // counts after `count`, exclusive prefixes after `scan`; [chunks] holds the total
  uint32_t* fpre;
  // emit
  float* offs;        // [V][3] cell-local offsets (x, y, z)
  int32_t* cells;     // [V][3] cell (x, y, z)
  int32_t* nbr;       // [V][6] vertex numbers of the -x +x -y +y -z +z neighbours, -1 = none (nullable)
  int32_t* faces;     // [F][3], numbered within the label
  int64_t nv, nf;
};

// the label whose chunks hold chunk `ch`: the last entry with base <= ch that is not empty
__device__ __forceinline__ int surf_find_label(const SurfLabel* __restrict__ t, int n, int ch) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {                    // at most 16 rounds
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid].base <= ch) lo = mid; else hi = mid - 1;
  }
  return lo;                           // empty labels share their successor's base and sort before it
}

// corner bits of cell (k, j, i): bit (a*4 + b*2 + e) = P[k+a][j+b][i+e].  Called by every lane of the wave
// (the x-1 column is the lane below's x column); lane 0 reads its own.
template <typename T>
__device__ __forceinline__ unsigned surf_corners(const T* __restrict__ src, int d, int h, int w, int c, int k, int j,
                                                 int i, int lane) {
  unsigned hi = 0, lo0 = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int z = k + (r >> 1) - 1, y = j + (r & 1) - 1;
    if (z < 0 || z >= d || y < 0 || y >= h) continue;
    const int64_t row = ((int64_t)z * h + y) * w;
    if (i < w) hi |= (unsigned)((int)src[row + i] == c) << r;
    if (lane == 0 && i >= 1 && i - 1 < w) lo0 |= (unsigned)((int)src[row + i - 1] == c) << r;
  }
  unsigned lo = __shfl_up(hi, 1);
  if (lane == 0) lo = lo0;
  unsigned m = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) m |= (((lo >> r) & 1u) << (2 * r)) | (((hi >> r) & 1u) << (2 * r + 1));
  return m;
}

// crossing edges whose lower end is the cell's lowest corner: bit 0 x-edge, bit 1 y-edge, bit 2 z-edge
__device__ __forceinline__ unsigned surf_own_edges(unsigned m) {
  const unsigned c0 = m & 1u;
  return (c0 ^ ((m >> 1) & 1u)) | ((c0 ^ ((m >> 2) & 1u)) << 1) | ((c0 ^ ((m >> 4) & 1u)) << 2);
}

struct SurfChunk { int label, k, j, cx; };
__device__ __forceinline__ SurfChunk surf_chunk(const SurfParams& p, int ch, SurfLabel* e) {
  SurfChunk s;
  s.label = surf_find_label(p.table, p.n_sel, ch);
  *e = p.table[s.label];
  const int r = ch - e->base;
  s.cx = e->cx0 + r % e->ncx;
  const int row = r / e->ncx;
  s.j = e->y0 + row % e->ny;
  s.k = e->z0 + row / e->ny;
  return s;
}

// ---- count: one wave per chunk
template <typename T>
__global__ __launch_bounds__(256) void surf_count_kernel(SurfParams p) {
  const int64_t ch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ch >= p.chunks) return;          // whole waves leave
  const int lane = threadIdx.x & 63;
  SurfLabel e;
  const SurfChunk s = surf_chunk(p, (int)ch, &e);
  const unsigned m = surf_corners<T>((const T*)p.lab, p.d, p.h, p.w, e.c, s.k, s.j, s.cx * 64 + lane, lane);
  const unsigned own = surf_own_edges(m);
  const int nq = __popc(own);
  const unsigned long long act = __ballot(m != 0u && m != 0xffu);
  const int quads = __popcll(__ballot(nq & 1)) + 2 * __popcll(__ballot(nq & 2));
  if (lane == 0) {
    p.mask[ch] = act;
    p.vpre[ch] = (uint32_t)__popcll(act);
    p.fpre[ch] = (uint32_t)(2 * quads);
  }
}

// ---- scan over the chunk counts (vertices and faces together)
// partials[b] = (vertices, faces) of block b; the totals of the partials scan: totals[0..1] = the sums,
// totals[2] = 1 when a sum passed 2^31 - 1 (the host then refuses the volume)
__global__ __launch_bounds__(256) void surf_sum_kernel(const uint32_t* __restrict__ v, const uint32_t* __restrict__ f,
                                                       int64_t n, uint32_t* __restrict__ partials) {
  __shared__ u32x2 s[256];
  u32x2 t{};
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)blockIdx.x * kSurfScan + threadIdx.x * 4 + u;
    if (i < n) { t[0] += v[i]; t[1] += f[i]; }
  }
  lv_block_scan<256>(t, s);
  if (threadIdx.x == 255) { partials[2 * blockIdx.x] = s[255][0]; partials[2 * blockIdx.x + 1] = s[255][1]; }
}
__global__ __launch_bounds__(256) void surf_scan_apply_kernel(uint32_t* v, uint32_t* f, int64_t n,
                                                              const uint32_t* __restrict__ partials,
                                                              const uint32_t* __restrict__ totals) {
  __shared__ u32x2 s[256];
  uint32_t cv[4], cf[4];
  u32x2 t{};
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)blockIdx.x * kSurfScan + threadIdx.x * 4 + u;
    cv[u] = i < n ? v[i] : 0u; cf[u] = i < n ? f[i] : 0u;
    t[0] += cv[u]; t[1] += cf[u];
  }
  const u32x2 before = lv_block_scan<256>(t, s);
  uint32_t rv = partials[2 * blockIdx.x] + before[0], rf = partials[2 * blockIdx.x + 1] + before[1];
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)blockIdx.x * kSurfScan + threadIdx.x * 4 + u;
    if (i < n) { v[i] = rv; f[i] = rf; }
    rv += cv[u]; rf += cf[u];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { v[n] = totals[0]; f[n] = totals[1]; }
}
// starts i32 [n_sel + 1][2]: the first vertex and first face of every label in the concatenated outputs, then
// the totals; starts[n_sel + 1][0] = the overflow flag
__global__ void surf_starts_kernel(SurfParams p, const uint32_t* __restrict__ totals, int32_t* starts) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l > p.n_sel) return;
  const int64_t ch = l < p.n_sel ? p.table[l].base : p.chunks;
  starts[2 * l] = (int32_t)p.vpre[ch];
  starts[2 * l + 1] = (int32_t)p.fpre[ch];
  if (l == p.n_sel) { starts[2 * l + 2] = (int32_t)totals[2]; starts[2 * l + 3] = 0; }
}

// ---- emit
// vertex number (in the concatenated output) of cell (k, j, i) of label e, -1 when the cell is outside the
// label's chunks or not active
__device__ __forceinline__ int surf_vertex(const SurfParams& p, const SurfLabel& e, int k, int j, int i) {
  const int rk = k - e.z0, rj = j - e.y0, rc = (i >> 6) - e.cx0;
  if (i < 0 || rk < 0 || rk >= e.nz || rj < 0 || rj >= e.ny || rc < 0 || rc >= e.ncx) return -1;
  const int64_t ch = (int64_t)e.base + ((int64_t)rk * e.ny + rj) * e.ncx + rc;
  const unsigned long long m = p.mask[ch];
  const int ln = i & 63;
  if (!((m >> ln) & 1ull)) return -1;
  return (int)(p.vpre[ch] + (uint32_t)__popcll(m & ((1ull << ln) - 1ull)));
}

template <typename T>
__global__ __launch_bounds__(256) void surf_emit_kernel(SurfParams p) {
  const int64_t ch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ch >= p.chunks) return;
  const int lane = threadIdx.x & 63;
  SurfLabel e;
  const SurfChunk s = surf_chunk(p, (int)ch, &e);
  const int k = s.k, j = s.j, i = s.cx * 64 + lane;
  const unsigned m = surf_corners<T>((const T*)p.lab, p.d, p.h, p.w, e.c, k, j, i, lane);
  const unsigned own = surf_own_edges(m);
  const int nq = __popc(own);
  const bool active = m != 0u && m != 0xffu;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long act = __ballot(active);
  const int qbefore = __popcll(__ballot(nq & 1) & below) + 2 * __popcll(__ballot(nq & 2) & below);
  if (!active) return;
  const int64_t vn = (int64_t)p.vpre[ch] + __popcll(act & below);
  if (vn >= p.nv) return;                                   // never with the totals of the same count
  {
    // mean of the doubled midpoints of the crossing edges: integer sums (x, y, z) and the edge count
    int sx = 0, sy = 0, sz = 0, n = 0;
#define BIT(a, b, c) ((m >> ((a) * 4 + (b) * 2 + (c))) & 1u)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if (BIT(a, b, 0) != BIT(a, b, 1)) { sx += 1; sy += 2 * b; sz += 2 * a; ++n; }   // x-edge at (y = b, z = a)
        if (BIT(a, 0, b) != BIT(a, 1, b)) { sx += 2 * b; sy += 1; sz += 2 * a; ++n; }   // y-edge at (x = b, z = a)
        if (BIT(0, a, b) != BIT(1, a, b)) { sx += 2 * b; sy += 2 * a; sz += 1; ++n; }   // z-edge at (x = b, y = a)
      }
#undef BIT
    const float den = (float)(2 * n);
    p.offs[vn * 3 + 0] = (float)sx / den;
    p.offs[vn * 3 + 1] = (float)sy / den;
    p.offs[vn * 3 + 2] = (float)sz / den;
    p.cells[vn * 3 + 0] = i;
    p.cells[vn * 3 + 1] = j;
    p.cells[vn * 3 + 2] = k;
  }
  if (p.nbr) {
    // a face of the cell is shared with the neighbour when its four corners are mixed
    const unsigned fm[6] = {0x55u, 0xaau, 0x33u, 0xccu, 0x0fu, 0xf0u};
    const int dk[6] = {0, 0, 0, 0, -1, 1}, dj[6] = {0, 0, -1, 1, 0, 0}, di[6] = {-1, 1, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const unsigned f = m & fm[q];
      p.nbr[vn * 6 + q] = (f != 0u && f != fm[q]) ? surf_vertex(p, e, k + dk[q], j + dj[q], i + di[q]) : -1;
    }
  }
  if (!nq) return;
  const int vbase = (int)p.vpre[e.base];
  int64_t fo = (int64_t)p.fpre[ch] + 2 * qbefore;
  const int self = (int)vn - vbase;
  const bool low_set = m & 1u;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    if (!((own >> axis) & 1u)) continue;
    int q0, q1, q3;
    if (axis == 0) {          // cells around the x-edge: (y-,z-) (y+,z-) (y+,z+) (y-,z+)
      q0 = surf_vertex(p, e, k - 1, j - 1, i); q1 = surf_vertex(p, e, k - 1, j, i); q3 = surf_vertex(p, e, k, j - 1, i);
    } else if (axis == 1) {   // y-edge: (z-,x-) (z+,x-) (z+,x+) (z-,x+)
      q0 = surf_vertex(p, e, k - 1, j, i - 1); q1 = surf_vertex(p, e, k, j, i - 1); q3 = surf_vertex(p, e, k - 1, j, i);
    } else {                  // z-edge: (x-,y-) (x+,y-) (x+,y+) (x-,y+)
      q0 = surf_vertex(p, e, k, j - 1, i - 1); q1 = surf_vertex(p, e, k, j - 1, i); q3 = surf_vertex(p, e, k, j, i - 1);
    }
    q0 -= vbase; q1 -= vbase; q3 -= vbase;
    int c0 = q0, c1 = q1, c2 = self, c3 = q3;
    if (!low_set) { c0 = q3; c1 = self; c2 = q1; c3 = q0; }   // the cycle reversed
    if (fo + 2 <= p.nf) {
      int32_t* f = p.faces + fo * 3;
      f[0] = c0; f[1] = c1; f[2] = c2;
      f[3] = c0; f[4] = c2; f[5] = c3;
    }
    fo += 2;
  }
}

// ---- relax: one Jacobi sweep
__global__ __launch_bounds__(256) void surf_relax_kernel(const float* __restrict__ in, const int32_t* __restrict__ nbr,
                                                         int64_t nv, float lambda, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  float ax = 0.f, ay = 0.f, az = 0.f;
  int n = 0;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const int u = nbr[v * 6 + q];
    if (u < 0 || u >= nv) continue;
    const float s = (q & 1) ? 1.f : -1.f;
    ax += in[(int64_t)u * 3 + 0] + (q < 2 ? s : 0.f);
    ay += in[(int64_t)u * 3 + 1] + ((q >> 1) == 1 ? s : 0.f);
    az += in[(int64_t)u * 3 + 2] + (q >= 4 ? s : 0.f);
    ++n;
  }
  float o[3] = {in[v * 3 + 0], in[v * 3 + 1], in[v * 3 + 2]};
  if (n) {
    const float fn = (float)n;
    const float mm[3] = {ax / fn, ay / fn, az / fn};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float t = o[a] + lambda * (mm[a] - o[a]);
      o[a] = fminf(fmaxf(t, 0.f), 1.f);
    }
  }
  out[v * 3 + 0] = o[0]; out[v * 3 + 1] = o[1]; out[v * 3 + 2] = o[2];
}

struct SurfGeom { double origin[3], dir[9], spacing[3]; };   // (x, y, z), direction row-major
__global__ __launch_bounds__(256) void surf_finish_kernel(const float* __restrict__ offs, const int32_t* __restrict__ cells,
                                                          int64_t nv, SurfGeom g, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  double s[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float idx = (float)(cells[v * 3 + a] - 1) + offs[v * 3 + a];   // the index coordinate, one f32 rounding
    s[a] = g.spacing[a] * (double)idx;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    out[v * 3 + a] = (float)(g.origin[a] + ((g.dir[3 * a] * s[0] + g.dir[3 * a + 1] * s[1]) + g.dir[3 * a + 2] * s[2]));
}

// ---- measure: grid (kSurfMeasureWgs, n_sel)
__device__ __forceinline__ void surf_st(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double surf_ld(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ __launch_bounds__(256) void surf_measure_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                           const int32_t* __restrict__ starts, int n_sel,
                                                           double* partials, unsigned ticket, double* out) {
  __shared__ double s_a[256], s_v[256];
  __shared__ int s_last;
  const int l = blockIdx.y, tid = threadIdx.x;
  const int64_t v0 = starts[2 * l], v1 = starts[2 * l + 2], f0 = starts[2 * l + 1], f1 = starts[2 * l + 3];
  const float* vp = verts + v0 * 3;
  const int64_t nv = v1 - v0;
  double area = 0.0, vol = 0.0;
  for (int64_t f = f0 + (int64_t)blockIdx.x * 256 + tid; f < f1; f += (int64_t)kSurfMeasureWgs * 256) {
    const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) continue;
    const double ax = vp[(int64_t)a * 3], ay = vp[(int64_t)a * 3 + 1], az = vp[(int64_t)a * 3 + 2];
    const double bx = vp[(int64_t)b * 3], by = vp[(int64_t)b * 3 + 1], bz = vp[(int64_t)b * 3 + 2];
    const double cx = vp[(int64_t)c * 3], cy = vp[(int64_t)c * 3 + 1], cz = vp[(int64_t)c * 3 + 2];
    // signed volume term p0 . (p1 x p2)
    vol += (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx);
    const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    area += sqrt((nx * nx + ny * ny) + nz * nz);
  }
  s_a[tid] = area; s_v[tid] = vol;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { s_a[tid] += s_a[tid + o]; s_v[tid] += s_v[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    surf_st(partials + ((int64_t)l * kSurfMeasureWgs + blockIdx.x) * 2, s_a[0]);
    surf_st(partials + ((int64_t)l * kSurfMeasureWgs + blockIdx.x) * 2 + 1, s_v[0]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned prev = __hip_atomic_fetch_add(&g_fin_tickets[ticket], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x * gridDim.y - 1;
    if (s_last) __hip_atomic_store(&g_fin_tickets[ticket], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  for (int q = tid; q < n_sel; q += 256) {
    double a = 0.0, v = 0.0;
    for (int b = 0; b < kSurfMeasureWgs; ++b) {
      a += surf_ld(partials + ((int64_t)q * kSurfMeasureWgs + b) * 2);
      v += surf_ld(partials + ((int64_t)q * kSurfMeasureWgs + b) * 2 + 1);
    }
    out[2 * q] = 0.5 * a;
    out[2 * q + 1] = v / 6.0;
  }
}

// ---- boxes of the selected labels: sel i32 [n_sel] ascending (device); boxes i32 [n_sel][6] inclusive
// (min z, max z, min y, max y, min x, max x), started at (INT_MAX, -1).  Per 64-voxel chunk the distinct values
// are walked with ballots; a box word is touched only when the chunk moves it.
__global__ void surf_boxes_init_kernel(int32_t* boxes, int n_sel) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_sel) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) { boxes[l * 6 + 2 * a] = 0x7fffffff; boxes[l * 6 + 2 * a + 1] = -1; }
}
template <typename T>
__global__ __launch_bounds__(256) void surf_boxes_kernel(const T* __restrict__ src, int d, int h, int w,
                                                         const int32_t* __restrict__ sel, int n_sel, int32_t* boxes) {
  const int lane = threadIdx.x & 63;
  const int64_t rows = (int64_t)d * h, nwaves = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nwaves) {
    const int z = (int)(r / h), y = (int)(r % h);
    for (int x0 = 0; x0 < w; x0 += 64) {
      const int x = x0 + lane;
      const int v = x < w ? (int)src[r * w + x] : 0;
      unsigned long long todo = __ballot(v > 0);
      while (todo) {                     // every round clears at least the leading bit
        const int lead = __ffsll((long long)todo) - 1;
        const int c = __shfl(v, lead);
        const unsigned long long mm = __ballot(v == c);
        todo &= ~mm;
        if (lane != lead) continue;
        int lo = 0, hi = n_sel - 1, at = -1;
        while (lo <= hi) {
          const int mid = (lo + hi) >> 1, sv = sel[mid];
          if (sv == c) { at = mid; break; }
          if (sv < c) lo = mid + 1; else hi = mid - 1;
        }
        if (at < 0) continue;
        int32_t* b = boxes + at * 6;
        const int xl = x0 + __ffsll((long long)mm) - 1, xh = x0 + 63 - __clzll((long long)mm);
        if (z < __hip_atomic_load(b + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(b + 0, z);
        if (z > __hip_atomic_load(b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(b + 1, z);
        if (y < __hip_atomic_load(b + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(b + 2, y);
        if (y > __hip_atomic_load(b + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(b + 3, y);
        if (xl < __hip_atomic_load(b + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(b + 4, xl);
        if (xh > __hip_atomic_load(b + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(b + 5, xh);
      }
    }
  }
}
// inclusive maxima -> half-open; an absent label gets the empty box 0 0 0 0 0 0
__global__ void surf_boxes_fin_kernel(int32_t* boxes, int n_sel) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_sel) return;
  const bool empty = boxes[l * 6 + 1] < 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    boxes[l * 6 + 2 * a] = empty ? 0 : boxes[l * 6 + 2 * a];
    boxes[l * 6 + 2 * a + 1] = empty ? 0 : boxes[l * 6 + 2 * a + 1] + 1;
  }
}

}  // namespace segmi

using namespace segmi;

#define SURF_COMMON_ARGS(what)                                                                                   \
  LV_CHECK_LABEL_BYTES(what, label_bytes);                                                                       \
  LV_CHECK_CELLS(what, d, h, w);                                                                                 \
  SEGMI_CHECK_ARG(n_sel >= 1 && n_sel <= kSurfMaxLabels, what ": 1 .. %d selected labels", kSurfMaxLabels)

extern "C" {

int segmi_surface_boxes(const void* labels, int label_bytes, int d, int h, int w, const int32_t* selected, int n_sel,
                        int32_t* boxes, void* stream) {
  SEGMI_CHECK_ARG(labels && selected && boxes, "surface_boxes: null pointer");
  SURF_COMMON_ARGS("surface_boxes");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(surf_boxes_init_kernel, cdiv(n_sel, 256), 256, 0, st, boxes, n_sel);
  const int64_t rows = (int64_t)d * h;
  const int grid = lv_grid(rows, 4, 4096);
#define BOXES(T) hipLaunchKernelGGL(surf_boxes_kernel<T>, grid, 256, 0, st, (const T*)labels, d, h, w, selected, n_sel, boxes)
  LV_BY_LABEL(label_bytes, BOXES);
#undef BOXES
  hipLaunchKernelGGL(surf_boxes_fin_kernel, cdiv(n_sel, 256), 256, 0, st, boxes, n_sel);
  SEGMI_LAUNCH_CHECK("surface_boxes");
  return SEGMI_OK;
}

int64_t segmi_surface_workspace_bytes(int d, int h, int w, const int32_t* selected_host, const int32_t* boxes_host,
                                      int n_sel) {
  if (!lv_cells_ok(d, h, w) || !selected_host || !boxes_host || n_sel < 1 || n_sel > kSurfMaxLabels) return 0;
  SurfLayout y;
  if (surf_layout(selected_host, boxes_host, n_sel, d, h, w, nullptr, &y)) return 0;
  return (int64_t)y.total;
}

static int surf_params(const char* what, const void* labels, int d, int h, int w, const int32_t* selected_host,
                       const int32_t* boxes_host, int n_sel, void* ws, size_t ws_bytes, SurfLabel* table,
                       SurfLayout* y, SurfParams* p) {
  const int bad = surf_layout(selected_host, boxes_host, n_sel, d, h, w, table, y);
  if (bad == 1) { set_error("%s: selected labels must ascend within 1 .. 65535 and boxes lie inside the volume", what); return SEGMI_EINVAL; }
  if (bad == 2) { set_error("%s: the label boxes hold 2^31 chunks or more", what); return SEGMI_EINVAL; }
  if (ws_bytes < y->total) { set_error("%s: workspace of %zu bytes, %zu needed", what, ws_bytes, y->total); return SEGMI_EINVAL; }
  char* w8 = (char*)ws;
  *p = SurfParams{};
  p->lab = labels; p->d = d; p->h = h; p->w = w; p->n_sel = n_sel; p->chunks = y->chunks;
  p->table = (const SurfLabel*)(w8 + y->table);
  p->mask = (unsigned long long*)(w8 + y->mask);
  p->vpre = (uint32_t*)(w8 + y->vpre);
  p->fpre = (uint32_t*)(w8 + y->fpre);
  return SEGMI_OK;
}

int segmi_surface_count(const void* labels, int label_bytes, int d, int h, int w, const int32_t* selected_host,
                        const int32_t* boxes_host, int n_sel, int32_t* starts, void* ws, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(labels && selected_host && boxes_host && starts && ws, "surface_count: null pointer");
  SURF_COMMON_ARGS("surface_count");
  SurfLabel* table = new SurfLabel[n_sel];
  SurfLayout y;
  SurfParams p;
  const int rc = surf_params("surface_count", labels, d, h, w, selected_host, boxes_host, n_sel, ws, ws_bytes, table, &y, &p);
  if (rc != SEGMI_OK) { delete[] table; return rc; }
  hipStream_t st = (hipStream_t)stream;
  char* w8 = (char*)ws;
  lv_upload_table<kSurfTableChunk>((const SurfLabel*)table, n_sel, LvStore<SurfLabel>{(SurfLabel*)(w8 + y.table)}, st);
  delete[] table;
  uint32_t* partials = (uint32_t*)(w8 + y.partials);
  const int64_t nb = cdiv64(y.chunks, kSurfScan);
  uint32_t* totals = partials + 2 * nb;
  if (y.chunks > 0) {
#define COUNT(T) hipLaunchKernelGGL(surf_count_kernel<T>, (unsigned)cdiv64(y.chunks, 4), 256, 0, st, p)
    LV_BY_LABEL(label_bytes, COUNT);
#undef COUNT
    hipLaunchKernelGGL(surf_sum_kernel, (unsigned)nb, 256, 0, st, (const uint32_t*)p.vpre, (const uint32_t*)p.fpre, y.chunks, partials);
  }
  hipLaunchKernelGGL(lv_scan_partials_kernel<2>, 1, 1024, 0, st, partials, nb, (uint32_t*)nullptr, totals + 2);
  // with no chunk at all the apply kernel still writes the (zero) totals behind the empty arrays
  hipLaunchKernelGGL(surf_scan_apply_kernel, (unsigned)(nb > 0 ? nb : 1), 256, 0, st, p.vpre, p.fpre, y.chunks,
                     (const uint32_t*)partials, (const uint32_t*)totals);
  hipLaunchKernelGGL(surf_starts_kernel, cdiv(n_sel + 1, 256), 256, 0, st, p, (const uint32_t*)totals, starts);
  SEGMI_LAUNCH_CHECK("surface_count");
  return SEGMI_OK;
}

int segmi_surface_emit(const void* labels, int label_bytes, int d, int h, int w, const int32_t* selected_host,
                       const int32_t* boxes_host, int n_sel, int64_t n_vertices, int64_t n_faces, float* offsets,
                       int32_t* cells, int32_t* neighbours, int32_t* faces, void* ws, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(labels && selected_host && boxes_host && ws, "surface_emit: null pointer");
  SURF_COMMON_ARGS("surface_emit");
  SEGMI_CHECK_ARG(n_vertices >= 0 && n_vertices < (1ll << 31) && n_faces >= 0 && n_faces < (1ll << 31),
                  "surface_emit: vertex / face counts must lie in 0 .. 2^31 - 1");
  SEGMI_CHECK_ARG((n_vertices == 0 || (offsets && cells)) && (n_faces == 0 || faces), "surface_emit: null output");
  SurfLayout y;
  SurfParams p;
  const int rc = surf_params("surface_emit", labels, d, h, w, selected_host, boxes_host, n_sel, ws, ws_bytes, nullptr, &y, &p);
  if (rc != SEGMI_OK) return rc;
  if (y.chunks == 0 || n_vertices == 0) return SEGMI_OK;
  p.offs = offsets; p.cells = cells; p.nbr = neighbours; p.faces = faces; p.nv = n_vertices; p.nf = n_faces;
  hipStream_t st = (hipStream_t)stream;
#define EMIT(T) hipLaunchKernelGGL(surf_emit_kernel<T>, (unsigned)cdiv64(y.chunks, 4), 256, 0, st, p)
  LV_BY_LABEL(label_bytes, EMIT);
#undef EMIT
  SEGMI_LAUNCH_CHECK("surface_emit");
  return SEGMI_OK;
}

int segmi_surface_relax(float* offsets, float* scratch, const int32_t* cells, const int32_t* neighbours,
                        int64_t n_vertices, int iterations, float relaxation, const double* geometry_host,
                        float* vertices, void* stream) {
  SEGMI_CHECK_ARG(n_vertices >= 0 && n_vertices < (1ll << 31), "surface_relax: 0 <= n_vertices < 2^31");
  SEGMI_CHECK_ARG(iterations >= 0, "surface_relax: iterations must be >= 0");
  SEGMI_CHECK_ARG(relaxation >= 0.f && relaxation <= 1.f, "surface_relax: relaxation must lie in [0, 1]");
  SEGMI_CHECK_ARG(geometry_host, "surface_relax: null geometry");
  if (n_vertices == 0) return SEGMI_OK;
  SEGMI_CHECK_ARG(offsets && cells && vertices, "surface_relax: null pointer");
  SEGMI_CHECK_ARG(iterations == 0 || (scratch && neighbours), "surface_relax: sweeps need the scratch and the neighbour table");
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)cdiv64(n_vertices, 256);
  float *a = offsets, *b = scratch;
  for (int t = 0; t < iterations; ++t) {
    hipLaunchKernelGGL(surf_relax_kernel, grid, 256, 0, st, (const float*)a, neighbours, n_vertices, relaxation, b);
    float* s = a; a = b; b = s;
  }
  SurfGeom g;
  for (int i = 0; i < 3; ++i) { g.origin[i] = geometry_host[i]; g.spacing[i] = geometry_host[12 + i]; }
  for (int i = 0; i < 9; ++i) g.dir[i] = geometry_host[3 + i];
  hipLaunchKernelGGL(surf_finish_kernel, grid, 256, 0, st, (const float*)a, cells, n_vertices, g, vertices);
  SEGMI_LAUNCH_CHECK("surface_relax");
  return SEGMI_OK;
}

int segmi_surface_measure(const float* vertices, const int32_t* faces, const int32_t* starts, int n_sel,
                          double* measures, void* ws, size_t ws_bytes, void* stream) {
  SEGMI_CHECK_ARG(starts && measures && ws, "surface_measure: null pointer");
  SEGMI_CHECK_ARG(n_sel >= 1 && n_sel <= kSurfMaxLabels, "surface_measure: 1 .. %d selected labels", kSurfMaxLabels);
  const size_t need = lv_align256((size_t)n_sel * kSurfMeasureWgs * 2 * sizeof(double));
  SEGMI_CHECK_ARG(ws_bytes >= need, "surface_measure: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const unsigned ticket = g_fin_next.fetch_add(1) % kFinTickets;
  hipLaunchKernelGGL(surf_measure_kernel, dim3(kSurfMeasureWgs, n_sel), 256, 0, st, vertices, faces, starts, n_sel,
                     (double*)ws, ticket, measures);
  SEGMI_LAUNCH_CHECK("surface_measure");
  return SEGMI_OK;
}

}  // extern "C"
