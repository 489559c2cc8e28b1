// conv_plan.h -- the host-side launch decisions of the convolution family (kernel family, channel chunk, output tiles
// per workgroup, tile shape, z-split, grid), each made once: conv_plan() / convt_plan() / wgrad_plan() make them from
// what the public queries receive.  The queries (statistics rows, kernel name, fusion capabilities, workspace size)
// READ a plan; the launchers CONSUME the same plan and refuse a grid that differs from it -- so a table the engine
// sized from a query is the table the kernel writes.  Host code only: no kernel, no __device__ function.
#pragma once
#include "common.h"

namespace segmi {

int bn_stats_rows_for(const segmi_act* x);   // norm_act.hip: rows of the generic statistics pass
// CUs the weight-gradient kernels size their grids for (the `cus` argument of segmi_conv3d_wgrad and of its
// workspace query; SEGMI_WGRAD_CUS overrides; wgrad.hip).  These
// kernels hold a CU exclusively (one 768-thread or 400-register workgroup per CU), so with one workgroup on
// EVERY CU the dependent chain of the main stream gets no CU until they retire; sized for half the chip the two
// streams really run side by side (5.55 -> 5.28 ms per training step, round 3).
int wgrad_cus(int cus);

// ------------------------------------------------------------------ thresholds, each written once
// workgroups that keep the chip busy (256 CUs x 2): a choice that shares work inside a workgroup (more output tiles
// per workgroup, fewer z-segments) is taken only while at least this many workgroups remain
constexpr int kFillWgs = 512;
// ... and a ring launch of fewer columns x segments than this leaves CUs idle: the tile kernels take the layer
constexpr int kRingMinWgs = 256;
// 32-bit offsets inside the kernels: one sample (or plane) of an operand below 2^31
constexpr int64_t kOffsetLimit = 1ll << 31;
// a wide output row takes the 16-voxel tiles, a narrow one (deep levels) the 8-voxel tiles
constexpr bool wide_row(int w) { return w > 8; }

struct Tile3 { int td, th, tw; };
// tile kernel (conv_fwd_impl.h): big tile when the output row is wide, small otherwise
constexpr Tile3 conv_tile_shape(int stride, bool wide) {
  return stride == 1 ? (wide ? Tile3{4, 8, 16} : Tile3{4, 4, 8}) : (wide ? Tile3{2, 4, 16} : Tile3{2, 4, 8});
}
// k-split kernel (conv_ks_impl.h): 128 output voxels (8 voxel tiles) per workgroup
constexpr Tile3 conv_ks_tile_shape(bool wide) { return wide ? Tile3{2, 4, 16} : Tile3{4, 4, 8}; }
// ring kernels: a column of 8 x 16 voxels marched in steps of 4 planes; the small-Cin kernel's tile
constexpr Tile3 kRingTile{4, 8, 16}, kSmallFwdTile{4, 8, 16};
// transposed tile kernel (convt_fwd_impl.h), in INPUT voxels; the persistent kernel's tile (convt_ps_impl.h)
constexpr Tile3 convt_tile_shape(bool wide) { return wide ? Tile3{2, 2, 16} : Tile3{2, 4, 8}; }
constexpr Tile3 kConvTPsTile{2, 2, 16};
constexpr int kCtPsMaxTiles = 16;     // persistent transposed kernel: tiles per workgroup (upper bound)
constexpr int kCtPsTargetWgs = 1024;  // ... and workgroups wanted before tiles are grouped

static inline int64_t tile_count(const Tile3& t, int n, int d, int h, int w, int* tz, int* ty, int* tx) {
  *tz = cdiv(d, t.td); *ty = cdiv(h, t.th); *tx = cdiv(w, t.tw);
  return (int64_t)n * *tz * *ty * *tx;
}
static inline int64_t tile_count(const Tile3& t, const segmi_act* a) {
  int tz, ty, tx;
  return tile_count(t, a->n, a->d, a->h, a->w, &tz, &ty, &tx);
}
// grid.x of `count` workgroups; 0 (no launch: the launchers refuse it) past the 2^31 a grid index holds
static inline int grid_of(int64_t count) { return count < kOffsetLimit ? (int)count : 0; }

static inline bool mfma_ok(int cin, int cout) { return cin % 16 == 0 && cout % 16 == 0; }
// layers of the first-layer kernels (conv_small.hip)
static inline bool conv_small_ok(int cin, int cout, int ksize) {
  return ksize == 3 && cin >= 1 && cin <= 4 && (cout == 16 || cout == 32);
}

// ------------------------------------------------------------------ forward convolution
enum ConvFamily { kConvRing3, kConvRing2, kConvKSplit, kConvTile, kConvSmallCin, kConvDirect };

struct ConvPlan {
  int family;
  int ck;                  // input channels staged per chunk
  int nt;                  // 16-channel output tiles per workgroup
  int td, th, tw;          // output tile of a workgroup (ring: of one z-step)
  int tz, ty, tx, zsplit;  // tiles along z / y / x; ring: z-segments a column is cut into (= tz)
  int grid_x, grid_y;      // grid_x = statistics rows the launch writes
  bool in_affine;          // takes segmi_in_affine (the ring kernels)
  bool bn_bwd_sums;        // takes segmi_bn_bwd_sums (the ring kernels' MODE 4: 16 -> 16 and 32 -> 32)
  bool split_act;          // takes segmi_conv3d_fwd_split_act (the tile kernel, k3 stride 2)
};

// Ring plan: columns = N * ceil(H/8) * ceil(W/16); each column is cut into `zsplit` z-segments so that
// >= ~512 workgroups exist, as long as every segment keeps >= 4 steps (else the 2-plane prologue
// overhead and the lost pipelining make the tile-at-a-time kernel the better choice).
// Returns zsplit, or 0 when the ring kernel should not be used.
static inline int conv_ring_zsplit(int dtype, int cin, int ksize, int stride, const segmi_act* out) {
  if (!(ksize == 3 && stride == 1 && cin == pick_ck(dtype, cin) && wide_row(out->w) && dtype_h16(dtype))) return 0;
  // the kernel addresses one sample with 32-bit "plane index x plane size" products (bytes for the
  // input, elements for the others); rows may be strided views (ld up to 4 x cin in this engine: skip
  // buffers, padded class axis).  Larger samples take the tile / K-split kernels (64-bit addressing).
  if ((int64_t)(out->d + 8) * out->h * out->w * (4 * cin) * 2 >= kOffsetLimit) return 0;
  const int columns = out->n * cdiv(out->h, kRingTile.th) * cdiv(out->w, kRingTile.tw);
  const int steps = cdiv(out->d, kRingTile.td);
  int zs = kFillWgs / columns;
  if (zs < 1) zs = 1;
  if (zs > steps / 4) zs = steps / 4;
  return zs < 1 || columns * zs < kRingMinWgs ? 0 : zs;
}
// ring3 (conv_ring3_impl.h: LDS-DMA staging) takes a ring layer when it has 16 input channels, 16-byte aligned
// input and output rows, and every operand sample stays below 2^31 BYTES (its out-of-range marker 2^31 + a plane offset must
// not wrap); ring2 takes the others (top conv inside the training step: 0.295 ms on ring3, 0.313 on ring2).
// ldr / ldbx: row strides of the residual and of the BatchNorm-backward input (0 = absent)
static inline bool conv_ring3_shape_ok(const segmi_act* in, const segmi_act* out, int ldr, int ldbx) {
  if (in->c != 16 || out->c % 16 != 0) return false;
  const int64_t isample = (int64_t)(in->d + 8) * in->h * in->w, osample = (int64_t)(out->d + 4) * out->h * out->w;
  return isample * in->ld * 2 < kOffsetLimit && osample * out->ld * 2 < kOffsetLimit &&
         osample * (ldr > 0 ? ldr : 1) * 2 < kOffsetLimit && osample * (ldbx > 0 ? ldbx : 1) * 2 < kOffsetLimit &&
         ((uintptr_t)in->data % 16) == 0 && in->ld % 8 == 0 &&
         ((uintptr_t)out->data % 16) == 0 && out->ld % 8 == 0;          // 16-byte DMA pieces and 16-byte stores
}
// Layers the k-split kernel takes: k3 s1 with at least one channel chunk (single-chunk layers
// included) of one-k-step-per-tap width.  Measured with cold caches (scripts/conv_microbench.py,
// batch 8): 128->128 @16^3 99 -> 56 us, 256->256 @8^3 60 -> 36 us, 256->128 @16^3 181 -> 98 us, 64->64 @32^3 119 -> 114 us;
// stride 2 does not gain (86 -> 97 us) and stays on conv_fwd_impl.h.
static inline bool conv_ks_ok(int dtype, int cin, int ksize, int stride) {
  const int ck = pick_ck(dtype, cin), spt = ck / (dtype == SEGMI_F32 ? 4 : 8);
  return ksize == 3 && stride == 1 && spt == 4 && cin >= ck;
}

// The plan of segmi_conv3d_fwd(dtype, in, out, ksize, stride).  ldr / ldbx (row strides of the residual and of the
// BatchNorm-backward input) only move a ring layer between ring3 and ring2, never grid_x or a capability: the
// queries pass out->ld for both, the launch its real strides.
static inline ConvPlan conv_plan(int dtype, const segmi_act* in, const segmi_act* out, int ksize, int stride, int ldr,
                                 int ldbx) {
  ConvPlan pl{};
  const bool wide = wide_row(out->w);
  const int ntiles = out->c / 16;
  pl.ck = pick_ck(dtype, in->c);
  pl.nt = pl.grid_y = 1;
  Tile3 t;
  if (!mfma_ok(in->c, out->c)) {
    // the first-layer kernel needs 4-element aligned output rows; everything else runs the direct kernel, whose
    // statistics are a separate pass over the written output
    pl.family = conv_small_ok(in->c, out->c, ksize) && out->ld % 4 == 0 &&
                ((uintptr_t)out->data % (4 * dtype_size(dtype))) == 0 ? kConvSmallCin : kConvDirect;
    if (pl.family == kConvDirect) { pl.grid_x = bn_stats_rows_for(out); return pl; }
    t = kSmallFwdTile;
  } else if ((pl.zsplit = conv_ring_zsplit(dtype, in->c, ksize, stride, out)) > 0) {
    pl.family = conv_ring3_shape_ok(in, out, ldr, ldbx) ? kConvRing3 : kConvRing2;
    // ring2 of 32-channel chunks: two output tiles share the staged planes when the output channels allow it
    if (pl.family == kConvRing2 && pl.ck == 32 && ntiles % 2 == 0) pl.nt = 2;
    t = kRingTile;
    pl.in_affine = true;
    pl.bn_bwd_sums = (in->c == 16 && out->c == 16) || (in->c == 32 && out->c == 32);
  } else if (conv_ks_ok(dtype, in->c, ksize, stride)) {
    pl.family = kConvKSplit;
    t = conv_ks_tile_shape(wide);
  } else {
    pl.family = kConvTile;
    t = conv_tile_shape(stride, wide);
    pl.split_act = ksize == 3 && stride == 2;
  }
  pl.td = t.td; pl.th = t.th; pl.tw = t.tw;
  int64_t wgs = tile_count(t, out->n, pl.zsplit ? t.td : out->d, out->h, out->w, &pl.tz, &pl.ty, &pl.tx);
  if (pl.zsplit) { pl.tz = pl.zsplit; wgs *= pl.zsplit; }
  pl.grid_x = grid_of(wgs);
  if (pl.family == kConvKSplit) {
    // two output tiles per workgroup (input fragment reuse) unless that leaves the chip unfilled
    if (ntiles % 2 == 0 && wgs * (ntiles / 2) >= kFillWgs) pl.nt = 2;
  } else if (pl.family == kConvTile) {
    // output-channel tiles per workgroup: as many as divide Cout (input tile reuse), but fewer
    // when the launch would not fill the chip (deep levels: 8^3 .. 16^3 voxels)
    pl.nt = ntiles % 4 == 0 ? 4 : (ntiles % 2 == 0 ? 2 : 1);
    while (pl.nt > 1 && wgs * (ntiles / pl.nt) < kFillWgs) pl.nt /= 2;
  }
  pl.grid_y = ntiles / pl.nt;
  return pl;
}

// MODE of a ring launch: 1 = PReLU, 2 = statistics, 4 = BatchNorm-backward sums in an input-gradient launch
// (neither PReLU nor statistics).  MODE 4 runs one 16-channel output tile per workgroup, 32 -> 32 as two tiles on
// grid.y (BASELINE config 4's full-resolution layers, round 4): with both tiles in one workgroup (NT = 2: 216 weight
// registers + the sums) the variant spills 96 registers and the step got slower.
static inline int conv_ring_mode(const ConvPlan& pl, bool sums, bool prelu, bool stats) {
  return pl.bn_bwd_sums && sums && !prelu && !stats ? 4 : (prelu ? 1 : 0) | (stats ? 2 : 0);
}

static inline const char* conv_plan_name(const ConvPlan& pl, int dtype, int ksize, int stride, char* buf, size_t n) {
  const char* dt = dtype_name(dtype);
  switch (pl.family) {
    case kConvRing3: snprintf(buf, n, "conv_ring3_kernel<%s, CK=16> (LDS-DMA ring)", dt); break;
    case kConvRing2: snprintf(buf, n, "conv_ring2_kernel<%s, CK=%d, NT=%d>", dt, pl.ck, pl.nt); break;
    case kConvKSplit: snprintf(buf, n, "conv_fwd_ks_kernel<%s, k%d s%d>", dt, ksize, stride); break;
    case kConvTile: snprintf(buf, n, "conv_fwd_mfma_kernel<%s, CK=%d, k%d s%d>", dt, pl.ck, ksize, stride); break;
    case kConvSmallCin: snprintf(buf, n, "conv_small_fwd_kernel<%s>", dt); break;
    default: snprintf(buf, n, "conv_direct_kernel<%s>", dt);
  }
  return buf;
}

// ------------------------------------------------------------------ transposed convolution (k3 s2 p1)
enum ConvTFamily { kConvTPersistent, kConvTTile, kConvTDirect };

struct ConvTPlan {
  int family;
  int ck, nt;              // channel chunk, 16-channel output tiles per workgroup
  int td, th, tw, tz, ty, tx;   // tile, in input voxels; tiles along z / y / x
  int64_t tiles;
  int tiles_per_wg;        // persistent kernel: consecutive tiles one workgroup walks
  int grid_x, grid_y;      // grid_x = statistics rows the launch writes
};

static inline ConvTPlan convt_plan(int dtype, const segmi_act* in, const segmi_act* out) {
  ConvTPlan pl{};
  pl.nt = pl.tiles_per_wg = pl.grid_y = 1;
  if (!mfma_ok(in->c, out->c)) { pl.family = kConvTDirect; pl.grid_x = bn_stats_rows_for(out); return pl; }
  // the persistent kernel takes the wide, few-channel layers: every weight fragment of the layer in LDS
  const int psck = dtype == SEGMI_F32 ? 16 : 32;
  const int nch = in->c / psck, ntiles = out->c / 16;
  const bool ps = in->c % psck == 0 && in->w >= 16 &&
                  ((ntiles == 1 && nch <= 2) || (ntiles == 2 && nch == 1 && dtype_h16(dtype)));
  pl.family = ps ? kConvTPersistent : kConvTTile;
  pl.ck = ps ? psck : pick_ck(dtype, in->c);
  pl.nt = ps ? ntiles : (ntiles % 2 == 0 ? 2 : 1);
  const Tile3 t = ps ? kConvTPsTile : convt_tile_shape(wide_row(in->w));
  pl.td = t.td; pl.th = t.th; pl.tw = t.tw;
  pl.tiles = tile_count(t, in->n, in->d, in->h, in->w, &pl.tz, &pl.ty, &pl.tx);
  if (ps) {
    const int64_t per = pl.tiles / kCtPsTargetWgs;
    pl.tiles_per_wg = per < 1 ? 1 : (per > kCtPsMaxTiles ? kCtPsMaxTiles : (int)per);
    pl.grid_x = grid_of(cdiv64(pl.tiles, pl.tiles_per_wg));
  } else {
    pl.grid_x = grid_of(pl.tiles);
    pl.grid_y = ntiles / pl.nt;
  }
  return pl;
}

// ------------------------------------------------------------------ weight gradient
enum WgradPath { kWgradWaveSpecialised, kWgradMfma, kWgradSmallCin, kWgradDirect };

struct WgradPlan {
  int path;
  int ct;                  // channel blocking of one workgroup, 10 * CTO + CTI (16-channel tiles of dY x of X)
  int td, th, tw;          // dY tile
  int gx;                  // voxel-range workgroups (= partial slabs) of one launch
  int parts;               // launches the batch is cut into (operands past the 4 GiB of a buffer descriptor)
  int slabs;               // parts * gx: what the workspace holds and the reduction folds
};

// channel blocking, bf16 / fp16 only: 2 output tiles share one staging of X when the output channels allow it (4x1
// measured slower: 360 VGPRs).  Layers with >= 32 input and output channels took the 2 x 2 tile
// (220 VGPRs, one workgroup per CU) until round 4; with the 2 x 1 tile (the wave-specialised kernel
// where the layer has the tiles for it, wgrad_mfma_kernel's 2 x 1 form elsewhere) the training step
// went 4.98 -> 4.75 ms and the 160^3 / 32-label step at batch 4 11.1 -> 9.9 ms, alternating runs (the
// operand read twice costs less than the 2 x 2 tile's occupancy).
static inline int wgrad_ct(int dtype, int cout) { return dtype_h16(dtype) && cout % 32 == 0 ? 21 : 11; }
// dY tile of the MFMA and wave-specialised kernels.  16 x 16 channel block (144 VGPRs, 50 KB of LDS), k3 s1: 4 output
// planes per tile halve the per-tile overhead (barriers, tile decode, LDS commit) and take the X halo from 2.8x to 2.1x
constexpr Tile3 wgrad_tile_shape(int ksize, int stride, int ct, bool wide) {
  return stride == 2 && ksize == 3 ? (wide ? Tile3{2, 4, 16} : Tile3{2, 8, 8})
                                   : (wide ? Tile3{ct == 11 && ksize == 3 ? 4 : 2, 8, 16} : Tile3{4, 8, 8});
}
static inline bool wgrad_rows_aligned(const segmi_act* a, int dtype) {
  return a->ld % (16 / dtype_size(dtype)) == 0 && ((uintptr_t)a->data % 16) == 0;
}
static inline segmi_act batch_part(const segmi_act* a, int parts, int i, int dtype) {
  segmi_act s = *a;
  s.n = a->n / parts;
  s.data = (char*)a->data + (int64_t)i * s.n * a->d * a->h * a->w * a->ld * dtype_size(dtype);
  return s;
}
// raw buffer loads of the wave-specialised kernel: 32-bit offsets / num_records over each tensor
static inline bool wgrad_in_descriptor(const segmi_act* x, const segmi_act* dy) {
  const int64_t lim = 0xfff00000ll;
  return act_voxels(x) * x->ld * 2 < lim && act_voxels(dy) * dy->ld * 2 < lim;
}
// grid.x of the wave-specialised kernel (wgrad_ws_impl.h) for one launch over (x, dy), 0 = it does not take it:
// bf16 / fp16 k3 layers whose two tile buffers fit one CU and that have enough tiles per workgroup for its pipeline
// to matter
static inline int wgrad_ws_gx(int dtype, const segmi_act* x, const segmi_act* dy, int stride, int ct, int chunks, int cus) {
  const int gx = wgrad_cus(cus) / chunks / 8 * 8;        // one 768-thread workgroup per CU, a multiple of the 8 XCDs
  if (gx < 8 || !wgrad_in_descriptor(x, dy)) return 0;
  const int64_t nt = tile_count(wgrad_tile_shape(3, stride, ct, wide_row(dy->w)), dy);
  return nt >= 4 * (int64_t)gx ? gx : 0;           // at least 4 tiles per workgroup
}

// The plan of segmi_conv3d_wgrad(dtype, x, dy, ksize, stride, cus).  The number of slabs fixes the summation order
// of the gradient, so it is part of the result's bits.
static inline WgradPlan wgrad_plan(int dtype, const segmi_act* x, const segmi_act* dy, int ksize, int stride, int cus_arg) {
  WgradPlan pl{};
  pl.parts = 1;
  if (x->c % 16 == 0 && dy->c % 16 == 0 && wgrad_rows_aligned(x, dtype) && wgrad_rows_aligned(dy, dtype) &&
      (ksize == 3 || ksize == 1)) {
    pl.ct = wgrad_ct(dtype, dy->c);
    const int cto = pl.ct / 10, cti = pl.ct % 10;
    const int chunks = (x->c / (16 * cti)) * (dy->c / (16 * cto));
    const Tile3 t = wgrad_tile_shape(ksize, stride, pl.ct, wide_row(dy->w));
    pl.td = t.td; pl.th = t.th; pl.tw = t.tw;
    int ws = 0;
    if (dtype_h16(dtype) && ksize == 3) {
      ws = wgrad_ws_gx(dtype, x, dy, stride, pl.ct, chunks, cus_arg);
      // The wave-specialised kernel addresses each operand through ONE buffer descriptor (32-bit offsets, < 4 GiB).  A
      // layer that misses it only for that (160^3 x 32 channels x batch 8 inside a 64-channel skip buffer = 4.2 GB) is
      // cut along the batch into 2 / 4 / 8 parts that fit: one launch per part, each with its own slabs, one reduce.
      if (!ws && !wgrad_in_descriptor(x, dy))
        for (int parts = 2; parts <= 8 && parts <= x->n && x->n % parts == 0; parts *= 2) {
          const segmi_act xs = batch_part(x, parts, 0, dtype), ys = batch_part(dy, parts, 0, dtype);
          if ((ws = wgrad_ws_gx(dtype, &xs, &ys, stride, pl.ct, chunks, cus_arg)) > 0) { pl.parts = parts; break; }
        }
    }
    pl.path = ws > 0 ? kWgradWaveSpecialised : kWgradMfma;
    pl.gx = ws;
    if (!ws) {
      // workgroups wanted = a multiple of the 256 CUs; one per CU once the kernel holds > 1 channel
      // tile (200-400 VGPRs, 55-110 KB slabs).  Measured on MI355X: 1x1 blocks
      // 704/508/540/608 us at 256/512/1024/2048 workgroups, 2x2 blocks 125/198/348 us at 256/512/1024.
      const int cus = wgrad_cus(cus_arg);
      const int want = (cto * cti == 1 ? 2 * cus : cus) / chunks;
      // ... capped by the tiles of the launch.  A k1, one-block (ct == 11), wide layer launches 2-plane tiles, but its
      // cap counts 4-plane tiles (the k3 shape): kept, because the slab count is part of the gradient's bits
      const int64_t nt = tile_count(wgrad_tile_shape(3, stride, pl.ct, wide_row(dy->w)), dy);
      pl.gx = (int)(want < 1 ? 1 : (want < nt ? want : nt));
    }
  } else if (conv_small_ok(x->c, dy->c, ksize) && wgrad_rows_aligned(dy, dtype)) {
    pl.path = kWgradSmallCin;
    pl.td = 2; pl.th = 8; pl.tw = 16;
    const int64_t nt = tile_count(Tile3{2, 8, 16}, dy);
    pl.gx = (int)(nt < 1024 ? nt : 1024);
  } else {
    pl.path = kWgradDirect;      // block b reduces 512-voxel chunks b, b + grid, ...
    pl.gx = (int)(cdiv64(act_voxels(dy), 512) > 1024 ? 1024 : cdiv64(act_voxels(dy), 512));
  }
  pl.slabs = pl.parts * pl.gx;
  return pl;
}

}  // namespace segmi
