"""The launchers' dispatch tables (SEGMI_BY_DTYPE, SEGMI_BY_DTYPE_PAIR, the label dispatch of common.h): the cells
of (entry point x storage type x label width) that no other test file reaches, and the refusal of every code outside
the tables.  The operations here copy, convert, compare or add exactly representable values, so the references are
plain torch on float64 / integer tensors and every comparison is bit equality: no tolerance is involved."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from segmantic_amd import _lib, ops  # noqa: E402
from tests.helpers import infer_ref as R  # noqa: E402

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
VOL = (12, 19, 30)
PAD = 16          # zero border of the padded reference volume: every origin below stays within it


def ints(shape, seed, lo=-100, hi=100):
    """integers of at most 7 bits as float64: exact in f32, bf16 and fp16, and so are sums of a few of them"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def origins(n, roi):
    """n window origins inside, across the border of and wholly outside VOL"""
    fixed = [(-3, -2, -5), (0, 0, 0), (4, 9, 14), (10, 17, 25), (-8, 0, 0), (12, 19, 30), (3, -8, 2)]
    return [fixed[i] if i < len(fixed) else (i % 7 - 1, (3 * i) % 16 - 2, (5 * i) % 29 - 3) for i in range(n)]


def padded(vol):
    """[..., D, H, W, C] -> the same with PAD zeros around the three spatial axes"""
    return torch.nn.functional.pad(vol, (0, 0, PAD, PAD, PAD, PAD, PAD, PAD))


def window(pv, z, y, x, roi):
    return pv[PAD + z:PAD + z + roi[0], PAD + y:PAD + y + roi[1], PAD + x:PAD + x + roi[2]]


# ------------------------------------------------------------------------------------------------ gather
# tests/test_infer_sweep_gpu.py reaches the 4-wide gather for every pair but f16 -> f16 and the scalar gather for
# f32 -> f32 / bf16 / f16, bf16 -> f32 and f16 -> f16; these are the other cells
@pytest.mark.parametrize("c,roi,src,dst", [(1, (8, 8, 8), "f16", "f16"), (1, (5, 6, 10), "bf16", "bf16"),
                                           (3, (8, 8, 8), "bf16", "bf16"), (1, (5, 6, 10), "f16", "f32"),
                                           (3, (8, 8, 8), "f16", "f32")])
def test_gather_pairs(c, roi, src, dst):
    img = ints(VOL + (c,), 3 + c)
    pv = padded(img)
    starts = origins(17, roi)                       # a second launch of the 16-per-call loop
    ref = torch.stack([window(pv, z, y, x, roi) for z, y, x in starts])
    wd = torch.full((17,) + roi + (c,), 9.0, dtype=DT[dst], device=DEV)
    ops.sw_gather(img[None].to(DT[src]).to(DEV), 0, starts, wd)
    torch.cuda.synchronize()
    assert torch.equal(wd.cpu().double(), ref)


# ------------------------------------------------------------------------------------------------ finalise
# sw_finalize is the f32 argmax with the count division in front; the sweep takes it with 1- and 2-byte labels
@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("label", [torch.uint8, torch.int16, torch.int32])
def test_finalize_label_widths(k, label):
    acc = ints((1,) + VOL + (k,), 20 + k, -8, 8).float()          # few values: many exact ties for the first-max rule
    cnt = ints(VOL, 30 + k, 1, 4).float()
    want = acc[0] / cnt[..., None]                                  # IEEE f32 division, as the kernel's
    lab = torch.full(VOL, 99, dtype=label, device=DEV)
    dacc = acc.to(DEV)
    ops.sw_finalize(dacc, cnt.to(DEV), lab, write_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(dacc.cpu()[0], want)
    assert torch.equal(lab.cpu().long(), torch.argmax(want, dim=-1))


# ------------------------------------------------------------------------------------------------ blend
# (kernel, storage type, label width) cells that the sweep's table leaves out
BLEND_CELLS = [R._bc("two-f32-int32", (8, 12, 20), (8, 8, 8), 0.5, 4, "f32", "int32"),
               R._bc("two-f16-uint8", (8, 12, 20), (8, 8, 8), 0.5, 8, "f16", "uint8"),
               R._bc("clamped-f32-int32", (9, 11, 13), (8, 8, 8), 0.5, 4, "f32", "int32"),
               R._bc("clamped-bf16-int32", (9, 11, 13), (8, 8, 8), 0.5, 8, "bf16", "int32"),
               R._bc("scalar-f16-uint8", (8, 12, 20), (8, 8, 8), 0.5, 3, "f16", "uint8")]


@pytest.mark.parametrize("case", BLEND_CELLS, ids=[c.name for c in BLEND_CELLS])
def test_blend_cells(case):
    assert case.kind == {"two": "blend2", "clamped": "blend", "scalar": "blend_scalar"}[case.name.split("-")[0]]
    cache, per_dim, wins, imp = R.blend_inputs(case)
    ref_l, ref_c, ref_lab, _, _ = R.blend_ref(cache, per_dim, 0, len(wins), case.roi, case.image, imp)
    D, H, W = case.image
    out = torch.empty((1, D, H, W, case.k), device=DEV)
    cnt = torch.empty((D, H, W), device=DEV)
    lab = torch.empty((D, H, W), dtype=getattr(torch, case.labels), device=DEV)
    args = (torch.from_numpy(cache).to(DT[case.dtype]).to(DEV), per_dim, 0, len(wins), case.roi, D, H, W)
    kw = dict(out_logits=out, out_count=cnt, labels=lab)
    name = ops.sw_blend_kernel_name(*args, **kw)
    assert name.startswith(f"sw_{case.kind}_kernel<{case.dtype},"), name
    ops.sw_blend(*args, **kw)
    torch.cuda.synchronize()
    got = {"logits": out[0].cpu().numpy(), "count": cnt.cpu().numpy(), "labels": lab.cpu().numpy()}
    bad = R.blend_violations(got, {"logits": ref_l, "count": ref_c, "labels": ref_lab}, None, exact=True)
    assert not bad, (case.name, name, bad)


# ------------------------------------------------------------------------------------------------ crop
@pytest.mark.parametrize("dst", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("c,roi", [(1, (8, 8, 8)), (3, (5, 6, 10))])
def test_crop_patches_cells(c, roi, dst):
    """17 patches of two volumes: every flip, origins across and beyond the border (zero fill), labels alongside"""
    img, lab = ints((2,) + VOL + (c,), 40 + c), ints((2,) + VOL + (1,), 50 + c, 0, 5)
    pi, pl = padded(img), padded(lab)
    starts = [(i % 2,) + o for i, o in enumerate(origins(17, roi))]
    flips = [i % 8 for i in range(17)]
    out = torch.full((17,) + roi + (c,), 9.0, dtype=DT[dst], device=DEV)
    olab = torch.full((17,) + roi, 9.0, device=DEV)
    ops.crop_patches(img.float().to(DEV), lab[..., 0].float().to(DEV), starts, flips, out, olab)
    torch.cuda.synchronize()
    for i, ((b, z, y, x), f) in enumerate(zip(starts, flips)):
        axes = [a for a in range(3) if f >> a & 1]                  # bit 0 = z, 1 = y, 2 = x
        wi, wl = window(pi[b], z, y, x, roi), window(pl[b], z, y, x, roi)[..., 0]
        assert torch.equal(out[i].cpu().double(), wi.flip(axes) if axes else wi), i
        assert torch.equal(olab[i].cpu().double(), wl.flip(axes) if axes else wl), i


# ------------------------------------------------------------------------------------------------ cast / transposes
@pytest.mark.parametrize("src,dst", [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"),
                                     ("f32", "f16"), ("f16", "f32"), ("f16", "f16")])
def test_cast_copy_pairs(src, dst):
    x = ints((2, 3, 5, 7, 3), 60)
    sbuf = torch.zeros((2, 3, 5, 7, 8), dtype=DT[src], device=DEV)        # rows wider than the channels on both sides
    dbuf = torch.full((2, 3, 5, 7, 4), 9.0, dtype=DT[dst], device=DEV)
    sbuf[..., :3] = x.to(DT[src]).to(DEV)
    ops.cast_copy(sbuf[..., :3], dbuf[..., :3])
    torch.cuda.synchronize()
    assert torch.equal(dbuf[..., :3].cpu().double(), x) and bool((dbuf[..., 3] == 9.0).all())


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("c", [1, 3])
def test_layout_transposes(c, dt):
    x = ints((2, c, 3, 5, 7), 70 + c)                                       # NCDHW
    ndhwc = torch.full((2, 3, 5, 7, c), 9.0, dtype=DT[dt], device=DEV)
    ops.nchw_to_ndhwc(x.float().to(DEV), ndhwc)
    back = torch.full((2, c, 3, 5, 7), 9.0, device=DEV)
    ops.ndhwc_to_nchw(ndhwc, back)
    torch.cuda.synchronize()
    assert torch.equal(ndhwc.cpu().double(), x.permute(0, 2, 3, 4, 1))
    assert torch.equal(back.cpu().double(), x)


# ------------------------------------------------------------------------------------------------ refusals
# every entry point that takes a storage-type code -> the positions of its codes
DTYPE_ARGS = {
    "segmi_wpack": (0,), "segmi_wpack_batch": (0,), "segmi_conv3d_fwd": (0,), "segmi_conv3d_fwd_split_act": (0,),
    "segmi_conv3d_fwd_pair": (0,), "segmi_dectop_fwd": (0,), "segmi_convT3d_fwd": (0,), "segmi_conv3d_wgrad": (0,),
    "segmi_bias_grad": (0,), "segmi_bn_stats": (0,), "segmi_bn_act_fwd": (0,), "segmi_add": (0,),
    "segmi_bn_act_bwd_reduce": (0,), "segmi_bn_act_bwd_fused": (0,), "segmi_bn_act_bwd_apply": (0,),
    "segmi_bn_act_bwd_apply_conv": (0,), "segmi_cast_copy": (0, 2), "segmi_nchw_to_ndhwc": (1,),
    "segmi_ndhwc_to_nchw": (0,), "segmi_softmax_dice_fwd": (0,), "segmi_softmax_dice_bwd": (0,),
    "segmi_softmax_dice_bwd_amp": (0,), "segmi_softmax_dice_ce_fwd": (0,), "segmi_softmax_dice_ce_bwd": (0,),
    "segmi_softmax_dice_ce_bwd_amp": (0,), "segmi_softmax_tversky_fwd": (0,), "segmi_softmax_tversky_bwd": (0,),
    "segmi_softmax_tversky_bwd_amp": (0,), "segmi_softmax_dice_focal_fwd": (0,), "segmi_softmax_dice_focal_bwd": (0,),
    "segmi_softmax_dice_focal_bwd_amp": (0,), "segmi_sw_gather": (0, 5), "segmi_sw_scatter_add": (0,),
    "segmi_sw_blend": (0,), "segmi_argmax": (0,), "segmi_crop_patches": (5,), "segmi_warp_crop_patches": (6,),
    "segmi_elastic_warp_crop_patches": (10,),
}
INT_ARGS = {"segmi_sw_gather": {2: 0}}        # integer arguments that must not be 4: the image index


def refusal_calls():
    for fn, pos in DTYPE_ARGS.items():
        for p in pos:
            yield fn, {p: 3}
        if len(pos) == 2:                           # the pair entry points: no conversion between the 16-bit types
            yield fn, {pos[0]: _lib.SEGMI_BF16, pos[1]: _lib.SEGMI_F16}
            yield fn, {pos[0]: _lib.SEGMI_F16, pos[1]: _lib.SEGMI_BF16}


@pytest.mark.parametrize("fn,codes", list(refusal_calls()),
                         ids=[f"{fn}-{'-'.join(map(str, c.values()))}@{min(c)}" for fn, c in refusal_calls()])
def test_unknown_storage_type_is_refused(fn, codes):
    """valid small arguments and a storage-type code outside the table: SEGMI_EINVAL with a message, before any
    launch -- the buffer every pointer argument names keeps its sentinel"""
    buf = torch.full((4, 4, 4, 4, 16), 7.0, device=DEV)
    a = ops.act(buf)
    descs = (_lib.WpackDesc * 4)()
    args = []
    for i, t in enumerate(_lib.SIGNATURES[fn][1]):
        if i in DTYPE_ARGS[fn]:
            args.append(codes.get(i, _lib.SEGMI_F32))
        elif t is _lib._AP:
            args.append(C.byref(a))
        elif t is C.c_void_p:
            args.append(C.c_void_p(buf.data_ptr()))
        elif t in (C.c_int, C.c_int64, C.c_uint32):
            args.append(INT_ARGS.get(fn, {}).get(i, 4))       # 4 patches / windows / control points, k = 4
        elif t in (C.c_float, C.c_double):
            args.append(0.5)
        else:                                                  # optional structures: absent, but a descriptor table
            args.append(descs if t is C.POINTER(_lib.WpackDesc) else None)
    rc = getattr(_lib.lib, fn)(*args)
    err = _lib.lib.segmi_last_error()
    torch.cuda.synchronize()
    assert rc == -1 and err, (fn, rc, err)                     # SEGMI_EINVAL
    assert b"dtype" in err or b"(ask segmi_" in err, err       # its own check, or the *_ok gate that holds it
    assert bool((buf == 7.0).all())
