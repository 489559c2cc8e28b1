"""Thin torch-tensor wrappers over the C-ABI of ``libsegmi.so``.

PyTorch is plumbing here (device memory, streams): every function below hands raw device
pointers + extents to a HIP kernel and returns.  Activations are ``[N, D, H, W, C]`` tensors
(NDHWC); a channel slice ``t[..., a:b]`` of such a tensor is a valid view (concat by offset).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import SEGMI_BF16, SEGMI_F16, SEGMI_F32, Act, BnBwdFin, BnBwdSums, BnFin, InAffine, Windows, check, lib

_DT = {torch.float32: SEGMI_F32, torch.bfloat16: SEGMI_BF16, torch.float16: SEGMI_F16}


def dtype_code(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported activation dtype {t.dtype} (float32 / bfloat16 / float16 only)")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_device(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            "segmantic_amd ops run on an MI355X only (tensor is on %s); there is no CPU path"
            % t.device)


class WindowBatch:
    """A batch of sliding windows read IN PLACE: ``volume`` [D, H, W] (contiguous, single channel, compute
    dtype) and the (z, y, x) origins of <= 32 windows of extent ``roi`` that lie inside it.  Quacks like the
    NDHWC tensor [n, *roi, 1] it stands for (``shape``, ``dtype``, ``device``); only the first-layer pair
    kernel (``conv3d_fwd_pair``) reads it (``segmi_windows``)."""

    def __init__(self, volume: torch.Tensor, starts, roi):
        if volume.dim() != 3 or not volume.is_contiguous():
            raise ValueError("WindowBatch: volume must be a contiguous [D, H, W] tensor")
        self.volume, self.roi = volume, tuple(int(r) for r in roi)
        self.starts = [tuple(int(v) for v in s) for s in starts]
        D, H, W = volume.shape
        if not 1 <= len(self.starts) <= SW_MAX_VIEWS:
            raise ValueError(f"WindowBatch: 1 .. {SW_MAX_VIEWS} windows")
        for s in self.starts:
            if any(a < 0 or a + r > n for a, r, n in zip(s, self.roi, (D, H, W))):
                raise ValueError(f"WindowBatch: window {s} + {self.roi} leaves the volume {tuple(volume.shape)}")
        self.shape = (len(self.starts),) + self.roi + (1,)
        self.dtype, self.device, self.is_cuda = volume.dtype, volume.device, volume.is_cuda

    @staticmethod
    def eligible(volume_shape, starts, roi) -> bool:
        """4-element alignment of rows and window origins (the kernel's staging loads)"""
        return (volume_shape[2] % 4 == 0 and roi[2] % 4 == 0 and (volume_shape[1] * volume_shape[2]) % 4 == 0
                and all(s[2] % 4 == 0 for s in starts))

    def windows(self) -> Windows:
        D, H, W = self.volume.shape
        w = Windows()
        w.count, w.row_stride, w.plane_stride = len(self.starts), W, H * W
        for i, (z, y, x) in enumerate(self.starts):
            w.offset[i] = (z * H + y) * W + x
        return w


def act(t) -> Act:
    """NDHWC view descriptor of a 5-D tensor whose last dim has stride 1."""
    if isinstance(t, WindowBatch):
        n, d, h, w, _ = t.shape
        return Act(t.volume.data_ptr(), n, d, h, w, 1, 1)
    _require_device(t)
    if t.dim() != 5:
        raise ValueError(f"expected a 5-D NDHWC tensor, got shape {tuple(t.shape)}")
    n, d, h, w, c = t.shape
    sn, sd, sh, sw, sc = t.stride()
    ld = sw
    if c > 1 and sc != 1:
        raise ValueError("channel dim must be contiguous")
    if w == 1:
        ld = max(ld, c)
    if not (sh == w * ld or h == 1) or not (sd == h * w * ld or d == 1) or \
            not (sn == d * h * w * ld or n == 1):
        raise ValueError(f"tensor is not a dense NDHWC view: shape {tuple(t.shape)} "
                         f"stride {t.stride()}")
    return Act(t.data_ptr(), n, d, h, w, c, ld)


def _ref(a: Optional[Act]):
    return C.byref(a) if a is not None else None


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    _require_device(t)
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ weights
def wpack_bytes(dtype: torch.dtype, kind: int, cin_k: int, cout_k: int, ksize: int) -> int:
    return int(lib.segmi_wpack_bytes(_DT[dtype], kind, cin_k, cout_k, ksize))


class WpackBatch:
    """Descriptor table for ``segmi_wpack_batch``: built once, re-run after every weight update.

    ``entries`` = [(kind, w_src, scale_or_None, cin_k, cout_k, ksize[, w_src2, cout_split]), ...];
    ``self.packed[i]`` is the device buffer entry ``i`` writes.  ``w_src2`` (kind 0): the source of the output
    channels from ``cout_split`` on (the pair pack of ``conv3d_fwd_split_act`` out of two parameter tensors)."""

    def __init__(self, dtype: torch.dtype, entries):
        self.dtype = dtype
        self.n = len(entries)
        self.packed = []
        self._keep = []
        self._host = (_lib.WpackDesc * self.n)()
        dev = entries[0][1].device
        for i, ent in enumerate(entries):
            kind, w, scale, cin_k, cout_k, ks = ent[:6]
            w2, split = (ent[6], ent[7]) if len(ent) > 6 else (None, 0)
            nbytes = wpack_bytes(dtype, kind, cin_k, cout_k, ks)
            if nbytes <= 0:
                raise ValueError(f"no MFMA pack for cin={cin_k} cout={cout_k}")
            out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.packed.append(out)
            self._keep.append((w, scale, w2))
            d = self._host[i]
            _require_device(w)
            d.w_src, d.packed = w.data_ptr(), out.data_ptr()
            if w2 is not None:
                if not ((kind == 0 and 0 < split < cout_k) or (kind == 2 and 0 < split < cin_k)):
                    raise ValueError("WpackBatch: a second source needs kind 0 (0 < split < cout_k) or kind 2 "
                                     "(0 < split < cin_k)")
                _require_device(w2)
                d.w_src2, d.cout_split = w2.data_ptr(), int(split)
            d.scale = scale.data_ptr() if scale is not None else None
            d.kind, d.cin_k, d.cout_k, d.ksize = kind, cin_k, cout_k, ks
        self._dev = torch.empty(C.sizeof(_lib.WpackDesc) * self.n, dtype=torch.uint8, device=dev)
        self._uploaded = False

    def run(self):
        check(lib.segmi_wpack_batch(_DT[self.dtype], self._host, self.n, _ptr(self._dev),
                                    0 if self._uploaded else 1, _stream()), "wpack_batch")
        self._uploaded = True


def wpack(dtype: torch.dtype, kind: int, w_src: torch.Tensor, cin_k: int, cout_k: int,
          ksize: int, scale: Optional[torch.Tensor] = None,
          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    nbytes = wpack_bytes(dtype, kind, cin_k, cout_k, ksize)
    if nbytes <= 0:
        raise ValueError(f"no MFMA pack for cin={cin_k} cout={cout_k}")
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=w_src.device)
    check(lib.segmi_wpack(_DT[dtype], kind, _ptr(w_src), _ptr(scale), cin_k, cout_k, ksize,
                          _ptr(out), _stream()), "wpack")
    return out


def mfma_ok(cin: int, cout: int) -> bool:
    return cin % 16 == 0 and cout % 16 == 0


# ------------------------------------------------------------------ convolution
def conv3d_stats_rows(x, y, ksize, stride) -> int:
    ax, ay = act(x), act(y)
    return int(lib.segmi_conv3d_stats_rows(dtype_code(x), C.byref(ax), C.byref(ay), ksize,
                                           stride))


def _in_affine(in_tf):
    """(scale, shift, prelu_alpha | None) device tensors -> segmi_in_affine (or NULL)"""
    if in_tf is None:
        return None
    scale, shift, alpha = in_tf
    for t in (scale, shift):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("in_tf: contiguous float32 scale / shift expected")
    return C.byref(InAffine(_ptr(scale), _ptr(shift), _ptr(alpha)))


def conv3d_fwd_kernel_name(x, y, ksize, stride) -> str:
    """kernel family ``conv3d_fwd`` runs for this layer (for benchmark / report labels)"""
    ax, ay = act(x), act(y)
    return lib.segmi_conv3d_fwd_kernel_name(dtype_code(x), C.byref(ax), C.byref(ay), ksize, stride).decode()


def conv3d_in_affine_ok(x, y, ksize, stride) -> bool:
    ax, ay = act(x), act(y)
    return bool(lib.segmi_conv3d_in_affine_ok(dtype_code(x), C.byref(ax), C.byref(ay), ksize, stride))


def conv3d_bn_bwd_sums_ok(x, y, ksize, stride) -> bool:
    ax, ay = act(x), act(y)
    return bool(lib.segmi_conv3d_bn_bwd_sums_ok(dtype_code(x), C.byref(ax), C.byref(ay), ksize, stride))


def wgrad_cus(cus: int) -> int:
    """compute units a weight-gradient call with the argument ``cus`` sizes its grid for (segmi_wgrad_cus:
    a multiple of 8 in [8, 256]; <= 0 = the whole chip; SEGMI_WGRAD_CUS overrides)"""
    return int(lib.segmi_wgrad_cus(int(cus)))


def cu_masked_stream(cus_enabled: int, device=None) -> "torch.cuda.Stream":
    """A torch stream over a HIP stream restricted to the first ``cus_enabled / 8`` CUs of every XCD
    (segmi_stream_create_cumask).  The HIP stream lives as long as the process."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    h = C.c_void_p()
    with torch.cuda.device(dev):
        check(lib.segmi_stream_create_cumask(int(cus_enabled), C.byref(h)), "stream_create_cumask")
    return torch.cuda.ExternalStream(h.value, device=dev)


def _bn_fin(fin):
    """fin = (count, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift)
    -> byref(segmi_bn_fin) or None: the launch that writes the statistics rows also finalises them"""
    if fin is None:
        return None
    count, gamma, beta, rm, rv, momentum, eps, mean, invstd, scale, shift = fin
    return C.byref(BnFin(float(count), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), float(momentum), float(eps),
                         _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift)))


def _bn_bwd_fin(fin):
    """fin = (count, dgamma, dbeta, dalpha, coef) -> segmi_bn_bwd_fin or None"""
    if fin is None:
        return None
    count, dgamma, dbeta, dalpha, coef = fin
    return BnBwdFin(float(count), _ptr(dgamma), _ptr(dbeta), _ptr(dalpha), _ptr(coef))


def conv3d_fwd(x, y, packed, w_src, w_kind, bias, ksize, stride, prelu_alpha=None,
               residual=None, stats=None, in_tf=None, bn_bwd=None, stats_fin=None, bn_bwd_fin=None) -> None:
    """``in_tf`` = (scale, shift, alpha): the producer's BatchNorm-apply + PReLU is applied to ``x``
    while it is staged (segmi_in_affine; only where ``conv3d_in_affine_ok``).
    ``bn_bwd`` = (x_raw, mean, invstd, gamma, beta, alpha | None, partials): this launch is an
    input-gradient conv whose output flows into that BatchNorm + PReLU; its epilogue also writes the
    partial rows of the BatchNorm-backward reduction (segmi_bn_bwd_sums; where ``conv3d_bn_bwd_sums_ok``).
    ``stats_fin`` / ``bn_bwd_fin``: the launch also finalises the ``stats`` / ``bn_bwd`` rows (``_bn_fin``,
    ``_bn_bwd_fin``): no separate bn_finalize / bn_act_bwd_finalize launch."""
    ax, ay = act(x), act(y)
    ar = act(residual) if residual is not None else None
    bb = None
    if bn_bwd is not None:
        xr, mean, invstd, gamma, beta, alpha, part = bn_bwd
        abx = act(xr)
        bf = _bn_bwd_fin(bn_bwd_fin)
        bb = C.byref(BnBwdSums(C.pointer(abx), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(alpha),
                               _ptr(part), C.pointer(bf) if bf is not None else None))
    check(lib.segmi_conv3d_fwd(dtype_code(x), C.byref(ax), C.byref(ay), _ptr(packed),
                               _ptr(w_src), w_kind, _ptr(bias), _ptr(prelu_alpha), _ref(ar),
                               _ptr(stats), ksize, stride, _in_affine(in_tf), bb, _bn_fin(stats_fin), _stream()),
          "conv3d_fwd")


def dectop_ok(x, y) -> bool:
    ax, ay = act(x), act(y)
    return bool(lib.segmi_dectop_ok(dtype_code(x), C.byref(ax), C.byref(ay)))


def dectop_up_frag(w_t: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """A-operand fragments of the transposed conv for ``segmi_dectop_fwd``: w_t [32, 16, 3, 3, 3] f32
    (torch ConvTranspose3d layout), scale f32[16] (folded BatchNorm) -> [27, 64, 8] of the layer's 16-bit
    storage ``dtype`` (bfloat16 / float16)."""
    ws = (w_t * scale.view(1, -1, 1, 1, 1)).reshape(32, 16, 27)
    return ws.permute(2, 0, 1).reshape(27, 4, 8, 16).permute(0, 1, 3, 2).contiguous().to(dtype).reshape(27, 64, 8)


def dectop_fwd(x, y, up_frag, up_bias, up_alpha, conv_packed, conv_bias, alpha_in_unit_range=False) -> None:
    """inference: ConvTranspose3d(32 -> 16) + folded BN + PReLU, then conv(16 -> 16) + identity residual,
    one launch (segmi_dectop_fwd)"""
    ax, ay = act(x), act(y)
    check(lib.segmi_dectop_fwd(dtype_code(x), C.byref(ax), C.byref(ay), _ptr(up_frag), _ptr(up_bias),
                               _ptr(up_alpha), int(bool(alpha_in_unit_range)), _ptr(conv_packed), _ptr(conv_bias),
                               _stream()), "dectop_fwd")


def conv3d_pair_ok(x, y_a, y_b) -> bool:
    ax, aa, ab = act(x), act(y_a), act(y_b)
    return bool(lib.segmi_conv3d_pair_ok(dtype_code(x), C.byref(ax), C.byref(aa), C.byref(ab)))


def conv3d_fwd_pair(x, y_a, w_a, bias_a, y_b, w_b, bias_b, stride, prelu_alpha_a=None,
                    stats_a=None, stats_fin_a=None) -> None:
    """Subunit-0 and residual convolution of a small-Cin ResidualUnit in one launch."""
    ax, aa, ab = act(x), act(y_a), act(y_b)
    win = C.byref(x.windows()) if isinstance(x, WindowBatch) else None
    check(lib.segmi_conv3d_fwd_pair(dtype_code(x), C.byref(ax), C.byref(aa), _ptr(w_a), _ptr(bias_a),
                                    _ptr(prelu_alpha_a), _ptr(stats_a), C.byref(ab), _ptr(w_b),
                                    _ptr(bias_b), stride, _bn_fin(stats_fin_a), win, _stream()), "conv3d_fwd_pair")


def conv3d_split_act_ok(x, y, ksize, stride) -> bool:
    ax, ay = act(x), act(y)
    return bool(lib.segmi_conv3d_split_act_ok(dtype_code(x), C.byref(ax), C.byref(ay), ksize, stride))


def conv3d_fwd_split_act(x, y, packed, bias, prelu_alpha, act_channels, ksize, stride, bias_b=None,
                         stats=None, stats_fin=None) -> None:
    """one conv with two weight sets (concatenated pack): PReLU on the first ``act_channels`` only.
    Training: ``prelu_alpha`` None, ``bias_b`` = the second convolution's bias, ``stats`` (+ ``stats_fin``) =
    BatchNorm statistics rows [conv3d_stats_rows][2][act_channels] of the first ``act_channels`` outputs."""
    ax, ay = act(x), act(y)
    check(lib.segmi_conv3d_fwd_split_act(dtype_code(x), C.byref(ax), C.byref(ay), _ptr(packed), _ptr(bias),
                                         _ptr(prelu_alpha), act_channels, ksize, stride, _ptr(bias_b),
                                         _ptr(stats), _bn_fin(stats_fin), _stream()),
          "conv3d_fwd_split_act")


def convT3d_stats_rows(x, y) -> int:
    ax, ay = act(x), act(y)
    return int(lib.segmi_convT3d_stats_rows(dtype_code(x), C.byref(ax), C.byref(ay)))


def convT3d_fwd(x, y, packed, w_src, bias, prelu_alpha=None, residual=None, stats=None,
                stats_fin=None) -> None:
    ax, ay = act(x), act(y)
    ar = act(residual) if residual is not None else None
    check(lib.segmi_convT3d_fwd(dtype_code(x), C.byref(ax), C.byref(ay), _ptr(packed),
                                _ptr(w_src), _ptr(bias), _ptr(prelu_alpha), _ref(ar),
                                _ptr(stats), _bn_fin(stats_fin), _stream()), "convT3d_fwd")


def conv3d_wgrad_workspace(x, dy, ksize, stride, cus: int = 0) -> int:
    """``cus``: the compute-unit budget the call will be made with (it sizes the partial slabs)"""
    ax, ay = act(x), act(dy)
    return int(lib.segmi_conv3d_wgrad_workspace(dtype_code(x), C.byref(ax), C.byref(ay), ksize,
                                                stride, int(cus)))


def conv3d_wgrad(x, dy, dw, db, ksize, stride, workspace, in_tf=None, cus: int = 0) -> None:
    """``cus``: compute units the kernel sizes its grid for (0 = the whole chip); per call, no global state"""
    ax, ay = act(x), act(dy)
    check(lib.segmi_conv3d_wgrad(dtype_code(x), C.byref(ax), C.byref(ay), _ptr(dw), _ptr(db),
                                 ksize, stride, _ptr(workspace), _in_affine(in_tf), int(cus), _stream()),
          "conv3d_wgrad")


def bias_grad(dy, db, workspace) -> None:
    ay = act(dy)
    check(lib.segmi_bias_grad(dtype_code(dy), C.byref(ay), _ptr(db), _ptr(workspace),
                              _stream()), "bias_grad")


# ------------------------------------------------------------------ norm + activation
def bn_stats_rows(x) -> int:
    ax = act(x)
    return int(lib.segmi_bn_stats_rows(C.byref(ax)))


def bn_stats(x, partials) -> None:
    ax = act(x)
    check(lib.segmi_bn_stats(dtype_code(x), C.byref(ax), _ptr(partials), _stream()), "bn_stats")


def bn_finalize(partials, rows, c, count, gamma, beta, running_mean, running_var, momentum,
                eps, mean, invstd, scale, shift) -> None:
    check(lib.segmi_bn_finalize(_ptr(partials), rows, c, float(count), _ptr(gamma), _ptr(beta),
                                _ptr(running_mean), _ptr(running_var), momentum, eps,
                                _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift), _stream()),
          "bn_finalize")


def bn_eval_affine(gamma, beta, running_mean, running_var, eps, scale, shift) -> None:
    check(lib.segmi_bn_eval_affine(running_mean.numel(), _ptr(gamma), _ptr(beta),
                                   _ptr(running_mean), _ptr(running_var), eps, _ptr(scale),
                                   _ptr(shift), _stream()), "bn_eval_affine")


def bn_act_fwd(x, y, scale, shift, prelu_alpha=None, residual=None, dropout=(0.0, 0)) -> None:
    """dropout = (p, seed): ADN dropout between norm and activation (mask recomputed in backward)."""
    ax, ay = act(x), act(y)
    ar = act(residual) if residual is not None else None
    check(lib.segmi_bn_act_fwd(dtype_code(x), C.byref(ax), C.byref(ay), _ptr(scale),
                               _ptr(shift), _ptr(prelu_alpha), _ref(ar), float(dropout[0]),
                               int(dropout[1]) & 0xFFFFFFFF, _stream()),
          "bn_act_fwd")


def bn_act_bwd_rows(x) -> int:
    ax = act(x)
    return int(lib.segmi_bn_act_bwd_rows(C.byref(ax)))


def bn_act_bwd_reduce(dy, x, mean, invstd, gamma, beta, prelu_alpha, partials,
                      dropout=(0.0, 0), fin=None) -> None:
    """``fin`` = (count, dgamma, dbeta, dalpha, coef): finalise in the same launch"""
    ady, ax = act(dy), act(x)
    bf = _bn_bwd_fin(fin)
    check(lib.segmi_bn_act_bwd_reduce(dtype_code(x), C.byref(ady), C.byref(ax), _ptr(mean),
                                      _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(prelu_alpha),
                                      _ptr(partials), float(dropout[0]), int(dropout[1]) & 0xFFFFFFFF,
                                      C.byref(bf) if bf is not None else None, _stream()), "bn_act_bwd_reduce")


def bn_act_bwd_fused_ok(dy, x, dx) -> bool:
    ady, ax, adx = act(dy), act(x), act(dx)
    return bool(lib.segmi_bn_act_bwd_fused_ok(dtype_code(x), C.byref(ady), C.byref(ax), C.byref(adx)))


def bn_act_bwd_fused_rows(x) -> int:
    a = act(x)
    return int(lib.segmi_bn_act_bwd_fused_rows(C.byref(a)))


def bn_act_bwd_fused(dy, x, dx, mean, invstd, gamma, beta, prelu_alpha, partials, fin, max_wgs: int = 0) -> None:
    """reduce + finalise + apply of the BatchNorm / PReLU backward in one launch (small tensors);
    ``fin`` = (count, dgamma, dbeta, dalpha, coef); ``max_wgs``: the most workgroups (= whole CUs) the launch
    may hold while its hand-off completes (0 = what the device holds at once)"""
    ady, ax, adx = act(dy), act(x), act(dx)
    bf = _bn_bwd_fin(fin)
    check(lib.segmi_bn_act_bwd_fused(dtype_code(x), C.byref(ady), C.byref(ax), C.byref(adx), _ptr(mean),
                                     _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(prelu_alpha), _ptr(partials),
                                     C.byref(bf), int(max_wgs), _stream()), "bn_act_bwd_fused")


def bn_act_bwd_fused_wgs(x, max_wgs: int = 0) -> int:
    """workgroups ``bn_act_bwd_fused`` would launch for ``x`` under ``max_wgs`` on the current device"""
    a = act(x)
    return int(lib.segmi_bn_act_bwd_fused_wgs(dtype_code(x), C.byref(a), int(max_wgs)))


def fused_timeouts(reset: bool = False) -> int:
    """expiries of ``bn_act_bwd_fused``'s bounded hand-off wait so far (host-visible counter, no device sync).
    Non-zero: some launch wrote NaN gradients instead of hanging -- see ``check_fused_timeouts``."""
    return int(lib.segmi_fused_timeouts(1 if reset else 0))


def check_fused_timeouts(where: str = "") -> None:
    """raise (and clear the counter) when a one-launch BatchNorm backward gave up waiting: its gradients are NaN, and
    every optimiser step since has poisoned the weights -- the reference stops on a non-finite loss
    (monai_unet.py:512-518); here the failure is an exception instead of a silent NaN run"""
    n = fused_timeouts(reset=True)
    if n:
        raise RuntimeError(
            f"{n} workgroup(s) of segmi_bn_act_bwd_fused gave up waiting for their launch's last workgroup"
            f"{' (' + where + ')' if where else ''}: the launch was never fully resident (GPU shared with another "
            "process, or CUs masked).  The gradients of that step are NaN and the weights are poisoned: restart "
            "from the last checkpoint with SEGMI_FUSE_BN_BWD_SMALL=0 (three launches, no grid-wide wait).")


def fused_test_hook(poll_limit: int = 0, no_publish: bool = False) -> None:
    """tests only: poll bound of the hand-off wait (0 = default) / withhold the flag so every waiter expires"""
    check(lib.segmi_fused_test_hook(int(poll_limit), 1 if no_publish else 0), "fused_test_hook")


def bn_act_bwd_apply_conv_ok(dy, x, dx, out) -> bool:
    ady, ax, adx, ao = act(dy), act(x), act(dx), act(out)
    return bool(lib.segmi_bn_act_bwd_apply_conv_ok(dtype_code(x), C.byref(ady), C.byref(ax), C.byref(adx),
                                                   C.byref(ao)))


def bn_act_bwd_apply_conv(dy, x, dx, mean, invstd, gamma, beta, prelu_alpha, coef, out, packed) -> None:
    """dx = bn_act_bwd_apply(dy, x) and out = conv_k3s2(dx) as ONE launch (the input gradient of a decoder
    level's transposed convolution; csrc/conv_bnbwd_impl.h): same bits as the two calls"""
    ady, ax, adx, ao = act(dy), act(x), act(dx), act(out)
    check(lib.segmi_bn_act_bwd_apply_conv(dtype_code(x), C.byref(ady), C.byref(ax), C.byref(adx), _ptr(mean),
                                          _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(prelu_alpha), _ptr(coef),
                                          C.byref(ao), _ptr(packed), _stream()), "bn_act_bwd_apply_conv")


def bn_act_bwd_finalize(partials, rows, c, count, gamma, invstd, dgamma, dbeta, dalpha,
                        coef) -> None:
    check(lib.segmi_bn_act_bwd_finalize(_ptr(partials), rows, c, float(count), _ptr(gamma),
                                        _ptr(invstd), _ptr(dgamma), _ptr(dbeta), _ptr(dalpha),
                                        _ptr(coef), _stream()), "bn_act_bwd_finalize")


def bn_act_bwd_apply(dy, x, dx, mean, invstd, gamma, beta, prelu_alpha, coef,
                     dropout=(0.0, 0)) -> None:
    ady, ax, adx = act(dy), act(x), act(dx)
    check(lib.segmi_bn_act_bwd_apply(dtype_code(x), C.byref(ady), C.byref(ax), C.byref(adx),
                                     _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta),
                                     _ptr(prelu_alpha), _ptr(coef), float(dropout[0]),
                                     int(dropout[1]) & 0xFFFFFFFF, _stream()),
          "bn_act_bwd_apply")


def add(a, b, out) -> None:
    aa, ao = act(a), act(out)
    ab = act(b) if b is not None else None
    check(lib.segmi_add(dtype_code(a), C.byref(aa), _ref(ab), C.byref(ao), _stream()), "add")


def cast_copy(src, dst) -> None:
    a, b = act(src), act(dst)
    check(lib.segmi_cast_copy(dtype_code(src), C.byref(a), dtype_code(dst), C.byref(b),
                              _stream()), "cast_copy")


def nchw_to_ndhwc(src: torch.Tensor, dst: torch.Tensor) -> None:
    """src f32 [N,C,D,H,W] contiguous -> dst NDHWC (f32, bf16 or fp16)."""
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("nchw_to_ndhwc expects a contiguous float32 NCDHW tensor")
    b = act(dst)
    check(lib.segmi_nchw_to_ndhwc(_ptr(src), dtype_code(dst), C.byref(b), _stream()),
          "nchw_to_ndhwc")


def ndhwc_to_nchw(src: torch.Tensor, dst: torch.Tensor) -> None:
    a = act(src)
    if dst.dtype != torch.float32 or not dst.is_contiguous():
        raise ValueError("ndhwc_to_nchw writes a contiguous float32 NCDHW tensor")
    check(lib.segmi_ndhwc_to_nchw(dtype_code(src), C.byref(a), _ptr(dst), _stream()),
          "ndhwc_to_nchw")


# ------------------------------------------------------------------ loss + optimiser
def dice_chunks(logits) -> int:
    a = act(logits)
    return int(lib.segmi_dice_chunks(C.byref(a)))


def dice_ce_chunks(logits) -> int:
    """chunks of the partials buffer f32 [chunks, n, rows, k] of a forward (rows: 4 with a cross-entropy / focal
    term, else 3)"""
    a = act(logits)
    return int(lib.segmi_dice_ce_chunks(C.byref(a)))


def _class_weight(class_weight, logits):
    if class_weight is not None and (class_weight.dtype != torch.float32 or class_weight.numel() != logits.shape[4]
                                     or not class_weight.is_contiguous()):
        raise ValueError(f"class_weight must be a contiguous float32 tensor of {logits.shape[4]} entries")
    return _ptr(class_weight)


def _loss_fwd(name, logits, labels, partials, coef, loss, *params) -> None:
    """``segmi_<name>``: ``params`` are the entry point's own arguments between ``loss`` and ``stream``"""
    a = act(logits)
    check(getattr(lib, "segmi_" + name)(dtype_code(logits), C.byref(a), _ptr(labels), _ptr(partials), _ptr(coef),
                                        _ptr(loss), *params, _stream()), name)


def _loss_bwd(name, logits, labels, coef, extra, scale, dlogits, scratch, bias_grad) -> None:
    """``segmi_<name>``: ``scale`` is the ``amp`` state tensor of an ``_amp`` entry point, else ``grad_scale``;
    ``extra``: the entry point's own arguments in front of it"""
    a, b = act(logits), act(dlogits)
    scale = _ptr(scale) if name.endswith("_amp") else float(scale)
    check(getattr(lib, "segmi_" + name)(dtype_code(logits), C.byref(a), _ptr(labels), _ptr(coef), *extra, scale,
                                        C.byref(b), _ptr(scratch), _ptr(bias_grad), _stream()), name)


def softmax_dice_fwd(logits, labels, partials, coef, loss, smooth_nr=1e-5, smooth_dr=1e-5):
    _loss_fwd("softmax_dice_fwd", logits, labels, partials, coef, loss, smooth_nr, smooth_dr)


def softmax_dice_bwd(logits, labels, coef, grad_scale, dlogits, scratch=None, bias_grad=None) -> None:
    """bias_grad (f32[K], optional): channel sums of dlogits, folded into the same pass; `scratch`
    is then the forward's partials buffer."""
    _loss_bwd("softmax_dice_bwd", logits, labels, coef, (), grad_scale, dlogits, scratch, bias_grad)


def softmax_dice_bwd_amp(logits, labels, coef, amp, dlogits, scratch=None, bias_grad=None) -> None:
    """softmax_dice_bwd with the loss scale read from ``amp[0]`` on the device (f32[3], see "dynamic loss scaling")."""
    _loss_bwd("softmax_dice_bwd_amp", logits, labels, coef, (), amp, dlogits, scratch, bias_grad)


def softmax_dice_ce_fwd(logits, labels, partials, coef, loss, smooth_nr=1e-5, smooth_dr=1e-5, lambda_dice=1.0,
                        lambda_ce=1.0, include_background=True, class_weight=None) -> None:
    """loss = lambda_dice * Dice + lambda_ce * CE (``segmi.h``); ``class_weight``: device f32[K] or None (ones);
    ``coef`` f32[n, 3, k] carries everything the backward needs."""
    _loss_fwd("softmax_dice_ce_fwd", logits, labels, partials, coef, loss, smooth_nr, smooth_dr, float(lambda_dice),
              float(lambda_ce), int(bool(include_background)), _class_weight(class_weight, logits))


def softmax_dice_ce_bwd(logits, labels, coef, grad_scale, dlogits, scratch=None, bias_grad=None) -> None:
    """as ``softmax_dice_bwd`` with the 3-row coefficients of ``softmax_dice_ce_fwd``"""
    _loss_bwd("softmax_dice_ce_bwd", logits, labels, coef, (), grad_scale, dlogits, scratch, bias_grad)


def softmax_dice_ce_bwd_amp(logits, labels, coef, amp, dlogits, scratch=None, bias_grad=None) -> None:
    """softmax_dice_ce_bwd with the loss scale read from ``amp[0]`` on the device."""
    _loss_bwd("softmax_dice_ce_bwd_amp", logits, labels, coef, (), amp, dlogits, scratch, bias_grad)


def softmax_tversky_fwd(logits, labels, partials, coef, loss, smooth_nr=1e-5, smooth_dr=1e-5, alpha=0.3, beta=0.7,
                        exponent=1.0, include_background=True) -> None:
    """loss = mean (1 - TI)^exponent (``segmi.h``); ``partials`` f32 [dice_ce_chunks, n, 3, k], ``coef`` f32 [n, 2, k]"""
    _loss_fwd("softmax_tversky_fwd", logits, labels, partials, coef, loss, smooth_nr, smooth_dr, float(alpha),
              float(beta), float(exponent), int(bool(include_background)))


def softmax_tversky_bwd(logits, labels, coef, grad_scale, dlogits, scratch=None, bias_grad=None) -> None:
    """as ``softmax_dice_bwd`` with the coefficient pair of ``softmax_tversky_fwd``"""
    _loss_bwd("softmax_tversky_bwd", logits, labels, coef, (), grad_scale, dlogits, scratch, bias_grad)


def softmax_tversky_bwd_amp(logits, labels, coef, amp, dlogits, scratch=None, bias_grad=None) -> None:
    """softmax_tversky_bwd with the loss scale read from ``amp[0]`` on the device."""
    _loss_bwd("softmax_tversky_bwd_amp", logits, labels, coef, (), amp, dlogits, scratch, bias_grad)


def softmax_dice_focal_fwd(logits, labels, partials, coef, loss, smooth_nr=1e-5, smooth_dr=1e-5, lambda_dice=1.0,
                           lambda_focal=1.0, gamma=2.0, include_background=True, class_weight=None) -> None:
    """loss = lambda_dice * Dice + lambda_focal * Focal (``segmi.h``); buffers as ``softmax_dice_ce_fwd``;
    ``gamma = 0`` runs the Dice + cross-entropy kernels."""
    _loss_fwd("softmax_dice_focal_fwd", logits, labels, partials, coef, loss, smooth_nr, smooth_dr, float(lambda_dice),
              float(lambda_focal), float(gamma), int(bool(include_background)), _class_weight(class_weight, logits))


def softmax_dice_focal_bwd(logits, labels, coef, gamma, grad_scale, dlogits, scratch=None, bias_grad=None) -> None:
    """as ``softmax_dice_ce_bwd`` with the forward's ``gamma``"""
    _loss_bwd("softmax_dice_focal_bwd", logits, labels, coef, (float(gamma),), grad_scale, dlogits, scratch, bias_grad)


def softmax_dice_focal_bwd_amp(logits, labels, coef, gamma, amp, dlogits, scratch=None, bias_grad=None) -> None:
    """softmax_dice_focal_bwd with the loss scale read from ``amp[0]`` on the device."""
    _loss_bwd("softmax_dice_focal_bwd_amp", logits, labels, coef, (float(gamma),), amp, dlogits, scratch, bias_grad)


def adam_step(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, lr, beta1, beta2, eps,
              weight_decay, step, grad_scale=1.0) -> None:
    check(lib.segmi_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                              _ptr(max_exp_avg_sq), param.numel(), lr, beta1, beta2, eps,
                              weight_decay, step, grad_scale, _stream()), "adam_step")


def sgd_step(param, grad, buf, lr, momentum, weight_decay, first_step, grad_scale=1.0) -> None:
    check(lib.segmi_sgd_step(_ptr(param), _ptr(grad), _ptr(buf), param.numel(), lr, momentum,
                             weight_decay, int(first_step), grad_scale, _stream()), "sgd_step")


def adabelief_step(param, grad, exp_avg, exp_avg_var, lr, beta1, beta2, eps, weight_decay,
                   weight_decouple, step, grad_scale=1.0) -> None:
    check(lib.segmi_adabelief_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_var),
                                   param.numel(), lr, beta1, beta2, eps, weight_decay,
                                   int(weight_decouple), step, grad_scale, _stream()),
          "adabelief_step")


# ------------------------------------------------------------------ dynamic loss scaling
# amp: f32[3] device tensor {scale, found_inf, skipped steps}; tracker: int32[1]; step: int64[1] (segmi.h)
def amp_check_finite(grad, amp) -> None:
    check(lib.segmi_amp_check_finite(_ptr(grad), grad.numel(), _ptr(amp), _stream()), "amp_check_finite")


def amp_update_scale(amp, tracker, step, growth_factor, backoff_factor, growth_interval) -> None:
    check(lib.segmi_amp_update_scale(_ptr(amp), _ptr(tracker), _ptr(step), float(growth_factor),
                                     float(backoff_factor), int(growth_interval), _stream()), "amp_update_scale")


def adam_step_amp(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, lr, beta1, beta2, eps, weight_decay,
                  amp, step, grad_scale=1.0) -> None:
    check(lib.segmi_adam_step_amp(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                  _ptr(max_exp_avg_sq), param.numel(), lr, beta1, beta2, eps, weight_decay,
                                  _ptr(amp), _ptr(step), grad_scale, _stream()), "adam_step_amp")


def sgd_step_amp(param, grad, buf, lr, momentum, weight_decay, amp, step, grad_scale=1.0) -> None:
    check(lib.segmi_sgd_step_amp(_ptr(param), _ptr(grad), _ptr(buf), param.numel(), lr, momentum, weight_decay,
                                 _ptr(amp), _ptr(step), grad_scale, _stream()), "sgd_step_amp")


def adabelief_step_amp(param, grad, exp_avg, exp_avg_var, lr, beta1, beta2, eps, weight_decay, weight_decouple,
                       amp, step, grad_scale=1.0) -> None:
    check(lib.segmi_adabelief_step_amp(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_var), param.numel(),
                                       lr, beta1, beta2, eps, weight_decay, int(weight_decouple), _ptr(amp),
                                       _ptr(step), grad_scale, _stream()), "adabelief_step_amp")


# ------------------------------------------------------------------ sliding window
def _starts(starts: Sequence[Sequence[int]], width: int):
    arr = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1, width))
    return arr, arr.ctypes.data_as(C.c_void_p)


SW_MAX_VIEWS = 32       # window views per first-layer call (segmi_windows.offset in include/segmi.h)
SW_MAX_WINDOWS = 16     # windows per segmi_sw_gather / segmi_sw_scatter_add call (kMaxWin in sliding.hip)


def sw_gather(image, img_index, starts, windows) -> None:
    a = act(image)
    for i in range(0, len(starts), SW_MAX_WINDOWS):      # larger groups: one launch per 16 windows
        arr, p = _starts(starts[i:i + SW_MAX_WINDOWS], 3)
        b = act(windows[i:i + arr.shape[0]])
        check(lib.segmi_sw_gather(dtype_code(image), C.byref(a), img_index, p, arr.shape[0],
                                  dtype_code(windows), C.byref(b), _stream()), "sw_gather")


def sw_scatter_add(pred, starts, acc, cnt, importance=None) -> None:
    b = act(acc)
    # larger groups: one launch per 16 windows, in schedule order (launches on one stream run in
    # order, so every voxel still receives its windows in the reference's sequence)
    for i in range(0, len(starts), SW_MAX_WINDOWS):
        arr, p = _starts(starts[i:i + SW_MAX_WINDOWS], 3)
        a = act(pred[i:i + arr.shape[0]])
        check(lib.segmi_sw_scatter_add(dtype_code(pred), C.byref(a), p, arr.shape[0],
                                       _ptr(importance), C.byref(b), _ptr(cnt), _stream()),
              "sw_scatter_add")


_LABEL_BYTES = {torch.uint8: 1, torch.int16: 2, torch.int32: 4}


def sw_finalize(acc, cnt, labels, write_logits=True) -> None:
    a = act(acc)
    check(lib.segmi_sw_finalize(C.byref(a), _ptr(cnt), int(write_logits), _ptr(labels),
                                _LABEL_BYTES[labels.dtype], _stream()), "sw_finalize")


def sw_blend(cache, starts_zyx, win_lo, win_hi, roi, d, h, w, importance=None, out_logits=None,
             out_count=None, labels=None, normalize=True) -> None:
    """cache [slots, rd, rh, rw, K] (NDHWC, f32, bf16 or fp16); starts_zyx = three ascending origin lists."""
    _require_device(cache)
    if cache.dim() != 5 or cache.stride(4) != 1 or not cache.is_contiguous():
        raise ValueError("sw_blend: cache must be a contiguous [slots, rd, rh, rw, K] tensor")
    arrs = [np.ascontiguousarray(np.asarray(sv, dtype=np.int32)) for sv in starts_zyx]
    k = cache.shape[4]
    ldo = out_logits.stride(-2) if out_logits is not None else 0
    if out_logits is not None and (out_logits.dtype != torch.float32 or out_logits.stride(-1) != 1):
        raise ValueError("sw_blend: out_logits must be float32 NDHWC")
    check(lib.segmi_sw_blend(
        dtype_code(cache), _ptr(cache), k, cache.stride(3),
        arrs[0].ctypes.data_as(C.c_void_p), len(arrs[0]), arrs[1].ctypes.data_as(C.c_void_p),
        len(arrs[1]), arrs[2].ctypes.data_as(C.c_void_p), len(arrs[2]), int(win_lo), int(win_hi),
        int(roi[0]), int(roi[1]), int(roi[2]), _ptr(importance), int(d), int(h), int(w),
        _ptr(out_logits), int(ldo), _ptr(out_count), _ptr(labels),
        _LABEL_BYTES[labels.dtype] if labels is not None else 1, int(bool(normalize)), _stream()),
        "sw_blend")


def sw_blend_kernel_name(cache, starts_zyx, win_lo, win_hi, roi, d, h, w, importance=None, out_logits=None,
                         out_count=None, labels=None, normalize=True) -> str:
    """The kernel ``sw_blend`` takes for these arguments (same signature; launches nothing):
    ``sw_blend2_kernel<..>``, ``sw_blend_kernel<..>`` or ``sw_blend_scalar_kernel<..>``, with G = channels per lane."""
    _require_device(cache)
    if cache.dim() != 5 or cache.stride(4) != 1 or not cache.is_contiguous():
        raise ValueError("sw_blend: cache must be a contiguous [slots, rd, rh, rw, K] tensor")
    arrs = [np.ascontiguousarray(np.asarray(sv, dtype=np.int32)) for sv in starts_zyx]
    ldo = out_logits.stride(-2) if out_logits is not None else 0
    return lib.segmi_sw_blend_kernel_name(
        dtype_code(cache), _ptr(cache), cache.shape[4], cache.stride(3),
        arrs[0].ctypes.data_as(C.c_void_p), len(arrs[0]), arrs[1].ctypes.data_as(C.c_void_p),
        len(arrs[1]), arrs[2].ctypes.data_as(C.c_void_p), len(arrs[2]),
        int(roi[0]), int(roi[1]), int(roi[2]), _ptr(out_logits), int(ldo)).decode()


def argmax(logits, labels) -> None:
    a = act(logits)
    check(lib.segmi_argmax(dtype_code(logits), C.byref(a), _ptr(labels),
                           _LABEL_BYTES[labels.dtype], _stream()), "argmax")


def label_counts(pred, truth, k, counts) -> None:
    check(lib.segmi_label_counts(_ptr(pred), _ptr(truth), pred.numel(), k, _ptr(counts),
                                 _stream()), "label_counts")


# ------------------------------------------------------------------ test-time augmentation
_TTA_LABEL_BYTES = {torch.uint8: 1, torch.int32: 4}


def tta_accumulate(logits, flip_mask: int, acc, first: bool) -> None:
    """logits f32 NDHWC [1, d, h, w, K] of the pass run on the volume mirrored along the axes in ``flip_mask``
    (bit 0 = d, 1 = h, 2 = w); acc dense f32 [d, h, w, K] receives (``first``) or adds the pass's softmax at the
    un-mirrored voxel."""
    if logits.dtype != torch.float32 or acc.dtype != torch.float32:
        raise TypeError("tta_accumulate: float32 logits and accumulator")
    a = act(logits)
    _require_device(acc)
    if not acc.is_contiguous() or tuple(acc.shape) != (a.d, a.h, a.w, a.c):
        raise ValueError(f"tta_accumulate: acc must be a dense [d, h, w, K] tensor, got {tuple(acc.shape)} "
                         f"for logits {tuple(logits.shape)}")
    check(lib.segmi_tta_accumulate(C.byref(a), int(flip_mask), _ptr(acc), int(bool(first)), _stream()),
          "tta_accumulate")


def tta_finalize(scores, labels, confidence=None, entropy=None, probs_out=None) -> None:
    """scores f32 NDHWC [n, d, h, w, K] (non-negative) -> labels uint8 / int32 [n, d, h, w] and, each optional,
    confidence / entropy f32 [n, d, h, w] and the normalised probabilities (NDHWC; may be ``scores`` itself)."""
    if scores.dtype != torch.float32:
        raise TypeError("tta_finalize: float32 scores")
    a = act(scores)
    nvox = a.n * a.d * a.h * a.w
    if labels.dtype not in _TTA_LABEL_BYTES:
        raise TypeError("tta_finalize: labels must be uint8 or int32")
    for t, what in ((labels, "labels"), (confidence, "confidence"), (entropy, "entropy")):
        if t is not None and (t.numel() != nvox or not t.is_contiguous()):
            raise ValueError(f"tta_finalize: {what} must be a dense tensor of {nvox} voxels")
    for t, what in ((confidence, "confidence"), (entropy, "entropy")):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"tta_finalize: float32 {what}")
    p = None
    if probs_out is not None:
        if probs_out.dtype != torch.float32:
            raise TypeError("tta_finalize: float32 probs_out")
        p = act(probs_out)
    check(lib.segmi_tta_finalize(C.byref(a), a.c, _ptr(labels), _TTA_LABEL_BYTES[labels.dtype], _ptr(confidence),
                                 _ptr(entropy), _ref(p), _stream()), "tta_finalize")


def label_means(labels, values, k: int, sums=None, counts=None):
    """Per label c < k: (sums f64 [k], counts i64 [k]) of ``values`` (f32) over the voxels of ``labels``
    (uint8 / int32) with that label; deterministic, on the device."""
    _require_device(labels)
    if labels.dtype not in _TTA_LABEL_BYTES or values.dtype != torch.float32:
        raise TypeError("label_means: uint8 / int32 labels and float32 values")
    if labels.numel() != values.numel() or not labels.is_contiguous() or not values.is_contiguous():
        raise ValueError("label_means: labels and values must be dense and of one size")
    if sums is None:
        sums = torch.empty(k, dtype=torch.float64, device=labels.device)
    if counts is None:
        counts = torch.empty(k, dtype=torch.int64, device=labels.device)
    if sums.dtype != torch.float64 or counts.dtype != torch.int64 or sums.numel() != k or counts.numel() != k:
        raise ValueError("label_means: sums f64 [k] and counts i64 [k]")
    check(lib.segmi_label_means(_ptr(labels), _TTA_LABEL_BYTES[labels.dtype], _ptr(values), labels.numel(), int(k),
                                _ptr(sums), _ptr(counts), _stream()), "label_means")
    return sums, counts


# ------------------------------------------------------------------ image ops
_PIXEL ={torch.float32: 0, torch.uint8: 1, torch.int16: 2, torch.int32: 3, torch.uint16: 4}


def resample3d(src: torch.Tensor, out_size_zyx, index_map, nearest=False, default=0.0, border=False,
               half_even=False):
    """src [z,y,x] -> dst [z,y,x]; index_map: 3x4 out-index(x,y,z,1) -> in-index(x,y,z).
    ``border``: clamp the continuous index to the buffer (MONAI ``padding_mode="border"``) instead
    of ITK's default-pixel-outside rule.  ``half_even`` (nearest only): round x.5 to the even index
    (torch ``grid_sample`` / MONAI) instead of up (ITK)."""
    _require_device(src)
    if src.dim() != 3 or not src.is_contiguous():
        raise ValueError("resample3d expects a contiguous [z,y,x] tensor")
    dz, dy, dx = (int(v) for v in out_size_zyx)
    dst = torch.empty((dz, dy, dx), dtype=src.dtype, device=src.device)
    m = np.ascontiguousarray(np.asarray(index_map, dtype=np.float64).reshape(12))
    sz, sy, sx = src.shape
    check(lib.segmi_resample3d(_PIXEL[src.dtype], _ptr(src), sx, sy, sz, _ptr(dst), dx, dy, dz,
                               m.ctypes.data_as(C.c_void_p), (1 if nearest else 0) | (2 if border else 0) | (4 if nearest and half_even else 0),
                               float(default), _stream()), "resample3d")
    return dst


# workgroups x threads one launch of the B-spline evaluate / label-Gaussian kernels covers before it strides
# (SEGMI_RESAMPLE_HQ_GRID_CAP in include/segmi.h)
RESAMPLE_HQ_GRID_LANES = 2048 * 256


def _resample_args(name: str, src: torch.Tensor, out_size_zyx, index_map):
    _require_device(src)
    if src.dim() != 3 or not src.is_contiguous():
        raise ValueError(f"{name} expects a contiguous [z,y,x] tensor")
    if src.dtype not in _PIXEL:
        raise TypeError(f"{name}: unsupported pixel type {src.dtype}")
    dz, dy, dx = (int(v) for v in out_size_zyx)
    dst = torch.empty((dz, dy, dx), dtype=src.dtype, device=src.device)
    m = np.ascontiguousarray(np.asarray(index_map, dtype=np.float64).reshape(12))
    return dst, m


def bspline_coefficients(src: torch.Tensor) -> torch.Tensor:
    """Cubic B-spline coefficients of src [z,y,x] (any pixel type) as a float64 tensor of the same shape: the
    recursive prefilter with whole-sample mirror boundaries (``scipy.ndimage.spline_filter(order=3, mode="mirror")``)."""
    _require_device(src)
    if src.dim() != 3 or not src.is_contiguous():
        raise ValueError("bspline_coefficients expects a contiguous [z,y,x] tensor")
    if src.dtype not in _PIXEL:
        raise TypeError(f"bspline_coefficients: unsupported pixel type {src.dtype}")
    sz, sy, sx = src.shape
    coef = torch.empty(int(lib.segmi_bspline_workspace(sx, sy, sz)) // 8, dtype=torch.float64,
                       device=src.device).view(sz, sy, sx)
    check(lib.segmi_bspline_prefilter(_PIXEL[src.dtype], _ptr(src), sx, sy, sz, _ptr(coef), _stream()),
          "bspline_prefilter")
    return coef


def resample3d_bspline(src: torch.Tensor, out_size_zyx, index_map, default=0.0, border=False, coef=None):
    """``resample3d`` with cubic B-spline interpolation (``map_coordinates(order=3, mode="mirror")``).  ``coef``:
    the result of ``bspline_coefficients(src)``, to resample one image onto several grids without refiltering."""
    dst, m = _resample_args("resample3d_bspline", src, out_size_zyx, index_map)
    if coef is None:
        coef = bspline_coefficients(src)
    _require_device(coef)
    if coef.dtype != torch.float64 or coef.shape != src.shape or not coef.is_contiguous() or coef.device != src.device:
        raise ValueError("resample3d_bspline: coef must be the contiguous float64 result of bspline_coefficients(src)")
    sz, sy, sx = src.shape
    dz, dy, dx = dst.shape
    check(lib.segmi_resample3d_bspline(_ptr(coef), sx, sy, sz, _PIXEL[src.dtype], _ptr(dst), dx, dy, dz,
                                       m.ctypes.data_as(C.c_void_p), 1 if border else 0, float(default), _stream()),
          "resample3d_bspline")
    return dst


def resample3d_label_gaussian(src: torch.Tensor, out_size_zyx, index_map, sigma=1.0, alpha=2.0, default=0.0,
                              border=False):
    """``resample3d`` of a label map with the label-Gaussian vote.  ``sigma``: a number or (x, y, z), in input
    voxels; the window radius is ceil(alpha * sigma) per axis (at most 8)."""
    dst, m = _resample_args("resample3d_label_gaussian", src, out_size_zyx, index_map)
    sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,)))
    sz, sy, sx = src.shape
    dz, dy, dx = dst.shape
    check(lib.segmi_resample3d_label_gaussian(_PIXEL[src.dtype], _ptr(src), sx, sy, sz, _ptr(dst), dx, dy, dz,
                                              m.ctypes.data_as(C.c_void_p), sg.ctypes.data_as(C.c_void_p),
                                              float(alpha), 1 if border else 0, float(default), _stream()),
          "resample3d_label_gaussian")
    return dst


# ------------------------------------------------------------------ registration (registration.hip)
JOINT_HIST_BINS = (16, 32, 64)
JOINT_HIST_MAX_CANDIDATES = 32        # SEGMI_JOINT_HIST_MAX_CANDIDATES
JOINT_HIST_GRID_CAP = 1024            # SEGMI_JOINT_HIST_GRID_CAP: workgroups of 256 per candidate group
JOINT_HIST_UNIT = 1 << 16             # fixed-point weight of one sample: table sums / JOINT_HIST_UNIT count samples
FIXED_BIN_IGNORE = 255


def _pixel_volume(name: str, t: torch.Tensor) -> None:
    _require_device(t)
    if t.dim() != 3 or not t.is_contiguous() or t.numel() == 0:
        raise ValueError(f"{name} expects a contiguous, non-empty [z,y,x] tensor, got shape {tuple(t.shape)}")
    if t.dtype not in _PIXEL:
        raise TypeError(f"{name}: unsupported pixel type {t.dtype}")


def shrink_factors(shape_zyx, factor: int):
    """Per-axis (z, y, x) block factors of the pyramid level ``factor``: the factor halved until the axis keeps
    at least 8 blocks; an axis of extent 1 always gets 1."""
    if factor not in (1, 2, 4, 8):
        raise ValueError(f"a pyramid level is 1, 2, 4 or 8, got {factor!r}")
    out = []
    for n in shape_zyx:
        f = int(factor)
        while f > 1 and (int(n) == 1 or int(n) // f < 8):
            f //= 2
        out.append(f)
    return tuple(out)


def bin_shrink(src: torch.Tensor, factors_zyx) -> torch.Tensor:
    """Block means of src [z,y,x] (any pixel type) as float32 [z // fz, y // fy, x // fx]: each block summed in
    float64 (x innermost, z outermost), divided by its count; tail samples are dropped."""
    _pixel_volume("bin_shrink", src)
    fz, fy, fx = (int(v) for v in factors_zyx)
    sz, sy, sx = src.shape
    if min(fz, fy, fx) < 1 or max(fz, fy, fx) > 8 or fz > sz or fy > sy or fx > sx:
        raise ValueError(f"bin_shrink: factors {tuple(factors_zyx)} must lie in 1 .. 8 and within {tuple(src.shape)}")
    dst = torch.empty((sz // fz, sy // fy, sx // fx), dtype=torch.float32, device=src.device)
    check(lib.segmi_bin_shrink(_PIXEL[src.dtype], _ptr(src), sx, sy, sz, fx, fy, fz, _ptr(dst), _stream()),
          "bin_shrink")
    return dst


def fixed_bins(image: torch.Tensor, lo: float, hi: float, bins: int, mask_mean: Optional[torch.Tensor] = None):
    """uint8 bin volume of a float32 level image: clamp(floor((v - lo) * ((bins-1)/(hi-lo)) + 0.5), 0, bins-1), and
    ``FIXED_BIN_IGNORE`` where ``mask_mean`` (float32, same shape) is below 0.5."""
    _pixel_volume("fixed_bins", image)
    if image.dtype != torch.float32:
        raise TypeError(f"fixed_bins: the level image is float32, not {image.dtype}")
    if bins not in JOINT_HIST_BINS:
        raise ValueError(f"bins must be one of {JOINT_HIST_BINS}, got {bins!r}")
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"fixed_bins: constant or non-finite image (lo {lo}, hi {hi})")
    if mask_mean is not None:
        _pixel_volume("fixed_bins", mask_mean)
        if mask_mean.dtype != torch.float32 or mask_mean.shape != image.shape or mask_mean.device != image.device:
            raise ValueError("fixed_bins: mask_mean must be float32 of the image's shape")
    out = torch.empty(image.shape, dtype=torch.uint8, device=image.device)
    check(lib.segmi_fixed_bins(_ptr(image), _ptr(mask_mean), image.numel(), float(lo), float(hi), int(bins), _ptr(out),
                               _stream()), "fixed_bins")
    return out


def joint_histogram_group(bins: int) -> int:
    """candidates that one workgroup of ``joint_histogram`` holds in LDS at a time (0: bins not supported)"""
    return int(lib.segmi_joint_histogram_group(int(bins)))


def joint_histogram(fixed_bin: torch.Tensor, moving: torch.Tensor, index_maps, bins: int, mlo: float, mscale: float):
    """int64 [T, bins, bins] joint histograms (fixed bin, moving bin) of the uint8 bin volume ``fixed_bin`` and
    ``moving`` (any pixel type) under T <= 32 index maps [T, 3, 4] (fixed index -> continuous moving index), in one
    launch; weights are fixed point, ``JOINT_HIST_UNIT`` per sample."""
    _pixel_volume("joint_histogram", fixed_bin)
    _pixel_volume("joint_histogram", moving)
    if fixed_bin.dtype != torch.uint8:
        raise TypeError(f"joint_histogram: fixed bins are uint8, not {fixed_bin.dtype}")
    if moving.device != fixed_bin.device:
        raise ValueError("joint_histogram: fixed bins and moving image live on different devices")
    if bins not in JOINT_HIST_BINS:
        raise ValueError(f"bins must be one of {JOINT_HIST_BINS}, got {bins!r}")
    m = np.ascontiguousarray(np.asarray(index_maps, dtype=np.float64))
    if m.ndim != 3 or m.shape[1:] != (3, 4) or not 1 <= m.shape[0] <= JOINT_HIST_MAX_CANDIDATES:
        raise ValueError(f"index_maps must be [T, 3, 4] with 1 <= T <= {JOINT_HIST_MAX_CANDIDATES}, got {m.shape}")
    if not (math.isfinite(mlo) and math.isfinite(mscale)):
        raise ValueError(f"joint_histogram: mlo / mscale must be finite, got {mlo}, {mscale}")
    T = m.shape[0]
    out = torch.empty((T, bins, bins), dtype=torch.int64, device=fixed_bin.device)
    fz, fy, fx = fixed_bin.shape
    mz, my, mx = moving.shape
    check(lib.segmi_joint_histogram(_ptr(fixed_bin), fx, fy, fz, _PIXEL[moving.dtype], _ptr(moving), mx, my, mz,
                                    m.ctypes.data_as(C.c_void_p), T, int(bins), float(mlo), float(mscale), _ptr(out),
                                    _stream()), "joint_histogram")
    return out


# ------------------------------------------------------------------ deformable registration (deformable.hip)
FFD_MAX_CONTROL_POINTS = 32768        # SEGMI_FFD_MAX_CONTROL_POINTS
FFD_MAX_CANDIDATES = 8                # SEGMI_FFD_MAX_CANDIDATES
FFD_HIST_GRID_CAP = 1024              # SEGMI_FFD_HIST_GRID_CAP
FFD_GRADIENT_GRID_CAP = 8             # SEGMI_FFD_GRADIENT_GRID_CAP: workgroups of 256 per control cell
FFD_JACOBIAN_GRID_CAP = 1024          # SEGMI_FFD_JACOBIAN_GRID_CAP
FFD_WARP_GRID_CAP = 1024              # SEGMI_FFD_WARP_GRID_CAP
FFD_GRADIENT_MAX_SUPPORT = 1 << 20    # SEGMI_FFD_GRADIENT_MAX_SUPPORT: launch voxels under one control point
FFD_QD_UNIT = 1 << 15                 # the derivative table and the image gradient are quantised to +- 2^15
FFD_WEIGHT_UNIT = 1 << 12             # a B-spline tensor weight is quantised to 0 .. 2^12


def _ffd_grid(name: str, level_zyx, full_zyx, factors_zyx, control: torch.Tensor, candidates: bool):
    """the ``segmi_ffd_grid`` of a launch and its control tensor, checked: control is float64 [3, nz, ny, nx] (or
    [T, 3, nz, ny, nx] with ``candidates``)"""
    from ._lib import FfdGrid
    _require_device(control)
    want = 5 if candidates else 4
    if control.dtype != torch.float64 or control.dim() != want or control.shape[-4] != 3 or not control.is_contiguous():
        raise ValueError(f"{name}: the control grid is a contiguous float64 {'[T, ' if candidates else '['}3, nz, ny, nx] "
                         f"tensor, got {control.dtype} {tuple(control.shape)}")
    nz, ny, nx = (int(v) for v in control.shape[-3:])
    if min(nz, ny, nx) < 4:
        raise ValueError(f"{name}: a control grid has at least 4 points per axis, got (nz, ny, nx) = {(nz, ny, nx)}")
    if nz * ny * nx > FFD_MAX_CONTROL_POINTS:
        raise ValueError(f"{name}: {nz * ny * nx} control points, at most {FFD_MAX_CONTROL_POINTS}")
    lz, ly, lx = (int(v) for v in level_zyx)
    dz, dy, dx = (int(v) for v in full_zyx)
    fz, fy, fx = (int(v) for v in factors_zyx)
    if min(fz, fy, fx) < 1 or max(fz, fy, fx) > 8 or lz * fz > dz or ly * fy > dy or lx * fx > dx or min(lz, ly, lx) < 1:
        raise ValueError(f"{name}: level grid {(lz, ly, lx)} with factors {(fz, fy, fx)} does not fit the fixed "
                         f"extent {(dz, dy, dx)}")
    return FfdGrid(lx, ly, lz, dx, dy, dz, fx, fy, fz, nx, ny, nz)


def _ffd_maps(name: str, index_map, r):
    m = np.ascontiguousarray(np.asarray(index_map, dtype=np.float64))
    rr = np.ascontiguousarray(np.asarray(r, dtype=np.float64))
    if m.shape != (3, 4) or rr.shape != (3, 3) or not (np.isfinite(m).all() and np.isfinite(rr).all()):
        raise ValueError(f"{name}: index_map is a finite [3, 4] and r a finite [3, 3] matrix, got {m.shape}, {rr.shape}")
    return m, rr


def ffd_joint_histogram(fixed_bin: torch.Tensor, moving: torch.Tensor, control: torch.Tensor, full_zyx, factors_zyx,
                        index_map, r, bins: int, mlo: float, mscale: float) -> torch.Tensor:
    """int64 [T, bins, bins] joint histograms of ``fixed_bin`` (uint8 level volume) and ``moving`` under T <= 8
    candidate control grids ``control`` float64 [T, 3, nz, ny, nx] (mm along the fixed array axes, components x, y, z)
    in one launch.  ``full_zyx`` / ``factors_zyx``: the full-resolution fixed extent and the level's block factors;
    ``index_map`` [3, 4]: level index -> moving index of the affine part; ``r`` [3, 3]: mm of displacement -> moving
    index units.  All-zero grids give ``joint_histogram(fixed_bin, moving, [index_map], ...)`` bit for bit."""
    _pixel_volume("ffd_joint_histogram", fixed_bin)
    _pixel_volume("ffd_joint_histogram", moving)
    if fixed_bin.dtype != torch.uint8:
        raise TypeError(f"ffd_joint_histogram: fixed bins are uint8, not {fixed_bin.dtype}")
    if moving.device != fixed_bin.device or control.device != fixed_bin.device:
        raise ValueError("ffd_joint_histogram: fixed bins, moving image and control grid live on different devices")
    if bins not in JOINT_HIST_BINS:
        raise ValueError(f"bins must be one of {JOINT_HIST_BINS}, got {bins!r}")
    g = _ffd_grid("ffd_joint_histogram", fixed_bin.shape, full_zyx, factors_zyx, control, True)
    T = int(control.shape[0])
    if not 1 <= T <= FFD_MAX_CANDIDATES:
        raise ValueError(f"ffd_joint_histogram: 1 .. {FFD_MAX_CANDIDATES} candidate grids per call, got {T}")
    m, rr = _ffd_maps("ffd_joint_histogram", index_map, r)
    if not (math.isfinite(mlo) and math.isfinite(mscale)):
        raise ValueError(f"ffd_joint_histogram: mlo / mscale must be finite, got {mlo}, {mscale}")
    out = torch.empty((T, bins, bins), dtype=torch.int64, device=fixed_bin.device)
    mz, my, mx = moving.shape
    check(lib.segmi_ffd_joint_histogram(_ptr(fixed_bin), C.byref(g), _ptr(control), T, _PIXEL[moving.dtype],
                                        _ptr(moving), mx, my, mz, m.ctypes.data_as(C.c_void_p),
                                        rr.ctypes.data_as(C.c_void_p), int(bins), float(mlo), float(mscale), _ptr(out),
                                        _stream()), "ffd_joint_histogram")
    return out


def ffd_gradient(fixed_bin: torch.Tensor, moving: torch.Tensor, control: torch.Tensor, full_zyx, factors_zyx,
                 index_map, r, bins: int, mlo: float, mscale: float, gscale: float, qd: torch.Tensor) -> torch.Tensor:
    """int64 [3, nz, ny, nx]: the integer gradient of the metric by the control values of ``control`` float64
    [3, nz, ny, nx].  ``qd``: int32 [bins, bins - 1], the quantised derivative table (|qd| <= 2^15); ``gscale``
    scales the image gradient into -1 .. 1.  Units: ``FFD_QD_UNIT`` ^ 2 * ``FFD_WEIGHT_UNIT`` = 2^42."""
    _pixel_volume("ffd_gradient", fixed_bin)
    _pixel_volume("ffd_gradient", moving)
    if fixed_bin.dtype != torch.uint8:
        raise TypeError(f"ffd_gradient: fixed bins are uint8, not {fixed_bin.dtype}")
    if bins not in JOINT_HIST_BINS:
        raise ValueError(f"bins must be one of {JOINT_HIST_BINS}, got {bins!r}")
    _require_device(qd)
    if qd.dtype != torch.int32 or tuple(qd.shape) != (bins, bins - 1) or not qd.is_contiguous():
        raise ValueError(f"ffd_gradient: qd is a contiguous int32 [{bins}, {bins - 1}] tensor, got {qd.dtype} "
                         f"{tuple(qd.shape)}")
    if not {moving.device, control.device, qd.device} == {fixed_bin.device}:
        raise ValueError("ffd_gradient: the tensors live on different devices")
    g = _ffd_grid("ffd_gradient", fixed_bin.shape, full_zyx, factors_zyx, control, False)
    support = 1
    for l, n in zip(fixed_bin.shape, control.shape[-3:]):
        support *= min(int(l), -(-4 * int(l) // (int(n) - 3)) + 1)
    if support > FFD_GRADIENT_MAX_SUPPORT:
        raise ValueError(f"ffd_gradient: {support} samples under one control point's support, at most "
                         f"{FFD_GRADIENT_MAX_SUPPORT}: use more control points (a smaller grid_spacing)")
    m, rr = _ffd_maps("ffd_gradient", index_map, r)
    if not (math.isfinite(mlo) and math.isfinite(mscale) and math.isfinite(gscale)):
        raise ValueError(f"ffd_gradient: mlo / mscale / gscale must be finite, got {mlo}, {mscale}, {gscale}")
    out = torch.empty(tuple(control.shape), dtype=torch.int64, device=fixed_bin.device)
    mz, my, mx = moving.shape
    check(lib.segmi_ffd_gradient(_ptr(fixed_bin), C.byref(g), _ptr(control), _PIXEL[moving.dtype], _ptr(moving), mx,
                                 my, mz, m.ctypes.data_as(C.c_void_p), rr.ctypes.data_as(C.c_void_p), int(bins),
                                 float(mlo), float(mscale), float(gscale), _ptr(qd), _ptr(out), _stream()),
          "ffd_gradient")
    return out


def ffd_jacobian(control: torch.Tensor, level_zyx, full_zyx, factors_zyx, inv_spacing_xyz, want_map: bool = False):
    """(folded, min_jacobian, map): the number of voxels of the level grid where det(I + du/ds) <= 0, the smallest
    determinant, and (``want_map``) the determinants as float32 [lz, ly, lx] (else None).  ``inv_spacing_xyz``:
    1 / control spacing in mm per axis (x, y, z), 0 on an axis of extent 1.  The two numbers are device tensors
    (int64 [1], float64 [1]): the caller reads them back."""
    g = _ffd_grid("ffd_jacobian", level_zyx, full_zyx, factors_zyx, control, False)
    ih = np.ascontiguousarray(np.asarray(inv_spacing_xyz, dtype=np.float64))
    if ih.shape != (3,) or not np.isfinite(ih).all():
        raise ValueError(f"ffd_jacobian: inv_spacing_xyz holds three finite numbers, got {inv_spacing_xyz!r}")
    folded = torch.empty(1, dtype=torch.int64, device=control.device)
    lowest = torch.empty(1, dtype=torch.float64, device=control.device)
    dmap = (torch.empty(tuple(int(v) for v in level_zyx), dtype=torch.float32, device=control.device)
            if want_map else None)
    check(lib.segmi_ffd_jacobian(C.byref(g), _ptr(control), ih.ctypes.data_as(C.c_void_p), _ptr(folded), _ptr(lowest),
                                 _ptr(dmap), _stream()), "ffd_jacobian")
    return folded, lowest, dmap


def ffd_warp(moving: Optional[torch.Tensor], control: torch.Tensor, full_zyx, index_map, r, nearest: bool = False,
             default: float = 0.0, direction=None, want_displacement: bool = False):
    """(warped, displacement): ``moving`` resampled onto the full-resolution fixed grid ``full_zyx`` through the
    transform (its pixel type; None when ``moving`` is None), and (``want_displacement``) the dense displacement
    float32 [3, z, y, x] in mm along the physical axes, ``direction`` [3, 3] being the fixed direction matrix."""
    g = _ffd_grid("ffd_warp", full_zyx, full_zyx, (1, 1, 1), control, False)
    if moving is None and not want_displacement:
        raise ValueError("ffd_warp: neither a moving image nor a displacement field was asked for")
    m, rr = _ffd_maps("ffd_warp", index_map, r)
    mx = my = mz = 0
    pixel, dst = 0, None
    if moving is not None:
        _pixel_volume("ffd_warp", moving)
        if moving.device != control.device:
            raise ValueError("ffd_warp: moving image and control grid live on different devices")
        mz, my, mx = moving.shape
        pixel = _PIXEL[moving.dtype]
        dst = torch.empty(tuple(int(v) for v in full_zyx), dtype=moving.dtype, device=control.device)
    dd, disp = None, None
    if want_displacement:
        dd = np.ascontiguousarray(np.asarray(direction, dtype=np.float64))
        if dd.shape != (3, 3) or not np.isfinite(dd).all():
            raise ValueError("ffd_warp: a displacement field needs the finite [3, 3] fixed direction matrix")
        disp = torch.empty((3,) + tuple(int(v) for v in full_zyx), dtype=torch.float32, device=control.device)
    if not math.isfinite(default):
        raise ValueError(f"ffd_warp: default must be finite, got {default}")
    check(lib.segmi_ffd_warp(C.byref(g), _ptr(control), pixel, _ptr(moving), mx, my, mz, m.ctypes.data_as(C.c_void_p),
                             rr.ctypes.data_as(C.c_void_p), 1 if nearest else 0, float(default), _ptr(dst),
                             None if dd is None else dd.ctypes.data_as(C.c_void_p), _ptr(disp), _stream()), "ffd_warp")
    return dst, disp


def normalize_intensity_(x: torch.Tensor) -> torch.Tensor:
    """in-place channel-wise (x-mean)/std of a contiguous f32 [C, ...] tensor."""
    _require_device(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("normalize_intensity_ expects contiguous float32")
    c = x.shape[0]
    nvox = x.numel() // c
    ws = torch.empty(int(lib.segmi_normalize_workspace(c, nvox)), dtype=torch.uint8,
                     device=x.device)
    check(lib.segmi_normalize_intensity(_ptr(x), c, nvox, _ptr(ws), _stream()),
          "normalize_intensity")
    return x


AUG_MAX_PATCHES = 16    # patches per segmi_crop_patches / warp_crop / intensity / kspace call (kMaxCrops)


def _patch_chunks(name, native, image, label, starts, flips, out_image, out_label) -> None:
    """The chunk loop of the three sampler gathers, one launch per 16 patches.  ``native(a, label, starts, flips,
    n, dst_dtype, out, out_label)`` is the library call, given the arguments every one of them takes."""
    a = act(image)
    fl = None if flips is None else np.asarray(flips, dtype=np.uint8).reshape(-1)
    for i in range(0, len(starts), AUG_MAX_PATCHES):
        arr, p = _starts(starts[i:i + AUG_MAX_PATCHES], 4)
        n = arr.shape[0]
        b = act(out_image[i:i + n])
        f = None if fl is None else np.ascontiguousarray(fl[i:i + n])
        check(native(C.byref(a), _ptr(label), p, None if f is None else f.ctypes.data_as(C.c_void_p), n,
                     dtype_code(out_image), C.byref(b), _ptr(None if out_label is None else out_label[i:i + n])),
              name)


def crop_patches(image, label, starts, flips, out_image, out_label) -> None:
    """``len(starts)`` crops (any number: one launch per 16) of ``image`` / ``label`` into
    ``out_image`` / ``out_label``."""
    _patch_chunks("crop_patches", lambda a, lab, p, fl, n, dt, b, ol: lib.segmi_crop_patches(
        a, lab, p, fl, n, dt, b, ol, _stream()), image, label, starts, flips, out_image, out_label)


def warp_crop_patches(image, label, starts, flips, index_map, out_image, out_label) -> None:
    """crop_patches with a 3x4 affine (augmented index (x,y,z,1) -> source index) composed in."""
    m = np.ascontiguousarray(np.asarray(index_map, dtype=np.float64).reshape(12))
    _patch_chunks("warp_crop_patches", lambda a, lab, p, fl, n, dt, b, ol: lib.segmi_warp_crop_patches(
        a, lab, p, fl, n, m.ctypes.data_as(C.c_void_p), dt, b, ol, _stream()),
        image, label, starts, flips, out_image, out_label)


def elastic_warp_crop_patches(image, label, starts, flips, index_map, control, out_image, out_label) -> None:
    """warp_crop_patches with a cubic B-spline displacement field added to the augmented index before
    the affine map (``index_map`` None = identity).  ``control``: contiguous f32 device tensor
    [3, n0, n1, n2] of displacements in voxels."""
    from .seg.augment import ELASTIC_MAX_CONTROL      # kMaxControl; seg.augment is numpy-only and imports nothing of ops
    _require_device(control)
    if control.dtype != torch.float32 or control.dim() != 4 or control.shape[0] != 3 or not control.is_contiguous():
        raise ValueError("elastic_warp_crop_patches: contiguous float32 [3, n0, n1, n2] control grid expected")
    n0, n1, n2 = (int(v) for v in control.shape[1:])
    if min(n0, n1, n2) < 4 or n0 * n1 * n2 > ELASTIC_MAX_CONTROL:
        raise ValueError(f"elastic_warp_crop_patches: control grid {n0} x {n1} x {n2}: at least 4 points per axis "
                         f"and at most {ELASTIC_MAX_CONTROL} in all")
    m = None if index_map is None else np.ascontiguousarray(np.asarray(index_map, dtype=np.float64).reshape(12))
    mp = None if m is None else m.ctypes.data_as(C.c_void_p)
    _patch_chunks("elastic_warp_crop_patches",
                  lambda a, lab, p, fl, n, dt, b, ol: lib.segmi_elastic_warp_crop_patches(
                      a, lab, p, fl, n, mp, _ptr(control), n0, n1, n2, dt, b, ol, _stream()),
                  image, label, starts, flips, out_image, out_label)


def _host_arrays():
    keep = []

    def arr(x, dt, i, n):
        if x is None:
            return None
        a = np.ascontiguousarray(np.asarray(x, dtype=dt)[i:i + n])
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)
    return arr


def intensity_augment(patches, contrast=None, hist=None, bias=None) -> None:
    """In-place RandAdjustContrast / RandHistogramShift / RandBiasField on f32 NDHWC patches.

    contrast = (on uint8[n], gamma f32[n]); hist = (on, ctrl f32[n][k]); bias = (on, coef f32[n][20]).
    Any n: one call per 16 patches (every transform is per patch)."""
    _require_device(patches)
    if patches.dtype != torch.float32 or patches.dim() != 5 or not patches.is_contiguous():
        raise ValueError("intensity_augment: dense float32 [n, d, h, w, c] patches expected")
    N, rd, rh, rw, c = patches.shape
    con, gam = (contrast if contrast is not None else (None, None))
    hon, ctl = (hist if hist is not None else (None, None))
    bon, cof = (bias if bias is not None else (None, None))
    nctrl = int(np.asarray(ctl).shape[1]) if ctl is not None else 0
    ws = torch.empty(int(lib.segmi_intensity_workspace(min(N, AUG_MAX_PATCHES))), dtype=torch.uint8,
                     device=patches.device)
    for i in range(0, N, AUG_MAX_PATCHES):
        n = min(AUG_MAX_PATCHES, N - i)
        arr = _host_arrays()
        check(lib.segmi_intensity_augment(_ptr(patches[i:i + n]), n, rd, rh, rw, c, arr(con, np.uint8, i, n),
                                          arr(gam, np.float32, i, n), arr(hon, np.uint8, i, n),
                                          arr(ctl, np.float32, i, n), nctrl, arr(bon, np.uint8, i, n),
                                          arr(cof, np.float32, i, n), _ptr(ws), _stream()),
              "intensity_augment")


def kspace_augment(patches, gibbs=None, spike=None, flips=None) -> None:
    """In-place RandGibbsNoise / RandKSpaceSpikeNoise on f32 NDHWC patches.

    gibbs = (on uint8[n], alpha f32[n]); spike = (on uint8[n], loc int32[n][3] (z,y,x), u f32[n]).
    ``flips`` (uint8[n], bit 0 = z, 1 = y, 2 = x): the patches were flipped before this call and the
    reference flips after it -- the Gibbs mask is evaluated at the mirrored bin (the spike location
    must come mirrored already: ``seg.augment.flip_params``).  Any n: one call per 16 patches."""
    _require_device(patches)
    if patches.dtype != torch.float32 or patches.dim() != 5 or not patches.is_contiguous():
        raise ValueError("kspace_augment: dense float32 [n, d, h, w, c] patches expected")
    N, rd, rh, rw, c = patches.shape
    gon, alpha = gibbs if gibbs is not None else (None, None)
    son, loc, u = spike if spike is not None else (None, None, None)
    ws = None
    for i in range(0, N, AUG_MAX_PATCHES):
        n = min(AUG_MAX_PATCHES, N - i)
        nsel = max(int(np.asarray(gon)[i:i + n].astype(bool).sum()) if gon is not None else 0,
                   int(np.asarray(son)[i:i + n].astype(bool).sum()) if son is not None else 0)
        if nsel == 0:
            continue
        if ws is None:
            ws = torch.empty(int(lib.segmi_kspace_workspace(min(N, AUG_MAX_PATCHES), rd, rh, rw)),
                             dtype=torch.uint8, device=patches.device)
        arr = _host_arrays()
        check(lib.segmi_kspace_augment(_ptr(patches[i:i + n]), n, rd, rh, rw, c, arr(gon, np.uint8, i, n),
                                       arr(alpha, np.float32, i, n), arr(son, np.uint8, i, n),
                                       arr(loc, np.int32, i, n), arr(u, np.float32, i, n),
                                       arr(flips, np.uint8, i, n), _ptr(ws), _stream()), "kspace_augment")


DEGRADE_MAX_RADIUS = 8      # blur radius floor(4 sigma + 0.5) the kernel stages (kMaxRadius): sigma <= 2.0


def degrade_augment(patches, noise=None, blur=None, brightness=None, lowres=None) -> None:
    """In-place noise / blur / brightness / low-resolution augmentation (``augment_degrade``)
    on f32 NDHWC patches, in that order.

    noise = (on uint8[n], variance f32[n], seed uint32[n]); blur = (on, sigma f32[n], voxels);
    brightness = (on, multiplier f32[n]); lowres = (on, m int32[n][3], the coarse extents (d0, d1, d2)).
    None skips a transform.  Any n: one call per 16 patches; the workspace is allocated only when a blur or
    a lowres fires."""
    _require_device(patches)
    if patches.dtype != torch.float32 or patches.dim() != 5 or not patches.is_contiguous():
        raise ValueError("degrade_augment: dense float32 [n, d, h, w, c] patches expected")
    N, rd, rh, rw, c = patches.shape
    non, var, seed = noise if noise is not None else (None, None, None)
    bon, sigma = blur if blur is not None else (None, None)
    ron, mult = brightness if brightness is not None else (None, None)
    lon, coarse = lowres if lowres is not None else (None, None)
    if bon is not None:
        bad = [float(s) for o, s in zip(np.asarray(bon), np.asarray(sigma, dtype=np.float64))
               if o and not (s > 0.0 and np.floor(4.0 * s + 0.5) <= DEGRADE_MAX_RADIUS)]
        if bad:
            raise ValueError(f"degrade_augment: blur sigma {bad}: 0 < sigma and a radius floor(4 sigma + 0.5) of at "
                             f"most {DEGRADE_MAX_RADIUS} (sigma <= 2.0) expected")
    ws = None
    for i in range(0, N, AUG_MAX_PATCHES):
        n = min(AUG_MAX_PATCHES, N - i)
        fired = [np.asarray(o)[i:i + n].astype(bool) for o in (non, bon, ron, lon) if o is not None]
        if not any(f.any() for f in fired):
            continue
        if ws is None and any(np.asarray(o)[i:i + n].any() for o in (bon, lon) if o is not None):
            ws = torch.empty(int(lib.segmi_degrade_workspace(min(N, AUG_MAX_PATCHES), rd, rh, rw, c)),
                             dtype=torch.uint8, device=patches.device)
        arr = _host_arrays()
        check(lib.segmi_degrade_augment(_ptr(patches[i:i + n]), n, rd, rh, rw, c, arr(non, np.uint8, i, n),
                                        arr(var, np.float32, i, n), arr(seed, np.uint32, i, n),
                                        arr(bon, np.uint8, i, n), arr(sigma, np.float32, i, n),
                                        arr(ron, np.uint8, i, n), arr(mult, np.float32, i, n),
                                        arr(lon, np.uint8, i, n), arr(coarse, np.int32, i, n), _ptr(ws), _stream()),
              "degrade_augment")


def _ptr_table(tensors, dtype):
    for t in tensors:
        _require_device(t)
        if t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"ensemble: contiguous {dtype} tensors expected")
    tab = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return tab


def ensemble_mean(logits, weights, out) -> None:
    """out = mean_e(logits[e] * w[e] / mean(w)) over same-shaped f32 tensors (MONAI MeanEnsemble)."""
    tab = _ptr_table(list(logits) + [out], torch.float32)
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32)) if weights is not None else None
    check(lib.segmi_ensemble_mean(tab, w.ctypes.data_as(C.c_void_p) if w is not None else None,
                                  len(logits), out.numel(), _ptr(out), _stream()), "ensemble_mean")


def ensemble_vote(labels, out) -> None:
    tab = _ptr_table(list(labels) + [out], torch.int32)
    check(lib.segmi_ensemble_vote(tab, len(labels), out.numel(), _ptr(out), _stream()), "ensemble_vote")


def ensemble_select(labels, tissue_model: dict, out) -> None:
    """SelectBestEnsemble: tissue_model = {tissue id: model index}, applied in dict order."""
    tab = _ptr_table(list(labels) + [out], torch.int32)
    ts = np.ascontiguousarray(np.asarray(list(tissue_model.keys()), dtype=np.int32))
    ms = np.ascontiguousarray(np.asarray(list(tissue_model.values()), dtype=np.int32))
    check(lib.segmi_ensemble_select(tab, len(labels), ts.ctypes.data_as(C.c_void_p),
                                    ms.ctypes.data_as(C.c_void_p), len(ts), out.numel(), _ptr(out),
                                    _stream()), "ensemble_select")


# ------------------------------------------------------------------ STAPLE label fusion (staple.hip)
STAPLE_MAX_RATERS = 16
STAPLE_MAX_CLASSES = 64
STAPLE_Q = 1 << 24            # fixed-point unit of the posteriors: sums / STAPLE_Q are expected voxel counts
STAPLE_MIN_PRIOR = 1e-12      # smallest share of a caller-supplied prior entry in the prior's sum


def staple_check_args(raters: int, num_classes, prior, max_iterations, tolerance):
    """The argument checks of ``staple`` that need no tensor; returns the prior as a host f64 array or None."""
    if not 1 <= int(raters) <= STAPLE_MAX_RATERS:
        raise ValueError(f"labels: 1 .. {STAPLE_MAX_RATERS} raters, got {raters}")
    if int(num_classes) != num_classes or not 2 <= int(num_classes) <= STAPLE_MAX_CLASSES:
        raise ValueError(f"num_classes must be an integer in 2 .. {STAPLE_MAX_CLASSES}, got {num_classes}")
    if int(max_iterations) != max_iterations or int(max_iterations) < 1:
        raise ValueError(f"max_iterations must be an integer >= 1, got {max_iterations}")
    if not (math.isfinite(float(tolerance)) and float(tolerance) >= 0.0):
        raise ValueError(f"tolerance must be finite and >= 0, got {tolerance}")
    if prior is None:
        return None
    p = np.ascontiguousarray(np.asarray(prior, dtype=np.float64))
    if p.shape != (int(num_classes),) or not np.isfinite(p).all():
        raise ValueError(f"prior must hold num_classes = {int(num_classes)} finite values")
    total = float(p.sum())
    if not total > 0.0 or not (p / total >= STAPLE_MIN_PRIOR).all():
        raise ValueError(f"prior: every entry must be at least {STAPLE_MIN_PRIOR} of the prior's sum")
    return p


def staple_table_name(raters: int, num_classes: int) -> str:
    """"lds" or "global": where the passes of ``staple`` accumulate S for this shape (the launch's own choice)"""
    return lib.segmi_staple_table_name(int(raters), int(num_classes)).decode()


def staple(labels, num_classes, *, prior=None, max_iterations=100, tolerance=1e-5, return_posterior=False):
    """Multi-label STAPLE fusion of 1 .. 16 label volumes (device tensors of one dtype among uint8 / int16 / int32,
    contiguous, of equal shape; labels in 0 .. num_classes - 1).  Returns (labels in the input dtype, sums int64
    [R, L, L] of the last M-step, prior float64 [L], iterations, converged[, posterior float32 [L, *shape]]).
    A label outside the range raises ValueError naming the rater and the value."""
    labels = list(labels)
    p = staple_check_args(len(labels), num_classes, prior, max_iterations, tolerance)
    first = labels[0]
    for r, t in enumerate(labels):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"labels[{r}] is not a tensor")
        _require_device(t)
        if t.dtype != first.dtype or t.shape != first.shape or t.device != first.device:
            raise ValueError(f"labels[{r}]: {t.dtype} {tuple(t.shape)} differs from labels[0]: {first.dtype} "
                             f"{tuple(first.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"labels[{r}] is not contiguous")
    lb = label_bytes(first)
    n = first.numel()
    if n == 0 or n >= CC_MAX_VOXELS:
        raise ValueError(f"labels hold 1 .. 2^31 - 1 voxels, got shape {tuple(first.shape)}")
    R, L = len(labels), int(num_classes)
    dev = first.device
    out = torch.empty_like(first)
    sums = torch.empty((R, L, L), dtype=torch.int64, device=dev)
    prior_out = torch.empty(L, dtype=torch.float64, device=dev)
    post = torch.empty((L,) + tuple(first.shape), dtype=torch.float32, device=dev) if return_posterior else None
    ws = torch.empty(int(lib.segmi_staple_workspace_bytes(R, L)), dtype=torch.uint8, device=dev)
    tab = (C.c_void_p * R)(*[t.data_ptr() for t in labels])
    info = (C.c_int32 * 4)()
    check(lib.segmi_staple(tab, R, lb, n, L, p.ctypes.data_as(C.c_void_p) if p is not None else None,
                           int(max_iterations), float(tolerance), _ptr(out), _ptr(sums), _ptr(prior_out), _ptr(post),
                           info, _ptr(ws), ws.numel(), _stream()), "staple")
    if info[2] >= 0:
        raise ValueError(f"staple: rater {info[2]} holds the label {info[3]}, outside 0 .. {L - 1}")
    res = (out, sums, prior_out, int(info[0]), bool(info[1]))
    return res + (post,) if return_posterior else res


# ------------------------------------------------------------------ patch-based label fusion (patch_fusion.hip)
PF_MAX_ATLASES = 16
PF_MAX_CLASSES = 64
PF_MAX_RADIUS = 3
PF_MAX_H2 = 65025             # 255^2: squared 8-bit quanta per patch voxel
PF_TABLE_ENTRIES = 1024
PF_MAX_WEIGHT = 65536


def pf_radius(radius, name: str) -> tuple:
    """a radius given as one integer or one per axis (z, y, x) -> (z, y, x), each in 0 .. 3"""
    r = (radius,) * 3 if isinstance(radius, (int, np.integer)) and not isinstance(radius, bool) else tuple(
        radius if hasattr(radius, "__len__") else (radius,))
    if len(r) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in r):
        raise ValueError(f"{name} must be one integer or three (z, y, x), got {radius!r}")
    if any(not 0 <= int(v) <= PF_MAX_RADIUS for v in r):
        raise ValueError(f"{name}: every component must lie in 0 .. {PF_MAX_RADIUS}, got {radius!r}")
    return tuple(int(v) for v in r)


def pf_check_args(atlases: int, num_classes, patch_radius, search_radius, h2, min_h2):
    """The argument checks of ``patch_fusion`` that need no tensor; returns (rp, rs, adaptive, h2 or min_h2)."""
    if not 1 <= int(atlases) <= PF_MAX_ATLASES:
        raise ValueError(f"1 .. {PF_MAX_ATLASES} atlases, got {atlases}")
    if isinstance(num_classes, bool) or int(num_classes) != num_classes or not 2 <= int(num_classes) <= PF_MAX_CLASSES:
        raise ValueError(f"num_classes must be an integer in 2 .. {PF_MAX_CLASSES}, got {num_classes}")
    rp, rs = pf_radius(patch_radius, "patch_radius"), pf_radius(search_radius, "search_radius")
    name, v = ("min_h2", min_h2) if h2 is None else ("h2", h2)
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= PF_MAX_H2:
        raise ValueError(f"{name} must be an integer in 1 .. {PF_MAX_H2}, got {v!r}")
    return rp, rs, h2 is None, int(v)


def quantise_range_check(lo, hi) -> tuple:
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"quantise_u8: lo < hi, both finite, got ({lo}, {hi})")
    if not math.isfinite(float(np.float32(255.0 / (hi - lo)))):
        raise ValueError(f"quantise_u8: the range ({lo}, {hi}) is too narrow for float32")
    return lo, hi


def quantise_u8(image: torch.Tensor, lo, hi) -> torch.Tensor:
    """uint8 tensor of the shape of ``image`` (float32, contiguous, on the device):
    clamp(floor((v - lo) * scale + 0.5), 0, 255) in float32, scale = float32(255 / (hi - lo)); NaN gives 0."""
    lo, hi = quantise_range_check(lo, hi)
    _require_device(image)
    if image.dtype != torch.float32 or not image.is_contiguous():
        raise ValueError(f"quantise_u8: a contiguous float32 tensor expected, got {image.dtype}")
    n = image.numel()
    if n == 0 or n >= CC_MAX_VOXELS:
        raise ValueError(f"quantise_u8: 1 .. 2^31 - 1 elements, got shape {tuple(image.shape)}")
    out = torch.empty(image.shape, dtype=torch.uint8, device=image.device)
    check(lib.segmi_quantise_u8(_ptr(image), n, lo, hi, _ptr(out), _stream()), "quantise_u8")
    return out


def patch_fusion_table(beta=1.0) -> np.ndarray:
    """The weight table of ``patch_fusion``: W[k] = floor(65536 * exp(-k / (64 * beta)) + 0.5), k = 0 .. 1023, in
    float64 numpy, as uint32.  k counts 64ths of the bandwidth, so W[64] is the weight at D = den for beta = 1."""
    if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)) or \
            not (math.isfinite(float(beta)) and float(beta) > 0.0):
        raise ValueError(f"beta must be finite and positive, got {beta!r}")
    k = np.arange(PF_TABLE_ENTRIES, dtype=np.float64)
    return np.floor(65536.0 * np.exp(-k / (64.0 * float(beta))) + 0.5).astype(np.uint32)


def pf_check_table(table) -> None:
    """a host table: 1024 integers in 0 .. 65536 with W[0] >= 1"""
    t = np.asarray(table)
    if t.shape != (PF_TABLE_ENTRIES,) or t.dtype.kind not in "iu":
        raise ValueError(f"table must hold {PF_TABLE_ENTRIES} integers, got {t.dtype} {t.shape}")
    if int(t.min()) < 0 or int(t.max()) > PF_MAX_WEIGHT or int(t[0]) < 1:
        raise ValueError(f"table: entries in 0 .. {PF_MAX_WEIGHT} with table[0] >= 1")


def patch_fusion_variant_name(num_classes: int, patch_radius=1, search_radius=2) -> str:
    """which form of the fusion kernel ``patch_fusion`` launches for these arguments (the launch's own choice)"""
    rp = (C.c_int32 * 3)(*pf_radius(patch_radius, "patch_radius"))
    rs = (C.c_int32 * 3)(*pf_radius(search_radius, "search_radius"))
    return lib.segmi_patch_fusion_variant_name(int(num_classes), rp, rs).decode()


def patch_fusion(target_q, atlas_q, atlas_labels, num_classes, *, patch_radius=1, search_radius=2, table, h2=None,
                 min_h2=4, return_scores=False, return_confidence=False):
    """Patch-based label fusion.  ``target_q``: uint8 [d, h, w] or [h, w] on the device;
    ``atlas_q``: 1 .. 16 uint8 tensors and ``atlas_labels`` as many label maps (one dtype among uint8 / int16 /
    int32, labels in 0 .. num_classes - 1), all contiguous and of the target's shape.  ``table``: 1024 weights
    (numpy integers, checked, or a uint32 / int32 device tensor, taken as it is).  ``h2``: fixed bandwidth
    den = npatch * h2; None: adaptive with the floor npatch * min_h2.  Returns labels in the dtype of the label maps,
    then (best, total) uint32-valued int32 tensors with ``return_confidence`` and scores [K, *shape] with
    ``return_scores``.  A label outside the range raises ValueError naming the atlas and the value."""
    atlas_q, atlas_labels = list(atlas_q), list(atlas_labels)
    if len(atlas_q) != len(atlas_labels):
        raise ValueError(f"{len(atlas_q)} atlas images for {len(atlas_labels)} label maps")
    rp, rs, adaptive, hv = pf_check_args(len(atlas_q), num_classes, patch_radius, search_radius, h2, min_h2)
    if not isinstance(table, torch.Tensor):
        pf_check_table(table)
    if not isinstance(target_q, torch.Tensor):
        raise TypeError("target_q is not a tensor")
    _require_device(target_q)
    if target_q.dtype != torch.uint8 or target_q.dim() not in (2, 3) or not target_q.is_contiguous():
        raise ValueError(f"target_q: a contiguous uint8 [d, h, w] or [h, w] tensor expected, got {target_q.dtype} "
                         f"{tuple(target_q.shape)}")
    n = target_q.numel()
    if n == 0 or n >= CC_MAX_VOXELS:
        raise ValueError(f"target_q holds 1 .. 2^31 - 1 voxels, got shape {tuple(target_q.shape)}")
    for a, (q, l) in enumerate(zip(atlas_q, atlas_labels)):
        for what, t in ((f"atlas_q[{a}]", q), (f"atlas_labels[{a}]", l)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{what} is not a tensor")
            _require_device(t)
            if t.shape != target_q.shape or t.device != target_q.device or not t.is_contiguous():
                raise ValueError(f"{what}: contiguous, of shape {tuple(target_q.shape)} on {target_q.device} expected, "
                                 f"got {tuple(t.shape)} on {t.device}")
        if q.dtype != torch.uint8:
            raise ValueError(f"atlas_q[{a}] is {q.dtype}, not uint8")
        if l.dtype != atlas_labels[0].dtype:
            raise ValueError(f"atlas_labels[{a}] is {l.dtype}, atlas_labels[0] is {atlas_labels[0].dtype}")
    lb = label_bytes(atlas_labels[0])
    dev = target_q.device
    if isinstance(table, torch.Tensor):
        _require_device(table)
        if table.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or table.numel() != PF_TABLE_ENTRIES or not table.is_contiguous():
            raise ValueError(f"table: {PF_TABLE_ENTRIES} contiguous int32 / uint32 entries expected")
        tab = table
    else:
        tab = torch.from_numpy(np.ascontiguousarray(np.asarray(table).astype(np.int32))).to(dev)
    A, K = len(atlas_q), int(num_classes)
    d, h, w = ((1,) + tuple(target_q.shape))[-3:]
    out = torch.empty_like(atlas_labels[0])
    conf = return_confidence
    best = torch.empty(target_q.shape, dtype=torch.int32, device=dev) if conf else None
    total = torch.empty(target_q.shape, dtype=torch.int32, device=dev) if conf else None
    scores = torch.empty((K,) + tuple(target_q.shape), dtype=torch.int32, device=dev) if return_scores else None
    ws = torch.empty(int(lib.segmi_patch_fusion_workspace_bytes(A, K)), dtype=torch.uint8, device=dev)
    qt = (C.c_void_p * A)(*[t.data_ptr() for t in atlas_q])
    lt = (C.c_void_p * A)(*[t.data_ptr() for t in atlas_labels])
    info = (C.c_int32 * 2)()
    check(lib.segmi_patch_fusion(_ptr(target_q), qt, lt, A, lb, d, h, w, K, (C.c_int32 * 3)(*rp), (C.c_int32 * 3)(*rs),
                                 int(adaptive), hv, _ptr(tab), _ptr(out), _ptr(best), _ptr(total), _ptr(scores), info,
                                 _ptr(ws), ws.numel(), _stream()), "patch_fusion")
    if info[0] >= 0:
        raise ValueError(f"patch_fusion: atlas {info[0]} holds the label {info[1]}, outside 0 .. {K - 1}")
    res = (out,)
    if conf:
        res += (best, total)
    if return_scores:
        res += (scores,)
    return res if len(res) > 1 else out


# ------------------------------------------------------------------ evaluation (distance.hip)
def label_bytes(t: torch.Tensor) -> int:
    """label_bytes of a label volume read in place: uint8 -> 1, int16 -> 2, int32 -> 4."""
    try:
        return _LABEL_BYTES[t.dtype]
    except KeyError:
        raise ValueError(f"label volumes are uint8, int16 or int32 (label_bytes 1, 2, 4), not {t.dtype}")


def _label_dims(t: torch.Tensor, ranks=(2, 3), limit: Optional[str] = None):
    """(d, h, w) of a contiguous label volume on the device whose rank is one of ``ranks`` ([h, w]: d = 1).
    ``limit`` "voxels" / "cells" also asks for a label dtype and 1 .. 2^31 - 1 voxels / cells (d+1)(h+1)(w+1)."""
    _require_device(t)
    if t.dim() not in ranks or not t.is_contiguous():
        raise ValueError(f"label volumes are contiguous {' or '.join(f'{r}-D' for r in ranks)} tensors, "
                         f"got shape {tuple(t.shape)}")
    d, h, w = (1,) * (3 - t.dim()) + tuple(int(v) for v in t.shape)
    if limit is not None:
        label_bytes(t)
        count = (d + 1) * (h + 1) * (w + 1) if limit == "cells" else d * h * w
        if t.numel() == 0 or count >= CC_MAX_VOXELS:
            raise ValueError(f"label volumes hold 1 .. 2^31 - 1 {limit}, got shape {tuple(t.shape)}")
    return d, h, w


def _like_labels(labels: torch.Tensor, t, what: str = "out", distinct: bool = False) -> torch.Tensor:
    """``t`` (None: a fresh tensor) checked to match ``labels`` in dtype and shape; ``distinct``: not labels itself"""
    if t is None:
        t = torch.empty_like(labels)
    if t.dtype != labels.dtype or t.shape != labels.shape or not t.is_contiguous() or \
            (distinct and t.data_ptr() == labels.data_ptr()):
        raise ValueError(f"{what} must match labels in dtype and shape" + (" and be another tensor" if distinct else ""))
    return t


def _i32_of(t: torch.Tensor, shape, what: str) -> None:
    _require_device(t)
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int32 tensor of shape {tuple(shape)}")


def _host(v, dtype, shape=None):
    """contiguous host array of ``dtype`` (reshaped to ``shape`` when given) and its ctypes pointer, None when empty"""
    a = np.ascontiguousarray(np.asarray(v, dtype=dtype))
    if shape is not None:
        a = np.ascontiguousarray(a.reshape(shape))
    return a, (a.ctypes.data_as(C.c_void_p) if a.size else None)


def _align256(nbytes: int) -> int:
    return (int(nbytes) + 255) // 256 * 256


def _workspace(workspace, need: int, device) -> torch.Tensor:
    """``workspace`` checked, or a fresh one of ``need`` bytes"""
    if workspace is None:
        return torch.empty(int(need), dtype=torch.uint8, device=device)
    _require_device(workspace)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("the workspace is a contiguous uint8 tensor")
    return workspace


def label_boxes(pred, truth, k, boxes, counts) -> None:
    """boxes i32 [k, 6] (half-open z0 z1 y0 y1 x0 x1 of pred==c | truth==c), counts i64 [k, 2]."""
    if pred.shape != truth.shape or pred.dtype != truth.dtype:
        raise ValueError("label_boxes: pred and truth differ in shape or dtype")
    d, h, w = _label_dims(pred)
    check(lib.segmi_label_boxes(_ptr(pred), _ptr(truth), label_bytes(pred), d, h, w, int(k), _ptr(boxes),
                                _ptr(counts), _stream()), "label_boxes")


def edt_workspace_bytes(box) -> int:
    z0, z1, y0, y1, x0, x1 = (int(v) for v in box)
    return int(lib.segmi_edt_workspace_bytes(z1 - z0, y1 - y0, x1 - x0))


def edt_sq(labels, label, feature, box, spacing_zyx, dist_sq, workspace) -> None:
    """Squared distance to label's foreground (feature 0) or signed, to its contour (feature 1), over box;
    dist_sq f32 [bd, bw, bh]."""
    d, h, w = _label_dims(labels)
    b, bp = _host(box, np.int32)
    sp, spp = _host(spacing_zyx, np.float32, 3)
    check(lib.segmi_edt_sq(_ptr(labels), label_bytes(labels), d, h, w, labels.dim(), int(label), int(feature), bp,
                           spp, _ptr(dist_sq), _ptr(workspace), workspace.numel(),
                           _stream()), "edt_sq")


def edt_sample(dist_sq, labels, label, query, box, stats, workspace, values=None, n_values=None) -> None:
    """stats f64[4] = count, sum, sum of squares, max of the distances at labels' query voxels;
    squared distances appended to values[n_values ...] when given."""
    d, h, w = _label_dims(labels)
    b, bp = _host(box, np.int32)
    check(lib.segmi_edt_sample(_ptr(dist_sq), _ptr(labels), label_bytes(labels), d, h, w, labels.dim(), int(label),
                               int(query), bp, _ptr(stats), _ptr(values), _ptr(n_values), _ptr(workspace),
                               workspace.numel(), _stream()), "edt_sample")


def select_workspace_bytes(n_ranks: int) -> int:
    return int(lib.segmi_select_workspace_bytes(int(n_ranks)))


def select_f32(values, n, ranks, out, workspace) -> None:
    """out[i] = value of rank ranks[i] among the first n[0] (device) non-negative f32 values."""
    check(lib.segmi_select_f32(_ptr(values), _ptr(n), _ptr(ranks), ranks.numel(), _ptr(out), _ptr(workspace),
                               workspace.numel(), _stream()), "select_f32")


def confusion_counts(pred, truth, k, cm) -> None:
    """cm i64 [k, k], cm[truth, pred]."""
    if pred.shape != truth.shape or pred.dtype != truth.dtype:
        raise ValueError("confusion_counts: pred and truth differ in shape or dtype")
    _require_device(pred)
    check(lib.segmi_confusion_counts(_ptr(pred), _ptr(truth), label_bytes(pred), pred.numel(), int(k), _ptr(cm),
                                     _stream()), "confusion_counts")


# ------------------------------------------------------------------ label clean-up (components.hip)
CC_MAX_VOXELS = 2 ** 31       # label volumes hold fewer voxels than this (linear indices are int32)
CC_MAX_KEEP = 8               # largest num_components of cc_keep_largest
CC_CLASS_TABLE = 65536        # label values of the clean-up transforms lie in 0 .. CC_CLASS_TABLE - 1
_MAP_BYTES = {torch.uint8: 1, torch.int16: 2, torch.int32: 4, torch.int64: 8}


def _cc_connectivity(connectivity, ndim: int) -> int:
    c = ndim if connectivity is None else int(connectivity)
    if not 1 <= c <= ndim:
        raise ValueError(f"connectivity must be 1 .. {ndim} for a {ndim}-D volume, got {connectivity}")
    return c


def _applied(applied):
    """host int32 array of the applied labels (empty = all) and its ctypes pointer"""
    return _host([] if applied is None else list(applied), np.int32, -1)


CC_FILL_WORDS = 2             # the int32 words per voxel (lo, hi) that end cc_layout in components.hip, each
                              # region rounded up to 256 bytes; only cc_fill_holes uses them


def _cc_workspace(t: torch.Tensor, workspace, fill_holes: bool = False) -> torch.Tensor:
    need = cc_workspace_bytes(t.shape) - (0 if fill_holes else CC_FILL_WORDS * _align256(4 * t.numel()))
    return _workspace(workspace, need, t.device)


def cc_workspace_bytes(shape) -> int:
    """bytes of the workspace shared by the cc_* calls for a [d, h, w] or [h, w] volume"""
    dims = tuple(int(v) for v in shape)
    if len(dims) not in (2, 3) or any(v <= 0 for v in dims) or int(np.prod(dims, dtype=np.int64)) >= CC_MAX_VOXELS:
        raise ValueError(f"label volumes are 2-D or 3-D with 1 .. 2^31 - 1 voxels, got shape {dims}")
    d, h, w = (1,) + dims if len(dims) == 2 else dims
    return int(lib.segmi_cc_workspace_bytes(d, h, w))


def cc_label(labels, connectivity=None, with_background=False, root=None, workspace=None) -> torch.Tensor:
    """root int32 (shape of labels): linear index of the first voxel of each voxel's component, -1 for voxels
    outside every component (the zeros, unless ``with_background``)."""
    d, h, w = _label_dims(labels, limit="voxels")
    ndim = labels.dim()
    c = _cc_connectivity(connectivity, ndim)
    if root is None:
        root = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    _i32_of(root, labels.shape, "root")
    ws = _cc_workspace(labels, workspace)
    check(lib.segmi_cc_label(_ptr(labels), label_bytes(labels), d, h, w, ndim, c, int(bool(with_background)),
                             _ptr(root), _ptr(ws), ws.numel(), _stream()), "cc_label")
    return root


def cc_sizes(root, size=None) -> torch.Tensor:
    """size int32 (shape of root): the voxel count of each component at its root, 0 elsewhere."""
    _i32_of(root, root.shape, "root")
    if root.numel() == 0 or root.numel() >= CC_MAX_VOXELS:
        raise ValueError("root holds 1 .. 2^31 - 1 voxels")
    if size is None:
        size = torch.empty_like(root)
    _i32_of(size, root.shape, "size")
    check(lib.segmi_cc_sizes(_ptr(root), root.numel(), _ptr(size), _stream()), "cc_sizes")
    return size


def cc_compact(root, comp=None, n_comp=None, workspace=None):
    """(comp int32: canonical component number 1 .. n of every voxel, 0 outside; n_comp int32 [1] on the device)."""
    _i32_of(root, root.shape, "root")
    if root.dim() not in (2, 3):
        raise ValueError("root has the shape of its 2-D or 3-D label volume")
    if comp is None:
        comp = torch.empty_like(root)
    _i32_of(comp, root.shape, "comp")
    if n_comp is None:
        n_comp = torch.empty(1, dtype=torch.int32, device=root.device)
    if n_comp.dtype != torch.int32 or n_comp.numel() != 1:
        raise ValueError("n_comp is one int32")
    ws = _cc_workspace(root, workspace)
    check(lib.segmi_cc_compact(_ptr(root), root.numel(), _ptr(comp), _ptr(n_comp), _ptr(ws), ws.numel(), _stream()),
          "cc_compact")
    return comp, n_comp


def cc_keep_largest(labels, root, size, applied=None, independent=True, num_components=1, out=None,
                    workspace=None) -> torch.Tensor:
    """Keep the ``num_components`` largest components per applied class (ties: the earlier first voxel); with
    ``independent=False`` root / size describe the union mask of the applied classes."""
    _label_dims(labels, limit="voxels")
    _i32_of(root, labels.shape, "root")
    _i32_of(size, labels.shape, "size")
    if not 1 <= int(num_components) <= CC_MAX_KEEP:
        raise ValueError(f"num_components must be 1 .. {CC_MAX_KEEP}, got {num_components}")
    out = _like_labels(labels, out)
    a, ap = _applied(applied)
    ws = _cc_workspace(labels, workspace)
    check(lib.segmi_cc_keep_largest(_ptr(labels), label_bytes(labels), labels.numel(), _ptr(root), _ptr(size), ap,
                                    a.size, int(bool(independent)), int(num_components), _ptr(out), _ptr(ws),
                                    ws.numel(), _stream()), "cc_keep_largest")
    return out


def cc_remove_small(labels, root, size, min_size, out=None) -> torch.Tensor:
    """Voxels of components smaller than ``min_size`` become 0."""
    _label_dims(labels, limit="voxels")
    _i32_of(root, labels.shape, "root")
    _i32_of(size, labels.shape, "size")
    if int(min_size) < 0:
        raise ValueError(f"min_size must be >= 0, got {min_size}")
    out = _like_labels(labels, out)
    check(lib.segmi_cc_remove_small(_ptr(labels), label_bytes(labels), labels.numel(), _ptr(root), _ptr(size),
                                    int(min(int(min_size), 2 ** 31 - 1)), _ptr(out), _stream()), "cc_remove_small")
    return out


def cc_fill_holes(labels, root, applied=None, connectivity=None, out=None, workspace=None) -> torch.Tensor:
    """Fill the enclosed 0-regions bordered by one single label; ``root`` = cc_label(labels, connectivity,
    with_background=True)."""
    d, h, w = _label_dims(labels, limit="voxels")
    ndim = labels.dim()
    c = _cc_connectivity(connectivity, ndim)
    _i32_of(root, labels.shape, "root")
    out = _like_labels(labels, out)
    a, ap = _applied(applied)
    ws = _cc_workspace(labels, workspace, fill_holes=True)
    check(lib.segmi_cc_fill_holes(_ptr(labels), label_bytes(labels), d, h, w, ndim, c, _ptr(root), ap, a.size,
                                  _ptr(out), _ptr(ws), ws.numel(), _stream()), "cc_fill_holes")
    return out


def map_labels(x, lut, out=None, out_dtype=torch.int64) -> torch.Tensor:
    """out = lut[x] for an integer tensor x (uint8 / int16 / int32 / int64) and a device int64 table.  The
    caller has checked 0 <= x < len(lut)."""
    if x.dtype not in _MAP_BYTES:
        raise TypeError(f"map_labels reads uint8, int16, int32 or int64, not {x.dtype}")
    _require_device(x)
    _require_device(lut)
    if lut.dtype != torch.int64 or lut.dim() != 1 or lut.numel() == 0 or not lut.is_contiguous():
        raise ValueError("map_labels: the table is a non-empty contiguous 1-D int64 tensor")
    if not x.is_contiguous() or x.numel() == 0:
        raise ValueError("map_labels: the input must be contiguous and non-empty")
    if out is None:
        if out_dtype not in _MAP_BYTES:
            raise TypeError(f"map_labels writes uint8, int16, int32 or int64, not {out_dtype}")
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    if out.dtype not in _MAP_BYTES or out.shape != x.shape or not out.is_contiguous():
        raise ValueError("map_labels: out must be a contiguous integer tensor of the input's shape")
    _require_device(out)
    check(lib.segmi_map_labels(_ptr(x), _MAP_BYTES[x.dtype], x.numel(), _ptr(lut), lut.numel(), _ptr(out),
                               _MAP_BYTES[out.dtype], _stream()), "map_labels")
    return out


# ------------------------------------------------------------------ label morphology (morphology.hip)
FT_NONZERO, FT_ZERO, FT_EQUAL, FT_NOT_EQUAL, FT_TABLE = 0, 1, 2, 3, 4
FT_TABLE_SIZE = 65536         # entries of the feature table of mode FT_TABLE (device uint8)


def _box_shape(labels: torch.Tensor, box):
    if box is None:
        return tuple(labels.shape)
    z0, z1, y0, y1, x0, x1 = (int(v) for v in box)
    return (z1 - z0, y1 - y0, x1 - x0) if labels.dim() == 3 else (y1 - y0, x1 - x0)


def feature_transform_workspace_bytes(shape) -> int:
    dims = tuple(int(v) for v in shape)
    d, h, w = (1,) + dims if len(dims) == 2 else dims
    return int(lib.segmi_feature_transform_workspace_bytes(d, h, w))


def feature_transform(labels, mode, spacing_zyx, label=0, table=None, box=None, index=None, dist=None,
                      dist_sqrt=False, with_dist=False, workspace=None):
    """-> (index int32, dist float32 or None) over ``box`` (host z0 z1 y0 y1 x0 x1; None: the whole volume):
    the linear index in the full volume of the nearest feature voxel (-1: none), ties to the smallest index,
    and its squared distance (``dist_sqrt``: its distance)."""
    d, h, w = _label_dims(labels, limit="voxels")
    ndim = labels.dim()
    shape = _box_shape(labels, box)
    if index is None:
        index = torch.empty(shape, dtype=torch.int32, device=labels.device)
    _i32_of(index, shape, "index")
    if dist is None and with_dist:
        dist = torch.empty(shape, dtype=torch.float32, device=labels.device)
    if dist is not None and (dist.dtype != torch.float32 or tuple(dist.shape) != tuple(shape)
                             or not dist.is_contiguous()):
        raise ValueError("dist must be a contiguous float32 tensor of the box's shape")
    if int(mode) == FT_TABLE:
        if table is None or table.dtype != torch.uint8 or table.numel() != FT_TABLE_SIZE or not table.is_contiguous():
            raise ValueError(f"mode FT_TABLE needs a contiguous uint8 table of {FT_TABLE_SIZE} entries")
    workspace = _workspace(workspace, feature_transform_workspace_bytes(shape), labels.device)
    bp = None if box is None else _host(box, np.int32)
    sp, spp = _host(spacing_zyx, np.float64, 3)
    check(lib.segmi_feature_transform(_ptr(labels), label_bytes(labels), d, h, w, ndim, int(mode), int(label),
                                      _ptr(table), None if bp is None else bp[1], spp, _ptr(index), _ptr(dist),
                                      int(bool(dist_sqrt)), _ptr(workspace), workspace.numel(), _stream()),
          "feature_transform")
    return index, dist


def morph_gather(labels, index, spacing_zyx, radius, out=None) -> torch.Tensor:
    """Zero voxels whose nearest feature ``index`` lies within ``radius`` take that voxel's label."""
    d, h, w = _label_dims(labels, limit="voxels")
    ndim = labels.dim()
    _i32_of(index, labels.shape, "index")
    out = _like_labels(labels, out, distinct=True)
    sp, spp = _host(spacing_zyx, np.float64, 3)
    check(lib.segmi_morph_gather(_ptr(labels), label_bytes(labels), d, h, w, ndim, _ptr(index), spp, float(radius),
                                 _ptr(out), _stream()), "morph_gather")
    return out


def morph_erode_select(labels, label, box, index, spacing_zyx, radius, out, keep=None) -> torch.Tensor:
    """out[v] = 0 for the voxels of ``label`` in ``box`` whose nearest feature (``index``, box-shaped) lies
    within ``radius``; ``out`` starts as a copy of ``labels``.  Voxels with ``keep != 0`` are left alone."""
    d, h, w = _label_dims(labels, limit="voxels")
    ndim = labels.dim()
    shape = _box_shape(labels, box)
    _i32_of(index, shape, "index")
    _like_labels(labels, out)
    if keep is not None:
        _like_labels(labels, keep, "keep")
    bp = None if box is None else _host(box, np.int32)
    sp, spp = _host(spacing_zyx, np.float64, 3)
    check(lib.segmi_morph_erode_select(_ptr(labels), label_bytes(labels), d, h, w, ndim, int(label),
                                       None if bp is None else bp[1], _ptr(index), spp, float(radius), _ptr(keep),
                                       _ptr(out), _stream()), "morph_erode_select")
    return out


def morph_index_planes(index: torch.Tensor) -> torch.Tensor:
    """-> int32 [ndim, ...]: the coordinates of the voxels ``index`` names, scipy's ``return_indices`` layout."""
    _i32_of(index, index.shape, "index")
    d, h, w = _label_dims(index, limit="voxels")
    planes = torch.empty((index.dim(),) + tuple(index.shape), dtype=torch.int32, device=index.device)
    check(lib.segmi_morph_index_planes(_ptr(index), d, h, w, index.dim(), _ptr(planes), _stream()),
          "morph_index_planes")
    return planes


# ------------------------------------------------------------------ label surfaces (surfaces.hip)
SURFACE_MAX_CELLS = 2 ** 31     # (d+1)(h+1)(w+1) stays below this
SURFACE_MAX_LABEL = 65535


def _surface_selected(selected):
    s = np.ascontiguousarray(np.asarray(list(selected), dtype=np.int64).reshape(-1))
    if s.size == 0 or s.size > SURFACE_MAX_LABEL or s.min() < 1 or s.max() > SURFACE_MAX_LABEL or \
            (np.diff(s) <= 0).any():
        raise ValueError(f"selected labels are 1 .. {SURFACE_MAX_LABEL} strictly ascending values in "
                         f"1 .. {SURFACE_MAX_LABEL}")
    return _host(s, np.int32)


def surface_boxes(labels: torch.Tensor, selected) -> torch.Tensor:
    """boxes int32 [n, 6] on the device: half-open z0 z1 y0 y1 x0 x1 of ``labels == selected[l]``."""
    d, h, w = _label_dims(labels, (3,), "cells")
    s, _ = _surface_selected(selected)
    sel = torch.from_numpy(s).to(labels.device)
    boxes = torch.empty((s.size, 6), dtype=torch.int32, device=labels.device)
    check(lib.segmi_surface_boxes(_ptr(labels), label_bytes(labels), d, h, w, _ptr(sel), s.size, _ptr(boxes),
                                  _stream()), "surface_boxes")
    return boxes


def surface_workspace_bytes(shape, selected, boxes_host) -> int:
    d, h, w = (int(v) for v in shape)
    s, sp = _surface_selected(selected)
    b, bp = _host(boxes_host, np.int32)
    if b.shape != (s.size, 6):
        raise ValueError("boxes_host is [n_selected, 6]")
    n = int(lib.segmi_surface_workspace_bytes(d, h, w, sp, bp, s.size))
    if n <= 0:
        raise ValueError("label surfaces: invalid boxes, or the label boxes hold 2^31 chunks of 64 cells or more")
    return n


def surface_count(labels: torch.Tensor, selected, boxes_host, workspace: torch.Tensor) -> torch.Tensor:
    """starts int32 [n + 2, 2] on the device: (first vertex, first face) per label, the totals, (overflow, 0)."""
    d, h, w = _label_dims(labels, (3,), "cells")
    s, sp = _surface_selected(selected)
    b, bp = _host(boxes_host, np.int32)
    starts = torch.empty((s.size + 2, 2), dtype=torch.int32, device=labels.device)
    check(lib.segmi_surface_count(_ptr(labels), label_bytes(labels), d, h, w, sp, bp, s.size, _ptr(starts),
                                  _ptr(workspace), workspace.numel(), _stream()), "surface_count")
    return starts


def surface_emit(labels: torch.Tensor, selected, boxes_host, workspace: torch.Tensor, n_vertices: int, n_faces: int,
                 with_neighbours: bool = False):
    """-> (offsets f32 [V, 3], cells i32 [V, 3], neighbours i32 [V, 6] or None, faces i32 [F, 3])."""
    d, h, w = _label_dims(labels, (3,), "cells")
    s, sp = _surface_selected(selected)
    b, bp = _host(boxes_host, np.int32)
    dev = labels.device
    offs = torch.empty((n_vertices, 3), dtype=torch.float32, device=dev)
    cells = torch.empty((n_vertices, 3), dtype=torch.int32, device=dev)
    nbr = torch.empty((n_vertices, 6), dtype=torch.int32, device=dev) if with_neighbours else None
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    check(lib.segmi_surface_emit(_ptr(labels), label_bytes(labels), d, h, w, sp, bp, s.size, int(n_vertices),
                                 int(n_faces), _ptr(offs), _ptr(cells), _ptr(nbr), _ptr(faces), _ptr(workspace),
                                 workspace.numel(), _stream()), "surface_emit")
    return offs, cells, nbr, faces


def surface_relax(offsets, cells, neighbours, iterations: int, relaxation: float, origin, direction,
                  spacing) -> torch.Tensor:
    """``iterations`` relaxation sweeps (offsets is clobbered), then the physical vertices f32 [V, 3] (x, y, z)."""
    _require_device(offsets)
    nv = offsets.shape[0]
    g = np.ascontiguousarray(np.concatenate([np.asarray(origin, np.float64).reshape(3),
                                             np.asarray(direction, np.float64).reshape(9),
                                             np.asarray(spacing, np.float64).reshape(3)]))
    verts = torch.empty((nv, 3), dtype=torch.float32, device=offsets.device)
    scratch = torch.empty_like(offsets) if iterations > 0 else None
    check(lib.segmi_surface_relax(_ptr(offsets), _ptr(scratch), _ptr(cells), _ptr(neighbours), nv, int(iterations),
                                  float(relaxation), g.ctypes.data_as(C.c_void_p), _ptr(verts), _stream()),
          "surface_relax")
    return verts


def surface_measure(vertices, faces, starts) -> torch.Tensor:
    """measures f64 [n, 2] on the device: (area, signed volume) of every label's mesh."""
    _require_device(starts)
    n = starts.shape[0] - 2
    out = torch.empty((n, 2), dtype=torch.float64, device=starts.device)
    ws = _workspace(None, _align256(n * 32 * 2 * 8), starts.device)
    check(lib.segmi_surface_measure(_ptr(vertices), _ptr(faces), _ptr(starts), n, _ptr(out), _ptr(ws), ws.numel(),
                                    _stream()), "surface_measure")
    return out


# ------------------------------------------------------------------ mesh decimation (decimate.hip)
DECIMATE_MAX_MESH_VERTICES = 2 ** 23    # the claim key keeps 23 bits for the vertex number within its mesh


def decimate_targets(starts_host, reduction: float) -> np.ndarray:
    """``ceil((1 - reduction) F)`` per mesh, in float64"""
    s = np.asarray(starts_host, np.int64)
    return np.asarray([math.ceil((1.0 - float(reduction)) * int(f)) for f in s[1:-1, 1] - s[:-2, 1]], np.int32)


def decimate_meshes(vertices: torch.Tensor, faces: torch.Tensor, starts: torch.Tensor, starts_host, reduction: float,
                    max_rounds: int = 128, stats: Optional[dict] = None):
    """Decimate a batch of meshes (``starts`` i32 [n + 2, 2] as ``surface_count`` returns it, ``starts_host`` its host
    copy; faces are numbered within their mesh and must be in range).  -> (vertices f32 [V', 3], faces i32 [F', 3],
    kept i32 [V'], starts i32 [n + 2, 2] on the device, its host copy).  One device-to-host copy per round (the
    live-face counts) and one for the output totals; ``stats`` receives ``rounds`` and ``d2h_copies``."""
    _require_device(vertices)
    _require_device(faces)
    _require_device(starts)
    sh = np.asarray(starts_host, np.int64)
    n = sh.shape[0] - 2
    nv, nf = int(sh[n, 0]), int(sh[n, 1])
    if vertices.dtype != torch.float32 or faces.dtype != torch.int32 or starts.dtype != torch.int32 or \
            tuple(vertices.shape) != (nv, 3) or tuple(faces.shape) != (nf, 3) or tuple(starts.shape) != (n + 2, 2) or \
            not (vertices.is_contiguous() and faces.is_contiguous() and starts.is_contiguous()):
        raise ValueError("decimate_meshes: contiguous vertices f32 [V, 3], faces i32 [F, 3] and starts i32 [n + 2, 2] "
                         "whose totals match")
    if int(max_rounds) < 1:
        raise ValueError(f"max_rounds must be >= 1, got {max_rounds!r}")
    if n < 1 or nv < 1 or nf < 1:
        raise ValueError("decimate_meshes: at least one mesh, one vertex and one face")
    if int((sh[1:n + 1, 0] - sh[:n, 0]).max()) >= DECIMATE_MAX_MESH_VERTICES:
        raise ValueError(f"decimation takes meshes of fewer than 2^23 vertices, got "
                         f"{int((sh[1:n + 1, 0] - sh[:n, 0]).max())}")
    dev = vertices.device
    size = int(lib.segmi_decimate_workspace_bytes(nv, nf, n))
    if size <= 0:
        raise ValueError("decimate_meshes: 1 .. 65535 meshes, V < 2^31 and 3 F < 2^31")
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    targets_host = decimate_targets(sh, reduction)
    targets = torch.from_numpy(targets_host).to(dev)
    live = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.segmi_decimate_init(_ptr(faces), _ptr(starts), n, nv, nf, _ptr(live), _ptr(ws), ws.numel(), _stream()),
          "decimate_init")
    count = (sh[1:n + 1, 1] - sh[:n, 1]).astype(np.int64)
    rounds = copies = 0
    active = count > targets_host
    while active.any() and rounds < int(max_rounds):
        check(lib.segmi_decimate_round(_ptr(vertices), _ptr(starts), _ptr(targets), n, nv, nf, rounds, _ptr(live),
                                       _ptr(ws), ws.numel(), _stream()), "decimate_round")
        rounds += 1
        now = live.cpu().numpy().astype(np.int64)            # host synchronisation: live faces per mesh
        copies += 1
        active = (now > targets_host) & (now < count)
        count = now
    out_starts = torch.empty((n + 2, 2), dtype=torch.int32, device=dev)
    check(lib.segmi_decimate_compact_count(_ptr(starts), n, nv, nf, _ptr(out_starts), _ptr(ws), ws.numel(), _stream()),
          "decimate_compact_count")
    out_host = out_starts.cpu().numpy()                      # host synchronisation: output totals
    copies += 1
    ov, of = int(out_host[n, 0]), int(out_host[n, 1])
    out_v = torch.empty((ov, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((of, 3), dtype=torch.int32, device=dev)
    kept = torch.empty(ov, dtype=torch.int32, device=dev)
    check(lib.segmi_decimate_compact_emit(_ptr(vertices), _ptr(starts), n, nv, nf, _ptr(out_v), _ptr(out_f), _ptr(kept),
                                          _ptr(ws), ws.numel(), _stream()), "decimate_compact_emit")
    if stats is not None:
        stats.update(rounds=rounds, d2h_copies=copies)
    return out_v, out_f, kept, out_starts, out_host


# ------------------------------------------------------------------ Nyul standardisation
NYUL_MAX_LANDMARKS = 64


def nyul_workspace_bytes(segments: int, n_quantiles: int) -> int:
    return int(lib.segmi_nyul_workspace_bytes(int(segments), int(n_quantiles)))


def nyul_landmarks(x: torch.Tensor, segments: int, nonzero: bool, quantiles, landmarks=None, counts=None,
                   workspace=None):
    """Quantile landmarks of each of ``segments`` equal slices of a contiguous f32 device tensor ``x``
    (mask ``x != 0`` when ``nonzero``); ``quantiles`` is a host sequence, sorted, in [0, 1].
    Returns (landmarks f32 [segments, L], counts i64 [segments]), both on the device."""
    _require_device(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("nyul_landmarks expects contiguous float32")
    if x.numel() == 0 or x.numel() % segments:
        raise ValueError("nyul_landmarks: the tensor does not split into that many non-empty segments")
    q = np.ascontiguousarray(np.asarray(quantiles, dtype=np.float64))
    nq = q.size
    if landmarks is None:
        landmarks = torch.empty(segments, nq, dtype=torch.float32, device=x.device)
    if counts is None:
        counts = torch.empty(segments, dtype=torch.int64, device=x.device)
    if workspace is None:
        workspace = torch.empty(nyul_workspace_bytes(segments, nq), dtype=torch.uint8, device=x.device)
    check(lib.segmi_nyul_landmarks(_ptr(x), int(segments), x.numel() // segments, int(bool(nonzero)),
                                   q.ctypes.data_as(C.c_void_p), nq, _ptr(landmarks), _ptr(counts),
                                   _ptr(workspace), workspace.numel(), _stream()), "nyul_landmarks")
    return landmarks, counts


def nyul_apply_(x: torch.Tensor, segments: int, nonzero: bool, landmarks, counts, standard_scale) -> torch.Tensor:
    """in place: the piecewise-linear map of each segment's landmarks onto ``standard_scale`` (host
    sequence) for its masked values; segments whose ``counts`` entry is 0 are untouched (None: none is)."""
    _require_device(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("nyul_apply_ expects contiguous float32")
    if x.numel() == 0 or x.numel() % segments:
        raise ValueError("nyul_apply_: the tensor does not split into that many non-empty segments")
    s = np.ascontiguousarray(np.asarray(standard_scale, dtype=np.float32))
    if landmarks.dtype != torch.float32 or not landmarks.is_contiguous() or landmarks.numel() != segments * s.size:
        raise ValueError("nyul_apply_: landmarks must be contiguous float32 [segments, len(standard_scale)]")
    check(lib.segmi_nyul_apply(_ptr(x), int(segments), x.numel() // segments, int(bool(nonzero)), _ptr(landmarks),
                               _ptr(counts), s.ctypes.data_as(C.c_void_p), s.size, _stream()), "nyul_apply")
    return x


# ------------------------------------------------------------------ vertebra landmarks
LANDMARK_MAX_LABELS = 255
HEATMAP_TAIL_OFFSET = 4        # words of the heatmap parameter buffer: k, stride, gamma, 0, tails[256], tables
HEATMAP_TABLE_OFFSET = 4 + 256


def _dense3(t: torch.Tensor, what: str):
    """(d, h, w) of a contiguous [d, h, w] or [c, d, h, w] device tensor"""
    _require_device(t)
    if t.dim() not in (3, 4) or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous [d, h, w] or [c, d, h, w] tensor")
    return tuple(int(v) for v in t.shape[-3:])


def label_centroids(labels, k, sums=None, flag=None):
    """sums i64 [k + 1, 4] = (count, sum x, sum y, sum z) of labels 0 .. k of a [d, h, w] label volume read in
    place; flag i32 [1] set when a label lies outside [0, k].  Both on the device, no host synchronisation."""
    if labels.dim() != 3:
        raise ValueError("label_centroids: labels are a contiguous [d, h, w] volume")
    d, h, w = _label_dims(labels)
    if sums is None:
        sums = torch.empty(int(k) + 1, 4, dtype=torch.int64, device=labels.device)
    if flag is None:
        flag = torch.empty(1, dtype=torch.int32, device=labels.device)
    check(lib.segmi_label_centroids(_ptr(labels), label_bytes(labels), d, h, w, int(k), _ptr(sums), _ptr(flag),
                                    _stream()), "label_centroids")
    return sums, flag


def vert_heatmap(params, k, sums, flag, shape_zyx, smooth_3d=False, out=None):
    """out f32 [k + 1, *shape_zyx], the closed-form heatmap of the centroid sums of label_centroids;
    params: the device parameter buffer (i32 words, see segmi.h)."""
    d, h, w = (int(v) for v in shape_zyx)
    if out is None:
        out = torch.empty(int(k) + 1, d, h, w, dtype=torch.float32, device=sums.device)
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (int(k) + 1, d, h, w):
        raise ValueError("vert_heatmap: out must be contiguous float32 [k + 1, d, h, w]")
    check(lib.segmi_vert_heatmap(_ptr(params), int(k), _ptr(sums), _ptr(flag), d, h, w, int(bool(smooth_3d)),
                                 _ptr(out), _stream()), "vert_heatmap")
    return out


def channel_argmax(x: torch.Tensor, keys=None, nan=None):
    """Per channel of a contiguous f32 [c, d, h, w] device tensor: keys u64 (as i64) [c] of the max and its
    first (x, y, z) in lexicographic order, nan i32 [c]; decode with decode_argmax_keys."""
    d, h, w = _dense3(x, "channel_argmax")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("channel_argmax: expected float32 [c, d, h, w]")
    c = int(x.shape[0])
    if keys is None:
        keys = torch.empty(c, dtype=torch.int64, device=x.device)
    if nan is None:
        nan = torch.empty(c, dtype=torch.int32, device=x.device)
    check(lib.segmi_channel_argmax(_ptr(x), c, d, h, w, _ptr(keys), _ptr(nan), _stream()), "channel_argmax")
    return keys, nan


def decode_argmax_keys(keys: np.ndarray, shape_zyx):
    """host u64 keys of channel_argmax -> (max values f32 [c], indices i64 [c, 3] in (x, y, z) order)"""
    d, h, _ = (int(v) for v in shape_zyx)
    k = np.asarray(keys).astype(np.uint64)
    hi = (k >> np.uint64(32)).astype(np.uint32)
    bits = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7FFFFFFF), ~hi).astype(np.uint32)
    lex = (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64)
    xyz = np.stack([lex // (h * d), (lex // d) % h, lex % d], axis=1)
    return bits.view(np.float32), xyz


_BBOX_DTYPES = {torch.float32: (4, 1), torch.uint8: (1, 0), torch.int16: (2, 0), torch.int32: (4, 0)}


def positive_bbox(x: torch.Tensor, box=None):
    """box i32 [6] = (x0, y0, z0, x1, y1, z1), the half-open box of the voxels > 0 of any channel of a
    contiguous [d, h, w] or [c, d, h, w] device tensor (f32, uint8, int16 or int32)."""
    d, h, w = _dense3(x, "positive_bbox")
    try:
        nbytes, is_float = _BBOX_DTYPES[x.dtype]
    except KeyError:
        raise ValueError(f"positive_bbox: float32, uint8, int16 or int32 data, not {x.dtype}")
    c = int(x.shape[0]) if x.dim() == 4 else 1
    if box is None:
        box = torch.empty(6, dtype=torch.int32, device=x.device)
    check(lib.segmi_positive_bbox(_ptr(x), nbytes, is_float, c, d, h, w, _ptr(box), _stream()), "positive_bbox")
    return box


# ------------------------------------------------------------------ MRI / CT preprocessing (N4, Otsu, CT scale)
SEGMI_EDATA = -4
N4_MAX_BINS = 512


def _vol3(t: torch.Tensor, dtype, what: str):
    """(nz, ny, nx) of a contiguous 2-D / 3-D device tensor of `dtype`"""
    _require_device(t)
    if t.dtype != dtype or not t.is_contiguous() or t.dim() not in (2, 3):
        raise ValueError(f"{what}: contiguous {dtype} [z, y, x] or [y, x] tensor expected")
    return (1,) + tuple(t.shape) if t.dim() == 2 else tuple(t.shape)


def _check_n4(rc: int, what: str) -> None:
    if rc == SEGMI_EDATA:
        raise ValueError(_lib.last_error())
    check(rc, what)


def otsu(x: torch.Tensor, bins: int = 200):
    """Otsu statistics of the finite values of a contiguous f32 device tensor: (counts i64 [bins],
    stats f64 [4] = (min, bin width, threshold, finite count)), both on the device; no host read."""
    _require_device(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError("otsu expects a non-empty contiguous float32 tensor")
    if not 2 <= bins <= N4_MAX_BINS:
        raise ValueError(f"otsu: 2 <= bins <= {N4_MAX_BINS}")
    counts = torch.empty(bins, dtype=torch.int64, device=x.device)
    stats = torch.empty(4, dtype=torch.float64, device=x.device)
    ws = torch.empty(int(lib.segmi_otsu_workspace_bytes(bins)), dtype=torch.uint8, device=x.device)
    check(lib.segmi_otsu(_ptr(x), x.numel(), bins, _ptr(counts), _ptr(stats), _ptr(ws), ws.numel(), _stream()),
          "otsu")
    return counts, stats


def n4_shrink(x: torch.Tensor, factors, mask: Optional[torch.Tensor] = None,
              otsu_stats: Optional[torch.Tensor] = None, inside: int = 0, outside: int = 1,
              want_image: bool = True, want_mask: bool = True, want_log: bool = False):
    """One gather of a f32 [z, y, x] / [y, x] volume at the shrink indices; `factors` per array axis.
    Mask: `mask` (uint8, same shape), else the Otsu threshold in `otsu_stats`, else all ones.
    Returns (image f32, mask uint8, log f64 with NaN off the fit set), each None when not wanted."""
    dims = _vol3(x, torch.float32, "n4_shrink")
    f = [1] * (3 - x.dim()) + [int(v) for v in factors]
    if len(f) != 3 or min(f) < 1:
        raise ValueError("n4_shrink: one factor >= 1 per axis")
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(x.shape)
                             or not mask.is_contiguous()):
        raise ValueError("n4_shrink: the mask must be a contiguous uint8 tensor of the image's shape")
    ns = [max(1, n // fa) for n, fa in zip(dims, f)]
    shape = tuple(ns[3 - x.dim():])
    img = torch.empty(shape, dtype=torch.float32, device=x.device) if want_image else None
    msk = torch.empty(shape, dtype=torch.uint8, device=x.device) if want_mask else None
    lg = torch.empty(shape, dtype=torch.float64, device=x.device) if want_log else None
    if otsu_stats is not None and (otsu_stats.dtype != torch.float64 or otsu_stats.numel() < 3):
        raise ValueError("n4_shrink: otsu_stats is the f64 [4] tensor of ops.otsu")
    check(lib.segmi_n4_shrink(_ptr(x), *dims, *f, _ptr(mask), _ptr(otsu_stats), int(inside), int(outside),
                              _ptr(img), _ptr(msk), _ptr(lg), _stream()), "n4_shrink")
    return img, msk, lg


def n4_lattice_shape(dims3, spans: int):
    return tuple(1 if n == 1 else spans + 3 for n in dims3)


def n4_fit(logimg: torch.Tensor, iterations, control_points: int = 4, bins: int = 200, fwhm: float = 0.15,
           noise: float = 0.01, threshold: float = 0.001, want_field: bool = False):
    """N4 on a f64 [z, y, x] / [y, x] grid of log values (NaN off the fit set).  Returns (lattice f64
    [Lz, Ly, Lx] on the device, field f64 on the grid or None, elapsed iterations per level, final CV).
    ValueError when the fit set is empty or constant."""
    dims = _vol3(logimg, torch.float64, "n4_fit")
    it = np.ascontiguousarray(np.asarray([int(v) for v in iterations], dtype=np.int32))
    levels = it.size
    if levels < 1 or (it < 0).any():
        raise ValueError("n4_fit: one non-negative iteration count per level")
    nbytes = int(lib.segmi_n4_workspace_bytes(*dims, int(control_points), levels, int(bins)))
    if nbytes <= 0:
        raise ValueError("n4_fit: unsupported size, number of levels, control points or bins")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=logimg.device)
    lat = torch.empty(n4_lattice_shape(dims, (int(control_points) - 3) << (levels - 1)), dtype=torch.float64,
                      device=logimg.device)
    field = torch.empty_like(logimg) if want_field else None
    elapsed = np.zeros(levels, np.int32)
    cv = C.c_double(0.0)
    _check_n4(lib.segmi_n4_fit(_ptr(logimg), *dims, it.ctypes.data_as(C.c_void_p), levels, int(control_points),
                               int(bins), float(fwhm), float(noise), float(threshold), _ptr(lat), _ptr(field),
                               elapsed.ctypes.data_as(C.c_void_p), C.byref(cv), _ptr(ws), ws.numel(), _stream()),
              "n4_fit")
    return lat, field, [int(v) for v in elapsed], float(cv.value)


def n4_sharpen(u: torch.Tensor, bins: int = 200, fwhm: float = 0.15, noise: float = 0.01):
    """One sharpening of the finite values of a f64 grid: (E f64 [bins], sharpened f64, NaN elsewhere)."""
    dims = _vol3(u, torch.float64, "n4_sharpen")
    nbytes = int(lib.segmi_n4_workspace_bytes(*dims, 4, 1, int(bins)))
    if nbytes <= 0:
        raise ValueError("n4_sharpen: unsupported size or bins")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=u.device)
    E = torch.empty(bins, dtype=torch.float64, device=u.device)
    out = torch.empty_like(u)
    check(lib.segmi_n4_sharpen(_ptr(u), *dims, int(bins), float(fwhm), float(noise), _ptr(E), _ptr(out), _ptr(ws),
                               ws.numel(), _stream()), "n4_sharpen")
    return E, out


def n4_bspline_fit(r: torch.Tensor, spans: int) -> torch.Tensor:
    """One BA fit of the finite values of a f64 grid at `spans` spans per axis: the lattice (f64)."""
    dims = _vol3(r, torch.float64, "n4_bspline_fit")
    nbytes = int(lib.segmi_n4_workspace_bytes(*dims, int(spans) + 3, 1, 2))
    if nbytes <= 0:
        raise ValueError("n4_bspline_fit: unsupported size or spans")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=r.device)
    lat = torch.empty(n4_lattice_shape(dims, int(spans)), dtype=torch.float64, device=r.device)
    check(lib.segmi_n4_bspline_fit(_ptr(r), *dims, int(spans), _ptr(lat), _ptr(ws), ws.numel(), _stream()),
          "n4_bspline_fit")
    return lat


def n4_refine(lat: torch.Tensor) -> torch.Tensor:
    """Exact cubic subdivision of a contiguous f64 [Lz, Ly, Lx] lattice."""
    dims = _vol3(lat, torch.float64, "n4_refine")
    if lat.dim() != 3:
        raise ValueError("n4_refine: [Lz, Ly, Lx] lattice expected")
    out = torch.empty(tuple(1 if n == 1 else 2 * (n - 3) + 3 for n in dims), dtype=torch.float64, device=lat.device)
    check(lib.segmi_n4_refine(_ptr(lat), *dims, _ptr(out), _stream()), "n4_refine")
    return out


def n4_evaluate(lat: torch.Tensor, shape, x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The field of a f64 [Lz, Ly, Lx] lattice over an index range `shape` ([z, y, x] or [y, x]) as f32, or
    x / exp(field) when the f32 volume x of that shape is given."""
    if lat.dtype != torch.float64 or not lat.is_contiguous() or lat.dim() != 3:
        raise ValueError("n4_evaluate: contiguous f64 [Lz, Ly, Lx] lattice expected")
    _require_device(lat)
    shape = tuple(int(v) for v in shape)
    dims = (1,) + shape if len(shape) == 2 else shape
    if x is not None and (_vol3(x, torch.float32, "n4_evaluate") != dims):
        raise ValueError("n4_evaluate: x does not have the evaluation shape")
    out = torch.empty(shape, dtype=torch.float32, device=lat.device)
    check(lib.segmi_n4_evaluate(_ptr(lat), *lat.shape, _ptr(x), _ptr(out), *dims, _stream()), "n4_evaluate")
    return out


def ct_scale(x: torch.Tensor) -> torch.Tensor:
    """radius-1 median (replicate borders), clamp to [-1100, 3100], (v + 1100) * 255 / 4200 of a f32 volume"""
    dims = _vol3(x, torch.float32, "ct_scale")
    out = torch.empty_like(x)
    check(lib.segmi_ct_scale(_ptr(x), *dims, _ptr(out), _stream()), "ct_scale")
    return out
