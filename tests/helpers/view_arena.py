"""Poisoned arenas around ``segmi_act`` views: where a kernel reads and writes, not what it computes.

An activation view is a base pointer, ``n d h w c`` and a row stride ``ld >= c``.  ``arena`` allocates the rows of a
view with ``guard`` extra rows in front and behind, fills every element (guards, sibling channels and the view itself)
with a quiet NaN whose payload no kernel produces, and returns the flat arena with the view cut out of it.  After a
launch

* ``outside_intact(arena, view)``: every element outside the view still holds the poison bits (nothing was stored
  outside the view), and
* ``inside_written(view)``: no element of the view holds them (every element of an output was stored).

A *read* outside an input view brings the NaN into the result unless the kernel discards it with a select; a test
sees that as a non-finite output.  The comparisons go through an integer view of the same width: NaN != NaN.
"""
from __future__ import annotations

import torch

POISON = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FC5, torch.float16: 0x7E5A}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
MIN_GUARD = 64


def forms(c: int) -> dict:
    """the view forms of a ``c``-channel view by name: (ld, c0)"""
    return {"dense": (c, 0), "left": (2 * c, 0), "right": (2 * c, c), "odd": (2 * c, 4)}


def guard_rows(shape_ndhwc) -> int:
    """a whole z-plane plus a row of overrun still lands in the guard"""
    _, _, h, w, _ = shape_ndhwc
    return max(MIN_GUARD, h * w + w)


def bits(t: torch.Tensor) -> torch.Tensor:
    """``t`` as integers of its own width (works on non-contiguous views: the element size is unchanged)"""
    return t.view(_INT[t.dtype])


def poison_of(dtype, device="cpu") -> torch.Tensor:
    """the poison as a 0-d tensor of ``dtype``"""
    return torch.tensor(POISON[dtype], dtype=torch.int32, device=device).to(_INT[dtype]).view(dtype)


def arena(shape_ndhwc, dtype, ld=None, c0=0, poison=None, device="cpu"):
    """(arena [guard + n*d*h*w + guard, ld], view [n, d, h, w, c] = rows[guard:-guard][..., c0:c0 + c]), all poison"""
    n, d, h, w, c = shape_ndhwc
    ld = c if ld is None else ld
    if c0 < 0 or c0 + c > ld:
        raise ValueError(f"channels [{c0}, {c0 + c}) do not fit a row of {ld}")
    poison = POISON[dtype] if poison is None else poison
    guard = guard_rows(shape_ndhwc)
    rows = torch.empty((guard + n * d * h * w + guard, ld), dtype=dtype, device=device)
    bits(rows).fill_(torch.tensor(poison, dtype=torch.int32).to(_INT[dtype]).item())
    view = rows[guard:guard + n * d * h * w].view(n, d, h, w, ld)[..., c0:c0 + c]
    return rows, view


def fill_view(view: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """operand data into an input view; the rest of its arena stays poisoned"""
    if tuple(values.shape) != tuple(view.shape):
        raise ValueError(f"values {tuple(values.shape)} do not match the view {tuple(view.shape)}")
    view.copy_(values.to(device=view.device, dtype=view.dtype))
    return view


def _locate(arena_rows: torch.Tensor, view: torch.Tensor):
    """(first row, rows, first channel, channels) of ``view`` inside ``arena_rows``"""
    esz = arena_rows.element_size()
    ld = arena_rows.shape[1]
    off = (view.data_ptr() - arena_rows.data_ptr()) // esz
    assert 0 <= off and (view.data_ptr() - arena_rows.data_ptr()) % esz == 0, "the view is not part of this arena"
    n, d, h, w, c = view.shape
    r0, c0 = divmod(off, ld)
    assert r0 + n * d * h * w <= arena_rows.shape[0] and c0 + c <= ld, "the view is not part of this arena"
    return r0, n * d * h * w, c0, c


def outside_intact(arena_rows: torch.Tensor, view: torch.Tensor, poison=None) -> bool:
    """every element of the arena outside the view still holds the exact poison bits"""
    poison = bits(poison_of(arena_rows.dtype)).item() if poison is None else poison
    r0, nr, c0, c = _locate(arena_rows, view)
    ok = bits(arena_rows) == poison
    ok[r0:r0 + nr, c0:c0 + c] = True
    return bool(ok.all())


def inside_written(view: torch.Tensor, poison=None) -> bool:
    """no element of the view holds the poison bits"""
    poison = bits(poison_of(view.dtype)).item() if poison is None else poison
    return not bool((bits(view) == poison).any())


def untouched(arena_rows: torch.Tensor, poison=None) -> bool:
    """the whole arena, view included, still holds the poison (a refused launch stored nothing)"""
    poison = bits(poison_of(arena_rows.dtype)).item() if poison is None else poison
    return bool((bits(arena_rows) == poison).all())
