"""The poisoned-arena helper notices what it claims to notice (CPU tensors, no GPU)."""
import pytest
import torch

from tests.helpers import view_arena as va

DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16"),
          pytest.param(torch.float16, id="f16")]
SHAPE = (2, 3, 5, 7, 8)            # ragged, two samples; guard = max(64, 5 * 7 + 7) = 64 rows
FORMS = sorted(va.forms(SHAPE[-1]).items())


def written(shape, dtype):
    g = torch.Generator().manual_seed(5)
    return (torch.rand(shape, generator=g) * 2 - 1).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_poison_is_a_quiet_nan_and_survives_copies_bit_for_bit(dtype):
    p = va.poison_of(dtype)
    assert bool(torch.isnan(p)) and p.dtype == dtype
    want = va.POISON[dtype]
    assert int(va.bits(p).item()) == want
    # quiet: the top fraction bit is set
    quiet = {torch.float32: 1 << 22, torch.bfloat16: 1 << 6, torch.float16: 1 << 9}[dtype]
    assert want & quiet
    rows, view = va.arena(SHAPE, dtype, 16, 4)
    for copy in (rows.clone(), rows.clone().contiguous().reshape(-1).clone().reshape(rows.shape), view.contiguous(),
                 torch.empty_like(rows).copy_(rows)):
        assert bool((va.bits(copy) == want).all())
        assert bool(torch.isnan(copy).all())


def test_guard_rows_cover_a_plane_and_a_row():
    assert va.guard_rows((2, 3, 5, 7, 8)) == 64
    assert va.guard_rows((1, 4, 20, 30, 16)) == 20 * 30 + 30
    rows, view = va.arena((1, 4, 20, 30, 16), torch.bfloat16)
    assert rows.shape == (2 * 630 + 4 * 20 * 30, 16)
    assert view.data_ptr() == rows.data_ptr() + 630 * 16 * 2


@pytest.mark.parametrize("name,ld_c0", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_clean_arena_passes_and_each_planted_violation_is_flagged(dtype, name, ld_c0):
    ld, c0 = ld_c0
    n, d, h, w, c = SHAPE
    nrows, guard = n * d * h * w, va.guard_rows(SHAPE)

    def fresh():
        rows, view = va.arena(SHAPE, dtype, ld, c0)
        assert view.shape == SHAPE and view.stride(3) == ld and view.stride(4) == 1
        assert view.data_ptr() == rows.data_ptr() + (guard * ld + c0) * rows.element_size()
        return rows, view

    rows, view = fresh()
    assert va.untouched(rows) and va.outside_intact(rows, view) and not va.inside_written(view)
    va.fill_view(view, written(SHAPE, dtype))
    assert va.outside_intact(rows, view) and va.inside_written(view) and not va.untouched(rows)
    assert torch.equal(view, written(SHAPE, dtype))

    # stores outside the view: leading guard, trailing guard, sibling channels of the first and last row
    plants = {"leading guard": (guard - 1, ld - 1), "trailing guard": (guard + nrows, 0),
              "far leading guard": (0, 0), "far trailing guard": (rows.shape[0] - 1, ld - 1)}
    if ld > c:
        sib = c0 + c if c0 + c < ld else c0 - 1
        plants["sibling channel of the first row"] = (guard, sib)
        plants["sibling channel of the last row"] = (guard + nrows - 1, sib)
        if c0 > 0 and c0 + c < ld:
            plants["sibling channel in front of the first row"] = (guard, c0 - 1)
    for what, (r, ch) in plants.items():
        rows, view = fresh()
        va.fill_view(view, written(SHAPE, dtype))
        rows[r, ch] = 0.0                      # even a zero is a store
        assert not va.outside_intact(rows, view), what
        assert va.inside_written(view), what
        # a NaN of another payload is a store too
        rows, view = fresh()
        va.bits(rows)[r, ch] = va.POISON[dtype] ^ 1
        assert not va.outside_intact(rows, view), what

    # one element of the interior left unwritten
    rows, view = fresh()
    vals = written(SHAPE, dtype)
    va.fill_view(view, vals)
    va.bits(view)[1, 1, 2, 3, c // 2] = va.POISON[dtype]
    assert not va.inside_written(view)
    assert va.outside_intact(rows, view)
    # ... and the corners of the view count as inside
    for idx in ((0, 0, 0, 0, 0), (n - 1, d - 1, h - 1, w - 1, c - 1)):
        rows, view = fresh()
        va.fill_view(view, vals)
        va.bits(view)[idx] = va.POISON[dtype]
        assert not va.inside_written(view) and va.outside_intact(rows, view)


def test_arena_refuses_a_slice_that_leaves_the_row_and_values_of_another_shape():
    with pytest.raises(ValueError):
        va.arena(SHAPE, torch.bfloat16, 12, 8)
    rows, view = va.arena(SHAPE, torch.float32)
    with pytest.raises(ValueError):
        va.fill_view(view, torch.zeros((2, 3, 5, 7, 4)))
