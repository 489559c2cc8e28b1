"""The landmark kernels (csrc/landmarks.hip) past one trip along x, at the V = 1 fallback behind a misaligned
pointer, at the full label table, past one pass of their capped grids and at one workgroup per channel, on the
MI355X.  Inputs and the proof that each crosses its limit: tests/helpers/preproc_limits.py and
tests/test_preproc_limits_host.py.  Centroid sums, argmax points and boxes are compared exactly with the oracle of
tests/helpers/detect_ref.py; heatmaps at the bound of tests/test_detect_gpu.py (1e-6 gamma) with its bit-zero checks.
Every call is made twice and must give identical bits."""
import numpy as np
import pytest
import torch

from segmantic_amd import ops
from segmantic_amd.detect.transforms import BoundingBoxd, VertHeatMap, _heatmap_params
from tests.helpers import detect_ref as ref
from tests.helpers import preproc_limits as lim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _aligned(a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.array(a)).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _misaligned(a: np.ndarray) -> torch.Tensor:
    """the same values as a contiguous view that starts lim.VIEW_OFFSET elements into a larger device buffer"""
    flat = torch.from_numpy(np.array(a).reshape(-1))
    buf = torch.zeros(flat.numel() + 8, dtype=flat.dtype, device=DEV)
    buf[lim.VIEW_OFFSET:lim.VIEW_OFFSET + flat.numel()].copy_(flat)
    view = buf[lim.VIEW_OFFSET:lim.VIEW_OFFSET + flat.numel()].view(a.shape)
    assert view.is_contiguous() and view.data_ptr() % (4 * view.element_size()) != 0
    return view


def _centroids_twice(t, k):
    sums, flag = ops.label_centroids(t, k)
    again, flag2 = ops.label_centroids(t, k)
    assert torch.equal(sums, again) and int(flag.item()) == int(flag2.item()) == 0
    return sums.cpu().numpy()


# ------------------------------------------------------------------ centroid sums
@pytest.mark.parametrize("dtype", lim.LABEL_DTYPES)
@pytest.mark.parametrize("shape", [lim.CENT_V4_SHAPE, lim.CENT_V1_SHAPE])
def test_centroid_sums_over_several_trips(dtype, shape):
    """centroid_kernel<T, 4> over three trips (x0 = 0, 256, 512; 8 live voxels on the last) and <T, 1> over four
    (the last ragged)"""
    lab = lim.cent_volume(shape, dtype)
    np.testing.assert_array_equal(_centroids_twice(_aligned(lab), lim.CENT_K), ref.centroid_sums(lab, lim.CENT_K))


@pytest.mark.parametrize("dtype", lim.LABEL_DTYPES)
def test_centroid_sums_behind_a_misaligned_pointer(dtype):
    """w % 4 == 0 but the base pointer is one element off: centroid_kernel<T, 1> over nine trips of 64"""
    lab = lim.cent_volume(lim.CENT_V4_SHAPE, dtype)
    np.testing.assert_array_equal(_centroids_twice(_misaligned(lab), lim.CENT_K), ref.centroid_sums(lab, lim.CENT_K))


@pytest.mark.parametrize("dtype", lim.LABEL_DTYPES)
def test_centroid_sums_of_255_labels_in_every_chunk(dtype):
    """k = kLmMaxLabels: the whole LDS table, the ballot loop with about 160 labels per chunk, uint8's 255 valid"""
    lab = lim.cent_dense(dtype)
    want = ref.centroid_sums(lab, lim.CENT_DENSE_K)
    assert (want[:, 0] > 0).all()
    np.testing.assert_array_equal(_centroids_twice(_aligned(lab), lim.CENT_DENSE_K), want)
    np.testing.assert_array_equal(_centroids_twice(_misaligned(lab), lim.CENT_DENSE_K), want)


@pytest.mark.parametrize("dtype", lim.LABEL_DTYPES)
def test_centroid_sum_x_of_a_label_past_the_first_trip(dtype):
    """a label only at x >= 256: its sum x comes through the x0 term alone"""
    lab = lim.cent_late(dtype)
    want = ref.centroid_sums(lab, lim.CENT_LATE_K)
    assert want[lim.CENT_LATE_LABEL, 1] >= 256 * want[lim.CENT_LATE_LABEL, 0] > 0
    np.testing.assert_array_equal(_centroids_twice(_aligned(lab), lim.CENT_LATE_K), want)


# ------------------------------------------------------------------ heatmap
def _check_heatmap(lab, k, gamma, smooth_3d):
    """the checks of tests/test_detect_gpu.py::_check_heatmap, and a second call with identical bits"""
    hm = VertHeatMap(keys="l", gamma=gamma, label_names=[f"v{i}" for i in range(k)], smooth_3d=smooth_3d)
    out = hm({"l": lab})["l"]
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (k + 1,) + np.shape(lab)[-3:]
    assert torch.equal(out.view(torch.int32), hm({"l": lab})["l"].view(torch.int32))
    got = out.cpu().numpy()
    want = ref.heatmap(lab, k, gamma, smooth_3d)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * gamma)
    for c in range(k + 1):
        if c == 0 or not np.any(lab == c):
            assert not np.any(got[c].view(np.uint32)), f"channel {c} is not bit-zero"
        elif not smooth_3d:
            cx = ref.centre(lab, c)[0]
            assert not np.any(np.delete(got[c], cx, axis=2)), f"channel {c} has values off the slice x = {cx}"
    return got


@pytest.mark.parametrize("smooth_3d", [False, True])
def test_heatmap_supports_across_the_trip_boundary(smooth_3d):
    """heatmap_kernel<true> with x += 256: centres at x = 250, 255, 256, 262 (supports over x = 256), 500 and 515
    (over x = 512, clipped at the far face)"""
    lab = np.array(lim.hm_trip_volume())
    got = _check_heatmap(lab, lim.HM_TRIP_K, 1000.0, smooth_3d)
    for c, (z, y, x) in lim.HM_TRIP_BLOCKS.items():
        assert got[c, z, y, x] == np.float32(1000.0) == got[c].max()      # the centre maps to exactly gamma


@pytest.mark.parametrize("smooth_3d", [False, True])
def test_heatmap_of_255_labels(smooth_3d):
    """k = kLmMaxLabels: 256 channels, 16 workgroups each over three passes of the rows, a table stride of 217 words,
    label 255's tail of 108 clipped on every axis"""
    lab = np.array(lim.hm_big_volume())
    got = _check_heatmap(lab, lim.HM_BIG_K, 1000.0, smooth_3d)
    for c, (z, y, x) in lim.HM_BIG_BLOCKS.items():
        assert got[c, z, y, x] == np.float32(1000.0) == got[c].max()
    if smooth_3d:                                  # label 255 reaches every row and x = 142 .. 299: both trips
        nz = np.nonzero(got[255])
        assert (nz[0].min(), nz[0].max(), nz[1].min(), nz[1].max()) == (0, 11, 0, 15)
        assert nz[2].min() <= 160 and nz[2].max() == 299 and not got[255, :, :, :142].any()


@pytest.mark.parametrize("smooth_3d", [False, True])
def test_heatmap_support_of_label_255_covers_the_volume(smooth_3d):
    """covers = true in hm_setup at the longest table: min P > 0 is subtracted, the far corner maps to exactly 0.
    The volume is sized so that min P <= 0.29 max P (tests/helpers/preproc_limits.py): the rescale multiplies the f32
    rounding of P by max P / (max P - min P), and a volume of (5, 6, 8), where that factor is 50, measured 3.5e-5 gamma
    with tables formed in f32 and 4e-6 gamma with correctly rounded ones, against the bound of 1e-6 gamma."""
    lab = np.array(lim.hm_cover_volume())
    got = _check_heatmap(lab, lim.HM_COVER_K, 1000.0, smooth_3d)
    if smooth_3d:
        assert got[255].min() == 0.0 and got[255].max() == np.float32(1000.0)
        want = ref.heatmap(lab, 255, 1000.0, True)[255]
        assert np.array_equal(got[255] == 0, want == 0) and 0 < np.count_nonzero(want == 0) <= 8


def test_heatmap_kernel_alone_at_255_labels():
    """ops.vert_heatmap on given sums: the same bits as the transform's call, no label volume needed"""
    lab = lim.hm_big_volume()
    sums = torch.from_numpy(ref.centroid_sums(lab, 255)).to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.vert_heatmap(_heatmap_params(DEV, 255, 1000.0), 255, sums, flag, lab.shape, True)
    want = VertHeatMap(keys="l", label_names=["v"] * 255, smooth_3d=True)({"l": np.array(lab)})["l"]
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------ channel argmax
def _argmax_twice(t):
    keys, nan = ops.channel_argmax(t)
    again, nan2 = ops.channel_argmax(t)
    assert torch.equal(keys, again) and torch.equal(nan, nan2)
    vals, xyz = ops.decode_argmax_keys(keys.cpu().numpy(), t.shape[1:])
    return vals, xyz, nan.cpu().numpy()


@pytest.mark.parametrize("shape, view", [(lim.AM_SHAPES[0], "aligned"), (lim.AM_SHAPES[0], "misaligned"),
                                         (lim.AM_SHAPES[1], "aligned")])
def test_argmax_past_the_first_trip_and_tied_across_it(shape, view):
    """argmax_kernel<true> over three trips and <false> over four (or nine, behind the misaligned pointer): a
    maximum past the first trip; one tied in the same lane of two trips, where the smaller x wins although it is
    later in [z, y, x] order"""
    x = lim.am_volume(shape)
    vals, xyz, nan = _argmax_twice(_aligned(x) if view == "aligned" else _misaligned(x))
    want_vals, want_xyz = lim.argmax_points(x)
    np.testing.assert_array_equal(xyz, want_xyz)
    np.testing.assert_array_equal(vals.view(np.uint32), want_vals.view(np.uint32))
    assert not nan.any()


def test_argmax_of_4100_channels():
    """more channels than kLmMaxWgs: lm_grid falls to one workgroup per channel, grid.y = 4100"""
    x = lim.am_many()
    vals, xyz, nan = _argmax_twice(_aligned(x))
    want_vals, want_xyz = lim.argmax_points(x)
    np.testing.assert_array_equal(xyz, want_xyz)
    np.testing.assert_array_equal(vals.view(np.uint32), want_vals.view(np.uint32))
    assert not nan.any()


def test_argmax_nan_flag_past_the_first_trip():
    x = lim.am_nan_volume()
    vals, xyz, nan = _argmax_twice(_aligned(x))
    assert nan.tolist() == [0, 1, 0]
    want_vals, want_xyz = lim.argmax_points(lim.am_volume(lim.AM_SHAPES[0]))   # the NaN replaced no maximum
    np.testing.assert_array_equal(xyz, want_xyz)
    np.testing.assert_array_equal(vals.view(np.uint32), want_vals.view(np.uint32))


# ------------------------------------------------------------------ positive box
def _box_twice(t):
    box = ops.positive_bbox(t)
    assert torch.equal(box, ops.positive_bbox(t))
    b = box.cpu().tolist()
    return [b[:3], b[3:]]


@pytest.mark.parametrize("dtype", lim.PBOX_DTYPES)
def test_box_of_a_voxel_in_the_second_pass_of_the_grid(dtype):
    """16 800 rows against 4096 workgroups x 4 rows: the only positive voxel lies in a row of the second pass"""
    x = lim.pbox_rows_volume(dtype)
    want = ref.bbox(x)
    assert want[1] != [0, 0, 0]
    assert _box_twice(_aligned(x)) == want
    assert BoundingBoxd(keys="x")({"x": np.array(x)})["result"]["bbox"] == want


@pytest.mark.parametrize("dtype", lim.PBOX_DTYPES)
@pytest.mark.parametrize("shape", lim.PBOX_TRIP_SHAPES)
def test_box_faces_from_later_trips(shape, dtype):
    """pbox_kernel<T, 4> over three trips, <T, 1> over four: both x faces come from trips after the first"""
    x = lim.pbox_trip_volume(shape, dtype)
    want = ref.bbox(x)
    assert _box_twice(_aligned(x)) == want
    if shape[3] % 4 == 0:
        assert _box_twice(_misaligned(x)) == want
