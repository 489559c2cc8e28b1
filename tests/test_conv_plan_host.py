"""The convolution family's launch decisions, pinned on the host.

``tests/golden/conv_plan_parent.json`` records what the queries (kernel name, statistics rows, fusion capabilities,
weight-gradient workspace) answered for 2604 layers on the commit before the decisions moved into one plan per launch
(``csrc/conv_plan.h``, ``WgradPlan``).  They are host arithmetic over the fields of the views, so the library under
test must reproduce every row exactly -- no GPU involved.  The statistics rows and the workspace are what the engine
allocates and the kernels write ``grid.x`` rows or slabs into, so a row that moves is an out-of-bounds write (or an
allocation that grew) on the device.
"""
import json
import os
import re
from pathlib import Path

import pytest

from segmantic_amd import _lib
from tests.helpers.conv_plan_queries import CASE_FIELDS, evaluate

GOLDEN = json.loads((Path(__file__).parent / "golden" / "conv_plan_parent.json").read_text())
NCASE = len(CASE_FIELDS)
NAMES, ROWS, TAGS = GOLDEN["names"], GOLDEN["rows"], GOLDEN["tags"]


def recorded(row):
    return [NAMES[row[NCASE]]] + row[NCASE + 1:]


def test_every_recorded_decision_is_reproduced():
    assert "SEGMI_WGRAD_CUS" not in os.environ, "SEGMI_WGRAD_CUS overrides the `cus` argument the table was recorded with"
    assert GOLDEN["fields"] == list(CASE_FIELDS) and len(ROWS) > 2000
    wrong = []
    for row in ROWS:
        got = evaluate(_lib, tuple(row[:NCASE]))
        if got != recorded(row):
            wrong.append((dict(zip(CASE_FIELDS, row)), recorded(row), got))
    assert not wrong, f"{len(wrong)} of {len(ROWS)} rows differ; first: {wrong[0]}"


def test_the_table_covers_every_kernel_name_the_code_can_produce():
    """Every forward family x the template arguments its name carries.  conv_fwd_mfma<CK=32, k3 s1> and
    <f32, CK=16, k3 s1> are not in the list because no layer reaches them: a k3 s1 layer whose chunk takes one k-step
    per tap (every f32 layer, every 16-bit layer of 32-channel chunks) goes to the k-split kernel first."""
    want = []
    for dt in ("bf16", "f16"):
        want += [f"conv_ring3_kernel<{dt}, CK=16> (LDS-DMA ring)", f"conv_ring2_kernel<{dt}, CK=16, NT=1>",
                 f"conv_ring2_kernel<{dt}, CK=32, NT=1>", f"conv_ring2_kernel<{dt}, CK=32, NT=2>",
                 f"conv_fwd_mfma_kernel<{dt}, CK=16, k3 s1>"]
        want += [f"conv_fwd_mfma_kernel<{dt}, CK={ck}, {ks}>" for ck in (16, 32) for ks in ("k3 s2", "k1 s1")]
    want += [f"conv_fwd_mfma_kernel<f32, CK=16, {ks}>" for ks in ("k3 s2", "k1 s1")]
    for dt in ("f32", "bf16", "f16"):
        want += [f"conv_fwd_ks_kernel<{dt}, k3 s1>", f"conv_small_fwd_kernel<{dt}>", f"conv_direct_kernel<{dt}>"]
    assert sorted(NAMES) == sorted(want)
    used = {row[NCASE] for row in ROWS}
    assert used == set(range(len(NAMES)))


FAMILY_OF_TAG = {"fwd:ring3": r"conv_ring3_kernel<bf16, CK=16>", "fwd:ring2 ck32 nt2": r"conv_ring2_kernel<bf16, CK=32, NT=2>",
                 "fwd:ring2 ck32 nt1": r"conv_ring2_kernel<bf16, CK=32, NT=1>", "fwd:ring2 ck16": r"conv_ring2_kernel<bf16, CK=16, NT=1>",
                 "fwd:k-split": r"conv_fwd_ks_kernel<bf16", "fwd:k-split wide": r"conv_fwd_ks_kernel<f32",
                 "fwd:tile k3 s1": r"conv_fwd_mfma_kernel<bf16, CK=16, k3 s1>", "fwd:tile k3 s2": r"conv_fwd_mfma_kernel<bf16, CK=32, k3 s2>",
                 "fwd:tile k1": r"conv_fwd_mfma_kernel<bf16, CK=16, k1 s1>", "fwd:small-cin": r"conv_small_fwd_kernel<f32>",
                 "fwd:direct": r"conv_direct_kernel<f32>"}


def test_the_named_layers_take_their_families_with_the_rows_recorded_for_them():
    """The layers tests/test_conv_plan_gpu.py launches: family and statistics rows as the issue's table lists them."""
    for tag, pat in FAMILY_OF_TAG.items():
        assert re.match(pat, recorded(ROWS[TAGS[tag]])[0]), tag
    rows = {tag: recorded(ROWS[i])[1] for tag, i in TAGS.items()}
    reserve = rows["fwd:k-split"] - 4          # 1 x 8 x 8 x 8 in 4 x 4 x 8 tiles: 4 workgroups
    assert reserve > 0
    assert rows["fwd:ring3"] == rows["fwd:ring2 ck32 nt2"] == rows["fwd:ring2 ck32 nt1"] == rows["fwd:ring2 ck16"] == 256 + reserve
    assert rows["fwd:k-split wide"] == 32 + reserve
    # both transposed families, with different rows: 16 persistent workgroups, 8 tiles
    tp, tt = recorded(ROWS[TAGS["convT:persistent"]]), recorded(ROWS[TAGS["convT:tile"]])
    assert tp[7] == 16 + reserve and tt[7] == 8 + reserve


def test_the_table_holds_every_weight_gradient_path_and_a_batch_split():
    """Wave-specialised, MFMA, small-Cin, direct, and the 4 GiB batch split: the slab workspace of each differs, and
    only the paths that size their grid by `cus` answer differently for 64 / 128 / the whole chip."""
    ws = {tag: recorded(ROWS[i])[4:7] for tag, i in TAGS.items() if tag.startswith("wgrad:")}
    assert set(ws) == {"wgrad:wave-specialised", "wgrad:mfma", "wgrad:small-cin", "wgrad:direct", "wgrad:batch parts"}
    assert len({tuple(v) for v in ws.values()}) == 5
    for tag in ("wgrad:wave-specialised", "wgrad:batch parts"):
        assert len(set(ws[tag])) > 1, tag
    # the MFMA layer (2 x 16^3) has 16 tiles, fewer than any grid `cus` would size: its slabs are its tiles
    for tag in ("wgrad:mfma", "wgrad:small-cin", "wgrad:direct"):
        assert len(set(ws[tag])) == 1, tag
    # the same layer 8 bytes in leaves the wave-specialised kernel for the direct one
    a, b = ROWS[TAGS["wgrad:wave-specialised"]], ROWS[TAGS["wgrad:direct"]]
    assert [x for x, y in zip(a[:NCASE], b[:NCASE]) if x != y] == [0]
    # the batch split: 8 x 160^3 x 32 channels in 96-wide rows is over the 4 GiB of a descriptor, each half is not.  Two launches of the
    # wave-specialised grid: 2 x 128 slabs sized for the whole chip, 2 x 64 sized for 128 CUs
    c = dict(zip(CASE_FIELDS, ROWS[TAGS["wgrad:batch parts"]]))
    assert c["n"] * c["d"] * c["h"] * c["w"] * c["ldi"] * 2 > 0xfff00000 > c["n"] // 2 * c["d"] * c["h"] * c["w"] * c["ldi"] * 2
    nout = c["cin"] * c["cout"] * 27 * 4
    assert ws["wgrad:batch parts"][0] - ws["wgrad:batch parts"][2] == (256 - 128) * nout


@pytest.mark.parametrize("null_in,null_out", [(True, False), (False, True)])
def test_queries_answer_zero_or_invalid_for_missing_views(null_in, null_out):
    import ctypes as C
    a = _lib.Act(0x1000, 1, 8, 8, 8, 16, 16)
    pi = None if null_in else C.byref(a)
    po = None if null_out else C.byref(a)
    lib = _lib.lib
    assert lib.segmi_conv3d_stats_rows(1, pi, po, 3, 1) == 0
    assert lib.segmi_convT3d_stats_rows(1, pi, po) == 0
    assert lib.segmi_conv3d_fwd_kernel_name(1, pi, po, 3, 1) == b"invalid"
    assert not lib.segmi_conv3d_in_affine_ok(1, pi, po, 3, 1) and not lib.segmi_conv3d_bn_bwd_sums_ok(1, pi, po, 3, 1)
    assert not lib.segmi_conv3d_split_act_ok(1, pi, po, 3, 1)
    assert lib.segmi_conv3d_wgrad_workspace(1, pi, po, 3, 1, 0) == 0
