"""Grow, shrink, open or close the labels of a directory of label maps by a radius in millimetres, on the MI355X.

    python scripts/label_morphology.py IN_DIR OUT_DIR --op dilate|erode|open|close|expand --radius MM
                                       [--labels N ...] [--input-glob '*.nii.gz']

The voxel spacing comes from each image's header.  dilate / erode / open / close treat the labels given with
--labels (default: every label); expand is scikit-image's expand_labels (every label grows, --labels is not
accepted).  The operations are those of segmantic_amd.seg.morphology; results are exact and canonical (equally
near labels: the voxel with the smallest raster index wins).  Outputs have the input's name, dtype and affine.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import List, Optional

import numpy as np
import typer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd.data.imageio import read_image, write_image  # noqa: E402
from segmantic_amd.seg import morphology  # noqa: E402

OPS = {"dilate": morphology.dilate_labels, "erode": morphology.erode_labels, "open": morphology.open_labels,
       "close": morphology.close_labels, "expand": morphology.expand_labels}


def array_spacing(affine: np.ndarray) -> tuple:
    """spacing per array axis [z, y, x]: the affine's columns are the voxel axes (x, y, z) in mm"""
    sp = np.sqrt((np.asarray(affine, np.float64)[:3, :3] ** 2).sum(0))
    if not (np.all(np.isfinite(sp)) and np.all(sp > 0)):
        raise ValueError(f"the image header gives no usable voxel spacing: {sp.tolist()}")
    return tuple(float(s) for s in sp[::-1])


def main(
    in_dir: Path = typer.Argument(..., help="directory of label maps"),
    out_dir: Path = typer.Argument(..., help="directory to write the results to"),
    op: str = typer.Option(..., "--op", help="dilate | erode | open | close | expand"),
    radius: float = typer.Option(..., "--radius", help="radius in millimetres (>= 0)"),
    labels: Optional[List[int]] = typer.Option(None, "--labels", help="labels to treat (default: all); repeatable"),
    input_glob: str = typer.Option("*.nii.gz", "--input-glob", help="glob of the label maps in IN_DIR"),
) -> None:
    if op not in OPS:
        raise typer.BadParameter(f"--op must be one of {', '.join(OPS)}, got {op!r}")
    if not (np.isfinite(radius) and radius >= 0):
        raise typer.BadParameter(f"--radius must be finite and >= 0, got {radius}")
    applied = [int(v) for v in labels] if labels else None
    if op == "expand" and applied is not None:
        raise typer.BadParameter("--labels does not apply to --op expand (every label grows); use dilate")
    paths = sorted(p for p in in_dir.glob(input_glob) if p.is_file())
    if not paths:
        raise RuntimeError(f"no label map in {in_dir} matches {input_glob!r}")
    out_dir.mkdir(parents=True, exist_ok=True)
    for p in paths:
        arr, affine = read_image(p)
        lab = np.ascontiguousarray(arr)
        sp = array_spacing(affine)
        if op == "expand":
            res = morphology.expand_labels(lab, radius, sp)
        else:
            res = OPS[op](lab, radius, sp, applied)
        write_image(out_dir / p.name, res, affine)
    print(f"{len(paths)} label maps written to {out_dir} ({op}, radius {radius} mm)")


def _spread_labels(argv: List[str]) -> List[str]:
    """--labels 1 2 3 -> --labels 1 --labels 2 --labels 3"""
    out, i = [], 0
    while i < len(argv):
        out.append(argv[i])
        if argv[i] == "--labels":
            i += 1
            first = True
            while i < len(argv) and argv[i].lstrip("-").isdigit():
                if not first:
                    out.append("--labels")
                out.append(argv[i])
                first = False
                i += 1
            continue
        i += 1
    return out


if __name__ == "__main__":
    sys.argv[1:] = _spread_labels(sys.argv[1:])
    typer.run(main)
