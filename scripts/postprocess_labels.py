"""Clean up a directory of label maps on the MI355X.

    python scripts/postprocess_labels.py IN_DIR OUT_DIR [--min-size N] [--keep-largest [K]] [--fill-holes]
                                         [--connectivity C] [--labels 1,2,...] [--input-glob '*.nii.gz']

Runs, in this order, the steps that were asked for: remove-small (components below N voxels), keep-largest
(the K largest components of every label, K = 1 when the option is given bare) and fill-holes, all from
segmantic_amd.seg.transforms.  --connectivity (default: full) applies to every step and --labels restricts
keep-largest and fill-holes to those labels.  Outputs have the input's name, dtype and affine.
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
from segmantic_amd.seg import transforms  # noqa: E402


def _bare_keep_largest(argv: List[str]) -> List[str]:
    """--keep-largest without a number means K = 1"""
    out = []
    for i, a in enumerate(argv):
        out.append(a)
        if a == "--keep-largest" and not (i + 1 < len(argv) and argv[i + 1].isdigit()):
            out.append("1")
    return out


def main(
    in_dir: Path = typer.Argument(..., help="directory of label maps"),
    out_dir: Path = typer.Argument(..., help="directory to write the cleaned label maps to"),
    keep_largest: int = typer.Option(0, "--keep-largest", help="keep the K largest components of every label"),
    min_size: int = typer.Option(0, "--min-size", help="remove components with fewer voxels than this"),
    fill_holes: bool = typer.Option(False, "--fill-holes", help="fill enclosed background regions"),
    connectivity: Optional[int] = typer.Option(None, "--connectivity", help="1 .. ndim (default: full)"),
    labels: Optional[str] = typer.Option(None, "--labels", help="comma-separated labels to treat (default: all)"),
    input_glob: str = typer.Option("*.nii.gz", "--input-glob", help="glob of the label maps in IN_DIR"),
) -> None:
    paths = sorted(p for p in in_dir.glob(input_glob) if p.is_file())
    if not paths:
        raise RuntimeError(f"no label map in {in_dir} matches {input_glob!r}")
    applied = [int(v) for v in labels.split(",") if v.strip()] if labels else None
    out_dir.mkdir(parents=True, exist_ok=True)
    for p in paths:
        arr, affine = read_image(p)
        lab = np.ascontiguousarray(arr)
        if min_size > 0:
            lab = transforms.remove_small_objects(lab, min_size, connectivity)
        if keep_largest > 0:
            lab = transforms.keep_largest_connected_component(lab, applied, True, connectivity, keep_largest)
        if fill_holes:
            lab = transforms.fill_holes(lab, applied, connectivity)
        write_image(out_dir / p.name, lab, affine)
    print(f"{len(paths)} label maps cleaned into {out_dir}")


if __name__ == "__main__":
    sys.argv[1:] = _bare_keep_largest(sys.argv[1:])
    typer.run(main)
