"""Fuse label maps of one grid -- several raters, or several models -- by multi-label STAPLE on the MI355X.

    python scripts/staple_labels.py OUTPUT INPUT [INPUT ...] [--tissue-list F] [--iterations N] [--tolerance T]
                                    [--performance CSV]

Every INPUT is a label map (NIfTI / MetaImage / NRRD) on the grid of the first; size, spacing, origin or direction
that differ from it are refused by name.  The number of classes is the tissue list's when one is given (iSEG
format), else the largest label + 1.  OUTPUT gets the fused labels with the first input's geometry and pixel type;
--performance writes sensitivity and positive predictive value per input and tissue (segmantic_amd.seg.staple).
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


def check_same_grid(first, other, first_path, other_path) -> None:
    """refuse ``other`` when its geometry differs from ``first``'s, naming what differs"""
    if first.GetSize() != other.GetSize():
        raise ValueError(f"{other_path}: size {other.GetSize()} differs from {first_path}: {first.GetSize()}")
    for what, a, b in (("spacing", first.GetSpacing(), other.GetSpacing()),
                       ("origin", first.GetOrigin(), other.GetOrigin()),
                       ("direction", first.GetDirection(), other.GetDirection())):
        if not np.allclose(a, b, rtol=0, atol=1e-5 * max(1.0, float(np.max(np.abs(a))))):
            raise ValueError(f"{other_path}: {what} {tuple(b)} differs from {first_path}: {tuple(a)}")


def main(
    output: Path = typer.Argument(..., metavar="OUTPUT", help="file to write the fused label map to"),
    inputs: List[Path] = typer.Argument(..., metavar="INPUT", help="label maps on one grid, one per rater"),
    tissue_list: Optional[Path] = typer.Option(None, "--tissue-list", help="label names in iSEG format"),
    iterations: int = typer.Option(100, "--iterations", help="most EM iterations"),
    tolerance: float = typer.Option(1e-5, "--tolerance", help="stop when no confusion-matrix entry moves by this much"),
    performance: Optional[Path] = typer.Option(None, "--performance", help="CSV of sensitivity / PPV per input and tissue"),
) -> None:
    from segmantic_amd.image.labels import load_tissue_list
    from segmantic_amd.image.processing import Image, read_image, write_image
    from segmantic_amd.seg import staple as S

    images = [read_image(p) for p in inputs]
    for p, im in zip(inputs[1:], images[1:]):
        check_same_grid(images[0], im, inputs[0], p)
    tissues = load_tissue_list(tissue_list) if tissue_list else None
    num_classes = max(max(tissues.values()) + 1, 2) if tissues else None
    res = S.staple(images, num_classes, max_iterations=iterations, tolerance=tolerance)
    fused = res.labels
    out = Image(fused.data.cpu(), images[0].spacing, images[0].origin, images[0].direction)
    output.parent.mkdir(parents=True, exist_ok=True)
    write_image(out, output)
    if performance:
        S.write_performance_csv(S.performance_table(res.sums, [p.name for p in inputs], tissues), performance)
    print(f"{len(inputs)} label maps fused into {output}: {res.iterations} iterations, "
          f"{'converged' if res.converged else 'not converged'}")


if __name__ == "__main__":
    typer.run(main)
