"""Put a moving image on the grid of a fixed image, on the MI355X (the reference's scripts/interpolate_to_reference.py).

    python scripts/interpolate_to_reference.py MOVING FIXED OUTPUT [--nearest]
                                [--interpolator linear|nearest|bspline|label-gaussian] [--sigma S] [--alpha A]

MOVING, FIXED and OUTPUT are NIfTI / MetaImage / NRRD files, 2-D or 3-D.  The result has FIXED's size, spacing,
origin and direction and MOVING's pixel type; voxels outside MOVING are 0.  Without --interpolator the choice is
linear, or nearest neighbour with --nearest.  bspline is the cubic B-spline for images, label-gaussian the
Gaussian label vote for label maps: --sigma (in voxels of MOVING, default 1) and --alpha (default 2) set its
window, radius ceil(alpha * sigma) voxels, at most 8.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import Optional

import typer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd.image import processing  # noqa: E402

INTERPOLATORS = {"linear": processing.sitkLinear, "nearest": processing.sitkNearestNeighbor,
                 "bspline": processing.sitkBSpline, "label-gaussian": processing.sitkLabelGaussian}


def main(
    moving: Path = typer.Argument(..., metavar="MOVING", help="image to resample"),
    fixed: Path = typer.Argument(..., metavar="FIXED", help="image whose grid the result gets"),
    output: Path = typer.Argument(..., metavar="OUTPUT", help="file to write"),
    nearest: bool = typer.Option(False, "--nearest", help="nearest-neighbour interpolation"),
    interpolator: Optional[str] = typer.Option(None, "--interpolator", help=" | ".join(INTERPOLATORS)),
    sigma: Optional[float] = typer.Option(None, "--sigma", help="label-gaussian: sigma in voxels of MOVING (default 1)"),
    alpha: Optional[float] = typer.Option(None, "--alpha", help="label-gaussian: window radius in sigmas (default 2)"),
) -> None:
    if interpolator is not None and interpolator not in INTERPOLATORS:
        raise typer.BadParameter(f"--interpolator must be one of {', '.join(INTERPOLATORS)}, got {interpolator!r}")
    name = INTERPOLATORS[interpolator] if interpolator is not None else None
    kwargs = {}
    if sigma is not None:
        kwargs["sigma"] = sigma
    if alpha is not None:
        kwargs["alpha"] = alpha
    try:
        processing._interpolator(nearest, name, kwargs.get("sigma", 1.0), kwargs.get("alpha", 2.0))
    except ValueError as e:
        raise typer.BadParameter(str(e))
    result = processing.resample_to_ref(processing.read_image(moving), processing.read_image(fixed), nearest,
                                        interpolator=name, **kwargs)
    processing.write_image(result, output)
    print(f"{output}: {moving.name} on the grid of {fixed.name}, size {result.GetSize()}, "
          f"{name or ('nearest' if nearest else 'linear')}")


if __name__ == "__main__":
    typer.run(main)
