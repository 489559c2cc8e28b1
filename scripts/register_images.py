"""Register a moving image to a fixed image by mutual information on the MI355X, and carry images or label maps
across the transform found.

    python scripts/register_images.py fit MOVING FIXED TRANSFORM.json [--transform-type translation|rigid|affine|bspline]
                                [--metric nmi|mi] [--levels 4,2,1] [--bins 16|32|64] [--fixed-mask F] [--init geometry]
                                [--grid-spacing MM] [--regularisation L] [--initial TRANSFORM.json]
    python scripts/register_images.py apply MOVING FIXED OUTPUT --transform TRANSFORM.json [--nearest]
                                [--interpolator linear|nearest|bspline|label-gaussian] [--sigma S] [--alpha A]
                                [--save-jacobian FILE]

MOVING, FIXED, F and OUTPUT are NIfTI / MetaImage / NRRD files, 2-D or 3-D.  ``fit`` writes the transform (fixed
physical points -> moving physical points) as JSON.  ``apply`` resamples MOVING onto FIXED's grid through it, with
the interpolators of scripts/interpolate_to_reference.py, so a label map follows its image (--interpolator
label-gaussian, or --nearest).

``--transform-type bspline`` fits a B-spline free-form deformation on top of an affine matrix:
the one in ``--initial`` (a file written by ``fit``), or, without it, the affine registration run first.  ``apply``
reads the kind from the file; through a bspline transform it interpolates linear or nearest only, FIXED must have the
geometry the transform was fitted on, and ``--save-jacobian`` writes the determinant map (<= 0 where it folds).
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import Optional

import typer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd.image import processing, registration  # noqa: E402

INTERPOLATORS = {"linear": processing.sitkLinear, "nearest": processing.sitkNearestNeighbor,
                 "bspline": processing.sitkBSpline, "label-gaussian": processing.sitkLabelGaussian}

app = typer.Typer(add_completion=False, help=__doc__)


def parse_levels(text: str):
    try:
        return tuple(int(v) for v in text.split(","))
    except ValueError:
        raise ValueError(f"--levels is a comma-separated list of pyramid factors such as 4,2,1, got {text!r}")


def fit(moving: Path, fixed: Path, transform_file: Path, transform_type: str = "rigid", metric: str = "nmi",
        levels=(4, 2, 1), bins: int = 32, fixed_mask: Optional[Path] = None, init: Optional[str] = None,
        grid_spacing: Optional[float] = None, regularisation: Optional[float] = None, initial: Optional[Path] = None):
    """Register the file ``moving`` to the file ``fixed`` and write ``transform_file``; returns the result."""
    if transform_type != registration.BSPLINE:
        for name, value in (("--grid-spacing", grid_spacing), ("--regularisation", regularisation), ("--initial", initial)):
            if value is not None:
                raise ValueError(f"{name} belongs to --transform-type {registration.BSPLINE}, not to {transform_type!r}")
    fixed_image = processing.read_image(fixed)
    mask = processing.read_image(fixed_mask) if fixed_mask is not None else None
    if transform_type == registration.BSPLINE:
        moving_image = processing.read_image(moving)
        if initial is not None:
            doc = registration.load_transform(initial)
            if doc["kind"] == registration.BSPLINE:
                raise ValueError(f"--initial {initial} holds a bspline transform; a matrix transform is needed")
            matrix = doc["matrix"]
        else:
            matrix = registration.register(fixed_image, moving_image, transform="affine", metric=metric, bins=bins,
                                           levels=levels, fixed_mask=mask, initial=init).transform
        result = registration.register_deformable(
            fixed_image, moving_image, initial=matrix, levels=levels, metric=metric, bins=bins, fixed_mask=mask,
            grid_spacing=16.0 if grid_spacing is None else grid_spacing,
            regularisation=0.01 if regularisation is None else regularisation)
        registration.save_transform(transform_file, result)
        return result
    result = registration.register(fixed_image, processing.read_image(moving), transform=transform_type, metric=metric,
                                   bins=bins, levels=levels, fixed_mask=mask, initial=init)
    registration.save_transform(transform_file, result, fixed_image)
    return result


def apply(moving: Path, fixed: Path, output: Path, transform_file: Path, nearest: bool = False,
          interpolator: Optional[str] = None, sigma: Optional[float] = None, alpha: Optional[float] = None,
          save_jacobian: Optional[Path] = None):
    """Resample the file ``moving`` onto the grid of ``fixed`` through the transform in ``transform_file``."""
    if interpolator is not None and interpolator not in INTERPOLATORS:
        raise ValueError(f"--interpolator must be one of {', '.join(INTERPOLATORS)}, got {interpolator!r}")
    name = INTERPOLATORS[interpolator] if interpolator is not None else None
    kwargs = {}
    if sigma is not None:
        kwargs["sigma"] = sigma
    if alpha is not None:
        kwargs["alpha"] = alpha
    processing._interpolator(nearest, name, kwargs.get("sigma", 1.0), kwargs.get("alpha", 2.0))
    doc = registration.load_transform(transform_file)
    moving_image, fixed_image = processing.read_image(moving), processing.read_image(fixed)
    if doc["kind"] == registration.BSPLINE:
        if name not in (None, processing.sitkLinear, processing.sitkNearestNeighbor):
            raise ValueError(f"--interpolator {interpolator} is not available through a bspline transform: linear or nearest")
        result = registration.warp(moving_image, fixed_image, doc["result"], nearest or name == processing.sitkNearestNeighbor)
        processing.write_image(result, output)
        if save_jacobian is not None:
            det = registration.jacobian_determinant(doc["result"]).cpu()
            processing.write_image(processing.Image(det, fixed_image.spacing, fixed_image.origin, fixed_image.direction),
                                   save_jacobian)
        return result
    if save_jacobian is not None:
        raise ValueError(f"--save-jacobian belongs to a bspline transform; {transform_file} holds a {doc['kind']} one")
    if moving_image.GetDimension() != doc["matrix"].shape[0] - 1 or fixed_image.GetDimension() != moving_image.GetDimension():
        raise ValueError(f"{transform_file} holds a {doc['matrix'].shape[0] - 1}-D transform; the images are "
                         f"{moving_image.GetDimension()}-D and {fixed_image.GetDimension()}-D")
    result = processing.apply_transform(moving_image, fixed_image, doc["matrix"], nearest, interpolator=name, **kwargs)
    processing.write_image(result, output)
    return result


@app.command("fit")
def fit_command(
    moving: Path = typer.Argument(..., metavar="MOVING", help="image to align"),
    fixed: Path = typer.Argument(..., metavar="FIXED", help="image to align it to"),
    transform_file: Path = typer.Argument(..., metavar="TRANSFORM.json", help="file to write"),
    transform_type: str = typer.Option("rigid", "--transform-type",
                                       help=" | ".join(registration.TRANSFORMS + (registration.BSPLINE,))),
    metric: str = typer.Option("nmi", "--metric", help=" | ".join(registration.METRICS)),
    levels: str = typer.Option("4,2,1", "--levels", help="pyramid factors, coarse to fine"),
    bins: int = typer.Option(32, "--bins", help="16 | 32 | 64"),
    fixed_mask: Optional[Path] = typer.Option(None, "--fixed-mask", help="image on FIXED's grid: samples where it is 0 are ignored"),
    init: Optional[str] = typer.Option(None, "--init", help="geometry: start with the grid centres aligned"),
    grid_spacing: Optional[float] = typer.Option(None, "--grid-spacing", help="bspline: control spacing of the finest level in mm (default 16)"),
    regularisation: Optional[float] = typer.Option(None, "--regularisation", help="bspline: weight of the membrane energy (default 0.01)"),
    initial: Optional[Path] = typer.Option(None, "--initial", help="bspline: matrix transform file to start from (default: fit an affine one first)"),
) -> None:
    try:
        r = fit(moving, fixed, transform_file, transform_type, metric, parse_levels(levels), bins, fixed_mask, init,
                grid_spacing, regularisation, initial)
    except (ValueError, TypeError) as e:
        raise typer.BadParameter(str(e))
    print(f"{transform_file}: {r.kind}, {r.metric} {r.value:.6f}, {sum(r.evaluations)} evaluations over levels "
          f"{','.join(str(v) for v in r.levels)}, {'converged' if r.converged else 'iteration limit reached'}")


@app.command("apply")
def apply_command(
    moving: Path = typer.Argument(..., metavar="MOVING", help="image or label map to resample"),
    fixed: Path = typer.Argument(..., metavar="FIXED", help="image whose grid the result gets"),
    output: Path = typer.Argument(..., metavar="OUTPUT", help="file to write"),
    transform_file: Path = typer.Option(..., "--transform", help="file written by `fit`"),
    nearest: bool = typer.Option(False, "--nearest", help="nearest-neighbour interpolation"),
    interpolator: Optional[str] = typer.Option(None, "--interpolator", help=" | ".join(INTERPOLATORS)),
    sigma: Optional[float] = typer.Option(None, "--sigma", help="label-gaussian: sigma in voxels of MOVING (default 1)"),
    alpha: Optional[float] = typer.Option(None, "--alpha", help="label-gaussian: window radius in sigmas (default 2)"),
    save_jacobian: Optional[Path] = typer.Option(None, "--save-jacobian", help="bspline: file for the Jacobian determinant map"),
) -> None:
    try:
        result = apply(moving, fixed, output, transform_file, nearest, interpolator, sigma, alpha, save_jacobian)
    except (ValueError, TypeError) as e:
        raise typer.BadParameter(str(e))
    print(f"{output}: {moving.name} on the grid of {fixed.name} through {transform_file.name}, size {result.GetSize()}, "
          f"{interpolator or ('nearest' if nearest else 'linear')}")


if __name__ == "__main__":
    app()
