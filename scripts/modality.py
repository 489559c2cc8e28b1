"""MRI bias-field correction and CT intensity scaling of a directory of images on the MI355X.

    python scripts/modality.py n4 IMAGE_DIR OUT_DIR [--mask-dir DIR] [--shrink-factor 4] [--levels 4]
                                  [--iterations 50] [--write-log-field] [--input-glob '*.nii.gz']
    python scripts/modality.py ct-scale IMAGE_DIR OUT_DIR [--inverse] [--input-glob '*.nii.gz']

``n4`` runs segmantic_amd.image.modality.bias_correct on every image (with the mask of the same name
from --mask-dir, else the Otsu mask); --write-log-field also writes NAME_logfield next to each output.
``ct-scale`` runs scale_clamp_ct (or unscale_ct with --inverse).  Outputs are float32, have the input's
name and keep its affine.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import Optional

import numpy as np
import typer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd.data.imageio import read_image, write_image  # noqa: E402
from segmantic_amd.image import modality  # noqa: E402
from segmantic_amd.image.processing import Image  # noqa: E402

app = typer.Typer(add_completion=False)


def _images(image_dir: Path, input_glob: str):
    paths = sorted(p for p in image_dir.glob(input_glob) if p.is_file())
    if not paths:
        raise RuntimeError(f"no image in {image_dir} matches {input_glob!r}")
    return paths


def _log_field_name(name: str) -> str:
    for suffix in (".nii.gz", ".nii", ".nrrd", ".mha", ".mhd"):
        if name.endswith(suffix):
            return name[: -len(suffix)] + "_logfield" + suffix
    return name + "_logfield"


@app.command()
def n4(
    image_dir: Path = typer.Argument(..., help="directory of MR images"),
    out_dir: Path = typer.Argument(..., help="directory to write the corrected images to"),
    mask_dir: Optional[Path] = typer.Option(None, "--mask-dir", help="masks of the same names (label 1)"),
    shrink_factor: int = typer.Option(4, "--shrink-factor", help="shrink factor along every axis"),
    levels: int = typer.Option(4, "--levels", help="number of fitting levels"),
    iterations: int = typer.Option(50, "--iterations", help="maximum iterations per level"),
    write_log_field: bool = typer.Option(False, "--write-log-field", help="also write NAME_logfield"),
    input_glob: str = typer.Option("*.nii.gz", "--input-glob", help="glob of the images in IMAGE_DIR"),
) -> None:
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = _images(image_dir, input_glob)
    for p in paths:
        arr, affine = read_image(p)
        img = Image(np.asarray(arr, np.float32))
        mask = None
        if mask_dir is not None:
            marr, _ = read_image(mask_dir / p.name)
            mask = Image(np.asarray(marr))
        if write_log_field:
            # the same steps as bias_correct, keeping the filter to read its field
            corrected, field = _n4_with_field(img, mask, shrink_factor, levels, iterations)
            write_image(out_dir / _log_field_name(p.name), field, affine)
        else:
            corrected = modality.bias_correct(img, mask, shrink_factor, levels, iterations).numpy()
        write_image(out_dir / p.name, corrected, affine)
    print(f"{len(paths)} images bias-corrected into {out_dir}")


def _n4_with_field(img: Image, mask, shrink_factor: int, levels: int, iterations: int):
    if mask is None:
        mask = modality.otsu_threshold(img, 0, 1, 200)
    small = modality.shrink(img, shrink_factor)
    small_mask = modality.shrink(mask, shrink_factor)
    corrector = modality.N4BiasFieldCorrectionImageFilter()
    corrector.SetMaximumNumberOfIterations([iterations] * levels)
    corrector.Execute(small, small_mask)
    field = corrector.GetLogBiasFieldAsImage(img).numpy()
    return img.numpy() / np.exp(field), field


@app.command("ct-scale")
def ct_scale(
    image_dir: Path = typer.Argument(..., help="directory of CT images"),
    out_dir: Path = typer.Argument(..., help="directory to write the scaled images to"),
    inverse: bool = typer.Option(False, "--inverse", help="undo the scaling (unscale_ct)"),
    input_glob: str = typer.Option("*.nii.gz", "--input-glob", help="glob of the images in IMAGE_DIR"),
) -> None:
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = _images(image_dir, input_glob)
    fn = modality.unscale_ct if inverse else modality.scale_clamp_ct
    for p in paths:
        arr, affine = read_image(p)
        write_image(out_dir / p.name, fn(Image(np.asarray(arr))).numpy(), affine)
    print(f"{len(paths)} images {'unscaled' if inverse else 'scaled'} into {out_dir}")


if __name__ == "__main__":
    app()
