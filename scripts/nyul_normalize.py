"""Nyul-Udupa intensity standardisation of a directory of images on the MI355X.

    python scripts/nyul_normalize.py fit IMAGE_DIR SCALE.json [--quantiles 0.01,0.1,...,0.99] [--nonzero]
                                         [--channel-wise] [--input-glob '*.nii.gz']
    python scripts/nyul_normalize.py apply IMAGE_DIR OUT_DIR --scale SCALE.json [--input-glob '*.nii.gz']

``fit`` learns a standard scale (segmantic_amd.seg.nyul_normalize.fit_standard_scale, landmarks mapped to
[0, 100] and averaged) and writes it with its quantiles and options; ``apply`` standardises every image
with it (NyulNormalize) and writes f32 images of the same names.  A 3-D volume is one channel; a 4-D
array is [C, z, y, x].
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import typer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd.data.imageio import read_image, write_image  # noqa: E402
from segmantic_amd.seg.nyul_normalize import NyulNormalize, fit_standard_scale  # noqa: E402

DEFAULT_QUANTILES = "0.01,0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9,0.99"
app = typer.Typer(add_completion=False)


def _images(image_dir: Path, input_glob: str):
    paths = sorted(p for p in image_dir.glob(input_glob) if p.is_file())
    if not paths:
        raise RuntimeError(f"no image in {image_dir} matches {input_glob!r}")
    return paths


def _channels_first(arr: np.ndarray) -> np.ndarray:
    a = np.asarray(arr, dtype=np.float32)
    return a[None] if a.ndim == 3 else a


@app.command()
def fit(
    image_dir: Path = typer.Argument(..., help="directory of training images"),
    scale_file: Path = typer.Argument(..., help="JSON file to write"),
    quantiles: str = typer.Option(DEFAULT_QUANTILES, "--quantiles", help="comma-separated quantiles in [0, 1]"),
    nonzero: bool = typer.Option(False, "--nonzero", help="landmarks of the nonzero voxels only"),
    channel_wise: bool = typer.Option(False, "--channel-wise", help="one set of landmarks per channel"),
    input_glob: str = typer.Option("*.nii.gz", "--input-glob", help="glob of the images in IMAGE_DIR"),
) -> None:
    q = np.sort(np.array([float(v) for v in quantiles.split(",")]), kind="stable")
    images = (_channels_first(read_image(p)[0]) for p in _images(image_dir, input_glob))
    scale, skipped = fit_standard_scale(images, q, nonzero=nonzero, channel_wise=channel_wise)
    scale_file.parent.mkdir(parents=True, exist_ok=True)
    scale_file.write_text(json.dumps({"quantiles": q.tolist(), "standard_scale": scale.tolist(),
                                      "nonzero": nonzero, "channel_wise": channel_wise}, indent=1))
    print(f"standard scale of {len(q)} landmarks written to {scale_file} ({skipped} segments skipped)")


@app.command()
def apply(
    image_dir: Path = typer.Argument(..., help="directory of images to standardise"),
    out_dir: Path = typer.Argument(..., help="directory to write the standardised images to"),
    scale: Path = typer.Option(..., "--scale", help="JSON file written by `fit`"),
    input_glob: str = typer.Option("*.nii.gz", "--input-glob", help="glob of the images in IMAGE_DIR"),
) -> None:
    cfg = json.loads(scale.read_text())
    tr = NyulNormalize(np.array(cfg["quantiles"]), np.array(cfg["standard_scale"]), nonzero=cfg["nonzero"],
                       channel_wise=cfg["channel_wise"])
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = _images(image_dir, input_glob)
    for p in paths:
        arr, affine = read_image(p)
        img = _channels_first(arr)
        tr(img)
        write_image(out_dir / p.name, img[0] if np.ndim(arr) == 3 else img, affine)
    print(f"{len(paths)} images standardised into {out_dir}")


if __name__ == "__main__":
    app()
