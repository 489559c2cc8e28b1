"""Vertebra landmarks of a directory of volumes on the MI355X.

    python scripts/vert_landmarks.py heatmap LABEL_DIR OUT_DIR --tissue-list labels.txt [--gamma 1000]
                                             [--smooth-3d] [--input-glob '*.nii.gz']
    python scripts/vert_landmarks.py extract HEATMAP_DIR OUT_DIR [--threshold 0.5] [--tissue-list labels.txt]
                                             [--input-glob '*.nii.gz']

``heatmap`` turns every vertebra label volume into a 4-D f32 heatmap [K + 1, z, y, x] NIfTI of the same name
(VertHeatMap; K from the tissue list).  ``extract`` writes one landmark JSON per heatmap, ``<stem>_landmarks
.json`` (ExtractVertPosition + SaveVert): world-space (RAS mm) points named by channel id, or by the tissue
list's names when one is given.
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

from segmantic_amd.data.imageio import read_image  # noqa: E402
from segmantic_amd.data.nifti import write_nifti  # noqa: E402
from segmantic_amd.detect.transforms import ExtractVertPosition, SaveVert, VertHeatMap  # noqa: E402
from segmantic_amd.image.labels import load_tissue_list  # noqa: E402

app = typer.Typer(add_completion=False)


def _images(image_dir: Path, input_glob: str):
    paths = sorted(p for p in image_dir.glob(input_glob) if p.is_file())
    if not paths:
        raise RuntimeError(f"no image in {image_dir} matches {input_glob!r}")
    return paths


def _label_names(tissue_list: Path):
    """names of labels 1 .. K, K the largest id of the tissue list"""
    ids = {i: n for n, i in load_tissue_list(tissue_list).items() if i != 0}
    return [ids.get(i, str(i)) for i in range(1, max(ids, default=0) + 1)]


def _nifti_name(p: Path) -> str:
    name = p.name
    for ext in (".nii.gz", ".nii", ".mha", ".mhd", ".nrrd", ".nhdr"):
        if name.endswith(ext):
            return name[: -len(ext)] + ".nii.gz"
    return name + ".nii.gz"


@app.command()
def heatmap(
    label_dir: Path = typer.Argument(..., help="directory of vertebra label volumes"),
    out_dir: Path = typer.Argument(..., help="directory to write the heatmaps to"),
    tissue_list: Path = typer.Option(..., "--tissue-list", help="iSEG tissue list naming labels 1 .. K"),
    gamma: float = typer.Option(1000.0, "--gamma", help="peak value of every heatmap channel"),
    smooth_3d: bool = typer.Option(False, "--smooth-3d", help="smooth along x too (isotropic heatmaps)"),
    input_glob: str = typer.Option("*.nii.gz", "--input-glob", help="glob of the label volumes in LABEL_DIR"),
) -> None:
    names = _label_names(tissue_list)
    tr = VertHeatMap(keys="label", gamma=gamma, label_names=names, smooth_3d=smooth_3d)
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = _images(label_dir, input_glob)
    for p in paths:
        arr, affine = read_image(p)
        heat = tr({"label": arr})["label"]
        write_nifti(out_dir / _nifti_name(p), heat.cpu().numpy(), affine)
    print(f"{len(paths)} heatmaps of {len(names) + 1} channels written to {out_dir}")


@app.command()
def extract(
    heatmap_dir: Path = typer.Argument(..., help="directory of [K + 1, z, y, x] heatmaps"),
    out_dir: Path = typer.Argument(..., help="directory to write the landmark JSON files to"),
    threshold: float = typer.Option(0.5, "--threshold", help="channels whose max is below it have no landmark"),
    tissue_list: Optional[Path] = typer.Option(None, "--tissue-list", help="name the landmarks by this list"),
    input_glob: str = typer.Option("*.nii.gz", "--input-glob", help="glob of the heatmaps in HEATMAP_DIR"),
) -> None:
    id_map = None
    if tissue_list is not None:
        id_map = {n: i for i, n in enumerate(_label_names(tissue_list), start=1)}
    ex = ExtractVertPosition(keys="vert", threshold=threshold)
    save = SaveVert(keys="vert", output_dir=out_dir, output_postfix="landmarks", separate_folder=False,
                    print_log=False)
    paths = _images(heatmap_dir, input_glob)
    found = 0
    for p in paths:
        arr, affine = read_image(p)
        if np.ndim(arr) != 4:
            raise ValueError(f"{p}: a heatmap is a 4-D [K + 1, z, y, x] image, got shape {np.shape(arr)}")
        meta = {"affine": affine, "filename_or_obj": str(p)}
        d = ex({"vert": np.asarray(arr, dtype=np.float32), "vert_meta_dict": meta})
        if id_map is not None:
            d["vert_meta_dict"] = {**meta, "id_map": {n: i for n, i in id_map.items() if i in d["vert"]}}
        save(d)
        found += len(d["vert"])
    print(f"{found} landmarks of {len(paths)} heatmaps written to {out_dir}")


if __name__ == "__main__":
    app()
