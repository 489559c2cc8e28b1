"""Extract one surface per tissue of a label volume on the MI355X and write each as a binary PLY.

    python scripts/visualize_label_surfaces.py FILE OUTPUT_DIR TISSUELIST [--selected-tissues 1 --selected-tissues 4]
                                               [--smooth N] [--relaxation F] [--decimate R]

The reference's script of the same name and argument order.  FILE is read through data/imageio.py (NIfTI,
MetaImage, NRRD); TISSUELIST is an iSEG tissue list (it may be missing: files are then called label_NNN.ply).
Meshes are discrete surface nets (segmantic_amd.image.surfaces), in the RAS millimetre frame of the file's affine.
--decimate R in (0, 1) decimates every mesh towards (1 - R) of its triangles by topology-preserving edge collapses;
the default 0 leaves them as extracted, 0.8 is the reference's vtkDecimatePro setting.  The default selection is every label present; a selected label that is absent writes no file.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import typer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd.data.imageio import read_image  # noqa: E402
from segmantic_amd.image.labels import load_tissue_list  # noqa: E402
from segmantic_amd.image.surfaces import extract_surfaces as _extract, surface_file_name, write_ply  # noqa: E402


def affine_geometry(affine: np.ndarray):
    """voxel (x, y, z) -> mm affine as (spacing, origin, direction row-major)"""
    A = np.asarray(affine, np.float64)
    sp = np.sqrt((A[:3, :3] ** 2).sum(0))
    sp[sp == 0] = 1.0
    return sp, A[:3, 3].copy(), (A[:3, :3] / sp).reshape(-1)


def extract_surfaces(
    file_path: Path = typer.Argument(..., help="label volume (.nii / .nii.gz / .mha / .mhd / .nrrd)"),
    output_dir: Path = typer.Argument(..., help="directory the PLY files are written to"),
    tissuelist_path: Path = typer.Argument(..., help="iSEG tissue list naming the labels (may be missing)"),
    selected_tissues: Optional[List[int]] = typer.Option(None, "--selected-tissues", help="labels to extract (default: all present)"),
    smooth: int = typer.Option(0, "--smooth", help="relaxation sweeps"),
    relaxation: float = typer.Option(0.5, "--relaxation", help="relaxation factor in [0, 1]"),
    decimate: float = typer.Option(0.0, "--decimate", help="share of the triangles to remove, in [0, 1); 0 = off, "
                                                           "--decimate 0.8 is the reference's setting"),
) -> None:
    arr, affine = read_image(file_path)
    tissues: Dict[int, str] = {}
    if tissuelist_path.exists():
        tissues = {i: name for name, i in load_tissue_list(tissuelist_path).items()}
    spacing, origin, direction = affine_geometry(affine)
    surfaces = _extract(np.ascontiguousarray(arr), selected_tissues or None, spacing, origin, direction, smooth,
                        relaxation, decimate)
    output_dir.mkdir(parents=True, exist_ok=True)
    for label, surf in surfaces.items():
        name = surface_file_name(label, tissues)
        print(f"Processing label {label:3d} : {name[:-4]}")
        if surf.faces.shape[0] == 0:
            print("    absent: no file")
            continue
        write_ply(output_dir / name, surf)
        print(f"    {surf.vertices.shape[0]} vertices, {surf.faces.shape[0]} faces, area {surf.area:.6g}, "
              f"volume {surf.volume:.6g}")


if __name__ == "__main__":
    typer.run(extract_surfaces)
