"""Fuse the label maps of atlases that already lie on the target's grid by patch-based label fusion on the MI355X.

    python scripts/patch_fuse_labels.py TARGET OUTPUT --atlas IMAGE LABELS [--atlas IMAGE LABELS ...]
                                        [--tissue-list F] [--patch-radius R] [--search-radius R] [--beta B]

Every atlas votes at every voxel of TARGET with a weight given by how well the patch of its IMAGE fits TARGET's
there, and from the neighbouring positions of the search window (segmantic_amd.seg.patch_fusion, DESIGN.md section
25).  IMAGE and LABELS must have TARGET's size, spacing, origin and direction; what differs is refused by name
(scripts/multi_atlas_segment.py --fusion patch registers the atlases first).  The number of classes is the tissue
list's when one is given (iSEG format), else the largest label + 1.  OUTPUT gets the fused labels with TARGET's
geometry; ``<output stem>_confidence.nii.gz`` next to it the winner's share of the votes.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import List, Optional

import typer

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "scripts"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

from multi_atlas_segment import cli, confidence_path, pair_up  # noqa: E402
from staple_labels import check_same_grid  # noqa: E402

app = typer.Typer(add_completion=False, help=__doc__)


def fuse(target: Path, output: Path, atlases, tissue_list: Optional[Path] = None, patch_radius=1, search_radius=2,
         beta: float = 1.0):
    """Run the fusion on files; returns the PatchFusionResult"""
    from segmantic_amd.image.labels import load_tissue_list
    from segmantic_amd.image.processing import Image, read_image, write_image
    from segmantic_amd.seg import patch_fusion as P

    atlases = list(atlases)
    if not 1 <= len(atlases) <= P.MAX_ATLASES:
        raise ValueError(f"1 .. {P.MAX_ATLASES} atlases, got {len(atlases)}")
    tissues = load_tissue_list(tissue_list) if tissue_list else None
    num_classes = max(max(tissues.values()) + 1, 2) if tissues else None
    fixed = read_image(target)
    images, labels = [], []
    for image_path, labels_path in atlases:
        for path, into in ((image_path, images), (labels_path, labels)):
            im = read_image(path)
            check_same_grid(fixed, im, target, path)
            into.append(im.data)
    res = P.patch_fusion(fixed.data, images, labels, num_classes, patch_radius=patch_radius, search_radius=search_radius,
                         beta=beta)
    output = Path(output)
    output.parent.mkdir(parents=True, exist_ok=True)
    write_image(Image(res.labels.cpu(), fixed.spacing, fixed.origin, fixed.direction), output)
    write_image(Image(res.confidence.cpu(), fixed.spacing, fixed.origin, fixed.direction), confidence_path(output))
    return res


@app.command()
def main(
    target: Path = typer.Argument(..., metavar="TARGET", help="image to segment"),
    output: Path = typer.Argument(..., metavar="OUTPUT", help="file to write the fused label map to"),
    atlas: List[Path] = typer.Option(..., "--atlas", metavar="IMAGE LABELS", help="an atlas image and its label map on TARGET's grid; repeat per atlas"),
    tissue_list: Optional[Path] = typer.Option(None, "--tissue-list", help="label names in iSEG format"),
    patch_radius: int = typer.Option(1, "--patch-radius", help="radius of the compared patches in voxels, 0 .. 3"),
    search_radius: int = typer.Option(2, "--search-radius", help="radius of the search window in voxels, 0 .. 3"),
    beta: float = typer.Option(1.0, "--beta", help="smoothing of the weights, exp(-D / (beta * bandwidth))"),
) -> None:
    try:
        pairs = pair_up(atlas)
        fuse(target, output, pairs, tissue_list, patch_radius, search_radius, beta)
    except (ValueError, TypeError) as e:
        raise typer.BadParameter(str(e))
    print(f"{output}: {len(pairs)} atlases fused by patch weights; confidence in {confidence_path(output).name}")


if __name__ == "__main__":
    app(args=cli())
