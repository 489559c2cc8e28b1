"""Segment a target image by multi-atlas label propagation on the MI355X.

    python scripts/multi_atlas_segment.py TARGET OUTPUT --atlas IMAGE LABELS [--atlas IMAGE LABELS ...]
                                [--tissue-list F] [--grid-spacing MM]
                                [--fusion staple|patch] [--patch-radius R] [--search-radius R] [--beta B]

Per atlas: the affine registration of IMAGE onto TARGET by mutual information, the B-spline registration on top of
it (segmantic_amd.image.registration, DESIGN.md sections 23 and 24), and LABELS carried onto TARGET's grid through the
transform with nearest-neighbour interpolation.  The warped label maps are fused by STAPLE (segmantic_amd.seg.staple);
OUTPUT gets the fused labels and ``staple_performance.csv`` next to it the sensitivity and positive predictive value
of every atlas per tissue.  With ``--fusion patch`` every atlas IMAGE is carried onto TARGET's grid as well (linear
interpolation) and the label maps are fused by patch-based label fusion (segmantic_amd.seg.patch_fusion, DESIGN.md
section 25), which weighs every atlas voxel by voxel by how well its image fits TARGET's; ``<output stem>_confidence.nii.gz``
next to OUTPUT gets the winner's share of the votes and no ``staple_performance.csv`` is written.  TARGET, IMAGE,
LABELS and OUTPUT are NIfTI / MetaImage / NRRD files, 2-D or 3-D.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import typer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd.image import processing, registration  # noqa: E402

app = typer.Typer(add_completion=False, help=__doc__)


def pair_up(values: Sequence[Path]) -> List[Tuple[Path, Path]]:
    """--atlas takes two files each time it is given: [IMAGE, LABELS, IMAGE, LABELS, ...] -> pairs"""
    values = list(values)
    if not values or len(values) % 2:
        raise ValueError(f"--atlas takes an IMAGE and a LABELS file each time it is given, got {len(values)} file(s)")
    return [(values[k], values[k + 1]) for k in range(0, len(values), 2)]


def segment(target: Path, output: Path, atlases: Sequence[Tuple[Path, Path]], tissue_list: Optional[Path] = None,
            grid_spacing: float = 16.0, levels=(4, 2, 1), max_iterations: int = 60, keep_affine: bool = False,
            fusion: str = "staple", patch_radius=1, search_radius=2, beta: float = 1.0) -> dict:
    """Run the pipeline on files; returns {"labels": the fused Image, "staple": the StapleResult (``fusion="staple"``),
    "results": the DeformableResult per atlas, "affine_labels": per atlas its labels under the affine transform alone
    (numpy, only with ``keep_affine``)}; with ``fusion="patch"`` "patch" holds the PatchFusionResult, "warped_labels"
    and "warped_images" what was fused and "confidence_path" the file the confidence went to."""
    from segmantic_amd.seg import staple as S
    if fusion not in ("staple", "patch"):
        raise ValueError(f"fusion must be staple or patch, got {fusion!r}")
    atlases = list(atlases)
    if not 1 <= len(atlases) <= S.MAX_RATERS:
        raise ValueError(f"1 .. {S.MAX_RATERS} atlases, got {len(atlases)}")
    tissues = None
    if tissue_list is not None:
        from segmantic_amd.image.labels import load_tissue_list
        tissues = load_tissue_list(tissue_list)
    num_classes = max(max(tissues.values()) + 1, 2) if tissues else None
    fixed = processing.read_image(target)
    warped, warped_images, results, affine_labels = [], [], [], []
    for image_path, labels_path in atlases:
        moving, labels = processing.read_image(image_path), processing.read_image(labels_path)
        if labels.GetSize() != moving.GetSize():
            raise ValueError(f"{labels_path} has size {labels.GetSize()}, {image_path} has {moving.GetSize()}")
        labels.CopyInformation(moving)
        affine = registration.register(fixed, moving, transform="affine", levels=levels, initial="geometry")
        result = registration.register_deformable(fixed, moving, initial=affine.transform, grid_spacing=grid_spacing,
                                                  levels=levels, max_iterations=max_iterations)
        warped.append(registration.warp(labels, fixed, result, nearest=True))
        if fusion == "patch":
            warped_images.append(registration.warp(moving, fixed, result, nearest=False))
        results.append(result)
        if keep_affine:
            affine_labels.append(processing.apply_transform(labels, fixed, affine.transform, True).numpy())
    if fusion == "patch":
        return _fuse_by_patches(fixed, output, warped, warped_images, num_classes, patch_radius, search_radius, beta,
                                results, affine_labels)
    fused = S.staple([w.data for w in warped], num_classes)
    out = processing.Image(fused.labels, fixed.spacing, fixed.origin, fixed.direction)
    processing.write_image(out, output)
    S.write_performance_csv(S.performance_table(fused.sums, [p.name for p, _ in atlases], tissues),
                            Path(output).parent / "staple_performance.csv")
    return {"labels": out, "staple": fused, "results": results, "affine_labels": affine_labels}


def confidence_path(output: Path) -> Path:
    """<output stem>_confidence.nii.gz next to ``output`` (the stem ends at the first dot: seg.nii.gz -> seg)"""
    output = Path(output)
    return output.parent / (output.name.split(".")[0] + "_confidence.nii.gz")


def _fuse_by_patches(fixed, output, warped, warped_images, num_classes, patch_radius, search_radius, beta, results,
                     affine_labels) -> dict:
    from segmantic_amd.seg import patch_fusion as P
    fused = P.patch_fusion(fixed.data, [w.data for w in warped_images], [w.data for w in warped], num_classes,
                           patch_radius=patch_radius, search_radius=search_radius, beta=beta)
    out = processing.Image(fused.labels, fixed.spacing, fixed.origin, fixed.direction)
    processing.write_image(out, output)
    conf = confidence_path(output)
    processing.write_image(processing.Image(fused.confidence, fixed.spacing, fixed.origin, fixed.direction), conf)
    return {"labels": out, "patch": fused, "results": results, "affine_labels": affine_labels, "warped_labels": warped,
            "warped_images": warped_images, "confidence_path": conf}


@app.command()
def main(
    target: Path = typer.Argument(..., metavar="TARGET", help="image to segment"),
    output: Path = typer.Argument(..., metavar="OUTPUT", help="file to write the fused label map to"),
    atlas: List[Path] = typer.Option(..., "--atlas", metavar="IMAGE LABELS", help="an atlas image and its label map; repeat per atlas"),
    tissue_list: Optional[Path] = typer.Option(None, "--tissue-list", help="label names in iSEG format"),
    grid_spacing: float = typer.Option(16.0, "--grid-spacing", help="control spacing of the finest level in mm"),
    fusion: str = typer.Option("staple", "--fusion", help="staple (label maps alone) or patch (intensity-weighted)"),
    patch_radius: int = typer.Option(1, "--patch-radius", help="patch: radius of the compared patches in voxels, 0 .. 3"),
    search_radius: int = typer.Option(2, "--search-radius", help="patch: radius of the search window in voxels, 0 .. 3"),
    beta: float = typer.Option(1.0, "--beta", help="patch: smoothing of the weights, exp(-D / (beta * bandwidth))"),
) -> None:
    try:
        r = segment(target, output, pair_up(atlas), tissue_list, grid_spacing, fusion=fusion, patch_radius=patch_radius,
                    search_radius=search_radius, beta=beta)
    except (ValueError, TypeError) as e:
        raise typer.BadParameter(str(e))
    folded = sum(x.folded for x in r["results"])
    if fusion == "patch":
        print(f"{output}: {len(r['results'])} atlases fused by patch weights"
              f"{'' if folded == 0 else f', {folded} folded voxels'}; confidence in {r['confidence_path'].name}")
        return
    print(f"{output}: {len(r['results'])} atlases fused by STAPLE in {r['staple'].iterations} iterations"
          f"{'' if folded == 0 else f', {folded} folded voxels'}; staple_performance.csv next to it")


def cli(argv: Optional[Sequence[str]] = None):
    """``--atlas IMAGE LABELS`` takes two values: they are split into ``--atlas IMAGE --atlas LABELS`` for the parser"""
    argv = list(sys.argv[1:] if argv is None else argv)
    out, k = [], 0
    while k < len(argv):
        if argv[k] == "--atlas" and k + 2 < len(argv) and not argv[k + 2].startswith("--"):
            out += ["--atlas", argv[k + 1], "--atlas", argv[k + 2]]
            k += 3
        else:
            out.append(argv[k])
            k += 1
    return out


if __name__ == "__main__":
    app(args=cli())
