"""Score predicted segmentations against references, one CSV row per (case, label).

    python scripts/evaluate_segmentations.py INPUT_DIR REFERENCE_DIR OUTPUT.csv [--input-glob '*.nii.gz']
                                             [--labels 1,2,3]

Files are paired by name.  Per label: Dice, false-negative error |R \\ S| / |R| and false-positive error
|S \\ R| / |S| (ITK LabelOverlapMeasures), Hausdorff and average Hausdorff (ITK HausdorffDistance), the
95th-percentile Hausdorff (MONAI) and the mean surface distance -- all on the MI355X
(segmantic_amd.seg.evaluation).  Spacing per array axis comes from the affine's column norms.
"""
from __future__ import annotations

import csv
import sys
from pathlib import Path
from typing import List, Optional

import numpy as np
import typer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from segmantic_amd.data.imageio import read_image, strip_image_suffix  # noqa: E402
from segmantic_amd.seg.evaluation import confusion_matrix, surface_distances  # noqa: E402

COLUMNS = ["case", "label", "dice", "false_negative_error", "false_positive_error", "hausdorff",
           "average_hausdorff", "hd95", "surface_mean"]


def spacing_zyx(affine: np.ndarray) -> List[float]:
    """voxel size per array axis [z, y, x] from a voxel (x, y, z) -> world affine"""
    cols = np.linalg.norm(np.asarray(affine, np.float64)[:3, :3], axis=0)
    return [float(v) for v in cols[::-1]]


def _ratio(a: float, b: float) -> float:
    return a / b if b > 0 else float("nan")


def evaluate(input_dir: Path, reference_dir: Path, output_file: Path, input_glob: str = "*.nii.gz",
             labels: Optional[str] = None) -> List[dict]:
    refs = {strip_image_suffix(p.name): p for p in sorted(reference_dir.iterdir()) if p.is_file()}
    pairs = [(p, refs[strip_image_suffix(p.name)]) for p in sorted(input_dir.glob(input_glob))
             if strip_image_suffix(p.name) in refs]
    if not pairs:
        raise RuntimeError(f"no prediction in {input_dir} matching {input_glob!r} has a reference in {reference_dir}")
    wanted = [int(v) for v in labels.split(",")] if labels else None
    rows = []
    for pred_path, ref_path in pairs:
        pred, affine = read_image(pred_path)
        ref, _ = read_image(ref_path)
        pred = np.asarray(pred).astype(np.int32)
        ref = np.asarray(ref).astype(np.int32)
        k = int(max(pred.max(), ref.max(), max(wanted) if wanted else 0)) + 1
        m = surface_distances(pred, ref, num_classes=k, spacing=spacing_zyx(affine)[-pred.ndim:], percentile=95.0)
        cm = confusion_matrix(k, pred, ref)
        for c in (wanted if wanted else [c for c in range(1, k) if m["n_pred"][c] > 0 or m["n_ref"][c] > 0]):
            inter, n_s, n_r = cm[c, c], m["n_pred"][c], m["n_ref"][c]
            rows.append({
                "case": strip_image_suffix(pred_path.name), "label": c,
                "dice": _ratio(2.0 * inter, n_s + n_r),
                "false_negative_error": _ratio(n_r - inter, n_r),
                "false_positive_error": _ratio(n_s - inter, n_s),
                "hausdorff": m["hausdorff"][c], "average_hausdorff": m["average_hausdorff"][c],
                "hd95": m["percentile_hausdorff"][c], "surface_mean": m["surface_mean"][c],
            })
    output_file.parent.mkdir(parents=True, exist_ok=True)
    with open(output_file, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=COLUMNS)
        wr.writeheader()
        wr.writerows(rows)
    return rows


def main(
    input_dir: Path = typer.Argument(..., help="directory of predicted label maps"),
    reference_dir: Path = typer.Argument(..., help="directory of reference label maps (same file names)"),
    output_file: Path = typer.Argument(..., help="CSV file to write"),
    input_glob: str = typer.Option("*.nii.gz", "--input-glob", help="glob of the predictions in INPUT_DIR"),
    labels: Optional[str] = typer.Option(None, "--labels", help="comma-separated label ids (default: all present)"),
) -> None:
    evaluate(input_dir, reference_dir, output_file, input_glob, labels)


if __name__ == "__main__":
    typer.run(main)
