"""Map the labels of every NIfTI file of a directory (reference ``scripts/map_labels.py``) on the MI355X.

    python scripts/map_labels.py INPUT_DIR OUTPUT_DIR INPUT_TISSUES INPUT2OUTPUT

INPUT_TISSUES is an iSEG tissue list of the input labels and INPUT2OUTPUT a JSON file that maps every input
tissue name to an output tissue name, e.g. ``{"Background": "Background", "Skull": "Bone", "Mandible":
"Bone", "Fat": "Fat"}``.  The output tissues are numbered alphabetically after Background
(segmantic_amd.image.labels.build_tissue_mapping); their list is written to OUTPUT_DIR/labels.txt and every
file is mapped through segmantic_amd.seg.transforms.MapLabels, keeping its name, dtype and affine.

The reference script also carries three name mappings of one lab's 16-tissue head model, selectable by
name; they are that lab's data and are not reproduced: pass the mapping as a JSON file.
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
from segmantic_amd.image.labels import build_tissue_mapping, load_tissue_list, save_tissue_list  # noqa: E402
from segmantic_amd.seg.transforms import MapLabels  # noqa: E402


def main(
    input_dir: Path = typer.Argument(..., help="directory of *.nii.gz label maps"),
    output_dir: Path = typer.Argument(..., help="directory to write the mapped label maps to"),
    input_tissues: Path = typer.Argument(..., help="iSEG tissue list of the input labels"),
    input2output: Path = typer.Argument(..., help="JSON file: input tissue name -> output tissue name"),
) -> None:
    imap = load_tissue_list(input_tissues)
    if not input2output.exists():
        raise RuntimeError(f"{input2output}: the mapping is a JSON file of input name -> output name")
    i2omap = json.loads(input2output.read_text())
    missing = sorted(n for n in imap if n not in i2omap)
    if missing:
        raise RuntimeError(f"{input2output} maps no output tissue for {missing}")
    omap, i2o = build_tissue_mapping(imap, lambda n: i2omap[n])

    output_dir.mkdir(parents=True, exist_ok=True)
    save_tissue_list(omap, output_dir / "labels.txt")
    paths = sorted(input_dir.glob("*.nii.gz"))
    for p in paths:
        arr, affine = read_image(p)
        arr = np.ascontiguousarray(arr)
        if arr.dtype.kind not in "iu":
            raise RuntimeError(f"{p}: not a label map ({arr.dtype})")
        dtype = arr.dtype if arr.dtype in (np.uint8, np.int16, np.int32, np.int64) else np.int32
        mapper = MapLabels({i: int(o) for i, o in enumerate(i2o)}, out_dtype=np.dtype(dtype))
        write_image(output_dir / p.name, mapper(arr).astype(arr.dtype), affine)
    print(f"{len(paths)} label maps mapped into {output_dir}")


if __name__ == "__main__":
    typer.run(main)
