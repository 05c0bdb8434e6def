#!/usr/bin/env python3
"""Golden vectors for the image ingest (dawn_image_ingest), produced by the installed Pillow:
`Image.fromarray(a).resize((Wo, Ho), Image.BILINEAR)` -- what `transforms.Resize` does to a PIL image (UVG:320-325) -- on the inputs
that tests/ingest_cases.py makes from a formula.  Only the expected OUTPUT bytes are stored (at most 32 x 32 x 3 per array, and three
parts of the 256 x 256 case); the Pillow version that made them is stored beside them.

    python tools/gen_goldens_ingest.py   ->  tests/golden/image_ingest.npz
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ingest_cases import CASES, parts_of, source  # noqa: E402

out = {"pillow_version": np.array(PIL.__version__)}
for name, (Hs, Ws, Ho, Wo, _) in CASES.items():
    a = source(name)
    assert a.shape == (Hs, Ws, 3) and a.dtype == np.uint8
    got = np.array(Image.fromarray(a).resize((Wo, Ho), Image.BILINEAR))
    assert got.shape == (Ho, Wo, 3)
    out.update(parts_of(name, got))
path = os.path.join(ROOT, "tests", "golden", "image_ingest.npz")
np.savez_compressed(path, **out)
print(f"{path}: {len(out) - 1} arrays, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")
