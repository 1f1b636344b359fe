"""Writes tests/golden/pil_resize.npz: Pillow's own ``Image.resize`` of the closed-form patterns of
tests/pil_resize_oracle.py - every (size, channels, filter) case as the sha256 of the output bytes, two small cases in full.
Made with Pillow 12.2.0 (recorded in the file), so a Pillow that resamples differently on another machine is noticed and
named by tests/test_pil_resize.py.

    python tests/golden/make_pil_resize_golden.py
"""
import hashlib
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pil_resize_oracle as O  # noqa: E402

FULL = {(2, 2, 3, O.BICUBIC), (1, 37, 1, O.BILINEAR)}


def case_name(h, w, c, filt):
    return f"{h}x{w}x{c}_{'bicubic' if filt == O.BICUBIC else 'bilinear'}"


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for h, w in O.SIZES:
        for c in (1, 3):
            img = O.pattern(h, w, c)
            for filt, size in O.TARGETS:
                res = np.asarray(Image.fromarray(img).resize((size[1], size[0]), filt))
                name = case_name(h, w, c, filt)
                out["sha256/" + name] = np.array(hashlib.sha256(res.tobytes()).hexdigest())
                if (h, w, c, filt) in FULL:
                    out["full/" + name] = res
    path = os.path.join(HERE, "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
