"""Writes tests/golden/softmax_loss_bits.npz: the bit patterns of ops.boundary_loss, ops.overlap_sums, ops.tversky_loss and
ops.focal_loss - losses, sums and gradients - on the seeded cases of tests/softmax_loss_bits.py, taken on an MI355X with the
build of the commit BEFORE the four kernels moved onto csrc/softmax_item.h.  tests/test_hip_softmax_loss_bits.py requires
the same bits of every later build.  Run it again only where a change of the arithmetic is intended.

    python tests/golden/make_softmax_loss_bits.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import softmax_loss_bits as S  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("make_softmax_loss_bits: needs a GPU")
    dev = torch.device("cuda:0")
    out = {}
    for C, layout in S.SMALL:
        out.update(S.record_small(dev, C, layout))
    for case in S.LARGE:
        out.update(S.record_large(dev, case))
    path = os.path.join(HERE, "softmax_loss_bits.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
