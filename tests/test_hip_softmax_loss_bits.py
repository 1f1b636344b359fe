"""Bit-identity of the float64 softmax losses (csrc/boundary_loss.hip, csrc/overlap_loss.hip on csrc/softmax_item.h) with the
build they were refactored from: ops.boundary_loss, ops.overlap_sums, ops.tversky_loss and ops.focal_loss on the seeded cases
of tests/softmax_loss_bits.py must give exactly the uint32 / uint64 words of tests/golden/softmax_loss_bits.npz
(tests/golden/make_softmax_loss_bits.py) - no tolerance."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_loss_bits as S  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "softmax_loss_bits.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def compare(got, prefix):
    want = {k: v for k, v in golden().items() if k.startswith(prefix + "/")}
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    assert any(k.endswith("/grad") or k.endswith("/grad_sum") for k in got)
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        differ = int((got[k] != want[k]).sum())
        assert differ == 0, f"{k}: {differ} of {got[k].size} words differ from the recorded bits"


@pytest.mark.parametrize("C,layout", S.SMALL)
def test_small_cases_give_the_recorded_bits(dev, C, layout):
    compare(S.record_small(dev, C, layout), f"C{C}_{layout}")


@pytest.mark.parametrize("case", list(S.LARGE))
def test_large_cases_give_the_recorded_bits(dev, case):
    compare(S.record_large(dev, case), case)


def test_every_recorded_entry_belongs_to_a_case():
    prefixes = [f"C{C}_{layout}" for C, layout in S.SMALL] + list(S.LARGE)
    assert all(k.split("/")[0] in prefixes for k in golden())
    assert {k.split("/")[0] for k in golden()} == set(prefixes)
