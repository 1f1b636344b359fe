"""The oracle of seeded region growing against an independent formulation and on hand-made cases, the option refusals of the
new ops (raised before anything asks for a device) and the declarations of the new entry points.  No device."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srg_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGN = so.IGNORE


def scores_from_classes(cls, C, hot=0.9):
    """(1,C,H,W) float32 scores whose maximum, ``hot``, sits at class ``cls[y, x]``; -1 there: all classes equal 1/C."""
    cls = np.asarray(cls)
    s = np.full((1, C) + cls.shape, (1.0 - hot) / (C - 1), dtype=np.float32)
    for c in range(C):
        s[0, c][cls == c] = hot
    s[0][:, cls < 0] = 1.0 / C
    return s


@pytest.mark.parametrize("i", range(len(so.SHAPES)))
def test_grow_equals_per_class_propagation(i):
    scores, seeds, thresh, grown, counts, stats = so.case(i)
    g2, c2 = so.grow_by_propagation(scores, seeds, thresh)
    assert np.array_equal(grown, g2) and np.array_equal(counts, c2)
    B, C, H, W = so.SHAPES[i]
    assert counts.shape == (B, C) and counts.sum() == ((grown >= 0) & (grown < C)).sum()
    seeded = (seeds >= 0) & (seeds < C)
    assert np.array_equal(grown[seeded], seeds[seeded])
    pres = np.ones((B, C), dtype=bool)
    pres[:, C - 1] = False
    g3, c3 = so.grow(scores, seeds, thresh, present=pres)
    g4, c4 = so.grow_by_propagation(scores, seeds, thresh, present=pres)
    assert np.array_equal(g3, g4) and np.array_equal(c3, c4)


def test_a_seed_outside_every_candidate_region_grows_nothing():
    cls = np.array([[1, 1, 1, -1, -1, -1]])
    seeds = np.full((1, 1, 6), IGN)
    seeds[0, 0, 4] = 1
    grown, counts = so.grow(scores_from_classes(cls, 2), seeds, [0.5, 0.5])
    assert grown.tolist() == [[[IGN, IGN, IGN, IGN, 1, IGN]]] and counts.tolist() == [[0, 1]]


def test_a_foreign_seed_inside_a_region_is_kept_and_does_not_block_it():
    cls = np.array([[1, 1, 1, 1, 1]])
    seeds = np.array([[[1, IGN, 0, IGN, IGN]]])
    grown, counts = so.grow(scores_from_classes(cls, 2), seeds, [0.5, 0.5])
    assert grown.tolist() == [[[1, 1, 0, 1, 1]]] and counts.tolist() == [[1, 4]]


def test_a_seed_does_not_grow_a_touching_region_of_another_class():
    cls = np.array([[1, 1, 2, 2], [1, 1, 2, 2]])
    seeds = np.full((1, 2, 4), IGN)
    seeds[0, 0, 0] = 1
    seeds[0, 1, 3] = 1                                   # a seed of class 1 on the class-2 region: kept, grows nothing
    grown, counts = so.grow(scores_from_classes(cls, 3), seeds, [0.5] * 3)
    assert grown.tolist() == [[[1, 1, IGN, IGN], [1, 1, IGN, 1]]] and counts.tolist() == [[0, 5, 0]]


def test_diagonal_contact_joins_under_eight_connectivity_only():
    lab = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]])
    c8 = so.components(lab, background=0, connectivity=8)
    c4, a4 = so.components(lab, background=0, connectivity=4, want_area=True)
    assert c8.tolist() == [[[0, -1, -1], [-1, 0, -1], [-1, -1, 0]]]
    assert c4.tolist() == [[[0, -1, -1], [-1, 4, -1], [-1, -1, 8]]] and a4.max() == 1
    both = so.components(lab, connectivity=8)            # without a background the zeros form components too
    assert both.tolist() == [[[0, 1, 1], [1, 0, 1], [1, 1, 0]]]
    assert so.components(lab, connectivity=4).tolist() == [[[0, 1, 1], [3, 4, 1], [3, 3, 8]]]
    # growing is 8-connected
    seeds = np.full((1, 3, 3), IGN)
    seeds[0, 0, 0] = 1
    grown, _ = so.grow(scores_from_classes(np.where(lab[0] == 1, 1, -1), 2), seeds, [0.5, 0.5])
    assert grown.tolist() == [[[1, IGN, IGN], [IGN, 1, IGN], [IGN, IGN, 1]]]


def test_a_tie_takes_the_lower_class_and_present_removes_a_class():
    s = np.full((1, 3, 1, 2), 0.4, dtype=np.float32)
    s[0, 0] = 0.2                                        # classes 1 and 2 tie at 0.4
    assert so.candidates(s, [0.3] * 3).tolist() == [[[1, 1]]]
    assert so.candidates(s, [0.3] * 3, present=[[1, 0, 1]]).tolist() == [[[2, 2]]]
    assert so.candidates(s, [0.3] * 3, present=[[1, 0, 0]]).tolist() == [[[-1, -1]]]     # 0.2 is not > 0.3
    assert so.candidates(s, [0.3] * 3, present=[[0, 0, 0]]).tolist() == [[[-1, -1]]]
    assert so.candidates(s, [0.4] * 3).tolist() == [[[-1, -1]]]                            # strict


def test_a_nan_score_is_a_candidate_of_nothing():
    s = scores_from_classes(np.array([[1, 1, 1]]), 2)
    s[0, 0, 0, 1] = np.nan
    assert so.candidates(s, [0.5, 0.5]).tolist() == [[[1, -1, 1]]]
    assert so.candidates(s, [0.5, 0.5], present=[[0, 1]]).tolist() == [[[1, 1, 1]]]        # the NaN is of an absent class
    seeds = np.array([[[1, IGN, IGN]]])
    grown, _ = so.grow(s, seeds, [0.5, 0.5])
    assert grown.tolist() == [[[1, IGN, IGN]]]                                              # the NaN pixel cuts the region


def test_weights_and_the_empty_group():
    grown = np.array([[[0, 0, 1, 2, IGN, 2]], [[1, 1, 1, IGN, IGN, IGN]]])
    counts = np.array([[2, 1, 2], [0, 3, 0]])
    w = so.weights(grown, counts, "fg_bg")
    assert np.array_equal(w, np.array([[[1 / 4, 1 / 4, 1 / 6, 1 / 6, 0, 1 / 6]], [[1 / 6, 1 / 6, 1 / 6, 0, 0, 0]]]))
    w = so.weights(grown, counts, "class")
    assert np.array_equal(w, np.array([[[1 / 4, 1 / 4, 1 / 2, 1 / 4, 0, 1 / 4]], [[1 / 6, 1 / 6, 1 / 6, 0, 0, 0]]]))
    assert np.array_equal(so.weights(grown, counts, "none"), ((grown >= 0) & (grown < 3)).astype(float))
    # a group the counts call empty contributes nothing, whatever the labels say: 0, not a division by zero
    w = so.weights(np.array([[[0, 1]]]), np.array([[1, 0]]), "fg_bg")
    assert w.tolist() == [[[1.0, 0.0]]] and np.isfinite(w).all()


def test_option_refusals_need_no_device():
    from weaklysuperviseddl_amd import ops, nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import PsuedoMasks
    lab = torch.zeros(1, 4, 4, dtype=torch.int64)
    for conn in (6, 0, 8.0, True, "8"):
        with pytest.raises(ValueError):
            ops.label_components(lab, connectivity=conn)
    with pytest.raises(ValueError):
        ops.label_components(lab, background=0.5)
    with pytest.raises(ValueError):
        ops.check_components_geometry(2, 1 << 15, 1 << 15)
    with pytest.raises(ValueError):
        ops.check_components_geometry(1, 0, 4)
    ops.check_components_geometry(1, 1, 2 ** 31 - 1)
    with pytest.raises(ops.WsdlError):
        ops.label_components(lab)                        # a host tensor: there is no CPU fallback
    assert ops.srg_thresholds(0.5, 3) == [0.5] * 3
    assert ops.srg_thresholds((0.99, 0.85), 4) == [0.99, 0.85, 0.85, 0.85]
    assert ops.srg_thresholds([0.1, 0.2, 0.3], 3) == [0.1, 0.2, 0.3]
    for bad in ((0.1, 0.2, 0.3), "0.5", None, float("nan"), (0.5, True)):
        with pytest.raises(ValueError):
            ops.srg_thresholds(bad, 4)
    scores, seeds = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.seeded_region_growing(scores, seeds, "high")
    with pytest.raises(ValueError):
        ops.seeded_region_growing(scores, seeds, 0.5, ignore_index=2.5)
    with pytest.raises(ops.WsdlError):
        ops.seeded_region_growing(scores, seeds, 0.5)
    with pytest.raises(ValueError):
        ops.balanced_seed_weights(seeds, torch.zeros(1, 2, dtype=torch.int64), balance="pixel")
    with pytest.raises(ValueError):
        wnn.SeededRegionGrowingLoss(balance="both")
    with pytest.raises(ValueError):
        wnn.SeededRegionGrowingLoss(thresh="0.9")
    crit = wnn.SeededRegionGrowingLoss()
    assert crit.balance == "fg_bg" and crit.ignore_index == 255 and crit.thresh is None and crit.thresh_ptr == 0
    with pytest.raises(ValueError):
        crit.set_thresh((0.5, None))
    with pytest.raises(ValueError):
        PsuedoMasks.seeds_from_cam(torch.zeros(2, 2), 0.6, 0.4)


def test_seeds_from_cam():
    from weaklysuperviseddl_amd.TraditionalModel import PsuedoMasks
    cam = torch.tensor([[0.0, 0.05, 0.3, 0.6, 1.0, float("nan")]])
    assert PsuedoMasks.seeds_from_cam(cam, 0.05, 0.6).tolist() == [[0, 0, 255, 1, 1, 255]]
    s = PsuedoMasks.seeds_from_cam(cam, 0.05, 0.6, ignore_index=-100)
    assert s.dtype == torch.int64 and s.tolist() == [[0, 0, -100, 1, 1, -100]]


def test_the_new_entry_points_are_declared_and_bound():
    from weaklysuperviseddl_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "wsdl_hip.h")).read()
    for name in ("wsdl_label_components_workspace", "wsdl_label_components", "wsdl_seeded_region_growing_workspace",
                 "wsdl_seeded_region_growing", "wsdl_balanced_seed_weights"):
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "components_grid.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "weaklysuperviseddl_amd", "csrc", "components_grid.hip"))
