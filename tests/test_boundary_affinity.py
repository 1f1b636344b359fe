"""Boundary-path ops without a device: the path tables of the library against the definition, the oracle of
tests/boundary_affinity_oracle.py against plain loops, torch autograd and PSA's dense matrix power, and the host-side refusals."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affinity_oracle as ao  # noqa: E402
import boundary_affinity_oracle as bo  # noqa: E402

# radius: (offsets, total path points, longest path)
TABLE = {2: (4, 12, 4), 3: (12, 56, 7), 4: (22, 128, 8), 5: (34, 242, 11), 6: (54, 464, 13), 7: (72, 714, 16), 8: (96, 1078, 16)}


def brute_force_path(dy, dx):
    """Point by point over a generous box: inside the rectangle between the ends and closer than 1 to the line."""
    out = []
    for y in range(-9, 10):
        for x in range(-9, 10):
            if not (0 <= y <= dy and min(0, dx) <= x <= max(0, dx)):
                continue
            if (dy * x - dx * y) ** 2 < dy * dy + dx * dx:
                out.append((y, x))
    return out


def test_path_tables_of_the_oracle():
    for r, (P, total, longest) in TABLE.items():
        offs, pts = ao.offsets(r), bo.paths(r)
        assert len(offs) == len(pts) == P
        assert sum(len(p) for p in pts) == total and max(len(p) for p in pts) == longest and min(len(p) for p in pts) == 2
        for (dy, dx), path in zip(offs, pts):
            assert path == brute_force_path(dy, dx) and path == sorted(path) and len(set(path)) == len(path)
            assert (0, 0) in path and (dy, dx) in path
            assert {y for y, _ in path} == set(range(dy + 1))                               # every row between the ends
            assert {x for _, x in path} == set(range(min(0, dx), max(0, dx) + 1))           # and every column
    assert bo.paths(2)[1] == [(0, -1), (0, 0), (1, -1), (1, 0)]                             # S_(1,-1)
    assert bo.paths(3)[ao.offsets(3).index((2, 1))] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]


def test_library_path_tables_equal_the_oracle():
    """wsdl_path_affinity_paths through ctypes and ops.affinity_paths, radius 2..8; 0 / WsdlError outside."""
    import weaklysuperviseddl_amd
    from weaklysuperviseddl_amd import ops
    lib = weaklysuperviseddl_amd.lib()
    for r, (P, total, _) in TABLE.items():
        assert lib.wsdl_path_affinity_paths(r, None, None) == total
        lengths, points = (ctypes.c_int * P)(), (ctypes.c_int * (2 * total))()
        assert lib.wsdl_path_affinity_paths(r, lengths, points) == total
        want = bo.paths(r)
        assert list(lengths) == [len(p) for p in want]
        flat = [v for path in want for point in path for v in point]
        assert list(points) == flat
        assert ops.affinity_paths(r) == want
    for bad in (1, 9, 0, -3):
        assert lib.wsdl_path_affinity_paths(bad, None, None) == 0
    for bad in (1, 9, 5.0, True, None):
        with pytest.raises(ops.WsdlError):
            ops.affinity_paths(bad)
    assert lib.wsdl_path_affinity_workspace(2, 16, 16, 5) > 0
    for geom in ((0, 8, 8, 5), (1, 8, 8, 9), (1, 8, 8, 1), (1, 1025, 1024, 5), (1, 0, 8, 5)):
        assert lib.wsdl_path_affinity_workspace(*geom) == 0


def loop_affinity(edge, radius):
    B, h, w = edge.shape
    offs, pts = ao.offsets(radius), bo.paths(radius)
    aff = torch.zeros(B, len(offs), h, w, dtype=torch.float64)
    arg = torch.zeros(B, len(offs), h, w, dtype=torch.int64)
    for b in range(B):
        for j, (dy, dx) in enumerate(offs):
            for y in range(h):
                for x in range(w):
                    if not (0 <= y + dy < h and 0 <= x + dx < w):
                        continue
                    best, at = None, 0
                    for t, (sy, sx) in enumerate(pts[j]):
                        v = float(edge[b, y + sy, x + sx])
                        if best is None or v > best:
                            best, at = v, t
                    aff[b, j, y, x], arg[b, j, y, x] = 1.0 - best, at
    return aff, arg


@pytest.mark.parametrize("radius", (2, 3, 5))
@pytest.mark.parametrize("content", ("smooth", "quantised"))
def test_oracle_slices_equal_per_pixel_loops(radius, content):
    edge = bo.make_edge(2, 5, 7, 1, content)
    aff, arg = bo.affinity(edge, radius)
    want_aff, want_arg = loop_affinity(edge.double(), radius)
    assert torch.equal(aff, want_aff) and torch.equal(arg, want_arg)
    a32, arg32 = bo.affinity(edge, radius, dtype=torch.float32)
    assert a32.dtype == torch.float32 and torch.equal(arg32, arg)
    if content == "quantised":
        _, _, valid = bo.path_max(edge, radius)
        assert (aff[valid] == 0).any() and (aff[valid] == 1).any()           # valid pairs at exactly 0 and exactly 1


def test_nan_follows_torch_max():
    edge = bo.make_edge(1, 5, 7, 2)
    edge[0, 2, 3] = float("nan")
    edge[0, 2, 4] = float("nan")
    aff, arg = bo.affinity(edge, 3)
    pts, offs = bo.paths(3), ao.offsets(3)
    j = offs.index((0, 2))
    assert torch.isnan(aff[0, j, 2, 2]) and arg[0, j, 2, 2].item() == 1    # path (0,0),(0,1),(0,2): the FIRST NaN
    assert pts[j] == [(0, 0), (0, 1), (0, 2)] and not torch.isnan(aff[0, j, 0, 0])


def test_explicit_arg_max_gradient_equals_autograd_of_amax():
    edge = bo.make_edge(2, 6, 7, 3).double()                               # smooth: tie-free
    for radius in (2, 5):
        e = edge.clone().requires_grad_()
        offs, pts = ao.offsets(radius), bo.paths(radius)
        daff = torch.randn(2, len(offs), 6, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
        total = e.sum() * 0
        for j, (dy, dx) in enumerate(offs):
            win = ao.window(6, 7, dy, dx)
            if win is None:
                continue
            ys, xs, _, _ = win
            m = torch.stack([e[:, ys.start + y:ys.stop + y, xs.start + x:xs.stop + x] for y, x in pts[j]], dim=0).amax(dim=0)
            total = total + ((1 - m) * daff[:, j, ys, xs]).sum()
        total.backward()
        _, arg, valid = bo.path_max(edge, radius)
        got = bo.affinity_backward(daff, arg, valid, radius)
        # (two summation orders of at most 242 terms whose magnitudes sum to less than 10^3: 242 x 2^-53 x 10^3 < 1e-10)
        assert (got - e.grad).abs().max().item() < 1e-10 and e.grad.abs().max().item() > 0


@pytest.mark.parametrize("variant", ("all", "no_bg", "ignored"))
def test_loss_gradient_equals_autograd_of_the_float64_loss(variant):
    logits = bo.make_logits(2, 6, 7, 5)
    labels = ao.make_labels(2, 6, 7, 6, variant)
    for radius in (2, 5):
        L, g = bo.loss(logits, labels, radius)
        want_L, want_g = bo.loss_autograd(logits, labels, radius)
        assert abs(L.item() - want_L.item()) < 1e-13 and (g - want_g).abs().max().item() < 1e-14
        assert torch.isfinite(L) and torch.isfinite(g).all()               # the +-40 logits stay finite
        if variant == "ignored":
            assert L.item() == 0.0 and not g.any()
        else:
            assert L.item() > 0 and g.abs().max().item() > 0
    L32, g32 = bo.loss(logits, labels, 5, dtype=torch.float32)
    assert L32.dtype == torch.float32 and g32.dtype == torch.float32


def test_stencil_walk_under_path_affinities_equals_the_dense_matrix_power():
    edge = bo.make_edge(1, 6, 7, 7)
    m = ao.make_scores(1, 2, 6, 7, 8)
    for radius, beta in ((5, 10.0), (2, 1.0), (8, 10.0)):
        aff, _ = bo.affinity(edge, radius)
        stencil = bo.edge_walk(edge, m, radius, beta, (16,))[16]
        dense = ao.dense_walk(aff, m.double() * (1 - edge.double())[:, None], beta, 16, radius)
        assert (stencil - dense).abs().max().item() < 1e-12


def test_a_full_height_column_of_one_cuts_every_pair_that_straddles_it():
    h, w, col = 7, 9, 4
    edge = torch.rand(1, h, w, generator=torch.Generator().manual_seed(9)) * 0.5
    edge[:, :, col] = 1.0
    for radius in (2, 5, 8):
        aff, _ = bo.affinity(edge, radius)
        _, _, valid = bo.path_max(edge, radius)
        for j, (dy, dx) in enumerate(ao.offsets(radius)):
            for x in range(w):
                lo, hi = min(x, x + dx), max(x, x + dx)
                straddles = lo <= col <= hi
                col_valid = valid[0, j, :, x]
                if straddles:
                    assert not aff[0, j, :, x][col_valid].any(), (radius, dy, dx, x)
                else:
                    assert (aff[0, j, :, x][col_valid] > 0).all()
    # scores that are zero on one side stay exactly zero there
    m = torch.zeros(1, 1, h, w)
    m[..., :col] = 1.0
    out = bo.edge_walk(edge, m, 5, 10.0, (64,))[64]
    assert not out[..., col:].any() and out[..., :col].min().item() > 0


def test_refusals_on_the_host():
    from weaklysuperviseddl_amd import ops
    e, lab, m = torch.zeros(2, 6, 6), torch.zeros(2, 6, 6, dtype=torch.int64), torch.zeros(2, 3, 6, 6)
    assert ops.check_path_affinity_options(5, edge=e, labels=lab, scores=m, beta=10.0, num_iter=256) == 34
    assert ops.check_path_affinity_options(2, edge=e[:, None], scores=m, out=torch.empty(2, 3, 6, 6)) == 4
    for kw in (dict(radius=1), dict(radius=9), dict(radius=2.0), dict(beta=0.0), dict(beta=float("nan")), dict(num_iter=-1),
               dict(num_iter=1.5), dict(weights=(1, 2)), dict(weights=(1, 2, float("inf"))), dict(eps=0.0), dict(eps=float("nan")),
               dict(edge=torch.zeros(6, 6)), dict(edge=torch.zeros(2, 2, 6, 6)), dict(edge=torch.zeros(2, 1, 1, 6, 6)),
               dict(edge=e.double()), dict(edge=lab), dict(edge=torch.zeros(2, 0, 6)), dict(edge=torch.zeros(1, 1025, 1024)),
               dict(edge=[[0.0]]), dict(edge=e, labels=torch.zeros(2, 6, 7, dtype=torch.int64)), dict(edge=e, labels=torch.zeros(2, 6, 6)),
               dict(edge=e, labels=torch.zeros(1, 6, 6, dtype=torch.int64)), dict(edge=e, scores=torch.zeros(2, 3, 6, 7)),
               dict(edge=e, scores=torch.zeros(2, 33, 6, 6)), dict(edge=e, scores=torch.zeros(3, 2, 6, 6)),
               dict(edge=e, scores=m, out=m), dict(edge=e, scores=m, out=torch.empty(2, 3, 6, 6).double()),
               dict(edge=e, scores=m, out=torch.empty(2, 2, 6, 6)), dict(edge=e, scores=m, out=torch.empty(2, 3, 6, 12)[..., ::2])):
        kw.setdefault("radius", 5)
        radius = kw.pop("radius")
        with pytest.raises(ops.WsdlError):
            ops.check_path_affinity_options(radius, **kw)
    # out= that aliases the boundary map
    flat = torch.zeros(2 * 6 * 6)
    with pytest.raises(ops.WsdlError, match="shares memory with edge"):
        ops.check_path_affinity_options(5, edge=flat.view(2, 6, 6), scores=torch.zeros(2, 1, 6, 6), out=flat.view(2, 1, 6, 6))
    # host tensors never reach a kernel
    for call in (lambda: ops.path_affinity(e), lambda: ops.path_affinity_loss(e, lab), lambda: ops.edge_random_walk(e, m),
                 lambda: ops.path_affinity(e, 9), lambda: ops.path_affinity_loss(e, lab, eps=0.0),
                 lambda: ops.path_affinity_loss(e, lab, weights=(1, 2)), lambda: ops.edge_random_walk(e, m, beta=-1.0),
                 lambda: ops.edge_random_walk(e, m, num_iter=2.5), lambda: ops.edge_random_walk(e, torch.zeros(2, 3, 6, 5))):
        with pytest.raises(ops.WsdlError):
            call()


def test_modules_validate_on_the_host():
    from weaklysuperviseddl_amd import ops, nn as wnn
    crit, walk = wnn.PathAffinityLoss(), wnn.EdgeRandomWalk()
    assert (crit.radius, crit.ignore_index, crit.weights) == (5, 255, (0.25, 0.25, 0.5))
    assert (walk.radius, walk.beta, walk.num_iter) == (5, 10.0, 256)
    assert not isinstance(crit, wnn._Criterion) and not list(crit.parameters()) and not list(walk.parameters())
    for bad in (lambda: wnn.PathAffinityLoss(radius=1), lambda: wnn.PathAffinityLoss(weights=(1, 2)), lambda: wnn.EdgeRandomWalk(beta=0),
                lambda: wnn.EdgeRandomWalk(num_iter=-3), lambda: wnn.EdgeRandomWalk(radius=12)):
        with pytest.raises(ops.WsdlError):
            bad()


def test_generate_pseudo_masks_refuses_combinations():
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import generate_pseudo_masks
    assert inspect.signature(generate_pseudo_masks).parameters["boundary"].default is None
    for other in (dict(pamr={}), dict(superpixels={"step": 8}), dict(affinity={"net": object()})):
        with pytest.raises(ValueError):
            generate_pseudo_masks([], None, boundary={"net": object()}, **other)
    with pytest.raises(ValueError):
        generate_pseudo_masks([], None, boundary={"radius": 5})                      # no net
    with pytest.raises(ValueError):
        generate_pseudo_masks([], None, boundary={"net": object(), "steps": 3})     # an unknown key
    with pytest.raises(ops.WsdlError):
        generate_pseudo_masks([], None, boundary={"net": object(), "radius": 11})
    with pytest.raises(ops.WsdlError):
        generate_pseudo_masks([], None, boundary={"net": object(), "beta": 0.0})


def test_boundary_net_parameters_and_shapes():
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import BoundaryNet, FrozenResNetCAM, train_boundary_net
    net = BoundaryNet(FrozenResNetCAM(37))
    head = {k: tuple(p.shape) for k, p in net.named_parameters() if p.requires_grad}
    assert head == {"fc_edge1.weight": (32, 64, 1, 1), "fc_edge2.weight": (32, 256, 1, 1), "fc_edge3.weight": (32, 512, 1, 1),
                    "fc_edge4.weight": (32, 1024, 1, 1), "fc_edge5.weight": (32, 2048, 1, 1), "fc_edge6.weight": (1, 160, 1, 1),
                    "fc_edge6.bias": (1,)}
    assert all(k.startswith("trunk.") for k, p in net.named_parameters() if not p.requires_grad)
    assert len(net.head_parameters()) == 7 and not net.train().trunk.training and net.training
    cams = [torch.zeros(1, 8, 8)]
    for kw in (dict(epochs=0), dict(epochs=1.5), dict(lo=0.5, hi=0.5), dict(cams=3)):
        kw.setdefault("cams", cams)
        with pytest.raises(ValueError):
            train_boundary_net(net, [], log=None, **kw)
    with pytest.raises(ValueError):
        train_boundary_net(torch.nn.Linear(1, 1), [], cams, log=None)
    for kw in (dict(radius=9), dict(weights=(1, 2))):
        with pytest.raises(ops.WsdlError):
            train_boundary_net(net, [], cams, log=None, **kw)
    assert all(p.device.type == "cpu" for p in net.parameters())            # refused before anything moved
