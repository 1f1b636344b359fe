"""The score-histogram kernels on the device (csrc/score_hist.hip) against the numpy oracle of tests/score_hist_oracle.py.

Counts, sums, curves, Otsu's k* / threshold / q and the masks are compared with ``torch.equal`` / ``np.array_equal``: there is no
tolerance in this file except the stated bound on the softmax confidence of ``confidence_histogram``.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_hist_oracle as O  # noqa: E402
from test_score_hist import NEIGHBOUR_TABLES, confidence_exempt, confidence_logits, edge_neighbours  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32

GEOMS = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 5, 7), (3, 37, 53), (2, 64, 64), (2, 96, 130), (1, 3, 300), (1, 256, 257)]
TABLES = [(1, 1), (1, 256), (2, 2), (2, 15), (2, 256), (3, 1024), (21, 15), (21, 192), (32, 125)]
_ids = lambda g: "x".join(map(str, g))  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(t, a):
    """A device tensor equals a numpy array bit for bit."""
    want = torch.from_numpy(np.ascontiguousarray(a))
    got = t.detach().cpu()
    if got.dtype == torch.float32:
        got, want = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)


def _offset_view(t):
    """The same values as a dense view at a storage offset of one element (off every 16-byte boundary)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == 1
    return v


def _path(ops, who="score_hist"):
    """(pixels per lane, LDS copies) of the last histogram launch"""
    trace = ops.last_launches()
    assert trace.count(who + "<") == 1, trace
    part = trace[trace.index(who + "<"):]
    return int(part[len(who) + 1]), int(part.split("copies=")[1].split()[0])


def _mixed(rng, shape, lo=0.0, hi=1.0):
    """noise over a little more than the range, with every special value sprinkled in"""
    v = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), shape).astype(F)
    flat = v.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, lo, hi, np.nextafter(F(hi), F(-np.inf))], dtype=F)
    if flat.size >= 4 * special.size:
        flat[rng.choice(flat.size, special.size, replace=False)] = special
    return v


def _groups(rng, shape, G):
    g = rng.integers(0, G, shape).astype(np.int64)
    if g.size >= 16:
        g[rng.random(shape) < 0.1] = rng.choice(np.array([2 if G <= 2 else G, 255, -1, G], dtype=np.int64))
        g.reshape(-1)[:4] = [G, 255, -1, G - 1]
    return g


def _check_hist(ops, dev, v, g, edges, G, per_image, want_sums, edges_dev=None, **kw):
    res = ops.score_histogram(_d(v, dev), None if g is None else _d(g, dev), edges=edges_dev if edges_dev is not None else _d(edges, dev),
                              num_groups=G, per_image=per_image, want_sums=want_sums, **kw)
    want = O.histogram(v, g, edges, G, per_image, want_sums)
    if want_sums:
        assert _same(res[0], want[0]) and _same(res[1], want[1])
    else:
        assert _same(res, want)
    return res


# ------------------------------------------------------------------------------------------------------------------- histogram
@pytest.mark.parametrize("per_image", [True, False], ids=["per_image", "pooled"])
@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
def test_histogram_geometries_both_access_paths(dev, geom, per_image):
    from weaklysuperviseddl_amd import ops
    B, H, W = geom
    rng = np.random.default_rng(B * 1000 + H * 10 + W)
    edges = O.uniform_edges(0, 1, 256)
    v, g = _mixed(rng, geom), _groups(rng, geom, 2)
    ops.launch_trace(True)
    try:
        for want_sums in (False, True):
            _check_hist(ops, dev, v, g, edges, 2, per_image, want_sums)
            V, copies = _path(ops)
            assert V == (4 if H * W % 4 == 0 else 1) and copies == 4
        _check_hist(ops, dev, v, None, edges, 1, per_image, True)
    finally:
        ops.launch_trace(False)


@pytest.mark.parametrize("table", TABLES, ids=_ids)
def test_histogram_tables_both_lds_layouts_and_the_limits(dev, table):
    from weaklysuperviseddl_amd import ops
    G, nb = table
    rng = np.random.default_rng(G * 10000 + nb)
    edges = O.uniform_edges(-1.0, 3.0, nb)
    ops.launch_trace(True)
    try:
        for geom in ((2, 64, 64), (3, 37, 53)):
            v, g = _mixed(rng, geom, -1.0, 3.0), _groups(rng, geom, G)
            for want_sums in (False, True):
                _check_hist(ops, dev, v, g, edges, G, True, want_sums)
                assert _path(ops)[1] == (4 if G * (nb + 3) <= 1040 else 1)
    finally:
        ops.launch_trace(False)


@pytest.mark.parametrize("nb,lo,hi", NEIGHBOUR_TABLES)
def test_edges_and_their_float32_neighbours_land_where_the_comparisons_put_them(dev, nb, lo, hi):
    """Fails on a kernel that bins by floor((v - lo) * nb / (hi - lo)) (tests/test_score_hist.py shows the guess is off on these)."""
    from weaklysuperviseddl_amd import ops
    edges = O.uniform_edges(lo, hi, nb)
    pts = edge_neighbours(edges)
    rng = np.random.default_rng(nb)
    v = np.concatenate([pts, rng.uniform(lo, hi, 4 * 3200 - pts.size).astype(F)]).reshape(4, 40, 80)
    g = _groups(rng, v.shape, 2)
    for want_sums in (False, True):
        _check_hist(ops, dev, v, g, edges, 2, True, want_sums)
    _check_hist(ops, dev, v.reshape(4, 25, 128)[:, :, :127].copy(), None, edges, 1, False, True)     # the one-pixel path
    res = ops.score_histogram(_d(v, dev), bins=nb, range=(lo, hi))                              # the cached uniform edges
    assert _same(res, O.histogram(v, None, edges))


@pytest.mark.parametrize("content", ["quantised", "cam", "zeros", "last_edge", "specials", "outside", "log_edges"])
def test_histogram_contents(dev, content):
    from weaklysuperviseddl_amd import ops
    rng = np.random.default_rng(7)
    shape = (2, 64, 66)
    edges = O.uniform_edges(0, 1, 256)
    if content == "quantised":
        v = (rng.integers(0, 257, shape) / 256).astype(F)
    elif content == "cam":
        v = np.where(rng.random(shape) < 0.6, 0, rng.uniform(0, 1, shape) ** 2).astype(F)
        v[0, 0, 0] = 1.0
    elif content == "zeros":
        v = np.zeros(shape, dtype=F)
    elif content == "last_edge":
        v = np.full(shape, edges[-1], dtype=F)
    elif content == "specials":
        v = rng.choice(np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 0.5, 1e-45, -1e-45], dtype=F), shape)
    elif content == "outside":
        v = rng.choice(np.array([-7.0, 9.0, 1.0000001, -1e-9, 3e38, -3e38], dtype=F), shape)
    else:
        edges = np.concatenate([[0], np.logspace(-6, 0, 97)]).astype(F)
        v = (10 ** rng.uniform(-7, 0.1, shape)).astype(F)
        v.reshape(-1)[:98] = edges
    for g, G in ((None, 1), (_groups(rng, shape, 2), 2)):
        for want_sums in (False, True):
            for per_image in (True, False):
                _check_hist(ops, dev, v, g, edges, G, per_image, want_sums)
    res = _check_hist(ops, dev, v, None, edges, 1, True, False)
    if content == "zeros":
        assert res[:, 0, 1].tolist() == [64 * 66] * 2                    # -0.0 / 0.0: the bin that 0 opens
    if content == "last_edge":
        assert res[:, 0, -2].tolist() == [64 * 66] * 2


def test_histogram_behaviour_out_reuse_inputs_untouched_reproducible_strided(dev):
    from weaklysuperviseddl_amd import ops
    rng = np.random.default_rng(11)
    shape = (3, 40, 52)
    edges = O.uniform_edges(0, 1, 64)
    v, g = _mixed(rng, shape), _groups(rng, shape, 2)
    vd, gd, ed = _d(v, dev), _d(g, dev), _d(edges, dev)
    v0, g0, e0 = vd.clone(), gd.clone(), ed.clone()
    out = {}
    c1, s1 = ops.score_histogram(vd, gd, edges=ed, num_groups=2, want_sums=True, out=out)
    assert out["counts"] is c1 and out["sums"] is s1
    keep = (c1.clone(), s1.clone())
    c1.fill_(12345), s1.fill_(-7)                                           # stale contents must not survive
    c2, s2 = ops.score_histogram(vd, gd, edges=ed, num_groups=2, want_sums=True, out=out)
    assert c2 is c1 and s2 is s1 and torch.equal(c2, keep[0]) and torch.equal(s2, keep[1])
    assert torch.equal(vd.view(torch.int32), v0.view(torch.int32)) and torch.equal(gd, g0) and torch.equal(ed, e0)
    want = O.histogram(v, g, edges, 2, True, True)
    assert _same(c2, want[0]) and _same(s2, want[1])
    # strided scores and groups (made dense first), an odd storage offset (the one-pixel path)
    big_v, big_g = _d(np.repeat(v, 2, axis=2), dev), _d(np.repeat(g, 2, axis=2), dev)
    c3 = ops.score_histogram(big_v[:, :, ::2], big_g[:, :, ::2], edges=ed, num_groups=2)
    assert torch.equal(c3, keep[0])
    ops.launch_trace(True)
    try:
        c4, s4 = ops.score_histogram(_offset_view(vd), gd, edges=ed, num_groups=2, want_sums=True)
        assert _path(ops)[0] == 1
        c5 = ops.score_histogram(vd, _offset_view(gd), edges=ed, num_groups=2)
        assert _path(ops)[0] == 1
        ops.score_histogram(vd, gd, edges=ed, num_groups=2)
        assert _path(ops)[0] == 4
    finally:
        ops.launch_trace(False)
    assert torch.equal(c4, keep[0]) and torch.equal(s4, keep[1]) and torch.equal(c5, keep[0])
    from weaklysuperviseddl_amd import WsdlError
    with pytest.raises(WsdlError, match="shares memory"):
        ops.score_histogram(vd, gd, edges=ed, num_groups=2, out={"counts": gd.view(-1)[:3 * 2 * 67].view(3, 2, 67)})
    with pytest.raises(WsdlError, match="ascending"):
        ops.score_histogram(vd, edges=_d(np.array([0, 1, 1], dtype=F), dev))


# ---------------------------------------------------------------------------------------------------------------------- curves
@pytest.mark.parametrize("nb", [1, 15, 256, 1024])
def test_threshold_curves_against_the_oracle_and_against_thresholding_on_the_device(dev, nb):
    from weaklysuperviseddl_amd import ops
    rng = np.random.default_rng(nb)
    shape = (3, 37, 53)
    edges = O.uniform_edges(0, 1, nb)
    v = _mixed(rng, shape)
    v.reshape(-1)[100:100 + min(nb + 1, 500)] = edges[:500]
    gt = rng.integers(0, 3, shape).astype(np.int64)                         # a trimap: 2 is not counted
    vd, gd = _d(v, dev), _d(gt, dev)
    counts = ops.score_histogram(vd, gd, bins=nb, num_groups=2)
    cv = ops.threshold_curves(counts)
    assert cv.shape == (3, nb + 1, 4) and _same(cv, O.curves(O.histogram(v, gt, edges, 2)))
    ks = sorted(set([0, nb // 3, nb // 2, nb - 1, nb]))
    for k in ks:
        pred = vd >= float(edges[k])
        pos, neg = gd == 1, gd == 0
        want = torch.stack([(pred & pos).flatten(1).sum(1), (pred & neg).flatten(1).sum(1), (~pred & pos).flatten(1).sum(1),
                            (~pred & neg).flatten(1).sum(1)], dim=1)
        assert torch.equal(cv[:, k], want), k
    pooled = ops.threshold_curves(ops.score_histogram(vd, gd, bins=nb, num_groups=2, per_image=False))
    assert torch.equal(pooled[0], cv.sum(dim=0))
    buf = torch.full_like(cv, -1)
    assert ops.threshold_curves(counts, out=buf) is buf and torch.equal(buf, cv)


# ------------------------------------------------------------------------------------------------------------------------ Otsu
def _otsu_case(name, rng, nb):
    n = 4000
    if name == "bimodal":
        v = np.concatenate([rng.normal(0.25, 0.05, n // 2), rng.normal(0.7, 0.08, n // 2)])
    elif name == "unimodal":
        v = rng.normal(0.5, 0.1, n)
    elif name == "one_bin":
        v = np.full(n, 0.3)
    elif name == "two_bins":
        v = rng.choice([0.3, 0.3 + 1.0 / nb], n)
    else:                                                                    # plateau: empty bins between two modes
        v = rng.choice([0.1, 0.9], n)
    return np.clip(v, 0, 0.999).astype(F)


@pytest.mark.parametrize("nb", [2, 64, 256, 1024])
def test_otsu_bitwise_equal_to_the_oracle(dev, nb):
    from weaklysuperviseddl_amd import ops
    rng = np.random.default_rng(nb)
    names = ["bimodal", "unimodal", "one_bin", "two_bins", "plateau"]
    v = np.stack([_otsu_case(n, rng, nb) for n in names]).reshape(5, 40, 100)
    g = rng.integers(0, 3, v.shape).astype(np.int64)
    g[1, :20] = 2
    edges = O.uniform_edges(0, 1, nb)
    counts = ops.score_histogram(_d(v, dev), _d(g, dev), bins=nb, num_groups=3)
    ed = ops.uniform_edges(0, 1, nb, dev)
    host = O.histogram(v, g, edges, 3)
    for groups in (None, [0, 2], [1]):
        k, t, q = ops.otsu_threshold(counts, ed, groups=groups, fallback=0.25)
        wk, wt, wq = O.otsu(host, edges, groups, 0.25)
        assert _same(k, wk) and _same(t, wt), (groups, k.tolist(), wk.tolist())
        assert np.array_equal(q.cpu().numpy().view(np.int64), wq.view(np.int64)), groups
    wk = O.otsu(host, edges, None, 0.25)[0]
    assert wk[2] == -1                                                      # one occupied bin: the fallback
    if nb >= 64:
        lo_bin, hi_bin = int(O.slots(F(0.1), edges)) - 1, int(O.slots(F(0.9), edges)) - 1
        assert wk[4] == lo_bin and hi_bin - lo_bin > 2                      # the first maximum of the plateau
        assert wk[3] == int(O.slots(F(0.3), edges)) - 1


def test_otsu_refuses_large_segments(dev):
    from weaklysuperviseddl_amd import WsdlError, ops
    n = (1 << 21) + 1
    counts = ops.score_histogram(torch.zeros(1, n, device=dev), bins=16)
    assert counts[0, 0, 1].item() == n
    ed = ops.uniform_edges(0, 1, 16, dev)
    with pytest.raises(WsdlError, match="2\\^21"):
        ops.otsu_threshold(counts, ed)
    ok = ops.score_histogram(torch.zeros(2, 1 << 20, device=dev), bins=16, per_image=True)
    assert ops.otsu_threshold(ok, ed)[0].tolist() == [-1, -1]
    with pytest.raises(WsdlError, match="2\\^21"):
        ops.otsu_threshold(ops.score_histogram(torch.zeros(4, 1 << 20, device=dev), bins=16, per_image=False), ed)
    # counts whose size nobody vouched for: the device refuses by itself
    big = counts.clone()
    big[0, 0, 5] = 7
    k, t, q = ops.otsu_threshold(big, ed)
    assert k.tolist() == [-2] and torch.isnan(t).all() and torch.isnan(q).all()


# ------------------------------------------------------------------------------------------------------------------- threshold
@pytest.mark.parametrize("geom", [(1, 1, 1), (2, 5, 7), (3, 37, 53), (2, 64, 64), (1, 256, 257)], ids=_ids)
def test_threshold_per_image_both_rules_counts_and_nan(dev, geom):
    from weaklysuperviseddl_amd import ops
    B = geom[0]
    rng = np.random.default_rng(sum(geom))
    v = _mixed(rng, geom, -0.5, 1.0)
    t = rng.uniform(-0.3, 0.8, B).astype(F)
    t[0] = v.reshape(-1)[0] if np.isfinite(v.reshape(-1)[0]) else 0.0       # a value exactly at the threshold is kept
    vd, td = _d(v, dev), _d(t, dev)
    for positive_only in (True, False):
        m, c = ops.threshold_per_image(vd, td, positive_only=positive_only, want_count=True)
        want = O.threshold_images(v, t, positive_only)
        assert _same(m, want) and c.tolist() == want.reshape(B, -1).sum(axis=1).tolist()
        assert _same(ops.threshold_per_image(_offset_view(vd), td, positive_only=positive_only), want)
    assert _same(ops.threshold_per_image(vd, 0.3), O.threshold_images(v, np.full(B, 0.3, dtype=F), True))
    tn = t.copy()
    tn[-1] = np.nan
    m, c = ops.threshold_per_image(vd, _d(tn, dev), positive_only=False, want_count=True)
    assert not m[-1].any() and c[-1].item() == 0 and _same(m, O.threshold_images(v, tn, False))
    out = {"mask": torch.full(geom, 9, dtype=torch.uint8, device=dev), "count": torch.full((B,), 9, dtype=torch.int64, device=dev)}
    m2, c2 = ops.threshold_per_image(vd, _d(tn, dev), positive_only=False, want_count=True, out=out)
    assert m2 is out["mask"] and c2 is out["count"] and torch.equal(m2, m) and torch.equal(c2, c)


# ------------------------------------------------------------------------------------------------------------------ confidence
@pytest.mark.parametrize("C_,seed", [(2, 0), (3, 1), (21, 2), (64, 3)])
def test_confidence_histogram(dev, C_, seed):
    from weaklysuperviseddl_amd import ops
    z = confidence_logits(C_, seed)
    B, _, H, W = z.shape
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C_, (B, H, W)).astype(np.int64)
    y[rng.random(y.shape) < 0.5] = -100
    y[1, 0, :3] = 0                                                         # the non-finite pixels are counted: the NaN slot
    _, p64 = O.confidence_planes(z, np.float64)
    y = np.where((y != -100) & (rng.random(y.shape) < 0.6), p64, y)          # most of the rest is right
    conf = torch.empty(B, H, W, device=dev)
    pred = torch.empty(B, H, W, device=dev, dtype=torch.int64)
    edges = O.uniform_edges(0, 1, 15)
    for per_image in (False, True):
        counts, sums = ops.confidence_histogram(_d(z, dev), _d(y, dev), bins=15, per_image=per_image, conf_out=conf, pred_out=pred)
        cf, pr = conf.cpu().numpy(), pred.cpu().numpy()
        want = O.histogram(cf, O.confidence_groups(pr, y), edges, 2, per_image, True)
        assert _same(counts, want[0]) and _same(sums, want[1])
    assert counts.sum().item() == (y != -100).sum() and counts[1, :, -1].sum().item() == 3
    c64, p64 = O.confidence_planes(z, np.float64)
    c32, _ = O.confidence_planes(z, np.float32)
    fin = np.isfinite(c64)
    bound = np.maximum(4 * np.abs(c32.astype(np.float64) - c64), 2.0 ** -23 * np.abs(c64))
    err = np.abs(cf.astype(np.float64) - c64)
    print("confidence C=%d: max error %.3e, max bound %.3e, worst ratio %.3f" % (C_, err[fin].max(), bound[fin].max(),
                                                                                (err[fin] / bound[fin]).max()))
    assert (err[fin] <= bound[fin]).all() and np.isnan(cf[~fin]).all()
    exempt = confidence_exempt(z, bound)
    assert exempt[fin].mean() <= 1e-3
    assert np.array_equal(pr[fin & ~exempt], p64[fin & ~exempt])
    assert (cf[0, :2] == 1.0).all()                                         # a gap of 40: exactly 1, the slot above the last edge
    # the same table without the planes; an all-ignored batch
    c2, s2 = ops.confidence_histogram(_d(z, dev), _d(y, dev), bins=15, per_image=True)
    assert torch.equal(c2, counts) and torch.equal(s2, sums)
    c0, s0 = ops.confidence_histogram(_d(z, dev), _d(np.full_like(y, -100), dev), bins=15)
    assert not c0.any() and not s0.any()
    ece, acc, cfd, cnt = ops.ece_from_counts(counts, sums)
    o = O.ece(cf[y != -100], (pr == y)[y != -100], 15)
    assert ece == pytest.approx(o[0], abs=1e-12) and np.array_equal(cnt, o[3])


# ------------------------------------------------------------------------------------------------------------------ launch plan
def test_a_plan_holds_histogram_curves_otsu_and_threshold(dev):
    from weaklysuperviseddl_amd import ops, plan
    rng = np.random.default_rng(21)
    shape = (3, 48, 52)

    def contents():
        v = np.where(rng.random(shape) < 0.6, 0, rng.uniform(0, 1, shape)).astype(F)
        return v, rng.integers(0, 3, shape).astype(np.int64)
    a, b = contents(), contents()
    vd, gd = _d(a[0], dev), _d(a[1], dev)
    ed = ops.uniform_edges(0, 1, 256, dev)
    hist_out, thr_out = {}, {}
    cv_out = torch.empty(3, 257, 4, dtype=torch.int64, device=dev)

    def call(v, g, hist_out, cv_out, thr_out):
        counts, sums = ops.score_histogram(v, g, edges=ed, num_groups=2, want_sums=True, out=hist_out)
        cv = ops.threshold_curves(counts, out=cv_out)
        k, t, q = ops.otsu_threshold(counts, ed, fallback=0.3)
        m, n = ops.threshold_per_image(v, t, positive_only=True, want_count=True, out=thr_out)
        return counts, sums, cv, k, t, q, m, n
    p, got = plan.record(call, vd, gd, hist_out, cv_out, thr_out)
    assert p.stats["kernels"] == 4 and p.stats["memsets"] == 3

    def check(res, v, g):
        edges = O.uniform_edges(0, 1, 256)
        counts, sums = O.histogram(v, g, edges, 2, True, True)
        k, t, q = O.otsu(counts, edges, None, 0.3)
        mask = O.threshold_images(v, t, True)
        for have, want in zip(res, (counts, sums, O.curves(counts), k, t, q, mask, mask.reshape(3, -1).sum(axis=1).astype(np.int64))):
            assert _same(have, want) if have.dtype != torch.float64 else np.array_equal(have.cpu().numpy().view(np.int64), want.view(np.int64))
    check(got, *a)
    vd.copy_(_d(b[0], dev)), gd.copy_(_d(b[1], dev))
    for t in got:
        t.fill_(3)
    p.replay()
    check(got, *b)
    eager = call(_d(b[0], dev), _d(b[1], dev), None, None, None)
    for have, want in zip(got, eager):
        assert torch.equal(have.view(torch.int64) if have.dtype == torch.float64 else have.view(torch.int32) if have.dtype == torch.float32 else have,
                           want.view(torch.int64) if want.dtype == torch.float64 else want.view(torch.int32) if want.dtype == torch.float32 else want)


# ---------------------------------------------------------------------------------------------------------------------- callers
def _cam_generator(dev):
    from weaklysuperviseddl_amd.TraditionalModel import FrozenResNetCAM, LayerCAMGenerator
    torch.manual_seed(0)
    model = FrozenResNetCAM(37)
    g = torch.Generator().manual_seed(3)
    for mod in model.modules():
        if hasattr(mod, "running_mean"):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return LayerCAMGenerator(model.to(dev).eval(), ["layer3", "layer4"])


def _pet_loader(n_batches, B, S, seed, classes=37):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 3, S, S, generator=g), (torch.randint(0, classes, (B,), generator=g), torch.randint(1, 4, (B, 1, S, S), generator=g)))
            for _ in range(n_batches)]


def test_sweep_cam_thresholds_against_the_fixed_threshold_evaluation_and_the_oracle(dev):
    from weaklysuperviseddl_amd.TraditionalModel import evaluate_layercam_on_test_set, sweep_cam_thresholds
    gen = _cam_generator(dev)
    loader = _pet_loader(3, 2, 64, 5)
    th = np.array([0.05, 0.1, 0.2, 0.3, 0.45, 0.6, 0.8], dtype=F)
    out = sweep_cam_thresholds(gen, loader, 1.0, th, device=dev, log=None)
    k = int(np.argmin(np.abs(th.astype(np.float64) - 0.3)))
    assert th[k] == F(0.3)                                                  # else the comparison below would not be the same rule
    fixed = evaluate_layercam_on_test_set(gen, loader, 1.0, 0.3, device=dev, log=None)
    assert out["mean_iou"][k] == fixed["layercam_fg_iou"] and out["mean_acc"][k] == fixed["layercam_fg_acc"]
    # the curve on the published CAMs
    want, otsu = [], []
    for img, (label, tm) in loader:
        cam = gen.generate_batch(img[:1].to(dev), 1.0, label[:1].to(dev))
        ih = torch.arange(64, device=dev) * cam.shape[-2] // 64
        cam = cam[:, ih][:, :, ih].cpu().numpy()
        counts = O.histogram(cam, (tm[:1, 0] == 1).long().numpy(), th, 2)
        want.append(O.curves(counts))
        otsu.append(O.otsu(counts, th, None, 0.3)[1])
    want = np.concatenate(want)
    assert np.array_equal(out["curves"], want) and out["curves"].shape == (3, 7, 4)
    assert np.array_equal(out["otsu_thresholds"], np.concatenate(otsu))
    assert np.array_equal(out["dataset_iou"], O.iou_curve(want.sum(axis=0)))
    assert out["best_mean_iou"] == (float(th[np.argmax(out["mean_iou"])]), float(out["mean_iou"].max()))
    assert out["best_dataset_iou"][1] == out["dataset_iou"].max()
    # the default thresholds: 255 of them, every batch image with first_only off
    full = sweep_cam_thresholds(gen, loader[:1], device=dev, first_only=False, log=None)
    assert full["curves"].shape == (2, 256, 4) and np.array_equal(full["thresholds"], O.uniform_edges(0, 1, 256)[1:])


def test_generate_adaptive_pseudo_masks(dev):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import generate_adaptive_pseudo_masks, generate_pseudo_masks
    gen = _cam_generator(dev)
    g = torch.Generator().manual_seed(41)
    loader = [(torch.rand(2, 3, 224, 224, generator=g), (torch.tensor([3, 11]), None))]
    kw = dict(cam_thresh=0.3, write_png=False, max_images=2, device_batch=0, keep_on_device=True)
    generate_pseudo_masks(loader, gen, **kw)
    plain = [t.clone() for t in generate_pseudo_masks.last_masks]
    generate_adaptive_pseudo_masks(loader, gen, None, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, generate_pseudo_masks.last_masks)) and len(plain) == 2
    imgs = loader[0][0].to(dev)
    cam, _ = gen.generate_batch(imgs, alpha=1.0, class_idx=loader[0][1][0].to(dev), thresh=0.3)
    ed = ops.uniform_edges(0.0, 1.0, 64, dev)

    def composed(score_map, floor, ceil):
        counts = ops.score_histogram(score_map.contiguous(), bins=64, range=(0.0, 1.0))
        t = ops.otsu_threshold(counts, ed, fallback=0.3)[1].clamp(floor, ceil)
        return ops.keep_largest_batched(ops.threshold_per_image(score_map.contiguous(), t, positive_only=True)), t
    generate_adaptive_pseudo_masks(loader, gen, dict(bins=64), **kw)
    want, t = composed(cam, 0.0, 1.0)
    got = torch.stack(generate_pseudo_masks.last_masks)
    assert torch.equal(got, want) and got.dtype == torch.uint8 and 0 < int(got.sum()) < got.numel()
    # against the oracle's threshold of the published CAM
    host = cam.cpu().numpy()
    assert np.array_equal(t.cpu().numpy(), O.otsu(O.histogram(host, None, O.uniform_edges(0, 1, 64)), O.uniform_edges(0, 1, 64), None, 0.3)[1])
    generate_adaptive_pseudo_masks(loader, gen, dict(bins=64, floor=0.5, ceil=0.5), **kw)        # the clamp: a fixed 0.5
    assert torch.equal(torch.stack(generate_pseudo_masks.last_masks), ops.keep_largest_batched(((cam >= 0.5) & (cam > 0)).to(torch.uint8)))
    generate_adaptive_pseudo_masks(loader, gen, dict(bins=64), pamr={}, **kw)
    want_p, _ = composed(ops.pamr(imgs, cam[:, None])[:, 0], 0.0, 1.0)
    assert torch.equal(torch.stack(generate_pseudo_masks.last_masks), want_p)
    with pytest.raises(ValueError):
        generate_adaptive_pseudo_masks(loader, gen, dict(method="li"), **kw)


def test_saliency_curve_metrics_against_the_oracle(dev):
    from weaklysuperviseddl_amd.PretrainedBasnetModel.RunInference import saliency_curve_metrics
    rng = np.random.default_rng(31)
    tri = rng.integers(1, 4, (2, 64, 64)).astype(np.int64)
    pred = np.clip(rng.normal(np.where(tri == 1, 0.7, 0.3), 0.25), 0, 1).astype(F)     # exact zeros and ones included
    got = saliency_curve_metrics(_d(pred, dev), _d(tri, dev))
    edges = O.uniform_edges(0, 1, 256)
    gt = (tri == 1).astype(np.int64)
    f = O.fbeta_curve(O.curves(O.histogram(pred, gt, edges, 2, per_image=False))[0])
    assert got["max_f"] == pytest.approx(f.max(), rel=1e-12) and got["best_threshold"] == float(edges[np.argmax(f)])
    assert got["mae"] == pytest.approx(O.mae(pred, gt), rel=1e-12) and 0.2 < got["mae"] < 0.4 and (pred == 1).sum() > 0


def test_evaluate_calibration_against_the_oracle(dev):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, evaluate_calibration
    torch.manual_seed(8)
    model = build_segmentation_model().to(dev).eval()
    loader = _pet_loader(2, 2, 64, 9)
    for binarize in ("notebook", "modular"):
        got = evaluate_calibration(model, loader, device=dev, binarize=binarize, bins=15)
        confs, rights = [], []
        with torch.no_grad():
            for img, (_l, tm) in loader:
                t = tm[0, 0].clone()
                t = 1 - torch.where(t == 2, torch.ones_like(t), t) if binarize == "notebook" else (t == 1).long()
                out = model(img[:1].to(dev))["out"].contiguous()
                conf = torch.empty(1, 64, 64, device=dev)
                pred = torch.empty(1, 64, 64, device=dev, dtype=torch.int64)
                ops.confidence_histogram(out, t[None].to(dev), conf_out=conf, pred_out=pred)
                confs.append(conf.cpu().numpy().reshape(-1))
                rights.append((pred.cpu() == t[None]).numpy().reshape(-1))
        conf, right = np.concatenate(confs), np.concatenate(rights)
        ece, acc, cf, cnt = O.ece(conf, right, 15)
        assert got["ece"] == pytest.approx(ece, abs=1e-12) and np.array_equal(got["count"], cnt) and cnt.sum() == 2 * 64 * 64
        assert np.allclose(got["accuracy"], acc, rtol=0, atol=1e-12, equal_nan=True) and np.allclose(got["confidence"], cf, rtol=0, atol=1e-12, equal_nan=True)
        edges = O.uniform_edges(0, 1, 15)
        assert got["tau_0.9"] == O.tau_for_precision(conf, right, edges, 0.9) and got["tau_0.95"] == O.tau_for_precision(conf, right, edges, 0.95)
