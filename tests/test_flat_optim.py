"""CPU checks of the flat optimiser (no GPU): the float64 oracle of csrc/flat_optim.hip (tests/flat_optim_oracle.py) against
live torch.optim.SGD / Adam / AdamW + clip_grad_norm_ in float64, PolyLR against torch's PolynomialLR, the weight-decay block
table, argument validation and the ABI table."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flat_optim_oracle as O  # noqa: E402

SHAPES = [(5, 3), (70,), (64,), (2, 2, 2), (129,)]      # 15, 70, 64, 8, 129 floats: non-multiples of 64 among them
NO_DECAY = [False, True, False, True, False]
STEPS = 4
GRAD_SCALES = [3.0, 0.01, 2.0, 0.02]                    # per step: with max_norm = 1 steps 1 and 3 clip, steps 2 and 4 do not
MAX_NORM = 1.0
GRAD_SCALE = 0.5                                        # the 1 / world_size of data parallelism


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def layout():
    from weaklysuperviseddl_amd import optim
    offsets, n = [], 0
    for s in SHAPES:
        offsets.append(n)
        n += (math.prod(s) + 63) // 64 * 64
    numels = [math.prod(s) for s in SHAPES]
    return offsets, numels, n, optim.build_decay_blocks(offsets, numels, n, NO_DECAY).numpy()


def flat(tensors, offsets, total):
    out = np.zeros(total)
    for t, off in zip(tensors, offsets):
        out[off:off + t.numel()] = t.detach().double().reshape(-1).numpy()
    return out


def torch_optimizer(algo, params, lr, wd, momentum, nesterov):
    groups = [{"params": [p for p, nd in zip(params, NO_DECAY) if not nd], "weight_decay": wd},
              {"params": [p for p, nd in zip(params, NO_DECAY) if nd], "weight_decay": 0.0}]
    if algo == O.SGD:
        return torch.optim.SGD(groups, lr=lr, momentum=momentum, nesterov=nesterov)
    if algo == O.ADAMW:
        return torch.optim.AdamW(groups, lr=lr)
    return torch.optim.Adam(groups, lr=lr)


def torch_state(algo, opt, params, offsets, total):
    m, v = np.zeros(total), np.zeros(total)
    for p, off in zip(params, offsets):
        st = opt.state.get(p, {})
        if algo == O.SGD:
            if st.get("momentum_buffer") is not None:
                m[off:off + p.numel()] = st["momentum_buffer"].reshape(-1).numpy()
        elif st:
            m[off:off + p.numel()] = st["exp_avg"].reshape(-1).numpy()
            v[off:off + p.numel()] = st["exp_avg_sq"].reshape(-1).numpy()
    return m, v


CASES = [(O.SGD, 0.9, True, 1e-2), (O.SGD, 0.9, False, 1e-2), (O.SGD, 0.0, False, 1e-2), (O.ADAM_L2, 0, False, 1e-2),
         (O.ADAMW, 0, False, 1e-2), (O.ADAM_L2, 0, False, 0.0)]


@pytest.mark.parametrize("algo,momentum,nesterov,wd", CASES)
@pytest.mark.parametrize("skip_at", [None, 2])
def test_oracle_matches_live_torch_float64(algo, momentum, nesterov, wd, skip_at):
    """4 steps, five parameters, decay groups as torch param groups, clipping by clip_grad_norm_, a skipped step as a step()
    that is not called.  Both sides float64, different operation order only: 1e-12 relative."""
    gen = torch.Generator().manual_seed(11)
    offsets, numels, total, table = layout()
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in SHAPES]
    lr = 0.05
    topt = torch_optimizer(algo, params, lr, wd, momentum, nesterov)
    orc = O.FlatOracle(algo, flat(params, offsets, total), lr=lr, weight_decay=wd, momentum=momentum, nesterov=nesterov,
                       grad_scale=GRAD_SCALE, max_norm=MAX_NORM, skip_nonfinite=True, decay_blocks=table)
    clipped = []
    for step in range(1, STEPS + 1):
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * GRAD_SCALES[step - 1] for s in SHAPES]
        if step == skip_at:
            grads[2].view(-1)[5] = float("inf")
        applied = orc.step(flat(grads, offsets, total))
        assert applied == (step != skip_at)
        if step == skip_at:
            continue                                    # torch: optimizer.step() is not called for this gradient
        for p, g in zip(params, grads):
            p.grad = g * GRAD_SCALE                     # the averaged gradient (exact: a power of two)
        norm = float(torch.nn.utils.clip_grad_norm_(params, MAX_NORM))
        clipped.append(norm > MAX_NORM)
        assert abs(orc.norm - norm) <= 1e-12 * norm
        assert (orc.clip < 1.0) == (norm > MAX_NORM)
        topt.step()
        m, v = torch_state(algo, topt, params, offsets, total)
        assert rel(orc.p, flat(params, offsets, total)) <= 1e-12, step
        assert rel(orc.m, m) <= 1e-12, step
        if algo != O.SGD:
            assert rel(orc.v, v) <= 1e-12, step
    # the reference itself clipped on at least one step and left at least one other alone
    assert any(clipped) and not all(clipped), clipped
    assert orc.skipped == (1 if skip_at else 0) and orc.step_no == STEPS - orc.skipped


def test_poly_lr_matches_torch_polynomial_lr():
    from weaklysuperviseddl_amd import optim

    class Opt:
        lr = 0.01

    w = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    topt = torch.optim.SGD([w], lr=0.01)
    tsched = torch.optim.lr_scheduler.PolynomialLR(topt, total_iters=8, power=0.9)
    mine = Opt()
    sched = optim.PolyLR(mine, 8, power=0.9)
    assert mine.lr == 0.01
    for _ in range(10):                                 # two steps past total_steps: the rate stays at its floor
        topt.step()
        tsched.step()
        sched.step()
        want = tsched.get_last_lr()[0]
        assert abs(mine.lr - want) <= 1e-12 * 0.01, (mine.lr, want)
    assert mine.lr == 0.0 and sched.get_last_lr() == [0.0]


def test_poly_lr_warmup_and_floor_closed_form():
    from weaklysuperviseddl_amd import optim

    class Opt:
        lr = 0.2

    o = Opt()
    s = optim.PolyLR(o, 10, power=2.0, warmup_steps=3, min_lr=0.02)
    got = [o.lr] + [s.step() for _ in range(12)]
    want = []
    for t in range(13):
        if t < 3:
            want.append(0.2 * (t + 1) / 4)              # the linear ramp reaches base_lr at t = warmup_steps
        else:
            want.append(0.02 + 0.18 * (1 - min(t - 3, 7) / 7) ** 2.0)
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert got[3] == 0.2 and got[10] == 0.02 and got[12] == 0.02
    for bad in (dict(total_steps=0), dict(total_steps=5, warmup_steps=5), dict(total_steps=5, min_lr=-1.0),
                dict(total_steps=5, power=0.0)):
        with pytest.raises(ValueError):
            optim.PolyLR(Opt(), **bad)


def test_decay_block_table_from_offsets_and_filter():
    from weaklysuperviseddl_amd import optim
    offsets, numels, total, table = layout()
    assert offsets == [0, 64, 192, 256, 320] and total == 512 and table.dtype == np.uint8
    #           (5,3) | (70,) two blocks | (64,) | (2,2,2) | (129,) three blocks
    assert table.tolist() == [1, 0, 0, 1, 0, 1, 1, 1]
    assert O.expand_blocks(table, total).sum() == 64 * 5
    with pytest.raises(ValueError):
        optim.build_decay_blocks([0, 70], [70, 5], 192, [False, True])     # a parameter off the 64-float grid
    # through the optimiser: a predicate and a collection give the same table; none at all gives no table
    ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    a = optim.FlatSGD(ps, lr=0.1, weight_decay=1e-4, no_decay=lambda p: p.numel() in (70, 8))
    assert a.offsets == offsets and a.decay_blocks.tolist() == table.tolist()
    ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    b = optim.FlatAdamW(ps, lr=0.1, no_decay=[ps[1], ps[3]])
    assert b.decay_blocks.tolist() == table.tolist() and b.weight_decay == 1e-2 and b.decoupled
    ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    assert optim.FlatAdam(ps, lr=0.1, weight_decay=1e-4).decay_blocks is None
    # segments slice the table on the boundaries they slice the buffers on
    assert b.decay_blocks[offsets[1] // 64:offsets[3] // 64].tolist() == [0, 0, 1]


def test_no_decay_norm_and_bias_helper():
    from weaklysuperviseddl_amd import nn as wnn, optim
    model = torch.nn.Sequential(wnn.Conv2d(3, 8, 3, bias=True), wnn.BatchNorm2d(8), torch.nn.BatchNorm2d(8), wnn.Linear(8, 2))
    got = {id(p) for p in optim.no_decay_norm_and_bias(model)}
    want = {id(model[0].bias), id(model[1].weight), id(model[1].bias), id(model[2].weight), id(model[2].bias), id(model[3].bias)}
    assert got == want
    assert id(model[0].weight) not in got and id(model[3].weight) not in got


def test_invalid_arguments_raise_on_construction():
    from weaklysuperviseddl_amd import optim
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer

    def ps():
        return [torch.nn.Parameter(torch.randn(4))]
    with pytest.raises(ValueError):
        optim.FlatSGD(ps(), lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        optim.FlatSGD(ps(), lr=0.1, weight_decay=-1e-4)
    with pytest.raises(ValueError):
        optim.FlatSGD(ps(), lr=0.1, momentum=-0.1)
    with pytest.raises(ValueError):
        optim.FlatAdam(ps(), lr=0.1, weight_decay=-1.0)
    with pytest.raises(ValueError):
        optim.FlatAdamW(ps(), lr=0.1, max_grad_norm=0.0)
    with pytest.raises(ValueError):
        optim.FlatAdam(ps(), lr=0.1, max_grad_norm=-2.0)
    with pytest.raises(ValueError):
        make_optimizer(torch.nn.Linear(2, 2), kind="lamb")
    # the valid neighbours construct, on the host, and are FlatAdam for the isinstance gates
    sgd = optim.FlatSGD(ps(), lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    assert isinstance(sgd, optim.FlatAdam) and sgd.exp_avg is not None and sgd.exp_avg_sq is None
    assert optim.FlatSGD(ps(), lr=0.1).exp_avg is None
    assert isinstance(make_optimizer(torch.nn.Linear(2, 2), kind="sgd", momentum=0.9), optim.FlatSGD)
    assert isinstance(make_optimizer(torch.nn.Linear(2, 2), kind="adamw"), optim.FlatAdamW)


def test_launch_selection_and_early_step_refusal_on_host():
    """Which launches a step issues is a function of the settings: the defaults select the old Adam launch; clipping and
    skipping refuse early segment steps, naming the switch."""
    from weaklysuperviseddl_amd import ops, optim

    def ps():
        return [torch.nn.Parameter(torch.randn(4))]
    assert optim.FlatAdam(ps(), lr=0.1).launch_key() == (None, False, False)
    assert optim.FlatAdam(ps(), lr=0.1, decoupled=True).algo() is None                  # no decay to decouple
    assert optim.FlatAdam(ps(), lr=0.1, weight_decay=1e-4).algo() == ops.FLAT_ADAM_L2
    assert optim.FlatAdamW(ps(), lr=0.1).algo() == ops.FLAT_ADAMW
    assert optim.FlatAdam(ps(), lr=0.1, skip_nonfinite=True).launch_key() == (ops.FLAT_ADAM_L2, True, False)
    assert optim.FlatSGD(ps(), lr=0.1).launch_key() == (ops.FLAT_SGD, False, False)
    opt = optim.FlatSGD(ps(), lr=0.1, max_grad_norm=1.0)
    with pytest.raises(RuntimeError, match="optimizer.early_step = False"):
        opt.early_step = True
    opt.early_step = False
    free = optim.FlatSGD(ps(), lr=0.1)
    free.early_step = True
    hv = optim.FlatSGD(ps(), lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4, max_grad_norm=2.0, skip_nonfinite=True,
                       grad_scale=0.5)._hyper_values()
    assert len(hv) == ops.FLAT_HYPER and hv[0] == 0.1 and hv[4:] == (0.5, 1e-4, 0.9, 1.0, 2.0, 1.0)


def test_new_symbols_are_in_the_header_and_bound():
    import re
    from weaklysuperviseddl_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "wsdl_hip.h")).read()
    for name in ("wsdl_grad_norm_partials", "wsdl_grad_norm_workspace", "wsdl_grad_sqnorm_partials", "wsdl_grad_clip_finalize",
                 "wsdl_flat_step_dev"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["wsdl_flat_step_dev"][1]) == 11 and len(_lib.SIGNATURES["wsdl_grad_clip_finalize"][1]) == 6
    for macro, value in (("WSDL_FLAT_HYPER", ops.FLAT_HYPER), ("WSDL_FLAT_STATS", ops.FLAT_STATS), ("WSDL_FLAT_ADAM_L2", ops.FLAT_ADAM_L2),
                         ("WSDL_FLAT_ADAMW", ops.FLAT_ADAMW), ("WSDL_FLAT_SGD", ops.FLAT_SGD)):
        assert re.search(r"#define %s %d\b" % (macro, value), src), macro
    assert (O.ADAM_L2, O.ADAMW, O.SGD) == (ops.FLAT_ADAM_L2, ops.FLAT_ADAMW, ops.FLAT_SGD)
    lib = _lib.lib()
    assert lib.wsdl_grad_norm_workspace() == 8 * lib.wsdl_grad_norm_partials() > 0
    assert "flat_optim.hip" in __import__("weaklysuperviseddl_amd._build", fromlist=["SOURCES"]).SOURCES


def test_trainers_take_optimizer_kind_keyword_only():
    import inspect
    from weaklysuperviseddl_amd.FullySupervisedModel.SupervisedModel import run_supervised_training
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer, train_segmentation_model
    for fn in (run_supervised_training, train_segmentation_model):
        sig = inspect.signature(fn).parameters
        for name, default in (("optimizer_kind", "adam"), ("optimizer_kwargs", None)):
            assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    sig = inspect.signature(make_optimizer).parameters
    assert list(sig)[:3] == ["model", "lr", "early_step"] and sig["kind"].kind is inspect.Parameter.KEYWORD_ONLY
