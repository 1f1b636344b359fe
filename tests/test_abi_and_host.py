"""CPU-side checks: the C-ABI library loads and exports every symbol include/wsdl_hip.h declares, the
ctypes table mirrors the header, the product path refuses host tensors (no CPU fallback), and the host
logic (keep_largest, FlatAdam layout, batch-stride detection) behaves.  No GPU, no compute calls."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "wsdl_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(wsdl_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from weaklysuperviseddl_amd import _lib
    names = header_functions()
    assert len(names) >= 40
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f"{n} declared in wsdl_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    lib = _lib.lib()
    assert lib.wsdl_target_arch() == b"gfx950" and lib.wsdl_version() >= 100
    assert lib.wsdl_reduce_workspace() > 0 and lib.wsdl_bn_workspace(64) > 0
    # geometry validation is host-side: a bad call is rejected without touching a device
    assert lib.wsdl_conv2d_wgrad_workspace(1, 8, 4, 4, 8, 3, 3, 1, 0, 4) == 0
    assert lib.wsdl_conv2d_wgrad_workspace(16, 2048, 32, 32, 256, 3, 3, 1, 12, 12) > 0


OPTION_DEFAULTS = {
    "conv_arith": 1, "conv_split": 1, "wgrad_split": 1, "conv_il": 1, "wgrad_chan_scale": 0, "range_sentinel": 0, "stem_kernel": 1,
    "wgrad_direct": 1, "wgrad_dyraw": 1, "layercam_tail_mod": 32, "tile_threshold": 400, "ksplit_target": 512, "ksplit_max": 8,
    "ksplit_min_chunks": 4, "group_tps10": 45, "wgrad_blocks": 768, "wgrad_min_tiles": 1, "wgrad_xcd": 1, "xcd_map": 1,
    "bn_resident": 1, "bn_wide_c": 512,
}
REMOVED_OPTIONS = (
    "bn_coop", "bn_coop_wide", "xcd_rowfast", "ms_rowfast", "ms_py", "group_interleave", "wgrad_force_s", "wgrad_bk", "tile_img_major",
    "bk32", "split_bk32", "ksplit_big", "tile256", "tile64", "col_bands", "stem_wgrad", "wgrad_imbalance_split",
)


def test_option_names_are_the_documented_ones():
    """wsdl_set_option (host code) takes the 21 options the header's table documents, at their defaults, and refuses every name
    removed with the experiments it switched - naming it in wsdl_last_error()."""
    from weaklysuperviseddl_amd import _lib
    lib = _lib.lib()
    assert len(OPTION_DEFAULTS) == 21 and not set(OPTION_DEFAULTS) & set(REMOVED_OPTIONS)
    table = open(os.path.join(ROOT, "include", "wsdl_hip.h")).read().split("Process-wide options.")[1].split("(Options measured slower")[0]
    for name, default in OPTION_DEFAULTS.items():
        assert lib.wsdl_set_option(name.encode(), default) == 0, name
        assert re.search(r"\b%s\s+%d\*" % (name, default), table), name        # the header states the same default
    for name in REMOVED_OPTIONS:
        assert lib.wsdl_set_option(name.encode(), 1) != 0, name
        assert name in lib.wsdl_last_error().decode(), name
        assert not re.search(r"^ \*   %s\b" % name, table, flags=re.M), name


def test_header_cites_reference_lines():
    src = open(os.path.join(ROOT, "include", "wsdl_hip.h")).read()
    for cite in ("AlternatingDirectionCutLoss.py:65-105", "AlternatingDirectionBoundaryLoss.py:12-70", "LayerCAM.py:52-76",
                 "PsuedoMasks.py:59-62", "SegmentationModel.py:90,107", "AlternatingDirectionCutLoss.py:612-637"):
        assert cite in src, cite


def test_no_cpu_fallback_and_no_oracle_import():
    from weaklysuperviseddl_amd import ops, WsdlError
    from weaklysuperviseddl_amd.TraditionalModel import LocalNormalizedCutLoss
    x = torch.randn(1, 8, 4, 4)
    with pytest.raises(WsdlError):
        ops.prep_weights(torch.randn(8, 8, 3, 3))
    with pytest.raises(WsdlError):
        LocalNormalizedCutLoss()(torch.randn(2, 8, 8), torch.rand(3, 8, 8))
    with pytest.raises(WsdlError):
        ops.cross_entropy(x, torch.zeros(1, 4, 4, dtype=torch.long))
    # nothing under the product package may import the oracle
    pkg = os.path.join(ROOT, "weaklysuperviseddl_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", txt, flags=re.M), os.path.join(d, f)


def test_keep_largest_product_bit_exact(golden):
    from weaklysuperviseddl_amd.TraditionalModel import keep_largest
    g = golden("keep_largest")
    for n in [k[3:] for k in g.files if k.startswith("in_")]:
        assert np.array_equal(keep_largest(g["in_" + n]), g["out_" + n]), n


def test_planes_batch_stride_detection():
    from weaklysuperviseddl_amd import ops
    t = torch.zeros(2, 10, 3, 4)
    ops._req = lambda t, name="tensor", dtype=torch.float32: t      # bypass the device check for this host test
    try:
        a, bs = ops._planes(t)
        assert bs == 10 * 12 and a is t
        v = t[:, 2:7]
        a, bs = ops._planes(v)
        assert bs == 10 * 12 and a.data_ptr() == v.data_ptr()          # channel slice: no copy
        w = t[:, :, :, 1:3]
        a, bs = ops._planes(w)
        assert a.is_contiguous() and bs == 10 * 3 * 2                  # anything else: copied
    finally:
        import importlib
        importlib.reload(ops)
    assert ops.conv_out_hw(256, 256, 7, 2, 3, 1) == (128, 128)
    assert ops.conv_out_hw(32, 32, 3, 1, 36, 36) == (32, 32)


def test_flat_adam_layout_on_host():
    from weaklysuperviseddl_amd.optim import FlatAdam
    from weaklysuperviseddl_amd import WsdlError
    ps = [torch.nn.Parameter(torch.randn(s)) for s in [(5, 3), (7,), (2, 2, 2)]]
    before = [p.detach().clone() for p in ps]
    opt = FlatAdam(ps, lr=1e-3)
    assert opt.numel % 64 == 0 and all(o % 64 == 0 for o in opt.offsets)
    for p, b, off in zip(ps, before, opt.offsets):
        assert torch.equal(p.detach(), b)
        assert p.data_ptr() == opt.flat_param.data_ptr() + 4 * off
        assert p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * off
    (ps[0].sum() * 2 + ps[1].sum()).backward()
    assert opt.flat_grad[:15].eq(2).all() and opt.flat_grad[64:71].eq(1).all()
    opt.zero_grad()
    assert opt.flat_grad.abs().sum() == 0
    with pytest.raises(WsdlError):
        opt.step()                      # host parameters: the HIP Adam kernel is the only implementation


def test_bench_synthetic_inputs():
    import bench
    img, masks = bench.synthetic_batch(2, 64, 64, "cpu", 1)
    assert img.shape == (2, 3, 64, 64) and masks.shape == (2, 64, 64) and masks.dtype == torch.int64
    assert set(masks.unique().tolist()) <= {0, 1} and 0.2 < masks.float().mean() < 0.8
    assert 1 <= bench.host_cores() <= 16


def test_reference_call_signatures_are_positionally_compatible():
    """The reference's Python call signatures for the hot path - the drop-in surfaces accept the same
    positional arguments with the same names and defaults; extras are keyword-only.  Each expected list is the
    reference's ``def`` line (cited), restated here: /root/reference does not travel with the tests."""
    import inspect
    import weaklysuperviseddl_amd.TraditionalModel as TM
    from weaklysuperviseddl_amd.TraditionalModel import AlternatingDirectionCutLoss as ADC
    P = inspect.Parameter
    want = {
        # AlternatingDirectionCutLoss.py:684  def train_model(model, optimizer, criterion_ce, num_epochs = 3)
        TM.train_model: [("model", P.empty), ("optimizer", P.empty), ("criterion_ce", None), ("num_epochs", 3)],
        # SegmentationModel.py:59  def train_segmentation_model(loss_fn, run_id, lr=1e-4, num_epochs=10, batch_size=4, val_split=0.2)
        TM.train_segmentation_model: [("loss_fn", P.empty), ("run_id", P.empty), ("lr", 1e-4), ("num_epochs", 10),
                                      ("batch_size", 4), ("val_split", 0.2)],
        # AlternatingDirectionCutLoss.py:709-710  def refine_pseudo_mask(model, image, mask, lambda_boundary=0.1, threshold=0.5,
        #                                                                lr=1e-2, num_steps=20, sigma_color=0.1, window_size=5)
        TM.refine_pseudo_mask: [("model", P.empty), ("image", P.empty), ("mask", P.empty), ("lambda_boundary", 0.1),
                                ("threshold", 0.5), ("lr", 1e-2), ("num_steps", 20), ("sigma_color", 0.1), ("window_size", 5)],
        # PsuedoMasks.py:23-29  def generate_pseudo_masks(loader, layercam_gen, cam_thresh=0.3, alpha=1.0, keep_largest_masks=True, run_id="default")
        TM.generate_pseudo_masks: [("loader", P.empty), ("layercam_gen", P.empty), ("cam_thresh", 0.3), ("alpha", 1.0),
                                   ("keep_largest_masks", True), ("run_id", "default")],
        # ClassificationModel.py:70  def train_fc_only(model, device, epochs=10, num_classes=37)
        TM.train_fc_only: [("model", P.empty), ("device", "cuda"), ("epochs", 10), ("num_classes", 37)],
        # ClassificationModel.py:109  def evaluate_classification(model, dataloader, device, num_classes=37)
        TM.evaluate_classification: [("model", P.empty), ("dataloader", P.empty), ("device", "cuda"), ("num_classes", 37)],
        # LayerCAM.py:84  def evaluate_layercam_on_test_set(layercam_gen, test_loader, alpha=1.0, cam_thresh=0.3)
        TM.evaluate_layercam_on_test_set: [("layercam_gen", P.empty), ("test_loader", P.empty), ("alpha", 1.0), ("cam_thresh", 0.3)],
        # AlternatingDirectionCutLoss.py:612  def compute_affinities(image, sigma_color=0.1, sigma_space=5, window_size=5)
        TM.compute_affinities: [("image", P.empty), ("sigma_color", 0.1), ("sigma_space", 5), ("window_size", 5)],
        # ExtraUtilities.py:4  def compute_iou_and_acc(pred_mask, true_mask)
        TM.compute_iou_and_acc: [("pred_mask", P.empty), ("true_mask", P.empty)],
    }
    for fn, params in want.items():
        got = list(inspect.signature(fn).parameters.values())
        head = got[:len(params)]
        assert [(p.name, p.default) for p in head] == params, (fn.__name__, [(p.name, p.default) for p in head])
        assert all(p.kind == P.POSITIONAL_OR_KEYWORD for p in head), fn.__name__
        # everything this framework adds can only be passed by keyword: a reference-style positional call cannot hit it
        # (generate_pseudo_masks keeps its historical positional extras: the reference has no further positionals to clash)
        if fn is not TM.generate_pseudo_masks:
            assert all(p.kind == P.KEYWORD_ONLY for p in got[len(params):]), (fn.__name__, got[len(params):])
    # class constructors / methods
    assert list(inspect.signature(TM.LocalNormalizedCutLoss).parameters) == ["sigma_color", "window_size"]      # :66
    assert inspect.signature(TM.LocalNormalizedCutLoss).parameters["sigma_color"].default == 0.05
    sig = inspect.signature(TM.ConstrainToBoundaryLossSingle).parameters                         # BoundaryLoss.py:13
    assert [(k, v.default) for k, v in sig.items()] == [("sigma_color", 0.1), ("sigma_space", 5), ("window_size", 5), ("eps", 1e-8)]
    assert list(inspect.signature(TM.LayerCAMGenerator.generate).parameters)[:4] == ["self", "images", "alpha", "class_idx"]
    assert inspect.signature(TM.FrozenResNetCAM).parameters["num_classes"].default == 37          # ClassificationModel.py:10
    # train_model: the reference's call ``train_model(model, optimizer, criterion_ce, num_epochs=3)`` must not read the
    # criterion as a loader; without any loader it says where the reference takes it from
    assert ADC.train_loader is None
    with pytest.raises(ValueError, match="train_loader"):
        TM.train_model(torch.nn.Identity(), None, torch.nn.CrossEntropyLoss(), 3)
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import resolve_criterion
    with pytest.raises(ValueError, match="label"):
        resolve_criterion(torch.nn.CrossEntropyLoss(label_smoothing=0.1))
    with pytest.raises(TypeError):
        resolve_criterion(3)
    with pytest.raises(TypeError, match="device"):
        TM.train_fc_only(torch.nn.Identity(), [1, 2, 3])
    with pytest.raises(ValueError, match="dataloader"):
        TM.train_fc_only(torch.nn.Identity(), "cuda")


def test_bench_spawn_logic_dry_run_for_8_ranks():
    """GPU-less dry run of what ``python bench.py --gpus 8`` does before any rank touches a GPU: the per-rank
    environments (the driver's own launch goes through torch.distributed.run and sets the same variables)."""
    import bench
    envs = bench.rank_environments(8, 8, {"PATH": "/usr/bin"}, port=29511)
    assert len(envs) == 8
    for r, e in enumerate(envs):
        assert (e["RANK"], e["LOCAL_RANK"], e["WORLD_SIZE"], e["LOCAL_WORLD_SIZE"]) == (str(r), str(r), "8", "8")
        assert e["MASTER_ADDR"] == "127.0.0.1" and e["MASTER_PORT"] == "29511"
        assert e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and "WSDL_DIST_BACKEND" not in e       # RCCL ("nccl"), one GPU each
        assert int(e["OMP_NUM_THREADS"]) >= 1
    # fewer GPUs than ranks: a rehearsal over gloo, at most 6 processes per GPU on this pool
    assert all(e["WSDL_DIST_BACKEND"] == "gloo" for e in bench.rank_environments(4, 1, {}))
    assert bench.rank_environments(8, 2, {})[7]["WSDL_DIST_BACKEND"] == "gloo"
    with pytest.raises(SystemExit):
        bench.rank_environments(8, 1, {})
    # an existing MASTER_PORT / backend choice of the caller is kept
    e = bench.rank_environments(2, 2, {"MASTER_PORT": "1234", "WSDL_DIST_BACKEND": "gloo"})[1]
    assert e["MASTER_PORT"] == "1234" and e["WSDL_DIST_BACKEND"] == "gloo"
    # rank 0 (and only rank 0) asks RCCL to report its topology and its algorithm / protocol choices into a file
    assert envs[0]["NCCL_DEBUG"] == "INFO" and "TUNING" in envs[0]["NCCL_DEBUG_SUBSYS"] and "%p" in envs[0]["NCCL_DEBUG_FILE"]
    assert all("NCCL_DEBUG" not in e for e in envs[1:])
    assert bench.rank_environments(2, 2, {"NCCL_DEBUG": "WARN"})[0]["NCCL_DEBUG"] == "INFO"        # VERSION / WARN are raised to INFO
    e0 = bench.rank_environments(2, 2, {"NCCL_DEBUG": "TRACE"})[0]
    assert e0["NCCL_DEBUG"] == "TRACE" and "NCCL_DEBUG_FILE" not in e0                            # a caller's own INFO / TRACE stays


def test_bench_dp_self_description_fields():
    """What the first run on a real 8-GPU node must say about itself: RCCL's own report parsed into
    (size -> algorithm, protocol), per-rank step times, measured per-bucket all-reduce times, the N = 1 reference."""
    import bench
    log = "\n".join([
        "node:1:2 [0] NCCL INFO RCCL version 2.22.3+hip7.0",
        "node:1:2 [0] NCCL INFO Channel 00/32 :    0   1   2   3   4   5   6   7",
        "node:1:2 [0] NCCL INFO Trees [0] 1/-1/-1->0->-1 [1] 1/-1/-1->0->-1",
        "node:1:2 [0] NCCL INFO Ring 00 : 7 -> 0 -> 1",
        "node:1:2 [0] NCCL INFO Connected all rings",
        "node:1:2 [0] NCCL INFO AllReduce: 50331648 Bytes -> Algo 1 proto 2 time 812.5",
        "node:1:2 [0] NCCL INFO AllReduce: 50331648 Bytes -> Algo 1 proto 2 time 812.5",
        "node:1:2 [0] NCCL INFO AllReduce: 1048576 Bytes -> Algo 0 proto 0 time 31.0",
        "node:1:2 [0] NCCL INFO Broadcast: 158500000 Bytes -> Algo 1 proto 2 time 2000.0"])
    d = bench.parse_rccl_log(log)
    assert d["version_line"].startswith("RCCL version") and d["ring_only"] is False and d["algorithms_used"] == ["Ring", "Tree"]
    big = [c for c in d["choices"] if c["collective"] == "AllReduce" and c["bytes"] == 50331648][0]
    assert (big["algo"], big["proto"], big["calls"], big["model_time_us"]) == ("Ring", "Simple", 2, 812.5)
    assert any(l.startswith("Ring 00") for l in d["topology_lines"]) and any(l.startswith("Channel 00") for l in d["topology_lines"])
    assert bench.parse_rccl_log("AllReduce: 64 Bytes -> Algo 1 proto 0")["ring_only"] is True
    dp = bench.dp_self_description(8, "nccl", "2.22.3", [18.9, 19.1, None], [{"bytes": 4096, "ms": 0.02, "samples": 5}],
                                   {"ms_per_step": 18.4, "img_s_per_gpu": 869.0}, log)
    assert dp["rccl"]["nranks"] == 8 and dp["rccl"]["backend"] == "nccl" and dp["rccl"]["debug"]["choices"]
    assert dp["ms_per_step_by_rank"] == [18.9, 19.1, None] and dp["bucket_allreduce_ms"][0]["bytes"] == 4096
    assert dp["n1_reference"]["img_s_per_gpu"] == 869.0
    assert bench.dp_self_description(1, "gloo", None, [1.0], None, None, None)["rccl"]["debug"] is None


def test_bench_wait_ranks_stops_everyone_when_one_rank_fails():
    """A rank that dies early must not leave the others sitting in their collectives until the backend's timeout
    (ADVICE r2): the first non-zero exit ends the run."""
    import subprocess
    import sys
    import time
    import bench
    sleeper = [sys.executable, "-c", """import time; print('{"ok": 1}', flush=True); time.sleep(120)"""]
    procs = [subprocess.Popen(sleeper, stdout=subprocess.PIPE),
             subprocess.Popen([sys.executable, "-c", "import sys, time; time.sleep(0.5); sys.exit(3)"], stdout=subprocess.DEVNULL),
             subprocess.Popen(sleeper, stdout=subprocess.DEVNULL)]
    t0 = time.monotonic()
    rcs = bench.wait_ranks(procs, timeout_s=60.0)
    assert time.monotonic() - t0 < 30.0
    assert rcs[1] == 3 and rcs[0] != 0 and rcs[2] != 0               # the sleepers were terminated
    assert '{"ok": 1}' in procs[0].captured
    # all ranks fine: exit codes 0, rank 0's line relayed
    procs = [subprocess.Popen([sys.executable, "-c", """print('{"v": %d}')""" % r],
                              stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL) for r in range(3)]
    assert bench.wait_ranks(procs, timeout_s=60.0) == [0, 0, 0] and '{"v": 0}' in procs[0].captured
    # deadline: ranks still running are stopped and reported as failed
    procs = [subprocess.Popen([sys.executable, "-c", "import time; time.sleep(60)"], stdout=subprocess.PIPE)]
    assert bench.wait_ranks(procs, timeout_s=1.0)[0] != 0


def test_generate_coalesced_merges_and_splits_batches_on_the_host():
    """``LayerCAMGenerator.generate_coalesced`` (the loop of ``generate_pseudo_masks``): loader batches are merged into device
    batches of at most ``device_batch`` images - never across different image shapes or across a batch with / without class
    indices - and the results come back per loader batch, in order.  Host logic only: the device work is replaced by a stub
    that returns each image's first pixel and class index."""
    import torch
    from weaklysuperviseddl_amd.TraditionalModel.LayerCAM import LayerCAMGenerator
    gen = object.__new__(LayerCAMGenerator)
    gen.model = torch.nn.Identity().eval()          # merging asserts eval mode
    seen = []

    def fake_batches(batches, alpha, class_idxs, thresh, streams):
        outs = []
        for b, c in zip(batches, class_idxs):
            seen.append((b.shape[0], tuple(b.shape[1:]), None if c is None else c.numel()))
            tag = b.flatten(1)[:, 0]
            cam = tag.view(-1, 1, 1).expand(-1, 2, 2).clone()
            mask = (c.view(-1, 1, 1).expand(-1, 2, 2).to(torch.uint8) if c is not None else torch.zeros(b.shape[0], 2, 2, dtype=torch.uint8))
            outs.append((cam, mask))
        return outs

    gen.generate_batches = fake_batches
    sizes = [3, 3, 2, 5, 1, 4, 4]
    batches, classes, k = [], [], 0
    for n in sizes:
        batches.append(torch.arange(k, k + n, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 3, 4, 4).contiguous())
        classes.append(torch.arange(k, k + n) % 7)
        k += n
    # greedy, in order; a loader batch larger than the device batch still travels whole (db = 4: the batch of 5)
    for db, want in ((8, [8, 6, 8]), (32, [22]), (4, [3, 3, 2, 5, 1, 4, 4]), (5, [3, 5, 5, 5, 4])):
        seen.clear()
        outs = gen.generate_coalesced(batches, 1.0, classes, 0.3, streams=3, device_batch=db)
        assert [s[0] for s in seen] == want, (db, seen)
        assert len(outs) == len(sizes)
        k = 0
        for n, (cam, mask) in zip(sizes, outs):
            assert cam.shape == (n, 2, 2) and mask.shape == (n, 2, 2)
            assert cam[:, 0, 0].tolist() == list(range(k, k + n))                  # every image came back in its place
            assert mask[:, 0, 0].tolist() == [(k + i) % 7 for i in range(n)]         # ... with its own class index
            k += n
    # different shapes / missing class indices are never merged; device_batch=0 and a single batch fall through
    seen.clear()
    mixed = [torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), torch.zeros(1, 3, 8, 8)]
    cls = [torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long), None, None]
    outs = gen.generate_coalesced(mixed, 1.0, cls, None, streams=2, device_batch=32)
    assert [(s[0], s[1][-1], s[2]) for s in seen] == [(2, 4, 2), (2, 8, 2), (3, 8, None)] and [o[0].shape[0] for o in outs] == [2, 2, 2, 1]
    seen.clear()
    gen.generate_coalesced(batches, 1.0, classes, 0.3, streams=3, device_batch=0)
    assert [s[0] for s in seen] == sizes
    gen.model.train()
    with pytest.raises(RuntimeError):
        gen.generate_coalesced(batches, 1.0, classes, 0.3, streams=3, device_batch=8)


def test_bench_roofline_prices_the_kernel_body_over_its_three_entry_points():
    """bench.py's roofline line: the 256 x 128 forward / input-gradient body has three entry points (plain, grouped, multi-source),
    each a timing class of its own; the line merges them (sum of nominal FLOPs / sum of time) and looks the rocprofv3 average up
    as sum of the three rows' time / sum of their calls in the committed kernel-stats file."""
    import bench
    recs = [{"kernel": bench.BODY_256x128[0], "launches": 66, "total_ms": 6.6, "work": 1.5e12, "executed": 1.45e12, "alg_bytes": 6e9, "avg_us": 100.0},
            {"kernel": bench.BODY_256x128[1], "launches": 1, "total_ms": 0.7, "work": 0.4e12, "executed": 0.1e12, "alg_bytes": 1e9, "avg_us": 700.0},
            {"kernel": bench.BODY_256x128[2], "launches": 1, "total_ms": 0.7, "work": 0.4e12, "executed": 0.1e12, "alg_bytes": 1e9, "avg_us": 700.0},
            {"kernel": "bn_fwd_resident_kernel<256, 16>", "launches": 11, "total_ms": 0.6, "work": 0.0, "executed": 0.0, "alg_bytes": 3e9, "avg_us": 54.5}]
    merged = bench.merge_body_classes(list(recs))
    assert len(merged) == 2 and merged[0]["kernel"] == bench.BODY_256x128_NAME and merged[0]["launches"] == 68
    assert abs(merged[0]["total_ms"] - 8.0) < 1e-9 and merged[0]["work"] == 2.3e12 and len(merged[0]["entries"]) == 3
    assert bench.merge_body_classes(recs[:1] + recs[3:]) == recs[:1] + recs[3:]          # one entry point only: nothing to merge
    us, calls, f, rows = bench.rocprof_avg_us_many(list(bench.BODY_256x128))
    assert f and f.startswith("profiles/") and rows and calls == sum(r["calls"] for r in rows)
    assert abs(us - sum(r["avg_us"] * r["calls"] for r in rows) / calls) < 1e-3
    assert min(r["avg_us"] for r in rows) <= us <= max(r["avg_us"] for r in rows)


def test_plan_recording_is_per_host_thread_and_options_are_guarded():
    """"no global state other than a lazily-built kernel table ... re-entrant".  The recording state of the launch
    plans is thread-local on both sides of the ABI (csrc/plan.hip `thread_local g_plan_rec`, ops.PLAN_REC): a second host
    thread that calls into the library while the first one records is NOT written into the first one's plan, can record a
    plan of its own, and the process-wide options cannot be changed under a recording (a plan freezes the tile choices made
    under the option set it was recorded with).  No kernel is launched: begin / end / abort / stats / set_option only."""
    import ctypes as C
    import threading
    from weaklysuperviseddl_amd import lib, ops
    L = lib()
    seen = {}

    assert L.wsdl_plan_recording() == 0
    assert L.wsdl_plan_begin() == 0 and L.wsdl_plan_recording() == 1
    ops.PLAN_REC[0] = "thread-A recording"

    def other():
        seen["recording_seen_by_b"] = L.wsdl_plan_recording()
        seen["slot_seen_by_b"] = ops.PLAN_REC[0]
        seen["begin_b"] = L.wsdl_plan_begin()                 # its own recording
        seen["recording_b"] = L.wsdl_plan_recording()
        seen["set_option_b"] = L.wsdl_set_option(b"ksplit_max", 8)
        seen["set_option_err"] = L.wsdl_last_error().decode()
        h = C.c_void_p()
        seen["end_b"] = L.wsdl_plan_end(C.byref(h))
        n = C.c_longlong(-1)
        seen["stats_b"] = L.wsdl_plan_stats(h, C.byref(n), None, None, None, None)
        seen["kernels_b"] = n.value
        L.wsdl_plan_destroy(h)
        seen["after_b"] = L.wsdl_plan_recording()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    try:
        assert seen["recording_seen_by_b"] == 0 and seen["slot_seen_by_b"] is None
        assert seen["begin_b"] == 0 and seen["recording_b"] == 1 and seen["end_b"] == 0 and seen["after_b"] == 0
        assert seen["stats_b"] == 0 and seen["kernels_b"] == 0
        assert seen["set_option_b"] != 0 and "being recorded" in seen["set_option_err"]
        assert L.wsdl_plan_recording() == 1 and ops.PLAN_REC[0] == "thread-A recording"     # thread A's is untouched
        assert L.wsdl_set_option(b"ksplit_max", 8) != 0                                      # ... and still guards the options
        assert L.wsdl_plan_begin() != 0                                                      # one recording per thread
    finally:
        ops.PLAN_REC[0] = None
        assert L.wsdl_plan_abort() == 0
    assert L.wsdl_plan_recording() == 0
    assert L.wsdl_set_option(b"ksplit_max", 8) == 0


def test_plan_key_sees_the_host_scalars_of_loss_objects():
    """a plan freezes every host scalar that was a kernel argument when it was recorded.  ``plan.host_scalars`` is the
    part of a plan's key that covers loss objects (attributes of objects and sub-modules, defaults and closure cells of
    functions); ``plan.loss_tag`` maps an inline lambda - a new function object per call - onto ONE planned step."""
    import torch
    from weaklysuperviseddl_amd import plan

    class Loss:
        def __init__(self, w):
            self.weight, self.window, self.name = w, 5, "ncut"
            self.table = torch.zeros(3)

    a, b = Loss(0.1), Loss(0.1)
    assert plan.host_scalars(a) == plan.host_scalars(b)
    b.weight = 0.2
    assert plan.host_scalars(a) != plan.host_scalars(b)
    m = torch.nn.Sequential(torch.nn.Dropout(0.1), torch.nn.ReLU())
    k0 = plan.host_scalars(m)
    m[0].p = 0.3
    assert plan.host_scalars(m) != k0

    def make(w, obj):
        return lambda o, i: w * obj.weight
    f1, f2, f3 = make(0.1, a), make(0.1, a), make(0.5, a)
    assert f1 is not f2 and plan.loss_tag(f1) == plan.loss_tag(f2) == plan.loss_tag(f3)     # same code, same captured object
    assert plan.loss_tag(make(0.1, b)) != plan.loss_tag(f1)                                  # another captured object
    assert plan.host_scalars(f1) == plan.host_scalars(f2) != plan.host_scalars(f3)           # the ramped weight is in the KEY
    a.weight = 0.7
    assert plan.host_scalars(f1) != plan.host_scalars(make(0.1, Loss(0.1)))
    assert plan.loss_tag(None) is None and plan.host_scalars(None) is None
    assert plan.loss_tag(a) == id(a)
    hash(plan.host_scalars(f1)), hash(plan.host_scalars(m)), hash(plan.loss_tag(f1))


def test_the_nine_criteria_keep_their_plan_key_state_dict_and_repr():
    """The loss criteria share one base class (``wnn._Criterion``); what a launch plan keys them on - ``plan.host_scalars``:
    the class name, the scalar attributes of ``__dict__`` and of the sub-modules - is behaviour, and so are the ``state_dict``
    keys and the ``repr``.  The literals are what the commit before the base class gave for default options and
    ``weight=None`` on the CPU: every ``*_ptr`` is 0 except the address of the one-element ``alpha_dev`` / ``lam_dev`` buffer,
    DEV below."""
    import torch
    from weaklysuperviseddl_amd import nn as wnn, plan
    DEV = "the address of the object's own one-element buffer"
    want = {
        "CrossEntropyLoss": (
         ('CrossEntropyLoss', (('_is_full_backward_hook', None), ('ignore_index', -100), ('label_smoothing', 0.0),
         ('pixel_weight_ptr', 0), ('pixel_weight_shape', ''), ('reduction', 'mean'), ('training', True),
         ('weight_ptr', 0))),
         [],
         "CrossEntropyLoss(ignore_index=-100, reduction='mean', label_smoothing=0.0, weight=False, pixel_weight=None)"),
        "MinedCrossEntropyLoss": (
         ('MinedCrossEntropyLoss', (('_is_full_backward_hook', None), ('drop_frac', 0.0), ('ignore_index', -100),
         ('kept_ptr', 0), ('label_smoothing', 0.0), ('min_kept', 0), ('mode', 'hard'), ('pixel_weight_ptr', 0),
         ('pixel_weight_shape', ''), ('reduction', 'mean'), ('scope', 'batch'), ('selection_ptr', 0), ('thresh', 0.7),
         ('threshold_ptr', 0), ('training', True), ('valid_ptr', 0), ('weight_ptr', 0))),
         [],
         "MinedCrossEntropyLoss(mode='hard', thresh=0.7, min_kept=0, drop_frac=0.0, scope='batch', ignore_index=-100, reduction='mean', label_smoothing=0.0, weight=False)"),
        "BoundaryAwareCrossEntropyLoss": (
         ('BoundaryAwareCrossEntropyLoss', (('_is_full_backward_hook', None), ('d2_in_ptr', 0), ('d2_out_ptr', 0),
         ('floor', 0.0), ('ignore_index', -100), ('label_smoothing', 0.0), ('pixel_weight_ptr', 0),
         ('pixel_weight_shape', ''), ('reduction', 'mean'), ('sigma', 3.0), ('training', True), ('value', 1),
         ('weight_ptr', 0))),
         [],
         "BoundaryAwareCrossEntropyLoss(sigma=3.0, floor=0.0, value=1, ignore_index=-100, reduction='mean', label_smoothing=0.0, weight=False)"),
        "BoundaryLoss": (
         ('BoundaryLoss', (('_is_full_backward_hook', None), ('classes_key', '1'), ('d2_in_ptr', 0), ('d2_out_ptr',
         0), ('ignore_index', -100), ('phi_ptr', 0), ('phi_shape', ''), ('scale_dev_ptr', 0), ('training', True))),
         [],
         'BoundaryLoss(classes=(1,), ignore_index=-100)'),
        "CrossEntropyBoundaryLoss": (
         ('CrossEntropyBoundaryLoss', (('_is_full_backward_hook', None), ('alpha_dev_ptr', DEV), ('ignore_index',
         -100), ('label_smoothing', 0.0), ('training', True), ('weight_ptr', 0), ('BoundaryLoss',
         (('_is_full_backward_hook', None), ('classes_key', '1'), ('d2_in_ptr', 0), ('d2_out_ptr', 0),
         ('ignore_index', -100), ('phi_ptr', 0), ('phi_shape', ''), ('scale_dev_ptr', 0), ('training', True))))),
         [],
         'CrossEntropyBoundaryLoss(\n  classes=(1,), ignore_index=-100, label_smoothing=0.0, weight=False\n  (boundary): BoundaryLoss(classes=(1,), ignore_index=-100)\n)'),
        "TverskyLoss": (
         ('TverskyLoss', (('_is_full_backward_hook', None), ('alpha', 0.5), ('beta', 0.5), ('classes', None),
         ('classes_key', 'all'), ('gamma', 1.0), ('ignore_index', -100), ('per_image', False), ('present_only',
         False), ('scale_dev_ptr', 0), ('smooth', 1.0), ('training', True))),
         [],
         'TverskyLoss(alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, classes=None, per_image=False, present_only=False, ignore_index=-100)'),
        "DiceLoss": (
         ('DiceLoss', (('_is_full_backward_hook', None), ('alpha', 0.5), ('beta', 0.5), ('classes', None),
         ('classes_key', 'all'), ('gamma', 1.0), ('ignore_index', -100), ('per_image', False), ('present_only',
         False), ('scale_dev_ptr', 0), ('smooth', 0.5), ('training', True))),
         [],
         'DiceLoss(smooth=1.0, classes=None, per_image=False, present_only=False, ignore_index=-100)'),
        "FocalLoss": (
         ('FocalLoss', (('_is_full_backward_hook', None), ('gamma', 2.0), ('ignore_index', -100), ('pixel_weight_ptr',
         0), ('pixel_weight_shape', ''), ('reduction', 'mean'), ('training', True), ('weight_ptr', 0))),
         [],
         "FocalLoss(gamma=2.0, ignore_index=-100, reduction='mean', weight=False)"),
        "CrossEntropyTverskyLoss": (
         ('CrossEntropyTverskyLoss', (('_is_full_backward_hook', None), ('ignore_index', -100), ('label_smoothing',
         0.0), ('lam_dev_ptr', DEV), ('training', True), ('weight_ptr', 0), ('TverskyLoss',
         (('_is_full_backward_hook', None), ('alpha', 0.5), ('beta', 0.5), ('classes', None), ('classes_key', 'all'),
         ('gamma', 1.0), ('ignore_index', -100), ('per_image', False), ('present_only', False), ('scale_dev_ptr', 0),
         ('smooth', 1.0), ('training', True))))),
         [],
         'CrossEntropyTverskyLoss(\n  alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, classes=None, per_image=False, present_only=False, ignore_index=-100, label_smoothing=0.0, weight=False\n  (tversky): TverskyLoss(alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, classes=None, per_image=False, present_only=False, ignore_index=-100)\n)'),
    }
    assert len(want) == 9
    for name, (key, state, text) in want.items():
        crit = getattr(wnn, name)()
        assert isinstance(crit, wnn._Criterion) and "_apply" not in vars(type(crit)) and "_refresh_pointers" not in vars(type(crit))
        dev = {"CrossEntropyBoundaryLoss": "alpha_dev", "CrossEntropyTverskyLoss": "lam_dev"}.get(name)
        if dev is not None:
            key = (key[0], tuple((k[0], getattr(crit, dev).data_ptr()) if isinstance(k, tuple) and k[1:] == (DEV,) else k for k in key[1]))
        assert plan.host_scalars(crit) == key, name
        assert sorted(crit.state_dict()) == state, name
        assert repr(crit) == text, name
        hash(plan.host_scalars(crit))
    w = wnn.FocalLoss(weight=torch.tensor([1.0, 2.0], dtype=torch.float64))
    assert sorted(w.state_dict()) == ["weight"] and w.weight.dtype == torch.float32 and w.weight_ptr == w.weight.data_ptr()


def test_the_range_guard_acts_by_default():
    """the sentinel must ACT in the default configuration (the reference's fp32 has no range floor), not
    only warn.  The product default is "auto"; tests/conftest.py pins "warn" inside tests (bit-for-bit comparisons need one
    option set), which is what the module-level list shows here."""
    from weaklysuperviseddl_amd import optim
    assert optim.RANGE_GUARD_DEFAULT == "auto"
    assert optim.RANGE_GUARD[0] == "warn"        # (the fixture; outside tests: WSDL_RANGE_GUARD or the default)
