"""The fully-supervised baseline (reference FullySupervisedModel/SupervisedModel.py, TraditionalModel/ExtraUtilities.py:24-63):
the Oxford-IIIT Pet reader, the aux-less DeepLabV3 model, the device count kernel (wsdl_seg_counts) and the drop-in
``SupervisedModel`` functions."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import report_line  # noqa: E402


# ---- fixtures ---------------------------------------------------------------------------------------------------------

def make_pet_tree(root, n_trainval, n_test, seed=0):
    """A synthetic tree in torchvision's OxfordIIITPet layout: JPEGs of odd sizes, trimaps {1 pet, 2 background, 3 border}."""
    from PIL import Image
    base = root / "oxford-iiit-pet"
    (base / "images").mkdir(parents=True)
    (base / "annotations" / "trimaps").mkdir(parents=True)
    rng = np.random.default_rng(seed)
    for split, n in (("trainval", n_trainval), ("test", n_test)):
        lines = []
        for i in range(n):
            name = f"{'Abyssinian' if i % 2 else 'boxer'}_{split}_{i}"
            w, h = int(rng.integers(150, 330)), int(rng.integers(140, 300))
            yy, xx = np.mgrid[0:h, 0:w]
            cy, cx, r = h * rng.uniform(0.3, 0.7), w * rng.uniform(0.3, 0.7), min(h, w) * rng.uniform(0.2, 0.4)
            d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            tri = np.where(d < r, 1, 2).astype(np.uint8)
            tri[np.abs(d - r) < 3] = 3
            img = np.stack([120 + 80 * (tri == 1) * np.sin(xx / 9.0 + c) + rng.normal(0, 12, (h, w)) for c in range(3)], -1)
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(base / "images" / f"{name}.jpg")
            Image.fromarray(tri).save(base / "annotations" / "trimaps" / f"{name}.png")
            cls = 1 + (i * 7) % 37
            lines.append(f"{name} {cls} {1 + i % 2} {1 + i % 12}\n")
        (base / "annotations" / f"{split}.txt").write_text("".join(lines))
    return root


def reference_item(root, name):
    """The reference's transform chain restated with PIL (torchvision's Resize / ToTensor / PILToTensor on PIL images)."""
    from PIL import Image
    base = root / "oxford-iiit-pet"
    image = Image.open(base / "images" / f"{name}.jpg").convert("RGB").resize((224, 224), Image.BICUBIC)
    x = torch.from_numpy(np.array(image, np.uint8, copy=True)).view(224, 224, 3).permute(2, 0, 1).contiguous()
    x = x.to(dtype=torch.get_default_dtype()).div(255)
    mask = Image.open(base / "annotations" / "trimaps" / f"{name}.png").resize((224, 224), Image.BICUBIC)
    m = torch.as_tensor(np.array(mask, copy=True)).view(224, 224, 1).permute(2, 0, 1)
    return x, m


def numpy_counts(logits, labels):
    """inter / npred / nlabel / correct of torch.argmax(logits, 1) vs labels, in numpy (NaN = maximum, first wins)."""
    C = logits.shape[1]
    pred = torch.argmax(torch.from_numpy(logits), dim=1).numpy()
    inter = [int(((pred == c) & (labels == c)).sum()) for c in range(C)]
    npred = [int((pred == c).sum()) for c in range(C)]
    nlabel = [int((labels == c).sum()) for c in range(C)]
    return np.array(inter + npred + nlabel + [int((pred == labels).sum())], dtype=np.int64)


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()
            if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]


def test_signatures_match_the_reference():
    from weaklysuperviseddl_amd.FullySupervisedModel import SupervisedModel as sm
    from weaklysuperviseddl_amd.TraditionalModel import ExtraUtilities as eu
    E = inspect.Parameter.empty
    # FullySupervisedModel/SupervisedModel.py:13, 18, 29, 45, 85-93
    assert _sig(sm.initialize_model) == [("num_classes", 2), ("device", None)]
    assert _sig(sm.get_dataloaders) == [("data_path", "./data"), ("train_ratio", 0.85), ("batch_size", 16), ("num_workers", 0)]
    assert _sig(sm.train_one_epoch) == [("model", E), ("dataloader", E), ("criterion", E), ("optimizer", E), ("device", E)]
    assert _sig(sm.evaluate_model) == [("model", E), ("dataloader", E), ("device", E), ("num_classes", 2)]
    assert _sig(sm.run_supervised_training) == [("data_path", "./data"), ("num_epochs", 10), ("batch_size", 16),
                                                ("train_ratio", 0.85), ("num_classes", 2), ("lr", 1e-4), ("device", None)]
    # TraditionalModel/ExtraUtilities.py:24, 43
    assert _sig(eu.download_data) == [("pth", None), ("split", "test")]
    assert _sig(eu.load_split_data) == [("pth", None), ("train_ratio", 0.8)]
    from weaklysuperviseddl_amd.FullySupervisedModel import run_supervised_training  # noqa: F401  (package export)


def test_model_matches_torchvision_layout_without_aux_head():
    import oracle
    from weaklysuperviseddl_amd.FullySupervisedModel.SupervisedModel import initialize_model
    model = initialize_model(2, device="cpu")
    ref = oracle.models.DeepLabV3ResNet50(num_classes=2, aux_loss=False)
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert mine == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert not any(k.startswith("aux_classifier") for k in mine) and "classifier.4.weight" in mine
    model.load_state_dict(ref.state_dict(), strict=True)
    assert torch.equal(model.state_dict()["classifier.4.weight"], ref.state_dict()["classifier.4.weight"])
    # a torchvision ResNet-50 state_dict (fc.* included) fills the backbone
    trunk = {k[len("backbone."):]: v for k, v in ref.state_dict().items() if k.startswith("backbone.")}
    trunk["fc.weight"], trunk["fc.bias"] = torch.zeros(1000, 2048), torch.zeros(1000)
    m2 = initialize_model(2, device="cpu", backbone_state_dict=trunk)
    assert torch.equal(m2.state_dict()["backbone.layer4.2.conv3.weight"], trunk["layer4.2.conv3.weight"])


def test_reader_items_match_the_reference_transforms(tmp_path):
    from weaklysuperviseddl_amd.TraditionalModel.ExtraUtilities import download_data, load_split_data
    root = make_pet_tree(tmp_path, 7, 3)
    ds = download_data(pth=str(root), split="trainval")
    assert len(ds) == 7
    listing = (root / "oxford-iiit-pet" / "annotations" / "trainval.txt").read_text().split("\n")
    for i in range(7):
        name, cls = listing[i].split()[:2]
        image, (category, mask) = ds[i]
        x, m = reference_item(root, name)
        assert category == int(cls) - 1
        assert image.dtype == torch.float32 and image.shape == (3, 224, 224) and torch.equal(image, x)
        assert mask.dtype == torch.uint8 and mask.shape == (1, 224, 224) and torch.equal(mask, m)
    assert len(download_data(pth=str(root))) == 3                     # split="test" by default
    # the split: random_split(full, [int(r N), N - int(r N)]) with the same generator
    from torch.utils.data import random_split
    tr, va = load_split_data(pth=str(root), train_ratio=0.6, generator=torch.Generator().manual_seed(5))
    rtr, rva = random_split(range(7), [4, 3], generator=torch.Generator().manual_seed(5))
    assert list(tr.indices) == list(rtr.indices) and list(va.indices) == list(rva.indices)
    torch.manual_seed(11)
    tr, _ = load_split_data(pth=str(root))                            # the global generator by default
    torch.manual_seed(11)
    assert list(tr.indices) == list(random_split(range(7), [5, 2])[0].indices)
    with pytest.raises(FileNotFoundError, match="oxford-iiit-pet"):
        download_data(pth=str(tmp_path / "nowhere"))
    with pytest.raises(FileNotFoundError):
        load_split_data(pth=None)


def test_metric_arithmetic_reproduces_the_reference_on_host_counts(golden):
    """The host half of evaluate_model (metrics_from_counts) on counts taken with numpy equals the reference body's result."""
    from weaklysuperviseddl_amd.FullySupervisedModel.SupervisedModel import metrics_from_counts
    g = golden("supervised_eval")
    for name, C in (("c2", 2), ("c3", 3)):
        logits, labels, sizes = g[f"{name}/logits"], g[f"{name}/labels"], g[f"{name}/sizes"]
        rows, pixels, s = [], [], 0
        for B in sizes:
            rows.append(numpy_counts(logits[s:s + B], labels[s:s + B]))
            pixels.append(labels[s:s + B].size)
            s += B
        acc, iou = metrics_from_counts(np.stack(rows), pixels, C)
        assert iou == g[f"{name}/result"][1] and acc == g[f"{name}/result"][0], name


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 3, 21, 64])
@pytest.mark.parametrize("B,H,W", [(1, 224, 224), (5, 37, 29), (16, 32, 48)])
def test_count_kernel_against_numpy(dev, C, B, H, W):
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(C * 1000 + B)
    logits = (torch.randint(-3, 4, (B, C, H, W), generator=g).float() / 2)          # many exact ties
    logits[torch.rand(B, C, H, W, generator=g) < 0.01] = float("nan")
    labels = torch.randint(-1, C + 2, (B, H, W), generator=g)                       # -1 and >= C included
    want = numpy_counts(logits.numpy(), labels.numpy())
    ld, yd = logits.to(dev), labels.to(dev)
    got = ops.seg_counts(ld, yd)
    again = ops.seg_counts(ld, yd)
    assert np.array_equal(got.cpu().numpy(), want) and torch.equal(got, again)
    row = torch.full((3 * C + 1,), 7, dtype=torch.int64, device=dev)
    ops.seg_counts(ld, yd, out=row, accumulate=True)
    ops.seg_counts(ld, yd, out=row, accumulate=True)
    assert np.array_equal(row.cpu().numpy(), 2 * want + 7)
    ops.seg_counts(ld, yd, out=row, accumulate=False)
    assert np.array_equal(row.cpu().numpy(), want)
    # logits that do not start on a 16-byte boundary take the scalar path
    buf = torch.empty(ld.numel() + 1, device=dev)
    shifted = buf[1:].view(ld.shape)
    shifted.copy_(ld)
    assert np.array_equal(ops.seg_counts(shifted, yd).cpu().numpy(), want)


@pytest.mark.gpu
def test_count_kernel_refuses_unsupported_classes(dev):
    from weaklysuperviseddl_amd import ops, WsdlError
    for C in (1, 65):
        with pytest.raises(WsdlError, match="2 <= C <= 64"):
            ops.seg_counts(torch.zeros(2, C, 8, 8, device=dev), torch.zeros(2, 8, 8, dtype=torch.int64, device=dev))
    with pytest.raises(WsdlError, match="int64"):
        ops.seg_counts(torch.zeros(2, 2, 8, 8, device=dev), torch.zeros(2, 8, 8, dtype=torch.int32, device=dev))


class _StubModel(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, images):
        return {"out": self.logits[int(images[0])]}


@pytest.mark.gpu
def test_evaluate_model_equals_the_reference_golden(dev, golden):
    from weaklysuperviseddl_amd.FullySupervisedModel import evaluate_model
    g = golden("supervised_eval")
    for name, C in (("c2", 2), ("c3", 3)):
        logits, labels, sizes = g[f"{name}/logits"], g[f"{name}/labels"], g[f"{name}/sizes"]
        per, loader, s = [], [], 0
        for k, B in enumerate(sizes):
            per.append(torch.from_numpy(logits[s:s + B]).to(dev))
            loader.append((torch.full((B,), k, device=dev), torch.from_numpy(labels[s:s + B]).to(dev)))
            s += B
        acc, iou = evaluate_model(_StubModel(per), loader, dev, num_classes=C)
        ref_acc, ref_iou = g[f"{name}/result"]
        assert iou == ref_iou, (name, iou, ref_iou)
        assert abs(acc - ref_acc) <= np.spacing(np.float32(ref_acc)), (name, acc, ref_acc)


def _aux_less(dev, seed):
    from weaklysuperviseddl_amd.FullySupervisedModel.SupervisedModel import initialize_model
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    torch.manual_seed(seed)
    model = initialize_model(2, device=dev).train()
    return model, make_optimizer(model, lr=1e-4)


@pytest.mark.gpu
def test_planned_step_on_the_aux_less_model_is_bit_identical_to_eager(dev):
    """Four train_one_epoch-style steps (train_step with nn.CrossEntropyLoss) planned and eager: identical losses,
    parameters, Adam moments and BatchNorm buffers; the planned run really replayed."""
    from weaklysuperviseddl_amd import plan
    from weaklysuperviseddl_amd.TraditionalModel import train_step
    crit = torch.nn.CrossEntropyLoss()
    gen = torch.Generator().manual_seed(2)
    batches = [((torch.rand(4, 3, 64, 64, generator=gen)).to(dev), (torch.rand(4, 64, 64, generator=gen) > 0.5).long().to(dev))
               for _ in range(2)]

    def run(planned):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            model, opt = _aux_less(dev, 0)
            torch.manual_seed(1234)
            losses = [float(train_step(model, opt, *batches[i % 2], criterion=crit)) for i in range(4)]
            torch.cuda.synchronize()
            st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
            state = [opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [b.clone() for b in model.buffers()]
            return losses, state, st
        finally:
            plan.PLAN_STEP[0] = old

    l0, s0, _ = run(False)
    l1, s1, st = run(True)
    assert st is not None and st.disabled is None, getattr(st, "disabled", "no planned step")
    assert st.replays >= 1, (st.records, st.replays)
    assert l0 == l1
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))


@pytest.mark.gpu
def test_run_supervised_training_end_to_end(dev, tmp_path):
    from weaklysuperviseddl_amd.FullySupervisedModel import SupervisedModel as sm
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DeviceLoader
    root = make_pet_tree(tmp_path / "data", 33, 9, seed=3)
    save = tmp_path / "model.pth"
    lines = []
    res = sm.run_supervised_training(str(root), num_epochs=2, batch_size=8, train_ratio=0.85, device=dev,
                                     save_path=str(save), seed=0, log=lines.append)
    nums = [res["train_loss"], res["val_pixel_acc"], res["val_iou"]] + res["test_pixel_accs"] + res["test_ious"]
    assert all(np.isfinite(v) for v in nums), res
    assert res["test_pixel_accs"][0] == res["test_pixel_accs"][2] and res["test_ious"][0] == res["test_ious"][2]
    assert lines[0] == "Train batches: 4 | Val batches: 1 | Test batches: 2"    # 28 train (8,8,8,4), 5 val, 9 test
    model = sm.initialize_model(2, device=dev)
    model.load_state_dict(torch.load(save, map_location=dev), strict=True)

    # the loaders: labels = (trimap == 1), images = ToTensor's values; a trailing single image is skipped in training only
    from weaklysuperviseddl_amd.TraditionalModel.ExtraUtilities import download_data
    tr, va, te = sm.get_dataloaders(str(root), 0.85, 8, device=dev, generator=torch.Generator().manual_seed(0), log=None)
    ds = download_data(str(root), "test")
    images, labels = next(iter(te))
    for i in range(8):
        x, (_c, m) = ds[i]
        assert torch.equal(images[i].cpu(), x) and torch.equal(labels[i].cpu(), (m[0] == 1).long())
    assert images.dtype == torch.float32 and labels.dtype == torch.int64 and images.is_cuda
    single = DeviceLoader(te.dataset, 8, shuffle=True, drop_single=True)
    assert len(single) == 1 and [b[0].shape[0] for b in single] == [8]
    assert [b[0].shape[0] for b in te] == [8, 1]

    # overfitting one fixed batch for 20 planned steps lowers its CE loss
    images, labels = next(iter(tr))
    model, opt = _aux_less(dev, 1)
    crit = torch.nn.CrossEntropyLoss()
    fixed = [(images, labels)] * 20
    first = sm.train_one_epoch(model, fixed[:1], crit, opt, dev)
    sm.train_one_epoch(model, fixed[1:], crit, opt, dev)
    last = sm.train_one_epoch(model, fixed[:1], crit, opt, dev)
    st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
    assert st is not None and st.disabled is None and st.replays > 10, getattr(st, "disabled", None)
    assert last < first, (first, last)
    report_line(f"supervised baseline, 33+9 synthetic Pet images, 2 epochs: train loss {res['train_loss']:.4f}, test "
                f"acc {res['test_pixel_acc']:.4f}, mIoU {res['test_iou']:.4f}; fixed batch CE {first:.4f} -> {last:.4f} in 20 steps")
