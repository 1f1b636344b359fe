"""The fully-supervised upper bound (reference FullySupervisedModel/SupervisedModel.py): DeepLabV3-ResNet50 trained on the
Oxford-IIIT Pet ground-truth masks, evaluated by pixel accuracy and mean IoU - the number every weakly-supervised result is
compared with.  Same functions and positional signatures; extras are keyword-only.

Where the reference's text cannot run, these decisions replace it:
  * items: ``download_data`` yields ``(image, (category, mask))`` but ``train_one_epoch`` unpacks ``(images, masks)``, and
    the mask is a (B,1,H,W) uint8 trimap {1,2,3} that CrossEntropyLoss rejects.  ``get_dataloaders`` yields
    ``(images, labels)`` with labels = (trimap == 1) int64 (B,H,W), foreground = pet (``PetDataset``);
  * ``random_split`` is not imported by the reference: ``ExtraUtilities.load_split_data`` imports it;
  * the ImageNet backbone torchvision would download is not reproduced: ``initialize_model`` initialises at random unless
    ``backbone_state_dict`` (torchvision ResNet-50 keys) is given.  The reference calls ``deeplabv3_resnet50(weights=None)``,
    whose default ``weights_backbone`` is the ImageNet one.

On the device: the dataset is decoded once and kept as uint8 (``PetDataset``); a training iteration is ``train_step`` (one
host call per step when the optimiser comes from ``make_optimizer``), the loss sum stays on the device until the epoch
ends; evaluation writes one row of integer counts per batch (``ops.seg_counts``, csrc/seg_metrics.hip) and reads them all
back once, where the reference reads 1 + 2C values per batch.
"""
import numpy as np
import torch
import torch.nn as nn

from ..TraditionalModel.ExtraUtilities import download_data, load_split_data
from ..TraditionalModel.SegmentationModel import SegmentationModel, make_optimizer, train_step
from .. import ops
from .PetDataset import DeviceLoader, DevicePetDataset

SAVE_PATH = "deeplabv3_resnet50_binary_segmentation.pth"


def _device(device):
    return torch.device("cuda" if device is None else device)


def initialize_model(num_classes=2, device=None, *, backbone_state_dict=None):
    """Reference ``initialize_model(num_classes=2, device=None)`` (SupervisedModel.py:13-16): torchvision's
    ``deeplabv3_resnet50(weights=None, num_classes=num_classes)`` - backbone.* and classifier.0-4.*, no aux head.
    ``backbone_state_dict``: a ResNet-50 state_dict with torchvision's keys (or a path to one; ``fc.*`` is ignored) loaded
    into the backbone; without it the backbone is initialised at random.  ``device=None`` means "cuda"."""
    model = SegmentationModel(num_classes=num_classes, aux_loss=False)
    if backbone_state_dict is not None:
        sd = backbone_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu")
        model.backbone.load_state_dict({k: v for k, v in sd.items() if not k.startswith("fc.")}, strict=True)
    return model.to(_device(device))


def get_dataloaders(data_path='./data', train_ratio=0.85, batch_size=16, num_workers=0, *, device=None, generator=None,
                    log=print, resize="host", augment=None):
    """Reference ``get_dataloaders(data_path='./data', train_ratio=0.85, batch_size=16, num_workers=0)``
    (SupervisedModel.py:18-27): the train / val split of 'trainval' (``load_split_data``) and 'test', as device loaders
    (``PetDataset.DeviceLoader``) over datasets decoded once.  ``num_workers`` is accepted and unused (the decode runs on a
    host thread pool of at most 16 workers, once).  ``generator``: the split's and the train loader's shuffling generator
    (default torch's global one, as the reference).  ``resize``: "host" (PIL resizes on the pool) or "device"
    (``DevicePetDataset(resize="device")``: the pool only decodes); the same tensors either way.  ``augment``: an
    ``augment.Augment`` for the TRAIN loader only (``DeviceLoader(augment=)``; the reference has none); validation and test
    are never augmented."""
    dev = _device(device)
    train_subset, val_subset = load_split_data(pth=data_path, train_ratio=train_ratio, generator=generator)
    trainval = DevicePetDataset(train_subset.dataset, device=dev, resize=resize)
    test = DevicePetDataset(download_data(pth=data_path, split='test'), device=dev, resize=resize)
    train_loader = DeviceLoader(trainval, batch_size, indices=train_subset.indices, shuffle=True, generator=generator,
                                drop_single=True, augment=augment)
    val_loader = DeviceLoader(trainval, batch_size, indices=val_subset.indices)
    test_loader = DeviceLoader(test, batch_size)
    if log:
        log(f"Train batches: {len(train_loader)} | Val batches: {len(val_loader)} | Test batches: {len(test_loader)}")
    return train_loader, val_loader, test_loader


def train_one_epoch(model, dataloader, criterion, optimizer, device):
    """Reference ``train_one_epoch`` (SupervisedModel.py:29-42): returns the mean loss over the batches trained.  Each
    iteration is ``train_step(..., criterion=criterion)``; the losses are summed in a float64 device scalar and read once."""
    model.train()
    dev = _device(device)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    n = 0
    for images, masks in dataloader:
        images, masks = images.to(dev), masks.to(dev)
        total += train_step(model, optimizer, images, masks.long(), criterion=criterion)
        n += 1
    return total.item() / n


def metrics_from_counts(counts, pixels, num_classes):
    """The reference's per-batch arithmetic (SupervisedModel.py:56-83) on rows of ``ops.seg_counts``: IoU per class =
    inter / union in float64, NaN when union == 0, ``np.nanmean`` per batch, the batch means averaged; pixel accuracy of a
    batch = correct / pixels as ``(preds == masks).float().mean()`` computes it (float32)."""
    C = num_classes
    total_pixel_acc, total_iou, num_batches = 0.0, 0.0, 0
    for row, npix in zip(np.asarray(counts), pixels):
        inter, npred, nlabel, correct = row[:C], row[C:2 * C], row[2 * C:3 * C], row[3 * C]
        total_pixel_acc += float(np.float32(correct) / np.float32(npix))
        ious = []
        for cls in range(C):
            intersection = int(inter[cls])
            union = int(npred[cls]) + int(nlabel[cls]) - intersection
            ious.append(float('nan') if union == 0 else intersection / union)
        total_iou += np.nanmean(ious)
        num_batches += 1
    return total_pixel_acc / num_batches, total_iou / num_batches


@torch.no_grad()
def evaluate_model(model, dataloader, device, num_classes=2):
    """Reference ``evaluate_model`` (SupervisedModel.py:44-83): returns (mean pixel accuracy, mean IoU) over the batches.
    The forward runs in eval mode; ``ops.seg_counts`` adds each batch's argmax counts to a row of its own on the device;
    after the loop one copy brings the rows to the host, where ``metrics_from_counts`` does the reference's arithmetic."""
    model.eval()
    dev = _device(device)
    C = int(num_classes)
    rows = torch.zeros(len(dataloader), 3 * C + 1, dtype=torch.int64, device=dev)
    pixels = []
    for i, (images, masks) in enumerate(dataloader):
        images, masks = images.to(dev), masks.to(dev).long()
        outputs = model(images)['out']
        ops.seg_counts(outputs, masks, out=rows[i], accumulate=True)
        pixels.append(masks.numel())
    host = rows[:len(pixels)].cpu().numpy()
    return metrics_from_counts(host, pixels, C)


def run_supervised_training(data_path='./data', num_epochs=10, batch_size=16, train_ratio=0.85, num_classes=2, lr=1e-4,
                            device=None, *, save_path=SAVE_PATH, seed=None, log=print, backbone_state_dict=None,
                            resize="host", augment=None, criterion=None, optimizer_kind="adam",
                            optimizer_kwargs=None):
    """Reference ``run_supervised_training`` (SupervisedModel.py:85-122): Adam(lr) (``make_optimizer``) on CrossEntropy,
    validation after every epoch, the final state_dict saved to ``save_path`` (None: not saved), then three evaluations
    of the test split.  ``seed`` seeds torch's global generator first (split, shuffling, initialisation).  Returns the
    final numbers as a dict (the reference returns None).  ``resize``, ``augment``: see ``get_dataloaders`` (the padding of
    ``fill="ignore"`` carries -100, which the CrossEntropyLoss below ignores).  ``criterion``: the loss object instead of
    the reference's ``nn.CrossEntropyLoss()`` - one with class weights, or a ``weaklysuperviseddl_amd.nn.CrossEntropyLoss``
    (label smoothing, pixel weights); see ``SegmentationModel.resolve_criterion``.  ``optimizer_kind`` / ``optimizer_kwargs``:
    ``make_optimizer``'s ``kind`` and keyword arguments - the DeepLabV3 recipe is ``optimizer_kind="sgd",
    optimizer_kwargs=dict(momentum=0.9, weight_decay=1e-4)``; the default is the reference's Adam(lr)."""
    dev = _device(device)
    if seed is not None:
        torch.manual_seed(seed)
    say = log or (lambda *a: None)
    train_loader, val_loader, test_loader = get_dataloaders(data_path, train_ratio, batch_size, device=dev, log=log, resize=resize,
                                                            augment=augment)
    model = initialize_model(num_classes=num_classes, device=dev, backbone_state_dict=backbone_state_dict)
    if criterion is None:
        criterion = nn.CrossEntropyLoss()
    optimizer = make_optimizer(model, lr=lr, kind=optimizer_kind, **(optimizer_kwargs or {}))

    train_loss = val_acc = val_iou = float('nan')
    for epoch in range(num_epochs):
        say(f"\nEpoch {epoch + 1}/{num_epochs}")
        train_loss = train_one_epoch(model, train_loader, criterion, optimizer, dev)
        val_acc, val_iou = evaluate_model(model, val_loader, dev, num_classes)
        say(f"Train Loss: {train_loss:.4f} | Val Acc: {val_acc:.4f} | Val IoU: {val_iou:.4f}")

    if save_path is not None:
        torch.save(model.state_dict(), save_path)

    test_runs = 3
    pixel_accs, ious = [], []
    for run in range(test_runs):
        say(f"\nTest Run {run + 1}/{test_runs}")
        pixel_acc, iou = evaluate_model(model, test_loader, dev, num_classes)
        pixel_accs.append(pixel_acc)
        ious.append(iou)
        say(f"Pixel Acc: {pixel_acc:.4f} | IoU: {iou:.4f}")

    say("\nFinal Test Results:")
    say(f"Avg Pixel Acc: {np.mean(pixel_accs):.4f} ± {np.std(pixel_accs):.4f}")
    say(f"Avg IoU: {np.mean(ious):.4f} ± {np.std(ious):.4f}")
    return {"train_loss": train_loss, "val_pixel_acc": val_acc, "val_iou": val_iou, "test_pixel_accs": pixel_accs,
            "test_ious": ious, "test_pixel_acc": float(np.mean(pixel_accs)), "test_iou": float(np.mean(ious))}
