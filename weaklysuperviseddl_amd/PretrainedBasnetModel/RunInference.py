"""BASNet saliency evaluation on the Oxford-IIIT Pet test split (reference PretrainedBasnetModel/RunInference.py), as functions.

The reference is a script that runs at import; here ``run_inference`` does what its lines 57-126 do, with one device forward per
``batch_size`` images and the per-image ``norm_pred`` + uint8 quantisation on the device (``ops.saliency_u8``).  The host keeps
what the reference does with PIL and numpy: the resize back to the image's size, the saliency PNG, the NEAREST trimap and the
metrics.
"""
import os

import numpy as np
import torch
from PIL import Image

from .. import ops
from ..TraditionalModel.SegmentationDataset import image_to_tensor
from .model import BASNet


def norm_pred(d):
    """(d - min) / (max - min + 1e-8) over the WHOLE tensor (the reference's batch is one image; ops.saliency_u8 normalises per
    image)."""
    ma = torch.max(d)
    mi = torch.min(d)
    return (d - mi) / (ma - mi + 1e-8)


def compute_metrics(pred_mask, gt_mask):
    """IoU and pixel accuracy of (pred_mask > 0.5) against (trimap == 1); IoU is 1 when the union is empty."""
    pred_bin = (pred_mask > 0.5).astype(np.uint8)
    gt_bin = (gt_mask == 1).astype(np.uint8)
    intersection = np.logical_and(pred_bin, gt_bin).sum()
    union = np.logical_or(pred_bin, gt_bin).sum()
    iou = intersection / union if union > 0 else 1.0
    accuracy = (pred_bin == gt_bin).sum() / pred_bin.size
    return iou, accuracy, pred_bin, gt_bin


def saliency_curve_metrics(pred, trimaps, bins=256):
    """The two numbers saliency papers report, for a batch of ``norm_pred`` maps ``pred`` (B,H,W) float32 in [0, 1] on the device
    against ``(trimaps == 1)`` (B,H,W): the maximum F-measure over ``bins + 1`` thresholds (beta^2 = 0.3, from the pooled
    precision and recall) and the mean absolute error, with the threshold that reaches the maximum.  One grouped histogram with
    sums and one curve launch on the device (``ops.score_histogram``, ``ops.threshold_curves``), the rest on the host copies of the
    counts.  Returns ``{"max_f", "mae", "best_threshold"}``; the MAE uses the maps' values truncated to 2^-24."""
    pred = pred.reshape((-1,) + tuple(pred.shape[-2:]))
    gt = (trimaps.reshape(pred.shape) == 1).long()
    counts, sums = ops.score_histogram(pred, gt, bins=bins, range=(0.0, 1.0), num_groups=2, per_image=False, want_sums=True)
    curves = ops.threshold_curves(counts).cpu().numpy()
    f, k = ops.max_fbeta(curves, beta2=0.3)
    return {"max_f": f, "mae": ops.mae_from_sums(counts, sums), "best_threshold": float(ops.uniform_edges(0.0, 1.0, bins)[k])}


def run_inference(model_path='./Weights/basnet.pth', dataset_root='./OxfordIIITPetDataset/oxford-iiit-pet',
                  output_folder='./basnet_outputs', n_images=10, batch_size=10, device='cuda', net=None, verbose=True):
    """-> (per-image results [(name, iou, acc)], mean IoU, mean pixel accuracy); writes ``{name}_saliency.png``."""
    image_folder = os.path.join(dataset_root, 'images')
    trimap_folder = os.path.join(dataset_root, 'annotations', 'trimaps')
    test_txt = os.path.join(dataset_root, 'annotations', 'test.txt')
    os.makedirs(output_folder, exist_ok=True)
    device = torch.device(device)
    if net is None:
        net = BASNet(3, 1)
        net.load_state_dict(torch.load(model_path, map_location='cpu'))
        net.to(device)
    net.eval()

    with open(test_txt, 'r') as f:
        names = [line.strip().split(' ')[0] for line in f.readlines()[:n_images]]

    results = []
    for i in range(0, len(names), batch_size):
        chunk = names[i:i + batch_size]
        images = [Image.open(os.path.join(image_folder, f"{n}.jpg")).convert('RGB') for n in chunk]
        batch = torch.stack([image_to_tensor(im, (256, 256)) for im in images]).to(device)
        with torch.no_grad():
            d1 = net(batch)[0]
            pred_u8 = ops.saliency_u8(d1).cpu().numpy()           # (B,256,256): (norm_pred(d1) * 255).astype(uint8)
        for fname, image, pred_img in zip(chunk, images, pred_u8):
            saliency = Image.fromarray(pred_img).resize(image.size)
            pred_resized = np.array(saliency) / 255.0
            saliency.save(os.path.join(output_folder, f"{fname}_saliency.png"))
            gt_mask = Image.open(os.path.join(trimap_folder, f"{fname}.png"))
            gt_mask_np = np.array(gt_mask.resize(image.size, resample=Image.NEAREST))
            iou, acc, _, _ = compute_metrics(pred_resized, gt_mask_np)
            if verbose:
                print(f"{fname} - IoU: {iou:.4f}, Pixel Accuracy: {acc:.4f}")
            results.append((fname, iou, acc))

    mean_iou = sum(r[1] for r in results) / len(results)
    mean_acc = sum(r[2] for r in results) / len(results)
    if verbose:
        print(f"Mean IoU: {mean_iou:.4f}, Mean Pixel Accuracy: {mean_acc:.4f}")
    return results, mean_iou, mean_acc
