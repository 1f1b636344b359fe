#!/usr/bin/env python3
"""Generate tests/golden/supervised_eval.npz from the reference's own ``evaluate_model`` body
(FullySupervisedModel/SupervisedModel.py:44-83).

Runs ONLY in the build container (needs /root/reference).  The reference module cannot be imported (torchvision is missing),
so the FunctionDef is selected with ``ast`` (``make_golden.lift``) and run on the CPU with a stub model whose forward
returns fixed logits per batch.  The fixture holds only those inputs and the (pixel accuracy, mean IoU) the body returned.

    python tests/golden/make_supervised_golden.py

Cases (logits quantised to halves so that exact ties between classes are frequent):
  c2  C = 2, batches of 4, 4, 3 (a partial last batch), 16 x 24;
  c3  C = 3, batches of 3, 3, 2, 16 x 16; in the second batch class 2 is neither predicted nor labelled (IoU NaN, dropped
      by np.nanmean).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import lift  # noqa: E402

REF = "/root/reference/FullySupervisedModel/SupervisedModel.py"


class StubModel(nn.Module):
    """model(images)['out'] = the logits of batch images[0] (an index)."""

    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, images):
        return {"out": self.logits[int(images[0])]}


def case(C, sizes, H, W, seed, absent=None):
    g = torch.Generator().manual_seed(seed)
    logits, labels = [], []
    for k, B in enumerate(sizes):
        lg = torch.randint(-4, 5, (B, C, H, W), generator=g).float() / 2
        lb = torch.randint(0, C, (B, H, W), generator=g)
        if absent is not None and k == absent[0]:
            lg[:, absent[1]] = -10.0
            lb[lb == absent[1]] = 0
        logits.append(lg)
        labels.append(lb)
    return logits, labels


def main():
    ns = lift(REF, {"evaluate_model"})
    out = {}
    for name, C, sizes, H, W, seed, absent in (("c2", 2, (4, 4, 3), 16, 24, 0, None),
                                               ("c3", 3, (3, 3, 2), 16, 16, 1, (1, 2))):
        logits, labels = case(C, sizes, H, W, seed, absent)
        loader = [(torch.full((B,), k), lb) for k, (B, lb) in enumerate(zip(sizes, labels))]
        acc, iou = ns["evaluate_model"](StubModel(logits), loader, "cpu", num_classes=C)
        out[f"{name}/logits"] = torch.cat(logits).numpy()
        out[f"{name}/labels"] = torch.cat(labels).numpy()
        out[f"{name}/sizes"] = np.array(sizes, dtype=np.int64)
        out[f"{name}/result"] = np.array([acc, iou], dtype=np.float64)
        ties = int((torch.cat(logits).max(1).values.unsqueeze(1) == torch.cat(logits)).sum(1).gt(1).sum())
        print(f"{name}: pixel acc {acc!r}, mean IoU {iou!r}, tied pixels {ties}")
    path = os.path.join(HERE, "supervised_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
