"""Oxford-IIIT Pet held on the device for the fully-supervised baseline (reference FullySupervisedModel/SupervisedModel.py).

The reference re-decodes and re-resizes every JPEG with PIL on one host thread in every epoch (``DataLoader(...,
num_workers=0)``).  Its pipeline has no augmentation, so the decoded, resized dataset is the same in every epoch: here it is
built once - decoded on a host thread pool (at most 16 workers) - and kept on the device as uint8 (images (N,3,224,224),
raw trimaps (N,224,224), categories (N,)): about 740 MB for trainval.

Batches are ``(images float32 (B,3,224,224), labels int64 (B,224,224))`` on the device:
  images = uint8 / 255 through a 256-entry table computed the way ToTensor computes it (bit-identical to the reference's
           items);
  labels = (trimap == 1): foreground = pet.  The reference hands the raw (B,1,H,W) uint8 trimap {1,2,3} to
           nn.CrossEntropyLoss, which rejects it; its model is a binary one (``deeplabv3_resnet50_binary_segmentation``).
           The binarisation is the "modular" convention the package already evaluates the weakly-supervised model with
           (``SegmentationModel.evaluate_model(binarize="modular")``), so the two numbers are comparable.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MAX_WORKERS = 16
_CHUNK = 256          # images decoded per host -> device copy


def _to_float_table():
    # ToTensor: uint8 -> float32, then .div(255)
    return torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)


class DevicePetDataset:
    """The items of an ``ExtraUtilities.OxfordIIITPetLocal`` as uint8 device tensors, decoded once."""

    def __init__(self, source, device="cuda", workers=MAX_WORKERS):
        n = len(source)
        self.device = torch.device(device)
        self.images = torch.empty(n, 3, 224, 224, dtype=torch.uint8, device=self.device)
        self.trimaps = torch.empty(n, 224, 224, dtype=torch.uint8, device=self.device)
        categories = np.empty(n, dtype=np.int64)
        self._table = _to_float_table().to(self.device)
        workers = max(1, min(int(workers), MAX_WORKERS))
        with ThreadPoolExecutor(max_workers=workers) as ex:
            for s in range(0, n, _CHUNK):
                items = list(ex.map(source.load_u8, range(s, min(n, s + _CHUNK))))
                img = torch.from_numpy(np.stack([it[0] for it in items])).permute(0, 3, 1, 2)
                tri = torch.from_numpy(np.stack([it[2] for it in items]))
                self.images[s:s + len(items)].copy_(img)
                self.trimaps[s:s + len(items)].copy_(tri)
                categories[s:s + len(items)] = [it[1] for it in items]
        self.categories = torch.from_numpy(categories).to(self.device)

    def __len__(self):
        return self.images.shape[0]

    def batch(self, idx):
        """(images float32 (B,3,224,224), labels int64 (B,224,224)) of the device index tensor ``idx``."""
        images = self._table[self.images[idx].to(torch.int32)]
        labels = (self.trimaps[idx] == 1).to(torch.int64)
        return images, labels


class DeviceLoader:
    """``DataLoader(subset, batch_size, shuffle)`` over a ``DevicePetDataset``: ``indices`` select the subset (a
    ``random_split`` Subset's), ``shuffle`` draws a new order every epoch with ``generator`` (torch's global generator when
    None, as DataLoader).  ``drop_single``: a trailing batch of ONE image is skipped, as ``InMemoryPseudoDataset.batches``
    does - train-mode BatchNorm in the ASPP pooling branch normalises one pooled value per channel and cannot take B = 1.
    The training loader sets it; evaluation keeps every image."""

    def __init__(self, dataset, batch_size, indices=None, shuffle=False, generator=None, drop_single=False):
        self.dataset, self.batch_size = dataset, int(batch_size)
        n = len(dataset)
        self.indices = torch.as_tensor(list(range(n)) if indices is None else list(indices), dtype=torch.int64)
        self.shuffle, self.generator, self.drop_single = shuffle, generator, drop_single

    def __len__(self):
        n, r = divmod(len(self.indices), self.batch_size)
        return n + (1 if r > (1 if self.drop_single and self.batch_size > 1 else 0) else 0)

    def __iter__(self):
        idx = self.indices
        if self.shuffle:
            idx = idx[torch.randperm(len(idx), generator=self.generator)]
        idx = idx.to(self.dataset.device)
        for s in range(0, len(self.indices), self.batch_size):
            part = idx[s:s + self.batch_size]
            if self.drop_single and part.numel() == 1 and self.batch_size > 1:
                continue
            yield self.dataset.batch(part)
