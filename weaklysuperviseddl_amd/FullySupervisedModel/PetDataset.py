"""Oxford-IIIT Pet held on the device for the fully-supervised baseline (reference FullySupervisedModel/SupervisedModel.py).

The reference re-decodes and re-resizes every JPEG with PIL on one host thread in every epoch (``DataLoader(...,
num_workers=0)``).  Its pipeline has no augmentation, so the decoded, resized dataset is the same in every epoch: here it is
built once - decoded on a host thread pool (at most 16 workers) - and kept on the device as uint8 (images (N,3,224,224),
raw trimaps (N,224,224), categories (N,)): about 740 MB for trainval.  An augmentation the reference does not have is opt-in:
``DeviceLoader(..., augment=Augment(...))`` warps image and label together in the launch that gathers the batch
(``ops.augment_batch``), so the resident tensors stay what they are.

Batches are ``(images float32 (B,3,224,224), labels int64 (B,224,224))`` on the device:
  images = uint8 / 255 through a 256-entry table computed the way ToTensor computes it (bit-identical to the reference's
           items);
  labels = (trimap == 1): foreground = pet.  The reference hands the raw (B,1,H,W) uint8 trimap {1,2,3} to
           nn.CrossEntropyLoss, which rejects it; its model is a binary one (``deeplabv3_resnet50_binary_segmentation``).
           The binarisation is the "modular" convention the package already evaluates the weakly-supervised model with
           (``SegmentationModel.evaluate_model(binarize="modular")``), so the two numbers are comparable.
"""
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MAX_WORKERS = 16
_CHUNK = 256          # images decoded per host -> device copy
_CHUNK_BYTES = 64 << 20     # resize="device": raw bytes per host -> device copy (Pet has images of several megapixels)
_CHUNK_ITEMS = 2048         # ... and items per copy at most (their descriptors travel behind the pixels)


def _to_float_table():
    # ToTensor: uint8 -> float32, then .div(255)
    return torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)


class DevicePetDataset:
    """The items of an ``ExtraUtilities.OxfordIIITPetLocal`` as uint8 device tensors, decoded once."""

    def __init__(self, source, device="cuda", workers=MAX_WORKERS, *, resize="host", chunk_bytes=_CHUNK_BYTES):
        """``resize="host"``: every item is decoded AND resized by PIL on the pool (``source.load_u8``).
        ``resize="device"``: the pool only decodes (``source.load_raw``); the raw pixels of a chunk - at most ``chunk_bytes``
        - are packed into one of two pinned staging buffers, copied once and resized straight into ``images`` / ``trimaps``
        by ``ops.pil_resize`` (Pillow's BICUBIC bit for bit), while the pool decodes the next chunk.  The same tensors
        either way."""
        if resize not in ("host", "device"):
            raise ValueError(f"resize {resize!r}: 'host' or 'device'")
        n = len(source)
        self.device = torch.device(device)
        self.images = torch.empty(n, 3, 224, 224, dtype=torch.uint8, device=self.device)
        self.trimaps = torch.empty(n, 224, 224, dtype=torch.uint8, device=self.device)
        categories = np.empty(n, dtype=np.int64)
        self._table = _to_float_table().to(self.device)
        workers = max(1, min(int(workers), MAX_WORKERS))
        with ThreadPoolExecutor(max_workers=workers) as ex:
            if resize == "device":
                self._build_on_device(source, ex, workers, int(chunk_bytes), categories)
            else:
                for s in range(0, n, _CHUNK):
                    items = list(ex.map(source.load_u8, range(s, min(n, s + _CHUNK))))
                    img = torch.from_numpy(np.stack([it[0] for it in items])).permute(0, 3, 1, 2)
                    tri = torch.from_numpy(np.stack([it[2] for it in items]))
                    self.images[s:s + len(items)].copy_(img)
                    self.trimaps[s:s + len(items)].copy_(tri)
                    categories[s:s + len(items)] = [it[1] for it in items]
        self.categories = torch.from_numpy(categories).to(self.device)

    def _build_on_device(self, source, ex, workers, chunk_bytes, categories):
        from .. import ops
        n = len(source)
        item = ops.PIL_IMAGE_DTYPE.itemsize
        tail = 8 + 2 * _CHUNK_ITEMS * item                     # alignment + the descriptors of a full chunk
        state = {"cap": 0, "stage": None, "dev": None, "events": [None, None]}

        def allocate(cap):
            for ev in state["events"]:
                if ev is not None:
                    ev.synchronize()
            state["cap"] = cap
            state["stage"] = [torch.empty(cap + tail, dtype=torch.uint8).pin_memory() for _ in range(2)]
            state["views"] = [t.numpy() for t in state["stage"]]
            state["dev"] = torch.empty(cap + tail, dtype=torch.uint8, device=self.device)
            state["events"] = [None, None]

        allocate(max(1, chunk_bytes))
        which, used, first = 0, 0, 0
        shapes = ([], [])            # (h, w) of the chunk's images / trimaps
        offsets = ([], [])

        def flush():
            nonlocal which, used, first
            m = len(shapes[0])
            if m == 0:
                return
            desc = np.concatenate([ops.pil_describe(shapes[k], offsets[k], (224, 224), ops.PIL_BICUBIC, self.device)
                                   for k in range(2)])
            d0 = (used + 7) // 8 * 8
            total = d0 + desc.nbytes
            state["views"][which][d0:total] = desc.view(np.uint8)
            dev = state["dev"]
            with torch.cuda.device(self.device):
                dev[:total].copy_(state["stage"][which][:total], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                state["events"][which] = ev
                ops.pil_resize(dev, dev[d0:d0 + m * item], 3, (224, 224), out=self.images[first:first + m])
                ops.pil_resize(dev, dev[d0 + m * item:total], 1, (224, 224), out=self.trimaps[first:first + m])
            first += m
            which, used = 1 - which, 0
            for k in range(2):
                shapes[k].clear()
                offsets[k].clear()
            if state["events"][which] is not None:            # the buffer about to be filled: its copy must have left
                state["events"][which].synchronize()

        pending, order = deque(), iter(range(n))

        def submit():
            i = next(order, None)
            if i is not None:
                pending.append(ex.submit(source.load_raw, i))

        for _ in range(4 * workers):
            submit()
        i = 0
        while pending:
            img, category, tri = pending.popleft().result()
            submit()
            need = img.nbytes + tri.nbytes
            if used + need > state["cap"] or len(shapes[0]) == _CHUNK_ITEMS:
                flush()
            if need > state["cap"]:                             # one item larger than the bound: the buffers grow to hold it
                torch.cuda.synchronize(self.device)
                allocate(need)
                which = 0
            view = state["views"][which]
            for k, a in enumerate((img, tri)):
                view[used:used + a.nbytes] = a.reshape(-1)
                shapes[k].append(a.shape[:2])
                offsets[k].append(used)
                used += a.nbytes
            categories[i] = category
            i += 1
        flush()
        torch.cuda.synchronize(self.device)                     # the staging buffers go away with this frame

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
    The training loader sets it; evaluation keeps every image.

    ``augment``: an ``augment.Augment`` (default None: the plain batches above, nothing else is imported or called).  A
    batch is then ONE launch, ``ops.augment_batch``: the gather, the uint8 -> float table, the joint warp of image and
    label, the photometric map and the ``trimap == 1`` mapping; padded pixels carry ``augment.pad_label``.  The parameters
    of a whole epoch are drawn from ``generator`` (after the epoch's order) and uploaded when the iteration starts; the
    identity augmentation yields the plain batches bit for bit."""

    def __init__(self, dataset, batch_size, indices=None, shuffle=False, generator=None, drop_single=False, augment=None):
        self.dataset, self.batch_size = dataset, int(batch_size)
        n = len(dataset)
        self.indices = torch.as_tensor(list(range(n)) if indices is None else list(indices), dtype=torch.int64)
        self.shuffle, self.generator, self.drop_single = shuffle, generator, drop_single
        self.augment = augment
        self._tables = None

    def _augment_tables(self):
        """(the dataset's float table per channel (3,256), the label table: 1 -> 1, else 0), made once."""
        if self._tables is None:
            ds = self.dataset
            label_lut = torch.zeros(256, dtype=torch.int64)
            label_lut[1] = 1
            self._tables = (ds._table.view(1, 256).repeat(3, 1).contiguous(), label_lut.to(ds.device))
        return self._tables

    def __len__(self):
        n, r = divmod(len(self.indices), self.batch_size)
        return n + (1 if r > (1 if self.drop_single and self.batch_size > 1 else 0) else 0)

    def __iter__(self):
        idx = self.indices
        if self.shuffle:
            idx = idx[torch.randperm(len(idx), generator=self.generator)]
        idx = idx.to(self.dataset.device)
        aug, ds = self.augment, self.dataset
        if aug is not None:
            lut, label_lut = self._augment_tables()
            params = aug.epoch_params(len(idx), ds.images.shape[-2:], ds.device, self.generator)
        for s in range(0, len(self.indices), self.batch_size):
            part = idx[s:s + self.batch_size]
            if self.drop_single and part.numel() == 1 and self.batch_size > 1:
                continue
            if aug is None:
                yield ds.batch(part)
            else:
                yield aug.apply(ds.images, ds.trimaps, part, params[s:s + self.batch_size], lut=lut, label_lut=label_lut)


class DeviceItemLoader:
    """``DataLoader(download_data(...), batch_size)`` over a ``DevicePetDataset``: yields what that loader collates -
    ``(images float32 (B,3,224,224), (categories int64 (B,), trimaps uint8 (B,1,224,224)))`` - from the resident tensors,
    so ``generate_pseudo_masks``, ``train_fc_only(dataloader=)``, ``evaluate_classification`` and
    ``evaluate_layercam_on_test_set`` run on real data without touching PIL after the dataset's one pass.  ``indices``,
    ``shuffle`` and ``generator`` as ``DeviceLoader``; the last partial batch is kept, as DataLoader keeps it."""

    def __init__(self, dataset, batch_size, indices=None, shuffle=False, generator=None):
        self.dataset, self.batch_size = dataset, int(batch_size)
        if self.batch_size < 1:
            raise ValueError(f"batch_size {batch_size}")
        n = len(dataset)
        self.indices = torch.as_tensor(list(range(n)) if indices is None else list(indices), dtype=torch.int64)
        self.shuffle, self.generator = shuffle, generator

    def __len__(self):
        return (len(self.indices) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        ds = self.dataset
        idx = self.indices
        if self.shuffle:
            idx = idx[torch.randperm(len(idx), generator=self.generator)]
        idx = idx.to(ds.images.device)
        for s in range(0, len(idx), self.batch_size):
            part = idx[s:s + self.batch_size]
            images = ds._table[ds.images[part].to(torch.int32)]
            yield images, (ds.categories[part], ds.trimaps[part].unsqueeze(1))
