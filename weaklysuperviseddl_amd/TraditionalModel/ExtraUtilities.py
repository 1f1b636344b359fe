"""Host-side helpers of reference TraditionalModel/ExtraUtilities.py: ``compute_iou_and_acc`` (:4-21) and the Oxford-IIIT Pet
reader ``download_data`` / ``load_split_data`` (:24-63).

The reference builds torchvision's ``OxfordIIITPet(..., download=True)``.  This package never downloads: the reader opens a
local tree in torchvision's layout and raises ``FileNotFoundError`` when it is missing.  Its items are what the reference's
dataset yields, bit for bit: ``(image, (category, mask))`` with
  image  ``Image.open(...).convert("RGB")`` -> Resize((224, 224), BICUBIC) -> ToTensor: (3,224,224) float32 = uint8 / 255
         (no Normalize: the reference has none),
  mask   the trimap as opened (values 1 pet, 2 background, 3 border) -> Resize((224, 224), BICUBIC) -> PILToTensor:
         (1,224,224) uint8,
  category = class id - 1 from ``annotations/{split}.txt``.
torchvision itself is not needed: on PIL images its Resize is ``Image.resize`` and ToTensor / PILToTensor are array copies.
"""
import os

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

SIZE = (224, 224)
LAYOUT = ("{root}/oxford-iiit-pet/images/{id}.jpg, {root}/oxford-iiit-pet/annotations/trimaps/{id}.png and "
          "{root}/oxford-iiit-pet/annotations/{trainval,test}.txt ('id class species breed' lines)")


def compute_iou_and_acc(pred_mask, true_mask):
    pred_fg, true_fg = pred_mask > 0, true_mask > 0
    inter = (pred_fg & true_fg).sum().item()
    union = (pred_fg | true_fg).sum().item()
    correct = (pred_mask == true_mask).sum().item()
    return inter / (union + 1e-8), correct / true_mask.numel()


class OxfordIIITPetLocal(Dataset):
    """torchvision ``OxfordIIITPet(root, split, target_types=("category", "segmentation"))`` over an existing tree, with
    the reference's transforms.  ``load_u8(i)`` is the same item before the float conversion: (image (224,224,3) uint8,
    category, trimap (224,224) uint8) - what the device-resident dataset keeps; ``load_raw(i)`` is it before the resize."""

    def __init__(self, root, split="test"):
        if split not in ("trainval", "test"):
            raise ValueError(f"split {split!r}: 'trainval' or 'test'")
        if root is None:
            raise FileNotFoundError("Oxford-IIIT Pet: no root given (this package never downloads); expected " + LAYOUT)
        base = os.path.join(os.fspath(root), "oxford-iiit-pet")
        self.root, self.split = os.fspath(root), split
        self._images_dir = os.path.join(base, "images")
        self._trimaps_dir = os.path.join(base, "annotations", "trimaps")
        listing = os.path.join(base, "annotations", f"{split}.txt")
        if not (os.path.isdir(self._images_dir) and os.path.isdir(self._trimaps_dir) and os.path.isfile(listing)):
            raise FileNotFoundError(f"Oxford-IIIT Pet not found under {root!r} (this package never downloads); expected "
                                    + LAYOUT)
        self.ids, self._labels = [], []
        with open(listing) as f:
            for line in f:
                image_id, label, *_ = line.strip().split()
                self.ids.append(image_id)
                self._labels.append(int(label) - 1)
        self._images = [os.path.join(self._images_dir, f"{i}.jpg") for i in self.ids]
        self._segs = [os.path.join(self._trimaps_dir, f"{i}.png") for i in self.ids]

    def __len__(self):
        return len(self.ids)

    def load_u8(self, idx):
        image = Image.open(self._images[idx]).convert("RGB").resize((SIZE[1], SIZE[0]), Image.BICUBIC)
        mask = Image.open(self._segs[idx]).resize((SIZE[1], SIZE[0]), Image.BICUBIC)
        img = np.array(image, dtype=np.uint8)
        tri = np.array(mask, copy=True)
        if img.shape != (SIZE[0], SIZE[1], 3) or tri.shape != SIZE or tri.dtype != np.uint8:
            raise ValueError(f"{self._segs[idx]}: an 8-bit single-channel trimap expected (mode {mask.mode})")
        return img, self._labels[idx], tri

    def load_raw(self, idx):
        """The item before any resize: (image H x W x 3 uint8 after ``convert("RGB")``, category, trimap h x w uint8) - what
        the device resize (``ops.pil_resize``, BICUBIC to 224x224) turns into ``load_u8``'s item.  A trimap that is not mode
        "L" (Pillow forces NEAREST for "P" and "1") is resized on the host as ``load_u8`` does and handed on at 224x224,
        which the device resize passes through unchanged."""
        img = np.array(Image.open(self._images[idx]).convert("RGB"), dtype=np.uint8)
        mask = Image.open(self._segs[idx])
        if mask.mode != "L":
            mask = mask.resize((SIZE[1], SIZE[0]), Image.BICUBIC)
        tri = np.array(mask, copy=True)
        if img.ndim != 3 or img.shape[2] != 3 or tri.ndim != 2 or tri.dtype != np.uint8:
            raise ValueError(f"{self._segs[idx]}: an 8-bit single-channel trimap expected (mode {mask.mode})")
        return img, self._labels[idx], tri

    def __getitem__(self, idx):
        img, category, tri = self.load_u8(idx)
        image = torch.from_numpy(img).permute(2, 0, 1).contiguous().to(torch.float32).div(255)     # ToTensor
        return image, (category, torch.from_numpy(tri).unsqueeze(0))                              # PILToTensor


def download_data(pth=None, split="test"):
    """Reference ``download_data(pth=None, split="test")`` (ExtraUtilities.py:24-41) over a local tree: nothing is
    downloaded; a missing tree raises ``FileNotFoundError``."""
    return OxfordIIITPetLocal(pth, split)


def load_split_data(pth=None, train_ratio=0.8, *, generator=None):
    """Reference ``load_split_data(pth=None, train_ratio=0.8)`` (ExtraUtilities.py:43-63): the 'trainval' split cut by
    ``random_split(full, [int(r * N), N - int(r * N)])`` (the reference calls it without importing it).  ``generator``:
    the split's generator (default: torch's global one, as the reference)."""
    from torch.utils.data import random_split
    assert 0 < train_ratio < 1, "train_ratio must be between 0 and 1 (exclusive)"
    full_dataset = download_data(pth=pth, split="trainval")
    total_size = len(full_dataset)
    train_size = int(train_ratio * total_size)
    val_size = total_size - train_size
    gen = generator if generator is not None else torch.default_generator
    train_dataset, val_dataset = random_split(full_dataset, [train_size, val_size], generator=gen)
    return train_dataset, val_dataset
