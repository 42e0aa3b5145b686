"""Instance-crop folder reader for stage 1 (u2seg/Instance_Clustering/selective_labeling/usl-imagenet.py:44-63 and
shared/utils/nn_utils_imagenet.py:411-430): torchvision's ``ImageFolder`` order and ``Resize(480)`` + ``CenterCrop(480)`` on
PIL images, yielding uint8 NHWC RGB batches; ``ToTensor`` + ``Normalize`` happen on the device (u2_vit_patchify).

torchvision is not a dependency: the folder order, the extension list, the resize-size rule and the crop offsets below are
restated from torchvision's documented behaviour (datasets/folder.py, transforms/functional.py) and are not pinned against a
torchvision run."""
import os

import numpy as np
import torch
from PIL import Image

# torchvision.datasets.folder.IMG_EXTENSIONS (matched case-insensitively)
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
MAX_WORKERS = 16


def find_classes(root):
    """Sorted names of the class directories under ``root`` -> (classes, {name: index})."""
    classes = sorted(entry.name for entry in os.scandir(root) if entry.is_dir())
    if not classes:
        raise FileNotFoundError("no class folder found in %s" % root)
    return classes, {c: i for i, c in enumerate(classes)}


def make_dataset(root, class_to_idx):
    """[(path, class index)] in ImageFolder's order: classes sorted, then ``sorted(os.walk(..., followlinks=True))`` and sorted
    file names within each directory."""
    out = []
    for cls in sorted(class_to_idx.keys()):
        d = os.path.join(root, cls)
        if not os.path.isdir(d):
            continue
        for sub, _, fnames in sorted(os.walk(d, followlinks=True)):
            for fname in sorted(fnames):
                path = os.path.join(sub, fname)
                if path.lower().endswith(IMG_EXTENSIONS):
                    out.append((path, class_to_idx[cls]))
    return out


def resize_size(w, h, size):
    """Resize(size) with an int size: the short side becomes ``size``, the long side ``int(size * long / short)`` -> (w, h)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


def center_crop_box(w, h, size):
    """CenterCrop(size) on an image at least ``size`` on both sides: PIL box (left, top, right, bottom)."""
    top = int(round((h - size) / 2.0))
    left = int(round((w - size) / 2.0))
    return left, top, left + size, top + size


def load_crop(path, size=480):
    """PIL convert("RGB") -> Resize(size, bilinear) -> CenterCrop(size) -> uint8 [size, size, 3]."""
    with open(path, "rb") as f:
        img = Image.open(f)
        img = img.convert("RGB")
    w, h = img.size
    nw, nh = resize_size(w, h, size)
    if (nw, nh) != (w, h):
        img = img.resize((nw, nh), Image.BILINEAR)
    if nw < size or nh < size:
        raise ValueError("%s: %dx%d after Resize(%d) is smaller than the crop" % (path, nw, nh, size))
    img = img.crop(center_crop_box(nw, nh, size))
    return np.asarray(img, dtype=np.uint8)


def sample_key(path):
    """The key of a crop in cluster_labels_decode.json: its last two path components, "<dir>/<file>" (nn_utils.py:85-89)."""
    return "/".join(path.replace(os.sep, "/").split("/")[-2:])


class CropFolder(torch.utils.data.Dataset):
    """ImageFolder(root) with the stage-1 transform; items are (uint8 [size, size, 3] tensor, class index)."""

    def __init__(self, root, size=480):
        self.root = root
        self.size = size
        self.classes, self.class_to_idx = find_classes(root)
        self.samples = make_dataset(root, self.class_to_idx)
        self.targets = [t for _, t in self.samples]

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        path, target = self.samples[i]
        return torch.from_numpy(load_crop(path, self.size).copy()), target

    def keys(self):
        return [sample_key(p) for p, _ in self.samples]


def crop_loader(dataset, batch_size=8, workers=MAX_WORKERS):
    """In-order uint8 NHWC batches (shuffle=False, as usl-imagenet.py's train_memory loader), pinned when a GPU is present."""
    workers = max(0, min(int(workers), MAX_WORKERS))
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=workers,
                                       pin_memory=torch.cuda.is_available(), drop_last=False)
