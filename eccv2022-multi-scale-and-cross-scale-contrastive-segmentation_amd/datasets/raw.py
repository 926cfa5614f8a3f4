"""Datasets of the raw input path: they only DECODE.  Every item is ``(img uint8 [H, W, 3], lbl uint8 [H, W], metadata)`` with the
label in the dataset's raw ids and the sample's augmentation plan in ``metadata['plan']``; everything from there to the
float32 / int64 batch happens on the device (datasets/augment.py).  Folder layouts as the reference's datasets/Cityscapes.py and
datasets/ADE20K.py.  PIL is imported inside the readers only."""
import os

import numpy as np
import torch
from torch.utils.data import Dataset


def list_collate(batch):
    """(list of images, list of labels, list of metadata): images of different sizes stay apart."""
    return [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch]


class _Raw(Dataset):
    """Shared: the planner, the epoch of its stream, the item tuple."""

    def __init__(self, planner):
        self.planner, self.epoch = planner, 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _item(self, index, img, lbl, **meta):
        img, lbl = torch.from_numpy(np.ascontiguousarray(img)), torch.from_numpy(np.ascontiguousarray(lbl))
        meta.update(index=index)
        if self.planner is not None:
            meta['plan'] = self.planner.plan(img.shape[0], img.shape[1], self.epoch, index)
        return img, lbl, meta

    def _read(self, index):
        from PIL import Image
        img = np.array(Image.open(self.images[index]).convert('RGB'), dtype=np.uint8)
        lbl = np.array(Image.open(self.targets[index]))
        if lbl.ndim != 2 or lbl.min() < 0 or lbl.max() > 255:
            raise ValueError(f'{self.targets[index]}: expected a single-channel label image with ids in [0, 255]')
        return self._item(index, img, lbl.astype(np.uint8), img_filename=self.images[index], target_filename=self.targets[index])

    def __len__(self):
        return len(self.images)

    def __getitem__(self, index):
        return self._read(index)


class Cityscapes(_Raw):
    """``<root>/leftImg8bit/<split>/<city>/*_leftImg8bit.png`` paired with ``<root>/gtFine/<split>/<city>/*_gtFine_labelIds.png``;
    ``split`` is 'train', 'val', 'test' or ['train', 'val']."""
    dataset, experiment = 'CITYSCAPES', 1

    def __init__(self, root, split='train', planner=None):
        super().__init__(planner)
        splits = list(split) if isinstance(split, (list, tuple)) else [split]
        assert all(s in ('train', 'val', 'test') for s in splits), f'split {split} is not valid'
        self.root, self.split = root, split
        self.images, self.targets = [], []
        for s in splits:
            images_dir, targets_dir = os.path.join(root, 'leftImg8bit', s), os.path.join(root, 'gtFine', s)
            for city in sorted(os.listdir(images_dir)):
                for name in sorted(os.listdir(os.path.join(images_dir, city))):
                    if '_leftImg8bit' not in name:
                        continue
                    target = os.path.join(targets_dir, city, '{}_gtFine_labelIds.png'.format(name.split('_leftImg8bit')[0]))
                    if not os.path.exists(target):
                        raise FileNotFoundError(f'{target} (the label of {name}) not found')
                    self.images.append(os.path.join(images_dir, city, name))
                    self.targets.append(target)


class ADE20K(_Raw):
    """``<root>/ADEChallengeData2016/images/<split>/*.jpg`` paired by stem with ``.../annotations/<split>/*.png``; ``split`` is
    'training' or 'validation' ('train' / 'val' are accepted for them)."""
    dataset, experiment = 'ADE20K', 1

    def __init__(self, root, split='training', planner=None):
        super().__init__(planner)
        split = {'train': 'training', 'val': 'validation'}.get(split, split)
        self.root, self.split = root, split
        base = os.path.join(root, 'ADEChallengeData2016')
        images_dir, targets_dir = os.path.join(base, 'images', split), os.path.join(base, 'annotations', split)
        self.images, self.targets = [], []
        for name in sorted(os.listdir(images_dir)):
            stem, ext = os.path.splitext(name)
            if ext.lower() not in ('.jpg', '.jpeg'):
                continue
            target = os.path.join(targets_dir, stem + '.png')
            if not os.path.exists(target):
                raise FileNotFoundError(f'{target} (the label of {name}) not found')
            self.images.append(os.path.join(images_dir, name))
            self.targets.append(target)


class PascalC(_Raw):
    """``<root>/<split>/image/*.jpg`` paired by stem with ``<root>/<split>/label/*.png`` (the reference's datasets/PascalC.py);
    ``split`` is 'train' or 'val'.  Raw ids: in experiment 1 raw 0 is the ignore class and raw k is class k - 1 of 59."""
    dataset, experiment = 'PASCALC', 1

    def __init__(self, root, split='train', planner=None):
        super().__init__(planner)
        assert split in ('train', 'val'), f'split {split} is not valid'
        self.root, self.split = root, split
        images_dir, targets_dir = os.path.join(root, split, 'image'), os.path.join(root, split, 'label')
        self.images, self.targets = [], []
        for name in sorted(os.listdir(images_dir)):
            stem, ext = os.path.splitext(name)
            if ext.lower() not in ('.jpg', '.jpeg'):
                continue
            target = os.path.join(targets_dir, stem + '.png')
            if not os.path.exists(target):
                raise FileNotFoundError(f'{target} (the label of {name}) not found')
            self.images.append(os.path.join(images_dir, name))
            self.targets.append(target)
        labels = sorted(n for n in os.listdir(targets_dir) if n.lower().endswith('.png'))
        assert len(labels) == len(self.targets), f'{targets_dir}: {len(labels)} labels for {len(self.images)} images'


def read_frame_table(path):
    """The rows of a CaDIS frame table (the reference's data/data.csv) as dicts of strings, in the file's order."""
    import csv
    if not os.path.exists(path):
        raise FileNotFoundError(f'{path}: the CaDIS frame table (config key data.frame_table) not found')
    with open(path, newline='') as f:
        rows = list(csv.DictReader(f))
    for column in ('img_path', 'lbl_path', 'vid_num'):
        if not rows or column not in rows[0]:
            raise KeyError(f'{path}: the frame table has no column {column}')
    return rows


def _is_one(row, column):
    """pandas' ``df[column] == 1`` on a row of strings: an empty cell, or a table without the column, is not 1."""
    v = row.get(column)
    return v not in (None, '') and float(v) == 1


class CaDIS(_Raw):
    """The frames of a CaDIS frame table, filtered as the reference's datasets/CaDIS.py get_cadis_dataframes does: ``subset``
    'train' keeps the frames of the train videos of ``DATA_SPLITS[split]``, 'valid' those of the validation videos that are not
    propagated; ``use_relabeled`` reads ``relabeled/<name>`` for relabeled frames (and takes them off the blacklist), ``blacklist``
    drops blacklisted frames.  With a three-way split, ``mode`` 'inference' validates on the test videos.  Paths are split on '\\',
    joined under ``root`` and decoded to raw ids; ``rows`` are the kept rows, ``self.rows[i]`` belongs to item i.

    Stated deviations: a table without a ``propagated`` column counts every frame as not propagated (the shipped table has none;
    the reference raises KeyError there); the reference tests ``mode`` for 'infer', which nothing sets."""
    dataset = 'CADIS'

    def __init__(self, root, frames, split=1, experiment=2, planner=None, mode='training', subset='train', use_relabeled=False,
                 blacklist=True):
        super().__init__(planner)
        from ..utils import DATASETS_INFO
        assert subset in ('train', 'valid'), f'subset {subset} is not valid'
        self.root, self.split, self.experiment, self.subset = root, int(split), experiment, subset
        rows = read_frame_table(frames) if isinstance(frames, (str, os.PathLike)) else list(frames)
        for column in ('img_path', 'lbl_path', 'vid_num'):
            if not rows or column not in rows[0]:
                raise KeyError(f'the frame table has no column {column}')
        splits = DATASETS_INFO['CADIS'].DATA_SPLITS[self.split]
        if len(splits) not in (2, 3):
            raise ValueError('splits must be a list of length 2 or 3')
        videos = splits[0] if subset == 'train' else splits[2] if len(splits) == 3 and mode == 'inference' else splits[1]
        rows = [dict(r) for r in rows if int(float(r['vid_num'])) in videos and not (subset == 'valid' and _is_one(r, 'propagated'))]
        if use_relabeled:
            for r in rows:
                if _is_one(r, 'relabeled'):
                    r['blacklisted'] = '0'
                    r['lbl_path'] = 'relabeled/' + r['lbl_path'].replace('\\', '/').split('/')[-1]
        if blacklist:
            rows = [r for r in rows if not _is_one(r, 'blacklisted')]
        self.rows = rows
        self.images = [os.path.join(root, *r['img_path'].split('\\')) for r in rows]
        self.targets = [os.path.join(root, *r['lbl_path'].split('\\')) for r in rows]
        for path in self.images + self.targets:
            if not os.path.exists(path):
                raise FileNotFoundError(f'{path} (a frame of the CaDIS frame table) not found')


class SyntheticRaw(_Raw):
    """uint8 images and blocky uint8 labels in the RAW ids of ``dataset`` (the ids its lookup table maps to a class, and the first
    unmapped one for the ignore class), without touching disk."""

    def __init__(self, length, size, dataset, experiment, planner=None, block=32, seed=0):
        super().__init__(planner)
        from .augment import network_lut
        self.length, self.size, self.block, self.seed = int(length), tuple(size), int(block), int(seed)
        lut = network_lut(dataset, experiment).numpy()
        ids = [int(np.nonzero(lut == k)[0][0]) for k in sorted(set(lut.tolist()))]      # one raw id per network id
        self.raw_ids = np.asarray(ids, dtype=np.uint8)

    def __len__(self):
        return self.length

    def __getitem__(self, index):
        rng = np.random.default_rng((self.seed, index))
        H, W = self.size
        b = self.block
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        small = self.raw_ids[rng.integers(0, len(self.raw_ids), (-(-H // b), -(-W // b)))]
        lbl = np.repeat(np.repeat(small, b, 0), b, 1)[:H, :W]
        return self._item(index, img, lbl, target_size=[H, W])
