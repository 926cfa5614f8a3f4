"""Repeat-factor sampling (the reference's utils/repeat_factor_sampling.py, after Gupta et al., LVIS) on the rows of the CaDIS
reader (datasets/raw.py): frames that hold a rare class are repeated, by a factor that is reached in expectation through stochastic
rounding.  No pandas: a row is a dict of the frame table's columns, and the per-class pixel counts are its canonical class columns.

  f(c)  = share of the frames that hold class c of the experiment (summed over the canonical classes the experiment merges into c,
          as the reference does, so it can exceed 1); an absent class gets f = t
  r(c)  = max(1, sqrt(t / f(c)))
  r(I)  = max of r(c) over the classes present in frame I, as float32

The generator calls are the reference's, in its order: ``torch.rand`` for the rounding on a generator seeded ``seed`` (1) once,
``manual_seed(seed + epoch)`` before the ``randperm``; with more than one replica its ``randint`` trim and ``islice(rank, None,
world)``.  Its indices are positions in the rows it was given."""
import math
from itertools import islice

import numpy as np
import torch
from torch.utils.data import Sampler

from .datasets_info import DATASETS_INFO


def _experiment_of_canonical(dataset, experiment):
    """canonical class name -> class of the experiment (the reference's rev_mapping[canonical_num_to_name[c]])."""
    info = DATASETS_INFO[dataset].CLASS_INFO
    to_exp = {raw: key for key, raws in info[experiment][0].items() for raw in raws}
    return {name: to_exp[num] for num, name in info[0][1].items() if num in to_exp}


def class_repeat_factors(rows, repeat_thresh, experiment, dataset='CADIS'):
    """{class of the experiment: r(c)} over ``rows``."""
    of = _experiment_of_canonical(dataset, experiment)
    n = len(rows)
    freqs = {}
    for name in DATASETS_INFO[dataset].CLASS_NAMES[0]:
        if name not in of:
            continue
        held = sum(1 for row in rows if float(row[name]) > 0)
        freqs[of[name]] = freqs.get(of[name], 0) + held / n
    out = {}
    for c in DATASETS_INFO[dataset].CLASS_INFO[experiment][1]:
        f = freqs.get(c, 0)
        if f == 0:
            f = repeat_thresh
        out[c] = np.maximum(1, np.sqrt(repeat_thresh / f))
    return out


def image_repeat_factors(rows, class_rfs, experiment, dataset='CADIS'):
    """float32 [len(rows)]: r(I)."""
    of = _experiment_of_canonical(dataset, experiment)
    names = [name for name in DATASETS_INFO[dataset].CLASS_NAMES[0] if name in of]
    rfs = []
    for i, row in enumerate(rows):
        present = [class_rfs[of[name]] for name in names if float(row[name]) > 0]
        if not present:
            raise ValueError(f"frame {i} ({row.get('img_path')}) holds no class: no repeat factor")
        rfs.append(np.max(present))
    return torch.tensor(rfs, dtype=torch.float32)


class RepeatFactorSampler(Sampler):
    """Always shuffles.  ``set_epoch(e)`` before an epoch, as for a DistributedSampler."""

    def __init__(self, rows, repeat_thresh, experiment, seed=None, dataset='CADIS', num_replicas=1, rank=0):
        assert 0 <= repeat_thresh < 1
        self.seed = 1 if seed is None else int(seed)
        self.repeat_thresh = repeat_thresh
        self.class_repeat_factors = class_repeat_factors(rows, repeat_thresh, experiment, dataset)
        self.repeat_factors = image_repeat_factors(rows, self.class_repeat_factors, experiment, dataset)
        self._int_part = torch.trunc(self.repeat_factors)
        self._frac_part = self.repeat_factors - self._int_part
        self.g = torch.Generator()
        self.g.manual_seed(self.seed)
        self.epoch = 0
        self.indices = None
        self.num_replicas, self.rank = int(num_replicas), int(rank)

    def __iter__(self):
        if self.num_replicas > 1:
            # the reference runs one whole pass for a log line before the pass it yields from; that pass draws from the same
            # generator, so it is made here too
            for _ in self._yield_indices():
                pass
            yield from islice(self._yield_indices(), self.rank, None, self.num_replicas)
        else:
            yield from self._yield_indices()

    def _yield_indices(self):
        # (the reference keeps the list a preceding len() drew, untrimmed, and draws a new one otherwise)
        if self.indices is not None:
            indices = torch.tensor(self.indices, dtype=torch.int64)
        else:
            indices = self._get_epoch_indices(self.g)
        left = len(self)
        self.g.manual_seed(self.seed + self.epoch)
        while left > 0:                             # an epoch's size varies with the stochastic rounding
            for item in indices[torch.randperm(len(indices), generator=self.g)]:
                yield int(item)
                left -= 1
        self.indices = None

    def __len__(self):
        if self.indices is not None:
            return len(self.indices)
        return len(self._get_epoch_indices(self.g))

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _get_epoch_indices(self, generator):
        rands = torch.rand(len(self._frac_part), generator=generator)
        rounded = self._int_part + (rands < self._frac_part).float()
        indices = []
        for index, factor in enumerate(rounded):
            indices.extend([index] * int(factor.item()))
        self.indices = indices
        if self.num_replicas > 1:                   # every process the same number of indices
            n = len(indices)
            per = math.ceil(n / self.num_replicas) if n % self.num_replicas == 0 else math.ceil((n - self.num_replicas) / self.num_replicas)
            keep = per * self.num_replicas
            kept = torch.randint(low=0, high=keep - 1, size=[keep], generator=generator)
            return torch.tensor(indices, dtype=torch.int64)[kept]
        return torch.tensor(indices, dtype=torch.int64)
