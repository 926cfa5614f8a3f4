"""Training runtime around the hot path, with the reference's call surface
(managers/BaseManager.py:37-555, LoggingManager.py): config dict in, ``load_model`` / ``load_loss`` /
``load_data`` / ``load_optimiser`` / ``train`` / ``train_one_epoch`` / ``validate`` /
``forward_step``; model and loss classes are resolved by NAME from ``mscs_amd.models`` /
``mscs_amd.losses`` exactly like the reference's ``globals()`` lookups (BaseManager.py:439, 474).

Process model (MI355X-first): one process per GPU.  Either the manager spawns them itself
(``parallel: true`` + ``gpu_device: [..]``, reference behaviour, mp.spawn + env:// rendezvous on
127.0.0.1), or it is started under ``torch.distributed.run`` (RANK / LOCAL_RANK / WORLD_SIZE in the
environment) and simply joins the group.  Gradients are all-reduced by DDP over RCCL/xGMI with
``gradient_as_bucket_view=True``; BatchNorm becomes SyncBatchNorm when ``graph.sync_bn``.  The
contrastive loss is rank-local, as in the reference (its ``concat_all_gather`` has no call site).
"""
import datetime
import os
import time

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from .. import losses as _losses
from .. import models as _models
from ..datasets import SyntheticSegmentation
from ..losses import LossWrapper
from ..losses.engine import StreamKTimeout
from ..utils import DATASETS_INFO, printlog
from ..utils.config import parse_config
from ..utils.lr_functions import LRFcts
from ..utils.metrics import (out_of_range, take_out_of_range, t_get_confusion_matrix, t_get_mean_iou, t_get_pixel_accuracy,
                             t_metrics_from_confusion_matrix)


def set_seeds(seed):
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


class BaseManager:
    # the datasets whose validation images are resized (resize_val) and scored at their original size: the reference's
    # post_process_output names PASCALC and ADE20K
    ORIGINAL_SIZE_DATASETS = ('ADE20K', 'PASCALC')

    def __init__(self, configuration, autostart=True):
        self.config = parse_config(configuration)
        cfg = self.config
        self.debugging = cfg['debugging']
        self.dataset = cfg['data']['dataset']
        self.experiment = cfg['data']['experiment']
        self.batch_size = cfg['data']['batch_size']
        self.valid_batch_size = cfg.get('valid_batch_size', 1)
        self.empty_cache = cfg.get('empty_cache', False)
        self.parallel = bool(cfg['parallel'])
        self.allocated_devices = list(cfg['gpu_device'])
        self.n_gpus = len(self.allocated_devices) if self.parallel else 1
        self.world_size = self.n_gpus
        self.rank = 0
        self.epoch = 0
        self.global_step = 0
        self.start_epoch = 0
        self.best_miou = -1.0
        self.best_loss = 1e10
        self._resumed = False
        self.load_report = None
        self.metrics = {}
        self.model = self.loss = self.optimiser = self.scheduler = None
        self.data_loaders, self.samplers = {}, {}
        self.return_features = False
        self.log_dir = cfg.get('log_dir')
        self.under_torchrun = int(os.environ.get('WORLD_SIZE', '1')) > 1
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')       # LoggingManager.py:136-137
        os.environ.setdefault('MASTER_PORT', '29500')
        if autostart:
            self.start()

    def start(self):
        """Reference behaviour of the constructor: build everything and, in parallel training mode,
        run the training loop (BaseManager.py:37-104)."""
        cfg = self.config
        if self.under_torchrun:
            self.setup()
            if cfg['mode'] == 'training':
                self.train()
        elif self.parallel and cfg['mode'] == 'training':
            set_seeds(cfg['seed'])
            mp.spawn(self.distributed_train_worker, nprocs=self.n_gpus, args=())
        else:
            self.setup()

    def setup(self):
        """Build model / loss / data / optimiser for THIS process (joins the process group when
        started under torch.distributed.run); does not train."""
        cfg = self.config
        if self.under_torchrun:
            self.parallel = True
            self.world_size = self.n_gpus = int(os.environ['WORLD_SIZE'])
            self._worker_setup(int(os.environ.get('LOCAL_RANK', '0')), int(os.environ['RANK']),
                               split_batch=cfg.get('batch_is_global', True))
            return
        set_seeds(cfg['seed'])
        use_cuda = cfg['cuda'] and torch.cuda.is_available()
        self.device = torch.device(f'cuda:{self.allocated_devices[0]}' if use_cuda else 'cpu')
        if use_cuda:
            torch.cuda.set_device(self.device)
        self.load_model()
        self.load_loss()
        self.load_data()
        self.load_optimiser()
        self._maybe_load_checkpoint()

    # ------------------------------------------------------------------ processes
    def distributed_train_worker(self, gpu):
        """Entry point of a spawned rank (reference: BaseManager.py:106-145)."""
        self._worker_setup(self.allocated_devices[gpu], gpu)
        self.train()

    def _worker_setup(self, device_index, rank, split_batch=True):
        set_seeds(self.config['seed'])
        self.rank = rank
        use_cuda = self.config['cuda'] and torch.cuda.is_available()
        if use_cuda:
            self.device = torch.device(f'cuda:{device_index}')
            torch.cuda.set_device(self.device)
        else:                                   # CPU ranks (gloo) -- used by the multi-process tests
            self.device = torch.device('cpu')
        if split_batch:
            self.batch_size = int(self.batch_size) // self.n_gpus    # global batch -> per rank (:128)
        if not dist.is_initialized():
            backend = self.config.get('dist_backend', 'nccl' if use_cuda else 'gloo')   # 'nccl' == RCCL on ROCm
            dist.init_process_group(backend=backend, world_size=self.world_size, rank=self.rank)
        self.load_model()
        self.load_loss()
        self.load_data()
        self.load_optimiser()
        self._maybe_load_checkpoint()

    # ------------------------------------------------------------------ construction
    def load_model(self):
        graph = self.config['graph']
        if self.config.get('mode') == 'training' and self.config.get('loss', {}).get('name') == 'LossWrapper' \
                and self.config.get('cuda', False):
            # This manager owns BOTH ends of the model's training outputs -- they go to this package's LossWrapper and
            # metrics, nowhere else (forward_step) -- so a reference JSON config, which knows neither key, gets the fused
            # consumers: the logits stay at 1/4 resolution (up-sampling + cross-entropy / arg-max in one kernel, models/ops.py
            # UpsampledLogits) and the projection heads' last 1x1 convolution is evaluated on the sampled pixels only
            # (models/Projector.LazyProjection).  Same losses and gradients (tests/test_hip_parity.py); a config that says
            # `false` -- or code that calls the model classes directly -- gets the reference's tensors.
            defaulted = [k for k in ('lazy_logits', 'lazy_projector') if k not in graph]
            graph.setdefault('lazy_logits', True)
            graph.setdefault('lazy_projector', True)
            if defaulted:
                # (said out loud, so that a subclass / hook that reads ret['output'] or ret['feats'] as plain tensors
                # knows why it sees UpsampledLogits / LazyProjection objects and which key turns them off)
                printlog(f"[mscs_amd] graph.{' / graph.'.join(defaulted)} not in the config: defaulting to true under this manager -- "
                         "the model's training outputs are UpsampledLogits (logits at 1/4 resolution) and LazyProjection "
                         "(projector rows on the sampled pixels) objects, consumed by this package's LossWrapper and metrics; "
                         "write `false` for the reference's tensors (INTEGRATION.md, 'Runtime behaviour')")
        model_class = getattr(_models, graph['model'])
        self.model = model_class(config=graph, experiment=self.experiment)
        self.return_features = getattr(self.model, 'projector_model', None) is not None \
            and self.config['mode'] == 'training'
        self.model = self.model.to(self.device)
        if self.config.get('channels_last', False):
            self.model = self.model.to(memory_format=torch.channels_last)
        if self.parallel:
            if graph.get('sync_bn', False):
                if self.device.type == 'cuda':
                    from ..models.fused_bn import convert_sync_batchnorm
                    self.model = convert_sync_batchnorm(self.model)
                else:
                    printlog('sync_bn requested but ranks are on CPU: SyncBatchNorm needs GPU modules, '
                             'keeping per-rank BatchNorm statistics')
            self.model = torch.nn.parallel.DistributedDataParallel(
                self.model, device_ids=[self.device] if self.device.type == 'cuda' else None,
                gradient_as_bucket_view=True)
        n_params = sum(p.numel() for p in self.model.parameters() if p.requires_grad)
        printlog(f"Using model '{graph['model']}' with backbone '{graph.get('backbone')}' : "
                 f"trainable parameters {n_params}")

    def _bare_model(self):
        return self.model.module if hasattr(self.model, 'module') else self.model

    def load_loss(self):
        lcfg = self.config['loss']
        lcfg['experiment'] = self.experiment
        lcfg['device'] = str(self.device)
        if lcfg['name'] == 'CrossEntropyLoss':
            names = DATASETS_INFO[self.dataset].CLASS_INFO[self.experiment][1]
            self.loss = torch.nn.CrossEntropyLoss(ignore_index=len(names) - 1 if 255 in names else -100)
        else:
            self.loss = getattr(_losses, lcfg['name'])(lcfg)
        self.loss = self.loss.to(self.device)
        if isinstance(self.loss, LossWrapper) and any('DenseContrastive' in t for t in self.loss.loss_classes):
            assert getattr(self._bare_model(), 'projector_model', None) is not None, \
                'model must have projector if DC loss is used'

    def load_data(self):
        dcfg = self.config['data']
        if dcfg.get('synthetic_raw', False) or not dcfg.get('synthetic', False):
            return self._load_raw_data()
        names = DATASETS_INFO[self.dataset].CLASS_INFO[self.experiment][1]
        size = dcfg.get('transform_values', {}).get('crop_shape', [512, 1024])
        train = SyntheticSegmentation(dcfg.get('synthetic_length', 64), size, len(names),
                                      mode=dcfg.get('synthetic_mode', 'iid'), seed=self.config['seed'])
        valid = SyntheticSegmentation(dcfg.get('synthetic_valid_length', 4), size, len(names),
                                      mode=dcfg.get('synthetic_mode', 'iid'), seed=self.config['seed'] + 1)
        sampler = DistributedSampler(train, num_replicas=self.world_size, rank=self.rank) if self.parallel else None
        self.samplers['train_loader'] = sampler
        self.data_loaders['train_loader'] = DataLoader(
            train, batch_size=self.batch_size, shuffle=sampler is None, sampler=sampler,
            num_workers=dcfg['num_workers'], drop_last=True, pin_memory=self.device.type == 'cuda')
        self.data_loaders['valid_loader'] = DataLoader(valid, batch_size=self.valid_batch_size, shuffle=False,
                                                       num_workers=0)
        self.train_schedule = {e: 'train_loader' for e in range(self.config['train']['epochs'])}

    def _load_raw_data(self):
        """The raw input path (datasets/raw.py, datasets/augment.py): the loaders only decode files (or draw ``synthetic_raw``
        pixels) and attach each sample's augmentation plan; ``_upload`` runs the augmentation on the device."""
        from ..datasets import ADE20K, Cityscapes, DeviceAugment, PascalC, SyntheticRaw, list_collate, network_lut, planner_for
        dcfg, seed = self.config['data'], self.config['seed']
        tv = dcfg.get('transform_values', {})
        plan_t = planner_for(dcfg.get('transforms', ['RandomCropImgLbl', 'torchvision_normalise']), tv, self.dataset,
                             self.experiment, seed)
        plan_v = planner_for(dcfg.get('transforms_val', ['torchvision_normalise']), dcfg.get('transform_values_val', tv),
                             self.dataset, self.experiment, seed + 1)
        if plan_v.resize_val and self.dataset not in self.ORIGINAL_SIZE_DATASETS:
            printlog("[mscs_amd] transforms_val holds resize_val: validate() will raise (the reference's original-label "
                     f"evaluation applies to {' and '.join(self.ORIGINAL_SIZE_DATASETS)} only)")
        if dcfg.get('synthetic_raw', False):
            size = dcfg.get('synthetic_raw_size', [1024, 2048])
            train = SyntheticRaw(dcfg.get('synthetic_length', 64), size, self.dataset, self.experiment, plan_t, seed=seed)
            valid = SyntheticRaw(dcfg.get('synthetic_valid_length', 4), size, self.dataset, self.experiment, plan_v, seed=seed + 1)
        else:
            if not self.config.get('data_path'):
                raise KeyError("data_path: the config names no dataset folder (set data_path, or data.synthetic / "
                               "data.synthetic_raw for generated data)")
            root = self.config['data_path']
            # data.split = [train split, validation split] as in the reference's configs (its managers/BaseManager.py load_data)
            if self.dataset == 'CITYSCAPES':
                split = dcfg.get('split', ['train', 'val'])
                train, valid = Cityscapes(root, split[0], plan_t), Cityscapes(root, split[1], plan_v)
            elif self.dataset == 'ADE20K':
                split = dcfg.get('split', ['train', 'val'])
                train, valid = ADE20K(root, split[0], plan_t), ADE20K(root, split[1], plan_v)
            elif self.dataset == 'PASCALC':
                split = dcfg.get('split', ['train', 'val'])
                train, valid = PascalC(root, split[0], plan_t), PascalC(root, split[1], plan_v)
            elif self.dataset == 'CADIS':
                train, valid = self._cadis_readers(root, plan_t, plan_v)
            else:
                raise NotImplementedError(f"no reader for dataset {self.dataset}: CITYSCAPES, ADE20K, PASCALC and CADIS are ported "
                                          "(SURVEY.md row 15)")
        self._augment = DeviceAugment(network_lut(self.dataset, self.experiment))
        sampler = DistributedSampler(train, num_replicas=self.world_size, rank=self.rank) if self.parallel else None
        self.samplers['train_loader'] = sampler
        self.data_loaders['train_loader'] = DataLoader(
            train, batch_size=self.batch_size, shuffle=sampler is None, sampler=sampler, num_workers=dcfg['num_workers'],
            drop_last=True, pin_memory=self.device.type == 'cuda', collate_fn=list_collate)
        self.data_loaders['valid_loader'] = DataLoader(valid, batch_size=self.valid_batch_size, shuffle=False, num_workers=0,
                                                       collate_fn=list_collate)
        self.train_schedule = {e: 'train_loader' for e in range(self.config['train']['epochs'])}
        self._schedule_repeat_factor(train)

    def _cadis_readers(self, root, plan_t, plan_v):
        """The CaDIS readers of the config (the reference's datasets/CaDIS.py get_cadis_dataframes): the frame table is
        data.frame_table, else data/data.csv under the working directory (as the reference), else <data_path>/data.csv."""
        from ..datasets import CaDIS, read_frame_table
        dcfg = self.config['data']
        if 'random_split' in dcfg:
            raise NotImplementedError("data.random_split (the reference's legacy split of frames) is not ported: name the video "
                                      "split with data.split")
        table = dcfg.get('frame_table') or next((p for p in (os.path.join('data', 'data.csv'), os.path.join(root, 'data.csv'))
                                                 if os.path.exists(p)), os.path.join(root, 'data.csv'))
        rows = read_frame_table(table)
        kw = dict(split=int(dcfg.get('split', 1)), experiment=self.experiment, mode=self.config.get('mode', 'training'),
                  use_relabeled=dcfg.get('use_relabeled', False), blacklist=dcfg.get('blacklist', True))
        return CaDIS(root, rows, planner=plan_t, subset='train', **kw), CaDIS(root, rows, planner=plan_v, subset='valid', **kw)

    def _schedule_repeat_factor(self, train):
        """data.repeat_factor [start, stop] (one number: until the last epoch): those epochs draw from train_repeat_factor_loader,
        a BatchSampler(drop_last) over the repeat-factor sampler of the reader's rows (the reference's load_data schedule)."""
        from ..datasets import list_collate
        dcfg, epochs = self.config['data'], self.config['train']['epochs']
        span = list(dcfg.get('repeat_factor') or [0, 0])
        if len(span) == 1:
            span.append(epochs)
        scheduled = [e for e in range(*span) if e < epochs]
        if not scheduled:
            return
        if not hasattr(train, 'rows'):
            raise ValueError(f"data.repeat_factor needs the per-frame class columns of the CaDIS frame table; the {self.dataset} "
                             "loader has none")
        from ..utils.repeat_factor_sampling import RepeatFactorSampler
        sampler = RepeatFactorSampler(train.rows, dcfg.get('repeat_factor_freq_thresh', 0.15), self.experiment, dataset=self.dataset,
                                      num_replicas=self.world_size if self.parallel else 1, rank=self.rank if self.parallel else 0)
        self.samplers['train_repeat_factor_loader'] = sampler
        self.data_loaders['train_repeat_factor_loader'] = DataLoader(
            train, batch_sampler=torch.utils.data.BatchSampler(sampler, batch_size=self.batch_size, drop_last=True),
            num_workers=dcfg['num_workers'], pin_memory=self.device.type == 'cuda', collate_fn=list_collate)
        for e in scheduled:
            self.train_schedule[e] = 'train_repeat_factor_loader'

    def _param_groups(self):
        """``train.opt_keys`` {substring: {lr_mult, wd_mult}} -> optimizer parameter groups (reference:
        utils/optimizer_utils.py:34-80): a parameter joins the group of the FIRST key its name contains, every other
        parameter the base group; frozen parameters stay out."""
        tcfg = self.config['train']
        keys = tcfg.get('opt_keys')
        if not keys:
            return self.model.parameters()
        # like the reference (optimizer_utils.py:38): opt_keys without train.weight_decay is a KeyError, not a silent
        # run with zero weight decay (every group carries an explicit value, so the optimiser's default never applies)
        base_lr, base_wd = tcfg['learning_rate'], tcfg['weight_decay']
        groups = {}
        for name, p in self.model.named_parameters():
            if not p.requires_grad:
                continue
            gname, lr, wd = 'base_lr_wd', base_lr, base_wd
            for key, mult in keys.items():
                if key in name:
                    lm, wm = mult.get('lr_mult', 1.0), mult.get('wd_mult', 1.0)
                    gname, lr, wd = f'{key}_lrm{lm}_wdm{wm}', lm * base_lr, wm * base_wd
                    break
            g = groups.setdefault(gname, {'params': [], 'group_name': gname, 'param_names': [], 'lr': lr,
                                          'weight_decay': wd})
            g['params'].append(p)
            g['param_names'].append(name)
        return list(groups.values())

    def load_optimiser(self):
        tcfg = self.config['train']
        params = self._param_groups()
        optim = tcfg.get('optim', 'Adam')
        # single-pass ("fused") parameter updates where torch has them for the device: the same update rule in ONE kernel pass
        # per tensor list instead of the foreach form's three (weight decay, momentum, step): 1.4 -> 0.5 ms of the W48 step,
        # at its very end where nothing overlaps (train.fused_optimizer = false keeps the foreach form)
        fused = {}
        params = list(params)
        flat = [p for g in params for p in (g['params'] if isinstance(g, dict) else [g])]
        if tcfg.get('fused_optimizer', True) and self.config.get('cuda', False) and \
                all(p.is_cuda and p.dtype == torch.float32 for p in flat):
            fused = {'fused': True}
        if optim == 'SGD':
            self.optimiser = torch.optim.SGD(params, lr=tcfg['learning_rate'], momentum=tcfg.get('momentum', 0.9),
                                             weight_decay=tcfg.get('weight_decay', 0.0005), **fused)
        elif optim == 'Adam':
            self.optimiser = torch.optim.Adam(params, lr=tcfg['learning_rate'])
        elif optim == 'AdamW':
            self.optimiser = torch.optim.AdamW(params, lr=tcfg['learning_rate'],
                                               betas=tuple(tcfg.get('betas', (0.9, 0.999))),
                                               weight_decay=tcfg.get('weight_decay', 0.01), **fused)
        else:
            raise ValueError(f"optimizer {optim} not recognized")
        # an invalid gradient of the contrastive loss (stream-K backward: a timed-out hand-over, losses/engine.py) must never
        # reach the parameters: checked right before every update (the error word was copied to the host at the START of the
        # backward pass, so this normally does not wait)
        self.optimiser.register_step_pre_hook(lambda *_a, **_k: self._check_backward())
        if tcfg['lr_batchwise']:
            total = sum(len(self.data_loaders[self.train_schedule[e]]) for e in range(tcfg['epochs']))
        else:
            total = tcfg['epochs']
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(
            self.optimiser, lr_lambda=LRFcts(tcfg, list(tcfg.get('lr_restarts', [])), max(total, 2)))

    # ------------------------------------------------------------------ loops
    def forward_step(self, img, lbl, **kwargs):
        raise NotImplementedError

    def _check_backward(self):
        if self.device.type == 'cuda':
            from ..losses.engine import streamk_check
            streamk_check()

    def train(self):
        tcfg = self.config['train']
        for self.epoch in range(self.start_epoch, tcfg['epochs']):
            sampler = self.samplers.get(self.train_schedule[self.epoch])
            if sampler is not None:
                sampler.set_epoch(self.epoch)
            dataset = self.data_loaders[self.train_schedule[self.epoch]].dataset
            if hasattr(dataset, 'set_epoch'):           # raw path: the epoch of the augmentation plans' stream
                dataset.set_epoch(self.epoch)
            self.train_one_epoch()
            if (self.epoch + 1) % self.config.get('valid_freq', 1) == 0 or self.epoch == tcfg['epochs'] - 1:
                self.validate()
        if self.parallel and dist.is_initialized():
            dist.barrier()

    def _upload(self, img, lbl, meta=None):
        """H2D of a batch on a dedicated input stream (+ the label's int64 conversion), and the event that marks
        it complete: the loss's label stage waits for THAT event only (engine.stage_labels), so it -- and the host
        plan built from it -- can run while the GPU is still in the previous step's backward.  A raw batch (lists of
        decoded uint8 tensors, the plans in ``meta``) is copied as it is and augmented on the same stream
        (datasets/augment.py DeviceAugment) before the event is recorded."""
        raw = isinstance(img, (list, tuple))
        plans = [m['plan'] for m in meta] if raw else None
        if self.device.type != 'cuda':
            if raw:
                return (*self._augment(list(img), list(lbl), plans), None)
            return img.to(self.device), lbl.to(self.device), None
        if getattr(self, '_in_stream', None) is None:
            self._in_stream = torch.cuda.Stream(device=self.device, priority=-1)    # own hardware queue
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._in_stream):
            if raw:
                img, lbl = self._augment([t.to(self.device, non_blocking=True) for t in img],
                                         [t.to(self.device, non_blocking=True) for t in lbl], plans)
            else:
                img = img.to(self.device, non_blocking=True)
                lbl = lbl.to(self.device, non_blocking=True).long()
            ready = torch.cuda.Event()
            ready.record(self._in_stream)
        cur.wait_event(ready)
        img.record_stream(cur)
        lbl.record_stream(cur)
        return img, lbl, ready

    def train_one_epoch(self):
        self.model.train()
        t_prev = time.perf_counter()
        for batch_num, batch in enumerate(self.data_loaders[self.train_schedule[self.epoch]]):
            img, lbl, ready = self._upload(*batch[:3])
            self.optimiser.zero_grad()
            ret = self.forward_step(img, lbl, label_ready=ready)
            ret['loss'].backward()
            try:
                self.optimiser.step()
            except StreamKTimeout as e:
                # raised by the pre-step hook BEFORE anything was applied (on every rank: the error word is all-reduced).  The
                # library has switched to the column-split backward: repeat the step on the same batch.  (The repeated forward
                # updates the norms' running statistics and draws the sampling permutations a second time.)
                printlog(f'[warning] {e}\n          repeating step {self.global_step}')
                self.optimiser.zero_grad()
                ret = self.forward_step(img, lbl, label_ready=ready)
                ret['loss'].backward()
                self.optimiser.step()
            if self.scheduler is not None and self.config['train']['lr_batchwise']:
                self.scheduler.step()
            if batch_num == 2 and self.debugging:
                break
            self.step_metrics(batch_num, ret, lbl, (time.perf_counter() - t_prev) * 1e3)
            t_prev = time.perf_counter()
            self.global_step += 1
        self.flush_logging()
        if self.scheduler is not None and not self.config['train']['lr_batchwise']:
            self.scheduler.step()

    def step_metrics(self, batch_num, ret, lbl, ms):
        """The per-step tail of the reference's loop (HRNet_Manager.py:117-121): confusion matrix (one HIP pass over
        the logits, utils/metrics.py), pixel accuracies, mIoU, logging."""
        cm = t_get_confusion_matrix(ret['output'], lbl, self.dataset)
        pa, pac, miou = t_metrics_from_confusion_matrix(cm)
        self.train_logging(batch_num, ret['loss'], pa, pac, miou, ms)

    def train_logging(self, batch_num, loss, pa, pac, miou, ms):
        """All scalars of the step travel in ONE asynchronous D2H (the reference issues one blocking .item() per
        logged value) and are read one step LATER, when the copy has long finished: the host never waits for the
        device here.  ``self.metrics`` therefore describes the previous step until ``flush_logging()``."""
        keys, vals = ['loss', 'pa', 'pac', 'miou'], [loss.detach().float(), pa, pac, miou]
        if isinstance(self.loss, LossWrapper):
            for k, v in self.loss.loss_vals.items():
                if torch.is_tensor(v):
                    keys.append(k)
                    vals.append(v.float())
        if loss.is_cuda:          # targets outside the class range, counted by the confusion-matrix kernel
            keys.append('_oob')
            vals.append(take_out_of_range(loss.device))           # this step's count; the counter restarts at 0
        dev_vals = torch.stack([v.reshape(()) for v in vals])
        self.flush_logging()                                        # the PREVIOUS step's record
        if loss.is_cuda:
            host = getattr(self, '_log_host', None)
            if host is None or host.numel() < dev_vals.numel():
                host = self._log_host = torch.empty(max(64, dev_vals.numel()), dtype=torch.float32, pin_memory=True)
            host[:dev_vals.numel()].copy_(dev_vals, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._log_pending = (keys, host, dev_vals.numel(), ev, batch_num, ms)
        else:
            self._log_pending = (keys, dev_vals, dev_vals.numel(), None, batch_num, ms)
            self.flush_logging()

    def flush_logging(self):
        pend, self._log_pending = getattr(self, '_log_pending', None), None
        if pend is None:
            return
        keys, host, n, ev, batch_num, ms = pend
        if ev is not None:
            ev.synchronize()
        vals = host[:n].tolist()
        if keys[-1] == '_oob':
            keys = keys[:-1]
            if vals.pop() > 0:
                raise RuntimeError('Class values must be smaller than num_classes.')   # F.one_hot's error in the
                # reference's t_get_confusion_matrix (utils/torch_utils.py:172-177), reported one step late
        self.metrics.update(zip(keys, vals))
        if self.rank == 0 and (batch_num % self.config.get('log_every_n_steps', 10) == 0):
            terms = ' '.join(f'{k}:{v:.4f}' for k, v in zip(keys, vals))
            printlog(f'ep {self.epoch} it {batch_num} t:{ms:.0f}ms {terms}')

    def _valid_batch(self, batch):
        """(img, lbl, original) of a validation batch on the device; on the raw path through the validation plan's geometry.
        ``original`` is None, or -- a raw batch whose plan resized (resize_val), on a dataset the reference scores at the original
        size -- per sample what utils.evaluate.evaluate_at_original needs: the raw label as decoded, (rh, rw), (H, W) and the
        device copy of the raw id -> network id table."""
        if not isinstance(batch[0], (list, tuple)):
            return batch[0].to(self.device), batch[1].to(self.device), None
        plans = [m['plan'] for m in batch[2]]
        resized = any((p.rh, p.rw) != (p.H, p.W) for p in plans)
        if resized and self.dataset not in self.ORIGINAL_SIZE_DATASETS:
            raise NotImplementedError("validation on resize_val needs the reference's original-label evaluation "
                                      "(Resize(return_original_labels=True)), which is not ported")
        img, lbl, _ = self._upload(*batch[:3])
        if not resized:
            return img, lbl, None
        lut = self._augment._lut_on(self.device)
        original = [{'label': raw.to(self.device, non_blocking=True), 'crop': (p.rh, p.rw), 'size': (p.H, p.W), 'lut': lut}
                    for raw, p in zip(batch[1], plans)]
        return img, lbl, original

    @staticmethod
    def _main_logits(out):
        """The main logits of a model's eval-mode return value (a tensor, an UpsampledLogits, or a tuple that holds them)."""
        logits = out[0] if isinstance(out, (tuple, list)) and len(getattr(out[0], 'shape', ())) == 4 and len(out) == 2 else out
        if isinstance(logits, (tuple, list)):
            logits = logits[1]
        return logits

    def _evaluate_original(self, output, original, cm, want_ids=False):
        """The reference's post_process_output and the confusion matrix after it, per sample (utils/evaluate.py): crop the
        fit_stride padding, resize to the original size with the bare model's align_corners, score against lut[raw label].
        Returns (cm + this batch's counts, [ids uint8 [H, W] per sample] when asked)."""
        from ..utils.evaluate import evaluate_at_original
        align = bool(self._bare_model().align_corners)
        lazy = hasattr(output, 'materialize')
        ids = []
        for n, o in enumerate(original):
            if lazy:
                one = output if output.lowres.shape[0] == 1 else type(output)(output.lowres[n:n + 1], output.size, output.align_corners)
            else:
                one = output[n:n + 1]
            ret = evaluate_at_original(one, o['label'], o['crop'], o['size'], align, self.dataset, label_lut=o['lut'],
                                       existing_matrix=cm if torch.is_tensor(cm) else None, return_ids=want_ids)
            if want_ids:
                cm, i = ret
                ids.append(i[0])
            else:
                cm = ret
        return cm, ids

    @torch.no_grad()
    def validate(self):
        if self.rank != 0:          # rank 0 only, like the reference (HRNet_Manager.py:150-156)
            return None
        self.model.eval()
        cm = 0
        panels = self._panel_writer() if self.config.get('save_valid_images', False) else None
        try:
            for i, batch in enumerate(self.data_loaders['valid_loader']):
                img, lbl, original = self._valid_batch(batch)
                if original is not None:
                    # scored at the original size; with graph.lazy_logits the model hands out its 1/4 map for it
                    bare = self._bare_model()
                    lazy = self.config['graph'].get('lazy_logits', False)
                    logits = self._main_logits(self._call_lazy(bare, img.float()) if lazy else bare(img.float()))
                    cm, ids = self._evaluate_original(logits, original, cm, want_ids=panels is not None)
                    if panels is not None:
                        self._save_panel_original(panels, i, img, original[0], ids[0])
                else:
                    out = self._bare_model()(img.float())
                    logits = out[0] if isinstance(out, (tuple, list)) and out[0].dim() == 4 and len(out) == 2 else out
                    if isinstance(logits, (tuple, list)):
                        logits = logits[1]
                    cm = cm + t_get_confusion_matrix(logits, lbl, self.dataset)
                    if panels is not None:
                        self._save_panel(panels, i, img, lbl, logits)
                if i + 1 >= self.config.get('max_valid_imgs', 10):
                    break
        finally:
            if panels is not None:
                panels[0].close()
        miou = float(t_get_mean_iou(cm).item())
        if torch.is_tensor(cm) and cm.is_cuda and int(take_out_of_range(cm.device).item()) > 0:
            # a validation label outside the class range: F.one_hot's error in the reference's confusion matrix
            # (utils/torch_utils.py:172-177), raised here instead of by the next training epoch's first flush
            self.model.train()
            raise RuntimeError('Class values must be smaller than num_classes.')
        self.metrics['final_miou'] = miou
        self.metrics['final_miou_step'] = self.global_step - 1
        is_best = miou > self.best_miou
        self.best_miou = max(self.best_miou, miou)
        printlog(f'validation epoch {self.epoch}: mIoU {miou:.4f}')
        # checkpoints as in valid_logging (LoggingManager.py:280-284): the best so far, and one every
        # log_every_n_epochs plus the final epoch; `save_checkpoints: false` turns them off (benchmarks)
        if self.config['mode'] == 'training' and self.config.get('save_checkpoints', True) \
                and self.optimiser is not None:
            if is_best:
                self.save_checkpoint(is_best=True)
            every = self.config.get('log_every_n_epochs', 100)
            if (self.epoch % every == 0 and self.epoch > 0) or self.epoch == self.config['train']['epochs'] - 1:
                self.save_checkpoint(is_best=False)
        self.model.train()
        return miou

    # ------------------------------------------------------------------ saved predictions (utils/predict.py)
    def _panel_writer(self):
        """(writer, palette) of ``save_valid_images``: <log_dir>/valid_images/record_NN_stepS.png, one image | label | prediction
        panel per validation record (the reference's to_comb_image, which it hands to TensorBoard)."""
        from ..utils.predict import PredictionWriter, class_palette
        palette = class_palette(self.dataset, self.experiment, self.config['data'].get('palette')).to(self.device)
        return PredictionWriter(os.path.join(self._log_dir(), 'valid_images'), self.config.get('save_depth', 2)), palette

    def _save_panel(self, panels, rec, img, lbl, logits):
        from ..utils import ignore_class
        from ..utils.predict import panel_image, predict_maps
        writer, palette = panels
        first = logits.materialize()[:1] if hasattr(logits, 'materialize') else logits[:1]
        ids = predict_maps(first)[0]
        ignore = ignore_class(self.dataset, self.experiment)
        panel = panel_image(img[0].float(), lbl[0], ids[0], palette, label_ignore=ignore, ids_ignore=ignore)
        writer.write('record_{:02d}_step{}.png'.format(rec, self.global_step), panel)

    def _save_panel_original(self, panels, rec, img, original, ids):
        """The panel of a record that was scored at its original size: the image is the network input without its padding, resized
        like the logits (three channels; the reference's post_process_output does the same), the label is lut[raw label]."""
        import torch.nn.functional as F
        from ..utils import ignore_class
        from ..utils.predict import panel_image
        writer, palette = panels
        (rh, rw), size = original['crop'], original['size']
        image = F.interpolate(img[:1, :, :rh, :rw].float(), size=size, mode='bilinear',
                              align_corners=bool(self._bare_model().align_corners))[0]
        label = original['lut'][original['label'].to(torch.int64)]
        ignore = ignore_class(self.dataset, self.experiment)
        panel = panel_image(image, label, ids, palette, label_ignore=ignore, ids_ignore=ignore)
        writer.write('record_{:02d}_step{}.png'.format(rec, self.global_step), panel)

    @staticmethod
    def _record_stem(batch, n, index):
        """File stem of sample ``n`` of a batch: its target_filename, else its img_filename, else record_{index:06d}."""
        meta = batch[2] if len(batch) > 2 else None
        if isinstance(meta, (list, tuple)) and n < len(meta):
            meta = meta[n]
            n = None
        if isinstance(meta, dict):
            for key in ('target_filename', 'img_filename'):
                name = meta.get(key)
                if isinstance(name, (list, tuple)) and n is not None and n < len(name):
                    name = name[n]
                if isinstance(name, (str, os.PathLike)) and str(name):
                    return os.path.splitext(os.path.basename(str(name)))[0]
        return 'record_{:06d}'.format(index)

    @staticmethod
    def _call_lazy(model, x):
        """model(x) with ``lazy_eval_logits`` set around the call where the model has it (HRNet, UPerNet: the logits stay at 1/4
        resolution, as for the test-time-augmentation wrappers, models/TTA.py); restored also when the call raises."""
        if not hasattr(model, 'lazy_eval_logits'):
            return model(x)
        saved = model.lazy_eval_logits
        model.lazy_eval_logits = True
        try:
            return model(x)
        finally:
            model.lazy_eval_logits = saved

    def _tta_model(self):
        """The reference's dispatch (BaseManager.py:610-635): CITYSCAPES -> TTAWrapperCTS (multi-scale, flip, sliding window),
        everything without a protocol of its own -> TTAWrapper (multi-scale, flip)."""
        cfg = self.config
        scales_list = [0.75, 1.25, 1.5, 1.75, 2] if not self.debugging else [1.0]
        if 'tta_scales' in cfg and not self.debugging:
            scales_list = cfg['tta_scales']
        if self.dataset == 'CITYSCAPES':
            crop_size = cfg['data']['transform_values']['crop_shape']
            strides = cfg['strides'] if 'strides' in cfg else crop_size
            flip = cfg['flip'] if 'flip' in cfg else True
            return _models.TTAWrapperCTS(self.model, scales_list, flip, strides, crop_size)
        if self.dataset == 'PASCALC':
            raise NotImplementedError("TTAWrapperPC (the reference's PASCAL-Context protocol: border padding through cv2) is "
                                      "not ported; only TTAWrapper and TTAWrapperCTS are (DESIGN.md, 'Test-time augmentation')")
        if self.dataset == 'ADE20K' and 'strides' in cfg:
            raise NotImplementedError("TTAWrapperSlide (the reference's ADE20K sliding-window protocol: every image resized to a "
                                      "hard-coded (2048 s, 512 s)) is not ported; drop `strides` from the config for TTAWrapper")
        return _models.TTAWrapper(self.model, scales_list)

    def _tta_wrapper(self):
        """What ``infer()`` wraps the model in: the two sliding-window protocols with equal-size windows (models/TTA.py, fused on
        libdcl_slide.so) -- PASCALC -> TTAWrapperPC, ADE20K with ``strides`` -> TTAWrapperSlide -- and ``_tta_model()`` for the
        rest.  ``tta_window_batch`` (default 8): windows per model call on their fused path."""
        cfg = self.config
        sliding = self.dataset == 'PASCALC' or (self.dataset == 'ADE20K' and 'strides' in cfg)
        if not sliding:
            return self._tta_model()
        scales_list = [0.75, 1.25, 1.5, 1.75, 2] if not self.debugging else [1.0]
        if 'tta_scales' in cfg and not self.debugging:
            scales_list = cfg['tta_scales']
        if self.dataset == 'PASCALC':
            wrapper = _models.TTAWrapperPC(self.model, scales_list, num_classes=self._bare_model().num_classes)
        else:
            crop_size = cfg['data']['transform_values']['crop_shape']
            flip = cfg['flip'] if 'flip' in cfg else True
            wrapper = _models.TTAWrapperSlide(self.model, scales_list, flip, cfg['strides'], crop_size)
        wrapper.tta_window_batch = int(cfg.get('tta_window_batch', 8))
        return wrapper

    @torch.no_grad()
    def infer(self):
        """Run the model over ``valid_loader`` the way the reference's ``infer()`` does (BaseManager.py:585-675): the checkpoint
        named by ``load_checkpoint`` (``load_last``: the last instead of the best one), with ``tta`` the model inside a test-time
        augmentation wrapper (``tta_scales``, ``strides``, ``flip``, ``data.transform_values.crop_shape``), the confusion matrix
        summed over the images.  Returns the metrics dict of ``t_get_mean_iou`` and logs the mIoU on rank 0.  The reference's
        ``post_process_output`` step (ADE20K and PASCALC on ``resize_val``: padding cut off, logits resized to the image's original size, scored
        against the label that was never resized) is one kernel per image after the model or the wrapper (utils/evaluate.py), and
        the saved files are then at the original size.  ``save_outputs: true`` (rank 0) writes, per image, the reference's two files
        (BaseManager.py:677-699): <log_dir>/outputs/<split>/debug/<stem>.png (colours) and .../submit/<stem>.png (dataset class
        ids), through utils/predict.py: without tta the model is then called with ``lazy_eval_logits`` and prediction and
        confusion matrix both come from its 1/4-resolution map."""
        cfg = self.config
        assert 'load_checkpoint' in cfg, 'load_checkpoint: "run_id" must be in config for inference mode!'
        self.model.eval()
        bare = self._bare_model()
        for flag in ('get_intermediate', 'return_features'):       # suppress the auxiliary output and the projector's features
            if hasattr(bare, flag):
                setattr(bare, flag, False)
        self.load_checkpoint(cfg['load_checkpoint'], 'last' if cfg.get('load_last', False) else 'best')
        tta_model = None
        if cfg['tta']:
            tta_model = self._tta_wrapper()
            printlog(f'** {tta_model.__class__.__name__} using tta with transforms \n ** flip and scales: {tta_model.scales}')
        confusion_matrix = None
        writer = None
        if cfg.get('save_outputs', False) and self.rank == 0:
            from ..utils.predict import PredictionWriter, class_palette, predict_maps, submission_lut
            split = cfg['data'].get('split')                        # [train split, validation split]; the parser's default is an int
            split = split[-1] if isinstance(split, (list, tuple)) and split else 'val'
            writer = PredictionWriter(os.path.join(self._log_dir(), 'outputs', str(split)), cfg.get('save_depth', 2))
            lut = submission_lut(self.dataset, self.experiment).to(self.device)
            palette = class_palette(self.dataset, self.experiment, cfg['data'].get('palette')).to(self.device)
            saved = 0
        try:
            for rec_num, batch in enumerate(self.data_loaders['valid_loader']):
                img, lbl, original = self._valid_batch(batch)
                if original is not None:
                    # the reference's post_process_output: files and matrix at the image's original size, from one kernel per
                    # image that reads the model's 1/4 map (or a wrapper's dense output)
                    output = tta_model(img.float()) if tta_model is not None else self._call_lazy(bare, img.float())
                    confusion_matrix, ids = self._evaluate_original(self._main_logits(output), original, confusion_matrix,
                                                                    want_ids=writer is not None)
                    for n, one in enumerate(ids):
                        stem = self._record_stem(batch, n, saved)
                        writer.write(os.path.join('debug', stem + '.png'), palette[one.to(torch.int64)])
                        writer.write(os.path.join('submit', stem + '.png'), lut[one.to(torch.int64)])
                        saved += 1
                else:
                    if writer is None:
                        output = tta_model(img.float()) if tta_model is not None else bare(img.float())
                    else:
                        output = tta_model(img.float()) if tta_model is not None else self._call_lazy(bare, img.float())
                        _, mapped, rgb = predict_maps(output, lut, palette)     # (leaves output.pred for the confusion matrix)
                        for n in range(mapped.shape[0]):
                            stem = self._record_stem(batch, n, saved)
                            writer.write(os.path.join('debug', stem + '.png'), rgb[n])
                            writer.write(os.path.join('submit', stem + '.png'), mapped[n])
                            saved += 1
                    confusion_matrix = t_get_confusion_matrix(output, lbl, self.dataset, confusion_matrix)
                if rec_num == 10 and self.debugging:
                    break
        finally:
            if writer is not None:
                writer.close()
        mious = t_get_mean_iou(confusion_matrix, self.experiment, self.dataset, True, rare=True)
        if self.rank == 0:
            msg_str = "miou:{:.4f} ".format(float(mious['mean_iou']))
            for categ, v in mious['categories'].items():
                msg_str += "- {}:{:.4f}".format(categ, float(v))
            printlog(msg_str)
        return mious

    # ------------------------------------------------------------------ demo_tsne (utils/tsne.py)
    TSNE_SCALES = {4: 0, 8: 1, 16: 2, 32: 3}

    def _tsne_feature_map(self, bare, backbone_out, s):
        """The feature map at pyramid level ``s`` out of what the bare model's ``backbone`` returned."""
        name = self.config['graph']['model']
        if name == 'HRNet':
            if bare.backbone.return_all_scales:
                return backbone_out[1][s]
            if s != 0:
                raise ValueError("demo_tsne: an HRNet without ms_projector / return_all_scales hands out its concatenated map "
                                 "only: tsne_scale must be 4")
            return backbone_out.materialize() if hasattr(backbone_out, 'materialize') else backbone_out
        from ..models.Swin import as_nchw
        return as_nchw(backbone_out[s])

    @torch.no_grad()
    def demo_tsne(self):
        """The reference's ``demo_tsne`` mode (BaseManager.py:701-783): the checkpoint named by ``load_checkpoint`` (``load_last``:
        the last instead of the best one), the model in eval mode over ``valid_loader``, per image up to a few pixels of every
        class out of the backbone's feature map at stride ``tsne_scale`` (4, 8, 16 or 32; caught by a forward hook on the bare
        model's ``backbone``), then the exact t-SNE of what was gathered (utils/tsne.py) and the scatter plot
        ``<run_id>_perp-<p>_its-<n>_feats-per-class-<f>_scale<s>.png`` under the log directory, an ``.npz`` beside it.  Optional
        keys ``tsne_iters``, ``tsne_perplexity``, ``tsne_feats_per_class`` default to the reference's 2000, 30 and 1000.  Any
        batch size (the reference asserts 1): one sample at a time.  Returns the embedding [N, 2] (numpy)."""
        cfg = self.config
        assert 'load_checkpoint' in cfg, 'load_checkpoint: "run_id" must be in config for demo_tsne mode!'
        from ..utils.tsne import TsneManager
        name = cfg['graph']['model']
        if name not in ('HRNet', 'UPerNet'):
            raise NotImplementedError(f"demo_tsne: no feature pyramid is defined for model {name} (HRNet and UPerNet, as in the reference)")
        scale = int(cfg.get('tsne_scale', 4))
        if scale not in self.TSNE_SCALES:
            raise ValueError(f"tsne_scale must be one of {sorted(self.TSNE_SCALES)}, got {scale}")
        self.model.eval()
        bare = self._bare_model()
        self.load_checkpoint(cfg['load_checkpoint'], 'last' if cfg.get('load_last', False) else 'best')
        run_id = cfg.get('run_id') or os.path.basename(self._log_dir())
        self.TsneManager = TsneManager(self.dataset, bare.num_classes, scale=scale, run_id=run_id,
                                       perplexity=cfg.get('tsne_perplexity', 30), iters=cfg.get('tsne_iters', 2000),
                                       feats_per_class=cfg.get('tsne_feats_per_class', 1000), seed=cfg['seed'],
                                       experiment=self.experiment, palette=cfg['data'].get('palette'))
        caught = {}
        hook = bare.backbone.register_forward_hook(lambda _m, _i, out: caught.__setitem__('out', out))
        try:
            for rec_num, batch in enumerate(self.data_loaders['valid_loader']):
                img, lbl, _ = self._valid_batch(batch)
                for n in range(img.shape[0]):
                    self.model(img[n:n + 1].float())
                    if img.is_cuda:
                        torch.cuda.synchronize(self.device)        # the pyramid levels come from the branches' own streams
                    f = self._tsne_feature_map(bare, caught.pop('out'), self.TSNE_SCALES[scale])
                    self.TsneManager.accumulate(f, lbl[n:n + 1])
                if rec_num == 100 and self.debugging:
                    break
        finally:
            hook.remove()
        printlog(f'computing tsne for feats of scale : {scale} dim : {self.TsneManager.feat_dim} '
                 f'counts : {list(enumerate(self.TsneManager.counts))}')
        return self.TsneManager.compute(self._log_dir())

    # ------------------------------------------------------------------ checkpoints
    def _log_dir(self):
        """``<log_path>/<run_id>`` like the reference (LoggingManager.py:81-91); created on first use so that runs
        which never save (benchmarks, tests) leave nothing behind."""
        if self.log_dir is None:
            run_id = self.config.get('run_id')
            if run_id is None:
                run_id = '{:%Y%m%d_%H%M%S}_e{}'.format(datetime.datetime.now(), self.experiment)
                if 'name' in self.config:
                    run_id = '__'.join((run_id, str(self.config['name'])))
            self.log_dir = os.path.join(self.config.get('log_path', 'logging'), run_id)
        os.makedirs(os.path.join(str(self.log_dir), 'chkpts'), exist_ok=True)
        return str(self.log_dir)

    def checkpoint_state(self, is_best=False):
        """The reference's checkpoint dictionary, key for key (LoggingManager.py:293-313)."""
        state = {'global_step': self.global_step - 1,       # the reference saves after train_logging's increment
                 'epoch': self.epoch,                        # absolute: train() resumes at start_epoch
                 'model_state_dict': self.model.state_dict(),
                 'optimiser_state_dict': self.optimiser.state_dict(),
                 'best_loss': self.best_loss,
                 'best_miou': self.best_miou,
                 'final_miou': self.metrics.get('final_miou', 0),
                 'final_miou_step': self.metrics.get('final_miou_step', 0),
                 'is_best': bool(is_best)}
        if self.scheduler is not None:
            state['scheduler_state_dict'] = self.scheduler.state_dict()
        return state

    def save_checkpoint(self, is_best=False, path=None):
        """``chkpts/chkpt_best.pt`` or ``chkpts/chkpt_epoch_NNN.pt`` under the run's log directory (or an explicit
        ``path``), written by rank 0 only; returns the path."""
        if self.rank != 0:
            return None
        state = self.checkpoint_state(is_best)
        if path is None:
            name = 'chkpt_best.pt' if is_best else 'chkpt_epoch_{:03d}.pt'.format(state['epoch'])
            path = os.path.join(self._log_dir(), 'chkpts', name)
        torch.save(state, path)
        printlog(f'Checkpoint saved: {path}')
        return path

    def _resolve_checkpoint(self, spec, chkpt_type):
        """``spec``: a .pt file, a run directory (with ``chkpts/``), or a run id under ``log_path``; picks
        ``chkpt_best.pt`` or the last ``chkpt_epoch_*.pt`` like LoggingManager.py:327-344."""
        spec = str(spec)
        if os.path.isfile(spec):
            return spec
        base = spec if os.path.isdir(spec) else os.path.join(self.config.get('log_path', 'logging'), spec)
        ck = os.path.join(base, 'chkpts') if os.path.isdir(os.path.join(base, 'chkpts')) else base
        if not os.path.isdir(ck):
            raise FileNotFoundError(f"load_checkpoint: '{spec}' is neither a checkpoint file nor a run directory")
        names = sorted(os.listdir(ck))
        epochs = [n for n in names if n.startswith('chkpt_epoch_')]
        if chkpt_type == 'last':
            if not epochs:
                raise ValueError("No checkpoint of type 'last' found.")
            return os.path.join(ck, epochs[-1])
        if 'chkpt_best.pt' in names:
            return os.path.join(ck, 'chkpt_best.pt')
        if epochs:
            printlog("No checkpoint of type 'best' found; loading the last one.")
            return os.path.join(ck, epochs[-1])
        raise ValueError(f'Neither chkpt of type "best" nor of type "last" was found in {names}')

    @staticmethod
    def match_module_prefix(state, target_keys):
        """Rename ``state``'s keys so that DDP's ``module.`` prefix agrees with the model it is loaded into, in
        BOTH directions (a single-GPU save into a DDP-wrapped model and vice versa; the reference only strips,
        LoggingManager.py:353-354 / check_module_prefix)."""
        want = any(k.startswith('module.') for k in target_keys)
        out = {}
        for k, v in state.items():
            has = k.startswith('module.')
            if want and not has:
                k = 'module.' + k
            elif has and not want:
                k = k[len('module.'):]
            out[k] = v
        return out

    def load_checkpoint(self, spec, chkpt_type='best', strict_keys=True):
        """Load a checkpoint in the reference's dictionary layout (LoggingManager.py:321-368).  Missing and
        unexpected keys are logged; a checkpoint that matches NO parameter of the model raises (the silent
        ``strict=False`` no-op of a prefix mismatch)."""
        path = self._resolve_checkpoint(spec, chkpt_type)
        chk = torch.load(path, map_location=self.device, weights_only=False)
        target = self.model.state_dict()
        state = self.match_module_prefix(chk['model_state_dict'], target.keys())
        matched = [k for k in state if k in target]
        if not matched:
            raise RuntimeError(f'checkpoint {path} shares no parameter name with the model '
                               f'(first keys: {list(state)[:3]} vs {list(target)[:3]})')
        ret = self.model.load_state_dict(state, strict=False)
        if ret.missing_keys or ret.unexpected_keys:
            printlog(f'load_state_dict: {len(matched)} tensors loaded, missing {len(ret.missing_keys)} '
                     f'{ret.missing_keys[:5]}, unexpected {len(ret.unexpected_keys)} {ret.unexpected_keys[:5]}')
            if strict_keys and self.config.get('strict_checkpoint', False):
                raise RuntimeError('checkpoint does not match the model (strict_checkpoint)')
        self.load_report = ret
        if self.config['mode'] == 'training':
            if 'optimiser_state_dict' in chk and self.optimiser is not None:
                self.optimiser.load_state_dict(chk['optimiser_state_dict'])
            if chk.get('scheduler_state_dict') and self.scheduler is not None:
                self.scheduler.load_state_dict(chk['scheduler_state_dict'])
            self.start_epoch = chk.get('epoch', -1) + 1
            self.global_step = chk.get('global_step', 0)
            self.best_loss = chk.get('best_loss', 1e10)
            self.best_miou = chk.get('best_miou', -1.0)
            self.metrics['final_miou'] = chk.get('final_miou')
            self._resumed = True
        printlog(f'rank {self.rank}: checkpoint loaded: {path} (type {chkpt_type})')
        return path

    def _maybe_load_checkpoint(self):
        """``load_checkpoint`` / ``load_last`` config keys (BaseManager.py:76-82, 139-144)."""
        if 'load_checkpoint' in self.config:
            kind = 'last' if self.config.get('load_last', False) else 'best'
            self.load_checkpoint(self.config['load_checkpoint'], kind)
