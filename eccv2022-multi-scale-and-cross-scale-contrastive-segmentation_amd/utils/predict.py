"""Prediction maps out of ``infer()`` / ``validate()`` (reference managers/BaseManager.py save_output, utils/utils.py to_comb_image):

  ``predict_maps``      (ids, mapped, rgb) of logits: arg-max, ``lut[ids]``, ``palette[ids]``; for CUDA fp32 one launch of
                        libdcl_pred.so (csrc/dcl_pred.hip) that reads the low-resolution logits of an ``UpsampledLogits`` directly
  ``panel_image``       the image | label | prediction panel of to_comb_image, one launch
  ``submission_lut``    train id -> dataset class id (reverse_mapping + remap_mask restated)
  ``class_palette``     train id -> colour
  ``PredictionWriter``  PNG files behind a ring of pinned host slots and one encoding thread

The reference takes ``argmax(Softmax2d(x))``; the softmax is monotonic per pixel and is skipped.  Stated deviation: the colours are
the config's ``data.palette`` or the public bit-interleaved PASCAL-VOC generator, not the reference's per-dataset tables."""
import os
import queue
import threading

import numpy as np
import torch

from ..debug import cfg as _dbg
from .datasets_info import DATASETS_INFO

MEAN = (0.485, 0.456, 0.406)        # torchvision_normalise (datasets/augment.py)
STD = (0.229, 0.224, 0.225)


# ---- the tables -----------------------------------------------------------------------------------------------------------------
def submission_lut(dataset, experiment):
    """uint8 [256]: 255 everywhere, then for every train id k != 255 of CLASS_INFO[experiment][0], in its order, and every class
    id c in its list, lut[k] = c (the last one wins; Cityscapes' class id -1 wraps to 255 as in a uint8 array)."""
    lut = np.full(256, 255, dtype=np.uint8)
    for k, ids in DATASETS_INFO[dataset].CLASS_INFO[experiment][0].items():
        if k == 255:
            continue
        for c in ids:
            lut[k] = int(c) & 255
    return torch.from_numpy(lut)


def voc_colour(i):
    """The PASCAL-VOC devkit's colour of index i: the bits of i dealt out to r, g, b from the top bit down."""
    r = g = b = 0
    for j in range(8):
        r |= ((i >> 0) & 1) << (7 - j)
        g |= ((i >> 1) & 1) << (7 - j)
        b |= ((i >> 2) & 1) << (7 - j)
        i >>= 3
    return r, g, b


def class_palette(dataset, experiment, override=None):
    """uint8 [256, 3]: ``override`` ([r, g, b] per train id, the config's data.palette) when given, else generator colour k + 1 for
    train id k (colour 0 is black, which is kept for the ignore id and every id >= the number of classes)."""
    names = DATASETS_INFO[dataset].CLASS_INFO[experiment][1]
    classes = len(names) - 1 if 255 in names else len(names)
    pal = np.zeros((256, 3), dtype=np.uint8)
    for k in range(min(classes, 255)):
        if override is not None:
            if k < len(override):
                pal[k] = [int(v) for v in override[k]]
        else:
            pal[k] = voc_colour(k + 1)
    return torch.from_numpy(pal)


def _table(t, device, shape):
    if t is None:
        return None
    t = torch.as_tensor(t)
    assert t.dtype == torch.uint8 and tuple(t.shape) == shape, f"table must be uint8 {list(shape)}"
    return t.to(device).contiguous()


# ---- logits -> maps -------------------------------------------------------------------------------------------------------------
def hip_applies(z, size, with_rgb):
    """CUDA fp32 [N, C, h, w] with the switch on and a shape dpr_supported takes; a missing library is an error here."""
    if not (_dbg.pred_hip and z.is_cuda and z.dtype == torch.float32 and z.dim() == 4 and not torch.is_autocast_enabled()):
        return False
    from .. import _lib_pred as lp
    return lp.supported(z.shape[0], z.shape[1], z.shape[2], z.shape[3], int(size[0]), int(size[1]), with_rgb)


@torch.no_grad()
def predict_maps(output, lut=None, palette=None):
    """(ids, mapped, rgb): uint8 [N, H, W] arg-max over the classes of ``output`` (a dense [N, C, H, W] tensor or an
    ``UpsampledLogits``, whose full-size logits are then never formed on the kernel path), ``lut[ids]`` (None without ``lut``
    uint8 [256]) and ``palette[ids]`` uint8 [N, H, W, 3] (None without ``palette`` uint8 [256, 3]).  For an ``UpsampledLogits``
    ``output.pred`` is set to ids, which utils.metrics.t_get_confusion_matrix then uses."""
    lazy = hasattr(output, 'materialize')
    z = output.lowres if lazy else output
    assert z.dim() == 4, "logits must be [N, C, H, W]"
    size = tuple(output.size) if lazy else (int(z.shape[2]), int(z.shape[3]))
    align = bool(output.align_corners) if lazy else False
    if z.shape[1] > 256:
        raise ValueError(f"{z.shape[1]} classes do not fit a uint8 map")
    lut, palette = _table(lut, z.device, (256,)), _table(palette, z.device, (256, 3))
    if hip_applies(z, size, palette is not None):
        from .. import _lib_pred as lp
        z = z.detach().contiguous()
        N, C, h, w = z.shape
        H, W = size
        ids = torch.empty((N, H, W), dtype=torch.uint8, device=z.device)
        mapped = torch.empty_like(ids) if lut is not None else None
        rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device=z.device) if palette is not None else None
        lp.check(lp.lib().dpr_predict(lp.ptr(z), N, C, h, w, H, W, 1 if align else 0, lp.ptr(lut), lp.ptr(palette), lp.ptr(ids),
                                      lp.ptr(mapped), lp.ptr(rgb), lp.stream_ptr(z.device)), "dpr_predict")
        lp.calls["predict"] += 1
    else:
        full = output.materialize() if lazy else output
        idx = full.detach().argmax(1)
        ids = idx.to(torch.uint8)
        mapped = lut[idx] if lut is not None else None
        rgb = palette[idx] if palette is not None else None
    if lazy:
        output.pred = ids
    return ids, mapped, rgb


@torch.no_grad()
def panel_image(img, label, ids, palette, mean=MEAN, std=STD, label_ignore=-1, ids_ignore=-1):
    """uint8 [H, 3 W, 3]: round(clamp(img * std + mean, 0, 1) * 255) of the normalised ``img`` f32 [3, H, W] | palette[label] |
    palette[ids]; the ignore ids (and labels outside [0, 255]) are black.  One launch of dpr_panel for CUDA tensors."""
    assert img.dim() == 3 and img.shape[0] == 3 and tuple(label.shape) == tuple(img.shape[1:]) == tuple(ids.shape)
    H, W = int(img.shape[1]), int(img.shape[2])
    palette = _table(palette, img.device, (256, 3))
    if label.dtype not in (torch.int64, torch.int32, torch.uint8):
        label = label.to(torch.int64)
    ids = ids.to(torch.uint8)
    if _dbg.pred_hip and img.is_cuda and img.dtype == torch.float32 and label.is_cuda and ids.is_cuda:
        from .. import _lib_pred as lp
        if lp.panel_supported(H, W, label.element_size()):
            img, label, ids = img.detach().contiguous(), label.contiguous(), ids.contiguous()
            out = torch.empty((H, 3 * W, 3), dtype=torch.uint8, device=img.device)
            lp.check(lp.lib().dpr_panel(lp.ptr(img), lp.ptr(label), label.element_size(), lp.ptr(ids), lp.ptr(palette), H, W,
                                        float(mean[0]), float(mean[1]), float(mean[2]), float(std[0]), float(std[1]), float(std[2]),
                                        int(label_ignore), int(ids_ignore), lp.ptr(out), lp.stream_ptr(img.device)), "dpr_panel")
            lp.calls["panel"] += 1
            return out
    m = torch.tensor(mean, dtype=torch.float32, device=img.device).view(3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=img.device).view(3, 1, 1)
    left = ((img.detach().float() * s + m).clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0)
    lab = label.to(torch.int64)
    bad = (lab < 0) | (lab > 255) | (lab == label_ignore)
    mid = palette[lab.clamp(0, 255)]
    mid[bad] = 0
    right = palette[ids.to(torch.int64)]
    right[ids.to(torch.int64) == ids_ignore] = 0
    return torch.cat([left, mid, right], dim=1).contiguous()


# ---- files ----------------------------------------------------------------------------------------------------------------------
class PredictionWriter:
    """PNG files under ``directory``.  ``write(relative path, uint8 [H, W] or [H, W, 3])`` of a CUDA tensor copies it into one of
    ``depth`` pinned host slots on a side stream (behind an event on the caller's stream) and returns; one thread waits for the
    copy, encodes with PIL and frees the slot, so the caller waits only when every slot is in use (``waits`` counts those).  A CPU
    tensor is handed to the same thread and waited for: the file exists when ``write`` returns.  ``close()`` joins the thread and
    re-raises the first error it met."""

    def __init__(self, directory, depth=2):
        from PIL import Image            # needed from the first file on: fail here, not in the thread
        self._image = Image
        self.directory = str(directory)
        self.depth = max(1, int(depth))
        self.waits = 0
        self.written = 0
        self._slots = [None] * self.depth
        self._free = queue.Queue()
        for i in range(self.depth):
            self._free.put(i)
        self._jobs = queue.Queue()
        self._streams = {}
        self._error = None
        self._closed = False
        self._thread = threading.Thread(target=self._work, name="PredictionWriter", daemon=True)
        self._thread.start()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def write(self, relpath, t):
        assert not self._closed, "write() after close()"
        assert t.dtype == torch.uint8 and (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)), "uint8 [H, W] or [H, W, 3]"
        path = os.path.join(self.directory, relpath)
        t = t.detach().contiguous()
        if not t.is_cuda:
            done = threading.Event()
            self._jobs.put((path, t.numpy(), None, None, done))
            done.wait()
            return path
        try:
            slot = self._free.get_nowait()
        except queue.Empty:
            self.waits += 1
            slot = self._free.get()              # the ring is full: wait for the oldest file
        n = t.numel()
        if self._slots[slot] is None or self._slots[slot].numel() < n:
            self._slots[slot] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        host = self._slots[slot][:n].view(t.shape)
        side = self._streams.get(t.device)
        if side is None:
            side = self._streams[t.device] = torch.cuda.Stream(device=t.device)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(t.device))
        side.wait_event(ready)
        with torch.cuda.stream(side):
            host.copy_(t, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(side)
        t.record_stream(side)
        self._jobs.put((path, host, copied, slot, None))
        return path

    def _encode(self, path, arr):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        self._image.fromarray(arr).save(path)
        self.written += 1

    def _work(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            path, arr, copied, slot, done = job
            try:
                if copied is not None:
                    copied.synchronize()
                    arr = arr.numpy()
                self._encode(path, arr)
            except BaseException as e:           # kept for close(); later files are still written and their slots freed
                if self._error is None:
                    self._error = e
            finally:
                if slot is not None:
                    self._free.put(slot)
                if done is not None:
                    done.set()

    def close(self):
        if self._closed:
            return
        self._closed = True
        self._jobs.put(None)
        self._thread.join()
        if self._error is not None:
            raise self._error
