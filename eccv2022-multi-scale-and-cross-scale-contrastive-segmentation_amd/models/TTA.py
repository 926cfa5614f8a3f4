"""Test-time-augmentation inference with the reference's call surface: ``TTAWrapper`` (models/TTA_wrapper.py: multi-scale and
flip) and ``TTAWrapperCTS`` (models/TTA_wrapper_CTS.py: the Cityscapes protocol -- multi-scale, flip, sliding window, exp).  Batch
1, fp32, under ``torch.no_grad()``.

For a CUDA fp32 image (``debug.cfg.tta_hip`` on, shapes ``dtt_supported`` takes) every view's logits go straight from the model
into the kernels of libdcl_tta.so (models/ops_tta.py): the flip and the resize of the 3-channel input stay in torch, the logits at
the scaled size, their mirrored copy and the copy resized to the image size are never written.  HRNet and UPerNet hand out their
quarter-resolution logits for that (``lazy_eval_logits``, set around each model call and restored); any other module returns full
logits, which the kernels take with an identity inner level.  Everything else (CPU, other dtypes, refused shapes) runs the
reference's composition in torch, the same operations in the same order.

Kept quirks of the reference: 1.0 is appended to the caller's ``scale_list`` in place when absent; ``TTAWrapper`` stores ``flip``
but always runs both orientations (``f == 0`` is the mirrored one) and resizes every view to the image size even at equal size;
``TTAWrapperCTS`` takes exp of the averaged logits, not a softmax, and does not divide the sum over the scales.  Not kept: a
DDP-wrapped model is unwrapped with ``model.module`` (the reference writes ``ddp.module``), the cv2 image dumps of ``debug`` are
gone, and a window grid with no rows or columns raises instead of dividing by a zero count.

``TTAWrapperPC`` (models/TTA_wrapper_PC.py: PASCAL-Context) and ``TTAWrapperSlide`` (models/TTAWrapperSlide.py: ADE20K with
``strides``) are sliding-window protocols whose windows all have one size per scale: PASCAL-Context pads the image and its partial
windows to the crop with ``-mean / std`` and does not shift the last window back, the ADE20K protocol shifts it back.  Their fused
path (``debug.cfg.slide_hip``, models/ops_slide.py on libdcl_slide.so) is, per view, one launch that writes the crop batch and its
mirrors from the original image, the model over that batch in chunks of ``tta_window_batch`` windows (a window and its mirror in
the same call), one launch that writes the averaged canvas, and the ``merge`` above with an identity inner level.  Kept quirks of
``TTAWrapperSlide``: every image is resized to ``(int(img_scale[0] * s), int(img_scale[1] * s))`` read as (height, width), whatever
its own size; with ``flip`` every scale is summed twice, once averaged with its mirror and once plain; an axis shorter than the
crop gives one short window; the sum over the views is not divided.  Kept of ``TTAWrapperPC``: it always flips, and its three
branches (whole image no larger than the crop, one side shorter, windows) are the reference's.  Not kept: a grid with no window
raises ``ValueError`` as ``TTAWrapperCTS`` does instead of dividing by zero, and the reference's timing print and image dumps are
gone."""
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.parallel import DistributedDataParallel as ddp

from ..utils import printlog
from . import ops_slide, ops_tta


class TTAWrapper(nn.Module):
    def __init__(self, model, scale_list=None, flip=True):
        super().__init__()
        self.scales = scale_list
        self.flip = flip
        if 1.0 not in self.scales:
            self.scales.append(1.0)
        self.model = model.module if isinstance(model, ddp) else model
        self.align_corners = self.model.align_corners if hasattr(self.model, 'align_corners') else True
        printlog(f'*** TTA wrapper with flip : [{flip}] --- scales : {self.scales} -- align_corners:{self.align_corners}')

    # ---- the model call
    def _call_model(self, x, lazy):
        """model(x) with ``return_features`` / ``get_intermediate`` cleared (the reference's infer() clears them for good) and,
        for the fused path, ``lazy_eval_logits`` set: HRNet / UPerNet then return their quarter-resolution logits.  Attributes the
        model does not have stay absent; all are restored, also when the call raises."""
        m = self.model
        saved = {}
        for name, value in (('return_features', False), ('get_intermediate', False), ('lazy_eval_logits', bool(lazy))):
            if hasattr(m, name):
                saved[name] = getattr(m, name)
                setattr(m, name, value)
        try:
            return m(x)
        finally:
            for name, value in saved.items():
                setattr(m, name, value)

    @staticmethod
    def _input(x):
        if isinstance(x, tuple):
            x = x[0]
            assert isinstance(x, torch.Tensor), f'x input must be a tensor instead got {type(x)}'
        assert len(x.shape) == 4, 'input must be B,C,H,W'
        return x

    @staticmethod
    def _acc_dtype(x):
        # fp32 like the reference's torch.zeros(...); a float64 image keeps float64 sums (the tests' reference runs)
        return torch.float64 if x.dtype == torch.float64 else torch.float32

    def maybe_resize(self, x, scale, in_shape):
        """scale in R+: resize to int(scale * in_shape); 1: a copy; -1: resize to in_shape (also at equal size)"""
        scaled_shape = [int(scale * in_shape[0]), int(scale * in_shape[1])]
        if scale != 1.0 and scale > 0:
            x = F.interpolate(x, size=scaled_shape, mode='bilinear', align_corners=self.align_corners)
        elif scale == -1:
            x = F.interpolate(x, size=list(in_shape), mode='bilinear', align_corners=self.align_corners)
        else:
            x = x.clone()
        return x

    def maybe_flip(self, x, f):
        return torch.flip(x, dims=[3]) if f == 0 else x.clone()

    def forward(self, x, **kwargs):
        x = self._input(x)
        in_shape = [int(x.shape[2]), int(x.shape[3])]
        fused = ops_tta.hip_applies(x)
        y_merged = torch.zeros([1, self.model.num_classes] + in_shape, dtype=self._acc_dtype(x), device=x.device)
        for f in range(2):
            x_f = self.maybe_flip(x, f)
            for s in self.scales:
                x_f_s = self.maybe_resize(x_f, s, in_shape)
                y = self._call_model(x_f_s, fused)
                if fused:
                    z, size, align = ops_tta.view_logits(y)
                    if ops_tta.supported(z, size, in_shape):
                        ops_tta.merge(z[0], size, align, f == 0, y_merged[0], self.align_corners)
                        continue
                y = self.maybe_flip(ops_tta.full_logits(y), f)
                y_merged += self.maybe_resize(y, -1, in_shape)
        return y_merged / (2 * len(self.scales))


class TTAWrapperCTS(TTAWrapper):
    def __init__(self, model, scale_list, flip=True, strides=None, crop_size=None, *, base_size=2048, num_classes=19):
        super().__init__(model, scale_list, flip)
        self.num_classes = num_classes
        self.crop_size = crop_size if crop_size else [512, 1024]
        self.strides = strides if strides else self.crop_size      # defaults to non-overlapping windows
        self.base_size = base_size
        printlog(f'Sliding window : strides : {self.strides} crop_size {self.crop_size}')

    def inference(self, image, flip=False):
        """exp of the logits, or of the mean of the logits and the un-mirrored logits of the mirrored image"""
        pred = ops_tta.full_logits(self._call_model(image, False))
        if flip:
            flip_output = ops_tta.full_logits(self._call_model(torch.flip(image, dims=[3]), False))
            pred = pred + torch.flip(flip_output, dims=[3])
            pred = pred * 0.5
        return pred.exp()

    def _fused_window(self, image, flip, canvas, h0, w0):
        """one crop (or the whole image) through the model and into ``canvas`` [C, Hc, Wc]; False where the kernels refuse it"""
        ch, cw = int(image.shape[2]), int(image.shape[3])
        z, size, align = ops_tta.view_logits(self._call_model(image, True))
        if tuple(size) != (ch, cw) or not ops_tta.supported(z, size, canvas.shape[-2:]):
            return False
        zf = None
        if flip:
            zf, size_f, align_f = ops_tta.view_logits(self._call_model(torch.flip(image, dims=[3]), True))
            if tuple(size_f) != (ch, cw) or align_f != align or zf.shape != z.shape:
                return False
            zf = zf[0]
        ops_tta.window_accum(z[0], zf, (ch, cw), align, canvas, h0, w0, ch, cw)
        return True

    def _plan(self, scale, ori_height, ori_width):
        new_h, new_w = ops_tta.cts_size(ori_height, ori_width, self.base_size, scale)
        if scale < 1.0:
            return new_h, new_w, [(0, new_h)], [(0, new_w)]
        rows = ops_tta.windows_1d(new_h, int(self.crop_size[0]), int(self.strides[0] * 1.0))
        cols = ops_tta.windows_1d(new_w, int(self.crop_size[1]), int(self.strides[1] * 1.0))
        if len(rows) < 1 or len(cols) < 1:
            raise ValueError(f'TTAWrapperCTS: scale {scale} gives a {new_h} x {new_w} image with {len(rows)} x {len(cols)} windows '
                             f'of crop {list(self.crop_size)} and strides {list(self.strides)}: the window count would be zero')
        return new_h, new_w, rows, cols

    def forward(self, x):
        x = self._input(x)
        batch, _, ori_height, ori_width = x.size()
        assert batch == 1, "only supporting batchsize 1."
        fused = ops_tta.hip_applies(x)
        final_pred = torch.zeros([1, self.num_classes, ori_height, ori_width], dtype=self._acc_dtype(x), device=x.device)
        for scale in self.scales:
            new_h, new_w, rows, cols = self._plan(scale, ori_height, ori_width)
            # cv2.resize(INTER_LINEAR) of a float image: half-pixel bilinear without antialiasing
            new_img = F.interpolate(x, size=[new_h, new_w], mode='bilinear', align_corners=False)
            flip = True if scale < 1.0 else self.flip
            preds = torch.zeros([1, self.num_classes, new_h, new_w], dtype=final_pred.dtype, device=x.device)
            use = fused and ops_tta.supported(preds, (new_h, new_w), (ori_height, ori_width))
            if use:
                for h0, h1 in rows:
                    for w0, w1 in cols:
                        use = use and self._fused_window(new_img[:, :, h0:h1, w0:w1], flip, preds[0], h0, w0)
            if use:
                rowcnt = ops_tta.counts_1d(new_h, rows).to(x.device)
                colcnt = ops_tta.counts_1d(new_w, cols).to(x.device)
                ops_tta.canvas_merge(preds[0], rowcnt, colcnt, final_pred[0], self.align_corners)
                continue
            if scale < 1.0:
                preds = self.inference(new_img, flip=True)[:, :, 0:new_h, 0:new_w]
            else:
                preds.zero_()
                count = torch.zeros([1, 1, new_h, new_w], dtype=preds.dtype, device=x.device)
                for h0, h1 in rows:
                    for w0, w1 in cols:
                        pred = self.inference(new_img[:, :, h0:h1, w0:w1], flip=self.flip)
                        preds[:, :, h0:h1, w0:w1] += pred[:, :, 0:h1 - h0, 0:w1 - w0]
                        count[:, :, h0:h1, w0:w1] += 1
                preds = preds / count
            preds = F.interpolate(preds, (ori_height, ori_width), mode='bilinear', align_corners=self.align_corners)
            final_pred += preds
        return final_pred


class _EqualWindows(TTAWrapper):
    """What TTAWrapperPC and TTAWrapperSlide share: the per-window ``inference`` of the composition and one fused view."""
    tta_window_batch = 8                # windows per model call on the fused path (config key of the same name)
    inference = TTAWrapperCTS.inference

    def _fused_view(self, x, final_pred, size, rows_lo, cols_lo, win, pad, mirror):
        """One view on the kernels: final_pred [1, C, H, W] += resize(mean over the windows of exp(.)); False, with nothing
        written, where a kernel refuses the shapes or the model's output is not a window-size map."""
        C = self.num_classes
        N = len(rows_lo) * len(cols_lo)
        out_hw = final_pred.shape[-2:]
        if not ops_slide.supported(x, C, win, win, rows_lo, cols_lo, size):
            return False
        from .. import _lib_tta as lt
        if not lt.supported(C, int(size[0]), int(size[1]), int(size[0]), int(size[1]), int(out_hw[0]), int(out_hw[1])):
            return False
        batch = ops_slide.crops(x[0], size, rows_lo, cols_lo, win, pad, mirror)
        step = max(int(self.tta_window_batch), 1)
        z = None
        for i0 in range(0, N, step):
            i1 = min(i0 + step, N)
            inp = torch.cat([batch[i0:i1], batch[N + i0:N + i1]]) if mirror else batch[i0:i1]
            zc, zsize, align = ops_tta.view_logits(self._call_model(inp, True))
            if tuple(zsize) != tuple(win) or zc.dim() != 4 or zc.shape[1] != C or zc.dtype != torch.float32:
                return False
            if z is None:
                z = zc.new_empty((2 if mirror else 1, N) + tuple(zc.shape[1:]))
                z_align = align
                if not ops_slide.supported(x, C, zc.shape[-2:], win, rows_lo, cols_lo, size):
                    return False
            if tuple(zc.shape[1:]) != tuple(z.shape[2:]) or align != z_align:
                return False
            z[0, i0:i1] = zc[:i1 - i0]
            if mirror:
                z[1, i0:i1] = zc[i1 - i0:]
        canvas = final_pred.new_empty((C, int(size[0]), int(size[1])))
        ops_slide.gather(z[0], z[1] if mirror else None, win, z_align, rows_lo, cols_lo, canvas)
        ops_tta.merge(canvas, size, False, False, final_pred[0], self.align_corners)
        return True


class TTAWrapperPC(_EqualWindows):
    MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    def __init__(self, model, scale_list, *, num_classes=59, crop_size=(512, 512), base_size=520):
        super().__init__(model, scale_list)
        self.num_classes = num_classes
        self.crop_size = crop_size
        self.base_size = base_size

    @property
    def padvalue(self):
        return [-1.0 * m / s for m, s in zip(self.MEAN, self.STD)]

    def _plan(self, scale, ori_height, ori_width):
        """(height, width) of the resized image and the windows [(lo, hi), ...] of its axes padded to the crop"""
        height, width = ops_tta.cts_size(ori_height, ori_width, self.base_size, scale)
        crop = (int(self.crop_size[0]), int(self.crop_size[1]))
        strides = ops_slide.pc_strides(crop)
        if min(strides) < 1:
            raise ValueError(f'TTAWrapperPC: crop {list(crop)} gives strides {list(strides)}: the window count would be undefined')
        rows = ops_slide.pc_windows_1d(max(height, crop[0]), crop[0], strides[0])
        cols = ops_slide.pc_windows_1d(max(width, crop[1]), crop[1], strides[1])
        return height, width, rows, cols

    def forward(self, x, ind=0):
        x = self._input(x)
        batch, _, ori_height, ori_width = x.size()
        assert batch == 1, "only supporting batchsize 1."
        assert x.shape[1] == len(self.MEAN), 'the border value is that of a normalised RGB image'
        fused = ops_slide.hip_applies(x)
        crop = (int(self.crop_size[0]), int(self.crop_size[1]))
        pad = self.padvalue
        final_pred = torch.zeros([1, self.num_classes, ori_height, ori_width], dtype=self._acc_dtype(x), device=x.device)
        for scale in self.scales:
            height, width, rows, cols = self._plan(scale, ori_height, ori_width)
            if fused and self._fused_view(x, final_pred, (height, width), [r[0] for r in rows], [c[0] for c in cols], crop, pad, True):
                continue
            # cv2.resize(INTER_LINEAR) of a float image: half-pixel bilinear without antialiasing
            new_img = F.interpolate(x, size=[height, width], mode='bilinear', align_corners=False)
            if max(height, width) <= min(crop):
                new_img = ops_slide.pad_to(new_img, crop, pad)
                preds = self.inference(new_img, flip=True)[:, :, 0:height, 0:width]
            else:
                if height < crop[0] or width < crop[1]:
                    new_img = ops_slide.pad_to(new_img, crop, pad)
                new_h, new_w = int(new_img.shape[2]), int(new_img.shape[3])
                preds = torch.zeros([1, self.num_classes, new_h, new_w], dtype=final_pred.dtype, device=x.device)
                count = torch.zeros([1, 1, new_h, new_w], dtype=final_pred.dtype, device=x.device)
                for h0, h1 in rows:
                    for w0, w1 in cols:
                        crop_img = new_img[:, :, h0:h1, w0:w1]
                        if h1 == new_h or w1 == new_w:
                            crop_img = ops_slide.pad_to(crop_img, crop, pad)
                        pred = self.inference(crop_img, flip=True)
                        preds[:, :, h0:h1, w0:w1] += pred[:, :, 0:h1 - h0, 0:w1 - w0]
                        count[:, :, h0:h1, w0:w1] += 1
                preds = preds / count
                preds = preds[:, :, :height, :width]
            preds = F.interpolate(preds, (ori_height, ori_width), mode='bilinear', align_corners=self.align_corners)
            final_pred += preds
        return final_pred


class TTAWrapperSlide(_EqualWindows):
    def __init__(self, model, scale_list, flip=True, strides=None, crop_size=None, *, num_classes=150, img_scale=(2048, 512)):
        super().__init__(model, scale_list, flip)
        self.num_classes = num_classes
        self.crop_size = crop_size if crop_size else [512, 512]
        self.strides = strides if strides else self.crop_size      # defaults to non-overlapping windows
        self.base_size = 512
        self.img_scale = img_scale
        printlog(f'Sliding window : strides : {self.strides} crop_size {self.crop_size} image_scales: {self.image_scales}')

    @property
    def image_flips(self):
        return [f for _ in self.scales for f in ((True, False) if self.flip else (False,))]

    @property
    def image_scales(self):
        """((height, width), scale) of every view: ``img_scale`` is read as (height, width) as the reference reads it"""
        return [((int(self.img_scale[0] * s), int(self.img_scale[1] * s)), s) for s in self.scales
                for _ in ((True, False) if self.flip else (False,))]

    def _plan(self, shape, scale):
        new_h, new_w = shape
        rows = ops_tta.windows_1d(new_h, int(self.crop_size[0]), int(self.strides[0])) if new_h >= 1 else []
        cols = ops_tta.windows_1d(new_w, int(self.crop_size[1]), int(self.strides[1])) if new_w >= 1 else []
        if len(rows) < 1 or len(cols) < 1:
            raise ValueError(f'TTAWrapperSlide: scale {scale} gives a {new_h} x {new_w} image with {len(rows)} x {len(cols)} windows '
                             f'of crop {list(self.crop_size)} and strides {list(self.strides)}: the window count would be zero')
        return rows, cols

    def forward(self, x):
        x = self._input(x)
        batch, _, ori_height, ori_width = x.size()
        assert batch == 1, "only supporting batchsize 1."
        fused = ops_slide.hip_applies(x)
        final_pred = torch.zeros([1, self.num_classes, ori_height, ori_width], dtype=self._acc_dtype(x), device=x.device)
        for flip, ((new_h, new_w), scale) in zip(self.image_flips, self.image_scales):
            rows, cols = self._plan((new_h, new_w), scale)
            win = (rows[0][1] - rows[0][0], cols[0][1] - cols[0][0])        # every window of a view has this size
            if fused and x.shape[1] <= 8 and self._fused_view(x, final_pred, (new_h, new_w), [r[0] for r in rows], [c[0] for c in cols],
                                                               win, [0.0] * x.shape[1], flip):
                continue
            new_img = F.interpolate(x, size=[new_h, new_w], mode='bilinear', align_corners=False)
            preds = torch.zeros([1, self.num_classes, new_h, new_w], dtype=final_pred.dtype, device=x.device)
            count = torch.zeros([1, 1, new_h, new_w], dtype=final_pred.dtype, device=x.device)
            for h0, h1 in rows:
                for w0, w1 in cols:
                    pred = self.inference(new_img[:, :, h0:h1, w0:w1], flip=flip)
                    preds[:, :, h0:h1, w0:w1] += pred[:, :, 0:h1 - h0, 0:w1 - w0]
                    count[:, :, h0:h1, w0:w1] += 1
            preds = preds / count
            preds = F.interpolate(preds, (ori_height, ori_width), mode='bilinear', align_corners=self.align_corners)
            final_pred += preds
        return final_pred
