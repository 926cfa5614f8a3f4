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
gone, and a window grid with no rows or columns raises instead of dividing by a zero count."""
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.parallel import DistributedDataParallel as ddp

from ..utils import printlog
from . import ops_tta


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
