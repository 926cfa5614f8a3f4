"""Dilated 3x3 convolution (stride 1, padding == dilation) on libdcl_dconv.so (csrc/dcl_dconv.hip): the ASPP branches of DeepLabv3
and the ResNet bottlenecks whose stride was replaced by dilation.  ``DilatedConv2d`` is nn.Conv2d with the same parameters and
state_dict; inputs its kernels do not take (CPU, other dtypes, autocast, shapes ``ddc_supported`` refuses, or
``debug.cfg.dconv_hip`` off) go through nn.Conv2d.forward."""
import torch

from ..debug import cfg as _dbg


class _DilatedConv3x3(torch.autograd.Function):
    """y = conv2d(x, w, bias, stride 1, padding d, dilation d) on ddc_fwd; the backward runs ddc_dgrad on the transposed,
    tap-mirrored fragments and ddc_wgrad; the bias gradient is a plain sum."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod):
        from .. import _lib_dconv as ld
        L = ld.lib()
        n, ci, h, w = x.shape
        co, d = weight.shape[0], mod.dilation[0]
        dev = x.device
        wamax, wp, _ = mod.packed_weights()
        y = torch.empty((n, co, h, w), dtype=torch.float32, device=dev)
        nbytes = ld.workspace_bytes(ld.FWD, n, ci, co, h, w, d)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ld.check(L.ddc_fwd(ld.ptr(x), ld.ptr(wp), ld.ptr(wamax), ld.ptr(bias), n, ci, co, h, w, d, ld.ptr(ws), nbytes, ld.ptr(y),
                           ld.stream_ptr(dev)), "ddc_fwd")
        ld.calls["fwd"] += 1
        ctx.save_for_backward(x, weight)
        ctx.mod, ctx.d, ctx.has_bias = mod, d, bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        from .. import _lib_dconv as ld
        L = ld.lib()
        x, weight = ctx.saved_tensors
        n, ci, h, w = x.shape
        co, d = weight.shape[0], ctx.d
        dev = x.device
        gy = gy.contiguous()
        st = ld.stream_ptr(dev)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wamax, _, wpt = ctx.mod.packed_weights()
            gx = torch.empty_like(x)
            nbytes = ld.workspace_bytes(ld.DGRAD, n, ci, co, h, w, d)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            ld.check(L.ddc_dgrad(ld.ptr(gy), ld.ptr(wpt), ld.ptr(wamax), n, ci, co, h, w, d, ld.ptr(ws), nbytes, ld.ptr(gx), st),
                     "ddc_dgrad")
            ld.calls["dgrad"] += 1
        if ctx.needs_input_grad[1]:
            gw = torch.empty_like(weight)
            nbytes = ld.workspace_bytes(ld.WGRAD, n, ci, co, h, w, d)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            ld.check(L.ddc_wgrad(ld.ptr(x), ld.ptr(gy), n, ci, co, h, w, d, ld.ptr(ws), nbytes, ld.ptr(gw), st), "ddc_wgrad")
            ld.calls["wgrad"] += 1
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum((0, 2, 3))
        return gx, gw, gb, None


def dilated_geometry(m) -> bool:
    """3x3, stride 1, padding == dilation == (d, d) with d >= 2, groups 1, zero padding."""
    return (m.kernel_size == (3, 3) and m.stride == (1, 1) and m.groups == 1 and m.dilation[0] == m.dilation[1]
            and m.dilation[0] >= 2 and tuple(m.padding) == tuple(m.dilation) and m.padding_mode == 'zeros')


class DilatedConv2d(torch.nn.Conv2d):
    """nn.Conv2d (same parameters / state_dict) whose 3x3 / stride 1 / padding == dilation >= 2 case runs on the dilated f16x3
    kernels for contiguous fp32 CUDA inputs; every other configuration falls through to nn.Conv2d.forward."""

    def eligible(self, x):
        if not (_dbg.dconv_hip and dilated_geometry(self) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                and self.weight.dtype == torch.float32 and self.weight.is_cuda and not torch.is_autocast_enabled()
                and x.is_contiguous() and self.weight.is_contiguous()):
            return False
        from .. import _lib_dconv as ld
        n, ci, h, w = x.shape
        return ci == self.weight.shape[1] and ld.supported(n, ci, self.weight.shape[0], h, w, self.dilation[0])

    def packed_weights(self):
        """(max|w|, forward fragments, data-gradient fragments), rebuilt when the weight tensor was modified."""
        from .. import _lib_dconv as ld
        w = self.weight
        key = (w._version, w.data_ptr())
        cache = getattr(self, "_packed", None)
        if cache is None or cache[0] != key:
            wd = w.detach()
            co, ci = wd.shape[0], wd.shape[1]
            wamax = torch.empty(1, dtype=torch.float32, device=wd.device)
            wp = torch.empty(ld.packed_bytes(co, ci, False), dtype=torch.uint8, device=wd.device)
            wpt = torch.empty(ld.packed_bytes(co, ci, True), dtype=torch.uint8, device=wd.device)
            ld.check(ld.lib().ddc_pack(ld.ptr(wd), co, ci, ld.ptr(wamax), ld.ptr(wp), ld.ptr(wpt), ld.stream_ptr(wd.device)),
                     "ddc_pack")
            cache = (key, wamax, wp, wpt)
            self._packed = cache
        return cache[1], cache[2], cache[3]

    def forward(self, x):
        from .amax import refuse_pre
        refuse_pre(x, "DilatedConv2d")        # this op fuses no norm: a deferred-norm input aliases the raw pre-norm tensor
        if self.eligible(x):
            return _DilatedConv3x3.apply(x, self.weight, self.bias, self)
        return super().forward(x)


def use_dilated_conv3x3(module: torch.nn.Module) -> torch.nn.Module:
    """Switch every plain nn.Conv2d with a 3x3 / stride 1 / padding == dilation >= 2 / groups 1 geometry to DilatedConv2d in place."""
    for m in module.modules():
        if type(m) is torch.nn.Conv2d and dilated_geometry(m):
            m.__class__ = DilatedConv2d
    return module
