"""Shared helpers of the operator modules (models/ops_*.py)."""


def _stream(t):
    from .. import _lib
    return _lib.stream_ptr(t.device)


def has_forward_hooks(*mods):
    """A forward or forward-pre hook is registered on one of ``mods`` or globally: a fusion that skips a module's call (the folded
    head) or hands it an alias instead of its output (a deferred norm) would hide the module's input / output from the hook."""
    from torch.nn.modules import module as _m
    return bool(_m._global_forward_hooks or _m._global_forward_pre_hooks) or \
        any(m._forward_hooks or m._forward_pre_hooks for m in mods)
