"""Footprint of the Lovasz-Softmax entries at the C ABI (include/dcl_lovasz.h): dlv_lovasz_fwd and dlv_lovasz_bwd on guarded
buffers (tests/_footprint.py): every band intact, coefficients / loss / gradient fully written, finite and independent of what
lies outside the inputs, and a workspace of exactly dlv_workspace_bytes whose bands stay untouched."""
import pytest
import torch

from _footprint import run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_lovasz
    _lib_lovasz.lib()
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


# (N, C, H, W, per_image, ignore id or None, share of ignored pixels, label dtype, classes considered or None)
CASES = [
    (2, 5, 37, 53, 0, None, 0.0, torch.int64, None),             # odd sizes, short tiles, nothing ignored
    (2, 19, 96, 160, 1, 19, 0.3, torch.uint8, None),             # several tiles per segment, 30 % ignored, per image
    (3, 7, 37, 53, 0, 7, 0.3, torch.int32, [0, 2, 5]),           # one full and one partial tile, a class list
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_lovasz_entries_footprint(dev, case):
    from mscs_amd import _lib_lovasz as lv
    from mscs_amd.losses import LovaszSoftmax
    N, C, H, W, per_image, ignore, share, ldt, consider = case
    L = lv.lib()
    st = lv.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(N * C + H)
    logits = torch.randn(N, C, H, W, device=dev, generator=g) * 2.0
    label = torch.randint(0, C, (N, H, W), device=dev, generator=g)
    if ignore is not None:
        label[torch.rand(N, H, W, device=dev, generator=g) < share] = ignore
    mask = None
    if consider is not None:
        mask = torch.zeros(C, dtype=torch.uint8, device=dev)
        mask[consider] = 1
    up = torch.full((1,), 0.75, device=dev)
    nbytes = lv.workspace_bytes(N, C, H * W, bool(per_image))
    assert nbytes > 16 * N * C * H * W

    def body(ar):
        x, t = ar.inp(logits, "logits"), ar.inp(label.to(ldt), "labels")
        ws = ar.out(nbytes, torch.uint8, "workspace")
        assert ws.data_ptr() % 256 == 0
        coef, loss = ar.out((N, C, H, W), name="coef"), ar.out(1, name="loss")
        lv.check(L.dlv_lovasz_fwd(_p(x), _p(t), t.element_size(), N, C, H * W, per_image, int(ignore is not None), ignore or 0,
                                  int(consider is None), _p(None if mask is None else ar.inp(mask, "consider")), _p(ws), nbytes,
                                  _p(coef), _p(loss), st), "dlv_lovasz_fwd")
        dx = ar.out((N, C, H, W), name="dlogits")
        lv.check(L.dlv_lovasz_bwd(_p(x), _p(coef), _p(ar.inp(up, "upstream")), N, C, H * W, _p(dx), st), "dlv_lovasz_bwd")
        return {"coef": coef, "loss": loss, "dlogits": dx}
    got = run_both(dev, body, ("lovasz", case))

    # and the values are those of the module (which takes the same entries through torch-allocated buffers)
    cfg = {"dataset": "CITYSCAPES", "experiment": 1, "per_image": bool(per_image), "classes_to_ignore": ignore}
    if consider is not None:
        cfg["classes_to_consider"] = consider
    x = logits.clone().requires_grad_(True)
    loss = LovaszSoftmax(cfg)(x, label.to(ldt))
    (0.75 * loss).backward()
    assert torch.equal(got["loss"][0], loss.detach()) and torch.equal(got["dlogits"], x.grad)
    if ignore is not None:
        assert bool(got["coef"][(label == ignore)[:, None].expand(N, C, H, W)].eq(0).all())
