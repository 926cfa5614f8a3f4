"""Prediction maps on the GPU (include/dcl_pred.h, utils/predict.py): dpr_predict against the arg-max of the float64 evaluation of
the same resize (computed in torch on the CPU, tests/_pred_cases.py), exact against torch.argmax on the identity level, the two
tables, the outputs that were not asked for, UpsampledLogits and the confusion matrix, run-to-run equality; dpr_panel against its
torch composition.

The comparison leaves a pixel out only when the float64 top-two margin is below 1e-5 * max|z| (about 20 x what four fp32 roundings
of a convex combination can move a difference), and at most 1 % of a case's pixels may be left out: a condition, not a tolerance
(the float64 evaluation alone leaves out at most one pixel per case on these seeds)."""
import os

import pytest
import torch

import _pred_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_pred
    _lib_pred.lib()
    return torch.device("cuda:0")


def _lazy(z, H, W, align):
    from mscs_amd.models.ops_logits import UpsampledLogits
    return UpsampledLogits(z, (H, W), align)


def _check(ids, ref, ok, what):
    ids = ids.cpu().long()
    left_out = float((~ok).float().mean())
    wrong = int((ids[ok] != ref[ok]).sum())
    print(what, "left out:", int((~ok).sum()), "of", ok.numel(), "wrong among the rest:", wrong)
    assert left_out <= cases.MAX_LEFT_OUT, what
    assert wrong == 0, what


@pytest.mark.parametrize("align", (False, True), ids=("ac0", "ac1"))
@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_predict_against_float64(dev, shape, align):
    from mscs_amd import _lib_pred as lp
    from mscs_amd.utils import predict_maps
    C, h, w, H, W = shape
    z, ref, ok = cases.reference(C, h, w, H, W, align)
    lut, pal = cases.tables()
    before = lp.calls["predict"]
    ids, mapped, rgb = predict_maps(_lazy(z.to(dev), H, W, align), lut.to(dev), pal.to(dev))
    assert lp.calls["predict"] == before + 1
    assert ids.dtype == torch.uint8 and tuple(ids.shape) == (1, H, W) and tuple(rgb.shape) == (1, H, W, 3)
    _check(ids, ref, ok, (shape, align))
    assert torch.equal(mapped.cpu(), lut[ids.cpu().long()]) and torch.equal(rgb.cpu(), pal[ids.cpu().long()])
    again = predict_maps(_lazy(z.to(dev), H, W, align), lut.to(dev), pal.to(dev))
    assert all(torch.equal(a, b) for a, b in zip((ids, mapped, rgb), again))           # bitwise the same from run to run


def test_predict_batch_of_three(dev):
    from mscs_amd.utils import predict_maps
    C, h, w, H, W = cases.SHAPES[1]
    z, ref, ok = cases.reference(C, h, w, H, W, False, 3)
    lut, pal = cases.tables()
    ids, mapped, rgb = predict_maps(_lazy(z.to(dev), H, W, False), lut.to(dev), pal.to(dev))
    assert tuple(ids.shape) == (3, H, W)
    _check(ids, ref, ok, "N = 3")
    assert torch.equal(mapped.cpu(), lut[ids.cpu().long()]) and torch.equal(rgb.cpu(), pal[ids.cpu().long()])
    one = predict_maps(_lazy(z[1:2].to(dev), H, W, False))[0]
    assert torch.equal(one[0], ids[1])                                                  # an image does not depend on its neighbours


def test_identity_level_is_torch_argmax(dev):
    from mscs_amd import _lib_pred as lp
    from mscs_amd.utils import predict_maps
    C, h, w, H, W = cases.IDENTITY
    z = cases.logits(C, h, w, 2)
    twin = z.clone()
    twin[:, 7] = twin[:, 3]                                    # two identical class planes: the lower index wins
    twin[:, 3] += 100.0
    twin[:, 7] += 100.0
    nans = z.clone()
    g = torch.Generator().manual_seed(4)
    nans.view(-1)[torch.randperm(nans.numel(), generator=g)[:400]] = float("nan")
    nans[0, :, 0, 0] = float("nan")                            # every class a NaN: the first one
    for name, t in (("random", z), ("twin planes", twin), ("NaNs", nans)):
        before = lp.calls["predict"]
        for view in (t, t[:, :, :, :21].contiguous(), t[:, :, :, 1:].contiguous()):       # 16-byte loads, a row length of 21, of 23
            ids = predict_maps(view.to(dev))[0]
            assert torch.equal(ids.cpu().long(), view.argmax(1)), name
        assert lp.calls["predict"] == before + 3
    assert bool((predict_maps(twin.to(dev))[0] == 3).all())
    # the same identical planes through an up-sampling case
    C, h, w, H, W = cases.SHAPES[1]
    low = cases.logits(C, h, w)
    low[:, 7] = low[:, 3]
    low[:, 3] += 100.0
    low[:, 7] += 100.0
    for align in (False, True):
        assert bool((predict_maps(_lazy(low.to(dev), H, W, align))[0] == 3).all())


def test_outputs_not_asked_for_are_not_written(dev):
    from mscs_amd import _lib_pred as lp
    C, h, w, H, W = cases.SHAPES[2]
    z = cases.logits(C, h, w).to(dev)
    lut, pal = (t.to(dev) for t in cases.tables())
    ids = torch.empty(1, H, W, dtype=torch.uint8, device=dev)
    mapped = torch.full((1, H, W), 77, dtype=torch.uint8, device=dev)
    rgb = torch.full((1, H, W, 3), 78, dtype=torch.uint8, device=dev)
    L, st = lp.lib(), lp.stream_ptr(dev)
    lp.check(L.dpr_predict(z.data_ptr(), 1, C, h, w, H, W, 0, None, None, ids.data_ptr(), None, None, st), "dpr_predict")
    torch.cuda.synchronize()
    assert bool((mapped == 77).all()) and bool((rgb == 78).all())
    # a table without its output, or the reverse, is refused before a launch
    assert L.dpr_predict(z.data_ptr(), 1, C, h, w, H, W, 0, lut.data_ptr(), None, ids.data_ptr(), None, None, st) != 0
    assert L.dpr_predict(z.data_ptr(), 1, C, h, w, H, W, 0, None, None, ids.data_ptr(), None, rgb.data_ptr(), st) != 0
    assert b"table" in L.dpr_last_error()
    assert L.dpr_predict(z.data_ptr(), 1, 257, h, w, H, W, 0, None, None, ids.data_ptr(), None, None, st) != 0
    torch.cuda.synchronize()
    assert bool((mapped == 77).all()) and bool((rgb == 78).all())


def test_upsampled_logits_and_the_confusion_matrix(dev):
    from mscs_amd import _lib_pred as lp
    from mscs_amd.utils import predict_maps, t_get_confusion_matrix
    C, h, w, H, W = cases.SHAPES[2]
    z = cases.logits(C, h, w, 2).to(dev)
    out = _lazy(z, H, W, True)
    ids = predict_maps(out)[0]
    assert out.pred is ids and out._full is None                                        # full-size logits were never formed
    raw = torch.empty_like(ids)
    lp.check(lp.lib().dpr_predict(z.data_ptr(), 2, C, h, w, H, W, 1, None, None, raw.data_ptr(), None, None, lp.stream_ptr(dev)),
             "dpr_predict")
    assert torch.equal(raw, ids)
    target = torch.randint(0, C + 1, (2, H, W), generator=torch.Generator().manual_seed(6)).to(dev)
    cm = t_get_confusion_matrix(out, target, "CITYSCAPES")
    assert out._full is None
    want = torch.bincount(ids.long().reshape(-1) * (C + 1) + target.reshape(-1), minlength=C * (C + 1)).view(C, C + 1)[:, :C]
    assert torch.equal(cm.long(), want)


def test_switch_off_takes_the_composition(dev, monkeypatch):
    from mscs_amd import _lib_pred as lp
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.utils import predict_maps
    C, h, w, H, W = cases.SHAPES[2]
    z, ref, ok = cases.reference(C, h, w, H, W, True)
    lut, pal = cases.tables()
    monkeypatch.setattr(dbg, "pred_hip", False)
    before = lp.calls["predict"]
    ids, mapped, rgb = predict_maps(_lazy(z.to(dev), H, W, True), lut, pal)
    assert lp.calls["predict"] == before and ids.is_cuda and ids.dtype == torch.uint8
    _check(ids, ref, ok, "composition")
    assert torch.equal(mapped.cpu(), lut[ids.cpu().long()]) and torch.equal(rgb.cpu(), pal[ids.cpu().long()])


@pytest.mark.parametrize("ldtype", (torch.uint8, torch.int64, torch.int32), ids=("u8", "i64", "i32"))
def test_panel_matches_its_composition(dev, monkeypatch, ldtype):
    from mscs_amd import _lib_pred as lp
    from mscs_amd.debug import cfg as dbg
    from mscs_amd.utils import panel_image
    g = torch.Generator().manual_seed(9)
    H, W = 18, 22
    img = torch.randn(3, H, W, generator=g) * 1.5
    img[0, 0, :4] = torch.tensor([-2.1179039, 2.2489083, 0.0, (0.5 / 255 - 0.485) / 0.229])      # the ends of the range, a half
    lbl = torch.randint(0, 21, (H, W), generator=g).to(ldtype)
    if ldtype != torch.uint8:
        lbl[1, :3] = torch.tensor([-1, 256, 255], dtype=ldtype)
    ids = torch.randint(0, 20, (H, W), generator=g, dtype=torch.uint8)
    pal = cases.tables()[1]
    before = lp.calls["panel"]
    got = panel_image(img.to(dev), lbl.to(dev), ids.to(dev), pal.to(dev), label_ignore=20, ids_ignore=19)
    assert lp.calls["panel"] == before + 1 and got.dtype == torch.uint8 and tuple(got.shape) == (H, 3 * W, 3)
    monkeypatch.setattr(dbg, "pred_hip", False)
    want_gpu = panel_image(img.to(dev), lbl.to(dev), ids.to(dev), pal.to(dev), label_ignore=20, ids_ignore=19)
    want_cpu = panel_image(img, lbl, ids, pal, label_ignore=20, ids_ignore=19)
    assert lp.calls["panel"] == before + 1
    assert torch.equal(got, want_gpu) and torch.equal(got.cpu(), want_cpu)
    assert bool((got[:, W:2 * W][(lbl == 20).to(dev)] == 0).all()) and bool((got[:, 2 * W:][(ids == 19).to(dev)] == 0).all())
    # a width of 24 takes the 4-byte stores: the same values
    img2, lbl2, ids2 = (torch.cat([t, t[..., :2]], dim=-1) for t in (img, lbl, ids))
    monkeypatch.setattr(dbg, "pred_hip", True)
    got2 = panel_image(img2.to(dev), lbl2.to(dev), ids2.to(dev), pal.to(dev), label_ignore=20, ids_ignore=19)
    assert torch.equal(got2.cpu(), panel_image(img2, lbl2, ids2, pal, label_ignore=20, ids_ignore=19))


def test_writer_on_cuda_tensors(dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import numpy as np
    from mscs_amd.utils import PredictionWriter
    g = torch.Generator().manual_seed(12)
    maps = [torch.randint(0, 256, (33, 47), generator=g, dtype=torch.uint8) for _ in range(5)]
    cols = [torch.randint(0, 256, (33 + i, 47, 3), generator=g, dtype=torch.uint8) for i in range(5)]
    with PredictionWriter(tmp_path, depth=2) as wr:
        for i in range(5):                                     # ten files through two slots of changing size
            wr.write(f"submit/{i}.png", maps[i].to(dev))
            wr.write(f"debug/{i}.png", cols[i].to(dev))
    assert wr.written == 10 and not wr._thread.is_alive()
    for i in range(5):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "submit" / f"{i}.png")), maps[i].numpy())
        assert np.array_equal(np.asarray(Image.open(tmp_path / "debug" / f"{i}.png")), cols[i].numpy())


def test_manager_saves_on_the_gpu(dev, tmp_path):
    """infer() with save_outputs on the device: the model hands out its 1/4 map, files and confusion matrix come from dpr_predict's
    ids; validate() with save_valid_images writes dpr_panel's panels."""
    Image = pytest.importorskip("PIL.Image")
    import numpy as np
    from mscs_amd import _lib_pred as lp
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import class_palette, set_verbosity, submission_lut
    from mscs_amd.utils.metrics import take_out_of_range
    set_verbosity(40)
    rng = (torch.get_rng_state(), np.random.get_state())
    take_out_of_range(dev)                      # (a process-wide counter: what earlier modules' out-of-range targets left is not this run's)

    def cfg(sub, **extra):
        c = {"name": "pred", "mode": "training", "manager": "HRNet", "cuda": True, "parallel": False, "gpu_device": [0], "seed": 3,
             "log_every_n_steps": 1000, "log_path": str(tmp_path / sub), "run_id": "run0", "save_checkpoints": False,
             "graph": {"model": "HRNet", "backbone": "hrnet18", "sync_bn": False, "pretrained": False, "align_corners": True},
             "data": {"dataset": "CITYSCAPES", "experiment": 1, "batch_size": 2, "num_workers": 0, "synthetic": True,
                      "synthetic_length": 2, "synthetic_valid_length": 2, "synthetic_mode": "blocky",
                      "transform_values": {"crop_shape": [64, 128]}},
             "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
             "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True, "epochs": 1}}
        c.update(extra)
        return c
    try:
        m = HRNetManager(cfg("train", save_valid_images=True), autostart=False)
        m.setup()
        path = m.save_checkpoint(path=str(tmp_path / "chk.pt"))
        calls = dict(lp.calls)
        miou = m.validate()
        assert 0.0 <= miou <= 1.0 and lp.calls["panel"] == calls["panel"] + 2 and lp.calls["predict"] == calls["predict"] + 2
        panels = sorted(os.listdir(tmp_path / "train" / "run0" / "valid_images"))
        assert panels == ["record_00_step0.png", "record_01_step0.png"]
        assert np.asarray(Image.open(tmp_path / "train" / "run0" / "valid_images" / panels[0])).shape == (64, 3 * 128, 3)
        m2 = HRNetManager(cfg("infer", mode="inference", load_checkpoint=path, tta=False, save_outputs=True), autostart=False)
        m2.setup()
        calls = dict(lp.calls)
        mious = m2.infer()
        assert lp.calls["predict"] == calls["predict"] + 2 and m2.model.lazy_eval_logits is False
        assert 0.0 <= float(mious["mean_iou"]) <= 1.0 and list(mious["per_class_iou"].shape) == [19]
        base = tmp_path / "infer" / "run0" / "outputs" / "val"
        lut, pal = submission_lut("CITYSCAPES", 1), class_palette("CITYSCAPES", 1)
        from mscs_amd.utils import predict_maps
        with torch.no_grad():
            for i, batch in enumerate(m2.data_loaders["valid_loader"]):
                out = m2._call_lazy(m2.model, batch[0].to(dev).float())
                assert hasattr(out, "materialize") and tuple(out.lowres.shape[-2:]) == (16, 32)     # the 1/4 map was handed out
                _, mapped, rgb = predict_maps(out, lut, pal)                            # the same kernels on the same input
                submit = np.asarray(Image.open(base / "submit" / f"record_{i:06d}.png"))
                debug = np.asarray(Image.open(base / "debug" / f"record_{i:06d}.png"))
                assert np.array_equal(submit, mapped[0].cpu().numpy()) and np.array_equal(debug, rgb[0].cpu().numpy())
        # without the key: no directory, today's path
        m3 = HRNetManager(cfg("plain", mode="inference", load_checkpoint=path, tta=False), autostart=False)
        m3.setup()
        calls = dict(lp.calls)
        m3.infer()
        assert not os.path.exists(tmp_path / "plain" / "run0") and lp.calls == calls
    finally:
        torch.set_rng_state(rng[0])
        np.random.set_state(rng[1])
