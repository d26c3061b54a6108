"""The device input path (csrc/device_aug.hip): TransformFixMatch on the GPU is byte-identical to the host
library's -- every pool op at every magnitude and sign, the resize / crop cases, the whole pipeline over the
batch builder's own random streams, and DeviceBatcher against HostBatcher.  torch.equal everywhere: there is
no tolerance."""
import numpy as np
import pytest
import torch

from endossl import host_aug

pytestmark = pytest.mark.gpu

S_OP = 48


def _sources(n, seed=0):
    """tests/test_gpu_host_input.py's frames: an up-scaled noise pattern, ragged sizes."""
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (40, 52, 3), dtype=np.uint8)
    return [host_aug.resize_bilinear(base ^ np.uint8(i * 37 % 256), (300 + 7 * i, 220 + 5 * i)) for i in range(n)]


def _chw(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


def _contents():
    g = np.random.default_rng(4)
    noise = g.integers(0, 256, (S_OP, S_OP, 3), dtype=np.uint8)
    smooth = host_aug.resize_bilinear(g.integers(0, 256, (6, 7, 3), dtype=np.uint8), (S_OP, S_OP))
    flat = np.empty((S_OP, S_OP, 3), np.uint8)
    flat[:] = (93, 0, 255)  # one level per channel: autocontrast's hi <= lo, equalize's single bin
    two = np.empty((S_OP, S_OP, 3), np.uint8)
    two[:] = (200, 31, 255)  # two levels, the rarer one below 255 pixels: equalize's step == 0 with two bins
    two[5:9, 7:29] = (40, 30, 0)
    return {"noise": noise, "smooth": smooth, "flat": flat, "two_level": two}


def _op_plan(op, v, neg, rect=(1, 1, 0, 0)):
    """One applied op, nothing else: no flip, the crop window on the image itself, an empty Cutout."""
    pad = int(S_OP * 0.125)
    return host_aug.aug_plan_from_draws(S_OP, 0, pad, pad, [op, 5], [v, 1], [1, 0], [neg, 0], rect)


CUTOUTS = [(0, 0, 7, 9), (40, 0, 48, 12), (0, 38, 16, 48), (36, 40, 48, 48), (10, 12, 26, 28), (-3, -4, 5, 6),
           (47, 47, 63, 63)]


@pytest.mark.parametrize("name", ["noise", "smooth", "flat", "two_level"])
def test_every_op_magnitude_and_sign(name):
    """One es_aug_strong_u8 launch: 14 ops x v = 1..9 x both signs (and Cutout at the corners and inside) on one
    content, each output against host_aug.aug_op / fill_rect."""
    img = _contents()[name]
    cases = [(op, v, neg) for op in range(14) for v in range(1, 10) for neg in (0, 1)]
    plans = [_op_plan(*c) for c in cases] + [_op_plan(5, 1, 0, r) for r in CUTOUTS]
    want = [host_aug.aug_op(img, *c) for c in cases] + [host_aug.fill_rect(img, r, 127) for r in CUTOUTS]
    weak = _chw(img).cuda().unsqueeze(0).repeat(len(plans), 1, 1, 1)
    got = host_aug.device_strong(weak, plans).cpu()
    for i, w in enumerate(want):
        assert torch.equal(got[i], _chw(w)), (name, (cases + CUTOUTS)[i])


def _ragged(S, is_crop):
    R = host_aug.resize_side(S, is_crop)
    g = np.random.default_rng(S + is_crop)
    sizes = [(R, 57), (45, R), (R, R), (30, 22), (301, 227), (R, 2 * R + 3), (3 * R - 1, R), (S + 1, S + 1), (500, 375)]
    return [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]


@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("is_crop", [True, False])
def test_resize_and_crop_equal_host_eval(S, is_crop):
    """Frames with w == R, h == R, both, up-scaling (30 x 22) and down-scaling (301 x 227) by non-integer
    ratios: the weak view is transform_batch(kind='eval')'s."""
    imgs = _ragged(S, is_crop)
    (want,) = host_aug.transform_batch(imgs, S, "eval", is_crop, threads=4)
    (got,) = host_aug.device_transform_batch(imgs, S, "eval", is_crop)
    assert got.is_cuda and torch.equal(got.cpu(), want)


def _coverage(imgs, S, seed):
    entries, _, _ = host_aug.fixmatch_device_plan([a.shape[1] for a in imgs], [a.shape[0] for a in imgs], S, True,
                                                  seed=seed)
    es = host_aug.plan_entries(entries)
    ops = {o.op for e in es for o in e.ops if o.applied}
    flips = {e.flip for e in es}
    clipped = any(e.rect[0] == 0 or e.rect[1] == 0 or e.rect[2] > S - 1 or e.rect[3] > S - 1 for e in es)
    return ops, flips, clipped


@pytest.mark.parametrize("n,S", [(256, 32), (32, 64), (4, 224)])
def test_whole_pipeline_equals_host_fixmatch(n, S):
    srcs = _sources(8) + _ragged(S, True)
    imgs = [srcs[i % len(srcs)] for i in range(n)]
    for seed in (5, (3 << 32) ^ 1):
        ww, ws_ = host_aug.transform_batch(imgs, S, "fixmatch", True, seed=seed, threads=8)
        gw, gs = host_aug.device_transform_batch(imgs, S, "fixmatch", True, seed=seed)
        assert torch.equal(gw.cpu(), ww)
        bad = [i for i in range(n) if not torch.equal(gs[i].cpu(), ws_[i])]
        assert not bad, (seed, bad[:8])
        if n == 256:  # P(an op never applied) < 1e-7: the plan itself meets the coverage condition
            ops, flips, clipped = _coverage(imgs, S, seed)
            assert ops == set(range(14)) and flips == {0, 1} and clipped


@pytest.mark.parametrize("resident", [False, True])
def test_device_batcher_equals_host_batcher(resident):
    srcs = _sources(6)
    hb = host_aug.HostBatcher(srcs, batch=8, size=64, seed=3, threads=4, device="cuda")
    db = host_aug.DeviceBatcher(srcs, batch=8, size=64, seed=3, device="cuda", resident=resident)
    for step in range(3):
        hw, hs = hb.next()
        dw, ds = db.next()
        assert (db._indices(step) == hb._indices(step)).all()
        torch.cuda.synchronize()
        assert dw.is_cuda and ds.is_cuda
        assert torch.equal(dw, hw) and torch.equal(ds, hs), step
    ev = host_aug.DeviceBatcher(srcs, batch=5, size=64, kind="eval", seed=3, resident=resident)
    (x,) = ev.next()
    (want,) = host_aug.transform_batch([srcs[i] for i in ev._indices(0)], 64, "eval", True)
    assert torch.equal(x.cpu(), want)


def test_fixmatch_step_on_device_batches():
    from endossl.fixmatch import FixMatch
    from endossl.utils import AttrDict
    from endossl.vit import NativeViT, ViTConfig
    B, MU = 2, 2
    model = NativeViT(ViTConfig(depth=2), seed=0)
    tr = FixMatch(model, device=torch.device("cuda"))
    cfg = AttrDict(DATA=AttrDict(BATCH_SIZE=B, MU=MU, IMG_SIZE=224, TARGET_NAME="target"),
                   MODEL=AttrDict(NAME="vit_small_patch16_224", NUM_CLASSES=23),
                   TRAIN=AttrDict(IS_FREEZE=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, EVAL_STEP=1,
                                  CLS_WEIGHT=False, THRES=0.5, T=1.0, LAMBDA_U=1.0, EPOCHS=1, WARMUP_EPOCHS=0,
                                  DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="const"))
    tr.get_dataloader((None, None), None)
    tr.get_config(cfg)
    srcs = _sources(5)
    lab = host_aug.HostBatcher(srcs, batch=B, size=224, kind="labeled", seed=1, threads=2)
    unl = host_aug.DeviceBatcher(srcs, batch=B * MU, size=224, kind="fixmatch", seed=2)
    for _ in range(2):
        (x,) = lab.next()
        uw, us = unl.next()
        y = torch.randint(0, 23, (B,), device="cuda")
        out = tr.step(((x, y), ((uw, us), None)))
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]).item()
