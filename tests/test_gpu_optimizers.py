"""The AdamW and SGD-Nesterov sweeps on the MI355X (es_adamw_ema_step, es_sgd_ema_step) against
torch.optim.AdamW / torch.optim.SGD on the CPU -- the reference's optimizers (code/optimizer.py:43-49) over its
two param groups -- and the trainers that reach them through opt_func.

Bar: rtol 1e-6, atol 1e-7, that of test_adam_ema_step_vs_torch_adam.  Bit equality with CPU torch is not
attainable (its add(alpha=) contracts to an FMA, the kernels round every operation); the two orders emulated in
unfused fp32 on the CPU stay inside this bar over three steps.  Every comparison prints its worst difference
before it asserts.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from endossl._lib import call, ptr  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 1e-6, 1e-7
D = 0.999  # EMA decay
G = 64  # floats per class-map byte
BIG = 4096 * 256 * 4 + 192  # one full stride of the capped grid (4096 x 256 float4) + a 3-granule tail
SIZES = [64, 64 * 301, BIG]
SENTINEL = 7.0  # what the class-0 slices of the moment buffers hold: the sweep must not touch them


def S():
    return torch.cuda.current_stream().cuda_stream


def _close(what, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    diff = (got - want).abs()
    over = int((diff > ATOL + RTOL * want.abs()).sum())
    print(f"{what}: max|diff| {diff.max().item() if diff.numel() else 0.0:.3e}, {over}/{diff.numel()} over the bar")
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


def _classes(n):
    """The class map of a test size: one granule of group 0; 1,2,0,1,2,0... changing at every granule; large
    blocks with the tail past the full grid stride holding one granule of each class."""
    g = n // G
    if g == 1:
        return torch.tensor([1], dtype=torch.uint8)
    lut = torch.tensor([1, 2, 0], dtype=torch.uint8)
    if g == 301:
        return lut[torch.arange(g) % 3]
    cls = lut[(torch.arange(g) // 1021) % 3]
    cls[-3:] = torch.tensor([2, 0, 1], dtype=torch.uint8)
    return cls


def _launch(kind, p, g, bufs, e, cls, t, lr=(1e-3, 1e-3), wd=(0.05, 0.0), grad_scale=1.0):
    n = p.numel()
    if kind == "AdamW":
        bc1, bc2 = 1 - 0.9 ** t, 1 - 0.999 ** t
        call("es_adamw_ema_step", ptr(p), ptr(g), ptr(bufs[0]), ptr(bufs[1]), ptr(e), ptr(cls), n, 0.9, 0.999, 1 - 0.9,
             1 - 0.999, 1e-8, math.sqrt(bc2), -(lr[0] / bc1), -(lr[1] / bc1), 1 - lr[0] * wd[0], 1 - lr[1] * wd[1], D, 1.0 - D,
             grad_scale, S())
    else:
        call("es_sgd_ema_step", ptr(p), ptr(g), ptr(bufs[0]), ptr(e), ptr(cls), n, 0.9, -lr[0], -lr[1], wd[0], wd[1],
             1, D, 1.0 - D, grad_scale, S())


_NBUF = {"AdamW": ("exp_avg", "exp_avg_sq"), "SGD": ("momentum_buffer",)}


def _torch_steps(kind, p0, grads, per_float, lr=(1e-3, 1e-3), wd=(0.05, 0.0)):
    """torch.optim on the CPU: the class-1 and class-2 elements as two tensors in two param groups, the
    class-0 elements owned by no optimizer.  Returns the full parameter vector, the state buffers scattered
    back (SENTINEL on class 0) and the EMA of the full vector."""
    idx = [(per_float == c).nonzero().squeeze(1) for c in (1, 2)]
    ts = [p0[i].clone().requires_grad_(True) for i in idx]
    groups = [{"params": [t], "lr": l, "weight_decay": w} for t, l, w in zip(ts, lr, wd)]
    if kind == "AdamW":
        opt = torch.optim.AdamW(groups, betas=(0.9, 0.999), eps=1e-8)
    else:
        opt = torch.optim.SGD(groups, lr=lr[0], momentum=0.9, nesterov=True)
    full, er = p0.clone(), p0.clone()
    for gr in grads:
        for t, i in zip(ts, idx):
            t.grad = gr[i].clone()
        opt.step()
        for t, i in zip(ts, idx):
            full[i] = t.detach()
        er = D * er + (1.0 - D) * full
    bufs = []
    for b in _NBUF[kind]:
        flat = torch.full_like(p0, SENTINEL)
        for t, i in zip(ts, idx):
            flat[i] = opt.state[t][b] if i.numel() else flat[i]
        bufs.append(flat)
    return full, bufs, er


_CACHE = {}


def _case(kind, n):
    """Inputs and the CPU reference of one (rule, size), computed once and left unchanged."""
    if (kind, n) not in _CACHE:
        gen = torch.Generator().manual_seed(6 + n % 97)
        cls = _classes(n)
        per_float = cls.repeat_interleave(G)
        p0 = torch.randn(n, generator=gen)
        grads = [torch.randn(n, generator=gen) * 10 ** (-i) for i in range(3)]
        _CACHE[(kind, n)] = (cls, per_float, p0, grads, _torch_steps(kind, p0, grads, per_float))
    return _CACHE[(kind, n)]


def _device_state(kind, p0, per_float):
    init = torch.where(per_float == 0, torch.full_like(p0, SENTINEL), torch.zeros_like(p0))
    return p0.to(DEV), [init.to(DEV) for _ in _NBUF[kind]], p0.to(DEV)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_sweep_vs_torch_optim(kind, n):
    cls, per_float, p0, grads, (pr, br, er) = _case(kind, n)
    p, bufs, e = _device_state(kind, p0, per_float)
    dcls = cls.to(DEV)
    for t, gr in enumerate(grads, 1):
        _launch(kind, p, gr.to(DEV), bufs, e, dcls, t)
    torch.cuda.synchronize()
    _close(f"{kind} n={n} p", p, pr)
    for name, b, r in zip(_NBUF[kind], bufs, br):
        _close(f"{kind} n={n} {name}", b, r)
    _close(f"{kind} n={n} ema", e, er)
    frozen = per_float == 0
    if frozen.any():  # class 0: parameters and moments keep their bits, the EMA still blends
        assert torch.equal(p.cpu()[frozen], p0[frozen])
        for b in bufs:
            assert torch.equal(b.cpu()[frozen], torch.full_like(p0[frozen], SENTINEL))
        ef = p0[frozen]
        for _ in grads:
            ef = D * ef + (1.0 - D) * p0[frozen]
        _close(f"{kind} n={n} ema of class 0", e.cpu()[frozen], ef)
    assert float((p.cpu()[~frozen] != p0[~frozen]).float().mean()) > 0.99  # the trained elements moved


@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_grad_scale_and_per_group_lr(kind):
    """One step with grad_scale 0.5 = the torch step on 0.5 g; each group with its own lr and weight decay."""
    n = 64 * 301
    cls, per_float, p0, grads, _ = _case(kind, n)
    lr, wd = (2e-3, 5e-4), (0.05, 0.0)
    pr, br, er = _torch_steps(kind, p0, [0.5 * grads[0]], per_float, lr=lr, wd=wd)
    p, bufs, e = _device_state(kind, p0, per_float)
    _launch(kind, p, grads[0].to(DEV), bufs, e, cls.to(DEV), 1, lr=lr, wd=wd, grad_scale=0.5)
    torch.cuda.synchronize()
    _close(f"{kind} grad_scale p", p, pr)
    for name, b, r in zip(_NBUF[kind], bufs, br):
        _close(f"{kind} grad_scale {name}", b, r)
    _close(f"{kind} grad_scale ema", e, er)


@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_null_ema_updates_parameters_only(kind):
    n = 64 * 301
    cls, per_float, p0, grads, _ = _case(kind, n)
    pr, br, _ = _torch_steps(kind, p0, grads[:1], per_float)
    p, bufs, e = _device_state(kind, p0, per_float)
    _launch(kind, p, grads[0].to(DEV), bufs, None, cls.to(DEV), 1)
    torch.cuda.synchronize()
    _close(f"{kind} no-ema p", p, pr)
    for name, b, r in zip(_NBUF[kind], bufs, br):
        _close(f"{kind} no-ema {name}", b, r)
    assert torch.equal(e.cpu(), p0)  # the EMA buffer the call was not given
    assert torch.equal(p.cpu()[per_float == 0], p0[per_float == 0])


# ------------------------------------------------------------------------------------ trainers
class _It:
    def __init__(self, items):
        self._it = iter(items)

    def next(self):
        return next(self._it)

    __next__ = next


class _DS:
    def __init__(self, df):
        self.df = df


class _DL:
    def __init__(self, items, df=None):
        self.items, self.dataset = items, _DS(df)

    def __iter__(self):
        return _It(self.items)

    def __len__(self):
        return len(self.items)


def _cfg(thres, steps, B, MU, img=64, freeze=False):
    from endossl.utils import AttrDict
    return AttrDict(
        DATA=AttrDict(BATCH_SIZE=B, MU=MU, IMG_SIZE=img, TARGET_NAME="target"),
        MODEL=AttrDict(NAME="vit_tiny_test", NUM_CLASSES=23, MARGIN="None", TYPE_SEMI="FixMatch"),
        TRAIN=AttrDict(IS_FREEZE=freeze, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, EVAL_STEP=steps, CLS_WEIGHT=True,
                       THRES=thres, T=1.0, LAMBDA_U=1.0, IS_SSL=True, EPOCHS=1, WARMUP_EPOCHS=0, DECAY_EPOCHS=10,
                       WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="const", FREQ_EVAL=1))


def _reference_optimizer(model, opt_func, lr):
    """code/optimizer.py:13-53 over a CPU module."""
    skip = model.no_weight_decay()
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if len(p.shape) == 1 or name.endswith(".bias") or name in skip else decay).append(p)
    groups = [{"params": decay}, {"params": no_decay, "weight_decay": 0.}]
    if opt_func == "AdamW":
        return torch.optim.AdamW(groups, eps=1e-8, betas=(0.9, 0.999), lr=lr, weight_decay=0.05)
    return torch.optim.SGD(groups, momentum=0.9, nesterov=True, lr=lr, weight_decay=0.05)


def _checked_step(tr, shadow, ref_opt, batch, tag):
    """One trainer step against one CPU torch.optim step: from the device's pre-step parameters and the flat
    gradient the step's backward wrote (the optimizer leaves it as it is), in the reference's two groups."""
    m = tr.model
    torch.cuda.synchronize()
    before, ema_before = m.flat.detach().cpu().clone(), tr.ema_model.ema.flat.detach().cpu().clone()
    for rg, ng in zip(ref_opt.param_groups, tr.optimizer.param_groups):
        assert rg["weight_decay"] == ng["weight_decay"]
        rg["lr"] = ng["lr"]
    tr.step(batch)
    torch.cuda.synchronize()
    grad = m.flat_grad.detach().cpu().clone()
    with torch.no_grad():
        shadow.flat.copy_(before)
    for name, p in shadow.named_parameters():
        o = shadow.offs[name]
        p.grad = grad[o:o + p.numel()].view(p.shape).clone() if p.requires_grad else None
    ref_opt.step()
    after = m.flat.detach().cpu()
    for name, p in shadow.named_parameters():
        o = shadow.offs[name]
        torch.testing.assert_close(after[o:o + p.numel()], p.detach().flatten(), rtol=RTOL, atol=ATOL,
                                   msg=lambda s, name=name: f"{tag} {name}: {s}")
    _close(f"{tag} flat", after, shadow.flat)
    _close(f"{tag} ema flat", tr.ema_model.ema.flat, D * ema_before + (1.0 - D) * after)
    return before, after


def _fixmatch(opt_func, freeze=False):
    import numpy as np
    import pandas as pd
    from endossl.fixmatch import FixMatch
    from endossl.vit import NativeViT, ViTConfig
    from oracle import ref
    vcfg = ViTConfig(img_size=64, dim=128, depth=2, heads=2, num_classes=23)
    rcfg = ref.Cfg(img_size=64, patch=16, dim=128, depth=2, heads=2, num_classes=23)
    params = ref.random_params(rcfg, seed=3, head_std=0.5)
    m = NativeViT(vcfg, seed=0)
    m.load_state_dict({k: v.clone() for k, v in params.items()})
    shadow = NativeViT(vcfg, seed=0)
    gen = torch.Generator().manual_seed(0)
    B, MU = 2, 2
    lab = [(torch.randn(B, 3, 64, 64, generator=gen), torch.randint(0, 23, (B,), generator=gen)) for _ in range(2)]
    unl = [((torch.randn(B * MU, 3, 64, 64, generator=gen), torch.randn(B * MU, 3, 64, 64, generator=gen)),
            torch.arange(B * MU)) for _ in range(2)]
    df = pd.DataFrame({"target": np.concatenate([np.full(i + 1, i) for i in range(23)])})
    tr = FixMatch(m.to(DEV), opt_func=opt_func, lr=1e-3, device=DEV)
    tr.get_dataloader((_DL(lab, df), _DL(unl)), None)
    tr.get_config(_cfg(0.05, 2, B, MU, freeze=freeze))
    if freeze:
        for p in shadow.parameters():
            p.requires_grad = False
        shadow.fc.requires_grad_(True)
    return tr, shadow, list(zip(lab, unl))


@pytest.mark.parametrize("opt_func", ["AdamW", "SGD"])
def test_fixmatch_trainer_steps_with(opt_func):
    """FixMatch(opt_func=...) on the tiny ViT, two steps, EMA on: model.flat after each step = one CPU
    torch.optim step on the pre-step parameters with the step's own gradient; the EMA model follows the blend."""
    from endossl.optimizer import NativeAdamW, NativeSGD
    tr, shadow, batches = _fixmatch(opt_func)
    assert type(tr.optimizer) is {"AdamW": NativeAdamW, "SGD": NativeSGD}[opt_func]
    ref_opt = _reference_optimizer(shadow, opt_func, lr=1e-3)
    for i, batch in enumerate(batches):
        before, after = _checked_step(tr, shadow, ref_opt, batch, f"{opt_func} step {i}")
        assert not torch.equal(before, after)


def test_fixmatch_frozen_trunk_keeps_its_bits_under_adamw():
    """IS_FREEZE with AdamW: weight decay would shrink every weight it reaches; the class map keeps the sweep
    off the frozen trunk, the head trains."""
    tr, shadow, batches = _fixmatch("AdamW", freeze=True)
    m = tr.model
    initial = m.flat.detach().cpu().clone()
    ref_opt = _reference_optimizer(shadow, "AdamW", lr=1e-3)
    for i, batch in enumerate(batches):
        _checked_step(tr, shadow, ref_opt, batch, f"frozen AdamW step {i}")
    final = m.flat.detach().cpu()
    for name, p in m.named_parameters():
        o = m.offs[name]
        same = torch.equal(final[o:o + p.numel()], initial[o:o + p.numel()])
        assert same != name.startswith("head."), name
    assert float(tr.optimizer.exp_avg[:m.offs["head.weight"]].abs().max()) == 0.0


def test_suplearning_resnet_steps_with_sgd():
    """SupLearning(opt_func="SGD") on a one-block-per-stage NativeResNet: the conv / BatchNorm grouping."""
    from endossl.optimizer import NativeSGD
    from endossl.resnet import NativeResNet, ResNetConfig
    from endossl.supervised import SupLearning
    from endossl.utils import AttrDict
    rc = ResNetConfig(layers=(1, 1, 1, 1), num_classes=23, img_size=64)
    m, shadow = NativeResNet(rc, seed=5), NativeResNet(rc, seed=5)
    gen = torch.Generator().manual_seed(8)
    batch = (torch.randn(8, 3, 64, 64, generator=gen), torch.randint(0, 23, (8,), generator=gen))

    class _DLL(list):
        dataset = _DS(None)

    tr = SupLearning(m.to(DEV), opt_func="SGD", lr=1e-3, device=DEV)
    tr.get_dataloader(_DLL([batch]), None, None)
    tr.get_config(AttrDict(DATA=AttrDict(BATCH_SIZE=8, IMG_SIZE=64, TARGET_NAME="target"),
                           MODEL=AttrDict(NAME="resnet18", NUM_CLASSES=23, MARGIN="None", IS_TRIPLET=False),
                           TRAIN=AttrDict(USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, CLS_WEIGHT=False, EPOCHS=1,
                                          WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8,
                                          SCH_NAME="const", FREQ_EVAL=1)))
    assert type(tr.optimizer) is NativeSGD
    decay, no_decay = tr.optimizer._group_names
    assert "layer1.0.conv1.weight" in decay and "fc.weight" in decay
    assert "layer1.0.bn1.weight" in no_decay and "bn1.bias" in no_decay and "fc.bias" in no_decay
    ref_opt = _reference_optimizer(shadow, "SGD", lr=1e-3)
    before, after = _checked_step(tr, shadow, ref_opt, batch, "ResNet SGD")
    o = m.offs["layer1.0.conv1.weight"]
    assert not torch.equal(before[o:o + 64], after[o:o + 64])
