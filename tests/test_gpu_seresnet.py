"""SE-ResNet-50 (endossl/resnet.py NativeSEResNet, `resnet50se`) on the MI355X against its plain-torch.nn restatement
(tests/seresnet_restatement.py, pinned to the reference's Bottleneck by tests/test_seresnet_cpu.py), the reference's
own block fixtures through NativeSEResNet._bottleneck, and one step of each trainer that takes the model.

Shapes: 2 images of 64^2, 5 classes -- stage maps 16^2, 8^2, 4^2, 2^2, as tests/test_gpu_resnet50.py.  The
comparisons and tolerances are that file's (which cites tests/test_gpu_resnet.py line by line), not new ones:
logits and BatchNorm buffers within 1e-3 of scale (test_gpu_resnet50.py:69,75), a gradient within 2e-3 |g| + 4x the
fp32 restatement's own distance from fp64 + 1e-4 of the largest gradient (:85-89), bf16 logits within twice the
bf16-contract emulation's distance from fp32 + 1e-3 of scale (:111)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.conformer_ref import is_buffer  # noqa: E402
from seresnet_restatement import SEBottleneck, SEResNet50, forward_contract  # noqa: E402

DEV = "cuda"
C = 5
GRAD_KEYS = ("conv1.weight", "layer1.0.downsample.0.weight", "layer4.2.conv3.weight", "fc.weight",
             "layer1.0.conv_down.weight", "layer3.1.conv_up.weight", "layer4.2.conv_down.weight", "layer2.0.bn3.weight",
             "layer4.2.bn3.weight", "layer1.1.bn3.bias")


def _model(seed=2, conv="fp32", buffers_seed=None):
    from endossl import resnet
    m = resnet.NativeSEResNet(resnet.ResNetConfig(num_classes=C, se=True, **resnet.RESNET50), seed=seed)
    sd = m.state_dict()
    g = torch.Generator().manual_seed(100 + seed)
    for k, v in sd.items():  # BatchNorm weights / biases off their 1 / 0 init: no term of the tail's backward vanishes
        if k.endswith("bn3.weight"):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        elif k.endswith("bn3.bias"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.2
        elif buffers_seed is not None and k.endswith("running_mean"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
        elif buffers_seed is not None and k.endswith("running_var"):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
    m.load_state_dict(sd)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).set_conv_precision(conv), state


def _restatement(state, dtype):
    ref = SEResNet50(C).to(dtype)
    ref.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()})
    return ref


@pytest.fixture(scope="module")
def case():
    """The fp32-conv model, its input, and the restatement's train-mode forward + backward in fp32 and fp64."""
    m, state = _model(conv="fp32")
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    g = torch.randn(2, C, generator=torch.Generator().manual_seed(4))
    refs = {}
    for dt in (torch.float32, torch.float64):
        ref = _restatement(state, dt).train()
        out = ref(x.to(dt))
        (out * g.to(dt)).sum().backward()
        refs[dt] = (out.detach(), {k: p.grad for k, p in ref.named_parameters()}, dict(ref.named_buffers()))
    return m, state, x, g, refs


def _grad_bar(named, g32, g64):
    """named: (key, device gradient) pairs; test_gpu_resnet50.py:85-89."""
    gmax = max(v.double().norm().item() for v in g32.values())
    bad = []
    for k, gh in named:
        gh = gh.double()
        nrm = g32[k].double().norm().item()
        e, env = (gh - g64[k]).norm().item(), 4 * (g32[k].double() - g64[k]).norm().item()
        print(f"grad {k}: |device - fp64| = {e:.3e}, 4 |fp32 - fp64| = {env:.3e}, |g| = {nrm:.3e}")
        if e > 2e-3 * nrm + env + 1e-4 * gmax:
            bad.append((k, e, env, nrm))
    assert not bad, bad


def test_seresnet_train_parity_fp32(case):
    m, state, x, g, refs = case
    m.train()
    m.flat_grad.zero_()
    h = m(x.to(DEV))
    r32 = refs[torch.float32][0].double()
    sc = max(1.0, r32.abs().max().item())
    e32 = (h.detach().cpu().double() - r32).abs().max().item()
    print(f"logits: |device - fp32| = {e32:.3e}, scale {sc:.3f}")
    assert e32 <= 1e-3 * sc, (e32, sc)
    bufs = refs[torch.float32][2]
    for k in ("bn1.running_mean", "layer1.0.bn3.running_var", "layer1.0.downsample.1.running_var",
              "layer3.0.bn3.running_mean", "layer4.2.bn3.running_mean", "layer4.2.bn3.running_var",
              "layer4.2.bn2.running_var"):
        ref = bufs[k]
        err = (m.get_buffer(k).cpu() - ref).abs().max().item()
        assert err <= 1e-3 * max(1.0, ref.abs().max().item()), (k, err)
    assert int(m.get_buffer("layer4.2.bn3.num_batches_tracked").item()) == 1
    (h * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    g32, g64 = refs[torch.float32][1], refs[torch.float64][1]
    _grad_bar([(k, m.gview(k).cpu().view(g32[k].shape)) for k in GRAD_KEYS], g32, g64)


def test_seresnet_bf16_logits_within_the_contract_envelope(case):
    _, state, x, _, refs = case
    m, _ = _model(conv="bf16")
    assert m.map_bf16 and m.conv_1x1
    p = {k: v.clone() for k, v in state.items() if not is_buffer(k)}
    bufs = {k: v.clone() for k, v in state.items() if is_buffer(k)}
    with torch.no_grad():
        r16 = forward_contract(p, bufs, x, train=True, bf16=True, maps=m.map_bf16).double()
    r32 = refs[torch.float32][0].double()
    m.train()
    m.flat_grad.zero_()
    out = m(x.to(DEV))
    h = out.detach().cpu().double()
    sc = max(1.0, r32.abs().max().item())
    e32, env = (h - r32).abs().max().item(), (r16 - r32).abs().max().item()
    print(f"bf16 logits: |device - fp32| = {e32:.3e}, |contract - fp32| = {env:.3e}, scale {sc:.3f}")
    assert e32 <= 2 * env + 1e-3 * sc, (e32, env, sc)
    # the statistics came from conv3's epilogue partials; the backward runs and reaches every SE weight
    out.sum().backward()
    torch.cuda.synchronize()
    assert int(m.get_buffer("layer2.1.bn3.num_batches_tracked").item()) == 1
    for k in ("layer1.0.conv_down.weight", "layer4.2.conv_up.weight", "layer3.5.bn3.weight", "conv1.weight"):
        gv = m.gview(k)
        assert bool(torch.isfinite(gv).all()) and gv.abs().max().item() > 0, k


def test_seresnet_fp32_maps_with_bf16_convs(case, monkeypatch):
    """ENDOSSL_MAP_BF16=0's configuration (bf16 conv operands, fp32 maps): the same contract bar."""
    from endossl import resnet
    _, state, x, _, refs = case
    monkeypatch.setattr(resnet, "MAP_BF16", False)
    m, _ = _model(conv="bf16")
    assert not m.map_bf16
    p = {k: v.clone() for k, v in state.items() if not is_buffer(k)}
    bufs = {k: v.clone() for k, v in state.items() if is_buffer(k)}
    with torch.no_grad():
        r16 = forward_contract(p, bufs, x, train=True, bf16=True, maps=False).double()
    r32 = refs[torch.float32][0].double()
    h = m.train()(x.to(DEV)).detach().cpu().double()
    sc = max(1.0, r32.abs().max().item())
    e32, env = (h - r32).abs().max().item(), (r16 - r32).abs().max().item()
    assert e32 <= 2 * env + 1e-3 * sc, (e32, env, sc)


def test_seresnet_eval_uses_running_statistics():
    m, state = _model(seed=7, conv="fp32", buffers_seed=8)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    ref = _restatement(state, torch.float32).eval()
    with torch.no_grad():
        r32 = ref(x).double()
        h = m.eval()(x.to(DEV)).cpu().double()
    sc = max(1.0, r32.abs().max().item())
    assert (h - r32).abs().max().item() <= 1e-3 * sc
    for k, v in m.state_dict().items():  # eval mode leaves the buffers alone, bit for bit
        if is_buffer(k):
            assert torch.equal(v.cpu(), state[k]), k


@pytest.mark.parametrize("tag", ["identity", "downsample"])
def test_reference_block_fixture_through_the_native_bottleneck(golden, tag):
    """The reference's own Bottleneck (tests/golden/se_block_*.npz) against NativeSEResNet._bottleneck on a model of
    matching widths (planes 32: layer1.0 = 64 -> 128 with a downsample, layer1.1 = 128 -> 128 without), fp32 convs."""
    from endossl import resnet
    from endossl.conformer import _join_queued
    d = golden(f"se_block_{tag}.npz")
    inp, planes, stride = int(d["inplanes"]), int(d["planes"]), int(d["stride"])
    pre = "layer1.1." if tag == "identity" else "layer1.0."
    m = resnet.NativeSEResNet(resnet.ResNetConfig(layers=(2,), widths=(planes,), block="bottleneck", se=True,
                                                  num_classes=C), seed=0)
    sd = m.state_dict()
    init = {k[5:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("init/")}
    assert [k[len(pre):] for k in sd if k.startswith(pre)] == list(init)
    for k, v in init.items():
        sd[pre + k] = v
    m.load_state_dict(sd)
    m = m.to(DEV).set_conv_precision("fp32").train()
    m.flat_grad.zero_()
    _join_queued.clear()
    m._bn_partials.clear()
    x = torch.from_numpy(d["x"]).permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    out = m._bottleneck(x, pre, inp, planes, stride, tag == "downsample")
    g = torch.from_numpy(d["g"]).permute(0, 2, 3, 1).contiguous().to(DEV)
    (out * g).sum().backward()
    torch.cuda.synchronize()
    o32 = torch.from_numpy(d["out_f32"]).double()
    sc = max(1.0, o32.abs().max().item())
    e = (out.detach().permute(0, 3, 1, 2).cpu().double() - o32).abs().max().item()
    print(f"{tag}: |device - fp32| = {e:.3e}, scale {sc:.3f}")
    assert e <= 1e-3 * sc, (e, sc)
    for k in d.files:
        if k.startswith("buf_f32/") and not k.endswith("num_batches_tracked"):
            ref = torch.from_numpy(d[k])
            err = (m.get_buffer(pre + k[8:]).cpu() - ref).abs().max().item()
            assert err <= 1e-3 * max(1.0, ref.abs().max().item()), (k, err)
    assert int(m.get_buffer(pre + "bn3.num_batches_tracked").item()) == 1
    g32 = {k[9:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("grad_f32/")}
    g64 = {k[5:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("grad/")}
    g32["x"], g64["x"] = torch.from_numpy(d["dx_f32"]), torch.from_numpy(d["dx"])
    named = [(k, m.gview(pre + k).cpu().view(g32[k].shape)) for k in g32 if k != "x"]
    named.append(("x", x.grad.permute(0, 3, 1, 2).cpu()))
    assert {"conv_down.weight", "conv_up.weight", "bn3.weight", "bn3.bias"} <= set(g32)
    _grad_bar(named, g32, g64)


def test_train_forward_on_several_ranks_raises(case, monkeypatch):
    """The tail refuses a train-mode forward at world size 2 before any launch (it takes one rank's statistics);
    eval mode does not ask."""
    from endossl import dist, resnet
    m = case[0]
    y = torch.zeros(1, 2, 2, 256, device=DEV)
    monkeypatch.setattr(dist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="one rank"):
        resnet._SETailFn.apply(y, y, m.train(), "layer1.0.", resnet.BN_EPS, None)
    with torch.no_grad():
        out = resnet._SETailFn.apply(y, y, m.eval(), "layer1.0.", resnet.BN_EPS, None)
    assert tuple(out.shape) == (1, 2, 2, 256) and bool(torch.isfinite(out).all())
    m.train()


class _DS:
    df = None


class _DL(list):
    dataset = _DS()


def _cfg():
    from endossl.utils import AttrDict
    return AttrDict(DATA=AttrDict(BATCH_SIZE=2, MU=1, IMG_SIZE=64, TARGET_NAME="target"),
                    MODEL=AttrDict(NAME="resnet50se", NUM_CLASSES=C, MARGIN="None", IS_TRIPLET=False,
                                   TYPE_SEMI="FixMatch", PRE_TRAIN_PATH="None"),
                    TRAIN=AttrDict(IS_SSL=True, IS_FREEZE=False, USE_EMA=True, EMA_DECAY=0.999,
                                   BASE_LR=1e-3, EVAL_STEP=1, CLS_WEIGHT=False, THRES=0.0, T=1.0, LAMBDA_U=1.0,
                                   LAMBDA_C=1.0, EPOCHS=1, WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8,
                                   SCH_NAME="const", FREQ_EVAL=1))


def _snapshot(m, tr):
    return ({k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
            {k: v.detach().cpu().clone() for k, v in tr.ema_model.ema.state_dict().items()})


def _assert_updated(before, after, what):
    changed = [k for k in before if not torch.equal(before[k], after[k])]
    for k in ("conv1.weight", "layer1.0.conv1.weight", "layer2.0.downsample.0.weight", "layer4.2.conv3.weight",
              "layer4.2.bn3.weight", "fc.weight", "layer3.5.bn2.running_mean", "layer4.0.downsample.1.running_var",
              "layer1.0.conv_down.weight", "layer1.0.conv_up.weight", "layer4.2.conv_down.weight",
              "layer4.2.conv_up.weight", "layer2.3.bn3.running_mean", "layer2.3.bn3.running_var"):
        assert k in changed, (what, k)
    assert all(bool(torch.isfinite(v).all()) for v in after.values() if v.is_floating_point()), what


def test_fixmatch_step():
    from endossl.build import build_model
    from endossl.fixmatch import FixMatch
    m = build_model(_cfg(), seed=4)
    assert type(m).__name__ == "NativeSEResNet"
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(2, 3, 64, 64, generator=g), torch.randint(0, C, (2,), generator=g)
    uw, us = torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 3, 64, 64, generator=g)
    tr = FixMatch(m, device=DEV)
    assert tr.cnn and tr.EMA_BUFFERS
    tr.get_dataloader((None, None), None)
    tr.get_config(_cfg())
    before = _snapshot(m, tr)
    out = tr.step(((x, y), ((uw, us), None)))
    torch.cuda.synchronize()
    for k in ("loss", "lx", "lu", "mask_mean"):
        assert bool(torch.isfinite(out[k])), k
    assert out["mask_mean"].item() == 1.0 and out["lu"].item() > 0  # THRES 0: every weak row is a pseudo-label
    assert int(m.get_buffer("layer1.0.bn3.num_batches_tracked").item()) == 1  # ONE forward over the six rows
    after = _snapshot(m, tr)
    _assert_updated(before[0], after[0], "model")
    _assert_updated(before[1], after[1], "ema")


def test_suplearning_step_runs_eagerly():
    from endossl.build import build_model
    from endossl.supervised import SupLearning
    g = torch.Generator().manual_seed(12)
    batches = [(torch.randn(2, 3, 64, 64, generator=g), torch.randint(0, C, (2,), generator=g)) for _ in range(2)]
    cfg = _cfg()
    cfg.TRAIN.IS_SSL = False
    m = build_model(cfg, seed=5)
    tr = SupLearning(m, opt_func="Adam", lr=1e-3, device=DEV)
    tr.get_dataloader(_DL(batches), None, None)
    tr.get_config(cfg)
    m = tr.model
    before = _snapshot(m, tr)
    x, y = batches[0]
    loss = tr.step((x.to(DEV), y.to(DEV)))["loss"]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    after = _snapshot(m, tr)
    _assert_updated(before[0], after[0], "model")
    _assert_updated(before[1], after[1], "ema")
    assert not [e for e in getattr(tr, "_graphs", {}).values() if e["graph"] is not None]  # no graph replay
