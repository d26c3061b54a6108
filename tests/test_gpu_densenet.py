"""DenseNet (endossl/densenet.py) on the MI355X against its plain-torch.nn restatement (tests/densenet_restatement.py;
timm and torchvision are absent), and one step of each trainer that takes it.

Two configs: a tiny one -- growth 48, bn_size 4, 96 stem features, blocks (6, 2), 5 classes, 3 images of 64^2: block 2
has 192 rows and the prefixes 192 / 240, one of each padding class -- and the full densenet161 at 2 images of 64^2
(8 rows in block 4).  The comparisons and tolerances are tests/test_gpu_resnet50.py's (cited line by line below),
not new ones."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from densenet_restatement import DenseNet, forward_contract  # noqa: E402
from oracle.conformer_ref import is_buffer  # noqa: E402

DEV = "cuda"
C = 5
TINY = dict(block_config=(6, 2), growth=48, bn_size=4, init_features=96)


def _config(which):
    from endossl.densenet import DENSENET161, DenseNetConfig
    return DenseNetConfig(num_classes=C, **(TINY if which == "tiny" else DENSENET161))


def _model(which, seed=2, conv="fp32", buffers_seed=None):
    from endossl.densenet import NativeDenseNet
    m = NativeDenseNet(_config(which), seed=seed)
    if buffers_seed is not None:  # non-trivial running statistics (the eval-mode test)
        g = torch.Generator().manual_seed(buffers_seed)
        sd = m.state_dict()
        for k, v in sd.items():
            if k.endswith("running_mean"):
                sd[k] = torch.randn(v.shape, generator=g) * 0.1
            elif k.endswith("running_var"):
                sd[k] = torch.rand(v.shape, generator=g) + 0.5
        m.load_state_dict(sd)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).set_conv_precision(conv), state


def _restatement(which, state, dtype):
    ref = DenseNet(_config(which)).to(dtype)
    ref.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()})
    return ref


def _last(which):
    cfg = _config(which)
    return len(cfg.block_config), cfg.block_config[-1]


_CASES = {}


@pytest.fixture(params=["tiny", "full"])
def case(request):
    """The fp32-conv model, its input, and the restatement's train-mode forward + backward in fp32 and fp64 (computed
    once per config and shared, unchanged, by the tests below)."""
    which = request.param
    if which not in _CASES:
        m, state = _model(which, conv="fp32")
        n = 3 if which == "tiny" else 2
        x = torch.randn(n, 3, 64, 64, generator=torch.Generator().manual_seed(3))
        g = torch.randn(n, C, generator=torch.Generator().manual_seed(4))
        refs = {}
        for dt in (torch.float32, torch.float64):
            ref = _restatement(which, state, dt).train()
            out = ref(x.to(dt))
            (out * g.to(dt)).sum().backward()
            refs[dt] = (out.detach(), {k: p.grad for k, p in ref.named_parameters()}, dict(ref.named_buffers()))
        _CASES[which] = (which, m, state, x, g, refs)
    return _CASES[which]


def test_densenet_train_parity_fp32(case):
    which, m, state, x, g, refs = case
    m.load_state_dict(state)  # the buffers as the restatement started from them
    m.train()
    m.flat_grad.zero_()
    h = m(x.to(DEV))
    r32 = refs[torch.float32][0].double()
    sc = max(1.0, r32.abs().max().item())
    e32 = (h.detach().cpu().double() - r32).abs().max().item()
    print(f"{which} logits: |device - fp32| = {e32:.3e}, scale {sc:.3f}")
    assert e32 <= 1e-3 * sc, (e32, sc)  # test_gpu_resnet50.py:69
    bufs = refs[torch.float32][2]
    nb, nl = _last(which)
    for k in ("features.norm0.running_mean", "features.denseblock1.denselayer1.norm1.running_var",
              "features.denseblock1.denselayer2.norm1.running_mean", "features.denseblock1.denselayer4.norm2.running_var",
              f"features.denseblock{nb}.denselayer{nl}.norm1.running_mean",
              f"features.denseblock{nb}.denselayer{nl}.norm1.running_var", "features.transition1.norm.running_var",
              "features.norm5.running_mean", "features.norm5.running_var"):
        ref = bufs[k]
        err = (m.get_buffer(k).cpu() - ref).abs().max().item()
        assert err <= 1e-3 * max(1.0, ref.abs().max().item()), (k, err)  # test_gpu_resnet50.py:74-75
    for k in ("features.norm0.", "features.denseblock1.denselayer1.norm1.", f"features.denseblock{nb}.denselayer{nl}.norm2.",
              "features.transition1.norm.", "features.norm5."):
        assert int(m.get_buffer(k + "num_batches_tracked").item()) == 1, k
    (h * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    g32, g64 = refs[torch.float32][1], refs[torch.float64][1]
    gmax = max(v.double().norm().item() for v in g32.values())
    bad = []
    for k in ("features.conv0.weight", "features.denseblock1.denselayer1.conv1.weight",
              "features.denseblock1.denselayer1.norm1.weight", f"features.denseblock{nb}.denselayer{nl}.conv2.weight",
              "features.transition1.conv.weight", "features.norm5.bias", "classifier.weight"):
        gh = m.gview(k).cpu().view(g32[k].shape).double()
        nrm = g32[k].double().norm().item()
        # test_gpu_resnet50.py:85-89: the device against fp64, within 2e-3 |g| + 4x the fp32 restatement's own
        # distance from fp64 + 1e-4 of the largest gradient
        e, env = (gh - g64[k]).norm().item(), 4 * (g32[k].double() - g64[k]).norm().item()
        print(f"{which} grad {k}: |device - fp64| = {e:.3e}, 4 |fp32 - fp64| = {env:.3e}, |g| = {nrm:.3e}")
        if e > 2e-3 * nrm + env + 1e-4 * gmax:
            bad.append((k, e, env, nrm))
    assert not bad, bad


def test_densenet_bf16_logits_within_the_contract_envelope_and_repeat(case):
    """The default bf16 convs and maps (padded operands, shared statistics): the device within twice the bf16-contract
    emulation's own distance from fp32 (+ 1e-3 of scale) -- test_gpu_resnet50.py:104-111 -- and a second run of the
    same step bit-identical (logits and the whole flat gradient: fixed reduction orders, no atomics)."""
    which, _, state, x, g, refs = case
    m, _ = _model(which, conv="bf16")
    assert m.map_bf16
    p = {k: v.clone() for k, v in state.items() if not is_buffer(k)}
    bufs = {k: v.clone() for k, v in state.items() if is_buffer(k)}
    with torch.no_grad():
        r16 = forward_contract(p, bufs, x, train=True, bf16=True, maps=m.map_bf16, cfg=m.cfg).double()
    r32 = refs[torch.float32][0].double()
    m.train()
    runs = []
    for _ in range(2):
        m.flat_grad.zero_()
        h = m(x.to(DEV))
        (h * g.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        runs.append((h.detach().cpu(), m.flat_grad.cpu().clone()))
    h = runs[0][0].double()
    sc = max(1.0, r32.abs().max().item())
    e32, env = (h - r32).abs().max().item(), (r16 - r32).abs().max().item()
    print(f"{which} bf16 logits: |device - fp32| = {e32:.3e}, |contract - fp32| = {env:.3e}, scale {sc:.3f}")
    assert e32 <= 2 * env + 1e-3 * sc, (e32, env, sc)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    fg = runs[0][1]
    assert bool(torch.isfinite(fg).all()) and fg.abs().max().item() > 0
    # nothing padded reaches the flat buffers: the alignment padding behind every padded norm1 is still zero
    for pre, c, cp in m.padded_norms():
        for nm in (pre + "weight", pre + "bias"):
            o = m.offs[nm]
            assert torch.all(fg[o + c:o + cp] == 0) and torch.all(m.flat[o + c:o + cp] == 0), nm


@pytest.mark.parametrize("conv", ["fp32", "bf16"])
def test_densenet_eval_uses_running_statistics(conv):
    m, state = _model("tiny", seed=7, conv=conv, buffers_seed=8)
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    ref = _restatement("tiny", state, torch.float32).eval()
    with torch.no_grad():
        r32 = ref(x).double()
        h = m.eval()(x.to(DEV)).cpu().double()
    sc = max(1.0, r32.abs().max().item())
    if conv == "fp32":
        assert (h - r32).abs().max().item() <= 1e-3 * sc  # the fp32 logits bar, test_gpu_resnet50.py:172
    else:  # the bf16 envelope of the train-mode test, in eval mode
        p = {k: v.clone() for k, v in state.items() if not is_buffer(k)}
        bufs = {k: v.clone() for k, v in state.items() if is_buffer(k)}
        with torch.no_grad():
            r16 = forward_contract(p, bufs, x, train=False, bf16=True, maps=m.map_bf16, cfg=m.cfg).double()
        assert (h - r32).abs().max().item() <= 2 * (r16 - r32).abs().max().item() + 1e-3 * sc
    for k, v in m.state_dict().items():  # eval mode leaves the buffers alone
        if is_buffer(k):
            assert torch.equal(v.cpu(), state[k]), k


def test_train_mode_on_several_ranks_is_refused(monkeypatch):
    from endossl import dist
    m, _ = _model("tiny", conv="bf16")
    monkeypatch.setattr(dist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="SyncBatchNorm"):
        m.train()(torch.zeros(2, 3, 64, 64, device=DEV))


class _DS:
    df = None


class _DL(list):
    dataset = _DS()


def _cfg(ssl=True, freeze=False):
    from endossl.utils import AttrDict
    return AttrDict(DATA=AttrDict(BATCH_SIZE=2, MU=1, IMG_SIZE=64, TARGET_NAME="target"),
                    MODEL=AttrDict(NAME="densenet161", NUM_CLASSES=C, MARGIN="None", IS_TRIPLET=False,
                                   TYPE_SEMI="FixMatch", PRE_TRAIN_PATH="None"),
                    TRAIN=AttrDict(IS_SSL=ssl, IS_FREEZE=freeze, USE_EMA=True, EMA_DECAY=0.999,
                                   BASE_LR=1e-3, EVAL_STEP=1, CLS_WEIGHT=False, THRES=0.0, T=1.0, LAMBDA_U=1.0,
                                   LAMBDA_C=1.0, EPOCHS=1, WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8,
                                   SCH_NAME="const", FREQ_EVAL=1))


def _snapshot(m, tr):
    return ({k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
            {k: v.detach().cpu().clone() for k, v in tr.ema_model.ema.state_dict().items()})


MOVED = ("features.conv0.weight", "features.denseblock1.denselayer1.conv1.weight",
         "features.denseblock1.denselayer2.norm1.weight", "features.denseblock1.denselayer6.conv2.weight",
         "features.denseblock4.denselayer1.norm1.bias", "features.denseblock4.denselayer24.conv2.weight",
         "features.transition2.conv.weight", "features.transition3.norm.weight", "features.norm5.weight",
         "classifier.weight", "classifier.bias", "features.denseblock1.denselayer3.norm1.running_mean",
         "features.denseblock4.denselayer24.norm2.running_var", "features.denseblock4.denselayer24.norm1.running_var",
         "features.transition3.norm.running_var", "features.norm5.running_mean")


def _assert_updated(before, after, what):
    changed = [k for k in before if not torch.equal(before[k], after[k])]
    for k in MOVED:
        assert k in changed, (what, k)
    assert all(bool(torch.isfinite(v).all()) for v in after.values() if v.is_floating_point()), what


def test_fixmatch_step():
    """A reference config with NAME 'densenet161', TYPE_SEMI 'FixMatch' builds and takes a step: one train-mode forward
    over cat(x, u_w, u_s), finite losses, parameters / BatchNorm buffers and their EMA updated."""
    from endossl.build import build_model
    from endossl.fixmatch import FixMatch
    m = build_model(_cfg(), seed=4)
    assert type(m).__name__ == "NativeDenseNet"
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(2, 3, 64, 64, generator=g), torch.randint(0, C, (2,), generator=g)
    uw, us = torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 3, 64, 64, generator=g)
    tr = FixMatch(m, device=DEV)
    assert tr.cnn and tr.EMA_BUFFERS
    tr.get_dataloader((None, None), None)
    tr.get_config(_cfg())
    m = tr.model
    before = _snapshot(m, tr)
    out = tr.step(((x, y), ((uw, us), None)))
    torch.cuda.synchronize()
    for k in ("loss", "lx", "lu", "mask_mean"):
        assert bool(torch.isfinite(out[k])), k
    assert out["mask_mean"].item() == 1.0 and out["lu"].item() > 0  # THRES 0: every weak row is a pseudo-label
    assert abs(out["loss"].item() - (out["lx"].item() + out["lu"].item())) <= 1e-5 * max(1.0, out["loss"].item())
    assert int(m.get_buffer("features.norm0.num_batches_tracked").item()) == 1  # ONE forward over the six rows
    assert int(m.get_buffer("features.denseblock3.denselayer36.norm1.num_batches_tracked").item()) == 1
    after = _snapshot(m, tr)
    _assert_updated(before[0], after[0], "model")
    _assert_updated(before[1], after[1], "ema")
    for pre, c, cp in m.padded_norms():  # the optimizer leaves the padding the padded convs read at zero
        o = m.offs[pre + "weight"]
        assert torch.all(m.flat[o + c:o + cp] == 0), pre


def test_suplearning_step_runs_eagerly():
    from endossl.build import build_model
    from endossl.supervised import SupLearning
    g = torch.Generator().manual_seed(12)
    batches = [(torch.randn(2, 3, 64, 64, generator=g), torch.randint(0, C, (2,), generator=g)) for _ in range(2)]
    m = build_model(_cfg(ssl=False), seed=5)
    tr = SupLearning(m, opt_func="Adam", lr=1e-3, device=DEV)
    tr.get_dataloader(_DL(batches), None, None)
    tr.get_config(_cfg(ssl=False))
    m = tr.model
    before = _snapshot(m, tr)
    losses = [tr.step((x.to(DEV), y.to(DEV)))["loss"] for x, y in batches]
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in losses)
    after = _snapshot(m, tr)
    _assert_updated(before[0], after[0], "model")
    _assert_updated(before[1], after[1], "ema")
    assert not [e for e in getattr(tr, "_graphs", {}).values() if e["graph"] is not None]  # no graph replay
    assert int(m.get_buffer("features.norm5.num_batches_tracked").item()) == 2


def test_is_freeze_trains_the_classifier_alone():
    """IS_FREEZE (code/fixmatch.py:45-48: `model.classifier` for densenet161): through the `fc` alias the trainer
    keeps the classifier trainable; the trunk stays off the tape -- its gradient is exactly zero and no trunk
    parameter moves, while the train-mode forward still updates the BatchNorm buffers."""
    from endossl.build import build_model
    from endossl.fixmatch import FixMatch
    m = build_model(_cfg(freeze=True), seed=6)
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(2, 3, 64, 64, generator=g), torch.randint(0, C, (2,), generator=g)
    uw, us = torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 3, 64, 64, generator=g)
    tr = FixMatch(m, device=DEV)
    tr.get_dataloader((None, None), None)
    tr.get_config(_cfg(freeze=True))
    m = tr.model
    assert m.frozen_trunk
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["classifier.weight", "classifier.bias"]
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    out = tr.step(((x, y), ((uw, us), None)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["loss"]))
    after = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    moved = [k for k in before if not is_buffer(k) and not torch.equal(before[k], after[k])]
    assert moved == ["classifier.weight", "classifier.bias"], moved
    o = m.offs["classifier.weight"]
    assert torch.all(m.flat_grad[:o] == 0) and m.flat_grad[o:].abs().max().item() > 0
    assert not torch.equal(before["features.norm5.running_mean"], after["features.norm5.running_mean"])
