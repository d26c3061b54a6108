"""ResNet-50 (endossl/resnet.py, bottleneck config) on the MI355X against its plain-torch.nn restatement
(tests/resnet50_restatement.py; timm is absent), and one step of each trainer that takes it.

Shapes: 2 images of 64^2, 5 classes -- the last map is 2 x 2 x 2048 (M = 8 rows for layer4's 1 x 1 convs), every
stage runs its first block with a downsample and the rest without.  The comparisons and tolerances are the
ResNet-18 parity test's (tests/test_gpu_resnet.py::test_resnet18_forward_backward_vs_oracle, cited line by line
below), not new ones."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.conformer_ref import is_buffer  # noqa: E402
from resnet50_restatement import ResNet50, forward_contract  # noqa: E402

DEV = "cuda"
C = 5


def _model(seed=2, conv="fp32", cls="NativeResNet", buffers_seed=None):
    from endossl import resnet
    cfg = resnet.ResNetConfig(num_classes=C, fc_bias=cls == "NativeResNet", **resnet.RESNET50)
    m = getattr(resnet, cls)(cfg, seed=seed)
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


def _restatement(state, dtype):
    ref = ResNet50(C).to(dtype)
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


def test_resnet50_train_parity_fp32(case):
    m, state, x, g, refs = case
    m.train()
    m.flat_grad.zero_()
    h = m(x.to(DEV))
    r32 = refs[torch.float32][0].double()
    sc = max(1.0, r32.abs().max().item())
    e32 = (h.detach().cpu().double() - r32).abs().max().item()
    print(f"logits: |device - fp32| = {e32:.3e}, scale {sc:.3f}")
    assert e32 <= 1e-3 * sc, (e32, sc)  # test_gpu_resnet.py:53
    bufs = refs[torch.float32][2]
    for k in ("bn1.running_mean", "layer1.0.downsample.1.running_var", "layer3.0.downsample.1.running_var",
              "layer4.2.bn3.running_mean", "layer4.2.bn2.running_var"):
        ref = bufs[k]
        err = (m.get_buffer(k).cpu() - ref).abs().max().item()
        assert err <= 1e-3 * max(1.0, ref.abs().max().item()), (k, err)  # test_gpu_resnet.py:56-57
    assert int(m.get_buffer("layer4.2.bn3.num_batches_tracked").item()) == 1
    (h * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    g32, g64 = refs[torch.float32][1], refs[torch.float64][1]
    gmax = max(v.double().norm().item() for v in g32.values())
    bad = []
    for k in ("conv1.weight", "layer1.0.downsample.0.weight", "layer4.2.conv3.weight", "fc.weight"):
        gh = m.gview(k).cpu().view(g32[k].shape).double()
        nrm = g32[k].double().norm().item()
        # test_gpu_resnet.py:74-79: the device against fp64, within 2e-3 |g| + 4x the fp32 restatement's own
        # distance from fp64 + 1e-4 of the largest gradient
        e, env = (gh - g64[k]).norm().item(), 4 * (g32[k].double() - g64[k]).norm().item()
        print(f"grad {k}: |device - fp64| = {e:.3e}, 4 |fp32 - fp64| = {env:.3e}, |g| = {nrm:.3e}")
        if e > 2e-3 * nrm + env + 1e-4 * gmax:
            bad.append((k, e, env, nrm))
    assert not bad, bad


def test_resnet50_bf16_logits_within_the_contract_envelope(case):
    """The default bf16 convs and maps (and the direct 1 x 1 kernels): the device within twice the bf16-contract
    emulation's own distance from fp32 (+ 1e-3 of scale) -- test_gpu_resnet.py:49-51, the criterion of
    test_gpu_conformer.py."""
    _, state, x, _, refs = case
    m, _ = _model(conv="bf16")
    assert m.map_bf16 and m.conv_1x1
    p = {k: v.clone() for k, v in state.items() if not is_buffer(k)}
    bufs = {k: v.clone() for k, v in state.items() if is_buffer(k)}
    with torch.no_grad():
        r16 = forward_contract(p, bufs, x, train=True, bf16=True, maps=m.map_bf16).double()
    r32 = refs[torch.float32][0].double()
    m.train()
    h = m(x.to(DEV)).detach().cpu().double()
    sc = max(1.0, r32.abs().max().item())
    e32, env = (h - r32).abs().max().item(), (r16 - r32).abs().max().item()
    print(f"bf16 logits: |device - fp32| = {e32:.3e}, |contract - fp32| = {env:.3e}, scale {sc:.3f}")
    assert e32 <= 2 * env + 1e-3 * sc, (e32, env, sc)


def test_direct_1x1_dispatch_is_bit_identical(case):
    """The bottleneck model under es_set_conv_1x1 0 (implicit kernels only), 1 (the default shape class) and 2 (every
    stride-1 1 x 1 conv direct): logits, every gradient (the accumulating data gradients into the blocks' shared
    sinks among them) and the BatchNorm buffers bit-identical -- and ResNet-18 never asks for the direct kernels."""
    from endossl import _lib
    from endossl.resnet import NativeResNet, ResNetConfig
    from endossl import conformer
    _, _, x, g, _ = case
    lib = _lib.load()
    runs, counts = [], []
    real_call = conformer.call

    def counting_call(name, *args):
        if name.startswith("es_conv1x1_"):
            counts[-1][name] = counts[-1].get(name, 0) + 1
        return real_call(name, *args)
    conformer.call = counting_call
    try:
        for mode in (0, 1, 2):
            assert lib.es_set_conv_1x1(mode) in (0, 1, 2)
            counts.append({})
            m, _ = _model(conv="bf16")
            m.train()
            m.flat_grad.zero_()
            h = m(x.to(DEV))
            (h * g.to(DEV)).sum().backward()
            torch.cuda.synchronize()
            runs.append((h.detach().cpu(), m.flat_grad.cpu().clone(),
                         {k: v.cpu().clone() for k, v in m.state_dict().items() if is_buffer(k)}))
    finally:
        conformer.call = real_call
        lib.es_set_conv_1x1(1)
    # resnet50's stride-1 1 x 1 convs: 16 conv1 + layer1.0.downsample.0 through conv(), 16 conv3 through bn_conv();
    # every one has a data gradient (the stem's max-pooled map takes one too)
    assert counts[0] == {}
    assert counts[2] == {"es_conv1x1_fwd_bf16_ex": 17, "es_conv1x1_fwd_bf16_bnin_ex": 16,
                         "es_conv1x1_bwd_data_bf16_ex": 33}
    # the default class, a reduction >= 512 deep: conv1 of layer2.1-3, layer3.0-5, layer4.0-2 (Cin 512 / 1024 /
    # 2048); conv3 of layer4 (Cin 512); data gradients of those conv3 (Cout 512 .. 2048: layer2-4, 13) and of
    # layer4's conv1 (Cout 512: 3)
    assert counts[1] == {"es_conv1x1_fwd_bf16_ex": 12, "es_conv1x1_fwd_bf16_bnin_ex": 3,
                         "es_conv1x1_bwd_data_bf16_ex": 16}
    assert bool(torch.isfinite(runs[0][1]).all()) and runs[0][1].abs().max().item() > 0
    for h, fg, bufs in runs[1:]:
        assert torch.equal(h, runs[0][0]) and torch.equal(fg, runs[0][1])
        for k, v in bufs.items():
            assert torch.equal(v, runs[0][2][k]), k
    assert not NativeResNet(ResNetConfig(num_classes=C), seed=0).conv_1x1


def test_resnet50_eval_uses_running_statistics():
    m, state = _model(seed=7, conv="fp32", buffers_seed=8)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    ref = _restatement(state, torch.float32).eval()
    with torch.no_grad():
        r32 = ref(x).double()
        h = m.eval()(x.to(DEV)).cpu().double()
    sc = max(1.0, r32.abs().max().item())
    assert (h - r32).abs().max().item() <= 1e-3 * sc  # the fp32 logits bar, test_gpu_resnet.py:53
    for k, v in m.state_dict().items():  # eval mode leaves the buffers alone
        if is_buffer(k):
            assert torch.equal(v.cpu(), state[k]), k


class _DS:
    df = None


class _DL(list):
    dataset = _DS()


def _cfg(margin="None"):
    from endossl.utils import AttrDict
    return AttrDict(DATA=AttrDict(BATCH_SIZE=2, MU=1, IMG_SIZE=64, TARGET_NAME="target"),
                    MODEL=AttrDict(NAME="resnet50", NUM_CLASSES=C, MARGIN=margin, IS_TRIPLET=False,
                                   TYPE_SEMI="FixMatch", PRE_TRAIN_PATH="None"),
                    TRAIN=AttrDict(IS_SSL=margin == "None", IS_FREEZE=False, USE_EMA=True, EMA_DECAY=0.999,
                                   BASE_LR=1e-3, EVAL_STEP=1, CLS_WEIGHT=False, THRES=0.0, T=1.0, LAMBDA_U=1.0,
                                   LAMBDA_C=1.0, EPOCHS=1, WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8,
                                   SCH_NAME="const", FREQ_EVAL=1))


def _snapshot(m, tr):
    return ({k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
            {k: v.detach().cpu().clone() for k, v in tr.ema_model.ema.state_dict().items()})


def _assert_updated(before, after, what):
    changed = [k for k in before if not torch.equal(before[k], after[k])]
    for k in ("conv1.weight", "layer1.0.conv1.weight", "layer2.0.downsample.0.weight", "layer4.2.conv3.weight",
              "layer4.2.bn3.weight", "fc.weight", "layer3.5.bn2.running_mean", "layer4.0.downsample.1.running_var"):
        assert k in changed, (what, k)
    assert all(bool(torch.isfinite(v).all()) for v in after.values() if v.is_floating_point()), what


def test_fixmatch_step():
    """A reference config with NAME 'resnet50', TYPE_SEMI 'FixMatch' builds and takes a step: one train-mode forward
    over cat(x, u_w, u_s), finite losses, parameters / BatchNorm buffers and their EMA updated."""
    from endossl.build import build_model
    from endossl.fixmatch import FixMatch
    m = build_model(_cfg(), seed=4)
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
    assert abs(out["loss"].item() - (out["lx"].item() + out["lu"].item())) <= 1e-5 * max(1.0, out["loss"].item())
    assert int(m.get_buffer("bn1.num_batches_tracked").item()) == 1  # ONE forward over the six rows
    after = _snapshot(m, tr)
    _assert_updated(before[0], after[0], "model")
    _assert_updated(before[1], after[1], "ema")


def test_suplearning_steps_and_graph_replay():
    """SupLearning.step: parameters and EMA move; the step after GRAPH_WARM eager ones is captured and the next
    one replays the graph -- each with the loss (and the state) of an all-eager trainer on a copy of the model."""
    from endossl.build import build_model
    from endossl.supervised import SupLearning
    g = torch.Generator().manual_seed(12)
    batches = [(torch.randn(2, 3, 64, 64, generator=g), torch.randint(0, C, (2,), generator=g)) for _ in range(4)]
    base = build_model(_cfg(), seed=5)
    assert type(base).__name__ == "NativeResNet"
    runs = {}
    for graph in (True, False):
        m = copy.deepcopy(base)
        tr = SupLearning(m, opt_func="Adam", lr=1e-3, device=DEV)
        tr.use_graph = graph
        tr.get_dataloader(_DL(batches), None, None)
        cfg = _cfg()
        cfg.TRAIN.IS_SSL = False
        tr.get_config(cfg)
        m = tr.model
        before = _snapshot(m, tr)
        losses = []
        for i, (x, y) in enumerate(batches):
            losses.append(tr.step((x.to(DEV), y.to(DEV)))["loss"])
            if i == 0:
                torch.cuda.synchronize()
                after = _snapshot(m, tr)
                _assert_updated(before[0], after[0], "model")
                _assert_updated(before[1], after[1], "ema")
        torch.cuda.synchronize()
        graphs = [e for e in getattr(tr, "_graphs", {}).values() if e["graph"] is not None]
        assert len(graphs) == (1 if graph else 0)
        assert SupLearning.GRAPH_WARM == 2  # steps 0, 1 eager; 2 captures and replays; 3 replays
        runs[graph] = ([v.item() for v in losses], _snapshot(m, tr)[0])
    (lg, sg), (le, se) = runs[True], runs[False]
    assert all(map(lambda v: v == v and abs(v) < 1e4, le))
    assert lg == le, (lg, le)
    for k in se:
        assert torch.equal(sg[k], se[k]), k


def test_margin_step_resnet50():
    from endossl.build import build_model
    from endossl.supervised import SupLearning
    m = build_model(_cfg("cosface"), seed=6)
    assert type(m).__name__ == "ModelMargin"
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(2, 3, 64, 64, generator=g), torch.randint(0, C, (2,), generator=g)
    tr = SupLearning(m, opt_func="Adam", lr=1e-3, device=DEV)
    tr.get_dataloader(_DL([(x, y)]), None, None)
    tr.get_config(_cfg("cosface"))
    assert tr.is_margin
    m = tr.model
    w0 = m.fc.weight.detach().cpu().clone()
    out = tr.step((x, y))
    torch.cuda.synchronize()
    assert tuple(out["fts"].shape) == (2, 2048) and bool(torch.isfinite(out["loss"]))
    gw = m.gview("fc.weight").cpu().view(C, 2048)
    assert bool(torch.isfinite(gw).all()) and gw.abs().max().item() > 0
    assert m.gview("layer1.0.conv1.weight").abs().max().item() > 0  # and the trunk, through backbone(x)
    assert not torch.equal(m.fc.weight.detach().cpu(), w0)
    with torch.no_grad():
        assert tuple(m.eval()(x.to(DEV)).shape) == (2, C)
