"""SE-ResNet-50 (`resnet50se`) host side (no GPU): the reference's state_dict (a fixture its own SEResNet wrote), the
factory branch and its refusals, round trips, the plain-torch.nn restatement pinned to the reference's Bottleneck by
the block fixtures, and every refusal of the csrc/se.hip entry points before a launch."""
import copy
import json
import os

import pytest
import torch

from conftest import GOLDEN
from seresnet_restatement import SEBottleneck, SEResNet50

C = 23
PARAMS = 26_070_103  # resnet50's 23,555,159 + sum over the 16 blocks of 2 * (4 planes) * (planes / 4) = 2,514,944


def _cfg(**model):
    from endossl.utils import AttrDict
    m = dict(NAME="resnet50se", NUM_CLASSES=C, MARGIN="None", TYPE_SEMI="FixMatch", IS_TRIPLET=False,
             PRE_TRAIN_PATH="None", LOW_DIM=64)
    train = {"IS_SSL": model.pop("IS_SSL", True)}
    m.update(model)
    return AttrDict(DATA=AttrDict(IMG_SIZE=224), MODEL=AttrDict(**m), TRAIN=AttrDict(**train))


def _fixture_layout():
    with open(os.path.join(GOLDEN, "seresnet50_state_dict.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)]


def test_layout_is_the_reference_state_dict():
    from endossl.resnet import RESNET50, NativeSEResNet, ResNetConfig, resnet_layout
    want = _fixture_layout()
    assert len(want) == 352
    cfg = ResNetConfig(num_classes=C, se=True, **RESNET50)
    assert [(n, tuple(s)) for n, s, _ in resnet_layout(cfg)] == want
    sd = NativeSEResNet(cfg, seed=0).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    keys = list(sd)
    i = keys.index("layer1.0.conv_down.weight")  # after bn3.*, before downsample.*
    assert keys[i - 1] == "layer1.0.bn3.num_batches_tracked" and keys[i + 1] == "layer1.0.conv_up.weight"
    assert keys[i + 2] == "layer1.0.downsample.0.weight"
    assert tuple(sd["layer4.2.conv_down.weight"].shape) == (128, 2048, 1, 1)
    assert tuple(sd["layer1.1.conv_up.weight"].shape) == (256, 16, 1, 1)
    # the restatement registers the same names in the same order
    assert [(k, tuple(v.shape)) for k, v in SEResNet50(C).state_dict().items()] == want
    # se=False is the resnet50 layout, unchanged
    plain = [n for n, _, _ in resnet_layout(ResNetConfig(num_classes=C, **RESNET50))]
    assert plain == [k for k, _ in want if ".conv_down." not in k and ".conv_up." not in k]


def test_parameter_count_and_init():
    from endossl.resnet import RESNET50, NativeSEResNet, ResNetConfig
    m = NativeSEResNet(ResNetConfig(num_classes=C, se=True, **RESNET50), seed=3)
    assert sum(p.numel() for p in m.parameters()) == PARAMS
    assert sum(p.numel() for p in SEResNet50(C).parameters()) == PARAMS
    sd = m.state_dict()
    # the reference's rule (se.py:78-84): normal(0, sqrt(2 / (k^2 Cout))) for every conv, the SE ones included
    w = sd["layer3.0.conv_up.weight"]  # [1024, 64, 1, 1]
    assert abs(w.std().item() / (2.0 / 1024) ** 0.5 - 1) < 0.02
    w = sd["layer4.0.conv_down.weight"]  # [128, 2048, 1, 1]
    assert abs(w.std().item() / (2.0 / 128) ** 0.5 - 1) < 0.02
    assert torch.all(sd["layer1.0.bn3.weight"] == 1) and torch.all(sd["layer4.2.bn3.bias"] == 0)
    assert sd["fc.weight"].abs().max().item() <= 2048 ** -0.5
    with pytest.raises(ValueError, match="se=True"):
        NativeSEResNet(ResNetConfig(num_classes=C, **RESNET50))
    with pytest.raises(ValueError, match="Bottleneck"):
        ResNetConfig(se=True)  # basic blocks carry no gate


def test_build_model_routes_resnet50se():
    from endossl.build import build_model
    from endossl.resnet import NativeResNet, NativeSEResNet
    for ssl in (True, False):  # FixMatch and plain SupLearning
        m = build_model(_cfg(IS_SSL=ssl))
        assert type(m) is NativeSEResNet and isinstance(m, NativeResNet)
        assert m.cfg.se and m.cfg.block == "bottleneck" and m.cfg.num_features == 2048 and m.conv_1x1
        assert tuple(m.fc.weight.shape) == (C, 2048) and tuple(m.fc.bias.shape) == (C,)
        assert not hasattr(m, "engine")  # FixMatch's cnn path
    assert type(m).__name__ != "NativeResNet"  # SupLearning's graph replay keys on that name: this model runs eagerly


@pytest.mark.parametrize("kw,what", [(dict(IS_TRIPLET=True, IS_SSL=False), "ModelwEmb"),
                                     (dict(IS_TRIPLET=True), "ModelwEmb"),
                                     (dict(TYPE_SEMI="CoMatch"), "CoMatch"),
                                     (dict(MARGIN="cosface", IS_SSL=False), "MODEL.MARGIN"),
                                     (dict(MARGIN="arcface"), "MODEL.MARGIN")])
def test_out_of_scope_modes_raise(kw, what):
    from endossl.build import build_model
    with pytest.raises(NotImplementedError, match=what):
        build_model(_cfg(**kw))


def test_pretrained_checkpoint_is_reheaded(tmp_path):
    """PRE_TRAIN_PATH: model_state_dict loaded with weights_only=True; a 2-class fc is dropped (code/build.py:158-165)."""
    from endossl.build import build_model
    from endossl.resnet import RESNET50, NativeSEResNet, ResNetConfig
    src = NativeSEResNet(ResNetConfig(num_classes=2, se=True, **RESNET50), seed=11)
    path = str(tmp_path / "abnormal.pth")
    torch.save({"model_state_dict": src.state_dict()}, path)
    m = build_model(_cfg(PRE_TRAIN_PATH=path), seed=5)
    fresh = build_model(_cfg(), seed=5)
    sd, ssd, fsd = m.state_dict(), src.state_dict(), fresh.state_dict()
    assert tuple(sd["fc.weight"].shape) == (C, 2048)
    for k, v in sd.items():
        assert torch.equal(v, fsd[k] if k.startswith("fc.") else ssd[k]), k
    same = NativeSEResNet(ResNetConfig(num_classes=C, se=True, **RESNET50), seed=12)
    torch.save({"model_state_dict": same.state_dict()}, path)
    m = build_model(_cfg(PRE_TRAIN_PATH=path), seed=5)
    assert torch.equal(m.state_dict()["fc.weight"], same.state_dict()["fc.weight"])  # a matching head is kept


def test_state_dict_round_trip_and_deepcopy():
    from endossl.resnet import RESNET50, NativeSEResNet, ResNetConfig
    ref = SEResNet50(C)
    m = NativeSEResNet(ResNetConfig(num_classes=C, se=True, **RESNET50), seed=1)
    rsd = ref.state_dict()
    g = torch.Generator().manual_seed(0)
    for k, v in rsd.items():
        if v.is_floating_point():
            v.copy_(torch.randn(v.shape, generator=g))
        else:
            v.fill_(7)
    m.load_state_dict(rsd)
    back = m.state_dict()
    for k, v in rsd.items():
        assert torch.equal(back[k], v), k
    SEResNet50(C).load_state_dict(back)  # strict: nothing missing, nothing unexpected
    p = m.get_parameter("layer2.1.conv_up.weight")  # a view of the flat buffer
    assert p.data_ptr() == m.flat.data_ptr() + 4 * m.offs["layer2.1.conv_up.weight"]
    e = copy.deepcopy(m)
    assert type(e) is type(m) and e.cfg.se and e.flat.data_ptr() != m.flat.data_ptr()
    assert torch.equal(e.flat, m.flat) and list(e.state_dict()) == list(back)
    e.flat.add_(1.0)
    assert torch.equal(m.state_dict()["layer2.1.conv_up.weight"], rsd["layer2.1.conv_up.weight"])
    # the weight-decay split is NativeResNet's
    assert m.no_weight_decay() == set()
    with pytest.raises(Exception):
        m(torch.zeros(1, 3, 64, 64))  # CPU: no fallback


@pytest.mark.parametrize("tag", ["identity", "downsample"])
def test_restatement_block_matches_the_reference_fixture(golden, tag):
    """The restatement's SEBottleneck against what the reference's own Bottleneck computed (float64 against float64,
    float32 against float32): the same torch ops on the same machine class, so the bars are a few ulps of the
    result's scale -- 1e-12 relative in float64, 1e-5 in float32 (sums of up to 1152 products)."""
    d = golden(f"se_block_{tag}.npz")
    inp, planes, stride = int(d["inplanes"]), int(d["planes"]), int(d["stride"])
    assert (inp, planes, stride) == ((128, 32, 1) if tag == "identity" else (64, 32, 2))
    for dt, sfx, tol in ((torch.float64, "", 1e-12), (torch.float32, "_f32", 1e-5)):
        blk = SEBottleneck(inp, planes, stride).to(dt).train()
        init = {k[5:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("init/")}
        assert list(blk.state_dict()) == list(init)
        blk.load_state_dict({k: (v.to(dt) if v.is_floating_point() else v) for k, v in init.items()})
        x = torch.from_numpy(d["x"]).to(dt).requires_grad_(True)
        out = blk(x)
        (out * torch.from_numpy(d["g"]).to(dt)).sum().backward()

        def close(got, name):
            want = torch.from_numpy(d[name]).to(dt)
            err = (got.detach() - want).abs().max().item()
            assert err <= tol * max(1.0, want.abs().max().item()), (tag, name, err)
        close(out, "out" + sfx)
        close(x.grad, "dx" + sfx)
        for k, p in blk.named_parameters():
            close(p.grad, f"grad{sfx}/{k}")
        for k, b in blk.named_buffers():
            if b.is_floating_point():
                close(b, f"buf{sfx}/{k}")
            else:
                assert int(b) == int(d[f"buf{sfx}/{k}"]) == 1


def test_se_entry_points_validate_before_any_launch():
    """Every csrc/se.hip entry point refuses what its kernels cannot take before touching the GPU: C not a multiple
    of 16 or outside [16, 2048], R outside [1, 128], N or HW below 1 (ES_BAD_SHAPE = -1); a null required pointer, a
    misaligned map or an unknown flag bit (ES_BAD_ARG = -2).  The pointers are never dereferenced on these paths."""
    from endossl import _lib
    lib = _lib.load()
    p = 0x7000000000
    good = dict(N=2, HW=4, C=64, R=16)
    bad_maps = [dict(C=24), dict(C=8), dict(C=0), dict(C=2064), dict(C=4096), dict(N=0), dict(HW=0), dict(N=-1)]
    bad_gate = [dict(C=24), dict(C=8), dict(C=4096), dict(N=0), dict(R=0), dict(R=129)]

    def squeeze(N, HW, C, R, y=p, mean=p, ybar=p, ws=p, flags=0):
        return lib.es_se_squeeze_ex(y, N, HW, C, mean, p, p, p, ybar, p, ws, flags, None)

    def gate_fwd(N, HW, C, R, a=p, wd=p, wu=p, h=p, s=p):
        return lib.es_se_gate_fwd(a, wd, wu, N, C, R, h, s, None)

    def apply(N, HW, C, R, y=p, res=p, s=p, out=p, beta=p, flags=0):
        return lib.es_se_bn_apply_ex(y, res, s, N, HW, C, p, p, p, beta, out, flags, None)

    def sums(N, HW, C, R, y=p, out=p, dout=p, p1=p, p2=p, ws=p, flags=0):
        return lib.es_se_bn_bwd_sums_ex(y, out, dout, N, HW, C, p, p, p1, p2, ws, flags, None)

    def gate_bwd(N, HW, C, R, p1=p, h=p, wu=p, dwd=p, dwu=p, da=p, dg=p, db=p, ws=p):
        return lib.es_se_gate_bwd(p1, p, p, p, h, p, p, wu, p, p, p, p, N, C, R, dwd, dwu, da, dg, db, ws, None)

    def dx(N, HW, C, R, y=p, out=p, dout=p, s=p, da=p, dg=p, db=p, dy=p, gres=p, train=1, flags=0):
        return lib.es_se_bn_bwd_dx_ex(y, out, dout, s, da, N, HW, C, p, p, p, dg, db, train, dy, gres, 0, flags, None)

    for fn, bads, nulls in ((squeeze, bad_maps, ("y", "mean", "ybar", "ws")),
                            (gate_fwd, bad_gate, ("a", "wd", "wu", "h", "s")),
                            (apply, bad_maps, ("y", "res", "s", "out", "beta")),
                            (sums, bad_maps, ("y", "out", "dout", "p1", "p2", "ws")),
                            (gate_bwd, bad_gate, ("p1", "h", "wu", "dwd", "dwu", "da", "dg", "db", "ws")),
                            (dx, bad_maps, ("y", "out", "dout", "s", "da", "dg", "db", "dy", "gres"))):
        for b in bads:
            assert fn(**{**good, **b}) == -1, (fn.__name__, b)
        for k in nulls:
            assert fn(**good, **{k: None}) == -2, (fn.__name__, k)
    for fn in (squeeze, apply, sums, dx):
        assert fn(**good, flags=2) == -2, fn.__name__
        assert fn(**good, y=p + 4) == -2, fn.__name__  # 16-byte vector accesses
    # workspace queries: 0 for an unsupported shape, otherwise at least one partial row per image
    assert lib.es_se_squeeze_workspace(2, 4, 24, 0) == 0 and lib.es_se_bn_bwd_sums_workspace(0, 4, 64, 0) == 0
    assert lib.es_se_gate_bwd_workspace(2, 64, 129) == 0
    assert lib.es_se_squeeze_workspace(2, 4, 64, 0) >= 2 * 64
    assert lib.es_se_bn_bwd_sums_workspace(2, 4, 64, 1) >= 2 * 2 * 64
    assert lib.es_se_gate_bwd_workspace(2, 64, 16) >= 2 * 64 + 2 * 16
    # the split grows with HW (2 x 56 x 56 x 64: more than one partial row per image)
    assert lib.es_se_squeeze_workspace(2, 56 * 56, 64, 1) > 2 * 64
    # es_se_bn_stats
    assert lib.es_se_bn_stats(p, p, 0, 64, 1e-5, 0.1, 1, p, p, p, p, None, None) == -1
    assert lib.es_se_bn_stats(None, p, 8, 64, 1e-5, 0.1, 1, p, p, p, p, None, None) == -2
    assert lib.es_se_bn_stats(p, p, 8, 64, 1e-5, 0.1, 1, None, p, p, p, None, None) == -2
