"""DenseNet-161 (`densenet161`) host side (no GPU): torchvision's state_dict (names, order, shapes, parameter counts)
against the plain-torch.nn restatement, round trips, the factory branch and its refusals, the config's validation and
the zero padding the padded convs rely on."""
import copy

import pytest
import torch

from densenet_restatement import DenseNet

C = 23
TINY = dict(block_config=(6, 2), growth=48, bn_size=4, init_features=96)


def _cfg(**model):
    from endossl.utils import AttrDict
    m = dict(NAME="densenet161", NUM_CLASSES=C, MARGIN="None", TYPE_SEMI="FixMatch", IS_TRIPLET=False,
             PRE_TRAIN_PATH="None", LOW_DIM=64)
    train = {"IS_SSL": model.pop("IS_SSL", True)}
    m.update(model)
    return AttrDict(DATA=AttrDict(IMG_SIZE=224), MODEL=AttrDict(**m), TRAIN=AttrDict(**train))


def _configs():
    from endossl.densenet import DENSENET161, DenseNetConfig
    return [DenseNetConfig(num_classes=C, **DENSENET161), DenseNetConfig(num_classes=5, **TINY)]


def test_layout_is_torchvisions_state_dict():
    from endossl.densenet import NativeDenseNet, densenet_layout
    for cfg in _configs():
        want = [(k, tuple(v.shape)) for k, v in DenseNet(cfg).state_dict().items()]
        assert [(n, tuple(s)) for n, s, _ in densenet_layout(cfg)] == want
        sd = NativeDenseNet(cfg, seed=0).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    keys = [k for k, _ in want]  # the tiny config's
    assert keys[:6] == ["features.conv0.weight", "features.norm0.weight", "features.norm0.bias",
                        "features.norm0.running_mean", "features.norm0.running_var",
                        "features.norm0.num_batches_tracked"]
    i = keys.index("features.denseblock1.denselayer1.conv1.weight")
    assert keys[i - 1] == "features.denseblock1.denselayer1.norm1.num_batches_tracked"
    assert keys[i + 1] == "features.denseblock1.denselayer1.norm2.weight"
    assert keys[-2:] == ["classifier.weight", "classifier.bias"]
    full = dict((k, tuple(v.shape)) for k, v in NativeDenseNet(_configs()[0], seed=0).state_dict().items())
    assert full["features.denseblock3.denselayer36.conv1.weight"] == (192, 2064, 1, 1)
    assert full["features.denseblock4.denselayer24.conv2.weight"] == (48, 192, 3, 3)
    assert full["features.transition3.conv.weight"] == (1056, 2112, 1, 1)
    assert full["features.norm5.running_var"] == (2208,) and full["classifier.weight"] == (C, 2208)
    assert full["features.transition1.norm.num_batches_tracked"] == ()


def test_parameter_counts_and_init():
    from endossl.densenet import DENSENET161, DenseNetConfig, NativeDenseNet
    m = NativeDenseNet(DenseNetConfig(num_classes=1000, **DENSENET161), seed=1)
    assert sum(p.numel() for p in m.parameters()) == 28_681_000
    m = NativeDenseNet(DenseNetConfig(num_classes=C, **DENSENET161), seed=1)
    assert sum(p.numel() for p in m.parameters()) == 26_522_807
    assert sum(p.numel() for n, p in m.named_parameters() if n.startswith("features.")) == 26_472_000
    assert sum(p.numel() for p in DenseNet(m.cfg).parameters()) == 26_522_807
    assert m.cfg.num_features == m.cfg.dim == 2208
    assert [b[2] for b in m.cfg.blocks()] == [384, 768, 2112, 2208] and [b[0] for b in m.cfg.blocks()] == [96, 192, 384, 1056]
    sd = m.state_dict()
    w = sd["features.denseblock3.denselayer5.conv1.weight"]  # kaiming_normal_: std = sqrt(2 / fan_in)
    assert abs(w.std().item() / (2.0 / w.shape[1]) ** 0.5 - 1) < 0.02
    w = sd["features.denseblock2.denselayer3.conv2.weight"]
    assert abs(w.std().item() / (2.0 / (192 * 9)) ** 0.5 - 1) < 0.02
    assert torch.all(sd["features.norm5.weight"] == 1) and torch.all(sd["features.transition2.norm.bias"] == 0)
    assert torch.all(sd["classifier.bias"] == 0) and 0 < sd["classifier.weight"].abs().max().item() <= 2208 ** -0.5
    # the surface the trainers use: `classifier` is a real submodule and `fc` is the same module
    assert m.fc is m.classifier and isinstance(m.classifier, torch.nn.Module)
    assert [n for n, _ in m.fc.named_parameters()] == ["weight", "bias"]
    assert not hasattr(m, "engine") and m.no_weight_decay() == set()
    assert not any(n.startswith("fc.") for n, _ in m.named_parameters())


def test_state_dict_round_trip_and_deepcopy():
    from endossl.densenet import DenseNetConfig, NativeDenseNet
    cfg = DenseNetConfig(num_classes=5, **TINY)
    ref = DenseNet(cfg)
    m = NativeDenseNet(cfg, seed=1)
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
    DenseNet(cfg).load_state_dict(back)  # strict: nothing missing, nothing unexpected
    name = "features.denseblock2.denselayer2.conv1.weight"
    assert m.get_parameter(name).data_ptr() == m.flat.data_ptr() + 4 * m.offs[name]
    e = copy.deepcopy(m)
    assert type(e) is type(m) and e.flat.data_ptr() != m.flat.data_ptr()
    assert torch.equal(e.flat, m.flat) and list(e.state_dict()) == list(back)
    e.flat.add_(1.0)
    assert torch.equal(m.state_dict()[name], rsd[name])
    with pytest.raises(Exception):
        m(torch.zeros(1, 3, 64, 64))  # CPU: no fallback


def test_build_model_routes_densenet161():
    from endossl.build import build_model
    from endossl.densenet import NativeDenseNet
    for ssl in (True, False):  # FixMatch and plain SupLearning
        m = build_model(_cfg(IS_SSL=ssl))
        assert type(m) is NativeDenseNet
        assert m.cfg.block_config == (6, 12, 36, 24) and m.cfg.growth == 48 and m.cfg.num_features == 2208
        assert tuple(m.fc.weight.shape) == (C, 2208) and tuple(m.classifier.bias.shape) == (C,)
        assert not hasattr(m, "engine")  # FixMatch's cnn path
    assert type(m).__name__ != "NativeResNet"  # SupLearning's graph replay keys on that name: this model runs eagerly


@pytest.mark.parametrize("kw,what", [(dict(TYPE_SEMI="CoMatch"), "densenet161 for .*ModelwEmb"),
                                     (dict(IS_TRIPLET=True, IS_SSL=False), "densenet161 for .*ModelwEmb"),
                                     (dict(MARGIN="cosface", IS_SSL=False), "timm's densenet161 has `classifier`")])
def test_out_of_scope_modes_raise(kw, what):
    from endossl.build import build_model
    with pytest.raises(NotImplementedError, match=what):
        build_model(_cfg(**kw))


def test_pretrained_checkpoint_is_reheaded(tmp_path):
    """PRE_TRAIN_PATH: model_state_dict loaded with weights_only=True; a 2-class classifier is dropped
    (code/build.py:190-193,213-216)."""
    from endossl.build import build_model
    from endossl.densenet import DENSENET161, DenseNetConfig, NativeDenseNet
    src = NativeDenseNet(DenseNetConfig(num_classes=2, **DENSENET161), seed=11)
    path = str(tmp_path / "abnormal.pth")
    torch.save({"model_state_dict": src.state_dict()}, path)
    m = build_model(_cfg(PRE_TRAIN_PATH=path), seed=5)
    fresh = build_model(_cfg(), seed=5)
    sd, ssd, fsd = m.state_dict(), src.state_dict(), fresh.state_dict()
    assert tuple(sd["classifier.weight"].shape) == (C, 2208)
    for k, v in sd.items():
        assert torch.equal(v, fsd[k] if k.startswith("classifier.") else ssd[k]), k
    same = NativeDenseNet(DenseNetConfig(num_classes=C, **DENSENET161), seed=12)
    torch.save({"model_state_dict": same.state_dict()}, path)
    m = build_model(_cfg(PRE_TRAIN_PATH=path), seed=5)
    assert torch.equal(m.state_dict()["classifier.weight"], same.state_dict()["classifier.weight"])  # kept


def test_config_validation():
    from endossl.densenet import DenseNetConfig
    DenseNetConfig(block_config=(6, 2))
    with pytest.raises(ValueError, match="240"):
        DenseNetConfig(block_config=(3, 2))  # block 1's output: 96 + 3 * 48 = 240 = 16 (mod 32)
    with pytest.raises(ValueError, match="growth"):
        DenseNetConfig(growth=40)
    with pytest.raises(ValueError, match="bn_size"):
        DenseNetConfig(growth=16, bn_size=1, init_features=64, block_config=(2, 2))
    with pytest.raises(ValueError, match="input width"):
        DenseNetConfig(init_features=80)


def test_flat_layout_zero_pads_the_padded_norms():
    """A conv1 over a prefix of 16 (mod 32) channels gathers 16 channels past its norm1: their gamma / beta are the
    flat layout's alignment padding -- at least 16 floats, zero, and nothing names them (no state_dict entry)."""
    from endossl.densenet import DENSENET161, DenseNetConfig, NativeDenseNet
    m = NativeDenseNet(DenseNetConfig(num_classes=C, **DENSENET161), seed=2)
    pads = m.padded_norms()
    assert len(pads) == 39 and all(c % 32 == 16 and cp == c + 16 for _, c, cp in pads)
    named = torch.zeros(m.numel, dtype=torch.bool)
    for name, p in m.named_parameters():
        named[m.offs[name]:m.offs[name] + p.numel()] = True
    m.flat.data[named] = 1.0  # every parameter non-zero: what stays zero is padding
    for pre, c, cp in pads:
        for nm in (pre + "weight", pre + "bias"):
            o = m.offs[nm]
            assert o % 64 == 0
            assert not named[o + c:o + cp].any() and torch.all(m.flat[o + c:o + cp] == 0), nm
    assert int(named.sum()) == 26_522_807
    m._check_padding()
    m.offs[pads[0][0] + "weight"] += 48  # a layout without the room is refused
    with pytest.raises(AssertionError, match="padding floats"):
        m._check_padding()
