"""ResNet-50 host side (no GPU): the factory branches, timm's state_dict through a plain-torch.nn restatement
(tests/resnet50_restatement.py; timm and torchvision are absent), ModelMargin's aliases, the scoped refusals of the
embedding-head modes, and ResNetConfig()'s unchanged ResNet-18 layout."""
import pytest
import torch

from resnet50_restatement import ResNet50

C = 23
PARAMS = 23_555_159  # timm resnet50: 23,508,032 trunk + 2048 * 23 + 23


def _cfg(**model):
    from endossl.utils import AttrDict
    m = dict(NAME="resnet50", NUM_CLASSES=C, MARGIN="None", TYPE_SEMI="FixMatch", IS_TRIPLET=False,
             PRE_TRAIN_PATH="None", LOW_DIM=64)
    train = {"IS_SSL": model.pop("IS_SSL", True)}
    m.update(model)
    return AttrDict(DATA=AttrDict(IMG_SIZE=224), MODEL=AttrDict(**m), TRAIN=AttrDict(**train))


def test_build_model_resnet50():
    from endossl.build import build_model
    from endossl.resnet import NativeResNet
    for ssl in (True, False):  # FixMatch and plain SupLearning
        m = build_model(_cfg(IS_SSL=ssl))
        assert type(m) is NativeResNet
        assert sum(p.numel() for p in m.parameters()) == PARAMS
        assert m.cfg.block == "bottleneck" and m.cfg.num_features == 2048 and m.conv_1x1
        assert tuple(m.fc.weight.shape) == (C, 2048) and tuple(m.fc.bias.shape) == (C,)
    stages = [(inp, w, s, ds) for _, inp, w, s, ds in m.cfg.blocks()]
    assert len(stages) == 16
    assert stages[0] == (64, 64, 1, True) and stages[1] == (256, 64, 1, False)
    assert stages[3] == (256, 128, 2, True) and stages[7] == (512, 256, 2, True) and stages[13] == (1024, 512, 2, True)
    assert stages[15] == (2048, 512, 1, False)


def test_state_dict_is_timm_resnet50():
    from endossl.resnet import RESNET50, NativeResNet, ResNetConfig
    ref = ResNet50(C)
    assert sum(p.numel() for p in ref.parameters()) == PARAMS
    m = NativeResNet(ResNetConfig(num_classes=C, **RESNET50), seed=1)
    sd, rsd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(rsd[k].shape) and sd[k].dtype == rsd[k].dtype, k
    # round trip: the restatement's (random) state into the native model and back, bit for bit
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
    ref2 = ResNet50(C)
    ref2.load_state_dict(back)  # strict: nothing missing, nothing unexpected


def test_init_convention():
    """kaiming fan-out convs, every BatchNorm weight 1 (bn3 too: zero_init_last_bn is not restated), fc uniform."""
    from endossl.resnet import RESNET50, NativeResNet, ResNetConfig
    sd = NativeResNet(ResNetConfig(num_classes=C, **RESNET50), seed=3).state_dict()
    assert torch.all(sd["layer1.0.bn3.weight"] == 1) and torch.all(sd["layer4.2.bn3.bias"] == 0)
    w = sd["layer3.0.conv3.weight"]  # [1024, 256, 1, 1]: std = sqrt(2 / 1024)
    assert abs(w.std().item() / (2.0 / 1024) ** 0.5 - 1) < 0.02
    assert sd["fc.weight"].abs().max().item() <= 2048 ** -0.5


def test_model_margin_resnet50():
    from endossl.build import build_model
    from endossl.resnet import ModelMargin
    m = build_model(_cfg(MARGIN="cosface", IS_SSL=False))
    assert type(m) is ModelMargin and m.cfg.block == "bottleneck"
    sd = m.state_dict()
    keys = list(sd)
    assert keys[-1] == "fc.weight" and all(k.startswith("model.") for k in keys[:-1])
    assert "model.fc.weight" in sd and "model.fc.bias" not in sd and "fc.bias" not in sd
    assert tuple(sd["fc.weight"].shape) == (C, 2048) and torch.equal(sd["fc.weight"], sd["model.fc.weight"])
    ref = ResNet50(C, fc_bias=False)
    assert keys[:-1] == ["model." + k for k in ref.state_dict()]
    # the reference's duplicate `backbone.N.*` listing of the trunk is skipped on load
    other = build_model(_cfg(MARGIN="cosface", IS_SSL=False), seed=9)
    load = dict(sd)
    load["backbone.0.weight"] = torch.zeros(1)
    load["backbone.4.0.conv1.weight"] = torch.zeros(1)
    other.load_state_dict(load)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(NotImplementedError, match="resnet18 and resnet50"):
        build_model(_cfg(NAME="vit_small_patch16_224", MARGIN="cosface", IS_SSL=False))


@pytest.mark.parametrize("kw,what", [(dict(TYPE_SEMI="CoMatch"), "ModelwEmb"),
                                     (dict(IS_TRIPLET=True, IS_SSL=False), "ModelwEmb"),
                                     (dict(IS_TRIPLET=True, IS_SSL=False, PRE_TRAIN_PATH="/x/sup_resnet50.pth"),
                                      "ModelwEmb"),  # the reference's kaggle_supervised_ezbm config
                                     (dict(PRE_TRAIN_PATH="/x/sup_resnet50.pth"), "PRE_TRAIN_PATH"),
                                     (dict(PRE_TRAIN_PATH="/x/sup_resnet50.pth", IS_SSL=False), "PRE_TRAIN_PATH")])
def test_out_of_scope_modes_raise(kw, what):
    from endossl.build import build_model
    with pytest.raises(NotImplementedError, match=what):
        build_model(_cfg(**kw))


def test_default_config_is_still_resnet18():
    """ResNetConfig() -> the layout ResNet-18 had before the bottleneck case existed, written out here."""
    from endossl.resnet import NativeResNet, ResNetConfig, resnet_layout

    def bn(pre, c):
        return [(pre + "weight", (c,), "p"), (pre + "bias", (c,), "p"), (pre + "running_mean", (c,), "rm"),
                (pre + "running_var", (c,), "rv"), (pre + "num_batches_tracked", (), "nbt")]
    want = [("conv1.weight", (64, 3, 7, 7), "p")] + bn("bn1.", 64)
    for pre, inp, w, ds in (("layer1.0.", 64, 64, False), ("layer1.1.", 64, 64, False),
                            ("layer2.0.", 64, 128, True), ("layer2.1.", 128, 128, False),
                            ("layer3.0.", 128, 256, True), ("layer3.1.", 256, 256, False),
                            ("layer4.0.", 256, 512, True), ("layer4.1.", 512, 512, False)):
        want += [(pre + "conv1.weight", (w, inp, 3, 3), "p")] + bn(pre + "bn1.", w)
        want += [(pre + "conv2.weight", (w, w, 3, 3), "p")] + bn(pre + "bn2.", w)
        if ds:
            want += [(pre + "downsample.0.weight", (w, inp, 1, 1), "p")] + bn(pre + "downsample.1.", w)
    want += [("fc.weight", (23, 512), "p"), ("fc.bias", (23,), "p")]
    cfg = ResNetConfig()
    assert resnet_layout(cfg) == want and len(want) == 122
    assert cfg.block == "basic" and cfg.expansion == 1 and cfg.num_features == 512
    m = NativeResNet(cfg, seed=0)
    assert sum(p.numel() for p in m.parameters()) == 11_188_311 and not m.conv_1x1
