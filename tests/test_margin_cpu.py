"""Angular-margin supervised mode, host side: build_model's routing to resnet.ModelMargin (layout, state-dict
names, deepcopy), SupLearning.get_config's errors, and the float64 restatement of the kernel's contract
(tests/margin_restatement.py) pinned to the reference-generated fixtures tests/golden/margin_*.npz to rtol 1e-9
-- the GPU tests then hold the kernel to that restatement where the reference itself is absent.

The same restatement in fp32 against the float32 fixtures is MEASURED here (printed, and recorded in DESIGN.md
"Angular-margin mode"): the reference's own fp32-vs-fp64 spread, in the units of the project's fp32 loss-kernel
bars (loss rtol 1e-5; gradients rtol 1e-4 / atol 1e-6, tests/test_gpu_triplet.py:6-10).  The only assertion on
it is that the reference's fp32 run itself sits inside those bars: the fixtures are well-posed for them.
"""
from copy import deepcopy

import pytest
import torch

import margin_restatement as mr


def _cfg(name="resnet18", margin="arcface", **model):
    from endossl.utils import AttrDict, with_defaults
    return with_defaults(AttrDict(MODEL=AttrDict(NAME=name, NUM_CLASSES=23, MARGIN=margin, **model),
                                  TRAIN=AttrDict(IS_SSL=False), DATA=AttrDict(IMG_SIZE=64)))


# ------------------------------------------------------------------------------------------ build_model
def test_build_model_routes_margin_to_model_margin():
    from endossl.build import build_model
    from endossl.resnet import ModelMargin, NativeResNet, resnet_layout, ResNetConfig
    # PRE_TRAIN_PATH is not read on this branch (code/build.py:173-174 comes first): a path that does not exist
    m = build_model(_cfg(PRE_TRAIN_PATH="/nonexistent/checkpoint.pth"))
    assert type(m) is ModelMargin and isinstance(m, NativeResNet)
    names = [n for n, _, _ in m.layout]
    assert "fc.weight" in names and "fc.bias" not in names and "fc.bias" not in m.offs
    assert m.numel == NativeResNet(ResNetConfig(num_classes=23), seed=0).numel - 64  # the bias' padded slot
    assert tuple(m.fc.weight.shape) == (23, 512) and getattr(m.fc, "bias", None) is None
    assert m.fc.weight.data_ptr() == m.pview("fc.weight").data_ptr()  # .fc exposes the flat buffer's view
    assert callable(m.backbone)
    # the plain model is unchanged
    p = build_model(_cfg(margin="None"))
    assert type(p) is NativeResNet and "fc.bias" in p.offs
    assert [n for n, _, _ in resnet_layout(ResNetConfig())][-2:] == ["fc.weight", "fc.bias"]


def test_model_margin_state_dict_names_and_loading():
    from endossl.build import build_model
    from endossl.resnet import NativeResNet, ResNetConfig
    m = build_model(_cfg(margin="cosface"), seed=1)
    sd = m.state_dict()
    plain = [k for k in NativeResNet(ResNetConfig(num_classes=23), seed=0).state_dict() if k != "fc.bias"]
    assert list(sd) == ["model." + k for k in plain] + ["fc.weight"]
    assert "model.fc.bias" not in sd and "fc.bias" not in sd
    assert sd["fc.weight"].data_ptr() == sd["model.fc.weight"].data_ptr()  # an alias, as in the reference
    # a reference checkpoint also lists the trunk as backbone.N.* (nn.Sequential over timm's children)
    new = {k: torch.full_like(v, 0.25) if v.is_floating_point() else v.clone() for k, v in sd.items()}
    new["backbone.0.weight"] = torch.zeros(64, 3, 7, 7)
    new["backbone.1.running_mean"] = torch.zeros(64)
    new["backbone.4.0.conv1.weight"] = torch.zeros(1)  # never read: not even its shape
    m.load_state_dict(new)
    assert float(m.flat[m.offs["conv1.weight"]]) == 0.25 and float(m.pview("fc.weight")[0]) == 0.25
    # the alias alone carries fc.weight too
    only_alias = {k: v for k, v in new.items() if k != "model.fc.weight"}
    only_alias["fc.weight"] = torch.full((23, 512), 0.5)
    m.load_state_dict(only_alias)
    assert float(m.pview("fc.weight")[-1]) == 0.5
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in new.items() if k != "model.conv1.weight"})  # strict: a missing key


def test_model_margin_deepcopy_gives_independent_flat():
    from endossl.build import build_model
    m = build_model(_cfg(), seed=2)
    e = deepcopy(m)
    assert type(e) is type(m) and e.flat.data_ptr() != m.flat.data_ptr()
    torch.testing.assert_close(e.flat, m.flat)
    e.flat.add_(1.0)
    assert float((e.flat - m.flat).abs().min()) > 0.5
    assert list(e.state_dict()) == list(m.state_dict())
    assert e.fc.weight.data_ptr() == e.pview("fc.weight").data_ptr() != m.fc.weight.data_ptr()
    with pytest.raises(Exception):
        m(torch.zeros(1, 3, 64, 64))  # CPU: no fallback
    with pytest.raises(Exception):
        m.backbone(torch.zeros(1, 3, 64, 64))


def test_margin_with_a_backbone_without_fc_raises():
    from endossl.build import build_model
    for name in ("vit_tiny_test", "vit_small_patch16_224"):
        with pytest.raises(NotImplementedError, match=r"\.fc"):
            build_model(_cfg(name=name))


# ------------------------------------------------------------------------------------------ get_config
class _DS:
    df = None


class _DL(list):
    dataset = _DS()


def _train_cfg(margin, triplet=False):
    from endossl.utils import AttrDict
    return AttrDict(DATA=AttrDict(BATCH_SIZE=4, IMG_SIZE=64, TARGET_NAME="target"),
                    MODEL=AttrDict(NAME="resnet18", NUM_CLASSES=23, MARGIN=margin, IS_TRIPLET=triplet),
                    TRAIN=AttrDict(USE_EMA=False, EMA_DECAY=0.999, BASE_LR=1e-3, CLS_WEIGHT=False, EPOCHS=1,
                                   WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="const",
                                   FREQ_EVAL=1, LAMBDA_C=1.0, THRES=0.5))


def test_get_config_margin_needs_backbone_and_fc():
    from endossl.resnet import NativeResNet, ResNetConfig
    from endossl.supervised import SupLearning
    from endossl.vit import NativeViT, ViTConfig
    for m in (NativeResNet(ResNetConfig(num_classes=23), seed=0),
              NativeViT(ViTConfig(img_size=64, dim=128, depth=2, heads=2, num_classes=23), seed=0)):
        tr = SupLearning(m, device="cpu")
        tr.get_dataloader(_DL([]), None)
        with pytest.raises(ValueError, match="backbone"):
            tr.get_config(_train_cfg("arcface"))


def test_get_config_margin_builds_the_loss():
    from endossl.build import build_model
    from endossl.loss import AngularPenaltySMLoss
    from endossl.supervised import SupLearning
    for kind, (s, m) in mr.DEFAULTS.items():
        tr = SupLearning(build_model(_cfg(margin=kind)), device="cpu")
        tr.get_dataloader(_DL([]), None)
        tr.get_config(_train_cfg(kind))
        assert tr.is_margin and not tr.is_triplet
        assert isinstance(tr.loss_fc, AngularPenaltySMLoss)
        assert (tr.loss_fc.loss_type, tr.loss_fc.s, tr.loss_fc.m, tr.loss_fc.eps) == (kind, s, m, 1e-7)
    tr.get_config(_train_cfg("None"))
    assert not tr.is_margin and tr.loss_fc is None
    with pytest.raises(ValueError):
        tr.get_config(_train_cfg("softmax"))  # not a margin loss


def test_margin_loss_defaults_and_overrides():
    from endossl.loss import AngularPenaltySMLoss
    from endossl.utils import AttrDict
    c = AttrDict(MODEL=AttrDict(MARGIN="sphereface"))
    a = AngularPenaltySMLoss(c)
    assert (a.s, a.m, a.eps) == (30.0, 1.35, 1e-7)
    a = AngularPenaltySMLoss(c, s=64.0, m=0.5, eps=1e-6)
    assert (a.s, a.m, a.eps) == (64.0, 0.5, 1e-6)


# ------------------------------------------------------------------ the restatement against the reference
CASES = [(k, v) for k in mr.KINDS for v in mr.VARIANTS + ("clamped",)]


def test_fixtures_cover_the_cases():
    for kind, variant in CASES:
        fx = mr.load_fixture(kind, variant)
        assert fx["kind"] == kind and (fx["s"], fx["m"]) == mr.DEFAULTS[kind] and fx["eps"] == 1e-7
        assert tuple(fx["x"].shape) == (24, 64) and tuple(fx["W"].shape) == (23, 64) and fx["y"].dtype == torch.int64
        assert (fx["w"] is not None) == (variant in ("weighted", "masked"))
        assert (fx["mask"] is not None) == (variant == "masked")
        if variant == "masked":
            assert set(fx["mask"].tolist()) == {0.0, 1.0}
        if variant == "clamped":
            rows = fx["clamped"].tolist()
            assert len(rows) == 5 and (fx["t"][rows].abs() > 1).all()
            assert (fx["t"][rows] > 1).any() and (fx["t"][rows] < -1).any()
        else:
            assert fx["t"].abs().max().item() <= 0.9 and fx["W"].norm(dim=1).max().item() <= 0.95 + 1e-6
        assert 0 in fx["y"].tolist() and 22 in fx["y"].tolist()


@pytest.mark.parametrize("kind,variant", CASES)
def test_restatement_reproduces_the_reference_float64(kind, variant):
    fx = mr.load_fixture(kind, variant)
    loss, dx, dW, _, _ = mr.loss_and_grads(fx["x"], fx["W"], fx["y"], kind, fx["s"], fx["m"], fx["eps"], w=fx["w"],
                                           mask=fx["mask"])
    torch.testing.assert_close(loss, torch.tensor(float(fx["loss"]), dtype=torch.float64), rtol=1e-9, atol=0)
    torch.testing.assert_close(dx, fx["dx"], rtol=1e-9, atol=1e-15)
    torch.testing.assert_close(dW, fx["dW"], rtol=1e-9, atol=1e-15)


def bar_units(d, ref, rtol=1e-4, atol=1e-6):
    """max |d - ref| / (atol + rtol |ref|): <= 1 is what assert_close(rtol, atol) accepts."""
    ref = ref.double()
    return ((d.double() - ref).abs() / (atol + rtol * ref.abs())).max().item()


def test_reference_fp32_spread_is_measured():
    """The reference's float32 run, and the restatement in float32, against the reference's float64 run on the
    smooth fixtures.  Printed per kind (run with -s); the figures are in DESIGN.md."""
    worst = {}
    for kind in mr.KINDS:
        ref32 = {"loss": 0.0, "dx": 0.0, "dW": 0.0}
        res32 = {"loss": 0.0, "dx": 0.0, "dW": 0.0}
        for variant in mr.VARIANTS:
            fx = mr.load_fixture(kind, variant)
            l64 = float(fx["loss"])
            ref32["loss"] = max(ref32["loss"], abs(float(fx["loss_f32"]) - l64) / abs(l64))
            ref32["dx"] = max(ref32["dx"], bar_units(fx["dx_f32"], fx["dx"]))
            ref32["dW"] = max(ref32["dW"], bar_units(fx["dW_f32"], fx["dW"]))
            loss, dx, dW, _, _ = mr.loss_and_grads(fx["x"], fx["W"], fx["y"], kind, fx["s"], fx["m"], fx["eps"],
                                                   w=fx["w"], mask=fx["mask"], dtype=torch.float32)
            res32["loss"] = max(res32["loss"], abs(float(loss) - l64) / abs(l64))
            res32["dx"] = max(res32["dx"], bar_units(dx, fx["dx"]))
            res32["dW"] = max(res32["dW"], bar_units(dW, fx["dW"]))
        print(f"{kind:10s} reference fp32 vs fp64: loss rel {ref32['loss']:.2e}, dx {ref32['dx']:.3f} bar, "
              f"dW {ref32['dW']:.3f} bar | restatement fp32: loss rel {res32['loss']:.2e}, dx {res32['dx']:.3f} bar, "
              f"dW {res32['dW']:.3f} bar")
        worst[kind] = ref32
    for kind, r in worst.items():
        # the comparison is well-posed: the reference's own fp32 run sits inside the project's fp32 bars
        assert r["loss"] <= 1e-5 and r["dx"] <= 1.0 and r["dW"] <= 1.0, (kind, r)
