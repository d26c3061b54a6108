"""NativeResNetEmb host side (no GPU): the opt-in routing of build_model, the reference's state_dict format against
the plain-torch.nn ModelwEmb restatement (tests/resnet_emb_restatement.py), MODEL.PRE_TRAIN_PATH into the trunk, the
data-parallel refusals of the trainers, and the exactness bound of the wide dense kernels' integer cases."""
import pytest
import torch

import head_cases as hc
from resnet50_restatement import ResNet50
from resnet_emb_restatement import ModelwEmb, native_keys

C = 6
REFUSALS = [(dict(TYPE_SEMI="CoMatch"), "ModelwEmb"),
            (dict(IS_TRIPLET=True, IS_SSL=False), "ModelwEmb"),
            (dict(IS_TRIPLET=True, IS_SSL=False, PRE_TRAIN_PATH="/x/sup_resnet50.pth"), "ModelwEmb"),
            (dict(PRE_TRAIN_PATH="/x/sup_resnet50.pth"), "PRE_TRAIN_PATH"),
            (dict(PRE_TRAIN_PATH="/x/sup_resnet50.pth", IS_SSL=False), "PRE_TRAIN_PATH")]
# (n, K, N) of tests/test_gpu_dense_wide.py's integer cases (the issue's table)
WIDE_SHAPES = [(1, 1, 1), (33, 65, 63), (31, 2, 257), (17, 2048, 512), (130, 2048, 768), (384, 2048, 512),
               (96, 2048, 192), (70, 192, 64), (70, 768, 256), (65, 512, 5), (3, 64, 2048)]


def _cfg(**model):
    from endossl.utils import AttrDict
    m = dict(NAME="resnet50", NUM_CLASSES=C, MARGIN="None", TYPE_SEMI="FixMatch", IS_TRIPLET=False,
             PRE_TRAIN_PATH="None", LOW_DIM=64)
    train = {"IS_SSL": model.pop("IS_SSL", True)}
    m.update(model)
    return AttrDict(DATA=AttrDict(IMG_SIZE=224), MODEL=AttrDict(**m), TRAIN=AttrDict(**train))


@pytest.mark.parametrize("kw,what", REFUSALS)
def test_switch_off_keeps_the_refusals(kw, what, monkeypatch):
    from endossl.build import build_model
    monkeypatch.delenv("ENDOSSL_CNN_EMB", raising=False)
    with pytest.raises(NotImplementedError, match=what) as e:
        build_model(_cfg(**kw))
    if what == "ModelwEmb":
        assert "ENDOSSL_CNN_EMB" in str(e.value) and "cnn_emb" in str(e.value)  # the message names the switch
    with pytest.raises(NotImplementedError, match=what):
        build_model(_cfg(**kw), cnn_emb=False)


@pytest.mark.parametrize("via", ["kwarg", "env"])
def test_switch_on_builds_the_embedding_model(via, monkeypatch):
    from endossl.build import TRIPLET_LOW_DIM, build_model
    from endossl.comatch_model import NativeResNetEmb
    from endossl.resnet import ModelMargin, NativeResNet, NativeSEResNet
    if via == "env":
        monkeypatch.setenv("ENDOSSL_CNN_EMB", "1")
        build = build_model
    else:
        monkeypatch.delenv("ENDOSSL_CNN_EMB", raising=False)
        build = lambda cfg: build_model(cfg, cnn_emb=True)  # noqa: E731
    for name, D in (("resnet50", 2048), ("resnet18", 512)):
        m = build(_cfg(NAME=name, TYPE_SEMI="CoMatch", LOW_DIM=32))
        assert type(m) is NativeResNetEmb and m.cfg.low_dim == 32 and m.cfg.dim == D and m.cfg.head == "emb"
        assert tuple(m.fc._modules["0"].weight.shape) == (D // 4, D)
        assert tuple(m.head_emb._modules["2"].weight.shape) == (32, 96)
        m = build(_cfg(NAME=name, IS_TRIPLET=True, IS_SSL=False, LOW_DIM=32))
        assert type(m) is NativeResNetEmb and m.cfg.low_dim == TRIPLET_LOW_DIM == 256
    # MODEL.MARGIN keeps its precedence, the plain modes their plain model, resnet50se its refusals
    assert type(build(_cfg(MARGIN="cosface", IS_TRIPLET=True, IS_SSL=False))) is ModelMargin
    assert type(build(_cfg(MARGIN="cosface", TYPE_SEMI="CoMatch"))) is ModelMargin
    assert type(build(_cfg())) is NativeResNet and type(build(_cfg(IS_SSL=False))) is NativeResNet
    assert type(build(_cfg(NAME="resnet50se"))) is NativeSEResNet
    for kw in (dict(TYPE_SEMI="CoMatch"), dict(IS_TRIPLET=True, IS_SSL=False)):
        with pytest.raises(NotImplementedError, match="resnet50se"):
            build(_cfg(NAME="resnet50se", **kw))
    with pytest.raises(NotImplementedError, match="PRE_TRAIN_PATH"):  # the simple re-head stays out of scope
        build(_cfg(PRE_TRAIN_PATH="/x/sup_resnet50.pth"))


def test_published_configs_build_and_the_trainers_accept_them(monkeypatch):
    """The MODEL / TRAIN sections of kaggle_semisupervised_real_1 / _1_1 (CoMatch, LOW_DIM 64) and
    kaggle_supervised_ezbm (IS_TRIPLET, no SSL) with the knob set, and the matching trainer's model checks."""
    from endossl.build import build_model
    from endossl.comatch_model import NativeResNetEmb
    monkeypatch.setenv("ENDOSSL_CNN_EMB", "1")
    for kw, L in ((dict(TYPE_SEMI="CoMatch", LOW_DIM=64), 64), (dict(IS_TRIPLET=True, IS_SSL=False), 256)):
        m = build_model(_cfg(**kw))
        assert type(m) is NativeResNetEmb and m.cfg.low_dim == L and m.cfg.num_classes == C
        assert getattr(m.cfg, "head") == "emb" and not hasattr(m, "engine")
        for attr in ("_run", "backward_from", "heads", "head_views", "dropout_keep", "bn_buffers"):
            assert callable(getattr(m, attr)), attr


def test_config_defaults_and_head_layout():
    from endossl.resnet import RESNET50, ResNetConfig, resnet_layout
    from endossl.vit import emb_head_layout
    plain = ResNetConfig(num_classes=C, **RESNET50)
    assert plain.head == "cls" and plain.low_dim == 64 and plain.dim == plain.num_features == 2048
    cfg = ResNetConfig(num_classes=C, head="emb", low_dim=16, **RESNET50)
    lay, base = resnet_layout(cfg), resnet_layout(plain)
    assert lay[:len(base) - 2] == base[:-2]  # the trunk entries first, without timm's fc
    rest = lay[len(base) - 2:]
    assert [(n, s) for n, s, k in rest if k == "p"] == emb_head_layout(cfg)
    assert [(n, k) for n, s, k in rest if k != "p"] == [("fc.3.running_mean", "rm"), ("fc.3.running_var", "rv"),
                                                       ("fc.3.num_batches_tracked", "nbt")]
    with pytest.raises(ValueError):
        ResNetConfig(head="embed")
    with pytest.raises(ValueError):
        ResNetConfig(head="emb", se=True, **RESNET50)


@pytest.fixture(scope="module")
def pair():
    from endossl.comatch_model import NativeResNetEmb
    from endossl.resnet import RESNET50, ResNetConfig
    torch.manual_seed(0)
    ref = ModelwEmb(C, low_dim=256)
    m = NativeResNetEmb(ResNetConfig(num_classes=C, head="emb", low_dim=256, **RESNET50), seed=1)
    return m, ref


def test_state_dict_is_the_reference_format(pair):
    m, ref = pair
    sd, rsd = m.state_dict(), ref.state_dict()
    keys = native_keys(ref)
    assert any(k.startswith("backbone.") for k in rsd) and len(keys) < len(rsd)
    assert list(sd) == keys
    for k in keys:
        assert tuple(sd[k].shape) == tuple(rsd[k].shape) and sd[k].dtype == rsd[k].dtype, k
    # the reference's order of groups: model.* (fc last, in timm's position), the fc.* aliases, head_emb.*
    first_fc = keys.index("fc.0.weight")
    assert all(k.startswith("model.") for k in keys[:first_fc]) and keys[first_fc - 1] == "model.fc.4.bias"
    assert keys[first_fc - 9] == "model.fc.0.weight" and keys[-1] == "head_emb.2.bias"
    for k in keys[first_fc:first_fc + 9]:  # aliases share storage (6 parameters, 3 buffers)
        assert sd[k].data_ptr() == sd["model." + k].data_ptr(), k
    n_ref = sum(p.numel() for p in ref.parameters())
    assert sum(p.numel() for p in m.parameters()) == n_ref == 26_331_718
    # head init: nn.Linear defaults, BatchNorm1d weight 1 / bias 0, fresh running statistics
    assert torch.all(sd["fc.3.weight"] == 1) and torch.all(sd["fc.3.bias"] == 0)
    assert torch.all(sd["fc.3.running_mean"] == 0) and torch.all(sd["fc.3.running_var"] == 1)
    assert sd["fc.3.num_batches_tracked"].dtype == torch.int64
    assert 0 < sd["fc.0.weight"].abs().max().item() <= 2048 ** -0.5
    assert 0 < sd["head_emb.2.bias"].abs().max().item() <= 768 ** -0.5


def test_state_dict_round_trip(pair):
    from endossl.comatch_model import NativeResNetEmb
    m, ref = pair
    rsd = ref.state_dict()
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for k, v in rsd.items():
            if k.startswith("model.") or k.startswith("head_emb."):  # every other key aliases a model.* tensor
                v.copy_(torch.randn(v.shape, generator=g)) if v.is_floating_point() else v.fill_(7)
    other = NativeResNetEmb(m.cfg, seed=5)
    other.load_state_dict(rsd)  # strict; backbone.* skipped
    back = other.state_dict()
    for k in native_keys(ref):
        assert torch.equal(back[k], rsd[k]), k
    again = NativeResNetEmb(m.cfg, seed=6)
    again.load_state_dict({k: v for k, v in back.items() if not k.startswith("model.fc.")})  # bare fc.* names alone
    bare = {k[len("model."):] if k.startswith("model.") else k: v for k, v in back.items()}
    last = NativeResNetEmb(m.cfg, seed=7)
    last.load_state_dict(bare)  # and the bare names throughout
    for k, v in back.items():
        assert torch.equal(again.state_dict()[k], v) and torch.equal(last.state_dict()[k], v), k
    ref2 = ModelwEmb(C, low_dim=256)
    res = ref2.load_state_dict(back, strict=False)  # all the restatement lacks is its own backbone.* listing
    assert not res.unexpected_keys and all(k.startswith("backbone.") for k in res.missing_keys)


def test_deepcopy_and_moves_carry_the_head_buffers(pair):
    import copy
    m, _ = pair
    m.get_buffer("fc.3.running_mean").fill_(0.25)
    m.get_buffer("fc.3.num_batches_tracked").fill_(3)
    try:
        c = copy.deepcopy(m)
        assert type(c) is type(m) and c.drop_seed == m.drop_seed
        assert torch.equal(c.bn_buffers()[0], m.bn_buffers()[0]) and int(c.bn_buffers()[2]) == 3
        assert c.flat.data_ptr() != m.flat.data_ptr() and c.bn_buffers()[0].data_ptr() != m.bn_buffers()[0].data_ptr()
        c.bn_buffers()[0].fill_(1.0)
        assert torch.all(m.bn_buffers()[0] == 0.25)
        d = c.to(torch.float32)  # _apply rebuilds the views over the layout's buffers
        assert torch.all(d.bn_buffers()[0] == 1.0) and len(list(d.named_buffers())) == len(list(m.named_buffers()))
        names = [k for k, _ in m.named_buffers()]
        assert names[-3:] == ["fc.3.running_mean", "fc.3.running_var", "fc.3.num_batches_tracked"]
    finally:
        m.get_buffer("fc.3.running_mean").zero_()
        m.get_buffer("fc.3.num_batches_tracked").zero_()


def test_pre_train_path_loads_the_trunk(tmp_path):
    from endossl.build import build_model
    torch.manual_seed(3)
    src = ResNet50(2)  # the 2-class abnormality checkpoint
    with torch.no_grad():
        for k, v in src.state_dict().items():
            if k.endswith("running_mean"):
                v.normal_()
            elif k.endswith("num_batches_tracked"):
                v.fill_(11)
    path = str(tmp_path / "sup_resnet50.pth")
    torch.save({"model_state_dict": src.state_dict(), "epoch": 3}, path)
    kw = dict(IS_TRIPLET=True, IS_SSL=False)
    m = build_model(_cfg(PRE_TRAIN_PATH=path, **kw), seed=4, cnn_emb=True)
    fresh = build_model(_cfg(**kw), seed=4, cnn_emb=True)
    sd, fsd, ssd = m.state_dict(), fresh.state_dict(), src.state_dict()
    for k, v in ssd.items():
        if not k.startswith("fc."):
            assert torch.equal(sd["model." + k], v), k
    assert not torch.equal(sd["model.conv1.weight"], fsd["model.conv1.weight"])
    for k in sd:  # the heads keep their seeded init
        if k.startswith(("fc.", "head_emb.", "model.fc.")):
            assert torch.equal(sd[k], fsd[k]), k
    lacking = {k: v for k, v in ssd.items() if k != "layer3.4.bn2.running_var"}
    torch.save({"model_state_dict": lacking}, path)
    with pytest.raises(KeyError, match="layer3.4.bn2.running_var"):
        build_model(_cfg(PRE_TRAIN_PATH=path, **kw), seed=4, cnn_emb=True)


class _DS:
    df = None


class _DL(list):
    dataset = _DS()


def _train_cfg(**model):
    from endossl.utils import AttrDict
    m = dict(NAME="resnet18", NUM_CLASSES=3, MARGIN="None", IS_TRIPLET=False, TYPE_SEMI="CoMatch", LOW_DIM=8)
    m.update(model)
    return AttrDict(DATA=AttrDict(BATCH_SIZE=2, MU=1, IMG_SIZE=64, TARGET_NAME="target"), MODEL=AttrDict(**m),
                    TRAIN=AttrDict(IS_SSL=True, IS_FREEZE=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3,
                                   EVAL_STEP=1, CLS_WEIGHT=False, THRES=0.5, LAMBDA_U=1.0, LAMBDA_C=1.0, EPOCHS=1,
                                   WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="const",
                                   FREQ_EVAL=1))


def test_data_parallel_runs_are_refused(monkeypatch):
    from endossl import dist
    from endossl.comatch import CoMatch
    from endossl.comatch_model import NativeResNetEmb
    from endossl.resnet import ResNetConfig
    from endossl.supervised import SupLearning
    m = NativeResNetEmb(ResNetConfig(num_classes=3, head="emb", low_dim=8), seed=0)
    co = CoMatch(m, device="cpu")
    co.get_dataloader((_DL([]), _DL([])), None)
    sup = SupLearning(m, device="cpu")
    sup.get_dataloader(_DL([]), None)
    monkeypatch.setattr(dist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="NativeResNetEmb"):
        co.get_config(_train_cfg())
    with pytest.raises(NotImplementedError, match="NativeResNetEmb"):
        sup.get_config(_train_cfg(IS_TRIPLET=True))
    monkeypatch.undo()
    co.get_config(_train_cfg())  # one process: accepted, and the EMA copy carries every buffer
    assert co.EMA_BUFFERS and co.cnn
    ema = dict(co.ema_model.ema.named_buffers())
    assert "fc.3.running_var" in ema and "layer4.1.bn2.running_mean" in ema
    assert [type(x).__name__ for x in co._trainable_when_frozen()] == ["Module", "Module"]
    sup.get_config(_train_cfg(IS_TRIPLET=True))
    assert sup.is_triplet and sup.EMA_BUFFERS


@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_dense_integer_cases_are_exact_in_fp32(shape):
    """Every partial sum of the integer cases stays below 2^24 (in units of 1/8) whatever the summation order, so
    any correct fp32 kernel, tiled and split however, gives the float64 result to the bit."""
    c = hc.dense_case(*shape)
    for with_keep in (False, True):
        assert hc.dense_magnitude(c, with_keep) < 2 ** 24
