"""Host side of the AdamW / SGD-Nesterov sweeps (no GPU compute): the class map the kernels read, the
torch.optim.AdamW / torch.optim.SGD state_dict interchange over the reference's two param groups
(code/optimizer.py:13-53), build_optimizer's routing, and the entry points' argument validation."""
import pytest
import torch

from endossl.optimizer import (GRANULE, NativeAdam, NativeAdamW, NativeSGD, build_optimizer, class_map,
                               weight_decay_groups)
from endossl.vit import NativeViT, ViTConfig


def _tiny_vit(seed=0, head="cls"):
    return NativeViT(ViTConfig(img_size=64, dim=128, depth=2, heads=2, num_classes=23, head=head), seed=seed)


def _tiny_conformer(seed=0):
    from endossl.conformer import ConformerConfig, NativeConformer
    return NativeConformer(ConformerConfig(img_size=64, embed_dim=128, depth=6, heads=2, num_classes=23), seed=seed)


def _tiny_resnet(seed=0):
    from endossl.resnet import NativeResNet, ResNetConfig
    return NativeResNet(ResNetConfig(layers=(1, 1, 1, 1), num_classes=23, img_size=64), seed=seed)


_MODELS = {"vit": (_tiny_vit, ("head",)), "conformer": (_tiny_conformer, ("conv_cls_head", "trans_cls_head")),
           "resnet": (_tiny_resnet, ("fc",))}


def _expected_map(model):
    """Element by element: the class of every float of the flat buffer (0 where no trained parameter lives)."""
    per_float = torch.zeros(model.numel, dtype=torch.uint8)
    params = dict(model.named_parameters())
    for c, names in enumerate(weight_decay_groups(model), 1):
        for name in names:
            o = model.offs[name]
            per_float[o:o + params[name].numel()] = c
    return per_float


@pytest.mark.parametrize("kind", sorted(_MODELS))
def test_class_map_carries_each_parameters_group(kind):
    make, _ = _MODELS[kind]
    m = make()
    cls = class_map(m)
    assert cls.dtype == torch.uint8 and cls.shape == (m.numel // GRANULE,)
    assert m.numel % GRANULE == 0 and all(o % GRANULE == 0 for o in m.offs.values())
    per_float = _expected_map(m).view(-1, GRANULE)
    # every granule holds one parameter's floats (then alignment padding): its class is that parameter's
    assert torch.equal(cls, per_float.max(dim=1).values)
    assert torch.equal(cls, per_float[:, 0])
    decay, no_decay = weight_decay_groups(m)
    params = dict(m.named_parameters())
    for c, names in ((1, decay), (2, no_decay)):
        for name in names:
            lo, hi = m.offs[name] // GRANULE, (m.offs[name] + params[name].numel() + GRANULE - 1) // GRANULE
            assert bool((cls[lo:hi] == c).all()), name
    # a granule no parameter reaches is padding: class 0
    covered = torch.zeros(m.numel // GRANULE, dtype=torch.bool)
    for name, p in params.items():
        covered[m.offs[name] // GRANULE:(m.offs[name] + p.numel() + GRANULE - 1) // GRANULE] = True
    assert bool((cls[~covered] == 0).all())
    assert int((cls == 1).sum()) > 0 and int((cls == 2).sum()) > 0


@pytest.mark.parametrize("kind", sorted(_MODELS))
def test_class_map_frozen_trunk_leaves_only_the_head(kind):
    make, heads = _MODELS[kind]
    m = make()
    for p in m.parameters():
        p.requires_grad = False
    for h in heads:  # IS_FREEZE (code/fixmatch.py:40-48, code/semiformer.py:50-56)
        getattr(m, h).requires_grad_(True)
    cls = class_map(m)
    params = dict(m.named_parameters())
    head = torch.zeros_like(cls, dtype=torch.bool)
    for name, p in params.items():
        if name.split(".")[0] in heads:
            lo, hi = m.offs[name] // GRANULE, (m.offs[name] + p.numel() + GRANULE - 1) // GRANULE
            head[lo:hi] = True
            assert bool((cls[lo:hi] == (1 if p.dim() > 1 else 2)).all()), name
    assert head.any() and bool((cls[~head] == 0).all()) and bool((cls[head] != 0).all())
    assert torch.equal(build_optimizer(m, "AdamW").cls, cls)  # rebuilt with the optimizer


def test_class_map_refuses_an_unaligned_layout():
    m = _tiny_vit()
    m.offs = dict(m.offs, **{"head.bias": m.offs["head.bias"] + 4})
    with pytest.raises(AssertionError):
        class_map(m)


def _reference(model, kind, lr=1e-3):
    """code/optimizer.py:13-53 as the reference builds AdamW / SGD over the same module."""
    skip = model.no_weight_decay()
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if len(p.shape) == 1 or name.endswith(".bias") or name in skip else decay).append(p)
    groups = [{"params": decay}, {"params": no_decay, "weight_decay": 0.}]
    if kind == "AdamW":
        return torch.optim.AdamW(groups, eps=1e-8, betas=(0.9, 0.999), lr=lr, weight_decay=0.05)
    return torch.optim.SGD(groups, momentum=0.9, nesterov=True, lr=lr, weight_decay=0.05)


_NATIVE = {"AdamW": (NativeAdamW, ("exp_avg", "exp_avg_sq")), "SGD": (NativeSGD, ("momentum_buffer",))}


@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_native_state_loads_into_torch_and_back(kind):
    torch.manual_seed(0)
    Native, bufs = _NATIVE[kind]
    m = _tiny_vit()
    opt = Native(m, lr=3e-4)
    assert opt.state_dict()["state"] == {}  # nothing before the first step, as torch
    for b in bufs:
        getattr(opt, b).copy_(torch.rand_like(getattr(opt, b)))
    opt.step_count = 7
    sd = opt.state_dict()
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.05, 0.0]

    ref = _reference(m, kind)
    assert [set(g) for g in sd["param_groups"]] == [set(g) for g in ref.state_dict()["param_groups"]]
    ref.load_state_dict(sd)  # raises on any layout mismatch
    by_name = dict(m.named_parameters())
    for name, p in by_name.items():
        st, o = ref.state[p], m.offs[name]
        assert set(st) == set(bufs) | ({"step"} if kind == "AdamW" else set())
        for b in bufs:
            assert torch.equal(st[b].flatten(), getattr(opt, b)[o:o + p.numel()]), (name, b)
        if kind == "AdamW":
            assert float(st["step"]) == 7
    assert ref.param_groups[0]["lr"] == 3e-4
    assert [g["weight_decay"] for g in ref.param_groups] == [0.05, 0.0]

    opt2 = Native(_tiny_vit(seed=1), lr=1e-3)
    opt2.load_state_dict(ref.state_dict())
    for b in bufs:
        for name, p in by_name.items():
            o = m.offs[name]
            assert torch.equal(getattr(opt2, b)[o:o + p.numel()], getattr(opt, b)[o:o + p.numel()]), (name, b)
    assert opt2.step_count == (7 if kind == "AdamW" else 1) and opt2.param_groups[1]["lr"] == 3e-4
    assert [g["weight_decay"] for g in opt2.param_groups] == [0.05, 0.0]


@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_torch_trained_state_resumes_natively(kind):
    """A torch optimizer that took two real CPU steps over the module, as the reference does."""
    torch.manual_seed(1)
    Native, bufs = _NATIVE[kind]
    m = _tiny_vit(head="emb")
    ref = _reference(m, kind)
    for _ in range(2):
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        ref.step()
    opt = Native(_tiny_vit(head="emb"))
    opt.load_state_dict(ref.state_dict())
    assert opt.step_count == (2 if kind == "AdamW" else 1)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.05, 0.0]
    flat = {b: torch.zeros(m.numel) for b in bufs}
    for name, p in m.named_parameters():
        o = m.offs[name]
        for b in bufs:
            flat[b][o:o + p.numel()] = ref.state[p][b].flatten()
    for b in bufs:
        assert torch.equal(getattr(opt, b), flat[b]), b
    # and what it saves again is what torch saved
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert sd["param_groups"] == rsd["param_groups"]
    assert sd["state"].keys() == rsd["state"].keys()
    for i, st in rsd["state"].items():
        for k, v in st.items():
            assert torch.equal(sd["state"][i][k], v), (i, k)


def test_sgd_state_without_buffers_loads_as_zeros():
    m = _tiny_vit()
    ref = _reference(m, "SGD")
    opt = NativeSGD(m)
    opt.momentum_buffer.fill_(3.0)
    opt.step_count = 1
    opt.load_state_dict(ref.state_dict())  # never stepped: no momentum_buffer anywhere
    assert opt.step_count == 0 and float(opt.momentum_buffer.abs().max()) == 0.0
    assert opt.state_dict()["state"] == {}


def test_groups_keep_their_own_lr_and_decay_from_a_checkpoint():
    m = _tiny_vit()
    ref = _reference(m, "AdamW")
    ref.param_groups[0]["lr"], ref.param_groups[1]["lr"] = 2e-4, 5e-4
    ref.param_groups[0]["weight_decay"] = 0.1
    opt = NativeAdamW(m)
    opt.load_state_dict(ref.state_dict())
    assert [g["lr"] for g in opt.param_groups] == [2e-4, 5e-4]
    assert [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0]
    assert all(g["decoupled_weight_decay"] is True for g in opt.param_groups)


def test_build_optimizer_routing():
    m = _tiny_vit()
    assert type(build_optimizer(m, "Adam")) is NativeAdam
    assert type(build_optimizer(m, "AdamW")) is NativeAdamW
    assert type(build_optimizer(m, "adamw", lr=2e-3)) is NativeAdamW
    sgd = build_optimizer(m, "SGD", lr=2e-3)
    assert type(sgd) is NativeSGD
    assert [g["weight_decay"] for g in sgd.param_groups] == [0.05, 0.0]
    assert all(g["momentum"] == 0.9 and g["nesterov"] is True and g["dampening"] == 0 and g["lr"] == 2e-3
               for g in sgd.param_groups)
    adamw = build_optimizer(m, "AdamW")
    assert [g["weight_decay"] for g in adamw.param_groups] == [0.05, 0.0]
    assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["decoupled_weight_decay"] is True
               for g in adamw.param_groups)
    assert [g["weight_decay"] for g in build_optimizer(m, "Adam").param_groups] == [0, 0.0]
    with pytest.raises(NotImplementedError):
        build_optimizer(m, "rmsprop")


@pytest.mark.parametrize("into,other", [("AdamW", "SGD"), ("SGD", "AdamW")])
def test_wrong_kind_of_state_is_a_value_error(into, other):
    m = _tiny_vit()
    src = _NATIVE[other][0](m)
    src.step_count = 1
    dst = _NATIVE[into][0](m)
    with pytest.raises(ValueError) as ei:
        dst.load_state_dict(src.state_dict())
    assert into in str(ei.value) and other in str(ei.value)
    with pytest.raises(ValueError):  # torch's own, too
        dst.load_state_dict(_reference(m, other).state_dict())


def test_adam_state_is_refused_by_adamw():
    m = _tiny_vit()
    adam = torch.optim.Adam([{"params": [p]} for p in list(m.parameters())[:2]], lr=1e-3)
    with pytest.raises(ValueError) as ei:
        NativeAdamW(m).load_state_dict(adam.state_dict())
    assert "Adam" in str(ei.value) and "AdamW" in str(ei.value)


def test_entries_validate_before_any_launch():
    """es_adamw_ema_step / es_sgd_ema_step refuse, before touching the GPU: n no multiple of 64
    (ES_BAD_SHAPE), a null class map or buffer (ES_BAD_ARG), a float buffer off 16 bytes (ES_BAD_ARG)."""
    from endossl import _lib
    lib = _lib.load()
    q = 0x7000000000  # never dereferenced on these paths

    def adamw(p=q, g=q, m=q, v=q, e=q, cls=q, n=128, omb2=1 - 0.999):
        return lib.es_adamw_ema_step(p, g, m, v, e, cls, n, 0.9, 0.999, 1 - 0.9, omb2, 1e-8, 1.0, -1e-3, -1e-3, 1.0,
                                     1.0, 0.999, 0.001, 1.0, None)

    def sgd(p=q, g=q, m=q, e=q, cls=q, n=128):
        return lib.es_sgd_ema_step(p, g, m, e, cls, n, 0.9, -1e-3, -1e-3, 0.05, 0.0, 1, 0.999, 0.001, 1.0, None)

    for rc in (adamw, sgd):
        assert rc(n=96) == -1 and rc(n=0) == -1 and rc(n=-64) == -1
        assert rc(cls=None) == -2 and rc(cls=q + 2) == -2  # the map is read as 32-bit words
        assert rc(p=q + 4) == -2
        assert rc(p=None) == -2 and rc(g=None) == -2 and rc(m=None) == -2
        assert rc(g=q + 8) == -2 and rc(m=q + 4) == -2 and rc(e=q + 4) == -2
    assert adamw(v=None) == -2 and adamw(v=q + 4) == -2
    assert adamw(omb2=0.1) == -2  # a complement that is not 1 - beta2
