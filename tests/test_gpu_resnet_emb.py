"""NativeResNetEmb (ModelwEmb over the native ResNet-50 trunk) on the MI355X against its plain-torch.nn restatement
(tests/resnet_emb_restatement.py), and one step of each trainer that takes it: the triplet step, CoMatch (also with
IS_FREEZE) and both EZBM stages.

Shapes: resnet50, C = 5, L = 8 (256 where build_model's triplet branch decides), images of 64^2 -- the last map is
2 x 2 x 2048.  No bar is new.  Trunk (tests/test_gpu_resnet50.py): outputs 1e-3 * scale; gradients 2e-3 |g| + 4 x the
fp32 restatement's own distance from fp64 + 1e-4 of the largest gradient.  Heads (tests/test_gpu_triplet.py):
1e-4 * scale; dl / dz rtol 1e-4, atol 1e-6; dfts and head gradients rtol 1e-4, atol 1e-5; losses rtol 1e-5.
EZBM stage 2: tests/test_gpu_ezbm.py's rtol 1e-4, atol 1e-6 against float64, losses 1e-5."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ezbm_restatement as er  # noqa: E402
import head_cases as hc  # noqa: E402
from oracle import ref  # noqa: E402
from oracle.conformer_ref import is_buffer  # noqa: E402
from resnet50_restatement import forward_contract  # noqa: E402
from resnet_emb_restatement import ModelwEmb  # noqa: E402

DEV = "cuda"
C, L, N = 5, 8, 4
F_ = 512  # D / 4
GRAD_KEYS = ("conv1.weight", "layer1.0.downsample.0.weight", "layer4.2.conv3.weight", "fc.0.weight", "fc.3.weight",
             "fc.4.weight", "head_emb.0.weight", "head_emb.2.weight")
BN_KEYS = ("bn1.running_mean", "layer1.0.downsample.1.running_var", "layer4.2.bn3.running_mean",
           "layer4.2.bn2.running_var", "fc.3.running_mean", "fc.3.running_var")


def bits(t):
    return t.contiguous().view(torch.int32)


def _rname(k):
    return k if k.startswith("head_emb.") else "model." + k


def _model(seed=2, conv="fp32", low_dim=L, buffers_seed=None):
    from endossl.comatch_model import NativeResNetEmb
    from endossl.resnet import RESNET50, ResNetConfig
    m = NativeResNetEmb(ResNetConfig(num_classes=C, head="emb", low_dim=low_dim, **RESNET50), seed=seed)
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


def _restatement(state, dtype, low_dim=L):
    r = ModelwEmb(C, low_dim=low_dim).to(dtype)
    res = r.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("backbone.") for k in res.missing_keys)
    return r


@pytest.fixture(scope="module")
def case():
    """The fp32-conv model, its input, and the restatement's train-mode forward + backward in fp32 and fp64."""
    m, state = _model()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 3, 64, 64, generator=g)
    keep = (torch.rand(N, F_, generator=g) >= 0.2).to(torch.uint8)
    gs = (torch.randn(N, C, generator=g), torch.randn(N, L, generator=g), torch.randn(N, 2048, generator=g) * 0.01)
    refs = {}
    for dt in (torch.float32, torch.float64):
        r = _restatement(state, dt).train()
        lg, fts, z = r(x.to(dt), keep)
        ((lg * gs[0].to(dt)).sum() + (z * gs[1].to(dt)).sum() + (fts * gs[2].to(dt)).sum()).backward()
        refs[dt] = ((lg.detach(), fts.detach(), z.detach()), {k: p.grad for k, p in r.named_parameters()},
                    dict(r.named_buffers()))
    return m, state, x, keep, gs, refs


def _check_grads(m, refs, what):
    g32, g64 = refs[torch.float32][1], refs[torch.float64][1]
    gmax = max(v.double().norm().item() for v in g32.values())
    bad = []
    for k in GRAD_KEYS:
        a, b = g32[_rname(k)], g64[_rname(k)]
        gh = m.gview(k).cpu().view(a.shape).double()
        nrm = a.double().norm().item()
        e, env = (gh - b).norm().item(), 4 * (a.double() - b).norm().item()
        print(f"{what} grad {k}: |device - fp64| = {e:.3e}, 4 |fp32 - fp64| = {env:.3e}, |g| = {nrm:.3e}")
        if e > 2e-3 * nrm + env + 1e-4 * gmax:
            bad.append((k, e, env, nrm))
    assert not bad, bad


def test_train_parity_autograd_and_step_paths(case):
    """model(x) + autograd, then _run + backward_from on the same input and keep mask: each within the bars of the
    restatement, and the two with equal bits in the outputs and in the whole flat gradient."""
    m, state, x, keep, gs, refs = case
    xd, kd = x.to(DEV), keep.to(DEV)
    gd = [t.to(DEV) for t in gs]
    m.train()
    m.flat_grad.zero_()
    out = m(xd, keep=kd)
    assert all(o.requires_grad for o in out)
    for name, o, r in zip(("logits", "fts", "z"), out, refs[torch.float32][0]):
        sc = max(1.0, r.abs().max().item())
        e = (o.detach().cpu().double() - r.double()).abs().max().item()
        print(f"{name}: |device - fp32| = {e:.3e}, scale {sc:.3f}")
        assert e <= 1e-3 * sc, (name, e, sc)
    bufs = refs[torch.float32][2]
    for k in BN_KEYS:
        want = bufs["model." + k]
        err = (m.get_buffer(k).cpu() - want).abs().max().item()
        assert err <= 1e-3 * max(1.0, want.abs().max().item()), (k, err)
    assert int(m.get_buffer("fc.3.num_batches_tracked")) == 1 and int(m.get_buffer("bn1.num_batches_tracked")) == 1
    torch.autograd.backward(list(out), [gd[0], gd[2], gd[1]])  # out = (logits, fts, z), gs = (g1, g2 for z, g3 for fts)
    torch.cuda.synchronize()
    _check_grads(m, refs, "autograd")
    a_out = [o.detach().clone() for o in out]
    a_grad = m.flat_grad.clone()
    o2 = m._run([xd[:1], xd[1:]], train=True, keep=kd)  # a list: ONE trunk pass over the concatenation
    b_out = [o.clone() for o in o2]
    g = m.backward_from(gd[0], gd[1], dfts_extra=gd[2])
    torch.cuda.synchronize()
    assert g.data_ptr() == m.flat_grad.data_ptr()
    _check_grads(m, refs, "step")
    for a, b in zip(a_out, b_out):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(a_grad), bits(m.flat_grad)) and bool(torch.isfinite(a_grad).all())
    assert int(m.get_buffer("bn1.num_batches_tracked")) == 2


def test_heads_wide_and_narrow_on_the_trunks_own_features(case):
    """The heads with `wide_heads` off and on, on the features `_run` produced for the test model (all-positive pooled
    maps): logits and z of each within the head bars of the float64 heads on those same features.  The gradients of
    the two families are printed against each other, not asserted: with 4 rows through BatchNorm1d torch's own fp32 on
    the CPU is 5x the gradient bar from float64 (fc.0.weight, measured on the CPU for this model); the trainer tests
    below hold the wide family's gradients to the fp32 oracle."""
    m, state, x, keep, gs, _ = case
    xd, kd = x.to(DEV), keep.to(DEV)
    p64 = {k: state[k].double() for k in state if k.startswith(("fc.", "head_emb.")) and not is_buffer(k)}
    grads = {}
    try:
        for wide in (False, True):
            m.wide_heads = wide
            assert m.heads().wide is wide
            logits, fts, z = (t.clone() for t in m._run(xd, train=True, keep=kd))
            m.backward_from(gs[0].to(DEV), gs[1].to(DEV), trunk=False)
            torch.cuda.synchronize()
            grads[wide] = m.flat_grad[m.offs["fc.0.weight"]:].cpu().double()
            bufs = {k: state[k].clone().double() if state[k].is_floating_point() else state[k].clone()
                    for k in ref.BN_BUFFERS}
            with torch.no_grad():
                lg64, z64 = ref.emb_heads(p64, bufs, fts.cpu().double(), keep, train=True)
            sc = max(1.0, lg64.abs().max().item())
            e = (logits.cpu().double() - lg64).abs().max().item()
            print(f"wide={wide}: logits |device - fp64| = {e:.3e}, scale {sc:.3f}; "
                  f"z {(z.cpu().double() - z64).abs().max().item():.3e}")
            assert bool((fts >= 0).all()) and e <= 1e-4 * sc, (wide, e, sc)
            torch.testing.assert_close(z.cpu(), z64.float(), rtol=1e-4, atol=1e-5)
    finally:
        m.wide_heads = True
    d = (grads[True] - grads[False]).abs().max().item()
    print(f"head gradients, wide against narrow: max |difference| = {d:.3e}, max |g| = {grads[False].abs().max().item():.3e}")
    assert bool(torch.isfinite(grads[True]).all()) and grads[True].abs().max().item() > 0


def test_eval_forward_fp32_and_bf16_envelope():
    m, state = _model(seed=7, buffers_seed=8)
    x = torch.randn(N, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    r = _restatement(state, torch.float32).eval()
    with torch.no_grad():
        r32 = [t.double() for t in r(x)]
        out = m.eval()(x.to(DEV))
        again = m(x.to(DEV))
    for name, o, want in zip(("logits", "fts", "z"), out, r32):
        assert not o.requires_grad
        sc = max(1.0, want.abs().max().item())
        assert (o.cpu().double() - want).abs().max().item() <= 1e-3 * sc, name
    for a, b in zip(out, again):  # clones, not views of the head buffers
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    for k, v in m.state_dict().items():  # eval mode leaves the buffers alone
        if is_buffer(k):
            assert torch.equal(v.cpu(), state[k]), k
    # the default bf16 convs and maps: within twice the bf16-contract emulation's own distance from fp32 + 1e-3 scale
    m16, _ = _model(seed=7, conv="bf16", buffers_seed=8)
    assert m16.map_bf16 and m16.conv_1x1
    own = {k[len("model."):]: v.clone() for k, v in state.items() if k.startswith("model.") and ".fc." not in k}
    p = {k: v for k, v in own.items() if not is_buffer(k)}
    p["fc.weight"] = torch.eye(2048)  # forward_contract ends in its fc: the identity hands the features out
    b = {k: v for k, v in own.items() if is_buffer(k)}
    with torch.no_grad():
        f16 = forward_contract(p, b, x, train=False, bf16=True, maps=m16.map_bf16)
        r16 = [f16.double()] + [t.double() for t in r.heads(f16)]
        o16 = m16.eval()(x.to(DEV))
    for name, o, want, emu in zip(("logits", "fts", "z"), o16, r32, (r16[1], r16[0], r16[2])):
        sc = max(1.0, want.abs().max().item())
        e32, env = (o.cpu().double() - want).abs().max().item(), (emu - want).abs().max().item()
        print(f"bf16 {name}: |device - fp32| = {e32:.3e}, |contract - fp32| = {env:.3e}, scale {sc:.3f}")
        assert e32 <= 2 * env + 1e-3 * sc, (name, e32, env, sc)


# ------------------------------------------------------------------------------------------------ trainers
class _DS:
    df = None

    def __init__(self, cls_num=None):
        self.cls_num = cls_num

    def get_cls_num_list(self):
        return self.cls_num

    def __len__(self):
        return 16


class _DL(list):
    def __init__(self, items=(), cls_num=None):
        super().__init__(items)
        self.dataset = _DS(cls_num)


def _cfg(mode, bs=2, freeze=False, thres=0.5, save_cp="."):
    from endossl.utils import AttrDict
    co = mode == "comatch"
    return AttrDict(
        DATA=AttrDict(BATCH_SIZE=bs, MU=1, IMG_SIZE=64, TARGET_NAME="target"),
        MODEL=AttrDict(NAME="resnet50", NUM_CLASSES=C, MARGIN="None", IS_TRIPLET=not co,
                       TYPE_SEMI="CoMatch" if co else "FixMatch", LOW_DIM=L, PRE_TRAIN_PATH="None"),
        TRAIN=AttrDict(IS_SSL=co, IS_FREEZE=freeze, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, EVAL_STEP=1,
                       CLS_WEIGHT=False, THRES=thres, T=1.0, LAMBDA_U=2.0, LAMBDA_C=2.0, EPOCHS=1, WARMUP_EPOCHS=0,
                       DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="const", FREQ_EVAL=1,
                       EXPANSION="balance", SAVE_CP=save_cp))


def _head_oracle(sd0, fts, keep):
    """ModelwEmb's heads (oracle/ref.py) in fp32 on the device's own features, as leaves for autograd."""
    hp = {k: sd0[k].clone().float().requires_grad_(True) for k in sd0
          if k.startswith(("fc.", "head_emb.")) and not is_buffer(k)}
    bufs = {k: sd0[k].clone() for k in ref.BN_BUFFERS}
    leaf = fts.detach().cpu().float().requires_grad_(True)
    lg, z = ref.emb_heads(hp, bufs, leaf, keep, train=True)
    return hp, leaf, lg, z


def _check_heads(o, lg_h, z_h):
    lg = o["logits"].detach().cpu()
    sc = max(1.0, lg_h.abs().max().item())
    e = (lg.double() - lg_h.double()).abs().max().item()
    print(f"heads: |device - fp32 oracle| = {e:.3e}, scale {sc:.3f}")
    assert e <= 1e-4 * sc, (e, sc)
    torch.testing.assert_close(o["z"].detach().cpu(), z_h.detach(), rtol=1e-4, atol=1e-5)


def _check_head_grads(m, n, hp, leaf):
    torch.testing.assert_close(m.heads().bufs(n)["dfts"].cpu(), leaf.grad, rtol=1e-4, atol=1e-5)
    for k, v in hp.items():
        torch.testing.assert_close(m.gview(k).cpu().view(v.shape), v.grad, rtol=1e-4, atol=1e-5,
                                   msg=lambda s, k=k: f"{k}: {s}")


def _check_trunk_grads(m, sd0, low_dim, imgs, dfts):
    """The trunk's gradients given the device's own dL/dfts, against the restatement in fp32 and fp64."""
    gr = {}
    for dt in (torch.float32, torch.float64):
        r = _restatement(sd0, dt, low_dim).train()
        fts = r.model.features(imgs.to(dt))
        fts.backward(dfts.to(dt))
        gr[dt] = {k: p.grad for k, p in r.named_parameters() if p.grad is not None}
    gmax = max(v.double().norm().item() for v in gr[torch.float32].values())
    bad = []
    for k in GRAD_KEYS[:3]:
        a, b = gr[torch.float32]["model." + k], gr[torch.float64]["model." + k]
        gh, nrm = m.gview(k).cpu().view(a.shape).double(), a.double().norm().item()
        e, env = (gh - b).norm().item(), 4 * (a.double() - b).norm().item()
        print(f"trunk grad {k}: |device - fp64| = {e:.3e}, 4 |fp32 - fp64| = {env:.3e}, |g| = {nrm:.3e}")
        if e > 2e-3 * nrm + env + 1e-4 * gmax:
            bad.append((k, e, env, nrm))
    assert not bad, bad


def _check_update(sd0, m, tr, frozen_trunk=False):
    """Adam's first step and the EMA blend of parameters and BatchNorm buffers (ModelEMA started as a copy)."""
    sd1, esd = m.state_dict(), tr.ema_model.ema.state_dict()
    still = []
    for k, v0 in sd0.items():
        new, e = sd1[k].cpu(), esd[k].cpu()
        if k.endswith("num_batches_tracked"):
            assert int(new) == 1 and int(e) == 0, k  # EMA of an int buffer truncates
            continue
        if not is_buffer(k):
            assert (new - v0).abs().max().item() <= 1e-3 + 1e-6, k  # |delta| <= lr
        if torch.equal(new, v0):
            still.append(k)
        blend = 0.999 * v0 + (1.0 - 0.999) * new
        torch.testing.assert_close(e, blend, rtol=1e-5, atol=1e-7, msg=lambda s, k=k: f"ema {k}: {s}")
    if frozen_trunk:
        head = lambda k: k.startswith(("fc.", "head_emb.", "model.fc."))  # noqa: E731
        assert all(not head(k) for k in still), still
        assert all(k in still for k in sd0 if not head(k) and not is_buffer(k))  # the trunk's parameters: unchanged
        assert not any(is_buffer(k) for k in still), still  # every BatchNorm buffer moved (training-mode trunk)
    else:
        assert not still, still


def triplet64(z, bs, alpha, grad_scale):
    """TripletLoss (alpha, mean) in float64 on the given rows, as tests/test_gpu_triplet.py::triplet_ref."""
    zd = z.double().clone().requires_grad_(True)
    a, p, n = zd[:bs], zd[bs:2 * bs], zd[2 * bs:]
    d_p, d_n = torch.norm(a - p, dim=1), torch.norm(a - n, dim=1)
    h = d_p - d_n + alpha
    losses = torch.max(h, torch.zeros(1, dtype=torch.float64))
    (losses.sum() * grad_scale).backward()
    return {"loss": losses.mean().item(), "d_ap": d_p.mean().item(), "d_an": d_n.mean().item(), "h": h.detach(),
            "dz": zd.grad}


def test_triplet_step_stage_by_stage():
    from endossl.build import build_model
    from endossl.comatch_model import NativeResNetEmb
    from endossl.supervised import SupLearning
    bs, Lt, lam_c = 2, 256, 2.0
    cfg = _cfg("triplet", bs=bs)
    m = build_model(cfg, seed=4, cnn_emb=True).set_conv_precision("fp32")
    assert type(m) is NativeResNetEmb and m.cfg.low_dim == Lt
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(21)
    imgs3 = tuple(torch.randn(bs, 3, 64, 64, generator=g) for _ in range(3))
    ys = tuple(torch.randint(0, C, (bs,), generator=g) for _ in range(3))
    keep = (torch.rand(3 * bs, F_, generator=g) >= 0.2).to(torch.uint8)
    tr = SupLearning(m, opt_func="Adam", lr=1e-3, device=DEV)
    tr.get_dataloader(_DL([(imgs3, ys)]), None)
    tr.get_config(cfg)
    assert tr.is_triplet and tr.EMA_BUFFERS
    o = tr.step((imgs3, ys), drop_keep=keep)
    torch.cuda.synchronize()
    assert set(o) == {"loss", "ce", "triplet", "d_ap", "d_an", "active", "logits", "fts", "z"}
    imgs = torch.cat(imgs3)
    with torch.no_grad():
        f32 = _restatement(sd0, torch.float32, Lt).train().model.features(imgs).double()
    fe, fsc = (o["fts"].cpu().double() - f32).abs().max().item(), max(1.0, f32.abs().max().item())
    print(f"fts: |device - fp32| = {fe:.3e}, scale {fsc:.3f}")
    assert tuple(o["fts"].shape) == (3 * bs, 2048) and fe <= 1e-3 * fsc
    hp, leaf, lg_h, z_h = _head_oracle(sd0, o["fts"], keep)
    _check_heads(o, lg_h, z_h)
    lg_leaf = o["logits"].detach().cpu().double().requires_grad_(True)
    ce = ref.poly_ce(lg_leaf[:bs], ys[0], None)
    tz = triplet64(o["z"].detach().cpu(), bs, 0.7, lam_c / bs)
    assert tz["h"].abs().min().item() > 1e-4
    want = {"ce": ce.item(), "triplet": tz["loss"], "d_ap": tz["d_ap"], "d_an": tz["d_an"],
            "loss": ce.item() + lam_c * tz["loss"]}
    for k, v in want.items():
        print(k, o[k].item(), v)
        assert abs(o[k].item() - v) <= 1e-5 * abs(v), (k, o[k].item(), v)  # losses: rtol 1e-5
    ce.backward()
    W = tr._triplet_workspace(bs, C, Lt)
    assert torch.all(W["dl"][bs:] == 0)
    torch.testing.assert_close(W["dl"].cpu(), lg_leaf.grad.float(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(W["dz"].cpu(), tz["dz"].float(), rtol=1e-4, atol=1e-6)
    torch.autograd.backward([lg_h, z_h], [lg_leaf.grad.float(), tz["dz"].float()])
    _check_head_grads(m, 3 * bs, hp, leaf)
    _check_trunk_grads(m, sd0, Lt, imgs, m.heads().bufs(3 * bs)["dfts"].cpu())
    _check_update(sd0, m, tr)


def _comatch_stage(thres, lam_u, lam_c, Q):
    """oracle/ref.py's CoMatchRef.losses on given logits / z: the stage reference, no trunk attached."""
    s = ref.CoMatchRef.__new__(ref.CoMatchRef)
    s.L, s.C, s.cw, s.thres, s.lambda_u, s.lambda_c = L, C, None, thres, lam_u, lam_c
    s.alpha, s.temperature, s.contrast_th, s.gamma = 0.9, 0.2, 0.8, 2
    s.queue_size, s.queue_ptr, s.prob_list = Q, 0, []
    s.queue_feats, s.queue_probs = torch.zeros(Q, L, dtype=torch.float64), torch.zeros(Q, C, dtype=torch.float64)
    return s


COMATCH_SEED = 32  # the weak rows' float64 scores differ by 0.017 and their top-2 gaps are 0.03: decided, one per side


def _comatch_inputs():
    g = torch.Generator().manual_seed(COMATCH_SEED)
    x, uw, u0, u1 = (torch.randn(2, 3, 64, 64, generator=g) for _ in range(4))
    y = torch.randint(0, C, (2,), generator=g)
    keep = (torch.rand(8, F_, generator=g) >= 0.2).to(torch.uint8)
    return x, y, uw, u0, u1, keep


def _comatch_run(freeze, thres):
    from endossl.build import build_model
    from endossl.comatch import CoMatch
    cfg = _cfg("comatch", freeze=freeze, thres=thres)
    m = build_model(cfg, seed=6, cnn_emb=True).set_conv_precision("fp32")
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, y, uw, u0, u1, keep = _comatch_inputs()
    tr = CoMatch(m, opt_func="Adam", lr=1e-3, device=DEV)
    tr.get_dataloader((_DL([(x, y)]), _DL([((uw, u0, u1), None)])), None)
    tr.get_config(cfg)
    tr.set_queue_size(4)  # B + mu B = 4 rows: the gated bank write fires
    o = tr.step(((x, y), ((uw, u0, u1), None)), drop_keep=keep)
    torch.cuda.synchronize()
    return m, tr, sd0, o, (x, y, uw, u0, u1, keep)


def _threshold_between_the_weak_rows(m_sd0):
    """THRES for the CoMatch step: midway between the two weak rows' smoothed scores in the float64 restatement of
    the whole model (no device value enters), so one row falls on each side by construction."""
    x, y, uw, u0, u1, keep = _comatch_inputs()
    r = _restatement(m_sd0, torch.float64).train()
    with torch.no_grad():
        lg, _, z = r(torch.cat([x, uw, u0, u1]).double(), keep)
    s = _comatch_stage(0.5, 2.0, 2.0, 4)
    rs = s.losses(lg, z, y, 2, 2)
    sc = rs["probs"].max(1).values
    assert (sc[0] - sc[1]).abs().item() > 100 * hc.DECIDE, sc
    top2 = rs["probs"].topk(2, -1).values  # and every weak row's pseudo-label is decided, in float64 alone
    assert bool(((top2[:, 0] - top2[:, 1]) > 100 * hc.DECIDE).all()), top2
    return float(sc.mean())


def test_comatch_step_stage_by_stage():
    from endossl.build import build_model
    probe = build_model(_cfg("comatch"), seed=6, cnn_emb=True)
    thres = _threshold_between_the_weak_rows({k: v.detach().clone() for k, v in probe.state_dict().items()})
    m, tr, sd0, o, (x, y, uw, u0, u1, keep) = _comatch_run(False, thres)
    bt = btu = 2
    imgs = torch.cat([x, uw, u0, u1])
    assert int(m.get_buffer("bn1.num_batches_tracked")) == 1  # ONE trunk pass over the 8 images
    hp, leaf, lg_h, z_h = _head_oracle(sd0, o["fts"], keep)
    _check_heads(o, lg_h, z_h)
    # pseudo-labels, mask and losses in float64 on the device's logits and z
    lg_leaf = o["logits"].detach().cpu().double().requires_grad_(True)
    z_leaf = o["z"].detach().cpu().double().requires_grad_(True)
    stage = _comatch_stage(thres, 2.0, 2.0, 4)
    rs = stage.losses(lg_leaf, z_leaf, y, bt, btu)
    p = rs["probs"]
    top2 = p.topk(2, -1).values
    scores = p.max(-1).values
    print("weak-row scores", scores.tolist(), "threshold", thres, "mask", o["mask"].tolist())
    assert bool(((top2[:, 0] - top2[:, 1]) > hc.DECIDE).all()) and bool(((scores - thres).abs() > hc.DECIDE).all())
    assert bool((scores > thres).any()) and bool((scores < thres).any())
    assert torch.equal(o["pseudo_label"].cpu().long(), rs["pseudo_label"])
    assert torch.equal(o["mask"].cpu().double(), rs["mask"].double())
    for k in ("lx", "lu", "lc", "loss"):
        print(k, o[k].item(), rs[k])
        assert abs(o[k].item() - rs[k]) <= 1e-5 * abs(rs[k]), (k, o[k].item(), rs[k])  # losses: rtol 1e-5
    torch.testing.assert_close(o["probs"].cpu(), p.float(), rtol=1e-5, atol=1e-6)
    assert tr.queue_ptr == 0 and stage.queue_ptr == 0  # 4 rows written into a 4-row bank: the pointer wrapped
    torch.testing.assert_close(tr.queue_feats.cpu(), stage.queue_feats.float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(tr.queue_probs.cpu(), stage.queue_probs.float(), rtol=1e-5, atol=1e-6)
    assert tr.queue_feats.abs().max().item() > 0
    rs["loss_t"].backward()
    W = tr._workspace(bt, btu, C, L)
    torch.testing.assert_close(W["dl"].cpu(), lg_leaf.grad.float(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(W["dz"].cpu(), z_leaf.grad.float(), rtol=1e-4, atol=1e-6)
    torch.autograd.backward([lg_h, z_h], [lg_leaf.grad.float(), z_leaf.grad.float()])
    _check_head_grads(m, 8, hp, leaf)
    _check_trunk_grads(m, sd0, L, imgs, m.heads().bufs(8)["dfts"].cpu())
    _check_update(sd0, m, tr)


def test_comatch_is_freeze_trains_the_heads_alone():
    m, tr, sd0, o, _ = _comatch_run(True, 0.2)
    assert tr.frozen and m.frozen_trunk
    first_head = m.offs["fc.0.weight"]
    assert torch.count_nonzero(m.flat_grad[:first_head]) == 0  # the trunk's gradients: exactly zero
    assert m.flat_grad[first_head:].abs().max().item() > 0 and bool(torch.isfinite(o["loss"]))
    _check_update(sd0, m, tr, frozen_trunk=True)


def test_ezbm_both_stages_checkpoint_and_evaluate(tmp_path):
    from endossl.build import build_model
    from endossl.ezbm import EZBM
    bs = 2
    cfg = _cfg("triplet", bs=bs, save_cp=str(tmp_path))
    cfg.TRAIN.LAMBDA_C = 4
    m = build_model(cfg, seed=8, cnn_emb=True)
    g = torch.Generator().manual_seed(5)
    batches = [(tuple(torch.randn(bs, 3, 64, 64, generator=g) for _ in range(3)),
                tuple((torch.arange(bs) + 2 * j + r) % C for r in range(3))) for j in range(3)]
    ez = EZBM(m, opt_func="Adam", lr=1e-3, device=DEV)
    ez.get_dataloader(_DL(batches, cls_num=[9, 7, 5, 3, 2]), _DL([(batches[0][0][0], batches[0][1][0])]))
    ez.get_config(cfg)
    for batch in batches:  # stage 1: the anchors' fts appended to the bank bit for bit
        out = ez.step_stage_1(batch)
        want = out["fts"][:bs].clone()
        bx, by = ez.bank()
        assert torch.equal(bits(bx[-bs:]), bits(want)) and torch.equal(by[-bs:].cpu(), batch[1][0])
    bx, by = ez.bank()
    assert tuple(bx.shape) == (3 * bs, 2048) and sorted(set(by.tolist())) == list(range(C))
    # stage 2 on the stage-1 bank itself (the all-positive pooled features the trainer will see), every bank row
    # once: the device against float64 within 4x the distance of torch's fp32 on the CPU from float64 on the same
    # operands + 1e-6, per tensor in the max-norm (the envelope of tests/test_gpu_dense_wide.py)
    ez.setup_stage_2()
    n1 = 3 * bs
    idx1, dual1 = torch.arange(n1, dtype=torch.int32), torch.tensor([3, 4, 5, 0, 1, 2], dtype=torch.int32)
    keep1 = (torch.rand(2 * n1, F_, generator=g) >= 0.2).to(torch.uint8)
    sd_a = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    o1 = ez.step_stage_2(idx=idx1, dual=dual1, drop_keep=keep1)
    torch.cuda.synchronize()
    X1 = er.mix(bx.cpu(), idx1, dual1, o1["lam"].cpu())
    args1 = ({k: sd_a["fc." + k] for k in er.FC_KEYS}, {k: sd_a["fc." + k] for k in er.BN_KEYS}, X1, keep1,
             o1["t"].cpu(), o1["td"].cpu(), 4.0)
    r64, r32 = er.head_step(*args1), er.head_step(*args1, dtype=torch.float32)
    got = {"logits": o1["logits"].cpu()}
    got.update({k: m.gview("fc." + k).cpu().view(r64["grads"][k].shape) for k in er.FC_KEYS})
    want = lambda r: {"logits": r["logits"], **r["grads"]}  # noqa: E731
    bad = []
    for k, v in got.items():
        e = (v.double() - want(r64)[k]).abs().max().item()
        env = (want(r32)[k].double() - want(r64)[k]).abs().max().item()
        print(f"stage-1 bank {k}: |device - fp64| = {e:.3e}, |cpu fp32 - fp64| = {env:.3e}")
        if not e <= 4 * env + 1e-6:
            bad.append((k, e, env))
    assert not bad, bad
    # stage 2: one step with replayed rows and Dropout mask against the float64 restatement of the head.  The bar is
    # the D = 32 fixture's; at D = 2048 BatchNorm1d over a few rows of all-positive pooled features cancels most of
    # every pre-activation, and torch's own fp32 on the CPU then sits at up to 3.8x that bar from float64 (measured
    # on the CPU for this head).  So the step runs on a set bank of 48 zero-mean rows with n = 32 rows per BatchNorm
    # group, where the CPU's fp32 is within 0.2x of the bar for the logits and every gradient.
    n, rows = 32, 48
    mem, mem_y = torch.randn(rows, 2048, generator=g), torch.arange(rows) % C
    ez.set_bank(mem.to(DEV), mem_y.to(DEV))
    bx, by = ez.bank()
    idx, dual = torch.randperm(rows, generator=g)[:n].int(), torch.randperm(rows, generator=g)[:n].int()
    keep = (torch.rand(2 * n, F_, generator=g) >= 0.2).to(torch.uint8)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    flat0 = m.flat.clone()
    o = ez.step_stage_2(idx=idx, dual=dual, drop_keep=keep)
    torch.cuda.synchronize()
    mem, mem_y = bx.cpu(), by.cpu()
    assert torch.equal(o["t"].cpu(), mem_y[idx.long()]) and torch.equal(o["td"].cpu(), mem_y[dual.long()])
    X = er.mix(mem, idx, dual, o["lam"].cpu())
    r = er.head_step({k: sd0["fc." + k] for k in er.FC_KEYS}, {k: sd0["fc." + k] for k in er.BN_KEYS}, X, keep,
                     o["t"].cpu(), o["td"].cpu(), 4.0)
    bar = dict(rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(o["logits"].cpu(), r["logits"].float(), **bar)
    for k in ("loss", "l_o", "l_s"):
        print(k, o[k].item(), r[k].item())
        assert abs(o[k].item() - r[k].item()) <= 1e-5 * abs(r[k].item()), k
    for k in er.FC_KEYS:
        torch.testing.assert_close(m.gview("fc." + k).cpu().view(r["grads"][k].shape), r["grads"][k].float(),
                                   msg=lambda s, k=k: f"{k}: {s}", **bar)
    sd1 = m.state_dict()
    torch.testing.assert_close(sd1["fc.3.running_mean"].cpu(), r["running_mean"].float(), **bar)
    torch.testing.assert_close(sd1["fc.3.running_var"].cpu(), r["running_var"].float(), **bar)
    assert int(sd1["fc.3.num_batches_tracked"]) == int(sd0["fc.3.num_batches_tracked"]) + 2
    # only fc's slice of the flat buffer moves
    lo, hi = m.offs["fc.0.weight"], m.offs["head_emb.0.weight"]
    assert torch.equal(bits(m.flat[:lo]), bits(flat0[:lo])) and torch.equal(bits(m.flat[hi:]), bits(flat0[hi:]))
    assert all(not torch.equal(sd1["fc." + k].cpu(), sd0["fc." + k]) for k in er.FC_KEYS)
    # evaluate_one (the EMA model, eval mode), a checkpoint round trip, deepcopy independence of the EMA model
    loss, metric = ez.evaluate_one()
    assert np.isfinite(loss.avg) and "macro/f1" in metric
    ez.epoch = 0
    path = ez.save_checkpoint(str(tmp_path))
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert list(ck["model_state_dict"]) == list(m.state_dict())
    other = build_model(cfg, seed=9, cnn_emb=True)
    ez2 = EZBM(other, opt_func="Adam", lr=1e-3, device=DEV)
    ez2.get_dataloader(_DL(batches, cls_num=[9, 7, 5, 3, 2]), None)
    ez2.get_config(cfg)
    ez2.load_checkpoint(path, is_train=True)
    assert ez2.stage == 2
    for k, v in m.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    for k, v in ez.ema_model.ema.state_dict().items():
        assert torch.equal(ez2.ema_model.ema.state_dict()[k], v), k
    ema = ez.ema_model.ema
    assert ema.flat.data_ptr() != m.flat.data_ptr() and not ema.training
    assert ema.get_buffer("fc.3.running_var").data_ptr() != m.get_buffer("fc.3.running_var").data_ptr()
    twin = copy.deepcopy(m)
    twin.flat.add_(1.0)
    twin.get_buffer("layer1.0.bn1.running_mean").add_(1.0)
    assert torch.equal(bits(m.flat), bits(other.flat))
    assert torch.equal(m.get_buffer("layer1.0.bn1.running_mean"), other.get_buffer("layer1.0.bn1.running_mean"))
