"""Supervised triplet mode on the MI355X: es_triplet_fwd_bwd and es_softmax_predict against float64 torch
(autograd for the gradient), the triplet SupLearning.step stage by stage against the oracle evaluated on the
HIP path's own inputs to each stage (the pattern of test_comatch_trainer_vs_reference_train_one), and
get_config / evaluate_one / test_one / inference.

Bars (this project's for fp32 loss kernels, tests/test_gpu_comatch.py): loss values rtol 1e-5, gradients rtol
1e-4 / atol 1e-6, counts and decided predictions exact.  A prediction is decided when the float64 softmax's
top-2 gap and |conf - thres| both exceed 1e-5.  Trainer: trunk features within 1e-3 * scale + a quarter of
the bf16 envelope of the bf16-contract oracle; heads 1e-4 * scale; losses 1e-4 * max(1, |v|); dl / dz rtol
1e-4, atol 1e-6; dfts and head parameter gradients rtol 1e-4, atol 1e-5.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402
from oracle import ref  # noqa: E402

DEV = "cuda"
ALPHA = 0.7
NAN = float("nan")


def S():
    return _lib.stream()


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _lib.load()


def _unit(t):
    return t / t.norm(dim=1, keepdim=True)


# ------------------------------------------------------------------------------------- es_triplet_fwd_bwd
def make_triplets(bs, L, seed, first_kind=0):
    """Unit rows [3 bs, L] (CPU fp32).  Triplet i is of kind (i + first_kind) % 3:
    0  positive at unit(a + 0.3 unit(noise)), random negative      -> inactive
    1  random positive and negative                                -> active
    2  random positive, negative at unit(a + 0.1 unit(noise))      -> active
    and triplet 1 has its positive EQUAL to its anchor with a near negative: active, d_p = 0."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: _unit(torch.randn(bs, L, generator=g))  # noqa: E731
    a, p, n = r(), r(), r()
    near_p, near_n = _unit(a + 0.3 * r()), _unit(a + 0.1 * r())
    kind = (torch.arange(bs) + first_kind) % 3
    p[kind == 0] = near_p[kind == 0]
    n[kind == 2] = near_n[kind == 2]
    if bs > 1:
        p[1], n[1] = a[1], near_n[1]
    return torch.cat([a, p, n]).contiguous()


def triplet_ref(z, bs, alpha, grad_scale):
    """TripletLoss (code/loss.py:170-190) in float64 on the given rows; the gradient of grad_scale * sum_i h_i^+."""
    zd = z.double().clone().requires_grad_(True)
    a, p, n = zd[:bs], zd[bs:2 * bs], zd[2 * bs:]
    d_p, d_n = torch.norm(a - p, dim=1), torch.norm(a - n, dim=1)
    h = d_p - d_n + alpha
    losses = torch.max(h, torch.zeros(1, dtype=torch.float64))
    (losses.sum() * grad_scale).backward()
    return {"loss": losses.mean().item(), "d_ap": d_p.mean().item(), "d_an": d_n.mean().item(), "h": h.detach(),
            "active": (h.detach() > 0), "dz": zd.grad}


TRIPLET_CASES = [(1, 64, 64, 0), (1, 64, 64, 1), (5, 3, 7, 0), (64, 64, 64, 0), (67, 256, 256, 0)]


@pytest.mark.parametrize("bs,L,ld,first_kind", TRIPLET_CASES)
def test_triplet_fwd_bwd_vs_float64_autograd(bs, L, ld, first_kind):
    scale = 2.0 / bs
    z = make_triplets(bs, L, seed=bs + L, first_kind=first_kind)
    r = triplet_ref(z, bs, ALPHA, scale)
    assert r["h"].abs().min().item() > 1e-4, "an undecidable triplet in the inputs"
    assert torch.isfinite(r["dz"]).all()
    act = r["active"]
    if bs == 1:
        assert bool(act[0]) == (first_kind == 1)
    else:
        assert act.any() and (~act).any() and bool(act[1])
    zp = torch.full((3 * bs, ld), NAN)
    zp[:, :L] = z
    zp = zp.to(DEV)
    dz = torch.full((3 * bs, ld), NAN, device=DEV)
    out = torch.full((4,), NAN, device=DEV)
    call("es_triplet_fwd_bwd", ptr(zp), ld, bs, L, ALPHA, scale, ptr(dz), ld, ptr(out), S())
    dz2, out2 = torch.full((3 * bs, ld), NAN, device=DEV), torch.full((4,), NAN, device=DEV)
    call("es_triplet_fwd_bwd", ptr(zp), ld, bs, L, ALPHA, scale, ptr(dz2), ld, ptr(out2), S())
    o, g = out.cpu(), dz.cpu()
    print({"out": o.tolist(), "ref": [r["loss"], r["d_ap"], r["d_an"], int(act.sum())],
           "dz_err": (g[:, :L].double() - r["dz"]).abs().max().item()})
    np.testing.assert_allclose(o[:3].numpy(), [r["loss"], r["d_ap"], r["d_an"]], rtol=1e-5)
    assert o[3].item() == (np.float32(int(act.sum())) / np.float32(bs)).item()
    torch.testing.assert_close(g[:, :L], r["dz"].float(), rtol=1e-4, atol=1e-6)
    assert torch.isnan(g[:, L:]).all()  # the padding columns are not written
    rows = torch.cat([~act, ~act, ~act])
    assert torch.all(g[rows][:, :L] == 0)  # inactive triplets: exact zeros over the NaN fill
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(dz[:, :L].contiguous().view(torch.int32), dz2[:, :L].contiguous().view(torch.int32))


def test_triplet_zero_distance_gradients():
    """p == a exactly: d_p = 0, the direction u_p is 0 (torch.norm's backward), the rest finite."""
    bs, L = 5, 64
    z = make_triplets(bs, L, seed=3).to(DEV)
    assert torch.equal(z[1], z[bs + 1])
    dz, out = torch.full((3 * bs, L), NAN, device=DEV), torch.zeros(4, device=DEV)
    call("es_triplet_fwd_bwd", ptr(z), L, bs, L, ALPHA, 1.0, ptr(dz), L, ptr(out), S())
    assert torch.isfinite(dz).all()
    assert torch.all(dz[bs + 1] == 0)  # -u_p
    assert torch.equal(dz[1], -dz[2 * bs + 1]) and dz[1].abs().max().item() > 0  # u_p - u_n = -u_n


def test_triplet_status_codes():
    lib = _lib.load()
    z, dz, out = torch.zeros(6, 8, device=DEV), torch.zeros(6, 8, device=DEV), torch.zeros(4, device=DEV)
    f = lambda **kw: lib.es_triplet_fwd_bwd(*[{**dict(z=ptr(z), ldz=8, bs=2, L=8, alpha=ALPHA, gs=1.0,  # noqa: E731
                                                    dz=ptr(dz), lddz=8, out=ptr(out), s=S()), **kw}[k]
                                              for k in ("z", "ldz", "bs", "L", "alpha", "gs", "dz", "lddz", "out", "s")])
    assert f() == 0
    for bad in (dict(bs=0), dict(bs=-1), dict(L=0), dict(L=2049), dict(ldz=7), dict(lddz=7)):
        assert f(**bad) == -1, bad  # ES_BAD_SHAPE
    for bad in (dict(z=None), dict(dz=None), dict(out=None)):
        assert f(**bad) == -2, bad  # ES_BAD_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- es_softmax_predict
THRES = 0.95


def make_logits(n, C, seed):
    """Rows of randn scaled by 1 .. 12 (max softmax probability from ~0.2 to ~1: both sides of 0.95)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, C, generator=g) * (1 + 11 * torch.rand(n, 1, generator=g))).contiguous()


def predict_ref(logits, thres):
    p = torch.softmax(logits.double(), -1)
    top2 = p.topk(2, -1).values
    conf, pred = p.max(-1)
    ok = ((top2[:, 0] - top2[:, 1]) > 1e-5) & ((conf - thres).abs() > 1e-5)
    return pred, conf, torch.where(conf > thres, pred, torch.zeros_like(pred)), ok


def _predict(lg, ldl, n, C, thres):
    pad = torch.full((n, ldl), NAN)
    pad[:, :C] = lg
    pad = pad.to(DEV)
    pred = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    label = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    conf = torch.full((n,), NAN, device=DEV)
    call("es_softmax_predict", ptr(pad), ldl, n, C, thres, ptr(pred), ptr(conf), ptr(label), S())
    return pred.cpu().long(), conf.cpu(), label.cpu().long()


@pytest.mark.parametrize("ldl", [23, 32])
@pytest.mark.parametrize("n", [1, 300, 5000])
def test_softmax_predict(n, ldl):
    C = 23
    lg = make_logits(max(n, 8), C, seed=n)
    lg[-1, 4] = lg[-1, 19] = lg[-1].max() + 1.0  # the two largest equal: the first index wins
    # n = 1: every row is its own one-row launch, so both label outcomes and the tie are still covered
    chunks = [lg] if n > 1 else [lg[i:i + 1] for i in range(lg.shape[0])]
    got = [_predict(c, ldl, c.shape[0], C, THRES) for c in chunks]
    pred, conf, label = (torch.cat([g[i] for g in got]) for i in range(3))
    rp, rc, rl, ok = predict_ref(lg, THRES)
    assert pred[-1].item() == 4 and not bool(ok[-1])
    ok_rest = ok[:-1]
    assert ok_rest.float().mean().item() >= 0.99
    decided = rl[:-1][ok_rest]
    hi = (rc[:-1][ok_rest] > THRES)
    assert hi.any() and (~hi).any(), "conf does not straddle the threshold"
    print({"n": n, "decidable": ok_rest.float().mean().item(), "above": int(hi.sum()),
           "conf_relerr": ((conf.double() - rc).abs() / rc).max().item()})
    assert torch.equal(pred[:-1][ok_rest], rp[:-1][ok_rest])
    assert torch.equal(label[:-1][ok_rest], decided)
    np.testing.assert_allclose(conf.numpy(), rc.numpy(), rtol=1e-5)
    assert label[-1].item() in (0, 4)


def test_softmax_predict_nullable_outputs_and_status():
    lib = _lib.load()
    n, C = 37, 23
    lg = make_logits(n, C, seed=5).to(DEV)
    full = _predict(lg.cpu(), C, n, C, THRES)
    pred = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    label = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    conf = torch.full((n,), NAN, device=DEV)
    assert lib.es_softmax_predict(ptr(lg), C, n, C, THRES, ptr(pred), None, None, S()) == 0
    assert lib.es_softmax_predict(ptr(lg), C, n, C, THRES, None, ptr(conf), None, S()) == 0
    assert lib.es_softmax_predict(ptr(lg), C, n, C, THRES, None, None, ptr(label), S()) == 0
    assert torch.equal(pred.cpu().long(), full[0]) and torch.equal(label.cpu().long(), full[2])
    assert torch.equal(conf.cpu(), full[1])
    assert lib.es_softmax_predict(ptr(lg), C, n, C, THRES, None, None, None, S()) == -2
    assert lib.es_softmax_predict(None, C, n, C, THRES, ptr(pred), None, None, S()) == -2
    assert lib.es_softmax_predict(ptr(lg), C, 0, C, THRES, ptr(pred), None, None, S()) == -1
    assert lib.es_softmax_predict(ptr(lg), 65, n, 65, THRES, ptr(pred), None, None, S()) == -1  # C > MAXC
    assert lib.es_softmax_predict(ptr(lg), C - 1, n, C, THRES, ptr(pred), None, None, S()) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- trainer
class _DL:
    def __init__(self, items, df=None):
        self.items = items

        class _DS:
            pass

        self.dataset = _DS()
        self.dataset.df = df

    def __iter__(self):
        return iter(self.items)

    def __len__(self):
        return len(self.items)


def _cfg(triplet=True, cls_weight=True, margin="None", thres=0.95, bs=4, sch="const"):
    from endossl.utils import AttrDict
    return AttrDict(
        DATA=AttrDict(BATCH_SIZE=bs, IMG_SIZE=64, TARGET_NAME="target"),
        MODEL=AttrDict(NAME="vit_tiny_test", NUM_CLASSES=23, MARGIN=margin, IS_TRIPLET=triplet, LOW_DIM=16,
                       PRE_TRAIN_PATH="None"),
        TRAIN=AttrDict(IS_SSL=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, CLS_WEIGHT=cls_weight, THRES=thres,
                       LAMBDA_C=2.0, EPOCHS=1, WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8,
                       SCH_NAME=sch, FREQ_EVAL=1))


# every class present, uneven counts: sklearn-"balanced" weights from 0.5 to 2
_DF = {"target": [c for c in range(23) for _ in range(1 + c % 4)]}


def test_triplet_trainer_step_stage_by_stage():
    """SupLearning.step in triplet mode (code/supervised.py:84-108), step 0: every stage after the trunk against
    the oracle evaluated on the HIP path's OWN inputs to that stage, fp32 against fp32 / float64; the trunk
    features against the bf16-contract emulation.  Then the update: parameters moved, EMA = the blend, BN count."""
    from endossl.build import build_model
    from endossl.comatch_model import NativeViTEmb
    from endossl.supervised import SupLearning
    from endossl.utils import balanced_class_weights
    bs, C, L, lam_c = 4, 23, 256, 2.0
    cfg = _cfg()
    m = build_model(cfg, seed=4)
    assert isinstance(m, NativeViTEmb) and m.cfg.low_dim == L
    rcfg = ref.Cfg(img_size=64, patch=16, dim=128, depth=2, heads=2, num_classes=C)
    names = [n for n, _ in ref.emb_param_shapes(rcfg, L)]
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert [k for k in sd0 if k not in ref.BN_BUFFERS] == names
    params = {k: sd0[k].float() for k in names}
    bufs = {k: sd0[k].clone() for k in ref.BN_BUFFERS}
    g = torch.Generator().manual_seed(21)
    a, p, n = (torch.randn(bs, 3, 64, 64, generator=g) for _ in range(3))
    ys = tuple(torch.randint(0, C, (bs,), generator=g) for _ in range(3))
    keep = (torch.rand(3 * bs, 32, generator=g) >= 0.2).to(torch.uint8)
    batch = ((a, p, n), ys)

    tr = SupLearning(m, opt_func="Adam", lr=1e-3, device=DEV)
    tr.get_dataloader(_DL([batch], df=_DF), None)
    tr.get_config(cfg)
    cw = torch.tensor(balanced_class_weights(_DF["target"]))
    assert torch.equal(tr.class_weights.cpu(), cw) and cw.min() < 0.7 and cw.max() > 1.5
    o = tr.step(batch, drop_keep=keep)
    torch.cuda.synchronize()
    assert set(o) == {"loss", "ce", "triplet", "d_ap", "d_an", "active", "logits", "fts", "z"}
    rec = {}

    # trunk: CLS features vs the bf16-contract emulation
    imgs = torch.cat([a, p, n])
    f16 = ref.vit_features(params, imgs, rcfg, bf16=True).double()
    f32_ = ref.vit_features(params, imgs, rcfg, bf16=False).double()
    f_hip = o["fts"].detach().cpu().double()
    fsc, fenv = max(1.0, f16.abs().max().item()), (f16 - f32_).abs().max().item()
    rec["fts_vs_bf16_contract"], rec["fts_bf16_envelope"] = (f_hip - f16).abs().max().item(), fenv
    print(rec)
    assert rec["fts_vs_bf16_contract"] <= 1e-3 * fsc + 0.25 * fenv, rec

    # heads on the HIP features (fp32 vs fp32)
    hp = {k: params[k].clone().requires_grad_(True) for k in names if k.startswith(("fc.", "head_emb."))}
    fts_leaf = o["fts"].detach().cpu().float().requires_grad_(True)
    lg_h, z_h = ref.emb_heads(hp, {k: v.clone() for k, v in bufs.items()}, fts_leaf, keep, train=True)
    lg = o["logits"].detach().cpu()
    sc = max(1.0, lg_h.abs().max().item())
    rec["heads_vs_oracle"] = (lg.double() - lg_h.double()).abs().max().item()
    print(rec)
    assert tuple(lg.shape) == (3 * bs, C) and tuple(o["z"].shape) == (3 * bs, L)
    assert rec["heads_vs_oracle"] <= 1e-4 * sc, rec
    torch.testing.assert_close(o["z"].detach().cpu(), z_h.detach(), rtol=1e-4, atol=1e-5)

    # the losses in float64 on the HIP logits and z
    lg_leaf = lg.double().requires_grad_(True)
    ce = ref.poly_ce(lg_leaf[:bs], ys[0], cw.double())
    tz = triplet_ref(o["z"].detach().cpu(), bs, ALPHA, lam_c / bs)
    assert tz["h"].abs().min().item() > 1e-4
    want = {"ce": ce.item(), "triplet": tz["loss"], "d_ap": tz["d_ap"], "d_an": tz["d_an"],
            "loss": ce.item() + lam_c * tz["loss"]}
    for k, v in want.items():
        rec[k] = [o[k].item(), v]
    print(rec)
    for k, v in want.items():
        assert abs(o[k].item() - v) <= 1e-4 * max(1.0, abs(v)), (k, o[k].item(), v)
    assert o["active"].item() == (np.float32(int(tz["active"].sum())) / np.float32(bs)).item()

    # d(loss)/d(logits, z)
    ce.backward()
    W = tr._triplet_workspace(bs, C, L)
    dl, dz = W["dl"].cpu(), W["dz"].cpu()
    assert torch.all(dl[bs:] == 0)
    torch.testing.assert_close(dl, lg_leaf.grad.float(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(dz, tz["dz"].float(), rtol=1e-4, atol=1e-6)

    # the heads backward on the HIP features, fed the oracle's dl / dz
    torch.autograd.backward([lg_h, z_h], [lg_leaf.grad.float(), tz["dz"].float()])
    dfts = m.heads().bufs(3 * bs)["dfts"].cpu()
    torch.testing.assert_close(dfts, fts_leaf.grad, rtol=1e-4, atol=1e-5)
    # (flat_grad was consumed by the optimizer but not cleared: backward_from zeroes it at the next step)
    eng = m.engine()
    for k, v in hp.items():
        torch.testing.assert_close(eng.view(m.flat_grad, k).cpu().view(v.shape), v.grad, rtol=1e-4, atol=1e-5,
                                   msg=lambda s, k=k: f"{k}: {s}")

    # the update
    sd1, esd = m.state_dict(), tr.ema_model.ema.state_dict()
    moved = 0
    for k in names:
        new = sd1[k].cpu()
        moved += int((new != sd0[k]).any())
        assert (new - sd0[k]).abs().max().item() <= 1e-3 + 1e-6, k  # Adam's first step: |delta| <= lr
        blend = 0.999 * sd0[k] + (1.0 - 0.999) * new  # ModelEMA started as a copy of the initial model
        torch.testing.assert_close(esd[k].cpu(), blend, rtol=1e-5, atol=1e-7, msg=lambda s, k=k: f"ema {k}: {s}")
    assert moved == len(names), f"only {moved} of {len(names)} parameter tensors moved"
    assert int(sd1["fc.3.num_batches_tracked"].item()) == 1
    assert int(esd["fc.3.num_batches_tracked"].item()) == 0  # EMA of an int buffer truncates
    assert not torch.equal(sd1["fc.3.running_mean"].cpu(), sd0["fc.3.running_mean"])


def test_triplet_train_one_collects_distances():
    """train_one: one AverageMeter entry and one (d_ap, d_an) pair per step, gathered at the epoch's end."""
    from endossl.build import build_model
    from endossl.supervised import SupLearning
    bs = 2
    cfg = _cfg(cls_weight=False, bs=bs, sch="cosine")  # train_one drives a scheduler
    m = build_model(cfg, seed=1)
    g = torch.Generator().manual_seed(2)
    batches = [(tuple(torch.randn(bs, 3, 64, 64, generator=g) for _ in range(3)),
                tuple(torch.randint(0, 23, (bs,), generator=g) for _ in range(3))) for _ in range(2)]
    tr = SupLearning(m, opt_func="Adam", lr=1e-3, device=DEV)
    tr.get_dataloader(_DL(batches), None)
    tr.get_config(cfg)
    meter = tr.train_one(0)
    d = tr.triplet_dist
    assert len(d["d_ap"]) == len(d["d_an"]) == 2 and all(isinstance(v, float) for v in d["d_ap"] + d["d_an"])
    assert all(0.0 < v <= 2.0 for v in d["d_ap"] + d["d_an"])  # distances of unit vectors
    assert np.isfinite(meter.avg) and meter.count == 2 * bs


def test_get_config_errors():
    from endossl.supervised import SupLearning
    from endossl.vit import NativeViT, ViTConfig
    m = NativeViT(ViTConfig(img_size=64, dim=128, depth=2, heads=2, num_classes=23), seed=0)
    tr = SupLearning(m, device=DEV)
    tr.get_dataloader(_DL([]), None)
    with pytest.raises(ValueError, match="build_model.*IS_TRIPLET|IS_TRIPLET.*build_model"):
        tr.get_config(_cfg(triplet=True, cls_weight=False))
    with pytest.raises(NotImplementedError):
        tr.get_config(_cfg(triplet=True, cls_weight=False, margin="arcface"))
    with pytest.raises(NotImplementedError):
        tr.get_config(_cfg(triplet=False, cls_weight=False, margin="arcface"))
    with pytest.raises(NotImplementedError):
        tr.get_dataloader(_DL([]), None, mixup_fn=lambda x, y: (x, y))


def _eval_case(emb):
    """A SupLearning over a model whose class head is scaled up (spread-out probabilities), and eval loaders of
    3 batches, the last one smaller."""
    from endossl.build import build_model
    from endossl.supervised import SupLearning
    cfg = _cfg(triplet=emb, cls_weight=False, bs=5)
    m = build_model(cfg, seed=6)
    sd = m.state_dict()
    key = "fc.4.weight" if emb else "head.weight"
    g = torch.Generator().manual_seed(13)
    sd[key] = torch.randn(sd[key].shape, generator=g) * (2.0 if emb else 0.6)
    m.load_state_dict(sd)
    sizes = (5, 5, 3)
    xs = [torch.randn(k, 3, 64, 64, generator=g) for k in sizes]
    ys = [torch.randint(0, 23, (k,), generator=g) for k in sizes]
    idx = [torch.arange(k) * 7 + 100 * (j + 1) for j, k in enumerate(sizes)]
    tr = SupLearning(m, opt_func="Adam", lr=1e-3, device=DEV)
    tr.get_dataloader(_DL([]), _DL(list(zip(xs, ys))))
    tr.get_config(cfg)
    return tr, xs, ys, idx


@pytest.mark.parametrize("emb", [True, False], ids=["emb_head", "plain_logits"])
def test_evaluate_test_one_inference(emb):
    """evaluate_one / test_one / inference against float64 torch on the eval model's own logits."""
    tr, xs, ys, idx = _eval_case(emb)
    ema = tr.ema_model.ema
    ema.eval()
    with torch.no_grad():
        outs = [ema(x.to(DEV)) for x in xs]
    assert isinstance(outs[0], tuple) == emb
    lgs = [(o[0] if emb else o).detach().cpu().double() for o in outs]
    lg, y = torch.cat(lgs), torch.cat(ys)
    p = torch.softmax(lg, -1)
    conf = p.max(-1).values
    srt = conf.sort().values
    thres = float((srt[len(srt) // 2 - 1] + srt[len(srt) // 2]) / 2)  # between the two middle confidences
    tr.config.TRAIN.THRES = thres
    rp, rc, rl, ok = predict_ref(lg, thres)
    print({"conf": conf.tolist(), "thres": thres, "decidable": ok.float().mean().item()})
    assert ok.float().mean().item() >= 0.99
    assert (rc > thres).any() and (rc < thres).any()

    loss, metric = tr.evaluate_one()
    want = float(np.mean([F.cross_entropy(l, t).item() for l, t in zip(lgs, ys)]))  # AverageMeter over the batches
    assert abs(loss.avg - want) <= 1e-5 * max(1.0, abs(want)), (loss.avg, want)
    assert abs(metric["micro/f1"] - (rp == y).double().mean().item()) <= 1e-12

    wrong = tr.test_one()
    assert wrong.dtype == torch.bool and wrong.device.type == "cpu" and tuple(wrong.shape) == (13,)
    assert torch.equal(wrong[ok], (rp != y)[ok])

    got = tr.inference(_DL(list(zip(xs, idx))))
    keys = torch.cat(idx).tolist()
    assert list(got.keys()) == keys and all(isinstance(v, int) for v in got.values())
    labels = torch.tensor([got[k] for k in keys])
    assert torch.equal(labels[ok], rl[ok])
    assert (labels[ok][rc[ok] < thres] == 0).all()  # below the threshold: class 0
