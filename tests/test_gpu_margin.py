"""Angular-margin supervised mode on the MI355X: es_margin_softmax_fwd_bwd against the reference-generated
float64 fixtures (tests/golden/margin_*.npz) and against the float64 restatement that test_margin_cpu.py pins to
them (tests/margin_restatement.py); loss.AngularPenaltySMLoss through autograd; consistency_loss's margin
branch; the margin SupLearning.step stage by stage against oracle/resnet_ref.py's ResNet-18 (bias-free fc) plus
the restatement; evaluate_one / inference / checkpoints on the margin model; get_config's errors.

Bars (this project's for fp32 loss kernels, tests/test_gpu_triplet.py:6-10): loss values rtol 1e-5, gradients
rtol 1e-4 / atol 1e-6, for every kind -- the reference's own fp32 run sits at 0.33 of the gradient bar at the
worst (acloss dW; test_margin_cpu.py measures it, DESIGN.md records it and the device's figures), so no kind
needs the wider 4x-the-reference's-spread bar.  Trainer: the bars of test_gpu_resnet.py (features 1e-3 of scale,
loss 1e-4 max(1, |v|), trunk gradients 2e-3 |g| + 4x the fp32 oracle's distance from fp64 + 1e-4 max |g|,
parameters within 2 lr, EMA within (1 - decay) 2 lr, BatchNorm buffers 1e-3 of scale); dfts and the fc.weight
gradient, on the device's own features, rtol 1e-4 / atol 1e-5 (test_gpu_triplet.py's for head gradients).
"""
import pytest
import torch

import margin_restatement as mr

pytestmark = pytest.mark.gpu

from endossl import _lib  # noqa: E402
from endossl._lib import ptr  # noqa: E402
from endossl.loss import MARGIN_KINDS  # noqa: E402
from oracle import ref  # noqa: E402
from oracle import resnet_ref as rr  # noqa: E402
from oracle.conformer_ref import is_buffer  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BAD_ARG = -2


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _lib.load()


def launch(x, W, y, kind, s, m, eps=1e-7, b=None, w=None, mask=None, ldx=None, lddx=None, want_rows=True,
           want_db=None, grad_scale=None, kind_id=None, n=None, F=None, C=None, null=(), fill=NAN):
    """One es_margin_softmax_fwd_bwd call on CPU inputs; every output buffer pre-filled with `fill`.  Returns the
    status and the outputs on the CPU (dx with its padding columns)."""
    n0, F0 = x.shape
    C0 = W.shape[0]
    ldx, lddx = ldx or F0, lddx or F0
    xp = torch.full((n0, ldx), NAN)
    xp[:, :F0] = x
    d = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    xd, Wd, bd, yd, wd, md = d(xp), d(W.float()), d(b), d(y), d(w), d(mask)
    dx = torch.full((n0, lddx), fill, device=DEV)
    dW = torch.full((C0, F0), fill, device=DEV)
    want_db = (b is not None) if want_db is None else want_db
    db = torch.full((C0,), fill, device=DEV) if want_db else None
    out = torch.full((1,), fill, device=DEV)
    rows = torch.full((n0,), fill, device=DEV) if want_rows else None
    nws = _lib.load().es_margin_softmax_workspace(n0, min(C0, 64))
    ws = torch.full((max(nws, 1),), fill, device=DEV)
    a = {"x": xd, "W": Wd, "targets": yd, "dx": dx, "dW": dW, "out": out, "workspace": ws}
    p = {k: (None if k in null else ptr(v)) for k, v in a.items()}
    rc = _lib.load().es_margin_softmax_fwd_bwd(
        p["x"], ldx, p["W"], ptr(bd), p["targets"], ptr(wd), ptr(md), n0 if n is None else n, F0 if F is None else F,
        C0 if C is None else C, MARGIN_KINDS[kind] if kind_id is None else kind_id, s, m, eps,
        1.0 / n0 if grad_scale is None else grad_scale, p["dx"], lddx, p["dW"], ptr(db), p["out"], ptr(rows), p["workspace"],
        _lib.stream())
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu()  # noqa: E731
    return rc, {"out": c(out), "dx": c(dx), "dW": c(dW), "db": c(db), "rows": c(rows)}


def bar_units(d, r, rtol=1e-4, atol=1e-6):
    r = r.double()
    return ((d.double() - r).abs() / (atol + rtol * r.abs())).max().item()


def logit_bound(W, s, m, b=None, w=None):
    """An upper bound of every |s z_ij| and |num_i|, times the largest class weight (it scales a row's loss):
    |z| <= max |W_c| (+ |b|), |num| <= s (|t| + m)."""
    v = s * (W.double().norm(dim=1).max().item() + m + (0.0 if b is None else b.abs().max().item()))
    return v * (1.0 if w is None else max(1.0, w.max().item()))


def check(o, loss, dx, dW, F, db=None, rows=None, tag="", check_loss=True, bound=None):
    """The kernel's outputs against float64 values at the project's bars; the measured errors are printed.
    check_loss=False: gradients only (a lone saturated row's loss, ~1e-14, is below what lse - num resolves).
    Per-row losses (no bar of the project's covers them): a row's loss is lse - num, a difference of two fp32
    numbers of size up to `bound` (logit_bound), so beside rtol 1e-5 it gets 4 ulp of that size, 4 * 2^-23 * bound,
    as its absolute term -- a saturated row's ~1e-5 loss is below one ulp of its operands."""
    gdx = o["dx"][:, :F]
    fig = {"loss_rel": abs(o["out"].item() - float(loss)) / abs(float(loss)), "dx_bar": bar_units(gdx, dx),
           "dW_bar": bar_units(o["dW"], dW)}
    if db is not None:
        fig["db_bar"] = bar_units(o["db"], db)
    print(tag, {k: f"{v:.3g}" for k, v in fig.items()})
    assert torch.isfinite(o["out"]).all() and torch.isfinite(gdx).all() and torch.isfinite(o["dW"]).all()
    assert torch.isnan(o["dx"][:, F:]).all()  # the padding columns are not written
    if check_loss:
        torch.testing.assert_close(o["out"][0].double(), torch.as_tensor(float(loss), dtype=torch.float64), rtol=1e-5,
                                   atol=0)
    torch.testing.assert_close(gdx, dx.float(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(o["dW"], dW.float(), rtol=1e-4, atol=1e-6)
    if db is not None:
        torch.testing.assert_close(o["db"], db.float(), rtol=1e-4, atol=1e-6)
    if rows is not None and o["rows"] is not None:
        torch.testing.assert_close(o["rows"], rows.float(), rtol=1e-5, atol=4 * 2.0 ** -23 * bound)
    return fig


# ------------------------------------------------------------------------- kernel against the fixtures
@pytest.mark.parametrize("variant", mr.VARIANTS)
@pytest.mark.parametrize("kind", mr.KINDS)
def test_kernel_vs_reference_fixture(kind, variant):
    fx = mr.load_fixture(kind, variant)
    rc, o = launch(fx["x"], fx["W"], fx["y"], kind, fx["s"], fx["m"], fx["eps"], w=fx["w"], mask=fx["mask"])
    assert rc == 0
    check(o, fx["loss"], fx["dx"], fx["dW"], 64, tag=f"{kind}/{variant}")


@pytest.mark.parametrize("kind", mr.KINDS)
def test_clamped_rows(kind):
    """Rows with |t| > 1: for every kind but cosface the clamp passes no gradient, so such a row's target term
    contributes exactly zero to dW[y_i] (and to db[y_i]) -- seen with a mask that keeps that row alone, where
    dW[y_i] holds nothing but the target term -- and the whole fixture still matches the reference."""
    fx = mr.load_fixture(kind, "clamped")
    rc, o = launch(fx["x"], fx["W"], fx["y"], kind, fx["s"], fx["m"], fx["eps"])
    assert rc == 0
    check(o, fx["loss"], fx["dx"], fx["dW"], 64, tag=f"{kind}/clamped")
    b = torch.linspace(-0.05, 0.05, 23)
    for r in fx["clamped"].tolist():
        yi = int(fx["y"][r])
        mask = torch.zeros(24)
        mask[r] = 1.0
        loss, dx, dW, db, _ = mr.loss_and_grads(fx["x"], fx["W"], fx["y"], kind, fx["s"], fx["m"], fx["eps"], b=b,
                                                mask=mask)
        rc, o = launch(fx["x"], fx["W"], fx["y"], kind, fx["s"], fx["m"], fx["eps"], b=b, mask=mask)
        assert rc == 0
        others = [c for c in range(23) if c != yi]
        assert o["dW"][others].abs().max().item() > 0 and dW[others].abs().max().item() > 0
        if kind == "cosface":  # no clamp: the target term is there
            assert o["dW"][yi].abs().max().item() > 0 and dW[yi].abs().max().item() > 0 and o["db"][yi].item() != 0
        else:
            assert torch.all(dW[yi] == 0) and float(db[yi]) == 0  # the restatement (autograd through the clamp)
            assert torch.all(o["dW"][yi] == 0) and o["db"][yi].item() == 0  # exact zeros over the NaN fill
        rows = [i for i in range(24) if i != r]
        assert torch.all(o["dx"][rows] == 0)  # masked rows: exact zeros
        check(o, loss, dx, dW, 64, db=db, tag=f"{kind}/clamped row {r}", check_loss=False)


# ------------------------------------------------------------------------- shapes where it can go wrong
def seeded_case(n, F, C, seed, wnorm=0.9, bias=False):
    """Seeded inputs whose rows of W have norm <= wnorm (|t| <= wnorm: away from acos' endpoints), targets
    hitting class 0 and class C - 1, features of uneven length.  Row 0 is barely aligned with its class, so its
    loss is O(s) and the mean is never a saturated ~1e-7 that lse - num cannot resolve in fp32."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(C, F, generator=g)
    W = W / W.norm(dim=1, keepdim=True) * torch.empty(C, 1).uniform_(0.4 * wnorm, wnorm, generator=g)
    y = torch.randint(0, C, (n,), generator=g)
    y[0] = 0
    y[-1] = C - 1
    Wy = W[y] / W[y].norm(dim=1, keepdim=True)
    alpha = torch.empty(n, 1).uniform_(-0.5, 1.5, generator=g)
    alpha[0] = 0.1
    x = torch.randn(n, F, generator=g) + alpha * (F ** 0.5) * Wy
    x = x * torch.empty(n, 1).uniform_(0.2, 4.0, generator=g)
    w = torch.empty(C).uniform_(0.4, 2.5, generator=g)
    mask = (torch.rand(n, generator=g) > 0.3).float()
    b = torch.empty(C).uniform_(-0.05, 0.05, generator=g) if bias else None
    return x, W, y, w, mask, b


SHAPES = [(n, F, C) for n in (1, 5, 67) for F in (4, 512, 2048) for C in (2, 23, 64)]


@pytest.mark.parametrize("n,F,C", SHAPES)
def test_kernel_shapes_vs_float64_restatement(n, F, C):
    """Every (n, F, C) corner, the kind / bias / class-weight / mask / padding / row-loss options cycling with
    the case so that each shows up at small and large sizes."""
    j = SHAPES.index((n, F, C))
    kind = mr.KINDS[j % 4]
    s, m = mr.DEFAULTS[kind]
    x, W, y, w, mask, b = seeded_case(n, F, C, seed=1000 + j, bias=j % 2 == 0)
    w = w if j % 3 != 0 else None
    mask = mask if j % 3 == 2 else None
    if mask is not None:
        mask[0] = 1.0
    ldx, lddx = (F + 4, F + 8) if (j // 2) % 2 == 0 else (F, F)
    loss, dx, dW, db, rows = mr.loss_and_grads(x, W, y, kind, s, m, b=b, w=w, mask=mask)
    rc, o = launch(x, W, y, kind, s, m, b=b, w=w, mask=mask, ldx=ldx, lddx=lddx, want_rows=j % 4 < 2)
    assert rc == 0
    assert (o["rows"] is None) == (j % 4 >= 2)
    check(o, loss, dx, dW, F, db=db, rows=rows, tag=f"n{n} F{F} C{C} {kind} ldx{ldx} lddx{lddx}",
          bound=logit_bound(W, s, m, b, w))


@pytest.mark.parametrize("kind", mr.KINDS)
def test_kernel_bias_and_db_each_alone(kind):
    """bias without db, and db without bias (db is then the column sums of the logit gradient all the same)."""
    s, m = mr.DEFAULTS[kind]
    x, W, y, w, _, b = seeded_case(5, 64, 23, seed=77, bias=True)
    loss, dx, dW, db, _ = mr.loss_and_grads(x, W, y, kind, s, m, b=b, w=w)
    rc, o = launch(x, W, y, kind, s, m, b=b, w=w, want_db=False)
    assert rc == 0 and o["db"] is None
    check(o, loss, dx, dW, 64, tag=f"{kind} bias, no db")
    zero_b = torch.zeros(23)
    loss, dx, dW, db, _ = mr.loss_and_grads(x, W, y, kind, s, m, b=zero_b, w=w)
    rc, o = launch(x, W, y, kind, s, m, w=w, want_db=True)
    assert rc == 0
    check(o, loss, dx, dW, 64, db=db, tag=f"{kind} db, no bias")


# ------------------------------------------------------------------------------------------ stability
@pytest.mark.parametrize("kind", mr.KINDS)
def test_kernel_stays_finite_where_the_literal_exp_overflows(kind):
    """s z reaching about +-200 (the reference's exp overflows fp32 past 88): finite, and the float64 value."""
    s, m = mr.DEFAULTS[kind]
    x, W, y, w, _, _ = seeded_case(24, 64, 23, seed=5, wnorm=1.0)
    x[::2] = -x[::2]  # half the rows point away from their class: large logits of both signs
    z = torch.nn.functional.normalize(x.double(), dim=1) @ W.double().t()
    W = W * (200.0 / (s * z.abs().max().item()))
    sz = s * (torch.nn.functional.normalize(x.double(), dim=1) @ W.double().t())
    assert 199.0 <= sz.abs().max().item() <= 201.0 and sz.max().item() > 150 and sz.min().item() < -150
    assert not torch.isfinite(torch.exp(sz.float())).all()  # the literal form does overflow here
    loss, dx, dW, _, rows = mr.loss_and_grads(x, W, y, kind, s, m, w=w)
    assert torch.isfinite(loss) and torch.isfinite(dx).all() and torch.isfinite(dW).all()
    rc, o = launch(x, W, y, kind, s, m, w=w)
    assert rc == 0
    check(o, loss, dx, dW, 64, rows=rows, tag=f"{kind} |s z| -> 200", bound=logit_bound(W, s, m, w=w))


# ---------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("n,F,C,kind", [(67, 512, 23, "arcface"), (5, 2048, 64, "acloss"), (1, 4, 2, "cosface")])
def test_kernel_is_deterministic_and_writes_every_entry(n, F, C, kind):
    s, m = mr.DEFAULTS[kind]
    x, W, y, w, mask, b = seeded_case(n, F, C, seed=31, bias=True)
    outs = []
    for fill in (NAN, NAN, 7.0):
        rc, o = launch(x, W, y, kind, s, m, b=b, w=w, mask=mask, fill=fill)
        assert rc == 0
        for k in ("out", "dx", "dW", "db", "rows"):
            assert not torch.isnan(o[k]).any(), k  # every entry written over the NaN fill
        outs.append(o)
    for o in outs[1:]:
        for k in ("out", "dx", "dW", "db", "rows"):
            assert torch.equal(o[k].view(torch.int32), outs[0][k].view(torch.int32)), k


def test_out_of_range_target_gives_nan_loss_and_no_gradient():
    x, W, y, _, _, _ = seeded_case(5, 64, 23, seed=3)
    y[2] = 23
    y[3] = -1
    rc, o = launch(x, W, y, "arcface", 30.0, 0.3)
    assert rc == 0 and torch.isnan(o["out"]).all() and torch.isnan(o["rows"][[2, 3]]).all()
    assert torch.isfinite(o["dx"]).all() and torch.isfinite(o["dW"]).all() and torch.isfinite(o["rows"][[0, 1, 4]]).all()
    assert torch.all(o["dx"][[2, 3]] == 0) and o["dx"][[0, 1, 4]].abs().max().item() > 0


# --------------------------------------------------------------------------------------- status codes
@pytest.mark.parametrize("what,kw", [
    ("C = 65", dict(C=65)), ("F = 6", dict(F=6)), ("F = 2052", dict(F=2052)), ("n = 0", dict(n=0)),
    ("unknown kind", dict(kind_id=4)), ("negative kind", dict(kind_id=-1)), ("null x", dict(null=("x",))),
    ("null W", dict(null=("W",))), ("null out", dict(null=("out",))), ("null targets", dict(null=("targets",))),
    ("null dx", dict(null=("dx",))), ("null dW", dict(null=("dW",))), ("null workspace", dict(null=("workspace",))),
    ("ldx < F", dict(F=64, ldx=60)), ("eps = 0", dict(eps=0.0))])
def test_bad_arguments_are_refused_before_any_launch(what, kw):
    """The header's bad-argument status, and every output left as it was."""
    if "ldx" in kw:
        x, W, y, _, _, b = seeded_case(5, 60, 23, seed=9, bias=True)
        kw = dict(F=64)  # F = 64 over rows of 60 floats
    else:
        x, W, y, _, _, b = seeded_case(5, 2052 if kw.get("F") == 2052 else 64, 23, seed=9, bias=True)
    rc, o = launch(x, W, y, "arcface", 30.0, 0.3, b=b, fill=7.0, **kw)
    assert rc == BAD_ARG, (what, rc)
    for k in ("out", "dx", "dW", "db", "rows"):
        assert torch.all(o[k] == 7.0), (what, k)
    assert _lib.load().es_margin_softmax_workspace(5, 65) == 0 and _lib.load().es_margin_softmax_workspace(0, 23) == 0
    assert _lib.load().es_margin_softmax_workspace(5, 23) == 5 * 25


def test_call_wrapper_raises_on_bad_argument():
    from endossl.loss import margin_softmax_fwd_bwd
    x, W = torch.zeros(4, 6, device=DEV), torch.zeros(23, 6, device=DEV)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.EndosslCallError, match="bad argument"):
        margin_softmax_fwd_bwd(x, W, None, y, None, None, "arcface", 30.0, 0.3, 1e-7, 0.25, torch.empty_like(x),
                               torch.empty_like(W), None, torch.zeros(1, device=DEV))


# --------------------------------------------------------------------- AngularPenaltySMLoss via autograd
def _margin_cfg(kind):
    from endossl.utils import AttrDict
    return AttrDict(MODEL=AttrDict(MARGIN=kind))


@pytest.mark.parametrize("variant", ["plain", "masked"])
@pytest.mark.parametrize("kind", mr.KINDS)
def test_angular_penalty_loss_autograd_vs_fixture(kind, variant):
    from endossl.loss import AngularPenaltySMLoss
    fx = mr.load_fixture(kind, variant)
    fc = torch.nn.Linear(64, 23, bias=False).to(DEV)
    with torch.no_grad():
        fc.weight.copy_(fx["W"])
    x = fx["x"].to(DEV).requires_grad_(True)
    crit = AngularPenaltySMLoss(_margin_cfg(kind), device=DEV)
    w = None if fx["w"] is None else fx["w"].to(DEV)
    loss = crit(x, fx["y"].to(DEV), fc, cls_weight=w, use_mask=fx["mask"] is not None,
                mask=None if fx["mask"] is None else fx["mask"].to(DEV))
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    o = {"out": loss.detach().cpu().view(1), "dx": x.grad.cpu(), "dW": fc.weight.grad.cpu(), "db": None, "rows": None}
    check(o, fx["loss"], fx["dx"], fx["dW"], 64, tag=f"autograd {kind}/{variant}")


def test_angular_penalty_loss_bias_and_upstream_gradient():
    """A Linear with a bias, a list of class weights, and a loss scaled before backward()."""
    from endossl.loss import AngularPenaltySMLoss
    x, W, y, w, _, b = seeded_case(9, 64, 23, seed=21, bias=True)
    fc = torch.nn.Linear(64, 23, bias=True).to(DEV)
    with torch.no_grad():
        fc.weight.copy_(W)
        fc.bias.copy_(b)
    xd = x.to(DEV).requires_grad_(True)
    crit = AngularPenaltySMLoss(_margin_cfg("sphereface"), device=DEV)
    (2.5 * crit(xd, y.to(DEV), fc, w.tolist())).backward()
    loss, dx, dW, db, _ = mr.loss_and_grads(x, W, y, "sphereface", 30.0, 1.35, b=b, w=w)
    torch.testing.assert_close(xd.grad.cpu(), (2.5 * dx).float(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(fc.weight.grad.cpu(), (2.5 * dW).float(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(fc.bias.grad.cpu(), (2.5 * db).float(), rtol=1e-4, atol=1e-6)


def test_consistency_loss_margin_branch():
    """code/loss.py:131-139 on a 16 x 23 case: the weak view's max-probabilities sit away from p_cutoff."""
    from endossl.loss import AngularPenaltySMLoss, consistency_loss
    g = torch.Generator().manual_seed(4)
    n, C, F, tau = 16, 23, 64, 0.7
    lw = torch.randn(n, C, generator=g)
    conf = torch.tensor([0.9, 0.5] * (n // 2))  # the max probability of each row, by construction
    top = torch.randint(0, C, (n,), generator=g)
    top[0], top[1] = 0, C - 1
    lw = torch.zeros(n, C)
    lw[torch.arange(n), top] = torch.log(conf * (C - 1) / (1 - conf))
    pw = torch.softmax(lw.double(), -1)
    assert (pw.max(-1).values - tau).abs().min().item() > 0.1 and torch.equal(pw.argmax(-1), top)
    mask = (pw.max(-1).values >= tau).double()
    assert 0 < mask.sum().item() < n
    x, W, _, _, _, _ = seeded_case(n, F, C, seed=8)
    fc = torch.nn.Linear(F, C, bias=False).to(DEV)
    with torch.no_grad():
        fc.weight.copy_(W)
    xd = x.to(DEV).requires_grad_(True)
    crit = AngularPenaltySMLoss(_margin_cfg("arcface"), device=DEV)
    loss, mask_mean = consistency_loss(lw.to(DEV), xd, p_cutoff=tau, loss_fc=crit, fc=fc)
    loss.backward()
    rl, dx, dW, _, _ = mr.loss_and_grads(x, W, top, "arcface", 30.0, 0.3, mask=mask)
    assert abs(loss.item() - float(rl)) <= 1e-5 * abs(float(rl)), (loss.item(), float(rl))
    assert mask_mean.item() == mask.mean().item()
    torch.testing.assert_close(xd.grad.cpu(), dx.float(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(fc.weight.grad.cpu(), dW.float(), rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------------------------------- the trainer
class _DS:
    df = None


class _DL(list):
    dataset = _DS()


def _cfg(margin="arcface", triplet=False, ema=True, sch="const"):
    from endossl.utils import AttrDict
    return AttrDict(DATA=AttrDict(BATCH_SIZE=8, IMG_SIZE=64, TARGET_NAME="target"),
                    MODEL=AttrDict(NAME="resnet18", NUM_CLASSES=23, MARGIN=margin, IS_TRIPLET=triplet,
                                   PRE_TRAIN_PATH="None"),
                    TRAIN=AttrDict(IS_SSL=False, USE_EMA=ema, EMA_DECAY=0.999, BASE_LR=1e-3, CLS_WEIGHT=False, EPOCHS=1,
                                   WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME=sch,
                                   FREQ_EVAL=1, THRES=0.05, LAMBDA_C=1.0))


LR, DECAY = 1e-3, 0.999
CW = torch.linspace(0.5, 2.0, 23)


def _trainer(kind, seed=5, sch="const"):
    from endossl.build import build_model
    from endossl.resnet import ModelMargin
    from endossl.supervised import SupLearning
    cfg = _cfg(kind, sch=sch)
    m = build_model(cfg, seed=seed)
    assert type(m) is ModelMargin
    state = {k[len("model."):]: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("model.")}
    m = m.to(DEV).set_conv_precision("fp32")
    g = torch.Generator().manual_seed(8)
    x, y = torch.randn(8, 3, 64, 64, generator=g), torch.randint(0, 23, (8,), generator=g)
    tr = SupLearning(m, opt_func="Adam", lr=LR, device=DEV)
    tr.get_dataloader(_DL([(x, y)]), _DL([(x, y), (x[:3], y[:3])]), None)
    tr.get_config(cfg)
    tr.class_weights = CW.to(DEV)
    return tr, m, state, x, y


def _oracle_chain(state, x, y, kind, dtype):
    """oracle/resnet_ref.py's ResNet-18 up to the pooled features (its fc replaced by the identity: the margin
    model's fc has no bias and enters through the loss), then the restatement: loss and every gradient."""
    s, mg = mr.DEFAULTS[kind]
    p = {k: v.clone().to(dtype).requires_grad_(True) for k, v in state.items() if not is_buffer(k)}
    bufs = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items() if is_buffer(k)}
    trunk = dict(p)
    trunk["fc.weight"], trunk["fc.bias"] = torch.eye(512, dtype=dtype), torch.zeros(512, dtype=dtype)
    fts = rr.resnet18_forward(trunk, bufs, x.to(dtype), train=True)
    fts.retain_grad()
    loss = mr.margin_loss(fts, p["fc.weight"], y, kind, s, mg, w=CW.to(dtype))
    loss.backward()
    return {"fts": fts.detach(), "loss": loss.item(), "dfts": fts.grad, "p": p, "bufs": bufs,
            "grads": {k: v.grad for k, v in p.items()}}


def test_margin_trainer_step_stage_by_stage(monkeypatch):
    """SupLearning.step in margin mode (code/supervised.py:117-119), arcface, class weights on, fp32 convs."""
    import endossl.supervised as sup
    tr, m, state, x, y = _trainer("arcface")
    seen = {}
    real = sup.margin_softmax_fwd_bwd

    def spy(*a, **k):
        seen["dfts"], seen["dW"], seen["n_calls"] = a[11], a[12], seen.get("n_calls", 0) + 1
        return real(*a, **k)
    monkeypatch.setattr(sup, "margin_softmax_fwd_bwd", spy)
    o32, o64 = _oracle_chain(state, x, y, "arcface", torch.float32), _oracle_chain(state, x, y, "arcface", torch.float64)
    ema0 = {k: v.detach().clone() for k, v in state.items()}
    out = tr.step((x, y))
    torch.cuda.synchronize()
    assert set(out) == {"loss", "fts"} and seen["n_calls"] == 1
    assert seen["dW"].data_ptr() == m.gview("fc.weight").data_ptr()  # written straight into the flat gradient

    # features: the device's trunk against the oracle's
    fts = out["fts"].cpu()
    sc = max(1.0, o32["fts"].abs().max().item())
    e_fts = (fts.double() - o32["fts"].double()).abs().max().item()
    # loss, dfts, fc.weight gradient: the restatement in float64 on the device's OWN features
    Wfc = state["fc.weight"]
    loss, dx, dW, _, _ = mr.loss_and_grads(fts, Wfc, y, "arcface", 30.0, 0.3, w=CW)
    dfts = seen["dfts"].cpu()
    gW = m.gview("fc.weight").cpu().view(23, 512)
    print({"fts_err": e_fts, "scale": sc, "loss": out["loss"].item(), "ref_loss": float(loss), "oracle_loss": o32["loss"],
           "dfts_err": (dfts.double() - dx).abs().max().item(), "dW_err": (gW.double() - dW).abs().max().item()})
    assert e_fts <= 1e-3 * sc, (e_fts, sc)
    assert abs(out["loss"].item() - float(loss)) <= 1e-4 * max(1.0, abs(float(loss)))
    torch.testing.assert_close(dfts, dx.float(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(gW, dW.float(), rtol=1e-4, atol=1e-5)

    # a sample of trunk gradients against the oracle's chain (test_resnet18_forward_backward_vs_oracle's bar)
    gmax = max(v.double().norm().item() for v in o32["grads"].values())
    bad = []
    for k in ("conv1.weight", "bn1.weight", "layer1.0.conv1.weight", "layer2.0.downsample.0.weight",
              "layer3.1.bn2.bias", "layer4.1.conv2.weight", "fc.weight"):
        gh = m.gview(k).cpu().view(o32["grads"][k].shape).double()
        g32, g64 = o32["grads"][k].double(), o64["grads"][k].double()
        e, env, nrm = (gh - g64).norm().item(), 4 * (g32 - g64).norm().item(), g32.norm().item()
        if e > 2e-3 * nrm + env + 1e-4 * gmax:
            bad.append((k, e, env, nrm))
    assert not bad, bad

    # the update: Adam(lr, wd 0) from the oracle's gradients, EMA over every state entry, BatchNorm buffers
    names = list(o32["p"])
    opt = torch.optim.Adam([o32["p"][k] for k in names], lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    opt.step()
    new = {k: o32["p"][k].detach() for k in names}
    new.update(o32["bufs"])
    ref.ema_update(ema0, new, DECAY)
    sd, esd = m.state_dict(), tr.ema_model.ema.state_dict()
    assert list(sd) == ["model." + k for k in state] + ["fc.weight"]
    for k, v in new.items():
        d, e = sd["model." + k].cpu(), esd["model." + k].cpu()
        if is_buffer(k):
            if k.endswith("num_batches_tracked"):
                assert int(d.item()) == 1 and int(e.item()) == 0  # EMA of an int buffer truncates
            else:
                assert (d - v).abs().max().item() <= 1e-3 * max(1.0, v.abs().max().item()), k
            continue
        assert (d - v).abs().max().item() <= 2 * LR + 1e-6, k
        assert (d - state[k]).abs().max().item() > 0, k  # every parameter moved, fc.weight among them
        assert (e - ema0[k]).abs().max().item() <= (1 - DECAY) * 2 * LR + 1e-6, k
    assert torch.equal(sd["fc.weight"], sd["model.fc.weight"])


def test_margin_trainer_step_cosface():
    tr, m, state, x, y = _trainer("cosface", seed=6)
    out = tr.step((x, y))
    torch.cuda.synchronize()
    fts = out["fts"].cpu()
    loss, _, dW, _, _ = mr.loss_and_grads(fts, state["fc.weight"], y, "cosface", 30.0, 0.4, w=CW)
    assert abs(out["loss"].item() - float(loss)) <= 1e-4 * max(1.0, abs(float(loss)))
    torch.testing.assert_close(m.gview("fc.weight").cpu().view(23, 512), dW.float(), rtol=1e-4, atol=1e-5)
    o32 = _oracle_chain(state, x, y, "cosface", torch.float32)
    assert abs(out["loss"].item() - o32["loss"]) <= 1e-3 * max(1.0, abs(o32["loss"]))  # through the oracle's trunk


def test_margin_model_eval_inference_checkpoint(tmp_path):
    """After a step: evaluate_one / test_one / inference run on the margin model's plain logits, and a checkpoint
    round-trips bit-exactly into a fresh trainer."""
    import numpy as np
    import torch.nn.functional as F
    tr, m, state, x, y = _trainer("arcface", sch="cosine")  # a scheduler with a state to save
    tr.step((x, y))
    ema = tr.ema_model.ema
    ema.eval()
    with torch.no_grad():
        lg = [ema(b.to(DEV)).cpu().double() for b, _ in tr.valid_dl]
        fts = ema.backbone(x.to(DEV))
    assert tuple(lg[0].shape) == (8, 23) and tuple(fts.shape) == (8, 512) and not fts.requires_grad
    # model(x) = fc(backbone(x)), plain logits: no normalisation, no bias
    want = fts.cpu().double() @ ema.fc.weight.detach().cpu().double().t()
    assert (lg[0] - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
    loss, metric = tr.evaluate_one()
    ce = float(np.mean([F.cross_entropy(l, t).item() for l, (_, t) in zip(lg, tr.valid_dl)]))
    assert abs(loss.avg - ce) <= 1e-5 * max(1.0, abs(ce)), (loss.avg, ce)
    pred = torch.cat(lg).argmax(1)
    assert abs(metric["micro/f1"] - (pred == torch.cat([y, y[:3]])).double().mean().item()) <= 1e-12
    wrong = tr.test_one()
    assert wrong.dtype == torch.bool and tuple(wrong.shape) == (11,)
    got = tr.inference(_DL([(x, torch.arange(8) + 100)]))
    assert list(got) == list(range(100, 108)) and all(isinstance(v, int) and 0 <= v < 23 for v in got.values())

    tr.epoch = 0
    path = tr.save_checkpoint(str(tmp_path))
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert "model.fc.weight" in ck["model_state_dict"] and "fc.weight" in ck["model_state_dict"]
    assert not any(k.endswith("fc.bias") for k in ck["model_state_dict"])
    tr2, m2, _, _, _ = _trainer("arcface", seed=11, sch="cosine")
    assert not torch.equal(m2.flat, m.flat)
    tr2.load_checkpoint(path, is_train=True)
    assert torch.equal(m2.flat, m.flat) and torch.equal(tr2.ema_model.ema.flat, ema.flat)
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    # and it trains on: the two trainers take the same step
    o1, o2 = tr.step((x, y)), tr2.step((x, y))
    torch.cuda.synchronize()
    assert torch.equal(o1["loss"], o2["loss"]) and torch.equal(m2.flat, m.flat)


def test_get_config_errors_on_the_device():
    from endossl.build import build_model
    from endossl.resnet import NativeResNet, ResNetConfig
    from endossl.supervised import SupLearning
    from endossl.vit import NativeViT, ViTConfig
    for m in (NativeResNet(ResNetConfig(num_classes=23), seed=0),
              NativeViT(ViTConfig(img_size=64, dim=128, depth=2, heads=2, num_classes=23), seed=0)):
        tr = SupLearning(m, device=DEV)
        tr.get_dataloader(_DL([]), None)
        with pytest.raises(ValueError, match="backbone"):
            tr.get_config(_cfg("arcface"))
        with pytest.raises(ValueError):
            tr.get_config(_cfg("arcface", triplet=True))
    # a margin together with IS_TRIPLET is the triplet step (code/supervised.py:84): the margin model has no
    # embedding head, so that is refused as any other model without one
    tr = SupLearning(build_model(_cfg("cosface")), device=DEV)
    tr.get_dataloader(_DL([]), None)
    with pytest.raises(ValueError):
        tr.get_config(_cfg("cosface", triplet=True))
    tr.get_config(_cfg("cosface"))
    assert tr.is_margin and not tr.is_triplet
    with pytest.raises(NotImplementedError):
        tr.get_dataloader(_DL([]), None, mixup_fn=lambda a, b: (a, b))
