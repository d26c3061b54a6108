"""The squeeze-excite tail kernels (csrc/se.hip) on the MI355X, in the style of tests/test_gpu_conv_exact.py.

Shapes (N, H x W, C): 1 x 1x1 x 16, 2 x 2x2 x 2048, 3 x 7x7 x 256, 2 x 4x4 x 96, 5 x 14x14 x 512, 2 x 56x56 x 64 (the
last splits HW in the two sums passes), each with fp32 and with bf16 maps; ONE float64 CPU reference per case,
computed once and shared.

Exact (torch.equal): the four passes over the maps -- squeeze, apply, sums, dx.  The operands are drawn so that
every intermediate and every result is exactly representable in fp32 and, for map outputs, in bf16 (multiples of
1/4 below 64), so neither the association of a sum nor an FMA contraction can change a bit:
  mean  integers in [-2, 2] (dx: [-1, 1]);   gamma, beta  integers in [-2, 2];   rstd in {1/4, 1/2, 1, 2};
  the gate s in {1/4, 1/2, 1, 2}, raised per element to 1/(4 rstd) where rstd s would fall below 1/4;
  y     integers in [-4, 4] (dx: [-2, 2]) built as k + (r - roll(r)) with k in [-2, 2], r in [-1, 1] (dx: k in
        [-1, 1], r in {0, 1}): every per-image channel sum is HW k exactly, so ybar = k and a = gamma (k - mean) rstd
        + beta is a multiple of 1/4 below 19;  res, dout integers in [-4, 4] / [-2, 2];
  apply:  |s o + res| <= 2 (6 * 2 * 2) + 2 * 2 + 4 = 56, a multiple of 1/4; out = 0 wherever that is <= 0;
  sums:   xhat = (y - mean) rstd is a multiple of 1/4 up to 12, P2's terms up to 24, 3136 of them: below 2^24 / 4;
  dx:     da = HW k', dbeta = M j, dgamma = M i with k', j in [-2, 2] and i in {-1, 0, 1} (times 4 where rstd = 1/4),
          so the three divisions are exact for any M; dy = rstd gamma ((g s + k' - j) - xhat i): |.| <=
          16 + 16 + 24 = 56, a multiple of 1/4.  out = 0 elements take no gradient (dy from the batch terms only,
          gres = 0); gres also in accumulate mode, on integers.
Repeated launches are bit-identical, and the outputs do not depend on what the output and workspace buffers held
(pre-filled with NaN).

es_se_bn_apply_ex with a gate of 1 is bit-identical to es_bn2d_fwd_ex(res, relu = 1) on random floats.

The [N, C]-sized launches (gate forward / backward, dgamma, dbeta, da) run on random floats against float64 at the
project's fp32 bar, rtol 1e-4 / atol 1e-6 (tests/test_gpu_margin.py).  Their inputs are scaled so that every
reduction (at most 2048 terms, in fp32 chains of at most 128) gives results of rms <= ~0.3: the accumulated rounding
error of such a sum is about 2^-24 * 0.3 * sqrt(128) ~ 2e-7 in absolute terms, inside atol where a result cancels
to near zero, and ~1e-6 relative elsewhere.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from endossl import _lib  # noqa: E402
from endossl._lib import ptr  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SHAPES = [(1, 1, 1, 16), (2, 2, 2, 2048), (3, 7, 7, 256), (2, 4, 4, 96), (5, 14, 14, 512), (2, 56, 56, 64)]
DTYPES = [torch.float32, torch.bfloat16]
QUARTERS = torch.tensor([0.25, 0.5, 1.0, 2.0], dtype=torch.float64)


def S():
    return _lib.stream()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _lib.load()


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


_CACHE = {}


def _case(shape, small):
    """Operands and float64 references of a shape (small: the dx ranges), computed once on the CPU."""
    key = (shape, small)
    if key in _CACHE:
        return _CACHE[key]
    N, H, W, C = shape
    HW, M = H * W, N * H * W
    g = torch.Generator().manual_seed(1000 + 7 * C + HW + (500 if small else 0))
    k = _ints(g, (N, 1, C), -1, 1) if small else _ints(g, (N, 1, C), -2, 2)
    r = _ints(g, (N, HW, C), 0, 1) if small else _ints(g, (N, HW, C), -1, 1)
    y = k + (r - torch.roll(r, 1, dims=1))
    mean = _ints(g, (C,), -1, 1) if small else _ints(g, (C,), -2, 2)
    rstd = QUARTERS[torch.randint(0, 4, (C,), generator=g)]
    gamma, beta = _ints(g, (C,), -2, 2), _ints(g, (C,), -2, 2)
    s = torch.maximum(QUARTERS[torch.randint(0, 4, (N, C), generator=g)], 0.25 / rstd)
    res, dout = _ints(g, (N, HW, C), -4, 4), _ints(g, (N, HW, C), -2, 2)
    xhat = (y - mean) * rstd
    o = gamma * xhat + beta
    ybar = y.mean(1)
    assert torch.equal(ybar, k[:, 0])
    out = torch.relu(s[:, None] * o + res)
    assert out.abs().max() <= 56 and torch.equal(out * 4, (out * 4).round()) and (out == 0).any() and (out > 0).any()
    gg = dout * (out > 0)
    d = dict(N=N, HW=HW, C=C, M=M, y=y, mean=mean, rstd=rstd, gamma=gamma, beta=beta, s=s, res=res, dout=dout,
             ybar=ybar, a=gamma * (ybar - mean) * rstd + beta, out=out, p1=gg.sum(1), p2=(gg * xhat).sum(1), g=gg)
    if small:
        da = HW * _ints(g, (N, C), -2, 2)
        dbeta = M * _ints(g, (C,), -2, 2)
        dgamma = M * _ints(g, (C,), -1, 1) * torch.where(rstd == 0.25, 4.0, 1.0)
        d_o = gg * s[:, None] + (da / HW)[:, None]
        dy_train = gamma * rstd * (d_o - dbeta / M - xhat * dgamma / M)
        dy_eval = gamma * rstd * d_o
        for t in (dy_train, dy_eval):
            assert t.abs().max() <= 56 and torch.equal(t * 4, (t * 4).round())
        gprev = _ints(g, (N, HW, C), -3, 3)
        d.update(da=da, dbeta=dbeta, dgamma=dgamma, dy_train=dy_train, dy_eval=dy_eval, gprev=gprev)
    _CACHE[key] = d
    return d


def _dev(t, dtype=torch.float32):
    out = t.to(dtype)
    assert torch.equal(out.double(), t), "operand not representable"
    return out.to(DEV).contiguous()


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _twice(run):
    """run() -> tuple of output tensors; launched twice into fresh NaN-filled buffers: the same bits."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert not torch.isnan(u.float()).any()
        assert torch.equal(u, v)
    return a


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_squeeze_exact(lib, shape, dtype):
    d = _case(shape, False)
    N, HW, C, fl = d["N"], d["HW"], d["C"], int(dtype == torch.bfloat16)
    y = _dev(d["y"], dtype)
    mean, rstd, gamma, beta = (_dev(d[k]) for k in ("mean", "rstd", "gamma", "beta"))
    nws = lib.es_se_squeeze_workspace(N, HW, C, fl)
    if shape == (2, 56, 56, 64):
        assert nws > N * C  # HW is split

    def run():
        ybar, a, ws = _nan((N, C)), _nan((N, C)), _nan((nws,))
        assert lib.es_se_squeeze_ex(ptr(y), N, HW, C, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(ybar), ptr(a),
                                    ptr(ws), fl, S()) == 0
        return ybar, a
    ybar, a = _twice(run)
    assert torch.equal(ybar.cpu().double(), d["ybar"])
    assert torch.equal(a.cpu().double(), d["a"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_apply_exact(lib, shape, dtype):
    d = _case(shape, False)
    N, HW, C, fl = d["N"], d["HW"], d["C"], int(dtype == torch.bfloat16)
    y, res = _dev(d["y"], dtype), _dev(d["res"], dtype)
    s, mean, rstd, gamma, beta = (_dev(d[k]) for k in ("s", "mean", "rstd", "gamma", "beta"))

    def run():
        out = _nan((N, HW, C), dtype)
        assert lib.es_se_bn_apply_ex(ptr(y), ptr(res), ptr(s), N, HW, C, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                     ptr(out), fl, S()) == 0
        return (out,)
    (out,) = _twice(run)
    assert torch.equal(out.cpu().double(), d["out"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bwd_sums_exact(lib, shape, dtype):
    d = _case(shape, False)
    N, HW, C, fl = d["N"], d["HW"], d["C"], int(dtype == torch.bfloat16)
    y, out, dout = _dev(d["y"], dtype), _dev(d["out"], dtype), _dev(d["dout"], dtype)
    mean, rstd = _dev(d["mean"]), _dev(d["rstd"])
    nws = lib.es_se_bn_bwd_sums_workspace(N, HW, C, fl)

    def run():
        p1, p2, ws = _nan((N, C)), _nan((N, C)), _nan((nws,))
        assert lib.es_se_bn_bwd_sums_ex(ptr(y), ptr(out), ptr(dout), N, HW, C, ptr(mean), ptr(rstd), ptr(p1), ptr(p2),
                                        ptr(ws), fl, S()) == 0
        return p1, p2
    p1, p2 = _twice(run)
    assert torch.equal(p1.cpu().double(), d["p1"])
    assert torch.equal(p2.cpu().double(), d["p2"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bwd_dx_exact(lib, shape, dtype):
    d = _case(shape, True)
    N, HW, C, fl = d["N"], d["HW"], d["C"], int(dtype == torch.bfloat16)
    y, out, dout = _dev(d["y"], dtype), _dev(d["out"], dtype), _dev(d["dout"], dtype)
    s, da, mean, rstd, gamma, dgamma, dbeta = (_dev(d[k]) for k in ("s", "da", "mean", "rstd", "gamma", "dgamma",
                                                                     "dbeta"))
    gprev = _dev(d["gprev"], dtype)
    for train, acc in ((1, 0), (0, 0), (1, 1)):
        def run():
            dy = _nan((N, HW, C), dtype)
            gres = gprev.clone() if acc else _nan((N, HW, C), dtype)
            assert lib.es_se_bn_bwd_dx_ex(ptr(y), ptr(out), ptr(dout), ptr(s), ptr(da), N, HW, C, ptr(mean), ptr(rstd),
                                          ptr(gamma), ptr(dgamma) if train else None, ptr(dbeta) if train else None,
                                          train, ptr(dy), ptr(gres), acc, fl, S()) == 0
            return dy, gres
        dy, gres = _twice(run)
        assert torch.equal(dy.cpu().double(), d["dy_train" if train else "dy_eval"]), (train, acc)
        assert torch.equal(gres.cpu().double(), d["g"] + (d["gprev"] if acc else 0)), (train, acc)
    dead = d["out"] == 0
    assert dead.any() and torch.equal(d["g"][dead], torch.zeros_like(d["g"][dead]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_apply_with_unit_gate_is_the_batchnorm_apply(lib, shape, dtype):
    """Random floats: es_bn2d_fwd_ex (train, residual, ReLU) computes the statistics and its output; the SE apply
    with s == 1 on the same mean / rstd gives the same bits."""
    N, H, W, C = shape
    HW, rows, fl = H * W, N * H * W, int(dtype == torch.bfloat16)
    g = torch.Generator().manual_seed(31 + C + HW)
    y = (torch.randn(N, HW, C, generator=g) * 1.5 + 0.3).to(dtype).to(DEV)
    res = torch.randn(N, HW, C, generator=g).to(dtype).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.3).to(DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, rstd = _nan((C,)), _nan((C,))
    ws = torch.empty(lib.es_chan_workspace(rows, C), device=DEV)
    want = _nan((N, HW, C), dtype)
    assert lib.es_bn2d_fwd_ex(ptr(y), rows, C, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), None, 0.1, 1e-5, 1, ptr(res), 1,
                              ptr(want), ptr(mean), ptr(rstd), ptr(ws), fl, S()) == 0
    out = _nan((N, HW, C), dtype)
    ones = torch.ones(N, C, device=DEV)
    assert lib.es_se_bn_apply_ex(ptr(y), ptr(res), ptr(ones), N, HW, C, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                 ptr(out), fl, S()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(want.float()).any()
    assert torch.equal(out, want)


def _gate_case(N, C, R):
    key = ("gate", N, C, R)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(77 + C + R)
    rn = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
    a = rn(N, C)
    wd = rn(R, C) * (0.3 / C ** 0.5)   # h = a W_down^T: rms ~0.3
    wu = rn(C, R) / R ** 0.5           # z = h W_up^T:  rms ~0.2; dh = dt W_up: rms ~0.03 sqrt(C / R)
    p1, p2 = rn(N, C) * 0.1, rn(N, C) * 0.1
    ybar = rn(N, C)
    gamma, beta = torch.rand(C, generator=g) + 0.5, rn(C) * 0.3
    mean, rstd = rn(C) * 0.2, torch.rand(C, generator=g) + 0.5
    D = torch.float64
    dead = ((a.to(D) @ wd.to(D).T) <= 0).all(0)  # a hidden unit no image excites: flipped, so every ReLU is live
    wd[dead] = -wd[dead]
    a64, wd64, wu64 = a.to(D), wd.to(D), wu.to(D)
    pre = a64 @ wd64.T
    assert (pre > 0).any(0).all()
    h = torch.relu(pre)
    s = torch.sigmoid(h @ wu64.T)
    # the backward takes the DEVICE's fp32 h and s; its float64 reference uses their fp32 roundings as inputs
    h32, s32 = h.float(), s.float()
    hd, sd = h32.to(D), s32.to(D)
    dt = (gamma.to(D) * p2.to(D) + beta.to(D) * p1.to(D)) * sd * (1 - sd)
    dh = (dt @ wu64) * (hd > 0)
    da = dh @ wd64
    xbar = (ybar.to(D) - mean.to(D)) * rstd.to(D)
    ref = dict(h=h, s=s, dwu=dt.T @ hd, dwd=dh.T @ a64, da=da, dbeta=(sd * p1.to(D) + da).sum(0),
               dgamma=(sd * p2.to(D) + da * xbar).sum(0))
    ops = dict(a=a, wd=wd, wu=wu, p1=p1, p2=p2, ybar=ybar, gamma=gamma, beta=beta, mean=mean, rstd=rstd, h=h32, s=s32)
    _CACHE[key] = (ops, ref)
    return ops, ref


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gate_forward_and_backward_vs_float64(lib, shape):
    """R = C / 16 (the model's planes / 4 over 4 planes): 1, 128, 16, 6, 32, 4 -- one, the largest, and a
    non-power-of-two reduction width among them."""
    N, _, _, C = shape
    R = C // 16
    ops, ref = _gate_case(N, C, R)
    o = {k: v.to(DEV).contiguous() for k, v in ops.items()}
    bar = dict(rtol=1e-4, atol=1e-6)

    def fwd():
        h, s = _nan((N, R)), _nan((N, C))
        assert lib.es_se_gate_fwd(ptr(o["a"]), ptr(o["wd"]), ptr(o["wu"]), N, C, R, ptr(h), ptr(s), S()) == 0
        return h, s
    h, s = _twice(fwd)
    torch.testing.assert_close(h.cpu(), ref["h"].float(), **bar)
    torch.testing.assert_close(s.cpu(), ref["s"].float(), **bar)
    nws = lib.es_se_gate_bwd_workspace(N, C, R)
    assert nws >= N * C + N * R

    def bwd():
        dwd, dwu, da, dg, db, ws = _nan((R, C)), _nan((C, R)), _nan((N, C)), _nan((C,)), _nan((C,)), _nan((nws,))
        assert lib.es_se_gate_bwd(ptr(o["p1"]), ptr(o["p2"]), ptr(o["ybar"]), ptr(o["a"]), ptr(o["h"]), ptr(o["s"]),
                                  ptr(o["wd"]), ptr(o["wu"]), ptr(o["gamma"]), ptr(o["beta"]), ptr(o["mean"]),
                                  ptr(o["rstd"]), N, C, R, ptr(dwd), ptr(dwu), ptr(da), ptr(dg), ptr(db), ptr(ws),
                                  S()) == 0
        return dwd, dwu, da, dg, db
    dwd, dwu, da, dg, db = _twice(bwd)
    for got, name in ((dwd, "dwd"), (dwu, "dwu"), (da, "da"), (dg, "dgamma"), (db, "dbeta")):
        torch.testing.assert_close(got.cpu(), ref[name].float(), msg=lambda m, n=name: f"{n}: {m}", **bar)
