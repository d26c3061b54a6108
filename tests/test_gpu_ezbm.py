"""EZBM on the MI355X: es_ezbm_sample_mix (indices exact against the numpy restatement, the mix bit for bit
against torch's fp32 expression), es_bn1d_groups_fwd / _bwd (G = 1 and the per-group order bit for bit against
es_bn1d_fwd / _bwd, G > 1 against float64), es_ezbm_ce_fwd_bwd against float64 autograd, the stage-2 step
against the reference-generated fixtures tests/golden/ezbm_stage2_*.npz, stage 1 bit for bit against
SupLearning's triplet step, and fit() end to end.

Bars (the project's for fp32 kernels, tests/test_gpu_triplet.py): loss values rtol 1e-5; everything else rtol
1e-4 / atol 1e-6; indices, counts and the mix exact.
"""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ezbm_restatement as er  # noqa: E402
from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BAR = dict(rtol=1e-4, atol=1e-6)


def S():
    return _lib.stream()


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _lib.load()


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------- es_ezbm_sample_mix
def make_bank(N, D, C, seed):
    """mem [N, D] fp32, targets with every class present (class C-1 exactly once), an imbalanced cls_num_list."""
    from endossl.ezbm import class_csr
    g = torch.Generator().manual_seed(seed)
    y = torch.cat([torch.arange(C), torch.randint(0, max(C - 1, 1), (N - C,), generator=g)])
    y = y[torch.randperm(N, generator=g)].to(torch.int64)
    mem = torch.randn(N, D, generator=g) * (1 + 3 * torch.rand(N, 1, generator=g))
    cls_num = [int(5 + 400 * 0.6 ** c) for c in range(C)]
    off, idx = class_csr(y.numpy(), C)
    return mem.contiguous(), y, cls_num, off, idx


def run_sample_mix(mem, ldm, y, C, off, idx, cdf, tab, seed, offset, n, ldx, idx_in=None, dual_in=None):
    N, D = mem.shape
    memp = torch.full((N, ldm), NAN)
    memp[:, :D] = mem
    d = lambda a: None if a is None else torch.as_tensor(a).to(DEV)  # noqa: E731
    memp, yd, offd, idxd, cdfd, tabd = d(memp), d(y), d(off), d(idx), d(cdf), d(tab)
    ii, di = d(idx_in), d(dual_in)
    X = torch.full((2 * n, ldx), NAN, device=DEV)
    t = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    td = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    lam = torch.full((n,), NAN, device=DEV)
    io = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    do = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    call("es_ezbm_sample_mix", ptr(memp), ldm, ptr(yd), N, D, C, ptr(offd), ptr(idxd), ptr(cdfd), ptr(tabd), seed,
         offset, ptr(ii), ptr(di), n, ptr(X), ldx, ptr(t), ptr(td), ptr(lam), ptr(io), ptr(do), S())
    return {k: v.cpu() for k, v in dict(X=X, t=t, td=td, lam=lam, idx=io, dual=do).items()}


SAMPLE_CASES = [  # n, D, ldm, ldx, C, N, expansion
    (1, 1, 1, 1, 2, 5, "balance"),
    (5, 4, 4, 4, 6, 40, "reverse"),
    (130, 100, 100, 100, 64, 200, "reverse"),
    (130, 384, 390, 388, 6, 97, "balance"),
    (5, 100, 101, 103, 2, 9, "reverse"),
]


@pytest.mark.parametrize("n,D,ldm,ldx,C,N,exp", SAMPLE_CASES)
def test_sample_mix_drawn_and_replayed(n, D, ldm, ldx, C, N, exp):
    from endossl.ezbm import class_cdf, lam_table
    mem, y, cls_num, off, idx = make_bank(N, D, C, seed=n + D + C)
    cdf, tab = class_cdf(cls_num, exp), lam_table(cls_num, exp)
    seed, offset = 0x1234567 + n, (1 << 33) + 12 * D
    o = run_sample_mix(mem, ldm, y, C, off, idx, cdf, tab, seed, offset, n, ldx)
    ra, rb, ca, cb = er.sample(n, C, off, idx, cdf, seed, offset)
    assert np.array_equal(o["idx"].numpy(), ra) and np.array_equal(o["dual"].numpy(), rb)
    assert np.array_equal(o["t"].numpy(), ca) and np.array_equal(o["td"].numpy(), cb)  # the row is of its drawn class
    assert torch.equal(o["t"], y[ra]) and torch.equal(o["td"], y[rb])
    lam = torch.from_numpy(tab)[o["t"] * C + o["td"]]
    assert torch.equal(bits(o["lam"]), bits(lam))
    want = er.mix(mem, torch.from_numpy(ra), torch.from_numpy(rb), lam)
    assert torch.equal(bits(o["X"][:, :D]), bits(want))  # both halves, bit for bit
    assert torch.isnan(o["X"][:, D:]).all()  # the padding columns are not written
    # replay: the indices come back, the batch is the same; the class table and the CDF are not needed
    r = run_sample_mix(mem, ldm, y, C, None, None, None, tab, 0, 0, n, ldx, idx_in=o["idx"], dual_in=o["dual"])
    for k in o:
        assert torch.equal(bits(r[k]) if r[k].dtype == torch.float32 else r[k],
                           bits(o[k]) if o[k].dtype == torch.float32 else o[k]), k


@pytest.mark.parametrize("exp", ["balance", "reverse"])
def test_sample_mix_class_frequencies(exp):
    """60,000 draws: each class within 5 binomial standard deviations of its probability -- the row's class
    uniform, the dual's class from the CDF."""
    from endossl.ezbm import class_cdf, lam_table
    n, C, N = 60000, 6, 97
    mem, y, _, off, idx = make_bank(N, 1, C, seed=3)
    cls_num = [400, 120, 60, 30, 12, 5]
    cdf, tab = class_cdf(cls_num, exp), lam_table(cls_num, exp)
    o = run_sample_mix(mem, 1, y, C, off, idx, cdf, tab, 99, 7, n, 1)
    ra, rb, _, _ = er.sample(n, C, off, idx, cdf, 99, 7)
    assert np.array_equal(o["idx"].numpy(), ra) and np.array_equal(o["dual"].numpy(), rb)
    p_dual = np.diff(np.concatenate([[0.0], cdf.astype(np.float64)]))
    for name, cls, p in (("row", o["t"], np.full(C, 1.0 / C)), ("dual", o["td"], p_dual)):
        f = np.bincount(cls.numpy(), minlength=C) / n
        sd = np.sqrt(p * (1 - p) / n)
        print({"expansion": exp, "draw": name, "freq": f.round(5).tolist(), "p": p.round(5).tolist(),
               "worst_sd": float(np.max(np.abs(f - p) / sd))})
        assert np.all(np.abs(f - p) <= 5 * sd), (name, f, p)
    # members: every row of a class is reached, about equally often (class 0 has the most rows)
    rows0 = idx[off[0]:off[1]]
    cnt = np.bincount(o["idx"].numpy(), minlength=N)[rows0]
    m, tot = len(rows0), cnt.sum()
    assert np.all(np.abs(cnt / tot - 1.0 / m) <= 5 * np.sqrt((1.0 / m) * (1 - 1.0 / m) / tot))


def test_sample_mix_bad_rows_and_status_codes():
    """A replay index outside the bank reads nothing: NaN rows and target -1 for that row only.  Refusals."""
    from endossl.ezbm import class_cdf, lam_table
    N, D, C, n = 9, 4, 2, 3
    mem, y, cls_num, off, idx = make_bank(N, D, C, seed=1)
    cdf, tab = class_cdf(cls_num, "balance"), lam_table(cls_num, "balance")
    o = run_sample_mix(mem, D, y, C, None, None, None, tab, 0, 0, n, D, idx_in=torch.tensor([2, N, 3], dtype=torch.int32),
                       dual_in=torch.tensor([1, 0, -1], dtype=torch.int32))
    assert o["t"].tolist() == [int(y[2]), -1, -1] and o["td"].tolist() == [int(y[1]), -1, -1]
    assert torch.isnan(o["X"][[1, 2, 4, 5]]).all() and torch.isfinite(o["X"][[0, 3]]).all()
    assert torch.isnan(o["lam"][1:]).all() and o["lam"][0] == 0.5
    lib = _lib.load()
    d = lambda a: torch.as_tensor(a).to(DEV)  # noqa: E731
    T = dict(mem=d(mem), ldm=D, y=d(y), N=N, D=D, C=C, off=d(off), idx=d(idx), cdf=d(cdf), tab=d(tab), seed=1, offset=0,
             ii=None, di=None, n=n, X=torch.zeros(2 * n, D, device=DEV), ldx=D,
             t=torch.zeros(n, dtype=torch.int64, device=DEV), td=torch.zeros(n, dtype=torch.int64, device=DEV),
             lam=torch.zeros(n, device=DEV), io=torch.zeros(n, dtype=torch.int32, device=DEV),
             do=torch.zeros(n, dtype=torch.int32, device=DEV))
    order = ("mem", "ldm", "y", "N", "D", "C", "off", "idx", "cdf", "tab", "seed", "offset", "ii", "di", "n", "X", "ldx",
             "t", "td", "lam", "io", "do")

    def f(**kw):
        a = {**T, **kw}
        return lib.es_ezbm_sample_mix(*[ptr(a[k]) if torch.is_tensor(a[k]) else a[k] for k in order], S())
    assert f() == 0
    for bad in (dict(n=0), dict(N=0), dict(N=1 << 24), dict(D=0), dict(D=2049), dict(C=0), dict(C=65), dict(ldm=D - 1),
                dict(ldx=D - 1)):
        assert f(**bad) == -1, bad  # ES_BAD_SHAPE
    for bad in (dict(mem=None), dict(y=None), dict(tab=None), dict(X=None), dict(t=None), dict(td=None), dict(lam=None),
                dict(io=None), dict(do=None), dict(off=None), dict(idx=None), dict(cdf=None),
                dict(ii=T["io"]), dict(di=T["do"])):
        assert f(**bad) == -2, bad  # ES_BAD_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- grouped BatchNorm1d
def bn_inputs(n, G, F, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(G * n, F, generator=g) * (0.5 + torch.rand(1, F, generator=g) * 3) + torch.randn(1, F, generator=g)
    if n <= 3:
        # Few rows: keep a feature's rows of a group 4 apart (sorted, then spread).  BatchNorm over 2 or 3 rows
        # that nearly coincide is ill-conditioned in its input (xhat ~ d / sqrt(d^2 + eps)), and dU is then a
        # difference of O(1) terms that cancels to O(eps / var): with rstd <= 0.5 the fp32 rounding of those
        # terms (a few 6e-8 |dy| gamma rstd) stays well under the bar's atol of 1e-6.
        u = u.view(G, n, F).sort(1).values + torch.arange(n, dtype=torch.float32)[None, :, None] * 4.0
        u = u.reshape(G * n, F)
    u = u + torch.arange(G).repeat_interleave(n)[:, None] * 0.7  # the groups differ in mean
    return dict(u=u.contiguous(), gamma=torch.rand(F, generator=g) + 0.5, beta=torch.randn(F, generator=g),
                rm=torch.randn(F, generator=g), rv=torch.rand(F, generator=g) + 0.5,
                dy=torch.randn(G * n, F, generator=g).contiguous())


def run_bn_groups(x, n, G, F, ld):
    pad = lambda t: torch.cat([t, torch.full((t.shape[0], ld - F), NAN)], 1).to(DEV)  # noqa: E731
    u, dy = pad(x["u"]), pad(x["dy"])
    gamma, beta, rm, rv = (x[k].clone().to(DEV) for k in ("gamma", "beta", "rm", "rv"))
    nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
    y, du = torch.full((G * n, ld), NAN, device=DEV), torch.full((G * n, ld), NAN, device=DEV)
    xhat, rstd = torch.full((G * n, F), NAN, device=DEV), torch.full((G, F), NAN, device=DEV)
    dg, db = torch.full((F,), NAN, device=DEV), torch.full((F,), NAN, device=DEV)
    call("es_bn1d_groups_fwd", ptr(u), ld, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), 0.1, 1e-5, ptr(y), ld,
         ptr(xhat), ptr(rstd), n, G, F, S())
    call("es_bn1d_groups_bwd", ptr(dy), ld, ptr(xhat), ptr(rstd), ptr(gamma), ptr(du), ld, ptr(dg), ptr(db), n, G, F, S())
    return {k: v.cpu() for k, v in dict(y=y, xhat=xhat, rstd=rstd, rm=rm, rv=rv, nbt=nbt, du=du, dg=dg, db=db).items()}


def run_bn_single_per_group(x, n, G, F, ld):
    """es_bn1d_fwd / es_bn1d_bwd once per group, in group order, on the same running buffers."""
    pad = lambda t: torch.cat([t, torch.full((t.shape[0], ld - F), NAN)], 1).to(DEV)  # noqa: E731
    u, dy = pad(x["u"]), pad(x["dy"])
    gamma, beta, rm, rv = (x[k].clone().to(DEV) for k in ("gamma", "beta", "rm", "rv"))
    nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
    y, du = torch.full((G * n, ld), NAN, device=DEV), torch.full((G * n, ld), NAN, device=DEV)
    xhat, rstd = torch.full((G * n, F), NAN, device=DEV), torch.full((G, F), NAN, device=DEV)
    dg, db = torch.full((G, F), NAN, device=DEV), torch.full((G, F), NAN, device=DEV)
    for g in range(G):
        r = slice(g * n, (g + 1) * n)
        call("es_bn1d_fwd", ptr(u[r]), ld, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), 0.1, 1e-5, 1, ptr(y[r]),
             ld, ptr(xhat[r]), ptr(rstd[g]), n, F, S())
        call("es_bn1d_bwd", ptr(dy[r]), ld, ptr(xhat[r]), ptr(rstd[g]), ptr(gamma), ptr(du[r]), ld, ptr(dg[g]),
             ptr(db[g]), n, F, S())
    return {k: v.cpu() for k, v in dict(y=y, xhat=xhat, rstd=rstd, rm=rm, rv=rv, nbt=nbt, du=du, dg=dg, db=db).items()}


@pytest.mark.parametrize("F", [1, 5, 96])
@pytest.mark.parametrize("n", [2, 3, 257])
@pytest.mark.parametrize("G", [1, 2, 3])
def test_bn1d_groups(G, n, F):
    ld = F + (3 if F == 5 else 0)  # a padded row stride
    x = bn_inputs(n, G, F, seed=100 * G + n + F)
    o = run_bn_groups(x, n, G, F, ld)
    s = run_bn_single_per_group(x, n, G, F, ld)
    # order check (G = 1: the identity with es_bn1d_fwd / es_bn1d_bwd): bit for bit
    for k in ("y", "du"):
        assert torch.equal(bits(o[k][:, :F]), bits(s[k][:, :F])), k
        assert torch.isnan(o[k][:, F:]).all()
    for k in ("xhat", "rstd", "rm", "rv"):
        assert torch.equal(bits(o[k]), bits(s[k])), k
    assert int(o["nbt"]) == 5 + G == int(s["nbt"])
    dg, db = s["dg"][0].clone(), s["db"][0].clone()
    for g in range(1, G):  # the groups' sums added in group order, in fp32
        dg, db = dg + s["dg"][g], db + s["db"][g]
    assert torch.equal(bits(o["dg"]), bits(dg)) and torch.equal(bits(o["db"]), bits(db))
    # float64
    d = {k: v.double() for k, v in x.items()}
    y, xhat, rstd, rm, rv = er.bn_groups(d["u"], d["gamma"], d["beta"], d["rm"], d["rv"], n, G)
    du, dgr, dbr = er.bn_groups_bwd(d["dy"], xhat, rstd, d["gamma"], n, G)
    # dU is judged on the kernel's own saved xhat / rstd as well as on the float64 ones: at n = 2 a feature's
    # two rows can lie close together, and xhat is then ill-conditioned in its input
    du_own, _, _ = er.bn_groups_bwd(d["dy"], o["xhat"].double(), o["rstd"].double(), d["gamma"], n, G)
    for k, got, ref in (("y", o["y"][:, :F], y), ("xhat", o["xhat"], xhat), ("rstd", o["rstd"], rstd),
                        ("running_mean", o["rm"], rm), ("running_var", o["rv"], rv), ("dU", o["du"][:, :F], du),
                        ("dU_own", o["du"][:, :F], du_own), ("dgamma", o["dg"], dgr), ("dbeta", o["db"], dbr)):
        err = ((got.double() - ref).abs() / (1e-6 + 1e-4 * ref.abs())).max().item()
        print({"G": G, "n": n, "F": F, "what": k, "bar_units": err})
    for k, got, ref in (("y", o["y"][:, :F], y), ("xhat", o["xhat"], xhat), ("rstd", o["rstd"], rstd),
                        ("running_mean", o["rm"], rm), ("running_var", o["rv"], rv), ("dU", o["du"][:, :F], du),
                        ("dgamma", o["dg"], dgr), ("dbeta", o["db"], dbr)):
        torch.testing.assert_close(got, ref.float(), msg=lambda m, k=k: f"{k}: {m}", **BAR)


def test_bn1d_groups_status_codes():
    lib = _lib.load()
    n, G, F = 4, 2, 8
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    T = dict(u=z(G * n, F), ldu=F, gamma=z(F), beta=z(F), rm=z(F), rv=z(F) + 1, nbt=None, mom=0.1, eps=1e-5,
             y=z(G * n, F), ldy=F, xhat=z(G * n, F), rstd=z(G, F), n=n, G=G, F=F)
    fo = ("u", "ldu", "gamma", "beta", "rm", "rv", "nbt", "mom", "eps", "y", "ldy", "xhat", "rstd", "n", "G", "F")
    B = dict(dy=z(G * n, F), lddy=F, xhat=T["xhat"], rstd=T["rstd"], gamma=T["gamma"], du=z(G * n, F), lddu=F, dg=z(F),
             db=z(F), n=n, G=G, F=F)
    bo = ("dy", "lddy", "xhat", "rstd", "gamma", "du", "lddu", "dg", "db", "n", "G", "F")
    arg = lambda v: ptr(v) if torch.is_tensor(v) else v  # noqa: E731
    fwd = lambda **kw: lib.es_bn1d_groups_fwd(*[arg({**T, **kw}[k]) for k in fo], S())  # noqa: E731
    bwd = lambda **kw: lib.es_bn1d_groups_bwd(*[arg({**B, **kw}[k]) for k in bo], S())  # noqa: E731
    assert fwd() == 0 and bwd() == 0  # num_batches_tracked is nullable
    for bad in (dict(n=1), dict(n=0), dict(G=0), dict(F=0), dict(ldu=F - 1), dict(ldy=F - 1)):
        assert fwd(**bad) == -1, bad
    for bad in (dict(n=1), dict(G=0), dict(F=0), dict(lddy=F - 1), dict(lddu=F - 1)):
        assert bwd(**bad) == -1, bad
    for bad in ("u", "gamma", "beta", "rm", "rv", "y", "xhat", "rstd"):
        assert fwd(**{bad: None}) == -2, bad
    for bad in ("dy", "xhat", "rstd", "gamma", "du", "dg", "db"):
        assert bwd(**{bad: None}) == -2, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- es_ezbm_ce_fwd_bwd
def ce_inputs(n, C, seed):
    """Logits [2n, C] with row scales from 1 to 80 / max|randn| (the largest entries reach +-80), targets with
    t == td on every third row."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(2 * n, C, generator=g)
    sc = 1 + 15 * torch.rand(2 * n, 1, generator=g)
    lg = lg * sc
    lg[0] = lg[0] / lg[0].abs().max() * 80.0
    lg[-1] = lg[-1] / lg[-1].abs().max() * 80.0
    t = torch.randint(0, C, (n,), generator=g)
    td = torch.randint(0, C, (n,), generator=g)
    td[::3] = t[::3]
    if n > 1:
        td[1] = (t[1] + 1) % C
    return lg.contiguous(), t, td


def run_ce(lg, t, td, n, C, ld, lam_c, gs):
    lp = torch.full((2 * n, ld), NAN)
    lp[:, :C] = lg
    lp = lp.to(DEV)
    dl, out = torch.full((2 * n, ld), NAN, device=DEV), torch.full((3,), NAN, device=DEV)
    a, b = t.to(DEV), td.to(DEV)  # held until the call returns
    call("es_ezbm_ce_fwd_bwd", ptr(lp), ld, ptr(a), ptr(b), n, C, lam_c, gs, ptr(dl), ld, ptr(out), S())
    torch.cuda.synchronize()
    return dl.cpu(), out.cpu()


@pytest.mark.parametrize("C", [2, 6, 23, 64])
@pytest.mark.parametrize("n", [1, 7, 300])
def test_ezbm_ce_vs_float64_autograd(n, C):
    ld = C + (5 if C == 23 else 0)  # a padded stride
    lam_c, gs = 4.0, 0.75
    lg, t, td = ce_inputs(n, C, seed=n + C)
    assert lg.abs().max().item() >= 79.9 and (t == td).any()
    leaf = lg.double().requires_grad_(True)
    loss, l_o, l_s = er.ezbm_loss(leaf, t, td, lam_c)
    (gs * loss).backward()
    dl, out = run_ce(lg, t, td, n, C, ld, lam_c, gs)
    dl2, out2 = run_ce(lg, t, td, n, C, ld, lam_c, gs)
    ref = [loss.item(), l_o.item(), l_s.item()]
    print({"n": n, "C": C, "out": out.tolist(), "ref": ref,
           "grad_bar_units": ((dl[:, :C].double() - leaf.grad).abs() / (1e-6 + 1e-4 * leaf.grad.abs())).max().item()})
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-5)
    torch.testing.assert_close(dl[:, :C], leaf.grad.float(), **BAR)
    assert torch.isnan(dl[:, C:]).all()
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(dl[:, :C]), bits(dl2[:, :C]))  # same bits again
    # t == td: the plain one-hot row
    i = int(torch.nonzero(t == td)[0, 0])
    one = gs * lam_c * (torch.softmax(lg[n + i].double(), 0) - torch.nn.functional.one_hot(t[i], C)) / n
    torch.testing.assert_close(dl[n + i, :C], one.float(), **BAR)


def test_ezbm_ce_out_of_range_target_and_status_codes():
    n, C = 7, 6
    lg, t, td = ce_inputs(n, C, seed=4)
    t2, td2 = t.clone(), td.clone()
    t2[2], td2[5] = C, -1
    dl, out = run_ce(lg, t2, td2, n, C, C, 4.0, 1.0)
    assert torch.isnan(out[0]) and torch.isnan(out[1])
    assert torch.all(dl[[2, n + 2, 5, n + 5]] == 0)
    good, _ = run_ce(lg, t, td, n, C, C, 4.0, 1.0)
    rest = [i for i in range(2 * n) if i not in (2, n + 2, 5, n + 5)]
    assert torch.equal(bits(dl[rest]), bits(good[rest]))  # the other rows are untouched by it
    lib = _lib.load()
    l, dl_, o = lg.to(DEV), torch.zeros(2 * n, C, device=DEV), torch.zeros(3, device=DEV)
    a, b = t.to(DEV), td.to(DEV)
    f = lambda **kw: lib.es_ezbm_ce_fwd_bwd(*[{**dict(l=ptr(l), ldl=C, t=ptr(a), td=ptr(b), n=n, C=C, lc=4.0,  # noqa: E731
                                                     gs=1.0, dl=ptr(dl_), lddl=C, o=ptr(o), s=S()), **kw}[k]
                                              for k in ("l", "ldl", "t", "td", "n", "C", "lc", "gs", "dl", "lddl", "o", "s")])
    assert f() == 0
    for bad in (dict(n=0), dict(n=-2), dict(C=0), dict(ldl=C - 1), dict(lddl=C - 1)):
        assert f(**bad) == -1, bad
    for bad in ("l", "t", "td", "dl", "o"):
        assert f(**{bad: None}) == -2, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- trainer
class _DS:
    df = None

    def __init__(self, cls_num, length):
        self._cls, self._len = list(cls_num), length

    def get_cls_num_list(self):
        return self._cls

    def __len__(self):
        return self._len


class _DL:
    def __init__(self, items, cls_num=None, length=0):
        self.items = items
        self.dataset = _DS(cls_num, length) if cls_num is not None else type("D", (), {"df": None})()

    def __iter__(self):
        return iter(self.items)

    def __len__(self):
        return len(self.items)


def _cfg(C, bs, mu, expansion="balance", lam_c=4, save_cp=".", name="vit_tiny_test", sch="const"):
    from endossl.utils import AttrDict
    return AttrDict(
        DATA=AttrDict(BATCH_SIZE=bs, MU=mu, IMG_SIZE=64, TARGET_NAME="target"),
        MODEL=AttrDict(NAME=name, NUM_CLASSES=C, MARGIN="None", IS_TRIPLET=True, LOW_DIM=16, PRE_TRAIN_PATH="None"),
        TRAIN=AttrDict(IS_SSL=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, CLS_WEIGHT=False, THRES=0.5,
                       LAMBDA_C=lam_c, EPOCHS=1, WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8,
                       SCH_NAME=sch, FREQ_EVAL=1, EXPANSION=expansion, SAVE_CP=save_cp))


def _head_only_model(D, C):
    """An embedding-head model whose `fc` has the fixture's sizes (D = 32, F = 8).  The ViT kernels need
    D % 128 == 0, so this trunk cannot run -- stage 2 never runs it: the step reads the bank and `fc` only."""
    from endossl.comatch_model import NativeViTEmb
    from endossl.vit import ViTConfig

    class HeadCfg(ViTConfig):
        def __init__(self):
            self.img_size, self.patch, self.dim, self.depth, self.heads = 32, 16, D, 1, 1
            self.num_classes, self.eps, self.head, self.low_dim = C, 1e-6, "emb", 8
            self.hidden, self.grid, self.np, self.T = 4 * D, 2, 4, 5
    return NativeViTEmb(HeadCfg(), seed=0)


@pytest.mark.parametrize("exp", ["balance", "reverse"])
def test_stage2_step_vs_reference_fixture(exp):
    """Two stage-2 steps with the fixture's rows and Dropout mask replayed, against the reference's float64 run."""
    from endossl.ezbm import EZBM
    fx = er.load_fixture(exp)
    n, C, D = fx["n"], 6, 32
    m = _head_only_model(D, C)
    sd = {"fc." + k: torch.as_tensor(fx[f"init/{k}"]) for k in er.FC_KEYS + er.BN_KEYS}
    missing = m.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    tr = EZBM(m, opt_func="Adam", lr=fx["lr"], device=DEV)
    tr.get_dataloader(_DL([], cls_num=fx["cls_num_list"].tolist(), length=40), None)
    tr.get_config(_cfg(C, 4, 3, expansion=exp, lam_c=fx["lambda_c"]))
    tr.set_bank(fx["mem"].to(DEV), fx["mem_y"].to(DEV))
    frozen0 = {k: v.detach().clone() for k, v in m.state_dict().items() if not k.startswith("fc.")}
    rec, checks = {}, []
    for s in range(fx["steps"]):
        o = tr.step_stage_2(idx=fx[f"s{s}/idx"], dual=fx[f"s{s}/dual"], drop_keep=fx[f"s{s}/keep"])
        torch.cuda.synchronize()
        assert torch.equal(o["lam"].cpu(), fx[f"s{s}/lam"])
        assert torch.equal(o["idx"].cpu(), fx[f"s{s}/idx"]) and torch.equal(o["dual"].cpu(), fx[f"s{s}/dual"])
        lg = o["logits"].cpu()
        checks += [(f"s{s}/logits_o", lg[:n], fx[f"s{s}/logits_o"]), (f"s{s}/logits_s", lg[n:], fx[f"s{s}/logits_s"])]
        for k in ("l_o", "l_s", "loss"):
            rec[f"s{s}/{k}"] = [o[k].item(), fx[f"s{s}/{k}"], abs(o[k].item() - fx[f"s{s}/{k}"]) / abs(fx[f"s{s}/{k}"])]
        sd1, esd = m.state_dict(), tr.ema_model.ema.state_dict()
        for k in er.FC_KEYS:
            g = m.engine().view(m.flat_grad, "fc." + k).cpu().view(fx[f"s{s}/grad/{k}"].shape)
            checks.append((f"s{s}/grad/{k}", g, fx[f"s{s}/grad/{k}"]))
        for k in er.FC_KEYS + er.BN_KEYS[:2]:
            checks.append((f"s{s}/param/{k}", sd1["fc." + k].cpu(), fx[f"s{s}/param/{k}"]))
            checks.append((f"s{s}/ema/{k}", esd["fc." + k].cpu(), fx[f"s{s}/ema/{k}"]))
        assert int(sd1["fc.3.num_batches_tracked"]) == 2 * (s + 1)
    for name, got, ref in checks:
        rec[name] = ((got.double() - ref).abs() / (1e-6 + 1e-4 * ref.abs())).max().item()
    print({"expansion": exp, "losses [hip, ref, rel err]": {k: v for k, v in rec.items() if isinstance(v, list)},
           "bar_units": {k: round(v, 4) for k, v in rec.items() if not isinstance(v, list)}})
    for k, v in rec.items():
        if isinstance(v, list):
            assert v[2] <= 1e-5, (k, v)
    for name, got, ref in checks:
        torch.testing.assert_close(got, ref.float(), msg=lambda msg, name=name: f"{name}: {msg}", **BAR)
    # the frozen parameters (trunk, head_emb): bit for bit what they were
    for k, v in m.state_dict().items():
        if not k.startswith("fc."):
            assert torch.equal(v, frozen0[k]), k
    with pytest.raises(ValueError, match="more than 1 value"):
        tr.step_stage_2(n=1)


def test_cls_ln_bwd_repeats_its_bits():
    """The final norm's dgamma / dbeta in the embedding-head backward: summed in a fixed order, so the triplet step
    that stage 1 is held to repeats its own bits (they were folded with fp32 atomics over 4-image workgroups)."""
    n, T, D = 203, 1, 128
    g = torch.Generator().manual_seed(0)
    dy, xhat = torch.randn(n, D, generator=g).to(DEV), torch.randn(n, D, generator=g).to(DEV)
    gam, rstd = (torch.rand(D, generator=g) + 0.5).to(DEV), (torch.rand(n, generator=g) + 0.5).to(DEV)
    runs = []
    for _ in range(4):
        dx = torch.zeros(n * T, D, device=DEV)
        dg, db = torch.full((D,), 0.25, device=DEV), torch.full((D,), -0.5, device=DEV)
        call("es_cls_ln_bwd", ptr(dy), D, ptr(gam), ptr(xhat), ptr(rstd), ptr(dx), D, T, ptr(dg), ptr(db), n, D, S())
        runs.append((dx.cpu(), dg.cpu(), db.cpu()))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(bits(a), bits(b))
    torch.testing.assert_close(runs[0][1], 0.25 + (dy.double() * xhat.double()).sum(0).float().cpu(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(runs[0][2], -0.5 + dy.double().sum(0).float().cpu(), rtol=1e-4, atol=1e-4)


def _triplet_batches(k, bs, C, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for j in range(k):
        imgs = tuple(torch.randn(bs, 3, 64, 64, generator=g) for _ in range(3))
        ys = tuple((torch.arange(bs) + j + r) % C for r in range(3))  # every class among the anchors of an epoch
        out.append((imgs, ys))
    return out


def test_stage1_is_the_triplet_step_plus_the_bank():
    """Three stage-1 steps: every output and every parameter after each step bit-identical to SupLearning's
    triplet step from the same seed; the bank = the anchors' fts and targets in step order; reset by an epoch."""
    from endossl.build import build_model
    from endossl.ezbm import EZBM
    from endossl.supervised import SupLearning
    bs, C = 4, 23
    cfg = _cfg(C, bs, 1, lam_c=2.0)
    batches = _triplet_batches(3, bs, C, seed=5)
    ma, mb = build_model(cfg, seed=4), build_model(cfg, seed=4)
    sup = SupLearning(ma, opt_func="Adam", lr=1e-3, device=DEV)
    sup.get_dataloader(_DL(batches), None)
    sup.get_config(cfg)
    ez = EZBM(mb, opt_func="Adam", lr=1e-3, device=DEV)
    ez.get_dataloader(_DL(batches, cls_num=list(range(C, 0, -1)), length=0), None)
    ez.get_config(cfg)
    fts, ys = [], []
    for batch in batches:
        a, b = sup.step(batch), ez.step_stage_1(batch)
        torch.cuda.synchronize()
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(bits(a[k].float()), bits(b[k].float())), k
        diff = {k: int((v != mb.state_dict()[k]).sum()) for k, v in ma.state_dict().items()}
        print({"step": len(fts), "parameter tensors that differ": {k: v for k, v in diff.items() if v}})
        assert torch.equal(bits(ma.flat), bits(mb.flat))
        assert torch.equal(bits(sup.ema_model.ema.flat), bits(ez.ema_model.ema.flat))
        for x, y in zip(ma.bn_buffers(), mb.bn_buffers()):
            assert torch.equal(x, y)
        fts.append(a["fts"][:bs].clone())
        ys.append(batch[1][0])
    bx, by = ez.bank()
    assert tuple(bx.shape) == (3 * bs, ma.cfg.dim) and by.dtype == torch.int64
    assert torch.equal(bits(bx), bits(torch.cat(fts))) and torch.equal(by.cpu(), torch.cat(ys))
    # a second epoch resets the bank: it holds that epoch's two batches only
    ez.train_dl = _DL(batches[:2], cls_num=list(range(C, 0, -1)))
    meter = ez.train_one_stage_1(1)
    bx, by = ez.bank()
    assert tuple(bx.shape) == (2 * bs, ma.cfg.dim) and torch.equal(by.cpu(), torch.cat(ys[:2]))
    assert np.isfinite(meter.avg) and meter.count == 2 * bs


class _Meter:
    def __init__(self, avg):
        self.avg = avg


def _fit_once(save_dir, script):
    from endossl.build import build_model
    from endossl.ezbm import EZBM
    bs, C = 4, 3
    os.makedirs(save_dir, exist_ok=True)
    # stage 2: 4 rows a step, 2 steps over 8 bank rows; a scheduler whose state the checkpoint stores
    cfg = _cfg(C, 2, 2, expansion="reverse", save_cp=save_dir, sch="cosine")
    batches = _triplet_batches(2, bs, C, seed=8)
    g = torch.Generator().manual_seed(9)
    valid = [(torch.randn(3, 3, 64, 64, generator=g), torch.randint(0, C, (3,), generator=g)) for _ in range(2)]
    m = build_model(cfg, seed=2)
    tr = EZBM(m, opt_func="Adam", lr=1e-3, device=DEV)
    tr.STAGE1_EPOCHS = tr.STAGE2_EPOCHS = 2
    tr.get_dataloader(_DL(batches, cls_num=[9, 5, 2], length=8), _DL(valid))
    tr.get_config(cfg)
    snap, evals = {}, []
    real_eval, real_setup = tr.evaluate_one, tr.setup_stage_2

    def scripted_eval(*a, **kw):
        loss, metric = real_eval(*a, **kw)  # the real evaluation runs; its figures are replaced by the script's
        assert np.isfinite(loss.avg) and "macro/f1" in metric
        v = script[len(evals)]
        evals.append(v)
        return _Meter(v[0]), {"macro/f1": v[1]}

    def setup():
        snap["end_of_stage_1"] = {k: v.detach().clone() for k, v in m.state_dict().items()}
        snap["ema"] = tr.ema_model.ema.flat.detach().clone()
        real_setup()
    tr.evaluate_one, tr.setup_stage_2 = scripted_eval, setup
    tr.fit()
    torch.cuda.synchronize()
    return tr, m, snap, evals


# (valid loss, macro f1) per evaluation: stage 1 epochs 0 and 1, stage 2 epochs 0 and 1
_SCRIPT = [(1.0, 0.30), (0.9, 0.40), (0.8, 0.50), (0.85, 0.45)]


def test_fit_end_to_end(tmp_path):
    from endossl.build import build_model
    from endossl.ezbm import EZBM
    tr, m, snap, evals = _fit_once(str(tmp_path / "a"), _SCRIPT)
    assert len(evals) == 4 and tr.stage == 2
    assert (tr.best_valid_loss, tr.best_valid_score) == (0.8, 0.50)  # better in both at stage 2's first evaluation
    sd = m.state_dict()
    changed = []
    for k, v in sd.items():
        if k.startswith("fc."):
            changed.append(k)
            assert not torch.equal(v, snap["end_of_stage_1"][k]), f"{k} did not change in stage 2"
        else:  # trunk and head_emb: frozen, bit for bit
            assert torch.equal(bits(v), bits(snap["end_of_stage_1"][k])), k
    assert {"fc.0.weight", "fc.4.bias", "fc.3.running_mean", "fc.3.running_var", "fc.3.num_batches_tracked"} <= set(changed)
    assert any(k.startswith("head_emb.") for k in sd) and any(k.startswith("blocks.") for k in sd)
    assert not torch.equal(tr.ema_model.ema.flat, snap["ema"])  # the EMA moved
    assert int(sd["fc.3.num_batches_tracked"]) == 4 + 2 * 2 * 2  # 4 stage-1 steps; 2 epochs x 2 steps x 2 groups
    # checkpoints: stage 1 saves nothing; stage 2 saved once (its epoch 0), and it loads into a fresh trainer
    files = sorted(glob.glob(os.path.join(str(tmp_path / "a"), "*.pth")))
    assert len(files) == 1 and files[0].endswith("_epoch_0.pth")
    ck = torch.load(files[0], map_location="cpu", weights_only=True)
    assert sum(len(g["params"]) for g in ck["optimizer"]["param_groups"]) == 6  # fc's parameters only
    fresh = EZBM(build_model(tr.config, seed=11), opt_func="Adam", lr=1e-3, device=DEV)
    fresh.get_dataloader(tr.train_dl, tr.valid_dl)
    fresh.get_config(tr.config)
    fresh.load_checkpoint(files[0], is_train=True)
    assert fresh.stage == 2 and fresh.epoch_start == 0 and fresh.optimizer.step_count == 2
    for k, v in fresh.model.state_dict().items():
        assert torch.equal(v.cpu(), ck["model_state_dict"][k]), k
    for k, v in fresh.ema_model.ema.state_dict().items():
        assert torch.equal(v.cpu(), ck["ema_state_dict"][k]), k
    # the same seeds again: the same bits
    tr2, m2, _, _ = _fit_once(str(tmp_path / "b"), _SCRIPT)
    assert torch.equal(bits(m2.flat), bits(m.flat))
    assert torch.equal(bits(tr2.ema_model.ema.flat), bits(tr.ema_model.ema.flat))
    for x, y in zip(m.bn_buffers(), m2.bn_buffers()):
        assert torch.equal(x, y)
