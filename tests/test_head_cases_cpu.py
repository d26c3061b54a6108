"""tests/head_cases.py on the CPU: the float64 restatements against oracle/ref.py and torch.nn.functional, and every
claim the case tables make, from the reference alone -- the exact-integer cases stay below 2^24, at most 2% of a
case's rows are undecidable and both sides of each threshold are populated, the contrastive thresholds keep clear of
every Q entry, the l2norm rows have power-of-two norms, the dropout hash restates splitmix64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_cases as hc
from oracle import ref

F64 = torch.float64
CLOSE = dict(rtol=1e-12, atol=1e-14)


# ------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("n,C", [(257, 23), (37, 2), (5, 1)])
def test_consistency_restatement_vs_oracle(n, C):
    lw, ls = hc.consistency_case(n, C)
    tau = 0.7
    r = hc.consistency64(lw, ls, tau, 1.0 / n)
    x = ls.double().clone().requires_grad_(True)
    loss, mm, idx, mask = ref.consistency(lw.double(), x, tau)
    loss.backward()
    assert torch.equal(idx, r["idx"]) and torch.equal(mask.double(), r["mask"])
    assert abs(loss.item() - r["loss"]) <= 1e-12
    assert abs(mm.item() - r["mask_mean"]) <= 1e-7  # the oracle's mask mean is an fp32 tensor
    torch.testing.assert_close(x.grad, r["dls"], **CLOSE)


def test_consistency_ties_give_the_first_index():
    lw, ls, want = hc.consistency_ties_case()
    r = hc.consistency64(lw, ls, 0.0, 1.0)
    assert torch.equal(r["idx"], want)
    assert int(want[4]) == lw.shape[1] - 1  # a unique maximum in the last class
    p = torch.softmax(lw.double(), -1)
    assert torch.equal(torch.max(p, -1).indices, want)  # oracle/ref.py's torch.max agrees on the ties


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,C", [(257, 23), (37, 2), (5, 1), (600, 64)])
def test_poly_and_weighted_ce_restatements(n, C, weighted):
    l = hc.logits(n, C, 3 * n + C)
    y, w = hc.targets_case(n, C, n + C)
    w = w if weighted else None
    assert int(y[0]) == 0 and int(y[-1]) == C - 1
    x = l.double().clone().requires_grad_(True)
    loss = ref.poly_ce(x, y, None if w is None else w.double(), 2.0)
    loss.backward()
    r = hc.poly64(l, y, w, 2.0, 1.0 / n)
    assert abs(loss.item() - r["loss"]) <= 1e-12 * max(1.0, abs(loss.item()))
    torch.testing.assert_close(x.grad, r["dl"], **CLOSE)
    x = l.double().clone().requires_grad_(True)
    loss = F.cross_entropy(x, y, weight=None if w is None else w.double())
    (2.5 * loss).backward()
    r = hc.ce_weighted64(l, y, w, 2.5)
    assert abs(loss.item() - r["loss"]) <= 1e-12 * max(1.0, abs(loss.item()))
    torch.testing.assert_close(x.grad, r["dl"], **CLOSE)


@pytest.mark.parametrize("bad", hc.INVALID_TARGETS)
def test_invalid_targets_in_the_restatements(bad):
    n, C = 9, 23
    l = hc.logits(n, C, 4)
    y, w = hc.targets_case(n, C, 5)
    good = hc.poly64(l, y, w, 2.0, 1.0 / n)
    y2 = y.clone()
    y2[4] = C if bad == "C" else bad
    r = hc.poly64(l, y2, w, 2.0, 1.0 / n)
    rows = [i for i in range(n) if i != 4]
    assert np.isnan(r["loss"]) and torch.all(r["dl"][4] == 0) and torch.equal(r["dl"][rows], good["dl"][rows])
    r = hc.ce_weighted64(l, y2, w, 1.0)
    assert np.isnan(r["loss"]) and np.isnan(r["wsum"]) and torch.all(r["dl"][4] == 0)


def test_weighted_ce_global_form_adds_up():
    n, C = 37, 23
    l = hc.logits(n, C, 8)
    y, w = hc.targets_case(n, C, 9)
    full = hc.ce_weighted64(l, y, w, 1.0)
    a = hc.ce_weighted64(l[:20], y[:20], w, 1.0, wsum=full["wsum"])
    b = hc.ce_weighted64(l[20:], y[20:], w, 1.0, wsum=full["wsum"])
    assert abs(a["loss"] + b["loss"] - full["loss"]) <= 1e-12
    torch.testing.assert_close(torch.cat([a["dl"], b["dl"]]), full["dl"], **CLOSE)


@pytest.mark.parametrize("n,C", hc.LOSS_SHAPES)
def test_consistency_cases_are_decidable(n, C):
    lw, ls = hc.consistency_case(n, C)
    tau = hc.loss_tau(n, C)
    r = hc.consistency64(lw, ls, tau, 1.0 / n)
    assert (~r["label_ok"]).sum().item() <= 0.02 * n and (~r["mask_ok"]).sum().item() <= 0.02 * n
    if n >= 3 and C >= 2:
        assert int(r["idx"][1]) == C - 1
    if hc.two_sided(n, C):
        ok = r["mask_ok"]
        assert (r["mask"][ok] == 1).any() and (r["mask"][ok] == 0).any()


def test_large_logit_cases_overflow_a_literal_exp():
    for n, C in hc.LARGE_SHAPES:
        for seed in (n, n + 1):
            l = hc.large_logits(n, C, seed)
            assert l.abs().max().item() > 150 and not torch.isfinite(torch.exp(l)).all()
        r = hc.consistency64(hc.large_logits(n, C, n), hc.large_logits(n, C, n + 1), 0.95, 1.0 / n)
        assert np.isfinite(r["loss"]) and torch.isfinite(r["dls"]).all()
        assert (~r["label_ok"]).sum().item() <= 0.02 * n and (~r["mask_ok"]).sum().item() <= 0.02 * n


# ------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("n,K,N", hc.DENSE_SHAPES)
def test_dense_cases_are_exact_in_fp32(n, K, N, act):
    c = hc.dense_case(n, K, N)
    for with_keep in (False, True):
        assert hc.dense_magnitude(c, with_keep) < 2 ** 24
        r = hc.dense64(c, act, with_keep)
        for k in ("Y", "dX", "dW", "db"):
            v = r[k] * 8
            assert torch.equal(v, v.round()) and v.abs().max().item() < 2 ** 24, k
            assert torch.equal(r[k].float().double(), r[k]), k  # representable in fp32
    if n * N >= 1000:
        assert (r["pre"] == 0).any()  # exact-zero pre-activations: the derivative read off the stored output
    if n * N >= 60:
        assert 0.7 <= c["keep"].float().mean().item() <= 0.9


def test_activation_derivative_at_zero_matches_torch():
    """ReLU: 0 at 0; LeakyReLU: the slope at 0 -- what the kernel reads off a stored output that is not > 0."""
    x = torch.zeros(3, dtype=F64, requires_grad=True)
    F.relu(x).sum().backward()
    assert torch.all(x.grad == 0)
    x = torch.zeros(3, dtype=F64, requires_grad=True)
    F.leaky_relu(x, hc.DENSE_SLOPE).sum().backward()
    assert torch.all(x.grad == hc.DENSE_SLOPE)
    c = hc.dense_case(17, 65, 64)
    r = hc.dense64(c, 2, False)
    zero = r["pre"] == 0
    assert zero.any()
    # dX restated by hand with the slope at the zeros
    d = c["dY"].double() * torch.where(r["pre"] > 0, 1.0, hc.DENSE_SLOPE)
    assert torch.equal(d @ c["W"].double(), r["dX"])


# ------------------------------------------------------------------------------------------ BatchNorm1d
@pytest.mark.parametrize("n,Fe", hc.BN_SHAPES)
def test_bn_restatement_vs_functional(n, Fe):
    c = hc.bn_case(n, Fe)
    r = hc.bn64(c)
    if n == 1:  # torch refuses one row in training mode: var = 0, the running variance takes the biased value
        assert torch.all(r["xhat"] == 0) and torch.equal(r["rv"], 0.9 * c["rv"].double())
        torch.testing.assert_close(r["Y"], c["beta"].double().expand(1, Fe), **CLOSE)
        return
    U, g, b = (c[k].double().clone().requires_grad_(True) for k in ("U", "gamma", "beta"))
    rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
    y = F.batch_norm(U, rm, rv, g, b, training=True, momentum=hc.BN_MOMENTUM, eps=hc.BN_EPS)
    y.backward(c["dY"].double())
    tol = dict(rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(y.detach(), r["Y"], **tol)
    torch.testing.assert_close(rm, r["rm"], **tol)
    torch.testing.assert_close(rv, r["rv"], **tol)
    torch.testing.assert_close(U.grad, r["dU"], **tol)
    torch.testing.assert_close(g.grad, r["dgamma"], **tol)
    torch.testing.assert_close(b.grad, r["dbeta"], **tol)
    torch.testing.assert_close(F.batch_norm(c["U"].double(), rm, rv, c["gamma"].double(), c["beta"].double(),
                                            training=False, eps=hc.BN_EPS), hc.bn_eval64(c, rm, rv), **tol)
    # the parameter-gradient sums do not cancel to near zero
    dY, xh = c["dY"].double(), r["xhat"]
    if n >= 255:
        assert (r["dbeta"].abs() >= 0.05 * dY.abs().sum(0)).all()
        assert (r["dgamma"].abs() >= 0.05 * (dY * xh).abs().sum(0)).all()


# ------------------------------------------------------------------------------------------ l2norm
@pytest.mark.parametrize("n,L", hc.L2_SHAPES)
def test_l2_exact_rows_have_power_of_two_norms(n, L):
    V = hc.l2_exact_case(n, L)
    r = hc.l2norm64(V)
    nz = (V != 0).sum(1)
    assert all(int(k) in (1, 4, 16, 64, 256) for k in nz) and int(nz[0]) == max(k for k in (1, 4, 16, 64, 256) if k <= L)
    m, e = np.frexp(r["norm"].numpy())
    assert np.all(m == 0.5)  # a power of two
    assert torch.equal(r["Z"].float().double(), r["Z"]) and torch.equal(r["norm"].float().double(), r["norm"])
    assert (V.pow(2).sum(1) < 2 ** 24).all()
    Vr, dZ = hc.l2_case(n, L)
    assert hc.l2norm64(Vr)["norm"].min().item() >= 0.5
    z = F.normalize(Vr.double(), dim=1)
    torch.testing.assert_close(z, hc.l2norm64(Vr)["Z"], **CLOSE)


# ------------------------------------------------------------------------------------------ pseudo-labels
def _pseudo_checks(c, r, nu, C):
    assert (~r["label_ok"]).sum().item() <= 0.02 * nu and (~r["mask_ok"]).sum().item() <= 0.02 * nu
    if hc.two_sided(nu, C):
        ok = r["mask_ok"]
        assert (r["mask"][ok] == 1).any() and (r["mask"][ok] == 0).any()
    torch.testing.assert_close(r["probs"].sum(1), torch.ones(nu, dtype=F64), rtol=0, atol=1e-6)


@pytest.mark.parametrize("d", hc.PSEUDO_CASES, ids=hc.case_id)
def test_pseudo_cases_are_decidable(d):
    c = hc.pseudo_case(**d)
    _pseudo_checks(c, hc.pseudo64(c, given=False), d["nu"], d["C"])


@pytest.mark.parametrize("cap,hlen,pos", hc.PSEUDO_RINGS)
def test_pseudo_ring_cases(cap, hlen, pos):
    c = hc.pseudo_case(**hc.PSEUDO_BASE, cap=cap, hlen=hlen, pos=pos)
    used = sorted((pos - j) % cap for j in range(hlen))
    assert [i for i in range(cap) if not torch.isnan(c["hist"][i]).any()] == used
    if (cap, hlen, pos) == (4, 3, 1):
        assert used == [0, 1, 3]  # the entries wrap through slot 3; slot 2 stays poisoned
    for given in (False, True):
        r = hc.pseudo64(c, given=given)
        assert torch.isfinite(r["probs"]).all()
        _pseudo_checks(c, r, 17, 23)


def test_pseudo_ties_restatement():
    c, want = hc.pseudo_ties_case()
    r = hc.pseudo64(c, given=True, alpha=1.0)
    assert torch.equal(r["label"], want)
    torch.testing.assert_close(r["probs"], torch.softmax(c["lw"].double(), 1), **CLOSE)


def test_colmean_restatement():
    lw = hc.logits(257, 23, 3)
    torch.testing.assert_close(hc.colmean64(lw).sum(), torch.tensor(1.0, dtype=F64), **CLOSE)


# ------------------------------------------------------------------------------------------ contrastive
def _kept_spread(kept):
    return bool((kept == 1).any() and (kept >= 3).any())


@pytest.mark.parametrize("d", hc.CONTRAST_SIZES, ids=hc.case_id)
def test_contrast_thresholds_keep_clear_of_q(d):
    z0, z1, probs = hc.contrast_case(**d)
    th, clear = hc.contrast_th(probs)
    assert 0.75 <= th <= 0.85 + 1e-6 and clear > hc.DECIDE, (th, clear)
    r = hc.contrastive64(z0, z1, probs, probs, 0, th, 2.0 / d["nu"], d["nu"])
    assert (r["kept"] >= 1).all() and np.isfinite(r["loss"])
    r0 = hc.contrastive64(z0, z1, probs, probs, 0, 0.0, 2.0 / d["nu"], d["nu"])
    assert (r0["kept"] == d["nu"]).all()  # th = 0 keeps every column


def test_contrast_threshold_with_lone_and_crowded_rows():
    z0, z1, probs = hc.contrast_case(37, 64, 23)
    th, clear = hc.contrast_th(probs, 0.3, 0.7, want=_kept_spread)
    assert th is not None and clear > hc.DECIDE
    r = hc.contrastive64(z0, z1, probs, probs, 0, th, 2.0 / 37, 37)
    assert _kept_spread(r["kept"])


def test_contrast_shards_add_up():
    z0, z1, probs = hc.contrast_case(37, 64, 23)
    th, _ = hc.contrast_th(probs)
    full = hc.contrastive64(z0, z1, probs, probs, 0, th, 2.0 / 37, 37)
    parts = [hc.contrastive64(z0[o:o + k], z1, probs[o:o + k], probs, o, th, 2.0 / 37, 37) for o, k in ((0, 20), (20, 17))]
    assert abs(parts[0]["loss"] + parts[1]["loss"] - full["loss"]) <= 1e-12
    torch.testing.assert_close(torch.cat([p["dz0"] for p in parts]), full["dz0"], **CLOSE)
    torch.testing.assert_close(parts[0]["dz1"] + parts[1]["dz1"], full["dz1"], **CLOSE)


# ------------------------------------------------------------------------------------------ focal, dropout
@pytest.mark.parametrize("gamma", hc.FOCAL_GAMMA)
def test_focal_restatement(gamma):
    ls, probs, mask = hc.focal_case(257, 23)
    r = hc.focal64(ls, probs, mask, gamma, 2.0 / 257)
    off = mask == 0
    assert off.any() and (~off).any()
    assert torch.all(r["rows"][off] == 0) and torch.all(r["dls"][off] == 0) and torch.isfinite(r["dls"]).all()
    if gamma == 2.0:  # the kernel header's closed form of the gradient
        l = ls.double()
        logp = -(F.log_softmax(l, 1) * probs.double()).sum(1) * mask.double()
        q = torch.exp(-logp)
        dL = 2 * (1 - q) * q * logp + (1 - q) ** 2
        g = (2.0 / 257) * dL.view(-1, 1) * (-mask.double().view(-1, 1)) * (
            probs.double() - torch.softmax(l, 1) * probs.double().sum(1, keepdim=True))
        torch.testing.assert_close(g, r["dls"], rtol=1e-10, atol=1e-14)
    ls, probs, mask = hc.focal_case(5, 1)
    assert hc.focal64(ls, probs, mask, gamma, 1.0)["loss"] == 0.0  # one class: log_softmax = 0


def _splitmix_keep(i, p, seed, offset):
    M = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (offset + i + 1)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return 1 if np.float32(z >> 40) * np.float32(1.0 / 16777216.0) >= np.float32(p) else 0


def test_dropout_hash_restatement():
    for p in hc.DROPOUT_P:
        a = hc.dropout_keep_np(300, p, 7, 0)
        assert a.dtype == np.uint8 and a.tolist() == [_splitmix_keep(i, p, 7, 0) for i in range(300)]
    assert hc.dropout_keep_np(4099, 0.0, 7).all()
    frac = hc.dropout_keep_np(1 << 16, 0.2, 7).mean()
    assert abs(frac - 0.8) < 0.01
    base = hc.dropout_keep_np(4099 + 256, 0.2, 2 ** 63 + 11, 0)
    for k in (1, 256):
        assert np.array_equal(hc.dropout_keep_np(4099, 0.2, 2 ** 63 + 11, k), base[k:k + 4099])
    assert 0 < hc.dropout_keep_np(1 << 16, 0.999, 7).sum() < 200
