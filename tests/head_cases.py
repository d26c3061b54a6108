"""Cases and float64 restatements for the loss kernels (csrc/losses.hip: consistency, poly-CE, weighted CE) and the
CoMatch head / step kernels (csrc/comatch.hip).  torch on the CPU only: test_head_cases_cpu.py pins the restatements
to oracle/ref.py and torch.nn.functional and checks every claim the case tables make (exact-integer bounds,
decidable rows, kept contrastive columns) from the reference alone; test_gpu_head_exact.py runs the kernels on them.

Every restatement is written from the formulas in the two kernel files' headers: float64 forward values, gradients
by float64 autograd.  The gradient outputs follow each entry point's convention (grad_scale times the derivative of
the SUM of the row losses, or of out[0] for the weighted CE), as the header in include/endossl.h states it.
"""
import numpy as np
import torch
import torch.nn.functional as F

NAN = float("nan")
F64 = torch.float64
DECIDE = 1e-5  # a label needs top1 - top2 > DECIDE, a mask |score - threshold| > DECIDE (float64)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def logits(n, C, seed, scale=6.0):
    """Rows of uneven sharpness: randn(n, C) * rand(n, 1) * scale."""
    g = gen(seed)
    return torch.randn(n, C, generator=g) * torch.rand(n, 1, generator=g) * scale


LARGE_SHAPES = [(257, 23), (600, 64)]


def large_logits(n, C, seed):
    """randn * 50: |l| reaches about 200, where a literal exp overflows fp32."""
    return torch.randn(n, C, generator=gen(seed)) * 50


def unit(t):
    return t / t.norm(dim=1, keepdim=True)


def bar_units(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 passes."""
    want = want.double()
    return ((got.double() - want).abs() / (atol + rtol * want.abs())).max().item()


# ====================================================================================== losses.hip
LOSS_SHAPES = [(n, C) for n in (1, 255, 256, 257, 600) for C in (1, 2, 23, 64)]
LOSS_VAL = dict(rtol=1e-5, atol=1e-6)
LOSS_GRAD = dict(rtol=1e-4, atol=1e-7)
INVALID_TARGETS = (-1, "C", 2 ** 31, 2 ** 32 + 3)


def loss_tau(n, C):
    """The two thresholds alternate over the shape table."""
    return (0.7, 0.95)[LOSS_SHAPES.index((n, C)) % 2]


def two_sided(n, C):
    """Whether a case can have rows on both sides of a threshold at all: one row cannot, and with one class the
    probability is 1 in every row.  The smallest shape the two-sided requirement was stated for has 17 rows."""
    return n >= 16 and C >= 2


def consistency_case(n, C, seed=None, scale=6.0):
    """Weak / strong logits; where there is room, row 1's unique maximum sits in the last class."""
    seed = 100 * n + C if seed is None else seed
    lw, ls = logits(n, C, seed, scale), logits(n, C, seed + 1, scale)
    if n >= 3 and C >= 2:
        lw[1, C - 1] = lw[1].max() + 1.0
    return lw, ls


def consistency_ties_case():
    """C = 5: rows whose two (or more) largest weak logits are equal, and a unique maximum in the last class.
    Returns lw, ls and the labels 'first index on ties' gives."""
    lw = torch.tensor([[1.0, 1.0, 0.0, 0.0, -1.0], [0.0, 2.0, 2.0, 1.0, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0],
                       [-3.0, 0.5, 0.25, 0.5, 0.0], [0.0, 1.0, 2.0, 3.0, 4.0], [-1.0, -2.0, -1.5, -1.0, -1.0]])
    ls = logits(6, 5, 77)
    return lw, ls, torch.tensor([0, 1, 0, 1, 4, 0])


def consistency64(lw, ls, tau, grad_scale):
    """p = softmax(lw); (pmax, idx) = max(p) [first index on ties]; mask = pmax >= tau;
    rows = CE(ls, idx) * mask; loss = mean(rows); dls = grad_scale * d(sum rows) / d ls."""
    lw, ls = lw.double(), ls.double().clone().requires_grad_(True)
    p = torch.softmax(lw, -1)
    idx = lw.argmax(-1)  # the first of equal maxima; softmax is monotone, so this is max(p)'s index
    pmax = p.gather(1, idx.view(-1, 1)).squeeze(1)
    top = p.topk(min(2, p.shape[1]), -1).values
    gap = top[:, 0] - top[:, 1] if p.shape[1] > 1 else torch.ones(p.shape[0], dtype=F64)
    mask = (pmax >= tau).double()
    ce = torch.logsumexp(ls, -1) - ls.gather(1, idx.view(-1, 1)).squeeze(1)
    rows = ce * mask
    (grad_scale * rows.sum()).backward()
    return {"idx": idx, "pmax": pmax, "gap": gap, "mask": mask, "rows": rows.detach(), "loss": rows.mean().item(),
            "mask_mean": mask.mean().item(), "dls": ls.grad, "label_ok": gap > DECIDE,
            "mask_ok": (pmax - tau).abs() > DECIDE}


def consistency_rows_fp32_error(ls, r):
    """The worst absolute error of the per-row loss when the kernel's formula, max + log(sum exp(l - max)) - l[idx],
    is evaluated in plain fp32 torch on the CPU, against the float64 rows of r = consistency64(...): at |l| ~ 200 one
    ulp of the log-sum-exp is 1.5e-5, which a small row loss cannot hide."""
    ls = ls.float()
    mx = ls.max(1).values
    lse = mx + torch.log(torch.exp(ls - mx[:, None]).sum(1))
    rows = (lse - ls.gather(1, r["idx"].view(-1, 1)).squeeze(1)) * r["mask"].float()
    return (rows.double() - r["rows"]).abs().max().item(), bar_units(rows, r["rows"], **LOSS_VAL)


def targets_case(n, C, seed):
    """Targets holding class 0 and class C - 1 (where n allows both), weights with exactly C entries."""
    g = gen(seed)
    y = torch.randint(0, C, (n,), generator=g)
    y[0] = 0
    y[-1] = C - 1
    w = torch.empty(C).uniform_(0.4, 2.5, generator=g)
    return y, w


def _valid(y, C):
    return (y >= 0) & (y < C)


def poly64(l, y, w, eps, grad_scale):
    """loss = mean_i(w[y_i] CE_i + eps (1 - p_i[y_i])); dl = grad_scale * d(sum_i ...) / dl.  A row whose target is
    outside [0, C) makes the loss NaN and has a zero gradient; the other rows' gradients do not depend on it."""
    n, C = l.shape
    l = l.double().clone().requires_grad_(True)
    ok = _valid(y, C)
    yy = torch.where(ok, y, torch.zeros_like(y))
    lse = torch.logsumexp(l, -1)
    ly = l.gather(1, yy.view(-1, 1)).squeeze(1)
    wy = torch.ones(n, dtype=F64) if w is None else w.double()[yy]
    rows = (wy * (lse - ly) + eps * (1 - torch.exp(ly - lse))) * ok.double()
    (grad_scale * rows.sum()).backward()
    loss = rows.mean().item() if bool(ok.all()) else NAN
    return {"loss": loss, "dl": l.grad, "valid": ok}


def ce_weighted64(l, y, w, grad_scale, wsum=None):
    """out = sum_i w[y_i] CE_i / W, W = sum_i w[y_i] (or the given global sum); dl = grad_scale * d out / dl.
    An invalid target makes W, the loss and the other rows' gradients NaN; its own row's gradient is zero."""
    n, C = l.shape
    l = l.double().clone().requires_grad_(True)
    ok = _valid(y, C)
    yy = torch.where(ok, y, torch.zeros_like(y))
    wy = (torch.ones(n, dtype=F64) if w is None else w.double()[yy]) * ok.double()
    W = wy.sum() if wsum is None else torch.as_tensor(float(wsum), dtype=F64)
    ce = torch.logsumexp(l, -1) - l.gather(1, yy.view(-1, 1)).squeeze(1)
    out = (wy * ce).sum() / W
    (grad_scale * out).backward()
    return {"loss": out.item() if bool(ok.all()) else NAN, "dl": l.grad, "wsum": wy.sum().item() if bool(ok.all())
            else NAN, "valid": ok}


# ====================================================================================== comatch.hip: heads
CM = dict(rtol=1e-4, atol=1e-6)  # the CoMatch kernels' bar against float64

DENSE_SHAPES = [(1, 1, 1), (17, 65, 63), (17, 65, 64), (33, 5, 257), (16, 2048, 64), (3, 64, 2048)]
DENSE_SLOPE, DENSE_KEEP_SCALE = 0.5, 1.25


def dense_case(n, K, N, seed=None):
    """Integers in {-2..2} and a keep mask of about 80% ones; dX0 is the integer prior accumulate_dx adds onto."""
    g = gen(1000 * n + 10 * K + N if seed is None else seed)
    r = lambda *s: torch.randint(-2, 3, s, generator=g).float()  # noqa: E731
    return {"X": r(n, K), "W": r(N, K), "b": r(N), "dY": r(n, N), "dX0": r(n, K),
            "keep": (torch.rand(n, N, generator=g) >= 0.2).to(torch.uint8)}


def dense64(c, act, with_keep, slope=DENSE_SLOPE, keep_scale=DENSE_KEEP_SCALE, bias=True):
    """Y = act(X W^T + b) (* keep * keep_scale); dX, dW, db by autograd."""
    X, W, b = (c[k].double().clone().requires_grad_(True) for k in ("X", "W", "b"))
    pre = X @ W.t() + (b if bias else 0.0)
    y = pre if act == 0 else (F.relu(pre) if act == 1 else F.leaky_relu(pre, slope))
    if with_keep:
        y = y * (c["keep"].double() * keep_scale)
    y.backward(c["dY"].double())
    return {"Y": y.detach(), "dX": X.grad, "dW": W.grad, "db": b.grad if bias else None, "pre": pre.detach()}


def dense_magnitude(c, with_keep, slope=DENSE_SLOPE, keep_scale=DENSE_KEEP_SCALE):
    """An upper bound, in units of 1/8, of every partial sum any summation order can meet in the forward, dX (with
    the prior), dW and db: each must stay below 2^24 for the fp32 result to be exact."""
    X, W, b, dY = (c[k].double().abs() for k in ("X", "W", "b", "dY"))
    ks = keep_scale if with_keep else 1.0
    fwd = (X @ W.t() + b).max().item() * ks
    dpre = dY * ks  # |act'| <= 1
    dx = (dpre @ W + c["dX0"].double().abs()).max().item()
    dw = (dpre.t() @ X).max().item()
    db = dpre.sum(0).max().item()
    return 8.0 * max(fwd, dx, dw, db)


BN_SHAPES = [(1, 3), (2, 1), (255, 4), (256, 4), (257, 4)]
BN_MOMENTUM, BN_EPS = 0.1, 1e-5


def bn_case(n, Fe, seed=None):
    """dY leans on U and has a non-zero mean, so that neither dbeta = sum dY nor dgamma = sum dY xhat is a sum
    that cancels to near zero."""
    g = gen(50 * n + Fe if seed is None else seed)
    U = torch.randn(n, Fe, generator=g) * 1.7 + 0.4
    return {"U": U, "gamma": 1 + 0.1 * torch.randn(Fe, generator=g), "beta": 0.1 * torch.randn(Fe, generator=g),
            "rm": torch.randn(Fe, generator=g) * 0.1, "rv": 1 + torch.rand(Fe, generator=g),
            "dY": 0.5 + 0.5 * torch.randn(n, Fe, generator=g) + 0.4 * U}


def bn64(c, momentum=BN_MOMENTUM, eps=BN_EPS):
    """nn.BatchNorm1d in training mode: batch mean / biased variance, running buffers with the unbiased variance
    (the biased one when n = 1, where torch refuses to run), xhat / rstd, and the backward."""
    U, g, b = (c[k].double().clone().requires_grad_(True) for k in ("U", "gamma", "beta"))
    n = U.shape[0]
    mean = U.mean(0)
    var = ((U - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (U - mean) * rstd
    y = xhat * g + b
    y.backward(c["dY"].double())
    unb = var * n / (n - 1) if n > 1 else var
    return {"Y": y.detach(), "xhat": xhat.detach(), "rstd": rstd.detach(),
            "rm": (1 - momentum) * c["rm"].double() + momentum * mean.detach(),
            "rv": (1 - momentum) * c["rv"].double() + momentum * unb.detach(),
            "dU": U.grad, "dgamma": g.grad, "dbeta": b.grad}


def bn_eval64(c, rm, rv, eps=BN_EPS):
    return (c["U"].double() - rm.double()) / torch.sqrt(rv.double() + eps) * c["gamma"].double() + c["beta"].double()


L2_SHAPES = [(1, 1), (4, 63), (5, 64), (5, 65), (3, 256), (2, 300)]


def l2_exact_case(n, L, seed=None):
    """Rows with exactly 4^m non-zero entries of +-2^j (one j per row): the norm is 2^(m + j) and every Z entry
    +-2^-m, in any summation order."""
    g = gen(7 * n + L if seed is None else seed)
    V = torch.zeros(n, L)
    for i in range(n):
        ms = [m for m in range(5) if 4 ** m <= L]
        m = ms[int(torch.randint(0, len(ms), (1,), generator=g))] if i else ms[-1]  # row 0: the most entries
        j = int(torch.randint(-3, 4, (1,), generator=g))
        pos = torch.randperm(L, generator=g)[:4 ** m]
        sign = torch.randint(0, 2, (4 ** m,), generator=g).float() * 2 - 1
        V[i, pos] = sign * 2.0 ** j
    return V


def l2_case(n, L, seed=None):
    """Random rows kept away from a zero norm (L = 1 included)."""
    g = gen(11 * n + L if seed is None else seed)
    V = torch.randn(n, L, generator=g)
    V = V + 0.5 * torch.sign(V)
    return V, torch.randn(n, L, generator=g)


def l2norm64(V, dZ=None):
    V = V.double().clone().requires_grad_(True)
    nrm = V.pow(2).sum(1, keepdim=True).sqrt()
    Z = V / nrm
    if dZ is not None:
        Z.backward(dZ.double())
    return {"Z": Z.detach(), "norm": nrm.detach().squeeze(1), "dV": V.grad}


# ====================================================================================== comatch.hip: step
PSEUDO_BASE = dict(nu=17, C=23, L=40, Q=300)
PSEUDO_VARY = {"C": (1, 16, 17, 32), "L": (1, 3, 4, 64), "nu": (1, 16, 65), "Q": (1, 15, 16, 17, 128, 129)}
PSEUDO_CASES = [dict(PSEUDO_BASE)] + [dict(PSEUDO_BASE, **{k: v}) for k, vs in PSEUDO_VARY.items() for v in vs]
PSEUDO_T, PSEUDO_ALPHA, PSEUDO_THRES = 0.2, 0.9, 0.6
# (cap, len, pos): the entries wrap through slot 3; the full ring; the newest entry alone
PSEUDO_RINGS = [(4, 3, 1), (4, 4, 2), (4, 1, 0)]


def case_id(d):
    return "-".join(f"{k}{v}" for k, v in d.items())


def pseudo_case(nu, C, L, Q, cap=4, hlen=3, pos=1, seed=None):
    """The history ring's unused slots hold NaN: they must not be read."""
    seed = nu * 1000003 + C * 10007 + L * 101 + Q + 13 * cap + 5 * hlen + pos if seed is None else seed
    g = gen(seed)
    lw = torch.randn(nu, C, generator=g) * torch.rand(nu, 1, generator=g) * 6
    zw = unit(torch.randn(nu, L, generator=g))
    bf = unit(torch.randn(Q, L, generator=g))
    bp = torch.softmax(torch.randn(Q, C, generator=g) * 3, -1)
    hist = torch.full((cap, C), NAN)
    for j in range(hlen):
        hist[(pos - j) % cap] = torch.softmax(torch.randn(C, generator=g), -1)
    return {"lw": lw, "zw": zw, "bf": bf, "bp": bp, "hist": hist, "cap": cap, "len": hlen, "pos": pos}


def pseudo64(c, given, T=PSEUDO_T, alpha=PSEUDO_ALPHA, thres=PSEUDO_THRES):
    """softmax -> distribution alignment over the ring's len newest entries (hist[pos] is this batch's mean unless
    given) -> memory smoothing against the bank -> score / first-index label / mask (>= thres)."""
    p = torch.softmax(c["lw"].double(), 1)
    hist = c["hist"].double().clone()
    if not given:
        hist[c["pos"]] = p.mean(0)
    used = [(c["pos"] - j) % c["cap"] for j in range(c["len"])]
    p = p / hist[used].mean(0)
    porig = p / p.sum(1, keepdim=True)
    A = torch.exp(c["zw"].double() @ c["bf"].double().t() / T)
    A = A / A.sum(1, keepdim=True)
    probs = alpha * porig + (1 - alpha) * A @ c["bp"].double()
    score, label = probs.max(1)
    top = probs.topk(min(2, probs.shape[1]), 1).values
    gap = top[:, 0] - top[:, 1] if probs.shape[1] > 1 else torch.ones(probs.shape[0], dtype=F64)
    return {"entry": hist[c["pos"]], "porig": porig, "probs": probs, "score": score, "label": label,
            "mask": (score >= thres).double(), "label_ok": gap > DECIDE, "mask_ok": (score - thres).abs() > DECIDE}


def pseudo_ties_case():
    """hist_given with a uniform entry, C = 4, alpha = 1: equal weak logits pass through identical arithmetic, so
    the smoothed probabilities tie exactly and the label is the first index."""
    c = pseudo_case(4, 4, 8, 20, cap=1, hlen=1, pos=0, seed=5)
    c["lw"] = torch.tensor([[1.0, 1.0, 0.0, 0.0], [0.0, 2.0, 2.0, 1.0], [3.0, 3.0, 3.0, 3.0], [0.0, -1.0, 0.5, 0.5]])
    c["hist"] = torch.full((1, 4), 0.25)
    return c, torch.tensor([0, 1, 0, 2])


def colmean64(lw):
    return torch.softmax(lw.double(), 1).mean(0)


COLMEAN_SHAPES = [(n, C) for n in (1, 257) for C in (1, 23, 32)]

CONTRAST_T = 0.2
CONTRAST_SIZES = ([dict(nu=nu, L=64, C=23) for nu in (1, 2, 255, 256, 257)] +
                  [dict(nu=37, L=L, C=23) for L in (1, 40, 65, 128)] + [dict(nu=37, L=64, C=1)])


def contrast_case(nu, L, C, seed=None):
    g = gen(nu * 1009 + L * 31 + C if seed is None else seed)
    z0, z1 = unit(torch.randn(nu, L, generator=g)), unit(torch.randn(nu, L, generator=g))
    probs = torch.softmax(torch.randn(nu, C, generator=g) * 4, -1) * 0.9
    return z0, z1, probs


def contrast_q(probs_r, probs_c, row_off):
    """Q before the threshold: p_i . p_j with the anchor's own column set to 1."""
    q = probs_r.double() @ probs_c.double().t()
    i = torch.arange(q.shape[0])
    q[i, row_off + i] = 1.0
    return q


def contrast_th(probs, lo=0.75, hi=0.85, want=None):
    """The threshold in [lo, hi] (a grid of 101 values, each as fp32) that lies farthest from every Q entry, so that
    no entry's keep / drop decision hangs on fp32 rounding.  want(kept_per_row) may narrow the choice."""
    q = contrast_q(probs, probs, 0)
    best, best_d = None, -1.0
    for th in torch.linspace(lo, hi, 101).tolist():
        th = float(torch.tensor(th, dtype=torch.float32))
        if want is not None and not want((q >= th).sum(1)):
            continue
        d = (q - th).abs().min().item()
        if d > best_d:
            best, best_d = th, d
    return best, best_d


def contrastive64(z0, z1, probs_r, probs_c, row_off, th, scale, loss_div, T=CONTRAST_T):
    """sim = exp(z0 z1^T / T), P = sim / rowsum; Q (own column 1, zero below th, row-normalised);
    L_i = -sum_j Q_ij log(P_ij + 1e-7); loss = sum_i L_i / loss_div; dz = scale * d(sum_i L_i) / dz."""
    a, b = z0.double().clone().requires_grad_(True), z1.double().clone().requires_grad_(True)
    sim = torch.exp(a @ b.t() / T)
    P = sim / sim.sum(1, keepdim=True)
    q = contrast_q(probs_r, probs_c, row_off)
    q = q * (q >= th).double()
    kept = (q > 0).sum(1)
    q = q / q.sum(1, keepdim=True)
    rows = -(torch.log(P + 1e-7) * q).sum(1)
    (scale * rows.sum()).backward()
    return {"loss": rows.sum().item() / loss_div, "dz0": a.grad, "dz1": b.grad, "kept": kept}


FOCAL_NU = (1, 255, 256, 257, 600)
FOCAL_GAMMA = (2.0, 1.0, 1.5, 3.0)


def focal_case(nu, C, seed=None):
    g = gen(nu * 17 + C if seed is None else seed)
    ls = torch.randn(nu, C, generator=g) * 3
    probs = torch.softmax(torch.randn(nu, C, generator=g) * 3, -1) * 0.9
    mask = (torch.rand(nu, generator=g) > 0.4).float()
    if nu >= 2:
        mask[0], mask[-1] = 0.0, 1.0
    return ls, probs, mask


def focal64(ls, probs, mask, gamma, scale):
    """logp = -mask sum_c log_softmax(l)_c p_c; L_i = (1 - e^-logp)^gamma logp; loss = mean; dls = scale d(sum)/dl."""
    l = ls.double().clone().requires_grad_(True)
    logp = -(F.log_softmax(l, 1) * probs.double()).sum(1) * mask.double()
    rows = (1 - torch.exp(-logp)) ** gamma * logp
    (scale * rows.sum()).backward()
    return {"loss": rows.mean().item(), "dls": l.grad, "rows": rows.detach()}


DROPOUT_N = (1, 255, 257, 4099)
DROPOUT_P = (0.0, 0.2, 0.999)


def dropout_keep_np(n, p, seed, offset=0):
    """The counter hash in uint64: splitmix64 of seed + golden * (offset + i + 1), u = top 24 bits / 2^24 as fp32,
    keep = u >= p (p as fp32)."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(offset) + i + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (u >= np.float32(p)).astype(np.uint8)
