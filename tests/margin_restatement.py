"""Torch restatement of es_margin_softmax_fwd_bwd's contract (include/endossl.h; the reference's
AngularPenaltySMLoss.forward, code/loss.py:228-266), shared by test_margin_cpu.py -- which pins it to the
reference-generated fixtures tests/golden/margin_*.npz in float64 -- and test_gpu_margin.py, which holds the
kernel to it where no fixture exists.  It runs in the dtype of its inputs; gradients come from autograd.

It differs from the reference's text in one place only: log(exp(num) + sum_j exp(s z_j)) is a logsumexp, which
is the same number wherever the reference's exp is finite and stays finite beyond it.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("cosface", "arcface", "sphereface", "acloss")
VARIANTS = ("plain", "weighted", "masked")
DEFAULTS = {"arcface": (30.0, 0.3), "sphereface": (30.0, 1.35), "cosface": (30.0, 0.4), "acloss": (30.0, 0.3)}


def g_theta(a, k=0.3):
    s1 = (1 + math.exp(-math.pi / 2.0 / k)) / (1 - math.exp(-math.pi / 2.0 / k))
    e = torch.exp(a / k - math.pi / 2.0 / k)
    return s1 * (1 - e) / (1 + e)


def numerator(t, kind, s, m, eps):
    if kind == "cosface":
        return s * (t - m)
    th = torch.acos(torch.clamp(t, -1. + eps, 1 - eps))
    if kind == "arcface":
        return s * torch.cos(th + m)
    if kind == "sphereface":
        return s * torch.cos(m * th)
    if kind == "acloss":
        return s * g_theta(th + m)
    raise ValueError(kind)


def row_losses(x, W, y, kind, s, m, eps=1e-7, b=None, w=None, mask=None):
    """-L_i per row (w and mask applied)."""
    z = F.linear(F.normalize(x, p=2, dim=1), W, b)  # W as it is: the reference never normalises it
    num = numerator(z.gather(1, y[:, None])[:, 0], kind, s, m, eps)
    v = (s * z).scatter(1, y[:, None], num[:, None])
    L = num - torch.logsumexp(v, dim=1)
    if w is not None:
        L = w[y] * L
    if mask is not None:
        L = L * mask
    return -L


def margin_loss(x, W, y, kind, s, m, eps=1e-7, b=None, w=None, mask=None):
    return row_losses(x, W, y, kind, s, m, eps, b, w, mask).mean()


def loss_and_grads(x, W, y, kind, s, m, eps=1e-7, b=None, w=None, mask=None, dtype=torch.float64):
    """(loss, dx, dW, db or None, row losses) of the plain mean, computed in `dtype`."""
    c = lambda t: None if t is None else t.detach().to(dtype)  # noqa: E731
    xi, Wi = c(x).requires_grad_(True), c(W).requires_grad_(True)
    bi = None if b is None else c(b).requires_grad_(True)
    rows = row_losses(xi, Wi, y, kind, s, m, eps, bi, c(w), c(mask))
    loss = rows.mean()
    loss.backward()
    return loss.detach(), xi.grad, Wi.grad, None if bi is None else bi.grad, rows.detach()


def load_fixture(kind, variant):
    d = np.load(os.path.join(GOLDEN, f"margin_{kind}_{variant}.npz"), allow_pickle=False)
    fx = {k: d[k] for k in d.files}
    fx["kind"] = str(fx["kind"])
    for k in ("s", "m", "eps"):
        fx[k] = float(fx[k])
    for k in ("x", "W", "w", "mask", "y", "dx", "dW", "dx_f32", "dW_f32", "t"):
        fx[k] = torch.from_numpy(fx[k])
    for k in ("w", "mask"):
        if fx[k].numel() == 0:
            fx[k] = None
    return fx


def rel_errors(loss, dx, dW, fx):
    """(relative loss error, max |d - ref| / max |ref| for dx and dW) against the float64 fixture values."""
    rl = abs(float(loss) - float(fx["loss"])) / abs(float(fx["loss"]))
    ex = (dx.double() - fx["dx"]).abs().max().item() / fx["dx"].abs().max().item()
    ew = (dW.double() - fx["dW"]).abs().max().item() / fx["dW"].abs().max().item()
    return rl, ex, ew
