"""Generate the angular-margin fixtures under tests/golden/ by running the REFERENCE loss class.

Test infrastructure only; like make_golden.py it runs where the read-only reference tree is mounted and
refuses to run anywhere else.  The reference's `loss.AngularPenaltySMLoss` (code/loss.py:194-266) is imported
(never copied) and run as it stands -- its weight "normalisation" loop that changes nothing, its literal
exp / log -- on a bias-free nn.Linear(64, 23), once in float64 and once in float32; the gradients are its
autograd's.  What is committed is DATA only: arrays, loadable with allow_pickle=False.

Every file (n = 24, F = 64, C = 23) holds
  kind, s, m, eps      the loss type and its constants (the reference's defaults for the kind)
  x [n, F], W [C, F]   fp32 inputs (the float64 run casts the same values up)
  y [n] int64, w [C] fp32 class weights, mask [n] fp32     (w / mask of length 0: absent)
  loss, dx, dW         the reference in float64
  loss_f32, dx_f32, dW_f32   the reference in float32
  t [n]                the float64 target logits x^ . W[y]
Files
  margin_<kind>_plain.npz / _weighted.npz / _masked.npz   "smooth": rows of W have norm <= 0.95 (no s z near
      the fp32 exp overflow) and every |t| <= 0.9 (acos' stays moderate); asserted below.  _masked carries
      class weights too, and a mask with both 0s and 1s.
  margin_<kind>_clamped.npz   rows CLAMPED_HI / CLAMPED_LO (also stored, as `clamped`) have their target's
      weight row scaled to norm 1.6 and x aligned with +- it, so t > 1 / t < -1: the clamp gives their target
      logit a zero gradient for every kind but cosface.

Usage (from the repo root):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_margin.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

import make_golden

OUT = os.path.dirname(os.path.abspath(__file__))
N, F, C = 24, 64, 23
KINDS = ("cosface", "arcface", "sphereface", "acloss")
CLAMPED_HI, CLAMPED_LO = (2, 9, 17), (5, 20)


def _import_reference_loss():
    if not os.path.isdir(make_golden.REF):
        raise SystemExit("make_golden_margin.py needs the reference tree (build container only)")
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    sys.path.insert(0, make_golden.REF)
    import loss as ref_loss
    return ref_loss


class _Cfg:
    def __init__(self, kind):
        self.MODEL = type("M", (), {"MARGIN": kind})()


def _inputs(seed, clamped):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(C, F, generator=g)
    W = W / W.norm(dim=1, keepdim=True) * torch.empty(C, 1).uniform_(0.5, 0.95, generator=g)
    y = torch.randint(0, C, (N,), generator=g)
    y[0], y[1] = 0, C - 1
    alpha = torch.empty(N, 1).uniform_(-0.5, 1.0, generator=g)
    if clamped:
        # each clamped row gets a class of its own, whose weight row is scaled up
        own = torch.randperm(C, generator=g)[:len(CLAMPED_HI + CLAMPED_LO)]
        for r, c in zip(CLAMPED_HI + CLAMPED_LO, own.tolist()):
            y[r] = c
            W[c] *= 1.6 / W[c].norm()
            alpha[r] = 4.0 if r in CLAMPED_HI else -4.0
        free = [c for c in range(C) if c not in own.tolist()]
        for r in range(N):
            if r not in CLAMPED_HI + CLAMPED_LO and int(y[r]) in own.tolist():
                y[r] = free[r % len(free)]
    Wy = W[y] / W[y].norm(dim=1, keepdim=True)
    x = torch.randn(N, F, generator=g) + alpha * (F ** 0.5) * Wy
    x = x * torch.empty(N, 1).uniform_(0.3, 3.0, generator=g)  # the loss must not depend on |x|
    w = torch.empty(C).uniform_(0.4, 2.5, generator=g)
    mask = (torch.arange(N) % 3 != 1).float()
    return x.float(), W.float(), y, w.float(), mask


def _run(ref_loss, kind, x, W, y, w, mask, dtype):
    fc = nn.Linear(F, C, bias=False).to(dtype)
    with torch.no_grad():
        fc.weight.copy_(W.to(dtype))
    xi = x.to(dtype).clone().requires_grad_(True)
    crit = ref_loss.AngularPenaltySMLoss(_Cfg(kind))
    loss = crit(xi, y, fc, cls_weight=None if w is None else w.to(dtype), use_mask=mask is not None,
                mask=None if mask is None else mask.to(dtype))
    assert loss.dtype == dtype
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(xi.grad).all() and torch.isfinite(fc.weight.grad).all()
    return crit, loss.detach().numpy(), xi.grad.numpy(), fc.weight.grad.numpy()


def main():
    ref_loss = _import_reference_loss()
    empty = np.zeros(0, dtype=np.float32)
    for ki, kind in enumerate(KINDS):
        for vi, variant in enumerate(("plain", "weighted", "masked", "clamped")):
            x, W, y, w, mask = _inputs(100 + 10 * ki + vi, clamped=variant == "clamped")
            use_w = w if variant in ("weighted", "masked") else None
            use_m = mask if variant == "masked" else None
            t = (torch.nn.functional.normalize(x.double(), dim=1) * W.double()[y]).sum(1)
            rows = np.array(CLAMPED_HI + CLAMPED_LO, dtype=np.int64) if variant == "clamped" else np.zeros(0, np.int64)
            if variant == "clamped":
                assert (t[list(CLAMPED_HI)] > 1.05).all() and (t[list(CLAMPED_LO)] < -1.05).all(), t
                rest = [r for r in range(N) if r not in CLAMPED_HI + CLAMPED_LO]
                assert (t[rest].abs() <= 0.9).all(), t
                assert (W.norm(dim=1) <= 1.6001).all()
            else:
                assert (t.abs() <= 0.9).all(), t
                assert (W.norm(dim=1) <= 0.95 + 1e-6).all()
                assert t.abs().max() > 0.5  # the margin terms are exercised away from 0 as well
            crit, l64, dx64, dW64 = _run(ref_loss, kind, x, W, y, use_w, use_m, torch.float64)
            _, l32, dx32, dW32 = _run(ref_loss, kind, x, W, y, use_w, use_m, torch.float32)
            np.savez_compressed(
                os.path.join(OUT, f"margin_{kind}_{variant}.npz"), kind=np.array(kind), s=np.float64(crit.s),
                m=np.float64(crit.m), eps=np.float64(crit.eps), x=x.numpy(), W=W.numpy(), y=y.numpy(),
                w=use_w.numpy() if use_w is not None else empty, mask=use_m.numpy() if use_m is not None else empty,
                loss=l64, dx=dx64, dW=dW64, loss_f32=l32, dx_f32=dx32, dW_f32=dW32, t=t.numpy(), clamped=rows)
            print(f"margin_{kind}_{variant}: loss {float(l64):.6f} (f32 {float(l32):.6f}) max|t| {float(t.abs().max()):.3f}")


if __name__ == "__main__":
    main()
