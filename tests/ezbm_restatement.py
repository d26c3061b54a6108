"""Restatement of the EZBM stage-2 device work (include/endossl.h "EZBM stage 2"; the reference's
EZBM.train_one_stage_2, code/ezbm.py:133-182, and EmbFeatEZBM, code/dataset.py:135-175), shared by
test_ezbm_cpu.py -- which pins it to the reference-generated fixtures tests/golden/ezbm_stage2_*.npz in float64
-- and test_gpu_ezbm.py, which holds the kernels to it.

  sample()        the sampler in numpy uint64: the splitmix64 counter hash and the integer / CDF draws, exact
  mix()           the batch X = [mem[idx]; lam mem[idx] + (1 - lam) mem[dual]] as torch forms it in fp32
  bn_groups()     BatchNorm1d (train) over G groups of n rows, running buffers updated in group order
  bn_groups_bwd() its backward from the saved xhat / rstd (closed form)
  ezbm_loss()     l_o + lambda_c l_s on the [2n, C] logits
  head_step()     fc(inputs), fc(mix), the loss and autograd's gradients, in the dtype asked for
  adam_ema()      torch.optim.Adam's step and ModelEMA's blend on a dict of tensors
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FC_KEYS = ("0.weight", "0.bias", "3.weight", "3.bias", "4.weight", "4.bias")
BN_KEYS = ("3.running_mean", "3.running_var", "3.num_batches_tracked")
DROP_P, BN_MOMENTUM, BN_EPS = 0.2, 0.1, 1e-5
_M64 = (1 << 64) - 1


def splitmix(seed, counter):
    """The hash of es_dropout_keep at element `counter` (Python ints, mod 2^64)."""
    z = (seed + 0x9E3779B97F4A7C15 * (counter + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def splitmix_np(seed, counters):
    """The same on a numpy uint64 array of counters (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        c = np.asarray(counters, dtype=np.uint64)
        z = np.uint64(seed & _M64) + np.uint64(0x9E3779B97F4A7C15) * (c + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample(n, C, cls_off, cls_idx, cdf, seed, offset):
    """(idx, dual, row class, dual class) int64 [n] of a drawn batch: row i uses counters offset + 4i + k."""
    cls_off, cls_idx = np.asarray(cls_off, dtype=np.int64), np.asarray(cls_idx, dtype=np.int64)
    cdf = np.asarray(cdf, dtype=np.float32)
    base = np.uint64(offset & _M64) + np.uint64(4) * np.arange(n, dtype=np.uint64)
    z = [splitmix_np(seed, base + np.uint64(k)) >> np.uint64(40) for k in range(4)]  # the top 24 bits

    def member(c, zz):
        m = (cls_off[c + 1] - cls_off[c]).astype(np.uint64)
        return cls_idx[cls_off[c] + ((zz * m) >> np.uint64(24)).astype(np.int64)]

    ca = ((z[0] * np.uint64(C)) >> np.uint64(24)).astype(np.int64)
    u = z[2].astype(np.float32) * np.float32(2.0 ** -24)
    below = u[:, None] < cdf[None, :]
    cb = np.where(below.any(1), below.argmax(1), C - 1).astype(np.int64)
    return member(ca, z[1]), member(cb, z[3]), ca, cb


def mix(mem, idx, dual, lam):
    """X [2n, D] fp32 on the CPU, torch's own fp32 expression (two rounded products, one rounded sum)."""
    a, b = mem[idx.long()].float(), mem[dual.long()].float()
    lt = lam.float().view(-1, 1)
    return torch.cat([a, lt * a + (1 - lt) * b])


def bn_groups(u, gamma, beta, rm, rv, n, G, momentum=BN_MOMENTUM, eps=BN_EPS):
    """(y, xhat, rstd [G, F], running_mean, running_var) in u's dtype; the running buffers after the G updates."""
    ys, xs, rs = [], [], []
    rm, rv = rm.clone(), rv.clone()
    for g in range(G):
        ug = u[g * n:(g + 1) * n]
        mean, var = ug.mean(0), ug.var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + eps)
        xh = (ug - mean) * rstd
        xs.append(xh)
        ys.append(xh * gamma + beta)
        rs.append(rstd)
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * n / (n - 1)
    return torch.cat(ys), torch.cat(xs), torch.stack(rs), rm, rv


def bn_groups_bwd(dy, xhat, rstd, gamma, n, G):
    """(dU, dgamma, dbeta) from the saved xhat / rstd: dU per group from its own sums, the parameter gradients
    summed over the groups."""
    dus, dg, db = [], 0, 0
    for g in range(G):
        d, xh = dy[g * n:(g + 1) * n], xhat[g * n:(g + 1) * n]
        s1, s2 = d.sum(0), (d * xh).sum(0)
        dus.append(gamma * rstd[g] * (d - s1 / n - xh * (s2 / n)))
        dg, db = dg + s2, db + s1
    return torch.cat(dus), dg, db


def ezbm_loss(logits, t, td, lambda_c):
    """(loss, l_o, l_s) of code/ezbm.py:165-167 on logits [2n, C] (rows [0, n) = outputs_o, [n, 2n) = outputs_s)."""
    n = t.shape[0]
    o, s = logits[:n], logits[n:]
    l_o = F.cross_entropy(o, t)
    l_s = 0.5 * F.cross_entropy(s, t) + 0.5 * F.cross_entropy(s, td)
    return l_o + lambda_c * l_s, l_o, l_s


def head_fwd(p, bufs, x, keep, n, G=2):
    """build_head(is_complex=True) on x [G n, D] with a replayed Dropout keep-mask: logits and the running
    buffers after it.  p: {"0.weight", ...}; bufs: {"3.running_mean", "3.running_var"}."""
    u = torch.relu(F.linear(x, p["0.weight"], p["0.bias"])) * (keep.to(x.dtype) * (1.0 / (1.0 - DROP_P)))
    y, _, _, rm, rv = bn_groups(u, p["3.weight"], p["3.bias"], bufs["3.running_mean"], bufs["3.running_var"], n, G)
    return F.linear(y, p["4.weight"], p["4.bias"]), rm.detach(), rv.detach()


def head_step(params, bufs, x, keep, t, td, lambda_c, dtype=torch.float64):
    """One stage-2 forward / backward in `dtype` on the batch x [2n, D]: dict with logits, loss, l_o, l_s, grads
    {key: tensor}, running_mean, running_var."""
    p = {k: params[k].detach().to(dtype).clone().requires_grad_(True) for k in FC_KEYS}
    b = {k: bufs[k].detach().to(dtype) for k in BN_KEYS[:2]}
    logits, rm, rv = head_fwd(p, b, x.to(dtype), keep, t.shape[0])
    loss, l_o, l_s = ezbm_loss(logits, t, td, lambda_c)
    loss.backward()
    return {"logits": logits.detach(), "loss": loss.detach(), "l_o": l_o.detach(), "l_s": l_s.detach(),
            "grads": {k: p[k].grad for k in FC_KEYS}, "running_mean": rm, "running_var": rv}


def adam_ema(params, grads, state, ema, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, decay=0.999):
    """torch.optim.Adam (weight_decay 0) on every key of `params`, then ModelEMA's d e + (1 - d) p; in place."""
    state["step"] = state.get("step", 0) + 1
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** state["step"], 1 - b2 ** state["step"]
    for k, g in grads.items():
        m = state.setdefault("m/" + k, torch.zeros_like(g))
        v = state.setdefault("v/" + k, torch.zeros_like(g))
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        params[k] = params[k] - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
        ema[k] = decay * ema[k] + (1 - decay) * params[k]


def load_fixture(expansion):
    d = np.load(os.path.join(GOLDEN, f"ezbm_stage2_{expansion}.npz"), allow_pickle=False)
    fx = {k: (torch.from_numpy(d[k]) if d[k].ndim else d[k].item()) for k in d.files}
    fx["expansion"] = str(fx["expansion"])
    return fx
