"""Selection-pattern inputs for the attention kernels (head dim 64, scale 1/8): softmax rows that are exactly
one-hot, or exactly (1/2, 1/2), so that every output of es_attn_fwd / es_attn_bwd / es_attn_cls_* is a bf16 number
known in closed form and the comparison is torch.equal, not a tolerance.  Shared by test_attn_patterns_cpu.py --
which holds the closed forms to float64 autograd of plain softmax attention -- and test_gpu_attention_exact.py, which
holds the kernels to them.  Torch only; everything is built on the CPU.

Layout as the kernels': qkv [n*T, 3*D] with column order [3][H][64], o / dout [n*T, D] with column h*64 + d,
lse / delta [n][H][T].

Why the patterns are exact.  fp32 exp reaches exact zero, denormals included, 104 nats below its argument's
maximum (exp2 at -150); both builders assert on their inputs that every unselected score lies at least MARGIN = 110
nats below the selected one(s).  The selected probabilities are then exp2(0) = 1 (two of them: the row sum is 2, a
power of two), every other one is 0 under any running maximum an online softmax can hold, and all remaining
arithmetic is on small integers and halves.
"""
import torch

HD = 64
SCALE = HD ** -0.5  # 1/8: a power of two
MARGIN = 110.0
# (n, T, H) of the GPU tests: one token; one / three / four tiles with a partial last one; four whole tiles; the 13-tile
# heads (197, and 208 with no partial tile); 16 tiles; the 37-tile kernels with masked tiles (300) and at T = 577
ONE_HOT_SHAPES = [(2, 1, 1), (3, 17, 2), (3, 40, 2), (2, 64, 1), (3, 197, 3), (2, 208, 2), (2, 250, 2), (1, 300, 1),
                  (2, 577, 3)]
TWO_HOT_SHAPES = [(3, 17, 2), (3, 40, 1), (2, 64, 2)]


def attention_ref(qkv, n, T, H, dtype=torch.float64):
    """Plain softmax attention of the kernels' layout in `dtype`: o [n*T, D], lse [n, H, T].  qkv may require grad."""
    D = H * HD
    q, k, v = qkv.to(dtype).view(n, T, 3, H, HD).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * SCALE
    lse = torch.logsumexp(s, -1)
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(n * T, D)
    return o, lse


def _pack(q, k, v):
    """[n, H, T, 64] x 3 -> qkv [n*T, 3*D] bf16 (every value here is a bf16 number: asserted)."""
    n, H, T, _ = q.shape
    x = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(n * T, 3 * H * HD)
    xb = x.to(torch.bfloat16)
    assert torch.equal(xb.double(), x.double())
    return xb


def _rows(t):
    """[n, H, T, 64] -> [n*T, D]"""
    n, H, T, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(n * T, H * HD)


def one_hot(n, T, H, seed=None, integer_v=False):
    """Per (image, head): keys k_j in {+-1}^64, a random permutation pi of the tokens, q_i = 64 k_pi(i).  Scores:
    512 at j = pi(i), at most 8 max_x elsewhere (max_x: the largest off-diagonal <k_i, k_j>); asserts
    (64 - max_x) * 8 >= MARGIN.  v: random bf16 (integer_v: integers in [-3, 3], with a dout of the same kind, so
    that dO.v - sum(dO * O) is exactly 0 in any summation order).

    Closed forms: o_i = v_pi(i), lse = 512; dV_pi(i) = dO_i, dQ = dK = 0; delta_i = sum_d dO_i O_i."""
    g = torch.Generator().manual_seed(T if seed is None else seed)
    k = (torch.randint(0, 2, (n, H, T, HD), generator=g) * 2 - 1).double()
    pi = torch.stack([torch.randperm(T, generator=g) for _ in range(n * H)]).view(n, H, T)
    idx = pi.unsqueeze(-1).expand(n, H, T, HD)
    q = 64.0 * k.gather(2, idx)
    if integer_v:
        v = torch.randint(-3, 4, (n, H, T, HD), generator=g).double()
        dout = torch.randint(-3, 4, (n, H, T, HD), generator=g).double()
    else:
        v = torch.randn(n, H, T, HD, generator=g).to(torch.bfloat16).double()
        dout = None
    gram = k @ k.transpose(-2, -1)
    off = gram - 2.0 * HD * torch.eye(T, dtype=gram.dtype)  # the diagonal (64) out of the way
    max_x = off.max().item() if T > 1 else float("-inf")
    margin = (HD - max_x) * 8.0
    assert margin >= MARGIN, (n, T, H, max_x)
    p = {"n": n, "T": T, "H": H, "pi": pi, "max_x": max_x, "margin": margin, "qkv": _pack(q, k, v),
         "o": _rows(v.gather(2, idx)).to(torch.bfloat16), "lse": 512.0}
    if integer_v:
        dv = torch.zeros_like(v).scatter_(2, idx, dout)  # dV[pi(i)] = dO[i]
        p["dout"] = _rows(dout).to(torch.bfloat16)
        p["dv"] = _rows(dv).to(torch.bfloat16)
        p["delta"] = (dout * v.gather(2, idx)).sum(-1).float()  # [n, H, T], integers
    return p


def hadamard64():
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < HD:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def two_hot(n, T, H, seed=None):
    """T <= 64.  Per (image, head): keys = rows 0 .. T-1 of the 64 x 64 Sylvester Hadamard matrix (mutually
    orthogonal), query i picks two distinct keys a_i != b_i (a = a random permutation, b = the same one rotated by one
    place: each key is picked exactly twice), q_i = 16 (k_a + k_b); v and dout in {-1, 0, 1}.  Scores: 128 at a and b,
    exactly 0 elsewhere, so P = (1/2, 1/2) exactly and lse = 128 + ln 2.

    Expected o and dqkv come from float64 autograd of plain softmax attention, rounded to bf16; the builder asserts
    that the rounding residual is below 1e-30 (every expected value is an integer-derived bf16 number, the residue
    being the float64 softmax's exp(-128))."""
    assert 2 <= T <= HD
    g = torch.Generator().manual_seed(1000 + T if seed is None else seed)
    had = hadamard64()
    k = had[:T].expand(n, H, T, HD).clone()
    a = torch.stack([torch.randperm(T, generator=g) for _ in range(n * H)]).view(n, H, T)
    b = torch.roll(a, 1, dims=-1)
    assert (a != b).all()
    ia, ib = (x.unsqueeze(-1).expand(n, H, T, HD) for x in (a, b))
    q = 16.0 * (k.gather(2, ia) + k.gather(2, ib))
    v = torch.randint(-1, 2, (n, H, T, HD), generator=g).double()
    dout = torch.randint(-1, 2, (n, H, T, HD), generator=g).double()
    s = (q @ k.transpose(-2, -1)) * SCALE
    sel = torch.zeros_like(s).scatter_(-1, a.unsqueeze(-1), 1.0).scatter_(-1, b.unsqueeze(-1), 1.0).bool()
    assert (s[sel] == 128.0).all() and (s[~sel] == 0.0).all() and 128.0 >= MARGIN
    assert (sel.sum(-1) == 2).all() and (sel.sum(-2) == 2).all()
    qkv = _pack(q, k, v)
    x = qkv.double().requires_grad_(True)
    o, lse = attention_ref(x, n, T, H)
    o.backward(_rows(dout))
    exp = {}
    for name, t in (("o", o.detach()), ("dqkv", x.grad)):
        tb = t.to(torch.bfloat16)
        assert (tb.double() - t).abs().max().item() < 1e-30, name
        exp[name] = tb
    return {"n": n, "T": T, "H": H, "a": a, "b": b, "qkv": qkv, "dout": _rows(dout).to(torch.bfloat16), "o": exp["o"],
            "dqkv": exp["dqkv"], "lse": lse.detach(), "delta": (_rows(dout) * o.detach()).view(n, T, H, HD).sum(-1)
            .permute(0, 2, 1).float()}
