"""es_dense_wide_fwd / es_dense_wide_bwd (csrc/dense_wide.hip: the head layers as tiled fp32 GEMMs on the f32-input
MFMA) against float64: bit-exact on integer operands over the variants of test_gpu_head_exact.py's
test_dense_exact_on_integers (tests/test_resnet_emb_cpu.py proves from the reference alone that every partial sum of
these cases is exact in fp32), within the fp32 envelope on random operands, the refusals, and repeated bits.

Shapes (n, K, N): the head layers at D = 2048 and the degenerate and odd ones of the issue's table, then one shape on
each side of every boundary the kernels have, derived from their constants (es_dense_wide_tile: row tile TM, column
tile TN, reduction step KT, and TARGET, the workgroup count the backward splits a reduction towards):
  * (TM - 1, KT - 1, TN - 1), (TM, KT, TN), (TM + 1, KT + 1, TN + 1): a ragged single tile, an exact one, and one
    row / column / reduction index into the next tile and the next step, in all three products at once;
  * dW [N, K] over n: with N = 16 TN and K = TARGET / 16 * TN its tiles number exactly TARGET, so the reduction is
    not split; with K one tile less they number TARGET - 16 and it is split in two -- at n = 2 KT + 6 the second
    split is one ragged step.  (dX [n, K] over N is split in both; the table's (17, 2048, 512) has it in 8.)"""
import pytest
import torch

import head_cases as hc
from test_gpu_head_exact import (BAD_ARG, BAD_SHAPE, DEV, OK, PAD, L, Out, S, _lib_loaded, _release_inputs,  # noqa: F401
                                 all_ways, inp, nanbuf, same)

pytestmark = pytest.mark.gpu

from endossl._lib import ptr  # noqa: E402

TABLE = [(1, 1, 1), (33, 65, 63), (31, 2, 257), (17, 2048, 512), (130, 2048, 768), (384, 2048, 512), (96, 2048, 192),
         (70, 192, 64), (70, 768, 256), (65, 512, 5), (3, 64, 2048)]


TM, TN, KT, TARGET = 32, 32, 32, 512  # csrc/dense_wide.hip's constants (test_constants_are_the_kernels)
K_FULL = TARGET // 16 * TN
EDGES = [(TM - 1, KT - 1, TN - 1), (TM, KT, TN), (TM + 1, KT + 1, TN + 1), (2 * KT + 6, K_FULL, 16 * TN),
         (2 * KT + 6, K_FULL - TN, 16 * TN)]
SHAPES = TABLE + [s for s in EDGES if s not in TABLE]


def test_constants_are_the_kernels():
    assert [L().es_dense_wide_tile(i) for i in range(4)] == [TM, TN, KT, TARGET]


def run_wide(c, act, with_keep, pad=0, accumulate=0, dx_null=False, db_null=False):
    n, K = c["X"].shape
    N = c["W"].shape[0]
    X, W, b, dY = inp(c["X"], pad), inp(c["W"]), inp(c["b"]), inp(c["dY"], pad)
    keep = inp(c["keep"]) if with_keep else None
    Y = Out(n, N, pad)
    assert L().es_dense_wide_fwd(ptr(X), K + pad, ptr(W), ptr(b), Y.p, N + pad, n, K, N, act, hc.DENSE_SLOPE,
                                 ptr(keep), hc.DENSE_KEEP_SCALE, S()) == OK
    dX = Out(n, K, pad, init=c["dX0"] if accumulate else None)
    dW, db = Out(N, K), Out(1, N)
    ws = nanbuf(L().es_dense_wide_bwd_workspace(n, K, N, 0 if dx_null else 1))
    assert ws.numel() >= n * N
    assert L().es_dense_wide_bwd(ptr(dY), N + pad, Y.p if act else None, N + pad, act, hc.DENSE_SLOPE, ptr(keep),
                                 hc.DENSE_KEEP_SCALE, ptr(X), K + pad, ptr(W), None if dx_null else dX.p, K + pad,
                                 accumulate, dW.p, None if db_null else db.p, n, K, N, ptr(ws), S()) == OK
    torch.cuda.synchronize()
    if dx_null:
        assert dX.untouched()
    if db_null:
        assert db.untouched()
    return {"Y": Y.get(), "dX": None if dx_null else dX.get(), "dW": dW.get(), "db": None if db_null else db.vec()}


@pytest.fixture(scope="module")
def refs():
    """dense_case and its float64 results per (shape, act, keep): computed once, shared, never changed."""
    cache = {}

    def get(shape, act, with_keep):
        if shape not in cache:
            cache[shape] = {"c": hc.dense_case(*shape)}
        if (act, with_keep) not in cache[shape]:
            cache[shape][(act, with_keep)] = hc.dense64(cache[shape]["c"], act, with_keep)
        return cache[shape]["c"], cache[shape][(act, with_keep)]
    return get


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "relu", "leaky"])
@pytest.mark.parametrize("n,K,N", SHAPES)
def test_dense_wide_exact_on_integers(n, K, N, act, refs):
    for with_keep in (False, True):
        c, r = refs((n, K, N), act, with_keep)
        assert hc.dense_magnitude(c, with_keep) < 2 ** 24
        o = all_ways(run_wide, c=c, act=act, with_keep=with_keep)
        for k in ("Y", "dX", "dW", "db"):
            assert torch.equal(o[k].double(), r[k]), (k, with_keep)
        a = run_wide(c, act, with_keep, pad=PAD, accumulate=1)
        assert torch.equal(a["dX"].double(), r["dX"] + c["dX0"].double()) and same(a["dW"], o["dW"])
        q = run_wide(c, act, with_keep, pad=PAD, dx_null=True)
        assert same(q["dW"], o["dW"]) and same(q["db"], o["db"])  # dX null: dW and db still written
        q = run_wide(c, act, with_keep, db_null=True)
        assert same(q["dW"], o["dW"]) and same(q["dX"], o["dX"])


@pytest.mark.parametrize("n,K,N", [(384, 2048, 512), (130, 2048, 768)])
def test_dense_wide_random_operands_within_the_fp32_envelope(n, K, N):
    """randn operands, ReLU and the keep mask: per output tensor, max |device - float64| <= 4 x the distance of fp32
    torch on the CPU from float64 on the same operands + 1e-6 (the envelope tests/test_gpu_resnet50.py uses)."""
    import torch.nn.functional as F
    g = hc.gen(7 * n + N)
    c = {"X": torch.randn(n, K, generator=g), "W": torch.randn(N, K, generator=g) * K ** -0.5,
         "b": torch.randn(N, generator=g), "dY": torch.randn(n, N, generator=g), "dX0": torch.zeros(n, K),
         "keep": (torch.rand(n, N, generator=g) >= 0.2).to(torch.uint8)}
    r64 = hc.dense64(c, 1, True)
    X, W, b = (c[k].clone().requires_grad_(True) for k in ("X", "W", "b"))
    y = F.relu(X @ W.t() + b) * (c["keep"].float() * hc.DENSE_KEEP_SCALE)
    y.backward(c["dY"])
    r32 = {"Y": y.detach(), "dX": X.grad, "dW": W.grad, "db": b.grad}
    o = run_wide(c, 1, True)
    assert same(o, run_wide(c, 1, True)), "a second launch gave other bits"
    bad = []
    for k in ("Y", "dX", "dW", "db"):
        e, env = (o[k].double() - r64[k]).abs().max().item(), (r32[k].double() - r64[k]).abs().max().item()
        print(f"{(n, K, N)} {k}: |device - fp64| = {e:.3e}, |cpu fp32 - fp64| = {env:.3e}")
        if not e <= 4 * env + 1e-6:
            bad.append((k, e, env))
    assert not bad, bad


def test_dense_wide_refusals():
    c = hc.dense_case(4, 8, 6)
    X, W, b, dY = (inp(c[k]) for k in ("X", "W", "b", "dY"))
    ws = nanbuf(L().es_dense_wide_bwd_workspace(4, 8, 6, 1))

    def fwd(rc, n=4, K=8, N=6, ldx=8, ldy=6, act=1, null=()):
        Y = Out(4, 6)
        a = {"X": ptr(X), "W": ptr(W), "Y": Y.p}
        a.update({k: None for k in null})
        assert L().es_dense_wide_fwd(a["X"], ldx, a["W"], ptr(b), a["Y"], ldy, n, K, N, act, 0.1, None, 1.0, S()) == rc
        torch.cuda.synchronize()
        assert Y.untouched()

    def bwd(rc, n=4, K=8, N=6, lddy=6, ldya=6, ldx=8, lddx=8, act=1, null=()):
        dX, dW, db = Out(4, 8), Out(6, 8), Out(1, 6)
        a = {"dY": ptr(dY), "Y": ptr(dY), "X": ptr(X), "W": ptr(W), "dW": dW.p, "ws": ptr(ws)}
        a.update({k: None for k in null})
        assert L().es_dense_wide_bwd(a["dY"], lddy, a["Y"], ldya, act, 0.1, None, 1.0, a["X"], ldx, a["W"], dX.p, lddx,
                                     0, a["dW"], db.p, n, K, N, a["ws"], S()) == rc
        torch.cuda.synchronize()
        assert dX.untouched() and dW.untouched() and db.untouched() and torch.isnan(ws).all()

    for kw in (dict(K=4097), dict(N=4097), dict(n=0), dict(n=65535 * 32 + 1), dict(N=0), dict(K=0), dict(act=3),
               dict(ldx=7), dict(ldy=5)):
        fwd(BAD_SHAPE, **kw)
    for k in ("X", "W", "Y"):
        fwd(BAD_ARG, null=(k,))
    for kw in (dict(N=4097), dict(K=4097), dict(n=0), dict(n=65535 * 32 + 1), dict(K=0), dict(N=0), dict(act=-1), dict(lddy=5), dict(ldya=5),
               dict(ldx=7), dict(lddx=7)):
        bwd(BAD_SHAPE, **kw)
    for k in ("dY", "Y", "X", "W", "dW", "ws"):
        bwd(BAD_ARG, null=(k,))
    for bad in ((0, 8, 6), (65535 * 32 + 1, 8, 6), (4, 0, 6), (4, 8, 0), (4, 4097, 6), (4, 8, 4097)):
        assert L().es_dense_wide_bwd_workspace(*bad, 1) == 0
    assert L().es_dense_wide_bwd_workspace(4, 8, 6, 0) >= 24


def test_heads_wide_against_narrow():
    """EmbHeads with `wide` on and off on the same features, parameters and gradients at ResNet-50's width: each
    within the head bars (tests/test_gpu_triplet.py) of the float64 heads on those features."""
    from endossl.comatch_model import EmbHeads
    from endossl.resnet import RESNET50, ResNetConfig
    from oracle import ref
    cfg = ResNetConfig(num_classes=5, head="emb", low_dim=64, **RESNET50)
    n, D, F_, C, Lw = 24, 2048, 512, 5, 64
    g = hc.gen(5)
    shapes = {"fc.0.weight": (F_, D), "fc.0.bias": (F_,), "fc.3.weight": (F_,), "fc.3.bias": (F_,),
              "fc.4.weight": (C, F_), "fc.4.bias": (C,), "head_emb.0.weight": (3 * Lw, D), "head_emb.0.bias": (3 * Lw,),
              "head_emb.2.weight": (Lw, 3 * Lw), "head_emb.2.bias": (Lw,)}
    p = {k: torch.randn(s, generator=g) * (s[-1] ** -0.5 if len(s) == 2 else 0.1) for k, s in shapes.items()}
    p["fc.3.weight"] = p["fc.3.weight"] + 1.0
    fts = torch.randn(n, D, generator=g)
    keep = (torch.rand(n, F_, generator=g) >= 0.2).to(torch.uint8)
    dl, dz = torch.randn(n, C, generator=g), torch.randn(n, Lw, generator=g)
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    f64 = fts.double().requires_grad_(True)
    bufs64 = {"fc.3.running_mean": torch.zeros(F_, dtype=torch.float64), "fc.3.running_var": torch.ones(F_, dtype=torch.float64),
              "fc.3.num_batches_tracked": torch.zeros((), dtype=torch.int64)}
    lg64, z64 = ref.emb_heads(p64, bufs64, f64, keep, train=True)
    torch.autograd.backward([lg64, z64], [dl.double(), dz.double()])
    dev = {k: v.to(DEV) for k, v in p.items()}
    out = {}
    for wide in (False, True):
        heads = EmbHeads(cfg, torch.device(DEV), wide=wide)
        grads = {k: torch.zeros_like(v) for k, v in dev.items()}
        bn = (torch.zeros(F_, device=DEV), torch.ones(F_, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV))
        fd, kd = fts.to(DEV), keep.to(DEV)
        lg, z = heads.forward(dev.__getitem__, bn, fd, kd, True)
        dfts = heads.backward(dev.__getitem__, grads.__getitem__, fd, kd, dl.to(DEV), dz.to(DEV))
        torch.cuda.synchronize()
        out[wide] = (lg.cpu(), z.cpu(), dfts.cpu(), {k: v.cpu() for k, v in grads.items()})
        sc = max(1.0, lg64.abs().max().item())
        e = (out[wide][0].double() - lg64.detach()).abs().max().item()
        print(f"wide={wide}: logits |device - fp64| = {e:.3e}, scale {sc:.3f}")
        assert e <= 1e-4 * sc
        torch.testing.assert_close(out[wide][1], z64.detach().float(), rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(out[wide][2], f64.grad.float(), rtol=1e-4, atol=1e-5)
        for k, v in out[wide][3].items():
            torch.testing.assert_close(v, p64[k].grad.float(), rtol=1e-4, atol=1e-5, msg=lambda s, k=k: f"{k}: {s}")
    assert out[True][0].shape == out[False][0].shape
