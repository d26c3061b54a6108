"""The attention kernels on the MI355X against closed forms (tests/attn_patterns.py; held to float64 autograd by
test_attn_patterns_cpu.py): softmax rows that are exactly one-hot, or exactly (1/2, 1/2), so o, dQ, dK, dV and delta
are compared with torch.equal / == 0 and an indexing error of any size shows -- a V row taken from the wrong key of
a tile, a tail key of the last partial tile leaking into P.V, a head or image offset wrong for one (image, head).
Only lse keeps the suite's rtol = 1e-3, atol = 2e-3.

Rounding points read in csrc/attention.hip, none of which needed a relaxation: the forward's P = exp2(s - max) is 1
at the selected keys and exp2 of at most -158 (an exact 0) elsewhere, o = acc * (1 / l) with l = 1 or 2; the
backward's p = exp2(s * sl - lse * log2 e) is 1 (or 1/2) to about 1e-4 before it is rounded to bf16, which gives 1
(1/2) exactly for dV, and dS = p * (dP - delta) is either an exact 0 (one-hot: dP = delta on integers) or at most an
8-bit integer over 4 times 1 + 1e-4, which its bf16 rounding returns to that number."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_patterns as ap  # noqa: E402
from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402

DEV = "cuda"
SCALE = 64 ** -0.5
FWD_VARIANTS = (2, 3, 7)
BWD_VARIANTS = (0, 1, 2, 3, 4)


def S():
    return _lib.stream()


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _lib.load()


def _pattern(rows, cols, dtype):
    """A finite, recognisable fill (bit-compared: no NaN)."""
    t = torch.arange(rows * cols, device=DEV, dtype=torch.float32).reshape(rows, cols) % 251 - 125.0
    return t.to(dtype)


def _pad_rows(t, mult=256):
    M = t.shape[0]
    out = torch.zeros(((M + mult - 1) // mult * mult,) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV)
    out[:M] = t.to(DEV)
    return out


@functools.lru_cache(maxsize=None)
def _one_hot(n, T, H, integer_v):
    return ap.one_hot(n, T, H, integer_v=integer_v)


@functools.lru_cache(maxsize=None)
def _two_hot(n, T, H):
    return ap.two_hot(n, T, H)


class _Knob:
    """lib.<setter>(v) for the duration of a block."""

    def __init__(self, setter, v):
        self.fn, self.v = getattr(_lib.load(), setter), v

    def __enter__(self):
        self.old = self.fn(self.v)

    def __exit__(self, *exc):
        self.fn(self.old)


def _fwd(qkv, n, T, H, variant):
    """es_attn_fwd on pattern-prefilled outputs -> (o, its prefill, lse)."""
    D = H * 64
    pat = _pattern(qkv.shape[0], D, torch.bfloat16)
    o = pat.clone()
    lse = torch.full((n * H * T,), -7.0, device=DEV)
    with _Knob("es_set_attn_variant", variant):
        call("es_attn_fwd", ptr(qkv), 3 * D, ptr(o), D, ptr(lse), n, T, H, SCALE, S())
        torch.cuda.synchronize()
    return o, pat, lse.view(n, H, T)


def _check_lse(lse, want):
    torch.testing.assert_close(lse, torch.as_tensor(want, dtype=torch.float32, device=DEV).expand_as(lse),
                               rtol=1e-3, atol=2e-3)


def _bwd(p, qkv, o, lse, variant, long=1):
    """es_attn_bwd on pattern-prefilled dqkv / delta -> (dqkv, its prefill, delta, its prefill)."""
    n, T, H = p["n"], p["T"], p["H"]
    D = H * 64
    dout = _pad_rows(p["dout"])
    pat = _pattern(qkv.shape[0], 3 * D, torch.bfloat16)
    dqkv = pat.clone()
    dpat = _pattern(n * H * T, 1, torch.float32).reshape(-1) + 0.5
    delta = dpat.clone()
    with _Knob("es_set_attn_bwd_variant", variant), _Knob("es_set_attn_bwd_long", long):
        call("es_attn_bwd", ptr(qkv), 3 * D, ptr(o), D, ptr(lse), ptr(delta), ptr(dout), D, ptr(dqkv), 3 * D, n, T, H,
             SCALE, S())
        torch.cuda.synchronize()
    return dqkv, pat, delta, dpat


def _check_delta(p, variant, delta, dpat):
    n, T, H = p["n"], p["T"], p["H"]
    if variant == 4 and (T + 15) // 16 == 13:  # the single-pass kernel keeps delta on chip (include/endossl.h)
        assert torch.equal(delta, dpat), "the single-pass backward leaves the delta workspace untouched"
    else:
        assert torch.equal(delta.view(n, H, T), p["delta"].to(DEV)), "delta"


# ------------------------------------------------------------------------------------- one-hot
@pytest.mark.parametrize("n,T,H", ap.ONE_HOT_SHAPES)
def test_one_hot_forward(n, T, H):
    """o_i = v_pi(i) bit for bit for random bf16 v under every forward variant, lse = 512, rows past n*T untouched."""
    p = _one_hot(n, T, H, False)
    qkv = _pad_rows(p["qkv"])
    want = p["o"].to(DEV)
    for variant in FWD_VARIANTS:
        o, pat, lse = _fwd(qkv, n, T, H, variant)
        assert torch.equal(o[:n * T], want), (variant, (o[:n * T].float() - want.float()).abs().max().item())
        assert torch.equal(o[n * T:], pat[n * T:]), (variant, "rows past n*T written")
        _check_lse(lse, 512.0)


@pytest.mark.parametrize("n,T,H", ap.ONE_HOT_SHAPES)
def test_one_hot_backward(n, T, H):
    """Integer v and dO: dV_pi(i) = dO_i bit for bit, dQ = dK = 0 (== 0: -0 accepted), delta = sum(dO * O) exactly,
    pad rows untouched, under every backward variant.  Past T = 256 es_set_attn_bwd_long(0) sends every variant to the
    plain loops, the kernels variant 0 runs there with the knob on: run once more under the default variant."""
    p = _one_hot(n, T, H, True)
    D, M = H * 64, n * T
    qkv = _pad_rows(p["qkv"])
    o, _, lse = _fwd(qkv, n, T, H, 7)
    assert torch.equal(o[:M], p["o"].to(DEV))
    o[M:] = 0
    runs = [(v, 1) for v in BWD_VARIANTS] + ([(4, 0)] if T > 256 else [])
    for variant, long in runs:
        dqkv, pat, delta, dpat = _bwd(p, qkv, o, lse, variant, long)
        tag = (variant, long)
        assert torch.equal(dqkv[:M, 2 * D:], p["dv"].to(DEV)), (tag, "dV")
        assert (dqkv[:M, :D] == 0).all(), (tag, "dQ")
        assert (dqkv[:M, D:2 * D] == 0).all(), (tag, "dK")
        assert torch.equal(dqkv[M:], pat[M:]), (tag, "pad rows written")
        _check_delta(p, variant, delta, dpat)


@pytest.mark.parametrize("n,T,H", ap.ONE_HOT_SHAPES)
def test_one_hot_cls_forward_backward(n, T, H):
    """es_attn_cls_fwd: oc = v_pi(0) per image and head, lse = 512.  es_attn_cls_bwd: dV = dO at the selected key and
    zero elsewhere, dQ = dK = 0, every token row of dqkv written (NaN prefill), pad rows untouched."""
    p = _one_hot(n, T, H, True)
    D, M = H * 64, n * T
    qkv = _pad_rows(p["qkv"])
    cls = torch.arange(n, device=DEV) * T
    opat = _pattern(n + 3, D, torch.bfloat16)
    oc = opat.clone()
    lc = torch.full((n * H,), -7.0, device=DEV)
    call("es_attn_cls_fwd", ptr(qkv), 3 * D, ptr(oc), D, ptr(lc), n, T, H, SCALE, S())
    torch.cuda.synchronize()
    assert torch.equal(oc[:n], p["o"].to(DEV)[cls]) and torch.equal(oc[n:], opat[n:])
    _check_lse(lc, 512.0)
    doc = p["dout"].to(DEV)[cls].contiguous()
    pat = _pattern(qkv.shape[0], 3 * D, torch.bfloat16)
    dqkv = pat.clone()
    dqkv[:M] = float("nan")
    call("es_attn_cls_bwd", ptr(qkv), 3 * D, ptr(oc), D, ptr(lc), ptr(doc), D, ptr(dqkv), 3 * D, n, T, H, SCALE, S())
    torch.cuda.synchronize()
    assert torch.isfinite(dqkv[:M]).all()
    # dV[img, pi(0), head] = dO[img, head]
    want = torch.zeros(n, T, H, 64)
    pi0 = p["pi"][:, :, 0]  # [n, H]
    dov = p["dout"].float().view(n, T, H, 64)[:, 0]  # [n, H, 64]
    for i in range(n):
        for h in range(H):
            want[i, pi0[i, h], h] = dov[i, h]
    assert torch.equal(dqkv[:M, 2 * D:], want.view(M, D).to(torch.bfloat16).to(DEV)), "dV"
    assert (dqkv[:M, :2 * D] == 0).all(), "dQ / dK"
    assert torch.equal(dqkv[M:], pat[M:]), "pad rows written"


# ------------------------------------------------------------------------------------- two-hot
@pytest.mark.parametrize("n,T,H", ap.TWO_HOT_SHAPES)
def test_two_hot_forward_backward(n, T, H):
    """P = (1/2, 1/2) on orthogonal keys: o, dQ, dK and dV torch.equal to float64 autograd's bf16 numbers under forward
    variants 2 and 3 and every backward variant (dQ and dK are nonzero here: their content, not only their zeros)."""
    p = _two_hot(n, T, H)
    D, M = H * 64, n * T
    qkv = _pad_rows(p["qkv"])
    want_o, want_d = p["o"].to(DEV), p["dqkv"].to(DEV)
    for variant in (2, 3):
        o, pat, lse = _fwd(qkv, n, T, H, variant)
        assert torch.equal(o[:M], want_o), (variant, (o[:M].float() - want_o.float()).abs().max().item())
        assert torch.equal(o[M:], pat[M:]), (variant, "rows past n*T written")
        _check_lse(lse, p["lse"].float())
    o[M:] = 0
    for variant in BWD_VARIANTS:
        dqkv, pat, delta, dpat = _bwd(p, qkv, o, lse, variant)
        for k, name in enumerate(("dQ", "dK", "dV")):
            a, b = dqkv[:M, k * D:(k + 1) * D], want_d[:, k * D:(k + 1) * D]
            assert torch.equal(a, b), (variant, name, (a.float() - b.float()).abs().max().item())
        assert torch.equal(dqkv[M:], pat[M:]), (variant, "pad rows written")
        _check_delta(p, variant, delta, dpat)
