"""The GEMM entry points the way the engine calls them (endossl/block.py), on the MI355X: row strides larger than the
widths, weight / bias / output sub-views, compact rows written at a token stride, a residual read at one -- under
every pinned NT family and tn tile, with pattern-filled outputs and guard rows.  Every comparison is bit for bit
(against the natural-stride launch, or against float64 on small integers) except the GELU values, held to the
suite's rtol = atol = 1e-2 of float64.  Also es_gemm_nt's argument checks, which run before any launch."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402

DEV = "cuda"
EPI_BF16, EPI_GELU, EPI_F32_RESID, EPI_DGELU, EPI_F32, EPI_PATCH, EPI_GELU_ACT, EPI_GELU_D, EPI_MULAUX = range(9)
F32_OUT = (EPI_F32_RESID, EPI_F32, EPI_PATCH)
HAS_C2 = (EPI_GELU, EPI_GELU_D)
AUX_F32, AUX_BF16 = (EPI_F32_RESID, EPI_PATCH), (EPI_DGELU, EPI_MULAUX)
GUARD = 3  # rows after row M - 1 of every output, filled with a pattern
GEMM_VARIANTS = [-1, 0, 1, 2, 5, 6, 10, 11]
ES_BAD_SHAPE, ES_BAD_ARG = -1, -2


def S():
    return _lib.stream()


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _lib.load()


class _Pinned:
    """es_set_gemm_variant(v) for the duration of a block."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old = _lib.load().es_set_gemm_variant(self.v)
        assert self.old != ES_BAD_ARG

    def __exit__(self, *exc):
        _lib.load().es_set_gemm_variant(self.old)


def _tiles(v, N):
    return N % (256 if v == 6 else 128) == 0


def _variants(N):
    return [v for v in GEMM_VARIANTS if _tiles(v, N)]


def _pattern(rows, cols, dtype):
    """A finite, recognisable fill (bit-compared: no NaN); every value is a bf16 number."""
    t = torch.arange(rows * cols, device=DEV, dtype=torch.float32).reshape(rows, cols) % 251 - 125.0
    return t.to(dtype)


def _rup(M, mult=256):
    return (M + mult - 1) // mult * mult


def _a_operand(vals, ld):
    """A GEMM's A: round_up(M, 256) rows at its own stride ld, zero pad rows (the kernels read whole tiles unguarded),
    the padding columns of the M real rows pattern-filled (nothing may read them)."""
    M, K = vals.shape
    out = torch.zeros(_rup(M), ld, dtype=vals.dtype, device=DEV)
    out[:M] = _pattern(M, ld, vals.dtype)
    out[:M, :K] = vals
    return out


def _strided(vals, ld):
    """vals [R, W] as the first W columns of a pattern-filled [R, ld]."""
    R, W = vals.shape
    out = _pattern(R, ld, vals.dtype)
    out[:, :W] = vals
    return out


def _ints(*shape, lo, hi, gen, dtype=torch.bfloat16):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int32).to(dtype).to(DEV)


def _odt(epi):
    return torch.float32 if epi in F32_OUT else torch.bfloat16


def _ld_out(epi, N, strided):
    return N + ((4 if epi in F32_OUT else 8) if strided else 0)


def _ld_aux(epi, N, strided):
    return N + ((4 if epi in AUX_F32 else 8) if strided else 0)


def _nt(epi, A, lda, B, ldb, bias, C, ldc, C2, aux, ldaux, M, N, K, np_=0):
    call("es_gemm_nt", epi, ptr(A), lda, ptr(B), ldb, ptr(bias), ptr(C), ldc, ptr(C2), ptr(aux), ldaux, M, N, K, np_,
         S())


def _launch(epi, M, N, K, a, b, bias, aux, strided, np_=0):
    """One es_gemm_nt launch on pattern-prefilled outputs; strided: every operand at a row stride above its width.
    Returns (C, C2 or None, the prefill pattern, the C row count of the real rows)."""
    lda, ldb = (K + 64, K + 8) if strided else (K, K)
    ldc, ldaux = _ld_out(epi, N, strided), _ld_aux(epi, N, strided)
    A, B = _a_operand(a, lda), _strided(b, ldb)
    X = None if aux is None else _strided(aux, ldaux)
    crows = M // np_ * (np_ + 1) if epi == EPI_PATCH else M
    pat = _pattern(crows + GUARD, ldc, _odt(epi))
    C = pat.clone()
    C2 = pat.clone() + 1 if epi in HAS_C2 else None
    _nt(epi, A, lda, B, ldb, bias, C, ldc, C2, X, ldaux if aux is not None else 0, M, N, K, np_)
    torch.cuda.synchronize()
    return C, C2, pat, crows


def _check_untouched(epi, C, C2, pat, crows, N, np_, tag):
    for name, got, p in (("C", C, pat), ("C2", C2, pat + 1)):
        if got is None:
            continue
        assert torch.equal(got[crows:], p[crows:]), (tag, name, "guard rows written")
        assert torch.equal(got[:, N:], p[:, N:]), (tag, name, "row padding written")
    if epi == EPI_PATCH:
        assert torch.equal(C[0:crows:np_ + 1], pat[0:crows:np_ + 1]), (tag, "CLS rows written")


# ------------------------------------------------------------------ 1. strided against packed, every epilogue
NP = 7


def _random_operands(epi, M, N, K, gen):
    dev_randn = lambda *sh: torch.randn(*sh, generator=gen).to(DEV)  # noqa: E731
    a = dev_randn(M, K).bfloat16()
    b = (dev_randn(N, K) * 0.05).bfloat16()
    bias = None if epi in AUX_BF16 else dev_randn(N) * 0.1
    aux = None
    if epi == EPI_F32_RESID:
        aux = dev_randn(M, N)
    elif epi == EPI_PATCH:
        aux = dev_randn(NP + 1, N)
    elif epi in AUX_BF16:
        aux = dev_randn(M, N).bfloat16()
    return a, b, bias, aux


@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (77, 256, 64)])
@pytest.mark.parametrize("variant", GEMM_VARIANTS)
def test_strided_operands_match_packed_bit_for_bit(variant, M, N, K):
    """Every epilogue, once with packed operands and once with A, B, C, C2 and aux all strided, on the same values:
    C[:M, :N] (and C2) bit-equal, the padding columns and the guard rows still the prefill pattern.  K = 64 is one K
    step: shorter than the three-stage rings' prologue.  EPI_PATCH: np = 7 patches per image (M a multiple of it), the
    position table strided, the CLS rows still the pattern."""
    gen = torch.Generator().manual_seed(M + N + K)
    with _Pinned(variant):
        for epi in range(9):
            np_ = NP if epi == EPI_PATCH else 0
            Me = M // NP * NP if epi == EPI_PATCH else M
            a, b, bias, aux = _random_operands(epi, Me, N, K, gen)
            res = {st: _launch(epi, Me, N, K, a, b, bias, aux, st, np_) for st in (False, True)}
            (C0, C20, _, crows), (C1, C21, pat1, _) = res[False], res[True]
            tag = (variant, epi)
            assert C0[:crows].float().abs().max() > 0, tag
            if epi == EPI_PATCH:  # the rows the kernel writes: every row but each image's first
                keep = torch.ones(crows, dtype=torch.bool, device=DEV)
                keep[0:crows:NP + 1] = False
                assert torch.equal(C1[:crows, :N][keep], C0[:crows][keep]), tag
                assert not torch.equal(C0[:crows][keep], _pattern(crows + GUARD, N, C0.dtype)[:crows][keep]), tag
            else:
                assert torch.equal(C1[:crows, :N], C0[:crows]), (tag, "C")
            if C20 is not None:
                assert torch.equal(C21[:crows, :N], C20[:crows]), (tag, "C2")
            _check_untouched(epi, C1, C21, pat1, crows, N, np_, tag)
            _check_untouched(epi, C0, C20, res[False][2], crows, N, np_, tag)


# ------------------------------------------------------------------ 2. exact integers on the strided launch
def _exact_case(epi, M, N, K, gen, with_bias):
    """Small-integer operands whose float64 result is exact in the output format (asserted by round trip)."""
    small = epi in (EPI_BF16, EPI_MULAUX)  # bf16 outputs: |acc + bias| <= K + 4 < 256
    lim = 1 if small else 3
    a, b = _ints(M, K, lo=-lim, hi=lim, gen=gen), _ints(N, K, lo=-lim, hi=lim, gen=gen)
    bias = _ints(N, lo=-4, hi=4, gen=gen, dtype=torch.float32) if with_bias and epi != EPI_MULAUX else None
    ref = a.double() @ b.double().t()
    if bias is not None:
        ref = ref + bias.double()
    aux = None
    if epi == EPI_F32_RESID:
        aux = _ints(M, N, lo=-50, hi=50, gen=gen, dtype=torch.float32)
        ref = ref + aux.double()
    elif epi == EPI_MULAUX:  # signed powers of two and zero: the product keeps acc's significand
        steps = torch.tensor([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
        aux = steps[torch.randint(0, 9, (M, N), generator=gen)].bfloat16().to(DEV)
        ref = ref * aux.double()
    assert torch.equal(ref.to(_odt(epi)).double(), ref), "the float64 result is a number of the output format"
    return a, b, bias, aux, ref


@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (77, 256, 64)])
@pytest.mark.parametrize("variant", GEMM_VARIANTS)
def test_strided_exact_integers(variant, M, N, K):
    """EPI_F32, EPI_BF16, EPI_F32_RESID and EPI_MULAUX on strided operands against float64 at rtol = atol = 0, and the
    bias = NULL form of the three bias-taking ones."""
    gen = torch.Generator().manual_seed(7 * M + K)
    with _Pinned(variant):
        for epi, with_bias in ((EPI_F32, True), (EPI_BF16, True), (EPI_F32_RESID, True), (EPI_MULAUX, False),
                               (EPI_F32, False), (EPI_BF16, False), (EPI_F32_RESID, False)):
            a, b, bias, aux, ref = _exact_case(epi, M, N, K, gen, with_bias)
            C, _, pat, _ = _launch(epi, M, N, K, a, b, bias, aux, True)
            tag = (variant, epi, with_bias)
            torch.testing.assert_close(C[:M, :N].double(), ref, rtol=0, atol=0, msg=lambda m: f"{tag}: {m}")
            _check_untouched(epi, C, None, pat, M, N, 0, tag)


# ------------------------------------------------------------------ 3. EPI_GELU_ACT
@pytest.mark.parametrize("variant,M,N", [(v, M, N) for M, N in [(777, 512), (40, 384)] for v in _variants(N)])
def test_gelu_act_bits_and_value(variant, M, N):
    """EPI_GELU_ACT (the weak-branch fc1): C is bit-equal to the C2 of EPI_GELU and of EPI_GELU_D on the same operands
    (the same gelu_and_grad_f8 on the same v: the header promises these bits for epi 7), and within the suite's
    rtol = atol = 1e-2 of float64 gelu(A B^T + bias).  Strided operands; every family that tiles N."""
    K = 384
    gen = torch.Generator().manual_seed(M + N)
    a, b, bias, _ = _random_operands(EPI_GELU, M, N, K, gen)
    with _Pinned(variant):
        act, _, pat, _ = _launch(EPI_GELU_ACT, M, N, K, a, b, bias, None, True)
        _, g1, _, _ = _launch(EPI_GELU, M, N, K, a, b, bias, None, True)
        _, g7, _, _ = _launch(EPI_GELU_D, M, N, K, a, b, bias, None, True)
    assert torch.equal(act[:M, :N], g1[:M, :N]) and torch.equal(act[:M, :N], g7[:M, :N])
    ref = F.gelu(a.double() @ b.double().t() + bias.double())
    torch.testing.assert_close(act[:M, :N].double(), ref, rtol=1e-2, atol=1e-2)
    _check_untouched(EPI_GELU_ACT, act, None, pat, M, N, 0, variant)


# ------------------------------------------------------------------ 4. tile edges
@pytest.mark.parametrize("M", [1, 63, 64, 65, 127, 129, 255, 257])
def test_tile_edges(M):
    """M below, at and just past each tile height (64 / 128 / 256), N = 256, K = 128, every family: EPI_F32 exact on
    integers against float64; EPI_GELU_D within rtol = atol = 1e-2 of float64 and bit-identical to family 0 -- every
    NT kernel of csrc/gemm.hip (gemm_nt_kernel, gemm_nt256_kernel, gemm_nt_big_kernel) adds an output element's
    K axis in the same order: one 16x16x32 MFMA per 32-wide K chunk, chunks ascending (a BK64 step is its two chunks
    in order, kk = 0, 1), lane group g holding k = 32 kk + 8 g .. + 7 of both operands, then acc + bias.  Guard rows
    untouched."""
    N, K = 256, 128
    gen = torch.Generator().manual_seed(M)
    ai, bi, biasi, _, refi = _exact_case(EPI_F32, M, N, K, gen, True)
    a, b, bias, _ = _random_operands(EPI_GELU_D, M, N, K, gen)
    pre = (a.double() @ b.double().t() + bias.double()).requires_grad_(True)
    F.gelu(pre).backward(torch.ones_like(pre))
    base = None
    for v in [0] + [x for x in GEMM_VARIANTS if x != 0]:
        with _Pinned(v):
            C, _, pat, _ = _launch(EPI_F32, M, N, K, ai, bi, biasi, None, True)
            torch.testing.assert_close(C[:M, :N].double(), refi, rtol=0, atol=0, msg=lambda m: f"family {v}: {m}")
            _check_untouched(EPI_F32, C, None, pat, M, N, 0, v)
            D_, G_, pat, _ = _launch(EPI_GELU_D, M, N, K, a, b, bias, None, True)
        _check_untouched(EPI_GELU_D, D_, G_, pat, M, N, 0, v)
        torch.testing.assert_close(D_[:M, :N].double(), pre.grad, rtol=1e-2, atol=1e-2)
        torch.testing.assert_close(G_[:M, :N].double(), F.gelu(pre.detach()), rtol=1e-2, atol=1e-2)
        if base is None:
            base = (D_, G_)
        else:
            assert torch.equal(D_, base[0]) and torch.equal(G_, base[1]), v


# ------------------------------------------------------------------ 5. the engine's split-Q write pattern
@pytest.mark.parametrize("variant", GEMM_VARIANTS)
def test_split_q_write_pattern(variant):
    """Chain.attn_fwd(split_q=True) on integers, D = 128, T = 5, n = 40: K / V for every token row through the weight
    and bias slice [D:] into the column block [:, D:] of qkv (N = 2D, ldc = 3D), then Q for the compact CLS rows
    through the slice [:D] onto rows img * T (ldc = T * 3D).  Zero tolerance: K / V of every token row and Q of the CLS
    rows equal float64, Q of every other row and the pad rows still hold the prefill pattern.  The 256-wide family
    (6) does not tile the N = 128 launch: that one runs on the per-shape choice."""
    D, T, n = 128, 5, 40
    M, Mp = n * T, _rup(n * T)
    gen = torch.Generator().manual_seed(5)
    h1 = _a_operand(_ints(M, D, lo=-1, hi=1, gen=gen), D)
    w = _ints(3 * D, D, lo=-1, hi=1, gen=gen)
    bias = _ints(3 * D, lo=-4, hi=4, gen=gen, dtype=torch.float32)
    ref = h1[:M].double() @ w.double().t() + bias.double()
    assert torch.equal(ref.bfloat16().double(), ref)
    pat = _pattern(Mp, 3 * D, torch.bfloat16)
    qkv = pat.clone()
    cls_h1 = _a_operand(h1[:M].view(n, T, D)[:, 0].contiguous(), D)
    with _Pinned(variant):
        _nt(EPI_BF16, h1, D, w[D:], D, bias[D:], qkv[:, D:], 3 * D, None, None, 0, M, 2 * D, D)
    with _Pinned(variant if _tiles(variant, D) else -1):
        _nt(EPI_BF16, cls_h1, D, w[:D], D, bias[:D], qkv, T * 3 * D, None, None, 0, n, D, D)
    torch.cuda.synchronize()
    got = qkv[:M].double()
    torch.testing.assert_close(got[:, D:], ref[:, D:], rtol=0, atol=0)
    torch.testing.assert_close(got[0::T, :D], ref[0::T, :D], rtol=0, atol=0)
    other = torch.ones(M, dtype=torch.bool, device=DEV)
    other[0::T] = False
    assert torch.equal(qkv[:M, :D][other], pat[:M, :D][other]), "Q of a non-CLS row written"
    assert torch.equal(qkv[M:], pat[M:]), "pad rows written"


@pytest.mark.parametrize("variant", [v for v in GEMM_VARIANTS if v != 6])
def test_cls_rows_residual_at_token_stride(variant):
    """Chain.mlp_fwd's unfused projection on the pruned last block's n compact CLS rows: EPI_F32_RESID reading its
    residual from rows img * T of a token buffer (ldaux = T * D).  Exact integers against float64."""
    D, T, n = 128, 5, 40
    gen = torch.Generator().manual_seed(6)
    o = _a_operand(_ints(n, D, lo=-3, hi=3, gen=gen), D)
    w = _ints(D, D, lo=-3, hi=3, gen=gen)
    bias = _ints(D, lo=-4, hi=4, gen=gen, dtype=torch.float32)
    x = _ints(_rup(n * T), D, lo=-50, hi=50, gen=gen, dtype=torch.float32)
    pat = _pattern(n + GUARD, D, torch.float32)
    xmid = pat.clone()
    with _Pinned(variant):
        _nt(EPI_F32_RESID, o, D, w, D, bias, xmid, D, None, x, T * D, n, D, D)
    torch.cuda.synchronize()
    ref = o[:n].double() @ w.double().t() + bias.double() + x[0:n * T:T].double()
    torch.testing.assert_close(xmid[:n].double(), ref, rtol=0, atol=0)
    assert torch.equal(xmid[n:], pat[n:])


# ------------------------------------------------------------------ 6. es_gemm_nt_resid_ln strided
@pytest.mark.parametrize("M", [5, 129, 591])
def test_resid_ln_strided_matches_two_launches(M):
    """es_gemm_nt_resid_ln against es_gemm_nt(EPI_F32_RESID) + es_layernorm_fwd at lda = D + 64, ldc = D + 4,
    ldaux = D + 8, ldh = D + 16: x, h, mean, rstd bit for bit, guard rows and padding columns untouched, launched
    twice on one stream (the kernel resets its own tile claims)."""
    D, eps = 384, 1e-6
    lda, ldc, ldaux, ldh = D + 64, D + 4, D + 8, D + 16
    torch.manual_seed(M)
    A = _a_operand(torch.randn(M, D, device=DEV).bfloat16(), lda)
    W = (torch.randn(D, D, device=DEV) * 0.05).bfloat16()
    bias = torch.randn(D, device=DEV) * 0.1
    res = torch.zeros(_rup(M), ldaux, device=DEV)
    res[:M] = _strided(torch.randn(M, D, device=DEV), ldaux)
    gamma = 1.0 + 0.1 * torch.randn(D, device=DEV)
    beta = 0.1 * torch.randn(D, device=DEV)

    def bufs():
        return (_pattern(M + GUARD, ldc, torch.float32), _pattern(M + GUARD, ldh, torch.bfloat16),
                _pattern(M + GUARD, 1, torch.float32).reshape(-1), _pattern(M + GUARD, 1, torch.float32).reshape(-1) + 1)

    x0, h0, m0, r0 = bufs()
    _nt(EPI_F32_RESID, A, lda, W, D, bias, x0, ldc, None, res, ldaux, M, D, D)
    call("es_layernorm_fwd", ptr(x0), ldc, ptr(gamma), ptr(beta), ptr(h0), ldh, ptr(m0), ptr(r0), M, D, eps, S())
    outs = []
    for _ in range(2):
        o = bufs()
        call("es_gemm_nt_resid_ln", ptr(A), lda, ptr(W), D, ptr(bias), ptr(o[0]), ldc, ptr(res), ldaux, ptr(gamma),
             ptr(beta), ptr(o[1]), ldh, ptr(o[2]), ptr(o[3]), M, D, D, eps, S())
        outs.append(o)
    torch.cuda.synchronize()
    fresh = bufs()
    assert x0[:M, :D].abs().max() > 0 and h0[:M, :D].float().abs().max() > 0
    for k, o in enumerate(outs):
        for name, got, ref, pat in zip(("x", "h", "mean", "rstd"), o, (x0, h0, m0, r0), fresh):
            if got.dim() == 2:
                assert torch.equal(got[:M, :D], ref[:M, :D]), (k, name)
                assert torch.equal(got[:M, D:], pat[:M, D:]), (k, name, "row padding written")
            else:
                assert torch.equal(got[:M], ref[:M]), (k, name)
            assert torch.equal(got[M:], pat[M:]), (k, name, "guard rows written")


# ------------------------------------------------------------------ 7. es_gemm_tn / es_gemm_tn_ex strided
@pytest.fixture(params=[-1, 0, 7], ids=["auto", "t0", "b7"])
def tn_variant(request):
    old = _lib.load().es_set_tn_variant(request.param)
    yield request.param
    _lib.load().es_set_tn_variant(old)


@pytest.mark.parametrize("M,N1,N2", [(1000, 384, 192), (1000, 256, 128)])
def test_gemm_tn_strided_exact_integers(M, N1, N2, tn_variant):
    """out = A1^T A2 at ld1 = N1 + 64, ld2 = N2 + 8 on integers, exact: with the fused bias gradient, without it, and
    accumulating.  Only A1's pad rows are zero (the header's contract); A2's hold nonzero integers, and so do the
    padding columns of both."""
    gen = torch.Generator().manual_seed(M + N1)
    ld1, ld2 = N1 + 64, N2 + 8
    A1 = _a_operand(_ints(M, N1, lo=-2, hi=2, gen=gen), ld1)
    A2 = _ints(_rup(M), ld2, lo=-2, hi=2, gen=gen)
    A2[M:] = _ints(_rup(M) - M, ld2, lo=1, hi=3, gen=gen)
    ref = A1[:M, :N1].double().t() @ A2[:M, :N2].double()
    bref = A1[:M, :N1].double().sum(0)
    lib = _lib.load()
    for splits in (0, 3):
        ws = torch.empty(lib.es_gemm_tn_workspace(N1, N2, splits), device=DEV)
        out = torch.full((N1, N2), 3.0, device=DEV)
        bias = torch.full((N1,), 5.0, device=DEV)
        call("es_gemm_tn", ptr(A1), ld1, ptr(A2), ld2, M, N1, N2, splits, ptr(ws), ptr(out), 0, ptr(bias), S())
        torch.testing.assert_close(out.double(), ref, rtol=0, atol=0)
        torch.testing.assert_close(bias.double(), bref, rtol=0, atol=0)
        out2 = torch.full((N1, N2), 3.0, device=DEV)
        call("es_gemm_tn", ptr(A1), ld1, ptr(A2), ld2, M, N1, N2, splits, ptr(ws), ptr(out2), 0, None, S())
        torch.testing.assert_close(out2.double(), ref, rtol=0, atol=0)
        call("es_gemm_tn", ptr(A1), ld1, ptr(A2), ld2, M, N1, N2, splits, ptr(ws), ptr(out2), 1, ptr(bias), S())
        torch.testing.assert_close(out2.double(), 2 * ref, rtol=0, atol=0)
        torch.testing.assert_close(bias.double(), 2 * bref, rtol=0, atol=0)


def test_gemm_tn_cls_rows_exact_integers(tn_variant):
    """The engine's Q weight gradient over the pruned last block's CLS rows (Chain.attn_bwd(split_q=True)): D = 384,
    T = 3, M = n = 64 (a whole 64-token step: no row past the buffers is read under either tile), A1 = dqkv's base at
    ld1 = T * 3D, A2 = h1's base at ld2 = T * D.  Expected dqkv[::T, :D]^T h1[::T] and its column sums, exact."""
    D, T, n = 384, 3, 64
    gen = torch.Generator().manual_seed(64)
    dqkv = _a_operand(_ints(n * T, 3 * D, lo=-2, hi=2, gen=gen), 3 * D)
    h1 = _a_operand(_ints(n * T, D, lo=-2, hi=2, gen=gen), D)
    ref = dqkv[0:n * T:T, :D].double().t() @ h1[0:n * T:T].double()
    bref = dqkv[0:n * T:T, :D].double().sum(0)
    ws = torch.empty(_lib.load().es_gemm_tn_workspace(D, D, 0), device=DEV)
    for ex in (-1, 7):  # the variant the caller names (a pin wins over it)
        out, bias = torch.full((D, D), 3.0, device=DEV), torch.full((D,), 5.0, device=DEV)
        call("es_gemm_tn_ex", ptr(dqkv), T * 3 * D, ptr(h1), T * D, n, D, D, 0, ptr(ws), ptr(out), 0, ptr(bias), ex, S())
        torch.testing.assert_close(out.double(), ref, rtol=0, atol=0)
        torch.testing.assert_close(bias.double(), bref, rtol=0, atol=0)


# ------------------------------------------------------------------ 8. es_gemm_nt's argument checks
def test_gemm_nt_argument_checks():
    """Every check runs before the launch, so the status is returned and nothing runs (called through the library
    handle: _lib.call would raise).  The buffer is large enough for the M = 64, N = 256, K = 64 problem regardless."""
    lib = _lib.load()
    z = torch.zeros(256, 1024, device=DEV)
    p = ptr(z)
    M, N, K = 64, 256, 64

    def rc(epi=EPI_F32, lda=K, ldb=K, ldc=N, c2=p, aux=p, ldaux=N, M=M, N=N, K=K, np_=8):
        return lib.es_gemm_nt(epi, p, lda, p, ldb, p, p, ldc, c2, aux, ldaux, M, N, K, np_, S())

    assert rc(N=192, ldc=192, ldaux=192) == ES_BAD_SHAPE and rc(N=64, ldc=64, ldaux=64) == ES_BAD_SHAPE
    assert rc(K=32, lda=32, ldb=32) == ES_BAD_SHAPE and rc(K=96, lda=96, ldb=96) == ES_BAD_SHAPE
    assert rc(lda=K + 4) == ES_BAD_SHAPE and rc(ldb=K + 4) == ES_BAD_SHAPE and rc(ldc=N + 2) == ES_BAD_SHAPE
    assert rc(M=0) == ES_BAD_SHAPE and rc(M=-1) == ES_BAD_SHAPE
    with _Pinned(6):
        assert rc(N=128, ldc=128, ldaux=128) == ES_BAD_SHAPE
    for epi in (EPI_GELU, EPI_GELU_D):
        assert rc(epi=epi, c2=None) == ES_BAD_ARG, epi
    for epi in AUX_F32 + AUX_BF16:
        assert rc(epi=epi, aux=None) == ES_BAD_ARG, epi
    assert rc(epi=EPI_PATCH, np_=0) == ES_BAD_ARG and rc(epi=EPI_PATCH, np_=-1) == ES_BAD_ARG
    # the aux row stride: 16-byte pieces at (m * ldaux + n), no row shorter than N
    for epi in AUX_F32:
        assert rc(epi=epi, ldaux=N + 2) == ES_BAD_SHAPE and rc(epi=epi, ldaux=N - 4) == ES_BAD_SHAPE, epi
        assert rc(epi=epi, ldaux=0) == ES_BAD_SHAPE, epi
    for epi in AUX_BF16:
        assert rc(epi=epi, ldaux=N + 4) == ES_BAD_SHAPE and rc(epi=epi, ldaux=N - 8) == ES_BAD_SHAPE, epi
        assert rc(epi=epi, ldaux=0) == ES_BAD_SHAPE, epi
