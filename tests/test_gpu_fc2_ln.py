"""es_gemm_nt_ln (the MLP's fc2 + residual + the next block's LayerNorm 1 in one launch) on the MI355X: the kernel
against es_gemm_nt(epi 2) followed by es_layernorm_fwd, and the engine with the fusion on against off, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402

DEV = "cuda"
EPI_F32_RESID = 2
D, EPS = 384, 1e-6
GUARD = 3  # rows after row M - 1 of every output, filled with a pattern


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


# tile edge and clamped operand rows; three images of 197 rows; more tiles than CUs (the tile loop, the claim
# counter running past the tile count and its reset: launched twice on one stream)
@pytest.mark.parametrize("ring", [0, 1], ids=["bk64x2", "bk32x3"])
@pytest.mark.parametrize("M,K,bias", [(1, 1536, True), (127, 1536, False), (128, 1536, True), (129, 1536, True),
                                      (129, 384, False), (591, 1536, True), (591, 384, True),
                                      (256 * 128 + 1, 1536, True), (256 * 128 + 1, 384, False)])
def test_fc2_ln_matches_two_launches_bit_for_bit(M, K, bias, ring):
    """x, h, mean, rstd of es_gemm_nt_ln equal es_gemm_nt(EPI_F32_RESID) + es_layernorm_fwd on the same inputs, with
    row strides larger than the widths for A, the residual, x and h; guard rows after row M - 1 stay untouched; a
    second launch on the same stream (the kernel resets its own counters) gives the same."""
    lib = _lib.load()
    torch.manual_seed(M * 7 + K)
    lda, ldr, ldx, ldh = K + 64, D + 8, D + 4, D + 16
    Mp = (M + 255) // 256 * 256
    A = torch.zeros(Mp, lda, device=DEV, dtype=torch.bfloat16)
    A[:M, :K] = torch.randn(M, K, device=DEV).bfloat16()
    W = (torch.randn(D, K, device=DEV) * 0.05).bfloat16()
    b = torch.randn(D, device=DEV) * 0.1 if bias else None
    res = torch.zeros(Mp, ldr, device=DEV)
    res[:M, :D] = torch.randn(M, D, device=DEV)
    gamma = 1.0 + 0.1 * torch.randn(D, device=DEV)
    beta = 0.1 * torch.randn(D, device=DEV)

    def bufs():
        return (_pattern(M + GUARD, ldx, torch.float32), _pattern(M + GUARD, ldh, torch.bfloat16),
                _pattern(M + GUARD, 1, torch.float32).reshape(-1), _pattern(M + GUARD, 1, torch.float32).reshape(-1) + 1)

    x0, h0, m0, r0 = bufs()
    call("es_gemm_nt", EPI_F32_RESID, ptr(A), lda, ptr(W), K, ptr(b), ptr(x0), ldx, None, ptr(res), ldr, M, D, K, 0, S())
    call("es_layernorm_fwd", ptr(x0), ldx, ptr(gamma), ptr(beta), ptr(h0), ldh, ptr(m0), ptr(r0), M, D, EPS, S())
    old = lib.endossl_nt_ln_ring(ring)
    try:
        outs = []
        for _ in range(2):
            o = bufs()
            call("es_gemm_nt_ln", ptr(A), lda, ptr(W), K, ptr(b), ptr(o[0]), ldx, ptr(res), ldr, ptr(gamma), ptr(beta),
                 ptr(o[1]), ldh, ptr(o[2]), ptr(o[3]), M, D, K, EPS, S())
            outs.append(o)
        torch.cuda.synchronize()
    finally:
        lib.endossl_nt_ln_ring(old)
    fresh = bufs()
    assert x0[:M, :D].abs().max() > 0 and h0[:M, :D].float().abs().max() > 0
    for k, o in enumerate(outs):
        for name, got, ref, pat in zip(("x", "h", "mean", "rstd"), o, (x0, h0, m0, r0), fresh):
            w = D if got.dim() == 2 else None
            g, r_ = (got[:M, :w], ref[:M, :w]) if w else (got[:M], ref[:M])
            assert torch.equal(g, r_), (k, name, (g.float() - r_.float()).abs().max().item())
            assert torch.equal(got[M:], pat[M:]), (k, name, "guard rows written")
            if w:
                assert torch.equal(got[:M, w:], pat[:M, w:]), (k, name, "row padding written")


@pytest.fixture(scope="module")
def vit_s():
    """The ViT-S/16 of tests/test_gpu_step.py's test_resid_ln_fusion_bit_identical (D = 384), packed once."""
    from endossl.vit import NativeViT, ViTConfig
    vcfg = ViTConfig(num_classes=23)
    m = NativeViT(vcfg, seed=11)
    with torch.no_grad():
        m.head.weight.copy_(0.5 * torch.randn(m.head.weight.shape, generator=torch.Generator().manual_seed(5)))
    m.mark_updated()
    m = m.to(DEV)
    eng = m.engine()
    eng.pack(m.flat, m.version)
    g = torch.Generator(device=DEV).manual_seed(6)
    nimg = 7
    x = torch.randn(nimg, 3, vcfg.img_size, vcfg.img_size, device=DEV, generator=g)
    dl = torch.randn(nimg, 23, device=DEV, generator=g) * 1e-2
    return m, eng, x, dl


SAVED = ("x", "h1", "mean1", "rstd1", "qkv", "o", "lse", "xmid", "h2", "mean2", "rstd2", "pre", "act")


@pytest.mark.parametrize("prune", [True, False], ids=["prune", "fullrows"])
@pytest.mark.parametrize("resid_ln", [True, False], ids=["residln", "noresidln"])
def test_engine_fc2_ln_fusion_bit_identical(vit_s, prune, resid_ln):
    """Engine.FC2_LN on against off (both minimum-row attributes 0 so the small batch takes the fused paths): the
    weak pass's logits, the train pass's logits, every saved activation of the train pass and the flat gradient
    after one backward are bit-equal, with PRUNE_LAST and RESID_LN on and off."""
    m, eng, x, dl = vit_s
    names = ("FC2_LN", "FC2_LN_MIN_M", "FC2_LN_TRAIN", "FC2_LN_WEAK", "RESID_LN", "RESID_LN_MIN_M", "PRUNE_LAST")
    launches = []
    real_call = eng._call
    out = {}
    try:
        eng.FC2_LN_MIN_M = eng.RESID_LN_MIN_M = 0
        eng.FC2_LN_TRAIN = eng.FC2_LN_WEAK = True
        eng.RESID_LN, eng.PRUNE_LAST = resid_ln, prune
        eng._call = lambda name, *a: (launches.append(name), real_call(name, *a))[1]
        for fused in (False, True):
            eng.FC2_LN = fused
            launches.clear()
            lw = eng.forward(m.flat, [x], train=False).clone()
            lt = eng.forward(m.flat, [x], train=True).clone()
            A = eng.acts(x.shape[0], True)
            saved = {k: getattr(A, k).clone() for k in SAVED}
            gr = torch.full_like(m.flat, 5.0)
            eng.backward(m.flat, gr, dlogits=dl)
            torch.cuda.synchronize()
            out[fused] = (lw, lt, saved, gr, launches.count("es_gemm_nt_ln"))
    finally:
        del eng._call
        for k in names:
            if k in eng.__dict__:
                delattr(eng, k)
    depth = eng.cfg.depth
    assert out[False][4] == 0 and out[True][4] == 2 * (depth - 1)  # blocks 0 .. depth - 2, both passes
    assert torch.equal(out[True][0], out[False][0]), "weak logits"
    assert torch.equal(out[True][1], out[False][1]), "train logits"
    M = x.shape[0] * eng.cfg.T
    for k in SAVED:
        a, b = out[True][2][k], out[False][2][k]
        rows = M * eng.cfg.heads if k == "lse" else M
        a, b = a[:, :rows], b[:, :rows]
        if prune and a.shape[0] == depth:  # the pruned last block works on compact CLS rows: its full-row slots are
            if k not in ("h1", "mean1", "rstd1", "qkv"):  # unused (only LayerNorm 1 and the qkv GEMM run there)
                a, b = a[:depth - 1], b[:depth - 1]
        assert a.float().abs().max() > 0, k
        assert torch.equal(a, b), (k, (a.float() - b.float()).abs().max().item())
    assert out[True][3].abs().max() > 0
    assert torch.equal(out[True][3], out[False][3]), (out[True][3] - out[False][3]).abs().max().item()
