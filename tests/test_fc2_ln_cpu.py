"""The fc2 + residual + next-block LayerNorm 1 fusion (es_gemm_nt_ln) without a GPU: the chain's launch lists with
`mlp_fwd(next_ln=)` / `attn_fwd(ln_done=True)` (pointer arguments included, in tests/test_block_chain_cpu.py's rig;
the expected launches are written out by hand from include/endossl.h's argument order), the defaults unchanged, and
the entry point's refusals, which return before any launch."""
import importlib.util
import os

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_block_chain_rig", os.path.join(_HERE, "test_block_chain_cpu.py"))
rig = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rig)

P, p, D, H, HD, T, EPS, S, BLK = rig.P, rig.p, rig.D, rig.H, rig.HD, rig.T, rig.EPS, rig.S, rig.BLK
SCALE = rig.SCALE


def _next_ln(r):
    """The next block's LayerNorm 1 operands: parameters and outputs of their own (named in the rig's table)."""
    import torch
    t = r.t
    t["p:next.norm1.weight"], t["p:next.norm1.bias"] = torch.zeros(D), torch.zeros(D)
    t["n_h1"] = torch.zeros(r.M + 8, D, dtype=torch.bfloat16)
    t["n_mean1"], t["n_rstd1"] = torch.zeros(r.M + 8), torch.zeros(r.M + 8)
    return (t["p:next.norm1.weight"], t["p:next.norm1.bias"], t["n_h1"], t["n_mean1"], t["n_rstd1"])


def _exp_fc2_ln(M):
    return ("es_gemm_nt_ln", P("act"), HD, P("wb:mlp.fc2.weight"), HD, p("mlp.fc2.bias"), P("out"), D, P("xmid"), D,
            P("p:next.norm1.weight"), P("p:next.norm1.bias"), P("n_h1"), D, P("n_mean1"), P("n_rstd1"), M, D, HD, EPS,
            S)


@pytest.mark.parametrize("case", ["train_gelu_d", "weak", "fused"])
def test_mlp_fwd_next_ln_replaces_the_fc2_launch(case, monkeypatch):
    """mlp_fwd(next_ln=): the list of the default chain with its last launch (fc2, epilogue 2) replaced by one
    es_gemm_nt_ln that also carries the next block's gamma / beta / h1 / mean1 / rstd1."""
    n = 4
    M = n * T
    r = rig.Rig(n, monkeypatch)
    train = case != "weak"
    label = "fc1_fwd" if train else "fc1_fwd_weak"
    R = r.rows()
    r.chain.attn_fwd(BLK, R)
    r.chain.mlp_fwd(BLK, R, train, fused=case == "fused", label=label, next_ln=_next_ln(r))
    epi = rig.GELU_ACT if case == "weak" else rig.GELU_D
    e = rig.exp_fwd_full(n, (label, epi), fused=case == "fused")
    assert e[-1][0] == "es_gemm_nt" and e[-1][1] == rig.F32_RESID
    e[-1] = _exp_fc2_ln(M)
    r.check(e)


def test_attn_fwd_ln_done_skips_only_the_layernorm(monkeypatch):
    """mlp_fwd(next_ln=) followed by attn_fwd(ln_done=True): the fused launch, then the qkv GEMM and the attention
    with no es_layernorm_fwd in front; the pruned last block's form keeps its split Q / K,V GEMMs."""
    n = 4
    M = n * T
    r = rig.Rig(n, monkeypatch)
    R = r.rows()
    r.chain.mlp_fwd(BLK, R, True, label="fc1_fwd", next_ln=_next_ln(r))
    r.chain.attn_fwd(BLK, R, ln_done=True)
    full = rig.exp_fwd_full(n, ("fc1_fwd", rig.GELU_D))
    mlp = full[3:-1] + [_exp_fc2_ln(M)]  # proj + residual, LN2, the bracket, fc1, then the fused fc2
    attn = full[1:3]                     # the qkv GEMM and the attention, without the LayerNorm (full[0])
    assert full[0][0] == "es_layernorm_fwd" and [x[0] for x in attn] == ["es_gemm_nt", "es_attn_fwd"]
    r.check(mlp + attn)

    r = rig.Rig(n, monkeypatch)
    R, Rc = r.rows(), r.cls_rows()
    r.chain.attn_fwd(BLK, R, cls=Rc, split_q=True, ln_done=True)
    assert [x[0] for x in r.log] == ["es_gemm_nt", "es_gemm_nt", "es_attn_cls_fwd"]
    r.check([("es_gemm_nt", rig.BF16, P("h1"), D, P("wb:attn.qkv.weight", D * D * 2), D, P("p:attn.qkv.bias", D * 4),
              P("qkv", D * 2), 3 * D, None, None, 0, M, 2 * D, D, 0, S),
             ("es_gemm_nt", rig.BF16, P("c_h1"), D, P("wb:attn.qkv.weight"), D, p("attn.qkv.bias"), P("qkv"), T * 3 * D,
              None, None, 0, n, D, D, 0, S),
             ("es_attn_cls_fwd", P("qkv"), 3 * D, P("c_o"), D, P("c_lse"), n, T, H, SCALE, S)])


@pytest.mark.parametrize("case", ["train_gelu_d", "weak", "fused"])
def test_defaults_give_the_two_launch_lists(case, monkeypatch):
    """next_ln=None / ln_done=False spelled out are the chain without the keywords."""
    n = 4
    r = rig.Rig(n, monkeypatch)
    train = case != "weak"
    label = "fc1_fwd" if train else "fc1_fwd_weak"
    R = r.rows()
    r.chain.attn_fwd(BLK, R, ln_done=False)
    r.chain.mlp_fwd(BLK, R, train, fused=case == "fused", label=label, next_ln=None)
    r.check(rig.exp_fwd_full(n, (label, rig.GELU_ACT if case == "weak" else rig.GELU_D), fused=case == "fused"))


def test_fc2_ln_entry_validates_before_any_launch():
    """es_gemm_nt_ln refuses what its kernel cannot take before touching the GPU (the pointers below are never
    dereferenced): any N but 384, K not a multiple of 64, M <= 0, misaligned or too short row strides
    (ES_BAD_SHAPE); a null or misaligned operand (ES_BAD_ARG)."""
    from endossl import _lib
    lib = _lib.load()
    q = 0x7000000000

    def rc(M=256, N=384, K=1536, lda=1536, ldb=1536, ldc=384, ldaux=384, ldh=384, A=q, B=q, bias=None, C=q, aux=q,
           gamma=q, beta=q, h=q, mean=q, rstd=q):
        return lib.es_gemm_nt_ln(A, lda, B, ldb, bias, C, ldc, aux, ldaux, gamma, beta, h, ldh, mean, rstd, M, N, K,
                                 1e-6, None)
    assert rc(N=768) == -1 and rc(N=256) == -1 and rc(K=1520) == -1 and rc(K=32) == -1 and rc(K=0) == -1
    assert rc(M=0) == -1 and rc(M=-5) == -1
    assert rc(lda=1540) == -1 and rc(ldb=1540) == -1 and rc(ldc=385) == -1 and rc(ldaux=385) == -1 and rc(ldh=385) == -1
    assert rc(lda=1024) == -1 and rc(ldc=256) == -1  # a row stride below the row's width
    for name in ("A", "B", "C", "aux", "gamma", "beta", "h", "mean", "rstd"):
        assert rc(**{name: None}) == -2, name
    for name, off in (("A", 8), ("B", 8), ("gamma", 4), ("beta", 4), ("bias", q + 4), ("C", 4), ("aux", 4), ("h", 2),
                      ("mean", 2), ("rstd", 2)):
        assert rc(**{name: off if name == "bias" else q + off}) == -2, name
