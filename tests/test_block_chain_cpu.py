"""The block chain's argument order (endossl/block.py), checked without a GPU or the library: each chain piece is
driven with CPU tensors at the vit_tiny_test shapes and a recording `call`; the expected launches below are
transcribed by hand from the call sites of the chain's seven hand-written copies as of commit 0991a0a (the
`vit.py:` / `conformer.py:` line numbers are that commit's), not produced by the code under test."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "endoscopy-image-classification_amd"))
from endossl import _lib, block  # noqa: E402

D, H, HD, T, EPS = 128, 2, 512, 17, 1e-6
S = 0x5EED  # the "current stream"
BF16, GELU, F32_RESID, DGELU, F32, PATCH, GELU_ACT, GELU_D, MULAUX = range(9)  # es_gemm_nt epilogues (endossl.h)
SCALE = 64 ** -0.5
F, B = torch.float32, torch.bfloat16
BLK = "blocks.1."
PARAMS = {"norm1.weight": D, "norm1.bias": D, "attn.qkv.weight": 3 * D * D, "attn.qkv.bias": 3 * D,
          "attn.proj.weight": D * D, "attn.proj.bias": D, "norm2.weight": D, "norm2.bias": D,
          "mlp.fc1.weight": HD * D, "mlp.fc1.bias": HD, "mlp.fc2.weight": D * HD, "mlp.fc2.bias": D}
MATS = {"attn.qkv.weight": (3 * D, D), "attn.proj.weight": (D, D), "mlp.fc1.weight": (HD, D), "mlp.fc2.weight": (D, HD)}


class P:
    """Expected pointer: the named buffer's data_ptr() plus a byte offset."""

    def __init__(self, name, off=0):
        self.name, self.off = name, off


class Rig:
    """Named CPU buffers in the engine's shapes (_Acts / _Grads), a recording call, the owner's callbacks."""

    def __init__(self, n, monkeypatch, gelu_d=True, conformer_ln=False):
        monkeypatch.setattr(block, "ptr", lambda t: None if t is None else t.data_ptr())
        monkeypatch.setattr(block, "stream", lambda: S)
        self.n, self.M, self.log = n, n * T, []
        Mp, Mc = n * T + 8, n + 8
        z = lambda *s, dt=F: torch.zeros(*s, dtype=dt)  # noqa: E731
        self.t = t = {}
        for k in ("x", "xmid", "out", "dx", "dxm", "dxm_cls"):
            t[k] = z(Mp, D)
        for k in ("h1", "h2", "o", "dxb", "dxmb", "do", "dh", "dxb_next"):
            t[k] = z(Mp, D, dt=B)
        for k in ("mean1", "rstd1", "mean2", "rstd2"):
            t[k] = z(Mp)
        t["qkv"], t["dqkv"] = z(Mp, 3 * D, dt=B), z(Mp, 3 * D, dt=B)
        t["pre"], t["act"], t["dpre"] = z(Mp, HD, dt=B), z(Mp, HD, dt=B), z(Mp, HD, dt=B)
        t["lse"], t["delta"] = z(n * H * T), z(n * H * T)
        for k in ("c_h1", "c_o", "c_h2", "c_dxb", "c_dxmb", "c_do", "c_dh"):
            t[k] = z(Mc, D, dt=B)
        for k in ("c_xmid", "c_xout", "c_dx"):
            t[k] = z(Mc, D)
        t["c_pre"], t["c_act"], t["c_dpre"] = z(Mc, HD, dt=B), z(Mc, HD, dt=B), z(Mc, HD, dt=B)
        t["c_lse"], t["c_mean2"], t["c_rstd2"] = z(n * H), z(Mc), z(Mc)
        t["ws_ln"] = z(2 * 1024 * D)
        wb, wt = {}, {}
        for name, numel in PARAMS.items():
            t["p:" + name], t["g:" + name] = z(numel), z(numel)
        for name, (N, K) in MATS.items():
            wb[BLK + name] = t["wb:" + name] = z(N, K, dt=B)
            wt[BLK + name] = t["wt:" + name] = z(K, N, dt=B)
        self.chain = block.Chain(self.call, lambda name: t["p:" + name[len(BLK):]], lambda name: t["g:" + name[len(BLK):]],
                                 wb, wt, H, EPS, gelu_d=gelu_d, bracket=self.bracket)
        self.conformer_ln = conformer_ln

    def call(self, name, *args):
        self.log.append((name,) + args)

    def bracket(self, label, flop, launch):
        self.log.append(("bracket", label, flop))
        launch()

    # the owner's callbacks, recorded in the same log
    def ln_bwd(self, dy, x, mean, rstd, gamma, dres, dx, dxb, dgamma, dbeta, M, lddx=None):
        # the direct form of Engine._ln_bwd (vit.py:624-626) / of the Conformer (conformer.py:978-980, 1001-1003)
        block.layernorm_bwd(self.call, dy, x, mean, rstd, gamma, dres, dx, dxb, dgamma, dbeta, self.t["ws_ln"], 1024, M, D,
                            0, lddx)

    def wgrad(self, dy, N1, x, N2, M, out, bias_out, ld1=None, ld2=None, label=None):
        self.log.append(("wgrad", dy.data_ptr(), N1, x.data_ptr(), N2, M, out.data_ptr(), bias_out.data_ptr(), ld1, ld2,
                         label))

    def before_ln1(self):
        self.log.append(("before_ln1",))

    def cap(self, kind, *ts):
        self.log.append(("cap", kind) + tuple(x.data_ptr() for x in ts))

    def rows(self):
        t = self.t
        return block.Rows(self.n, T, H, x=t["x"], h1=t["h1"], mean1=t["mean1"], rstd1=t["rstd1"],
                          qkv=t["qkv"], o=t["o"], lse=t["lse"], xmid=t["xmid"], h2=t["h2"], mean2=t["mean2"],
                          rstd2=t["rstd2"], pre=t["pre"], act=t["act"], out=t["out"], dxb=t["dxb"], dpre=t["dpre"],
                          dh=t["dh"], dres=t["dx"], dxm=t["dxm"], dxmb=t["dxmb"], do=t["do"], delta=t["delta"],
                          dqkv=t["dqkv"], dh1=t["dh"], dx=t["dx"], dxb_next=t["dxb_next"])

    def cls_rows(self):
        t = self.t
        return block.Rows(self.n, 1, H, ldx=T * D, lddxm=T * D, x=t["x"], h1=t["c_h1"], o=t["c_o"], lse=t["c_lse"],
                          xmid=t["c_xmid"], h2=t["c_h2"], mean2=t["c_mean2"], rstd2=t["c_rstd2"], pre=t["c_pre"],
                          act=t["c_act"], out=t["c_xout"], dxb=t["c_dxb"], dpre=t["c_dpre"], dh=t["c_dh"], dres=t["c_dx"],
                          dxm=t["dxm_cls"], dxmb=t["c_dxmb"], do=t["c_do"])

    def check(self, expected):
        """Names in order, len(args) == the C signature's, every scalar equal, every pointer the named buffer's."""
        assert [e[0] for e in self.log] == [e[0] for e in expected]
        for got, exp in zip(self.log, expected):
            name = got[0]
            if name.startswith("es_"):
                assert len(got) - 1 == len(_lib.SIGNATURES[name][1]), name
            assert len(got) == len(exp), (name, got, exp)
            for j, (g, e) in enumerate(zip(got[1:], exp[1:])):
                if isinstance(e, P):
                    e = self.t[e.name].data_ptr() + e.off
                assert g == e and type(g) is type(e), (name, j, g, e)


def p(name):
    return P("p:" + name)


def g(name):
    return P("g:" + name)


def exp_ln1_qkv(M):
    # vit.py:476-478 (LN1), 488-490 (qkv GEMM); conformer.py:894-897
    return [("es_layernorm_fwd", P("x"), D, p("norm1.weight"), p("norm1.bias"), P("h1"), D, P("mean1"), P("rstd1"), M, D,
             EPS, S),
            ("es_gemm_nt", BF16, P("h1"), D, P("wb:attn.qkv.weight"), D, p("attn.qkv.bias"), P("qkv"), 3 * D, None, None,
             0, M, 3 * D, D, 0, S)]


def exp_fwd_full(n, fc1, fused=False):
    M = n * T
    e = exp_ln1_qkv(M)
    # vit.py:496; conformer.py:898
    e += [("es_attn_fwd", P("qkv"), 3 * D, P("o"), D, P("lse"), n, T, H, SCALE, S)]
    if fused:  # vit.py:498-501
        e += [("es_gemm_nt_resid_ln", P("o"), D, P("wb:attn.proj.weight"), D, p("attn.proj.bias"), P("xmid"), D, P("x"),
               D, p("norm2.weight"), p("norm2.bias"), P("h2"), D, P("mean2"), P("rstd2"), M, D, D, EPS, S)]
    else:  # vit.py:503-507; conformer.py:899-902
        e += [("es_gemm_nt", F32_RESID, P("o"), D, P("wb:attn.proj.weight"), D, p("attn.proj.bias"), P("xmid"), D, None,
               P("x"), D, M, D, D, 0, S),
              ("es_layernorm_fwd", P("xmid"), D, p("norm2.weight"), p("norm2.bias"), P("h2"), D, P("mean2"), P("rstd2"), M,
               D, EPS, S)]
    label, epi = fc1
    e += [("bracket", label, 2.0 * M * HD * D)]  # vit.py:377-378 (Engine._gemm: the probed launch's flop)
    if epi == GELU_ACT:  # vit.py:514-516 (weak); conformer.py:907-908
        e += [("es_gemm_nt", GELU_ACT, P("h2"), D, P("wb:mlp.fc1.weight"), D, p("mlp.fc1.bias"), P("act"), HD, None, None,
               0, M, HD, D, 0, S)]
    else:  # vit.py:509-512 (train: GELU_D or GELU); conformer.py:904-905
        e += [("es_gemm_nt", epi, P("h2"), D, P("wb:mlp.fc1.weight"), D, p("mlp.fc1.bias"), P("pre"), HD, P("act"), None,
               0, M, HD, D, 0, S)]
    # vit.py:517-518; conformer.py:909-910
    e += [("es_gemm_nt", F32_RESID, P("act"), HD, P("wb:mlp.fc2.weight"), HD, p("mlp.fc2.bias"), P("out"), D, None,
           P("xmid"), D, M, D, HD, 0, S)]
    return e


@pytest.mark.parametrize("case", ["train_gelu_d", "train_gelu", "weak", "fused"])
def test_forward_full_rows(case, monkeypatch):
    n = 4
    r = Rig(n, monkeypatch, gelu_d=case != "train_gelu")
    train = case != "weak"
    label = "fc1_fwd" if train else "fc1_fwd_weak"
    R = r.rows()
    r.chain.attn_fwd(BLK, R)
    r.chain.mlp_fwd(BLK, R, train, fused=case == "fused", label=label)
    epi = {"train_gelu": GELU, "weak": GELU_ACT}.get(case, GELU_D)
    r.check(exp_fwd_full(n, (label, epi), fused=case == "fused"))


@pytest.mark.parametrize("split_q", [True, False])
def test_forward_cls_tail(split_q, monkeypatch):
    """The pruned last block: vit.py:476-486 (or 488-490 without PRUNE_Q), then _last_block_cls_fwd, vit.py:546-559."""
    n = 4
    M = n * T
    r = Rig(n, monkeypatch)
    R, Rc = r.rows(), r.cls_rows()
    r.chain.attn_fwd(BLK, R, cls=Rc, split_q=split_q)
    r.chain.mlp_fwd(BLK, Rc, True)
    e = exp_ln1_qkv(M)
    if split_q:  # vit.py:482-486: K / V for every token, Q for the CLS rows into their rows of qkv
        e[1:] = [("es_gemm_nt", BF16, P("h1"), D, P("wb:attn.qkv.weight", D * D * 2), D, P("p:attn.qkv.bias", D * 4),
                  P("qkv", D * 2), 3 * D, None, None, 0, M, 2 * D, D, 0, S),
                 ("es_gemm_nt", BF16, P("c_h1"), D, P("wb:attn.qkv.weight"), D, p("attn.qkv.bias"), P("qkv"), T * 3 * D,
                  None, None, 0, n, D, D, 0, S)]
    e += [("es_attn_cls_fwd", P("qkv"), 3 * D, P("c_o"), D, P("c_lse"), n, T, H, SCALE, S),  # vit.py:546
          ("es_gemm_nt", F32_RESID, P("c_o"), D, P("wb:attn.proj.weight"), D, p("attn.proj.bias"), P("c_xmid"), D, None,
           P("x"), T * D, n, D, D, 0, S),  # vit.py:547-548
          ("es_layernorm_fwd", P("c_xmid"), D, p("norm2.weight"), p("norm2.bias"), P("c_h2"), D, P("c_mean2"),
           P("c_rstd2"), n, D, EPS, S),  # vit.py:549-550
          ("bracket", None, 2.0 * n * HD * D),  # (no probed label on the compact rows: vit.py:552 calls directly)
          ("es_gemm_nt", GELU_D, P("c_h2"), D, P("wb:mlp.fc1.weight"), D, p("mlp.fc1.bias"), P("c_pre"), HD, P("c_act"),
           None, 0, n, HD, D, 0, S),  # vit.py:552-554
          ("es_gemm_nt", F32_RESID, P("c_act"), HD, P("wb:mlp.fc2.weight"), HD, p("mlp.fc2.bias"), P("c_xout"), D, None,
           P("c_xmid"), D, n, D, HD, 0, S)]  # vit.py:558-559
    r.check(e)
    if split_q:  # vit.py:484: LN1's CLS rows gathered for the Q projection
        r.t["h1"][:M].view(n, T, D)[:, 0] = 1.0
        r.chain.attn_fwd(BLK, R, cls=Rc, split_q=True)
        assert bool((r.t["c_h1"][:n] == 1).all()) and bool((r.t["c_h1"][n:] == 0).all())


def exp_bwd_full(n, gelu_d=True):
    """vit.py:853-887 (full rows)."""
    M = n * T
    return [
        ("cap", "b_dxb", P("dxb")),  # vit.py:854
        ("es_gemm_nt", MULAUX if gelu_d else DGELU, P("dxb"), D, P("wt:mlp.fc2.weight"), D, None, P("dpre"), HD, None,
         P("pre"), HD, M, HD, D, 0, S),  # vit.py:855-856
        ("wgrad", P("dxb"), D, P("act"), HD, M, g("mlp.fc2.weight"), g("mlp.fc2.bias"), None, None, None),  # vit.py:857
        ("es_gemm_nt", BF16, P("dpre"), HD, P("wt:mlp.fc1.weight"), HD, None, P("dh"), D, None, None, 0, M, D, HD, 0,
         S),  # vit.py:858-859 (EPI_DH = EPI_BF16: DH_BF16)
        ("wgrad", P("dpre"), HD, P("h2"), D, M, g("mlp.fc1.weight"), g("mlp.fc1.bias"), None, None, "fc1_wgrad"),  # :860
        ("cap", "b_dpre", P("dpre")), ("cap", "b_dh2", P("dh")),  # vit.py:862-863
        # vit.py:864-865 through Engine._ln_bwd's direct form, vit.py:625-626
        ("es_layernorm_bwd_b16", P("dh"), D, P("xmid"), D, P("mean2"), P("rstd2"), p("norm2.weight"), P("dx"), D,
         P("dxm"), D, P("dxmb"), D, g("norm2.weight"), g("norm2.bias"), P("ws_ln"), 1024, M, D, 0, S),
        ("es_gemm_nt", BF16, P("dxmb"), D, P("wt:attn.proj.weight"), D, None, P("do"), D, None, None, 0, M, D, D, 0,
         S),  # vit.py:867-868
        ("wgrad", P("dxmb"), D, P("o"), D, M, g("attn.proj.weight"), g("attn.proj.bias"), None, None, None),  # vit.py:869
        ("cap", "b_dxm", P("dxm"), P("dxmb")), ("cap", "b_do", P("do")),  # vit.py:871-872
        ("es_attn_bwd", P("qkv"), 3 * D, P("o"), D, P("lse"), P("delta"), P("do"), D, P("dqkv"), 3 * D, n, T, H, SCALE,
         S),  # vit.py:873-874
        ("es_gemm_nt", BF16, P("dqkv"), 3 * D, P("wt:attn.qkv.weight"), 3 * D, None, P("dh"), D, None, None, 0, M, D,
         3 * D, 0, S),  # vit.py:875-876
        ("wgrad", P("dqkv"), 3 * D, P("h1"), D, M, g("attn.qkv.weight"), g("attn.qkv.bias"), None, None, None),  # :877
        ("cap", "b_dqkv", P("dqkv")), ("cap", "b_dh1", P("dh")),  # vit.py:879-880
        ("before_ln1",),  # vit.py:881-885: flush_layer / done[i] / the wait on done[i + 1]
        # vit.py:886-887
        ("es_layernorm_bwd_b16", P("dh"), D, P("x"), D, P("mean1"), P("rstd1"), p("norm1.weight"), P("dxm"), D, P("dx"),
         D, P("dxb_next"), D, g("norm1.weight"), g("norm1.bias"), P("ws_ln"), 1024, M, D, 0, S)]


@pytest.mark.parametrize("gelu_d", [True, False])
def test_reverse_full_rows(gelu_d, monkeypatch):
    n = 4
    r = Rig(n, monkeypatch, gelu_d=gelu_d)
    R = r.rows()
    r.chain.mlp_bwd(BLK, R, r.ln_bwd, r.wgrad, r.cap, label="fc1_wgrad")
    r.chain.attn_bwd(BLK, R, r.ln_bwd, r.wgrad, r.before_ln1, r.cap)
    r.check(exp_bwd_full(n, gelu_d=gelu_d))


@pytest.mark.parametrize("n", [32, 4])
def test_reverse_pruned_last_block(n, monkeypatch):
    """vit.py:809-838: the MLP half on n compact CLS rows, the attention half over the full token image; the
    CLS-row Q split of the qkv weight gradient (vit.py:827-831) needs n % 32 == 0."""
    M = n * T
    split = n % 32 == 0
    r = Rig(n, monkeypatch)
    R, Rc = r.rows(), r.cls_rows()
    R.dxm = r.t["dxm_cls"]
    r.chain.mlp_bwd(BLK, Rc, r.ln_bwd, r.wgrad)
    r.chain.attn_bwd(BLK, R, r.ln_bwd, r.wgrad, r.before_ln1, cls=Rc, split_q=split)
    e = [("es_gemm_nt", MULAUX, P("c_dxb"), D, P("wt:mlp.fc2.weight"), D, None, P("c_dpre"), HD, None, P("c_pre"), HD, n,
          HD, D, 0, S),  # vit.py:809-811
         ("wgrad", P("c_dxb"), D, P("c_act"), HD, n, g("mlp.fc2.weight"), g("mlp.fc2.bias"), None, None, None),  # :812
         ("es_gemm_nt", BF16, P("c_dpre"), HD, P("wt:mlp.fc1.weight"), HD, None, P("c_dh"), D, None, None, 0, n, D, HD, 0,
          S),  # vit.py:813-814
         ("wgrad", P("c_dpre"), HD, P("c_h2"), D, n, g("mlp.fc1.weight"), g("mlp.fc1.bias"), None, None, None),  # :815
         ("es_layernorm_bwd_b16", P("c_dh"), D, P("c_xmid"), D, P("c_mean2"), P("c_rstd2"), p("norm2.weight"), P("c_dx"),
          D, P("dxm_cls"), T * D, P("c_dxmb"), D, g("norm2.weight"), g("norm2.bias"), P("ws_ln"), 1024, n, D, 0, S),
         # vit.py:817-818 (lddx = T * D)
         ("es_gemm_nt", BF16, P("c_dxmb"), D, P("wt:attn.proj.weight"), D, None, P("c_do"), D, None, None, 0, n, D, D, 0,
          S),  # vit.py:819-820
         ("wgrad", P("c_dxmb"), D, P("c_o"), D, n, g("attn.proj.weight"), g("attn.proj.bias"), None, None, None),  # :821
         ("es_attn_cls_bwd", P("qkv"), 3 * D, P("c_o"), D, P("c_lse"), P("c_do"), D, P("dqkv"), 3 * D, n, T, H, SCALE, S),
         # vit.py:822-823
         ("es_gemm_nt", BF16, P("dqkv"), 3 * D, P("wt:attn.qkv.weight"), 3 * D, None, P("dh"), D, None, None, 0, M, D,
          3 * D, 0, S)]  # vit.py:824-825
    if split:  # vit.py:830-831
        e += [("wgrad", P("dqkv", D * 2), 2 * D, P("h1"), D, M, P("g:attn.qkv.weight", D * D * 4),
               P("g:attn.qkv.bias", D * 4), 3 * D, None, None),
              ("wgrad", P("dqkv"), D, P("h1"), D, n, g("attn.qkv.weight"), g("attn.qkv.bias"), T * 3 * D, T * D, None)]
    else:  # vit.py:833
        e += [("wgrad", P("dqkv"), 3 * D, P("h1"), D, M, g("attn.qkv.weight"), g("attn.qkv.bias"), None, None, None)]
    e += [("before_ln1",),  # vit.py:834-836
          ("es_layernorm_bwd_b16", P("dh"), D, P("x"), D, P("mean1"), P("rstd1"), p("norm1.weight"), P("dxm_cls"), D,
           P("dx"), D, P("dxb_next"), D, g("norm1.weight"), g("norm1.bias"), P("ws_ln"), 1024, M, D, 0, S)]  # :837-838
    r.check(e)


def test_wrappers_outside_the_chain(monkeypatch):
    """The patch-embedding GEMM (vit.py:464-466), the casts (vit.py:798-800, conformer.py:944), the fp32 LayerNorm
    backward (vit.py:615: by dy's dtype) and the Conformer's LN1 backward without a bf16 copy (conformer.py:1001-1003)."""
    n, npatch, K0 = 4, 16, 768
    r = Rig(n, monkeypatch)
    t = r.t
    t["patches"], t["wpatch"], t["pos"], t["dhf"] = (torch.zeros(n * npatch, K0, dtype=B), torch.zeros(D, K0, dtype=B),
                                                     torch.zeros(T * D), torch.zeros(n * T + 8, D))
    block.gemm_nt(r.call, PATCH, t["patches"], t["wpatch"], t["p:attn.proj.bias"], t["x"], n * npatch, D, K0, aux=t["pos"],
                  ldaux=D, npatch=npatch)
    block.cast_f32_bf16(r.call, t["dx"], t["dxb"], n * T * D)
    r.ln_bwd(t["dhf"], t["x"], t["mean1"], t["rstd1"], t["p:norm1.weight"], t["dxm"], t["dx"], t["dxb_next"],
             t["g:norm1.weight"], t["g:norm1.bias"], n * T)
    r.ln_bwd(t["dh"], t["x"], t["mean1"], t["rstd1"], t["p:norm1.weight"], t["dxm"], t["dx"], None, t["g:norm1.weight"],
             t["g:norm1.bias"], n * T)
    ln = (P("x"), D, P("mean1"), P("rstd1"), p("norm1.weight"), P("dxm"), D, P("dx"), D)
    tail = (g("norm1.weight"), g("norm1.bias"), P("ws_ln"), 1024, n * T, D, 0, S)
    r.check([("es_gemm_nt", PATCH, P("patches"), K0, P("wpatch"), K0, p("attn.proj.bias"), P("x"), D, None, P("pos"), D,
              n * npatch, D, K0, npatch, S),
             ("es_cast_f32_bf16", P("dx"), P("dxb"), n * T * D, S),
             ("es_layernorm_bwd", P("dhf"), D) + ln + (P("dxb_next"), D) + tail,
             ("es_layernorm_bwd_b16", P("dh"), D) + ln + (None, 0) + tail])


def test_tn_table_fill():
    """The es_tn_problem fill (vit.py:966-968, 1006-1008; conformer.py:292-295)."""
    t = [torch.zeros(8) for _ in range(4)]
    orig, block.ptr = block.ptr, lambda x: None if x is None else x.data_ptr()
    try:
        tab = block.tn_table([(t[0], 384, t[1], 192, 1000, t[2], t[3], 1152, 192, "label"),
                              (t[1], 768, t[0], 384, 64, t[3], None, 768, 6528)])
    finally:
        block.ptr = orig
    e = tab[0]
    assert (e.dy, e.x, e.out, e.bias_out) == tuple(x.data_ptr() for x in t)
    assert (e.M, e.N1, e.N2, e.ld1, e.ld2) == (1000, 384, 192, 1152, 192)
    e = tab[1]
    assert (e.dy, e.x, e.out, e.bias_out) == (t[1].data_ptr(), t[0].data_ptr(), t[3].data_ptr(), None)
    assert (e.M, e.N1, e.N2, e.ld1, e.ld2) == (64, 768, 384, 768, 6528)
