"""The selection patterns of tests/attn_patterns.py, checked without a GPU: the builders' input conditions hold at
every shape test_gpu_attention_exact.py uses, and float64 autograd of plain softmax attention reproduces the closed
forms to 1e-30 -- so the GPU test is never "exact" against a wrong expectation."""
import pytest
import torch

import attn_patterns as ap

TOL = 1e-30


@pytest.mark.parametrize("n,T,H", ap.ONE_HOT_SHAPES)
def test_one_hot_closed_forms(n, T, H):
    D = H * ap.HD
    for integer_v in (False, True):
        p = ap.one_hot(n, T, H, integer_v=integer_v)
        assert p["margin"] >= ap.MARGIN and p["qkv"].shape == (n * T, 3 * D) and p["qkv"].dtype == torch.bfloat16
        # q = 64 k_pi: entries +-64; k: +-1; each pi a permutation
        assert (p["qkv"][:, :D].float().abs() == 64).all() and (p["qkv"][:, D:2 * D].float().abs() == 1).all()
        assert (p["pi"].sort(-1).values == torch.arange(T)).all()
        x = p["qkv"].double().requires_grad_(True)
        o, lse = ap.attention_ref(x, n, T, H)
        assert (o.detach() - p["o"].double()).abs().max().item() < TOL
        assert (lse - p["lse"]).abs().max().item() < 1e-12  # 512 + log(1 + residues): float64 rounding of 512
        if not integer_v:
            continue
        v = p["qkv"][:, 2 * D:].float()
        assert (v == v.round()).all() and v.abs().max() <= 3
        assert (p["dout"].float() == p["dout"].float().round()).all() and p["dout"].float().abs().max() <= 3
        o.backward(p["dout"].double())
        gq, gk, gv = x.grad[:, :D], x.grad[:, D:2 * D], x.grad[:, 2 * D:]
        assert gq.abs().max().item() < TOL and gk.abs().max().item() < TOL
        assert (gv - p["dv"].double()).abs().max().item() < TOL
        delta = (p["dout"].double() * p["o"].double()).view(n, T, H, ap.HD).sum(-1).permute(0, 2, 1)
        assert torch.equal(delta.float(), p["delta"]) and (p["delta"] == p["delta"].round()).all()


@pytest.mark.parametrize("n,T,H", ap.ONE_HOT_SHAPES)
def test_one_hot_in_fp32(n, T, H):
    """The same in fp32 torch, whose exp is exactly zero below the margin: the closed forms bit for bit."""
    p = ap.one_hot(n, T, H, integer_v=True)
    D = H * ap.HD
    x = p["qkv"].float().requires_grad_(True)
    o, lse = ap.attention_ref(x, n, T, H, dtype=torch.float32)
    assert torch.equal(o.detach(), p["o"].float()) and (lse == 512.0).all()
    o.backward(p["dout"].float())
    assert (x.grad[:, :2 * D] == 0).all() and torch.equal(x.grad[:, 2 * D:], p["dv"].float())


@pytest.mark.parametrize("n,T,H", ap.TWO_HOT_SHAPES)
def test_two_hot_closed_forms(n, T, H):
    """two_hot asserts its own input conditions (scores 128 / 0, two picks per query and per key) and that float64
    autograd lands on bf16 numbers; here its o against the closed form (v_a + v_b) / 2, dV against
    (dO_i / 2 summed over the two queries that pick the key), and nonzero dQ and dK (the pattern's purpose)."""
    p = ap.two_hot(n, T, H)
    D = H * ap.HD
    v = p["qkv"][:, 2 * D:].double().view(n, T, H, ap.HD).permute(0, 2, 1, 3)
    ia, ib = (t.unsqueeze(-1).expand(n, H, T, ap.HD) for t in (p["a"], p["b"]))
    o = 0.5 * (v.gather(2, ia) + v.gather(2, ib))
    assert torch.equal(ap._rows(o), p["o"].double())
    do = p["dout"].double().view(n, T, H, ap.HD).permute(0, 2, 1, 3)
    dv = torch.zeros_like(v).scatter_add_(2, ia, 0.5 * do).scatter_add_(2, ib, 0.5 * do)
    assert torch.equal(ap._rows(dv), p["dqkv"][:, 2 * D:].double())
    assert p["dqkv"][:, :D].float().abs().max() > 0 and p["dqkv"][:, D:2 * D].float().abs().max() > 0
    assert (p["lse"] - (128.0 + torch.log(torch.tensor(2.0, dtype=torch.float64)))).abs().max().item() < 1e-12
    # the hadamard rows are orthogonal
    h = ap.hadamard64()
    assert torch.equal(h @ h.t(), 64.0 * torch.eye(64, dtype=torch.float64))
