"""The transformer block's launch chain, written once for the ViT engine (vit.Engine) and the Conformer's
transformer branch (conformer._BlockFn).

  * Launch wrappers: one per C-ABI entry point of the chain, the only code that knows its argument order.  They take
    tensors; a leading dimension is the tensor's row stride unless passed (the few strided operands); the stream is
    the current one unless a chain piece, which reads it once, hands it in.
  * `Chain`: the block in four pieces (attention half and MLP half, forward and reverse) over a row set (`Rows`).
  * The grouped weight-gradient launch (es_gemm_tn_big_grouped), its problem table and its stream context.
"""
import contextlib
import ctypes

import torch

from . import _lib
from ._lib import ptr, stream

EPI_BF16, EPI_GELU, EPI_F32_RESID, EPI_DGELU, EPI_F32, EPI_PATCH, EPI_GELU_ACT, EPI_GELU_D, EPI_MULAUX = range(9)
ATTN_SCALE = 64 ** -0.5  # head_dim 64 (the attention kernels' only shape)


# ------------------------------------------------------------------------------------ launch wrappers
def gemm_nt(call, epi, a, w, bias, c, M, N, K, c2=None, aux=None, ldc=None, ldaux=None, npatch=0, s=None):
    """c[M, N] = epilogue(a[M, K] w[N, K]^T + bias); c2 / aux: the epilogue's second output / extra input."""
    call("es_gemm_nt", epi, ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(c), ldc or c.stride(0), ptr(c2),
         ptr(aux), 0 if aux is None else ldaux or aux.stride(0), M, N, K, npatch, stream() if s is None else s)


def gemm_nt_resid_ln(call, a, w, bias, xmid, xin, gamma, beta, h, mean, rstd, M, N, K, eps, s=None):
    """xmid = xin + a w^T + bias and h, mean, rstd = LayerNorm(xmid) in one launch."""
    call("es_gemm_nt_resid_ln", ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(xmid), xmid.stride(0),
         ptr(xin), xin.stride(0), ptr(gamma), ptr(beta), ptr(h), h.stride(0), ptr(mean), ptr(rstd), M, N, K, eps,
         stream() if s is None else s)


def gemm_nt_ln(call, a, w, bias, xout, xmid, gamma, beta, h, mean, rstd, M, N, K, eps, s=None):
    """xout = xmid + a w^T + bias and h, mean, rstd = LayerNorm(xout) in one launch (N = 384, K % 64 == 0)."""
    call("es_gemm_nt_ln", ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(xout), xout.stride(0), ptr(xmid),
         xmid.stride(0), ptr(gamma), ptr(beta), ptr(h), h.stride(0), ptr(mean), ptr(rstd), M, N, K, eps,
         stream() if s is None else s)


def layernorm_fwd(call, x, gamma, beta, y, mean, rstd, M, D, eps, s=None):
    call("es_layernorm_fwd", ptr(x), x.stride(0), ptr(gamma), ptr(beta), ptr(y), y.stride(0), ptr(mean), ptr(rstd), M,
         D, eps, stream() if s is None else s)


def layernorm_bwd(call, dy, x, mean, rstd, gamma, dres, dx, dxb, dgamma, dbeta, ws, blocks, M, D, accumulate,
                  lddx=None, s=None):
    """dx = dres + LN'(dy) (dxb: its bf16 copy, or None); dgamma / dbeta reduced from `ws`, or, both None, their
    per-workgroup partials left in it.  The bf16-dy form by dy's dtype."""
    call("es_layernorm_bwd_b16" if dy.dtype == torch.bfloat16 else "es_layernorm_bwd", ptr(dy), dy.stride(0), ptr(x),
         x.stride(0), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), dres.stride(0), ptr(dx), lddx or dx.stride(0),
         ptr(dxb), 0 if dxb is None else dxb.stride(0), ptr(dgamma), ptr(dbeta), ptr(ws), blocks, M, D, accumulate,
         stream() if s is None else s)


def attn_fwd(call, qkv, o, lse, n, T, H, s=None, cls=False):
    """cls: the CLS queries only, over all keys (o / lse compact: [n, D] / [n * H])."""
    call("es_attn_cls_fwd" if cls else "es_attn_fwd", ptr(qkv), qkv.stride(0), ptr(o), o.stride(0), ptr(lse), n, T, H,
         ATTN_SCALE, stream() if s is None else s)


def attn_bwd(call, qkv, o, lse, delta, do, dqkv, n, T, H, s=None):
    call("es_attn_bwd", ptr(qkv), qkv.stride(0), ptr(o), o.stride(0), ptr(lse), ptr(delta), ptr(do), do.stride(0),
         ptr(dqkv), dqkv.stride(0), n, T, H, ATTN_SCALE, stream() if s is None else s)


def attn_cls_bwd(call, qkv, o, lse, do, dqkv, n, T, H, s=None):
    call("es_attn_cls_bwd", ptr(qkv), qkv.stride(0), ptr(o), o.stride(0), ptr(lse), ptr(do), do.stride(0), ptr(dqkv),
         dqkv.stride(0), n, T, H, ATTN_SCALE, stream() if s is None else s)


def cast_f32_bf16(call, src, dst, numel, s=None):
    call("es_cast_f32_bf16", ptr(src), ptr(dst), numel, stream() if s is None else s)


# ------------------------------------------------------------------------------------ the chain
nop = lambda *args: None  # noqa: E731 -- a callback the owner does not use


class Rows:
    """A row set: the block's buffers, by the chain's names, for n images of T token rows each (T = 1: compact CLS
    rows).  ldx / lddxm: the row strides of x and d(xmid) where they are the CLS rows of a full token buffer."""

    def __init__(self, n, T, H, ldx=None, lddxm=None, **bufs):
        self.n, self.T, self.rows, self.ldx, self.lddxm = n, T, n * T, ldx, lddxm
        self.__dict__.update(bufs)


class Chain:
    """One owner's block chain.  p(name) / g(name): the fp32 parameter / its gradient; wb / wt: the bf16 weight
    images W [N, K] / W^T [K, N] by parameter name; b: a block's name prefix.  The reverse pieces take the owner's
    ln_bwd(dy, x, mean, rstd, gamma, dres, dx, dxb, dgamma, dbeta, M, lddx=) and its callbacks, each called at its
    place in the launch order: wgrad(dy, N1, x, N2, M, out, bias_out, ld1=, ld2=, label=) for out = dy^T x once dy
    is made, before_ln1() once all the block's weight gradients are recorded, cap(kind, *tensors): the test hook."""

    def __init__(self, call, p, g, wb, wt, heads, eps, gelu_d=True, dh_bf16=True, bracket=lambda lb, fl, f: f()):
        self.call, self.p, self.g, self.wb, self.wt, self.heads, self.eps = call, p, g, wb, wt, heads, eps
        self.gelu_d = gelu_d  # the train fc1 stores GELU'(pre) for the fc2 data gradient to multiply by
        self.epi_dh = EPI_BF16 if dh_bf16 else EPI_F32  # d(LN output) from the fc1 / qkv data gradients
        self.bracket = bracket  # the owner's launch of a labelled site (Engine._bracket: timed when probed)

    def attn_fwd(self, b, R, cls=None, split_q=False, ln_done=False):
        """LN1 -> qkv GEMM -> attention.  cls (a pruned last block's compact row set): the CLS queries' attention
        only, into cls.o / cls.lse; split_q: Q for the CLS rows only (gathered into cls.h1), onto their rows of qkv;
        ln_done: R.h1 / R.mean1 / R.rstd1 are there already (the previous block's mlp_fwd(next_ln=) wrote them)."""
        call, p, s, M, D = self.call, self.p, stream(), R.rows, R.h1.shape[1]
        if not ln_done:
            layernorm_fwd(call, R.x, p(b + "norm1.weight"), p(b + "norm1.bias"), R.h1, R.mean1, R.rstd1, M, D,
                          self.eps, s)
        w, bias = self.wb[b + "attn.qkv.weight"], p(b + "attn.qkv.bias")
        if cls is not None and split_q:
            gemm_nt(call, EPI_BF16, R.h1, w[D:], bias[D:], R.qkv[:, D:], M, 2 * D, D, s=s)
            cls.h1[:R.n].copy_(R.h1[:M].view(R.n, R.T, D)[:, 0])
            gemm_nt(call, EPI_BF16, cls.h1, w[:D], bias[:D], R.qkv, R.n, D, D, ldc=R.T * 3 * D, s=s)
        else:
            gemm_nt(call, EPI_BF16, R.h1, w, bias, R.qkv, M, 3 * D, D, s=s)
        Ro = R if cls is None else cls
        attn_fwd(call, R.qkv, Ro.o, Ro.lse, R.n, R.T, self.heads, s, cls is not None)

    def mlp_fwd(self, b, R, train, fused=False, label=None, next_ln=None):
        """proj + residual -> LN2 -> fc1 -> fc2 (fused: the first two as one es_gemm_nt_resid_ln launch).  train:
        fc1 keeps R.pre for the backward beside R.act; label: the fc1 launch goes through the owner's bracket.
        next_ln = (gamma, beta, h1, mean1, rstd1) of the next block: fc2, its residual add and that block's
        LayerNorm 1 as one es_gemm_nt_ln launch (the next attn_fwd then takes ln_done=True)."""
        call, p, wb, s, M = self.call, self.p, self.wb, stream(), R.rows
        D, Hd = R.h2.shape[1], R.act.shape[1]
        if fused:
            gemm_nt_resid_ln(call, R.o, wb[b + "attn.proj.weight"], p(b + "attn.proj.bias"), R.xmid, R.x,
                             p(b + "norm2.weight"), p(b + "norm2.bias"), R.h2, R.mean2, R.rstd2, M, D, D, self.eps, s)
        else:
            gemm_nt(call, EPI_F32_RESID, R.o, wb[b + "attn.proj.weight"], p(b + "attn.proj.bias"), R.xmid, M, D, D,
                    aux=R.x, ldaux=R.ldx, s=s)
            layernorm_fwd(call, R.xmid, p(b + "norm2.weight"), p(b + "norm2.bias"), R.h2, R.mean2, R.rstd2, M, D,
                          self.eps, s)
        epi, c, c2 = (EPI_GELU_D if self.gelu_d else EPI_GELU, R.pre, R.act) if train else (EPI_GELU_ACT, R.act, None)
        fc1 = lambda: gemm_nt(call, epi, R.h2, wb[b + "mlp.fc1.weight"], p(b + "mlp.fc1.bias"), c, M, Hd, D,  # noqa: E731
                              c2=c2, s=s)
        self.bracket(label, 2.0 * M * Hd * D, fc1)
        if next_ln is not None:
            gamma, beta, h1, mean1, rstd1 = next_ln
            gemm_nt_ln(call, R.act, wb[b + "mlp.fc2.weight"], p(b + "mlp.fc2.bias"), R.out, R.xmid, gamma, beta, h1,
                       mean1, rstd1, M, D, Hd, self.eps, s)
            return
        gemm_nt(call, EPI_F32_RESID, R.act, wb[b + "mlp.fc2.weight"], p(b + "mlp.fc2.bias"), R.out, M, D, Hd,
                aux=R.xmid, s=s)

    def mlp_bwd(self, b, R, ln_bwd, wgrad=None, cap=nop, label=None):
        """fc2 data gradient -> fc1 data gradient -> LN2 backward -> proj data gradient: R.dxb (bf16 d(block
        output)) and R.dres (its fp32 residual path) -> R.dxm / R.dxmb and R.do.  label: the fc1 weight gradient's."""
        call, p, g, wt, s, M = self.call, self.p, self.g, self.wt, stream(), R.rows
        D, Hd = R.dxb.shape[1], R.dpre.shape[1]
        cap("b_dxb", R.dxb)
        gemm_nt(call, EPI_MULAUX if self.gelu_d else EPI_DGELU, R.dxb, wt[b + "mlp.fc2.weight"], None, R.dpre, M, Hd, D,
                aux=R.pre, s=s)
        if wgrad is not None:
            wgrad(R.dxb, D, R.act, Hd, M, g(b + "mlp.fc2.weight"), g(b + "mlp.fc2.bias"))
        gemm_nt(call, self.epi_dh, R.dpre, wt[b + "mlp.fc1.weight"], None, R.dh, M, D, Hd, s=s)
        if wgrad is not None:
            wgrad(R.dpre, Hd, R.h2, D, M, g(b + "mlp.fc1.weight"), g(b + "mlp.fc1.bias"), label=label)
        cap("b_dpre", R.dpre)
        cap("b_dh2", R.dh)
        ln_bwd(R.dh, R.xmid, R.mean2, R.rstd2, p(b + "norm2.weight"), R.dres, R.dxm, R.dxmb, g(b + "norm2.weight"),
               g(b + "norm2.bias"), M, lddx=R.lddxm)
        gemm_nt(call, EPI_BF16, R.dxmb, wt[b + "attn.proj.weight"], None, R.do, M, D, D, s=s)
        if wgrad is not None:
            wgrad(R.dxmb, D, R.o, D, M, g(b + "attn.proj.weight"), g(b + "attn.proj.bias"))
        cap("b_dxm", R.dxm, R.dxmb)
        cap("b_do", R.do)

    def attn_bwd(self, b, R, ln_bwd, wgrad=None, before_ln1=nop, cap=nop, cls=None, split_q=False):
        """attention backward -> qkv data gradient -> LN1 backward: R.do and R.dxm -> R.dx / R.dxb_next (read after
        before_ln1()).  cls: the CLS queries' attention of a pruned last block, dqkv a full token image; split_q: the
        Q weight gradient over the CLS rows, the only ones with a nonzero dQ (rows img * T of dqkv and h1)."""
        call, p, g, s, M, T = self.call, self.p, self.g, stream(), R.rows, R.T
        D = R.dh1.shape[1]
        if cls is None:
            attn_bwd(call, R.qkv, R.o, R.lse, R.delta, R.do, R.dqkv, R.n, T, self.heads, s)
        else:
            attn_cls_bwd(call, R.qkv, cls.o, cls.lse, cls.do, R.dqkv, R.n, T, self.heads, s)
        gemm_nt(call, self.epi_dh, R.dqkv, self.wt[b + "attn.qkv.weight"], None, R.dh1, M, D, 3 * D, s=s)
        if wgrad is not None:
            gw, gb = g(b + "attn.qkv.weight"), g(b + "attn.qkv.bias")
            if cls is not None and split_q:
                wgrad(R.dqkv[:, D:], 2 * D, R.h1, D, M, gw[D * D:], gb[D:], ld1=3 * D)
                wgrad(R.dqkv, D, R.h1, D, R.n, gw[:D * D], gb[:D], ld1=T * 3 * D, ld2=T * D)
            else:
                wgrad(R.dqkv, 3 * D, R.h1, D, M, gw, gb)
        cap("b_dqkv", R.dqkv)
        cap("b_dh1", R.dh1)
        before_ln1()
        ln_bwd(R.dh1, R.x, R.mean1, R.rstd1, p(b + "norm1.weight"), R.dxm, R.dx, R.dxb_next, g(b + "norm1.weight"),
               g(b + "norm1.bias"), M)


# ------------------------------------------------------------------------------------ grouped weight gradients
class _TNProblem(ctypes.Structure):
    """es_tn_problem (include/endossl.h): one GEMM of a grouped weight-gradient launch."""
    _fields_ = [("dy", ctypes.c_void_p), ("x", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("bias_out", ctypes.c_void_p), ("M", ctypes.c_int), ("N1", ctypes.c_int), ("N2", ctypes.c_int),
                ("ld1", ctypes.c_int), ("ld2", ctypes.c_int), ("mchunk", ctypes.c_int), ("tile0", ctypes.c_int),
                ("pad", ctypes.c_int)]


def on_stream(st, *after):
    """The context of stream `st` once it waits for the streams `after` (st None: the current stream as it is)."""
    if st is None:
        return contextlib.nullcontext()
    for w in after:
        st.wait_stream(w)
    return torch.cuda.stream(st)


def tn_table(problems):
    """The es_tn_problem table of problems = [(dy, N1, x, N2, M, out, bias_out, ld1, ld2, ...)]: out = dy^T x over
    M rows of row strides ld1 / ld2, bias_out (or None) = column sums of dy."""
    tab = (_TNProblem * len(problems))()
    for e, q in zip(tab, problems):
        e.dy, e.x, e.out, e.bias_out = ptr(q[0]), ptr(q[2]), ptr(q[5]), ptr(q[6])
        e.N1, e.N2, e.M, e.ld1, e.ld2 = q[1], q[3], q[4], q[7], q[8]
    return tab


def tn_big_grouped(problems, target, workspace, timed=None):
    """One es_gemm_tn_big_grouped launch (384 x 192 tiles, split-K sized to `target` workgroups) + its reduce over
    `problems` (tn_table's form) on the current stream, outputs overwritten; the table travels in the kernel arguments
    (capturable).  workspace(need): the fp32 slab; timed: two _lib.KernelEvent.  Returns the launch dims."""
    lib = _lib.load()
    n, tab = len(problems), tn_table(problems)
    need = lib.es_gemm_tn_big_grouped_workspace(ctypes.byref(tab), n, target)
    ws = workspace(need)
    if need > ws.numel():
        raise RuntimeError(f"grouped weight-gradient workspace too small: {need} > {ws.numel()} floats")
    raw = ctypes.create_string_buffer(lib.es_gemm_tn_big_grouped_table_bytes(n))
    dims = (ctypes.c_int * 3)()
    rc = lib.es_gemm_tn_big_grouped_prepare(ctypes.byref(tab), n, target, ptr(ws), ws.numel(), raw, dims)
    if rc != 0:
        raise _lib.EndosslLibraryError(f"es_gemm_tn_big_grouped_prepare: status {rc}")
    if timed is None:
        _lib.call("es_gemm_tn_big_grouped", raw, n, dims, stream())
    else:
        _lib.call("es_gemm_tn_big_grouped_timed", raw, n, dims, timed[0].handle, timed[1].handle, stream())
    return dims
