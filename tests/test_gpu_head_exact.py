"""The loss kernels (csrc/losses.hip: consistency, poly-CE, weighted CE and its data-parallel form) and every CoMatch
head / step kernel (csrc/comatch.hip) on the MI355X against the float64 restatements of tests/head_cases.py, in the
style of the other exact files:

  * integer operands where the result is then independent of the summation order (dense, l2norm, bank write, the
    dropout hash): torch.equal; random floats against float64 at the project's bars for these kernels -- losses.hip
    values rtol 1e-5 / atol 1e-6, gradients rtol 1e-4 / atol 1e-7, CoMatch kernels rtol 1e-4 / atol 1e-6;
  * every operand and output with a leading dimension also as a strided view (ld = width + 3): NaN in the input gaps,
    a sentinel in the output gaps and in a guard row before and after, which must survive bit for bit, and the
    strided results torch.equal to the packed ones;
  * outputs and workspaces pre-filled with NaN (the accumulate_dx prior and the running buffers excepted);
  * a second launch on the same inputs gives the same bits, for every entry point;
  * refusals through lib.es_* directly: the status, and the outputs left as they were.

Entry point -> the tests here that call it directly:
  es_fm_consistency_fwd_bwd       test_consistency_*, test_losses_stay_finite_..., test_loss_refusals
  es_poly_ce_fwd_bwd              test_poly_and_weighted_ce_shapes, test_invalid_target_..., test_losses_stay_finite_...
  es_ce_weighted_fwd_bwd, es_ce_weight_sum, es_ce_weighted_fwd_bwd_global
                                  the same three, and test_weighted_ce_global_form; test_loss_refusals
  es_dense_fwd / es_dense_bwd (+ _workspace)   test_dense_exact_on_integers, test_dense_refusals
  es_bn1d_fwd / es_bn1d_bwd       test_bn1d_vs_float64, test_bn1d_refusals
  es_bn1d_sums, es_bn1d_fwd_global, es_bn1d_bwd_sums, es_bn1d_bwd_global
                                  test_sync_bn1d_shards_vs_float64_and_one_process, test_bn1d_refusals
  es_l2norm_fwd / es_l2norm_bwd   test_l2norm_exact_and_vs_float64, test_l2norm_refusals
  es_comatch_pseudo / _ex (+ _workspace)   test_pseudo_sizes_vs_float64, test_pseudo_history_ring,
                                  test_pseudo_deterministic_ties, test_pseudo_refusals
  es_softmax_colmean              test_softmax_colmean_*
  es_comatch_bank_write           test_bank_write_exact, test_bank_write_bounds
  es_comatch_contrastive_fwd_bwd / _ex (+ workspaces)   test_contrastive_*
  es_comatch_focal_fwd_bwd        test_focal_vs_float64, test_focal_refusals
  es_dropout_keep                 test_dropout_keep_byte_exact, test_dropout_keep_refusals
(es_softmax_predict, es_triplet_fwd_bwd and es_margin_softmax_fwd_bwd have test_gpu_triplet.py / test_gpu_margin.py.)

Labels and masks are compared on decidable rows only (head_cases.DECIDE; test_head_cases_cpu.py caps the undecidable
rows at 2% from the reference alone).  Each measured error is printed in units of its bar before it is asserted.
"""
import numpy as np
import pytest
import torch

import head_cases as hc

pytestmark = pytest.mark.gpu

from endossl import _lib  # noqa: E402
from endossl._lib import ptr  # noqa: E402

DEV = "cuda"
NAN = float("nan")
OK, BAD_SHAPE, BAD_ARG = 0, -1, -2
PAD = 3
# sentinel (gaps and guard rows) and pre-fill (the entries a launch must write) per dtype
SENT = {torch.float32: -1234.5, torch.int32: -77, torch.uint8: 0xEE, torch.int64: -77}
FILL = {torch.float32: NAN, torch.int32: -99, torch.uint8: 0xDD, torch.int64: -99}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _lib.load()


_ALIVE = []  # the device inputs of the running test: a pointer handed to a launch must outlive it


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def L():
    return _lib.load()


def S():
    return _lib.stream()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    """Bit-identical (NaN included); tensors or dicts of tensors / None."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def inp(t, pad=0):
    """An input of leading dimension width + pad on the device, the gap columns poisoned with NaN; kept alive until
    the test ends."""
    if t is None:
        return None
    if pad == 0 or not t.is_floating_point():
        buf = t.contiguous()
    else:
        buf = torch.full((t.shape[0], t.shape[1] + pad), NAN)
        buf[:, :t.shape[1]] = t
    _ALIVE.append(buf.to(DEV))
    return _ALIVE[-1]


class Out:
    """An output of n rows x w columns at leading dimension w + pad: the entries a launch must write pre-filled
    (NaN for floats, or `init`), the gap columns and one guard row before and after holding a sentinel."""

    def __init__(self, n, w, pad=0, dtype=torch.float32, init=None):
        self.n, self.w, self.ld, self.dtype = n, w, w + pad, dtype
        self.full = torch.full((n + 2, self.ld), SENT[dtype], dtype=dtype)
        self.full[1:n + 1, :w] = FILL[dtype] if init is None else init.view(n, w)
        self.full = self.full.to(DEV)
        self.view = self.full[1:n + 1]

    @property
    def p(self):
        return self.view.data_ptr()

    def get(self):
        """The written entries on the CPU, after checking that the sentinel survived around them."""
        f = self.full.cpu()
        g = f.clone()
        g[1:self.n + 1, :self.w] = SENT[self.dtype]
        assert torch.all(g == SENT[self.dtype]), "a gap or guard entry was overwritten"
        return f[1:self.n + 1, :self.w].contiguous()

    def vec(self):
        return self.get().reshape(-1)

    def untouched(self):
        v = self.get()
        return bool(torch.isnan(v).all()) if self.dtype == torch.float32 else bool(torch.all(v == FILL[self.dtype]))


def nanbuf(k):
    return torch.full((max(int(k), 1),), NAN, device=DEV)


def close(got, want, tag, rtol, atol):
    want = torch.as_tensor(want, dtype=torch.float64)
    got = torch.as_tensor(got).double()
    print(f"{tag}: {hc.bar_units(got, want, rtol, atol):.3g} of the bar (rtol {rtol:g}, atol {atol:g})")
    assert torch.isfinite(got).all(), tag
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda m: f"{tag}: {m}")


def all_ways(run, **kw):
    """Packed, packed again (the same bits), and strided (the same bits once more); returns the packed result."""
    a = run(pad=0, **kw)
    assert same(a, run(pad=0, **kw)), "a second launch gave other bits"
    assert same(a, run(pad=PAD, **kw)), "the strided layout gave other bits"
    return a


# ====================================================================================== losses.hip
def run_consistency(lw, ls, tau, gs, pad=0, null=(), ov=None, rc=OK):
    n, C = ls.shape
    o = {"pl": Out(n, 1, dtype=torch.int32), "mask": Out(n, 1, dtype=torch.uint8), "rows": Out(n, 1),
         "dls": Out(n, C, pad), "out": Out(1, 2)}
    a = dict(n=n, C=C, ldw=C + pad, lds=C + pad, lddls=C + pad, lw=ptr(inp(lw, pad)), ls=ptr(inp(ls, pad)))
    a.update(ov or {})
    p = {k: (None if k in null else v.p) for k, v in o.items()}
    got = L().es_fm_consistency_fwd_bwd(a["lw"], a["ldw"], a["ls"], a["lds"], a["n"], a["C"], tau, gs, p["pl"], p["mask"],
                                        p["rows"], p["dls"], a["lddls"], p["out"], S())
    torch.cuda.synchronize()
    assert got == rc, (got, rc)
    if rc != OK:
        assert all(v.untouched() for v in o.values())
        return None
    for k in null:
        assert o[k].untouched()
    return {k: v.get() for k, v in o.items() if k not in null}


def check_consistency(o, r, n, tag, rows_atol=None):
    ok = r["label_ok"] & r["mask_ok"]
    assert torch.equal(o["pl"].view(-1).long()[r["label_ok"]], r["idx"][r["label_ok"]])
    assert torch.equal(o["mask"].view(-1).double()[ok], r["mask"][ok])
    close(o["rows"].view(-1)[ok], r["rows"][ok], tag + " rows", rtol=hc.LOSS_VAL["rtol"],
          atol=rows_atol or hc.LOSS_VAL["atol"])
    close(o["dls"][ok], r["dls"][ok], tag + " dls", **hc.LOSS_GRAD)
    close(o["out"][0, 0], o["rows"].double().mean(), tag + " out[0] vs mean(rows)", rtol=1e-6, atol=0)
    if bool(ok.all()):
        close(o["out"][0, 0], r["loss"], tag + " loss", **hc.LOSS_VAL)
        assert abs(o["out"][0, 1].item() - r["mask_mean"]) <= 1e-6
    assert torch.all(o["dls"][o["mask"].view(-1) == 0] == 0)  # unmasked rows: exact zeros


@pytest.mark.parametrize("n,C", hc.LOSS_SHAPES)
def test_consistency_shapes(n, C):
    lw, ls = hc.consistency_case(n, C)
    tau = hc.loss_tau(n, C)
    r = hc.consistency64(lw, ls, tau, 1.0 / n)
    o = all_ways(run_consistency, lw=lw, ls=ls, tau=tau, gs=1.0 / n)
    check_consistency(o, r, n, f"consistency n{n} C{C}")
    for null in (("pl",), ("mask",), ("rows",), ("pl", "mask", "rows")):
        q = run_consistency(lw, ls, tau, 1.0 / n, pad=PAD, null=null)
        assert same(q, {k: v for k, v in o.items() if k not in null}), null


def test_consistency_ties_and_last_class():
    lw, ls, want = hc.consistency_ties_case()
    o = all_ways(run_consistency, lw=lw, ls=ls, tau=0.0, gs=1.0)
    assert torch.equal(o["pl"].view(-1).long(), want)
    assert torch.all(o["mask"] == 1) and o["out"][0, 1].item() == 1.0  # tau = 0: mask mean exactly 1
    r = hc.consistency64(lw, ls, 0.0, 1.0)
    close(o["dls"], r["dls"], "ties dls", **hc.LOSS_GRAD)


def test_consistency_threshold_is_inclusive_on_bits():
    """C = 1: p = 1.0 exactly at tau = 1.0; C = 2 with equal logits: p = 0.5 exactly at tau = 0.5."""
    g = hc.gen(3)
    for C, tau in ((1, 1.0), (2, 0.5)):
        lw = (torch.randn(7, 1, generator=g) * 3).expand(7, C).contiguous()
        ls = hc.logits(7, C, 5)
        o = all_ways(run_consistency, lw=lw, ls=ls, tau=tau, gs=1.0 / 7)
        assert torch.all(o["mask"] == 1) and o["out"][0, 1].item() == 1.0 and torch.all(o["pl"] == 0)


def test_consistency_threshold_extremes():
    lw, ls = hc.consistency_case(257, 23)
    o = all_ways(run_consistency, lw=lw, ls=ls, tau=0.0, gs=1.0 / 257)
    assert o["out"][0, 1].item() == 1.0 and torch.all(o["mask"] == 1)
    o = all_ways(run_consistency, lw=lw, ls=ls, tau=1.5, gs=1.0 / 257)
    assert o["out"][0, 0].item() == 0.0 and o["out"][0, 1].item() == 0.0
    assert torch.all(o["dls"] == 0) and torch.all(o["rows"] == 0) and torch.all(o["mask"] == 0)


def run_poly(l, y, w, gs, pad=0, eps=2.0, ov=None, rc=OK):
    n, C = l.shape
    dl, out = Out(n, C, pad), Out(1, 1)
    a = dict(n=n, C=C, ldl=C + pad, lddl=C + pad, l=ptr(inp(l, pad)), y=ptr(inp(y)), dl=dl.p, out=out.p)
    a.update(ov or {})
    got = L().es_poly_ce_fwd_bwd(a["l"], a["ldl"], a["y"], ptr(inp(w)), a["n"], a["C"], eps, gs, a["dl"], a["lddl"],
                                 a["out"], S())
    torch.cuda.synchronize()
    assert got == rc, (got, rc)
    if rc != OK:
        assert dl.untouched() and out.untouched()
        return None
    return {"dl": dl.get(), "out": out.vec()}


def run_cew(l, y, w, gs, pad=0, wsum=None, ov=None, rc=OK):
    """es_ce_weighted_fwd_bwd, or its _global form when wsum (a device tensor) is given."""
    n, C = l.shape
    dl, out = Out(n, C, pad), Out(1, 1)
    a = dict(n=n, C=C, ldl=C + pad, lddl=C + pad, l=ptr(inp(l, pad)), y=ptr(inp(y)), dl=dl.p, out=out.p)
    a.update(ov or {})
    if wsum is None:
        got = L().es_ce_weighted_fwd_bwd(a["l"], a["ldl"], a["y"], ptr(inp(w)), a["n"], a["C"], gs, a["dl"], a["lddl"],
                                         a["out"], S())
    else:
        got = L().es_ce_weighted_fwd_bwd_global(a["l"], a["ldl"], a["y"], ptr(inp(w)), ptr(wsum), a["n"], a["C"], gs,
                                                a["dl"], a["lddl"], a["out"], S())
    torch.cuda.synchronize()
    assert got == rc, (got, rc)
    if rc != OK:
        assert dl.untouched() and out.untouched()
        return None
    return {"dl": dl.get(), "out": out.vec()}


def run_wsum(y, w, C, rc=OK, n=None):
    out = Out(1, 1)
    got = L().es_ce_weight_sum(ptr(inp(y)), ptr(inp(w)), y.shape[0] if n is None else n, C, out.p, S())
    torch.cuda.synchronize()
    assert got == rc
    if rc != OK:
        assert out.untouched()
        return None
    return out.vec()


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("n,C", hc.LOSS_SHAPES)
def test_poly_and_weighted_ce_shapes(n, C, weighted):
    l = hc.logits(n, C, 3 * n + C)
    y, w = hc.targets_case(n, C, n + C)
    w = w if weighted else None
    tag = f"n{n} C{C} {'w' if weighted else 'plain'}"
    r = hc.poly64(l, y, w, 2.0, 1.0 / n)
    o = all_ways(run_poly, l=l, y=y, w=w, gs=1.0 / n)
    close(o["out"][0], r["loss"], "poly loss " + tag, **hc.LOSS_VAL)
    close(o["dl"], r["dl"], "poly dl " + tag, **hc.LOSS_GRAD)
    r = hc.ce_weighted64(l, y, w, 1.5)
    o = all_ways(run_cew, l=l, y=y, w=w, gs=1.5)
    close(o["out"][0], r["loss"], "weighted CE loss " + tag, **hc.LOSS_VAL)
    close(o["dl"], r["dl"], "weighted CE dl " + tag, **hc.LOSS_GRAD)
    ws = run_wsum(y, w, C)
    assert same(ws, run_wsum(y, w, C))
    close(ws[0], r["wsum"], "weight sum " + tag, rtol=1e-6, atol=0)


@pytest.mark.parametrize("n,C", hc.LARGE_SHAPES)
def test_losses_stay_finite_where_a_literal_exp_overflows(n, C):
    """Logits randn * 50 (|l| to about 200): finite, and on the bars of the ordinary cases -- but for the consistency
    kernel's per-row losses at (257, 23).  A row loss is lse - l[idx] with lse ~ 200, one fp32 ulp of which is
    1.5e-5: the same formula in plain fp32 torch on the CPU misses float64 by 1.04e-5 at the worst there, 2.61 of the
    rtol 1e-5 / atol 1e-6 bar (at (600, 64): 1.41e-5, 0.95 of the bar, which therefore stays).  Where the fp32
    formula itself cannot meet the bar, the rows' atol is 4x its worst error: 4.16e-5 at (257, 23).  The figure
    comes from head_cases.consistency_rows_fp32_error, on the CPU, never from the kernel's output; the device's rows
    measured 2.61 of the ordinary bar at (257, 23).  The mean loss, the gradients, poly-CE and the weighted CE
    meet their ordinary bars."""
    lw, ls = hc.large_logits(n, C, n), hc.large_logits(n, C, n + 1)
    r = hc.consistency64(lw, ls, 0.95, 1.0 / n)
    o = all_ways(run_consistency, lw=lw, ls=ls, tau=0.95, gs=1.0 / n)
    assert all(torch.isfinite(v.double()).all() for v in o.values())
    err32, units32 = hc.consistency_rows_fp32_error(ls, r)
    print(f"fp32 formula on the CPU: worst row error {err32:.3g}, {units32:.3g} of the bar")
    check_consistency(o, r, n, f"large consistency n{n} C{C}", rows_atol=4 * err32 if units32 > 1 else None)
    y, w = hc.targets_case(n, C, n + C)
    r = hc.poly64(ls, y, w, 2.0, 1.0 / n)
    o = all_ways(run_poly, l=ls, y=y, w=w, gs=1.0 / n)
    close(o["out"][0], r["loss"], "large poly loss", **hc.LOSS_VAL)
    close(o["dl"], r["dl"], "large poly dl", **hc.LOSS_GRAD)
    r = hc.ce_weighted64(ls, y, w, 1.0)
    o = all_ways(run_cew, l=ls, y=y, w=w, gs=1.0)
    close(o["out"][0], r["loss"], "large weighted CE loss", **hc.LOSS_VAL)
    close(o["dl"], r["dl"], "large weighted CE dl", **hc.LOSS_GRAD)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("bad", hc.INVALID_TARGETS, ids=["minus1", "C", "2p31", "2p32plus3"])
def test_invalid_target_gives_nan_loss_and_no_gradient(bad, weighted):
    """One invalid 64-bit target in an otherwise valid batch: the range check is on the 64-bit value (2^32 + 3 is
    not class 3).  The weights hold exactly C entries."""
    n, C = 9, 23
    l = hc.logits(n, C, 4)
    y, w = hc.targets_case(n, C, 5)
    w = w if weighted else None
    y[4] = C if bad == "C" else bad
    rows = [i for i in range(n) if i != 4]
    r = hc.poly64(l, y, w, 2.0, 1.0 / n)
    o = all_ways(run_poly, l=l, y=y, w=w, gs=1.0 / n)
    assert torch.isnan(o["out"]).all() and torch.all(o["dl"][4] == 0)
    close(o["dl"][rows], r["dl"][rows], "poly dl of the valid rows", **hc.LOSS_GRAD)
    o = all_ways(run_cew, l=l, y=y, w=w, gs=1.0)
    assert torch.isnan(o["out"]).all() and torch.all(o["dl"][4] == 0)
    ws = run_wsum(y, w, C)
    assert torch.isnan(ws).all()
    o = run_cew(l, y, w, 1.0, wsum=ws.to(DEV))
    assert torch.isnan(o["out"]).all() and torch.all(o["dl"][4] == 0)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_weighted_ce_global_form(weighted):
    """37 rows as shards of 20 and 17 with the whole batch's weight sum: the shares add up to the single-launch
    loss, and every gradient row has the single launch's bits."""
    n, C = 37, 23
    l = hc.logits(n, C, 8)
    y, w = hc.targets_case(n, C, 9)
    w = w if weighted else None
    full = all_ways(run_cew, l=l, y=y, w=w, gs=2.0)
    ws = run_wsum(y, w, C).to(DEV)
    r = hc.ce_weighted64(l, y, w, 2.0)
    parts = [all_ways(run_cew, l=l[a:b], y=y[a:b], w=w, gs=2.0, wsum=ws) for a, b in ((0, 20), (20, 37))]
    close(parts[0]["out"].double() + parts[1]["out"].double(), full["out"].double(), "shares vs one launch", rtol=1e-6,
          atol=0)
    assert torch.equal(torch.cat([p["dl"] for p in parts]), full["dl"])
    close(full["out"][0], r["loss"], "global loss", **hc.LOSS_VAL)
    close(torch.cat([p["dl"] for p in parts]), r["dl"], "global dl", **hc.LOSS_GRAD)
    for (a, b), p in zip(((0, 20), (20, 37)), parts):
        rs = hc.ce_weighted64(l[a:b], y[a:b], w, 2.0, wsum=r["wsum"])
        close(p["out"][0], rs["loss"], f"share of rows {a}..{b}", **hc.LOSS_VAL)


def test_loss_refusals():
    lw, ls = hc.consistency_case(5, 23)
    y, w = hc.targets_case(5, 23, 1)
    one = torch.zeros(1, device=DEV)
    for ov in (dict(C=65), dict(n=0), dict(C=0), dict(ldw=22), dict(lds=22), dict(lddls=22)):
        run_consistency(lw, ls, 0.7, 0.2, ov=ov, rc=BAD_SHAPE)
    for ov in (dict(lw=None), dict(ls=None)):
        run_consistency(lw, ls, 0.7, 0.2, ov=ov, rc=BAD_ARG)
    run_consistency(lw, ls, 0.7, 0.2, null=("dls",), rc=BAD_ARG)
    run_consistency(lw, ls, 0.7, 0.2, null=("out",), rc=BAD_ARG)
    for ov in (dict(C=65), dict(n=0), dict(ldl=22), dict(lddl=22)):
        run_poly(ls, y, w, 0.2, ov=ov, rc=BAD_SHAPE)
    for ov in (dict(n=0), dict(C=0), dict(ldl=22), dict(lddl=22)):
        run_cew(ls, y, w, 1.0, ov=ov, rc=BAD_SHAPE)
        run_cew(ls, y, w, 1.0, wsum=one, ov=ov, rc=BAD_SHAPE)
    for ov in (dict(l=None), dict(y=None), dict(dl=None), dict(out=None)):
        run_poly(ls, y, w, 0.2, ov=ov, rc=BAD_ARG)
        run_cew(ls, y, w, 1.0, ov=ov, rc=BAD_ARG)
        run_cew(ls, y, w, 1.0, wsum=one, ov=ov, rc=BAD_ARG)
    run_wsum(y, w, 23, rc=BAD_SHAPE, n=0)
    run_wsum(y, w, 0, rc=BAD_SHAPE)


# ====================================================================================== dense
def run_dense(c, act, with_keep, pad=0, accumulate=0, dx_null=False, db_null=False):
    n, K = c["X"].shape
    N = c["W"].shape[0]
    X, W, b, dY = inp(c["X"], pad), inp(c["W"]), inp(c["b"]), inp(c["dY"], pad)
    keep = inp(c["keep"]) if with_keep else None
    Y = Out(n, N, pad)
    assert L().es_dense_fwd(ptr(X), K + pad, ptr(W), ptr(b), Y.p, N + pad, n, K, N, act, hc.DENSE_SLOPE, ptr(keep),
                            hc.DENSE_KEEP_SCALE, S()) == OK
    dX = Out(n, K, pad, init=c["dX0"] if accumulate else None)
    dW, db = Out(N, K), Out(1, N)
    ws = nanbuf(L().es_dense_bwd_workspace(n, N))
    assert ws.numel() >= n * N
    assert L().es_dense_bwd(ptr(dY), N + pad, Y.p if act else None, N + pad, act, hc.DENSE_SLOPE, ptr(keep),
                            hc.DENSE_KEEP_SCALE, ptr(X), K + pad, ptr(W), None if dx_null else dX.p, K + pad, accumulate,
                            dW.p, None if db_null else db.p, n, K, N, ptr(ws), S()) == OK
    torch.cuda.synchronize()
    if dx_null:
        assert dX.untouched()
    if db_null:
        assert db.untouched()
    return {"Y": Y.get(), "dX": None if dx_null else dX.get(), "dW": dW.get(), "db": None if db_null else db.vec()}


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "relu", "leaky"])
@pytest.mark.parametrize("n,K,N", hc.DENSE_SHAPES)
def test_dense_exact_on_integers(n, K, N, act):
    c = hc.dense_case(n, K, N)
    for with_keep in (False, True):
        r = hc.dense64(c, act, with_keep)
        o = all_ways(run_dense, c=c, act=act, with_keep=with_keep)
        for k in ("Y", "dX", "dW", "db"):
            assert torch.equal(o[k].double(), r[k]), (k, with_keep)
        a = all_ways(run_dense, c=c, act=act, with_keep=with_keep, accumulate=1)
        assert torch.equal(a["dX"].double(), r["dX"] + c["dX0"].double()) and same(a["dW"], o["dW"])
        q = run_dense(c, act, with_keep, pad=PAD, dx_null=True)
        assert same(q["dW"], o["dW"]) and same(q["db"], o["db"])  # dX null: dW and db still written
        q = run_dense(c, act, with_keep, db_null=True)
        assert same(q["dW"], o["dW"]) and same(q["dX"], o["dX"])


def test_dense_refusals():
    c = hc.dense_case(4, 8, 6)
    X, W, b, dY = (inp(c[k]) for k in ("X", "W", "b", "dY"))
    ws = nanbuf(4 * 6)

    def fwd(rc, n=4, K=8, N=6, ldx=8, ldy=6, act=1, null=()):
        Y = Out(4, 6)
        a = {"X": ptr(X), "W": ptr(W), "Y": Y.p}
        a.update({k: None for k in null})
        assert L().es_dense_fwd(a["X"], ldx, a["W"], ptr(b), a["Y"], ldy, n, K, N, act, 0.1, None, 1.0, S()) == rc
        torch.cuda.synchronize()
        assert Y.untouched()

    def bwd(rc, n=4, K=8, N=6, lddy=6, ldya=6, ldx=8, lddx=8, act=1, null=()):
        dX, dW, db = Out(4, 8), Out(6, 8), Out(1, 6)
        a = {"dY": ptr(dY), "Y": ptr(dY), "X": ptr(X), "W": ptr(W), "dW": dW.p, "ws": ptr(ws)}
        a.update({k: None for k in null})
        assert L().es_dense_bwd(a["dY"], lddy, a["Y"], ldya, act, 0.1, None, 1.0, a["X"], ldx, a["W"], dX.p, lddx, 0,
                                a["dW"], db.p, n, K, N, a["ws"], S()) == rc
        torch.cuda.synchronize()
        assert dX.untouched() and dW.untouched() and db.untouched() and torch.isnan(ws).all()

    for kw in (dict(K=2049), dict(n=0), dict(N=0), dict(act=3), dict(ldx=7), dict(ldy=5)):
        fwd(BAD_SHAPE, **kw)
    for k in ("X", "W", "Y"):
        fwd(BAD_ARG, null=(k,))
    for kw in (dict(N=2049), dict(n=0), dict(K=0), dict(act=-1), dict(lddy=5), dict(ldya=5), dict(ldx=7), dict(lddx=7)):
        bwd(BAD_SHAPE, **kw)
    for k in ("dY", "Y", "X", "W", "dW", "ws"):
        bwd(BAD_ARG, null=(k,))


# ====================================================================================== BatchNorm1d
def run_bn(c, pad=0, with_nbt=True):
    n, Fe = c["U"].shape
    U, g, b, dY = inp(c["U"], pad), inp(c["gamma"]), inp(c["beta"]), inp(c["dY"], pad)
    rm, rv = Out(1, Fe, init=c["rm"]), Out(1, Fe, init=c["rv"])
    nbt = Out(1, 1, dtype=torch.int64, init=torch.tensor([5]))
    Y, xhat, rstd = Out(n, Fe, pad), Out(n, Fe), Out(1, Fe)
    assert L().es_bn1d_fwd(ptr(U), Fe + pad, ptr(g), ptr(b), rm.p, rv.p, nbt.p if with_nbt else None, hc.BN_MOMENTUM,
                           hc.BN_EPS, 1, Y.p, Fe + pad, xhat.p, rstd.p, n, Fe, S()) == OK
    dU, dg, db = Out(n, Fe, pad), Out(1, Fe), Out(1, Fe)
    assert L().es_bn1d_bwd(ptr(dY), Fe + pad, xhat.p, rstd.p, ptr(g), dU.p, Fe + pad, dg.p, db.p, n, Fe, S()) == OK
    Ye = Out(n, Fe, pad)  # eval mode on the updated running buffers; xhat / rstd null
    assert L().es_bn1d_fwd(ptr(U), Fe + pad, ptr(g), ptr(b), rm.p, rv.p, None, hc.BN_MOMENTUM, hc.BN_EPS, 0, Ye.p,
                           Fe + pad, None, None, n, Fe, S()) == OK
    torch.cuda.synchronize()
    assert int(nbt.vec()[0]) == (6 if with_nbt else 5)
    return {"Y": Y.get(), "xhat": xhat.get(), "rstd": rstd.vec(), "rm": rm.vec(), "rv": rv.vec(), "dU": dU.get(),
            "dgamma": dg.vec(), "dbeta": db.vec(), "Yeval": Ye.get()}


def check_bn(o, r, c, tag):
    for k in ("Y", "xhat", "rstd", "rm", "rv", "dU", "dgamma", "dbeta"):
        close(o[k], r[k], f"{tag} {k}", **hc.CM)


@pytest.mark.parametrize("n,Fe", hc.BN_SHAPES)
def test_bn1d_vs_float64(n, Fe):
    c = hc.bn_case(n, Fe)
    r = hc.bn64(c)
    o = all_ways(run_bn, c=c)
    check_bn(o, r, c, f"bn1d n{n} F{Fe}")
    close(o["Yeval"], hc.bn_eval64(c, r["rm"], r["rv"]), "eval", **hc.CM)
    assert same(run_bn(c, with_nbt=False), o)  # num_batches_tracked null is accepted
    if n == 1:  # var = 0: the running variance takes the biased value
        assert torch.all(o["xhat"] == 0) and torch.all(o["dU"] == 0)
        close(o["rv"], 0.9 * c["rv"].double(), "running variance of one row", **hc.CM)


def run_sync_bn(c, cuts, pad=0):
    """The data-parallel chain on the shards [cuts[i], cuts[i+1]); the fp32 host sum of the shards' sums stands in
    for the all-reduce.  Every shard starts from the same running buffers, as every rank does."""
    n, Fe = c["U"].shape
    N = float(n)
    g, b = inp(c["gamma"]), inp(c["beta"])
    sh = [(a, e) for a, e in zip(cuts[:-1], cuts[1:])]
    U = [inp(c["U"][a:e], pad) for a, e in sh]
    dY = [inp(c["dY"][a:e], pad) for a, e in sh]

    def allreduce(outs):
        s = outs[0].vec().clone()
        for o in outs[1:]:
            s = s + o.vec()
        return s.to(DEV)

    s1 = [Out(1, Fe) for _ in sh]
    for u, (a, e), o in zip(U, sh, s1):
        assert L().es_bn1d_sums(ptr(u), Fe + pad, e - a, Fe, None, N, o.p, S()) == OK
    S1 = allreduce(s1)
    s2 = [Out(1, Fe) for _ in sh]
    for u, (a, e), o in zip(U, sh, s2):
        assert L().es_bn1d_sums(ptr(u), Fe + pad, e - a, Fe, ptr(S1), N, o.p, S()) == OK
    S2 = allreduce(s2)
    res = []
    for u, d, (a, e) in zip(U, dY, sh):
        k = e - a
        rm, rv = Out(1, Fe, init=c["rm"]), Out(1, Fe, init=c["rv"])
        nbt = Out(1, 1, dtype=torch.int64, init=torch.tensor([5]))
        Y, xhat, rstd = Out(k, Fe, pad), Out(k, Fe), Out(1, Fe)
        assert L().es_bn1d_fwd_global(ptr(u), Fe + pad, ptr(g), ptr(b), ptr(S1), ptr(S2), N, rm.p, rv.p, nbt.p,
                                      hc.BN_MOMENTUM, hc.BN_EPS, Y.p, Fe + pad, xhat.p, rstd.p, k, Fe, S()) == OK
        sl = Out(1, 2 * Fe)
        assert L().es_bn1d_bwd_sums(ptr(d), Fe + pad, xhat.p, k, Fe, sl.p, S()) == OK
        res.append(dict(rm=rm, rv=rv, nbt=nbt, Y=Y, xhat=xhat, rstd=rstd, sl=sl, d=d, k=k))
    Sg = allreduce([x["sl"] for x in res])
    for x in res:
        x["dU"], x["dg"], x["db"] = Out(x["k"], Fe, pad), Out(1, Fe), Out(1, Fe)
        assert L().es_bn1d_bwd_global(ptr(x["d"]), Fe + pad, x["xhat"].p, x["rstd"].p, ptr(g), ptr(Sg), x["sl"].p, N,
                                      x["dU"].p, Fe + pad, x["dg"].p, x["db"].p, x["k"], Fe, S()) == OK
    torch.cuda.synchronize()
    out = {k: torch.cat([x[k].get() for x in res]) for k in ("Y", "xhat", "dU")}
    for x in res:
        assert int(x["nbt"].vec()[0]) == 6
        for k in ("rm", "rv", "rstd"):
            assert same(x[k].vec(), res[0][k].vec())  # every rank holds the same statistics
    out.update({k: res[0][k].vec() for k in ("rm", "rv", "rstd")})
    out["dgamma"] = sum(x["dg"].vec().double() for x in res)
    out["dbeta"] = sum(x["db"].vec().double() for x in res)
    return out


def test_sync_bn1d_shards_vs_float64_and_one_process():
    c = hc.bn_case(17, 5)
    r = hc.bn64(c)
    o = all_ways(run_sync_bn, c=c, cuts=(0, 5, 17))
    check_bn(o, r, c, "sync bn1d 5 + 12 rows")  # the running buffers: updated with N = 17
    one = run_bn(c)
    for k in ("Y", "xhat", "rstd", "rm", "rv", "dU"):  # another summation order: the bar, not the bits
        close(o[k], one[k].double(), f"sync vs one process {k}", **hc.CM)
    close(o["dgamma"], one["dgamma"].double(), "sync vs one process dgamma", **hc.CM)
    close(o["dbeta"], one["dbeta"].double(), "sync vs one process dbeta", **hc.CM)


def test_bn1d_refusals():
    c = hc.bn_case(6, 4)
    U, g, b = inp(c["U"]), inp(c["gamma"]), inp(c["beta"])
    rm, rv, Y, xhat, rstd = Out(1, 4), Out(1, 4), Out(6, 4), Out(6, 4), Out(1, 4)
    dU, dg, db, s = Out(6, 4), Out(1, 4), Out(1, 4), Out(1, 8)
    outs = (rm, rv, Y, xhat, rstd, dU, dg, db, s)
    lib = L()

    def fwd(n=6, Fe=4, ldu=4, ldy=4, U_=ptr(U)):
        return lib.es_bn1d_fwd(U_, ldu, ptr(g), ptr(b), rm.p, rv.p, None, 0.1, 1e-5, 1, Y.p, ldy, xhat.p, rstd.p, n, Fe, S())

    def bwd(n=6, Fe=4, lddy=4, lddu=4, dY=ptr(U)):
        return lib.es_bn1d_bwd(dY, lddy, ptr(U), ptr(g), ptr(g), dU.p, lddu, dg.p, db.p, n, Fe, S())

    def sums(n=6, N=6.0, ldu=4, U_=ptr(U)):
        return lib.es_bn1d_sums(U_, ldu, n, 4, None, N, s.p, S())

    def fwdg(n=6, N=6.0, ldu=4, ldy=4, S1=ptr(g)):
        return lib.es_bn1d_fwd_global(ptr(U), ldu, ptr(g), ptr(b), S1, ptr(g), N, rm.p, rv.p, None, 0.1, 1e-5, Y.p, ldy,
                                      xhat.p, rstd.p, n, 4, S())

    def bsums(n=6, lddy=4, dY=ptr(U)):
        return lib.es_bn1d_bwd_sums(dY, lddy, ptr(U), n, 4, s.p, S())

    def bwdg(n=6, N=6.0, lddy=4, lddu=4, Sg=ptr(U)):
        return lib.es_bn1d_bwd_global(ptr(U), lddy, ptr(U), ptr(g), ptr(g), Sg, ptr(U), N, dU.p, lddu, dg.p, db.p, n, 4,
                                      S())

    shape = [fwd(n=0), fwd(Fe=0), fwd(ldu=3), fwd(ldy=3), bwd(n=0), bwd(lddy=3), bwd(lddu=3), sums(n=0), sums(N=5.0),
             sums(ldu=3), fwdg(N=5.0), fwdg(ldu=3), fwdg(ldy=3), fwdg(n=0), bsums(n=0), bsums(lddy=3), bwdg(N=5.0),
             bwdg(lddy=3), bwdg(lddu=3)]
    arg = [fwd(U_=None), bwd(dY=None), sums(U_=None), fwdg(S1=None), bsums(dY=None), bwdg(Sg=None)]
    torch.cuda.synchronize()
    assert shape == [BAD_SHAPE] * len(shape), shape
    assert arg == [BAD_ARG] * len(arg), arg
    assert all(o.untouched() for o in outs)


# ====================================================================================== l2norm
def run_l2(V, dZ=None, pad=0):
    n, Lw = V.shape
    Z, nrm = Out(n, Lw, pad), Out(1, n)
    assert L().es_l2norm_fwd(ptr(inp(V, pad)), Lw + pad, Z.p, Lw + pad, nrm.p, n, Lw, S()) == OK
    o = {}
    if dZ is not None:
        dV = Out(n, Lw, pad)
        assert L().es_l2norm_bwd(ptr(inp(dZ, pad)), Lw + pad, Z.p, Lw + pad, nrm.p, dV.p, Lw + pad, n, Lw, S()) == OK
        o["dV"] = dV
    torch.cuda.synchronize()
    return dict({"Z": Z.get(), "norm": nrm.vec()}, **{k: v.get() for k, v in o.items()})


@pytest.mark.parametrize("n,Lw", hc.L2_SHAPES)
def test_l2norm_exact_and_vs_float64(n, Lw):
    V = hc.l2_exact_case(n, Lw)
    r = hc.l2norm64(V)
    o = all_ways(run_l2, V=V)
    assert torch.equal(o["Z"].double(), r["Z"]) and torch.equal(o["norm"].double(), r["norm"])
    V, dZ = hc.l2_case(n, Lw)
    r = hc.l2norm64(V, dZ)
    o = all_ways(run_l2, V=V, dZ=dZ)
    for k in ("Z", "norm", "dV"):
        close(o[k], r[k], f"l2norm n{n} L{Lw} {k}", **hc.CM)


def test_l2norm_refusals():
    V = inp(torch.ones(3, 8))
    Z, nrm, dV = Out(3, 8), Out(1, 3), Out(3, 8)
    lib = L()
    f = lambda n=3, Lw=8, ldv=8, ldz=8, V_=ptr(V): lib.es_l2norm_fwd(V_, ldv, Z.p, ldz, nrm.p, n, Lw, S())  # noqa: E731
    b = lambda n=3, Lw=8, a=8, z=8, d=8, V_=ptr(V): lib.es_l2norm_bwd(V_, a, ptr(V), z, ptr(V), dV.p, d, n, Lw, S())  # noqa: E731
    shape = [f(n=0), f(Lw=0), f(ldv=7), f(ldz=7), b(n=0), b(Lw=0), b(a=7), b(z=7), b(d=7)]
    arg = [f(V_=None), b(V_=None)]
    torch.cuda.synchronize()
    assert shape == [BAD_SHAPE] * len(shape) and arg == [BAD_ARG] * len(arg), (shape, arg)
    assert Z.untouched() and nrm.untouched() and dV.untouched()


# ====================================================================================== pseudo-labels
def run_pseudo(c, given, pad=0, ex=True, T=hc.PSEUDO_T, alpha=hc.PSEUDO_ALPHA, thres=hc.PSEUDO_THRES, ov=None, rc=OK):
    nu, C = c["lw"].shape
    Lw, Q = c["zw"].shape[1], c["bf"].shape[0]
    lw, zw, bf, bp = inp(c["lw"], pad), inp(c["zw"], pad), inp(c["bf"]), inp(c["bp"])
    hist = c["hist"].clone().to(DEV)
    o = {"probs": Out(nu, C), "porig": Out(nu, C), "pl": Out(nu, 1, dtype=torch.int32), "mask": Out(nu, 1)}
    nws = L().es_comatch_pseudo_workspace(nu, C, Q)
    assert nws == ((Q + 127) // 128) * nu * (C + 1)
    ws = nanbuf(nws)
    a = dict(nu=nu, C=C, L=Lw, Q=Q, cap=c["cap"], len=c["len"], pos=c["pos"], lw=ptr(lw), ws=ptr(ws))
    a.update(ov or {})
    head = (a["lw"], C + pad, a["nu"], a["C"], ptr(hist), a["cap"], a["len"], a["pos"])
    tail = (ptr(zw), Lw + pad, a["L"], ptr(bf), ptr(bp), a["Q"], T, alpha, thres, o["probs"].p, o["porig"].p, o["pl"].p,
            o["mask"].p, a["ws"], S())
    if ex:
        got = L().es_comatch_pseudo_ex(*head, 1 if given else 0, *tail)
    else:
        assert not given
        got = L().es_comatch_pseudo(*head, *tail)
    torch.cuda.synchronize()
    assert got == rc, (got, rc)
    if rc != OK:
        assert all(v.untouched() for v in o.values()) and same(hist.cpu(), c["hist"]) and torch.isnan(ws).all()
        return None
    res = {k: v.get() for k, v in o.items()}
    res["hist"] = hist.cpu()
    return res


def check_pseudo(o, r, c, given, tag):
    h = o["hist"]
    keep = [i for i in range(c["cap"]) if given or i != c["pos"]]
    assert same(h[keep], c["hist"][keep])  # the other ring slots (the poisoned ones too) are as they were
    close(h[c["pos"]], r["entry"], tag + " history entry", **hc.CM)
    close(o["porig"], r["porig"], tag + " probs_orig", **hc.CM)
    close(o["probs"], r["probs"], tag + " probs", **hc.CM)
    assert torch.equal(o["pl"].view(-1).long()[r["label_ok"]], r["label"][r["label_ok"]])
    assert torch.equal(o["mask"].view(-1).double()[r["mask_ok"]], r["mask"][r["mask_ok"]])
    assert torch.all((o["mask"] == 0) | (o["mask"] == 1))


@pytest.mark.parametrize("d", hc.PSEUDO_CASES, ids=hc.case_id)
def test_pseudo_sizes_vs_float64(d):
    c = hc.pseudo_case(**d)
    r = hc.pseudo64(c, given=False)
    o = all_ways(run_pseudo, c=c, given=False)
    check_pseudo(o, r, c, False, "pseudo " + hc.case_id(d))
    assert same(run_pseudo(c, False, pad=PAD, ex=False), o)  # es_comatch_pseudo: the same launch chain


@pytest.mark.parametrize("given", [False, True], ids=["local", "given"])
@pytest.mark.parametrize("cap,hlen,pos", hc.PSEUDO_RINGS)
def test_pseudo_history_ring(cap, hlen, pos, given):
    c = hc.pseudo_case(**hc.PSEUDO_BASE, cap=cap, hlen=hlen, pos=pos)
    r = hc.pseudo64(c, given=given)
    o = all_ways(run_pseudo, c=c, given=given)
    check_pseudo(o, r, c, given, f"ring cap{cap} len{hlen} pos{pos}")


def test_pseudo_deterministic_ties():
    c, want = hc.pseudo_ties_case()
    o = all_ways(run_pseudo, c=c, given=True, alpha=1.0)
    assert torch.equal(o["pl"].view(-1).long(), want)
    close(o["probs"], torch.softmax(c["lw"].double(), 1), "ties probs", **hc.CM)


def test_pseudo_refusals():
    c = hc.pseudo_case(5, 23, 8, 20)
    for ov in (dict(C=33), dict(L=65), dict(nu=0), dict(Q=0), dict(len=5), dict(len=0), dict(pos=4), dict(pos=-1),
               dict(cap=0)):
        run_pseudo(c, False, ov=ov, rc=BAD_SHAPE)
    for ov in (dict(lw=None), dict(ws=None)):
        run_pseudo(c, False, ov=ov, rc=BAD_ARG)


def run_colmean(lw, pad=0, ov=None, rc=OK):
    n, C = lw.shape
    out = Out(1, C)
    a = dict(n=n, C=C, l=ptr(inp(lw, pad)), out=out.p)
    a.update(ov or {})
    got = L().es_softmax_colmean(a["l"], C + pad, a["n"], a["C"], a["out"], S())
    torch.cuda.synchronize()
    assert got == rc
    if rc != OK:
        assert out.untouched()
        return None
    return {"mean": out.vec()}


@pytest.mark.parametrize("n,C", hc.COLMEAN_SHAPES)
def test_softmax_colmean_vs_float64_and_repeatable(n, C):
    lw = hc.logits(n, C, 31 * n + C)
    o = all_ways(run_colmean, lw=lw)
    for _ in range(3):  # a fixed-order reduction: the same bits on every launch
        assert same(run_colmean(lw), o)
    close(o["mean"], hc.colmean64(lw), f"colmean n{n} C{C}", **hc.CM)


def test_softmax_colmean_matches_the_pseudo_kernels_own_mean():
    c = hc.pseudo_case(65, 23, 40, 300)
    o = run_pseudo(c, False)
    m = run_colmean(c["lw"])["mean"]
    close(m, o["hist"][c["pos"]].double(), "colmean vs the DA kernel's entry", rtol=1e-5, atol=1e-7)
    for ov in (dict(C=33), dict(n=0), dict(C=0)):
        run_colmean(c["lw"], ov=ov, rc=BAD_SHAPE)
    for ov in (dict(l=None), dict(out=None)):
        run_colmean(c["lw"], ov=ov, rc=BAD_ARG)


# ====================================================================================== bank write
def run_bank(zw, zx, po, y, C, Q, at, pad=0, rc=OK, nu=None, bt=None):
    Lw = zw.shape[1]
    nu = zw.shape[0] if nu is None else nu
    bt = zx.shape[0] if bt is None else bt
    g = hc.gen(1)
    bf0, bp0 = torch.randn(Q, Lw, generator=g), torch.randn(Q, C, generator=g)
    bf, bp = Out(Q, Lw, init=bf0), Out(Q, C, init=bp0)
    got = L().es_comatch_bank_write(ptr(inp(zw, pad)), Lw + pad, nu, ptr(inp(zx, pad)), Lw + pad, bt, Lw, ptr(inp(po)),
                                    ptr(inp(y)), C, bf.p, bp.p, at, Q, S())
    torch.cuda.synchronize()
    assert got == rc, (got, rc)
    return {"bf": bf.get(), "bp": bp.get()}, bf0, bp0


@pytest.mark.parametrize("nu,bt,Lw", [(14, 3, 16), (0, 3, 16), (14, 0, 16), (5, 4, 65), (0, 0, 8)])
def test_bank_write_exact(nu, bt, Lw):
    C, Q, at = 23, 48, 16
    g = hc.gen(nu + bt + Lw)
    zw, zx = torch.randn(max(nu, 1), Lw, generator=g), torch.randn(max(bt, 1), Lw, generator=g)
    po = torch.rand(max(nu, 1), C, generator=g)
    y = torch.tensor([3, -1, C, C - 1], dtype=torch.int64)[:max(bt, 1)]  # -1 and C: all-zero probability rows
    for pad in (0, PAD):
        o, bf0, bp0 = run_bank(zw, zx, po, y, C, Q, at, pad=pad, nu=nu, bt=bt)
        wf, wp = bf0.clone(), bp0.clone()
        wf[at:at + nu], wp[at:at + nu] = zw[:nu], po[:nu]
        wf[at + nu:at + nu + bt] = zx[:bt]
        onehot = torch.zeros(bt, C)
        for i in range(bt):
            if 0 <= int(y[i]) < C:
                onehot[i, int(y[i])] = 1.0
        wp[at + nu:at + nu + bt] = onehot
        assert torch.equal(o["bf"], wf) and torch.equal(o["bp"], wp)  # rows outside the range untouched
    if bt >= 3:
        assert torch.all(o["bp"][at + nu + 1] == 0) and torch.all(o["bp"][at + nu + 2] == 0)


def test_bank_write_bounds():
    C, Q = 23, 48
    zw, zx, po = torch.ones(14, 16), torch.ones(2, 16), torch.ones(14, C)
    y = torch.tensor([1, 2], dtype=torch.int64)
    o, bf0, bp0 = run_bank(zw, zx, po, y, C, Q, Q - 16)  # ptr + nu + bt == Q is accepted
    assert torch.all(o["bf"][Q - 16:] == 1) and torch.equal(o["bf"][:Q - 16], bf0[:Q - 16])
    for kw in (dict(at=Q - 15), dict(at=-1), dict(at=0, nu=-1), dict(at=0, bt=-1)):
        o, bf0, bp0 = run_bank(zw, zx, po, y, C, Q, rc=BAD_SHAPE, **kw)  # one more row is refused
        assert torch.equal(o["bf"], bf0) and torch.equal(o["bp"], bp0)


# ====================================================================================== contrastive
def run_contrast(z0, z1, pr, pc, off, th, gs, div, pad=0, ex=True, ov=None, rc=OK):
    nr, Lw = z0.shape
    nc, C = pc.shape
    loss, dz0, dz1 = Out(1, 1), Out(nr, Lw, pad), Out(nc, Lw, pad)
    if ex:
        nws = L().es_comatch_contrastive_ex_workspace(nr, nc)
    else:
        nws = L().es_comatch_contrastive_workspace(nr)
    assert nws == nr * nc + nr
    ws = nanbuf(nws)
    a = dict(nr=nr, nc=nc, off=off, z0=ptr(inp(z0, pad)), ws=ptr(ws))
    a.update(ov or {})
    if ex:
        got = L().es_comatch_contrastive_fwd_bwd_ex(a["z0"], Lw + pad, ptr(inp(z1, pad)), Lw + pad, ptr(inp(pr)),
                                                    ptr(inp(pc)), a["nr"], a["nc"], a["off"], Lw, C, hc.CONTRAST_T, th, gs,
                                                    div, loss.p, dz0.p, Lw + pad, dz1.p, Lw + pad, a["ws"], S())
    else:
        assert nr == nc and off == 0 and div == nr
        got = L().es_comatch_contrastive_fwd_bwd(a["z0"], Lw + pad, ptr(inp(z1, pad)), Lw + pad, ptr(inp(pc)), a["nr"],
                                                 Lw, C, hc.CONTRAST_T, th, gs, loss.p, dz0.p, Lw + pad, dz1.p, Lw + pad,
                                                 a["ws"], S())
    torch.cuda.synchronize()
    assert got == rc, (got, rc)
    if rc != OK:
        assert loss.untouched() and dz0.untouched() and dz1.untouched() and torch.isnan(ws).all()
        return None
    return {"loss": loss.vec(), "dz0": dz0.get(), "dz1": dz1.get()}


def check_contrast(o, r, tag):
    close(o["loss"][0], r["loss"], tag + " loss", **hc.CM)
    close(o["dz0"], r["dz0"], tag + " dz0", **hc.CM)
    close(o["dz1"], r["dz1"], tag + " dz1", **hc.CM)


@pytest.mark.parametrize("d", hc.CONTRAST_SIZES, ids=hc.case_id)
def test_contrastive_sizes_vs_float64(d):
    nu = d["nu"]
    z0, z1, probs = hc.contrast_case(**d)
    th, _ = hc.contrast_th(probs)
    for t in (th, 0.0):
        r = hc.contrastive64(z0, z1, probs, probs, 0, t, 2.0 / nu, nu)
        o = all_ways(run_contrast, z0=z0, z1=z1, pr=probs, pc=probs, off=0, th=t, gs=2.0 / nu, div=float(nu), ex=False)
        check_contrast(o, r, f"contrastive {hc.case_id(d)} th {t:.4f}")


def test_contrastive_lone_and_crowded_rows():
    z0, z1, probs = hc.contrast_case(37, 64, 23)
    th, _ = hc.contrast_th(probs, 0.3, 0.7, want=lambda kept: bool((kept == 1).any() and (kept >= 3).any()))
    r = hc.contrastive64(z0, z1, probs, probs, 0, th, 2.0 / 37, 37)
    assert (r["kept"] == 1).any() and (r["kept"] >= 3).any()
    o = all_ways(run_contrast, z0=z0, z1=z1, pr=probs, pc=probs, off=0, th=th, gs=2.0 / 37, div=37.0, ex=False)
    check_contrast(o, r, f"contrastive th {th:.4f} (rows keeping 1 and >= 3 columns)")


def test_contrastive_ex_shards():
    """Rows 0-19 and 20-36 of 37 against all 37 columns: each anchor row's arithmetic is the single launch's, so
    dz0 has its bits; the dz1 shares and the losses (loss_div = 37) add up to it at the bar."""
    z0, z1, probs = hc.contrast_case(37, 64, 23)
    th, _ = hc.contrast_th(probs)
    gs = 2.0 / 37
    full = all_ways(run_contrast, z0=z0, z1=z1, pr=probs, pc=probs, off=0, th=th, gs=gs, div=37.0, ex=False)
    assert same(run_contrast(z0, z1, probs, probs, 0, th, gs, 37.0, ex=True), full)
    parts = [all_ways(run_contrast, z0=z0[a:a + k], z1=z1, pr=probs[a:a + k], pc=probs, off=a, th=th, gs=gs, div=37.0)
             for a, k in ((0, 20), (20, 17))]
    assert torch.equal(torch.cat([p["dz0"] for p in parts]), full["dz0"])
    close(parts[0]["dz1"].double() + parts[1]["dz1"].double(), full["dz1"].double(), "dz1 shares", **hc.CM)
    close(parts[0]["loss"].double() + parts[1]["loss"].double(), full["loss"].double(), "loss shares", **hc.CM)
    for (a, k), p in zip(((0, 20), (20, 17)), parts):
        check_contrast(p, hc.contrastive64(z0[a:a + k], z1, probs[a:a + k], probs, a, th, gs, 37), f"shard at {a}")


def test_contrastive_refusals():
    z0, z1, probs = hc.contrast_case(6, 8, 5)
    for ov in (dict(nc=8193, nr=6), dict(off=1), dict(nr=7), dict(nr=0), dict(off=-1)):
        run_contrast(z0, z1, probs, probs, 0, 0.8, 1.0, 6.0, ov=ov, rc=BAD_SHAPE)
    for ov in (dict(z0=None), dict(ws=None)):
        run_contrast(z0, z1, probs, probs, 0, 0.8, 1.0, 6.0, ov=ov, rc=BAD_ARG)
        run_contrast(z0, z1, probs, probs, 0, 0.8, 1.0, 6.0, ex=False, ov=ov, rc=BAD_ARG)


# ====================================================================================== focal
def run_focal(ls, probs, mask, gamma, gs, pad=0, ov=None, rc=OK):
    nu, C = ls.shape
    loss, dls = Out(1, 1), Out(nu, C, pad)
    ws = nanbuf(nu)
    a = dict(nu=nu, C=C, ldl=C + pad, lddl=C + pad, ls=ptr(inp(ls, pad)), ws=ptr(ws))
    a.update(ov or {})
    got = L().es_comatch_focal_fwd_bwd(a["ls"], a["ldl"], ptr(inp(probs)), ptr(inp(mask)), a["nu"], a["C"], gamma, gs,
                                       loss.p, dls.p, a["lddl"], a["ws"], S())
    torch.cuda.synchronize()
    assert got == rc, (got, rc)
    if rc != OK:
        assert loss.untouched() and dls.untouched() and torch.isnan(ws).all()
        return None
    return {"loss": loss.vec(), "dls": dls.get()}


@pytest.mark.parametrize("gamma", hc.FOCAL_GAMMA)
@pytest.mark.parametrize("nu", hc.FOCAL_NU)
def test_focal_vs_float64(nu, gamma):
    ls, probs, mask = hc.focal_case(nu, 23)
    gs = 2.0 / nu
    r = hc.focal64(ls, probs, mask, gamma, gs)
    o = all_ways(run_focal, ls=ls, probs=probs, mask=mask, gamma=gamma, gs=gs)
    close(o["loss"][0], r["loss"], f"focal nu{nu} gamma{gamma} loss", **hc.CM)
    close(o["dls"], r["dls"], f"focal nu{nu} gamma{gamma} dls", **hc.CM)
    assert torch.all(o["dls"][mask == 0] == 0)  # masked rows: zero in every entry
    if nu == 257:  # every row masked: loss 0; one class: loss 0
        o = run_focal(ls, probs, torch.zeros(nu), gamma, gs)
        assert o["loss"][0].item() == 0.0 and torch.all(o["dls"] == 0)
        ls1, p1, m1 = hc.focal_case(nu, 1)
        o = all_ways(run_focal, ls=ls1, probs=p1, mask=m1, gamma=gamma, gs=gs)
        assert o["loss"][0].item() == 0.0 and torch.isfinite(o["dls"]).all()


def test_focal_refusals():
    ls, probs, mask = hc.focal_case(5, 23)
    for ov in (dict(nu=0), dict(C=0), dict(ldl=22), dict(lddl=22)):
        run_focal(ls, probs, mask, 2.0, 1.0, ov=ov, rc=BAD_SHAPE)
    for ov in (dict(ls=None), dict(ws=None)):
        run_focal(ls, probs, mask, 2.0, 1.0, ov=ov, rc=BAD_ARG)


# ====================================================================================== dropout keep mask
def run_keep(n, p, seed, offset=0, rc=OK, n_arg=None):
    out = Out(1, max(n, 1), dtype=torch.uint8)
    got = L().es_dropout_keep(out.p, n if n_arg is None else n_arg, p, seed, offset, S())
    torch.cuda.synchronize()
    assert got == rc, (got, rc)
    return out


@pytest.mark.parametrize("p", hc.DROPOUT_P)
@pytest.mark.parametrize("n", hc.DROPOUT_N)
def test_dropout_keep_byte_exact(n, p):
    seed = 2 ** 63 + 11  # the top bit set: 64-bit arithmetic all the way
    a = run_keep(n, p, seed).vec()
    assert same(a, run_keep(n, p, seed).vec())
    assert np.array_equal(a.numpy(), hc.dropout_keep_np(n, p, seed))
    if p == 0.0:
        assert torch.all(a == 1)
    for k in (1, 256):  # counter property: mask(seed, offset = k)[i] == mask(seed, 0)[i + k]
        base = hc.dropout_keep_np(n + k, p, seed)
        assert np.array_equal(run_keep(n, p, seed, offset=k).vec().numpy(), base[k:])


def test_dropout_keep_refusals():
    assert run_keep(4, 1.0, 7, rc=BAD_SHAPE).untouched()
    assert run_keep(4, -0.1, 7, rc=BAD_SHAPE).untouched()
    assert run_keep(4, NAN, 7, rc=BAD_SHAPE).untouched()
    assert run_keep(4, 0.2, 7, rc=BAD_SHAPE, n_arg=-1).untouched()
    assert run_keep(4, 0.2, 7, rc=OK, n_arg=0).untouched()  # n = 0 is accepted and writes nothing
    assert L().es_dropout_keep(None, 4, 0.2, 7, 0, S()) == BAD_ARG
