"""The exact-integer convolution cases of tests/conv_cases.py, checked without a GPU: the float64 torch reference
equals an explicit loop over taps on every case, every intermediate stays an fp32 integer, and the restated dispatch
(`paths`) reaches, over the cases x the knob grid of test_gpu_conv_exact.py, each kernel class the cases are there
for -- asserted one by one, so that removing a case says what it loses."""
import itertools

import pytest
import torch

import conv_cases as cc

ALL = dict(cc.CASES, **cc.FP32_CASES, STEM=cc.STEM_CASE)


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name, case in ALL.items():
        ops = cc.operands(case)
        out[name] = (ops, cc.reference(case, ops))
    return out


@pytest.mark.parametrize("name", list(ALL))
def test_reference_equals_naive_loop(name, refs):
    case = ALL[name]
    ops, ref = refs[name]
    for k, v in ops.items():
        lo, hi = {"mean": (-1, 1), "beta": (-1, 1), "rstd": (1, 2), "gamma": (1, 2)}.get(k, (-2, 2))
        assert v.dtype == torch.int64 and lo <= v.min().item() and v.max().item() <= hi, k
    nv = cc.naive_conv(case, ops)
    assert torch.equal(ref["y"], (nv["y"] + ops["bias"]).double())
    assert torch.equal(ref["y_acc"], (nv["y"] + ops["prior_y"]).double())
    assert torch.equal(ref["dx"], nv["dx"].double()) and torch.equal(ref["dx_acc"], (nv["dx"] + ops["prior_dx"]).double())
    assert torch.equal(ref["dw"], nv["dw"].double()) and torch.equal(ref["dw_acc"], (nv["dw"] + ops["prior_dw"]).double())
    nb = cc.naive_conv(case, ops, x=cc.bn_relu(ops))
    assert torch.equal(ref["y_bn"], nb["y"].double()) and torch.equal(ref["dw_bn"], nb["dw"].double())
    # the partials' sum half is the integer block sum; M2 against the uncentred form sum y^2 - (sum y)^2 / nb
    y = (nv["y"] + ops["bias"]).reshape(-1, case[4])
    for b, part in enumerate(ref["partials"]):
        blk = y[b * cc.NT_BM:(b + 1) * cc.NT_BM]
        assert torch.equal(part[0], blk.sum(0).double())
        m2 = (blk * blk).sum(0).double() - blk.sum(0).double() ** 2 / blk.shape[0]
        assert (part[1] - m2).abs().max().item() <= 1e-9 * max(1.0, m2.max().item())


@pytest.mark.parametrize("name", list(ALL))
def test_magnitudes_stay_exact_in_fp32(name, refs):
    """Bounds on every partial sum, whatever the order: K * 4 per output (K * 26 with the BatchNorm-ed input, whose
    values reach 13), M * 4 per weight gradient (M * 26), the accumulate sums, the block sums of the partials."""
    N, H, W, Cin, Cout, kh, kw, s, p = ALL[name]
    ops, ref = refs[name]
    Ho, Wo = cc.out_hw(ALL[name])
    M = N * Ho * Wo
    assert cc.bn_relu(ops).max().item() <= 13
    for bound in (Cin * kh * kw * 26 + 2, Cout * kh * kw * 4 + 2, M * 26 + 2, cc.NT_BM * (Cin * kh * kw * 4 + 2)):
        assert bound < cc.EXACT
    for k in ("y", "y_acc", "y_bn", "dx", "dx_acc", "dw", "dw_acc", "dw_bn"):
        assert ref[k].abs().max().item() < cc.EXACT and torch.equal(ref[k], ref[k].round()), k
        assert torch.equal(ref[k].float().double(), ref[k]), k
    assert ref["partials"][:, 0].abs().max().item() < cc.EXACT


def test_bf16_outputs_really_round():
    """Case D's sums pass 256, where bf16 has no odd integers: its bf16 output maps test the one rounding."""
    ops = cc.operands(cc.CASES["D"])
    y = cc.reference(cc.CASES["D"], ops)["y"]
    assert y.abs().max().item() > 256 and not torch.equal(y.float().bfloat16().double(), y)


def test_coverage_of_kernel_classes():
    seen = {"fwd": set(), "dx": set(), "dw_tile": set(), "dw_loads": set(), "fwd_bnin": set()}
    nk, zero_tap, small_phase = set(), set(), set()
    for (name, case), (ring, dw_buf, small), flags in itertools.product(cc.CASES.items(), cc.KNOBS, range(4)):
        r = cc.paths(case, flags, ring, dw_buf, small)
        seen["fwd"].add((r["fwd"]["kernel"], r["fwd"]["bn"]))
        seen["fwd_bnin"].add((r["fwd_bnin"]["kernel"], r["fwd_bnin"]["bn"]))
        seen["dx"].add((r["dx"]["kernel"], r["dx"]["bn"]))
        seen["dw_tile"].add(r["dw"]["tile"])
        seen["dw_loads"].add(r["dw"]["loads"])
        for kind in ("fwd", "dx"):
            if r[kind]["kernel"] == "ring":
                nk.add((kind, r[kind]["nk"]))
        for q in r["dx"]["phases"]:
            if q["twy"] * q["twx"] == 0:
                zero_tap.add(name)
            if q["M"] < r["dx"]["M"]:
                small_phase.add(name)
    for kind in ("fwd", "dx"):
        for kernel in ("ring", "staged-bufl", "staged-branchy"):
            for bn in (64, 128):
                assert (kernel, bn) in seen[kind], f"{kind}: no case reaches the {kernel} kernel on the {bn}-column tile"
    assert not any(k == "ring" for k, _ in seen["fwd_bnin"]), "the BatchNorm-in forward has no ring kernel"
    for kernel in ("staged-bufl", "staged-branchy"):
        for bn in (64, 128):
            assert (kernel, bn) in seen["fwd_bnin"], f"BatchNorm-in forward: {kernel} on the {bn}-column tile"
    for tile in ((128, 128), (64, 128), (128, 64), (64, 64)):
        assert tile in seen["dw_tile"], f"no case reaches the {tile[0]} x {tile[1]} weight-gradient tile"
    assert seen["dw_loads"] == {"buf", "branchy"}
    assert zero_tap, "no data-gradient phase without a tap (twy * twx == 0)"
    assert small_phase, "no data-gradient phase smaller than the largest"
    for kind in ("fwd", "dx"):
        for n in (1, 2):
            assert (kind, n) in nk, f"{kind}: no ring launch with nk = {n} (a prologue shorter than the stage count)"
        assert any(n > 4 for k, n in nk if k == kind), f"{kind}: no ring launch deeper than the ring"


def test_coverage_of_shapes():
    geo = {name: (case[0] * cc.out_hw(case)[0] * cc.out_hw(case)[1],) + cc.out_hw(case) for name, case in cc.CASES.items()}
    assert any(M < 128 for M, _, _ in geo.values()), "no case with M < 128"
    assert any(M == 128 for M, _, _ in geo.values()), "no case with M == 128"
    assert any(M > 128 and M % 128 for M, _, _ in geo.values()), "no case with a partial second row block"
    assert any(Wo < 32 and 32 // Wo + 1 < Ho for _, Ho, Wo in geo.values()), "no case on the branch-free pixel walk"
    assert any(Wo < 32 and 32 % Wo and 32 // Wo + 1 < Ho for _, Ho, Wo in geo.values()), "no carry in w in advance32"
    assert any(Wo > 32 for _, _, Wo in geo.values()), "no map wider than 32"
    assert any(Ho * Wo < 32 for _, Ho, Wo in geo.values()), "no map smaller than one 32-pixel step"
    assert any(c[1] != c[2] for c in cc.CASES.values()) and any(c[5] != c[6] for c in cc.CASES.values())
    assert any((c[1] + 2 * c[8] - c[5]) % c[7] for c in cc.CASES.values()), "no input row that no output reads"
    assert set(cc.VIEW_CASES) <= set(cc.CASES)
    # what the comments of CASES promise, by name
    assert geo["A"][0] == 189 and geo["D"][0] == 300 and geo["E"][0] == 128 and geo["I"][0] == 16 and geo["M"][0] == 135
    assert geo["B"][1:] == (6, 4) and geo["G"][1:] == (12, 3) and geo["L"][2] == 40 and geo["H"][1:] == (2, 2)
    assert len(cc.dx_phases(cc.CASES["I"])) == 16 and all(q["twy"] * q["twx"] == 1 and q["nk"] == 2
                                                          for q in cc.dx_phases(cc.CASES["I"]))
    assert len({q["M"] for q in cc.dx_phases(cc.CASES["B"])}) > 1
    assert sum(q["twy"] * q["twx"] == 0 for q in cc.dx_phases(cc.CASES["C"])) == 3


def test_untouched_input_has_zero_gradient(refs):
    """Case K: the last row and column of x are read by no output; case C: the three tap-less stride phases."""
    dx = refs["K"][1]["dx"]
    assert (dx[:, -1] == 0).all() and (dx[:, :, -1] == 0).all() and (dx[:, :-1, :-1] != 0).any()
    dx = refs["C"][1]["dx"]
    assert (dx[:, 1::2] == 0).all() and (dx[:, :, 1::2] == 0).all() and (dx[:, ::2, ::2] != 0).any()


def test_paths_follows_the_knobs():
    """Spot values of the restated dispatch, derived by hand from csrc/conv_bf16.hip."""
    A, C, F_ = cc.CASES["A"], cc.CASES["C"], cc.CASES["F"]
    assert cc.paths(A, 1, 3, 1, 128)["fwd"]["kernel"] == "ring" and cc.paths(A, 0, 3, 1, 128)["fwd"]["kernel"] == "staged-bufl"
    assert cc.paths(A, 1, 0, 0, 128)["fwd"]["kernel"] == "staged-branchy"
    assert cc.paths(F_, 3, 3, 1, 128)["fwd"]["kernel"] == "staged-bufl"  # widening: never the ring
    assert cc.paths(F_, 3, 3, 1, 128)["dx"]["kernel"] == "ring"
    assert cc.paths(A, 3, 4, 1, 0)["fwd_bnin"]["kernel"] == "staged-bufl"
    assert cc.paths(C, 0, 3, 1, 0)["fwd"]["bn"] == 128 and cc.paths(C, 0, 3, 1, 128)["fwd"]["bn"] == 64
    assert cc.paths(C, 0, 3, 1, 0)["dx"]["bn"] == 128 and cc.paths(C, 0, 3, 1, 1 << 20)["dx"]["bn"] == 64
    assert cc.paths(A, 0, 3, 1, 128)["dw"] == {"tile": (64, 128), "M": 189, "K": 576, "loads": "buf"}
    assert cc.paths(A, 0, 3, 0, 128)["dw"]["loads"] == "branchy"
    assert cc.paths(cc.CASES["H"], 0, 3, 1, 128)["dw"]["loads"] == "branchy"  # 32 / Wo + 1 = 17 >= Ho
