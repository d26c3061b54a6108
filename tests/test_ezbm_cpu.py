"""EZBM, host side: the ctypes table, the float64 restatement of stage 2 (tests/ezbm_restatement.py) pinned to
the reference-generated fixtures tests/golden/ezbm_stage2_{balance,reverse}.npz at rtol 1e-12 -- the GPU tests
then hold the kernels to that restatement where the reference itself is absent --, the lam / CDF / class-table
builders against the reference's formulas on hand cases, and get_config's refusals.

The reference's own fp32-versus-float64 spread on the fixtures is MEASURED here (printed; DESIGN.md "EZBM"), in
units of the project's fp32 bars (loss rtol 1e-5; the rest rtol 1e-4 / atol 1e-6).
"""
import os
import re

import numpy as np
import pytest
import torch

import ezbm_restatement as er
from conftest import ROOT

EXPANSIONS = ("balance", "reverse")
CLS_NUM = [400, 120, 60, 30, 12, 5]


# ------------------------------------------------------------------------------------------ the ABI table
def test_ctypes_table_has_the_entry_points():
    from endossl import _lib
    txt = open(os.path.join(ROOT, "include", "endossl.h")).read().replace("\n", " ")
    want = {"es_ezbm_sample_mix": 23, "es_bn1d_groups_fwd": 17, "es_bn1d_groups_bwd": 13, "es_ezbm_ce_fwd_bwd": 12}
    for name, count in want.items():
        assert name in _lib.SIGNATURES, name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/endossl.h"
        params = [p for p in m.group(1).split(",") if p.strip()]
        assert len(params) == len(_lib.SIGNATURES[name][1]) == count, name
    lib = _lib.load()
    for name in want:
        assert hasattr(lib, name), name


# ------------------------------------------------------------------ the restatement against the reference
def _init(fx):
    return ({k: fx[f"init/{k}"] for k in er.FC_KEYS}, {k: fx[f"init/{k}"] for k in er.BN_KEYS})


def bar_units(d, ref, rtol=1e-4, atol=1e-6):
    """max |d - ref| / (atol + rtol |ref|): <= 1 is what assert_close(rtol, atol) accepts."""
    d, ref = torch.as_tensor(d).double(), torch.as_tensor(ref).double()
    return ((d - ref).abs() / (atol + rtol * ref.abs())).max().item()


def test_fixtures_cover_the_cases():
    for exp in EXPANSIONS:
        fx = er.load_fixture(exp)
        assert fx["expansion"] == exp and fx["n"] == 12 and fx["steps"] == 2 and fx["lambda_c"] == 4
        assert tuple(fx["mem"].shape) == (40, 32) and fx["mem_y"].dtype == torch.int64
        assert fx["cls_num_list"].tolist() == CLS_NUM
        assert tuple(fx["init/0.weight"].shape) == (8, 32) and tuple(fx["init/4.weight"].shape) == (6, 8)
        assert int(torch.bincount(fx["mem_y"], minlength=6).min()) == 1  # a class with one stored row
        for s in range(2):
            t, td = fx["mem_y"][fx[f"s{s}/idx"].long()], fx["mem_y"][fx[f"s{s}/dual"].long()]
            assert (t == td).any() and (t != td).any()
            assert tuple(fx[f"s{s}/keep"].shape) == (24, 8) and set(fx[f"s{s}/keep"].unique().tolist()) == {0, 1}
            assert fx[f"s{s}/lam"].dtype == torch.float32
        if exp == "balance":
            assert all((fx[f"s{s}/lam"] == 0.5).all() for s in range(2))
        else:
            assert fx["s0/lam"].unique().numel() > 3


@pytest.mark.parametrize("exp", EXPANSIONS)
def test_restatement_reproduces_the_reference_float64(exp):
    """lam, the mix, both logits, the losses, the fc gradients, the running buffers, and the parameters and EMA
    after each of the two Adam steps, in float64 against the reference's float64 run."""
    from endossl.ezbm import lam_table
    fx = er.load_fixture(exp)
    params, bufs = _init(fx)
    p = {k: v.double() for k, v in params.items()}
    ema = {k: v.double() for k, v in params.items()}
    b = {k: v.double() for k, v in bufs.items() if k != "3.num_batches_tracked"}
    eb = {k: v.clone() for k, v in b.items()}
    tab = torch.from_numpy(lam_table(fx["cls_num_list"].tolist(), exp)).view(6, 6)
    state, n = {}, fx["n"]
    tol = dict(rtol=1e-12, atol=1e-15)
    for s in range(fx["steps"]):
        idx, dual = fx[f"s{s}/idx"].long(), fx[f"s{s}/dual"].long()
        t, td = fx["mem_y"][idx], fx["mem_y"][dual]
        lam = tab[t, td]
        assert torch.equal(lam, fx[f"s{s}/lam"])  # fp32, exact
        x = er.mix(fx["mem"], idx, dual, lam)
        r = er.head_step(p, b, x, fx[f"s{s}/keep"], t, td, fx["lambda_c"])
        torch.testing.assert_close(r["logits"][:n], fx[f"s{s}/logits_o"], **tol)
        torch.testing.assert_close(r["logits"][n:], fx[f"s{s}/logits_s"], **tol)
        for k in ("l_o", "l_s", "loss"):
            assert abs(r[k].item() - fx[f"s{s}/{k}"]) <= 1e-12 * abs(fx[f"s{s}/{k}"]), (k, r[k].item())
        for k in er.FC_KEYS:
            torch.testing.assert_close(r["grads"][k], fx[f"s{s}/grad/{k}"], msg=lambda m, k=k: f"grad {k}: {m}", **tol)
        er.adam_ema(p, r["grads"], state, ema, lr=fx["lr"], decay=fx["ema_decay"])
        b = {"3.running_mean": r["running_mean"], "3.running_var": r["running_var"]}
        for k in b:  # ModelEMA blends the buffers too
            eb[k] = fx["ema_decay"] * eb[k] + (1 - fx["ema_decay"]) * b[k]
            torch.testing.assert_close(b[k], fx[f"s{s}/param/{k}"], **tol)
            torch.testing.assert_close(eb[k], fx[f"s{s}/ema/{k}"], **tol)
        assert fx[f"s{s}/param/3.num_batches_tracked"] == 2 * (s + 1)  # fc(inputs), fc(mix): two updates a step
        for k in er.FC_KEYS:
            # Adam divides by sqrt(v) + 1e-8: where |g| is tiny the step amplifies the last bits of g
            torch.testing.assert_close(p[k], fx[f"s{s}/param/{k}"], rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(ema[k], fx[f"s{s}/ema/{k}"], rtol=1e-9, atol=1e-12)


def test_reference_fp32_spread_is_measured():
    """The reference's float32 run and the restatement in float32, against the reference's float64 run.  Printed
    per fixture (run with -s); the figures are in DESIGN.md."""
    for exp in EXPANSIONS:
        fx = er.load_fixture(exp)
        params, bufs = _init(fx)
        n = fx["n"]
        idx, dual = fx["s0/idx"].long(), fx["s0/dual"].long()
        t, td = fx["mem_y"][idx], fx["mem_y"][dual]
        x = er.mix(fx["mem"], idx, dual, fx["s0/lam"])
        r32 = er.head_step(params, bufs, x, fx["s0/keep"], t, td, fx["lambda_c"], dtype=torch.float32)
        ref, res = {}, {}
        for s in range(fx["steps"]):
            for k in ("l_o", "l_s", "loss"):
                ref[k] = max(ref.get(k, 0.0), abs(fx[f"s{s}/{k}_f32"] - fx[f"s{s}/{k}"]) / abs(fx[f"s{s}/{k}"]))
            for k in ("logits_o", "logits_s"):
                ref[k] = max(ref.get(k, 0.0), bar_units(fx[f"s{s}/{k}_f32"], fx[f"s{s}/{k}"]))
            for kind in ("grad", "param", "ema"):
                keys = er.FC_KEYS + (er.BN_KEYS[:2] if kind != "grad" else ())
                ref[kind] = max([ref.get(kind, 0.0)] + [bar_units(fx[f"s{s}/{kind}_f32/{k}"], fx[f"s{s}/{kind}/{k}"])
                                                        for k in keys])
        res["loss"] = abs(r32["loss"].item() - fx["s0/loss"]) / abs(fx["s0/loss"])
        res["logits"] = bar_units(r32["logits"], torch.cat([fx["s0/logits_o"], fx["s0/logits_s"]]))
        res["grad"] = max(bar_units(r32["grads"][k], fx[f"s0/grad/{k}"]) for k in er.FC_KEYS)
        print(f"{exp:8s} reference fp32 vs fp64: " + ", ".join(f"{k} {v:.3g}" for k, v in ref.items())
              + " | restatement fp32 (step 0): " + ", ".join(f"{k} {v:.3g}" for k, v in res.items())
              + "   (losses: relative error; the rest: units of the rtol 1e-4 / atol 1e-6 bar)")
        # the comparison is well-posed: the reference's own fp32 forward, loss and gradients sit inside the bars
        assert max(ref["l_o"], ref["l_s"], ref["loss"]) <= 1e-5, ref
        assert max(ref["logits_o"], ref["logits_s"], ref["grad"]) <= 1.0, ref
        assert n == 12


# ------------------------------------------------------------------------------------------ the builders
def test_lam_table_matches_the_reference_formula():
    from endossl.ezbm import lam_table
    cnt = np.array(CLS_NUM)
    for exp in EXPANSIONS:
        tab = lam_table(CLS_NUM, exp).reshape(6, 6)
        assert tab.dtype == np.float32
        for t in range(6):
            for td in range(6):
                lam = torch.tensor(np.array([cnt[t] / (cnt[t] + cnt[td])]), dtype=torch.float)  # code/ezbm.py:156-157
                want = 0.5 * torch.ones_like(lam) if exp == "balance" else 1 - lam
                assert tab[t, td] == want.item(), (exp, t, td)
    rev = lam_table(CLS_NUM, "reverse").reshape(6, 6)
    assert all(rev[c, c] == 0.5 for c in range(6))  # t == td
    assert rev[0, 5] == np.float32(1) - np.float32(400 / 405) and rev[5, 0] == np.float32(1) - np.float32(5 / 405)
    with pytest.raises(ValueError, match="EXPANSION"):
        lam_table(CLS_NUM, "uniform")


def test_class_cdf_matches_the_reference_formula():
    from endossl.ezbm import class_cdf
    bal = class_cdf(CLS_NUM, "balance")
    assert bal.dtype == np.float32 and bal[-1] == 1.0
    np.testing.assert_array_equal(bal, (np.arange(1, 7) / 6).astype(np.float32))
    rev = class_cdf(CLS_NUM, "reverse")
    prob = list(np.array(CLS_NUM) / np.sum(np.array(CLS_NUM)))  # code/dataset.py:148-151
    prob.reverse()
    np.testing.assert_array_equal(rev, np.cumsum(np.array(prob)).astype(np.float32))
    p = np.diff(np.concatenate([[0.0], rev.astype(np.float64)]))
    np.testing.assert_allclose(p, np.array(CLS_NUM[::-1]) / 627.0, atol=1e-7)  # class c: cls_num[C-1-c] / sum
    assert rev[-1] == 1.0 and rev[0] == np.float32(5 / 627)
    with pytest.raises(ValueError, match="EXPANSION"):
        class_cdf(CLS_NUM, None)


def test_class_csr_hand_cases():
    from endossl.ezbm import class_csr
    off, idx = class_csr(np.array([2, 0, 1, 2, 2, 0]), 3)
    assert off.dtype == np.int32 and idx.dtype == np.int32
    assert off.tolist() == [0, 2, 3, 6] and idx.tolist() == [1, 5, 2, 0, 3, 4]  # class 1: one row; ascending rows
    off, idx = class_csr(torch.tensor([1, 0]).numpy(), 2)
    assert off.tolist() == [0, 1, 2] and idx.tolist() == [1, 0]
    with pytest.raises(ValueError, match="class 1 "):
        class_csr(np.array([0, 2, 2, 0]), 3)  # the refused empty class, named
    with pytest.raises(ValueError, match="class 3 "):
        class_csr(np.array([0, 1, 2]), 5)
    with pytest.raises(ValueError):
        class_csr(np.array([0, 1, 3]), 3)


def test_sampler_restatement_hand_cases():
    """The integer draw covers [0, m) and the CDF draw its classes; the numpy form equals the Python-int form."""
    z = er.splitmix_np(7, np.arange(1000, dtype=np.uint64) + np.uint64(5))
    assert [int(v) for v in z[:50]] == [er.splitmix(7, 5 + i) for i in range(50)]
    off, idx = np.array([0, 1, 4, 6]), np.array([3, 0, 2, 5, 1, 4])
    cdf = np.array([0.25, 0.5, 1.0], dtype=np.float32)
    a, b, ca, cb = er.sample(3000, 3, off, idx, cdf, seed=11, offset=1 << 40)
    cls_of = np.array([1, 2, 1, 0, 2, 1])
    assert np.array_equal(cls_of[a], ca) and np.array_equal(cls_of[b], cb)
    assert set(a.tolist()) == set(range(6)) and set(b.tolist()) == set(range(6))
    f = np.bincount(cb, minlength=3) / 3000.0
    assert np.all(np.abs(f - [0.25, 0.25, 0.5]) < 5 * np.sqrt(0.25 / 3000))
    a2, b2, _, _ = er.sample(10, 3, off, idx, cdf, seed=11, offset=(1 << 40) + 4 * 5)
    assert np.array_equal(a2, a[5:15]) and np.array_equal(b2, b[5:15])  # counters, not a stream


# ------------------------------------------------------------------------------------------ get_config
class _DS:
    df = None

    def get_cls_num_list(self):
        return [9, 5, 2]

    def __len__(self):
        return 16


class _DL(list):
    dataset = _DS()


def _train_cfg(expansion="balance", **train):
    from endossl.utils import AttrDict
    t = dict(USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, CLS_WEIGHT=False, EPOCHS=1, WARMUP_EPOCHS=0,
             DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="const", FREQ_EVAL=1, LAMBDA_C=4, THRES=0.5)
    if expansion is not None:
        t["EXPANSION"] = expansion
    t.update(train)
    return AttrDict(DATA=AttrDict(BATCH_SIZE=4, MU=2, IMG_SIZE=64, TARGET_NAME="target"),
                    MODEL=AttrDict(NAME="vit_tiny_test", NUM_CLASSES=3, MARGIN="None", IS_TRIPLET=False),
                    TRAIN=AttrDict(**t))


def _emb_model(C=3):
    from endossl.comatch_model import NativeViTEmb
    from endossl.vit import ViTConfig
    return NativeViTEmb(ViTConfig(img_size=64, dim=128, depth=2, heads=2, num_classes=C, head="emb", low_dim=16), seed=0)


def test_get_config_refusals(monkeypatch):
    from endossl import dist
    from endossl.ezbm import EZBM
    from endossl.vit import NativeViT, ViTConfig
    plain = NativeViT(ViTConfig(img_size=64, dim=128, depth=2, heads=2, num_classes=3), seed=0)
    tr = EZBM(plain, device="cpu")
    tr.get_dataloader(_DL([]), None)
    with pytest.raises(ValueError, match="build_model.*IS_TRIPLET"):  # the wrong model, and how to build the right one
        tr.get_config(_train_cfg())
    tr = EZBM(_emb_model(), device="cpu")
    tr.get_dataloader(_DL([]), None)
    for bad in ("uniform", None, "Balance"):
        with pytest.raises(ValueError, match="EXPANSION"):
            tr.get_config(_train_cfg(bad))
    monkeypatch.setattr(dist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="bank"):
        tr.get_config(_train_cfg())
    monkeypatch.undo()
    tr = _with_dl(EZBM(_emb_model(C=5), device="cpu"))
    with pytest.raises(ValueError, match="classes"):  # get_cls_num_list() of another class count than the model
        tr.get_config(_train_cfg())


def _with_dl(tr):
    tr.get_dataloader(_DL([]), None)
    return tr


def test_get_config_runs_the_triplet_step_whatever_is_triplet_says():
    from endossl.ezbm import EZBM
    from endossl.supervised import SupLearning
    tr = _with_dl(EZBM(_emb_model(), device="cpu"))
    cfg = _train_cfg("reverse")
    tr.get_config(cfg)
    assert isinstance(tr, SupLearning) and tr.is_triplet and not tr.is_margin
    assert tr.config is cfg and cfg.MODEL.IS_TRIPLET is False  # the caller's config is not rewritten
    assert tr.cls_num_list == [9, 5, 2] and tr.stage == 1
    assert (EZBM.STAGE1_EPOCHS, EZBM.STAGE2_EPOCHS) == (100, 100)
    # stage 2 set-up: fc alone trains, head_emb stays frozen, the scheduler gets len(train_dl) // MU
    tr.setup_stage_2()
    names = [n for n, p in tr.model.named_parameters() if p.requires_grad]
    assert names == ["fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias", "fc.4.weight", "fc.4.bias"]
    assert tr.stage == 2 and sum(len(g) for g in tr.optimizer._group_names) == 6
