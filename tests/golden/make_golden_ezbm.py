"""Generate the EZBM stage-2 fixtures tests/golden/ezbm_stage2_{balance,reverse}.npz by running the REFERENCE.

Test infrastructure only; like make_golden.py it runs where the read-only reference tree is mounted (CPU) and
refuses to run anywhere else.  The reference's own `EZBM.train_one_stage_2` (code/ezbm.py:133-182) and
`EmbFeatEZBM` (code/dataset.py:135-175) are imported (never copied) and driven as they stand, on an object whose
model has `fc = build_head(D, C, is_complex=True)`, Adam(lr 1e-3) and ModelEMA(0.999).  What the run computes is
observed from outside: forward hooks on `fc` (inputs, logits) and on its Dropout (the keep mask), a recording
wrapper around the names the reference module looks up (`ce_loss`, `AverageMeter`) and around `optimizer.step`
(the gradients).  The float64 run feeds `fc` the reference's fp32 batch cast up (a forward pre-hook: the
reference's FloatTensor bank cannot enter a float64 head otherwise) and records the Dropout mask; the float32
run replays that mask and must draw the same rows.

`lam` is a local of the reference; the value stored is the fp32 cnt[t] / (cnt[t] + cnt[td]) rule, accepted only
if it reproduces the reference's own `mix` rows BIT FOR BIT from the recorded rows (asserted below).

Sizes: N = 40 bank rows, D = 32, F = 8, C = 6, cls_num_list 400 / 120 / 60 / 30 / 12 / 5, n = 12
(BATCH_SIZE 4 x MU 3), LAMBDA_C = 4; the epoch has 4 steps (12, 12, 12, 4 rows), the first two are stored.
Committed: DATA only, loadable with allow_pickle=False.

Usage (from the repo root):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ezbm.py
"""
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn as nn

import make_golden

OUT = os.path.dirname(os.path.abspath(__file__))
N, D, F, C = 40, 32, 8, 6
CLS_NUM = [400, 120, 60, 30, 12, 5]
B, MU, LAMBDA_C, LR, EMA_DECAY = 4, 3, 4, 1e-3, 0.999
STEPS = 2
FC_KEYS = ("0.weight", "0.bias", "3.weight", "3.bias", "4.weight", "4.bias")
BN_KEYS = ("3.running_mean", "3.running_var", "3.num_batches_tracked")


def _import_reference():
    if not os.path.isdir(make_golden.REF):
        raise SystemExit("make_golden_ezbm.py needs the reference tree (build container only)")
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    make_golden._install_stubs()
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.datasets = types.ModuleType("torchvision.datasets")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    sys.modules.setdefault("torchvision.datasets", tv.datasets)
    td = types.ModuleType("timm.data")
    td.Mixup = object
    sys.modules["timm.data"] = td
    sys.modules["timm"].data = td
    fp = types.ModuleType("fastprogress")
    fpp = types.ModuleType("fastprogress.fastprogress")
    fpp.master_bar = lambda it: it
    fpp.progress_bar = lambda it, parent=None: it
    fp.fastprogress = fpp
    sys.modules["fastprogress"] = fp
    sys.modules["fastprogress.fastprogress"] = fpp
    sys.path.insert(0, make_golden.REF)
    import ezbm as ref_ezbm
    import dataset as ref_dataset
    import ema as ref_ema
    import optimizer as ref_optimizer
    from models import custom_model as ref_custom
    return ref_ezbm, ref_dataset, ref_ema, ref_optimizer, ref_custom


class _Model(nn.Module):
    def __init__(self, head):
        super().__init__()
        self.fc = head


class _Sched:
    def step_update(self, t):
        pass


def _bank(seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.cat([torch.arange(C), torch.randint(0, C, (N - C - 1,), generator=g), torch.tensor([C - 1])])
    y = y[torch.randperm(N, generator=g)]
    # one class with a single row: move the surplus rows of class 4 to class 0
    for i in torch.nonzero(y == 4)[1:, 0].tolist():
        y[i] = 0
    centers = torch.randn(C, D, generator=g)
    mem = (centers[y] + 0.7 * torch.randn(N, D, generator=g)).float().contiguous()
    assert int(torch.bincount(y, minlength=C).min()) == 1
    return mem, y.to(torch.int64)


def _run(mods, expansion, mem, mem_y, init, dtype, replay_keep):
    ref_ezbm, ref_dataset, ref_ema, ref_optimizer, ref_custom = mods
    random.seed(1234)
    np.random.seed(1234)
    torch.manual_seed(1234)
    model = _Model(ref_custom.build_head(D, C, is_complex=True))
    model.fc.load_state_dict(init)
    model.to(dtype)
    tr = ref_ezbm.EZBM(model, opt_func="Adam", lr=LR, device="cpu")
    T = lambda **kw: types.SimpleNamespace(**kw)  # noqa: E731
    tr.config = T(TRAIN=T(EXPANSION=expansion, LAMBDA_C=LAMBDA_C, USE_EMA=True, EMA_DECAY=EMA_DECAY, BASE_LR=LR),
                  DATA=T(BATCH_SIZE=B, MU=MU))
    tr.ema_model = ref_ema.ModelEMA(model=model, decay=EMA_DECAY, device="cpu")
    tr.optimizer = ref_optimizer.build_optimizer(model, opt_func="Adam", lr=LR)
    tr.lr_scheduler = _Sched()
    tr.mb = None
    tr.cls_num_list = CLS_NUM
    tr.mem_features = [r for r in mem.numpy()]
    tr.mem_targets = [t for t in mem_y.numpy()]

    rec = {"fc_in": [], "fc_out": [], "keep": [], "ce": [], "ce_t": [], "grads": [], "loss": [], "after": [],
           "items": []}
    kstate = {"i": 0}

    model.fc.register_forward_pre_hook(lambda m, a: (a[0].to(dtype),))

    def fc_hook(m, a, out):
        rec["fc_in"].append(a[0].detach().clone())
        rec["fc_out"].append(out.detach().clone())
    model.fc.register_forward_hook(fc_hook)

    def drop_hook(m, a, out):
        if replay_keep is None:
            rec["keep"].append((out != 0).to(torch.uint8))
            return None
        k = replay_keep[kstate["i"]]
        kstate["i"] += 1
        rec["keep"].append(k)
        return a[0] * (k.to(dtype) * (1.0 / (1.0 - m.p)))
    model.fc[2].register_forward_hook(drop_hook)

    orig_ce, orig_meter, orig_get = ref_ezbm.ce_loss, ref_ezbm.AverageMeter, ref_dataset.EmbFeatEZBM.__getitem__

    def ce_rec(logits, targets, *a, **kw):
        v = orig_ce(logits, targets, *a, **kw)
        rec["ce"].append(v.detach().clone())
        rec["ce_t"].append(targets.detach().clone())
        return v

    class Meter(orig_meter):
        def update(self, val, n=1):
            rec["loss"].append(val)
            rec["after"].append({"p": {k: v.detach().clone() for k, v in model.fc.state_dict().items()},
                                 "e": {k: v.detach().clone() for k, v in tr.ema_model.ema.fc.state_dict().items()}})
            super().update(val, n)

    def get_rec(self, item):
        out = orig_get(self, item)
        rows = [int(torch.nonzero((mem == out[j]).all(1))[0, 0]) for j in (0, 2)]
        assert int(mem_y[rows[0]]) == int(out[1]) and int(mem_y[rows[1]]) == int(out[3])
        rec["items"].append(rows)
        return out

    opt_step = tr.optimizer.step

    def step_rec(*a, **kw):
        rec["grads"].append({k: p.grad.detach().clone() for k, p in model.fc.named_parameters()})
        return opt_step(*a, **kw)

    ref_ezbm.ce_loss, ref_ezbm.AverageMeter, ref_dataset.EmbFeatEZBM.__getitem__ = ce_rec, Meter, get_rec
    tr.optimizer.step = step_rec
    try:
        tr.train_one_stage_2(0)
    finally:
        ref_ezbm.ce_loss, ref_ezbm.AverageMeter, ref_dataset.EmbFeatEZBM.__getitem__ = orig_ce, orig_meter, orig_get
    return rec


def _lam_rule(t, td, expansion):
    cnt = np.array(CLS_NUM)
    lam = (cnt[t] / (cnt[t] + cnt[td])).astype(np.float32)
    if expansion == "balance":
        return np.full_like(lam, 0.5)
    return np.float32(1.0) - lam


def main():
    mods = _import_reference()
    for ei, expansion in enumerate(("balance", "reverse")):
        mem, mem_y = _bank(70 + ei)
        torch.manual_seed(500 + ei)
        head = mods[4].build_head(D, C, is_complex=True)
        with torch.no_grad():
            head[3].weight.uniform_(0.5, 1.5)
            head[3].bias.normal_(0.0, 0.1)
        init = {k: v.detach().clone() for k, v in head.state_dict().items()}
        r64 = _run(mods, expansion, mem, mem_y, init, torch.float64, None)
        r32 = _run(mods, expansion, mem, mem_y, init, torch.float32, r64["keep"])
        assert r64["items"] == r32["items"], "the two runs drew different rows"
        n = B * MU
        assert len(r64["loss"]) == 4 and [x.shape[0] for x in r64["fc_in"]] == [n, n, n, n, n, n, 4, 4]
        out = {"expansion": np.array(expansion), "mem": mem.numpy(), "mem_y": mem_y.numpy(),
               "cls_num_list": np.array(CLS_NUM, dtype=np.int64), "lambda_c": np.float64(LAMBDA_C),
               "lr": np.float64(LR), "ema_decay": np.float64(EMA_DECAY), "n": np.int64(n), "steps": np.int64(STEPS)}
        for k, v in init.items():
            out[f"init/{k}"] = v.numpy()
        for s in range(STEPS):
            items = np.array(r64["items"][s * n:(s + 1) * n], dtype=np.int32)
            idx, dual = items[:, 0], items[:, 1]
            t, td = mem_y.numpy()[idx], mem_y.numpy()[dual]
            assert np.array_equal(r64["ce_t"][3 * s].numpy(), t) and np.array_equal(r64["ce_t"][3 * s + 2].numpy(), td)
            lam = _lam_rule(t, td, expansion)
            lt = torch.from_numpy(lam)[:, None]
            mix = lt * mem[idx] + (1 - lt) * mem[dual]
            for r in (r64, r32):  # the reference's own batch: the rows drawn, and its mix bit for bit
                assert torch.equal(r["fc_in"][2 * s].float(), mem[idx])
                assert torch.equal(r["fc_in"][2 * s + 1].float().view(torch.int32), mix.view(torch.int32))
            out[f"s{s}/idx"], out[f"s{s}/dual"], out[f"s{s}/lam"] = idx, dual, lam
            out[f"s{s}/keep"] = torch.cat([r64["keep"][2 * s], r64["keep"][2 * s + 1]]).numpy()
            for tag, r in (("", r64), ("_f32", r32)):
                ce = r["ce"][3 * s:3 * s + 3]
                out[f"s{s}/logits_o{tag}"] = r["fc_out"][2 * s].numpy()
                out[f"s{s}/logits_s{tag}"] = r["fc_out"][2 * s + 1].numpy()
                out[f"s{s}/l_o{tag}"] = ce[0].numpy()
                out[f"s{s}/l_s{tag}"] = (0.5 * ce[1] + 0.5 * ce[2]).numpy()
                out[f"s{s}/loss{tag}"] = np.array(r["loss"][s], dtype=np.float64)
                for k in FC_KEYS:
                    out[f"s{s}/grad{tag}/{k}"] = r["grads"][s][k].numpy()
                    out[f"s{s}/param{tag}/{k}"] = r["after"][s]["p"][k].numpy()
                    out[f"s{s}/ema{tag}/{k}"] = r["after"][s]["e"][k].numpy()
                for k in BN_KEYS:
                    out[f"s{s}/param{tag}/{k}"] = r["after"][s]["p"][k].numpy()
                    out[f"s{s}/ema{tag}/{k}"] = r["after"][s]["e"][k].numpy()
            same = int((t == td).sum())
            print(f"ezbm_stage2_{expansion} step {s}: loss {r64['loss'][s]:.6f} (f32 {r32['loss'][s]:.6f}) "
                  f"t == td in {same} of {n} rows, lam {lam.min():.4f} .. {lam.max():.4f}")
        np.savez_compressed(os.path.join(OUT, f"ezbm_stage2_{expansion}.npz"), **out)


if __name__ == "__main__":
    main()
