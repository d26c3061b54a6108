"""The squeeze-excite block tail (csrc/se.hip) against the plain BatchNorm + residual + ReLU tail it replaces, in
isolation, at the four stage shapes of ResNet-50 at 224^2 (N = 64 images, bf16 maps), and one whole supervised step
of `resnet50se` beside `resnet50`.
  python scripts/se_tail_bench.py [--n 64] [--iters 9] [--reps 20] [--steps 12] [--md table.md]
Forward: es_bn2d_fwd_partials_ex (statistics only) + es_se_squeeze_ex + es_se_gate_fwd + es_se_bn_apply_ex against
es_bn2d_fwd_partials_ex(res, relu) on the same buffers.  Backward: es_se_bn_bwd_sums_ex + es_se_gate_bwd +
es_se_bn_bwd_dx_ex against es_bn2d_bwd_ex(relu, gout).  Interleaved, `iters` windows of `reps` back-to-back launch
chains between two device events each; the median window / reps in us and the spread (max - min) / median of the
windows.  (The statistics launch folds its partials in place, so the repeats time the launches, not the values.)
Expected from the byte counts alone: the apply and the two backward passes move what the plain passes move; the
forward adds one read of conv3's map.  No bar is set: these are first measurements, the parent figures for moving the
squeeze into conv3's epilogue.
The step: SupLearning.step at B = `n`, 224^2, 23 classes, Adam + EMA, in one process -- resnet50se (eager: it has no
graph replay), resnet50 eager, resnet50 with its default graph replay; median and spread over `steps` steps."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endoscopy-image-classification_amd"))
import torch  # noqa: E402

from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402

SHAPES = [("layer1", 56, 256), ("layer2", 28, 512), ("layer3", 14, 1024), ("layer4", 7, 2048)]


def _windows(fns, iters, reps):
    """{name: [ms per window]}: the chains interleaved window by window."""
    out = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def _stat(ws, reps):
    ws = sorted(ws)
    med = ws[len(ws) // 2]
    return med / reps * 1e3, (ws[-1] - ws[0]) / med


def tails(a, lib, s):
    dev, N = "cuda", a.n
    rows = []
    for name, H, C in SHAPES:
        HW, M, R = H * H, N * H * H, C // 16
        bf = torch.bfloat16
        y = torch.randn(N, HW, C, device=dev).to(bf)
        res = torch.randn(N, HW, C, device=dev).to(bf)
        dout = torch.randn(N, HW, C, device=dev).to(bf)
        out_se, out_bn, dy, gres = (torch.empty_like(y) for _ in range(4))
        # conv3's epilogue partials: from the conv itself (Cin = C / 4)
        Cin = C // 4
        x = torch.randn(M, Cin, device=dev).to(bf)
        w = torch.randn(C, Cin, device=dev) * 0.05
        wp, wt = (torch.empty(w.numel(), dtype=bf, device=dev) for _ in range(2))
        call("es_conv2d_pack_bf16", ptr(w), C, Cin, 1, 1, ptr(wp), ptr(wt), s)
        part = torch.empty(lib.es_conv2d_bnstats_size(M, C), device=dev)
        call("es_conv2d_fwd_bf16_ex", ptr(x), N, H, H, Cin, HW * Cin, H * Cin, Cin, 1, ptr(wp), None, C, 1, 1, 1, 0,
             ptr(y), HW * C, H * C, C, 0, ptr(part), 3, s)
        gam, bet = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        nbt = torch.zeros((), dtype=torch.int64, device=dev)
        mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        wd, wu = torch.randn(R, C, device=dev) * (2.0 / R) ** 0.5, torch.randn(C, R, device=dev) * (2.0 / C) ** 0.5
        ybar, av, sg, p1, p2, da = (torch.empty(N, C, device=dev) for _ in range(6))
        hh = torch.empty(N, R, device=dev)
        dwd, dwu, dg, db = torch.empty_like(wd), torch.empty_like(wu), torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws_sq = torch.empty(lib.es_se_squeeze_workspace(N, HW, C, 1), device=dev)
        ws_su = torch.empty(lib.es_se_bn_bwd_sums_workspace(N, HW, C, 1), device=dev)
        ws_g = torch.empty(lib.es_se_gate_bwd_workspace(N, C, R), device=dev)
        ws_bn = torch.empty(lib.es_chan_workspace(M, C), device=dev)

        def stats(yp, resp, relu):
            call("es_bn2d_fwd_partials_ex", ptr(y), M, C, ptr(part), ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(nbt), 0.1,
                 1e-5, resp, relu, yp, ptr(mean), ptr(rstd), 1, s)

        def se_fwd():
            stats(None, None, 1)
            call("es_se_squeeze_ex", ptr(y), N, HW, C, ptr(mean), ptr(rstd), ptr(gam), ptr(bet), ptr(ybar), ptr(av),
                 ptr(ws_sq), 1, s)
            call("es_se_gate_fwd", ptr(av), ptr(wd), ptr(wu), N, C, R, ptr(hh), ptr(sg), s)
            call("es_se_bn_apply_ex", ptr(y), ptr(res), ptr(sg), N, HW, C, ptr(mean), ptr(rstd), ptr(gam), ptr(bet),
                 ptr(out_se), 1, s)

        def bn_fwd():
            stats(ptr(out_bn), ptr(res), 1)

        def se_bwd():
            call("es_se_bn_bwd_sums_ex", ptr(y), ptr(out_se), ptr(dout), N, HW, C, ptr(mean), ptr(rstd), ptr(p1), ptr(p2),
                 ptr(ws_su), 1, s)
            call("es_se_gate_bwd", ptr(p1), ptr(p2), ptr(ybar), ptr(av), ptr(hh), ptr(sg), ptr(wd), ptr(wu), ptr(gam),
                 ptr(bet), ptr(mean), ptr(rstd), N, C, R, ptr(dwd), ptr(dwu), ptr(da), ptr(dg), ptr(db), ptr(ws_g), s)
            call("es_se_bn_bwd_dx_ex", ptr(y), ptr(out_se), ptr(dout), ptr(sg), ptr(da), N, HW, C, ptr(mean), ptr(rstd),
                 ptr(gam), ptr(dg), ptr(db), 1, ptr(dy), ptr(gres), 0, 1, s)

        def bn_bwd():
            call("es_bn2d_bwd_ex", ptr(y), ptr(out_bn), ptr(dout), M, C, 1, ptr(gam), ptr(mean), ptr(rstd), 1, ptr(rv),
                 1e-5, ptr(dy), ptr(gres), ptr(dg), ptr(db), 0, ptr(ws_bn), 1, s)

        for fn in (se_fwd, bn_fwd, se_bwd, bn_bwd):  # warm-up
            fn()
        torch.cuda.synchronize()
        w = _windows({"se_fwd": se_fwd, "bn_fwd": bn_fwd, "se_bwd": se_bwd, "bn_bwd": bn_bwd}, a.iters, a.reps)
        row = {"shape": f"{name} {N}x{H}x{H}x{C}", "map_MiB": round(y.numel() * 2 / 2 ** 20, 1)}
        for k, v in w.items():
            row[k + "_us"], row[k + "_spread"] = (round(t, 4) for t in _stat(v, a.reps))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


class _DS:
    df = None


class _DL(list):
    dataset = _DS()


def steps(a):
    from endossl.build import build_model
    from endossl.supervised import SupLearning
    from endossl.utils import AttrDict
    out = []
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.n, 3, 224, 224, generator=g).cuda()
    yv = torch.randint(0, 23, (a.n,), generator=g).cuda()
    for name, graph in (("resnet50se", False), ("resnet50", False), ("resnet50", True)):
        cfg = AttrDict(DATA=AttrDict(BATCH_SIZE=a.n, MU=1, IMG_SIZE=224, TARGET_NAME="target"),
                       MODEL=AttrDict(NAME=name, NUM_CLASSES=23, MARGIN="None", IS_TRIPLET=False, TYPE_SEMI="FixMatch",
                                      PRE_TRAIN_PATH="None"),
                       TRAIN=AttrDict(IS_SSL=False, IS_FREEZE=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3,
                                      EVAL_STEP=1, CLS_WEIGHT=False, THRES=0.0, T=1.0, LAMBDA_U=1.0, LAMBDA_C=1.0,
                                      EPOCHS=1, WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8,
                                      SCH_NAME="const", FREQ_EVAL=1))
        tr = SupLearning(build_model(cfg, seed=0), opt_func="Adam", lr=1e-3, device="cuda")
        tr.use_graph = graph
        tr.get_dataloader(_DL([(x, yv)]), None, None)
        tr.get_config(cfg)
        for _ in range(4):  # warm-up (the graph is captured at the third step)
            tr.step((x, yv))
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = tr.step((x, yv))["loss"]
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        med = ts[len(ts) // 2]
        row = {"step": name + (" graph" if graph else " eager"), "B": a.n, "median_ms": round(med, 3),
               "spread": round((ts[-1] - ts[0]) / med, 4), "loss_finite": bool(torch.isfinite(loss))}
        out.append(row)
        print(json.dumps(row), flush=True)
        del tr
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--md", default=None, help="also write the tables as markdown to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("se_tail_bench.py times kernels on the MI355X: no GPU here")
    lib = _lib.load()
    rows = tails(a, lib, _lib.stream())
    srows = steps(a) if a.steps > 0 else []
    if a.md:
        with open(a.md, "w") as f:
            f.write("| shape | map MiB | SE fwd us | BN fwd us | SE bwd us | BN bwd us |\n|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['shape']} | {r['map_MiB']} | {r['se_fwd_us']:.1f} ({100 * r['se_fwd_spread']:.1f} %) | "
                        f"{r['bn_fwd_us']:.1f} ({100 * r['bn_fwd_spread']:.1f} %) | "
                        f"{r['se_bwd_us']:.1f} ({100 * r['se_bwd_spread']:.1f} %) | "
                        f"{r['bn_bwd_us']:.1f} ({100 * r['bn_bwd_spread']:.1f} %) |\n")
            f.write("\n| step | B | median ms | spread |\n|---|---|---|---|\n")
            for r in srows:
                f.write(f"| {r['step']} | {r['B']} | {r['median_ms']:.2f} | {100 * r['spread']:.1f} % |\n")


if __name__ == "__main__":
    main()
