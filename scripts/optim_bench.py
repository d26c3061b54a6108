"""Optimizer sweep microbenchmark at ViT-S/16's parameter count, EMA on: es_adam_ema_step, es_adamw_ema_step and
es_sgd_ema_step alternated in one process (device events around `--iters` back-to-back launches per sample,
`--rounds` samples each after a warm-up), median / p10 / p90 per launch and bytes/s from the algorithmic byte
counts: Adam 36 B per element (p, g, m, v, ema read; p, m, v, ema written), AdamW the same + n/64 B of class
map, SGD 28 B per element + the map.  The class map is the model's own (class_map(NativeViT)).
  python scripts/optim_bench.py [--rounds 40] [--iters 10] [--out profiles/optim_sweep.txt]"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endoscopy-image-classification_amd"))
import torch  # noqa: E402

from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402
from endossl.optimizer import class_map  # noqa: E402
from endossl.vit import NativeViT, ViTConfig  # noqa: E402


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, int(round(q * (len(xs) - 1)))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py times kernels on the MI355X: no GPU here, nothing measured")
    model = NativeViT(ViTConfig(), seed=0)
    n = model.numel
    cls = class_map(model).cuda()
    torch.manual_seed(0)
    p0 = model.flat.cuda()
    g = torch.randn(n, device="cuda") * 1e-2
    state = {k: (p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), p0.clone())
             for k in ("adam", "adamw", "sgd")}
    s = _lib.stream()
    d, lr, t = 0.999, 1e-3, [0]

    def adam():
        p, m, v, e = state["adam"]
        bc1, bc2 = 1 - 0.9 ** t[0], 1 - 0.999 ** t[0]
        call("es_adam_ema_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(e), n, 0.9, 0.999, 1e-8, -lr / bc1,
             math.sqrt(bc2), d, 1.0 - d, 1.0, s)

    def adamw():
        p, m, v, e = state["adamw"]
        bc1, bc2 = 1 - 0.9 ** t[0], 1 - 0.999 ** t[0]
        call("es_adamw_ema_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(e), ptr(cls), n, 0.9, 0.999, 1 - 0.9, 1 - 0.999,
             1e-8, math.sqrt(bc2), -lr / bc1, -lr / bc1, 1 - lr * 0.05, 1.0, d, 1.0 - d, 1.0, s)

    def sgd():
        p, m, _, e = state["sgd"]
        call("es_sgd_ema_step", ptr(p), ptr(g), ptr(m), ptr(e), ptr(cls), n, 0.9, -lr, -lr, 0.05, 0.0, 1, d, 1.0 - d,
             1.0, s)

    kernels = {"es_adam_ema_step": (adam, 36 * n), "es_adamw_ema_step": (adamw, 36 * n + n // 64),
               "es_sgd_ema_step": (sgd, 28 * n + n // 64)}
    for _ in range(args.warmup):
        t[0] += 1
        for f, _b in kernels.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in kernels}
    for _ in range(args.rounds):
        for k, (f, _b) in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                t[0] += 1
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)  # us per launch
    trained = int((cls != 0).sum()) * 64
    lines = [f"optimizer sweeps, n = {n} floats (ViT-S/16, {trained} in trained granules), EMA on, "
             f"{args.rounds} samples x {args.iters} launches each, alternated in one process",
             f"{'entry':<20}{'median us':>11}{'p10 us':>9}{'p90 us':>9}{'bytes':>12}{'TB/s (median)':>15}"]
    for k, (_f, byts) in kernels.items():
        med, lo, hi = _pct(times[k], 0.5), _pct(times[k], 0.1), _pct(times[k], 0.9)
        lines.append(f"{k:<20}{med:>11.2f}{lo:>9.2f}{hi:>9.2f}{byts:>12d}{byts / med / 1e6:>15.3f}")
    a, w = times["es_adam_ema_step"], times["es_adamw_ema_step"]
    gap, spread = _pct(w, 0.5) - _pct(a, 0.5), _pct(a, 0.9) - _pct(a, 0.1)
    lines.append(f"AdamW median - Adam median = {gap:+.2f} us; Adam p90 - p10 = {spread:.2f} us: "
                 f"{'within' if gap <= spread else 'OUTSIDE'} Adam's own spread")
    lines.append(f"SGD median / Adam median = {_pct(times['es_sgd_ema_step'], 0.5) / _pct(a, 0.5):.3f} "
                 f"(byte ratio {28 / 36:.3f})")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
