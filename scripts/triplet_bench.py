"""Supervised triplet step timing at ViT-S/16, 224², bs = 64 triplets (192 train rows), Adam + EMA, beside the
plain supervised ViT step over the same 192 rows: both trainers in one process, alternated sample by sample
(device events around `--iters` back-to-back steps per sample, `--rounds` samples each after a warm-up), median /
p10 / p90 per step.  The batches live on the device, so the figures are the step's launches (forward, losses,
backward, optimizer + EMA sweep), not a loader.
  python scripts/triplet_bench.py [--rounds 20] [--iters 3] [--out profiles/triplet_step.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endoscopy-image-classification_amd"))
import torch  # noqa: E402

from endossl.build import build_model  # noqa: E402
from endossl.supervised import SupLearning  # noqa: E402
from endossl.utils import AttrDict  # noqa: E402


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, int(round(q * (len(xs) - 1)))))]


class _DL(list):
    class dataset:
        df = None


def _trainer(triplet, bs):
    cfg = AttrDict(DATA=AttrDict(BATCH_SIZE=bs, IMG_SIZE=224, TARGET_NAME="target"),
                   MODEL=AttrDict(NAME="vit_small_patch16_224", NUM_CLASSES=23, MARGIN="None", IS_TRIPLET=triplet,
                                  PRE_TRAIN_PATH="None"),
                   TRAIN=AttrDict(IS_SSL=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, CLS_WEIGHT=False,
                                  THRES=0.95, LAMBDA_C=1.0, EPOCHS=1, WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4,
                                  LR_DECAY=0.8, SCH_NAME="const", FREQ_EVAL=1))
    tr = SupLearning(build_model(cfg, seed=0), opt_func="Adam", lr=1e-3, device="cuda")
    tr.get_dataloader(_DL(), None)
    tr.get_config(cfg)
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("triplet_bench.py times steps on the MI355X: no GPU here, nothing measured")
    bs = args.bs
    g = torch.Generator().manual_seed(0)
    imgs = tuple(torch.randn(bs, 3, 224, 224, generator=g).cuda() for _ in range(3))
    ys = tuple(torch.randint(0, 23, (bs,), generator=g).cuda() for _ in range(3))
    trip, plain = _trainer(True, bs), _trainer(False, 3 * bs)
    tbatch = (imgs, ys)
    pbatch = (torch.cat(imgs), torch.cat(ys))
    steps = {"triplet step (3 x %d rows)" % bs: lambda: trip.step(tbatch),
             "plain supervised step (%d rows)" % (3 * bs): lambda: plain.step(pbatch)}
    for _ in range(args.warmup):
        for f in steps.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k, f in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                out = f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.iters)  # ms per step
    assert torch.isfinite(out["loss"]).item()
    lines = [f"ViT-S/16 224^2, 23 classes, Adam + EMA, device-resident batches; {args.rounds} samples x {args.iters} "
             f"steps each, the two trainers alternated in one process",
             f"{'step':<36}{'median ms':>11}{'p10 ms':>9}{'p90 ms':>9}{'rows/s (median)':>17}"]
    for k in steps:
        med, lo, hi = _pct(times[k], 0.5), _pct(times[k], 0.1), _pct(times[k], 0.9)
        lines.append(f"{k:<36}{med:>11.3f}{lo:>9.3f}{hi:>9.3f}{3 * bs / med * 1e3:>17.0f}")
    a, b = (_pct(times[k], 0.5) for k in steps)
    lines.append(f"triplet median / plain median = {a / b:.3f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
