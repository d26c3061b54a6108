"""EZBM stage-2 step timing at ViT-S/16's head (D = 384, F = 96, C = 6, n = 192 rows: the published config's
32 x 6), Adam + EMA, and how much of that step is the optimizer + EMA sweep over the whole flat buffer
(the trainer's _finish_step alone, on the same trainer): the two alternated sample by sample in one process (device
events around `--iters` back-to-back calls per sample, `--rounds` samples each after a warm-up), median / p10 /
p90.  The bank lives on the device (random features, every class present); the trunk is never run.
  python scripts/ezbm_bench.py [--rounds 40] [--iters 10] [--out profiles/ezbm_stage2.txt]
--model resnet50 times the published config's backbone instead (NativeResNetEmb, build_model's cnn_emb opt-in: D = 2048,
F = 512, n = 192): --heads narrow | wide | both selects the head kernel family (comatch.hip's es_dense_* / the tiled
es_dense_wide_* of EmbHeads.WIDE_LAYERS); `both` alternates the two on the one trainer, sample by sample.
  python scripts/ezbm_bench.py --model resnet50 --heads both --out profiles/ezbm_stage2_resnet50.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endoscopy-image-classification_amd"))
import torch  # noqa: E402

from endossl.build import build_model  # noqa: E402
from endossl.ezbm import EZBM  # noqa: E402
from endossl.utils import AttrDict  # noqa: E402

CLS_NUM = [400, 120, 60, 30, 12, 5]


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, int(round(q * (len(xs) - 1)))))]


class _DS:
    df = None

    def get_cls_num_list(self):
        return CLS_NUM

    def __len__(self):
        return sum(CLS_NUM)


class _DL(list):
    dataset = _DS()


def _trainer(bs, mu, expansion, model="vit_small_patch16_224"):
    cfg = AttrDict(DATA=AttrDict(BATCH_SIZE=bs, MU=mu, IMG_SIZE=224, TARGET_NAME="target"),
                   MODEL=AttrDict(NAME=model, NUM_CLASSES=len(CLS_NUM), MARGIN="None", IS_TRIPLET=True,
                                  PRE_TRAIN_PATH="None"),
                   TRAIN=AttrDict(IS_SSL=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, CLS_WEIGHT=False,
                                  THRES=0.95, LAMBDA_C=4, EPOCHS=1, WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4,
                                  LR_DECAY=0.8, SCH_NAME="const", FREQ_EVAL=1, EXPANSION=expansion))
    tr = EZBM(build_model(cfg, seed=0, cnn_emb=model.startswith("resnet")), opt_func="Adam", lr=1e-3, device="cuda")
    tr.get_dataloader(_DL(), None)
    tr.get_config(cfg)
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--mu", type=int, default=6)
    ap.add_argument("--expansion", default="balance")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="vit_small_patch16_224", choices=["vit_small_patch16_224", "resnet50"])
    ap.add_argument("--heads", default="both", choices=["narrow", "wide", "both"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ezbm_bench.py times steps on the MI355X: no GPU here, nothing measured")
    tr = _trainer(args.bs, args.mu, args.expansion, args.model)
    n, D, C = args.bs * args.mu, tr.model.cfg.dim, len(CLS_NUM)
    g = torch.Generator().manual_seed(0)
    N = sum(CLS_NUM)
    y = torch.cat([torch.full((c,), i, dtype=torch.int64) for i, c in enumerate(CLS_NUM)])[torch.randperm(N, generator=g)]
    tr.set_bank(torch.randn(N, D, generator=g).cuda(), y.cuda())
    tr.setup_stage_2()
    def step(wide=None):
        if wide is not None:
            tr.model.wide_heads = wide
        return tr.step_stage_2(n=n)

    if args.model == "resnet50":
        fams = {"narrow": (False,), "wide": (True,), "both": (False, True)}[args.heads]
        calls = {f"stage-2 step ({n} rows), heads {'wide' if w else 'narrow'}": (lambda w=w: step(w)) for w in fams}
    else:
        calls = {f"stage-2 step ({n} rows, 2 x {n} through fc)": step}
    calls["optimizer + EMA sweep alone (_finish_step)"] = lambda: (tr._inflight.wait(), tr._finish_step())
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.iters * 1e3)  # us per call
    out = tr.step_stage_2(n=n)
    assert torch.isfinite(out["loss"]).item()
    lines = [f"EZBM stage 2 at {'ViT-S/16' if args.model != 'resnet50' else 'ResNet-50'}'s head: D = {D}, F = {D // 4}, C = {C}, n = {n} rows a step, bank of {N} rows, "
             f"EXPANSION '{args.expansion}', Adam + EMA over the flat buffer of {tr.model.flat.numel()} floats; "
             f"{args.rounds} samples x {args.iters} calls each, alternated in one process; device events around "
             f"back-to-back calls (host launch gaps included)",
             f"{'call':<48}{'median us':>11}{'p10 us':>9}{'p90 us':>9}"]
    for k in calls:
        lines.append(f"{k:<48}{_pct(times[k], 0.5):>11.1f}{_pct(times[k], 0.1):>9.1f}{_pct(times[k], 0.9):>9.1f}")
    a, b = (_pct(times[k], 0.5) for k in (list(calls)[0], list(calls)[-1]))
    lines.append(f"sweep median / step median = {b / a:.3f}; step - sweep = {a - b:.1f} us for the sampler, the head's "
                 f"forward and backward over {2 * n} rows and the loss")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
