"""ResNet-50 SupLearning.step time on the MI355X (bench.py measures the flagship ViT workload; this is the
bench.py-independent number DESIGN.md quotes): 224^2, 23 classes, Adam + EMA, the default bf16 convs and maps, graph
replay as SupLearning runs it.
  python scripts/resnet50_step_bench.py [--batch 16 64] [--steps 30] [--warmup 8] [--conv1x1 1 0]
Per batch size and es_set_conv_1x1 value (interleaved: the values alternate within a batch size, `--rounds` times):
a host clock around `steps` steps that ends in a device synchronise, after `warmup` steps (GRAPH_WARM eager steps and
the capture among them).  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endoscopy-image-classification_amd"))
import torch  # noqa: E402

from endossl import _lib  # noqa: E402
from endossl.build import build_model  # noqa: E402
from endossl.supervised import SupLearning  # noqa: E402
from endossl.utils import AttrDict  # noqa: E402


class _DS:
    df = None


class _DL(list):
    dataset = _DS()


def trainer(batch):
    cfg = AttrDict(DATA=AttrDict(BATCH_SIZE=batch, IMG_SIZE=224, TARGET_NAME="target"),
                   MODEL=AttrDict(NAME="resnet50", NUM_CLASSES=23, MARGIN="None", IS_TRIPLET=False,
                                  TYPE_SEMI="FixMatch", PRE_TRAIN_PATH="None"),
                   TRAIN=AttrDict(IS_SSL=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, CLS_WEIGHT=False, EPOCHS=1,
                                  WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="const",
                                  FREQ_EVAL=1))
    tr = SupLearning(build_model(cfg, seed=0), opt_func="Adam", lr=1e-3, device="cuda")
    tr.get_dataloader(_DL([None]), None, None)
    tr.get_config(cfg)
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--conv1x1", type=int, nargs="+", default=[1, 0])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet50_step_bench.py times steps on the MI355X: no GPU here")
    lib = _lib.load()
    for B in a.batch:
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, 3, 224, 224, generator=g).cuda()
        y = torch.randint(0, 23, (B,), generator=g).cuda()
        trs = {}
        for v in a.conv1x1:  # one trainer (and one captured graph) per knob value: the capture fixes the launches
            lib.es_set_conv_1x1(v)
            trs[v] = trainer(B)
            for _ in range(a.warmup):
                out = trs[v].step((x, y))
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out["loss"]))
        for r in range(a.rounds):
            for v in a.conv1x1:
                lib.es_set_conv_1x1(v)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    out = trs[v].step((x, y))
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / a.steps
                print(json.dumps({"model": "resnet50", "batch": B, "img": 224, "conv_1x1": v, "round": r,
                                  "ms_per_step": round(dt * 1e3, 3), "img_per_s": round(B / dt, 1),
                                  "loss": round(out["loss"].item(), 4)}), flush=True)
        lib.es_set_conv_1x1(1)
        del trs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
