"""The device input path (endossl.host_aug.DeviceBatcher, csrc/device_aug.hip) measured three ways, on
synthetic decoded RGB 500 x 375 frames, IS_CROP, S = 224 (the frames of bench.py --host-input):

  (a) host: images/s of the plan-and-copy producer (what DeviceBatcher's host thread does per batch: frames
      copied into the arena + esh_fixmatch_device_plan) against transform_batch("fixmatch") on the same
      frames.  The producer is one thread; the transforms are timed at 1 thread and at --threads.
      Needs no GPU:  python scripts/device_aug_bench.py --part a
      transform_batch("comatch") and transform_batch("labeled") are timed the same way.
  (b) device: HIP-event time of one 448-image es_aug_fixmatch_u8 batch (resize + crop + strong chain), and of
      es_aug_comatch_u8 and es_aug_labeled_u8 on the same frames in the same run.
  (c) the F1 step (ViT-S/16, B = 64, mu = 7) fed by DeviceBatcher with resident False / True, beside the same
      step fed by HostBatcher and the same step on a batch that stays in HBM.
  (d) the C1 step (CoMatch ViT-S/16, bench.py's c1 sizes: B = 64, mu = 7, L = 64, a 65,536-entry bank) fed by
      HostBatcher, by DeviceBatcher(resident=True) for both the unlabeled and the labeled batch, and on a
      batch that stays in HBM.

  python scripts/device_aug_bench.py [--part a|b|c|d|all] [--steps 20] [--threads N]
Prints one JSON line per part.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "endoscopy-image-classification_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from endossl import host_aug  # noqa: E402

S, B, MU = 224, 64, 7


def frames(n=64):
    g = np.random.default_rng(7)
    base = g.integers(0, 256, (60, 80, 3), dtype=np.uint8)
    return [host_aug.resize_bilinear(base ^ np.uint8(i * 29 % 256), (500, 375)) for i in range(n)]


def granted_cpus():
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    for k in ("OMP_NUM_THREADS", "MAX_JOBS"):
        if os.environ.get(k, "").isdigit():
            n = min(n, int(os.environ[k]))
    return max(1, n)


def part_a(srcs, threads, reps=5):
    n = B * MU
    ws = np.array([a.shape[1] for a in srcs], np.int32)
    hs = np.array([a.shape[0] for a in srcs], np.int32)
    arena = np.empty(n * 500 * 375 * 3, np.uint8)
    entries = np.empty(n * host_aug.ENTRY_BYTES, np.uint8)
    coeffs = np.empty(1 << 16, np.int32)
    offs = np.arange(len(srcs), dtype=np.int64) * (500 * 375 * 3)
    g = np.random.default_rng(0)
    res = {"part": "a", "batch": n, "host_threads": threads}
    for name, kw in (("copy_and_plan_images_per_s_1thread", dict(arena=arena, threads=1)),
                     ("copy_and_plan_images_per_s_4thread", dict(arena=arena, threads=4)),
                     ("plan_only_resident_images_per_s_1thread", dict(offsets=offs))):
        best = 1e9
        for r in range(reps + 1):  # the first pass touches the arena's pages
            idx = g.integers(0, len(srcs), n)
            t0 = time.perf_counter()
            host_aug.plan_and_copy(srcs, ws, hs, idx, S, True, r, entries, coeffs, **kw)
            if r:
                best = min(best, time.perf_counter() - t0)
        res[name] = round(n / best, 1)
    imgs = [srcs[i] for i in g.integers(0, len(srcs), n)]
    for t in sorted({1, threads}):
        host_aug.transform_batch(imgs[:8], S, "fixmatch", threads=t)
        t0 = time.perf_counter()
        host_aug.transform_batch(imgs, S, "fixmatch", seed=1, threads=t)
        res[f"transform_batch_fixmatch_pairs_per_s_{t}thread"] = round(n / (time.perf_counter() - t0), 1)
        for kind, unit in (("comatch", "triplets"), ("labeled", "images")):
            host_aug.transform_batch(imgs[:8], S, kind, threads=t)
            t0 = time.perf_counter()
            host_aug.transform_batch(imgs, S, kind, seed=1, threads=t)
            res[f"transform_batch_{kind}_{unit}_per_s_{t}thread"] = round(n / (time.perf_counter() - t0), 1)
    return res


def part_b(srcs, reps=10):
    n = B * MU
    imgs = [srcs[i % len(srcs)] for i in range(n)]
    dev = torch.device("cuda")
    lib = host_aug._device()
    ws = [a.shape[1] for a in imgs]
    hs = [a.shape[0] for a in imgs]
    arena = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    out = {}
    for label, kind in (("weak_and_strong", "fixmatch"), ("weak_only", "eval"), ("comatch", "comatch"),
                        ("labeled", "labeled")):
        entries, coeffs, used = host_aug.device_plan(kind, ws, hs, S, True, seed=1)
        ent = host_aug._dev_u8(entries, dev)
        coef = torch.from_numpy(coeffs[:used]).to(dev)
        wsp = torch.empty(getattr(lib, host_aug._CALLS[kind][1])(n, S, 1, max(ws), max(hs)), dtype=torch.uint8,
                          device=dev)
        ms = []
        for r in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            host_aug._run_device(kind, arena, arena.numel(), ent, coef, used, n, S, True, max(hs), wsp, dev)
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ms.append(e0.elapsed_time(e1))
        out[label + "_ms_median"] = round(float(np.median(ms)), 3)
        out[label + "_ms_min"] = round(min(ms), 3)
    out["images_per_s"] = round(n / out["weak_and_strong_ms_median"] * 1e3, 1)
    out["comatch_over_fixmatch"] = round(out["comatch_ms_median"] / out["weak_and_strong_ms_median"], 2)
    return {"part": "b", "batch": n, "frames": "500x375", "S": S, **out}


def part_c(srcs, threads, steps):
    from endossl.fixmatch import FixMatch
    from endossl.utils import AttrDict
    from endossl.vit import NativeViT, ViTConfig
    dev = torch.device("cuda")
    tr = FixMatch(NativeViT(ViTConfig(), seed=0), device=dev)
    cfg = AttrDict(DATA=AttrDict(BATCH_SIZE=B, MU=MU, IMG_SIZE=S, TARGET_NAME="target"),
                   MODEL=AttrDict(NAME="vit_small_patch16_224", NUM_CLASSES=23),
                   TRAIN=AttrDict(IS_FREEZE=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, EVAL_STEP=1,
                                  CLS_WEIGHT=False, THRES=0.95, T=1.0, LAMBDA_U=1.0, EPOCHS=1, WARMUP_EPOCHS=0,
                                  DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="const"))
    tr.get_dataloader((None, None), None)
    tr.get_config(cfg)
    tr.class_weights = torch.linspace(0.5, 2.0, 23, device=dev)
    y = torch.randint(0, 23, (B,), device=dev)
    res = {"part": "c", "B": B, "mu": MU, "steps": steps, "host_threads": threads, "unit": "unlabeled images/s"}

    def timed(name, one):
        for _ in range(3):
            one()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[name] = {"value": round(B * MU * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3)}

    w0, s0 = host_aug.device_transform_batch([srcs[i % len(srcs)] for i in range(B * MU)], S, "fixmatch", seed=5)
    (x0,) = host_aug.transform_batch(srcs[:B], S, "labeled", seed=5, threads=threads)
    x0 = x0.to(dev)
    timed("hbm_resident_batch", lambda: tr.step(((x0, y), ((w0, s0), None))))

    def fed(make_unl, lab_threads):
        lab = host_aug.HostBatcher(srcs, batch=B, size=S, kind="labeled", seed=1, threads=lab_threads, device=dev)
        unl = make_unl()

        def one():
            (x,) = lab.next()
            uw, us = unl.next()
            return tr.step(((x, y), ((uw, us), None)))
        return one

    timed("host_batcher", fed(lambda: host_aug.HostBatcher(srcs, batch=B * MU, size=S, kind="fixmatch", seed=2,
                                                           threads=threads, device=dev), threads))
    # the labeled transform (64 images a step) stays on the host: with every granted thread it competes with the
    # thread that launches the step, so the device-fed runs are also timed with a quarter of them
    for lab_threads in sorted({threads, max(1, threads // 4)}, reverse=True):
        for resident in (False, True):
            timed(f"device_batcher_resident_{resident}_labeled_threads_{lab_threads}",
                  fed(lambda: host_aug.DeviceBatcher(srcs, batch=B * MU, size=S, kind="fixmatch", seed=2, device=dev,
                                                     resident=resident), lab_threads))
    # the unlabeled producer alone on the device path: labeled batch fixed in HBM (what remains of the gap to the
    # resident-batch step is then the device transform itself)
    for resident in (False, True):
        unl = host_aug.DeviceBatcher(srcs, batch=B * MU, size=S, kind="fixmatch", seed=2, device=dev,
                                     resident=resident)

        def only_unl():
            uw, us = unl.next()
            return tr.step(((x0, y), ((uw, us), None)))
        timed(f"device_batcher_resident_{resident}_labeled_in_hbm", only_unl)
    return res


def part_d(srcs, threads, steps):
    from endossl.comatch import CoMatch
    from endossl.comatch_model import NativeViTEmb
    from endossl.utils import AttrDict
    from endossl.vit import ViTConfig
    dev = torch.device("cuda")
    L, Q = 64, 65536
    tr = CoMatch(NativeViTEmb(ViTConfig(head="emb", low_dim=L), seed=0), device=dev)
    cfg = AttrDict(DATA=AttrDict(BATCH_SIZE=B, MU=MU, IMG_SIZE=S, TARGET_NAME="target"),
                   MODEL=AttrDict(NAME="vit_small_patch16_224", NUM_CLASSES=23, LOW_DIM=L, TYPE_SEMI="CoMatch"),
                   TRAIN=AttrDict(IS_FREEZE=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, EVAL_STEP=1,
                                  CLS_WEIGHT=False, THRES=0.95, T=1.0, LAMBDA_U=2.0, LAMBDA_C=2.0, EPOCHS=1,
                                  WARMUP_EPOCHS=0, DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="const"))
    tr.get_dataloader((None, None), None)
    tr.get_config(cfg)
    tr.set_queue_size(Q)
    g = torch.Generator(device=dev).manual_seed(1000)
    tr.queue_feats.copy_(torch.nn.functional.normalize(torch.randn(Q, L, generator=g, device=dev), dim=1))
    tr.queue_probs.copy_(torch.softmax(torch.randn(Q, 23, generator=g, device=dev) * 3, 1))
    y = torch.randint(0, 23, (B,), device=dev)
    res = {"part": "d", "B": B, "mu": MU, "steps": steps, "host_threads": threads, "unit": "unlabeled images/s"}

    def timed(name, one):
        for _ in range(3):
            one()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[name] = {"value": round(B * MU * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3)}

    u0 = host_aug.device_transform_batch([srcs[i % len(srcs)] for i in range(B * MU)], S, "comatch", seed=5)
    (x0,) = host_aug.device_transform_batch(srcs[:B], S, "labeled", seed=5)
    timed("hbm_resident_batch", lambda: tr.step(((x0, y), (u0, None))))

    def fed(batcher, **kw):
        lab = batcher(srcs, batch=B, size=S, kind="labeled", seed=1, device=dev, **kw)
        unl = batcher(srcs, batch=B * MU, size=S, kind="comatch", seed=2, device=dev, **kw)

        def one():
            (x,) = lab.next()
            return tr.step(((x, y), (unl.next(), None)))
        return one

    timed("host_batcher", fed(host_aug.HostBatcher, threads=threads))
    timed("device_batcher_resident_True", fed(host_aug.DeviceBatcher, resident=True))
    timed("device_batcher_resident_False", fed(host_aug.DeviceBatcher, resident=False))
    timed("hbm_resident_batch_again", lambda: tr.step(((x0, y), (u0, None))))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["a", "b", "c", "d", "all"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args()
    threads = args.threads or granted_cpus()
    srcs = frames()
    if args.part in ("a", "all"):
        print(json.dumps(part_a(srcs, threads)), flush=True)
    if args.part in ("b", "all"):
        print(json.dumps(part_b(srcs)), flush=True)
    if args.part in ("c", "all"):
        print(json.dumps(part_c(srcs, threads, args.steps)), flush=True)
    if args.part in ("d", "all"):
        print(json.dumps(part_d(srcs, threads, args.steps)), flush=True)


if __name__ == "__main__":
    main()
