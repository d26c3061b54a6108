"""The direct 1 x 1 conv kernels (es_conv1x1_*) against the implicit-GEMM kernels (es_conv2d_*_bf16_ex) in isolation,
over the twelve distinct stride-1 1 x 1 conv shapes of ResNet-50 at 224^2 (N = 64 images), bf16 maps.
  python scripts/conv1x1_bench.py [--n 64] [--iters 9] [--reps 20] [--md table.md]
Per shape and pass (fwd: forward with the BatchNorm statistics, as conv1 / downsample.0 run; fwd_bnin: forward with
the input BatchNorm and the statistics, as conv3 runs; dgrad: data gradient): both kernels on the same buffers,
interleaved, `iters` windows of `reps` back-to-back launches between two device events each; the median window /
reps in us and the spread (max - min) / median of the windows.  `faster`: the direct kernel's median is below the
implicit kernel's by more than the implicit kernel's spread.  Outputs are compared bit for bit first."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endoscopy-image-classification_amd"))
import torch  # noqa: E402

from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402

# (name, H, Cin, Cout): timm resnet50's stride-1 1 x 1 convs (the stride sits on conv2, so a stage's first conv1
# runs at the previous stage's resolution); layer1.0.downsample.0 is l1_conv3's shape
SHAPES = [("l1.0_conv1_64to64", 56, 64, 64), ("l1_conv3_64to256", 56, 64, 256), ("l1_conv1_256to64", 56, 256, 64),
          ("l2.0_conv1_256to128", 56, 256, 128), ("l2_conv3_128to512", 28, 128, 512),
          ("l2_conv1_512to128", 28, 512, 128), ("l3.0_conv1_512to256", 28, 512, 256),
          ("l3_conv3_256to1024", 14, 256, 1024), ("l3_conv1_1024to256", 14, 1024, 256), ("l4.0_conv1_1024to512", 14, 1024, 512),
          ("l4_conv3_512to2048", 7, 512, 2048), ("l4_conv1_2048to512", 7, 2048, 512)]
PASSES = ("fwd", "fwd_bnin", "dgrad")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--md", default=None, help="also write the table as markdown to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv1x1_bench.py times kernels on the MI355X: no GPU here")
    lib = _lib.load()
    s = _lib.stream()
    dev = "cuda"
    N = a.n
    rows = []
    for name, H, Cin, Cout in SHAPES:
        M = N * H * H
        x = torch.randn(M, Cin, device=dev).bfloat16()
        dy = torch.randn(M, Cout, device=dev).bfloat16()
        w = torch.randn(Cout, Cin, device=dev) * 0.05
        wp = torch.empty(w.numel(), dtype=torch.bfloat16, device=dev)
        wt = torch.empty_like(wp)
        call("es_conv2d_pack_bf16", ptr(w), Cout, Cin, 1, 1, ptr(wp), ptr(wt), s)
        y = {v: torch.empty(M, Cout, device=dev, dtype=torch.bfloat16) for v in ("implicit", "direct")}
        dx = {v: torch.empty(M, Cin, device=dev, dtype=torch.bfloat16) for v in ("implicit", "direct")}
        part = {v: torch.empty(lib.es_conv2d_bnstats_size(M, Cout), device=dev) for v in ("implicit", "direct")}
        mean, rstd = torch.randn(Cin, device=dev) * 0.1, torch.rand(Cin, device=dev) + 0.5
        gam, bet = torch.rand(Cin, device=dev) + 0.5, torch.randn(Cin, device=dev) * 0.1
        bn = (ptr(mean), ptr(rstd), ptr(gam), ptr(bet))
        xs, ys = (H * H * Cin, H * Cin, Cin, 1), (H * H * Cout, H * Cout, Cout)
        fns = {
            ("fwd", "implicit"): lambda: call("es_conv2d_fwd_bf16_ex", ptr(x), N, H, H, Cin, *xs, ptr(wp), None, Cout,
                                              1, 1, 1, 0, ptr(y["implicit"]), *ys, 0, ptr(part["implicit"]), 3, s),
            ("fwd", "direct"): lambda: call("es_conv1x1_fwd_bf16_ex", ptr(x), M, Cin, ptr(wp), None, Cout,
                                            ptr(y["direct"]), 0, ptr(part["direct"]), 3, s),
            ("fwd_bnin", "implicit"): lambda: call("es_conv2d_fwd_bf16_bnin_ex", ptr(x), N, H, H, Cin, *xs, ptr(wp),
                                                   None, Cout, 1, 1, 1, 0, ptr(y["implicit"]), *ys, 0,
                                                   ptr(part["implicit"]), 3, *bn, s),
            ("fwd_bnin", "direct"): lambda: call("es_conv1x1_fwd_bf16_bnin_ex", ptr(x), M, Cin, ptr(wp), None, Cout,
                                                 ptr(y["direct"]), 0, ptr(part["direct"]), 3, *bn, s),
            ("dgrad", "implicit"): lambda: call("es_conv2d_bwd_data_bf16_ex", ptr(dy), *ys, ptr(wt), N, H, H, Cin, Cout,
                                                1, 1, 1, 0, ptr(dx["implicit"]), *xs, 0, 3, s),
            ("dgrad", "direct"): lambda: call("es_conv1x1_bwd_data_bf16_ex", ptr(dy), M, Cout, ptr(wt), Cin,
                                              ptr(dx["direct"]), 0, 3, s),
        }
        # warm-up of every launch, and the outputs bit for bit (the statistics partials with them)
        for pas in PASSES:
            fns[(pas, "implicit")]()
            fns[(pas, "direct")]()
            torch.cuda.synchronize()
            a_, b_ = (dx["implicit"], dx["direct"]) if pas == "dgrad" else (y["implicit"], y["direct"])
            if not torch.equal(a_, b_) or (pas != "dgrad" and not torch.equal(part["implicit"], part["direct"])):
                raise SystemExit(f"{name} {pas}: the direct kernel's output differs from the implicit kernel's")
        ts = {k: [] for k in fns}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.iters):
            for k, fn in fns.items():
                e0.record(torch.cuda.current_stream())
                for _ in range(a.reps):
                    fn()
                e1.record(torch.cuda.current_stream())
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        rec = {"shape": name, "M": M, "Cin": Cin, "Cout": Cout}
        for pas in PASSES:
            for v in ("implicit", "direct"):
                t = sorted(ts[(pas, v)])
                med = t[len(t) // 2]
                rec[f"{pas}_{v}"] = {"us": round(med, 1), "spread": round((t[-1] - t[0]) / med, 3)}
            i, d = rec[f"{pas}_implicit"], rec[f"{pas}_direct"]
            rec[f"{pas}_faster"] = bool(d["us"] < i["us"] * (1.0 - i["spread"]))
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        del x, dy, y, dx
        torch.cuda.empty_cache()
    head = " | ".join(f"{p} implicit us (spread) | {p} direct us | direct faster" for p in PASSES)
    lines = [f"| shape (N = {N}) | M | {head} |", "|---|---|" + "---|" * (3 * len(PASSES))]
    for r in rows:
        cells = []
        for p in PASSES:
            i, d = r[f"{p}_implicit"], r[f"{p}_direct"]
            cells += [f"{i['us']} ({100 * i['spread']:.1f} %)", f"{d['us']}", "yes" if r[f"{p}_faster"] else "no"]
        lines.append(f"| {r['shape']} | {r['M']} | " + " | ".join(cells) + " |")
    print("\n".join(lines), flush=True)
    if a.md:
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
