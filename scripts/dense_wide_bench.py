"""The embedding heads' dense layers at ResNet-50's width (D = 2048): comatch.hip's es_dense_fwd / es_dense_bwd (the
yardstick) against the tiled f32-MFMA es_dense_wide_fwd / es_dense_wide_bwd (csrc/dense_wide.hip) on the same buffers,
alternated sample by sample in one process -- device events around `--iters` back-to-back calls per sample,
`--rounds` samples each after a warm-up; median / p10 / p90 in microseconds per call.

Rows n and embedding width L of the reference's ResNet-50 configs: n = 384 (EZBM stage 2: 2 x 192 rows, fc only, no
dX), n = 96 (the triplet step at B = 32, L = 256), n = 512 and 704 (CoMatch at B = 32, mu = 5 / 7, L = 64).
A layer belongs on the wide family only where its wide p90 is below the existing kernels' p10 in this run, forward
and backward, at every n it runs at: the last lines of the output say which do (EmbHeads.WIDE_LAYERS follows them).
  python scripts/dense_wide_bench.py [--rounds 30] [--iters 20] [--out profiles/dense_wide.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endoscopy-image-classification_amd"))
import torch  # noqa: E402

from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402

D, C = 2048, 6


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, int(round(q * (len(xs) - 1)))))]


def cases():
    """(n, layer, K, N, act, keep, want_dx)"""
    out = [(384, "fc.0", D, D // 4, 1, True, False), (384, "fc.4", D // 4, C, 0, False, True)]
    for n, L in ((96, 256), (512, 64), (704, 64)):
        out += [(n, "fc.0", D, D // 4, 1, True, True), (n, "fc.4", D // 4, C, 0, False, True),
                (n, "head_emb.0", D, 3 * L, 2, False, True), (n, "head_emb.2", 3 * L, L, 0, False, True)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_wide_bench.py times kernels on the MI355X: no GPU here, nothing measured")
    lib, s = _lib.load(), _lib.stream()
    g = torch.Generator().manual_seed(0)
    lines = [f"dense head layers at D = {D}: es_dense_* (existing) vs es_dense_wide_* (tiled f32 MFMA), the same buffers, "
             f"alternated sample by sample; {args.rounds} samples x {args.iters} back-to-back calls, device events; "
             f"us per call", f"{'n':>4} {'layer':<11}{'K':>5}{'N':>5} {'pass':<4}"
             f"{'existing med':>13}{'p10':>8}{'p90':>8}{'wide med':>10}{'p10':>8}{'p90':>8}  wide p90 < existing p10"]
    wins = {}
    for n, layer, K, N, act, keep, want_dx in cases():
        r = lambda *sh: torch.randn(*sh, generator=g).cuda()  # noqa: E731
        X, W, b, dY, Y = r(n, K), r(N, K) * K ** -0.5, r(N), r(n, N), torch.empty(n, N, device="cuda")
        kp = (torch.rand(n, N, generator=g) >= 0.2).to(torch.uint8).cuda() if keep else None
        dX, dW, db = torch.empty(n, K, device="cuda"), torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
        ws = torch.empty(max(lib.es_dense_bwd_workspace(n, N), lib.es_dense_wide_bwd_workspace(n, K, N, 1)), device="cuda")
        dxp = ptr(dX) if want_dx else None
        fns = {}
        for fam in ("es_dense", "es_dense_wide"):
            fns[(fam, "fwd")] = lambda fam=fam: call(fam + "_fwd", ptr(X), K, ptr(W), ptr(b), ptr(Y), N, n, K, N, act, 0.1,
                                                     ptr(kp), 1.25, s)
            fns[(fam, "bwd")] = lambda fam=fam: call(fam + "_bwd", ptr(dY), N, ptr(Y), N, act, 0.1, ptr(kp), 1.25, ptr(X),
                                                     K, ptr(W), dxp, K, 0, ptr(dW), ptr(db), n, K, N, ptr(ws), s)
        for _ in range(args.warmup):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.iters * 1e3)
        for ps in ("fwd", "bwd"):
            e, w = times[("es_dense", ps)], times[("es_dense_wide", ps)]
            win = _pct(w, 0.9) < _pct(e, 0.1)
            wins.setdefault(layer, []).append(win)
            lines.append(f"{n:>4} {layer:<11}{K:>5}{N:>5} {ps + ('' if want_dx or ps == 'fwd' else '*'):<4}"
                         f"{_pct(e, 0.5):>13.1f}{_pct(e, 0.1):>8.1f}{_pct(e, 0.9):>8.1f}"
                         f"{_pct(w, 0.5):>10.1f}{_pct(w, 0.1):>8.1f}{_pct(w, 0.9):>8.1f}  {'yes' if win else 'no'}")
    lines.append("(* backward without dX: EZBM stage 2)")
    for layer, w in wins.items():
        lines.append(f"{layer}: wide p90 below the existing p10 in {sum(w)} of {len(w)} rows -> "
                     f"{'wide family' if all(w) else 'stays on the existing kernels'}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
