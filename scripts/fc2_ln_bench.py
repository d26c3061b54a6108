"""es_gemm_nt_ln (fc2 + residual + the next block's norm1 in one launch) vs es_gemm_nt(EPI_F32_RESID) +
es_layernorm_fwd at the F1 train / weak row counts and a rank's share at N = 2 / 4 / 8 (K = 1536): bit-identity and
interleaved timings (µs, the median of 5 groups of 20 launches each way), for both rings of the fused kernel.
  python scripts/fc2_ln_bench.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endoscopy-image-classification_amd"))
import torch  # noqa: E402

from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402

D, K, EPS = 384, 1536, 1e-6


def main():
    lib = _lib.load()
    s = _lib.stream()
    for name, M in (("f1_train", 512 * 197), ("f1_weak", 448 * 197), ("n2_train", 256 * 197), ("n2_weak", 224 * 197),
                    ("n4_train", 128 * 197), ("n4_weak", 112 * 197), ("n8_train", 64 * 197), ("n8_weak", 56 * 197)):
        torch.manual_seed(0)
        A = torch.randn((M + 255) // 256 * 256, K, device="cuda").bfloat16()
        W = (torch.randn(D, K, device="cuda") * 0.05).bfloat16()
        bias = torch.randn(D, device="cuda") * 0.1
        xmid = torch.randn(M, D, device="cuda")
        g, b = 1 + 0.1 * torch.randn(D, device="cuda"), 0.1 * torch.randn(D, device="cuda")
        outs = [(torch.empty(M, D, device="cuda"), torch.empty(M, D, dtype=torch.bfloat16, device="cuda"),
                 torch.empty(M, device="cuda"), torch.empty(M, device="cuda")) for _ in range(3)]

        def gemm(o):
            call("es_gemm_nt", 2, ptr(A), K, ptr(W), K, ptr(bias), ptr(o[0]), D, None, ptr(xmid), D, M, D, K, 0, s)

        def two(o):
            gemm(o)
            call("es_layernorm_fwd", ptr(o[0]), D, ptr(g), ptr(b), ptr(o[1]), D, ptr(o[2]), ptr(o[3]), M, D, EPS, s)

        def one(o):
            call("es_gemm_nt_ln", ptr(A), K, ptr(W), K, ptr(bias), ptr(o[0]), D, ptr(xmid), D, ptr(g), ptr(b),
                 ptr(o[1]), D, ptr(o[2]), ptr(o[3]), M, D, K, EPS, s)

        def ring(v):
            def f(o):
                lib.endossl_nt_ln_ring(v)
                one(o)
            return f

        two(outs[0])
        ring(0)(outs[1])
        ring(1)(outs[2])
        torch.cuda.synchronize()
        same = all(torch.equal(a, c) and torch.equal(a, d) for a, c, d in zip(*outs))
        runs = (("gemm", gemm), ("two", two), ("one_bk64x2", ring(0)), ("one_bk32x3", ring(1)))
        t = {k: [] for k, _ in runs}
        it = 20
        for _ in range(5):
            for k, f in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(it):
                    f(outs[0])
                e1.record()
                torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) / it * 1e3)
        lib.endossl_nt_ln_ring(0)
        print(name, json.dumps({"M": M, "bit_identical": same, **{k + "_us": round(sorted(v)[2], 1) for k, v in t.items()}}),
              flush=True)


if __name__ == "__main__":
    main()
