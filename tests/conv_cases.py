"""Exact-integer cases for the convolution kernels (csrc/conv_bf16.hip and the conv part of csrc/conv.hip).

With operands in {-2..2} every product and every fp32 partial sum of a convolution, of its data gradient and of its
weight gradient is an integer far below 2^24, so the result does not depend on the summation order: ONE CPU
reference anchors every kernel path, column tile, ring depth, split count and map type with torch.equal, and a bf16
output map is that integer rounded once.  Shared by test_conv_cases_cpu.py -- which holds `reference` to an explicit
loop over taps, the magnitudes to 2^24 and `paths` to the kernel classes the cases are there to reach -- and by
test_gpu_conv_exact.py, which holds the kernels to `reference`.  Torch only; everything is built on the CPU.

Layout as the kernels': maps NHWC (x [N, H, W, Cin], y / dy [N, Ho, Wo, Cout]), weights [Cout, Cin, kh, kw].
"""
import torch
import torch.nn.functional as F

# (N, H, W, Cin, Cout, kh, kw, s, p): the smallest shape that still reaches what the comment names
CASES = {
    # M = 189: two row blocks, the second partial; ring forward (Cout <= Cin); dw tile 64 x 128, partial last K tile
    "A": (3, 9, 7, 64, 64, 3, 3, 1, 1),
    # rectangular 3 x 2 kernel, stride phases of unequal size (11 rows), Cout = 96: partial second 64-column tile,
    # Wo = 4: the branchy dw walk
    "B": (2, 11, 6, 32, 96, 3, 2, 2, 1),
    # the ResNet downsample: three of the four dx phases have no tap; the 128-column tile under es_set_conv_small(0)
    "C": (2, 5, 12, 128, 128, 1, 1, 2, 0),
    # M = 300, 72 K steps, deep ring, sums up to ~450 so that bf16 stores really round; dw tile 128 x 128
    "D": (5, 6, 10, 256, 128, 3, 3, 1, 1),
    # M = 128 exactly; dw tile 64 x 64
    "E": (2, 8, 8, 64, 64, 1, 1, 1, 0),
    # dw tile 128 x 64 (K = 32); a widening forward: the staged kernel runs even on bf16 maps
    "F": (2, 4, 20, 32, 128, 1, 1, 1, 0),
    # Wo = 3, Ho = 12: the branch-free advance32 with a carry in w and in h on every step; Cout = 32: half-empty tile
    "G": (4, 12, 3, 64, 32, 3, 3, 1, 1),
    # 2 x 2 maps (ResNet-50's last stage at 64^2): a 32-pixel step spans 8 images, most taps are padding
    "H": (7, 2, 2, 64, 64, 3, 3, 1, 1),
    # the patch conv: 16 dx phases of one tap each (nk = 2); M = 16
    "I": (2, 16, 8, 32, 64, 4, 4, 4, 0),
    # large rectangular kernel (35 taps), pad 3, odd sizes in both dimensions
    "J": (1, 15, 13, 32, 32, 7, 5, 2, 3),
    # (H + 2p - k) % s = 1: the last row and column of x are never read, their dx is exactly 0 (or the prior value)
    "K": (2, 10, 10, 64, 64, 3, 3, 2, 0),
    # Wo = 40 > 32: 32 / Wo = 0, a step never leaves the row pair
    "L": (2, 3, 40, 32, 64, 3, 3, 1, 1),
    # nk = 1 in the forward and the data gradient: a ring prologue shorter than the stage count; M = 135
    "M": (3, 5, 9, 32, 32, 1, 1, 1, 0),
}
# the cases that also run inside strided views with poisoned gaps and guard bands
VIEW_CASES = ("A", "B", "G", "M")
# csrc/conv.hip's fp32 kernels: these bf16 cases, and three with channel counts off every vector width (each
# forward / dx row tile -- Cout or Cin <= 16, <= 32, above -- and each dw tile on a non-square map)
FP32_CASES = {k: CASES[k] for k in ("B", "G", "H", "J", "K")}
FP32_CASES.update({
    "P": (3, 7, 10, 5, 7, 3, 2, 2, 1),     # 256 x 16 forward rows, scalar loads, dw tile 16 x 64
    "Q": (2, 9, 4, 40, 33, 3, 3, 1, 1),    # 64 x 64 rows with a 1-channel second column tile, dw tile 64 x 64
    "R": (2, 6, 14, 16, 64, 1, 1, 1, 0),   # dx rows 256 x 16, dw tile 64 x 16 (K = 16)
})
# the 3 -> 64 channel stem: Wo = 23 is a partial 64-pixel row segment, and H != W
STEM_CASE = (2, 30, 46, 3, 64, 7, 7, 2, 3)

EXACT = 1 << 24  # integers below this are fp32 numbers
NT_BM = 128      # output pixels per forward workgroup, and per BatchNorm-partials block
TWO_GIB = 0x7fff0000


def out_hw(case):
    N, H, W, Cin, Cout, kh, kw, s, p = case
    return (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1


def _seed(case):
    return sum((i + 1) * 131 ** i * v for i, v in enumerate(case)) % (1 << 31)


def operands(case, seed=None):
    """int64 x, w, dy, bias, prior_y, prior_dx, prior_dw in {-2..2}, and BatchNorm-in parameters that keep
    relu((x - mean) * rstd * gamma + beta) an integer (at most 13) in any evaluation order: mean, beta in {-1, 0, 1},
    rstd, gamma in {1, 2}."""
    N, H, W, Cin, Cout, kh, kw, s, p = case
    Ho, Wo = out_hw(case)
    g = torch.Generator().manual_seed(_seed(case) if seed is None else seed)

    def ints(*shape, lo=-2, hi=2):
        return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)
    return {"x": ints(N, H, W, Cin), "w": ints(Cout, Cin, kh, kw), "dy": ints(N, Ho, Wo, Cout), "bias": ints(Cout),
            "prior_y": ints(N, Ho, Wo, Cout), "prior_dx": ints(N, H, W, Cin), "prior_dw": ints(Cout, Cin, kh, kw),
            "mean": ints(Cin, lo=-1, hi=1), "rstd": ints(Cin, lo=1, hi=2), "gamma": ints(Cin, lo=1, hi=2),
            "beta": ints(Cin, lo=-1, hi=1)}


def bn_relu(ops):
    """The BatchNorm-in conv's operand: relu((x - mean) * rstd * gamma + beta), int64."""
    return ((ops["x"] - ops["mean"]) * ops["rstd"] * ops["gamma"] + ops["beta"]).clamp(min=0)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def bn_partials(y):
    """es_conv2d_fwd_bf16_bnstats' layout: per block of 128 consecutive output pixels in (n, ho, wo) order
    [sum | M2] of every channel, M2 the block-centred sum of squares.  y: [N, Ho, Wo, Cout] float64 (bias included)."""
    rows = y.reshape(-1, y.shape[-1])
    out = []
    for b in range(0, rows.shape[0], NT_BM):
        blk = rows[b:b + NT_BM]
        out.append(torch.stack([blk.sum(0), ((blk - blk.mean(0)) ** 2).sum(0)]))
    return torch.stack(out)  # [blocks, 2, Cout]


def reference(case, ops):
    """Everything the GPU tests compare against, in float64 on the CPU (torch's convolution and its two gradient
    functions), NHWC: y = conv(x, w) + bias, y_acc = prior_y + conv(x, w), y_bn = conv(bn_relu(x), w), dx / dx_acc
    (plain and added to prior_dx), dw / dw_bn (of x and of the BatchNorm-ed input) with dw_acc = prior_dw + dw, and
    partials = bn_partials(y)."""
    N, H, W, Cin, Cout, kh, kw, s, p = case
    d = {k: v.double() for k, v in ops.items()}
    x, w, dy = _nchw(d["x"]), d["w"], _nchw(d["dy"])
    xb = _nchw(bn_relu(ops).double())
    conv = F.conv2d(x, w, stride=s, padding=p)
    r = {"y": _nhwc(conv) + d["bias"], "y_acc": _nhwc(conv) + d["prior_y"],
         "y_bn": _nhwc(F.conv2d(xb, w, stride=s, padding=p))}
    r["dx"] = _nhwc(torch.nn.grad.conv2d_input(x.shape, w, dy, stride=s, padding=p))
    r["dx_acc"] = r["dx"] + d["prior_dx"]
    r["dw"] = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=s, padding=p)
    r["dw_acc"] = r["dw"] + d["prior_dw"]
    r["dw_bn"] = torch.nn.grad.conv2d_weight(xb, w.shape, dy, stride=s, padding=p)
    r["partials"] = bn_partials(r["y"])
    return r


def naive_conv(case, ops, x=None):
    """y (without bias), dx and dw by an explicit loop over the taps, in int64, from slicing and einsum alone -- no
    F.conv2d, so that `reference` is not taken on trust for rectangular or strided geometry.  x: another input map
    (the BatchNorm-ed one) in place of ops["x"]."""
    N, H, W, Cin, Cout, kh, kw, s, p = case
    Ho, Wo = out_hw(case)
    x = ops["x"] if x is None else x
    w, dy = ops["w"], ops["dy"]
    xp = torch.zeros(N, H + 2 * p, W + 2 * p, Cin, dtype=torch.int64)
    xp[:, p:p + H, p:p + W] = x
    dxp = torch.zeros_like(xp)
    y = torch.zeros(N, Ho, Wo, Cout, dtype=torch.int64)
    dw = torch.zeros(Cout, Cin, kh, kw, dtype=torch.int64)
    for ky in range(kh):
        for kx in range(kw):
            # the input pixels tap (ky, kx) pairs with the output pixels: (ho s - p + ky, wo s - p + kx)
            rows, cols = slice(ky, ky + (Ho - 1) * s + 1, s), slice(kx, kx + (Wo - 1) * s + 1, s)
            tap = w[:, :, ky, kx]  # [Cout, Cin]
            y += torch.einsum("nhwc,oc->nhwo", xp[:, rows, cols], tap)
            dxp[:, rows, cols] += torch.einsum("nhwo,oc->nhwc", dy, tap)
            dw[:, :, ky, kx] = torch.einsum("nhwo,nhwc->oc", dy, xp[:, rows, cols])
    return {"y": y, "dx": dxp[:, p:p + H, p:p + W].contiguous(), "dw": dw}


def dx_phases(case):
    """The data gradient's stride phases (py, px) as convb_nt_kernel / convb_nt_ring_kernel decompose them: the x
    pixels (hq s + py, wq s + px), Hm x Wm of them per image, reached by twy x twx taps (ky = ky0 + s kyq)."""
    N, H, W, Cin, Cout, kh, kw, s, p = case
    out = []
    for py in range(s):
        for px in range(s):
            Hm, Wm = (H - py + s - 1) // s, (W - px + s - 1) // s
            ky0, kx0 = (py + p) % s, (px + p) % s
            twy = (kh - ky0 + s - 1) // s if kh > ky0 else 0
            twx = (kw - kx0 + s - 1) // s if kw > kx0 else 0
            out.append({"py": py, "px": px, "Hm": Hm, "Wm": Wm, "twy": twy, "twx": twx, "M": N * Hm * Wm,
                        "nk": twy * twx * (Cout // 32)})
    return out


def dw_tile(Cout, K):
    return (64 if Cout <= 64 else 128, 64 if K <= 64 else 128)


def paths(case, flags, ring, dw_buf, small):
    """The kernel class each bf16 entry point takes for `case` under map flags `flags` (bit 0: the gathered / input
    map is bf16) and the knobs es_set_conv_ring(ring), es_set_conv_dw_buf(dw_buf), es_set_conv_small(small).

    A restatement of the host dispatch in csrc/conv_bf16.hip -- conv_fwd_bf16_impl, es_conv2d_bwd_data_bf16_ex,
    launch_ring, launch_nt / nt_extents, launch_dw and dw_tile -- and it must be updated with them: the coverage
    assertions of test_conv_cases_cpu.py are only as true as this function.

    Returns {"fwd", "fwd_bnin", "dx", "dw"}: forward and data gradient as {"kernel": "ring" | "staged-bufl" |
    "staged-branchy", "bn": 64 | 128 (column tile), "M", "nk"} (dx: M of the largest phase, plus "phases" =
    dx_phases(case) and "olin"), dw as {"tile": (b1, b2), "loads": "buf" | "branchy", "M", "K"}."""
    N, H, W, Cin, Cout, kh, kw, s, p = case
    Ho, Wo = out_hw(case)
    in16 = bool(flags & 1)

    def small_grid(wgs):
        return wgs < small

    def nt_kernel(src_elems, C, Ncol, dx, bnin):
        # launch_ring: a bf16 gathered map and weights under 2 GiB, no input BatchNorm, no widening forward
        src_bytes, w_bytes = src_elems * 2, Ncol * kh * kw * C * 2
        if ring and in16 and not bnin and src_bytes < TWO_GIB and w_bytes < TWO_GIB and (dx or Ncol <= C):
            return "ring"
        # launch_nt / nt_extents: branch-free buffer loads when the knob is on and both operands are under 2 GiB
        sb = src_elems * (2 if in16 else 4)
        return "staged-bufl" if dw_buf and sb < TWO_GIB and w_bytes < TWO_GIB else "staged-branchy"

    M = N * Ho * Wo
    g128 = ((M + 127) // 128) * (Cout // 128)
    fwd_bn = 128 if Cout % 128 == 0 and not small_grid(g128) else 64
    fwd = {"bn": fwd_bn, "M": M, "nk": kh * kw * (Cin // 32), "olin": True}
    r = {"fwd": dict(fwd, kernel=nt_kernel(N * H * W * Cin, Cin, Cout, False, False)),
         "fwd_bnin": dict(fwd, kernel=nt_kernel(N * H * W * Cin, Cin, Cout, False, True))}
    Mq = N * ((H + s - 1) // s) * ((W + s - 1) // s)  # the largest phase
    dx128 = Cin % 128 == 0 and not small_grid(((Mq + 127) // 128) * (Cin // 128) * s * s)
    ph = dx_phases(case)
    r["dx"] = {"kernel": nt_kernel(N * Ho * Wo * Cout, Cout, Cin, True, False), "bn": 128 if dx128 else 64, "M": Mq,
               "nk": max(q["nk"] for q in ph), "phases": ph, "olin": s == 1}
    K = Cin * kh * kw
    r["dw"] = {"tile": dw_tile(Cout, K), "M": M, "K": K,
               # launch_dw: the select-only pixel walk needs one wrap per dimension per 32-pixel step at most
               "loads": "buf" if dw_buf and 32 // Wo + 1 < Ho else "branchy"}
    return r


# the knob grid of test_gpu_conv_exact.py: (es_set_conv_ring, es_set_conv_dw_buf) x es_set_conv_small
KNOBS = [(ring, dw_buf, small) for ring, dw_buf in ((0, 0), (0, 1), (3, 1), (4, 1)) for small in (0, 1 << 20)]
DEFAULT_KNOBS = {"ring": 3, "dw_buf": 1, "small": 128, "dw_target": 512}
