"""csrc/densenet.hip on the MI355X, exactly: every kernel against the dense kernel it generalises (torch.equal on
contiguous copies -- they share their reduction code, csrc/bn_rows.h) or against a float64 CPU reference on
integer-valued operands (the padded convs, in the style of tests/conv_cases.py).  Shapes are the smallest that leave
a prefix inside a wider buffer, a 16 (mod 32) channel count, and more than one 128-pixel block."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402

DEV = "cuda"
EPS = 1e-5
POISON = 768.0  # a bf16 number


def _lib():
    from endossl import _lib
    return _lib


def call(name, *args):
    return _lib().call(name, *args)


def ptr(t, elems=0):
    return None if t is None else t.data_ptr() + elems * t.element_size()


def S():
    return _lib().stream()


def ws_for(rows, C):
    return torch.empty(_lib().load().es_chan_workspace(rows, C), device=DEV)


def fl(dt):
    return 1 if dt == torch.bfloat16 else 0


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def bn_arrays(C, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(C, generator=g) * 0.2).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV),
            (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.3).to(DEV))  # mean rstd gamma beta


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,C,ld", [(30, 144, 208), (192, 96, 160)])
def test_bn_bwd_recompute_ld_equals_the_dense_kernel(rows, C, ld, dt):
    g = torch.Generator().manual_seed(rows + C)
    xb = torch.randn(rows, ld, generator=g).to(dt).to(DEV)
    ldy = C + 16
    dyb = torch.randn(rows, ldy, generator=g).to(dt).to(DEV)
    mean, rstd, gam, bet = bn_arrays(C, 5)
    f = fl(dt)
    xc, dyc = xb[:, :C].contiguous(), dyb[:, :C].contiguous()
    dxc = torch.empty_like(xc)
    dg0, db0 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    call("es_bn2d_bwd_recompute_ex", ptr(xc), ptr(dyc), rows, C, ptr(gam), ptr(bet), ptr(mean), ptr(rstd), ptr(dxc),
         ptr(dg0), ptr(db0), 0, ptr(ws_for(rows, C)), f, S())

    def run(flags, dx):
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        call("es_bn2d_bwd_recompute_ld_ex", ptr(xb), ld, ptr(dyb), ldy, rows, C, ptr(gam), ptr(bet), ptr(mean),
             ptr(rstd), ptr(dx), ld, ptr(dg), ptr(db), 0, ptr(ws_for(rows, C)), flags, S())
        torch.cuda.synchronize()
        assert torch.equal(dg, dg0) and torch.equal(db, db0)
        return dx

    # dx in the maps' type, overwritten: the dense kernel's bits; columns beyond the prefix untouched
    poison = torch.full((rows, ld), POISON, dtype=dt, device=DEV)
    dx = run(f, poison.clone())
    assert torch.equal(dx[:, :C], dxc)
    assert same_bytes(dx[:, C:], poison[:, C:])
    # fp32 dx whatever the maps are: the unrounded value, which rounds to the dense kernel's
    p32 = torch.full((rows, ld), POISON, device=DEV)
    dxf = run(f | 2, p32.clone())
    assert torch.equal(dxf[:, :C].to(dt), dxc) and same_bytes(dxf[:, C:], p32[:, C:])
    if dt == torch.float32:
        assert torch.equal(dxf[:, :C], dxc)
    # accumulating into fp32 prior contents: prior + dx, one fp32 add
    prior = torch.randn(rows, ld, generator=g).to(DEV)
    acc = run(f | 2 | 4, prior.clone())
    assert torch.equal(acc[:, :C], prior[:, :C] + dxf[:, :C])
    assert same_bytes(acc[:, C:], prior[:, C:])
    assert bool(torch.isfinite(dxc.float()).all()) and dxc.float().abs().max().item() > 0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_stats_ld_and_apply_ld_equal_the_dense_batchnorm(dt):
    rows, C, ld, off = 192, 48, 160, 96
    g = torch.Generator().manual_seed(11)
    xb = (torch.randn(rows, ld, generator=g) * 1.5 + 0.3).to(dt).to(DEV)
    xc = xb[:, off:off + C].contiguous()
    _, _, gam, bet = bn_arrays(C, 6)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    yc, mean0, rstd0 = torch.empty_like(xc), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    call("es_bn2d_fwd_ex", ptr(xc), rows, C, ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(nbt), 0.1, EPS, 1, None, 1, ptr(yc),
         ptr(mean0), ptr(rstd0), ptr(ws_for(rows, C)), fl(dt), S())
    arr = torch.full((3, ld), POISON, device=DEV)
    call("es_bn2d_stats_ld_ex", ptr(xb, off), rows, C, ld, EPS, ptr(arr[0], off), ptr(arr[1], off), ptr(arr[2], off),
         ptr(ws_for(rows, C)), fl(dt), S())
    torch.cuda.synchronize()
    assert torch.equal(arr[0, off:off + C], mean0) and torch.equal(arr[1, off:off + C], rstd0)
    assert torch.all(arr[:, :off] == POISON) and torch.all(arr[:, off + C:] == POISON)
    m2 = ((xc.double() - xc.double().mean(0)) ** 2).sum(0)
    assert torch.allclose(arr[2, off:off + C].double(), m2, rtol=1e-5)  # fp32 sums of 192 squares
    # the apply pass between strided views: es_bn2d_fwd_ex's y
    yb = torch.full((rows, ld), POISON, dtype=dt, device=DEV)
    call("es_bn2d_apply_ld_ex", ptr(xb, off), ld, rows, C, ptr(arr[0], off), ptr(arr[1], off), ptr(gam), ptr(bet), 1,
         ptr(yb, 16), ld, fl(dt) * 3, S())
    torch.cuda.synchronize()
    assert torch.equal(yb[:, 16:16 + C], yc)
    assert torch.all(yb[:, :16].float() == POISON) and torch.all(yb[:, 16 + C:].float() == POISON)
    # eval mode: running statistics -> arrays (zero-padded) -> the same apply
    rv2 = (torch.rand(C, generator=g) + 0.5).to(DEV)
    ye = torch.empty_like(xc)
    call("es_bn2d_fwd_ex", ptr(xc), rows, C, ptr(gam), ptr(bet), ptr(mean0), ptr(rv2), None, 0.1, EPS, 0, None, 1, ptr(ye),
         None, None, None, fl(dt), S())
    em, er = torch.full((64,), POISON, device=DEV), torch.full((64,), POISON, device=DEV)
    call("es_bn2d_eval_stats", ptr(mean0), ptr(rv2), C, 64, EPS, ptr(em), ptr(er), S())
    y2 = torch.empty_like(xc)
    call("es_bn2d_apply_ld_ex", ptr(xc), C, rows, C, ptr(em), ptr(er), ptr(gam), ptr(bet), 1, ptr(y2), C, fl(dt) * 3, S())
    torch.cuda.synchronize()
    assert torch.equal(y2, ye) and torch.equal(em[:C], mean0) and torch.all(em[C:] == 0) and torch.all(er[C:] == 0)


@pytest.mark.parametrize("rows", [192, 128 * 65 + 7])  # one and a half blocks; more than 64 blocks (two levels)
def test_stats_from_partials_equals_bn2d_fwd_partials(rows):
    C, PC, off = 48, 64, 16
    g = torch.Generator().manual_seed(rows)
    y = (torch.randn(rows, PC, generator=g) * 2 + 0.5)
    part = cc.bn_partials(y.double()).float().to(DEV)  # [blocks, 2, PC]
    y = y.to(DEV)
    gam, bet = torch.ones(PC, device=DEV), torch.zeros(PC, device=DEV)
    rm, rv = torch.zeros(PC, device=DEV), torch.ones(PC, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    mean0, rstd0 = torch.empty(PC, device=DEV), torch.empty(PC, device=DEV)
    call("es_bn2d_fwd_partials_ex", ptr(y), rows, PC, ptr(part.clone()), ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(nbt),
         0.1, EPS, None, 1, None, ptr(mean0), ptr(rstd0), 0, S())
    arr = torch.full((3, 80), POISON, device=DEV)
    call("es_bn2d_stats_from_partials", ptr(part.clone()), rows, C, PC, EPS, ptr(arr[0], off), ptr(arr[1], off),
         ptr(arr[2], off), S())
    torch.cuda.synchronize()
    assert torch.equal(arr[0, off:off + C], mean0[:C]) and torch.equal(arr[1, off:off + C], rstd0[:C])
    assert torch.all(arr[:, :off] == POISON) and torch.all(arr[:, off + C:] == POISON)
    m2 = ((y[:, :C].double() - y[:, :C].double().mean(0)) ** 2).sum(0)  # the centred square sum (fp32 combination)
    assert torch.allclose(arr[2, off:off + C].double(), m2, rtol=1e-4)


def _run_table(entries, device):
    raw = b"".join(bytes(e) for e in entries)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def test_running_multi_equals_the_single_batchnorm_update():
    """3 BatchNorms of widths 96 / 144 / 192 over one statistics array (a block's norm1s): each one's buffers after
    the table-driven launch equal what the single-BatchNorm kernel leaves from the same partials."""
    from endossl.densenet import _RunEntry
    rows, C = 192, 192
    g = torch.Generator().manual_seed(21)
    y = torch.randn(rows, C, generator=g) + 0.2
    part = cc.bn_partials(y.double()).float().to(DEV)  # [2, 2, 192]
    y = y.to(DEV)
    arr = torch.zeros(3, C, device=DEV)
    call("es_bn2d_stats_from_partials", ptr(part.clone()), rows, C, C, EPS, ptr(arr[0]), ptr(arr[1]), ptr(arr[2]), S())
    widths, bufs, ents, want = (96, 144, 192), [], [], []
    for w in widths:
        rm, rv = torch.randn(w, generator=g).to(DEV), (torch.rand(w, generator=g) + 0.5).to(DEV)
        nbt = torch.full((), 3, dtype=torch.int64, device=DEV)
        ref = (rm.clone(), rv.clone(), nbt.clone())
        gam, bet = torch.ones(w, device=DEV), torch.zeros(w, device=DEV)
        mean, rstd = torch.empty(w, device=DEV), torch.empty(w, device=DEV)
        call("es_bn2d_fwd_partials_ex", ptr(y), rows, w, ptr(part[:, :, :w].contiguous()), ptr(gam), ptr(bet), ptr(ref[0]),
             ptr(ref[1]), ptr(ref[2]), 0.1, EPS, None, 1, None, ptr(mean), ptr(rstd), 0, S())
        assert torch.equal(mean, arr[0, :w]) and torch.equal(rstd, arr[1, :w])
        bufs.append((rm, rv, nbt))
        want.append(ref)
        ents.append(_RunEntry(rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), w, 0))
    assert _lib().load().es_bn_running_entry_size() == ctypes.sizeof(_RunEntry)
    tab = _run_table(ents, DEV)
    call("es_bn2d_running_multi", ptr(tab), 3, 192, ptr(arr[0]), ptr(arr[2]), rows, 0.1, S())
    torch.cuda.synchronize()
    for (rm, rv, nbt), (rm0, rv0, nbt0), w in zip(bufs, want, widths):
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0), w
        assert int(nbt) == int(nbt0) == 4
        assert not torch.equal(rm, torch.zeros_like(rm))


@pytest.mark.parametrize("fin,fout", [(0, 0), (1, 1), (0, 1)], ids=["f32", "bf16", "f32-to-bf16"])
def test_strided_pool_equals_the_dense_pool(fin, fout):
    N, H, W, C, ld, off = 2, 6, 8, 48, 80, 16
    tin, tout = (torch.bfloat16 if fin else torch.float32), (torch.bfloat16 if fout else torch.float32)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(N, H, W, C, generator=g).to(tin).to(DEV)
    yc = torch.empty(N, H // 2, W // 2, C, dtype=tout, device=DEV)
    call("es_avgpool2d_fwd_ex", ptr(x), N, H, W, C, 2, ptr(yc), fin | (fout << 1), S())
    yb = torch.full((N, H // 2, W // 2, ld), POISON, dtype=tout, device=DEV)
    call("es_avgpool2_ld_fwd_ex", ptr(x), N, H, W, C, ptr(yb, off), ld, fin | (fout << 1), S())
    torch.cuda.synchronize()
    assert torch.equal(yb[..., off:off + C], yc)
    assert torch.all(yb[..., :off].float() == POISON) and torch.all(yb[..., off + C:].float() == POISON)
    # backward: the gradient source is the strided view
    dyb = torch.randn(N, H // 2, W // 2, ld, generator=g).to(tin).to(DEV)
    dyc = dyb[..., off:off + C].contiguous()
    dxc = torch.empty(N, H, W, C, dtype=tout, device=DEV)
    call("es_avgpool2d_bwd_ex", ptr(dyc), N, H, W, C, 2, ptr(dxc), 0, fin | (fout << 1), S())
    dx = torch.empty(N, H, W, C, dtype=tout, device=DEV)
    call("es_avgpool2_ld_bwd_ex", ptr(dyb, off), ld, N, H, W, C, ptr(dx), fin | (fout << 1), S())
    torch.cuda.synchronize()
    assert torch.equal(dx, dxc) and dx.float().abs().max().item() > 0


def test_pack_pad_equals_the_pack_of_a_zero_padded_weight():
    Cout, Cin, k, Cop, Cip = 48, 144, 3, 64, 160
    g = torch.Generator().manual_seed(41)
    w = torch.randn(Cout, Cin, k, k, generator=g).to(DEV)
    wpad = torch.zeros(Cop, Cip, k, k, device=DEV)
    wpad[:Cout, :Cin] = w
    n = Cop * Cip * k * k
    wp0, wt0 = (torch.empty(n, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    call("es_conv2d_pack_bf16", ptr(wpad), Cop, Cip, k, k, ptr(wp0), ptr(wt0), S())
    wp, wt = (torch.full((n,), POISON, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    call("es_conv2d_pack_bf16_pad", ptr(w), Cout, Cin, k, k, Cop, Cip, ptr(wp), ptr(wt), S())
    torch.cuda.synchronize()
    assert torch.equal(wp, wp0) and torch.equal(wt, wt0)
    lib = _lib().load()
    assert lib.es_conv2d_pack_bf16_pad(ptr(w), Cout, Cin, k, k, 40, Cip, ptr(wp), ptr(wt), None) == -1  # Cout_p < Cout
    assert lib.es_conv2d_pack_bf16_pad(ptr(w), Cout, Cin, k, k, Cop, 148, ptr(wp), ptr(wt), None) == -1  # % 8
    assert lib.es_conv2d_pack_bf16_pad(None, Cout, Cin, k, k, Cop, Cip, ptr(wp), ptr(wt), None) == -2


def test_padded_convs_are_exact_and_unpad_into_the_flat_gradient():
    """A dense layer's two convs at the 48-channel granularity, on integer operands against float64: conv1 (1 x 1,
    144 -> 192, inputs padded to 160) gathers relu(bn(.)) from the prefix of a 208-wide buffer whose next 16 channels
    hold real data; conv2 (3 x 3, 192 -> 48, outputs padded to 64) writes the slice [96, 144) of a 208-wide buffer,
    zeros over [144, 160) and nothing else.  Both weight gradients land padded in a scratch arena; one
    es_dw_unpad_multi writes the true tensors into a flat gradient."""
    from endossl.densenet import _UnpadEntry
    lib = _lib().load()
    N, H, W, ld = 2, 8, 12, 208
    rows = N * H * W  # 192: one and a half 128-pixel blocks
    c1 = (N, H, W, 144, 192, 1, 1, 1, 0)
    c2 = (N, H, W, 192, 48, 3, 3, 1, 1)
    o1, o2 = cc.operands(c1), cc.operands(c2)
    r1, r2 = cc.reference(c1, o1), cc.reference(c2, o2)
    g = torch.Generator().manual_seed(51)
    flat_grad = torch.full((64 + 192 * 144 + 64 + 48 * 192 * 9 + 64,), POISON, device=DEV)
    dst1, dst2 = flat_grad[64:64 + 192 * 144], flat_grad[128 + 192 * 144:128 + 192 * 144 + 48 * 192 * 9]
    arena = torch.full((192 * 160 + 64 * 192 * 9,), POISON, device=DEV)
    s1, s2 = arena[:192 * 160], arena[192 * 160:]

    # ---- conv1: Cin 144 padded to 160, reading the prefix of the 208-wide bf16 buffer
    buf = torch.randint(-2, 3, (N, H, W, ld), generator=g).to(torch.bfloat16)
    buf[..., :144] = o1["x"].to(torch.bfloat16)
    buf = buf.to(DEV)

    def padded(v, fill):  # per-channel arrays over the 160 gathered channels: gamma = beta = 0 in the padding
        out = torch.full((160,), float(fill))
        out[:144] = v.float()
        return out.to(DEV)
    mean, rstd = padded(o1["mean"], 1.0), padded(o1["rstd"], 2.0)
    gam, bet = padded(o1["gamma"], 0.0), padded(o1["beta"], 0.0)
    w1 = o1["w"].float().to(DEV)
    wp1, wt1 = (torch.empty(192 * 160, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    call("es_conv2d_pack_bf16_pad", ptr(w1), 192, 144, 1, 1, 192, 160, ptr(wp1), ptr(wt1), S())
    y1 = torch.empty(N, H, W, 192, device=DEV)
    call("es_conv2d_fwd_bf16_bnin_ex", ptr(buf), N, H, W, 160, H * W * ld, W * ld, ld, 1, ptr(wp1), None, 192, 1, 1, 1, 0,
         ptr(y1), H * W * 192, W * 192, 192, 0, None, 1, ptr(mean), ptr(rstd), ptr(gam), ptr(bet), S())
    dy1 = o1["dy"].float().to(DEV)
    ws = torch.empty(lib.es_conv2d_bwd_weight_bf16_workspace(rows, 192, 160, 1, 1, 0), device=DEV)
    call("es_conv2d_bwd_weight_bf16_bnin_ex", ptr(buf), N, H, W, 160, H * W * ld, W * ld, ld, 1, ptr(dy1), H * W * 192,
         W * 192, 192, 192, 1, 1, 1, 0, 0, ptr(ws), ptr(s1), 0, 1, ptr(mean), ptr(rstd), ptr(gam), ptr(bet), S())
    da = torch.empty(N, H, W, 160, device=DEV)
    call("es_conv2d_bwd_data_bf16_ex", ptr(dy1), H * W * 192, W * 192, 192, ptr(wt1), N, H, W, 160, 192, 1, 1, 1, 0,
         ptr(da), H * W * 160, W * 160, 160, 1, 0, 0, S())

    # ---- conv2: Cout 48 padded to 64, writing the slice [96, 144) of an fp32 208-wide buffer
    x2 = o2["x"].to(torch.bfloat16).to(DEV)
    m2_, r2_, g2_, b2_ = (o2[k].float().to(DEV) for k in ("mean", "rstd", "gamma", "beta"))
    w2 = o2["w"].float().to(DEV)
    wp2, wt2 = (torch.empty(64 * 192 * 9, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    call("es_conv2d_pack_bf16_pad", ptr(w2), 48, 192, 3, 3, 64, 192, ptr(wp2), ptr(wt2), S())
    out = torch.full((N, H, W, ld), POISON, device=DEV)
    part = torch.empty(lib.es_conv2d_bnstats_size(rows, 64), device=DEV)
    call("es_conv2d_fwd_bf16_bnin_ex", ptr(x2), N, H, W, 192, H * W * 192, W * 192, 192, 1, ptr(wp2), None, 64, 3, 3, 1, 1,
         ptr(out, 96), H * W * ld, W * ld, ld, 0, ptr(part), 1, ptr(m2_), ptr(r2_), ptr(g2_), ptr(b2_), S())
    # the slice's gradient inside an fp32 gradient buffer; the 16 channels after it are the next slice's gradient
    gbuf = torch.randint(-2, 3, (N, H, W, ld), generator=g).float()
    gbuf[..., 96:144] = o2["dy"].float()
    gbuf = gbuf.to(DEV)
    ws2 = torch.empty(lib.es_conv2d_bwd_weight_bf16_workspace(rows, 64, 192, 3, 3, 0), device=DEV)
    call("es_conv2d_bwd_weight_bf16_bnin_ex", ptr(x2), N, H, W, 192, H * W * 192, W * 192, 192, 1, ptr(gbuf, 96),
         H * W * ld, W * ld, ld, 64, 3, 3, 1, 1, 0, ptr(ws2), ptr(s2), 0, 1, ptr(m2_), ptr(r2_), ptr(g2_), ptr(b2_), S())
    dx2 = torch.empty(N, H, W, 192, device=DEV)
    call("es_conv2d_bwd_data_bf16_ex", ptr(gbuf, 96), H * W * ld, W * ld, ld, ptr(wt2), N, H, W, 192, 64, 3, 3, 1, 1,
         ptr(dx2), H * W * 192, W * 192, 192, 1, 0, 0, S())

    # ---- both padded weight gradients into the flat gradient, one launch
    assert lib.es_dw_unpad_entry_size() == ctypes.sizeof(_UnpadEntry)
    tab = _run_table([_UnpadEntry(s1.data_ptr(), dst1.data_ptr(), 192, 160, 192, 144, 1, 0),
                      _UnpadEntry(s2.data_ptr(), dst2.data_ptr(), 64, 192, 48, 192, 9, 0)], DEV)
    call("es_dw_unpad_multi", ptr(tab), 2, 48 * 192 * 9, S())
    torch.cuda.synchronize()

    assert torch.equal(y1.cpu().double(), r1["y_bn"])
    assert torch.equal(da[..., :144].cpu().double(), r1["dx"]) and torch.all(da[..., 144:] == 0)
    assert torch.equal(out[..., 96:144].cpu().double(), r2["y_bn"])
    assert torch.all(out[..., 144:160] == 0)  # the 16 pad channels
    assert torch.all(out[..., :96] == POISON) and torch.all(out[..., 160:] == POISON)  # nothing else touched
    assert torch.equal(dx2.cpu().double(), r2["dx"])
    assert torch.equal(dst1.cpu().double().view(192, 144, 1, 1), r1["dw_bn"])
    assert torch.equal(dst2.cpu().double().view(48, 192, 3, 3), r2["dw_bn"])
    keep = torch.ones_like(flat_grad, dtype=torch.bool)
    keep[64:64 + 192 * 144] = False
    keep[128 + 192 * 144:128 + 192 * 144 + 48 * 192 * 9] = False
    assert torch.all(flat_grad[keep] == POISON)  # nothing padded reaches the flat gradient
    # the slice's statistics from the padded conv's partials: the first 48 of 64 channels
    want = cc.bn_partials(r2["y_bn"])  # [2, 2, 48]
    got = part.view(-1, 2, 64).cpu().double()
    assert torch.equal(got[:, 0, :48], want[:, 0])  # integer block sums: exact
    # the block-centred squares exceed 2^24: tests/test_gpu_conv_exact.py's bar for this half, 2^-19 ref + 2^-10
    assert bool(((got[:, 1, :48] - want[:, 1]).abs() <= 2.0 ** -19 * want[:, 1] + 2.0 ** -10).all())
    assert torch.all(got[:, :, 48:] == 0)
