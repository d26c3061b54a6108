"""The direct 1 x 1 convolution kernels (es_conv1x1_fwd_bf16_ex / _bnin_ex / es_conv1x1_bwd_data_bf16_ex) on the MI355X.

Exact-integer products against a CPU integer matmul (operands in {-2..2}, sums far below 2^24: no tolerance), the
BatchNorm partials against the implicit kernel's, random bf16 operands against fp64 beside the implicit kernel, and
the edges: M = 8, M off the 128-row tile, Cout below the 128-column tile, reads / writes inside sentinel-filled
buffers.  Each shape runs on both column tiles where Cout allows (es_set_conv_small 0: the 128-column tile)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from endossl import _lib  # noqa: E402
from endossl._lib import call, ptr  # noqa: E402

DEV = "cuda"

# (N, H, W, Cin, Cout): M = 8 (the last stage of a 64^2 image pair); M = 200, off the tile; M = 385 = 3 * 128 + 1
# with Cout below the 128-column tile; M, Cin, Cout all whole tiles (two row blocks, two K steps, one 128 tile)
SHAPES = [(2, 2, 2, 2048, 512), (2, 10, 10, 64, 256), (5, 7, 11, 256, 64), (4, 8, 8, 128, 128)]


def S():
    return _lib.stream()


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _lib.load()


@pytest.fixture(params=[128, 0], ids=["tile-auto", "tile-128"])
def tile(request):
    """es_set_conv_small: 128 (default: small grids on the 64-column tile) or 0 (the 128-column tile whenever
    Cout % 128 == 0) -- for the direct and the implicit kernels alike."""
    lib = _lib.load()
    assert lib.es_set_conv_small(request.param) >= 0
    yield request.param
    lib.es_set_conv_small(128)


def _ints(gen, *shape, lo=-2, hi=3):
    return torch.randint(lo, hi, shape, generator=gen, dtype=torch.int64)


def _pack(w):
    """[Cout, Cin] fp32 on the device -> the forward and the transposed bf16 images."""
    Cout, Cin = w.shape
    wp = torch.empty(w.numel(), dtype=torch.bfloat16, device=DEV)
    wt = torch.empty_like(wp)
    call("es_conv2d_pack_bf16", ptr(w.contiguous()), Cout, Cin, 1, 1, ptr(wp), ptr(wt), S())
    return wp, wt


@pytest.mark.parametrize("N,H,W,Cin,Cout", SHAPES)
def test_exact_integers(N, H, W, Cin, Cout, tile):
    M = N * H * W
    g = torch.Generator().manual_seed(M + Cin)
    xi, wi, dyi = _ints(g, M, Cin), _ints(g, Cout, Cin), _ints(g, M, Cout)
    x, dy = xi.to(torch.bfloat16).to(DEV), dyi.to(torch.bfloat16).to(DEV)
    wp, wt = _pack(wi.float().to(DEV))
    # forward, fp32 and bf16 output maps
    y = torch.full((M, Cout), 7.0, device=DEV)
    call("es_conv1x1_fwd_bf16_ex", ptr(x), M, Cin, ptr(wp), None, Cout, ptr(y), 0, None, 1, S())
    want = xi @ wi.t()
    assert torch.equal(y.cpu().to(torch.int64), want) and torch.equal(y.cpu(), want.float())
    y16 = torch.zeros(M, Cout, device=DEV, dtype=torch.bfloat16)
    call("es_conv1x1_fwd_bf16_ex", ptr(x), M, Cin, ptr(wp), None, Cout, ptr(y16), 0, None, 3, S())
    assert torch.equal(y16.cpu(), want.float().bfloat16())  # one rounding of the exact sum
    # bias and the accumulating store
    bias = _ints(g, Cout).float().to(DEV)
    ya = y.clone()
    call("es_conv1x1_fwd_bf16_ex", ptr(x), M, Cin, ptr(wp), ptr(bias), Cout, ptr(ya), 1, None, 1, S())
    assert torch.equal(ya.cpu(), (2 * want + bias.cpu().to(torch.int64)).float())
    # BatchNorm-in forward: gamma 1, beta 0, integer mean, rstd a power of two -> integral operands <= 6
    mean_i, rstd_i = _ints(g, Cin, lo=-1, hi=2), 1 + _ints(g, Cin, lo=0, hi=2)
    mean, rstd = mean_i.float().to(DEV), rstd_i.float().to(DEV)
    gam, bet = torch.ones(Cin, device=DEV), torch.zeros(Cin, device=DEV)
    yb = torch.full((M, Cout), 7.0, device=DEV)
    call("es_conv1x1_fwd_bf16_bnin_ex", ptr(x), M, Cin, ptr(wp), None, Cout, ptr(yb), 0, None, 1, ptr(mean), ptr(rstd),
         ptr(gam), ptr(bet), S())
    a = ((xi - mean_i) * rstd_i).clamp(min=0)
    assert torch.equal(yb.cpu(), (a @ wi.t()).float())
    # data gradient dx = dy . W, plain and accumulating
    dx = torch.full((M, Cin), 7.0, device=DEV)
    call("es_conv1x1_bwd_data_bf16_ex", ptr(dy), M, Cout, ptr(wt), Cin, ptr(dx), 0, 1, S())
    wantx = dyi @ wi
    assert torch.equal(dx.cpu(), wantx.float())
    call("es_conv1x1_bwd_data_bf16_ex", ptr(dy), M, Cout, ptr(wt), Cin, ptr(dx), 1, 1, S())
    assert torch.equal(dx.cpu(), (2 * wantx).float())


@pytest.mark.parametrize("N,H,W,Cin,Cout", SHAPES)
def test_bn_partials_match_implicit_kernel(N, H, W, Cin, Cout, tile):
    """The forward's BatchNorm partials against es_conv2d_fwd_bf16_bnstats' on the same input: the same layout
    ([128-row block][sum | M2][Cout]) and the same bits, and so the same mean / rstd / running buffers out of
    es_bn2d_fwd_partials_ex -- no ulp of slack is needed: both kernels run the same MFMA sequence per tile and
    share the epilogue."""
    lib = _lib.load()
    M = N * H * W
    g = torch.Generator(device=DEV).manual_seed(M)
    x = torch.randn(M, Cin, device=DEV, generator=g).bfloat16()
    w = torch.randn(Cout, Cin, device=DEV, generator=g) * 0.05
    wp, _ = _pack(w)
    n = lib.es_conv2d_bnstats_size(M, Cout)
    pd, pi = torch.full((n,), -1.0, device=DEV), torch.full((n,), -2.0, device=DEV)
    yd, yi = torch.empty(M, Cout, device=DEV), torch.empty(M, Cout, device=DEV)
    call("es_conv1x1_fwd_bf16_ex", ptr(x), M, Cin, ptr(wp), None, Cout, ptr(yd), 0, ptr(pd), 1, S())
    xf = x.float()  # the same values as an fp32 map (the implicit kernel rounds them back to bf16, exactly)
    call("es_conv2d_fwd_bf16_bnstats", ptr(xf), N, H, W, Cin, H * W * Cin, W * Cin, Cin, 1, ptr(wp), None, Cout, 1, 1,
         1, 0, ptr(yi), H * W * Cout, W * Cout, Cout, ptr(pi), S())
    assert torch.equal(yd, yi) and torch.equal(pd, pi)
    out = []
    for y, part in ((yd, pd), (yi, pi)):
        mean, rstd = torch.empty(Cout, device=DEV), torch.empty(Cout, device=DEV)
        rm, rv = torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        gam, bet = torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV)
        call("es_bn2d_fwd_partials_ex", ptr(y), M, Cout, ptr(part.clone()), ptr(gam), ptr(bet), ptr(rm), ptr(rv),
             ptr(nbt), 0.1, 1e-5, None, 1, None, ptr(mean), ptr(rstd), 0, S())
        out.append((mean, rstd, rm, rv))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    # and they are the batch statistics (fp64 of the fp32 output; fp32 partial sums: 1e-5 relative)
    ref = yd.double()
    assert (out[0][0].double() - ref.mean(0)).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())
    want_rstd = (ref.var(0, unbiased=False) + 1e-5).rsqrt()
    assert ((out[0][1].double() - want_rstd) / want_rstd).abs().max().item() <= 1e-4


@pytest.mark.parametrize("N,H,W,Cin,Cout", SHAPES)
def test_random_operands_vs_fp64_and_implicit_kernel(N, H, W, Cin, Cout, tile):
    """Random bf16 operands: the direct kernels' max error against an fp64 CPU product of the same bf16 values is at
    most 2x the implicit kernels' (both sum the same bf16 products in fp32, so a factor of two covers a different
    order and nothing else) -- and, as include/endossl.h states, the outputs are the implicit kernels' bit for
    bit: forward, BatchNorm-in forward, data gradient."""
    M = N * H * W
    g = torch.Generator(device=DEV).manual_seed(M + Cout)
    x = torch.randn(M, Cin, device=DEV, generator=g).bfloat16()
    dy = torch.randn(M, Cout, device=DEV, generator=g).bfloat16()
    w = torch.randn(Cout, Cin, device=DEV, generator=g) * 0.05
    wp, wt = _pack(w)
    wb = w.bfloat16().double().cpu()
    mean, rstd = torch.randn(Cin, device=DEV, generator=g) * 0.3, torch.rand(Cin, device=DEV, generator=g) + 0.5
    gam, bet = torch.rand(Cin, device=DEV, generator=g) + 0.5, torch.randn(Cin, device=DEV, generator=g) * 0.2
    xs, ys = (H * W * Cin, W * Cin, Cin, 1), (H * W * Cout, W * Cout, Cout)
    yd, yi, bd, bi = (torch.empty(M, Cout, device=DEV) for _ in range(4))
    dd, di = torch.empty(M, Cin, device=DEV), torch.empty(M, Cin, device=DEV)
    call("es_conv1x1_fwd_bf16_ex", ptr(x), M, Cin, ptr(wp), None, Cout, ptr(yd), 0, None, 1, S())
    call("es_conv2d_fwd_bf16_ex", ptr(x), N, H, W, Cin, *xs, ptr(wp), None, Cout, 1, 1, 1, 0, ptr(yi), *ys, 0, None, 1,
         S())
    call("es_conv1x1_fwd_bf16_bnin_ex", ptr(x), M, Cin, ptr(wp), None, Cout, ptr(bd), 0, None, 1, ptr(mean), ptr(rstd),
         ptr(gam), ptr(bet), S())
    call("es_conv2d_fwd_bf16_bnin_ex", ptr(x), N, H, W, Cin, *xs, ptr(wp), None, Cout, 1, 1, 1, 0, ptr(bi), *ys, 0,
         None, 1, ptr(mean), ptr(rstd), ptr(gam), ptr(bet), S())
    call("es_conv1x1_bwd_data_bf16_ex", ptr(dy), M, Cout, ptr(wt), Cin, ptr(dd), 0, 1, S())
    call("es_conv2d_bwd_data_bf16_ex", ptr(dy), *ys, ptr(wt), N, H, W, Cin, Cout, 1, 1, 1, 0, ptr(di), *xs, 0, 1, S())
    torch.cuda.synchronize()
    # the BatchNorm-in operand as bn() stores it: fma((x - mean) rstd, gamma, beta), ReLU, rounded to bf16
    xn = torch.addcmul(bet, (x.float() - mean) * rstd, gam).clamp(min=0).bfloat16()
    refs = {"fwd": x.double().cpu() @ wb.t(), "bnin": xn.double().cpu() @ wb.t(), "bwd_data": dy.double().cpu() @ wb}
    for name, d, i in (("fwd", yd, yi), ("bnin", bd, bi), ("bwd_data", dd, di)):
        ed = (d.double().cpu() - refs[name]).abs().max().item()
        ei = (i.double().cpu() - refs[name]).abs().max().item()
        print(f"{name} M={M} Cin={Cin} Cout={Cout} tile={tile}: direct max err {ed:.3e}, implicit {ei:.3e}")
        assert ed <= 2 * ei, (name, ed, ei)
        assert torch.equal(d, i), name


@pytest.mark.parametrize("N,H,W,Cin,Cout", SHAPES)
def test_guards_leave_the_sentinels(N, H, W, Cin, Cout, tile):
    """X, dY, Y and dX inside larger sentinel-filled buffers: the rows are read from inside (the values after
    X + M Cin are NaN: a row < M built from them would show), and every byte before Y and after Y + M Cout keeps
    the sentinel -- rows past M of the last 128-row tile and columns past Cout are not stored."""
    M = N * H * W
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(M)
    pad = 4096  # elements on either side (16-byte aligned starts)
    w = torch.randn(Cout, Cin, device=DEV, generator=g) * 0.05
    wp, wt = _pack(w)

    def inside(rows, cols, dtype, fill):
        buf = torch.full((pad + rows * cols + pad,), fill, dtype=dtype, device=DEV)
        return buf, buf[pad:pad + rows * cols].view(rows, cols)
    xbuf, x = inside(M, Cin, torch.bfloat16, float("nan"))
    x.copy_(torch.randn(M, Cin, device=DEV, generator=g))
    dybuf, dy = inside(M, Cout, torch.bfloat16, float("nan"))
    dy.copy_(torch.randn(M, Cout, device=DEV, generator=g))
    SENT = -12345.0
    for od, fl in ((torch.float32, 1), (torch.bfloat16, 3)):
        sent = torch.tensor(SENT, dtype=od).item()
        ybuf, y = inside(M, Cout, od, SENT)
        part = torch.empty(lib.es_conv2d_bnstats_size(M, Cout), device=DEV)
        call("es_conv1x1_fwd_bf16_ex", ptr(x), M, Cin, ptr(wp), None, Cout, ptr(y), 0, ptr(part), fl, S())
        dxbuf, dx = inside(M, Cin, od, SENT)
        call("es_conv1x1_bwd_data_bf16_ex", ptr(dy), M, Cout, ptr(wt), Cin, ptr(dx), 0, fl, S())
        torch.cuda.synchronize()
        for buf, t in ((ybuf, y), (dxbuf, dx)):
            assert bool((buf[:pad] == sent).all()) and bool((buf[pad + t.numel():] == sent).all())
            assert bool(torch.isfinite(t.float()).all()) and not bool((t == sent).any())
        assert bool(torch.isfinite(part).all())
        # and the rows are the product: fp32 sums of K exact bf16 products (K u sum|terms|, u = 2^-24), plus the
        # one rounding of a bf16 output map (2^-9 relative, taken as 2^-8)
        wb = w.bfloat16().double()
        ref, absum = x.double() @ wb.t(), (x.double().abs() @ wb.abs().t()).max().item()
        tol = Cin * 2.0 ** -24 * absum + (2.0 ** -8 * ref.abs().max().item() if od == torch.bfloat16 else 0.0)
        assert (y.double() - ref).abs().max().item() <= tol


def test_knob_and_selection():
    """es_set_conv_1x1: 0 = never, 1 = the measured shape class (default: a reduction 512 deep or more -- Cin of a
    forward, Cout of a data gradient), 2 = every eligible shape; returns the previous value, -2 (unchanged)
    otherwise.  es_conv1x1_bf16_select refuses what the kernels cannot take."""
    lib = _lib.load()
    try:
        for kind in (0, 1):
            assert lib.es_conv1x1_bf16_select(kind, 200, 512, 128) == 1
            assert lib.es_conv1x1_bf16_select(kind, 200, 256, 1024) == 0
        assert lib.es_conv1x1_bf16_select(2, 200, 128, 512) == 1 and lib.es_conv1x1_bf16_select(2, 200, 512, 128) == 0
        assert lib.es_set_conv_1x1(2) == 1  # the default
        assert lib.es_set_conv_1x1(7) == -2 and lib.es_set_conv_1x1(-1) == -2
        for kind in (0, 1, 2):
            assert lib.es_conv1x1_bf16_select(kind, 200, 64, 256) == 1
            assert lib.es_conv1x1_bf16_select(kind, 200, 48, 256) == 0   # channel counts % 32
            assert lib.es_conv1x1_bf16_select(kind, 1 << 30, 64, 64) == 0  # maps of 2 GiB and more
        assert lib.es_conv1x1_bf16_select(3, 200, 64, 256) == 0
        assert lib.es_set_conv_1x1(0) == 2
        assert lib.es_conv1x1_bf16_select(0, 200, 64, 256) == 0
    finally:
        lib.es_set_conv_1x1(1)
    x = torch.zeros(8, 64, device=DEV)  # an fp32 map: flags bit 0 clear is refused, not reinterpreted
    y = torch.zeros(8, 64, device=DEV)
    wp = torch.zeros(64 * 64, dtype=torch.bfloat16, device=DEV)
    assert lib.es_conv1x1_fwd_bf16_ex(ptr(x), 8, 64, ptr(wp), None, 64, ptr(y), 0, None, 0, S()) == -1
