"""The host half of the device input path's CoMatch and labeled transforms (csrc/host_aug.cpp:
esh_comatch_device_plan, esh_labeled_device_plan and the explicit-draw builders): the plans' draws are the batch
builder's own in its own order, the resolved rotation walks as Image.rotate does, the three plan entries are one
struct each in both libraries and in ctypes, and every entry point refuses bad arguments before doing anything.
No GPU: the pixels are checked in tests/test_gpu_device_aug_comatch.py."""
import ctypes

import numpy as np
import pytest
import torch

from endossl import host_aug


def _frames(n, seed):
    """Ragged small frames, some with a side already at the resize target of S = 32 / 64 (38 / 76)."""
    g = np.random.default_rng(seed)
    sides = [38, 76, 32, 64, 30, 22, 51, 97, 45, 120]
    return [g.integers(0, 256, (sides[g.integers(0, 10)], sides[g.integers(0, 10)], 3), dtype=np.uint8)
            for _ in range(n)]


def _hwc(t):
    return np.ascontiguousarray(t.numpy().transpose(1, 2, 0))


def _hue_factor(shift):
    """A factor adjust_hue truncates to `shift`: (int)(f * 255.0) == shift, |f| <= 0.5 for |shift| <= 127."""
    return 0.0 if shift == 0 else (shift + (0.5 if shift > 0 else -0.5)) / 255.0


def _jitter(a, j):
    """An AugJitter's draws through the single-op entry points."""
    if j.applied:
        for k in range(j.nops):
            o = j.order[k]
            assert j.kind[k] == (o if o == 3 or j.factor[o] != 1.0 else host_aug.JIT_NONE)
            if o == 3:
                a = host_aug.adjust_hue(a, _hue_factor(j.hue))
            else:
                a = host_aug.enhance(a, ("brightness", "contrast", "color")[o], j.factor[o])
    else:
        assert list(j.kind) == [host_aug.JIT_NONE] * 4
    assert all(j.kind[k] == host_aug.JIT_NONE for k in range(j.nops, 4))
    if j.gray:
        a = host_aug.grayscale3(a)
    if j.flip:
        a = np.ascontiguousarray(a[:, ::-1])
    return a


@pytest.mark.parametrize("S", [32, 64])
def test_plan_replay_equals_host_comatch(S):
    """The CoMatch plan's draws, replayed on the eval view, give transform_batch's three views: the duplicated
    draw order is comatch_triplet's (2 seeds x 128 images = 256 (seed, index) pairs)."""
    ops, firsts, lasts, seen = set(), set(), set(), set()
    for seed in (11, (7 << 32) ^ 5):
        imgs = _frames(128, seed & 0xffff)
        w, s0, s1 = host_aug.transform_batch(imgs, S, "comatch", True, seed=seed, threads=4)
        (ev,) = host_aug.transform_batch(imgs, S, "eval", True, threads=4)
        entries, _, _ = host_aug.comatch_device_plan([a.shape[1] for a in imgs], [a.shape[0] for a in imgs], S, True,
                                                     seed=seed)
        pad = int(S * 0.125)
        for i, e in enumerate(host_aug.plan_entries(entries, "comatch")):
            base = _hwc(ev[i])
            a = np.ascontiguousarray(base[:, ::-1]) if e.flip_w else base
            assert np.array_equal(a, _hwc(w[i])), (seed, i)
            assert (e.s0.top, e.s0.left) == (pad, pad)
            a = np.ascontiguousarray(base[:, ::-1]) if e.s0.flip else base
            for o in e.s0.ops:
                assert 1 <= o.v <= 9 and 0 <= o.op < 14
                if o.applied:
                    a = host_aug.aug_op(a, o.op, o.v, bool(o.neg))
                    ops.add(o.op)
            a = host_aug.fill_rect(a, tuple(e.s0.rect), 127)
            assert np.array_equal(a, _hwc(s0[i])), (seed, i)
            j = e.jit
            assert j.nops == 4 and sorted(j.order) == [0, 1, 2, 3] and -25 <= j.hue <= 25
            assert all(np.float32(0.6) <= f <= np.float32(1.4) for f in j.factor) or not j.applied
            assert np.array_equal(_jitter(base, j), _hwc(s1[i])), (seed, i)
            seen.update([("applied", j.applied), ("gray", j.gray), ("flip", j.flip), ("flip_w", e.flip_w)])
            if j.applied:
                firsts.add(j.order[0])
                lasts.add(j.order[3])
    assert ops == set(range(14)) and firsts == lasts == {0, 1, 2, 3}
    assert seen == {(k, v) for k in ("applied", "gray", "flip", "flip_w") for v in (0, 1)}


def _walk(img, a):
    """Pillow's 16.16 affine walk (NEAREST, black fill) in closed form under the plan's six integers."""
    R = img.shape[0]
    y, x = np.mgrid[0:R, 0:R].astype(np.int64)
    wrap = lambda v: ((v + 2 ** 31) % 2 ** 32) - 2 ** 31  # noqa: E731 -- int32 wrap-around
    xi, yi = wrap(a[2] + y * a[1] + x * a[0]) >> 16, wrap(a[5] + y * a[4] + x * a[3]) >> 16
    ok = (xi >= 0) & (xi < R) & (yi >= 0) & (yi < R)
    out = np.zeros_like(img)
    out[ok] = img[yi[ok], xi[ok]]
    return out


@pytest.mark.parametrize("S,is_crop", [(32, True), (64, True), (32, False)])
def test_plan_replay_equals_host_labeled(S, is_crop):
    """The labeled plan's draws, replayed through resize / flips / rotate / crop / enhance, give
    transform_batch(kind='labeled'); the resolved 16.16 matrix walks the R x R image as rotate() does."""
    R = host_aug.resize_side(S, is_crop)
    seen, orders = set(), set()
    for seed in (11, (7 << 32) ^ 5):
        imgs = _frames(128, seed & 0xffff)
        (want,) = host_aug.transform_batch(imgs, S, "labeled", is_crop, seed=seed, threads=4)
        entries, _, _ = host_aug.labeled_device_plan([a.shape[1] for a in imgs], [a.shape[0] for a in imgs], S,
                                                     is_crop, seed=seed)
        for i, e in enumerate(host_aug.plan_entries(entries, "labeled")):
            c = e.head.crop
            assert c == ((R - S) // 2 if is_crop else 0) and -20.0 <= e.angle < 20.0 and e.rot == 1
            a = host_aug.resize_bilinear(imgs[i], (R, R))
            if e.hflip:
                a = a[:, ::-1]
            if e.vflip:
                a = a[::-1]
            a = np.ascontiguousarray(a)
            rot = host_aug.rotate(a, e.angle)
            assert np.array_equal(_walk(a, list(e.a)), rot), (seed, i)
            j = e.jit
            assert j.applied == 1 and j.nops == 3 and sorted(j.order[:3]) == [0, 1, 2] and not j.gray and not j.flip
            assert all(np.float32(0.8) <= f <= np.float32(1.2) for f in j.factor)
            a = _jitter(np.ascontiguousarray(rot[c:c + S, c:c + S]), j)
            assert np.array_equal(a, _hwc(want[i])), (seed, i)
            seen.update([("hflip", e.hflip), ("vflip", e.vflip), ("neg", int(e.angle < 0))])
            orders.add(tuple(j.order[:3]))
    assert seen == {(k, v) for k in ("hflip", "vflip", "neg") for v in (0, 1)} and len(orders) == 6


def test_explicit_draws_resolve_as_the_stream_plans_do():
    """The *_from_draws builders over an entry's own draws give the entry's transform bytes back."""
    S = 64
    entries, _, _ = host_aug.comatch_device_plan([80] * 64, [70] * 64, S, True, seed=3)
    for e in host_aug.plan_entries(entries, "comatch"):
        j = e.jit
        r = host_aug.jitter_plan_from_draws(list(j.order), list(j.factor), _hue_factor(j.hue), j.gray, j.flip, j.applied)
        assert bytes(r) == bytes(j)
    entries, _, _ = host_aug.labeled_device_plan([80] * 64, [70] * 64, S, True, seed=3)
    off = host_aug.LabEntry.hflip.offset
    for e in host_aug.plan_entries(entries, "labeled"):
        r = host_aug.labeled_plan_from_draws(S, True, e.hflip, e.vflip, e.angle, list(e.jit.order[:3]), list(e.jit.factor))
        assert bytes(r)[off:] == bytes(e)[off:] and r.head.crop == e.head.crop == 6
    # a factor of exactly 1 and a zero or sub-resolution angle resolve to "nothing to run"
    j = host_aug.jitter_plan_from_draws(["hue", "contrast", "brightness", "saturation"], (1.0, 0.9, 1.0), 0.0)
    assert list(j.kind) == [3, 1, host_aug.JIT_NONE, host_aug.JIT_NONE] and j.hue == 0
    assert list(host_aug.jitter_plan_from_draws([0, 1, 2, 3], (0.5, 0.5, 0.5), 0.1, applied=False).kind) == [4] * 4
    for angle in (0.0, 360.0, -720.0, 1e-15, -1e-15):
        assert host_aug.labeled_plan_from_draws(S, True, 0, 0, angle).rot == 0, angle
    assert host_aug.labeled_plan_from_draws(S, True, 0, 0, 1e-3).rot == 1
    assert host_aug.labeled_plan_from_draws(S, False, 0, 0, 5.0).head.crop == 0


def test_entry_sizes_agree_and_bad_arguments_are_refused():
    from endossl import _lib
    h, d = host_aug.load(), _lib.load()
    assert h.esh_comatch_entry_size() == d.es_aug_comatch_entry_size() == ctypes.sizeof(host_aug.CoEntry)
    assert h.esh_labeled_entry_size() == d.es_aug_labeled_entry_size() == ctypes.sizeof(host_aug.LabEntry)
    assert h.esh_aug_entry_size() == d.es_aug_entry_size() == ctypes.sizeof(host_aug.AugEntry)
    assert host_aug.AugEntry.flip.offset + ctypes.sizeof(host_aug.AugStrong) == ctypes.sizeof(host_aug.AugEntry)
    assert host_aug.AugHead.crop.offset == host_aug.AugEntry.crop.offset
    P = host_aug._ptr
    ws, hs = np.array([40], np.int32), np.array([30], np.int32)
    for fn, cls in ((h.esh_comatch_device_plan, host_aug.CoEntry), (h.esh_labeled_device_plan, host_aug.LabEntry)):
        ent = np.zeros(ctypes.sizeof(cls), np.uint8)
        co = np.zeros(4096, np.int32)
        used = ctypes.c_size_t()

        def plan(ws_=ws, hs_=hs, n=1, S=32, ent_=ent, co_=co, cap=4096, used_=used):
            return fn(None if ws_ is None else P(ws_), P(hs_), None, n, S, 1, 0, None if ent_ is None else P(ent_),
                      None if co_ is None else P(co_), cap, ctypes.byref(used_) if used_ is not None else None)
        assert plan() == 0 and used.value == 38 * (2 + 5) + 38 * (2 + 3)  # 40 -> 38: 5 taps, 30 -> 38: 3
        assert plan(ws_=None) == 2 and plan(ent_=None) == 2 and plan(used_=None) == 2 and plan(n=0) == 2
        assert plan(S=1) == 3 and plan(ws_=np.array([0], np.int32)) == 3
        assert plan(cap=10) == 3 and used.value == 38 * 12 and plan(co_=None) == 3
    for bad in ([0, 1, 2, 2], [0, 1, 4, 3], [0, 1], [0, 1, 3]):  # a repeat, out of range, too few, hue among three
        with pytest.raises(host_aug.HostLibraryError):
            host_aug.jitter_plan_from_draws(bad)
    with pytest.raises(host_aug.HostLibraryError):
        host_aug.jitter_plan_from_draws([0, 1, 2, 3], hue=0.51)
    for angle in (90.0, 180.0, -90.0, float("nan")):
        with pytest.raises(host_aug.HostLibraryError):
            host_aug.labeled_plan_from_draws(32, True, 0, 0, angle)
    with pytest.raises(host_aug.HostLibraryError):
        host_aug.labeled_plan_from_draws(1, True, 0, 0, 3.0)
    with pytest.raises(host_aug.HostLibraryError):
        host_aug.labeled_plan_from_draws(32, True, 0, 0, 3.0, order=[0, 1, 3])
    # device: every refusal comes before any launch (the pointers are never dereferenced)
    p = 0x7000000000
    tmp = ((4 * 50 * 38 * 3 + 255) // 256) * 256
    need_c = d.es_aug_comatch_workspace(4, 32, 1, 60, 50)
    need_l = d.es_aug_labeled_workspace(4, 32, 1, 60, 50)
    assert need_c == tmp + 4 * 3 * 32 * 32 + 4 * 6 * 32 * 32 and need_l == tmp + 4 * 3 * 38 * 38
    assert d.es_aug_labeled_workspace(4, 32, 0, 60, 50) == ((4 * 50 * 32 * 3 + 255) // 256) * 256 + 4 * 3 * 32 * 32
    for q in (d.es_aug_comatch_workspace, d.es_aug_labeled_workspace):
        assert q(0, 32, 1, 60, 50) == 0 and q(4, 1, 1, 60, 50) == 0 and q(4, 32, 1, 60, 0) == 0

    def cm(frames=p, fb=1000, ent_=p, co_=p, n=4, S=32, max_h=50, weak=p, s0=p, s1=p, wsp=p, wb=need_c):
        return d.es_aug_comatch_u8(frames, fb, ent_, co_, 100, n, S, 1, max_h, weak, s0, s1, wsp, wb, None)

    def lb(frames=p, fb=1000, ent_=p, co_=p, n=4, S=32, max_h=50, weak=p, wsp=p, wb=need_l, **_):
        return d.es_aug_labeled_u8(frames, fb, ent_, co_, 100, n, S, 1, max_h, weak, wsp, wb, None)
    for f, need in ((cm, need_c), (lb, need_l)):
        assert f(n=0) == -1 and f(S=1) == -1 and f(S=5000) == -1 and f(max_h=0) == -1 and f(n=70000) == -1
        assert f(frames=None) == -2 and f(ent_=None) == -2 and f(weak=None) == -2 and f(wsp=None) == -2
        assert f(wb=need - 1) == -2 and f(ent_=p + 4) == -2 and f(co_=p + 2) == -2 and f(fb=0) == -2
    assert cm(s0=None) == -2 and cm(s1=None) == -2

    def jt(x=p, pl=p, n=4, S=32, out=p + 4096):
        return d.es_aug_jitter_u8(x, pl, n, S, out, None)
    assert jt(n=0) == -1 and jt(S=1) == -1 and jt(S=5000) == -1 and jt(n=70000) == -1
    assert jt(x=None) == -2 and jt(pl=None) == -2 and jt(out=None) == -2 and jt(out=p) == -2 and jt(pl=p + 2) == -2
