"""The device input path's host half (csrc/host_aug.cpp: esh_fixmatch_device_plan, esh_aug_plan_from_draws):
the plan's draws are the batch builder's own, its resize tables are Pillow's, and the plan entry is one struct
in both libraries.  No GPU: the pixels are checked in tests/test_gpu_device_aug.py."""
import ctypes

import numpy as np
import pytest
import torch

from endossl import host_aug


def _frames(n, seed):
    """Ragged small frames, some with a side already at the resize target of S = 32 / 64 (38 / 76, 32 / 64)."""
    g = np.random.default_rng(seed)
    sides = [38, 76, 32, 64, 30, 22, 51, 97, 45, 120]
    out = []
    for i in range(n):
        w, h = sides[g.integers(0, len(sides))], sides[g.integers(0, len(sides))]
        out.append(g.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return out


def _hwc(t):
    return np.ascontiguousarray(t.numpy().transpose(1, 2, 0))


@pytest.mark.parametrize("S", [32, 64])
def test_plan_replay_equals_host_fixmatch(S):
    """The plan's draws, replayed through the single-op entry points on the eval view, give transform_batch's
    strong view: the duplicated draw order is fixmatch_pair's (2 seeds x 128 images = 256 (seed, index) pairs)."""
    seen = set()
    for seed in (11, (7 << 32) ^ 5):
        imgs = _frames(128, seed & 0xffff)
        weak, strong = host_aug.transform_batch(imgs, S, "fixmatch", True, seed=seed, threads=4)
        (ev,) = host_aug.transform_batch(imgs, S, "eval", True, threads=4)
        assert torch.equal(weak, ev)
        entries, _, _ = host_aug.fixmatch_device_plan([a.shape[1] for a in imgs], [a.shape[0] for a in imgs], S, True,
                                                      seed=seed)
        pad = int(S * 0.125)
        for i, e in enumerate(host_aug.plan_entries(entries)):
            a = _hwc(ev[i])
            if e.flip:
                a = np.ascontiguousarray(a[:, ::-1])
            a = host_aug.pad_reflect_crop(a, pad, e.top, e.left, S)
            for o in e.ops:
                assert 1 <= o.v <= 9 and 0 <= o.op < 14
                if o.applied:
                    a = host_aug.aug_op(a, o.op, o.v, bool(o.neg))
                    seen.add(o.op)
            a = host_aug.fill_rect(a, tuple(e.rect), 127)
            assert np.array_equal(a, _hwc(strong[i])), (seed, i)
    assert seen == set(range(14))


def test_plan_from_draws_resolves_as_the_stream_plan_does():
    """esh_aug_plan_from_draws over an entry's own draws gives the entry's strong-chain bytes back."""
    S = 64
    entries, _, _ = host_aug.fixmatch_device_plan([80] * 64, [70] * 64, S, True, seed=3)
    off = host_aug.AugEntry.flip.offset
    for e in host_aug.plan_entries(entries):
        r = host_aug.aug_plan_from_draws(S, e.flip, e.top, e.left, [o.op for o in e.ops], [o.v for o in e.ops],
                                         [o.applied for o in e.ops], [o.neg for o in e.ops], list(e.rect))
        assert bytes(r)[off:] == bytes(e)[off:]


def _apply_tables(img, coeffs, e, R):
    """Pillow's two passes in numpy int32 under the plan's tables (resize_h then resize_v)."""
    def one(src, off, ksize, axis):
        if off < 0:
            return src
        bounds = coeffs[off:off + 2 * R].reshape(R, 2)
        kk = coeffs[off + 2 * R:off + 2 * R + R * ksize].reshape(R, ksize)
        src = np.moveaxis(src, axis, 0).astype(np.int32)
        out = np.empty((R,) + src.shape[1:], np.uint8)
        for j in range(R):
            lo, cnt = bounds[j]
            acc = np.int32(1 << 21) + np.tensordot(kk[j, :cnt].astype(np.int32), src[lo:lo + cnt], axes=(0, 0))
            out[j] = np.clip(acc >> 22, 0, 255)
        return np.moveaxis(out, 0, axis)
    t = one(img, e.coef_h, e.ksize_h, 1)
    return one(t, e.coef_v, e.ksize_v, 0)


@pytest.mark.parametrize("w,h,R", [(30, 22, 48), (301, 227, 48), (48, 48, 48), (48, 100, 48), (17, 48, 48),
                                   (500, 375, 268)])
def test_coefficient_tables_reproduce_resize_bilinear(w, h, R):
    g = np.random.default_rng(w * 1000 + h)
    img = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    entries, coeffs, used = host_aug.fixmatch_device_plan([w], [h], R, False, seed=0)
    e = host_aug.plan_entries(entries)[0]
    assert (e.coef_h < 0) == (w == R) and (e.coef_v < 0) == (h == R) and e.crop == 0
    assert used == sum(R * (2 + k) for k, off in ((e.ksize_h, e.coef_h), (e.ksize_v, e.coef_v)) if off >= 0)
    assert np.array_equal(_apply_tables(img, coeffs, e, R), host_aug.resize_bilinear(img, (R, R)))


def test_tables_are_shared_between_equal_sizes_and_crop_offset_is_center_crops():
    entries, coeffs, used = host_aug.fixmatch_device_plan([100, 100, 76, 100], [90, 90, 100, 76], 64, True, seed=1)
    es = host_aug.plan_entries(entries)
    assert es[0].coef_h == es[1].coef_h == es[3].coef_h == es[2].coef_v and es[0].coef_v == es[1].coef_v
    assert es[2].coef_h == -1 and es[3].coef_v == -1 and all(e.crop == 6 for e in es)  # (76 - 64) / 2
    assert [e.frame_off for e in es] == [0, 27000, 54000, 76800]
    assert used == 2 * 76 * (2 + 5)  # 100 -> 76 and 90 -> 76, both 5 taps


def test_entry_sizes_agree_and_bad_arguments_are_refused():
    from endossl import _lib
    h, d = host_aug.load(), _lib.load()
    assert h.esh_aug_entry_size() == d.es_aug_entry_size() == ctypes.sizeof(host_aug.AugEntry) == host_aug.ENTRY_BYTES
    # host: the plan
    ws, hs = np.array([40], np.int32), np.array([30], np.int32)
    ent = np.zeros(host_aug.ENTRY_BYTES, np.uint8)
    co = np.zeros(4096, np.int32)
    used = ctypes.c_size_t()
    P = host_aug._ptr

    def plan(ws_=ws, hs_=hs, n=1, S=32, ent_=ent, co_=co, cap=4096, used_=used):
        return h.esh_fixmatch_device_plan(None if ws_ is None else P(ws_), P(hs_), None, n, S, 1, 0,
                                          None if ent_ is None else P(ent_), None if co_ is None else P(co_), cap,
                                          ctypes.byref(used_) if used_ is not None else None)
    assert plan() == 0 and used.value == 38 * (2 + 5) + 38 * (2 + 3)  # 40 -> 38: 5 taps, 30 -> 38: 3
    assert plan(ws_=None) == 2 and plan(ent_=None) == 2 and plan(used_=None) == 2 and plan(n=0) == 2
    assert plan(S=1) == 3 and plan(ws_=np.array([0], np.int32)) == 3
    assert plan(cap=10) == 3 and used.value == 38 * 12 and plan(co_=None) == 3
    with pytest.raises(host_aug.HostLibraryError):
        host_aug.aug_plan_from_draws(32, 0, 0, 0, [14, 0], [1, 1], [1, 1], [0, 0], [0, 0, 1, 1])
    with pytest.raises(host_aug.HostLibraryError):
        host_aug.aug_plan_from_draws(32, 0, 0, 0, [0, 0], [11, 1], [1, 1], [0, 0], [0, 0, 1, 1])
    with pytest.raises(host_aug.HostLibraryError):
        host_aug.aug_plan_from_draws(32, 0, 9, 0, [0, 0], [1, 1], [1, 1], [0, 0], [0, 0, 1, 1])  # top > 2 * pad
    with pytest.raises(host_aug.HostLibraryError):
        host_aug.aug_plan_from_draws(1, 0, 0, 0, [0, 0], [1, 1], [1, 1], [0, 0], [0, 0, 1, 1])
    # device: every refusal comes before any launch (the pointers are never dereferenced)
    p = 0x7000000000
    need = d.es_aug_fixmatch_workspace(4, 32, 1, 60, 50)
    assert need == ((4 * 50 * 38 * 3 + 255) // 256) * 256 + 4 * 6 * 32 * 32
    assert d.es_aug_strong_workspace(4, 32) == 4 * 6 * 32 * 32
    assert d.es_aug_fixmatch_workspace(0, 32, 1, 60, 50) == 0 and d.es_aug_fixmatch_workspace(4, 1, 1, 60, 50) == 0

    def fm(frames=p, fb=1000, ent_=p, co_=p, n=4, S=32, max_h=50, weak=p, wsp=p, wb=need):
        return d.es_aug_fixmatch_u8(frames, fb, ent_, co_, 100, n, S, 1, max_h, weak, p, wsp, wb, None)
    assert fm(n=0) == -1 and fm(S=1) == -1 and fm(S=5000) == -1 and fm(max_h=0) == -1 and fm(n=70000) == -1
    assert fm(frames=None) == -2 and fm(ent_=None) == -2 and fm(weak=None) == -2 and fm(wsp=None) == -2
    assert fm(wb=need - 1) == -2 and fm(ent_=p + 4) == -2 and fm(co_=p + 2) == -2 and fm(fb=0) == -2

    def st(weak=p, ent_=p, n=4, S=32, strong=p, wsp=p, wb=4 * 6 * 32 * 32):
        return d.es_aug_strong_u8(weak, ent_, n, S, strong, wsp, wb, None)
    assert st(n=0) == -1 and st(S=1) == -1
    assert st(weak=None) == -2 and st(ent_=None) == -2 and st(strong=None) == -2 and st(wsp=None) == -2
    assert st(wb=4 * 6 * 32 * 32 - 1) == -2


def test_copy_frames_packs_the_chosen_frames_and_plan_and_copy_uses_their_offsets():
    imgs = _frames(12, 3)
    ws = np.array([a.shape[1] for a in imgs], np.int32)
    hs = np.array([a.shape[0] for a in imgs], np.int32)
    idx = np.array([5, 0, 5, 11, 2], np.int64)
    need = int(sum(imgs[i].size for i in idx))
    arena = np.zeros(need + 7, np.uint8)
    entries = np.zeros(len(idx) * host_aug.ENTRY_BYTES, np.uint8)
    coeffs = np.zeros(1 << 14, np.int32)
    for threads in (1, 3):
        arena[:] = 0
        nbytes, used = host_aug.plan_and_copy(imgs, ws, hs, idx, 32, True, 9, entries, coeffs, arena=arena,
                                              threads=threads)
        assert nbytes == need and used > 0 and not arena[need:].any()
        for e, i in zip(host_aug.plan_entries(entries), idx):
            assert (e.w, e.h) == (imgs[i].shape[1], imgs[i].shape[0])
            assert np.array_equal(arena[e.frame_off:e.frame_off + imgs[i].size], imgs[i].reshape(-1))
    ref, _, _ = host_aug.fixmatch_device_plan(ws[idx], hs[idx], 32, True, seed=9)
    assert np.array_equal(ref.reshape(-1), entries)  # packed in order = the default offsets
    with pytest.raises(host_aug.HostLibraryError):
        host_aug.plan_and_copy(imgs, ws, hs, idx, 32, True, 9, entries, coeffs, arena=arena[:need - 1])
    with pytest.raises(ValueError):
        host_aug.plan_and_copy(imgs, ws, hs, idx, 32, True, 9, entries, coeffs[:8], arena=arena)
    # frame set resident: the offsets are the caller's
    offs = np.arange(12, dtype=np.int64) * 100000
    nbytes, _ = host_aug.plan_and_copy(imgs, ws, hs, idx, 32, True, 9, entries, coeffs, offsets=offs)
    assert nbytes == 0 and [e.frame_off for e in host_aug.plan_entries(entries)] == [500000, 0, 500000, 1100000, 200000]
