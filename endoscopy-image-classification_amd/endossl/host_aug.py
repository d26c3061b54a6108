"""Host-side input path: the reference's training transforms on the host,
native, feeding the device's uint8 patch gather.

The reference builds its SSL batches with torchvision / PIL transforms in DataLoader workers
(`code/dataset.py:24-56` TransformFixMatch, `:185-207` the labeled train transform,
`code/randaugment.py:207-222` RandAugmentMC) and normalises to fp32 on the host.  Here the same
transforms run in C++ (`csrc/host_aug.cpp`, C-ABI `include/endossl_host.h`, `libendossl_host.so`)
on a pool of host threads and write planar uint8 batches into pinned memory; ToTensor + Normalize
happen on the device inside the patch gather (`es_patch_im2col_u8`), so the host never makes fp32
and the H2D copy is a quarter of the fp32 bytes.

  TransformFixMatchNative(config)(pil_image) -> (weak, strong) uint8 [3, S, S] tensors
  HostBatcher(images, ...) -> pinned uint8 [n, 3, S, S] batches, copied to the device on a side stream

Parity: every PIL op is pinned bit-exact to PIL itself (tests/test_host_aug.py); the random
parameters follow the reference's distributions on the library's own per-image streams (the
reference's Python / numpy / torch generator streams are not reproduced).
"""
import ctypes
import os
import threading

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ENDOSSL_HOST_LIB", os.path.join(_HERE, "lib", "libendossl_host.so"))
ABI_VERSION = 2

# fixmatch_augment_pool() order (code/randaugment.py:147-163)
POOL = ("AutoContrast", "Brightness", "Color", "Contrast", "Equalize", "Identity", "Posterize", "Rotate",
        "Sharpness", "ShearX", "ShearY", "Solarize", "TranslateX", "TranslateY")
ENHANCE = {"brightness": 0, "color": 1, "contrast": 2, "sharpness": 3}

_P = ctypes.c_void_p
_I = ctypes.c_int
_SIG = {
    "esh_abi_version": (_I, []),
    "esh_aug_op": (_I, [_I, _P, _P, _I, _I, _I, _I]),
    "esh_enhance": (_I, [_I, _P, _P, _I, _I, ctypes.c_float]),
    "esh_color_op": (_I, [_I, _P, _P, _I, _I, ctypes.c_double]),
    "esh_rotate": (_I, [_P, _P, _I, _I, ctypes.c_double]),
    "esh_resize_bilinear": (_I, [_P, _I, _I, _P, _I, _I]),
    "esh_fill_rect": (_I, [_P, _I, _I, _I, _I, _I, _I, _I]),
    "esh_pad_reflect_crop": (_I, [_P, _I, _I, _I, _I, _I, _I, _P]),
    "esh_transform_batch": (_I, [_I, ctypes.POINTER(_P), ctypes.POINTER(_I), ctypes.POINTER(_I), _I, _I, _I,
                                 ctypes.c_uint64, _I, _P, _P, _P]),
    "esh_aug_entry_size": (_I, []),
    "esh_aug_plan_from_draws": (_I, [_I, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I),
                                     ctypes.POINTER(_I), ctypes.POINTER(_I), _P]),
    "esh_copy_frames": (_I, [_P, _P, _P, _I, _P, ctypes.c_size_t, _P, ctypes.POINTER(ctypes.c_size_t), _I]),
    "esh_fixmatch_device_plan": (_I, [_P, _P, _P, _I, _I, _I, ctypes.c_uint64, _P, _P, ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_size_t)]),
    "esh_comatch_entry_size": (_I, []),
    "esh_labeled_entry_size": (_I, []),
    "esh_comatch_device_plan": (_I, [_P, _P, _P, _I, _I, _I, ctypes.c_uint64, _P, _P, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t)]),
    "esh_labeled_device_plan": (_I, [_P, _P, _P, _I, _I, _I, ctypes.c_uint64, _P, _P, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t)]),
    "esh_jitter_plan_from_draws": (_I, [_I, _I, ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_float), ctypes.c_double,
                                        _I, _I, _P]),
    "esh_labeled_plan_from_draws": (_I, [_I, _I, _I, _I, ctypes.c_double, ctypes.POINTER(_I),
                                         ctypes.POINTER(ctypes.c_float), _P]),
}


class AugOp(ctypes.Structure):
    """EsAugOp (include/endossl_aug_plan.h): one RandAugmentMC slot with its parameters resolved."""
    _fields_ = [("op", ctypes.c_int32), ("v", ctypes.c_int32), ("applied", ctypes.c_int32),
                ("neg", ctypes.c_int32), ("kind", ctypes.c_int32),
                ("alpha", ctypes.c_float), ("mask", ctypes.c_int32), ("thresh", ctypes.c_int32),
                ("a", ctypes.c_int32 * 6), ("shift_x", ctypes.c_int32), ("shift_y", ctypes.c_int32)]


class AugEntry(ctypes.Structure):
    """EsAugEntry: one image's plan for the device input path."""
    _fields_ = [("frame_off", ctypes.c_int64), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
                ("coef_h", ctypes.c_int32), ("ksize_h", ctypes.c_int32), ("coef_v", ctypes.c_int32),
                ("ksize_v", ctypes.c_int32), ("crop", ctypes.c_int32), ("flip", ctypes.c_int32),
                ("top", ctypes.c_int32), ("left", ctypes.c_int32), ("ops", AugOp * 2), ("rect", ctypes.c_int32 * 4)]


class AugHead(ctypes.Structure):
    """EsAugHead: the frame / resize fields every entry begins with."""
    _fields_ = [("frame_off", ctypes.c_int64), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
                ("coef_h", ctypes.c_int32), ("ksize_h", ctypes.c_int32), ("coef_v", ctypes.c_int32),
                ("ksize_v", ctypes.c_int32), ("crop", ctypes.c_int32)]


class AugStrong(ctypes.Structure):
    """EsAugStrong: the strong chain's fields (AugEntry's from `flip` on)."""
    _fields_ = [("flip", ctypes.c_int32), ("top", ctypes.c_int32), ("left", ctypes.c_int32), ("ops", AugOp * 2),
                ("rect", ctypes.c_int32 * 4)]


class AugJitter(ctypes.Structure):
    """EsAugJitter: a ColorJitter chain, RandomGrayscale and the flip; order / kind hold JITTER indices."""
    _fields_ = [("applied", ctypes.c_int32), ("nops", ctypes.c_int32), ("order", ctypes.c_int32 * 4),
                ("factor", ctypes.c_float * 3), ("hue", ctypes.c_int32), ("gray", ctypes.c_int32),
                ("flip", ctypes.c_int32), ("kind", ctypes.c_int32 * 4)]


class CoEntry(ctypes.Structure):
    """EsAugCoEntry: one image's TransformCoMatch plan."""
    _fields_ = [("head", AugHead), ("flip_w", ctypes.c_int32), ("s0", AugStrong), ("jit", AugJitter)]


class LabEntry(ctypes.Structure):
    """EsAugLabEntry: one image's labeled-transform plan."""
    _fields_ = [("head", AugHead), ("hflip", ctypes.c_int32), ("vflip", ctypes.c_int32), ("rot", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("angle", ctypes.c_double), ("a", ctypes.c_int32 * 6),
                ("jit", AugJitter)]


ENTRY_BYTES = ctypes.sizeof(AugEntry)
AUG_NONE, AUG_SHIFT = 5, 14  # EsAugOp.kind beside the pool indices
JITTER = ("brightness", "contrast", "saturation", "hue")  # EsAugJitter.order / kind; 4 = none
JIT_NONE = 4
# the device path's kinds: entry type, the two libraries' size queries, the host plan function
_PLANS = {"fixmatch": (AugEntry, "esh_aug_entry_size", "es_aug_entry_size", "esh_fixmatch_device_plan"),
          "eval": (AugEntry, "esh_aug_entry_size", "es_aug_entry_size", "esh_fixmatch_device_plan"),
          "comatch": (CoEntry, "esh_comatch_entry_size", "es_aug_comatch_entry_size", "esh_comatch_device_plan"),
          "labeled": (LabEntry, "esh_labeled_entry_size", "es_aug_labeled_entry_size", "esh_labeled_device_plan")}
_lib = None
_lock = threading.Lock()


class HostLibraryError(RuntimeError):
    pass


def load():
    """libendossl_host.so with its signatures bound (built by `make` in csrc/, or __graft_entry__.build())."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise HostLibraryError(f"{LIB_PATH} missing: run `make` in csrc/ (or __graft_entry__.build())")
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in _SIG.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            if lib.esh_abi_version() != ABI_VERSION:
                raise HostLibraryError(f"host ABI {lib.esh_abi_version()} != {ABI_VERSION}")
            for cls, query, _, _ in _PLANS.values():
                if getattr(lib, query)() != ctypes.sizeof(cls):
                    raise HostLibraryError(f"{query}() is {getattr(lib, query)()} bytes in the host library, "
                                           f"host_aug.{cls.__name__} is {ctypes.sizeof(cls)}")
            _lib = lib
    return _lib


def _check(rc, name):
    if rc != 0:
        raise HostLibraryError(f"{name} failed with status {rc}")


def _hwc(img):
    """RGB image (PIL or HWC uint8 array) -> C-contiguous HWC uint8 numpy array."""
    a = np.asarray(img.convert("RGB") if hasattr(img, "convert") else img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected an RGB HWC uint8 image, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _ptr(a):
    return a.ctypes.data_as(_P)


# ---- single ops (the reference's augment pool, for tests and custom pipelines) -----------------
def aug_op(img, op, v, neg=False):
    """Pool op `op` (name or index) at magnitude v on one image; neg = the op's sign draw."""
    a = _hwc(img)
    k = POOL.index(op) if isinstance(op, str) else int(op)
    out = np.empty_like(a)
    _check(load().esh_aug_op(k, _ptr(a), _ptr(out), a.shape[1], a.shape[0], int(v), int(bool(neg))), "esh_aug_op")
    return out


def enhance(img, kind, factor):
    a = _hwc(img)
    out = np.empty_like(a)
    _check(load().esh_enhance(ENHANCE[kind], _ptr(a), _ptr(out), a.shape[1], a.shape[0], float(factor)), "esh_enhance")
    return out


def adjust_hue(img, factor):
    a = _hwc(img)
    out = np.empty_like(a)
    _check(load().esh_color_op(0, _ptr(a), _ptr(out), a.shape[1], a.shape[0], float(factor)), "esh_color_op")
    return out


def grayscale3(img):
    a = _hwc(img)
    out = np.empty_like(a)
    _check(load().esh_color_op(1, _ptr(a), _ptr(out), a.shape[1], a.shape[0], 0.0), "esh_color_op")
    return out


def rotate(img, angle):
    a = _hwc(img)
    out = np.empty_like(a)
    _check(load().esh_rotate(_ptr(a), _ptr(out), a.shape[1], a.shape[0], float(angle)), "esh_rotate")
    return out


def resize_bilinear(img, size):
    """Image.resize(size=(w, h), BILINEAR)."""
    a = _hwc(img)
    w, h = size
    out = np.empty((h, w, 3), np.uint8)
    _check(load().esh_resize_bilinear(_ptr(a), a.shape[1], a.shape[0], _ptr(out), w, h), "esh_resize_bilinear")
    return out


def fill_rect(img, xy, v=127):
    a = _hwc(img).copy()
    _check(load().esh_fill_rect(_ptr(a), a.shape[1], a.shape[0], *[int(t) for t in xy], int(v)), "esh_fill_rect")
    return a


def pad_reflect_crop(img, pad, top, left, size):
    a = _hwc(img)
    out = np.empty((size, size, 3), np.uint8)
    _check(load().esh_pad_reflect_crop(_ptr(a), a.shape[1], a.shape[0], pad, top, left, size, _ptr(out)),
           "esh_pad_reflect_crop")
    return out


# ---- batches --------------------------------------------------------------------------------------
KINDS = {"fixmatch": (0, 2), "labeled": (1, 1), "comatch": (2, 3), "eval": (3, 1)}  # kind -> (id, outputs)


def transform_batch(images, size, kind="fixmatch", is_crop=True, seed=0, threads=None, outs=None):
    """Run one of the reference's transforms over a list of RGB images on `threads` host threads.

    kind 'fixmatch': TransformFixMatch (code/dataset.py:24-56) -> (weak, strong); 'comatch':
    TransformCoMatch (:58-110) -> (weak, strong_0, strong_1); 'labeled': the labeled train transform
    (:185-207) -> (x,); 'eval': Resize -> CenterCrop (:217-231) -> (x,).  Each output uint8
    [n, 3, S, S]; `outs` may hold preallocated (e.g. pinned) CPU tensors.  Image i's randomness is
    keyed on (seed, i) only."""
    arrs = [_hwc(im) for im in images]
    n = len(arrs)
    k, nout = KINDS[kind]
    shape = (n, 3, size, size)
    outs = list(outs) if outs is not None else [torch.empty(shape, dtype=torch.uint8) for _ in range(nout)]
    if len(outs) != nout:
        raise ValueError(f"kind {kind!r} writes {nout} outputs")
    for t in outs:
        if tuple(t.shape) != shape or t.dtype != torch.uint8 or not t.is_contiguous() or t.device.type != "cpu":
            raise ValueError(f"output must be a contiguous CPU uint8 tensor of shape {shape}")
    ptrs = (_P * n)(*[a.ctypes.data for a in arrs])
    ws = (_I * n)(*[a.shape[1] for a in arrs])
    hs = (_I * n)(*[a.shape[0] for a in arrs])
    threads = threads or min(16, os.cpu_count() or 1)
    op = [t.data_ptr() for t in outs] + [None] * (3 - nout)
    rc = load().esh_transform_batch(k, ptrs, ws, hs, n, size, int(bool(is_crop)), int(seed) & (2 ** 64 - 1),
                                    int(threads), *op)
    _check(rc, "esh_transform_batch")
    return tuple(outs)


class TransformFixMatchNative:
    """Drop-in for the reference's TransformFixMatch(config, mean, std) (code/dataset.py:24-56), minus
    the normalisation (done on the device): __call__(img) -> (weak, strong) uint8 [3, S, S]."""

    def __init__(self, config, mean=None, std=None, seed=0):
        self.size = int(config.DATA.IMG_SIZE)
        self.is_crop = bool(getattr(config.DATA, "IS_CROP", True))
        self.seed = seed
        self.calls = 0

    def __call__(self, x):
        w, s = transform_batch([x], self.size, "fixmatch", self.is_crop, seed=self.seed + self.calls, threads=1)
        self.calls += 1
        return w[0], s[0]


class HostBatcher:
    """Double-buffered host producer: builds batch k+1 (uint8, pinned) on host threads while batch k is
    consumed, and copies it to the device on a side stream (code/dataset.py's DataLoader role).

    images: list of RGB images (PIL or HWC uint8); each batch draws `batch` of them uniformly (with a
    fresh per-batch seed) and next() returns the kind's views as device uint8 [batch, 3, S, S] tensors
    ('fixmatch': (weak, strong), 'comatch': (weak, strong_0, strong_1), 'labeled' / 'eval': (x,)),
    ready for es_patch_im2col_u8."""

    def __init__(self, images, batch, size, kind="fixmatch", is_crop=True, seed=0, threads=None, device="cuda"):
        self.images = [_hwc(im) for im in images]
        self.batch, self.size, self.kind, self.is_crop = batch, size, kind, is_crop
        self.seed, self.threads, self.device = seed, threads, device
        self.step = 0
        nout = KINDS[kind][1]
        pin = torch.cuda.is_available() and str(device).startswith("cuda")
        shape = (batch, 3, size, size)
        self._host = [[torch.empty(shape, dtype=torch.uint8, pin_memory=pin) for _ in range(nout)] for _ in range(2)]
        self._stream = torch.cuda.Stream(device=device) if pin else None
        self._events = [None, None]
        self._worker = None
        self._error = None
        self._submit(0)

    def _indices(self, step):
        g = np.random.default_rng((self.seed, step))
        return g.integers(0, len(self.images), self.batch)

    def _build(self, step):
        try:
            slot = step & 1
            if self._events[slot] is not None:  # the copy out of this slot two batches ago must be done
                self._events[slot].synchronize()
            idx = self._indices(step)
            transform_batch([self.images[i] for i in idx], self.size, self.kind, self.is_crop,
                            seed=(self.seed << 32) ^ step, threads=self.threads, outs=self._host[slot])
        except BaseException as e:  # surfaced by next()
            self._error = e

    def _submit(self, step):
        self._worker = threading.Thread(target=self._build, args=(step,), daemon=True)  # ctypes drops the GIL
        self._worker.start()

    def next(self):
        """The next batch on the device (the copy is ordered before any later work on the caller's stream)."""
        self._worker.join()
        if self._error is not None:
            raise self._error
        slot = self.step & 1
        bufs = self._host[slot]
        if self._stream is None:
            out = tuple(b.clone() for b in bufs)
        else:
            cur = torch.cuda.current_stream(self.device)
            self._stream.wait_stream(cur)
            with torch.cuda.stream(self._stream):
                out = tuple(b.to(self.device, non_blocking=True) for b in bufs)
                ev = torch.cuda.Event()
                ev.record(self._stream)
            self._events[slot] = ev
            cur.wait_stream(self._stream)
            for d in out:
                d.record_stream(cur)
        self.step += 1
        self._submit(self.step)
        return out


# ---- the device input path: the plan on the host, the pixels on the GPU (csrc/device_aug.hip) ------------
_dev = None


def _device():
    """libendossl_hip.so, once its three plan entries are known to be the host library's and this module's."""
    global _dev
    if _dev is None:
        from . import _lib
        lib = _lib.load()
        load()
        for cls, _, query, _ in _PLANS.values():
            if getattr(lib, query)() != ctypes.sizeof(cls):
                raise HostLibraryError(f"{query}() is {getattr(lib, query)()} bytes in the device library, "
                                       f"{ctypes.sizeof(cls)} in the host library")
        _dev = lib
    return _dev


def resize_side(size, is_crop=True):
    """The side TransformFixMatch resizes to: int(1.2 S) before CenterCrop(S) with IS_CROP, else S."""
    return int(size * 1.2) if is_crop else size


def aug_plan_from_draws(size, flip, top, left, ops, v, applied, neg, rect):
    """One AugEntry's strong-chain fields from explicit draws (two op slots; ops by name or pool index)."""
    ops = [POOL.index(o) if isinstance(o, str) else int(o) for o in ops]
    e = AugEntry()
    arr = lambda xs, k: (_I * k)(*[int(x) for x in xs])  # noqa: E731
    _check(load().esh_aug_plan_from_draws(int(size), int(flip), int(top), int(left), arr(ops, 2), arr(v, 2),
                                          arr(applied, 2), arr(neg, 2), arr(rect, 4), ctypes.addressof(e)),
           "esh_aug_plan_from_draws")
    return e


def jitter_plan_from_draws(order, factors=(1.0, 1.0, 1.0), hue=0.0, gray=False, flip=False, applied=True):
    """One AugJitter from explicit draws: order = 3 or 4 ops (JITTER names or indices; 'hue' only among 4),
    factors = brightness, contrast, saturation, hue = adjust_hue's factor in [-0.5, 0.5]."""
    order = [JITTER.index(o) if isinstance(o, str) else int(o) for o in order]
    j = AugJitter()
    _check(load().esh_jitter_plan_from_draws(int(bool(applied)), len(order), (_I * len(order))(*order),
                                             (ctypes.c_float * 3)(*[float(f) for f in factors]), float(hue),
                                             int(bool(gray)), int(bool(flip)), ctypes.addressof(j)),
           "esh_jitter_plan_from_draws")
    return j


def labeled_plan_from_draws(size, is_crop, hflip, vflip, angle, order=(0, 1, 2), factors=(1.0, 1.0, 1.0)):
    """One LabEntry's transform fields from explicit draws (angle in degrees; order / factors as above, three
    ops); its frame and resize fields are empty: device_transform_batch(plans=...) fills them."""
    order = [JITTER.index(o) if isinstance(o, str) else int(o) for o in order]
    e = LabEntry()
    _check(load().esh_labeled_plan_from_draws(int(size), int(bool(is_crop)), int(bool(hflip)), int(bool(vflip)),
                                              float(angle), (_I * len(order))(*order),
                                              (ctypes.c_float * 3)(*[float(f) for f in factors]), ctypes.addressof(e)),
           "esh_labeled_plan_from_draws")
    return e


def fixmatch_device_plan(ws, hs, size, is_crop=True, seed=0, frame_offs=None, entries=None, coeffs=None):
    """The plan of transform_batch(kind='fixmatch') for frames of sizes ws x hs and the same (seed, index).

    Returns (entries, coeffs, used): entries a uint8 array [n, ENTRY_BYTES] (view it with
    plan_entries()), coeffs an int32 array whose first `used` values are the resize tables.  `entries` /
    `coeffs` may be preallocated (e.g. numpy views of pinned tensors); a coeffs buffer that is too small is
    replaced by a fresh array.  frame_offs: each frame's byte offset in the arena (default: packed in order)."""
    return device_plan("fixmatch", ws, hs, size, is_crop, seed, frame_offs, entries, coeffs)


def comatch_device_plan(ws, hs, size, is_crop=True, seed=0, frame_offs=None, entries=None, coeffs=None):
    """The plan of transform_batch(kind='comatch'): fixmatch_device_plan's contract with CoEntry entries
    (plan_entries(entries, 'comatch'))."""
    return device_plan("comatch", ws, hs, size, is_crop, seed, frame_offs, entries, coeffs)


def labeled_device_plan(ws, hs, size, is_crop=True, seed=0, frame_offs=None, entries=None, coeffs=None):
    """The plan of transform_batch(kind='labeled'): fixmatch_device_plan's contract with LabEntry entries
    (plan_entries(entries, 'labeled'))."""
    return device_plan("labeled", ws, hs, size, is_crop, seed, frame_offs, entries, coeffs)


def device_plan(kind, ws, hs, size, is_crop=True, seed=0, frame_offs=None, entries=None, coeffs=None):
    """The plan of transform_batch(kind) ('eval' shares 'fixmatch's): see fixmatch_device_plan."""
    cls, _, _, fn = _PLANS[kind]
    ws = np.ascontiguousarray(ws, np.int32)
    hs = np.ascontiguousarray(hs, np.int32)
    n = len(ws)
    if entries is None:
        entries = np.zeros((n, ctypes.sizeof(cls)), np.uint8)
    if coeffs is None:
        coeffs = np.zeros(4096, np.int32)
    offs = None if frame_offs is None else np.ascontiguousarray(frame_offs, np.int64)
    used = ctypes.c_size_t()
    plan = getattr(load(), fn)
    for _ in range(2):
        rc = plan(_ptr(ws), _ptr(hs), None if offs is None else _ptr(offs), n, int(size), int(bool(is_crop)),
                  int(seed) & (2 ** 64 - 1), _ptr(entries), _ptr(coeffs), coeffs.size, ctypes.byref(used))
        if rc == 3 and used.value > coeffs.size:  # sized by the refused call
            coeffs = np.zeros(used.value, np.int32)
            continue
        break
    _check(rc, fn)
    return entries, coeffs, used.value


def plan_entries(entries, kind="fixmatch"):
    """A uint8 plan buffer as a ctypes array of the kind's entry type (sharing its memory)."""
    cls = _PLANS[kind][0]
    n = entries.size // ctypes.sizeof(cls)
    return (cls * n).from_buffer(entries)


def _dev_u8(a, device):
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(device)


def device_strong(weak, entries, workspace=None):
    """The strong chain (flip -> reflect crop -> two ops -> Cutout) of a device uint8 [n, 3, S, S] batch
    under explicit plans (a list of AugEntry or a plan buffer): es_aug_strong_u8."""
    from . import _lib
    lib = _device()
    n, _, S, _ = weak.shape
    if not isinstance(entries, np.ndarray):
        entries = np.frombuffer(bytearray(b"".join(bytes(e) for e in entries)), np.uint8)
    if entries.size != n * ENTRY_BYTES:
        raise ValueError("one plan entry per image")
    ent = _dev_u8(entries, weak.device)
    nbytes = lib.es_aug_strong_workspace(n, S)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=weak.device)
    strong = torch.empty_like(weak)
    _lib.call("es_aug_strong_u8", _lib.ptr(weak.contiguous()), _lib.ptr(ent), n, S, _lib.ptr(strong),
              _lib.ptr(workspace), workspace.numel(), _lib.stream())
    return strong


def device_jitter(x, plans):
    """One jitter chain (the ColorJitter ops in each plan's order, grayscale, flip) over a device uint8
    [n, 3, S, S] batch under explicit plans (a list of AugJitter): es_aug_jitter_u8."""
    from . import _lib
    _device()
    n, _, S, _ = x.shape
    if len(plans) != n:
        raise ValueError("one plan per image")
    ent = _dev_u8(np.frombuffer(bytearray(b"".join(bytes(j) for j in plans)), np.uint8), x.device)
    out = torch.empty_like(x, memory_format=torch.contiguous_format)
    _lib.call("es_aug_jitter_u8", _lib.ptr(x.contiguous()), _lib.ptr(ent), n, S, _lib.ptr(out), _lib.stream())
    return out


# the device calls by kind: (entry point, workspace query, views)
_CALLS = {"fixmatch": ("es_aug_fixmatch_u8", "es_aug_fixmatch_workspace", 2),
          "eval": ("es_aug_fixmatch_u8", "es_aug_fixmatch_workspace", 1),
          "comatch": ("es_aug_comatch_u8", "es_aug_comatch_workspace", 3),
          "labeled": ("es_aug_labeled_u8", "es_aug_labeled_workspace", 1)}


def _check_kind(kind):
    if kind not in _CALLS:
        raise ValueError(f"the device input path runs {sorted(_CALLS)}, not {kind!r}")


def _run_device(kind, frames, frames_bytes, ent, coef, used, n, size, is_crop, max_h, workspace, device):
    """The kind's es_aug_*_u8 call on the current stream over device buffers; returns the views."""
    from . import _lib
    fn, _, nout = _CALLS[kind]
    outs = [torch.empty((n, 3, size, size), dtype=torch.uint8, device=device) for _ in range(nout)]
    views = [_lib.ptr(t) for t in outs] + ([None] if kind == "eval" else [])  # eval: fixmatch without a strong view
    _lib.call(fn, _lib.ptr(frames), frames_bytes, _lib.ptr(ent), _lib.ptr(coef) if used else None, used, n, size,
              int(bool(is_crop)), max_h, *views, _lib.ptr(workspace), workspace.numel(), _lib.stream())
    return tuple(outs)


def device_transform_batch(images, size, kind="fixmatch", is_crop=True, seed=0, device="cuda", plans=None):
    """transform_batch(kind='fixmatch' | 'eval' | 'comatch' | 'labeled') with the pixels made on the GPU: the
    frames are copied to the device as they are, the host only builds the plan.  Returns device uint8
    [n, 3, S, S] tensors, byte for byte transform_batch's for the same seed.
    plans: one explicit entry per image (e.g. labeled_plan_from_draws) whose transform fields replace the seeded
    draws; the frame and resize fields stay the plan's own."""
    _check_kind(kind)
    lib = _device()
    arrs = [_hwc(im) for im in images]
    n = len(arrs)
    ws = [a.shape[1] for a in arrs]
    hs = [a.shape[0] for a in arrs]
    entries, coeffs, used = device_plan(kind, ws, hs, size, is_crop, seed)
    if plans is not None:
        if len(plans) != n:
            raise ValueError("one plan per image")
        skip = AugHead.crop.offset + 4
        for i, e in enumerate(plans):
            entries[i, skip:] = np.frombuffer(bytes(e), np.uint8)[skip:]
    arena = np.concatenate([a.reshape(-1) for a in arrs])
    dev = torch.device(device)
    with torch.cuda.device(dev):
        nbytes = getattr(lib, _CALLS[kind][1])(n, size, int(bool(is_crop)), max(ws), max(hs))
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        coef = torch.from_numpy(coeffs[:max(used, 1)]).to(dev)
        return _run_device(kind, torch.from_numpy(arena).to(dev), arena.size, _dev_u8(entries, dev), coef, used, n,
                           size, is_crop, max(hs), workspace, dev)


def plan_and_copy(images, ws, hs, idx, size, is_crop, seed, entries, coeffs, arena=None, offsets=None, threads=1,
                  kind="fixmatch"):
    """The host's whole share of one device-path batch: frames images[idx] copied back to back into `arena` on
    `threads` host threads (or, with the frame set already on the device, `offsets` = every frame's offset
    there) and the plan written into `entries` / `coeffs` (numpy views, e.g. of pinned tensors).  Returns
    (arena bytes, coefficient count)."""
    ws, hs = np.ascontiguousarray(ws[idx], np.int32), np.ascontiguousarray(hs[idx], np.int32)
    if offsets is not None:
        offs, pos = offsets[idx], 0
    else:
        ptrs = np.fromiter((images[i].ctypes.data for i in idx), np.uint64, len(idx))
        offs = np.empty(len(idx), np.int64)
        used = ctypes.c_size_t()
        _check(load().esh_copy_frames(_ptr(ptrs), _ptr(ws), _ptr(hs), len(idx), _ptr(arena), arena.size, _ptr(offs),
                                      ctypes.byref(used), int(threads)), "esh_copy_frames")
        pos = used.value
    _, out, used = device_plan(kind, ws, hs, size, is_crop, seed=seed, frame_offs=offs, entries=entries, coeffs=coeffs)
    if out is not coeffs:
        raise ValueError(f"coefficient buffer of {coeffs.size} int32 is too small: {used} needed")
    return pos, used


class DeviceBatcher:
    """HostBatcher's contract (constructor, _indices, per-batch seed, next()) with the transforms on the GPU:
    next() returns the same bytes as HostBatcher.next() for the same seed.

    For each batch a host thread copies the chosen frames into a pinned arena, builds the plan
    (esh_*_device_plan) and sends arena, plan and coefficient tables on the side stream, event-ordered
    against the reuse of the pinned slot as HostBatcher's copies are; next() makes the caller's stream wait for
    that event and runs the kind's one es_aug_*_u8 call on it.
    resident=True uploads the whole frame set once; a step then sends only the plan and the tables.
    kind: 'fixmatch' -> (weak, strong), 'comatch' -> (weak, strong_0, strong_1), 'labeled' / 'eval' -> (x,)."""

    def __init__(self, images, batch, size, kind="fixmatch", is_crop=True, seed=0, threads=None, device="cuda",
                 resident=False):
        _check_kind(kind)
        self._lib = _device()
        self.images = [_hwc(im) for im in images]
        self.batch, self.size, self.kind, self.is_crop = batch, size, kind, is_crop
        self.seed, self.threads, self.device, self.resident = seed, threads, torch.device(device), resident
        self.step = 0
        self._ws = np.array([a.shape[1] for a in self.images], np.int32)
        self._hs = np.array([a.shape[0] for a in self.images], np.int32)
        nbytes = self._ws.astype(np.int64) * self._hs * 3
        self._max_h = int(self._hs.max())
        R = resize_side(size, is_crop)
        ks = lambda s: int(np.ceil(max(1.0, s / R))) * 2 + 1  # noqa: E731 -- precompute()'s kernel size
        sides = set(self._ws.tolist()) | set(self._hs.tolist())
        coef_cap = max(1, sum(R * (2 + ks(s)) for s in sides if s != R))
        with torch.cuda.device(self.device):
            wbytes = getattr(self._lib, _CALLS[kind][1])(batch, size, int(bool(is_crop)), int(self._ws.max()),
                                                         self._max_h)
            self._workspace = torch.empty(max(wbytes, 1), dtype=torch.uint8, device=self.device)
            if resident:
                self._offs = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
                self._frames = torch.from_numpy(np.concatenate([a.reshape(-1) for a in self.images])).to(self.device)
                arena_cap = 0
            else:
                arena_cap = batch * int(nbytes.max())
        self._host = [{"arena": torch.empty(max(arena_cap, 1), dtype=torch.uint8, pin_memory=True),
                       "entries": torch.empty(batch * ctypes.sizeof(_PLANS[kind][0]), dtype=torch.uint8,
                                              pin_memory=True),
                       "coeffs": torch.empty(coef_cap, dtype=torch.int32, pin_memory=True),
                       "used": 0, "bytes": 0} for _ in range(2)]
        self._stream = torch.cuda.Stream(device=self.device)
        self._events = [None, None]
        self._worker = None
        self._error = None
        self._submit(0)

    def _indices(self, step):
        g = np.random.default_rng((self.seed, step))
        return g.integers(0, len(self.images), self.batch)

    def _build(self, step):
        try:
            slot = step & 1
            if self._events[slot] is not None:  # the copies out of this slot two batches ago must be done
                self._events[slot].synchronize()
            h = self._host[slot]
            idx = self._indices(step)
            h["bytes"], h["used"] = plan_and_copy(self.images, self._ws, self._hs, idx, self.size, self.is_crop,
                                                  (self.seed << 32) ^ step, h["entries"].numpy(), h["coeffs"].numpy(),
                                                  arena=None if self.resident else h["arena"].numpy(),
                                                  offsets=self._offs if self.resident else None,
                                                  threads=self.threads or 4, kind=self.kind)
            # the copies start here, on the side stream, so they run under the step that is still computing
            with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
                ent = h["entries"].to(self.device, non_blocking=True)
                coef = h["coeffs"][:max(h["used"], 1)].to(self.device, non_blocking=True)
                frames = None if self.resident else h["arena"][:h["bytes"]].to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self._stream)
            h["sent"] = (ent, coef, frames)
            self._events[slot] = ev
        except BaseException as e:  # surfaced by next()
            self._error = e

    def _submit(self, step):
        self._worker = threading.Thread(target=self._build, args=(step,), daemon=True)  # ctypes drops the GIL
        self._worker.start()

    def next(self):
        """The next batch on the device, produced on the caller's current stream (no host synchronisation)."""
        self._worker.join()
        if self._error is not None:
            raise self._error
        slot = self.step & 1
        h = self._host[slot]
        ent, coef, frames = h["sent"]
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self._events[slot])
            for d in (ent, coef, frames):
                if d is not None:
                    d.record_stream(cur)
            if self.resident:
                frames = self._frames
            out = _run_device(self.kind, frames, frames.numel(), ent, coef, h["used"], self.batch, self.size,
                              self.is_crop, self._max_h, self._workspace, self.device)
        h["sent"] = None
        self.step += 1
        self._submit(self.step)
        return out
