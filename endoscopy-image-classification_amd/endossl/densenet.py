"""Native DenseNet-161 -- the backbone of `local_semisupervised.yaml` (FixMatch), `local_reproduce.yaml` and
`kaggle_supervised_patho.yaml` (supervised) -- with its dense blocks computed in place.

Reference: `build_model` -> timm `densenet161` (`code/build.py:196-197,218-220`, timm==0.5.4, absent from this image:
the architecture is restated here, it is torchvision's): features.conv0 7x7/2 -> norm0 -> ReLU -> max-pool 3/2 ->
four dense blocks of 6 / 12 / 36 / 24 layers (norm1 -> ReLU -> conv1 1x1 to bn_size * growth = 192 -> norm2 -> ReLU ->
conv2 3x3 to growth = 48 channels, concatenated after the layer's input) with transitions between them (norm -> ReLU
-> conv 1x1 to half the channels -> avg-pool 2/2) -> norm5 -> ReLU -> global average pool -> classifier.  `model(x) ->
logits`; torchvision's state_dict (names and order), so checkpoints interchange.  It is the one backbone the
reference's trainers name (`code/fixmatch.py:45-48,213-216`: `model.classifier` under IS_FREEZE); `model.fc` is an
alias of it here, so the trainers' `.fc` paths work unchanged.

MI355X layout (NativeConformer's plumbing: one flat fp32 parameter buffer, NHWC maps, conv.hip / conv_bf16.hip):

  * a dense block is ONE buffer [N, H, W, ld], ld = C_out + 16, zero-filled.  The block input lands in channels
    [0, C_0); layer i's conv1 reads the prefix [0, C_i) as a strided map with norm1 + ReLU applied in its gathers
    (es_conv2d_fwd_bf16_bnin_ex) and its conv2 writes the slice [C_i, C_i + 48) through the conv's output strides:
    no torch.cat, no normalised map;
  * every later norm1 normalises the same channels with the same batch statistics, so a channel's mean / rstd are
    computed once per block (from conv2's epilogue partials; the block input by one strided pass) into arrays the
    block shares; each BatchNorm keeps its own affine parameters and running buffers, which one table-driven launch
    per block updates.  The transition's norm and norm5 read the same arrays.  Eval mode: each BatchNorm's own
    running statistics;
  * the bf16 conv kernels take channel counts % 32.  Half the prefixes are 16 (mod 32) wide and conv2 has 48
    outputs: the packed weight images are zero-padded instead (conv1 to roundup32(C_i) inputs, conv2 to 64 outputs).
    The 16 extra input channels are the next slice -- zeros or real data, finite either way -- and meet zero weights
    AND a zero gamma / beta (the flat layout's 64-float rounding leaves >= 16 zero floats after such a norm1's
    parameters: asserted at build); the 16 extra outputs are zeros written ahead of the slice and overwritten by the
    next layer, which is why ld = C_out + 16.  Padded weight gradients land in a scratch arena and one launch per
    block copies the true rows into the flat gradient;
  * the backward runs the layers in reverse over one fp32 gradient buffer of the block's geometry (a prefix
    channel is accumulated into by up to 36 layers): conv2's weight and data gradients from the strided slice,
    norm2's backward, conv1's gradients, and norm1's mask-rebuilding backward accumulating into the prefix
    (es_bn2d_bwd_recompute_ld_ex).  The whole dense trunk is one autograd Function (_DenseTrunkFn): autograd would
    cast an fp32 gradient buffer handed between two Functions to the bf16 buffer's dtype.

`set_conv_precision("fp32")` runs the same structure on conv.hip's fp32 kernels with fp32 buffers, no padding and
norm1 / norm2 materialised per layer (es_bn2d_apply_ld_ex): the parity anchor.
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import _lib, dist
from ._lib import call, ptr
from .conformer import (BN_MOMENTUM, CONV_BF16, MAP_BF16, NativeConformer, _fl, _join_queued, _Map, _map_dtype,
                        _MaxPoolFn, _own, _rup, _s, bn, conv)

BN_EPS = 1e-5  # nn.BatchNorm2d's default, every BatchNorm of the network


class DenseNetConfig:
    """timm / torchvision DenseNet; the defaults are densenet161's."""

    def __init__(self, block_config=(6, 12, 36, 24), growth=48, bn_size=4, init_features=96, num_classes=23,
                 img_size=224):
        self.block_config = tuple(int(n) for n in block_config)
        self.growth, self.bn_size, self.init_features = int(growth), int(bn_size), int(init_features)
        self.num_classes, self.img_size = num_classes, img_size
        if not self.block_config or min(self.block_config) < 1:
            raise ValueError(f"block_config {block_config!r}: at least one block of at least one layer")
        if self.growth % 16:
            raise ValueError(f"growth {growth}: the slices start at 16-channel boundaries (growth % 16 == 0)")
        if self.mid % 32:
            raise ValueError(f"bn_size * growth = {self.mid}: the bottleneck map feeds the bf16 convs (% 32 == 0)")
        for b, (c0, n, cout) in enumerate(self.blocks(), 1):
            last = b == len(self.block_config)
            widths = [("input", c0), ("output", cout)] + ([] if last else [("transition output", cout // 2)])
            for what, c in widths:
                if c % 32:
                    raise ValueError(f"dense block {b}: {what} width {c} is not a multiple of 32")

    @property
    def mid(self):
        """conv1's output channels (bn_size * growth = 192)."""
        return self.bn_size * self.growth

    @property
    def slice_pad(self):
        """Channels a padded conv2 writes beyond its slice (the block buffers' extra width)."""
        return _rup(self.growth, 32) - self.growth

    def blocks(self):
        """(input width, layers, output width) per dense block."""
        out, c = [], self.init_features
        for i, n in enumerate(self.block_config):
            out.append((c, n, c + n * self.growth))
            c = (c + n * self.growth) // 2
        return out

    @property
    def num_features(self):
        return self.blocks()[-1][2]

    @property
    def dim(self):
        return self.num_features


DENSENET161 = dict(block_config=(6, 12, 36, 24), growth=48, bn_size=4, init_features=96)


def _bn_entries(pre, C):
    return [(pre + "weight", (C,), "p"), (pre + "bias", (C,), "p"), (pre + "running_mean", (C,), "rm"),
            (pre + "running_var", (C,), "rv"), (pre + "num_batches_tracked", (), "nbt")]


def densenet_layout(cfg):
    """(name, shape, kind) in torchvision densenet's state_dict order."""
    f0, g, mid = cfg.init_features, cfg.growth, cfg.mid
    out = [("features.conv0.weight", (f0, 3, 7, 7), "p")] + _bn_entries("features.norm0.", f0)
    nb = len(cfg.block_config)
    for b, (c0, n, cout) in enumerate(cfg.blocks(), 1):
        for l in range(n):
            pre, c = f"features.denseblock{b}.denselayer{l + 1}.", c0 + l * g
            out += _bn_entries(pre + "norm1.", c) + [(pre + "conv1.weight", (mid, c, 1, 1), "p")]
            out += _bn_entries(pre + "norm2.", mid) + [(pre + "conv2.weight", (g, mid, 3, 3), "p")]
        if b < nb:
            pre = f"features.transition{b}."
            out += _bn_entries(pre + "norm.", cout) + [(pre + "conv.weight", (cout // 2, cout, 1, 1), "p")]
    out += _bn_entries("features.norm5.", cfg.num_features)
    out += [("classifier.weight", (cfg.num_classes, cfg.num_features), "p"), ("classifier.bias", (cfg.num_classes,), "p")]
    return out


def init_densenet_(flat, layout, offs, generator=None):
    """torchvision / timm DenseNet.__init__: Conv2d kaiming_normal_ (fan_in, gain sqrt 2), BatchNorm 1 / 0, the
    classifier at nn.Linear's default weight (U(+-1/sqrt(fan_in))) with bias 0."""
    for name, shape, kind in layout:
        if kind != "p":
            continue
        t = flat[offs[name]:offs[name] + math.prod(shape)].view(shape)
        if len(shape) == 4:
            t.normal_(0.0, math.sqrt(2.0 / (shape[1] * shape[2] * shape[3])), generator=generator)
        elif name == "classifier.weight":
            bound = 1.0 / math.sqrt(shape[1])
            t.uniform_(-bound, bound, generator=generator)
        elif name.endswith("weight"):
            t.fill_(1.0)
        else:
            t.zero_()


# ---- device tables (the entry layouts of csrc/densenet.hip) ----------------------------------------------------
class _PackEntry(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("wp", ctypes.c_void_p), ("wt", ctypes.c_void_p), ("Cout", ctypes.c_int),
                ("Cin", ctypes.c_int), ("T", ctypes.c_int), ("Cout_p", ctypes.c_int), ("Cin_p", ctypes.c_int),
                ("pad", ctypes.c_int)]


class _UnpadEntry(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("Cout_p", ctypes.c_int), ("Cin_p", ctypes.c_int),
                ("Cout", ctypes.c_int), ("Cin", ctypes.c_int), ("T", ctypes.c_int), ("pad", ctypes.c_int)]


class _RunEntry(ctypes.Structure):
    _fields_ = [("rm", ctypes.c_void_p), ("rv", ctypes.c_void_p), ("nbt", ctypes.c_void_p), ("C", ctypes.c_int),
                ("off", ctypes.c_int)]


def _table(entries, size_fn, device):
    esz = getattr(_lib.load(), size_fn)()
    if esz != ctypes.sizeof(type(entries[0])):
        raise _lib.EndosslLibraryError(f"{size_fn}() = {esz}, the Python entry has {ctypes.sizeof(type(entries[0]))}")
    raw = b"".join(bytes(e) for e in entries)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def _at(t, elems):
    """Device address of element `elems` of tensor t."""
    return ptr(t) + t.element_size() * elems


class _Blk:
    """What one dense block's forward leaves for its backward."""
    __slots__ = ("buf", "geom", "ld", "c0", "n", "cout", "mean", "rstd", "m2", "y1", "st2", "b")


class _DenseTrunkFn(torch.autograd.Function):
    """Pooled stem map [N, H, W, init_features] -> relu(norm5(last block)) [N, h, w, num_features]: every dense block,
    transition and norm5 (module docstring).  One Function: the blocks hand each other fp32 gradient buffers."""

    @staticmethod
    def forward(ctx, x0, m):
        keep = bool(ctx.needs_input_grad[0])
        out, blks = m._dense_forward(x0.contiguous(), keep)
        ctx.m, ctx.blks, ctx.train = m, blks, m.training
        return out

    @staticmethod
    def backward(ctx, dout):
        _own(dout)
        if not ctx.train or ctx.blks is None:
            raise NotImplementedError("NativeDenseNet's backward runs through a train-mode forward (batch statistics)")
        blks, ctx.blks = ctx.blks, None
        return ctx.m._dense_backward(blks, dout.contiguous()), None


class _HeadFn(torch.autograd.Function):
    """AdaptiveAvgPool2d(1) + flatten + classifier: conformer._ConvHeadFn with the Linear on the tiled fp32 GEMMs
    (es_dense_wide_*): 2208 features are past es_dense_fwd's 2048."""

    @staticmethod
    def forward(ctx, x, m, anchor=None):
        N, H, W, C = x.shape
        if H != W:
            raise ValueError(f"the global-pool head expects square maps, got {H}x{W}")
        ncls = m.cfg.num_classes
        pooled = torch.empty(N, C, device=x.device)
        call("es_avgpool2d_fwd_ex", ptr(x.contiguous()), N, H, W, C, H, ptr(pooled), _fl(x), _s())
        logits = torch.empty(N, ncls, device=x.device)
        call("es_dense_wide_fwd", ptr(pooled), C, ptr(m.pview("classifier.weight")), ptr(m.pview("classifier.bias")),
             ptr(logits), ncls, N, C, ncls, 0, 0.0, None, 1.0, _s())
        ctx.save_for_backward(pooled)
        ctx.m, ctx.geom, ctx.dt = m, (N, H, W, C), x.dtype
        return logits

    @staticmethod
    def backward(ctx, dl):
        _own(dl)
        (pooled,) = ctx.saved_tensors
        m = ctx.m
        N, H, W, C = ctx.geom
        ncls = m.cfg.num_classes
        dl = dl.contiguous()
        frozen = getattr(m, "frozen_trunk", False)  # IS_FREEZE: the classifier's parameters only
        dpooled = None if frozen else torch.empty(N, C, device=dl.device)
        ws = torch.empty(_lib.load().es_dense_wide_bwd_workspace(N, C, ncls, 0 if frozen else 1), device=dl.device)
        call("es_dense_wide_bwd", ptr(dl), ncls, None, 0, 0, 0.0, None, 1.0, ptr(pooled), C,
             ptr(m.pview("classifier.weight")), ptr(dpooled), C, 0, ptr(m.gview("classifier.weight")),
             ptr(m.gview("classifier.bias")), N, C, ncls, ptr(ws), _s())
        if frozen:
            return None, None, None
        dx = torch.empty(N, H, W, C, dtype=ctx.dt, device=dl.device)
        call("es_avgpool2d_bwd_ex", ptr(dpooled), N, H, W, C, H, ptr(dx), 0, _fl(dx) << 1, _s())
        return dx, None, None


class NativeDenseNet(NativeConformer):
    """DenseNet-161 (or any DenseNetConfig) whose compute runs in libendossl_hip.so; state_dict identical to
    torchvision's densenet161.  Shares NativeConformer's flat-parameter plumbing (views, BatchNorm buffers, device
    moves, deepcopy, eval mode on the running statistics, set_conv_precision)."""

    def __init__(self, cfg=None, seed=None, **kw):
        nn.Module.__init__(self)
        self.cfg = cfg if cfg is not None else DenseNetConfig(**{**DENSENET161, **kw})
        self.layout = densenet_layout(self.cfg)
        self.offs, o = {}, 0
        for name, shape, kind in self.layout:
            if kind == "p":
                self.offs[name] = o
                o = _rup(o + math.prod(shape), 64)
        self.numel = o
        self.shapes = {name: shape for name, shape, _ in self.layout}
        self._check_padding()
        flat = torch.zeros(self.numel, dtype=torch.float32)
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        init_densenet_(flat, self.layout, self.offs, generator=gen)
        self._build(flat, device=torch.device("cpu"))
        self.version = 0
        self.cur_n = 0
        self.conv_bf16 = CONV_BF16

    def padded_norms(self):
        """(norm1 prefix, C, roundup32(C)) of every dense layer whose conv1 reads a zero-padded prefix."""
        out, g = [], self.cfg.growth
        for b, (c0, n, _) in enumerate(self.cfg.blocks(), 1):
            for l in range(n):
                c = c0 + l * g
                if c % 32:
                    out.append((f"features.denseblock{b}.denselayer{l + 1}.norm1.", c, _rup(c, 32)))
        return out

    def _check_padding(self):
        """A padded conv1 gathers roundup32(C) - C channels past its norm1: their gamma / beta are the flat
        layout's alignment padding, which must be there (and stays zero: no gradient is ever written to it)."""
        for pre, c, cp in self.padded_norms():
            for nm in (pre + "weight", pre + "bias"):
                room = _rup(self.offs[nm] + c, 64) - (self.offs[nm] + c)
                assert room >= cp - c, f"{nm}: {room} padding floats after {c} channels, the padded conv reads {cp - c}"

    def _build(self, flat, device, buffers=None):
        super()._build(flat, device, buffers)
        self._dn = {}  # device tables / arenas keyed by what they point into

    @property
    def map_bf16(self):
        """bf16 activation maps (and block buffers) after the stem's max-pool: every later conv runs on the bf16
        kernels (padded where a channel count is 16 mod 32)."""
        return bool(self.conv_bf16 and MAP_BF16)

    @property
    def fc(self):  # the trainers' name for the classifier (IS_FREEZE's trainable part): the same module
        return self._modules["classifier"]

    def no_weight_decay(self):
        return set()

    def _pack(self):  # no transformer weight images
        return None

    # ---- packed weights / tables ----------------------------------------------------------------------------
    def _convs(self):
        """(weight name, Cout, Cin, k, Cout_p, Cin_p) of every conv after the stem."""
        out = []
        for name, shape, kind in self.layout:
            if kind == "p" and len(shape) == 4 and name != "features.conv0.weight":
                out.append((name, shape[0], shape[1], shape[2], _rup(shape[0], 32), _rup(shape[1], 32)))
        return out

    def _wimg(self, name):
        """(wp, wt, Cout_p, Cin_p) of conv weight `name`: the zero-padded bf16 images, all packed in one launch per
        parameter version (es_conv2d_pack_bf16_pad_multi)."""
        st = self._dn.get("pack")
        if st is None:
            dev, convs = self.flat.device, self._convs()
            total = sum(cop * cip * k * k for _, _, _, k, cop, cip in convs)
            arena = torch.zeros(2 * total, dtype=torch.bfloat16, device=dev)
            imgs, ents, o, mx = {}, [], 0, 0
            for name_, co, ci, k, cop, cip in convs:
                n = cop * cip * k * k
                wp, wt = arena[o:o + n], arena[total + o:total + o + n]
                imgs[name_] = (wp, wt, cop, cip)
                ents.append(_PackEntry(ptr(self.pview(name_)), ptr(wp), ptr(wt), co, ci, k * k, cop, cip, 0))
                o, mx = o + n, max(mx, n)
            st = self._dn["pack"] = {"imgs": imgs, "tab": _table(ents, "es_conv_pack_pad_entry_size", dev),
                                     "n": len(ents), "mx": mx, "version": None, "arena": arena}
        if st["version"] != self.version:
            call("es_conv2d_pack_bf16_pad_multi", ptr(st["tab"]), st["n"], st["mx"], _s())
            st["version"] = self.version
        return st["imgs"][name]

    def _dw_slot(self, b, name):
        """Where conv `name` of block b (0 = none: a transition) writes its weight gradient: the flat gradient, or --
        padded -- its slot of the block's scratch arena (copied out by _dw_unpad)."""
        key = ("dw", b, self.flat_grad.data_ptr())
        st = self._dn.get(key)
        if st is None:
            pre = f"features.denseblock{b}."
            pads = [c for c in self._convs() if c[0].startswith(pre) and (c[4] != c[1] or c[5] != c[2])]
            total = sum(cop * cip * k * k for _, _, _, k, cop, cip in pads)
            arena = torch.zeros(max(total, 1), device=self.flat.device)
            slots, ents, o, mx = {}, [], 0, 1
            for name_, co, ci, k, cop, cip in pads:
                slots[name_] = arena[o:o + cop * cip * k * k]
                ents.append(_UnpadEntry(ptr(slots[name_]), ptr(self.gview(name_)), cop, cip, co, ci, k * k, 0))
                o, mx = o + cop * cip * k * k, max(mx, co * ci * k * k)
            tab = _table(ents, "es_dw_unpad_entry_size", self.flat.device) if ents else None
            st = self._dn[key] = {"slots": slots, "tab": tab, "n": len(ents), "mx": mx, "arena": arena}
        return st["slots"].get(name, self.gview(name))

    def _dw_unpad(self, b):
        st = self._dn.get(("dw", b, self.flat_grad.data_ptr()))
        if st is not None and st["n"]:
            call("es_dw_unpad_multi", ptr(st["tab"]), st["n"], st["mx"], _s())

    def _running_update(self, b, blk, consumer):
        """One launch: the running buffers of block b's norm1s and of `consumer` (the transition's norm / norm5),
        all over the block's shared statistics."""
        st = self._dn.get(("run", b))
        if st is None:
            ents, g = [], self.cfg.growth
            pres = [(f"features.denseblock{b}.denselayer{l + 1}.norm1.", blk.c0 + l * g) for l in range(blk.n)]
            for pre, c in pres + [(consumer, blk.cout)]:
                rm, rv, nbt = self.bn_buffers(pre)
                ents.append(_RunEntry(ptr(rm), ptr(rv), ptr(nbt), c, 0))
            st = self._dn[("run", b)] = (_table(ents, "es_bn_running_entry_size", self.flat.device), len(ents))
        rows = blk.geom[0] * blk.geom[1] * blk.geom[2]
        call("es_bn2d_running_multi", ptr(st[0]), st[1], blk.cout, ptr(blk.mean), ptr(blk.m2), rows, BN_MOMENTUM, _s())

    # ---- BatchNorm + ReLU + 1 x 1 conv over a buffer prefix (a layer's norm1 / conv1, a transition's norm / conv)
    def _norm_arrays(self, blk, bnpre, C, Cp):
        """mean / rstd the gathers of a conv over [0, Cp) read: the block's shared arrays (train), or this
        BatchNorm's running statistics zero-padded to Cp (eval)."""
        if self.training:
            return blk.mean, blk.rstd
        rm, rv, _ = self.bn_buffers(bnpre)
        mean, rstd = torch.empty(Cp, device=rm.device), torch.empty(Cp, device=rm.device)
        call("es_bn2d_eval_stats", ptr(rm), ptr(rv), C, Cp, BN_EPS, ptr(mean), ptr(rstd), _s())
        return mean, rstd

    def _prefix_conv_fwd(self, blk, C, bnpre, wname, Cout, part=None):
        """conv1x1(relu(bn(buf[..., :C]))) -> dense [N, H, W, Cout]."""
        N, H, W = blk.geom
        ld, buf, dev = blk.ld, blk.buf, blk.buf.device
        gam, bet = self.pview(bnpre + "weight"), self.pview(bnpre + "bias")
        y = torch.empty(N, H, W, Cout, dtype=buf.dtype, device=dev)
        if self.conv_bf16:
            wp, _, _, Cp = self._wimg(wname)
            mean, rstd = self._norm_arrays(blk, bnpre, C, Cp)
            call("es_conv2d_fwd_bf16_bnin_ex", ptr(buf), N, H, W, Cp, H * W * ld, W * ld, ld, 1, ptr(wp), None, Cout, 1, 1,
                 1, 0, ptr(y), H * W * Cout, W * Cout, Cout, 0, ptr(part), _fl(buf) | (_fl(y) << 1), ptr(mean), ptr(rstd),
                 ptr(gam), ptr(bet), _s())
            return y
        mean, rstd = self._norm_arrays(blk, bnpre, C, C)
        a = torch.empty(N, H, W, C, device=dev)
        call("es_bn2d_apply_ld_ex", ptr(buf), ld, N * H * W, C, ptr(mean), ptr(rstd), ptr(gam), ptr(bet), 1, ptr(a), C, 0,
             _s())
        call("es_conv2d_fwd", ptr(a), N, H, W, C, H * W * C, W * C, C, 1, ptr(self.pview(wname)), None, Cout, 1, 1, 1, 0,
             ptr(y), H * W * Cout, W * Cout, Cout, 0, _s())
        return y

    def _dw_f32(self, x, N, H, W, Cin, dy_ptr, syn, syh, syw, Cout, k, p, dw):
        lib = _lib.load()
        M = N * H * W
        tiles = lib.es_conv2d_dw_tiles(Cout, Cin, k, k)
        splits = max(1, min(-(-M // 64), -(-2048 // tiles)))
        ws = torch.empty(lib.es_conv2d_bwd_weight_workspace(Cout, Cin, k, k, splits), device=x.device)
        call("es_conv2d_bwd_weight", ptr(x), N, H, W, Cin, H * W * Cin, W * Cin, Cin, 1, dy_ptr, syn, syh, syw, Cout, k, k,
             1, p, splits, ptr(ws), ptr(dw), 0, _s())

    def _prefix_conv_bwd(self, b, blk, C, bnpre, wname, dy, gbuf):
        """The backward of _prefix_conv_fwd: dy dense [N, H, W, Cout] -> the conv's weight gradient, the BatchNorm's
        parameter gradients, and d(buf[..., :C]) ACCUMULATED into the fp32 gradient buffer's prefix."""
        N, H, W = blk.geom
        ld, buf, dev, rows = blk.ld, blk.buf, blk.buf.device, N * H * W
        Cout = dy.shape[3]
        lib = _lib.load()
        gam, bet = self.pview(bnpre + "weight"), self.pview(bnpre + "bias")
        dw = self._dw_slot(b, wname)
        if self.conv_bf16:
            _, wt, _, Cp = self._wimg(wname)
            ws = torch.empty(lib.es_conv2d_bwd_weight_bf16_workspace(rows, Cout, Cp, 1, 1, 0), device=dev)
            call("es_conv2d_bwd_weight_bf16_bnin_ex", ptr(buf), N, H, W, Cp, H * W * ld, W * ld, ld, 1, ptr(dy),
                 H * W * Cout, W * Cout, Cout, Cout, 1, 1, 1, 0, 0, ptr(ws), ptr(dw), 0, _fl(buf) | (_fl(dy) << 1),
                 ptr(blk.mean), ptr(blk.rstd), ptr(gam), ptr(bet), _s())
            da = torch.empty(N, H, W, Cp, dtype=buf.dtype, device=dev)
            call("es_conv2d_bwd_data_bf16_ex", ptr(dy), H * W * Cout, W * Cout, Cout, ptr(wt), N, H, W, Cp, Cout, 1, 1, 1,
                 0, ptr(da), H * W * Cp, W * Cp, Cp, 1, 0, _fl(dy) | (_fl(da) << 1), _s())
            lda = Cp
        else:
            a = torch.empty(N, H, W, C, device=dev)
            call("es_bn2d_apply_ld_ex", ptr(buf), ld, rows, C, ptr(blk.mean), ptr(blk.rstd), ptr(gam), ptr(bet), 1, ptr(a),
                 C, 0, _s())
            self._dw_f32(a, N, H, W, C, ptr(dy), H * W * Cout, W * Cout, Cout, Cout, 1, 0, dw)
            da = torch.empty(N, H, W, C, device=dev)
            call("es_conv2d_bwd_data", ptr(dy), H * W * Cout, W * Cout, Cout, ptr(self.pview(wname)), N, H, W, C, Cout, 1,
                 1, 1, 0, ptr(da), H * W * C, W * C, C, 1, 0, _s())
            lda = C
        ws = torch.empty(lib.es_chan_workspace(rows, C), device=dev)
        call("es_bn2d_bwd_recompute_ld_ex", ptr(buf), ld, ptr(da), lda, rows, C, ptr(gam), ptr(bet), ptr(blk.mean),
             ptr(blk.rstd), ptr(gbuf), ld, ptr(self.gview(bnpre + "weight")), ptr(self.gview(bnpre + "bias")), 0, ptr(ws),
             _fl(buf) | 2 | 4, _s())

    # ---- the trunk -------------------------------------------------------------------------------------------
    def _slice_stats(self, blk, c, width, part):
        """Batch statistics of buf[..., c : c + width] into the block's arrays: from the producing conv's epilogue
        partials (bf16 convs; `part` covers roundup32(width) channels) or by one strided pass."""
        N, H, W = blk.geom
        rows = N * H * W
        tail = (BN_EPS, _at(blk.mean, c), _at(blk.rstd, c), _at(blk.m2, c))
        if part is not None:
            call("es_bn2d_stats_from_partials", ptr(part), rows, width, _rup(width, 32), *tail, _s())
            return
        ws = torch.empty(_lib.load().es_chan_workspace(rows, width), device=blk.buf.device)
        call("es_bn2d_stats_ld_ex", _at(blk.buf, c), rows, width, blk.ld, *tail, ptr(ws), _fl(blk.buf), _s())

    def _new_block(self, b, N, H, W):
        cfg = self.cfg
        c0, n, cout = cfg.blocks()[b - 1]
        blk = _Blk()
        blk.b, blk.c0, blk.n, blk.cout, blk.geom = b, c0, n, cout, (N, H, W)
        blk.ld = cout + cfg.slice_pad
        if N * H * W * blk.ld >= 2 ** 31:
            raise ValueError(f"dense block {b}: a {N}x{H}x{W}x{blk.ld} buffer exceeds the kernels' 2^31-element maps")
        dev = self.flat.device
        # zero-filled: the padded gathers read channels not written yet, which must be finite
        blk.buf = torch.zeros(N, H, W, blk.ld, dtype=_map_dtype(self), device=dev)
        blk.mean, blk.rstd, blk.m2 = (torch.zeros(blk.ld, device=dev) for _ in range(3))
        blk.y1, blk.st2 = [], []
        return blk

    def _layer_fwd(self, blk, l, keep):
        cfg, lib = self.cfg, _lib.load()
        N, H, W = blk.geom
        rows, ld, buf, dev = N * H * W, blk.ld, blk.buf, blk.buf.device
        g, mid, train = cfg.growth, cfg.mid, self.training
        c = blk.c0 + l * g
        pre = f"features.denseblock{blk.b}.denselayer{l + 1}."
        b16 = self.conv_bf16
        part1 = torch.empty(lib.es_conv2d_bnstats_size(rows, mid), device=dev) if (b16 and train) else None
        y1 = self._prefix_conv_fwd(blk, c, pre + "norm1.", pre + "conv1.weight", mid, part1)
        gam2, bet2 = self.pview(pre + "norm2.weight"), self.pview(pre + "norm2.bias")
        rm2, rv2, nbt2 = self.bn_buffers(pre + "norm2.")
        mean2, rstd2 = torch.empty(mid, device=dev), torch.empty(mid, device=dev)
        part2 = None
        if b16:
            if train:
                call("es_bn2d_fwd_partials_ex", ptr(y1), rows, mid, ptr(part1), ptr(gam2), ptr(bet2), ptr(rm2), ptr(rv2),
                     ptr(nbt2), BN_MOMENTUM, BN_EPS, None, 1, None, ptr(mean2), ptr(rstd2), _fl(y1), _s())
                part2 = torch.empty(lib.es_conv2d_bnstats_size(rows, _rup(g, 32)), device=dev)
            else:
                call("es_bn2d_eval_stats", ptr(rm2), ptr(rv2), mid, mid, BN_EPS, ptr(mean2), ptr(rstd2), _s())
            wp, _, gp, _ = self._wimg(pre + "conv2.weight")
            call("es_conv2d_fwd_bf16_bnin_ex", ptr(y1), N, H, W, mid, H * W * mid, W * mid, mid, 1, ptr(wp), None, gp, 3, 3,
                 1, 1, _at(buf, c), H * W * ld, W * ld, ld, 0, ptr(part2), _fl(y1) | (_fl(buf) << 1), ptr(mean2),
                 ptr(rstd2), ptr(gam2), ptr(bet2), _s())
        else:
            h2 = torch.empty_like(y1)
            ws = torch.empty(lib.es_chan_workspace(rows, mid), device=dev)
            call("es_bn2d_fwd_ex", ptr(y1), rows, mid, ptr(gam2), ptr(bet2), ptr(rm2), ptr(rv2),
                 ptr(nbt2) if train else None, BN_MOMENTUM, BN_EPS, 1 if train else 0, None, 1, ptr(h2), ptr(mean2),
                 ptr(rstd2), ptr(ws), 0, _s())
            call("es_conv2d_fwd", ptr(h2), N, H, W, mid, H * W * mid, W * mid, mid, 1,
                 ptr(self.pview(pre + "conv2.weight")), None, g, 3, 3, 1, 1, _at(buf, c), H * W * ld, W * ld, ld, 0, _s())
        if train:
            self._slice_stats(blk, c, g, part2)
        if keep:
            blk.y1.append(y1)
            blk.st2.append((mean2, rstd2))

    def _layer_bwd(self, blk, l, gbuf):
        cfg, lib = self.cfg, _lib.load()
        N, H, W = blk.geom
        rows, ld, dev = N * H * W, blk.ld, blk.buf.device
        g, mid = cfg.growth, cfg.mid
        c = blk.c0 + l * g
        pre = f"features.denseblock{blk.b}.denselayer{l + 1}."
        y1, (mean2, rstd2) = blk.y1[l], blk.st2[l]
        blk.y1[l] = None
        gam2, bet2 = self.pview(pre + "norm2.weight"), self.pview(pre + "norm2.bias")
        dw2 = self._dw_slot(blk.b, pre + "conv2.weight")
        dh2 = torch.empty_like(y1)
        gy = _at(gbuf, c)  # the layer's complete output gradient: the strided fp32 slice
        if self.conv_bf16:
            _, wt, gp, _ = self._wimg(pre + "conv2.weight")
            ws = torch.empty(lib.es_conv2d_bwd_weight_bf16_workspace(rows, gp, mid, 3, 3, 0), device=dev)
            call("es_conv2d_bwd_weight_bf16_bnin_ex", ptr(y1), N, H, W, mid, H * W * mid, W * mid, mid, 1, gy, H * W * ld,
                 W * ld, ld, gp, 3, 3, 1, 1, 0, ptr(ws), ptr(dw2), 0, _fl(y1), ptr(mean2), ptr(rstd2), ptr(gam2),
                 ptr(bet2), _s())
            call("es_conv2d_bwd_data_bf16_ex", gy, H * W * ld, W * ld, ld, ptr(wt), N, H, W, mid, gp, 3, 3, 1, 1, ptr(dh2),
                 H * W * mid, W * mid, mid, 1, 0, _fl(dh2) << 1, _s())
        else:
            h2 = torch.empty_like(y1)
            call("es_bn2d_apply_ld_ex", ptr(y1), mid, rows, mid, ptr(mean2), ptr(rstd2), ptr(gam2), ptr(bet2), 1, ptr(h2),
                 mid, 0, _s())
            self._dw_f32(h2, N, H, W, mid, gy, H * W * ld, W * ld, ld, g, 3, 1, dw2)
            call("es_conv2d_bwd_data", gy, H * W * ld, W * ld, ld, ptr(self.pview(pre + "conv2.weight")), N, H, W, mid, g,
                 3, 3, 1, 1, ptr(dh2), H * W * mid, W * mid, mid, 1, 0, _s())
        dy1 = torch.empty_like(y1)
        ws = torch.empty(lib.es_chan_workspace(rows, mid), device=dev)
        call("es_bn2d_bwd_recompute_ex", ptr(y1), ptr(dh2), rows, mid, ptr(gam2), ptr(bet2), ptr(mean2), ptr(rstd2),
             ptr(dy1), ptr(self.gview(pre + "norm2.weight")), ptr(self.gview(pre + "norm2.bias")), 0, ptr(ws), _fl(y1),
             _s())
        self._prefix_conv_bwd(blk.b, blk, c, pre + "norm1.", pre + "conv1.weight", dy1, gbuf)

    def _dense_forward(self, x0, keep):
        cfg = self.cfg
        N, H, W, _ = x0.shape
        nb = len(cfg.block_config)
        blks, train = [], self.training
        blk = self._new_block(1, N, H, W)
        blk.buf[..., :blk.c0].copy_(x0)  # the pooled stem map into the first block's prefix
        for b in range(1, nb + 1):
            if train:
                self._slice_stats(blk, 0, blk.c0, None)
            for l in range(blk.n):
                self._layer_fwd(blk, l, keep)
            consumer = f"features.transition{b}.norm." if b < nb else "features.norm5."
            if train:
                self._running_update(b, blk, consumer)
            blks.append(blk)
            if b == nb:
                break
            t = self._prefix_conv_fwd(blk, blk.cout, consumer, f"features.transition{b}.conv.weight", blk.cout // 2)
            nxt = self._new_block(b + 1, N, blk.geom[1] // 2, blk.geom[2] // 2)
            call("es_avgpool2_ld_fwd_ex", ptr(t), N, blk.geom[1], blk.geom[2], blk.cout // 2, ptr(nxt.buf), nxt.ld,
                 _fl(t) | (_fl(nxt.buf) << 1), _s())
            if not keep:
                blk.buf = None
            blk = nxt
        N, H, W = blk.geom
        C = blk.cout
        mean, rstd = self._norm_arrays(blk, "features.norm5.", C, C)
        out = torch.empty(N, H, W, C, dtype=blk.buf.dtype, device=blk.buf.device)
        fl = _fl(blk.buf)
        call("es_bn2d_apply_ld_ex", ptr(blk.buf), blk.ld, N * H * W, C, ptr(mean), ptr(rstd),
             ptr(self.pview("features.norm5.weight")), ptr(self.pview("features.norm5.bias")), 1, ptr(out), C,
             fl | (fl << 1), _s())
        return out, (blks if keep else None)

    def _dense_backward(self, blks, dout):
        lib = _lib.load()
        nb = len(blks)
        blk = blks[-1]
        N, H, W = blk.geom
        dev, C = blk.buf.device, blk.cout
        if dout.dtype != blk.buf.dtype:
            dout = dout.to(blk.buf.dtype)
        # one fp32 gradient buffer per block, zero-filled: every consumer of a channel accumulates into it
        gbuf = torch.zeros(N, H, W, blk.ld, device=dev)
        ws = torch.empty(lib.es_chan_workspace(N * H * W, C), device=dev)
        call("es_bn2d_bwd_recompute_ld_ex", ptr(blk.buf), blk.ld, ptr(dout), C, N * H * W, C,
             ptr(self.pview("features.norm5.weight")), ptr(self.pview("features.norm5.bias")), ptr(blk.mean),
             ptr(blk.rstd), ptr(gbuf), blk.ld, ptr(self.gview("features.norm5.weight")),
             ptr(self.gview("features.norm5.bias")), 0, ptr(ws), _fl(blk.buf) | 2 | 4, _s())
        for b in range(nb, 0, -1):
            blk = blks[b - 1]
            for l in range(blk.n - 1, -1, -1):
                self._layer_bwd(blk, l, gbuf)
            self._dw_unpad(b)
            if b == 1:
                break
            prev = blks[b - 2]
            N, H, W = prev.geom
            ct = prev.cout // 2
            dt = torch.empty(N, H, W, ct, dtype=prev.buf.dtype, device=dev)
            call("es_avgpool2_ld_bwd_ex", ptr(gbuf), blk.ld, N, H, W, ct, ptr(dt), _fl(dt) << 1, _s())
            gprev = torch.zeros(N, H, W, prev.ld, device=dev)
            self._prefix_conv_bwd(0, prev, prev.cout, f"features.transition{b - 1}.norm.",
                                  f"features.transition{b - 1}.conv.weight", dt, gprev)
            blk.buf, gbuf = None, gprev
        return gbuf[..., :blk.c0].to(blk.buf.dtype).contiguous()  # dense, the pooled stem map's type

    def forward(self, x):
        cfg = self.cfg
        if not self.flat.is_cuda:
            raise _lib.EndosslCallError(f"{type(self).__name__} runs on the MI355X only: move it to a cuda device first")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected [n, 3, H, W] images, got {tuple(x.shape)}")
        if self.training and dist.world_size() > 1:
            raise NotImplementedError("NativeDenseNet's dense blocks share one rank's BatchNorm statistics: "
                                      f"SyncBatchNorm over {dist.world_size()} ranks is not built (eval mode works)")
        _join_queued.clear()
        self._bn_partials.clear()
        n, H, W = x.shape[0], x.shape[2], x.shape[3]
        self.cur_n = n
        x = x.float().permute(0, 2, 3, 1).contiguous()  # NHWC once (the stem's 3-channel gathers)
        img = _Map(x, n, H, W, 3, sn=3 * H * W, sh=3 * W, sw=3, sc=1)
        on_tape = torch.is_grad_enabled() and self.training
        frozen = getattr(self, "frozen_trunk", False)
        anchor = self._anchor if (on_tape and not frozen) else None
        h = conv(self, x, img, "features.conv0.weight", None, cfg.init_features, 7, 2, 3, anchor=anchor,
                 out_dtype=torch.float32)
        h = _MaxPoolFn.apply(bn(self, h, "features.norm0.", eps=BN_EPS, relu=True), 3, 2, 1, _map_dtype(self))
        h = _DenseTrunkFn.apply(h, self)
        return _HeadFn.apply(h, self, self._anchor if (on_tape and frozen) else None)
