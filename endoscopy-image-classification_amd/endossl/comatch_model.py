"""ModelwEmb over the native ViT (CoMatch's model): `model(x) -> (logits, fts, z)`.

Reference: `ModelwEmb` (code/models/custom_model.py:147-213) with `build_head(in_fts, C,
is_complex=True)` (:107-120) and `head_emb` + `Normalize(2)` (:136-145,201-205).  The reference's
`ModelwEmb` cannot build a working ViT (its `backbone = Sequential(children[:-1])` drops the
cls-token / pos-embed logic); here `fts` is what a ViT backbone provides: the
final-LayerNorm CLS token, and the parameter names keep ModelwEmb's head indices
(fc.0 / fc.3 / fc.4, head_emb.0 / head_emb.2) after the timm trunk names.

The heads run as fp32 kernels (comatch.hip) on [n, D] rows -- 0.3 GFLOP per 1,408 images against
the trunk's 13 TFLOP; BatchNorm1d couples the rows, so the backward covers every image.

`NativeResNetEmb` is the same ModelwEmb over the native ResNet trunk (resnet18 / resnet50), the form the reference's
CoMatch, triplet and EZBM configs use: fts = the globally pooled last map, [n, 512 | 2048].
"""
import torch
import torch.nn as nn

from . import _lib, dist
from ._lib import call, ptr
from .conformer import _own, join_wgrad_stream
from .resnet import NativeResNet, ResNetConfig, _GlobalPoolFn
from .vit import NativeViT, ViTConfig

DROP_P = 0.2          # Dropout(0.2) in build_head (code/models/custom_model.py:113)
BN_MOMENTUM, BN_EPS = 0.1, 1e-5
LEAKY_SLOPE = 0.1     # LeakyReLU(negative_slope=0.1) (code/models/custom_model.py:202)


class EmbHeads:
    """Launch sequence of ModelwEmb's fc / head_emb on the features (forward, backward)."""

    # the layers that run on the wide kernel family (csrc/dense_wide.hip) under `wide`: those where it measured faster
    # at D = 2048 (profiles/dense_wide.txt); fc.4 (N = C < 64) keeps the small-N kernel
    WIDE_LAYERS = ("fc.0", "head_emb.0", "head_emb.2")

    def __init__(self, cfg, device, wide=False):
        """wide: the dense layers of WIDE_LAYERS on es_dense_wide_* (set by NativeResNetEmb, never by the ViT)."""
        self.cfg, self.device, self.wide = cfg, device, bool(wide)
        self._bufs = {}

    def _fwd(self, layer):
        return "es_dense_wide_fwd" if self.wide and layer in self.WIDE_LAYERS else "es_dense_fwd"

    def _bwd(self, layer):
        return "es_dense_wide_bwd" if self.wide and layer in self.WIDE_LAYERS else "es_dense_bwd"

    def _ws_floats(self, n):
        D, F, C, L = self.cfg.dim, self.cfg.dim // 4, self.cfg.num_classes, self.cfg.low_dim
        size = n * max(F, C, 3 * L, L)
        if self.wide:
            lib = _lib.load()
            shapes = {"fc.0": (D, F), "head_emb.0": (D, 3 * L), "head_emb.2": (3 * L, L)}
            size = max([size] + [lib.es_dense_wide_bwd_workspace(n, *shapes[k], 1) for k in self.WIDE_LAYERS])
        return size

    def bufs(self, n):
        if n not in self._bufs:
            D, F, C, L = self.cfg.dim, self.cfg.dim // 4, self.cfg.num_classes, self.cfg.low_dim
            z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)  # noqa: E731
            self._bufs[n] = {
                "u": z(n, F), "xhat": z(n, F), "rstd": z(2, F), "y": z(n, F), "logits": z(n, C),  # rstd: a row per BN group
                "e": z(n, 3 * L), "v": z(n, L), "z": z(n, L), "norm": z(n),
                "dy": z(n, F), "du": z(n, F), "dv": z(n, L), "de": z(n, 3 * L), "dfts": z(n, D),
                "ws": z(self._ws_floats(n)), "keep": torch.ones(n, F, dtype=torch.uint8, device=self.device),
                "s1": z(F), "s2": z(F), "sb": z(2 * F), "sbl": z(2 * F)}
        return self._bufs[n]

    def forward(self, view, bn, fts, keep, train):
        """view(name) -> parameter view; bn = (running_mean, running_var, num_batches_tracked);
        keep: uint8 [n, D/4] dropout keep-mask (train only).  Returns (logits, z) buffer views."""
        return self.fc_forward(view, bn, fts, keep, train), self.emb_forward(view, fts)

    def fc_forward(self, view, bn, x, keep, train, groups=1):
        """`fc` on the rows x [n, D]: fc.0 + ReLU + Dropout -> BatchNorm1d -> fc.4; returns the logits buffer.
        groups = 2 (EZBM stage 2, one process only): the first and the second n / 2 rows are two passes through
        BatchNorm1d, each with its own batch statistics and its own update of the running buffers."""
        cfg, s = self.cfg, _lib.stream()
        n, D = int(x.shape[0]), cfg.dim
        F, C = D // 4, cfg.num_classes
        b = self.bufs(n)
        kp = ptr(keep) if train else None
        call(self._fwd("fc.0"), ptr(x), D, ptr(view("fc.0.weight")), ptr(view("fc.0.bias")), ptr(b["u"]), F, n, D, F, 1,
             0.0, kp, 1.0 / (1.0 - DROP_P), s)
        world = dist.world_size()
        if groups > 1:
            call("es_bn1d_groups_fwd", ptr(b["u"]), F, ptr(view("fc.3.weight")), ptr(view("fc.3.bias")), ptr(bn[0]),
                 ptr(bn[1]), ptr(bn[2]), BN_MOMENTUM, BN_EPS, ptr(b["y"]), F, ptr(b["xhat"]), ptr(b["rstd"]),
                 n // groups, groups, F, s)
        elif train and world > 1:
            # SyncBatchNorm: batch statistics over every rank's rows (the one-process batch of the
            # reference); two all-reduces of F floats (sum, then the centred sum of squares)
            N = float(n * world)
            call("es_bn1d_sums", ptr(b["u"]), F, n, F, None, N, ptr(b["s1"]), s)
            dist.allreduce_inplace_(b["s1"])
            call("es_bn1d_sums", ptr(b["u"]), F, n, F, ptr(b["s1"]), N, ptr(b["s2"]), s)
            dist.allreduce_inplace_(b["s2"])
            call("es_bn1d_fwd_global", ptr(b["u"]), F, ptr(view("fc.3.weight")), ptr(view("fc.3.bias")), ptr(b["s1"]),
                 ptr(b["s2"]), N, ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), BN_MOMENTUM, BN_EPS, ptr(b["y"]), F,
                 ptr(b["xhat"]), ptr(b["rstd"]), n, F, s)
        else:
            call("es_bn1d_fwd", ptr(b["u"]), F, ptr(view("fc.3.weight")), ptr(view("fc.3.bias")), ptr(bn[0]),
                 ptr(bn[1]), ptr(bn[2]) if train else None, BN_MOMENTUM, BN_EPS, 1 if train else 0, ptr(b["y"]), F,
                 ptr(b["xhat"]), ptr(b["rstd"]), n, F, s)
        call("es_dense_fwd", ptr(b["y"]), F, ptr(view("fc.4.weight")), ptr(view("fc.4.bias")), ptr(b["logits"]), C, n,
             F, C, 0, 0.0, None, 1.0, s)
        return b["logits"]

    def emb_forward(self, view, fts):
        """`head_emb` on the features: head_emb.0 + LeakyReLU -> head_emb.2 -> l2norm; returns the z buffer."""
        cfg, s = self.cfg, _lib.stream()
        n, D, L = int(fts.shape[0]), cfg.dim, cfg.low_dim
        b = self.bufs(n)
        call(self._fwd("head_emb.0"), ptr(fts), D, ptr(view("head_emb.0.weight")), ptr(view("head_emb.0.bias")), ptr(b["e"]),
             3 * L, n, D, 3 * L, 2, LEAKY_SLOPE, None, 1.0, s)
        call(self._fwd("head_emb.2"), ptr(b["e"]), 3 * L, ptr(view("head_emb.2.weight")), ptr(view("head_emb.2.bias")),
             ptr(b["v"]), L, n, 3 * L, L, 0, 0.0, None, 1.0, s)
        call("es_l2norm_fwd", ptr(b["v"]), L, ptr(b["z"]), L, ptr(b["norm"]), n, L, s)
        return b["z"]

    def backward(self, view, gview, fts, keep, dlogits, dz):
        """dlogits [n, C], dz [n, L] -> head parameter grads (written through gview) and returns
        dfts [n, D].  Uses the activations of the last train forward."""
        self.fc_backward(view, gview, fts, keep, dlogits)  # writes dfts,
        return self.emb_backward(view, gview, fts, dz)     # adds to it

    def fc_backward(self, view, gview, x, keep, dlogits, groups=1, want_dx=True):
        """fc.4 -> BatchNorm1d -> fc.0 of the last train fc_forward(x, groups): `fc`'s parameter grads, and with
        want_dx the dfts buffer overwritten with d/dx (returned)."""
        cfg, s = self.cfg, _lib.stream()
        n, D = int(x.shape[0]), cfg.dim
        F, C = D // 4, cfg.num_classes
        b = self.bufs(n)
        ws = b["ws"]
        call("es_dense_bwd", ptr(dlogits), C, None, 0, 0, 0.0, None, 1.0, ptr(b["y"]), F, ptr(view("fc.4.weight")),
             ptr(b["dy"]), F, 0, ptr(gview("fc.4.weight")), ptr(gview("fc.4.bias")), n, F, C, ptr(ws), s)
        world = dist.world_size()
        if groups > 1:
            call("es_bn1d_groups_bwd", ptr(b["dy"]), F, ptr(b["xhat"]), ptr(b["rstd"]), ptr(view("fc.3.weight")),
                 ptr(b["du"]), F, ptr(gview("fc.3.weight")), ptr(gview("fc.3.bias")), n // groups, groups, F, s)
        elif world > 1:  # SyncBatchNorm backward: the global means of dY and dY * xhat
            call("es_bn1d_bwd_sums", ptr(b["dy"]), F, ptr(b["xhat"]), n, F, ptr(b["sbl"]), s)
            b["sb"].copy_(b["sbl"])
            dist.allreduce_inplace_(b["sb"])
            call("es_bn1d_bwd_global", ptr(b["dy"]), F, ptr(b["xhat"]), ptr(b["rstd"]), ptr(view("fc.3.weight")),
                 ptr(b["sb"]), ptr(b["sbl"]), float(n * world), ptr(b["du"]), F, ptr(gview("fc.3.weight")),
                 ptr(gview("fc.3.bias")), n, F, s)
        else:
            call("es_bn1d_bwd", ptr(b["dy"]), F, ptr(b["xhat"]), ptr(b["rstd"]), ptr(view("fc.3.weight")), ptr(b["du"]),
                 F, ptr(gview("fc.3.weight")), ptr(gview("fc.3.bias")), n, F, s)
        dx = b["dfts"] if want_dx else None
        call(self._bwd("fc.0"), ptr(b["du"]), F, ptr(b["u"]), F, 1, 0.0, ptr(keep), 1.0 / (1.0 - DROP_P), ptr(x), D,
             ptr(view("fc.0.weight")), ptr(dx), D if want_dx else 0, 0, ptr(gview("fc.0.weight")),
             ptr(gview("fc.0.bias")), n, D, F, ptr(ws), s)
        return dx

    def emb_backward(self, view, gview, fts, dz):
        """l2norm -> head_emb.2 -> head_emb.0: `head_emb`'s parameter grads; d/dfts is ADDED to the dfts buffer
        (returned)."""
        cfg, s = self.cfg, _lib.stream()
        n, D, L = int(fts.shape[0]), cfg.dim, cfg.low_dim
        b = self.bufs(n)
        ws = b["ws"]
        call("es_l2norm_bwd", ptr(dz), L, ptr(b["z"]), L, ptr(b["norm"]), ptr(b["dv"]), L, n, L, s)
        call(self._bwd("head_emb.2"), ptr(b["dv"]), L, None, 0, 0, 0.0, None, 1.0, ptr(b["e"]), 3 * L,
             ptr(view("head_emb.2.weight")), ptr(b["de"]), 3 * L, 0, ptr(gview("head_emb.2.weight")),
             ptr(gview("head_emb.2.bias")), n, 3 * L, L, ptr(ws), s)
        call(self._bwd("head_emb.0"), ptr(b["de"]), 3 * L, ptr(b["e"]), 3 * L, 2, LEAKY_SLOPE, None, 1.0, ptr(fts), D,
             ptr(view("head_emb.0.weight")), ptr(b["dfts"]), D, 1, ptr(gview("head_emb.0.weight")),
             ptr(gview("head_emb.0.bias")), n, D, 3 * L, ptr(ws), s)
        return b["dfts"]


class _BN(nn.Module):
    """Holds BatchNorm1d's buffers under ModelwEmb's state_dict names (fc.3.running_mean, ...)."""


class _ViTEmbFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, module, *params):
        ctx.module = module
        logits, fts, z = module._run(x, train=True)
        return logits.clone(), fts.clone(), z.clone()

    @staticmethod
    def backward(ctx, dlogits, dfts, dz):
        m = ctx.module
        C, L = m.cfg.num_classes, m.cfg.low_dim
        n = m._last_n
        dlogits = dlogits if dlogits is not None else torch.zeros(n, C, device=m.flat.device)
        dz = dz if dz is not None else torch.zeros(n, L, device=m.flat.device)
        g = m.backward_from(dlogits.float().contiguous(), dz.float().contiguous(),
                            None if dfts is None else dfts.float().contiguous())
        return (None, None) + tuple(m.engine().view(g, name).view(shape) for name, shape in m.layout)


class NativeViTEmb(NativeViT):
    """ModelwEmb (CoMatch model) over the native ViT trunk: forward(x) -> (logits, fts, z)."""

    def __init__(self, cfg=None, seed=None, **kw):
        cfg = cfg if cfg is not None else ViTConfig(head="emb", **kw)
        if cfg.head != "emb":
            raise ValueError("NativeViTEmb needs ViTConfig(head='emb')")
        super().__init__(cfg, seed=seed)
        self._init_bn_buffers(torch.device("cpu"))
        self._heads = None
        self.drop_seed = 0 if seed is None else int(seed)
        self._drop_counter = 0
        self._last_n = 0

    def _init_bn_buffers(self, device):
        F = self.cfg.dim // 4
        bn = self.fc._modules["3"]
        bn.register_buffer("running_mean", torch.zeros(F, device=device))
        bn.register_buffer("running_var", torch.ones(F, device=device))
        bn.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.int64, device=device))

    @property
    def fc(self):  # ModelwEmb.fc = the complex head (code/models/custom_model.py:196)
        return self._modules["fc"]

    @property
    def head_emb(self):
        return self._modules["head_emb"]

    def bn_buffers(self):
        bn = self.fc._modules["3"]
        return bn.running_mean, bn.running_var, bn.num_batches_tracked

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        bn = self.fc._modules["3"]
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            bn._buffers[k] = fn(bn._buffers[k])
        self._heads = None
        return self

    def __deepcopy__(self, memo):
        other = NativeViTEmb.__new__(NativeViTEmb)
        nn.Module.__init__(other)
        other.cfg, other.layout, other.offs, other.numel = self.cfg, self.layout, self.offs, self.numel
        other._set_flat(self.flat.detach().clone())
        other._init_bn_buffers(self.flat.device)
        for a, b in zip(other.bn_buffers(), self.bn_buffers()):
            a.copy_(b)
        other._engine, other._heads = None, None
        other.precision = self.precision
        other.version = 0
        other.drop_seed, other._drop_counter, other._last_n = self.drop_seed, self._drop_counter, 0
        other.train(self.training)
        return other

    def heads(self):
        if self._heads is None or self._heads.device != self.flat.device:
            self._heads = EmbHeads(self.cfg, self.flat.device)
        return self._heads

    def head_views(self):
        """(view, gview): name -> the flat parameter / flat gradient slice of a head tensor, for EmbHeads."""
        eng = self.engine()
        return (lambda nm: eng.view(self.flat, nm)), (lambda nm: eng.view(self.flat_grad, nm))

    def dropout_keep(self, n):
        """Fresh Dropout(0.2) keep-mask for n rows (device hash, reproducible from drop_seed)."""
        keep = self.heads().bufs(n)["keep"]
        call("es_dropout_keep", ptr(keep), keep.numel(), DROP_P, self.drop_seed, self._drop_counter, _lib.stream())
        self._drop_counter += keep.numel()
        return keep

    def _run(self, images, train, keep=None, trunk_train=None):
        """Trunk features + heads.  images: tensor or list of tensors (one batch, no concat).
        trunk_train=False: the trunk in inference form (no saved activations; a frozen trunk)."""
        eng = self.engine()
        eng.pack(self.flat, self.version)
        imgs = images if isinstance(images, (list, tuple)) else [images]
        trunk_train = train if trunk_train is None else trunk_train
        self._last_trunk_train = trunk_train
        fts = eng.forward(self.flat, imgs, train=trunk_train)
        n = int(fts.shape[0])
        self._last_n = n
        if train and keep is None:
            keep = self.dropout_keep(n)
        self._last_keep = keep
        logits, z = self.heads().forward(lambda nm: eng.view(self.flat, nm), self.bn_buffers(), fts, keep, train)
        return logits, fts, z

    def backward_from(self, dlogits, dz, dfts_extra=None, grad_ready=None, trunk=True):
        """Gradient of the last train forward: dlogits [n, C], dz [n, L] (and optionally a direct
        dL/dfts) -> flat grad (returned).  grad_ready: Engine.backward's per-block hook.
        trunk=False (IS_FREEZE): the heads' parameter gradients only, the trunk's stay zero."""
        eng = self.engine()
        g = self.flat_grad
        g.zero_()
        fts = eng.acts(self._last_n, getattr(self, "_last_trunk_train", True)).fts
        dfts = self.heads().backward(lambda nm: eng.view(self.flat, nm), lambda nm: eng.view(g, nm), fts,
                                     self._last_keep, dlogits, dz)
        if dfts_extra is not None:
            dfts.add_(dfts_extra)
        if not trunk:
            return g
        return eng.backward(self.flat, g, dfts=dfts, zero_grad=False, grad_ready=grad_ready)

    def forward(self, x):
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters()):
            params = [self.get_parameter(name) for name, _ in self.layout]
            return _ViTEmbFunction.apply(x, self, *params)
        logits, fts, z = self._run(x, train=self.training)
        return logits.clone(), fts.clone(), z.clone()


class _EmbHeadsFn(torch.autograd.Function):
    """ModelwEmb's heads on the pooled features, on the autograd tape: fts [n, D] -> (logits, z).  Forward and
    backward are NativeResNetEmb's own head passes, the ones `_run` / `backward_from` call."""

    @staticmethod
    def forward(ctx, fts, m, keep, anchor=None):
        ctx.m = m
        logits, z = m._heads_forward(fts.detach(), keep, True)
        return logits.clone(), z.clone()

    @staticmethod
    def backward(ctx, dlogits, dz):
        _own(dlogits)
        _own(dz)
        dfts = ctx.m._heads_backward(dlogits, dz)
        return (dfts.clone() if ctx.needs_input_grad[0] else None), None, None, None


class NativeResNetEmb(NativeResNet):
    """ModelwEmb over the native ResNet trunk (resnet18 / resnet50): forward(x) -> (logits, fts, z).

      fts       flatten(avgpool(trunk(x)))                                             [n, D], D = 512 | 2048
      fc        Linear(D, D/4) -> ReLU -> Dropout(0.2) -> BatchNorm1d(D/4) -> Linear(D/4, C)   indices 0, 3, 4
      head_emb  Linear(D, 3L) -> LeakyReLU(0.1) -> Linear(3L, L) -> x / |x|_2                  indices 0, 2

    The trunk is NativeResNet's (autograd over the conv / BatchNorm Functions), the heads are EmbHeads' launch
    sequence; fc.3's running buffers are layout entries like the trunk's BatchNorm2d buffers, so device moves,
    deepcopy, state_dict and the EMA buffer blend carry them.  `_run` / `backward_from` / `heads` / `dropout_keep` /
    `bn_buffers` have NativeViTEmb's signatures: the CoMatch, triplet and EZBM trainers take either model.

    state_dict, the reference's format: `model.<own key>` for the trunk and then `model.fc.0.weight` ...
    `model.fc.4.bias` (timm's fc position), the `fc.*` aliases of the same tensors, `head_emb.*`.  The reference
    also lists the trunk a second time as `backbone.N.*`: not written, skipped on load (as ModelMargin)."""

    cnn_emb = True  # the trainers refuse a data-parallel run of this model (untested there)

    def __init__(self, cfg=None, seed=None, **kw):
        cfg = cfg if cfg is not None else ResNetConfig(head="emb", **kw)
        if getattr(cfg, "head", "cls") != "emb":
            raise ValueError("NativeResNetEmb needs ResNetConfig(head='emb')")
        super().__init__(cfg, seed=seed)
        self._heads = None
        self.wide_heads = True  # the heads' wide dense layers on csrc/dense_wide.hip (EmbHeads.WIDE_LAYERS)
        self.drop_seed = 0 if seed is None else int(seed)
        self._drop_counter = 0
        self._last_n, self._last_fts, self._last_keep, self._fts_tape, self._last_heads = 0, None, None, None, None

    def __deepcopy__(self, memo):
        other = super().__deepcopy__(memo)
        other._heads, other.wide_heads = None, self.wide_heads
        other.drop_seed, other._drop_counter = self.drop_seed, self._drop_counter
        other._last_n, other._last_fts, other._last_keep, other._fts_tape, other._last_heads = 0, None, None, None, None
        if hasattr(self, "frozen_trunk"):
            other.frozen_trunk = self.frozen_trunk
        return other

    def bn_buffers(self, pre="fc.3."):
        return super().bn_buffers(pre)

    def heads(self):
        """EmbHeads of the current device and `wide_heads` setting (one per setting: each owns its buffers)."""
        key = (self.flat.device, bool(self.wide_heads))
        if not isinstance(self._heads, dict):
            self._heads = {}
        if key not in self._heads:
            self._heads[key] = EmbHeads(self.cfg, self.flat.device, wide=self.wide_heads)
        return self._heads[key]

    def head_views(self):
        """(view, gview): name -> the flat parameter / flat gradient slice of a head tensor, for EmbHeads."""
        return self.pview, self.gview

    def dropout_keep(self, n):
        """Fresh Dropout(0.2) keep-mask for n rows (device hash, reproducible from drop_seed)."""
        keep = self.heads().bufs(n)["keep"]
        call("es_dropout_keep", ptr(keep), keep.numel(), DROP_P, self.drop_seed, self._drop_counter, _lib.stream())
        self._drop_counter += keep.numel()
        return keep

    # ---- the one implementation under the step path (_run / backward_from) and the autograd path (forward) ----
    def _features(self, x, train, on_tape):
        """Pooled trunk features [n, D] with the module in `train` mode; on the autograd tape only with on_tape
        (and not under frozen_trunk, where NativeResNet._trunk keeps its convs off it)."""
        was = self.training
        self.training = bool(train)
        try:
            with torch.enable_grad() if on_tape else torch.no_grad():
                h, anchor = self._trunk(x)
                return _GlobalPoolFn.apply(h), anchor
        finally:
            self.training = was

    def _heads_forward(self, fts, keep, train):
        fts = fts.contiguous()
        self._last_n, self._last_fts, self._last_keep = int(fts.shape[0]), fts, keep
        self._last_heads = self.heads()  # the backward reads this one's activations, whatever wide_heads says then
        return self._last_heads.forward(self.pview, self.bn_buffers(), fts, keep, train)

    def _heads_backward(self, dlogits, dz):
        """Head parameter gradients of the last train forward into flat_grad; returns the heads' d/dfts buffer."""
        return self._last_heads.backward(self.pview, self.gview, self._last_fts, self._last_keep,
                                     dlogits.float().contiguous(), dz.float().contiguous())

    def _run(self, images, train, keep=None, trunk_train=None):
        """Trunk features + heads -> (logits, fts, z), buffers valid until the next call.  images: a tensor, or a list
        of tensors concatenated into ONE trunk pass (BatchNorm couples the rows: FixMatch._step_cnn).
        trunk_train=False (IS_FREEZE): the trunk off the autograd tape but still in training mode -- batch statistics,
        running buffers updated -- as frozen_trunk does for NativeResNet."""
        x = torch.cat(list(images)) if isinstance(images, (list, tuple)) else images
        trunk_train = train if trunk_train is None else trunk_train
        fts, _ = self._features(x, train, on_tape=bool(train and trunk_train))
        self._fts_tape = fts if fts.requires_grad else None
        if train and keep is None:
            keep = self.dropout_keep(int(fts.shape[0]))
        logits, z = self._heads_forward(fts.detach(), keep, train)
        return logits, self._last_fts, z

    def backward_from(self, dlogits, dz, dfts_extra=None, grad_ready=None, trunk=True):
        """Gradient of the last train `_run`: dlogits [n, C], dz [n, L] (and optionally a direct dL/dfts) -> flat grad
        (returned): the heads' backward, autograd from fts through the trunk, the weight-gradient stream joined.
        grad_ready is accepted for NativeViTEmb's signature and unused (no per-block hook here).
        trunk=False (IS_FREEZE): the heads' parameter gradients only, the trunk's stay zero."""
        g = self.flat_grad
        g.zero_()
        dfts = self._heads_backward(dlogits, dz)
        if dfts_extra is not None:
            dfts.add_(dfts_extra)
        fts, self._fts_tape = self._fts_tape, None
        if trunk and fts is not None:
            torch.autograd.backward([fts], [dfts])
            join_wgrad_stream(g.device)
        return g

    def forward(self, x, keep=None):
        """(logits, fts, z).  Eval mode: clones computed with the running statistics.  Training mode under grad:
        differentiable in all three outputs (the parameter gradients land in flat_grad, as NativeResNet's).
        keep: a uint8 [n, D/4] Dropout keep-mask to replay instead of a fresh draw (training mode)."""
        if self.training and keep is None:
            keep = self.dropout_keep(int(x.shape[0]))
        if torch.is_grad_enabled() and self.training:
            fts, anchor = self._features(x, True, on_tape=True)
            logits, z = _EmbHeadsFn.apply(fts, self, keep, anchor)
            return logits, fts, z
        fts, _ = self._features(x, self.training, on_tape=False)
        logits, z = self._heads_forward(fts, keep, self.training)
        return logits.clone(), fts.clone(), z.clone()

    # ---- the reference's state_dict format -------------------------------------------------------------------
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        if args:
            raise TypeError("NativeResNetEmb.state_dict takes destination / prefix / keep_vars by keyword")
        own = super().state_dict(prefix="", keep_vars=keep_vars)
        out = type(own)() if destination is None else destination
        for k, v in own.items():
            if not k.startswith("head_emb."):
                out[prefix + "model." + k] = v
        for k, v in own.items():
            if k.startswith(("fc.", "head_emb.")):
                out[prefix + k] = v
        return out

    @staticmethod
    def _own_keys(state_dict):
        own = {}
        for k, v in state_dict.items():
            if not k.startswith("backbone."):
                own[k[len("model."):] if k.startswith("model.") else k] = v
        return own

    def load_state_dict(self, state_dict, strict=True):
        return super().load_state_dict(self._own_keys(state_dict), strict=strict)

    def load_trunk(self, state_dict):
        """A plain ResNet checkpoint (the 2-class abnormality model of MODEL.PRE_TRAIN_PATH) into the trunk, as
        ModelwEmb takes it: every trunk tensor required, the checkpoint's own `fc.*` dropped, the heads untouched."""
        sd = {k: v for k, v in self._own_keys(state_dict).items() if not k.startswith(("fc.", "head_emb."))}
        trunk = [name for name, _, _ in self.layout if not name.startswith(("fc.", "head_emb."))]
        missing = [k for k in trunk if k not in sd]
        if missing:
            raise KeyError(f"PRE_TRAIN_PATH checkpoint lacks the trunk tensor {missing[0]!r}"
                           + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
        extra = [k for k in sd if k not in set(trunk)]
        if extra:
            raise KeyError(f"PRE_TRAIN_PATH checkpoint has the tensor {extra[0]!r}, which this trunk has not")
        return super().load_state_dict(sd, strict=False)
