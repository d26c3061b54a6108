"""Native ResNet-18 -- the supervised baseline of BASELINE configs[0] (SURVEY.md §8(d) P0:
`supervised.py` ResNet-18, 23 classes, B=16, 224²) -- and ResNet-50, the backbone most reference configs name
(`code/configs/*`: `NAME: 'resnet50'`), on the Conformer's CNN kernels.

Reference: `build_model` -> timm `resnet18` (`code/build.py:160-211`, timm==0.5.4, absent from this
image: its architecture is restated here -- conv1 7x7/2 -> BatchNorm -> ReLU -> max-pool 3/2 -> four
stages of two BasicBlocks (3x3 conv -> BN -> ReLU -> 3x3 conv -> BN, + identity or 1x1/2 conv + BN
shortcut, ReLU) -> global average pool -> fc).  `model(x) -> logits`, the timm state_dict (names
and order), so checkpoints interchange.  resnet50 (`ResNetConfig(**RESNET50)`): the same stem and head around
stages of 3 / 4 / 6 / 3 Bottlenecks (1x1 conv -> BN -> ReLU -> 3x3 conv with the stride -> BN -> ReLU -> 1x1 conv
to 4x the width -> BN, + identity or 1x1 conv with the stride + BN shortcut, ReLU), fc over 2048 features;
its stride-1 1x1 convs run on the direct kernels (es_conv1x1_*) where those are faster.

MI355X layout (as NativeConformer, whose parameter plumbing it shares): parameters in one flat fp32
buffer, NHWC maps, every conv an implicit GEMM (bf16 operands for channel counts % 32 == 0 --
all but the 3-channel stem; `set_conv_precision("fp32")` for parity), BatchNorm with the residual add
and ReLU fused into its apply pass, SyncBatchNorm at N > 1 (as the Conformer).  With the bf16 convs
the activation and gradient maps after the stem's max-pool are bf16 (map_bf16; the stem and BatchNorm
statistics stay fp32, ENDOSSL_MAP_BF16=0 keeps fp32 maps): every conv after the stem is bf16-eligible.

`NativeSEResNet` is the reference's own `resnet50se` (code/models/se.py:8-119, code/build.py:152-170): ResNet-50 with
a squeeze-excite gate on bn3's output in every Bottleneck (`ResNetConfig(se=True)`: conv_down / conv_up per block).
Only the block tail differs, and it runs on csrc/se.hip without writing bn3's output (`_SETailFn`).

`ModelMargin` (code/models/custom_model.py:122-134) is the same network with a bias-free fc and a `backbone(x)`
that stops at the pooled features: the model of the angular-margin supervised mode (MODEL.MARGIN).
"""
import math

import torch
import torch.nn as nn

from . import _lib, dist
from ._lib import call, ptr
from .conformer import (BN_EPS_STEM, BN_MOMENTUM, CONV_BF16, GRAD_SINKS, MAP_BF16, NativeConformer, _ConvHeadFn, _fl,
                        _GradSink, _Map, _map_dtype, _MaxPoolFn, _join_queued, _own, _rup, _s, bn, bn_conv, conv)
from .vit import emb_head_layout

BN_EPS = 1e-5  # timm BasicBlock norm_layer = nn.BatchNorm2d (default eps)


class ResNetConfig:
    """The default is timm's resnet18 (BasicBlocks); `RESNET50` below is its resnet50 (Bottlenecks)."""

    def __init__(self, layers=(2, 2, 2, 2), num_classes=23, img_size=224, widths=(64, 128, 256, 512), fc_bias=True,
                 block="basic", se=False, head="cls", low_dim=64):
        if block not in ("basic", "bottleneck"):
            raise ValueError(f"block {block!r}: 'basic' or 'bottleneck'")
        if head not in ("cls", "emb"):
            raise ValueError(f"head {head!r}: 'cls' (timm's fc) or 'emb' (ModelwEmb's fc / head_emb)")
        if head == "emb" and (se or not fc_bias):
            raise ValueError("head='emb': ModelwEmb's heads over the plain ResNet trunk (no se, no bias-free fc)")
        # "emb": ModelwEmb's heads on the pooled features (comatch_model.NativeResNetEmb), low_dim = L
        self.head, self.low_dim = head, int(low_dim)
        if se and block != "bottleneck":
            raise ValueError("se=True: the squeeze-excite gate sits in a Bottleneck (code/models/se.py:8-58)")
        self.se = bool(se)  # SEResNet's Bottleneck: conv_down / conv_up gate bn3's output (NativeSEResNet)
        self.layers, self.widths = tuple(layers), tuple(widths)
        self.num_classes, self.img_size = num_classes, img_size
        self.fc_bias = bool(fc_bias)  # False: ModelMargin's nn.Linear(num_features, C, bias=False)
        self.block = block
        self.expansion = 4 if block == "bottleneck" else 1  # timm Bottleneck.expansion / BasicBlock.expansion

    @property
    def num_features(self):
        """Channels of the last stage = the pooled feature width = fc's fan-in (512 | 2048)."""
        return self.widths[-1] * self.expansion

    @property
    def dim(self):
        """The feature width under the name the embedding heads and the trainers read (ViTConfig.dim)."""
        return self.num_features

    def blocks(self):
        """(prefix, inplanes, planes, stride, downsample) per block in state_dict order; a block's output has
        planes * expansion channels."""
        out, inp = [], 64
        for si, (n, w) in enumerate(zip(self.layers, self.widths)):
            for bi in range(n):
                stride = 2 if (si > 0 and bi == 0) else 1
                out.append((f"layer{si + 1}.{bi}.", inp, w, stride, stride != 1 or inp != w * self.expansion))
                inp = w * self.expansion
        return out


# timm resnet50: Bottleneck, layers [3, 4, 6, 3] -- stage outputs 256 / 512 / 1024 / 2048
RESNET50 = dict(layers=(3, 4, 6, 3), widths=(64, 128, 256, 512), block="bottleneck")


def _bn_entries(pre, C):
    return [(pre + "weight", (C,), "p"), (pre + "bias", (C,), "p"), (pre + "running_mean", (C,), "rm"),
            (pre + "running_var", (C,), "rv"), (pre + "num_batches_tracked", (), "nbt")]


def resnet_layout(cfg):
    """(name, shape, kind) in timm resnet18's / resnet50's state_dict order."""
    out = [("conv1.weight", (64, 3, 7, 7), "p")] + _bn_entries("bn1.", 64)
    bottleneck = getattr(cfg, "block", "basic") == "bottleneck"
    for pre, inp, w, stride, ds in cfg.blocks():
        outp = w * getattr(cfg, "expansion", 1)
        if bottleneck:
            out += [(pre + "conv1.weight", (w, inp, 1, 1), "p")] + _bn_entries(pre + "bn1.", w)
            out += [(pre + "conv2.weight", (w, w, 3, 3), "p")] + _bn_entries(pre + "bn2.", w)
            out += [(pre + "conv3.weight", (outp, w, 1, 1), "p")] + _bn_entries(pre + "bn3.", outp)
            if getattr(cfg, "se", False):  # code/models/se.py:23-26, registered after bn3 and before downsample
                out += [(pre + "conv_down.weight", (w // 4, outp, 1, 1), "p"),
                        (pre + "conv_up.weight", (outp, w // 4, 1, 1), "p")]
        else:
            out += [(pre + "conv1.weight", (w, inp, 3, 3), "p")] + _bn_entries(pre + "bn1.", w)
            out += [(pre + "conv2.weight", (w, w, 3, 3), "p")] + _bn_entries(pre + "bn2.", w)
        if ds:
            out += [(pre + "downsample.0.weight", (outp, inp, 1, 1), "p")] + _bn_entries(pre + "downsample.1.", outp)
    if getattr(cfg, "head", "cls") == "emb":
        # ModelwEmb: timm's fc replaced by the complex head, head_emb after it; fc.3 is a BatchNorm1d whose running
        # buffers ride the same flat-parameter plumbing as the trunk's BatchNorm2d buffers
        for name, shape in emb_head_layout(cfg):
            out.append((name, shape, "p"))
            if name == "fc.3.bias":
                out += _bn_entries("fc.3.", shape[0])[2:]
        return out
    C = cfg.num_classes
    out += [("fc.weight", (C, cfg.widths[-1] * getattr(cfg, "expansion", 1)), "p")]
    if getattr(cfg, "fc_bias", True):
        out += [("fc.bias", (C,), "p")]
    return out


def init_resnet_(flat, layout, offs, generator=None):
    """timm ResNet.init_weights: kaiming-normal (fan_out, ReLU) convs, BatchNorm weight 1 / bias 0,
    fc as nn.Linear's default (uniform +-1/sqrt(fan_in) for weight and bias).  Every BatchNorm weight is 1, a
    block's last one (bn2 / bn3) included: timm's zero_init_last_bn is not restated."""
    fan_in = next((shape[1] for name, shape, _ in layout if name == "fc.weight"), None)
    shapes = {name: shape for name, shape, _ in layout}
    for name, shape, kind in layout:
        if kind != "p":
            continue
        t = flat[offs[name]:offs[name] + math.prod(shape)].view(shape)
        if fan_in is None and name.startswith(("fc.", "head_emb.")):
            # ModelwEmb's heads keep the PyTorch defaults, as NativeViTEmb's (vit.timm_init_): Linear
            # kaiming_uniform(a=sqrt(5)) with bias U(+-1/sqrt(fan_in)), BatchNorm1d weight 1 / bias 0
            if name.startswith("fc.3."):
                t.fill_(1.0 if name.endswith("weight") else 0.0)
            elif len(shape) == 2:
                nn.init.kaiming_uniform_(t, a=math.sqrt(5), generator=generator)
            else:
                bound = 1.0 / math.sqrt(shapes[name[:-len("bias")] + "weight"][1])
                nn.init.uniform_(t, -bound, bound, generator=generator)
        elif len(shape) == 4:
            std = math.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
            t.normal_(0.0, std, generator=generator)
        elif name.startswith("fc."):
            bound = 1.0 / math.sqrt(fan_in)
            t.uniform_(-bound, bound, generator=generator)
        elif name.endswith("weight"):
            t.fill_(1.0)
        else:
            t.zero_()


class NativeResNet(NativeConformer):
    """ResNet-18 / ResNet-50 whose compute runs in libendossl_hip.so; state_dict identical to timm's resnet18 /
    resnet50.
    Shares NativeConformer's flat-parameter plumbing (views, BatchNorm buffers, bf16 conv images,
    device moves, deepcopy) and its conv / BatchNorm / pooling / head autograd Functions."""

    def __init__(self, cfg=None, seed=None, **kw):
        nn.Module.__init__(self)
        self.cfg = cfg if cfg is not None else ResNetConfig(**kw)
        self.layout = resnet_layout(self.cfg)
        self.offs, o = {}, 0
        for name, shape, kind in self.layout:
            if kind == "p":
                self.offs[name] = o
                o = _rup(o + math.prod(shape), 64)
        self.numel = o
        self.shapes = {name: shape for name, shape, _ in self.layout}
        flat = torch.zeros(self.numel, dtype=torch.float32)
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        init_resnet_(flat, self.layout, self.offs, generator=gen)
        self._build(flat, device=torch.device("cpu"))
        self.version = 0
        self.cur_n = 0
        self.conv_bf16 = CONV_BF16

    @property
    def map_bf16(self):
        """bf16 activation / gradient maps after the stem's max-pool (every later conv has channel counts
        % 32 == 0, so all of them run on the bf16 kernels)."""
        return bool(self.conv_bf16 and MAP_BF16)

    @property
    def fc(self):  # a real submodule here (timm's classifier, IS_FREEZE's trainable part)
        return self._modules["fc"]

    def no_weight_decay(self):
        return set()

    def _pack(self):  # no transformer weight images
        return None

    @property
    def conv_1x1(self):
        """The stride-1 1 x 1 convs over dense bf16 maps on the direct kernels (es_conv1x1_*, where the library's
        es_set_conv_1x1 knob selects them): the bottleneck configs, whose work is mostly such convs.  ResNet-18's
        only 1 x 1 convs are its strided shortcuts: it keeps the implicit kernels."""
        return self.cfg.block == "bottleneck"

    def _bottleneck(self, x, pre, inp, planes, stride, ds):
        """timm Bottleneck.forward: relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + shortcut), the stride on
        conv2 (timm 0.5.4's resnet50), shortcut = x or downsample.1(downsample.0(x)) (1 x 1 conv with the stride).
        Composed as the Conformer's ConvBlock (_conv_block_head / _conv_block_tail): bn1 + ReLU applied by conv2's
        gathers only where BN_CONV_FUSED_KXK allows, bn2 + ReLU by conv3's loads (bn_conv)."""
        outp = planes * self.cfg.expansion
        sink = _GradSink() if GRAD_SINKS else None  # x's two gradient contributions summed in place
        h = conv(self, x, _Map.nhwc(x), pre + "conv1.weight", None, planes, 1, 1, 0, stats=True, sink=sink)
        h = bn_conv(self, h, pre + "bn1.", pre + "conv2.weight", None, planes, 3, stride, 1, stats=True, eps=BN_EPS)
        h = bn_conv(self, h, pre + "bn2.", pre + "conv3.weight", None, outp, 1, 1, 0, stats=True, eps=BN_EPS)
        if ds:
            sc = conv(self, x, _Map.nhwc(x), pre + "downsample.0.weight", None, outp, 1, stride, 0, stats=True,
                      sink=sink)
            sc = bn(self, sc, pre + "downsample.1.", eps=BN_EPS)
            return self._bottleneck_tail(h, pre, sc, None)
        return self._bottleneck_tail(h, pre, x, sink)

    def _bottleneck_tail(self, h, pre, res, res_sink):
        """conv3's output -> the block's output: relu(bn3(h) + res)."""
        return bn(self, h, pre + "bn3.", eps=BN_EPS, relu=True, res=res, res_sink=res_sink)

    def _block(self, x, pre, inp, planes, stride, ds):
        """timm BasicBlock.forward: relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut); Bottleneck: _bottleneck."""
        if self.cfg.block == "bottleneck":
            return self._bottleneck(x, pre, inp, planes, stride, ds)
        sink = _GradSink() if GRAD_SINKS else None  # x's two gradient contributions summed in place
        h = conv(self, x, _Map.nhwc(x), pre + "conv1.weight", None, planes, 3, stride, 1, stats=True, sink=sink)
        # bn1 + ReLU feed conv2 alone: applied by conv2's gathers where the bf16 kernels run it (bn_conv)
        h = bn_conv(self, h, pre + "bn1.", pre + "conv2.weight", None, planes, 3, 1, 1, stats=True, eps=BN_EPS)
        if ds:
            sc = conv(self, x, _Map.nhwc(x), pre + "downsample.0.weight", None, planes, 1, stride, 0, stats=True,
                      sink=sink)
            sc = bn(self, sc, pre + "downsample.1.", eps=BN_EPS)
            return bn(self, h, pre + "bn2.", eps=BN_EPS, relu=True, res=sc)
        return bn(self, h, pre + "bn2.", eps=BN_EPS, relu=True, res=x, res_sink=sink)

    def _trunk(self, x):
        """Images -> (the last stage's NHWC map, the head's tape anchor under a frozen trunk)."""
        cfg = self.cfg
        if not self.flat.is_cuda:
            raise _lib.EndosslCallError(f"{type(self).__name__} runs on the MI355X only: move it to a cuda device first")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected [n, 3, H, W] images, got {tuple(x.shape)}")
        _join_queued.clear()
        self._bn_partials.clear()
        n, H, W = x.shape[0], x.shape[2], x.shape[3]
        self.cur_n = n
        x = x.float().permute(0, 2, 3, 1).contiguous()  # NHWC once (the stem's 3-channel gathers)
        img = _Map(x, n, H, W, 3, sn=3 * H * W, sh=3 * W, sw=3, sc=1)
        on_tape = torch.is_grad_enabled() and self.training
        frozen = getattr(self, "frozen_trunk", False)
        anchor = self._anchor if (on_tape and not frozen) else None
        h = conv(self, x, img, "conv1.weight", None, 64, 7, 2, 3, anchor=anchor, out_dtype=torch.float32)
        h = _MaxPoolFn.apply(bn(self, h, "bn1.", eps=BN_EPS_STEM, relu=True), 3, 2, 1, _map_dtype(self))
        for pre, inp, planes, stride, ds in cfg.blocks():
            h = self._block(h, pre, inp, planes, stride, ds)
        return h, (self._anchor if (on_tape and frozen) else None)

    def forward(self, x):
        h, head_anchor = self._trunk(x)
        return _ConvHeadFn.apply(h, self, head_anchor, "fc.")


class _GlobalPoolFn(torch.autograd.Function):
    """AdaptiveAvgPool2d(1) + flatten: NHWC map (fp32 or bf16) -> [N, C] fp32 features."""

    @staticmethod
    def forward(ctx, x):
        N, H, W, C = x.shape
        if H != W:
            raise ValueError(f"the global pool expects square maps, got {H}x{W}")
        pooled = torch.empty(N, C, device=x.device)
        call("es_avgpool2d_fwd_ex", ptr(x.contiguous()), N, H, W, C, H, ptr(pooled), _fl(x), _s())
        ctx.geom, ctx.dt = (N, H, W, C), x.dtype
        return pooled

    @staticmethod
    def backward(ctx, dp):
        _own(dp)
        N, H, W, C = ctx.geom
        dp = dp.float().contiguous()
        dx = torch.empty(N, H, W, C, dtype=ctx.dt, device=dp.device)
        call("es_avgpool2d_bwd_ex", ptr(dp), N, H, W, C, H, ptr(dx), 0, _fl(dx) << 1, _s())
        return dx


class _LinearNoBiasFn(torch.autograd.Function):
    """fts [N, K] -> fts fc.weight^T; the weight gradient goes to the flat gradient (overwritten)."""

    @staticmethod
    def forward(ctx, fts, m, anchor=None):
        N, K = fts.shape
        ncls = m.cfg.num_classes
        fts = fts.contiguous()
        logits = torch.empty(N, ncls, device=fts.device)
        call("es_dense_fwd", ptr(fts), K, ptr(m.pview("fc.weight")), None, ptr(logits), ncls, N, K, ncls, 0, 0.0, None,
             1.0, _s())
        ctx.save_for_backward(fts)
        ctx.m = m
        return logits

    @staticmethod
    def backward(ctx, dl):
        _own(dl)
        (fts,) = ctx.saved_tensors
        m = ctx.m
        N, K = fts.shape
        ncls = m.cfg.num_classes
        dl = dl.contiguous()
        dfts = torch.empty(N, K, device=dl.device)
        ws = torch.empty(_lib.load().es_dense_bwd_workspace(N, ncls), device=dl.device)
        call("es_dense_bwd", ptr(dl), ncls, None, 0, 0, 0.0, None, 1.0, ptr(fts), K, ptr(m.pview("fc.weight")),
             ptr(dfts), K, 0, ptr(m.gview("fc.weight")), None, N, K, ncls, ptr(ws), _s())
        return (dfts if ctx.needs_input_grad[0] else None), None, None


class ModelMargin(NativeResNet):
    """ModelMargin over resnet18 or resnet50 (code/models/custom_model.py:122-134): the ResNet with a bias-free fc, for
    the angular-margin losses (loss.AngularPenaltySMLoss reads `fc.weight`, code/supervised.py:117-119).

      model(x)            plain logits fc(pool(trunk(x))), no normalisation (evaluate_one / inference)
      model.backbone(x)   the pooled [n, F] features (F = 512 | 2048), on the autograd tape in training mode
      model.fc            the classifier module; `.weight` [C, F] is a view of the flat buffer

    state_dict: the reference's `model.*` keys (timm's resnet names under `model.`, `model.fc.weight`, no
    bias) followed by its `fc.weight` alias of the same tensor.  The reference also lists every trunk tensor a
    second time as `backbone.N.*` (nn.Sequential over timm's children): loading skips those keys, and they are
    not written -- timm is absent, so the index map N is unpinned."""

    def __init__(self, cfg=None, seed=None, **kw):
        cfg = cfg if cfg is not None else ResNetConfig(fc_bias=False, **kw)
        if cfg.fc_bias:
            raise ValueError("ModelMargin's fc has no bias: build its config with fc_bias=False")
        super().__init__(cfg, seed=seed)

    def backbone(self, x):
        h, _ = self._trunk(x)
        return _GlobalPoolFn.apply(h)

    def forward(self, x):
        h, head_anchor = self._trunk(x)
        return _LinearNoBiasFn.apply(_GlobalPoolFn.apply(h), self, head_anchor)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        if args:
            raise TypeError("ModelMargin.state_dict takes destination / prefix / keep_vars by keyword")
        own = super().state_dict(prefix="", keep_vars=keep_vars)
        out = type(own)() if destination is None else destination
        for k, v in own.items():
            out[prefix + "model." + k] = v
        out[prefix + "fc.weight"] = own["fc.weight"]
        return out

    def load_state_dict(self, state_dict, strict=True):
        own = {}
        for k, v in state_dict.items():
            if k.startswith("backbone."):
                continue
            own[k[len("model."):] if k.startswith("model.") else k] = v
        return super().load_state_dict(own, strict=strict)


class _SETailFn(torch.autograd.Function):
    """The tail of an SE-ResNet Bottleneck (code/models/se.py:43-58) after conv3, on csrc/se.hip:
    out = relu(s * bn3(y) + res), s = sigmoid(conv_up(relu(conv_down(pool(bn3(y)))))), with bn3's output never
    written -- its pool is bn3's affine map of y's per-image channel means (es_se_squeeze_ex, the one added read
    of y), the gate is [N, C]-sized (es_se_gate_fwd) and the apply pass is BatchNorm's with the gate
    (es_se_bn_apply_ex).  Statistics as bn(): from conv3's epilogue partials where it left them (train mode, bf16
    convs, one rank), else from the library's channel sums; eval mode reads the running buffers.  Backward: one sums
    pass (es_se_bn_bwd_sums_ex), the gate's backward with bn3's and both SE weights' gradients written to the flat
    gradient (es_se_gate_bwd), one dx pass that also writes the shortcut's gradient (es_se_bn_bwd_dx_ex)."""

    @staticmethod
    def forward(ctx, y, res, m, pre, eps, res_sink=None):
        y, res = y.contiguous(), res.contiguous()
        if res.dtype != y.dtype or res.shape != y.shape:
            raise _lib.EndosslCallError(f"{pre}: residual map {res.dtype} {tuple(res.shape)} vs conv3's "
                                        f"{y.dtype} {tuple(y.shape)}")
        N, H, W, C = y.shape
        HW, rows = H * W, N * H * W
        R = m.shapes[pre + "conv_down.weight"][0]
        train = m.training
        if train and getattr(m, "sync_bn", True) and dist.world_size() > 1:
            raise NotImplementedError("the SE tail takes one rank's BatchNorm statistics: SyncBatchNorm over "
                                      f"{dist.world_size()} ranks is not built for NativeSEResNet (eval mode works)")
        lib, dev, fl = _lib.load(), y.device, _fl(y)
        bnp = pre + "bn3."
        gam, bet = m.pview(bnp + "weight"), m.pview(bnp + "bias")
        rm, rv, nbt = m.bn_buffers(bnp)
        mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        part = m._bn_partials.pop(y.data_ptr(), None) if train else None
        if part is not None and part[1] == y.shape:
            call("es_bn2d_fwd_partials_ex", ptr(y), rows, C, ptr(part[0]), ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(nbt),
                 BN_MOMENTUM, eps, None, 1, None, ptr(mean), ptr(rstd), fl, _s())
        elif train:
            sums = torch.empty(2, C, device=dev)
            ws = torch.empty(lib.es_chan_workspace(rows, C), device=dev)
            call("es_bn2d_sums_ex", ptr(y), rows, C, 0, None, 0, ptr(sums[0]), ptr(ws), fl, _s())
            call("es_bn2d_sums_ex", ptr(y), rows, C, 1, ptr(sums[0]), rows, ptr(sums[1]), ptr(ws), fl, _s())
            call("es_se_bn_stats", ptr(sums[0]), ptr(sums[1]), rows, C, eps, BN_MOMENTUM, 1, ptr(mean), ptr(rstd), ptr(rm),
                 ptr(rv), ptr(nbt), _s())
        else:
            call("es_se_bn_stats", None, None, rows, C, eps, BN_MOMENTUM, 0, ptr(mean), ptr(rstd), ptr(rm), ptr(rv), None,
                 _s())
        ybar, a, s = (torch.empty(N, C, device=dev) for _ in range(3))
        h = torch.empty(N, R, device=dev)
        ws = torch.empty(lib.es_se_squeeze_workspace(N, HW, C, fl), device=dev)
        call("es_se_squeeze_ex", ptr(y), N, HW, C, ptr(mean), ptr(rstd), ptr(gam), ptr(bet), ptr(ybar), ptr(a), ptr(ws),
             fl, _s())
        call("es_se_gate_fwd", ptr(a), ptr(m.pview(pre + "conv_down.weight")), ptr(m.pview(pre + "conv_up.weight")), N,
             C, R, ptr(h), ptr(s), _s())
        out = torch.empty_like(y)
        call("es_se_bn_apply_ex", ptr(y), ptr(res), ptr(s), N, HW, C, ptr(mean), ptr(rstd), ptr(gam), ptr(bet), ptr(out),
             fl, _s())
        ctx.save_for_backward(y, out, mean, rstd, ybar, a, h, s)
        ctx.m, ctx.pre, ctx.train, ctx.res_sink = m, pre, train, res_sink
        return out

    @staticmethod
    def backward(ctx, dout):
        _own(dout)
        y, out, mean, rstd, ybar, a, h, s = ctx.saved_tensors
        m, pre = ctx.m, ctx.pre
        N, H, W, C = y.shape
        HW, R = H * W, h.shape[1]
        lib, dev, fl = _lib.load(), y.device, _fl(y)
        dout = dout.contiguous()
        if dout.dtype != y.dtype:
            dout = dout.to(y.dtype)
        bnp = pre + "bn3."
        gam, bet = m.pview(bnp + "weight"), m.pview(bnp + "bias")
        dgam, dbet = m.gview(bnp + "weight"), m.gview(bnp + "bias")
        p1, p2, da = (torch.empty(N, C, device=dev) for _ in range(3))
        ws = torch.empty(lib.es_se_bn_bwd_sums_workspace(N, HW, C, fl), device=dev)
        call("es_se_bn_bwd_sums_ex", ptr(y), ptr(out), ptr(dout), N, HW, C, ptr(mean), ptr(rstd), ptr(p1), ptr(p2),
             ptr(ws), fl, _s())
        wsg = torch.empty(lib.es_se_gate_bwd_workspace(N, C, R), device=dev)
        call("es_se_gate_bwd", ptr(p1), ptr(p2), ptr(ybar), ptr(a), ptr(h), ptr(s),
             ptr(m.pview(pre + "conv_down.weight")), ptr(m.pview(pre + "conv_up.weight")), ptr(gam), ptr(bet), ptr(mean),
             ptr(rstd), N, C, R, ptr(m.gview(pre + "conv_down.weight")), ptr(m.gview(pre + "conv_up.weight")), ptr(da),
             ptr(dgam), ptr(dbet), ptr(wsg), _s())
        # the shortcut's gradient: into the block input's _GradSink where the shortcut is the identity (this
        # backward runs before conv1's, as bn3's does in NativeResNet: it is the sink's first writer)
        sink = ctx.res_sink
        gres, acc = sink.take(lambda: torch.empty_like(y)) if sink is not None else (torch.empty_like(y), 0)
        dy = torch.empty_like(y)
        call("es_se_bn_bwd_dx_ex", ptr(y), ptr(out), ptr(dout), ptr(s), ptr(da), N, HW, C, ptr(mean), ptr(rstd), ptr(gam),
             ptr(dgam), ptr(dbet), 1 if ctx.train else 0, ptr(dy), ptr(gres), acc, fl, _s())
        if sink is not None:
            gres = sink.give(gres, acc)
        return dy, gres, None, None, None, None


class NativeSEResNet(NativeResNet):
    """SE-ResNet-50, the reference's `resnet50se` (code/build.py:152-170: SEResNet(Bottleneck, [3, 4, 6, 3]),
    code/models/se.py:8-119): ResNet-50 with a squeeze-excite gate on bn3's output in every Bottleneck.  The stem, the
    stride on conv2, the downsample, the init rule and fc are NativeResNet's; only the block tail differs
    (_SETailFn).  state_dict = the reference's (conv_down / conv_up after bn3.*, before downsample.*).

    The pool before fc is the global one: the reference's nn.AvgPool2d(7) equals it at 224^2 (a 7 x 7 last map)
    and fails or reads a corner at other sizes.  A train-mode forward on more than one rank raises
    (the tail takes one rank's BatchNorm statistics); steps run eagerly (no graph replay)."""

    def __init__(self, cfg=None, seed=None, **kw):
        cfg = cfg if cfg is not None else ResNetConfig(se=True, **{**RESNET50, **kw})
        if not getattr(cfg, "se", False):
            raise ValueError("NativeSEResNet's blocks carry conv_down / conv_up: build its config with se=True")
        super().__init__(cfg, seed=seed)

    def _bottleneck_tail(self, h, pre, res, res_sink):
        return _SETailFn.apply(h, res, self, pre, BN_EPS, res_sink)
