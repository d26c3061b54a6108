"""Test helper (not a test): timm 0.5.4's / torchvision's DenseNet restated in plain torch.nn -- both are absent.

  DenseNet            the nn.Module for any endossl.densenet.DenseNetConfig, with torchvision's module names
                      (features.conv0 / norm0 / denseblock{b}.denselayer{l}.{norm1,conv1,norm2,conv2} /
                      transition{b}.{norm,conv} / norm5, classifier), so state_dict() has torchvision's keys and order.
  forward_contract    the same forward, functional over a state dict, with the device's bf16 rounding points: every
                      conv after the stem takes bf16 operands (padded ones included: the padding is zero), a conv
                      output is stored as a bf16 map while its BatchNorm statistics come from the fp32 accumulators
                      (a block's input: from the stored map, one strided pass), a BatchNorm + ReLU applied in a
                      conv's gathers is rounded to the map type, the pools accumulate in fp32.
"""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

BN_EPS = 1e-5


class _DenseLayer(nn.Module):
    def __init__(self, cin, growth, bn_size):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, bn_size * growth, 1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth)
        self.conv2 = nn.Conv2d(bn_size * growth, growth, 3, padding=1, bias=False)

    def forward(self, x):
        return self.conv2(F.relu(self.norm2(self.conv1(F.relu(self.norm1(x))))))


class _DenseBlock(nn.Module):
    def __init__(self, n, cin, growth, bn_size):
        super().__init__()
        for l in range(n):
            self.add_module(f"denselayer{l + 1}", _DenseLayer(cin + l * growth, growth, bn_size))

    def forward(self, x):
        for layer in self.children():
            x = torch.cat([x, layer(x)], 1)
        return x


class _Transition(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm = nn.BatchNorm2d(cin)
        self.conv = nn.Conv2d(cin, cout, 1, bias=False)

    def forward(self, x):
        return F.avg_pool2d(self.conv(F.relu(self.norm(x))), 2, 2)


class DenseNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        f0 = cfg.init_features
        mods = OrderedDict(conv0=nn.Conv2d(3, f0, 7, stride=2, padding=3, bias=False), norm0=nn.BatchNorm2d(f0))
        nb = len(cfg.block_config)
        for b, (c0, n, cout) in enumerate(cfg.blocks(), 1):
            mods[f"denseblock{b}"] = _DenseBlock(n, c0, cfg.growth, cfg.bn_size)
            if b < nb:
                mods[f"transition{b}"] = _Transition(cout, cout // 2)
        mods["norm5"] = nn.BatchNorm2d(cfg.num_features)
        self.features = nn.Sequential(mods)
        self.classifier = nn.Linear(cfg.num_features, cfg.num_classes)

    def forward(self, x):
        f = self.features
        h = F.max_pool2d(F.relu(f.norm0(f.conv0(x))), 3, 2, 1)
        for name, mod in f.named_children():
            if name.startswith(("denseblock", "transition")):
                h = mod(h)
        h = F.relu(f.norm5(h))
        return self.classifier(F.adaptive_avg_pool2d(h, 1).flatten(1))


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def forward_contract(p, bufs, x, train=True, bf16=True, maps=True, cfg=None):
    """logits from parameters `p` / buffers `bufs` (dicts under torchvision's names).  bf16: the convs after the stem
    on bf16 operands; maps (with bf16): bf16 activation maps; cfg: the DenseNetConfig (default densenet161).  Call
    under torch.no_grad()."""
    if cfg is None:
        from endossl.densenet import DENSENET161, DenseNetConfig
        cfg = DenseNetConfig(**DENSENET161)
    maps = bool(maps and bf16)
    rm = _bf if maps else (lambda v: v)
    op = _bf if bf16 else (lambda v: v)

    def bn(src, stored, pre):
        """BatchNorm over `stored` (the map as the device keeps it) with batch statistics of `src` (the values the
        device computed them from), buffers updated in train mode."""
        sh = (1, -1, 1, 1)
        if not train:
            mean, var = bufs[pre + "running_mean"], bufs[pre + "running_var"]
        else:
            n = src.numel() // src.shape[1]
            mean, var = src.mean((0, 2, 3)), src.var((0, 2, 3), unbiased=False)
            bufs[pre + "running_mean"].mul_(0.9).add_(0.1 * mean)
            bufs[pre + "running_var"].mul_(0.9).add_(0.1 * var * n / max(n - 1, 1))
            bufs[pre + "num_batches_tracked"] += 1
        return (stored - mean.view(sh)) * torch.rsqrt(var.view(sh) + BN_EPS) * p[pre + "weight"].view(sh) + \
            p[pre + "bias"].view(sh)

    def conv(a, name, padding=0):
        return F.conv2d(op(a), op(p[name]), padding=padding)

    h = F.conv2d(x, p["features.conv0.weight"], stride=2, padding=3)
    h = rm(F.max_pool2d(F.relu(bn(h, h, "features.norm0.")), 3, 2, 1))
    src = h  # a block input's statistics: one pass over the stored map
    nb = len(cfg.block_config)
    for b, (c0, n, cout) in enumerate(cfg.blocks(), 1):
        for l in range(n):
            pre = f"features.denseblock{b}.denselayer{l + 1}."
            y1 = conv(rm(F.relu(bn(src, h, pre + "norm1."))), pre + "conv1.weight")
            y2 = conv(rm(F.relu(bn(y1, rm(y1), pre + "norm2."))), pre + "conv2.weight", padding=1)
            src, h = torch.cat([src, y2], 1), torch.cat([h, rm(y2)], 1)
        if b < nb:
            pre = f"features.transition{b}."
            t = rm(conv(rm(F.relu(bn(src, h, pre + "norm."))), pre + "conv.weight"))
            h = rm(F.avg_pool2d(t, 2, 2))
            src = h
    h = rm(F.relu(bn(src, h, "features.norm5.")))
    return F.linear(F.adaptive_avg_pool2d(h, 1).flatten(1), p["classifier.weight"], p["classifier.bias"])
