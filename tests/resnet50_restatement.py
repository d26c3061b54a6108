"""Test helper (not a test): timm 0.5.4's `resnet50` restated in plain torch.nn -- timm and torchvision are absent.

  ResNet50            the nn.Module: conv1 7x7/2 -> bn1 -> ReLU -> max-pool 3/2/1 -> layers [3, 4, 6, 3] of Bottlenecks
                      (conv1 1x1 -> bn1 -> ReLU -> conv2 3x3 with the stride -> bn2 -> ReLU -> conv3 1x1 to 4 planes ->
                      bn3, + identity or downsample = Sequential(1x1 conv with the stride, BN), ReLU) -> global average
                      pool -> fc.  Module registration order = timm's, so state_dict() has timm's keys and order.
  forward_contract    the same forward, functional over a state dict, with the device's bf16 rounding points
                      (oracle.conformer_ref.conv2d operands; with maps the bf16 activation maps, as
                      oracle.resnet_ref.resnet18_forward emulates them for ResNet-18).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.conformer_ref import _bn_map, _RoundMap, conv2d
from oracle.resnet_ref import BN_EPS, _bn

LAYERS, WIDTHS = (3, 4, 6, 3), (64, 128, 256, 512)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride):
        super().__init__()
        outp = planes * self.expansion
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, outp, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(outp)
        if stride != 1 or inplanes != outp:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, outp, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(outp))
        else:
            self.downsample = None

    def forward(self, x):
        h = F.relu(self.bn1(self.conv1(x)))
        h = F.relu(self.bn2(self.conv2(h)))
        h = self.bn3(self.conv3(h))
        return F.relu(h + (x if self.downsample is None else self.downsample(x)))


class ResNet50(nn.Module):
    def __init__(self, num_classes, fc_bias=True):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inp = 64
        for si, (n, w) in enumerate(zip(LAYERS, WIDTHS)):
            blocks = []
            for bi in range(n):
                blocks.append(Bottleneck(inp, w, 2 if (si > 0 and bi == 0) else 1))
                inp = w * Bottleneck.expansion
            setattr(self, f"layer{si + 1}", nn.Sequential(*blocks))
        self.fc = nn.Linear(inp, num_classes, bias=fc_bias)

    def features(self, x):
        h = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        for si in range(4):
            h = getattr(self, f"layer{si + 1}")(h)
        return F.adaptive_avg_pool2d(h, 1).flatten(1)

    def forward(self, x):
        return self.fc(self.features(x))


def forward_contract(p, bufs, x, train=True, bf16=True, maps=True):
    """logits from parameters `p` / buffers `bufs` (dicts under timm's names); bf16 / maps as
    oracle.resnet_ref.resnet18_forward."""
    maps = bool(maps and bf16)
    if maps:
        rm = _RoundMap.apply

        def bn(y, pre):
            return _bn_map(y, p, bufs, pre, BN_EPS, train)
    else:
        def rm(v):
            return v

        def bn(y, pre):
            return _bn(y, p, bufs, pre, train)
    h = rm(F.max_pool2d(F.relu(_bn(F.conv2d(x, p["conv1.weight"], stride=2, padding=3), p, bufs, "bn1.", train)),
                        3, 2, 1))
    inp = 64
    for si, (n, w) in enumerate(zip(LAYERS, WIDTHS)):
        for bi in range(n):
            pre, stride = f"layer{si + 1}.{bi}.", 2 if (si > 0 and bi == 0) else 1
            o = rm(F.relu(bn(conv2d(h, p[pre + "conv1.weight"], bf16=bf16), pre + "bn1.")))
            o = rm(F.relu(bn(conv2d(o, p[pre + "conv2.weight"], stride=stride, padding=1, bf16=bf16), pre + "bn2.")))
            o = bn(conv2d(o, p[pre + "conv3.weight"], bf16=bf16), pre + "bn3.")
            sc = rm(bn(conv2d(h, p[pre + "downsample.0.weight"], stride=stride, bf16=bf16), pre + "downsample.1.")) \
                if (stride != 1 or inp != 4 * w) else h
            h = rm(F.relu(o + sc))
            inp = 4 * w
    return F.linear(F.adaptive_avg_pool2d(h, 1).flatten(1), p["fc.weight"], p.get("fc.bias"))
