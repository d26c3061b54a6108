"""Test helper (not a test): the reference's `resnet50se` -- SEResNet(Bottleneck, [3, 4, 6, 3]), code/models/se.py:8-119
-- restated in plain torch.nn, with a global average pool before fc (the reference's nn.AvgPool2d(7) equals it at
224^2, where the last map is 7 x 7, and fails or reads a corner at other sizes).  Pinned to the reference by the
block-level fixtures tests/golden/se_block_{identity,downsample}.npz, which the reference's own Bottleneck produced
(tests/test_seresnet_cpu.py), and by the state-dict fixture tests/golden/seresnet50_state_dict.json.

  SEBottleneck        conv1 1x1 -> bn1 -> ReLU -> conv2 3x3 with the stride -> bn2 -> ReLU -> conv3 1x1 to 4 planes ->
                      bn3 = o; gate s = sigmoid(conv_up(relu(conv_down(global_pool(o))))) (both 1x1, bias-free,
                      planes / 4 channels in between); relu(s * o + shortcut), shortcut = x or
                      downsample = Sequential(1x1 conv with the stride, BN).  Registration order = the reference's.
  SEResNet50          conv1 7x7/2 -> bn1 -> ReLU -> max-pool 3/2/1 -> layers [3, 4, 6, 3] -> global pool -> fc
  forward_contract    the same forward, functional over a state dict, rounding where the device does with bf16 convs
                      and maps:
                        * conv operands rounded to bf16, fp32 accumulation (oracle.conformer_ref.conv2d);
                        * every conv output is stored as a bf16 map; a BatchNorm takes its batch statistics from
                          the fp32 conv output and normalises the rounded map (oracle.conformer_ref._bn_map);
                        * bn1 / bn2 + ReLU and the downsample's BatchNorm are rounded to bf16 maps;
                        * the tail: o = bn3 of the rounded conv3 map is kept in fp32 and never stored; the squeeze
                          sums the bf16 conv3 map in fp32 (so the pooled a is the fp32 pool of o), the gate
                          (conv_down, ReLU, conv_up, sigmoid) is fp32 throughout with fp32 weights, and
                          out = relu(s * o + shortcut) is rounded to bf16 once.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.conformer_ref import _bn_map, _RoundMap, conv2d
from oracle.resnet_ref import BN_EPS, _bn

LAYERS, WIDTHS = (3, 4, 6, 3), (64, 128, 256, 512)


class SEBottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        outp = planes * self.expansion
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, outp, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(outp)
        self.conv_down = nn.Conv2d(outp, planes // 4, 1, bias=False)
        self.conv_up = nn.Conv2d(planes // 4, outp, 1, bias=False)
        if stride != 1 or inplanes != outp:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, outp, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(outp))
        else:
            self.downsample = None

    def forward(self, x):
        h = F.relu(self.bn1(self.conv1(x)))
        h = F.relu(self.bn2(self.conv2(h)))
        o = self.bn3(self.conv3(h))
        s = torch.sigmoid(self.conv_up(F.relu(self.conv_down(F.adaptive_avg_pool2d(o, 1)))))
        return F.relu(s * o + (x if self.downsample is None else self.downsample(x)))


class SEResNet50(nn.Module):
    def __init__(self, num_classes, layers=LAYERS, widths=WIDTHS):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inp = 64
        for si, (n, w) in enumerate(zip(layers, widths)):
            blocks = []
            for bi in range(n):
                blocks.append(SEBottleneck(inp, w, 2 if (si > 0 and bi == 0) else 1))
                inp = w * SEBottleneck.expansion
            setattr(self, f"layer{si + 1}", nn.Sequential(*blocks))
        self.nlayers = len(layers)
        self.fc = nn.Linear(inp, num_classes)
        for m in self.modules():  # the reference's init rule (se.py:78-84)
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0.0, (2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)) ** 0.5)

    def forward(self, x):
        h = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        for si in range(self.nlayers):
            h = getattr(self, f"layer{si + 1}")(h)
        return self.fc(F.adaptive_avg_pool2d(h, 1).flatten(1))


def forward_contract(p, bufs, x, train=True, bf16=True, maps=True):
    """logits from parameters `p` / buffers `bufs` (dicts under the reference's names); the rounding points are
    listed in the module docstring.  bf16 False: plain fp32."""
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
            o = bn(conv2d(o, p[pre + "conv3.weight"], bf16=bf16), pre + "bn3.")  # fp32, never stored
            a = F.adaptive_avg_pool2d(o, 1)
            s = torch.sigmoid(F.conv2d(F.relu(F.conv2d(a, p[pre + "conv_down.weight"])), p[pre + "conv_up.weight"]))
            sc = rm(bn(conv2d(h, p[pre + "downsample.0.weight"], stride=stride, bf16=bf16), pre + "downsample.1.")) \
                if (stride != 1 or inp != 4 * w) else h
            h = rm(F.relu(s * o + sc))
            inp = 4 * w
    return F.linear(F.adaptive_avg_pool2d(h, 1).flatten(1), p["fc.weight"], p["fc.bias"])
