"""Generate the SE-ResNet fixtures under tests/golden/ by running the REFERENCE model classes.

Test infrastructure only; like make_golden.py it runs where the read-only reference tree is mounted and refuses to
run anywhere else.  The reference's `SEResNet` / `Bottleneck` (code/models/se.py:8-119) are imported (never
copied) and run as they stand.  What is committed is DATA only: a JSON list and arrays loadable with
allow_pickle=False.

  seresnet50_state_dict.json   [[name, shape], ...] of SEResNet(Bottleneck, [3, 4, 6, 3], num_classes=23)
                               .state_dict(), in its order (code/build.py:158,167 builds this model)
  se_block_identity.npz        Bottleneck(128, 32): stride 1, no downsample      } inplanes / planes chosen so that
  se_block_downsample.npz      Bottleneck(64, 32, stride 2, downsample 1x1/2+BN) } the identity block's 128 = 4 * 32
      each: two 8 x 8 inputs, train mode, one forward + backward of sum(out * g) in float64 and in float32
        inplanes, planes, stride
        init/<name>         the block's state_dict before the forward (fp32; BatchNorm weights / biases and running
                            statistics randomised so that no term of the tail's backward vanishes)
        x [2, inplanes, 8, 8], g [2, 128, Ho, Wo]     fp32 (the float64 run casts the same values up)
        out, dx, grad/<name>, buf/<name>              the reference in float64 (buf: buffers after the forward)
        out_f32, dx_f32, grad_f32/<name>, buf_f32/<name>   the reference in float32

Usage (from the repo root):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_seresnet.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

import make_golden

OUT = os.path.dirname(os.path.abspath(__file__))
PLANES = 32


def _import_reference_se():
    if not os.path.isdir(make_golden.REF):
        raise SystemExit("make_golden_seresnet.py needs the reference tree (build container only)")
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    sys.path.insert(0, make_golden.REF)
    from models import se as ref_se
    return ref_se


def _block(ref_se, inplanes, stride, seed):
    torch.manual_seed(seed)
    ds = None
    if stride != 1 or inplanes != PLANES * 4:
        ds = nn.Sequential(nn.Conv2d(inplanes, PLANES * 4, kernel_size=1, stride=stride, bias=False),
                           nn.BatchNorm2d(PLANES * 4))  # SEResNet._make_layer's downsample (se.py:88-93)
    blk = ref_se.Bottleneck(inplanes, PLANES, stride, ds)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, t in blk.state_dict().items():
            if t.dim() == 4:
                t.normal_(0.0, (2.0 / (t.shape[0] * t.shape[2] * t.shape[3])) ** 0.5, generator=g)  # se.py:79-81
            elif name.endswith("running_var"):
                t.uniform_(0.5, 1.5, generator=g)
            elif name.endswith("running_mean"):
                t.normal_(0.0, 0.1, generator=g)
            elif name.endswith("weight"):
                t.uniform_(0.5, 1.5, generator=g)
            elif name.endswith("bias"):
                t.normal_(0.0, 0.2, generator=g)
    return blk


def _run(blk, init, x, g, dtype):
    import copy
    b = copy.deepcopy(blk).to(dtype).train()
    b.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in init.items()})
    xi = x.to(dtype).clone().requires_grad_(True)
    out = b(xi)
    assert out.dtype == dtype
    (out * g.to(dtype)).sum().backward()
    grads = {k: p.grad.numpy() for k, p in b.named_parameters()}
    bufs = {k: v.detach().numpy() for k, v in b.named_buffers()}
    return out.detach().numpy(), xi.grad.numpy(), grads, bufs


def main():
    ref_se = _import_reference_se()
    model = ref_se.SEResNet(ref_se.Bottleneck, [3, 4, 6, 3], num_classes=23)
    layout = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(OUT, "seresnet50_state_dict.json"), "w") as f:
        json.dump(layout, f)
        f.write("\n")
    print(f"seresnet50_state_dict.json: {len(layout)} entries, "
          f"{sum(p.numel() for p in model.parameters())} parameters")
    for tag, inplanes, stride, seed in (("identity", PLANES * 4, 1, 11), ("downsample", 64, 2, 21)):
        blk = _block(ref_se, inplanes, stride, seed)
        assert (blk.downsample is None) == (tag == "identity")
        init = {k: v.detach().clone() for k, v in blk.state_dict().items()}
        gen = torch.Generator().manual_seed(seed + 2)
        x = torch.randn(2, inplanes, 8, 8, generator=gen)
        ho = 8 // stride
        g = torch.randn(2, PLANES * 4, ho, ho, generator=gen)
        o64, dx64, g64, b64 = _run(blk, init, x, g, torch.float64)
        o32, dx32, g32, b32 = _run(blk, init, x, g, torch.float32)
        assert (o64 == 0).any() and (o64 > 0).any()  # both sides of the last ReLU
        arrays = dict(inplanes=np.int64(inplanes), planes=np.int64(PLANES), stride=np.int64(stride), x=x.numpy(),
                      g=g.numpy(), out=o64, dx=dx64, out_f32=o32, dx_f32=dx32)
        arrays.update({"init/" + k: v.numpy() for k, v in init.items()})
        arrays.update({"grad/" + k: v for k, v in g64.items()})
        arrays.update({"grad_f32/" + k: v for k, v in g32.items()})
        arrays.update({"buf/" + k: v for k, v in b64.items()})
        arrays.update({"buf_f32/" + k: v for k, v in b32.items()})
        path = os.path.join(OUT, f"se_block_{tag}.npz")
        np.savez_compressed(path, **arrays)
        print(f"se_block_{tag}.npz: {os.path.getsize(path)} bytes, |out| max {np.abs(o64).max():.3f}, "
              f"|out64 - out32| max {np.abs(o64 - o32).max():.2e}")


if __name__ == "__main__":
    main()
