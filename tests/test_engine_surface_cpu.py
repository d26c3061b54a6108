"""The host-side surfaces the trainers call, checked without a GPU: method signatures and the autograd
bindings of the native models (a method shadowed by a stray definition fails here, not on the GPU box)."""
import inspect
import os
import sys
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "endoscopy-image-classification_amd"))
from endossl import conformer, vit  # noqa: E402


def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_vit_engine_surface():
    assert _params(vit.Engine.forward) == ["self", "flat", "images_list", "train"]
    assert _params(vit.Engine.backward)[:4] == ["self", "flat", "grad", "dlogits"]
    assert issubclass(vit._ViTFunction, torch.autograd.Function)
    assert _params(vit._ViTFunction.forward)[:3] == ["ctx", "x", "module"]
    # every Engine method is a plain function of the class (no autograd-style ctx methods leaked into it)
    for name, fn in inspect.getmembers(vit.Engine, inspect.isfunction):
        ps = _params(fn)
        assert not ps or ps[0] == "self", (name, ps)


def test_conformer_autograd_bindings():
    for name in ("_ConvFn", "_BNFn", "_MaxPoolFn"):
        cls = getattr(conformer, name)
        assert issubclass(cls, torch.autograd.Function), name
        assert _params(cls.forward)[0] == "ctx" and _params(cls.backward)[0] == "ctx", name


def test_split_q_rows_fill_the_token_steps_of_the_tile_chosen():
    """Engine.backward's choice of the CLS-rows-only Q weight gradient (Engine._split_q_rows).  The expectations are
    written down from the kernels' token steps (csrc/gemm.hip: 32 rows on the 128 x 128 tile and in the grouped
    launch, 64 on the 384 x 192 tile, which tn_pick gives a D x D problem only where D % 384 == 0): at the CLS-row
    strides a partial step would read rows past the token buffers, so n must be a whole number of steps."""
    def f(n, D, pin, shared, precision="bf16"):
        eng = types.SimpleNamespace(cfg=types.SimpleNamespace(dim=D), precision=precision,
                                    _tn_shared=lambda M, N1, N2: shared and N1 % 384 == 0 and N2 % 192 == 0)
        return vit.Engine._split_q_rows(eng, n, pin)

    for D in (128, 384, 768):
        for pin in (-1, 0, 7):
            assert not f(40, D, pin, False) and not f(16, D, pin, True)  # never a partial 32-row step
            assert f(64, D, pin, True) and f(128, D, pin, False)  # whole steps under either tile
    # n % 64 == 32: fine on the 128 x 128 tile ...
    assert f(32, 384, -1, False) and f(96, 768, -1, False) and f(96, 384, 0, True)
    assert f(32, 128, 7, False) and f(96, 128, -1, True)  # ... and at D = 128 the big tile never tiles
    # ... but not where the 384 x 192 tile is pinned, named by the engine, or picked by the library (n >= 65536)
    assert not f(32, 384, 7, False) and not f(96, 768, 7, False) and not f(160, 384, 7, True)
    assert not f(96, 384, -1, True) and not f(65536 + 32, 384, -1, False)
    assert f(65536 + 32, 384, 0, False) and f(65536 + 64, 384, -1, False)
    assert f(96, 384, 7, True, precision="fp32")  # the fp32 parity engine has no kernel variants
    # the real _tn_shared: a token axis below TN_SHARE_MIN_M never names the big tile
    eng = types.SimpleNamespace(cfg=types.SimpleNamespace(dim=384), precision="bf16", TN_SHARE=0.5, overlap=True,
                                TN_SHARE_MIN_M=16384)
    eng._tn_shared = types.MethodType(vit.Engine._tn_shared, eng)
    assert vit.Engine._split_q_rows(eng, 96, -1) and not vit.Engine._split_q_rows(eng, 16384 + 32, -1)
