"""Supervised triplet mode, host side: build_model's routing (code/build.py:198-200: IS_TRIPLET without IS_SSL
builds ModelwEmb with its default 256-d embedding) and the ctypes table of the two new entry points."""
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "endossl.h")


def _cfg(**over):
    from endossl.utils import AttrDict, with_defaults
    model = dict(NAME="vit_tiny_test", NUM_CLASSES=23, MARGIN="None", LOW_DIM=16)
    train = dict(IS_SSL=False)
    for k, v in over.items():
        (train if k == "IS_SSL" else model)[k] = v
    return with_defaults(AttrDict(MODEL=AttrDict(**model), TRAIN=AttrDict(**train), DATA=AttrDict(IMG_SIZE=64)))


def test_build_model_routes_triplet_to_embedding_head():
    from endossl.build import build_model
    from endossl.comatch_model import NativeViTEmb
    m = build_model(_cfg(IS_TRIPLET=True))
    assert isinstance(m, NativeViTEmb) and m.cfg.head == "emb"
    assert m.cfg.low_dim == 256  # ModelwEmb's default; MODEL.LOW_DIM (16 here) is not read on this branch
    sd = m.state_dict()
    for k in ("fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias", "fc.3.running_mean", "fc.3.running_var",
              "fc.3.num_batches_tracked", "fc.4.weight", "fc.4.bias", "head_emb.0.weight", "head_emb.0.bias",
              "head_emb.2.weight", "head_emb.2.bias"):
        assert k in sd, k
    assert tuple(sd["head_emb.0.weight"].shape) == (768, 128) and tuple(sd["head_emb.2.weight"].shape) == (256, 768)
    assert tuple(sd["fc.4.weight"].shape) == (23, 32)
    assert "head.weight" not in sd


def test_build_model_without_triplet_is_unchanged():
    from endossl.build import build_model
    from endossl.comatch_model import NativeViTEmb
    from endossl.vit import NativeViT
    m = build_model(_cfg(IS_TRIPLET=False))
    assert type(m) is NativeViT and m.cfg.head == "cls" and "head.weight" in m.state_dict()
    # IS_TRIPLET under IS_SSL is not this branch (code/build.py:175 comes first): FixMatch's plain ViT
    m = build_model(_cfg(IS_TRIPLET=True, IS_SSL=True))
    assert type(m) is NativeViT
    # a margin model is not this branch either (code/build.py:173)
    m = build_model(_cfg(IS_TRIPLET=True, MARGIN="arcface"))
    assert not isinstance(m, NativeViTEmb)


def test_build_model_comatch_still_takes_low_dim():
    from endossl.build import build_model
    from endossl.comatch_model import NativeViTEmb
    m = build_model(_cfg(TYPE_SEMI="CoMatch", IS_SSL=True, IS_TRIPLET=True))
    assert isinstance(m, NativeViTEmb) and m.cfg.low_dim == 16


def test_signatures_have_the_triplet_entry_points():
    from endossl import _lib
    txt = open(HEADER).read().replace("\n", " ")
    for name in ("es_triplet_fwd_bwd", "es_softmax_predict"):
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.I
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/endossl.h"
        params = [p.strip() for p in m.group(1).split(",") if p.strip()]
        assert len(params) == len(args), (name, params)
        for p, a in zip(params, args):  # pointers and the stream as void*, int as c_int, float as c_float
            want = _lib.V if ("*" in p or "hipStream_t" in p) else (_lib.F if p.startswith("float") else _lib.I)
            assert a is want, (name, p)
