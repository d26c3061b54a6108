"""build_model (code/build.py:29-222) for the SSL hot path.

The reference builds its FixMatch backbone with `timm.create_model(name, pretrained=True,
num_classes=C)` (code/build.py:196-197) -- a network weight download, and timm is absent here.
This factory returns the native ViT for the `vit_*` names instead (random timm-style init, or a
checkpoint from MODEL.PRE_TRAIN_PATH loaded with weights_only=True, head dropped when its class
count differs -- the reference re-heads abnormality checkpoints the same way, :180-194).
For MODEL.TYPE_SEMI == 'CoMatch' it returns ModelwEmb over the native ViT (:175-178;
comatch_model.NativeViTEmb, forward -> (logits, fts, z), LOW_DIM-d embedding); the supervised
triplet mode (MODEL.IS_TRIPLET without TRAIN.IS_SSL, :198-200) gets the same model with ModelwEmb's
default 256-d embedding.
For 'conformer' it returns the native Conformer-Ti of code/build.py:135-142 (patch 16,
channel_ratio 1, embed 384, depth 12, 6 heads, qkv_bias; conformer.NativeConformer, forward ->
(conv_logits, trans_logits)) -- SemiFormer's backbone.  With MODEL.MARGIN set (code/build.py:173-174, checked
first) `resnet18` / `resnet50` give resnet.ModelMargin, the ResNet with a bias-free fc that the angular-margin step
reads; a margin with any other backbone raises (ModelMargin needs `.fc`) unless IS_TRIPLET is set too, which the
trainer tests first and which keeps building the plain backbone.
`resnet18` and `resnet50` (the backbone ten of the reference's eighteen configs name) give resnet.NativeResNet with
timm's state_dict -- for FixMatch and for the plain supervised mode.  The modes that wrap the backbone in ModelwEmb
(CoMatch, IS_TRIPLET without SSL, EZBM) get comatch_model.NativeResNetEmb -- ModelwEmb over the native ResNet trunk,
LOW_DIM-d under CoMatch and 256-d otherwise, MODEL.PRE_TRAIN_PATH (the 2-class abnormality checkpoint) loaded into the
trunk -- when asked to: build_model(config, cnn_emb=True), or ENDOSSL_CNN_EMB=1 for a script that calls
build_model(config).  Without the switch they raise for resnet50 instead of returning a logits-only model (and
resnet18 keeps its logits-only model), as before NativeResNetEmb existed.  `resnet50se` (code/build.py:152-170, the reference's own
SEResNet, code/models/se.py) gives resnet.NativeSEResNet for FixMatch and the plain supervised mode, with the 2-class
abnormality checkpoint of MODEL.PRE_TRAIN_PATH re-headed as the reference does; IS_TRIPLET, CoMatch and MARGIN raise
for it.  `densenet161` (three configs, `local_semisupervised.yaml` among them) gives densenet.NativeDenseNet with
torchvision's state_dict for FixMatch and the plain supervised mode, MODEL.PRE_TRAIN_PATH re-headed the same way
(`classifier.*` dropped when its class count differs); CoMatch, IS_TRIPLET without SSL and MARGIN raise for it.
Other CNN / Swin backbones are outside the hot path.
"""
import os

import torch

from .comatch_model import NativeResNetEmb, NativeViTEmb
from .conformer import ConformerConfig, NativeConformer
from .densenet import DENSENET161, DenseNetConfig, NativeDenseNet
from .resnet import RESNET50, ModelMargin, NativeResNet, NativeSEResNet, ResNetConfig
from .vit import VIT_CONFIGS, NativeViT, ViTConfig

TRIPLET_LOW_DIM = 256  # ModelwEmb's default low_dim (code/models/custom_model.py:147)
RESNETS = {"resnet18": {}, "resnet50": RESNET50}  # ResNetConfig arguments per timm name

def _build_resnet50se(config, C, seed):
    """code/build.py:152-170: SEResNet(Bottleneck, [3, 4, 6, 3]) (code/models/se.py) -> NativeSEResNet.  The branch is
    tested before MARGIN / IS_SSL there; the modes whose trainer cannot use the logits-only model it builds raise."""
    if getattr(config.MODEL, "IS_TRIPLET", False):  # :153-155
        raise NotImplementedError("resnet50se for IS_TRIPLET: ModelwEmb (code/models/custom_model.py:136-213) over "
                                  "a CNN trunk is not built -- the native embedding-head models are the ViTs; "
                                  "resnet50se is native for FixMatch and plain supervised")
    if getattr(config.TRAIN, "IS_SSL", True) and getattr(config.MODEL, "TYPE_SEMI", "FixMatch") == "CoMatch":
        raise NotImplementedError("resnet50se for TYPE_SEMI 'CoMatch': the reference builds a logits-only SEResNet "
                                  "(code/build.py:156-170) that its CoMatch trainer, which reads (logits, fts, z), "
                                  "cannot use; ModelwEmb over a CNN trunk is not built")
    if str(getattr(config.MODEL, "MARGIN", "None")) != "None":
        raise NotImplementedError("resnet50se with MODEL.MARGIN: the reference ignores the margin at build "
                                  "(code/build.py:152 precedes :173) and its trainer then fails on model.backbone; "
                                  "the native ModelMargin backbones are resnet18 and resnet50")
    model = NativeSEResNet(ResNetConfig(num_classes=C, se=True, **RESNET50), seed=seed)
    path = getattr(config.MODEL, "PRE_TRAIN_PATH", "None")
    if path not in (None, "None", ""):
        # :158-165 loads the 2-class abnormality checkpoint and re-heads it (build_head: a plain Linear)
        ck = torch.load(path, map_location="cpu", weights_only=True)
        sd = ck.get("model_state_dict", ck)
        if sd.get("fc.weight") is not None and sd["fc.weight"].shape[0] != C:
            sd = {k: v for k, v in sd.items() if not k.startswith("fc.")}
        model.load_state_dict(sd, strict=False)
    return model


def _emb_mode(config):
    """The mode that wraps the backbone in ModelwEmb (code/build.py:175-178,198-200), or None: (message text,
    low_dim).  CoMatch reads MODEL.LOW_DIM; the triplet branch passes none, so ModelwEmb's default holds."""
    ssl = bool(getattr(getattr(config, "TRAIN", None), "IS_SSL", True))  # a config without TRAIN: the SSL default
    if ssl and getattr(config.MODEL, "TYPE_SEMI", "FixMatch") == "CoMatch":
        return "TYPE_SEMI 'CoMatch'", int(getattr(config.MODEL, "LOW_DIM", 64))
    if not ssl and getattr(config.MODEL, "IS_TRIPLET", False):
        return "IS_TRIPLET without IS_SSL (the triplet mode, EZBM)", TRIPLET_LOW_DIM
    return None


def _build_resnet_emb(config, name, C, low_dim, seed):
    """ModelwEmb over the native ResNet trunk.  MODEL.PRE_TRAIN_PATH: the 2-class abnormality checkpoint into the
    trunk (code/models/custom_model.py:180-190: its own fc dropped, the heads freshly initialised)."""
    model = NativeResNetEmb(ResNetConfig(num_classes=C, head="emb", low_dim=low_dim, **RESNETS[name]), seed=seed)
    path = getattr(config.MODEL, "PRE_TRAIN_PATH", "None")
    if path not in (None, "None", ""):
        ck = torch.load(path, map_location="cpu", weights_only=True)
        model.load_trunk(ck["model_state_dict"])
    return model


def _build_densenet161(config, C, seed):
    """code/build.py:196-197,218-220: timm.create_model('densenet161', num_classes=C) -> NativeDenseNet, for FixMatch
    and the plain supervised mode.  The modes that need more than logits from the backbone raise."""
    if str(getattr(config.MODEL, "MARGIN", "None")) != "None":  # code/build.py:173-174, checked first there
        raise NotImplementedError("MODEL.MARGIN with backbone 'densenet161': ModelMargin needs a backbone with a .fc "
                                  "classifier (code/models/custom_model.py:129) and timm's densenet161 has "
                                  "`classifier`; the native ModelMargin backbones are resnet18 and resnet50")
    mode = _emb_mode(config)
    if mode is not None:
        raise NotImplementedError(f"densenet161 for {mode[0]}: ModelwEmb (code/models/custom_model.py:136-213) over "
                                  "the DenseNet trunk is not built -- densenet161 is native for FixMatch and plain "
                                  "supervised")
    model = NativeDenseNet(DenseNetConfig(num_classes=C, **DENSENET161), seed=seed)
    path = getattr(config.MODEL, "PRE_TRAIN_PATH", "None")
    if path not in (None, "None", ""):
        # code/build.py:190-193,213-216: the 2-class abnormality checkpoint, re-headed (build_head: a plain Linear)
        ck = torch.load(path, map_location="cpu", weights_only=True)
        sd = ck.get("model_state_dict", ck)
        if sd.get("classifier.weight") is not None and sd["classifier.weight"].shape[0] != C:
            sd = {k: v for k, v in sd.items() if not k.startswith("classifier.")}
        model.load_state_dict(sd, strict=False)
    return model


def build_model(config, is_pathology=True, seed=0, cnn_emb=None):
    """cnn_emb: build ModelwEmb over resnet18 / resnet50 (comatch_model.NativeResNetEmb) for the modes that need it;
    None reads ENDOSSL_CNN_EMB (default "0": those modes keep raising for resnet50, and resnet18 keeps its
    logits-only model)."""
    if cnn_emb is None:
        cnn_emb = os.environ.get("ENDOSSL_CNN_EMB", "0") == "1"
    name = config.MODEL.NAME
    C = int(config.MODEL.NUM_CLASSES)
    if name == "resnet50se":
        return _build_resnet50se(config, C, seed)
    if name == "densenet161":
        return _build_densenet161(config, C, seed)
    if name != "conformer" and str(getattr(config.MODEL, "MARGIN", "None")) != "None":
        # code/build.py:173-174: checked before IS_SSL / IS_TRIPLET / PRE_TRAIN_PATH, none of which is read here
        if name in RESNETS:
            return ModelMargin(ResNetConfig(num_classes=C, fc_bias=False, **RESNETS[name]), seed=seed)
        # With IS_TRIPLET also set the trainer never reads the margin (code/supervised.py:84 tests the triplet
        # first): such a config keeps building the plain backbone below, as before the margin mode existed.
        if not getattr(config.MODEL, "IS_TRIPLET", False):
            raise NotImplementedError(f"MODEL.MARGIN with backbone {name!r}: ModelMargin needs a backbone with a .fc "
                                      "classifier (code/models/custom_model.py:129); the native ones are resnet18 and "
                                      "resnet50")
    if name == "conformer":
        img = int(config.DATA.IMG_SIZE) if "IMG_SIZE" in config.DATA else 224
        model = NativeConformer(ConformerConfig(img_size=img, patch=16, channel_ratio=1, embed_dim=384, depth=12,
                                                heads=6, mlp_ratio=4, num_classes=C), seed=seed)
        path = getattr(config.MODEL, "PRE_TRAIN_PATH", "None")
        if path not in (None, "None", ""):
            ck = torch.load(path, map_location="cpu", weights_only=True)
            sd = ck.get("model_state_dict", ck)
            sd = {k: v for k, v in sd.items() if not k.startswith(("conv_cls_head.", "trans_cls_head."))
                  or v.shape[0] == C}
            model.load_state_dict(sd, strict=False)
        return model
    if name in RESNETS:
        # the supervised baseline (BASELINE configs[0]; code/build.py:218-220 timm.create_model('resnet18',
        # num_classes=C): ImageNet weights are a download, unavailable here -- timm's random init) and resnet50,
        # FixMatch's (code/build.py:196-197) and the supervised mode's backbone in most reference configs
        # code/build.py:175-178,198-200 wrap the backbone in ModelwEmb (logits, fts, z) -- checked before
        # PRE_TRAIN_PATH there too; the triplet step and both EZBM stages read fts / z
        mode = _emb_mode(config)
        if mode is not None and cnn_emb:
            return _build_resnet_emb(config, name, C, mode[1], seed)
        if mode is not None and name != "resnet18":
            raise NotImplementedError(f"{name} for {mode[0]}: ModelwEmb (code/models/custom_model.py:136-213) over "
                                      "a CNN trunk is not built by default -- the native embedding-head models are "
                                      f"the ViTs; {name} is native for FixMatch, plain supervised and MODEL.MARGIN.  "
                                      "build_model(config, cnn_emb=True) or ENDOSSL_CNN_EMB=1 builds "
                                      "NativeResNetEmb, ModelwEmb over the native ResNet trunk")
        if getattr(config.MODEL, "PRE_TRAIN_PATH", "None") not in (None, "None", ""):
            raise NotImplementedError(f"{name} + PRE_TRAIN_PATH swaps fc for build_head's MLP "
                                      "(code/build.py:202-211): outside the native scope")
        return NativeResNet(ResNetConfig(num_classes=C, **RESNETS[name]), seed=seed)
    if name not in VIT_CONFIGS:
        raise NotImplementedError(f"backbone {name!r}: native builds exist for {sorted(VIT_CONFIGS)}")
    comatch = getattr(config.MODEL, "TYPE_SEMI", "FixMatch") == "CoMatch" and getattr(config.TRAIN, "IS_SSL", True)
    # code/build.py:198-200: ModelwEmb without a low_dim argument -- its default, MODEL.LOW_DIM is not read
    triplet = (bool(getattr(config.MODEL, "IS_TRIPLET", False)) and not getattr(config.TRAIN, "IS_SSL", True)
               and str(getattr(config.MODEL, "MARGIN", "None")) == "None")
    kw = dict(VIT_CONFIGS[name])
    if "IMG_SIZE" in config.DATA and int(config.DATA.IMG_SIZE) != kw["img_size"]:
        kw["img_size"] = int(config.DATA.IMG_SIZE)
    if comatch:
        model = NativeViTEmb(ViTConfig(num_classes=C, head="emb", low_dim=int(config.MODEL.LOW_DIM), **kw), seed=seed)
    elif triplet:
        model = NativeViTEmb(ViTConfig(num_classes=C, head="emb", low_dim=TRIPLET_LOW_DIM, **kw), seed=seed)
    else:
        model = NativeViT(ViTConfig(num_classes=C, **kw), seed=seed)
    path = getattr(config.MODEL, "PRE_TRAIN_PATH", "None")
    if path not in (None, "None", ""):
        ck = torch.load(path, map_location="cpu", weights_only=True)
        sd = ck.get("model_state_dict", ck)
        if sd.get("head.weight") is not None and sd["head.weight"].shape[0] != C:
            sd = {k: v for k, v in sd.items() if not k.startswith("head.")}
        model.load_state_dict(sd, strict=False)
    return model
