"""ModelwEmb over ResNet-50 in plain torch.nn, written from the layer list (timm is absent): the model the CoMatch,
triplet and EZBM configs with NAME 'resnet50' train.

  model     the ResNet-50 restatement (tests/resnet50_restatement.py) whose `fc` is replaced by the complex head
  fc        = model.fc: Linear(D, D/4) -> ReLU -> Dropout(0.2) -> BatchNorm1d(D/4) -> Linear(D/4, C)  (0, 3, 4)
  backbone  Sequential over model's children without the last (fc): the same tensors a second time
  head_emb  Linear(D, 3L) -> LeakyReLU(0.1) -> Linear(3L, L), then x / |x|_2                          (0, 2)

Attributes are registered in that order, so state_dict() lists model.* / fc.* / backbone.* / head_emb.*.
forward(x, keep) -> (logits, fts, z); keep: the Dropout keep-mask [n, D/4] to replay (None: no dropout), scaled
by 1 / (1 - 0.2) as nn.Dropout does."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from resnet50_restatement import ResNet50

DROP_P, LEAKY = 0.2, 0.1


def build_head(D, C):
    return nn.Sequential(nn.Linear(D, D // 4), nn.ReLU(), nn.Dropout(DROP_P), nn.BatchNorm1d(D // 4),
                         nn.Linear(D // 4, C))


class ModelwEmb(nn.Module):
    def __init__(self, num_classes, low_dim=256, base=None):
        super().__init__()
        self.model = base if base is not None else ResNet50(num_classes)
        D = self.model.fc.in_features
        self.model.fc = build_head(D, num_classes)
        self.fc = self.model.fc
        self.backbone = nn.Sequential(*list(self.model.children())[:-1])
        self.head_emb = nn.Sequential(nn.Linear(D, 3 * low_dim), nn.LeakyReLU(LEAKY), nn.Linear(3 * low_dim, low_dim))

    def heads(self, fts, keep=None):
        u = F.relu(self.fc[0](fts))
        if keep is not None:
            u = u * (keep.to(u.dtype) / (1.0 - DROP_P))
        logits = self.fc[4](self.fc[3](u))
        v = self.head_emb(fts)
        return logits, v / v.pow(2).sum(1, keepdim=True).pow(0.5)

    def forward(self, x, keep=None):
        fts = self.model.features(x)
        logits, z = self.heads(fts, keep)
        return logits, fts, z


def native_keys(ref):
    """The restatement's state_dict keys as the native model writes them: `backbone.*` left out."""
    return [k for k in ref.state_dict() if not k.startswith("backbone.")]
