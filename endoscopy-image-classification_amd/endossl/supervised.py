"""Supervised trainer with the reference's API (`SupLearning`, code/supervised.py:23-360) over the
native models -- BASELINE configs[0] (ResNet-18, 23 classes, B=16, 224²) as a GPU step.

Same constructor and methods -- get_dataloader(train_dl, valid_dl, mixup_fn, test_dl), get_config,
train_one, evaluate_one, save_checkpoint, load_checkpoint, fit -- plus `step(batch)`.  One step
(:111-138, the plain path: MODEL.MARGIN 'None', no triplet, no mixup):

  fwd    logits = model(images)
  loss   F.cross_entropy(logits, y, weight=class_weights, reduction='mean')   (ce_loss type 'none',
         code/loss.py:118) -- value and d(loss)/d(logits) in one kernel (es_ce_weighted_fwd_bwd)
  bwd    autograd over the HIP ops
  opt    Adam + EMA of the parameters in one sweep, EMA of the BatchNorm buffers, LR update
         (trainer.Trainer._finish_step; set-up and checkpoints are the base's too)

The triplet mode (MODEL.IS_TRIPLET, :84-108) runs on the embedding-head ViT (comatch_model.NativeViTEmb) as
a direct launch sequence, no autograd:

  fwd    (logits, fts, z) = model([anchors; poss; negs])     one trunk pass over 3 bs images
  loss   ce = PolyCE(logits[:bs], y_a, w) (es_poly_ce_fwd_bwd); triplet = mean(max(d_p - d_n + 0.7, 0)) on z
         (es_triplet_fwd_bwd); losses = ce + LAMBDA_C * triplet
  bwd    heads backward -> dL/dfts -> trunk backward (model.backward_from)
  opt    as above

`test_one` (:198-236) and `inference` (:238-268, the pseudo-labelling pass; es_softmax_predict) take
tuple-returning and plain-logit models.

The margin mode (MODEL.MARGIN in cosface / arcface / sphereface / acloss, :117-119) runs on resnet.ModelMargin:

  fwd    fts = model.backbone(images)                         the pooled [n, 512] features
  loss   AngularPenaltySMLoss(fts, y, model.fc, class_weights) with d/dfts and d/dfc.weight in one call
         (es_margin_softmax_fwd_bwd; the weight gradient goes straight into the flat gradient)
  bwd    autograd from dfts through the trunk
  opt    as above

step() returns {"loss", "fts"} there.  With IS_TRIPLET also set the triplet step runs, as in the reference (:84).
The mixup path is dead code in the reference (dataset.py always returns mixup_fn = None) and raises
NotImplementedError.
"""
import os

import numpy as np
import torch

from . import _lib, dist
from ._lib import call, ptr
from .conformer import join_wgrad_stream
from .loss import AngularPenaltySMLoss, margin_softmax_fwd_bwd, weighted_ce_fwd_bwd
from .trainer import Trainer
from .utils import AverageMeter


class MarginModelError(ValueError, NotImplementedError):
    """MODEL.MARGIN with a model the margin step cannot run on (no `.backbone` / `.fc`): a wrong value for this
    model, and -- as callers of the earlier, margin-less trainer caught it -- not implemented for it."""


class SupLearning(Trainer):
    BEST_FIELDS = ("best_valid_loss", "best_valid_score")
    RESTORE_BEST = False  # load_checkpoint (code/supervised.py:295) reads neither back
    CKPT_PRINT = False

    def __init__(self, model, opt_func="Adam", lr=1e-3, device='cpu', wandb=None):
        super().__init__(model, opt_func=opt_func, lr=lr, device=device)
        self.wandb = wandb

    def get_dataloader(self, train_dl, valid_dl, mixup_fn=None, test_dl=None):
        self.train_dl = train_dl
        self.valid_dl = valid_dl
        self.test_dl = test_dl
        if mixup_fn is not None:
            raise NotImplementedError("mixup (code/supervised.py:112-113) is outside the native step's scope")
        self.mixup_fn = None

    def get_config(self, config):
        print('Training mode: Supervised Learning')
        margin = str(getattr(config.MODEL, "MARGIN", "None")) != "None"
        self.is_triplet = bool(getattr(config.MODEL, "IS_TRIPLET", False))
        emb = getattr(getattr(self.model, "cfg", None), "head", None) == "emb"
        # code/supervised.py:84: IS_TRIPLET is tested first, so a margin config with it runs the triplet step
        self.is_margin = margin and not self.is_triplet
        if margin and not (self.is_triplet and emb) and not (hasattr(self.model, "backbone")
                                                             and hasattr(self.model, "fc")):
            raise MarginModelError("MODEL.MARGIN needs a model with .backbone and .fc (code/supervised.py:118-119): "
                                   "build it with build_model(config) with MODEL.MARGIN set (resnet18)")
        self.loss_fc = AngularPenaltySMLoss(config, device=self.device) if margin else None
        if self.is_triplet and not emb:
            raise ValueError("MODEL.IS_TRIPLET needs the embedding-head model (logits, fts, z): build it with "
                             "build_model(config) with MODEL.IS_TRIPLET set and TRAIN.IS_SSL off")
        if self.is_triplet and dist.world_size() > 1 and getattr(self.model, "cnn_emb", False):
            raise NotImplementedError("the triplet step over NativeResNetEmb runs in one process: the SyncBatchNorm1d "
                                      "head over a SyncBatchNorm trunk is untested data-parallel")
        self.triplet_alpha = 0.7  # TripletLoss(alpha=0.7) (code/supervised.py:60)
        self.triplet_dist = {"d_ap": [], "d_an": []}
        self._tws = {}
        self._setup_model(config)
        self._setup_optim(config, len(self.train_dl) if self.train_dl is not None else 1, self.train_dl)

    # The forward / loss / backward of a step as one hipGraph (torch.cuda.CUDAGraph over the C-ABI launches,
    # the conv weight-gradient side stream forked and joined inside): ResNet-18 at B=16 is host-bound eager
    # (Python autograd walks ~250 launches a step).  Captured after GRAPH_WARM eager steps of a shape (the
    # first versions build the conv-weight pack table; the captured step packs in one launch), then
    # replayed; inputs are copied into the graph's own buffers.  The optimizer, EMA and LR schedule stay
    # outside (their scalars change per step).  One process only: at world > 1 the weighted loss
    # all-reduces inside the step.  ENDOSSL_SUP_GRAPH=0 keeps every step eager.
    use_graph = os.environ.get("ENDOSSL_SUP_GRAPH", "1") == "1"
    GRAPH_WARM = 2

    def _compute(self, images, targets):
        """Forward, weighted CE and its gradient, backward into model.flat_grad (no host sync)."""
        dev = self.model.flat.device
        logits = self.model(images)
        stats = torch.zeros(1, dtype=torch.float32, device=dev)
        dl = torch.empty_like(logits)
        weighted_ce_fwd_bwd(logits.detach(), targets, self.class_weights, dl, stats)
        self.optimizer.zero_grad()
        torch.autograd.backward([logits], [dl])
        join_wgrad_stream(dev)
        return stats, logits.detach()

    def _graph_key(self, images, targets):
        """Everything that changes the captured launch sequence: shapes, buffers, the model's precision / map /
        freezing state and which parameters take gradients."""
        m = self.model
        cw = self.class_weights
        return (tuple(images.shape), images.dtype, tuple(targets.shape), m.flat.data_ptr(), m.flat_grad.data_ptr(),
                cw.data_ptr() if cw is not None else 0, getattr(m, "conv_bf16", None), getattr(m, "map_bf16", None),
                bool(getattr(m, "frozen_trunk", False)), tuple(p.requires_grad for p in m.parameters()))

    def _run_graph(self, images, targets):
        """One step replayed from the graph captured for its key (one graph per key, so the smaller last batch
        of an epoch runs eagerly / gets its own graph without discarding the main one).  Returns fresh copies
        of the graph's static outputs: the next replay overwrites them."""
        key = self._graph_key(images, targets)
        graphs = self.__dict__.setdefault("_graphs", {})
        ent = graphs.get(key)
        if ent is None:
            ent = graphs[key] = {"warm": 0, "graph": None}
        if ent["graph"] is None:
            if ent["warm"] < self.GRAPH_WARM:
                ent["warm"] += 1
                return self._compute(images, targets)
            gin = (images.clone(), targets.clone())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                gout = self._compute(*gin)
            ent.update(graph=g, gin=gin, gout=gout)
        else:
            for dst, src in zip(ent["gin"], (images, targets)):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src, non_blocking=True)
        ent["graph"].replay()
        return tuple(t.clone() for t in ent["gout"])

    def _triplet_workspace(self, bs, C, L):
        """dl / dz of a batch shape.  dl's rows >= bs are zeroed here and never written: only the anchors'
        logits enter the loss."""
        key = (bs, C, L)
        if key not in self._tws:
            dev = self.model.flat.device
            self._tws[key] = {"dl": torch.zeros(3 * bs, C, device=dev), "dz": torch.empty(3 * bs, L, device=dev)}
        return self._tws[key]

    def _step_triplet(self, batch, drop_keep=None):
        """code/supervised.py:84-108 as a launch sequence (no autograd, no host sync)."""
        (anchors, poss, negs), targets = batch
        dev = self.model.flat.device
        self._inflight.wait()
        y = targets[0].to(dev, non_blocking=True).to(torch.int64).contiguous()  # the anchors' labels (:86)
        imgs = [t.to(dev, non_blocking=True) for t in (anchors, poss, negs)]
        bs = int(imgs[0].shape[0])
        if any(int(t.shape[0]) != bs for t in imgs) or int(y.shape[0]) != bs:
            raise ValueError("triplet batch: anchors, positives, negatives and the anchors' targets differ in length")
        m, cfg = self.model, self.config
        m.train()
        C, L = m.cfg.num_classes, m.cfg.low_dim
        s = _lib.stream()
        W = self._triplet_workspace(bs, C, L)
        dl, dz = W["dl"], W["dz"]
        keep = None if drop_keep is None else drop_keep.to(dev, torch.uint8).contiguous()
        logits, fts, z = m._run(imgs, train=True, keep=keep)
        lam_c = float(cfg.TRAIN.LAMBDA_C)
        stats = torch.empty(6, dtype=torch.float32, device=dev)  # ce, triplet, d_ap, d_an, active, total
        call("es_poly_ce_fwd_bwd", ptr(logits), C, ptr(y), ptr(self.class_weights), bs, C, 2.0, 1.0 / bs, ptr(dl), C,
             ptr(stats[0:1]), s)
        call("es_triplet_fwd_bwd", ptr(z), L, bs, L, self.triplet_alpha, lam_c / bs, ptr(dz), L, ptr(stats[1:5]), s)
        torch.add(stats[0], stats[1], alpha=lam_c, out=stats[5])
        m.backward_from(dl, dz)
        self._finish_step()
        return {"loss": stats[5], "ce": stats[0], "triplet": stats[1], "d_ap": stats[2], "d_an": stats[3],
                "active": stats[4], "logits": logits, "fts": fts, "z": z}

    def _step_margin(self, batch):
        """code/supervised.py:117-119 (MODEL.MARGIN set): fts = model.backbone(images); the margin loss on
        (fts, y, model.fc, class weights) -- value, d/dfts and d/dfc.weight in one es_margin_softmax_fwd_bwd
        call, the weight gradient written straight into the flat gradient; autograd from dfts through the
        trunk.  Eager (not part of the graph replay), no host sync.  Data-parallel: each rank's plain mean over
        its equal shard (grad_scale 1 / n_local), so the gradient average over ranks is the global mean's."""
        images, targets = batch
        m, lf = self.model, self.loss_fc
        dev = m.flat.device
        self._inflight.wait()
        targets = targets.to(dev, non_blocking=True).to(torch.int64).contiguous()
        images = images.to(dev, non_blocking=True)
        m.train()
        fts = m.backbone(images)
        n = int(fts.shape[0])
        x = fts.detach()
        stats = torch.empty(1, dtype=torch.float32, device=dev)
        dfts = torch.empty_like(x)
        self.optimizer.zero_grad()
        margin_softmax_fwd_bwd(x, m.pview("fc.weight").view(m.shapes["fc.weight"]), None, targets, self.class_weights,
                               None, lf.loss_type, lf.s, lf.m, lf.eps, 1.0 / n, dfts,
                               m.gview("fc.weight").view(m.shapes["fc.weight"]), None, stats)
        if fts.requires_grad:  # not under a frozen trunk (IS_FREEZE): fc.weight alone trains then
            torch.autograd.backward([fts], [dfts])
        join_wgrad_stream(dev)
        dist.allreduce_mean_(stats)  # every rank logs the global mean
        self._finish_step()
        return {"loss": stats[0], "fts": x}

    def step(self, batch, drop_keep=None):
        """batch = (images [n, 3, H, W], targets [n]) -> {"loss", "logits"} (device tensors); margin mode:
        {"loss", "fts"}.
        Triplet mode: batch = ((anchors, poss, negs), (y_a, y_p, y_n)), each image tensor [bs, 3, H, W] ->
        {"loss", "ce", "triplet", "d_ap", "d_an", "active", "logits", "fts", "z"}; drop_keep: optional uint8
        [3 bs, D/4] Dropout keep-mask to replay (parity tests)."""
        if getattr(self, "is_triplet", False):
            return self._step_triplet(batch, drop_keep)
        if getattr(self, "is_margin", False):
            return self._step_margin(batch)
        images, targets = batch
        dev = self.model.flat.device
        self._inflight.wait()
        targets = targets.to(dev, non_blocking=True).to(torch.int64).contiguous()
        images = images.to(dev, non_blocking=True)
        self.model.train()
        # graph replay for the ResNet models (the host-bound P0 step); the ViT models step eagerly here
        if self.use_graph and dist.world_size() == 1 and images.is_cuda and type(self.model).__name__ == "NativeResNet":
            stats, logits = self._run_graph(images, targets)
        else:
            stats, logits = self._compute(images, targets)
        self._finish_step()
        return {"loss": stats[0], "logits": logits.detach()}

    def train_one(self, epoch):
        dists = []

        def step(batch):
            out = self.step(batch)
            if "d_ap" in out:  # triplet mode: the step's mean distances (code/supervised.py:99-100)
                dists.append(torch.stack((out["d_ap"], out["d_an"])))
            return out
        summary_loss = self._train_steps(step, self.train_dl, epoch * len(self.train_dl))
        if getattr(self, "is_triplet", False):
            d = torch.stack(dists).cpu().tolist() if dists else []
            self.triplet_dist = {"d_ap": [r[0] for r in d], "d_an": [r[1] for r in d]}
        return summary_loss

    def evaluate_one(self, epoch=None, show_metric=False, show_report=False, show_cf_matrix=False):
        """code/supervised.py:148-196: unweighted CE mean, prediction = argmax softmax(logits)."""
        eval_model = self._eval_model()
        summary_loss = AverageMeter()
        outs, tgts = [], []
        dev = self.model.flat.device
        with torch.no_grad():
            for images, targets in self.valid_dl:
                logits = self._first(eval_model(images.to(dev)))
                targets = targets.to(dev).to(torch.int64).contiguous()
                st = torch.zeros(1, device=dev)
                scratch = torch.empty_like(logits)
                call("es_ce_weighted_fwd_bwd", ptr(logits), logits.shape[1], ptr(targets), None, logits.shape[0],
                     logits.shape[1], 1.0, ptr(scratch), logits.shape[1], ptr(st), _lib.stream())
                summary_loss.update(st.item(), self.config.DATA.BATCH_SIZE)
                outs.append(logits.argmax(1).cpu().numpy())
                tgts.append(targets.cpu().numpy())
        return summary_loss, self._metrics(outs, tgts, show_metric, show_report)

    def _predict(self, logits, thres, want_label):
        """es_softmax_predict on a batch of logits -> int32 device tensor (argmax, or the thresholded label)."""
        logits = logits.float().contiguous()
        n, C = logits.shape
        res = torch.empty(n, dtype=torch.int32, device=logits.device)
        call("es_softmax_predict", ptr(logits), C, n, C, float(thres), None if want_label else ptr(res), None,
             ptr(res) if want_label else None, _lib.stream())
        return res

    def test_one(self, show_metric=False, show_report=False, show_cf_matrix=False):
        """code/supervised.py:198-236: CPU bool tensor over valid_dl in loader order, True where the argmax
        prediction differs from the target.  Predictions stay on the device until the one copy at the end."""
        eval_model = self._eval_model()
        dev = self.model.flat.device
        wrong = []
        with torch.no_grad():
            for images, targets in self.valid_dl:
                logits = self._first(eval_model(images.to(dev, non_blocking=True)))
                pred = self._predict(logits, 0.0, want_label=False)
                wrong.append(pred != targets.to(dev, non_blocking=True).view(-1).to(torch.int32))
        if not wrong:
            return torch.zeros(0, dtype=torch.bool)
        return torch.cat(wrong).cpu()

    def inference(self, dl_test):
        """code/supervised.py:238-268: {index: label} over dl_test's (images, index) batches, label =
        argmax(p) where max(p) > TRAIN.THRES (strict) and 0 below it -- class 0, the reference's
        `argmax * cond`.  One device-to-host copy at the end."""
        eval_model = self._eval_model()
        dev = self.model.flat.device
        thres = float(self.config.TRAIN.THRES)
        labels, index = [], []
        with torch.no_grad():
            for images, idx in dl_test:
                logits = self._first(eval_model(images.to(dev, non_blocking=True)))
                labels.append(self._predict(logits, thres, want_label=True))
                index += idx.tolist() if torch.is_tensor(idx) else np.array(idx).tolist()
        if not labels:
            return {}
        return dict(zip(index, torch.cat(labels).cpu().tolist()))

    def _track_best(self, valid_loss, f1, save):
        """The reference's rule (code/supervised.py:344-358, code/ezbm.py:369-382,413-426): better in loss AND score
        -> new best (saved when `save`); worse in either -> 1 towards the early stop (never reset); returns that
        increment."""
        if self.best_valid_loss and self.best_valid_score:
            if self.best_valid_loss > valid_loss and self.best_valid_score < f1:
                self.best_valid_loss, self.best_valid_score = valid_loss, f1
                if save and dist.rank() == 0:
                    self.save_checkpoint(self.config.TRAIN.SAVE_CP)
            elif self.best_valid_loss < valid_loss or self.best_valid_score > f1:
                return 1
            return 0
        self.best_valid_loss, self.best_valid_score = valid_loss, f1
        if save and dist.rank() == 0:
            self.save_checkpoint(self.config.TRAIN.SAVE_CP)
        return 0

    def fit(self):
        count_early_stop = 0
        for epoch in range(self.epoch_start, self.config.TRAIN.EPOCHS):
            if count_early_stop > 5:
                print('Early stopping')
                break
            self.epoch = epoch
            train_loss = self.train_one(self.epoch)
            print(f'\tTrain Loss: {train_loss.avg:.3f}')
            if epoch % self.config.TRAIN.FREQ_EVAL == 0 and self.valid_dl is not None:
                valid_loss, valid_metric = self.evaluate_one(self.epoch)
                count_early_stop += self._track_best(valid_loss.avg, float(valid_metric['macro/f1']), save=True)
                print(f'\tValid Loss: {valid_loss.avg:.3f}')
                print(f'\tMetric: {valid_metric}')
