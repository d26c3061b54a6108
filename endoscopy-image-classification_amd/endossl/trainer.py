"""The host-side scaffolding every trainer shares (FixMatch, SupLearning and SemiFormer derive from `Trainer`;
CoMatch from FixMatch, EZBM from SupLearning): set-up, the update tail of a step, the evaluation tail, checkpoints,
and the helpers `train_one` / `fit` are written with.

A trainer writes what is its own: `get_config` (its checks and freezing, around the two set-up calls), `step`, the
batch body of `evaluate_one`, and `train_one` / `fit` as a few lines over the helpers.  The class attributes below
say where the reference's trainers differ in the rest.
"""
import os
from datetime import date, datetime

import numpy as np
import torch

from . import dist
from .ema import ModelEMA
from .lr_scheduler import build_scheduler
from .optimizer import build_optimizer
from .throttle import StepThrottle
from .utils import AverageMeter, balanced_class_weights, calculate_metrics


def _next(it):
    return it.next() if hasattr(it, "next") else next(it)


def _restarting(dl, what):
    """next-batch function over loader `dl`, started anew when exhausted.  An empty loader raises (a RuntimeError,
    not the StopIteration that would end a caller's generator quietly)."""
    it = [iter(dl)]

    def take():
        try:
            return _next(it[0])
        except StopIteration:
            it[0] = iter(dl)
        try:
            return _next(it[0])
        except StopIteration:
            raise RuntimeError(f"the {what} loader is empty") from None
    return take


class Trainer:
    INFLIGHT_DEPTH = 1                  # queued steps (throttle.py); 2 for the ViT trainers
    EMA_BUFFERS = True                  # _finish_step blends the BatchNorm buffers into the EMA model
    BEST_FIELDS = ("best_valid_perf",)  # saved with a checkpoint ...
    RESTORE_BEST = True                 # ... and read back by load_checkpoint
    CKPT_SIZE_SUFFIX = False            # file name ends in _size_<IMG_SIZE>
    CKPT_PRINT = True                   # save_checkpoint prints 'Saved checkpoint'

    def __init__(self, model, opt_func="Adam", lr=1e-3, device='cpu'):
        self.model = model
        self.opt_func = opt_func
        self.device = device
        self.model.to(self.device)
        self.epoch_start = 0
        for name in self.BEST_FIELDS:
            setattr(self, name, None)
        self._inflight = StepThrottle(self.INFLIGHT_DEPTH)

    def get_dataloader(self, train_dl, valid_dl, test_dl=None):
        self.train_labeled_dl, self.train_unlabeled_dl = train_dl
        self.valid_dl = valid_dl
        self.test_dl = test_dl

    # ------------------------------------------------------------------ set-up (get_config)
    def _setup_model(self, config):
        """Identical replicas on every rank before the first step, then the EMA copy of the model as it is now
        (a trainer that freezes does so before or after this call, as its reference does)."""
        self.config = config
        dist.broadcast_(self.model.flat)
        self.model.mark_updated()
        self.ema_model = ModelEMA(model=self.model, decay=config.TRAIN.EMA_DECAY, device=self.device) \
            if config.TRAIN.USE_EMA else None

    def _setup_optim(self, config, n_iter_per_epoch, labeled_dl):
        """Optimizer over the parameters that train now, scheduler (None for SCH_NAME 'const'), class weights."""
        self.optimizer = build_optimizer(self.model, opt_func=self.opt_func, lr=config.TRAIN.BASE_LR)
        self.lr_scheduler = build_scheduler(config=config, optimizer=self.optimizer,
                                            n_iter_per_epoch=n_iter_per_epoch)
        if config.TRAIN.CLS_WEIGHT:
            w = balanced_class_weights(labeled_dl.dataset.df[config.DATA.TARGET_NAME])
            self.class_weights = torch.tensor(w, dtype=torch.float).to(self.device)
        else:
            self.class_weights = None

    # ------------------------------------------------------------------ the update tail of a step
    def _finish_step(self, grad_scale=None):
        """Gradient all-reduce (unless its scale is handed in: dist.GradBuckets.finish()), optimizer + parameter
        EMA in one sweep, EMA of the BatchNorm buffers."""
        if grad_scale is None:
            grad_scale = dist.allreduce_sum_(self.model.flat_grad)
        ema = self.ema_model
        self.optimizer.step(ema_flat=ema.ema.flat if ema is not None else None,
                            ema_decay=float(ema.decay) if ema is not None else 0.0, grad_scale=grad_scale)
        if ema is not None:
            if self.EMA_BUFFERS:
                ema.update_buffers(self.model)
            ema.ema.mark_updated()
        self._inflight.record()

    # ------------------------------------------------------------------ train_one
    def _paired_batches(self, steps):
        """`steps` (labeled, unlabeled) batch pairs; each loader restarts on its own when exhausted."""
        lab = _restarting(self.train_labeled_dl, "labeled")
        unl = _restarting(self.train_unlabeled_dl, "unlabeled")
        for _ in range(steps):
            yield lab(), unl()

    def _train_steps(self, step, batches, first_update, weight=None):
        """step(batch) over `batches`, lr_scheduler.step_update(first_update + i) after the i-th; the losses stay
        on the device until the loop is done (one host sync per epoch) -> AverageMeter, each loss weighted with
        `weight` (DATA.BATCH_SIZE)."""
        self.model.train()
        pending = []
        for i, batch in enumerate(batches):
            out = step(batch)
            if self.lr_scheduler is not None:
                self.lr_scheduler.step_update(first_update + i)
            pending.append(out["loss"].detach().clone())
        meter = AverageMeter()
        for v in pending:
            meter.update(v.item(), self.config.DATA.BATCH_SIZE if weight is None else weight)
        return meter

    # ------------------------------------------------------------------ evaluate_one
    def _eval_model(self):
        eval_model = self.ema_model.ema if self.config.TRAIN.USE_EMA else self.model
        eval_model.eval()
        return eval_model

    @staticmethod
    def _first(out):
        """The logits of a model output: the first entry of ModelwEmb's (logits, fts, z)."""
        return out[0] if isinstance(out, (tuple, list)) else out

    def _metrics(self, outs, tgts, show_metric, show_report):
        """The per-batch predictions and targets (numpy) -> calculate_metrics' dict."""
        pred, tgt = np.concatenate(outs), np.concatenate(tgts)
        metric = calculate_metrics(pred, tgt, self.config)
        if show_metric:
            print('Metric:')
            print(metric)
        if show_report:
            from sklearn import metrics
            print(metrics.classification_report(tgt, pred))
        return metric

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, foldname):
        """The reference's dict keys and file name (MM_DD_YYYY_HH_MM_SS_epoch_<e>[_size_<s>].pth, HH its
        `int(hour) + 2`)."""
        checkpoint = {}
        if self.config.TRAIN.USE_EMA:
            checkpoint['ema_state_dict'] = self.ema_model.ema.state_dict()
        d = date.today().strftime("%m_%d_%Y")
        h = datetime.now().strftime("%H_%M_%S").split('_')
        h[0] = str(int(h[0]) + 2)
        filename = d + '_' + '_'.join(h) + '_epoch_' + str(self.epoch)
        if self.CKPT_SIZE_SUFFIX:
            filename += '_size_' + str(self.config.DATA.IMG_SIZE)
        checkpoint['epoch'] = self.epoch
        for name in self.BEST_FIELDS:
            checkpoint[name] = getattr(self, name)
        checkpoint['model_state_dict'] = self.model.state_dict()
        checkpoint['optimizer'] = self.optimizer.state_dict()
        checkpoint['scheduler'] = self.lr_scheduler.state_dict() if self.lr_scheduler is not None else {}
        f = os.path.join(foldname, filename + '.pth')
        torch.save(checkpoint, f)
        if self.CKPT_PRINT:
            print('Saved checkpoint')
        return f

    def _set_trainable(self, is_train):
        """requires_grad after load_checkpoint(is_train)."""
        for p in self.model.parameters():
            p.requires_grad = bool(is_train)

    def load_checkpoint(self, checkpoint_dir, is_train=False):
        checkpoint = torch.load(checkpoint_dir, map_location='cpu', weights_only=True)
        self.model.load_state_dict(checkpoint['model_state_dict'])
        self._set_trainable(is_train)
        if self.config.TRAIN.USE_EMA:
            self.ema_model.ema.load_state_dict(checkpoint['ema_state_dict'])
        self.epoch_start = checkpoint['epoch']
        if self.RESTORE_BEST:
            for name in self.BEST_FIELDS:
                setattr(self, name, checkpoint[name])
        self.optimizer.load_state_dict(checkpoint['optimizer'])
        if self.lr_scheduler is not None:
            self.lr_scheduler.load_state_dict(checkpoint['scheduler'])

    # ------------------------------------------------------------------ fit
    def _fit_epoch(self, epoch):
        """One epoch of the `best_valid_perf` trainers: train, evaluate every FREQ_EVAL epochs, keep the lowest
        validation loss, save every evaluated epoch on rank 0."""
        self.epoch = epoch
        lr = self.optimizer.param_groups[0]["lr"]
        best = f"{float(self.best_valid_perf):.3f}" if self.best_valid_perf else "inf"
        print(f'Training epoch: {self.epoch} | Current LR: {lr:.6f} | The best loss: {best}')
        train_loss = self.train_one(self.epoch)
        print(f'\tTrain Loss: {train_loss.avg:.3f}')
        if epoch % self.config.TRAIN.FREQ_EVAL == 0 and self.valid_dl is not None:
            valid_loss, valid_metric = self.evaluate_one()
            if self.best_valid_perf is None or self.best_valid_perf > valid_loss.avg:
                self.best_valid_perf = valid_loss.avg
            if dist.rank() == 0:
                self.save_checkpoint(self.config.TRAIN.SAVE_CP)
            print(f'\tValid Loss: {valid_loss.avg:.3f}')
            print(f'\tMetric: {valid_metric}')
