"""SemiFormer trainer with the reference's API (code/semiformer.py:18-262) over the native Conformer.

Same constructor and methods -- get_dataloader, get_config, train_one, evaluate_one,
save_checkpoint, load_checkpoint, fit -- plus `step(batch)` (one SSL step) and `step_sup(batch)`
(the supervised warm-up step of epochs < TRAIN.EVAL_STEP_SUP).  One SSL step (:103-146):

  fwd    (out_conv, out_trans) = model([x; u_w; u_s])   one pass over B + 2muB images: BatchNorm
                                                         couples the rows, so every row is kept
  loss   lx = CE_w(out_conv[:B], y) + CE_w(out_trans[:B], y)          fused value+grad kernels
         lu = consistency(conv weak, conv strong) + consistency(conv weak, trans strong)
              -- the CONV head's weak logits supervise both heads
         losses = lx + LAMBDA_U * lu
  bwd    autograd over the HIP ops from d(losses)/d(logits) (weak rows: zero, detached)
  opt    Adam + EMA of the parameters in one sweep, EMA of the BatchNorm buffers, LR update
         (trainer.Trainer._finish_step, as are set-up, checkpoints and the epoch body of `fit`)
"""
import torch

from . import _lib
from .conformer import join_wgrad_stream
from ._lib import call, ptr
from .loss import weighted_ce_fwd_bwd
from .trainer import Trainer
from .utils import AverageMeter


class SemiFormer(Trainer):
    def get_config(self, config):
        print('Training mode: SemiFormer')
        self._setup_model(config)
        # code/semiformer.py:50-56: IS_FREEZE trains conv_cls_head and trans_cls_head only; the native
        # forward then keeps the trunk off the autograd tape (NativeConformer.frozen_trunk) so only the
        # heads' backward runs, and the trunk's gradient stays exactly zero
        self.frozen = bool(config.TRAIN.IS_FREEZE)
        self.model.frozen_trunk = self.frozen
        if self.frozen:
            for p in self.model.parameters():
                p.requires_grad = False
            self.model.conv_cls_head.requires_grad_(True)
            self.model.trans_cls_head.requires_grad_(True)
        self._setup_optim(config, config.TRAIN.EVAL_STEP, self.train_labeled_dl)

    # ------------------------------------------------------------------ steps
    def _ce(self, logits, y, dl, out):
        weighted_ce_fwd_bwd(logits, y, self.class_weights, dl, out)

    def _finish(self, out_conv, out_trans, dconv, dtrans):
        self.optimizer.zero_grad()
        torch.autograd.backward([out_conv, out_trans], [dconv, dtrans])
        join_wgrad_stream(self.model.flat.device)  # (the backward's final callback already did)
        self._finish_step()

    def step(self, batch):
        """batch = ((x, y), ((u_w, u_s), idx)) -> dict of device scalars / tensors."""
        (inputs_x, targets_x), ((inputs_u_w, inputs_u_s), _) = batch
        dev = self.model.flat.device
        self._inflight.wait()
        bs, nu = int(inputs_x.shape[0]), int(inputs_u_w.shape[0])
        targets_x = targets_x.to(dev, non_blocking=True).to(torch.int64).contiguous()
        inputs = torch.cat((inputs_x.to(dev), inputs_u_w.to(dev), inputs_u_s.to(dev)))
        self.model.train()
        out_conv, out_trans = self.model(inputs)
        C = out_conv.shape[1]
        lam = float(self.config.TRAIN.LAMBDA_U)
        s = _lib.stream()
        stats = torch.zeros(7, dtype=torch.float32, device=dev)  # lx_c, lx_t, lu_c, mask, lu_t, mask, total
        pl = torch.empty(nu, dtype=torch.int32, device=dev)
        mask = torch.empty(nu, dtype=torch.uint8, device=dev)
        dconv = torch.zeros_like(out_conv)
        dtrans = torch.zeros_like(out_trans)
        oc, ot = out_conv.detach(), out_trans.detach()
        self._ce(oc[:bs], targets_x, dconv[:bs], stats[0:1])
        self._ce(ot[:bs], targets_x, dtrans[:bs], stats[1:2])
        weak = oc[bs:bs + nu]
        call("es_fm_consistency_fwd_bwd", ptr(weak), C, ptr(oc[bs + nu:]), C, nu, C, float(self.config.TRAIN.THRES),
             lam / nu, ptr(pl), ptr(mask), None, ptr(dconv[bs + nu:]), C, ptr(stats[2:4]), s)
        call("es_fm_consistency_fwd_bwd", ptr(weak), C, ptr(ot[bs + nu:]), C, nu, C, float(self.config.TRAIN.THRES),
             lam / nu, None, None, None, ptr(dtrans[bs + nu:]), C, ptr(stats[4:6]), s)
        lx = stats[0] + stats[1]
        lu = stats[2] + stats[4]
        loss = lx + lam * lu
        self._finish(out_conv, out_trans, dconv, dtrans)
        return {"loss": loss, "lx": lx, "lu": lu, "mask_mean": stats[5], "pseudo_label": pl, "mask": mask,
                "out_conv": oc, "out_trans": ot}

    def step_sup(self, batch):
        """Supervised warm-up step (code/semiformer.py:75-101): CE on both heads."""
        images, targets = batch
        dev = self.model.flat.device
        self._inflight.wait()
        targets = targets.to(dev).to(torch.int64).contiguous()
        self.model.train()
        out_conv, out_trans = self.model(images.to(dev))
        stats = torch.zeros(2, dtype=torch.float32, device=dev)
        dconv, dtrans = torch.zeros_like(out_conv), torch.zeros_like(out_trans)
        self._ce(out_conv.detach(), targets, dconv, stats[0:1])
        self._ce(out_trans.detach(), targets, dtrans, stats[1:2])
        self._finish(out_conv, out_trans, dconv, dtrans)
        return {"loss": stats.sum()}

    def train_one(self, epoch):
        if epoch < self.config.TRAIN.EVAL_STEP_SUP:
            dl = self.train_labeled_dl
            return self._train_steps(self.step_sup, dl, epoch * len(dl))
        n = self.config.TRAIN.EVAL_STEP
        return self._train_steps(self.step, self._paired_batches(n), epoch * n)

    def evaluate_one(self, show_metric=False, show_report=False, show_cf_matrix=False):
        """code/semiformer.py:150-198: CE of both heads, prediction = argmax softmax(conv + trans)."""
        eval_model = self._eval_model()
        summary_loss = AverageMeter()
        outs, tgts = [], []
        dev = self.model.flat.device
        with torch.no_grad():
            for images, targets in self.valid_dl:
                out_conv, out_trans = eval_model(images.to(dev))
                targets = targets.to(dev).to(torch.int64).contiguous()
                st = torch.zeros(2, device=dev)
                scratch = torch.empty_like(out_conv)
                call("es_ce_weighted_fwd_bwd", ptr(out_conv), out_conv.shape[1], ptr(targets), None,
                     out_conv.shape[0], out_conv.shape[1], 1.0, ptr(scratch), out_conv.shape[1], ptr(st[0:1]),
                     _lib.stream())
                call("es_ce_weighted_fwd_bwd", ptr(out_trans), out_trans.shape[1], ptr(targets), None,
                     out_trans.shape[0], out_trans.shape[1], 1.0, ptr(scratch), out_trans.shape[1], ptr(st[1:2]),
                     _lib.stream())
                summary_loss.update(st.sum().item(), self.config.DATA.BATCH_SIZE)
                # argmax of softmax(conv + trans) == argmax of (conv + trans)
                outs.append((out_conv + out_trans).argmax(1).cpu().numpy())
                tgts.append(targets.cpu().numpy())
        return summary_loss, self._metrics(outs, tgts, show_metric, show_report)

    def fit(self):
        for epoch in range(self.epoch_start, self.config.TRAIN.EPOCHS):
            self._fit_epoch(epoch)
