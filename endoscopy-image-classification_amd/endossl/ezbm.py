"""EZBM trainer with the reference's API (`EZBM`, code/ezbm.py:23-426; config code/configs/
kaggle_supervised_ezbm.yaml) over the embedding-head ViT (comatch_model.NativeViTEmb): the reference's
imbalance-handling recipe in two stages.

Stage 1 (:78-132) is SupLearning's triplet step, unchanged (same launches, same bits), plus a device-resident
feature bank: after each step the anchors' trunk features `fts[:bs]` and targets are copied into it with a
device copy (no host sync, no numpy list).  The bank is reset at the start of every stage-1 epoch, so it holds
the last epoch run.

Stage 2 (:133-182, set up at :386-397) freezes every parameter but `model.fc` and trains that head on
class-balanced mixes of the stored features.  One step on n rows, a launch sequence with no host sync and no
autograd:

  sample   es_ezbm_sample_mix: X [2n, D] = [mem[idx]; lam mem[idx] + (1 - lam) mem[dual]], t, td, lam
           (EmbFeatEZBM.__getitem__ for the whole batch: a uniform class then a uniform member for the row; the
           dual's class from the 'balance' / 'reverse' CDF; a counter hash, not Python's `random`)
  fwd      es_dropout_keep [2n, F]; EmbHeads.fc_forward with 2 BatchNorm groups: fc.0 + ReLU + Dropout over the 2n
           rows; es_bn1d_groups_fwd with G = 2 (the `o` rows, then the `s` rows, each with its own batch statistics
           -- fc(inputs), then fc(mix)); fc.4
  loss     es_ezbm_ce_fwd_bwd: l_o + LAMBDA_C * l_s and d/dlogits
  bwd      EmbHeads.fc_backward, 2 groups, no dX: es_dense_bwd fc.4 (dW over the 2n rows = the sum of both passes),
           es_bn1d_groups_bwd, es_dense_bwd fc.0 with dX = NULL
  opt      Trainer._finish_step (trainer.py): optimizer + EMA sweep, EMA of the BatchNorm buffers

The flat gradient outside `fc` is ZERO in stage 2: it is zeroed when stage 2 is set up and at the start of every
stage-2 epoch, and a step overwrites `fc`'s six slices only.  The optimizer is rebuilt for stage 2 (zero
moments), so the sweep leaves every frozen parameter bit for bit unchanged.

One process only: every rank would hold a different bank, so a world size above 1 raises NotImplementedError.
"""
import numpy as np
import torch

from . import _lib, dist
from ._lib import call, ptr
from .lr_scheduler import build_scheduler
from .optimizer import build_optimizer
from .supervised import SupLearning
from .utils import AttrDict, count_parameters

EXPANSIONS = ("balance", "reverse")


def _check_expansion(expansion):
    if expansion not in EXPANSIONS:
        raise ValueError(f"TRAIN.EXPANSION {expansion!r}: 'balance' or 'reverse' (code/dataset.py:157-165)")


def class_csr(targets, num_classes):
    """The bank rows by class: (cls_off int32 [C+1], cls_idx int32 [N]), rows ascending within a class --
    EmbFeatEZBM.class_dict (code/dataset.py:143-145).  A class with no stored row raises (the reference's
    random.choice fails on it)."""
    t = np.asarray(targets).astype(np.int64).reshape(-1)
    if t.size and (t.min() < 0 or t.max() >= num_classes):
        raise ValueError(f"feature-bank target outside [0, {num_classes}): {int(t.min())} .. {int(t.max())}")
    counts = np.bincount(t, minlength=num_classes)
    empty = np.nonzero(counts == 0)[0]
    if empty.size:
        raise ValueError(f"EZBM stage 2: class {int(empty[0])} has no stored feature row (classes without rows: "
                         f"{empty.tolist()}); every class must occur in the last stage-1 epoch")
    off = np.zeros(num_classes + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    idx = np.argsort(t, kind="stable").astype(np.int32)
    return off, idx


def class_cdf(cls_num_list, expansion):
    """fp32 CDF [C] of the dual item's class (code/dataset.py:147-165): 'balance' uniform; 'reverse' class c with
    probability cls_num[C-1-c] / sum (the reversed class frequencies)."""
    _check_expansion(expansion)
    cnt = np.array(cls_num_list)
    C = len(cnt)
    if expansion == "balance":
        return (np.arange(1, C + 1, dtype=np.float64) / C).astype(np.float32)
    prob = list(cnt / np.sum(cnt))
    prob.reverse()
    return np.cumsum(np.array(prob)).astype(np.float32)


def lam_table(cls_num_list, expansion):
    """fp32 [C*C], entry t * C + td (code/ezbm.py:156-161): the float64 quotient cnt[t] / (cnt[t] + cnt[td])
    rounded to fp32; 'balance' 0.5 everywhere; 'reverse' the fp32 1 - lam."""
    _check_expansion(expansion)
    cnt = np.array(cls_num_list)
    lam = (cnt[:, None] / (cnt[:, None] + cnt[None, :])).astype(np.float32)
    if expansion == "balance":
        lam = np.full_like(lam, 0.5)
    else:
        lam = np.float32(1.0) - lam
    return np.ascontiguousarray(lam.reshape(-1))


class EZBM(SupLearning):
    STAGE1_EPOCHS = 100  # code/ezbm.py:352,388: both stages hard-code 100 epochs
    STAGE2_EPOCHS = 100

    def get_config(self, config):
        if getattr(getattr(self.model, "cfg", None), "head", None) != "emb":
            raise ValueError("EZBM needs the embedding-head model (logits, fts, z) with the complex `fc` head: build "
                             "it with build_model(config) with MODEL.IS_TRIPLET set and TRAIN.IS_SSL off")
        self.expansion = getattr(config.TRAIN, "EXPANSION", None)
        _check_expansion(self.expansion)
        if dist.world_size() > 1:
            raise NotImplementedError("EZBM runs in one process: each rank would store a different feature bank")
        # the triplet step whatever MODEL.IS_TRIPLET / MODEL.MARGIN say (code/ezbm.py:78-132 reads neither)
        sup = AttrDict(config)
        sup["MODEL"] = AttrDict(config.MODEL)
        sup["MODEL"]["IS_TRIPLET"] = True
        sup["MODEL"]["MARGIN"] = "None"
        super().get_config(sup)
        self.config = config
        print('Training mode: EZBM Learning')
        self.cls_num_list = list(self.train_dl.dataset.get_cls_num_list())
        if len(self.cls_num_list) != self.model.cfg.num_classes:
            raise ValueError(f"get_cls_num_list() has {len(self.cls_num_list)} classes, the model "
                             f"{self.model.cfg.num_classes}")
        self.stage = 1
        self.sample_seed = int(getattr(self.model, "drop_seed", 0))
        self._sample_counter = 0
        self._bank_x = self._bank_y = None
        self._bank_n = 0
        self._tables = None
        self._s2ws = {}

    # ------------------------------------------------------------------------------------ stage 1
    def _bank_reserve(self, rows):
        """Room for `rows` bank rows: len(train_dl.dataset) rows up front where the dataset has a length, doubling
        after that (device copies only)."""
        dev, D = self.model.flat.device, self.model.cfg.dim
        cap = 0 if self._bank_x is None else int(self._bank_x.shape[0])
        if rows <= cap and self._bank_x.device == dev:
            return
        try:
            want = len(self.train_dl.dataset)
        except TypeError:
            want = 0
        new_cap = max(rows, want if cap == 0 else 2 * cap)
        x = torch.empty(new_cap, D, dtype=torch.float32, device=dev)
        y = torch.empty(new_cap, dtype=torch.int64, device=dev)
        if self._bank_n:
            x[:self._bank_n].copy_(self._bank_x[:self._bank_n])
            y[:self._bank_n].copy_(self._bank_y[:self._bank_n])
        self._bank_x, self._bank_y = x, y

    def bank(self):
        """(features [N, D], targets [N]) stored so far: views of the device bank."""
        if self._bank_x is None:
            dev = self.model.flat.device
            return (torch.empty(0, self.model.cfg.dim, device=dev), torch.empty(0, dtype=torch.int64, device=dev))
        return self._bank_x[:self._bank_n], self._bank_y[:self._bank_n]

    def set_bank(self, features, targets):
        """Replace the bank's content with features [N, D] and targets [N] (e.g. features stored by another run)."""
        n = int(features.shape[0])
        if features.dim() != 2 or int(features.shape[1]) != self.model.cfg.dim or int(targets.shape[0]) != n:
            raise ValueError(f"set_bank: features [N, {self.model.cfg.dim}] and targets [N] expected")
        self._bank_n = 0
        self._bank_reserve(n)
        self._bank_x[:n].copy_(features)
        self._bank_y[:n].copy_(targets)
        self._bank_n = n
        self._tables = None

    def step_stage_1(self, batch, drop_keep=None):
        """SupLearning's triplet step on batch = ((anchors, poss, negs), (y_a, y_p, y_n)) -- same outputs, same
        bits -- then the anchors' fts and targets appended to the feature bank (code/ezbm.py:114-115)."""
        out = self._step_triplet(batch, drop_keep)
        bs = int(batch[0][0].shape[0])
        dev = self.model.flat.device
        self._bank_reserve(self._bank_n + bs)
        self._bank_x[self._bank_n:self._bank_n + bs].copy_(out["fts"][:bs])
        self._bank_y[self._bank_n:self._bank_n + bs].copy_(batch[1][0].to(dev, non_blocking=True).view(-1))
        self._bank_n += bs
        self._tables = None
        return out

    def train_one_stage_1(self, epoch):
        self._bank_n = 0  # the bank holds the last epoch run (code/ezbm.py:86)
        self._tables = None
        return self._train_steps(self.step_stage_1, self.train_dl, epoch * len(self.train_dl))

    # ------------------------------------------------------------------------------------ stage 2
    def _fc_param_count(self):
        return sum(1 for _ in self.model.fc.parameters())

    def setup_stage_2(self):
        """code/ezbm.py:386-397: freeze everything but `fc` (head_emb stays frozen), rebuild the optimizer and the
        scheduler (n_iter_per_epoch = len(train_dl) // MU, the reference's value)."""
        for p in self.model.parameters():
            p.requires_grad = False
        self.model.fc.requires_grad_(True)
        self.optimizer = build_optimizer(self.model, opt_func=self.opt_func, lr=self.config.TRAIN.BASE_LR)
        n_iter = len(self.train_dl) // int(self.config.DATA.MU) if self.train_dl is not None else 1
        self.lr_scheduler = build_scheduler(config=self.config, optimizer=self.optimizer, n_iter_per_epoch=n_iter)
        self.model.flat_grad.zero_()
        self.stage = 2

    def _stage2_tables(self):
        """Class table, CDF and lam table of the current bank, on the device (one host copy of the bank's targets
        per epoch; rebuilt when the bank changes)."""
        if self._tables is None:
            if self._bank_n < 1:
                raise ValueError("EZBM stage 2: the feature bank is empty (run a stage-1 epoch first)")
            dev = self.model.flat.device
            C, exp = self.model.cfg.num_classes, self.expansion
            off, idx = class_csr(self._bank_y[:self._bank_n].cpu().numpy(), C)
            d = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
            self._tables = {"off": d(off), "idx": d(idx), "cdf": d(class_cdf(self.cls_num_list, exp)),
                            "lam": d(lam_table(self.cls_num_list, exp))}
        return self._tables

    def _stage2_workspace(self, n):
        if n not in self._s2ws:
            dev, cfg = self.model.flat.device, self.model.cfg
            D, C = cfg.dim, cfg.num_classes
            e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
            self._s2ws[n] = {"X": e(2 * n, D), "t": e(n, dt=torch.int64), "td": e(n, dt=torch.int64), "lam": e(n),
                             "idx": e(n, dt=torch.int32), "dual": e(n, dt=torch.int32), "dl": e(2 * n, C)}
        return self._s2ws[n]

    def step_stage_2(self, n=None, idx=None, dual=None, drop_keep=None):
        """One stage-2 step on n rows (default BATCH_SIZE * MU) -> {"loss", "l_o", "l_s", "logits", "t", "td",
        "lam", "idx", "dual"} (device tensors).  idx / dual: int [n] bank rows to replay instead of a draw;
        drop_keep: uint8 [2n, D/4] Dropout keep-mask to replay (parity tests)."""
        if getattr(self, "stage", 1) != 2:
            self.setup_stage_2()
        m, cfg = self.model, self.config
        dev = m.flat.device
        if idx is not None:
            n = int(idx.shape[0])
        elif n is None:
            n = int(cfg.DATA.BATCH_SIZE) * int(cfg.DATA.MU)
        if n < 2:
            raise ValueError(f"EZBM stage 2: a batch of {n} row(s): BatchNorm1d in training needs more than 1 value "
                             "per channel")
        T = self._stage2_tables()
        self._inflight.wait()
        m.train()
        D, F, C = m.cfg.dim, m.cfg.dim // 4, m.cfg.num_classes
        N = self._bank_n
        s = _lib.stream()
        W = self._stage2_workspace(n)
        heads = m.heads()
        view, gview = m.head_views()
        if idx is not None:
            idx_in = idx.to(dev, torch.int32).contiguous()
            dual_in = dual.to(dev, torch.int32).contiguous()
            if int(dual_in.shape[0]) != n:
                raise ValueError("step_stage_2: idx and dual differ in length")
        else:
            idx_in = dual_in = None
        call("es_ezbm_sample_mix", ptr(self._bank_x), D, ptr(self._bank_y), N, D, C, ptr(T["off"]), ptr(T["idx"]),
             ptr(T["cdf"]), ptr(T["lam"]), self.sample_seed, self._sample_counter, ptr(idx_in), ptr(dual_in), n,
             ptr(W["X"]), D, ptr(W["t"]), ptr(W["td"]), ptr(W["lam"]), ptr(W["idx"]), ptr(W["dual"]), s)
        if idx is None:
            self._sample_counter += 4 * n
        keep = m.dropout_keep(2 * n) if drop_keep is None else drop_keep.to(dev, torch.uint8).contiguous()
        if tuple(keep.shape) != (2 * n, F):
            raise ValueError(f"step_stage_2: drop_keep of shape {tuple(keep.shape)}, [{2 * n}, {F}] expected")
        # fc(inputs) and fc(mix) as the two BatchNorm groups of one pass over the 2n rows (comatch_model.EmbHeads)
        logits = heads.fc_forward(view, m.bn_buffers(), W["X"], keep, train=True, groups=2)
        stats = torch.empty(3, dtype=torch.float32, device=dev)  # loss, l_o, l_s
        call("es_ezbm_ce_fwd_bwd", ptr(logits), C, ptr(W["t"]), ptr(W["td"]), n, C, float(cfg.TRAIN.LAMBDA_C), 1.0,
             ptr(W["dl"]), C, ptr(stats), s)
        heads.fc_backward(view, gview, W["X"], keep, W["dl"], groups=2, want_dx=False)
        self._finish_step()
        return {"loss": stats[0], "l_o": stats[1], "l_s": stats[2], "logits": logits, "t": W["t"], "td": W["td"],
                "lam": W["lam"], "idx": W["idx"], "dual": W["dual"]}

    def train_one_stage_2(self, epoch):
        """One pass of ceil(N / (BATCH_SIZE * MU)) steps over a bank of N rows, the last one on the rows left (the
        reference's DataLoader over EmbFeatEZBM; its index is ignored by __getitem__, so only the sizes matter)."""
        if getattr(self, "stage", 1) != 2:
            self.setup_stage_2()
        self.model.flat_grad.zero_()
        bsz = int(self.config.DATA.BATCH_SIZE) * int(self.config.DATA.MU)
        N = self._bank_n
        self._stage2_tables()
        sizes = [min(bsz, N - first) for first in range(0, N, bsz)]
        return self._train_steps(lambda n: self.step_stage_2(n=n), sizes, epoch * len(sizes), weight=bsz)

    # ------------------------------------------------------------------------------------ checkpoints, fit
    def load_checkpoint(self, checkpoint_dir, is_train=False):
        """SupLearning.load_checkpoint; a stage-2 checkpoint (its optimizer lists `fc`'s parameters only) sets up
        stage 2 first, so the optimizer state finds its param groups."""
        ck = torch.load(checkpoint_dir, map_location='cpu', weights_only=True)
        n_ck = sum(len(g["params"]) for g in ck["optimizer"]["param_groups"])
        n_now = sum(len(names) for names in self.optimizer._group_names)
        if n_ck != n_now and n_ck == self._fc_param_count():
            self.setup_stage_2()
        super().load_checkpoint(checkpoint_dir, is_train=is_train)

    def _log(self, values):
        if self.wandb is not None:
            self.wandb.log(values)

    def fit(self):
        print('-' * 10, 'Stage 1', '-' * 10)
        print(f"Total Trainable Params: {count_parameters(self.model)}")
        self.config.TRAIN.EPOCHS = self.STAGE1_EPOCHS
        count_early_stop = 0
        for epoch in range(self.epoch_start, self.config.TRAIN.EPOCHS):
            if count_early_stop > 5:
                print('Early stopping stage 1')
                break
            self.epoch = epoch
            train_loss = self.train_one_stage_1(self.epoch)
            self._log({"Loss/train_s1": train_loss.avg})
            if epoch % self.config.TRAIN.FREQ_EVAL == 0 and self.valid_dl is not None:
                valid_loss, valid_metric = self.evaluate_one()
                f1 = float(valid_metric['macro/f1'])
                self._log({"Loss/valid_s1": valid_loss.avg, "Metric/f1_s1": f1})
                count_early_stop += self._track_best(valid_loss.avg, f1, save=False)  # stage 1 saves nothing

        print('-' * 10, 'Stage 2', '-' * 10)
        print('Freeze backbone')
        self.config.TRAIN.EPOCHS = self.STAGE2_EPOCHS
        count_early_stop = 0
        self.setup_stage_2()
        print(f"Total Trainable Params: {count_parameters(self.model)}")
        for epoch in range(self.epoch_start, self.config.TRAIN.EPOCHS):
            if count_early_stop > 10:
                print('Early stopping stage 2')
                break
            self.epoch = epoch
            train_loss = self.train_one_stage_2(self.epoch)
            self._log({"Loss/train_s2": train_loss.avg})
            if epoch % self.config.TRAIN.FREQ_EVAL == 0 and self.valid_dl is not None:
                valid_loss, valid_metric = self.evaluate_one()
                f1 = float(valid_metric['macro/f1'])
                self._log({"Loss/valid_s2": valid_loss.avg, "Metric/f1_s2": f1})
                count_early_stop += self._track_best(valid_loss.avg, f1, save=True)
