"""The trainers' host loops, pinned on the CPU: batch order, scheduler index, loss meter, epoch ranges, the
best-so-far rules, checkpoint keys / file names / restore, and what get_config leaves behind.

`step` (and `step_sup`, `step_stage_1/2`) and `evaluate_one` are replaced on the instance by stubs, so nothing
here launches a kernel: a step stub records its batch and returns {"loss": tensor(k)}, k = 1, 2, ...; an
`evaluate_one` stub returns a scripted (AverageMeter, {"macro/f1": ...}).  Everything else -- train_one, fit,
save_checkpoint, load_checkpoint, get_config -- is the trainers' own code on the tiny models the GPU tests use.
"""
import os
import re
from datetime import datetime

import pytest
import torch

from endossl.utils import AttrDict, AverageMeter

LABELED, UNLABELED = ["a", "b"], ["u", "v", "w"]
SSL = ("FixMatch", "CoMatch", "SemiFormer")
ALL = SSL + ("SupLearning", "EZBM")


# ------------------------------------------------------------------------------------------ fakes
class _DS:
    def __init__(self, df=None):
        self.df = df

    def get_cls_num_list(self):
        return [5] * 23

    def __len__(self):
        return 16


class _DL:
    """List-backed loader: a fresh iterator per iter(), as a DataLoader."""

    def __init__(self, items, df=None):
        self.items, self.dataset = list(items), _DS(df)

    def __iter__(self):
        return iter(self.items)

    def __len__(self):
        return len(self.items)


class _OldIter:
    """An iterator of the reference's era: `.next()` beside `__next__`; counts which one is used."""

    def __init__(self, items, used):
        self.it, self.used = iter(items), used

    def __iter__(self):
        return self

    def next(self):
        self.used.append("next")
        return next(self.it)

    def __next__(self):
        self.used.append("__next__")
        return next(self.it)


class _OldDL(_DL):
    def __init__(self, items):
        super().__init__(items)
        self.used = []

    def __iter__(self):
        return _OldIter(self.items, self.used)


class _Sched:
    """Recording scheduler: every step_update argument, and what load_state_dict was handed."""

    def __init__(self):
        self.updates, self.loaded = [], None

    def step_update(self, num_updates):
        self.updates.append(num_updates)

    def state_dict(self):
        return {"last_update": self.updates[-1] if self.updates else -1}

    def load_state_dict(self, sd):
        self.loaded = sd


def _cfg(**train):
    t = dict(IS_FREEZE=False, USE_EMA=True, EMA_DECAY=0.999, BASE_LR=1e-3, EVAL_STEP=3, EVAL_STEP_SUP=0,
             CLS_WEIGHT=False, THRES=0.5, T=1.0, LAMBDA_U=1.0, LAMBDA_C=1.0, EPOCHS=3, WARMUP_EPOCHS=0,
             DECAY_EPOCHS=10, WARMUP_LR=5e-4, LR_DECAY=0.8, SCH_NAME="step", FREQ_EVAL=1, SAVE_CP=".",
             EXPANSION="balance")
    t.update(train)
    return AttrDict(DATA=AttrDict(BATCH_SIZE=2, MU=2, IMG_SIZE=64, TARGET_NAME="target"),
                    MODEL=AttrDict(NAME="tiny", NUM_CLASSES=23, LOW_DIM=16, MARGIN="None", IS_TRIPLET=False),
                    TRAIN=AttrDict(**t))


def _model(kind):
    from endossl.vit import NativeViT, ViTConfig
    if kind == "FixMatch":
        return NativeViT(ViTConfig(img_size=64, dim=128, depth=2, heads=2, num_classes=23), seed=0)
    if kind in ("CoMatch", "EZBM"):
        from endossl.comatch_model import NativeViTEmb
        return NativeViTEmb(ViTConfig(img_size=64, dim=128, depth=2, heads=2, num_classes=23, head="emb", low_dim=16),
                            seed=0)
    if kind == "SemiFormer":
        from endossl.conformer import ConformerConfig, NativeConformer
        return NativeConformer(ConformerConfig(img_size=64, patch=16, base_channel=16, embed_dim=128, depth=3, heads=2,
                                               num_classes=23), seed=0)
    from endossl.build import build_model
    from endossl.utils import with_defaults
    return build_model(with_defaults(AttrDict(MODEL=AttrDict(NAME="resnet18", NUM_CLASSES=23, MARGIN="None"),
                                              TRAIN=AttrDict(IS_SSL=False), DATA=AttrDict(IMG_SIZE=64))))


def _cls(kind):
    import importlib
    mod = {"FixMatch": "fixmatch", "CoMatch": "comatch", "SemiFormer": "semiformer", "SupLearning": "supervised",
           "EZBM": "ezbm"}[kind]
    return getattr(importlib.import_module("endossl." + mod), kind)


def _trainer(kind, cfg=None, labeled=LABELED, unlabeled=UNLABELED, valid=(), df=None, sched=True):
    """A trainer after get_dataloader + get_config on the CPU, with a recording scheduler (sched=True)."""
    tr = _cls(kind)(_model(kind), device="cpu")
    valid_dl = None if valid is None else _DL(valid)
    if kind in SSL:
        tr.get_dataloader((labeled if isinstance(labeled, _DL) else _DL(labeled, df),
                           unlabeled if isinstance(unlabeled, _DL) else _DL(unlabeled)), valid_dl)
    else:
        tr.get_dataloader(_DL(labeled, df), valid_dl)
    tr.get_config(cfg if cfg is not None else _cfg())
    if sched:
        tr.lr_scheduler = _Sched()
    return tr


def _stub_step(tr, name="step"):
    """Replace tr.<name> by a stub -> the list its calls are recorded in."""
    calls = []

    def stub(*batch, **kw):
        calls.append(batch[0] if batch else kw)
        return {"loss": torch.tensor(float(len(calls)))}
    setattr(tr, name, stub)
    return calls


def _stub_eval(tr, script):
    """evaluate_one -> the scripted (loss, f1) pairs in turn; returns the list of epochs it was called in."""
    seen, script = [], list(script)

    def stub(*a, **kw):
        loss, f1 = script[len(seen)]
        seen.append(getattr(tr, "epoch", None))
        m = AverageMeter()
        m.update(loss, 1)
        return m, {"macro/f1": f1}
    tr.evaluate_one = stub
    return seen


def _saved(folder):
    return sorted(os.listdir(folder))


# ------------------------------------------------------------------------------------------ train_one
def test_fixmatch_train_one_pairs_restart_each_loader_on_its_own():
    tr = _trainer("FixMatch")
    calls = _stub_step(tr)
    meter = tr.train_one(2)
    assert calls == [("a", "u"), ("b", "v"), ("a", "w")]  # exactly EVAL_STEP steps
    assert tr.lr_scheduler.updates == [2 * 3 + 0, 2 * 3 + 1, 2 * 3 + 2]  # epoch * EVAL_STEP + i
    assert meter.avg == pytest.approx(2.0) and meter.count == 3 * 2  # updated with DATA.BATCH_SIZE
    tr = _trainer("FixMatch", _cfg(EVAL_STEP=5))
    calls = _stub_step(tr)
    tr.train_one(0)
    assert calls == [("a", "u"), ("b", "v"), ("a", "w"), ("b", "u"), ("a", "v")]
    assert tr.lr_scheduler.updates == [0, 1, 2, 3, 4]


def test_comatch_train_one_walks_the_unlabeled_loader_with_the_first_labeled_batch():
    tr = _trainer("CoMatch", _cfg(EVAL_STEP=5))
    calls = _stub_step(tr)
    meter = tr.train_one(2)
    assert calls == [("a", "u"), ("a", "v"), ("a", "w")]
    assert tr.lr_scheduler.updates == [10, 11, 12]  # epoch * EVAL_STEP + i, whatever the loader's length
    assert meter.avg == pytest.approx(2.0) and meter.count == 3 * 2


def test_semiformer_train_one_supervised_epochs_then_the_fixmatch_pairing():
    tr = _trainer("SemiFormer", _cfg(EVAL_STEP_SUP=2))
    sup, ssl = _stub_step(tr, "step_sup"), _stub_step(tr, "step")
    meter = tr.train_one(1)  # epoch < EVAL_STEP_SUP
    assert sup == ["a", "b"] and ssl == []
    assert tr.lr_scheduler.updates == [1 * 2 + 0, 1 * 2 + 1]  # epoch * len(labeled loader) + i
    assert meter.avg == pytest.approx(1.5) and meter.count == 2 * 2
    tr.lr_scheduler.updates.clear()
    meter = tr.train_one(2)
    assert sup == ["a", "b"] and ssl == [("a", "u"), ("b", "v"), ("a", "w")]
    assert tr.lr_scheduler.updates == [6, 7, 8]  # epoch * EVAL_STEP + i
    assert meter.avg == pytest.approx(2.0) and meter.count == 3 * 2


def test_suplearning_train_one_walks_train_dl():
    tr = _trainer("SupLearning", labeled=["a", "b", "c"])
    calls = _stub_step(tr)
    meter = tr.train_one(4)
    assert calls == ["a", "b", "c"]
    assert tr.lr_scheduler.updates == [12, 13, 14]  # epoch * len(train_dl) + i
    assert meter.avg == pytest.approx(2.0) and meter.count == 3 * 2


def test_ezbm_train_one_both_stages():
    tr = _trainer("EZBM", labeled=["a", "b", "c"])
    tr._bank_n = 7  # a previous epoch's rows: the bank holds the last epoch run
    calls = _stub_step(tr, "step_stage_1")
    meter = tr.train_one_stage_1(3)
    assert calls == ["a", "b", "c"] and tr._bank_n == 0
    assert tr.lr_scheduler.updates == [9, 10, 11]  # epoch * len(train_dl) + i
    assert meter.avg == pytest.approx(2.0) and meter.count == 3 * 2
    # stage 2: ceil(N / (BATCH_SIZE * MU)) steps, the last on the rows left; the meter weighs BATCH_SIZE * MU
    tr.set_bank(torch.randn(23 + 3, 128), torch.arange(23 + 3) % 23)
    tr.setup_stage_2()
    tr.lr_scheduler = _Sched()
    calls = _stub_step(tr, "step_stage_2")
    meter = tr.train_one_stage_2(2)
    assert calls == [{"n": 4}] * 6 + [{"n": 2}]
    assert tr.lr_scheduler.updates == [2 * 7 + i for i in range(7)]
    assert meter.avg == pytest.approx(4.0) and meter.count == 7 * 4


@pytest.mark.parametrize("kind", ["FixMatch", "SemiFormer"])
@pytest.mark.parametrize("which", ["labeled", "unlabeled"])
def test_an_empty_loader_raises(kind, which):
    tr = _trainer(kind, **{which: []})
    calls = _stub_step(tr)
    # the restart finds nothing either: StopIteration, or the RuntimeError it turns into inside a generator
    with pytest.raises((StopIteration, RuntimeError)):
        tr.train_one(0)
    assert calls == []


def test_comatch_empty_labeled_loader_raises():
    tr = _trainer("CoMatch", labeled=[])
    _stub_step(tr)
    with pytest.raises((StopIteration, RuntimeError)):
        tr.train_one(1)


def test_loader_pairing_goes_through_next():
    """Iterators with a `.next` method are advanced through it (fixmatch._next)."""
    from endossl.fixmatch import _next
    lab, unl = _OldDL(LABELED), _OldDL(UNLABELED)
    tr = _trainer("FixMatch", labeled=lab, unlabeled=unl)
    calls = _stub_step(tr)
    tr.train_one(0)
    assert calls == [("a", "u"), ("b", "v"), ("a", "w")]
    assert set(lab.used) == {"next"} and set(unl.used) == {"next"}
    assert _next(iter([7])) == 7


def test_fixmatch_train_one_without_a_scheduler():
    tr = _trainer("FixMatch", _cfg(SCH_NAME="const"), sched=False)
    assert tr.lr_scheduler is None
    _stub_step(tr)
    assert tr.train_one(0).avg == pytest.approx(2.0)


# ------------------------------------------------------------------------------------------ fit
@pytest.mark.parametrize("kind", SSL)
def test_fit_of_the_best_valid_perf_trainers(kind, tmp_path, capsys):
    """FixMatch / CoMatch: range(epoch_start = 1, EPOCHS + 1); SemiFormer: range(0, EPOCHS).  The minimum is kept
    and every evaluated epoch saves on rank 0."""
    tr = _trainer(kind, _cfg(SAVE_CP=str(tmp_path)))
    first = 0 if kind == "SemiFormer" else 1
    assert tr.epoch_start == first and tr.best_valid_perf is None
    _stub_step(tr)
    seen = _stub_eval(tr, [(0.5, 0.1), (0.7, 0.2), (0.3, 0.3)])
    tr.fit()
    assert seen == [first, first + 1, first + 2]
    assert tr.best_valid_perf == 0.3
    files = _saved(tmp_path)
    assert len(files) == 3
    best = {torch.load(tmp_path / f, weights_only=True)["epoch"]: torch.load(tmp_path / f, weights_only=True)[
        "best_valid_perf"] for f in files}
    assert best == {first: 0.5, first + 1: 0.5, first + 2: 0.3}
    out = capsys.readouterr().out
    assert f"Training epoch: {first} | Current LR: 0.001000 | The best loss: inf" in out
    assert f"Training epoch: {first + 1} | Current LR: 0.001000 | The best loss: 0.500" in out
    assert "\tTrain Loss: 2.000" in out and "\tValid Loss: 0.700" in out and "\tMetric: {'macro/f1': 0.2}" in out
    assert out.count("Saved checkpoint") == 3


@pytest.mark.parametrize("kind", ["FixMatch", "CoMatch"])
def test_fit_evaluates_only_when_epoch_start_is_epochs(kind, tmp_path, capsys):
    tr = _trainer(kind, _cfg(SAVE_CP=str(tmp_path)))
    calls = _stub_step(tr)
    seen = _stub_eval(tr, [(0.5, 0.1)])
    tr.epoch_start = 3
    tr.fit()
    assert calls == [] and len(seen) == 1 and _saved(tmp_path) == [] and tr.best_valid_perf is None
    out = capsys.readouterr().out
    assert "\tValid Loss: 0.500" in out and "Training epoch" not in out


@pytest.mark.parametrize("kind", SSL)
def test_fit_saves_on_rank_0_only_and_skips_evaluation_without_valid_dl(kind, tmp_path, monkeypatch):
    from endossl import dist
    tr = _trainer(kind, _cfg(SAVE_CP=str(tmp_path), FREQ_EVAL=2))
    _stub_step(tr)
    seen = _stub_eval(tr, [(0.5, 0.1), (0.4, 0.1)])
    monkeypatch.setattr(dist, "rank", lambda: 1)
    tr.fit()
    assert seen == ([0, 2] if kind == "SemiFormer" else [2])  # epoch % FREQ_EVAL == 0
    assert _saved(tmp_path) == [] and tr.best_valid_perf == (0.4 if kind == "SemiFormer" else 0.5)
    tr = _trainer(kind, _cfg(SAVE_CP=str(tmp_path)), valid=None)
    _stub_step(tr)
    seen = _stub_eval(tr, [])
    tr.fit()
    assert seen == [] and tr.best_valid_perf is None


# better in loss AND score -> new best, saved; worse in either -> one towards the early stop, never reset;
# neither (equal score) -> nothing.  Epoch 0 has no best yet.
SCRIPT = [(1.0, 0.5),    # first: taken, saved
          (0.8, 0.6),    # better in both: saved
          (0.9, 0.7),    # worse loss: count 1
          (0.7, 0.6),    # better loss, equal score: neither
          (0.6, 0.8),    # better in both: saved, the count stays 1
          (0.5, 0.7), (0.7, 0.9), (0.7, 0.7), (0.9, 0.9), (0.9, 0.1)]  # worse in one or both: count 2 .. 6


def test_suplearning_fit_best_rule_and_early_stop(tmp_path, capsys):
    tr = _trainer("SupLearning", _cfg(SAVE_CP=str(tmp_path), EPOCHS=30))
    assert tr.epoch_start == 0 and tr.best_valid_loss is None and tr.best_valid_score is None
    _stub_step(tr)
    seen = _stub_eval(tr, SCRIPT + [(0.1, 0.99)] * 5)
    tr.fit()
    assert seen == list(range(10))  # range(0, EPOCHS), stopped once the count is past 5
    assert (tr.best_valid_loss, tr.best_valid_score) == (0.6, 0.8)
    files = _saved(tmp_path)
    assert sorted(torch.load(tmp_path / f, weights_only=True)["epoch"] for f in files) == [0, 1, 4]
    out = capsys.readouterr().out
    assert out.count("Early stopping") == 1 and out.count("\tTrain Loss: ") == 10 and "\tTrain Loss: 1.500" in out
    assert "\tValid Loss: 0.900" in out and "Saved checkpoint" not in out


def test_suplearning_fit_runs_all_epochs_without_an_early_stop(tmp_path):
    tr = _trainer("SupLearning", _cfg(SAVE_CP=str(tmp_path), EPOCHS=3))
    _stub_step(tr)
    seen = _stub_eval(tr, SCRIPT)
    tr.fit()
    assert seen == [0, 1, 2]


def test_ezbm_fit_stage_1_saves_nothing_stage_2_stops_past_10(tmp_path, capsys):
    tr = _trainer("EZBM", _cfg(SAVE_CP=str(tmp_path)))
    tr.STAGE1_EPOCHS, tr.STAGE2_EPOCHS = 20, 30
    ran = {1: [], 2: []}

    def one(stage):
        def stub(epoch):
            ran[stage].append(epoch)
            m = AverageMeter()
            m.update(1.0, 1)
            return m
        return stub
    tr.train_one_stage_1, tr.train_one_stage_2 = one(1), one(2)
    stage2 = [(0.5, 0.9)] + [(0.9, 0.1)] * 11 + [(0.1, 0.99)] * 5
    seen = _stub_eval(tr, SCRIPT + stage2)
    tr.fit()
    assert ran[1] == list(range(10))  # stopped past 5
    assert ran[2] == list(range(12))  # the best carries over; stopped past 10
    assert len(seen) == 22 and tr.stage == 2
    assert (tr.best_valid_loss, tr.best_valid_score) == (0.5, 0.9)
    files = _saved(tmp_path)
    assert len(files) == 1  # stage 1 saved nothing; stage 2 its one better epoch
    ck = torch.load(tmp_path / files[0], weights_only=True)
    assert ck["epoch"] == 0 and (ck["best_valid_loss"], ck["best_valid_score"]) == (0.5, 0.9)
    out = capsys.readouterr().out
    assert "Early stopping stage 1" in out and "Early stopping stage 2" in out and "Freeze backbone" in out


# ------------------------------------------------------------------------------------------ checkpoints
def _same_state(a, b):
    """Every state_dict entry equal (the flat buffers' padding between entries is not state)."""
    sa, sb = a.state_dict(), b.state_dict()
    return list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def _best_keys(kind):
    return {"best_valid_perf"} if kind in SSL else {"best_valid_loss", "best_valid_score"}


@pytest.mark.parametrize("kind", ALL)
@pytest.mark.parametrize("use_ema", [True, False])
def test_checkpoint_keys_and_file_name(kind, use_ema, tmp_path, capsys):
    tr = _trainer(kind, _cfg(USE_EMA=use_ema))
    tr.epoch = 7
    h0 = datetime.now().hour
    path = tr.save_checkpoint(str(tmp_path))
    h1 = datetime.now().hour
    ck = torch.load(path, map_location="cpu", weights_only=True)
    want = {"epoch", "model_state_dict", "optimizer", "scheduler"} | _best_keys(kind)
    assert set(ck) == (want | {"ema_state_dict"} if use_ema else want)
    assert ck["epoch"] == 7 and ck["scheduler"] == {"last_update": -1}
    suffix = "_epoch_7_size_64" if kind in ("FixMatch", "CoMatch") else "_epoch_7"
    m = re.fullmatch(r"\d\d_\d\d_\d{4}_(\d+)_\d\d_\d\d" + suffix + r"\.pth", os.path.basename(path))
    assert m and os.path.dirname(path) == str(tmp_path)
    assert int(m.group(1)) in (h0 + 2, h1 + 2)  # the reference's `int(hour) + 2`
    printed = "Saved checkpoint" in capsys.readouterr().out
    assert printed == (kind in SSL)


@pytest.mark.parametrize("kind", ALL)
def test_load_checkpoint_restores_epoch_and_best(kind, tmp_path):
    tr = _trainer(kind)
    tr.epoch = 5
    for k in _best_keys(kind):
        setattr(tr, k, 0.25)
    tr.lr_scheduler.updates.append(41)
    with torch.no_grad():
        tr.model.flat.add_(1.0)
        tr.ema_model.ema.flat.sub_(1.0)
    tr.optimizer.step_count = 9
    path = tr.save_checkpoint(str(tmp_path))
    new = _trainer(kind)
    assert not _same_state(new.model, tr.model)
    new.load_checkpoint(path, is_train=True)
    assert new.epoch_start == 5
    assert _same_state(new.model, tr.model) and _same_state(new.ema_model.ema, tr.ema_model.ema)
    assert not _same_state(new.model, new.ema_model.ema)
    assert new.optimizer.step_count == 9 and new.lr_scheduler.loaded == {"last_update": 41}
    if kind in SSL:
        assert new.best_valid_perf == 0.25
    else:  # SupLearning.load_checkpoint does not restore its best loss / score
        assert new.best_valid_loss is None and new.best_valid_score is None


FROZEN = {"FixMatch": ("head.",), "CoMatch": ("fc.", "head_emb."),
          "SemiFormer": ("conv_cls_head.", "trans_cls_head.")}


def _trainable(model):
    return [n for n, p in model.named_parameters() if p.requires_grad]


@pytest.mark.parametrize("kind", SSL)
def test_is_freeze_in_get_config_and_after_load_checkpoint(kind, tmp_path):
    tr = _trainer(kind, _cfg(IS_FREEZE=True))
    names = [n for n, _ in tr.model.named_parameters()]
    heads = [n for n in names if n.startswith(FROZEN[kind])]
    assert heads and _trainable(tr.model) == heads and tr.frozen
    assert sum(len(g) for g in tr.optimizer._group_names) == len(heads)
    # the EMA copy: FixMatch / CoMatch freeze before it is made (the ViT's copy does not carry the flags),
    # SemiFormer after, so its copy is neither frozen nor marked frozen_trunk
    ema = tr.ema_model.ema
    assert _trainable(ema) == names
    if kind == "SemiFormer":
        assert tr.model.frozen_trunk is True and not getattr(ema, "frozen_trunk", False)
    tr.epoch = 1
    path = tr.save_checkpoint(str(tmp_path))
    tr.load_checkpoint(path, is_train=False)
    assert _trainable(tr.model) == []
    tr.load_checkpoint(path, is_train=True)
    # FixMatch / CoMatch re-apply the IS_FREEZE split (_trainable_when_frozen); SemiFormer trains everything
    assert _trainable(tr.model) == (names if kind == "SemiFormer" else heads)
    tr = _trainer(kind)
    assert _trainable(tr.model) == names and not tr.frozen


@pytest.mark.parametrize("kind", ["SupLearning", "EZBM"])
def test_load_checkpoint_requires_grad_follows_is_train(kind, tmp_path):
    tr = _trainer(kind)
    names = [n for n, _ in tr.model.named_parameters()]
    tr.epoch = 0
    path = tr.save_checkpoint(str(tmp_path))
    tr.load_checkpoint(path, is_train=False)
    assert _trainable(tr.model) == []
    tr.load_checkpoint(path, is_train=True)
    assert _trainable(tr.model) == names


def test_ezbm_load_checkpoint_sets_up_stage_2_for_a_stage_2_checkpoint(tmp_path):
    tr = _trainer("EZBM")
    tr.setup_stage_2()
    tr.lr_scheduler = _Sched()
    tr.epoch = 3
    path = tr.save_checkpoint(str(tmp_path))
    new = _trainer("EZBM", sched=False)
    assert new.stage == 1
    new.load_checkpoint(path, is_train=True)
    assert new.stage == 2 and new.epoch_start == 3
    assert sum(len(g) for g in new.optimizer._group_names) == 6


# ------------------------------------------------------------------------------------------ get_config
@pytest.mark.parametrize("kind", ALL)
def test_get_config_class_weights_scheduler_and_throttle(kind):
    df = {"target": [0, 0, 1, 2]}
    tr = _trainer(kind, _cfg(CLS_WEIGHT=True), df=df, sched=False)
    assert tr.class_weights.dtype == torch.float32 and tr.class_weights.device.type == "cpu"
    torch.testing.assert_close(tr.class_weights, torch.tensor([4 / 6, 4 / 3, 4 / 3]))
    assert tr.ema_model is not None and tr.ema_model.decay == 0.999
    assert tr.ema_model.ema is not tr.model and torch.equal(tr.ema_model.ema.flat, tr.model.flat)
    # the scheduler's steps per epoch: EVAL_STEP for the SSL trainers, len(train_dl) for the supervised ones
    per_epoch = 3 if kind in SSL else 2
    assert tr.lr_scheduler.decay_t == 10 * per_epoch
    tr = _trainer(kind, _cfg(USE_EMA=False, SCH_NAME="const"), sched=False)
    assert tr.class_weights is None and tr.ema_model is None and tr.lr_scheduler is None
    env = os.environ.get("ENDOSSL_MAX_INFLIGHT_STEPS")
    depth = 2 if kind in ("FixMatch", "CoMatch") else 1  # throttle.py: the ViT engine keeps its own buffers
    assert tr._inflight.depth == (int(env) if env is not None else depth)


def test_get_dataloader_forms():
    tr = _trainer("SemiFormer")
    assert tr.train_labeled_dl.items == LABELED and tr.train_unlabeled_dl.items == UNLABELED and tr.test_dl is None
    sup = _cls("SupLearning")(_model("SupLearning"), device="cpu")
    with pytest.raises(NotImplementedError, match="mixup"):
        sup.get_dataloader(_DL([]), None, mixup_fn=lambda x: x)
    sup.get_dataloader(_DL(["a"]), None, None, "t")
    assert sup.train_dl.items == ["a"] and sup.test_dl == "t" and sup.mixup_fn is None


# ------------------------------------------------------------------------------------------ evaluate_one
class _FakeModel:
    """Stands in for the evaluated model: logits that put row i in class (i + shift) % 23."""

    def __init__(self, as_tuple):
        self.flat, self.as_tuple, self.evals = torch.zeros(1), as_tuple, 0

    def eval(self):
        self.evals += 1

    def __call__(self, images):
        logits = torch.nn.functional.one_hot(images.view(-1).long() % 23, 23).float()
        return (logits, "fts", "z") if self.as_tuple else logits


@pytest.mark.parametrize("kind", ["FixMatch", "CoMatch"])
def test_evaluate_one_takes_the_logits_of_either_model_form(kind, monkeypatch, capsys):
    """FixMatch's model returns logits, CoMatch's (logits, fts, z): the same loop serves both.  The loss kernel is
    replaced (torch's CE) -- this pins the loop, the meter and the metrics tail, not the arithmetic."""
    import endossl.comatch
    import endossl.fixmatch
    for mod in (endossl.fixmatch, endossl.comatch):
        monkeypatch.setattr(mod, "ce_loss", lambda o, t, reduction: torch.nn.functional.cross_entropy(o, t),
                            raising=False)
    x = torch.arange(6)
    tr = _trainer(kind, _cfg(USE_EMA=False), valid=[(x[:4], x[:4]), (x[4:], (x[4:] + 1) % 23)])
    tr.model = _FakeModel(as_tuple=kind == "CoMatch")
    loss, metric = tr.evaluate_one(show_metric=True)
    assert tr.model.evals == 1 and loss.count == 2 * 2  # updated with DATA.BATCH_SIZE per batch
    assert metric["micro/f1"] == pytest.approx(4 / 6)
    assert set(metric) == {"micro/precision", "micro/recall", "micro/f1", "macro/precision", "macro/recall",
                           "macro/f1", "sen/spec"}
    assert capsys.readouterr().out.startswith("Metric:\n")


# ------------------------------------------------------------------------------------------ no scheduler
@pytest.mark.parametrize("kind", ["SupLearning", "SemiFormer"])
def test_none_scheduler_is_tolerated(kind, tmp_path):
    """NEW BEHAVIOUR with the shared trainer base: SCH_NAME 'const' (build_scheduler -> None) trains, saves {} and
    loads, as FixMatch always did; these two trainers raised AttributeError before."""
    cfg = _cfg(SCH_NAME="const", EVAL_STEP_SUP=1)
    tr = _trainer(kind, cfg, sched=False)
    assert tr.lr_scheduler is None
    _stub_step(tr)
    _stub_step(tr, "step_sup")
    assert tr.train_one(0).count == 2 * 2
    assert tr.train_one(1).count == (3 if kind == "SemiFormer" else 2) * 2
    tr.epoch = 1
    path = tr.save_checkpoint(str(tmp_path))
    assert torch.load(path, weights_only=True)["scheduler"] == {}
    new = _trainer(kind, cfg, sched=False)
    new.load_checkpoint(path, is_train=True)
    assert new.epoch_start == 1 and new.lr_scheduler is None
