"""The reverse pass's ordering decisions (endossl/vit.py, _WgradSchedule), checked without a GPU or the library: the
scheduler is driven alone, in the order Engine.backward and the block chain call it, with stub streams, a recording
`on_stream` and recording launchers.  The expected event / launch lists below are transcribed by hand from
Engine.backward as of commit c7397e9 (the `vit.py:` / `block.py:` line numbers are that commit's), not produced by
the code under test."""
import contextlib
import os
import sys
import types

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "endoscopy-image-classification_amd"))
from endossl import vit  # noqa: E402

DEPTH, GROUP_LAYERS, MIN_M = 5, 2, 100
M, M_PATCH, M_CLS = 200, 150, 8  # token rows, patch rows (both >= MIN_M), the last block's CLS rows (< MIN_M)
# (kind, N1, N2): a block's four weight gradients in the chain's order (block.py:162, 165, 172, 193) -- all multiples
# of the 384 x 192 tile -- and the patch embedding's (vit.py:790)
KINDS = [("fc2", 384, 1536), ("fc1", 1536, 384), ("proj", 384, 384), ("qkv", 1152, 384)]
PATCH = ("patch", 384, 768)


class Stream:
    """Logs wait_stream / wait_event / record_event; its events are named <stream>#<count>."""

    def __init__(self, name, log):
        self.name, self.log, self.count = name, log, 0

    def wait_stream(self, other):
        self.log.append(("wait_stream", self.name, other.name))

    def wait_event(self, ev):
        self.log.append(("wait_event", self.name, ev))

    def record_event(self):
        ev = f"{self.name}#{self.count}"
        self.count += 1
        self.log.append(("record_event", self.name, ev))
        return ev


class Rig:
    """A scheduler over stub streams and recording launchers, and the calls of one reverse pass."""

    def __init__(self, overlap=True, group_wgrad="0", layer_wgrad=True, tokens=M, grad_ready=False, capture=False):
        self.log, self.cur = [], "main"
        self.main = Stream("main", self.log)
        self.side = Stream("side", self.log) if overlap else None
        ready = (lambda lo, hi, evs: self.log.append(("grad_ready", lo, hi, tuple(evs)))) if grad_ready else None
        # grouped as Engine.backward decides it (vit.py:648, 861-864)
        eng = types.SimpleNamespace(precision="bf16", GROUP_WGRAD=group_wgrad, GROUP_WGRAD_MAX_M=16384)
        grouped = vit.Engine._grouped_wgrad(eng, tokens, ready)
        self.sets = [f"G{k}" for k in range(DEPTH + 1)] if grouped else ["A", "B"]  # vit.py:639, 654
        self.sched = vit._WgradSchedule(
            self.sets, tokens, DEPTH, grouped, layer_wgrad=layer_wgrad, defer_ln=True, bf16=True, capture=capture,
            group_layers=GROUP_LAYERS, min_m=MIN_M, main=self.main, side=self.side, wgrad=self.wgrad,
            wgrad_layer=self.wgrad_layer, launch_grouped=self.launch_grouped, ln_flush=self.ln_flush, grad_ready=ready,
            block_range=lambda i: (10 * i, 10 * i + 10), on_stream=self.on_stream)

    @contextlib.contextmanager
    def on_stream(self, st, *after):
        """block.on_stream (block.py:210-216): st waits for `after`, then is the current stream; None: no change."""
        if st is None:
            yield
            return
        for w in after:
            st.wait_stream(w)
        self.cur, prev = st.name, self.cur
        yield
        self.cur = prev

    # the engine's launchers: what was launched, on which stream
    def wgrad(self, dy, N1, x, N2, Mw, out, bias_out=None, ld1=None, ld2=None, label=None):
        self.log.append(("wgrad", self.cur, label))

    def wgrad_layer(self, problems, i):
        self.log.append(("wgrad_layer", self.cur, i, tuple(q[9] for q in problems)))

    def launch_grouped(self, problems, slot):
        self.log.append(("launch_grouped", self.cur, slot, tuple(q[0] for q in problems)))

    def ln_flush(self, pending):  # Engine._ln_grads_flush clears the list it reduced (vit.py:619)
        self.log.append(("ln_flush", self.cur, tuple(pending)))
        pending.clear()

    def ln_bwd(self, name):
        """A LayerNorm backward as Engine._ln_bwd (vit.py:584-592): deferred, or reduced on the chain."""
        if self.sched.defer is not None:
            self.sched.defer.append(name)
        else:
            self.log.append(("ln_chain", name))

    def run(self, cls_q=False):
        """One reverse pass in Engine.backward's order (vit.py:746-797) with the chain's callback order
        (block.py:153-198): fc2, fc1, LN2, proj, qkv, before_ln1, LN1, then block_done.  cls_q: the last block's
        qkv problem over the CLS rows only."""
        s = self.sched
        for i in reversed(range(DEPTH)):
            for kind, N1, N2 in KINDS:
                rows = M_CLS if cls_q and kind == "qkv" and i == DEPTH - 1 else M
                s.wgrad(f"{kind}.{i}", N1, "x", N2, rows, "out", "bias", label=f"{kind}.{i}")
                if kind == "fc1":
                    self.ln_bwd(f"ln2.{i}")
            s.before_ln1(i)
            self.ln_bwd(f"ln1.{i}")
            s.block_done(i)
        kind, N1, N2 = PATCH
        s.wgrad(kind, N1, "x", N2, M_PATCH, "out", "bias", label=kind)
        s.finish()
        return self.log


def names(i):
    return tuple(f"{kind}.{i}" for kind, _, _ in KINDS)


def each_on_side(label):
    # vit.py:679-680 through block.py:214-216: the side stream waits for the caller's, then launches
    return [("wait_stream", "side", "main"), ("wgrad", "side", label)]


def test_each_overlapped():
    r = Rig(layer_wgrad=False)
    assert r.sched.mode == "each" and r.sched.defer is None  # vit.py:662, 665-666 (neither grouped nor layer_wg)
    e = []
    for k, i in enumerate(reversed(range(DEPTH))):
        e += each_on_side(f"fc2.{i}") + each_on_side(f"fc1.{i}") + [("ln_chain", f"ln2.{i}")]
        e += each_on_side(f"proj.{i}") + each_on_side(f"qkv.{i}")
        e += [("record_event", "side", f"side#{k}")]  # vit.py:757-758 (flush_layer returned at 687-688)
        if k > 0:  # vit.py:759-760: block i + 1's event
            e += [("wait_event", "main", f"side#{k - 1}")]
        e += [("ln_chain", f"ln1.{i}")]  # block_done: nothing (vit.py:699, 708)
    e += each_on_side("patch")  # vit.py:790
    e += [("wait_stream", "main", "side")]  # vit.py:796-797
    assert r.run() == e
    assert not r.sched.problems


def test_each_serial():
    r = Rig(overlap=False, layer_wgrad=False)
    assert r.sched.mode == "each" and r.sched.defer is None
    e = []
    for i in reversed(range(DEPTH)):  # vit.py:679-680 with side None (block.py:212-213): the caller's stream, no events
        e += [("wgrad", "main", f"fc2.{i}"), ("wgrad", "main", f"fc1.{i}"), ("ln_chain", f"ln2.{i}"),
              ("wgrad", "main", f"proj.{i}"), ("wgrad", "main", f"qkv.{i}"), ("ln_chain", f"ln1.{i}")]
    e += [("wgrad", "main", "patch")]  # vit.py:790; no join (vit.py:796)
    assert r.run() == e


def test_layer_overlapped_deferred():
    r = Rig()
    assert r.sched.mode == "layer" and r.sched.defer == []  # vit.py:662, 665-666
    top = DEPTH - 1
    e = each_on_side(f"qkv.{top}")  # M_CLS < TN_SHARE_MIN_M: misses vit.py:675, goes out at 679-680
    for k, i in enumerate(reversed(range(DEPTH))):
        lp = names(i)[:3] if i == top else names(i)
        pending = (f"ln2.{i}",) if i == top else (f"ln1.{i + 1}", f"ln2.{i}")
        # before_ln1 -> flush_layer(i), vit.py:689-694: one context, the block's launch, the LayerNorm flush
        e += [("wait_stream", "side", "main"), ("wgrad_layer", "side", i, lp), ("ln_flush", "side", pending)]
        e += [("record_event", "side", f"side#{k}")]  # vit.py:757-758
        if k > 0:
            e += [("wait_event", "main", f"side#{k - 1}")]  # vit.py:759-760
    # vit.py:790-791: the patch problem fits the rule, flush_layer(-1) with block 0's LayerNorm 1; 794: nothing left
    e += [("wait_stream", "side", "main"), ("wgrad_layer", "side", -1, ("patch",)), ("ln_flush", "side", ("ln1.0",))]
    e += [("wait_stream", "main", "side")]  # vit.py:796-797
    assert r.run(cls_q=True) == e
    assert r.sched.defer == [] and not r.sched.problems


def test_layer_needs_the_token_count():
    """vit.py:662: below TN_SHARE_MIN_M tokens LAYER_WGRAD gives way to one launch per GEMM, and nothing is deferred."""
    r = Rig(tokens=MIN_M - 1)
    assert r.sched.mode == "each" and r.sched.defer is None


def test_grouped_deferred():
    r = Rig(group_wgrad="1")
    assert r.sched.mode == "grouped" and r.sched.defer == []
    lns = lambda *blocks: tuple(f"{ln}.{i}" for i in blocks for ln in ("ln2", "ln1"))  # noqa: E731
    e = [  # vit.py:699-707: the blocks i > 0 with i % GROUP_LAYERS == 0, on the side stream; no events (ovw, vit.py:656)
        ("wait_stream", "side", "main"), ("launch_grouped", "side", 4, names(4)), ("ln_flush", "side", lns(4)),
        ("wait_stream", "side", "main"), ("launch_grouped", "side", 2, names(3) + names(2)),
        ("ln_flush", "side", lns(3, 2)),
        # vit.py:792-797: slot 0 and the last flush on the caller's stream, then the join
        ("launch_grouped", "main", 0, names(1) + names(0) + ("patch",)), ("ln_flush", "main", lns(1, 0)),
        ("wait_stream", "main", "side")]
    assert r.run() == e
    # vit.py:749: one dY set per layer, the spare for block 0's d(block input); vit.py:722: the top of the stack
    assert [r.sched.grad_sets(i) for i in range(DEPTH)] == [("G0", "G5"), ("G1", "G0"), ("G2", "G1"), ("G3", "G2"),
                                                            ("G4", "G3")]


def test_two_alternating_sets():
    r = Rig()  # vit.py:751 (and 722: block depth - 1's set)
    assert [r.sched.grad_sets(i) for i in range(DEPTH)] == [("A", "B"), ("B", "A"), ("A", "B"), ("B", "A"), ("A", "B")]


def test_grad_ready_hand_over():
    r = Rig(group_wgrad="1", grad_ready=True)
    # vit.py:862-863: never grouped with a hand-over; vit.py:665: no deferral
    assert r.sched.mode == "layer" and r.sched.defer is None
    e = []
    for k, i in enumerate(reversed(range(DEPTH))):
        e += [("ln_chain", f"ln2.{i}")]
        e += [("wait_stream", "side", "main"), ("wgrad_layer", "side", i, names(i))]  # vit.py:689-692
        e += [("record_event", "side", f"side#{k}")]  # vit.py:758: done[i]
        if k > 0:
            e += [("wait_event", "main", f"side#{k - 1}")]  # vit.py:759-760: done[i + 1]
        e += [("ln_chain", f"ln1.{i}")]
        # vit.py:710-713: the caller's stream's event and done[i]
        e += [("record_event", "main", f"main#{k}"), ("grad_ready", 10 * i, 10 * i + 10, (f"main#{k}", f"side#{k}"))]
    e += [("wait_stream", "side", "main"), ("wgrad_layer", "side", -1, ("patch",))]  # vit.py:790-791
    e += [("wait_stream", "main", "side")]  # vit.py:796-797
    assert r.run() == e


def test_capture_keeps_the_reductions_on_the_chain():
    """vit.py:665: with the test hook set nothing is deferred."""
    assert Rig(capture=True).sched.defer is None and Rig(group_wgrad="1", capture=True).sched.defer is None
