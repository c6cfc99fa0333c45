"""Distributed optimizers over the sparse allreduce engine.

Three surfaces, the first two mirroring the reference:

* DistributedOptimizer — Horovod-style wrapper (factory parity with
  /root/reference/VGG/distributed_optimizer.py:203): autograd hooks capture
  per-parameter gradients into flat buckets (size-merged like the reference's
  _generate_merged_parameters, VGG/allreducer.py:272-366), each completed
  bucket is sparse-allreduced, `synchronize()` + `step()` apply the inner
  optimizer.  Unlike the reference there is no background Python thread: the
  gradients accumulate directly into bucket-flat storage (p.grad is a view),
  and bucket completion fires the reduce inline from the hook so RCCL comm
  overlaps the rest of backward on its own stream.

* FlatBertAdam — BertAdam parity (/root/reference/BERT/bert/transformers/
  optimization.py:68-227): one flat gradient vector for the whole model,
  one engine.run() per step, warmup-scheduled lr, fused Adam step kernels.

* FlatSGD — the DistributedOptimizer machinery with the SGD step itself on
  flat per-bucket storage: one fused launch per bucket, taking the bucket's
  gradient in sparse form where the engine hands it over that way.
"""
from __future__ import annotations

import math
import os
import queue
import threading
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from . import ops
from .allreducer import AllReducer
from .comm import Comm
from .config import EngineConfig

__all__ = ["DistributedOptimizer", "FlatBertAdam", "FlatSGD", "SCHEDULES"]


# -- BertAdam warmup schedules (reference optimization.py:40-58) -----------

def warmup_cosine(x: float, warmup: float = 0.002) -> float:
    if x < warmup:
        return x / warmup
    return 0.5 * (1.0 + math.cos(math.pi * x))


def warmup_constant(x: float, warmup: float = 0.002) -> float:
    if x < warmup:
        return x / warmup
    return 1.0


def warmup_linear(x: float, warmup: float = 0.002) -> float:
    if x < warmup:
        return x / warmup
    return max((x - 1.0) / (warmup - 1.0), 0.0)


def warmup_poly(x: float, warmup: float = 0.002, degree: float = 0.5) -> float:
    # reference optimization.py:55-58
    if x < warmup:
        return x / warmup
    return (1.0 - x) ** degree


SCHEDULES = {
    "warmup_cosine": warmup_cosine,
    "warmup_constant": warmup_constant,
    "warmup_linear": warmup_linear,
    "warmup_poly": warmup_poly,
    "none": lambda x, warmup=0: 1.0,
}


class _Bucket:
    def __init__(self, name: str, params: List[torch.Tensor], device, dtype=torch.float32):
        self.name = name
        self.params = params
        self.numel = sum(p.numel() for p in params)
        self.flat = torch.zeros(self.numel, dtype=dtype, device=device)
        self.slots: List[Tuple[int, int]] = []
        off = 0
        for p in params:
            self.slots.append((off, p.numel()))
            off += p.numel()
        self.pending = 0
        self.ready = False

    def attach_grads(self) -> None:
        """Point every p.grad at its slice of the flat buffer so autograd
        accumulates straight into bucket storage (no copies)."""
        for p, (off, n) in zip(self.params, self.slots):
            p.grad = self.flat[off : off + n].view_as(p)

    def reset(self) -> None:
        self.pending = len(self.params)
        self.ready = False


class _ReducerWorker:
    """Background reducer thread — the reference's architecture
    (VGG/distributed_optimizer.py:57-59, VGG/allreducer.py:549): all engine
    collectives issue from this ONE thread in bucket-completion order, so
    RCCL waits and host readbacks (size exchanges, .item() syncs) overlap
    the backward pass instead of stalling the autograd-hook thread.

    Determinism: buckets are enqueued in autograd completion order, which is
    identical on every rank for identical graphs (the same assumption DDP
    and the reference make), so collective issue order matches across ranks.
    GPU kernels from this thread go on the caller's default stream — stream
    order alone serialises them correctly against backward (the hook fires
    after the grad accumulation was enqueued).
    """

    def __init__(self, reducer: AllReducer, device: torch.device):
        self._reducer = reducer
        self._device = device
        self._q: "queue.Queue" = queue.Queue()
        self._done: "queue.Queue" = queue.Queue()
        self._exc: Optional[BaseException] = None
        self._inflight = 0
        # submit() runs on the autograd-hook thread, drain() on the main
        # thread; backward()'s join orders them in practice, but the lock
        # makes the counter safe under any interleaving
        self._lock = threading.Lock()
        self._thread = threading.Thread(
            target=self._loop, daemon=True, name="oktopk-reducer")
        self._thread.start()

    def _loop(self) -> None:
        if self._device.type == "cuda":
            torch.cuda.set_device(self._device)
        while True:
            item = self._q.get()
            if item is None:
                return
            try:
                if self._exc is None:  # after a failure, drain without work
                    if isinstance(item, list):
                        self._reducer.run_many(item)
                    else:
                        # (name, flat, grad_src[, sparse_ok]); the keyword
                        # is passed only where a bucket asks for it
                        name, flat, grad = item[:3]
                        kw = {"sparse_ok": True} if item[3:] == (True,) else {}
                        self._reducer.run(name, flat, grad_src=grad, **kw)
            except BaseException as e:  # noqa: BLE001 — repropagated in drain()
                self._exc = e
            finally:
                self._done.put(None)

    def submit(self, item) -> None:
        with self._lock:
            self._inflight += 1
        self._q.put(item)

    def drain(self) -> None:
        """Block until every submitted item finished; re-raise any engine
        exception on the caller (the reference's msg_queue2 'DONE' join,
        VGG/distributed_optimizer.py:96-105)."""
        while True:
            with self._lock:
                if self._inflight == 0:
                    break
            self._done.get()
            with self._lock:
                self._inflight -= 1
        if self._exc is not None:
            exc, self._exc = self._exc, None
            raise exc

    def stop(self) -> None:
        if self._thread.is_alive():
            self._q.put(None)
            self._thread.join(timeout=30)


class _DistributedOptimizer:
    # whether completed buckets ask the engine for the sparse hand-over
    # (AllReducer.run sparse_ok); only a step() that consumes
    # reducer.sparse_results may turn it on (FlatSGD)
    _sparse_ok = False

    def __init__(
        self,
        optimizer: torch.optim.Optimizer,
        named_parameters: Iterable[Tuple[str, torch.Tensor]],
        comm: Optional[Comm] = None,
        cfg: Optional[EngineConfig] = None,
        max_grad_norm: float = 0.0,
        momentum_correction: float = 0.0,
        overlap: Optional[bool] = None,
    ):
        self.optimizer = optimizer
        # post-reduce gradient clipping (reference clips for the LSTM recipe,
        # VGG/main_trainer.py:96-99); 0 disables
        self.max_grad_norm = max_grad_norm
        # pre-reduce momentum (reference momentum_correction,
        # VGG/distributed_optimizer.py:56,81-88: momentum accumulates on the
        # LOCAL gradient BEFORE sparsification, and the inner step must then
        # run with momentum=0).  0 disables (the reference's default too).
        self.momentum_correction = momentum_correction
        self._mc_bufs: Dict[str, torch.Tensor] = {}
        self.comm = comm or Comm(None)
        self.cfg = cfg or EngineConfig()
        self.reducer = AllReducer(self.comm, self.cfg)
        # comm is skipped while local=True (gradient accumulation,
        # reference VGG/distributed_optimizer.py:78)
        self.local = False

        named = [(n, p) for n, p in named_parameters if p.requires_grad]
        if not named:
            raise ValueError("no trainable parameters")
        device = named[0][1].device
        # bucket in REVERSE model order: backward completes last layers first,
        # so reverse order lets comm start while early layers still compute.
        rev = list(reversed(named))
        self.buckets: List[_Bucket] = []
        cur: List[Tuple[str, torch.Tensor]] = []
        cur_bytes = 0
        esize = 4
        for n, p in rev:
            cur.append((n, p))
            cur_bytes += p.numel() * esize
            if cur_bytes >= self.cfg.bucket_bytes:
                self._seal_bucket(cur, device)
                cur, cur_bytes = [], 0
        if cur:
            self._seal_bucket(cur, device)

        self._param_bucket: Dict[torch.Tensor, _Bucket] = {}
        for b in self.buckets:
            for p in b.params:
                self._param_bucket[p] = b
        self._hooks = []
        for b in self.buckets:
            b.attach_grads()
            b.reset()
        for n, p in named:
            h = p.register_post_accumulate_grad_hook(self._make_hook(p))
            self._hooks.append(h)

        # Background reducer (on by default whenever there is real
        # communication to hide; at world-1 the engine never blocks on
        # comm, so inline is cheaper).
        if overlap is None:
            overlap = self.comm.size > 1
        self._worker = (
            _ReducerWorker(self.reducer, device) if overlap else None
        )

    def _seal_bucket(self, items, device):
        name = f"bucket_{len(self.buckets)}"
        self.buckets.append(_Bucket(name, [p for _, p in items], device))

    # -- hook plumbing --------------------------------------------------
    def _make_hook(self, p: torch.Tensor):
        def hook(*_):
            if self.local:
                return
            b = self._param_bucket[p]
            b.pending -= 1
            if b.pending == 0:
                self._apply_mc(b)
                if self._worker is not None:
                    # hand the completed bucket to the reducer thread and
                    # return immediately — backward keeps running while the
                    # engine's collectives and host syncs proceed there
                    self._worker.submit(self._item(b, self._sparse_ok))
                else:
                    self._run_bucket(b, self._sparse_ok)
                b.ready = True

        return hook

    @staticmethod
    def _item(b, sparse_ok: bool):
        """Work item for the reducer thread."""
        return (b.name, b.flat, None, True) if sparse_ok else (b.name, b.flat, None)

    def _run_bucket(self, b, sparse_ok: bool) -> None:
        if sparse_ok:
            self.reducer.run(b.name, b.flat, sparse_ok=True)
        else:
            self.reducer.run(b.name, b.flat)

    # reference API surface (VGG/distributed_optimizer.py:185-201) ------
    def stop(self) -> None:
        """Stop the background reducer thread (reference stop,
        VGG/distributed_optimizer.py:185-187).  Safe to call twice; the
        optimizer falls back to inline reduces afterwards."""
        if self._worker is not None:
            self._worker.drain()
            self._worker.stop()
            self._worker = None

    def add_train_epoch(self) -> None:
        self.reducer.train_epoch += 1

    def get_current_density(self) -> float:
        return self.reducer.get_current_density()

    def _apply_mc(self, b) -> None:
        if not self.momentum_correction:
            return
        buf = self._mc_bufs.get(b.name)
        if buf is None:
            buf = self._mc_bufs[b.name] = torch.zeros_like(b.flat)
        buf.mul_(self.momentum_correction).add_(b.flat)
        b.flat.copy_(buf)

    # -- optimizer surface ----------------------------------------------
    @property
    def param_groups(self):
        return self.optimizer.param_groups

    @property
    def state(self):
        return self.optimizer.state

    def zero_grad(self, set_to_none: bool = False):
        # grads are bucket views; zero the flat storage and re-arm counters
        for b in self.buckets:
            b.flat.zero_()
            b.reset()
            b.attach_grads()

    def synchronize(self):
        """Finish this step's reduces (reference synchronize,
        VGG/distributed_optimizer.py:96-105): reduce any bucket whose hook
        set never completed — params untouched this step, or ALL buckets
        when hooks were muted (hipGraph replay, gradient-accumulation
        boundary) — then join the background reducer.  The all-buckets case
        goes through run_many so bucket i's collectives overlap bucket
        i+1's selection instead of reducing serially."""
        if self.local:
            return
        leftovers = [b for b in self.buckets if not b.ready]
        for b in leftovers:
            self._apply_mc(b)
            b.ready = True
        whole_step = len(leftovers) == len(self.buckets) and len(leftovers) > 1
        sparse_ok = self._sparse_ok
        if whole_step and sparse_ok and self.comm.size == 1:
            # run_many's pipeline always densifies, and at world 1 there is
            # no communication for it to overlap: reduce serially and keep
            # the sparse hand-over
            whole_step = False
        if self._worker is not None:
            if whole_step:
                self._worker.submit([(b.name, b.flat, None) for b in leftovers])
            else:
                for b in leftovers:
                    self._worker.submit(self._item(b, sparse_ok))
            self._worker.drain()
        elif whole_step:
            self.reducer.run_many([(b.name, b.flat, None) for b in leftovers])
        else:
            for b in leftovers:
                self._run_bucket(b, sparse_ok)

    def step(self, closure=None):
        if not self.local:
            self.synchronize()
        if self.max_grad_norm and self.max_grad_norm > 0:
            # global-norm clip with NO host sync: fp64 sumsq accumulates
            # across buckets on device, the scale is a device scalar and
            # the bucket multiplies broadcast it (reference clips host-
            # side per step, VGG/main_trainer.py:96-99)
            dev = self.buckets[0].flat.device
            acc = torch.zeros(1, dtype=torch.float64, device=dev)
            for b in self.buckets:
                ops.sumsq_into_(acc, b.flat)
            gn = acc.sqrt().to(torch.float32)
            mx = self.max_grad_norm
            scale = torch.where(gn > mx, mx / (gn + 1e-6),
                                torch.ones_like(gn))
            for b in self.buckets:
                b.flat.mul_(scale)
        out = self.optimizer.step(closure)
        return out

    def state_dict(self):
        return {
            "optimizer": self.optimizer.state_dict(),
            "reducer": {
                name: st.state_dict() for name, st in self.reducer.states.items()
            },
        }

    def load_state_dict(self, d):
        self.optimizer.load_state_dict(d["optimizer"])
        self._load_reducer_states(d)

    def _load_reducer_states(self, d):
        for name, st_d in d.get("reducer", {}).items():
            if name in self.reducer.states:
                self.reducer.states[name].load_state_dict(st_d)
            else:
                # rebuild on the bucket device (checkpoint may be CPU-mapped)
                from .allreducer import TensorState

                dev = self.buckets[0].flat.device if self.buckets else st_d["residual"].device
                st = TensorState(residual=st_d["residual"].clone().to(dev))
                st.load_state_dict(st_d)
                self.reducer.states[name] = st


def DistributedOptimizer(
    optimizer: torch.optim.Optimizer,
    named_parameters: Iterable[Tuple[str, torch.Tensor]],
    comm: Optional[Comm] = None,
    cfg: Optional[EngineConfig] = None,
    compression: Optional[str] = None,
    is_sparse: Optional[bool] = None,
    density: Optional[float] = None,
    norm_clip: Optional[float] = None,
    momentum_correction: float = 0.0,
    overlap: Optional[bool] = None,
    **_ignored,
) -> _DistributedOptimizer:
    """Factory with the reference's calling convention
    (VGG/distributed_optimizer.py:203: DistributedOptimizer(optimizer,
    named_parameters, compression, is_sparse, density, ...)).
    `overlap` forces the background reducer thread on/off (default: on
    when world size > 1)."""
    cfg = cfg or EngineConfig()
    if compression is not None:
        cfg.compressor = compression
    if is_sparse is False:
        cfg.compressor = "dense"
    if density is not None:
        cfg.density = density
    return _DistributedOptimizer(optimizer, named_parameters, comm, cfg,
                                 max_grad_norm=norm_clip or 0.0,
                                 momentum_correction=momentum_correction,
                                 overlap=overlap)


class FlatSGD(_DistributedOptimizer):
    """SGD (momentum / nesterov / weight decay, no dampening) over flat
    per-bucket storage, with no inner torch optimizer.

    Buckets, hooks, the reducer thread, `local`, synchronize(), stop() and
    add_train_epoch() are _DistributedOptimizer's.  Each bucket also owns a
    flat fp32 copy of its parameters (every p.data is aliased into it, as
    FlatBertAdam does) and a flat momentum buffer, so the step is ONE fused
    launch per bucket (ops.sgd_step_) instead of torch's multi-tensor SGD
    over every parameter tensor.

    Buckets are reduced with sparse_ok=True (OKTOPK_SPARSE_STEP=0 turns it
    off): where the engine hands a bucket's result over as a SparseGrad,
    the clip sum and the step (ops.sgd_step_sparse_) consume the selection
    directly — no zero fill, no scatter, no dense norm read, no gradient
    read; same bits.  One step may mix sparse and dense buckets.  The
    all-buckets drain (graph replay, accumulation boundary) keeps the
    hand-over at world 1 only: at world > 1 it goes through run_many,
    whose pipeline densifies.

    `param_groups` is one persistent group read at every step, so
    `g["lr"] = ...` from Trainer.adjust_learning_rate or an external
    scheduler takes effect on the next step."""

    def __init__(
        self,
        named_parameters: Iterable[Tuple[str, torch.Tensor]],
        comm: Optional[Comm] = None,
        cfg: Optional[EngineConfig] = None,
        lr: float = 0.1,
        momentum: float = 0.9,
        weight_decay: float = 0.0,
        nesterov: bool = False,
        max_grad_norm: float = 0.0,
        momentum_correction: float = 0.0,
        overlap: Optional[bool] = None,
    ):
        named = [(n, p) for n, p in named_parameters if p.requires_grad]
        # checked before anything is allocated or aliased, so a caller can
        # fall back to the torch route with the model untouched
        for n, p in named:
            if p.dtype != torch.float32:
                raise ValueError(
                    f"FlatSGD needs fp32 parameters; {n} is {p.dtype}")
            if not p.is_contiguous():
                raise ValueError(
                    f"FlatSGD needs contiguous parameters; {n} is not")
        super().__init__(None, named, comm, cfg, max_grad_norm=max_grad_norm,
                         momentum_correction=momentum_correction,
                         overlap=overlap)
        for b in self.buckets:
            b.flat_param = torch.empty_like(b.flat)
            b.momentum_buf = torch.zeros_like(b.flat)
            for p, (off, n_) in zip(b.params, b.slots):
                b.flat_param[off : off + n_].copy_(p.data.view(-1))
                # the module keeps its Parameter objects; .data becomes a view
                p.data = b.flat_param[off : off + n_].view_as(p)
        self._groups = [{
            "lr": float(lr), "momentum": float(momentum),
            "weight_decay": float(weight_decay), "nesterov": bool(nesterov),
            "params": [p for _, p in named],
        }]
        # buckets x steps that took the sparse route, and the last step's
        # clip factor (1-elem device tensor, None without clipping)
        self.sparse_bucket_steps = 0
        self.last_clip_scale: Optional[torch.Tensor] = None

    @property
    def _sparse_ok(self) -> bool:
        return os.environ.get("OKTOPK_SPARSE_STEP", "1") != "0"

    @property
    def param_groups(self):
        return self._groups

    @property
    def state(self):
        return {b.name: {"flat_param": b.flat_param,
                         "momentum_buffer": b.momentum_buf}
                for b in self.buckets}

    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FlatSGD.step takes no closure")
        if not self.local:
            self.synchronize()
        g = self._groups[0]
        lr, mom, wd, nesterov = (g["lr"], g["momentum"], g["weight_decay"],
                                 g["nesterov"])
        # each hand-over is consumed once: a step without a reduce (local)
        # must not see the previous step's selection
        res = self.reducer.sparse_results
        sgs = [res.pop(b.name, None) for b in self.buckets]
        if self.local:
            sgs = [None] * len(sgs)
        gscale = None
        if self.max_grad_norm and self.max_grad_norm > 0:
            # global-norm clip, device-resident: one fp64 sum of squares
            # across buckets (over the ~k entries for a sparse bucket), the
            # factor stays on the device and scales the step's gradient
            # read — no multiply pass, no host sync
            dev = self.buckets[0].flat.device
            acc = torch.zeros(1, dtype=torch.float64, device=dev)
            for b, sg in zip(self.buckets, sgs):
                if sg is not None:
                    ops.sparse_sumsq_into_(acc, sg.idx, sg.val, sg.scale,
                                           sg.tau, n=b.numel)
                else:
                    ops.sumsq_into_(acc, b.flat)
            gscale = ops.clip_scale_from_sumsq(acc, self.max_grad_norm)
        self.last_clip_scale = gscale
        for b, sg in zip(self.buckets, sgs):
            if sg is not None:
                ops.sgd_step_sparse_(b.flat_param, sg.idx, sg.val, 0, sg.scale,
                                     sg.tau, b.momentum_buf, lr, mom, wd,
                                     nesterov, gscale=gscale)
                self.sparse_bucket_steps += 1
            else:
                ops.sgd_step_(b.flat_param, b.flat, b.momentum_buf, lr, mom,
                              wd, nesterov, gscale=gscale)

    def state_dict(self):
        g = self._groups[0]
        return {
            "param_group": {k: g[k] for k in
                            ("lr", "momentum", "weight_decay", "nesterov")},
            "buckets": {b.name: {"flat_param": b.flat_param,
                                 "momentum_buf": b.momentum_buf}
                        for b in self.buckets},
            "reducer": {
                name: st.state_dict() for name, st in self.reducer.states.items()
            },
        }

    def load_state_dict(self, d):
        self._groups[0].update(d["param_group"])
        for b in self.buckets:
            sd = d["buckets"][b.name]
            if sd["flat_param"].numel() != b.numel:
                raise ValueError(f"{b.name}: checkpoint has "
                                 f"{sd['flat_param'].numel()} elements, the "
                                 f"model {b.numel}")
            # copy_ crosses devices (a checkpoint may be mapped elsewhere)
            b.flat_param.copy_(sd["flat_param"])
            b.momentum_buf.copy_(sd["momentum_buf"])
        self._load_reducer_states(d)


class FlatBertAdam:
    """BertAdam over one flat gradient (reference optimization.py:135-224):
    flatten -> engine.run -> fused Adam per param with warmup-scheduled lr,
    optional grad clipping, decoupled weight decay."""

    def __init__(
        self,
        named_parameters: Iterable[Tuple[str, torch.Tensor]],
        comm: Optional[Comm] = None,
        cfg: Optional[EngineConfig] = None,
        lr: float = 2e-4,
        warmup: float = -1.0,
        t_total: int = -1,
        schedule: str = "warmup_linear",
        betas: Tuple[float, float] = (0.9, 0.999),
        eps: float = 1e-6,
        weight_decay: float = 0.01,
        max_grad_norm: float = 1.0,
        no_decay_keys: Tuple[str, ...] = ("bias", "ln", "layernorm", "layer_norm"),
    ):
        self.comm = comm or Comm(None)
        self.cfg = cfg or EngineConfig.preset("bert")
        self.reducer = AllReducer(self.comm, self.cfg)
        named = [(n, p) for n, p in named_parameters if p.requires_grad]
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        self.lr = lr
        self.warmup = warmup
        self.t_total = t_total
        self.schedule = SCHEDULES[schedule]
        self.betas = betas
        self.eps = eps
        self.weight_decay = weight_decay
        self.max_grad_norm = max_grad_norm
        self.step_count = 0
        device = self.params[0].device
        self.numel = sum(p.numel() for p in self.params)

        # Fully-flat layout: params are reordered [decay group | no-decay
        # group] so the Adam step is TWO fused kernel launches over
        # contiguous slices instead of one launch per parameter (the
        # reference pays a python loop over ~200 params,
        # optimization.py:170-224, plus a torch.cat of 109.5M floats per
        # step at :160-163 — here both gather and update are zero-copy).
        def _decays(n: str) -> bool:
            low = n.lower()
            return not any(k in low for k in no_decay_keys)

        order = sorted(range(len(named)), key=lambda i: 0 if _decays(named[i][0]) else 1)
        self.names = [named[i][0] for i in order]
        self.params = [named[i][1] for i in order]
        self.decay_numel = sum(
            named[i][1].numel() for i in order if _decays(named[i][0])
        )
        self._decay_count = sum(1 for i in order if _decays(named[i][0]))
        # pad the group boundary to 8 elements so BOTH fused-Adam launches
        # see 16-byte-aligned float4 (and 8-byte short4 mirror) slices; the
        # pad region has zero grad/state and never moves
        pad = (-self.decay_numel) % 8
        self.decay_numel += pad
        self.numel += pad
        # Mixed precision: when the model runs in pure bf16 (no autocast —
        # the per-layer weight-cast kernels of autocast were ~1000 extra
        # launches/step on BERT-base, measured in profiles/), keep fp32
        # MASTER weights + Adam state here and mirror to the bf16 model
        # copy with one bulk cast per step.
        self.model_dtype = self.params[0].dtype
        self.flat_grad = torch.zeros(self.numel, dtype=torch.float32, device=device)
        self.flat_param = torch.zeros_like(self.flat_grad)
        self.exp_avg = torch.zeros_like(self.flat_grad)
        self.exp_avg_sq = torch.zeros_like(self.flat_grad)
        if self.model_dtype != torch.float32:
            self.flat_param_model = torch.zeros(self.numel, dtype=self.model_dtype, device=device)
            self.flat_grad_model = torch.zeros(self.numel, dtype=self.model_dtype, device=device)
        else:
            self.flat_param_model = self.flat_param
            self.flat_grad_model = self.flat_grad
        self.slots = []
        off = 0
        for j, p in enumerate(self.params):
            if j == self._decay_count:
                off = self.decay_numel  # skip the alignment pad
            n_ = p.numel()
            self.slots.append((off, n_))
            self.flat_param[off : off + n_].copy_(p.data.view(-1).float())
            # alias param storage into the flat model-dtype buffer (module
            # keeps the same Parameter objects; their .data becomes a view)
            p.data = self.flat_param_model[off : off + n_].view_as(p)
            off += n_
        if self.model_dtype != torch.float32:
            self.flat_param_model.copy_(self.flat_param)
        for p, (o, n_) in zip(self.params, self.slots):
            p.grad = self.flat_grad_model[o : o + n_].view_as(p)
        self._bind_direct_grad()

    # -- direct gradient slots -------------------------------------------
    # A bound parameter's backward node (ops/fused_linear.py) writes the
    # gradient into its slot instead of returning it, so the slot needs no
    # zeroing and autograd runs no `slot += g` kernel for it.
    #
    # OWNERSHIP RULE: a slot is owned only if the module using the parameter
    # runs in EVERY backward of the model — an owned slot is never zeroed,
    # so a backward that skips its module would leave the previous step's
    # gradient in it.  The model states that with mark_every_backward(); this
    # optimizer binds only marked parameters, only on the bf16 GPU path, and
    # only with OKTOPK_DIRECT_GRAD != 0.  As a guard the nodes record what
    # they wrote: a parameter that an eager backward left unwritten (say the
    # NSP head in a run without NSP labels) is zeroed, unbound and returned
    # to the zero + accumulate path before its gradient is used.
    _ZERO_MERGE_GAP = 1 << 16  # elements; see _plan_zero_ranges

    def _bind_direct_grad(self) -> None:
        from .ops.fused_linear import (GradSlotOwner, bind_grad_slot,
                                       direct_grad_enabled, runs_every_backward)

        self._dg_owner = None
        self._dg_params: List[torch.Tensor] = []
        self._zero_ranges: Optional[List[Tuple[int, int]]] = None
        if not (direct_grad_enabled() and self.model_dtype == torch.bfloat16
                and self.flat_grad_model.is_cuda):
            return
        owner = GradSlotOwner()
        for p in self.params:
            if runs_every_backward(p):
                bind_grad_slot(p, p.grad, owner)
                self._dg_params.append(p)
        if self._dg_params:
            self._dg_owner = owner
            self._plan_zero_ranges()

    def _plan_zero_ranges(self) -> None:
        """Ranges of the flat buffer zero_grad() must fill: everything no
        bound parameter owns (unrouted parameters, the alignment pad).
        Neighbouring ranges separated by less than _ZERO_MERGE_GAP owned
        elements are merged into one fill — zeroing an owned slot is
        harmless (its node overwrites it) and a 128 KB fill is cheaper than
        a second launch — which leaves BERT with two fills: the position +
        token-type embeddings, and the bias/LayerNorm tail."""
        bound = {id(p) for p in self._dg_params}
        owned = sorted((o, o + n_) for p, (o, n_) in zip(self.params, self.slots)
                       if id(p) in bound)
        free, cur = [], 0
        for a, b in owned:
            if a > cur:
                free.append([cur, a])
            cur = max(cur, b)
        if cur < self.numel:
            free.append([cur, self.numel])
        merged: List[List[int]] = []
        for a, b in free:
            if merged and a - merged[-1][1] < self._ZERO_MERGE_GAP:
                merged[-1][1] = b
            else:
                merged.append([a, b])
        self._zero_ranges = [(a, b) for a, b in merged]

    def _settle_direct_grad(self) -> None:
        """After an eager backward: any bound slot it did not write holds a
        stale gradient — zero it and give the parameter back to the zero +
        accumulate path.  Graph replays record nothing and skip this (the
        captured backward is the one checked before capture)."""
        owner = self._dg_owner
        if owner is None or not owner.written:
            return
        from .ops.fused_linear import unbind_grad_slot

        missing = [p for p in self._dg_params if id(p) not in owner.written]
        owner.written.clear()
        if missing:
            gone = {id(p) for p in missing}
            for p, (o, n_) in zip(self.params, self.slots):
                if id(p) in gone:
                    self.flat_grad_model[o : o + n_].zero_()
                    unbind_grad_slot(p)
            self._dg_params = [p for p in self._dg_params if id(p) not in gone]
            self._plan_zero_ranges()

    def set_substep(self, sub: int) -> None:
        """Gradient-accumulation protocol (Trainer.step): sub-step 0 starts
        a fresh accumulation, so every bound slot's next write overwrites;
        in later sub-steps the nodes accumulate into what is there."""
        if sub == 0 and self._dg_owner is not None:
            self._settle_direct_grad()
            self._dg_owner.written.clear()

    def zero_grad(self, set_to_none: bool = False):
        self._settle_direct_grad()
        if self._zero_ranges is None:
            self.flat_grad_model.zero_()
        else:
            for a, b in self._zero_ranges:
                self.flat_grad_model[a:b].zero_()
        for p, (o, n_) in zip(self.params, self.slots):
            p.grad = self.flat_grad_model[o : o + n_].view_as(p)

    @property
    def param_groups(self):
        """Minimal torch-optimizer-surface shim (LR tooling interop)."""
        return [{"lr": self.lr, "params": self.params}]

    def current_lr(self) -> float:
        if self.t_total > 0:
            return self.lr * self.schedule(self.step_count / self.t_total, self.warmup)
        return self.lr

    def get_lr(self) -> list:
        """Reference BertAdam.get_lr surface (optimization.py:120-133):
        one scheduled lr per param group — here one flat group."""
        if self.step_count == 0:
            return [0]
        return [self.current_lr()]

    def step(self):
        self._settle_direct_grad()
        # 1. sparse allreduce of the whole flat gradient.  The engine may
        # hand the result over in sparse form (AllReducer.run sparse_ok):
        # flat_grad is then left unwritten and clip + Adam below consume the
        # ~k selected entries directly — same bits, three tensor-scale
        # passes less.  OKTOPK_SPARSE_STEP=0 keeps the dense hand-over.
        sparse_ok = os.environ.get("OKTOPK_SPARSE_STEP", "1") != "0"
        self.reducer.sparse_result = None
        if self.cfg.compressor in ("dense", "none") and self.model_dtype != torch.float32:
            # dense baseline: allreduce the bf16 grads directly (half wire
            # volume — the right dense baseline on MI355X), then upcast
            self.reducer.run("flat", self.flat_grad_model)
            self.flat_grad.copy_(self.flat_grad_model)
        elif self.flat_grad_model is not self.flat_grad:
            # bf16 grads: the upcast is fused into the engine's EF restore
            self.reducer.run("flat", self.flat_grad, grad_src=self.flat_grad_model,
                             sparse_ok=sparse_ok)
        else:
            self.reducer.run("flat", self.flat_grad, sparse_ok=sparse_ok)
        sg = self.reducer.sparse_result
        # 2. grad clip on the reduced gradient (reference optimization.py:197)
        # — device-resident: the clip factor stays on GPU and is applied by
        # the Adam kernel's gradient read (no host sync, no extra full-
        # tensor mul pass)
        gscale = None
        if self.max_grad_norm and self.max_grad_norm > 0:
            if sg is not None:
                gscale = ops.grad_clip_scale_sparse(
                    sg.idx, sg.val, sg.scale, sg.tau, self.max_grad_norm,
                    self.numel)
            else:
                gscale = ops.grad_clip_scale(self.flat_grad, self.max_grad_norm)
        # 3. fused Adam: one launch per weight-decay group (2 total); on
        # the bf16 path the model-weight mirror is written BY the Adam
        # kernel (saves a separate 660 MB cast pass)
        lr = self.current_lr()
        b1, b2 = self.betas
        d = self.decay_numel
        mirrored = self.flat_param_model is not self.flat_param
        def _adam(sl, wd):
            if sg is not None:
                # `base`: the slice's offset in the flat layout; entries of
                # the selection outside the slice are ignored by the op
                base = sl.start or 0
                if mirrored:
                    ops.fused_adam_sparse_mirror_(
                        self.flat_param[sl], sg.idx, sg.val, base, sg.scale,
                        sg.tau, self.exp_avg[sl], self.exp_avg_sq[sl],
                        self.flat_param_model[sl], lr, b1, b2, self.eps, wd,
                        gscale=gscale,
                    )
                else:
                    ops.fused_adam_sparse_(
                        self.flat_param[sl], sg.idx, sg.val, base, sg.scale,
                        sg.tau, self.exp_avg[sl], self.exp_avg_sq[sl], lr, b1,
                        b2, self.eps, wd, gscale=gscale,
                    )
            elif mirrored:
                ops.fused_adam_mirror_(
                    self.flat_param[sl], self.flat_grad[sl], self.exp_avg[sl],
                    self.exp_avg_sq[sl], self.flat_param_model[sl], lr, b1, b2,
                    self.eps, wd, gscale=gscale,
                )
            else:
                ops.fused_adam_(
                    self.flat_param[sl], self.flat_grad[sl], self.exp_avg[sl],
                    self.exp_avg_sq[sl], lr, b1, b2, self.eps, wd,
                    gscale=gscale,
                )
        if d > 0:
            _adam(slice(None, d), self.weight_decay)
        if d < self.numel:
            _adam(slice(d, None), 0.0)
        self.step_count += 1

    def sync_master_from_model(self) -> None:
        """Re-derive the fp32 master weights from the (model-dtype) module
        params — required after loading a model state_dict WITHOUT optimizer
        state, else the next step would overwrite the loaded weights with
        updates of the stale master."""
        if self.flat_param_model is not self.flat_param:
            self.flat_param.copy_(self.flat_param_model)

    def state_dict(self):
        return {
            "step_count": self.step_count,
            # fp32 master weights: the model state_dict only carries the
            # model-dtype (bf16) mirrors
            "flat_param": self.flat_param,
            "exp_avg": self.exp_avg,
            "exp_avg_sq": self.exp_avg_sq,
            "reducer": {n: s.state_dict() for n, s in self.reducer.states.items()},
        }

    def load_state_dict(self, d):
        self.step_count = int(d["step_count"])
        if "flat_param" in d:
            self.flat_param.copy_(d["flat_param"])
            if self.flat_param_model is not self.flat_param:
                self.flat_param_model.copy_(self.flat_param)
        else:
            self.sync_master_from_model()
        self.exp_avg.copy_(d["exp_avg"])
        self.exp_avg_sq.copy_(d["exp_avg_sq"])
        for name, st_d in d.get("reducer", {}).items():
            from .allreducer import TensorState

            st = self.reducer.states.get(name)
            if st is None:
                # checkpoint tensors may be on CPU (map_location): place the
                # restored state on the optimizer's device
                dev = self.flat_grad.device
                st = TensorState(residual=st_d["residual"].clone().to(dev))
                self.reducer.states[name] = st
            st.load_state_dict(st_d)
