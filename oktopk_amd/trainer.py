"""Training driver with synthetic data (bench + smoke path).

Capability parity with the reference trainers (VGG/dl_trainer.py DLTrainer,
BERT/bert/main_bert.py): model build, fwd/bwd, distributed optimizer, LR
schedule hooks, per-phase timing.  Real-dataset loaders are out of scope for
the benchmark contract (no network): batches are synthetic with the exact
shapes of the reference configs.
"""
from __future__ import annotations

import logging
import os
from typing import Optional

import torch

from . import models
from .comm import Comm
from .config import EngineConfig
from .optimizer import DistributedOptimizer, FlatBertAdam, FlatSGD

logger = logging.getLogger("oktopk_amd")


_CIFAR = {"vgg11", "vgg13", "vgg16", "vgg19", "resnet20", "resnet32", "resnet44",
          "resnet56", "resnet110", "preresnet20", "preresnet32", "preresnet44",
          "preresnet56", "preresnet110", "resnet_mod20", "resnet_mod32",
          "resnet_mod44", "resnet_mod56", "resnet_mod110", "alexnet",
          "caffe_cifar", "densenet", "resnext"}
_IMAGENET = {"resnet18", "resnet34", "resnet50", "resnet101", "resnet152"}


def model_family(name: str) -> str:
    if name in _CIFAR:
        return "cifar"
    if name in _IMAGENET:
        return "imagenet"
    if name == "mnistnet":
        return "mnist"
    if name == "lstm":
        return "ptb"
    if name == "lstman4":
        return "an4"
    if name.startswith("bert"):
        return "bert"
    raise ValueError(name)


class SyntheticBatches:
    """Deterministic per-rank synthetic batches with reference shapes."""

    def __init__(self, model_name: str, batch_size: int, device, seq_len: int = 128,
                 rank: int = 0, vocab_size: int = 30522):
        self.model_name = model_name
        self.bs = batch_size
        self.device = device
        self.seq_len = seq_len
        self.vocab = vocab_size
        g = torch.Generator().manual_seed(1234 + rank)
        self.family = model_family(model_name)
        if self.family == "cifar":
            # CIFAR-10 shape, bs 16/rank in the reference (vgg16_oktopk.sh)
            self.x = torch.randn(batch_size, 3, 32, 32, generator=g)
            self.y = torch.randint(0, 10, (batch_size,), generator=g)
        elif self.family == "imagenet":
            self.x = torch.randn(batch_size, 3, 224, 224, generator=g)
            self.y = torch.randint(0, 1000, (batch_size,), generator=g)
        elif self.family == "mnist":
            self.x = torch.randn(batch_size, 1, 28, 28, generator=g)
            self.y = torch.randint(0, 10, (batch_size,), generator=g)
        elif self.family == "ptb":
            # PTB word-LM: (seq, batch) int tokens + shifted targets
            self.tokens = torch.randint(0, 10000, (35, batch_size), generator=g)
            self.targets = torch.randint(0, 10000, (35, batch_size), generator=g)
        elif model_name == "lstman4":
            # AN4 spectrograms: (N, 1, freq=161, time~200), bs 2/rank
            self.x = torch.randn(batch_size, 1, 161, 201, generator=g)
            t_out = 101  # conv time stride 2 once
            self.target = torch.randint(1, 29, (batch_size, 20), generator=g)
            self.in_len = torch.full((batch_size,), t_out, dtype=torch.int32)
            self.tgt_len = torch.full((batch_size,), 20, dtype=torch.int32)
        elif model_name.startswith("bert"):
            # seq 128, bs 8/rank (bert_oktopk.sh)
            self.input_ids = torch.randint(0, vocab_size, (batch_size, seq_len), generator=g)
            self.token_type = torch.randint(0, 2, (batch_size, seq_len), generator=g)
            self.attn = torch.ones(batch_size, seq_len, dtype=torch.long)
            labels = torch.full((batch_size, seq_len), -1, dtype=torch.long)
            mask_pos = torch.rand(batch_size, seq_len, generator=g) < 0.15
            labels[mask_pos] = torch.randint(0, vocab_size, (int(mask_pos.sum()),), generator=g)
            self.mlm_labels = labels
            self.nsp = torch.randint(0, 2, (batch_size,), generator=g)
        else:
            raise ValueError(model_name)
        for k, v in list(self.__dict__.items()):
            if isinstance(v, torch.Tensor):
                setattr(self, k, v.to(device))
        self._roll = 0

    def randomize_(self) -> None:
        """Re-roll batch CONTENT in place (buffers keep identity, so a
        captured hipGraph that reads them stays valid)."""
        self._roll += 1
        g = torch.Generator().manual_seed(99991 * self._roll + 7)
        if self.family in ("cifar", "imagenet", "mnist"):
            self.x.copy_(torch.randn(self.x.shape, generator=g).to(self.x.device))
            self.y.copy_(torch.randint(0, int(self.y.max().clamp(min=9)) + 1,
                                       self.y.shape, generator=g).to(self.y.device))
        elif self.family == "ptb":
            self.tokens.copy_(torch.randint(0, 10000, self.tokens.shape, generator=g).to(self.tokens.device))
            self.targets.copy_(torch.randint(0, 10000, self.targets.shape, generator=g).to(self.targets.device))
        elif self.family == "an4":
            self.x.copy_(torch.randn(self.x.shape, generator=g).to(self.x.device))
        elif self.family == "bert":
            dev = self.input_ids.device
            self.input_ids.copy_(torch.randint(0, self.vocab, self.input_ids.shape, generator=g).to(dev))
            labels = torch.full(self.mlm_labels.shape, -1, dtype=torch.long)
            mask_pos = torch.rand(*self.mlm_labels.shape, generator=g) < 0.15
            labels[mask_pos] = torch.randint(0, self.vocab, (int(mask_pos.sum()),), generator=g)
            self.mlm_labels.copy_(labels.to(dev))
            self.nsp.copy_(torch.randint(0, 2, self.nsp.shape, generator=g).to(dev))


class Trainer:
    def __init__(
        self,
        model_name: str = "bert_base",
        batch_size: int = 8,
        seq_len: int = 128,
        device: Optional[torch.device] = None,
        comm: Optional[Comm] = None,
        cfg: Optional[EngineConfig] = None,
        optimizer: str = "auto",  # auto | sgd | adam | flat_sgd
        lr: float = None,
        dtype: str = "bf16",
        nsteps_update: int = 1,
        model_kwargs: Optional[dict] = None,
    ):
        self.comm = comm or Comm(None)
        self.device = device or (
            torch.device("cuda", torch.cuda.current_device())
            if torch.cuda.is_available()
            else torch.device("cpu")
        )
        self.model_name = model_name
        if not model_name.startswith("bert"):
            # conv/RNN recipes dispatch through MIOpen: the full find mode
            # picks measurably better solvers (vgg16 2.69 -> 2.51 ms/step,
            # profiles/README.md r02-q); search cost amortizes in warmup
            import os as _os

            _os.environ.setdefault("MIOPEN_FIND_MODE", "1")
        self.cfg = cfg or EngineConfig.preset(
            "bert" if model_name.startswith("bert") else
            ("lstm" if model_name.startswith("lstm") else "vgg")
        )
        # BERT runs in PURE bf16 with fp32 master weights in FlatBertAdam
        # (autocast's per-layer weight casts are ~1000 extra kernel launches
        # per step — measured in profiles/); conv/LSTM recipes use autocast.
        self.pure_bf16 = (
            dtype == "bf16" and self.device.type == "cuda" and model_name.startswith("bert")
        )
        # MIOpen's fused RNN path has no bf16 kernels: under autocast the
        # LSTM falls back to the unfused cell loop (105 vs 27 ms/step
        # measured on lstman4) — run the RNN recipes in fp32
        self.autocast = (
            dtype == "bf16" and self.device.type == "cuda"
            and not self.pure_bf16 and not model_name.startswith("lstm")
        )
        self.nsteps_update = max(1, nsteps_update)

        if self.device.type == "cuda":
            # static shapes throughout: let MIOpen find fast conv algos
            torch.backends.cudnn.benchmark = True
        self.model = models.create_net(model_name, **(model_kwargs or {})).to(self.device)
        # opt-in NHWC for conv recipes (MIOpen layout A/B; hurts nothing else)
        self.channels_last = (
            os.environ.get("OKTOPK_CHANNELS_LAST", "0") == "1"
            and self.device.type == "cuda"
        )
        if self.channels_last:
            self.model = self.model.to(memory_format=torch.channels_last)
        # broadcast initial weights (reference comm.bcast(state_dict),
        # VGG/main_trainer.py:52)
        if self.comm.size > 1:
            for p in self.model.parameters():
                self.comm.broadcast_(p.data, src=0)
        if self.pure_bf16:
            self.model = self.model.to(torch.bfloat16)

        if optimizer == "auto":
            optimizer = "adam" if model_name.startswith("bert") else "sgd"
        if optimizer == "sgd" and os.environ.get("OKTOPK_FLAT_SGD", "0") == "1":
            optimizer = "flat_sgd"
        if optimizer == "flat_sgd":
            # same hyper-parameters as the torch route below
            try:
                self.opt = FlatSGD(
                    self.model.named_parameters(), comm=self.comm, cfg=self.cfg,
                    lr=lr or 0.1, momentum=0.9, weight_decay=5e-4,
                )
            except ValueError as e:
                logger.warning("flat_sgd unavailable (%s); using torch SGD "
                               "under DistributedOptimizer", e)
                optimizer = "sgd"
        self.opt_kind = optimizer
        if optimizer == "flat_sgd":
            pass
        elif optimizer == "adam":
            self.opt = FlatBertAdam(
                self.model.named_parameters(),
                comm=self.comm,
                cfg=self.cfg,
                lr=lr or 2e-4,
            )
        else:
            inner = torch.optim.SGD(
                self.model.parameters(), lr=lr or 0.1, momentum=0.9, weight_decay=5e-4
            )
            self.opt = DistributedOptimizer(
                inner, self.model.named_parameters(), comm=self.comm, cfg=self.cfg
            )

        self.batches = SyntheticBatches(
            model_name, batch_size, self.device, seq_len=seq_len, rank=self.comm.rank
        )
        if self.channels_last and getattr(self.batches, "x", None) is not None \
                and self.batches.x.dim() == 4:
            self.batches.x = self.batches.x.contiguous(
                memory_format=torch.channels_last)
        self.iteration = 0
        self.last_loss = 0.0
        # hipGraph capture of fwd+bwd (the step is launch-bound at small
        # per-GPU batches — measured in profiles/): grads accumulate into
        # the optimizer's flat views, so one graph replays the whole
        # fwd+bwd; the sparse engine (data-dependent sizes + RCCL) stays
        # outside the graph.
        self._graph = None
        self._graph_loss = None

    # ------------------------------------------------------------------
    def _forward_loss(self) -> torch.Tensor:
        b = self.batches
        if b.family in ("cifar", "imagenet", "mnist"):
            out = self.model(b.x)
            return torch.nn.functional.cross_entropy(out, b.y)
        if b.family == "ptb":
            logits, _ = self.model(b.tokens)
            return torch.nn.functional.cross_entropy(
                logits.view(-1, logits.size(-1)).float(), b.targets.view(-1)
            )
        if self.model_name == "lstman4":
            logits = self.model(b.x)  # (T, N, C)
            logp = torch.nn.functional.log_softmax(logits, dim=-1)
            t = logp.size(0)
            in_len = torch.clamp(b.in_len, max=t)
            return torch.nn.functional.ctc_loss(
                logp.float(), b.target, in_len, b.tgt_len, blank=0, zero_infinity=True
            )
        return self.model(
            b.input_ids,
            token_type_ids=b.token_type,
            attention_mask=b.attn,
            masked_lm_labels=b.mlm_labels,
            next_sentence_label=b.nsp,
        )

    def update_nworker(self, new_comm) -> None:
        """Continue training in a shrunken world (reference
        DLTrainer.update_nworker, VGG/dl_trainer.py:472-493: rebuilds the
        DistributedSampler; here the per-rank synthetic shard is re-seeded
        and the engine communicator swapped)."""
        self.comm = new_comm
        if hasattr(self.opt, "reducer"):
            self.opt.reducer.set_comm(new_comm)
        if hasattr(self.opt, "comm"):
            self.opt.comm = new_comm
        self.batches = SyntheticBatches(
            self.model_name, self.batches.bs, self.device,
            seq_len=self.batches.seq_len, rank=new_comm.rank,
        )

    def capture_graph(self) -> bool:
        """Capture fwd+bwd into a hipGraph (call after a few eager warmup
        steps).  Returns False (and stays eager) when the model is not
        capturable (e.g. CTC loss) or no GPU is present."""
        if self.device.type != "cuda" or self.nsteps_update != 1:
            return False
        if getattr(self.opt, "local", False):
            return False
        # hook-driven optimizers: capture with hooks muted (local=True, the
        # hooks are python callbacks and never fire during graph REPLAY
        # anyway); bucket reduces then run post-replay from synchronize()
        from .optimizer import _DistributedOptimizer

        hook_driven = isinstance(self.opt, _DistributedOptimizer)
        try:
            if hook_driven:
                self.opt.local = True
            torch.cuda.synchronize()
            self.opt.zero_grad()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):  # warm up allocator on the side stream
                    self.opt.zero_grad()
                    loss = self._forward_loss()
                    loss.backward()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.opt.zero_grad()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                loss = self._forward_loss()
                loss.backward()
            self._graph = g
            self._graph_loss = loss
            return True
        except Exception:
            self._graph = None
            self._graph_loss = None
            return False
        finally:
            if hook_driven:
                self.opt.local = False

    def memory_stats(self) -> dict:
        """GPU memory snapshot in MiB (reference DLTrainer's GPU-mem
        profiling, VGG/dl_trainer.py — logged per epoch under --profiling).
        Zeros on CPU."""
        if self.device.type != "cuda":
            return {"allocated_mib": 0.0, "max_allocated_mib": 0.0,
                    "reserved_mib": 0.0}
        mib = 1024 * 1024
        return {
            "allocated_mib": round(torch.cuda.memory_allocated() / mib, 1),
            "max_allocated_mib": round(torch.cuda.max_memory_allocated() / mib, 1),
            "reserved_mib": round(torch.cuda.memory_reserved() / mib, 1),
        }

    def set_epoch(self, epoch: int) -> None:
        """Advance the engine's dynamic density schedule (reference
        train_epoch plumbing, VGG/allreducer.py:207-208) and apply the LR
        schedule."""
        red = getattr(self.opt, "reducer", None)
        if red is not None:
            red.train_epoch = epoch
        self.adjust_learning_rate(epoch)

    def adjust_learning_rate(self, epoch: int) -> None:
        """Step-decay LR schedules for the SGD recipes (reference
        _adjust_learning_rate_general, VGG/dl_trainer.py:507-570: x0.1 at
        the milestone epochs of each workload)."""
        groups = getattr(self.opt, "param_groups", None)
        if not groups:
            return
        base = self._base_lr if hasattr(self, "_base_lr") else None
        if base is None:
            self._base_lr = base = groups[0]["lr"]
        if self.model_name.startswith("bert"):
            return  # BertAdam has its own warmup schedule
        if self.model_name == "lstman4":
            # reference _adjust_learning_rate_lstman4: lr /= 1.01 per epoch
            for g in groups:
                g["lr"] = base / (1.01 ** epoch)
            return
        if self.model_name == "lstm":
            # reference _adjust_learning_rate_lstmptb (:514-529).  As written
            # there, first=63 > second=60 makes the 0.1x branch unreachable —
            # effective schedule: base below 63, x0.01 at 63, x0.001 at 80;
            # reproduced faithfully.
            factor = 1.0 if epoch < 63 else (0.01 if epoch < 80 else 0.001)
            for g in groups:
                g["lr"] = base * factor
            return
        milestones = (81, 122) if self.batches.family == "cifar" else (10, 20)
        factor = 0.1 ** sum(1 for m in milestones if epoch >= m)
        for g in groups:
            g["lr"] = base * factor

    @torch.no_grad()
    def evaluate(self, n_batches: int = 4) -> dict:
        """Synthetic-shape eval (reference DLTrainer.test,
        VGG/dl_trainer.py:709-784): top-1 for classifiers, greedy-decode WER
        for CTC, perplexity for LMs, loss for BERT."""
        from .utils import GreedyDecoder, accuracy_topk, perplexity, wer

        self.model.eval()
        try:
            b = self.batches
            if b.family in ("cifar", "imagenet", "mnist"):
                out = self.model(b.x)
                top1 = accuracy_topk(out.float(), b.y, (1,))[0]
                return {"top1": top1}
            if b.family == "ptb":
                logits, _ = self.model(b.tokens)
                nll = torch.nn.functional.cross_entropy(
                    logits.view(-1, logits.size(-1)).float(), b.targets.view(-1)
                )
                return {"perplexity": perplexity(float(nll))}
            if self.model_name == "lstman4":
                logits = self.model(b.x)
                dec = GreedyDecoder("_'abcdefghijklmnopqrstuvwxyz ")
                hyps = dec.decode(logits.float())
                refs = ["" for _ in hyps]  # synthetic targets have no text
                return {"wer": sum(wer(h, r) for h, r in zip(hyps, refs)) / len(hyps)}
            loss = self._forward_loss()
            return {"loss": float(loss.float())}
        finally:
            self.model.train()

    def step(self) -> float:
        """One optimizer step (with nsteps_update grad-accumulation substeps)."""
        if self._graph is not None and self.nsteps_update == 1:
            self.opt.zero_grad()
            self._graph.replay()
            self.opt.step()
            self.iteration += 1
            self.last_loss = float(self._graph_loss.detach().float().item())
            return self.last_loss
        self.opt.zero_grad()
        for sub in range(self.nsteps_update):
            if hasattr(self.opt, "local"):
                self.opt.local = sub < self.nsteps_update - 1
            if hasattr(self.opt, "set_substep"):
                # direct gradient slots: sub-step 0 overwrites, later ones
                # accumulate (a captured graph is always sub-step 0)
                self.opt.set_substep(sub)
            if self.autocast:
                with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                    loss = self._forward_loss()
            else:
                loss = self._forward_loss()
            loss.backward()
        self.opt.step()
        self.iteration += 1
        self.last_loss = float(loss.detach().float().item())
        return self.last_loss
