"""ops.hip_ctc on the CPU: ctc_loss is F.ctc_loss(F.log_softmax(.)) to the bit,
loss and gradient, and the trainer's switch changes nothing without a GPU."""
import pytest
import torch
import torch.nn.functional as F

from oktopk_amd.ops.hip_ctc import ctc_loss, hip_ctc_available


def inputs(padded):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(9, 3, 6, generator=g)
    tgt_len = torch.tensor([3, 1, 2])
    targets = torch.randint(1, 6, (3, 3), generator=g)
    if not padded:
        targets = torch.cat([targets[n, :l] for n, l in enumerate(tgt_len)])
    return logits, targets, torch.tensor([9, 5, 7]), tgt_len


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("padded", [True, False])
def test_cpu_is_torch_to_the_bit(padded, reduction):
    logits, targets, in_len, tgt_len = inputs(padded)
    assert not hip_ctc_available(logits, targets, in_len, tgt_len)
    w = torch.arange(1., 4.) if reduction == "none" else torch.tensor(1.)
    res = []
    for fn in (lambda x: ctc_loss(x, targets, in_len, tgt_len, reduction=reduction),
               lambda x: F.ctc_loss(F.log_softmax(x, -1), targets, in_len, tgt_len,
                                    reduction=reduction)):
        x = logits.clone().requires_grad_()
        loss = fn(x)
        res.append((loss.detach(), torch.autograd.grad((loss * w).sum(), x)[0]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_trainer_switch_is_inert_on_cpu(monkeypatch):
    from oktopk_amd.comm import Comm
    from oktopk_amd.trainer import Trainer

    tr = Trainer(model_name="lstman4", batch_size=2, comm=Comm(None), dtype="fp32",
                 device=torch.device("cpu"), model_kwargs=dict(rnn_hidden_size=32, nb_layers=1))
    tr.model.eval()  # the same dropout-free forward twice
    monkeypatch.delenv("OKTOPK_HIP_CTC", raising=False)
    off = tr._forward_loss().detach()
    monkeypatch.setenv("OKTOPK_HIP_CTC", "1")
    on = tr._forward_loss().detach()
    assert torch.isfinite(off) and torch.equal(on, off)
