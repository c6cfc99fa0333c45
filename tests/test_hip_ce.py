"""ops.hip_ce on the CPU: cross_entropy is F.cross_entropy to the bit, loss and
gradient, and with the switch unset the trainer's and BERT's loss calls are
F.cross_entropy calls."""
import pytest
import torch
import torch.nn.functional as F

from oktopk_amd.ops.hip_ce import cross_entropy, hip_ce_available


@pytest.mark.parametrize("switch", [None, "1"])
@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_cpu_is_torch_to_the_bit(monkeypatch, reduction, switch):
    monkeypatch.delenv("OKTOPK_HIP_CE", raising=False)
    if switch:
        monkeypatch.setenv("OKTOPK_HIP_CE", switch)
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(6, 11, generator=g)
    target = torch.tensor([3, -1, 0, 10, -1, 7])
    assert not hip_ce_available(logits, target)
    w = torch.arange(1., 7.) if reduction == "none" else torch.tensor(1.)
    res = []
    for fn in (cross_entropy, F.cross_entropy):
        x = logits.clone().requires_grad_()
        loss = fn(x, target, ignore_index=-1, reduction=reduction)
        res.append((loss.detach(), torch.autograd.grad((loss * w).sum(), x)[0]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def counting(monkeypatch):
    calls = []
    plain = F.cross_entropy
    monkeypatch.delenv("OKTOPK_HIP_CE", raising=False)
    monkeypatch.setattr(F, "cross_entropy",
                        lambda *a, **kw: calls.append(kw) or plain(*a, **kw))
    return calls


def test_trainer_loss_is_torchs_when_unset(monkeypatch):
    from oktopk_amd.comm import Comm
    from oktopk_amd.trainer import Trainer

    calls = counting(monkeypatch)
    tr = Trainer(model_name="mnistnet", batch_size=2, comm=Comm(None), dtype="fp32",
                 device=torch.device("cpu"))
    assert torch.isfinite(tr._forward_loss()) and len(calls) == 1


def test_bert_loss_is_torchs_when_unset(monkeypatch):
    from oktopk_amd.models.bert import bert_base

    calls = counting(monkeypatch)
    model = bert_base(num_hidden_layers=1, hidden_size=32, num_attention_heads=2,
                      intermediate_size=64, vocab_size=50)
    ids = torch.arange(16).view(2, 8)
    labels = torch.where(ids % 3 == 0, ids, -1)
    loss = model(ids, attention_mask=torch.ones_like(ids), masked_lm_labels=labels,
                 next_sentence_label=torch.tensor([0, 1]))
    assert torch.isfinite(loss) and len(calls) == 2
    assert calls[0]["ignore_index"] == -1
