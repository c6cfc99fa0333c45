"""Carried state, batch-tile pairs and the stacked front end of the fused LSTM
kernels (ops/csrc/lstm_cell.hip), under the rule of test_hip_lstm_gpu.py: per
tensor, rel_fro against reference.lstm_layer_ref in fp64 at most
R.LSTM_REF32_FACTOR times that of the same loop in fp32 on the CPU on the
same inputs; no absolute tolerance.  Inputs as in layer_inputs, plus h0, c0
and the gradients at the final state, standard normal.  Measured ratios:
profiles/README.md r18.
"""
import copy
import functools

import pytest
import torch

from oktopk_amd.models import small_cnns
from oktopk_amd.ops import reference as R
from oktopk_amd.ops.hip_lstm import lstm_layer, lstm_stack
from test_hip_lstm_gpu import check, layer_inputs

pytestmark = pytest.mark.gpu

NAMES = ("y", "h_n", "c_n", "dx", "dW_ih", "dW_hh", "db_ih", "db_hh", "dh0", "dc0")
# N = 17: a pair with one tile nearly empty; 33: a full pair and a second
# block row; T = 1: first = last step; the last entry is the PTB recipe's width
SHAPES = [(H, N, T) for H in (4, 36) for N in (1, 17, 33) for T in (1, 3)]
SHAPES.append((1500, 20, 2))


def state_inputs(T, N, H):
    """fp64 CPU ([x, W_ih, W_hh, b_ih, b_hh, h0, c0], [gy, g_hn, g_cn])."""
    *args, gy = layer_inputs(T, N, H)
    g = torch.Generator().manual_seed(1)
    h0, c0, g_hn, g_cn = (torch.randn(N, H, generator=g, dtype=torch.float64)
                          for _ in range(4))
    return args + [h0, c0], [gy, g_hn, g_cn]


def run_layer(fn, args, gouts, reverse, **kw):
    """The ten tensors of NAMES."""
    args = [a.detach().requires_grad_() for a in args]
    outs = fn(*args[:5], reverse=reverse, h0=args[5], c0=args[6],
              return_state=True, **kw)
    return [o.detach() for o in outs] + list(torch.autograd.grad(outs, args, gouts))


@functools.lru_cache(maxsize=None)
def cpu_side(T, N, H, reverse):
    """(fp64 inputs, fp64 oracle, the fp32 yardstick's rel_fro per tensor)."""
    args, gouts = state_inputs(T, N, H)
    ref64 = run_layer(R.lstm_layer_ref, args, gouts, reverse)
    ref32 = run_layer(R.lstm_layer_ref, [a.float() for a in args],
                      [g.float() for g in gouts], reverse)
    return (args, gouts), ref64, [R.lstm_rel_fro(a, b) for a, b in zip(ref32, ref64)]


def on_gpu(inputs):
    return [[t.float().cuda() for t in part] for part in inputs]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("H, N, T", SHAPES)
def test_layer_with_state_against_fp64(H, N, T, reverse):
    inputs, ref64, yard = cpu_side(T, N, H, reverse)
    check(run_layer(lstm_layer, *on_gpu(inputs), reverse), ref64, yard, NAMES)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("N", [17, 33])
def test_batch_tiles_same_bits(N, reverse):
    args, gouts = on_gpu(state_inputs(3, N, 36))
    one = run_layer(lstm_layer, args, gouts, reverse, batch_tiles=1)
    two = run_layer(lstm_layer, args, gouts, reverse, batch_tiles=2)
    assert [n for n, a, b in zip(NAMES, one, two) if not torch.equal(a, b)] == []


def test_graph_replays_equal_eager():
    args, gouts = on_gpu(state_inputs(3, 17, 36))
    eager = run_layer(lstm_layer, args, gouts, False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_layer(lstm_layer, args, gouts, False)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run_layer(lstm_layer, args, gouts, False)
    for _ in range(3):
        for o in out:
            o.fill_(float("nan"))
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))


def two_windows(model, tokens, targets):
    """[loss] + every parameter gradient of two BPTT windows with the hidden
    state carried across, undetached; the final state enters the loss."""
    hidden, loss = None, 0.
    for tok, tgt in zip(tokens, targets):
        out, hidden = model(tok, hidden)
        loss = loss + (out - tgt).square().mean()
    loss = loss + hidden[0].square().mean() + hidden[1].square().mean()
    return [loss.detach()] + list(torch.autograd.grad(loss, list(model.parameters())))


def test_ptblstm_against_fp64(monkeypatch):
    torch.manual_seed(7)
    m32 = small_cnns.PTBLSTM(vocab_size=50, emb=12, hidden=8, layers=2, dropout=0.0)
    tokens = torch.randint(0, 50, (2, 3, 17))
    tgt = torch.randn(2, 3, 17, 50)
    ref64 = two_windows(copy.deepcopy(m32).double(), tokens, tgt.double())
    yard = [R.lstm_rel_fro(a, b) for a, b in zip(two_windows(m32, tokens, tgt), ref64)]

    calls = []
    monkeypatch.setenv("OKTOPK_HIP_LSTM", "1")
    monkeypatch.setattr(small_cnns, "lstm_stack",
                        lambda *a, **k: calls.append(1) or lstm_stack(*a, **k))
    gpu = copy.deepcopy(m32).cuda()
    got = two_windows(gpu, tokens.cuda(), tgt.cuda())
    assert len(calls) == 2, "the switch did not reach lstm_stack"
    assert list(gpu.state_dict()) == list(m32.state_dict())
    check(got, ref64, yard, ["loss"] + [n for n, _ in m32.named_parameters()])

    monkeypatch.delenv("OKTOPK_HIP_LSTM")
    with torch.no_grad():
        hidden = tuple(torch.randn(2, 17, 8, device="cuda") for _ in range(2))
        out, (h_n, c_n) = gpu(tokens[0].cuda(), hidden)
        y, (h_d, c_d) = gpu.rnn(gpu.encoder(tokens[0].cuda()), hidden)
    assert len(calls) == 2
    assert torch.equal(out, gpu.decoder(y))
    assert torch.equal(h_n, h_d) and torch.equal(c_n, c_d)
