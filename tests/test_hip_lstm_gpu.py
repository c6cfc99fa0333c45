"""Fused LSTM step kernels (ops/csrc/lstm_cell.hip) through
ops.hip_lstm.lstm_layer, against reference.lstm_layer_ref in fp64.

Per tensor (y and the gradients of x, W_ih, W_hh, b_ih, b_hh) the kernel's
rel_fro against the fp64 oracle must stay within R.LSTM_REF32_FACTOR (3) times
that of lstm_layer_ref in fp32 on the CPU on the same inputs; no absolute
tolerance.  Weights are uniform in +-1/sqrt(H), x standard normal, the input
size differs from H.  The model-level tests apply the same rule to the loss
and every parameter gradient of a BatchRNN and a 2-layer DeepSpeech, against
the same module on the CPU.  Measured ratios: profiles/README.md r17.
"""
import copy
import functools

import pytest
import torch

from oktopk_amd.models import lstm as lstm_model
from oktopk_amd.ops import reference as R
from oktopk_amd.ops.hip_lstm import hip_lstm_available, lstm_layer

pytestmark = pytest.mark.gpu

NAMES = ("y", "dx", "dW_ih", "dW_hh", "db_ih", "db_hh")


def layer_inputs(T, N, H, seed=0):
    """fp64 CPU (x, W_ih, W_hh, b_ih, b_hh, gy)."""
    g = torch.Generator().manual_seed(seed)
    F = H + 3
    w = [(torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1) / H ** 0.5
         for s in ((4 * H, F), (4 * H, H), (4 * H,), (4 * H,))]
    x = torch.randn(T, N, F, generator=g, dtype=torch.float64)
    gy = torch.randn(T, N, H, generator=g, dtype=torch.float64)
    return [x] + w + [gy]


def run_layer(fn, inputs, reverse):
    """[y, dx, dW_ih, dW_hh, db_ih, db_hh] of fn on (views of) the inputs."""
    *args, gy = inputs
    args = [a.detach().requires_grad_() for a in args]
    y = fn(*args, reverse=reverse)
    return [y.detach()] + list(torch.autograd.grad(y, args, gy))


@functools.lru_cache(maxsize=None)
def cpu_side(T, N, H, reverse):
    """(fp64 inputs, fp64 oracle, the fp32 yardstick's rel_fro per tensor)."""
    inputs = layer_inputs(T, N, H)
    ref64 = run_layer(R.lstm_layer_ref, inputs, reverse)
    ref32 = run_layer(R.lstm_layer_ref, [a.float() for a in inputs], reverse)
    return inputs, ref64, [R.lstm_rel_fro(a, b) for a, b in zip(ref32, ref64)]


def check(got, ref64, yard, names=NAMES):
    bad = {}
    for n, a, b, y in zip(names, got, ref64, yard):
        if not b.any():  # dW_hh at T = 1: no product ran, exactly zero
            assert not a.any(), n
            continue
        err = R.lstm_rel_fro(a, b)
        print(f"{n}: kernel {err:.3e} yardstick {y:.3e}")
        if not err <= R.LSTM_REF32_FACTOR * y:
            bad[n] = (err, y)
    assert not bad, bad


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 16, 17])
@pytest.mark.parametrize("H", [4, 8, 36])
def test_layer_against_fp64(H, N, T, reverse):
    inputs, ref64, yard = cpu_side(T, N, H, reverse)
    got = run_layer(lstm_layer, [a.float().cuda() for a in inputs], reverse)
    check(got, ref64, yard)


@pytest.mark.parametrize("reverse", [False, True])
def test_recipe_width(reverse):
    inputs, ref64, yard = cpu_side(3, 17, 800, reverse)
    got = run_layer(lstm_layer, [a.float().cuda() for a in inputs], reverse)
    check(got, ref64, yard)


def test_offset_views():
    """Every tensor 4 bytes off 16-byte alignment: the scalar-load kernels."""
    inputs, ref64, yard = cpu_side(5, 17, 36, False)
    views = []
    for a in inputs:
        buf = torch.empty(a.numel() + 1, device="cuda")
        v = buf[1:].view(a.shape).copy_(a)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        views.append(v)
    check(run_layer(lstm_layer, views, False), ref64, yard)


def test_graph_replays_equal_eager():
    inputs = [a.float().cuda() for a in layer_inputs(5, 17, 36)]
    eager = run_layer(lstm_layer, inputs, False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_layer(lstm_layer, inputs, False)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run_layer(lstm_layer, inputs, False)
    for _ in range(3):
        for o in out:
            o.fill_(float("nan"))
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))


def model_results(model, x, target):
    """[loss] + every parameter gradient, for a squared distance to target."""
    loss = (model(x) - target).square().mean()
    params = list(model.parameters())
    return [loss.detach()] + list(torch.autograd.grad(loss, params))


def batchnorm_on_running_stats(model):
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()
    return model


# BatchRNN: BatchNorm in training mode, whose input gradient reaches no
# parameter.  DeepSpeech: every BatchNorm on its running statistics, an affine
# map.  In training mode its input gradient is a difference of nearly equal
# terms and DeepSpeech chains three of them between the loss and the
# convolutions: the rounding noise of everything downstream, convolutions
# and the BatchNorms themselves included, then reaches the measured
# gradients 50 - 150 times enlarged in one common direction, and a ratio of
# two single draws of that says nothing about the LSTM (profiles/README.md
# r17: MIOpen's nn.LSTM in the same module on the same GPU misses the factor
# on the same tensors).  With the affine map every parameter has a gradient
# of its own, the convolution biases too.
@pytest.mark.parametrize("build, shape", [
    (lambda: lstm_model.BatchRNN(11, 8, bidirectional=True), (5, 17, 11)),
    (lambda: batchnorm_on_running_stats(
        lstm_model.DeepSpeech(rnn_hidden_size=8, nb_layers=2)), (3, 1, 161, 12)),
], ids=["BatchRNN", "DeepSpeech"])
def test_model_against_fp64(monkeypatch, build, shape):
    torch.manual_seed(7)
    m32 = build()
    x = torch.randn(*shape)
    tgt = torch.randn_like(m32(x))
    ref64 = model_results(copy.deepcopy(m32).double(), x.double(), tgt.double())
    yard = [R.lstm_rel_fro(a, b)
            for a, b in zip(model_results(m32, x, tgt), ref64)]

    calls = []
    monkeypatch.setenv("OKTOPK_HIP_LSTM", "1")
    monkeypatch.setattr(lstm_model, "lstm_layer",
                        lambda *a, **k: calls.append(1) or lstm_layer(*a, **k))
    gpu = copy.deepcopy(m32).cuda()
    got = model_results(gpu, x.cuda(), tgt.cuda())
    assert calls, "the switch did not reach lstm_layer"
    assert list(gpu.state_dict()) == list(m32.state_dict())
    names = ["loss"] + [n for n, _ in m32.named_parameters()]
    check(got, ref64, yard, names)


def test_availability():
    x = torch.randn(4, 2, 1312, device="cuda")
    assert hip_lstm_available(x, torch.nn.LSTM(1312, 800).cuda())
    assert hip_lstm_available(x[..., :800], torch.nn.LSTM(800, 800).cuda())
    assert not hip_lstm_available(x[..., :6], torch.nn.LSTM(6, 6).cuda())
    assert not hip_lstm_available(x.bfloat16(), torch.nn.LSTM(1312, 800).cuda())
