"""reference.lstm_layer_ref, the oracle of the fused LSTM kernels, against
nn.LSTM in fp64, and the BatchRNN switch on the CPU (where lstm_layer runs
that reference).

Bound 2^-40 on rel_fro: far above fp64 rounding over K * T terms, far below
what a wrong gate order or a wrong shift of h_prev gives.
"""
import pytest
import torch
import torch.nn as nn

from oktopk_amd.models import lstm as lstm_model
from oktopk_amd.ops import reference as R
from oktopk_amd.utils.flops import get_model_complexity_info

BOUND = 2.0 ** -40
T, N, F, H = 5, 3, 7, 12


@pytest.mark.parametrize("reverse", [False, True])
def test_ref_matches_nn_lstm_fp64(reverse):
    torch.manual_seed(3)
    rnn = nn.LSTM(F, H, bidirectional=True).double()
    sfx = "_reverse" if reverse else ""
    params = [getattr(rnn, n + sfx) for n in
              ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    x = torch.randn(T, N, F, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(T, N, H, dtype=torch.float64)

    want = rnn(x)[0][..., H:] if reverse else rnn(x)[0][..., :H]
    got = R.lstm_layer_ref(x, *params, reverse=reverse)
    pairs = [(got, want)] + list(zip(torch.autograd.grad(got, [x] + params, gy),
                                     torch.autograd.grad(want, [x] + params, gy)))
    for a, b in pairs:
        assert R.lstm_rel_fro(a, b) <= BOUND


@pytest.mark.parametrize("bidirectional", [False, True])
def test_batch_rnn_switch_keeps_result_and_flops(monkeypatch, bidirectional):
    torch.manual_seed(4)
    m = lstm_model.BatchRNN(F, H, bidirectional=bidirectional).double()
    x = torch.randn(T, N, F, dtype=torch.float64)
    want = m(x)
    flops = get_model_complexity_info(m, input_constructor=lambda _: x)[0]
    m.train()

    monkeypatch.setenv("OKTOPK_HIP_LSTM", "1")
    monkeypatch.setattr(lstm_model, "hip_lstm_available", lambda x, rnn: True)
    monkeypatch.setattr(m.rnn, "forward", None)  # the switch must not call it
    assert R.lstm_rel_fro(m(x), want) <= BOUND
    assert get_model_complexity_info(m, input_constructor=lambda _: x)[0] == flops
