"""The CPU path of ops.hip_lstm.lstm_stack — reference.lstm_layer_ref per
layer, with carried state — in fp64 against torch.nn.LSTM in fp64: outputs,
final state and every gradient, the state's included.

Bound: rel_fro <= 1e-12.  Both sides run the same formula in fp64 and differ
in summation order alone; the sums have at most 16 terms over 5 steps, so a
few hundred units of 1.1e-16 is the expected size and 1e-12 leaves two orders
of margin.
"""
import torch

from oktopk_amd.ops import reference as R
from oktopk_amd.ops.hip_lstm import lstm_stack


def test_stack_matches_nn_lstm_fp64():
    torch.manual_seed(3)
    L, H, N, T = 2, 8, 3, 5
    rnn = torch.nn.LSTM(6, H, num_layers=L).double()
    x = torch.randn(T, N, 6, dtype=torch.float64)
    hidden = [torch.randn(L, N, H, dtype=torch.float64) for _ in range(2)]
    gouts = [torch.randn(T, N, H, dtype=torch.float64)] + [torch.randn_like(h) for h in hidden]

    def run(fn):
        leaves = [t.detach().requires_grad_() for t in [x] + hidden]
        y, (h_n, c_n) = fn(leaves[0], (leaves[1], leaves[2]))
        grads = torch.autograd.grad([y, h_n, c_n], leaves + list(rnn.parameters()), gouts)
        return [y.detach(), h_n.detach(), c_n.detach()] + list(grads)

    want = run(rnn)
    got = run(lambda a, hid: lstm_stack(a, rnn, hid))
    assert len(got) == len(want) == 6 + 4 * L
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and R.lstm_rel_fro(a, b) <= 1e-12, i


def test_ref_without_state_is_unchanged():
    torch.manual_seed(4)
    T, N, F, H = 5, 3, 6, 8
    x = torch.randn(T, N, F)
    w_ih, w_hh, b_ih, b_hh = (torch.randn(s) * 0.3
                              for s in ((4 * H, F), (4 * H, H), (4 * H,), (4 * H,)))
    for reverse in (False, True):
        # the loop as it stood before the state arguments
        gx = (x.reshape(T * N, -1) @ w_ih.t() + (b_ih + b_hh)).view(T, N, 4 * H)
        h, c, ys = x.new_zeros(N, H), x.new_zeros(N, H), [None] * T
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            i, f, g, o = (gx[t] + h @ w_hh.t()).chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            ys[t] = h
        assert torch.equal(R.lstm_layer_ref(x, w_ih, w_hh, b_ih, b_hh, reverse),
                           torch.stack(ys))
        _, h_n, c_n = R.lstm_layer_ref(x, w_ih, w_hh, b_ih, b_hh, reverse,
                                       return_state=True)
        assert torch.equal(h_n, h) and torch.equal(c_n, c)
