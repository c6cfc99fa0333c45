"""One fp32 LSTM direction whose time loop is hand-written HIP
(ops/csrc/lstm_cell.hip), forward and backward.

What stays in torch, once per layer: the input projection x @ W_ih^T + b, the
three weight-gradient products and dx — large, well-filled GEMMs.  The
recurrence is `_hip_ops.lstm_fwd` / `lstm_bwd`: one binding call each, which
enqueues one step kernel per time step on the current stream with no host
sync, so the layer can be captured in a graph.

`BatchRNN` (models/lstm.py) takes this path when OKTOPK_HIP_LSTM=1 and
`hip_lstm_available` holds; otherwise it calls its nn.LSTM as before
(profiles/README.md r17 has the A/B).  On a CPU tensor `lstm_layer` runs
`reference.lstm_layer_ref`.
"""
from __future__ import annotations

import os

import torch

from . import reference as _ref


def hip_lstm_enabled() -> bool:
    return os.environ.get("OKTOPK_HIP_LSTM", "0") == "1"


def hip_lstm_available(x, rnn) -> bool:
    """Whether lstm_layer's kernels take input x [T, N, F] with rnn's
    parameters: a one-layer fp32 nn.LSTM with biases, time-major, no
    projection, H % 4 == 0, on the GPU, outside autocast."""
    if not (isinstance(rnn, torch.nn.LSTM) and rnn.num_layers == 1 and rnn.bias
            and not rnn.batch_first and rnn.proj_size == 0
            and rnn.hidden_size % 4 == 0
            and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32
            and x.size(0) >= 1 and x.size(1) >= 1
            and not torch.is_autocast_enabled()
            and all(p.dtype == torch.float32 and p.device == x.device
                    for p in rnn.parameters())):
        return False
    from . import hip_available

    return hip_available()


class _LstmLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, reverse):
        from . import _backend

        hip = _backend(x)  # raises when the extension is not built
        x = x.contiguous()
        T, N, F = x.shape
        H = w_hh.shape[1]
        gx = torch.addmm(b_ih + b_hh, x.view(T * N, F), w_ih.t()).view(T, N, 4 * H)
        # gx becomes the activations (i, f, g, o): what backward needs
        y, c = hip.lstm_fwd(gx, w_hh.contiguous(), reverse)
        ctx.save_for_backward(x, w_ih, w_hh, gx, c, y)
        ctx.reverse = reverse
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import _backend

        x, w_ih, w_hh, act, c, y = ctx.saved_tensors
        T, N, F = x.shape
        H = w_hh.shape[1]
        dg = _backend(x).lstm_bwd(gy.contiguous(), act, c, y,
                                  w_hh.t().contiguous(), ctx.reverse)
        dg2 = dg.view(T * N, 4 * H)
        # h_prev is y shifted by one step of the recurrence with a zero first
        # row, which drops out of the product
        if ctx.reverse:
            dg_rec, h_prev = dg[:-1], y[1:]
        else:
            dg_rec, h_prev = dg[1:], y[:-1]
        need = ctx.needs_input_grad
        dx = (dg2 @ w_ih).view(T, N, F) if need[0] else None
        dw_ih = dg2.t() @ x.view(T * N, F) if need[1] else None
        dw_hh = (dg_rec.reshape(-1, 4 * H).t() @ h_prev.reshape(-1, H)
                 if need[2] else None)
        db_ih = dg2.sum(0) if need[3] or need[4] else None
        # two tensors: the two .grad must not share storage
        db_hh = db_ih.clone() if need[3] and need[4] else db_ih
        return dx, dw_ih, dw_hh, db_ih, db_hh, None


def lstm_layer(x, w_ih, w_hh, b_ih, b_hh, reverse: bool = False):
    """y [T, N, H] of one LSTM direction over x [T, N, F] with zero initial
    state; torch's gate order and parameter shapes, differentiable in x and
    the four parameters.  fp32 with H % 4 == 0 on the GPU
    (hip_lstm_available); reference.lstm_layer_ref on the CPU."""
    from . import _backend

    if _backend(x) is _ref:
        return _ref.lstm_layer_ref(x, w_ih, w_hh, b_ih, b_hh, reverse)
    return _LstmLayerFn.apply(x, w_ih, w_hh, b_ih, b_hh, bool(reverse))
