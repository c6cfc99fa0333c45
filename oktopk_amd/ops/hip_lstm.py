"""fp32 LSTM layers whose time loop is hand-written HIP
(ops/csrc/lstm_cell.hip), forward and backward: one direction with
`lstm_layer`, a unidirectional nn.LSTM stack with `lstm_stack`.

What stays in torch, once per layer: the input projection x @ W_ih^T + b, the
three weight-gradient products and dx — large, well-filled GEMMs.  The
recurrence is `_hip_ops.lstm_fwd` / `lstm_bwd`: one binding call each, which
enqueues one step kernel per time step on the current stream with no host
sync, so the layer can be captured in a graph.  The recurrence may start from
a given (h0, c0) and hand back its final state, with gradients both ways, so
a state can be carried from one BPTT window to the next.

`BatchRNN` (models/lstm.py) and `PTBLSTM` (models/small_cnns.py) take this
path when OKTOPK_HIP_LSTM=1 and `hip_lstm_available` /
`hip_lstm_stack_available` holds; otherwise they call their nn.LSTM as before
(profiles/README.md r17 and r18 have the A/Bs).  On a CPU tensor `lstm_layer`
runs `reference.lstm_layer_ref`.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import reference as _ref


def hip_lstm_enabled() -> bool:
    return os.environ.get("OKTOPK_HIP_LSTM", "0") == "1"


def _kernels_take(x, rnn) -> bool:
    """The conditions every layer of rnn must meet, whatever their number."""
    if not (isinstance(rnn, torch.nn.LSTM) and rnn.bias
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


def hip_lstm_available(x, rnn) -> bool:
    """Whether lstm_layer's kernels take input x [T, N, F] with rnn's
    parameters: a one-layer fp32 nn.LSTM with biases, time-major, no
    projection, H % 4 == 0, on the GPU, outside autocast."""
    return (isinstance(rnn, torch.nn.LSTM) and rnn.num_layers == 1
            and _kernels_take(x, rnn))


def hip_lstm_stack_available(x, rnn) -> bool:
    """Whether lstm_stack's kernels take x [T, N, F] with rnn: as
    hip_lstm_available, for any number of layers of one direction."""
    return (isinstance(rnn, torch.nn.LSTM) and not rnn.bidirectional
            and _kernels_take(x, rnn))


class _LstmLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, h0, c0, reverse, return_state,
                batch_tiles):
        from . import _backend

        hip = _backend(x)  # raises when the extension is not built
        x = x.contiguous()
        T, N, F = x.shape
        H = w_hh.shape[1]
        gx = torch.addmm(b_ih + b_hh, x.view(T * N, F), w_ih.t()).view(T, N, 4 * H)
        if h0 is not None:
            h0, c0 = h0.contiguous(), c0.contiguous()
        # gx becomes the activations (i, f, g, o): what backward needs
        y, c = hip.lstm_fwd(gx, w_hh.contiguous(), reverse, h0, c0, batch_tiles)
        ctx.save_for_backward(x, w_ih, w_hh, gx, c, y, h0, c0)
        ctx.reverse, ctx.batch_tiles = reverse, batch_tiles
        ctx.set_materialize_grads(False)
        if not return_state:
            return y
        last = 0 if reverse else T - 1
        # tensors of their own: a view of y would tie their gradients to gy
        return y, y[last].clone(), c[last].clone()

    @staticmethod
    def backward(ctx, gy, g_hn=None, g_cn=None):
        from . import _backend

        x, w_ih, w_hh, act, c, y, h0, c0 = ctx.saved_tensors
        T, N, F = x.shape
        H = w_hh.shape[1]
        gy = torch.zeros_like(y) if gy is None else gy.contiguous()
        g_hn = None if g_hn is None else g_hn.contiguous()
        g_cn = None if g_cn is None else g_cn.contiguous()
        need = ctx.needs_input_grad
        out = _backend(x).lstm_bwd(gy, act, c, y, w_hh.t().contiguous(),
                                   ctx.reverse, g_hn, g_cn, c0,
                                   h0 is not None and need[5], ctx.batch_tiles)
        dg, dh0, dc0 = out if isinstance(out, tuple) else (out, None, None)
        dg2 = dg.view(T * N, 4 * H)
        # h_prev is y shifted by one step of the recurrence; its first row is
        # h0, added below, or zeros, which drop out of the product
        if ctx.reverse:
            dg_rec, h_prev, dg_first = dg[:-1], y[1:], dg[-1]
        else:
            dg_rec, h_prev, dg_first = dg[1:], y[:-1], dg[0]
        dx = (dg2 @ w_ih).view(T, N, F) if need[0] else None
        dw_ih = dg2.t() @ x.view(T * N, F) if need[1] else None
        dw_hh = (dg_rec.reshape(-1, 4 * H).t() @ h_prev.reshape(-1, H)
                 if need[2] else None)
        if need[2] and h0 is not None:
            dw_hh = torch.addmm(dw_hh, dg_first.t(), h0)
        db_ih = dg2.sum(0) if need[3] or need[4] else None
        # two tensors: the two .grad must not share storage
        db_hh = db_ih.clone() if need[3] and need[4] else db_ih
        if h0 is None:
            dc0 = None
        return dx, dw_ih, dw_hh, db_ih, db_hh, dh0, dc0, None, None, None


def lstm_layer(x, w_ih, w_hh, b_ih, b_hh, reverse: bool = False, h0=None,
               c0=None, return_state: bool = False, batch_tiles: int = 0):
    """y [T, N, H] of one LSTM direction over x [T, N, F], from the state
    (h0, c0) [N, H] — both or neither; zeros when absent; torch's gate order
    and parameter shapes, differentiable in x, the four parameters and the
    state.  With return_state: (y, h_n, c_n), the state after the last step
    of the recurrence.  fp32 with H % 4 == 0 on the GPU (hip_lstm_available);
    reference.lstm_layer_ref on the CPU.  batch_tiles: 16-row batch tiles per
    block of the step kernels, 0 (auto), 1 or 2; the bits do not depend on it."""
    from . import _backend

    if (h0 is None) != (c0 is None):
        raise ValueError("lstm_layer: h0 and c0 go together")
    if _backend(x) is _ref:
        return _ref.lstm_layer_ref(x, w_ih, w_hh, b_ih, b_hh, reverse, h0, c0,
                                   return_state)
    return _LstmLayerFn.apply(x, w_ih, w_hh, b_ih, b_hh, h0, c0, bool(reverse),
                              bool(return_state), int(batch_tiles))


def lstm_stack(x, rnn, hidden=None, training=None):
    """nn.LSTM's forward for a unidirectional, time-major stack on
    lstm_layer, read from rnn's own parameters: x [T, N, F] and an optional
    hidden = (h0, c0), both [layers, N, H] -> (y, (h_n, c_n)).  Between
    layers F.dropout(p=rnn.dropout), where nn.LSTM places it; `training`
    defaults to rnn.training.  The masks are torch's own draws, not the ones
    MIOpen's RNN would make from the same generator state."""
    if training is None:
        training = rnn.training
    h_n, c_n = [], []
    y = x
    for l in range(rnn.num_layers):
        params = [getattr(rnn, f"{n}_l{l}")
                  for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        h0, c0 = (None, None) if hidden is None else (hidden[0][l], hidden[1][l])
        y, h, c = lstm_layer(y, *params, h0=h0, c0=c0, return_state=True)
        h_n.append(h)
        c_n.append(c)
        if l + 1 < rnn.num_layers and rnn.dropout > 0:
            y = F.dropout(y, rnn.dropout, training)
    return y, (torch.stack(h_n), torch.stack(c_n))
