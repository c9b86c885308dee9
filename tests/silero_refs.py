"""Staged CPU reference of the Silero VAD network - TEST HELPER.  The three functions mirror `ac_silero_frontend`, `ac_silero_lstm`
and `ac_silero_out` (include/audiocut_hip.h) and their argument conventions, in plain torch with a `dtype` argument: float64 is the
reference, float32 the yardstick that says how far an honest float32 evaluation of the same stage lands from it.  `weights` is the
state-dict-named numpy dict of `audio_cut_amd/testing/silero_synth.py`; arrays in, numpy arrays of `dtype` out."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

WINDOW = 512
CONTEXT = 64
HIDDEN = 128


def _t(weights, name, dtype):
    return torch.from_numpy(np.asarray(weights[name], dtype=np.float32)).to(dtype)


def _in(a, dtype):
    """A stage's input as it is (float32 from a kernel, or the previous stage's unrounded result), carried to `dtype`."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def frontend_input(x16, win_start, dtype=torch.float64) -> torch.Tensor:
    """[n, 640]: 64 samples of context (zeros where win_start = -(index) - 1) | the 512-sample window | 64 reflected samples."""
    x = _in(x16, dtype)
    ws = torch.as_tensor(np.asarray(win_start, dtype=np.int64))
    first = ws < 0
    base = torch.where(first, -(ws + 1), ws)
    idx = base[:, None] + torch.arange(-CONTEXT, WINDOW)[None, :]                       # [n, 576]
    valid = ~(first[:, None] & (idx < base[:, None]))
    assert int(idx[valid].min()) >= 0 and int(idx.max()) < x.numel(), "a window reaches outside x16"
    inp = torch.where(valid, x[idx.clamp(min=0)], torch.zeros((), dtype=dtype))
    return torch.cat([inp, inp[:, 511:575].flip(1)], dim=1)                               # F.pad(mode="reflect"): x[574 - j], j < 64


def frontend(weights, x16, win_start, dtype=torch.float64) -> np.ndarray:
    """gates_x [n, 512] = weight_ih feat + bias_ih + bias_hh of every window."""
    t = lambda name: _t(weights, name, dtype)
    with torch.no_grad():
        inp = frontend_input(x16, win_start, dtype)
        spec = F.conv1d(inp[:, None, :], t("stft.forward_basis_buffer"), stride=128)      # [n, 258, 4]
        y = torch.sqrt(spec[:, :129] ** 2 + spec[:, 129:] ** 2)
        for layer, stride in ((0, 1), (1, 2), (2, 2), (3, 1)):
            y = F.relu(F.conv1d(y, t(f"encoder.{layer}.reparam_conv.weight"), t(f"encoder.{layer}.reparam_conv.bias"), padding=1, stride=stride))
        feat = y[:, :, 0]                                                                   # [n, 128]
        gates = F.linear(feat, t("decoder.rnn.weight_ih"), t("decoder.rnn.bias_ih")) + t("decoder.rnn.bias_hh")
    return gates.numpy()


def lstm(weights, gates_x, seg_first, seg_count, dtype=torch.float64) -> np.ndarray:
    """h [n, 128]: LSTMCell (gate order i, f, g, o) over windows seg_first[s] .. + seg_count[s] of every chunk s, state zero at the
    chunk's first window.  Rows no chunk owns stay NaN."""
    gx = _in(gates_x, dtype)
    whh = _t(weights, "decoder.rnn.weight_hh", dtype)
    out = torch.full((gx.shape[0], HIDDEN), float("nan"), dtype=dtype)
    with torch.no_grad():
        for first, count in zip(np.asarray(seg_first).tolist(), np.asarray(seg_count).tolist()):
            h = torch.zeros(HIDDEN, dtype=dtype); c = torch.zeros(HIDDEN, dtype=dtype)
            for w in range(first, first + count):
                i, f, g, o = (gx[w] + whh @ h).chunk(4)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                out[w] = h
    return out.numpy()


def out(weights, h, dtype=torch.float64) -> np.ndarray:
    """probs [n] = sigmoid(bias + weight . relu(h))."""
    hh = _in(h, dtype)
    with torch.no_grad():
        logit = F.relu(hh) @ _t(weights, "decoder.decoder.2.weight", dtype).reshape(HIDDEN) + _t(weights, "decoder.decoder.2.bias", dtype)[0]
        return torch.sigmoid(logit).numpy()


def chain(weights, x16, win_start, seg_first, seg_count, dtype=torch.float64) -> np.ndarray:
    """The three stages in one precision, each fed with the previous one's unrounded result."""
    return out(weights, lstm(weights, frontend(weights, x16, win_start, dtype), seg_first, seg_count, dtype), dtype)
