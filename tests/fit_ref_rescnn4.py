"""TEST INFRASTRUCTURE: the training step of rescnn4 restated in torch on the CPU, in float64 (the yardstick) or float32
(its own error is the scale the device is judged by).  The reference has no CNN, so this file is the definition: the
recipe of tests/fit_ref.py (the Keras step of the MLP) applied to the network of corintho_ai_amd/nets.py:

  * every conv + bias -> BatchNorm -> ReLU (the stem, both convolutions of the four blocks, the two 1x1 head
    convolutions) normalises, in training mode, with the batch mean and the BIASED batch variance per channel over all
    B x 16 (row, pixel) pairs, epsilon 1e-3; a block adds its input to the second BatchNorm's output before the ReLU;
    the dense layers have no BatchNorm.  Inference mode uses the moving statistics (tests/ref_nets.rescnn4_forward_f64);
  * the 11 BatchNorms' moving statistics move by moving -= (moving - batch_stat) * 0.01;
  * loss = mean (tanh v - z)^2 + 0.25 * mean(-sum t log_softmax(logits)), and Adam = TF ResourceApplyAdam, as fit_ref.
Weights, gradients and Adam's slots use the flat layout of nets._rescnn4_shapes().  RefBackend drives
corintho_ai_amd.fit.fit(..., net=NET_RESCNN4) with it."""
import numpy as np
import torch
import torch.nn.functional as F

from corintho_ai_amd import nets
from tests.fit_ref import ADAM_EPS, B1, B2, MOMENTUM, losses, synthetic_samples  # noqa: F401

# the BatchNorms in the order of the layout (and of the batch statistics forward() returns)
BN_PREFIXES = ["stem"] + ["b%d_c%d" % (b, c) for b in range(nets.RES_BLOCKS) for c in (1, 2)] + ["p", "v"]


def offsets():
    """{name: (flat offset, shape)} of every array of the layout"""
    out, p = {}, 0
    for name, shape in nets._rescnn4_shapes():
        out[name] = (p, shape)
        p += int(np.prod(shape))
    assert p == nets.RESCNN4_NUM_WEIGHTS
    return out


def _slice(off, name):
    p, shape = off[name]
    return slice(p, p + int(np.prod(shape)))


def stat_mask():
    """True at the moving statistics (not trained by Adam)"""
    off = offsets()
    m = np.zeros(nets.RESCNN4_NUM_WEIGHTS, bool)
    for pre in BN_PREFIXES:
        m[_slice(off, pre + "_bn2")] = True
        m[_slice(off, pre + "_bn3")] = True
    return m


def tensors():
    """[(name, slice, slice of the tensor its gradient's scale is taken from)] of every trainable tensor.  A bias that
    feeds a training-mode BatchNorm has the gradient 0 exactly; its scale is that BatchNorm's beta gradient."""
    off = offsets()
    out = []
    for name, _ in nets._rescnn4_shapes():
        if name.endswith("_bn2") or name.endswith("_bn3"):
            continue
        pre = name[:-2]
        scale = pre + "_bn1" if name.endswith("_b") and pre in BN_PREFIXES else name
        out.append((name, _slice(off, name), _slice(off, scale)))
    return out


def _unpack(wt):
    return {name: wt[p:p + int(np.prod(shape))].view(*shape) for name, (p, shape) in offsets().items()}


def _planes(x):
    """[B, 70] -> NCHW [B, 10, 4, 4] (nets.rescnn4_input_planes)"""
    n = x.shape[0]
    board = x[:, :64].reshape(n, 16, 4)
    res = x[:, None, 64:70].expand(n, 16, 6)
    return torch.cat([board, res], 2).reshape(n, 4, 4, nets.RES_CIN).permute(0, 3, 1, 2)


def forward(wt, x, train=True):
    """wt: flat tensor (any dtype), x [B, 70].  Returns logits [B, 96], v [B] (pre-tanh) and aux = {"stats": the 11
    (mean, biased variance) batch statistics in BN_PREFIXES order (train) or None, "relu_inputs": every ReLU's input}"""
    W = _unpack(wt)
    stats, pre_relu = [], []

    def conv(t, prefix, pad):
        k = W[prefix + "_k"]
        if k.dim() == 2:
            k = k.view(1, 1, *k.shape)
        return F.conv2d(t, k.permute(3, 2, 0, 1), W[prefix + "_b"], padding=pad)  # HWIO -> OIHW

    def bn(z, prefix):
        if train:
            m = z.mean((0, 2, 3))
            var = ((z - m.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
            stats.append((m, var))
        else:
            m, var = W[prefix + "_bn2"], W[prefix + "_bn3"]
        xh = (z - m.view(1, -1, 1, 1)) * torch.rsqrt(var.view(1, -1, 1, 1) + nets.BN_EPS)
        return W[prefix + "_bn0"].view(1, -1, 1, 1) * xh + W[prefix + "_bn1"].view(1, -1, 1, 1)

    def relu(t):
        pre_relu.append(t)
        return torch.relu(t)

    h = relu(bn(conv(_planes(x), "stem", 1), "stem"))
    for b in range(nets.RES_BLOCKS):
        y = relu(bn(conv(h, "b%d_c1" % b, 1), "b%d_c1" % b))
        y = bn(conv(y, "b%d_c2" % b, 1), "b%d_c2" % b)
        h = relu(h + y)
    p = relu(bn(conv(h, "p", 0), "p"))
    p = p.permute(0, 2, 3, 1).reshape(p.shape[0], 64)  # pixel * 4 + channel
    logits = p @ W["p_dk"] + W["p_db"]
    v = relu(bn(conv(h, "v", 0), "v"))
    v = v.permute(0, 2, 3, 1).reshape(v.shape[0], 32)  # pixel * 2 + channel
    v = relu(v @ W["v_d1k"] + W["v_d1b"])
    v = (v @ W["v_d2k"]).view(-1) + W["v_d2b"]
    return logits, v, {"stats": stats if train else None, "relu_inputs": pre_relu}


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def loss_and_grad(w, states, evals, probs, dtype=torch.float64):
    """(flat gradient of value + 0.25 policy, (total, value, policy), batch statistics) for one batch, train mode"""
    wt = _t(w, dtype).clone().requires_grad_(True)
    logits, v, aux = forward(wt, _t(states, dtype), True)
    lv, lp = losses(logits, v, _t(evals, dtype), _t(probs, dtype))
    loss = lv + 0.25 * lp
    loss.backward()
    g = wt.grad.detach().numpy().copy()
    g[stat_mask()] = 0.0
    st = [(m.detach().numpy(), s.detach().numpy()) for m, s in aux["stats"]]
    return g, (float(loss.detach()), float(lv.detach()), float(lp.detach())), st


def kink_margin(w, states):
    """smallest |ReLU input| / its tensor's largest, over the batch in float64 (training mode): where it is tiny a ReLU
    sits at its kink, the gradient is not defined there, and float32 rounding picks either side"""
    with torch.no_grad():
        _, _, aux = forward(_t(w, torch.float64), _t(states, torch.float64), True)
    return min(float(t.abs().min() / t.abs().max()) for t in aux["relu_inputs"])


def evaluate(w, states, evals, probs, dtype=torch.float64):
    """inference mode (moving statistics): (total, value, policy) means and the outputs (tanh v, softmax)"""
    with torch.no_grad():
        logits, v, _ = forward(_t(w, dtype), _t(states, dtype), False)
        lv, lp = losses(logits, v, _t(evals, dtype), _t(probs, dtype))
        return (float(lv + 0.25 * lp), float(lv), float(lp)), (torch.tanh(v).numpy(), torch.softmax(logits, 1).numpy())


def adam_step(w, m, v, g, iterations, lr, stats, np_dtype=np.float64):
    """one step in place of (w, m, v): Adam on the trainable weights, the moving statistics toward `stats`"""
    t = iterations + 1
    f = np_dtype
    lr_t = f(lr) * np.sqrt(f(1) - f(B2) ** f(t)) / (f(1) - f(B1) ** f(t))
    mask = ~stat_mask()
    gg = g.astype(f)
    m[mask] = m[mask] + (gg[mask] - m[mask]) * (f(1) - f(B1))
    v[mask] = v[mask] + (gg[mask] * gg[mask] - v[mask]) * (f(1) - f(B2))
    w[mask] = w[mask] - lr_t * m[mask] / (np.sqrt(v[mask]) + f(ADAM_EPS))
    off = offsets()
    for pre, (bm, bv) in zip(BN_PREFIXES, stats):
        for name, bs in ((pre + "_bn2", bm), (pre + "_bn3", bv)):
            sl = _slice(off, name)
            w[sl] = w[sl] - (w[sl] - bs.astype(f)) * f(1 - MOMENTUM)
    return t


class RefBackend:
    """the Fitter interface of corintho_ai_amd.fit for rescnn4, computed by this restatement (float64 by default)"""

    def __init__(self, dtype=torch.float64):
        self.dtype = dtype
        self.np_dtype = np.float64 if dtype == torch.float64 else np.float32
        self.trained_rows = []  # the row order of every train() call
        self.lrs = []

    def set_weights(self, w):
        self.w = np.asarray(w, self.np_dtype).copy()

    def get_weights(self):
        return self.w.astype(np.float32)

    def set_optimizer(self, m, v, iterations):
        self.m = np.asarray(m, self.np_dtype).copy()
        self.v = np.asarray(v, self.np_dtype).copy()
        self.it = int(iterations)

    def get_optimizer(self):
        return self.m.astype(np.float32), self.v.astype(np.float32), self.it

    def set_data(self, s, e, p):
        self.data = (np.asarray(s), np.asarray(e), np.asarray(p))

    def train(self, rows, batch_size, lr, batch_losses=False):
        rows = np.asarray(rows)
        self.trained_rows.append(rows.copy())
        self.lrs.append(float(lr))
        s, e, p = self.data
        tot = np.zeros(3)
        per = []
        for b0 in range(0, rows.size, batch_size):
            r = rows[b0:b0 + batch_size]
            g, ls, st = loss_and_grad(self.w, s[r], e[r], p[r], self.dtype)
            self.it = adam_step(self.w, self.m, self.v, g, self.it, lr, st, self.np_dtype)
            per.append(ls)
            tot += np.asarray(ls) * r.size
        out = tuple(tot / rows.size)
        return (out, np.asarray(per)) if batch_losses else out

    def evaluate(self, row0, n_rows, batch_size):
        s, e, p = self.data
        tot = np.zeros(3)
        for b0 in range(row0, row0 + n_rows, batch_size):
            b1 = min(b0 + batch_size, row0 + n_rows)
            ls, _ = evaluate(self.w, s[b0:b1], e[b0:b1], p[b0:b1], self.dtype)
            tot += np.asarray(ls) * (b1 - b0)
        return tuple(tot / n_rows)

    def close(self):
        pass
