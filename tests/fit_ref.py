"""TEST INFRASTRUCTURE: the reference's Keras training step for mlp12x100 restated in torch on the CPU, in float64 (the
yardstick) or float32 (its own error is the scale the device is judged by).  Written from tf.keras 2.x, one comment per
point of what it does (corintho_ai_amd/fit.py; wrapper.py:256-282, main.pyx:249-260):

  * BatchNorm, training mode: batch mean and BIASED batch variance, gamma (a - mean) rsqrt(var + 1e-3) + beta; the moving
    statistics move by moving -= (moving - batch_stat) * 0.01 (Keras's non-fused rank-2 path; torch's BatchNorm1d keeps
    the unbiased variance, so it is not used);
  * loss = mean (tanh v - z)^2 + 0.25 * mean(-sum t log_softmax(logits))  (cross-entropy from the logits);
  * Adam = TF ResourceApplyAdam: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), m += (g - m)(1 - b1), v += (g^2 - v)(1 - b2),
    w -= lr_t m / (sqrt(v) + 1e-7); kernels, biases, gamma and beta only.
Gradients come from autograd.  RefBackend drives corintho_ai_amd.fit.fit() with it."""
import numpy as np
import torch

from corintho_ai_amd import nets

B1, B2, ADAM_EPS, MOMENTUM = 0.9, 0.999, 1e-7, 0.99
LAYERS = 12


def layer_offsets():
    """[(kernel, bias, gamma, beta, mean, var, in_dim) per layer], (Kv, bv, Kp, bp) as flat offsets"""
    out, p, fan_in = [], 0, nets.GAME_STATE_SIZE
    for _ in range(LAYERS):
        k = p
        b = k + fan_in * 100
        out.append((k, b, b + 100, b + 200, b + 300, b + 400, fan_in))
        p = b + 500
        fan_in = 100
    return out, (p, p + 100, p + 101, p + 101 + 9600)


def stat_mask():
    """True at the moving statistics (not trained by Adam)"""
    m = np.zeros(nets.MLP_NUM_WEIGHTS, bool)
    for (_, _, _, _, mu, va, _) in layer_offsets()[0]:
        m[mu:mu + 100] = True
        m[va:va + 100] = True
    return m


def forward(wt, x, train=True):
    """wt: flat tensor (any dtype), x [B, 70].  Returns logits [B, 96], v [B] (pre-tanh) and the batch statistics
    [(mean, biased var)] of the 12 layers (train) or None."""
    lay, (kv, bv, kp, bp) = layer_offsets()
    stats = []
    h = x
    for (k, b, g, be, mu, va, fi) in lay:
        a = torch.relu(h @ wt[k:k + fi * 100].view(fi, 100) + wt[b:b + 100])
        if train:
            m = a.mean(0)
            var = ((a - m) ** 2).mean(0)
            stats.append((m, var))
        else:
            m, var = wt[mu:mu + 100], wt[va:va + 100]
        h = wt[g:g + 100] * ((a - m) * torch.rsqrt(var + nets.BN_EPS)) + wt[be:be + 100]
    logits = h @ wt[kp:kp + 9600].view(100, 96) + wt[bp:bp + 96]
    v = (h @ wt[kv:kv + 100].view(100, 1)).view(-1) + wt[bv]
    return logits, v, (stats if train else None)


def losses(logits, v, z, t):
    """(value MSE, policy cross-entropy from the logits), each a mean over the rows"""
    lv = ((torch.tanh(v) - z) ** 2).mean()
    lp = (-(t * torch.log_softmax(logits, dim=1)).sum(1)).mean()
    return lv, lp


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def loss_and_grad(w, states, evals, probs, dtype=torch.float64):
    """(flat gradient of value + 0.25 policy, (total, value, policy), batch statistics) for one batch, train mode"""
    wt = _t(w, dtype).clone().requires_grad_(True)
    logits, v, stats = forward(wt, _t(states, dtype), True)
    lv, lp = losses(logits, v, _t(evals, dtype), _t(probs, dtype))
    loss = lv + 0.25 * lp
    loss.backward()
    g = wt.grad.detach().numpy().copy()
    g[stat_mask()] = 0.0
    st = [(m.detach().numpy(), s.detach().numpy()) for m, s in stats]
    return g, (float(loss.detach()), float(lv.detach()), float(lp.detach())), st


def evaluate(w, states, evals, probs, dtype=torch.float64):
    """inference mode (moving statistics): (total, value, policy) means and the outputs (tanh v, softmax)"""
    with torch.no_grad():
        logits, v, _ = forward(_t(w, dtype), _t(states, dtype), False)
        lv, lp = losses(logits, v, _t(evals, dtype), _t(probs, dtype))
        return (float(lv + 0.25 * lp), float(lv), float(lp)), (torch.tanh(v).numpy(), torch.softmax(logits, 1).numpy())


def adam_step(w, m, v, g, iterations, lr, stats, np_dtype=np.float64):
    """one Keras step in place of (w, m, v): Adam on the trainable weights, the moving statistics toward `stats`"""
    t = iterations + 1
    f = np_dtype
    lr_t = f(lr) * np.sqrt(f(1) - f(B2) ** f(t)) / (f(1) - f(B1) ** f(t))
    mask = ~stat_mask()
    gg = g.astype(f)
    m[mask] = m[mask] + (gg[mask] - m[mask]) * (f(1) - f(B1))
    v[mask] = v[mask] + (gg[mask] * gg[mask] - v[mask]) * (f(1) - f(B2))
    w[mask] = w[mask] - lr_t * m[mask] / (np.sqrt(v[mask]) + f(ADAM_EPS))
    lay, _ = layer_offsets()
    for (_, _, _, _, mu, va, _), (bm, bv) in zip(lay, stats):
        for off, bs in ((mu, bm), (va, bv)):
            w[off:off + 100] = w[off:off + 100] - (w[off:off + 100] - bs.astype(f)) * f(1 - MOMENTUM)
    return t


class RefBackend:
    """the Fitter interface of corintho_ai_amd.fit, computed by this restatement (float64 by default)"""

    def __init__(self, dtype=torch.float64):
        self.dtype = dtype
        self.np_dtype = np.float64 if dtype == torch.float64 else np.float32
        self.trained_rows = []  # the row order of every train() call (tests of fit's host logic)

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


def synthetic_samples(n, seed):
    """rows with the shape of self-play samples: binary board bits, reserve counters in quarters, a policy target on
    a random subset of moves summing to 1, values in {-1, 0, 1}"""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, nets.GAME_STATE_SIZE), np.float32)
    s[:, :64] = rng.integers(0, 2, (n, 64))
    s[:, 64:] = rng.integers(0, 5, (n, 6)) * 0.25
    p = rng.random((n, nets.NUM_MOVES)) * (rng.random((n, nets.NUM_MOVES)) < 0.2)
    p[:, 0] += 1e-3
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    z = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), n)
    return s, z.astype(np.float32), p
