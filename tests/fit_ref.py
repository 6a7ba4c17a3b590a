"""TEST INFRASTRUCTURE: what is particular to mlp12x100 in the restatement of the reference's Keras training step
(tests/fit_ref_step.py has the step, for this network and for tests/fit_ref_rescnn4.py's): the forward in torch on the CPU,
in any dtype, and where the layout keeps what.

  * BatchNorm, training mode: batch mean and BIASED batch variance, gamma (a - mean) rsqrt(var + 1e-3) + beta (Keras's
    non-fused rank-2 path; torch's BatchNorm1d keeps the unbiased variance, so it is not used)."""
import numpy as np
import torch

from corintho_ai_amd import nets

NET = "mlp12x100"
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


def bn_slices():
    """[(moving mean, moving variance)] as slices, in the order of the batch statistics forward() returns"""
    return [(slice(mu, mu + 100), slice(va, va + 100)) for (_, _, _, _, mu, va, _) in layer_offsets()[0]]


def tensors():
    """[(name, slice, slice of the tensor the gradient's scale is taken from)] of every trainable tensor"""
    lay, (kv, bv, kp, bp) = layer_offsets()
    out = []
    for i, (k, b, g, be, _, _, fi) in enumerate(lay):
        out += [("k%d" % i, slice(k, k + fi * 100)), ("b%d" % i, slice(b, b + 100)), ("gamma%d" % i, slice(g, g + 100)),
                ("beta%d" % i, slice(be, be + 100))]
    out += [("kv", slice(kv, kv + 100)), ("bv", slice(bv, bv + 1)), ("kp", slice(kp, kp + 9600)), ("bp", slice(bp, bp + 96))]
    return [(name, sl, sl) for name, sl in out]


def forward(wt, x, train=True):
    """wt: flat tensor (any dtype), x [B, 70].  Returns logits [B, 96], v [B] (pre-tanh) and aux = {"stats": the 12
    layers' (mean, biased variance) batch statistics (train) or None, "relu_inputs": every ReLU's input}"""
    lay, (kv, bv, kp, bp) = layer_offsets()
    stats, pre_relu = [], []
    h = x
    for (k, b, g, be, mu, va, fi) in lay:
        pre_relu.append(h @ wt[k:k + fi * 100].view(fi, 100) + wt[b:b + 100])
        a = torch.relu(pre_relu[-1])
        if train:
            m = a.mean(0)
            var = ((a - m) ** 2).mean(0)
            stats.append((m, var))
        else:
            m, var = wt[mu:mu + 100], wt[va:va + 100]
        h = wt[g:g + 100] * ((a - m) * torch.rsqrt(var + nets.BN_EPS)) + wt[be:be + 100]
    logits = h @ wt[kp:kp + 9600].view(100, 96) + wt[bp:bp + 96]
    v = (h @ wt[kv:kv + 100].view(100, 1)).view(-1) + wt[bv]
    return logits, v, {"stats": stats if train else None, "relu_inputs": pre_relu}


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
