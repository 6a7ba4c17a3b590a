"""TEST INFRASTRUCTURE: what is particular to rescnn4 in the restatement of the training step (tests/fit_ref_step.py has
the step, for this network and for tests/fit_ref.py's): the forward in torch on the CPU, in any dtype, and where the
layout keeps what.  The reference has no CNN, so this file is the definition: the recipe of the Keras step of the MLP
applied to the network of corintho_ai_amd/nets.py:

  * every conv + bias -> BatchNorm -> ReLU (the stem, both convolutions of the four blocks, the two 1x1 head
    convolutions) normalises, in training mode, with the batch mean and the BIASED batch variance per channel over all
    B x 16 (row, pixel) pairs, epsilon 1e-3; a block adds its input to the second BatchNorm's output before the ReLU;
    the dense layers have no BatchNorm.  Inference mode uses the moving statistics (tests/ref_nets.rescnn4_forward_f64);
Weights, gradients and Adam's slots use the flat layout of nets._rescnn4_shapes()."""
import numpy as np
import torch
import torch.nn.functional as F

from corintho_ai_amd import nets
from tests.fit_ref import synthetic_samples  # noqa: F401

NET = "rescnn4"
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


def bn_slices():
    """[(moving mean, moving variance)] as slices, in the order of the batch statistics forward() returns"""
    off = offsets()
    return [(_slice(off, pre + "_bn2"), _slice(off, pre + "_bn3")) for pre in BN_PREFIXES]


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
