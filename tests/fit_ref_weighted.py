"""TEST INFRASTRUCTURE: the training step with per-sample weights under the reference's loss, as the tests of the
weighted kernels call it: tests/fit_ref_step.py's step with LossOptions' defaults (tests/fit_ref_loss.py has the loss and
what the weights mean).  ref: tests/fit_ref.py (mlp12x100) or tests/fit_ref_rescnn4.py (rescnn4)."""
import torch

from tests import fit_ref_step as S
from tests.fit_ref_step import kink_margin  # noqa: F401


def loss_and_grad(ref, w, states, evals, probs, sample_weight, dtype=torch.float64):
    """(flat gradient of value + 0.25 policy, (total, value, policy)) of one batch in training mode"""
    return S.loss_and_grad(ref, w, states, evals, probs, None, sample_weight, dtype)[:2]


def evaluate(ref, w, states, evals, probs, sample_weight, dtype=torch.float64):
    """inference mode (moving statistics): the (total, value, policy) weighted losses of one batch"""
    return S.evaluate(ref, w, states, evals, probs, None, sample_weight, dtype)[0]


def tensors(ref):
    """[(name, slice, slice of the tensor the gradient's scale is taken from)] of every trainable tensor of either network"""
    return ref.tensors()
