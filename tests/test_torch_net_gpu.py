"""corintho_ai_amd.torch_net.TorchNet: a torch-ROCm module as the network of fused mode, called inside run() on the
run's streams, on device tensors.

The module is built from element-wise operations only -- for each of the 70 columns acc = acc + x[:, j:j+1] * w[j], the
multiply and the add separate operations, so nothing can contract them into a fused multiply-add -- which makes it
batch-invariant by construction and lets float32 numpy arithmetic on the host reproduce it exactly.  The yardstick is
oracle.Trainer under the plain protocol, driven with that numpy twin.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # before the engine is loaded: one HIP runtime in the process (corintho_ai_amd/torch_net.py)

from oracle import oracle as O
from tests import harness as H
from tests.engines import make_trainer

GS, NM = H.GS, H.NM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = np.random.default_rng(2024).uniform(-1.0, 1.0, (GS, 1 + NM)).astype(np.float32)


def numpy_twin(states):
    acc = np.zeros((states.shape[0], 1 + NM), np.float32)
    for j in range(GS):
        acc = acc + states[:, j:j + 1] * W[j]
    return np.clip(acc[:, 0], np.float32(-1.0), np.float32(1.0)), np.abs(acc[:, 1:]) + np.float32(2.0 ** -10)


def torch_module():
    class Columns(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("w", torch.from_numpy(W))

        def forward(self, x):
            acc = torch.zeros((x.shape[0], 1 + NM), dtype=torch.float32, device=x.device)
            for j in range(GS):
                acc = acc + x[:, j:j + 1] * self.w[j]
            return torch.clamp(acc[:, 0], -1.0, 1.0), torch.abs(acc[:, 1:]) + 2.0 ** -10

    return Columns().to("cuda").eval()


def test_the_package_does_not_import_torch():
    """importing corintho_ai_amd alone leaves torch out (a fresh child process: this one has it already)"""
    code = "import sys; import corintho_ai_amd; import corintho_ai_amd.net; sys.exit(1 if 'torch' in sys.modules else 0)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


@pytest.fixture(scope="module")
def oracle_run():
    G, S_, spe = 8, 30, 4
    o = O.Trainer(G, seed=7, max_searches=S_, searches_per_eval=spe, num_threads=4)
    o.enable_trace()
    o.set_stagger(False)
    H.play_generation(o, G, spe, numpy_twin)
    return {"samples": [x.tobytes() for x in H.get_samples(o)], "traces": [o.trace(g).tobytes() for g in range(G)],
            "score": o.score(), "num_samples": o.num_samples()}


@pytest.mark.gpu
def test_the_twin_is_exact():
    """the premise: the module's outputs are the numpy twin's, bit for bit, in batches of different sizes"""
    model = torch_module()
    s = (np.random.default_rng(1).integers(0, 5, (67, GS)) / 4.0).astype(np.float32)
    e, p = numpy_twin(s)
    with torch.inference_mode():
        for n in (67, 1):
            v, q = model(torch.from_numpy(s[:n]).cuda())
            assert v.cpu().numpy().tobytes() == e[:n].tobytes() and q.cpu().numpy().tobytes() == p[:n].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("pools", [1, 3])
def test_torch_module_inside_the_run(pools, oracle_run):
    from corintho_ai_amd.torch_net import TorchNet

    G, S_, spe = 8, 30, 4
    t = make_trainer("hip", G, "", 7, S_, spe, 1.0, 0.25, 0, 1, False, trace=True, stagger=False, pools=pools)
    net = TorchNet(torch_module(), t)
    assert net.states.shape == (G * spe, GS) and net.evals.shape == (G * spe,) and net.probs.shape == (G * spe, NM)
    assert t.run()
    assert net.calls > 0 and net.rows_asked >= t.stats()["nn_rows"]
    assert t.num_samples() == oracle_run["num_samples"] and t.score() == oracle_run["score"]
    for x, y in zip(H.get_samples(t), oracle_run["samples"]):
        assert x.tobytes() == y, "samples differ from the oracle's"
    for g in range(G):
        assert t.trace(g).tobytes() == oracle_run["traces"][g], "per-ply trace of game %d" % g
