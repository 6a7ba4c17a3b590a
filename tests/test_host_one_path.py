"""The host engine's single paths: the three ways samples leave a trainer give the same rows, net_bench widens the
caller's 70-float rows on the device like net_forward, a tournament reports a network it cannot build with the
code a trainer reports (CA_ERR_ARG), and one trainer gives the same generation through each of its protocols in turn."""
import numpy as np
import pytest
import torch  # before the engine is loaded: the process then holds ONE HIP runtime, torch's (corintho_ai_amd/torch_net.py)

from corintho_ai_amd import Tourney, _lib, nets
from corintho_ai_amd import trainer as T
from tests import harness as H
from tests.engines import ENGINES, cdll, make_trainer

SAMPLE_FLOATS = T.GAME_STATE_SIZE + T.NUM_MOVES


def _packed_on_device(engine, t, n):
    """the rows pack_samples_device writes into caller memory of n rows: a numpy buffer stands for device memory on the
    emulation build, a torch tensor holds it on the device"""
    if engine == "emu":
        sp, oc = np.full((n, SAMPLE_FLOATS), -7.0, np.float32), np.full(n, -7.0, np.float32)
        assert t.pack_samples_device(sp.ctypes.data, oc.ctypes.data, n) == n
        return sp, oc
    sp = torch.full((n, SAMPLE_FLOATS), -7.0, dtype=torch.float32, device="cuda:0")
    oc = torch.full((n,), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert t.pack_samples_device(sp.data_ptr(), oc.data_ptr(), n) == n
    return sp.cpu().numpy(), oc.cpu().numpy()


def _assert_sample_exits_agree(engine, t):
    n = t.num_samples()
    assert n > 0
    sp, oc = t.export_samples()
    assert sp.shape == (n, SAMPLE_FLOATS) and oc.shape == (n,)
    dsp, doc = _packed_on_device(engine, t, n)
    assert sp.tobytes() == dsp.tobytes() and oc.tobytes() == doc.tobytes()
    # ... and, through another kernel with its own use of the offset index: expanded x8 they are writeSamples' arrays
    for x, y in zip(T.expand_samples(sp, oc, _cdll=cdll(engine)), H.get_samples(t)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("engine", ENGINES)
def test_sample_exits_agree(engine):
    """10 games on 4 resident slots, stopped in mid-generation and at the end: at every stop export_samples ==
    pack_samples_device, and expanded x8 == writeSamples, byte for byte.  The games that have not started are blocks of
    zero rows behind the others: where the offset index can go wrong.  After run(max_iterations=20) the four resident games are two
    plies old (measured: samples per game [2, 2, 2, 2, 0, 0, 0, 0, 0, 0], none done -- a ply of 50 simulations takes seven
    iterations of 8), so the generation is stopped a third time, the first time a game has ended while another has yet
    to start: finished, running and unstarted games side by side."""
    G = 10
    t = make_trainer(engine, G, "", 7, 50, 8, 1.0, 0.25, 0, 1, False, stagger=False, resident=4)
    t.set_net(T.NET_MLP12X100, nets.init_mlp12x100(seed=3, bn_noise=True))

    def per_game(key):
        return [t.game_info(g)[key] for g in range(G)]

    assert not t.run(max_iterations=20)
    print("samples per game after 20 iterations:", per_game("n_samples"), "done:", per_game("done"))
    assert 0 in per_game("n_samples") and max(per_game("n_samples")) > 0  # zero-length blocks beside filled ones
    _assert_sample_exits_agree(engine, t)
    while not any(per_game("done")):
        assert not t.run(max_iterations=20)
    print("samples per game at the first finished game:", per_game("n_samples"), "done:", per_game("done"))
    assert 0 in per_game("n_samples") and not all(per_game("done"))
    _assert_sample_exits_agree(engine, t)
    assert t.run()
    _assert_sample_exits_agree(engine, t)


@pytest.mark.parametrize("engine", ENGINES)
def test_net_bench_takes_rows_as_the_caller_holds_them(engine):
    """33 rows of 70 floats (not a whole wavefront of floats: 2310 = 36 x 64 + 6) in a trainer of 4 games x 16"""
    t = make_trainer(engine, 4, "", 1, 32, 16, 1.0, 0.25, 0, 1, False)
    t.set_net(T.NET_MLP12X100, nets.init_mlp12x100(seed=4, bn_noise=True))
    rows = np.random.default_rng(5).integers(0, 5, (33, T.GAME_STATE_SIZE)).astype(np.float32) / 4.0
    ev0, pr0 = t.net_forward(rows)
    assert np.all(np.isfinite(ev0)) and np.all(np.abs(pr0.sum(axis=1) - 1.0) < 1e-3)
    ms = t.net_bench(rows, reps=2)
    assert ms > 0.0 if engine == "hip" else ms >= 0.0  # (the emulation build has no clock)
    ev1, pr1 = t.net_forward(rows)
    assert ev0.tobytes() == ev1.tobytes() and pr0.tobytes() == pr1.tobytes()
    # ... and it leaves the protocol's request rows alone: the same batch before and after it
    cap = 4 * 16
    assert not t.doIteration(np.zeros(cap, np.float32), np.zeros((cap, T.NUM_MOVES), np.float32))
    n = t.num_requests()
    before, after = np.zeros((cap, T.GAME_STATE_SIZE), np.float32), np.zeros((cap, T.GAME_STATE_SIZE), np.float32)
    t.writeRequests(before)
    t.net_bench(rows, reps=1)
    t.writeRequests(after)
    assert n > 0 and before[:n].any() and before.tobytes() == after.tobytes()


@pytest.mark.parametrize("engine", ENGINES)
def test_one_trainer_through_its_modes(engine, tmp_path):
    """ONE trainer (10 games on 4 slots, the first two logged), three generations of seed 5: A fused (run), B driven by
    the host through the evaluation cache with the trainer's own net_forward as the caller's network, C fused again
    after the cache is switched off.  Each hand-over rebuilds what the launches are given (pools, table, the pending
    leaves' cache words, the logs' records), so: the samples and both log files of B and of C are A's, byte for byte.
    (B = A rests on a row's outputs not depending on its batch: tests/test_net_precision.py.)"""
    G, R, spe = 10, 4, 8
    t = make_trainer(engine, G, str(tmp_path), 5, 50, spe, 1.0, 0.25, 2, 1, False, stagger=False, resident=R)
    t.set_net(T.NET_MLP12X100, nets.init_mlp12x100(3, bn_noise=True))
    logs = [tmp_path / "game_0.txt", tmp_path / "game_1.txt"]

    def harvest():
        """what the generation left: its samples and log files (taken away, so that the next one has to write them)"""
        sp, oc = t.export_samples()
        out = (sp.tobytes(), oc.tobytes()) + tuple(f.read_bytes() for f in logs)
        for f in logs:
            f.unlink()
        return out

    assert t.run()
    a = harvest()
    print("generation A: %d sample rows, logs of %d and %d bytes" % (t.num_samples(), len(a[2]), len(a[3])))
    assert t.num_samples() > 0 and len(a[2]) > 0 and len(a[3]) > 0

    t.reset(5)
    t.set_host_cache(6)
    cap = R * spe
    gs = np.zeros((cap, T.GAME_STATE_SIZE), np.float32)
    ev, pr = np.zeros(cap, np.float32), np.zeros((cap, T.NUM_MOVES), np.float32)
    calls = 0
    while not t.doIteration(ev, pr, -1):
        calls += 1
        assert calls < 10 ** 5, "the host-driven generation did not end"
        n = t.num_requests(-1)
        assert 0 <= n <= cap
        if n:
            t.writeRequests(gs, -1)
            t.net_forward(gs[:n], out_evals=ev, out_probs=pr)
    b = harvest()

    t.reset(5)
    t.set_host_cache(False)
    assert t.run()
    c = harvest()
    assert c == a, "the fused generation after the host-driven one differs from the first"
    assert b == a, "the host-driven generation differs from the fused ones"


def _one_match(engine):
    t = Tourney(1, "", _cdll=cdll(engine))
    t.addPlayer(0, 0, 8, 4, 1.0, 0.25, False)
    t.addPlayer(1, 0, 8, 4, 1.0, 0.25, False)
    t.addMatch(0, 1, False)
    return t


def test_tourney_unknown_net_kind_is_an_argument_error():
    t = _one_match("emu")
    t.set_net(0, 99, nets.init_mlp12x100(seed=1))
    with pytest.raises(_lib.EngineError, match=r"error -1.*unknown net kind"):
        t.run()


@pytest.mark.gpu
def test_tourney_out_of_range_f16_weights_are_an_argument_error():
    """as a trainer's set_net reports them (CA_ERR_ARG), not as a device error"""
    w = nets.init_mlp12x100(seed=1).copy()
    w[0] = 1e6
    t = _one_match("hip")
    t.set_net(0, T.NET_MLP12X100_H3, w)
    with pytest.raises(_lib.EngineError) as info:
        t.run()
    assert "error -1" in str(info.value) and "fp16 range" in str(info.value)
