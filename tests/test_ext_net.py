"""A caller-supplied network inside the fused run (ca_trainer_set_net_fn / Trainer.set_net_fn, ca_tourney_set_net_fn,
ca_net_*): the library lays a launch's request rows out in the caller's DEVICE buffer, calls the caller's function on the
launch's stream, and scatters the answers the function leaves in the caller's output buffers.

The caller's network is harness.hash_net, a function of the row alone; the yardstick is oracle.Trainer under the plain
protocol with the same network (tests/test_host_cache.py oracle_generation: played once per session, shared, unchanged).

  * emulation build: the "device" buffers are numpy arrays; the function reads them, and the device's row count, through
    ctypes, answers the rows below the count and poisons the answers above it with NaN;
  * hip (-m gpu): the buffers are torch tensors; the function synchronises the stream it is given, evaluates a host copy
    of ALL the rows it is handed with the numpy network and copies the answers back.
"""
import collections
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine is loaded: the process then holds ONE HIP runtime, torch's (corintho_ai_amd/torch_net.py)

from corintho_ai_amd import NET_MLP12X100, NET_MLP12X100_H3, NET_RESCNN4_H3, Tourney, _lib, nets
from corintho_ai_amd.analyse import Analyser
from corintho_ai_amd.net import Net
from oracle import oracle as O
from tests import harness as H
from tests.engines import ENGINES, cdll, make_trainer
from tests.test_host_cache import assert_equals_oracle, oracle_generation

GS, NM = H.GS, H.NM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Call = collections.namedtuple("Call", "row0 cap count rows")


class Buffers:
    """the caller's three buffers of `rows` rows (and one int32), as the engine's device holds memory"""

    def __init__(self, engine, rows):
        self.engine, self.rows = engine, rows
        if engine == "emu":
            self.states = np.zeros((rows, GS), np.float32)
            self.evals = np.zeros(rows, np.float32)
            self.probs = np.zeros((rows, NM), np.float32)
            self.count = np.zeros(1, np.int32)
            self.ptrs = (self.states.ctypes.data, self.evals.ctypes.data, self.probs.ctypes.data)
            self.count_ptr = self.count.ctypes.data
        else:
            self.torch = torch
            self.states = torch.zeros((rows, GS), dtype=torch.float32, device="cuda")
            self.evals = torch.zeros(rows, dtype=torch.float32, device="cuda")
            self.probs = torch.zeros((rows, NM), dtype=torch.float32, device="cuda")
            self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            self.ptrs = (self.states.data_ptr(), self.evals.data_ptr(), self.probs.data_ptr())
            self.count_ptr = self.count.data_ptr()

    def fill(self, states=None, evals=None, probs=None, count=None):
        for name, v in (("states", states), ("evals", evals), ("probs", probs), ("count", count)):
            if v is None:
                continue
            dst = getattr(self, name)
            if self.engine == "emu":
                dst[...] = v
            else:
                dtype = np.int32 if name == "count" else np.float32
                dst.copy_(self.torch.from_numpy(np.array(np.broadcast_to(v, tuple(dst.shape)), dtype=dtype)))
        if self.engine != "emu":
            self.torch.cuda.synchronize()

    def host(self, name):
        a = getattr(self, name)
        return a.copy() if self.engine == "emu" else a.cpu().numpy()


class ExtNet(Buffers):
    """hash_net behind the function of set_net_fn"""

    def __init__(self, engine, rows, salt=0, fail_at=0, inside=None):
        super().__init__(engine, rows)
        self.salt, self.fail_at, self.inside = salt, fail_at, inside
        self.calls = []

    def fn(self, row0, cap, d_rows_ptr, stream_ptr):
        if self.fail_at and len(self.calls) + 1 == self.fail_at:
            self.calls.append(None)
            raise ValueError("the caller's network failed in call %d" % self.fail_at)
        if self.inside is not None:
            self.inside()
        assert 0 <= row0 and cap >= 1 and row0 + cap <= self.rows, (row0, cap, self.rows)
        if self.engine == "emu":
            n = C.c_int32.from_address(d_rows_ptr).value
            rows = self.states[row0:row0 + cap].copy()
            self.calls.append(Call(row0, cap, n, rows))
            assert 0 <= n <= cap
            e, p = H.hash_net(rows[:n], self.salt)
            self.evals[row0:row0 + n] = e
            self.probs[row0:row0 + n] = p
            self.evals[row0 + n:row0 + cap] = np.nan  # answers beyond the count are ignored
            self.probs[row0 + n:row0 + cap] = np.nan
        else:
            torch = self.torch
            torch.cuda.ExternalStream(stream_ptr).synchronize()
            rows = self.states[row0:row0 + cap].cpu().numpy()
            self.calls.append(Call(row0, cap, None, rows))
            e, p = H.hash_net(rows, self.salt)
            self.evals[row0:row0 + cap] = torch.from_numpy(e).cuda()
            self.probs[row0:row0 + cap] = torch.from_numpy(p).cuda()
            torch.cuda.synchronize()

    def install(self, t, slot=0, flop_per_row=0.0):
        t.set_net_fn(self.fn, *self.ptrs, self.rows, slot=slot, flop_per_row=flop_per_row)
        return self


def ext_trainer(engine, G, S_, spe, c_puct, eps, resident=0, pools=1, eval_cache=False, seed=7, **kw):
    t = make_trainer(engine, G, "", seed, S_, spe, c_puct, eps, 0, 1, False, trace=True, stagger=False, resident=resident,
                     pools=pools, eval_cache=eval_cache, **kw)
    return t, ExtNet(engine, t.request_rows()).install(t)


# G, sims, spe, c_puct, eps, resident slots
SHAPES = [
    pytest.param(8, 30, 1, 1.0, 0.0, 0, id="G8-30sims-spe1-eps0"),
    pytest.param(12, 64, 16, 3.0, 0.25, 0, id="G12-64sims-spe16-cpuct3"),
    pytest.param(21, 40, 4, 1.0, 0.25, 5, id="G21-on-5-slots-40sims-spe4"),
]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("eval_cache", [False, 16], ids=["nocache", "cache16"])
@pytest.mark.parametrize("pools", [1, 3])
@pytest.mark.parametrize("G,S_,spe,c_puct,eps,resident", SHAPES)
def test_same_generation(engine, G, S_, spe, c_puct, eps, resident, pools, eval_cache):
    """1. the oracle's generation, byte for byte, whatever the pools and the cache"""
    ref = oracle_generation(G, S_, spe, c_puct, eps, 7, False)
    t, ext = ext_trainer(engine, G, S_, spe, c_puct, eps, resident, pools, eval_cache)
    assert t.request_rows() == (resident or G) * spe
    assert t.run()
    assert_equals_oracle(t, ref, G)
    st = t.stats()
    assert st["nn_rows"] == ref["total_rows"]
    assert st["pools"] == pools
    assert ext.calls, "the caller's function was never called"


@functools.lru_cache(maxsize=None)
def oracle_row_counts(G, S_, spe, c_puct, eps, seed):
    """the oracle's request log as a multiset of rows"""
    o = O.Trainer(G, seed=seed, max_searches=S_, searches_per_eval=spe, c_puct=c_puct, epsilon=eps, num_threads=4)
    o.set_stagger(False)
    r = H.play_generation(o, G, spe, H.hash_net, record=True)
    return collections.Counter(b[i].tobytes() for _, b in r["log"] for i in range(b.shape[0]))


@pytest.mark.parametrize("eval_cache", [False, 16], ids=["nocache", "cache16"])
def test_what_the_function_sees(eval_cache):
    """2. every call's arguments and rows (emulation build: the device's count is readable there)"""
    G, S_, spe, c_puct, eps = 12, 64, 16, 3.0, 0.25
    ref = oracle_generation(G, S_, spe, c_puct, eps, 7, False)
    want = oracle_row_counts(G, S_, spe, c_puct, eps, 7)
    t, ext = ext_trainer("emu", G, S_, spe, c_puct, eps, 0, 3, eval_cache)
    assert t.run()
    assert_equals_oracle(t, ref, G)  # (the answers beyond the count were NaN: nobody read them)
    got = collections.Counter()
    prev_end, prev_row0 = 0, -1
    for c in ext.calls:
        assert 0 <= c.count <= c.cap and c.row0 + c.cap <= ext.rows
        # the pools of one iteration are called in ascending row order: a call that does not start higher than the one
        # before it begins the next iteration
        if c.row0 <= prev_row0:
            prev_end = 0
        prev_row0 = c.row0
        assert c.row0 >= prev_end, "row ranges of one iteration's pools overlap"
        prev_end = c.row0 + c.cap
        assert not c.rows[c.count:].any(), "rows beyond the count are not zero"
        got.update(c.rows[i].tobytes() for i in range(c.count))
    starts = sorted(set(c.row0 for c in ext.calls))
    assert starts == [0, 4 * spe, 8 * spe], "three pools of four games"
    if eval_cache is False:
        assert got == want, "the rows handed to the function are not the oracle's request log"
    else:
        assert set(got) <= set(want)
        assert sum(got.values()) < sum(want.values())
        assert sum(got.values()) == t.stats()["nn_rows_evaluated"]


def _quarter_rows(n, seed):
    return (np.random.default_rng(seed).integers(0, 5, (n, GS)) / 4.0).astype(np.float32)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("n", [1, 3, 64, 257])
def test_gather_and_scatter_edges(engine, n):
    """3a. co_k_host_rows_out / _in with an identity index, strides {1, 96}, at row counts where neither 70 n nor 97 n is
    a multiple of 64: net_forward through an external slot = hash_net of the inputs"""
    t = make_trainer(engine, 17, "", 1, 32, 16, 1.0, 0.25, 0, 1, False)
    ext = ExtNet(engine, t.request_rows(), salt=3).install(t)
    ext.fill(states=-1.0)  # nothing of an earlier call can pass for a row
    s = _quarter_rows(n, n)
    ev, pr = t.net_forward(s)
    e, p = H.hash_net(s, 3)
    assert ev.tobytes() == e.tobytes() and pr.tobytes() == p.tobytes()
    c = ext.calls[-1]
    assert (c.row0, c.cap) == (0, n) and c.rows.tobytes() == s.tobytes()


NET_KINDS = [pytest.param("emu", NET_MLP12X100, id="emu-mlp12x100"),
             pytest.param("hip", NET_MLP12X100_H3, id="hip-mlp12x100-f16x3", marks=pytest.mark.gpu),
             pytest.param("hip", NET_RESCNN4_H3, id="hip-rescnn4-f16x3", marks=pytest.mark.gpu)]


def _weights(kind):
    return nets.init_rescnn4(seed=3, bn_noise=True) if kind == NET_RESCNN4_H3 else nets.init_mlp12x100(seed=1, bn_noise=True)


@pytest.mark.parametrize("engine,kind", NET_KINDS)
def test_net_forward_device(engine, kind):
    """3b. Net.forward_device on 257 rows with a device count of 0, 1 and 257: the rows below the count are
    Trainer.net_forward's of the same weights, the rows above it keep their sentinel"""
    n = 257
    w = _weights(kind)
    t = make_trainer(engine, 17, "", 1, 32, 16, 1.0, 0.25, 0, 1, False)
    t.set_net(kind, w)
    s = _quarter_rows(n, 5)
    ev, pr = t.net_forward(s)
    net = Net(kind, w, n, _cdll=cdll(engine))
    b = Buffers(engine, n)
    for count in (0, 1, n):
        b.fill(states=s, evals=-7.0, probs=-7.0, count=count)
        net.forward_device(b.ptrs[0], n, b.count_ptr, b.ptrs[1], b.ptrs[2])
        e, p = b.host("evals"), b.host("probs")
        assert e[:count].tobytes() == ev[:count].tobytes() and p[:count].tobytes() == pr[:count].tobytes(), count
        assert (e[count:] == -7.0).all() and (p[count:] == -7.0).all(), "rows beyond the count were written (count %d)" % count
    with pytest.raises(_lib.EngineError, match="error -1"):
        net.forward_device(b.ptrs[0], n + 1, b.count_ptr, b.ptrs[1], b.ptrs[2])
    net.close()


@pytest.mark.parametrize("engine,kind", [NET_KINDS[0], NET_KINDS[2]])
@pytest.mark.parametrize("pools,flop_per_row", [(1, 0.0), (3, 1e7)], ids=["1pool-nocache", "3pools-cache"])
def test_library_kernel_through_the_mechanism(engine, kind, pools, flop_per_row):
    """4. the function calls Net.forward_device on the stream it is given: the generation of set_net with the same kind
    and weights, sample for sample (3 pools: flop_per_row turns the automatic evaluation cache on)"""
    G, S_, spe = 12, 64, 16
    w = _weights(kind)
    a = make_trainer(engine, G, "", 7, S_, spe, 1.0, 0.25, 0, 1, False, trace=True, stagger=False, pools=pools)
    a.set_net(kind, w)
    assert a.run()
    t = make_trainer(engine, G, "", 7, S_, spe, 1.0, 0.25, 0, 1, False, trace=True, stagger=False, pools=pools)
    b = Buffers(engine, t.request_rows())
    net = Net(kind, w, b.rows, _cdll=cdll(engine))
    asked = []

    def fn(row0, cap, d_rows_ptr, stream_ptr):
        asked.append(cap)
        net.forward_device(b.ptrs[0] + row0 * GS * 4, cap, d_rows_ptr, b.ptrs[1] + row0 * 4, b.ptrs[2] + row0 * NM * 4, stream_ptr)

    t.set_net_fn(fn, *b.ptrs, b.rows, flop_per_row=flop_per_row)
    assert t.run()
    assert asked
    for x, y in zip(H.get_samples(t), H.get_samples(a)):
        assert x.tobytes() == y.tobytes()
    assert t.num_samples() == a.num_samples() > 0 and t.score() == a.score()
    for g in range(G):
        assert t.trace(g).tobytes() == a.trace(g).tobytes(), "game %d" % g
    sa, st = a.stats(), t.stats()
    assert st["nn_rows"] == sa["nn_rows"]
    if flop_per_row:
        assert st["nn_rows_evaluated"] < st["nn_rows"], "the evaluation cache was not on"
    net.close()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("eval_cache", [False, 16], ids=["nocache", "cache16"])
def test_capped_and_resumed(engine, eval_cache):
    """5a. run(max_iterations=5) until done = one run(); the function replaced between two capped runs -- with the
    cache on the table is emptied (a position handed out before is handed out again), the games do not change"""
    G, S_, spe = 12, 64, 16
    ref = oracle_generation(G, S_, spe, 3.0, 0.25, 7, False)
    t, ext = ext_trainer(engine, G, S_, spe, 3.0, 0.25, 0, 1, eval_cache)
    runs = 0
    while not t.run(max_iterations=5):
        runs += 1
        assert runs < 10 ** 4
        if runs == 6:
            before = len(ext.calls)
            ext.install(t)  # the same function again
    assert runs > 6 and t.stats()["iterations"] >= 5 * runs
    assert_equals_oracle(t, ref, G)
    assert t.stats()["nn_rows"] == ref["total_rows"]
    if engine == "emu" and eval_cache:
        seen = set(c.rows[i].tobytes() for c in ext.calls[:before] for i in range(c.count))
        again = [c.rows[i].tobytes() for c in ext.calls[before:] for i in range(c.count)]
        assert seen & set(again), "the table was not emptied when the network was replaced"
        # ... and behind the emptying nothing is handed out twice: the table of 2^16 entries keeps everything
        later = set()
        for c in ext.calls[before:]:
            now = set(c.rows[i].tobytes() for i in range(c.count))
            assert not (now & later)
            later |= now


@pytest.mark.parametrize("engine", ENGINES)
def test_replacement_that_toggles_the_cache_in_mid_generation(engine):
    """5b. automatic cache: off for flop_per_row = 0 (unknown); a replacement worth a cache is refused in mid-generation"""
    G, S_, spe = 8, 30, 4
    ref = oracle_generation(G, S_, spe, 1.0, 0.25, 7, False)
    t, ext = ext_trainer(engine, G, S_, spe, 1.0, 0.25, eval_cache=True)
    assert not t.run(max_iterations=5)
    rc = cdll(engine).ca_trainer_set_net_fn(t._t, 0, t._net_fns[0].c, None, *ext.ptrs, ext.rows, 2e6)
    assert rc == -4 and b"evaluation cache on" in cdll(engine).ca_last_error()
    with pytest.raises(_lib.EngineError, match="error -4"):
        ext.install(t, flop_per_row=2e6)
    assert t.run()
    assert t.stats()["nn_rows_evaluated"] == t.stats()["nn_rows"]  # no cache
    assert_equals_oracle(t, ref, G)
    # at the boundary it is accepted, and the next generation has a cache
    ext.install(t, flop_per_row=2e6)
    t.reset(7)
    assert t.run()
    assert t.stats()["nn_rows_evaluated"] < t.stats()["nn_rows"]
    assert_equals_oracle(t, ref, G)


@pytest.mark.parametrize("engine", ENGINES)
def test_arena(engine):
    """6a. testing=True: slot 0 the best model, slot 1 the new one; the oracle arena driven by the reference loop"""
    G, S_, spe = 8, 40, 8
    t = make_trainer(engine, G, "", 9, S_, spe, 1.0, 0.25, 0, 1, True, trace=True)
    best = ExtNet(engine, t.request_rows(), salt=1).install(t, slot=0)
    new = ExtNet(engine, t.request_rows(), salt=2).install(t, slot=1)
    assert t.run()
    o = O.Trainer(G, seed=9, max_searches=S_, searches_per_eval=spe, testing=True)
    o.enable_trace()
    H.play_generation(o, G, spe, None, nets_by_player=(lambda s: H.hash_net(s, 2), lambda s: H.hash_net(s, 1)))  # to_play 0: new
    for g in range(G):
        assert np.array_equal(t.trace(g), o.trace(g)), "game %d" % g
        assert t.game_info(g)["result"] == o.game_result(g)
    assert t.score() == o.score()
    assert len(best.calls) == len(new.calls) > 0  # both are queued every iteration
    if engine == "emu":  # ... and the idle one is asked for nothing but zero rows
        assert not any(a.count and b.count for a, b in zip(best.calls, new.calls))
        assert all(c.cap == G * spe and c.row0 == 0 for c in best.calls + new.calls)


def _golden_positions(n):
    """positions of tests/golden/rules_corpus.npz that have a legal move, as DockerMC constructor arguments"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "rules_corpus.npz"))
    idx = [i for i in range(200, z["boards"].shape[0], 397) if z["masks"][i].any()][:n]
    boards = np.array([[(int(z["boards"][i]) >> k) & 1 for k in range(64)] for i in idx], np.int32)
    metas = [int(z["metas"][i]) for i in idx]
    pieces = np.array([[(m >> (3 * k)) & 7 for k in range(6)] for m in metas], np.int32)
    to_play = np.array([(m >> 18) & 1 for m in metas], np.int32)
    return boards, to_play, pieces


@pytest.mark.parametrize("engine", ENGINES)
def test_analysis(engine):
    """6b. four positions searched with the caller's network inside run() = the host-driven search of the same positions"""
    n, S_, spe = 4, 48, 8
    boards, tp, pc = _golden_positions(n)
    seeds = np.arange(n, dtype=np.int32) + 40
    f = Analyser(boards, tp, pc, seeds, S_, spe, _cdll=cdll(engine))
    ext = ExtNet(engine, f.request_rows(), salt=4)
    f.set_net_fn(ext.fn, *ext.ptrs, ext.rows)
    assert f.run()
    h = Analyser(boards, tp, pc, seeds, S_, spe, _cdll=cdll(engine))
    cap = n * spe
    evals, probs, gs = np.zeros(cap, np.float32), np.zeros((cap, NM), np.float32), np.zeros((cap, GS), np.float32)
    while not h.doIteration(evals, probs):
        k = h.num_requests()
        h.writeRequests(gs)
        evals[:k], probs[:k] = H.hash_net(gs[:k], 4)
    assert f.results() == h.results()
    assert all("move" in r and r["nodes_searched"] > 1 for r in f.results())


@pytest.mark.parametrize("engine", ENGINES)
def test_tourney(engine):
    """6c. six matches, two model ids, both the caller's functions: the oracle tournament under the reference loop"""
    players = [(0, 0, 40, 8, 1.0, 0.25, False), (1, 1, 32, 8, 1.0, 0.25, False), (2, 1, 24, 4, 2.0, 0.25, False),
               (3, -1, 0, 0, 1.0, 0.25, True)]
    matches = [(0, 1), (1, 0), (2, 0), (0, 3), (3, 2), (1, 2)]

    def build(factory):
        t = factory()
        for p in players:
            t.addPlayer(*p)
        for a, b in matches:
            t.addMatch(a, b, False)
        return t

    f = build(lambda: Tourney(1, "", trace=True, _cdll=cdll(engine)))
    rows = len(matches) * 8
    small = ExtNet(engine, rows - 1, salt=11)
    f.set_net_fn(0, small.fn, *small.ptrs, small.rows)
    exts = {0: ExtNet(engine, rows, salt=11), 1: ExtNet(engine, rows, salt=22)}
    f.set_net_fn(1, exts[1].fn, *exts[1].ptrs, rows)
    with pytest.raises(_lib.EngineError, match="error -1"):  # buffers smaller than matches x searches_per_eval
        f.run()
    f.set_net_fn(0, exts[0].fn, *exts[0].ptrs, rows)
    assert not f.run(max_rounds=3)
    assert f.run()
    o = build(lambda: O.Tourney(2, "", trace=True))
    H.play_tourney(o, [-1, 0, 1], {0: lambda s: H.hash_net(s, 11), 1: lambda s: H.hash_net(s, 22)},
                   sum(players[a][3] + players[b][3] for a, b in matches))
    for i in range(len(matches)):
        assert np.array_equal(f.trace(i), o.trace(i)), "per-ply trace of match %d" % i
        assert f.match_score(i) == o.match_score(i)
    assert exts[0].calls and exts[1].calls and not small.calls


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("pools", [1, 3])
def test_function_that_fails(engine, pools):
    """7a. the function raises in its 7th call: run() raises that exception, the generation is unusable until reset(),
    and after reset() with a healthy function it is the oracle's"""
    G, S_, spe = 12, 64, 16
    ref = oracle_generation(G, S_, spe, 3.0, 0.25, 7, False)
    t = make_trainer(engine, G, "", 7, S_, spe, 3.0, 0.25, 0, 1, False, trace=True, stagger=False, pools=pools, eval_cache=False)
    ext = ExtNet(engine, t.request_rows(), fail_at=7).install(t)
    with pytest.raises(ValueError, match="failed in call 7") as info:
        t.run()
    assert isinstance(info.value.__cause__, _lib.EngineError) and "error -6" in str(info.value.__cause__)
    assert "slot 0" in str(info.value.__cause__)
    assert len(ext.calls) == 7, "the function was called again after it had failed"
    for call in (t.run, lambda: t.net_forward(_quarter_rows(2, 1))):
        with pytest.raises(_lib.EngineError, match="error -4.*ca_trainer_reset"):
            call()
    assert len(ext.calls) == 7
    ext.fail_at = 0
    t.reset(7)
    assert t.run()
    assert_equals_oracle(t, ref, G)


@pytest.mark.parametrize("engine", ENGINES)
def test_function_that_calls_its_trainer_and_bad_arguments(engine):
    """7b. an entry point of the same trainer from inside the function is CA_ERR_STATE; argument errors are CA_ERR_ARG"""
    L = cdll(engine)
    G, S_, spe = 8, 30, 4
    t = make_trainer(engine, G, "", 7, S_, spe, 1.0, 0.25, 0, 1, False, stagger=False)
    ext = ExtNet(engine, t.request_rows(), inside=lambda: t.num_samples()).install(t)
    with pytest.raises(_lib.EngineError, match="error -4.*inside a caller-supplied network function"):
        t.run()
    assert len(ext.calls) == 0
    cb = t._net_fns[0].c
    rows = t.request_rows()
    assert rows == G * spe
    p = ext.ptrs
    assert L.ca_trainer_set_net_fn(t._t, 0, cb, None, p[0], p[1], p[2], rows - 1, 0.0) == -1 and L.ca_last_error()
    for k in range(3):  # a null buffer
        q = list(p)
        q[k] = None
        assert L.ca_trainer_set_net_fn(t._t, 0, cb, None, q[0], q[1], q[2], rows, 0.0) == -1
    assert L.ca_trainer_set_net_fn(t._t, 0, C.cast(None, _lib.NET_FN), None, p[0], p[1], p[2], rows, 0.0) == -1
    assert L.ca_trainer_set_net_fn(t._t, 2, cb, None, p[0], p[1], p[2], rows, 0.0) == -1
    assert L.ca_trainer_set_net_fn(t._t, -1, cb, None, p[0], p[1], p[2], rows, 0.0) == -1
    assert L.ca_trainer_request_rows(t._t, None) == -1
    with pytest.raises(_lib.EngineError, match="error -1"):
        t.set_net_fn(ext.fn, *p, rows, slot=2)
    # none of it replaced the slot or cured the generation; a reset and a healthy function do
    ext.inside = None
    t.reset(7)
    ref = oracle_generation(G, S_, spe, 1.0, 0.25, 7, False)
    assert t.run()
    for x, y in zip(H.get_samples(t), ref["samples"]):
        assert x.tobytes() == y
