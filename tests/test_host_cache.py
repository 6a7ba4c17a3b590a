"""The host-driven Trainer protocol with the evaluation cache (ca_trainer_set_host_cache, Trainer.set_host_cache):
num_requests / writeRequests hand the caller only the rows whose position has no stored evaluation in this generation,
doIteration takes the answers to exactly those rows, and every game plays what it plays under the plain protocol.

The yardstick is oracle.Trainer played with the same network under the plain protocol (tests/test_engine_parity.py
pins the engine's plain protocol to it row for row, so the oracle's request log IS the plain protocol's).  The caller's
network is harness.hash_net: a function of the row alone, which is the mode's precondition.  Each oracle generation is
played once per session and shared, unchanged, by the tests that need it.

Runs on the emulation build here and on the MI355X with -m gpu.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from corintho_ai_amd import _lib
from oracle import oracle as O
from tests import harness as H
from tests.engines import ENGINES, cdll, make_trainer

GS, NM = H.GS, H.NM
CA_ERR_ARG, CA_ERR_STATE = -1, -4


@functools.lru_cache(maxsize=None)
def oracle_generation(G, S_, spe, c_puct, eps, seed, stagger):
    """the plain protocol's generation: what the games produce and every row they request"""
    o = O.Trainer(G, seed=seed, max_searches=S_, searches_per_eval=spe, c_puct=c_puct, epsilon=eps, num_threads=4)
    o.enable_trace()
    o.set_stagger(stagger)
    r = H.play_generation(o, G, spe, H.hash_net, record=True)
    rows = set()
    total = 0
    for _, b in r["log"]:
        total += b.shape[0]
        rows.update(b[i].tobytes() for i in range(b.shape[0]))
    return {
        "samples": tuple(x.tobytes() for x in H.get_samples(o)),
        "score": o.score(),
        "mate": o.avg_mate_length(),
        "num_samples": o.num_samples(),
        "results": tuple(o.game_result(g) for g in range(G)),
        "traces": tuple(o.trace(g).tobytes() for g in range(G)),
        "rows": frozenset(rows),
        "total_rows": total,
        "first_row": r["log"][0][1][0].tobytes(),
        "iterations": r["iterations"],
    }


def play_cached(t, G, spe, net, answers=None, max_iters=10 ** 6):
    """The loop of main.pyx:142-168 as a caller of the cached protocol writes it, i.e. harness.play_generation without
    its `n == 0 -> "No requests during training"` line (which is why that function cannot drive a cached trainer: with
    the cache a batch of 0 rows while games run means every row was served from the table).  Returns the batches handed
    out, one array per doIteration call that did not end the generation (empty ones included).  `answers`: (evals,
    probs) for rows the caller has fetched already, when the loop takes over a generation in progress."""
    cap = G * spe
    evals = np.zeros(cap, np.float32)
    probs = np.zeros((cap, NM), np.float32)
    if answers is not None:
        evals[:answers[0].shape[0]] = answers[0]
        probs[:answers[1].shape[0]] = answers[1]
    game_states = np.zeros((cap, GS), np.float32)
    batches = []
    while not t.doIteration(evals, probs, -1):
        assert len(batches) < max_iters, "play loop did not terminate"
        n = t.num_requests(-1)
        assert 0 <= n <= cap
        if n:
            game_states[:] = -1.0  # nothing of an earlier batch can pass for a row of this one
            t.writeRequests(game_states, -1)
            e, p = net(game_states[:n])
            evals[:n] = e
            probs[:n] = p
            evals[n:] = np.nan  # the engine may read the n answers only
            probs[n:] = np.nan
        batches.append(game_states[:n].copy())
    return batches


def assert_first_batch_is_the_start_position(batch, ref, G):
    """Every game asks for the start position in its first iteration, and the cache resolves rows of one batch against
    each other: ONE row is what the first batch is expected to be, and what it is whenever the games' wavefronts reach
    the table one after another (the emulation build on one thread: always).  Exactly one cannot be asserted: a
    wavefront that finds a slot claimed an instant ago, its key words not yet visible, takes the next slot for the same
    position (search_step.h co_cache_resolve: "correctness does not depend on who wins a race") -- seen on the emulation build
    with OpenMP threads as 2 or 3 copies of one position in a batch, in 1 run of 4.  What holds in every schedule: the
    batch holds nothing but the start position, at least once and at most once per game."""
    assert 1 <= batch.shape[0] <= G
    for k in range(batch.shape[0]):
        assert batch[k].tobytes() == ref["first_row"]


def assert_equals_oracle(t, ref, G):
    for x, y in zip(H.get_samples(t), ref["samples"]):
        assert x.tobytes() == y, "samples differ from the plain protocol's"
    assert t.num_samples() == ref["num_samples"]
    assert t.score() == ref["score"]
    assert t.avg_mate_length() == ref["mate"]
    for g in range(G):
        info = t.game_info(g)
        assert info["done"] == 1 and info["error"] == 0 and info["n_pending"] == 0, (g, info)
        assert info["result"] == ref["results"][g], "result of game %d" % g
        assert t.trace(g).tobytes() == ref["traces"][g], "per-ply trace of game %d" % g


def assert_rows_accounted(t, batches, ref, strictly_fewer):
    handed = sum(b.shape[0] for b in batches)
    st = t.stats()
    print("rows handed out %d, evaluated (stats) %d, requested %d, plain protocol %d; iterations %d (plain %d)" %
          (handed, st["nn_rows_evaluated"], st["nn_rows"], ref["total_rows"], st["iterations"], ref["iterations"]))
    assert st["nn_rows_evaluated"] == handed
    assert st["nn_rows"] == ref["total_rows"]
    assert st["iterations"] == len(batches) + 1  # doIteration calls
    assert handed <= st["nn_rows"]
    if strictly_fewer:
        assert handed < st["nn_rows"]
    for i, b in enumerate(batches):
        for k in range(b.shape[0]):
            assert b[k].tobytes() in ref["rows"], "row %d of batch %d is no row of the plain protocol" % (k, i)


# G, sims, spe, c_puct, eps, resident slots
SAME_GENERATION = [
    pytest.param(8, 30, 1, 1.0, 0.0, 0, id="G8-30sims-spe1-eps0"),
    pytest.param(12, 64, 16, 3.0, 0.25, 0, id="G12-64sims-spe16-cpuct3"),
    pytest.param(21, 40, 4, 1.0, 0.25, 5, id="G21-on-5-slots-40sims-spe4"),
]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("G,S_,spe,c_puct,eps,resident", SAME_GENERATION)
def test_same_generation_fewer_rows(engine, G, S_, spe, c_puct, eps, resident):
    """1. the generation of the plain protocol, from fewer rows: a table of 2^16 entries is never emptied here"""
    ref = oracle_generation(G, S_, spe, c_puct, eps, 7, False)
    t = make_trainer(engine, G, "", 7, S_, spe, c_puct, eps, 0, 1, False, trace=True, stagger=False, resident=resident)
    t.set_host_cache(16)
    batches = play_cached(t, G, spe, H.hash_net)
    assert_equals_oracle(t, ref, G)
    assert_rows_accounted(t, batches, ref, strictly_fewer=True)
    assert_first_batch_is_the_start_position(batches[0], ref, G)
    # a position evaluated in an EARLIER iteration is never handed out again while the table keeps everything
    seen = set()
    for i, b in enumerate(batches):
        now = set(b[k].tobytes() for k in range(b.shape[0]))
        assert not (now & seen), "batch %d repeats a position of an earlier batch" % i
        seen |= now


@pytest.mark.parametrize("engine", ENGINES)
def test_table_that_keeps_being_emptied(engine):
    """2. 64 entries under batches of up to 192 rows: the table is emptied in mid-generation over and over (no entry
    is claimed in the iteration behind an emptying, value elements of pending leaves stay) -- results do not move.
    Orderings only, no cache counts."""
    G, S_, spe = 12, 64, 16
    ref = oracle_generation(G, S_, spe, 3.0, 0.25, 7, False)
    t = make_trainer(engine, G, "", 7, S_, spe, 3.0, 0.25, 0, 1, False, trace=True, stagger=False)
    t.set_host_cache(6)
    batches = play_cached(t, G, spe, H.hash_net)
    assert_equals_oracle(t, ref, G)
    assert_rows_accounted(t, batches, ref, strictly_fewer=False)


@pytest.mark.parametrize("engine", ENGINES)
def test_batch_edges(engine):
    """3. the batch sizes at which co_k_host_rows_out / co_k_host_rows_in can go wrong, through the protocol.
    G = 4, spe = 16 (capacity 64 rows), 64 simulations, seed 7, hash_net, 2^16 entries; found on the emulation build
    (batch i = the rows handed out after doIteration call i, from 0; the sizes begin 1, 24, 44, 52, 47, 0, 41, 55):
      * 0 rows while games run ............ batch 5 (every row a hit) -- and the loop goes on without an error
      * 1 row ............................. batch 0 (the start position, asked for by all four games)
      * not a multiple of 64 .............. batch 1 (24 rows) and most others
      * the capacity G * spe = 64 ......... batch 13 (again 18 and 23): hash_net's priors send the four games down
                                            different lines soon enough, no other caller network is needed
    A batch holds every position no earlier batch held at least once; racing wavefronts can add copies (see
    assert_first_batch_is_the_start_position), so a size is asserted exactly only where no copy is possible: 0, and the
    capacity.    The batch sizes follow from the games alone (which positions a batch holds that no earlier one did), not from the
    order in which wavefronts reach the table, so they are the same on the device."""
    G, S_, spe = 4, 64, 16
    ref = oracle_generation(G, S_, spe, 1.0, 0.25, 7, False)
    t = make_trainer(engine, G, "", 7, S_, spe, 1.0, 0.25, 0, 1, False, trace=True, stagger=False)
    t.set_host_cache(16)
    batches = play_cached(t, G, spe, H.hash_net)
    sizes = [b.shape[0] for b in batches]
    print("batch sizes:", sizes)
    assert_first_batch_is_the_start_position(batches[0], ref, G)
    assert sizes[5] == 0 and len(sizes) > 6, "no iteration was served from the table alone"
    assert 1 in sizes
    assert 24 <= sizes[1] < 64
    assert sizes[13] == G * spe == max(sizes), "the capacity batch: largest is %d rows" % max(sizes)
    assert_equals_oracle(t, ref, G)
    assert_rows_accounted(t, batches, ref, strictly_fewer=True)


@pytest.mark.parametrize("engine", ENGINES)
def test_second_generation_starts_with_an_empty_table(engine):
    """4. reset(seed): nothing evaluated in the first generation serves the second -- its first batch is the start
    position again, and it is the oracle's generation for that seed"""
    G, S_, spe = 6, 24, 4
    t = make_trainer(engine, G, "", 7, S_, spe, 1.0, 0.25, 0, 1, False, trace=True, stagger=False)
    t.set_host_cache(16)
    for seed in (7, 11):
        ref = oracle_generation(G, S_, spe, 1.0, 0.25, seed, False)
        if seed != 7:
            t.reset(seed)
        batches = play_cached(t, G, spe, H.hash_net)
        assert_first_batch_is_the_start_position(batches[0], ref, G)
        assert_equals_oracle(t, ref, G)
        assert_rows_accounted(t, batches, ref, strictly_fewer=True)
    # switching at the boundary behind a reset: off, and the plain protocol is back
    t.reset(7)
    t.set_host_cache(False)
    ref = oracle_generation(G, S_, spe, 1.0, 0.25, 7, False)
    r = H.play_generation(t, G, spe, H.hash_net, record=True)
    assert sum(b.shape[0] for _, b in r["log"]) == ref["total_rows"]
    assert_equals_oracle(t, ref, G)


@pytest.mark.parametrize("engine", ENGINES)
def test_staggered_start(engine):
    """5. the reference's staggered start (trainer.cpp:184-186): game g waits for iteration g / max(G / sims, 1); an
    iteration whose started games are all served from the table hands out 0 rows without error"""
    G, S_, spe = 24, 30, 1
    ref = oracle_generation(G, S_, spe, 1.0, 0.25, 7, True)
    t = make_trainer(engine, G, "", 7, S_, spe, 1.0, 0.25, 0, 1, False, trace=True, stagger=True)
    t.set_host_cache(16)
    batches = play_cached(t, G, spe, H.hash_net)
    assert batches[0].shape[0] == 1  # game 0 alone has started: nobody to race with
    assert_equals_oracle(t, ref, G)
    assert_rows_accounted(t, batches, ref, strictly_fewer=True)


def _rc(L, t, log2):
    return L.ca_trainer_set_host_cache(t._t, log2)


@pytest.mark.parametrize("engine", ENGINES)
def test_refusals(engine):
    """6. each refusal with its error code"""
    L = cdll(engine)
    G, S_, spe = 4, 8, 2
    ev, pr, gs = np.zeros(G * spe, np.float32), np.zeros((G * spe, NM), np.float32), np.zeros((G * spe, GS), np.float32)
    # a testing trainer, an analysis trainer: the cache is training-only
    arena = make_trainer(engine, G, "", 1, S_, spe, 1.0, 0.25, 0, 1, True)
    assert _rc(L, arena, 16) == CA_ERR_STATE and L.ca_last_error()
    analysis = make_trainer(engine, G, "", 1, S_, spe, 1.0, 0.25, 0, 1, False, analyse=True)
    assert _rc(L, analysis, 0) == CA_ERR_STATE
    with pytest.raises(_lib.EngineError, match="error -4"):
        arena.set_host_cache(True)
    # sizes
    t = make_trainer(engine, G, "", 1, S_, spe, 1.0, 0.25, 0, 1, False, stagger=False)
    for bad in (1, 3, 5, 31):
        assert _rc(L, t, bad) == CA_ERR_ARG
    with pytest.raises(ValueError):
        t.set_host_cache(3)
    # switching on after the first doIteration
    assert not t.doIteration(ev, pr, -1)
    assert _rc(L, t, 16) == CA_ERR_STATE
    t.set_host_cache(False)  # (off while it is off: nothing to switch)
    # ... and off in a generation it is driving
    c = make_trainer(engine, G, "", 1, S_, spe, 1.0, 0.25, 0, 1, False, stagger=False)
    c.set_host_cache(True)
    assert c.num_requests(-1) == 0  # before the first iteration nothing is asked
    assert not c.doIteration(ev, pr, -1)
    assert _rc(L, c, -1) == CA_ERR_STATE
    assert _rc(L, c, 16) == CA_ERR_STATE
    # run() during a host-cached generation
    done = C.c_int32()
    assert L.ca_trainer_run(c._t, 0, C.byref(done)) == CA_ERR_STATE
    # to_play = 0 (and 1) in each of the three calls
    n = C.c_int32()
    for tp in (0, 1):
        assert L.ca_trainer_num_requests(c._t, tp, C.byref(n)) == CA_ERR_ARG
        assert L.ca_trainer_write_requests(c._t, gs.ctypes.data_as(_lib.f32p), tp) == CA_ERR_ARG
        assert L.ca_trainer_do_iteration(c._t, ev.ctypes.data_as(_lib.f32p), pr.ctypes.data_as(_lib.f32p), tp,
                                         C.byref(done)) == CA_ERR_ARG
    # none of the refused calls moved the generation: it still ends as the oracle's
    n0 = c.num_requests(-1)
    ref = oracle_generation(G, S_, spe, 1.0, 0.25, 1, False)
    c.writeRequests(gs, -1)
    assert_first_batch_is_the_start_position(gs[:n0], ref, G)
    batches = [gs[:n0].copy()] + play_cached(c, G, spe, H.hash_net, answers=H.hash_net(gs[:n0]))
    assert_equals_oracle_no_trace(c, ref, G)
    assert sum(b.shape[0] for b in batches) == c.stats()["nn_rows_evaluated"]


def assert_equals_oracle_no_trace(t, ref, G):
    for x, y in zip(H.get_samples(t), ref["samples"]):
        assert x.tobytes() == y
    assert t.score() == ref["score"]
    assert [t.game_info(g)["result"] for g in range(G)] == list(ref["results"])


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("switch", ["never", "false"])
def test_off_means_off(engine, switch):
    """7. a trainer that never calls set_host_cache, and one that calls it with False, speak the plain protocol: the
    oracle's request log row for row"""
    G, S_, spe = 8, 30, 4
    t = make_trainer(engine, G, "", 7, S_, spe, 1.0, 0.25, 0, 1, False)
    if switch == "false":
        t.set_host_cache(False)
    o = O.Trainer(G, seed=7, max_searches=S_, searches_per_eval=spe, num_threads=4)
    ra = H.play_generation(t, G, spe, H.hash_net, record=True)
    rb = H.play_generation(o, G, spe, H.hash_net, record=True)
    assert ra["iterations"] == rb["iterations"]
    assert len(ra["log"]) == len(rb["log"])
    for i, (a, b) in enumerate(zip(ra["log"], rb["log"])):
        assert a[1].shape == b[1].shape and a[1].tobytes() == b[1].tobytes(), "request rows differ at iteration %d" % i
    for x, y in zip(H.get_samples(t), H.get_samples(o)):
        assert x.tobytes() == y.tobytes()
