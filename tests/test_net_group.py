"""Rows of many models of one kind through one launch (NetGroup, ca_net_group_*): every row comes back with the bits
the row's own model gives it alone, the grouping kernel's tables are a deterministic counting sort, and a weight set an
f16x3 kernel cannot hold is refused with the model named.

The split-precision kinds of mlp12x100 (128 rows per workgroup) and rescnn4 at f16x3 (16 positions per workgroup) run one
grouped kernel; every other kind, and the emulation build, run the per-model fallback on the same index lists."""
import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, NET_MLP12X100_H3, NET_MLP12X100_X6, NET_RESCNN4_H3, _lib, nets
from corintho_ai_amd.net import NetGroup
from tests.engines import ENGINES, cdll, make_trainer

HIP = [pytest.param("hip", marks=pytest.mark.gpu, id="hip")]


def _states(n, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 70), np.float32)
    s[:, :64] = rng.integers(0, 2, (n, 64))
    s[:, 64:] = rng.integers(0, 5, (n, 6)) * 0.25
    return s


def _interleaved(sizes, seed):
    """model_of_row with sizes[m] rows of model m, shuffled so that the gather matters"""
    m = np.concatenate([np.full(n, i, np.int32) for i, n in enumerate(sizes)])
    np.random.default_rng(seed).shuffle(m)
    return m


def _mlp_sets():
    return [nets.trained_like_mlp12x100(0), nets.init_mlp12x100(1, bn_noise=True), nets.trained_like_mlp12x100(2),
            nets.init_mlp12x100(3, bn_noise=True)]


def _alone(engine, kind, weights, states, model_of_row):
    """every row through its own model, one net_forward per model on that model's rows"""
    t = make_trainer(engine, 64, "", 1, 50, 16, 1.0, 0.25, 0, 1, False)
    ev, pr = np.zeros(len(states), np.float32), np.zeros((len(states), 96), np.float32)
    for m, w in enumerate(weights):
        rows = np.flatnonzero(model_of_row == m)
        if rows.size:
            t.set_net(kind, w)
            ev[rows], pr[rows] = t.net_forward(states[rows])
    return ev, pr


def _check_equal(engine, kind, weights, sizes, grouped_kernel):
    model_of_row = _interleaved(sizes, 11)
    states = _states(len(model_of_row), 12)
    g = NetGroup(kind, weights, max_rows=1024, _cdll=cdll(engine))
    assert g.grouped_kernel == grouped_kernel and g.models == len(weights)
    ev, pr = g.forward(states, model_of_row)
    ev1, pr1 = _alone(engine, kind, weights, states, model_of_row)
    assert np.isfinite(ev).all() and np.isfinite(pr).all()
    assert ev.tobytes() == ev1.tobytes(), "values differ from the per-model launches"
    assert pr.tobytes() == pr1.tobytes(), "priors differ from the per-model launches"
    return g, model_of_row


def _check_tables(g, model_of_row, sizes):
    t = g.tables()
    assert list(t["seg_count"]) == list(sizes)
    seen = []
    for m, n in enumerate(sizes):
        seg = t["idx"][t["seg_start"][m]:t["seg_start"][m] + n]
        assert list(seg) == list(np.flatnonzero(model_of_row == m)), "model %d: its rows, in row order" % m
        seen += list(seg)
    assert sorted(seen) == list(range(len(model_of_row))), "every row index once"
    wg = t["wg"]
    assert len(wg) == sum((n + g.tile - 1) // g.tile for n in sizes)
    assert list(wg[:, 0]) == sorted(wg[:, 0]), "workgroups in model order"
    covered = []
    for m, first, n in wg:
        assert 0 < n <= g.tile
        lo, hi = t["seg_start"][m], t["seg_start"][m] + sizes[m]
        assert lo <= first and first + n <= hi, "a workgroup spans two models"
        covered += list(range(first, first + n))
    want = [i for m, n in enumerate(sizes) for i in range(t["seg_start"][m], t["seg_start"][m] + n)]
    assert covered == want, "the workgroups cover every segment once, in order"
    if g.grouped_kernel:
        assert list(t["seg_start"]) == list(np.concatenate([[0], np.cumsum(sizes)[:-1]])), "segments packed"
    return t


@pytest.mark.parametrize("engine", HIP)
def test_grouped_mlp12x100_f16x3_equals_the_per_model_launches(engine):
    """129, 0, 1, 128 rows: one over the 128-row workgroup, a model without rows, a single row, exactly one workgroup"""
    sizes = [129, 0, 1, 128]
    g, model_of_row = _check_equal(engine, NET_MLP12X100_H3, _mlp_sets(), sizes, True)
    _check_tables(g, model_of_row, sizes)


@pytest.mark.parametrize("engine", HIP)
def test_grouped_mlp12x100_x6_equals_the_per_model_launches(engine):
    """the template gives every width of the split kernel its grouped instance: the three-term one"""
    _check_equal(engine, NET_MLP12X100_X6, _mlp_sets()[:3], [130, 5, 127], True)


@pytest.mark.parametrize("engine", HIP)
def test_grouped_rescnn4_f16x3_equals_the_per_model_launches(engine):
    """the grouped small-batch kernel, 16 positions per workgroup: one fewer than, exactly and one more than a workgroup's,
    none, one"""
    weights = [nets.trained_like_rescnn4(0), nets.init_rescnn4(1, bn_noise=True), nets.trained_like_rescnn4(2), nets.init_rescnn4(3),
               nets.init_rescnn4(4, bn_noise=True)]
    sizes = [15, 16, 17, 0, 1]
    g, model_of_row = _check_equal(engine, NET_RESCNN4_H3, weights, sizes, True)
    assert g.tile == 16
    t = _check_tables(g, model_of_row, sizes)
    assert [tuple(e) for e in t["wg"]] == [(0, 0, 15), (1, 15, 16), (2, 31, 16), (2, 47, 1), (4, 48, 1)]


@pytest.mark.parametrize("engine", HIP)
def test_grouped_rescnn4_f16x3_many_workgroups_and_interleaved_rows(engine):
    """more workgroups than models, rows that are no multiple of anything, segments across several workgroups"""
    weights = [nets.trained_like_rescnn4(0), nets.init_rescnn4(1, bn_noise=True), nets.trained_like_rescnn4(2)]
    g, model_of_row = _check_equal(engine, NET_RESCNN4_H3, weights, [77, 3, 150], True)
    _check_tables(g, model_of_row, [77, 3, 150])


@pytest.mark.parametrize("engine", HIP)
def test_rescnn4_kinds_without_a_grouped_kernel_use_the_fallback(engine):
    from corintho_ai_amd import NET_RESCNN4_X3

    weights = [nets.trained_like_rescnn4(0), nets.init_rescnn4(1, bn_noise=True)]
    _check_equal(engine, NET_RESCNN4_X3, weights, [17, 16], False)


@pytest.mark.parametrize("engine", ENGINES)
def test_fallback_equals_the_per_model_launches(engine):
    """a kind without a grouped kernel (fp32 MFMA; the emulation build: its host network): one launch per model segment"""
    sizes = [129, 0, 1, 128]
    g, model_of_row = _check_equal(engine, NET_MLP12X100, _mlp_sets(), sizes, False)
    _check_tables(g, model_of_row, sizes)


@pytest.mark.parametrize("engine,kind", [pytest.param("emu", NET_MLP12X100, id="emu"),
                                         pytest.param("hip", NET_MLP12X100_H3, marks=pytest.mark.gpu, id="hip")])
def test_tables_are_the_same_from_call_to_call(engine, kind):
    """placement is a counting sort, no atomic decides an order: two calls leave identical tables; more models than a
    lane's share (65 > 64 lanes) and rows that are no multiple of the lanes"""
    weights = _mlp_sets()
    many = [weights[i % 4] for i in range(65)]
    rng = np.random.default_rng(3)
    model_of_row = rng.integers(0, 65, 1000).astype(np.int32)
    model_of_row[model_of_row == 17] = 18  # a model without rows in the middle
    sizes = [int((model_of_row == m).sum()) for m in range(65)]
    states = _states(1000, 4)
    g = NetGroup(kind, many, max_rows=1000, _cdll=cdll(engine))
    out1 = g.forward(states, model_of_row)
    t1 = _check_tables(g, model_of_row, sizes)
    out2 = g.forward(states, model_of_row)
    t2 = g.tables()
    live = np.zeros(len(t1["idx"]), bool)  # (the index list beyond the segments is never written)
    for m, n in enumerate(sizes):
        live[t1["seg_start"][m]:t1["seg_start"][m] + n] = True
    assert t1["idx"][live].tobytes() == t2["idx"][live].tobytes()
    for k in ("wg", "seg_start", "seg_count"):
        assert t1[k].tobytes() == t2[k].tobytes(), k
    assert out1[0].tobytes() == out2[0].tobytes() and out1[1].tobytes() == out2[1].tobytes()
    # a smaller batch through the same group: the tables follow the batch
    g.forward(states[:7], model_of_row[:7])
    _check_tables(g, model_of_row[:7], [int((model_of_row[:7] == m).sum()) for m in range(65)])


@pytest.mark.parametrize("engine", HIP)
def test_weights_beyond_fp16_range_are_refused_with_the_model_named(engine):
    weights = _mlp_sets()[:3]
    weights[2] = weights[2].copy()
    weights[2][10] = 1.0e6
    with pytest.raises(_lib.EngineError, match="model 2 of the group.*fp16 range"):
        NetGroup(NET_MLP12X100_H3, weights, max_rows=256, _cdll=cdll(engine))


@pytest.mark.parametrize("engine", HIP)
def test_rescnn4_weights_beyond_fp16_range_are_refused_with_the_model_named(engine):
    weights = [nets.init_rescnn4(0), nets.init_rescnn4(1).copy()]
    weights[1][100] = 1.0e6  # a stem convolution weight
    with pytest.raises(_lib.EngineError, match="model 1 of the group.*fp16 range"):
        NetGroup(NET_RESCNN4_H3, weights, max_rows=64, _cdll=cdll(engine))


@pytest.mark.parametrize("engine", ENGINES)
def test_bad_arguments_are_errors(engine):
    L = cdll(engine)
    w = _mlp_sets()[:2]
    g = NetGroup(NET_MLP12X100, w, max_rows=64, _cdll=L)
    with pytest.raises(_lib.EngineError, match="names model 2 of 2"):
        g.forward(_states(3, 0), np.array([0, 2, 1], np.int32))
    with pytest.raises(_lib.EngineError, match="more rows"):
        g.forward(_states(65, 0), np.zeros(65, np.int32))
    with pytest.raises(_lib.EngineError, match="65535"):
        NetGroup(NET_MLP12X100, w, max_rows=70000, _cdll=L)
    with pytest.raises(_lib.EngineError, match="model 0 of the group.*unknown net kind"):
        NetGroup(99, w, max_rows=64, _cdll=L)
    with pytest.raises(_lib.EngineError, match="ca_net_group_bench"):
        g.bench(_states(0, 0), np.zeros(0, np.int32))
    with pytest.raises(_lib.EngineError, match="ca_net_group_bench"):
        g.bench(_states(3, 0), np.zeros(3, np.int32), reps=0)
