"""The consistent move table without a GPU: the symmetry tables the kernels are compiled from against the oracle's, the
group facts about them, the rules' legal-move masks under the eight symmetries, samples_io.expand_host against the
oracle's writeSamples, and the run driver's `augmentation` setting."""
import json
import os

import numpy as np
import pytest

from corintho_ai_amd import RunParams, samples_io
from corintho_ai_amd import run as R
from corintho_ai_amd.fit import fit_samples
from oracle import oracle as O
from tests import harness as H
from tests.symmetry_cases import gather, same
from tests.test_run_cpu import StubFitter, open_run, small


def _oracle_tables():
    L = O.lib()
    return np.ctypeslib.as_array(L.co_space_symmetries(), (8, 16)), np.ctypeslib.as_array(L.co_move_symmetries(), (8, 96))


def _products(table):
    """P[a][b] = the index of table[a] o table[b], as the gathers compose: x[table[b]][table[a]] = x[table[a o b]]"""
    out = np.zeros((8, 8), np.int64)
    for a in range(8):
        for b in range(8):
            both = table[b][table[a]]
            ks = [k for k in range(8) if np.array_equal(table[k], both)]
            assert len(ks) == 1
            out[a, b] = ks[0]
    return out


def test_the_tables_are_the_oracles_and_mc_exchanges_rows_2_and_6():
    space, move, consistent = samples_io.symmetry_tables()
    o_space, o_move = _oracle_tables()
    assert space.dtype == move.dtype == consistent.dtype == np.int32
    assert np.array_equal(space, o_space) and np.array_equal(move, o_move)
    assert np.array_equal(consistent, move[[0, 1, 6, 3, 4, 5, 2, 7]])
    assert not np.array_equal(move[2], move[6])


def test_mc_multiplies_as_the_space_table_and_ms_as_its_transpose():
    space, move, consistent = samples_io.symmetry_tables()
    T = _products(space)
    assert not np.array_equal(T, T.T)  # the group is not abelian: the order matters
    assert np.array_equal(_products(consistent), T)
    assert np.array_equal(_products(move), T.T)


def _bits(mask):
    return np.array([mask >> i & 1 for i in range(96)], bool)


def test_legal_masks_turn_with_mc_and_not_with_ms():
    """positions of 400 seeded random games that have no line on the board: the legal moves of the turned position are
    the turned legal moves under MC for every k, on every one of them; under MS on fewer than half"""
    space, move, consistent = samples_io.symmetry_tables()
    g = gather()[:, :64]
    rng = np.random.default_rng(11)
    total = kept = with_ms = 0
    for _ in range(400):
        game = O.Game()
        while True:
            mask, lines = game.legal_mask()
            if mask == 0:
                break
            total += 1
            legal = _bits(mask)
            if not lines:
                kept += 1
                cells = np.array([game.board >> c & 1 for c in range(64)])
                ms_all = True
                for k in range(8):
                    turned = O.Game.from_arrays(cells[g[k]], game.to_play, game.pieces.copy())
                    got = _bits(turned.legal_mask()[0])
                    assert np.array_equal(got, legal[consistent[k]]), (total, k)
                    ms_all &= np.array_equal(got, legal[move[k]])
                with_ms += ms_all
            moves = np.flatnonzero(legal)
            game.do_move(int(moves[rng.integers(moves.size)]))
    print("%d positions, %d without a line, %d of them equivariant under MS too" % (total, kept, with_ms))
    assert kept >= 0.8 * total and kept > 5000
    assert with_ms < 0.5 * kept


@pytest.fixture(scope="module")
def oracle_samples():
    """the expanded samples of an oracle generation of 8 games at 32 searches, and their un-augmented rows"""
    o = O.Trainer(8, seed=5, max_searches=32, searches_per_eval=4)
    H.play_generation(o, 8, 4, H.hash_net)
    gs, ev, pr = H.get_samples(o)
    sp = np.ascontiguousarray(np.concatenate([gs[::8], pr[::8]], axis=1))  # symmetry 0 is the position as played
    return (gs, ev, pr), sp, np.ascontiguousarray(ev[::8])


def test_expand_host_reference_is_write_samples(oracle_samples):
    want, sp, oc = oracle_samples
    assert sp.shape[0] > 50
    for got, w in zip(samples_io.expand_host(sp, oc), want):
        assert same(got, w)
    for got, w in zip(samples_io.expand_host(sp, oc, "reference"), want):
        assert same(got, w)


def test_expand_host_consistent_exchanges_the_policies_of_rows_2_and_6(oracle_samples):
    (gs, ev, pr), sp, oc = oracle_samples
    cs, ce, cp = samples_io.expand_host(sp, oc, "consistent")
    assert same(cs, gs) and same(ce, ev)
    rows = np.arange(pr.shape[0])
    swapped = np.where(rows % 8 == 2, rows + 4, np.where(rows % 8 == 6, rows - 4, rows))
    assert same(cp, pr[swapped])
    differ = np.flatnonzero((cp != pr).any(axis=1))
    assert differ.size and set(differ % 8) == {2, 6}
    with pytest.raises(ValueError, match="augmentation"):
        samples_io.expand_host(sp, oc, "both")


# ---------------------------------------------------------------------------------------------------- the run's setting
def test_the_setting_from_toml_and_from_the_command_line(tmp_path):
    assert RunParams(seed=1).augmentation == "reference"
    assert R.parse_args(["--seed", "1"])[0].augmentation == "reference"
    assert R.parse_args(["--seed", "1", "--augmentation", "consistent"])[0].augmentation == "consistent"
    toml = tmp_path / "aug.toml"
    toml.write_text('[hyperparameters]\nnum_games = 16\naugmentation = "consistent"\n', encoding="utf-8")
    p, _ = R.parse_args(["--config", str(toml), "--seed", "1"])
    assert p.augmentation == "consistent" and p.num_games == 16
    assert R.parse_args(["--config", str(toml), "--seed", "1", "--augmentation", "reference"])[0].augmentation == "reference"
    assert RunParams(seed=1, augmentation="consistent").as_dict()["augmentation"] == "consistent"
    with pytest.raises(ValueError, match="augmentation"):
        RunParams(seed=1, augmentation="mirror")
    with pytest.raises(SystemExit):
        R.parse_args(["--seed", "1", "--augmentation", "mirror"])


class AugFitter(StubFitter):
    """the stub fitter of tests/test_run_cpu.py with the setter: it writes down what it is set to, and when"""

    def __init__(self):
        self.calls = []
        super().__init__()

    def clear_data(self):
        self.calls.append("clear_data")
        super().clear_data()

    def set_augmentation(self, augmentation):
        self.calls.append(("set_augmentation", augmentation))

    def add_samples(self, sp, oc):
        self.calls.append("add")
        super().add_samples(sp, oc)


@pytest.mark.parametrize("augmentation", ["reference", "consistent"])
def test_the_run_sets_the_fitter_before_the_samples_and_stores_the_setting(tmp_path, augmentation):
    fitter = AugFitter()
    run = open_run(small(tmp_path, augmentation=augmentation), fitter)
    run.generation()
    calls = [c for c in fitter.calls if c != "clear_data"]
    assert calls[0] == ("set_augmentation", augmentation) and calls[1] == "add"
    assert [c for c in calls if isinstance(c, tuple)] == [("set_augmentation", augmentation)]
    meta = os.path.join(run.root, "generations", "gen_1", "metadata.txt")
    assert R.generation_settings(meta)["augmentation"] == augmentation
    # a directory from before the setting existed reads as the reference's
    with open(meta, encoding="utf-8") as f:
        d = json.load(f)
    del d["augmentation"], d["merge_symmetries"]
    old = tmp_path / "old_metadata.txt"
    old.write_text(json.dumps(d), encoding="utf-8")
    got = R.generation_settings(str(old))
    assert got["augmentation"] == "reference" and got["merge_symmetries"] is False and got["num_games"] == 8


def test_a_fitter_without_the_setter_serves_the_reference_only(tmp_path):
    open_run(small(tmp_path, name="a"), StubFitter()).generation()
    with pytest.raises(ValueError, match="set_augmentation"):
        open_run(small(tmp_path, name="b", augmentation="consistent"), StubFitter()).generation()
    sp = np.zeros((16, 166), np.float32)
    with pytest.raises(ValueError, match="set_augmentation"):
        fit_samples(np.zeros(R.nets.MLP_NUM_WEIGHTS, np.float32), sp, np.zeros(16, np.float32), augmentation="consistent",
                    batch_size=8, _backend=StubFitter())
    with pytest.raises(ValueError, match="augmentation"):
        fit_samples(np.zeros(R.nets.MLP_NUM_WEIGHTS, np.float32), sp, np.zeros(16, np.float32), augmentation="mirror")
