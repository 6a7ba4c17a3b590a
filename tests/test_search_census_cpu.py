"""Which branches of the search do the fast parity cases take?  CPU only.

Bit-for-bit replay on the oracle checks only the branches its games happen to take.  This file plays every host-driven
parity case of tests/test_engine_parity.py, test_tourney.py, test_analyse.py and test_search_paths.py (each of them
also runs on the MI355X) on the oracle with its branch counters (oracle.census), and the self-play ones on the
emulation build with the grouped search's own counters (-DCO_SB_STATS), and asserts

  * a branch classed reachable is taken at least 5 times, a whole-game event (a drawn game, a drawn match) at least twice;
  * a branch classed unreachable is never taken: a change that opens one fails here and owes a case for it;
  * the table printed is the table of DESIGN.md section 2 (between the census markers).

Why each unreachable branch is unreachable is argued in DESIGN.md next to the table."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import harness as H
from tests import search_cases as SC

MIN_HITS, MIN_EVENTS = 5, 2
CO_MAX_PLIES, CO_PATH_MAX, CO_WAVE = 44, 48, 64  # engine_defs.h; the wide-node exit is for more edges than lanes

# (census name, where, classed reachable)
ORACLE_BRANCHES = [
    ("deduced_win", "propagate_terminal: lost child, parent won", True),
    ("deduced_draw", "propagate_terminal: all children known, one drawn", False),
    ("deduced_loss", "propagate_terminal: all children known", True),
    ("score_drawn_child", "choose_next: open drawn child, prior alone", False),
    ("score_visited_child", "choose_next: open child, PUCT score", True),
    ("score_closed_child", "choose_next: decided or all-visited child", True),
    ("score_unvisited_edge", "choose_next: edge without a child", True),
    ("search_retreat_below", "mc_search: nothing searchable below the root", True),
    ("search_retreat_root", "mc_search: nothing searchable at the root", True),
    ("search_leaf_drawn", "mc_search: terminal leaf, drawn", True),
    ("search_leaf_lost", "mc_search: terminal leaf, lost", True),
    ("search_new_first_child", "mc_search: new child is the first child", True),
    ("search_new_behind_sibling", "mc_search: new child behind a sibling", True),
    ("iter_rerequest", "mc_do_iteration: all-visited root asked again", True),
    ("move_won", "mc_choose_move: root won", True),
    ("move_lost", "mc_choose_move: root lost", True),
    ("move_drawn_root", "mc_choose_move: root drawn", False),
    ("move_opening_reset", "choose_move_opening: no visits, fresh tree", True),
    ("move_opening", "choose_move_opening: sampled by visits", True),
    ("move_normal_reset", "choose_move_normal: no visits, fresh tree", True),
    ("move_normal", "choose_move_normal: most visits", True),
    ("move_tie_by_eval", "choose_move_normal: tie on visits, by evaluation", True),
    ("move_drawn_child", "choose_move_normal: drawn child weighed", True),
    ("opp_move_found", "mc_receive_opponent_move: child becomes root", True),
    ("opp_move_new_root", "mc_receive_opponent_move: new root", True),
    ("game_drawn", "sp_end_game: drawn game", True),
    ("game_decisive", "sp_end_game: decisive game", True),
    ("match_drawn", "match_end_game: drawn match", True),
    ("match_decisive", "match_end_game: decisive match", True),
]
EVENTS = ("game_drawn", "match_drawn")
# engine counter (search_state.h CO_SBS) -> classed reachable
ENGINE_COUNTERS = [(i, i not in (4, 5)) for i in sorted(SC.SB_NAMES)]


def _old_analysis():
    from tests import test_analyse as TA

    for S_, spe in SC.ANALYSIS_SETTINGS:  # test_batched_analysis_matches_dockermc, with the MI355X's 40 positions
        boards, tp, pc = TA._positions(40, seed=S_)
        seeds = np.arange(40, dtype=np.int32) * 7 + 3
        for i in range(40):
            SC.analyse_on_oracle(boards[i], tp[i], pc[i], seeds[i], S_, spe, H.hash_net)


def _new_analysis():
    boards, tp, pc, seeds, _, _ = SC.load_positions()
    for net in SC.ANALYSIS_NETS:
        for S_, spe in SC.ANALYSIS_SETTINGS:
            for i in range(len(seeds)):
                SC.analyse_on_oracle(boards[i], tp[i], pc[i], seeds[i], S_, spe, SC.NETS[net]())


def _old_tourneys():
    from tests import test_tourney as TT

    for players, matches in ((TT.PLAYERS_A, TT.MATCHES_A), (TT.PLAYERS_B, TT.MATCHES_B)):
        t = SC.build_tourney(lambda: O.Tourney(2, ""), players, matches)
        H.play_tourney(t, sorted({p[1] for p in players}), TT._nets(), SC.tourney_rows(players, matches))
    t, counter, _ = TT._few_searches_tourney(lambda: O.Tourney(1, ""))
    H.play_tourney(t, list(range(counter)), {m: (lambda s, m=m: H.hash_net(s, 100 + m)) for m in range(1, 7)}, 48)
    for max_searches, spe in ((2, 1), (2, 2), (5, 3), (9, 9), (16, 1), (16, 16)):  # test_reference_match_few_searches
        for random_id in (0, 1, 2):
            t = O.Tourney(1, "")
            t.addPlayer(0, 0, max_searches, spe, 1.0, 0.25, random_id == 0)
            t.addPlayer(1, 1, max_searches, spe, 1.0, 0.25, random_id == 1)
            t.addMatch(0, 1, False)
            H.play_tourney(t, [0, 1], {0: lambda s: H.hash_net(s, 5), 1: lambda s: H.hash_net(s, 6)}, spe)


def _new_tourneys():
    for salt in SC.DRAWN_TOURNEY_SALTS:
        t = SC.build_tourney(lambda: O.Tourney(2, ""), SC.DRAWN_TOURNEY_PLAYERS, SC.DRAWN_TOURNEY_MATCHES)
        H.play_tourney(t, [-1, 0, 1], SC.drawn_tourney_nets(salt),
                       SC.tourney_rows(SC.DRAWN_TOURNEY_PLAYERS, SC.DRAWN_TOURNEY_MATCHES))


def _selfplay(cases):
    def run():
        for c in cases:
            SC.run_selfplay_on_oracle(c)
    return run


GROUPS = [
    ("self-play", _selfplay(SC.OLD_SELFPLAY), SC.OLD_SELFPLAY),
    ("arena", _selfplay(SC.OLD_ARENA), SC.OLD_ARENA),
    ("tournament", _old_tourneys, []),
    ("analysis", _old_analysis, []),
    ("deep lines", _selfplay(SC.DEEP), SC.DEEP),
    ("drawn self-play", _selfplay(SC.DRAWN), SC.DRAWN),
    ("drawn arena", _selfplay(SC.DRAWN_ARENA), SC.DRAWN_ARENA),
    ("one-simulation arena", _selfplay(SC.FEW_ARENA), SC.FEW_ARENA),
    ("drawn tournament", _new_tourneys, []),
    ("rare positions", _new_analysis, []),
]


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    """{group: oracle census}, {group: engine counters}; the oracle's counters are process wide, so one group at a time"""
    L = SC.sb_stats_lib(tmp_path_factory.mktemp("sbstats"))
    oracle, engine = {}, {}
    for name, run, cases in GROUPS:
        O.census_reset()
        run()
        oracle[name] = O.census()
        if cases:
            SC.sb_reset(L)
            for c in cases:
                SC.run_selfplay_on_engine(L, c)
            engine[name] = SC.sb_read(L)
    O.census_reset()
    return oracle, engine


def _row(label, where, reachable, by_group):
    total = sum(by_group.values())
    best = max(by_group, key=lambda g: by_group[g]) if total else "-"
    return "| %s | %s | %s | %s | %d |" % (label, where, "reachable" if reachable else "unreachable", best, total)


def _table(oracle, engine):
    lines = ["| branch | where | class | most hits from | hits |", "|---|---|---|---|---|"]
    for name, where, reachable in ORACLE_BRANCHES:
        lines.append(_row("oracle `%s`" % name, where, reachable, {g: c[name] for g, c in oracle.items()}))
    for i, reachable in ENGINE_COUNTERS:
        lines.append(_row("engine counter %d" % i, SC.SB_NAMES[i], reachable,
                          {g: s[i] for g, s in engine.items()}))
    for name, bound in (("max_plies", CO_MAX_PLIES), ("max_path", CO_PATH_MAX)):
        best = max(oracle, key=lambda g: oracle[g][name])
        lines.append("| oracle `%s` | largest seen, bound %d | bound | %s | %d |" % (name, bound, best, oracle[best][name]))
    return "\n".join(lines)


def test_reachable_branches_are_taken_and_unreachable_ones_are_not(census):
    oracle, engine = census
    print("\n" + _table(oracle, engine))
    for name, _, reachable in ORACLE_BRANCHES:
        total = sum(c[name] for c in oracle.values())
        if reachable:
            assert total >= (MIN_EVENTS if name in EVENTS else MIN_HITS), (name, total)
        else:
            assert total == 0, "%s was classed unreachable and is taken %d times: it owes a parity case" % (name, total)
    for i, reachable in ENGINE_COUNTERS:
        total = sum(s[i] for s in engine.values())
        if reachable:
            assert total >= MIN_HITS, (SC.SB_NAMES[i], total)
        else:
            assert total == 0, "engine exit '%s' was classed unreachable and is taken %d times" % (SC.SB_NAMES[i], total)
    assert max(c["max_plies"] for c in oracle.values()) <= CO_MAX_PLIES
    assert max(c["max_path"] for c in oracle.values()) < CO_PATH_MAX


def test_the_new_cases_reach_what_the_old_ones_missed(census):
    """the reason for tests/test_search_paths.py, as numbers: before it the too-deep exit, drawn games and matches and the
    drawn child at a move choice were reached by nothing"""
    oracle, engine = census
    old = ("self-play", "arena", "tournament", "analysis")
    for name in ("game_drawn", "match_drawn", "move_drawn_child"):
        assert sum(oracle[g][name] for g in old) == 0
    assert sum(engine[g][6] for g in ("self-play", "arena")) == 0
    assert engine["deep lines"][6] >= MIN_HITS and engine["deep lines"][20] >= MIN_HITS
    # (6, 120, 40) is in the suite for its second round of pending-leaf records and its later backup batches: it has them
    assert engine["self-play"][25] >= MIN_HITS and engine["self-play"][27] >= MIN_HITS
    assert oracle["arena"]["search_leaf_drawn"] == 0 and oracle["tournament"]["search_leaf_drawn"] == 0
    assert oracle["drawn arena"]["game_drawn"] >= MIN_EVENTS and oracle["drawn tournament"]["match_drawn"] >= MIN_EVENTS


def test_design_holds_the_printed_table(census):
    text = open(os.path.join(SC.ROOT, "DESIGN.md")).read()
    m = re.search(r"<!-- census:begin -->\n(.*?)\n<!-- census:end -->", text, re.S)
    assert m, "DESIGN.md has no census table"
    want = _table(*census)
    assert m.group(1).strip() == want, "DESIGN.md section 2 is out of date; the table is now\n" + want


def test_no_board_has_more_legal_moves_than_a_wavefront_has_lanes():
    """the wide-node exit needs more than 64 edges.  48 is the most any 0/1 board can have (an empty
    square takes at most 3 placements and no move, an occupied one at most 1 placement, and of the 24 pairs of
    neighbours at most one direction is a legal move), whatever set_positions is given; spot-checked here on boards
    nobody could reach by play, with a hill climb from each"""
    rng = np.random.default_rng(5)
    best = 0
    for restart in range(40):
        board = 0
        density = rng.uniform(0.05, 0.6)
        for i in range(64):
            if rng.random() < density:
                board |= 1 << i
        pieces = [int(x) for x in rng.integers(0, 5, 6)] if restart % 2 else [4] * 6
        to_play = int(rng.integers(0, 2))
        cur = bin(O.Game(board, pieces, to_play).legal_mask()[0]).count("1")
        for _ in range(150):
            b2 = board ^ (1 << int(rng.integers(0, 64)))
            c2 = bin(O.Game(b2, pieces, to_play).legal_mask()[0]).count("1")
            if c2 >= cur:
                board, cur = b2, c2
        best = max(best, cur)
    assert 40 <= best <= 48 < CO_WAVE
