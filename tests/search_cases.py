"""The fast search cases of the suite as data, and how each runs on the oracle alone: what
tests/test_search_census_cpu.py counts branches over, and what tests/test_search_paths.py adds.

A self-play case is (G, sims, spe, eps, c_puct, seed, net, stagger, game_base, total_games, testing); `net` names a
stand-in network of NETS (arena mode plays NETS[net] with salts 1 and 2, as test_arena_mode_matches_oracle does)."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle as O
from tests import harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SelfPlay = collections.namedtuple("SelfPlay", "G sims spe eps c_puct seed net stagger game_base total_games testing",
                                  defaults=(0.25, 1.0, 12345, "hash", True, 0, 0, False))

NETS = {
    "hash": lambda salt=0: (lambda s: H.hash_net(s, salt)),
    "peaked": lambda salt=0: H.peaked_net(32.0, value_scale=0.1, salt=salt),       # long lines, values that still steer
    "peaked_low": lambda salt=0: H.peaked_net(32.0, value_const=-0.9, salt=salt),  # every leaf looks lost to its mover
    "peaked64_low": lambda salt=0: H.peaked_net(64.0, value_const=-0.9, salt=salt),  # ... and one line takes nearly all
}


def nets_of(case):
    """-> (net, nets_by_player) as harness.play_generation takes them"""
    if case.testing:
        return None, (NETS[case.net](1), NETS[case.net](2))
    return NETS[case.net](), None


# ---- what the suite had before: tests/test_engine_parity.py (CASES, the c_puct 3 case, arena mode, writeScores, shards)
OLD_SELFPLAY = [
    SelfPlay(64, 50, 16), SelfPlay(16, 50, 1), SelfPlay(8, 200, 16, 0.0), SelfPlay(6, 400, 16), SelfPlay(40, 8, 4),
    SelfPlay(5, 1, 1), SelfPlay(5, 2, 1), SelfPlay(5, 3, 2), SelfPlay(6, 120, 40),
    SelfPlay(12, 64, 16, 0.25, 3.0, 99, "hash", False),
    SelfPlay(14, 24, 8, seed=21),
    SelfPlay(12, 24, 8, seed=77, stagger=False),
]
OLD_ARENA = [SelfPlay(10, 40, 8, seed=5, testing=True), SelfPlay(14, 24, 8, seed=21, testing=True)]

# ---- what tests/test_search_paths.py adds
# the counts are the emulation build's grouped-search exits and levels (search_group.h counters 6, 20, 23)
DEEP = [
    SelfPlay(8, 200, 16, 0.0, net="peaked", stagger=False),        # too deep 198, shared levels 1865, row form 14513
    SelfPlay(6, 400, 16, 0.25, net="peaked_low", stagger=False),   # too deep 73, shared 2524, row form 11467
    SelfPlay(4, 200, 16, 0.0, net="peaked64_low", stagger=False),  # all four rows in one node: shared 1073 in 2553 groups
]
# 8-game slices of 2048-game generations (8 simulations, 4 per evaluation, no stagger) around a game the oracle draws:
# games 1975 and 1099 (found by playing the whole generations on the oracle)
DRAWN = [
    SelfPlay(8, 8, 4, seed=12345, stagger=False, game_base=1972, total_games=2048),
    SelfPlay(8, 8, 4, seed=7, stagger=False, game_base=1096, total_games=2048),
]
# arena games are not independent of their neighbours (a model's first call after the other's turn reads the rows that
# are still in the buffers, main.pyx:150-154), so no slices: whole 8-game arenas with a drawn game, seeds found by scanning
DRAWN_ARENA = [SelfPlay(8, 8, 4, seed=16, testing=True), SelfPlay(8, 8, 4, seed=441, testing=True)]
# the FewSearches corner in arena mode: one simulation per move, so every move finds a root without a visited child and
# starts a fresh tree (choose_move_normal's reset; the training games of that corner take the opening's reset instead)
FEW_ARENA = [SelfPlay(5, 1, 1, testing=True)]
# 8-match tournaments with a drawn match (match 2, model against the random player), salts found by scanning
# (player_id, model_id, max_searches, spe, c_puct, epsilon, random)
DRAWN_TOURNEY_PLAYERS = [(0, 0, 8, 4, 1.0, 0.25, False), (1, 1, 8, 4, 1.0, 0.25, False), (2, -1, 0, 0, 1.0, 0.25, True)]
DRAWN_TOURNEY_MATCHES = [(0, 1), (1, 0), (0, 2), (2, 1)] * 2
DRAWN_TOURNEY_SALTS = [2, 18]


def drawn_tourney_nets(salt):
    return {0: lambda s: H.hash_net(s, 1000 + salt), 1: lambda s: H.hash_net(s, 2000 + salt)}


def build_tourney(factory, players, matches):
    t = factory()
    for p in players:
        t.addPlayer(*p)
    for a, b in matches:
        t.addMatch(a, b, False)
    return t


def tourney_rows(players, matches):
    spe = {p[0]: p[3] for p in players}
    return max(1, sum(spe[a] + spe[b] for a, b in matches))


# ---- positions for the Analyser (tools/gen_search_paths_golden.py)
ANALYSIS_SETTINGS = [(48, 8), (200, 16), (7, 1)]
ANALYSIS_NETS = ["hash", "peaked"]


def load_positions():
    d = np.load(os.path.join(ROOT, "tests", "golden", "search_paths_positions.npz"))
    return (d["boards"].astype(np.int32), d["to_play"].astype(np.int32), d["pieces"].astype(np.int32),
            d["seeds"].astype(np.int32), d["kind"], [str(k) for k in d["kinds"]])


def analyse_on_oracle(board, tp, pc, seed, sims, spe, net):
    """docker/choose_move.pyx:155-221 with a fixed search budget (as tests/test_analyse.py drives it)"""
    mc = O.DockerMC(int(seed), sims, spe, 1.0, 0.25, board, int(tp), pc)
    if mc.done():
        return {"pre-result": "draw" if mc.drawn() else "win"}, []
    evals = np.zeros(spe, np.float32)
    probs = np.zeros((spe, 96), np.float32)
    gs = np.zeros((spe, 70), np.float32)
    log = []
    while not mc.doIteration(evals, probs):
        n = mc.num_requests()
        if n == 0:
            break
        mc.writeRequests(gs)
        e, p = net(gs[:n])
        evals[:n] = e
        probs[:n] = p
        log.append(gs[:n].copy())
    move = mc.chooseMove()
    done = mc.done()
    nodes = mc.num_nodes()
    ev = mc.eval()
    return {"move": move, "is_done": done, "has_won": bool(done and not mc.drawn()),
            "legal_moves": [] if done else [i for i in range(96) if mc.getLegalMoves()[i]],
            "nodes_searched": nodes, "eval_sum": ev}, log


def run_selfplay_on_oracle(case, trace=False):
    o = O.Trainer(case.G, seed=case.seed, max_searches=case.sims, searches_per_eval=case.spe, c_puct=case.c_puct,
                  epsilon=case.eps, num_threads=4, testing=case.testing, game_base=case.game_base,
                  total_games=case.total_games)
    if trace:
        o.enable_trace()
    o.set_stagger(case.stagger)
    net, pair = nets_of(case)
    r = H.play_generation(o, case.G, case.spe, net, nets_by_player=pair, record=trace)
    return o, r


# ---- the engine's structural counters (search_state.h CO_SBS, -DCO_SB_STATS on the emulation build)
SB_NAMES = {3: "co_search_rows: nothing searchable", 4: "co_search_rows: terminal child", 5: "co_search_rows: wide node",
            6: "co_search_rows: too deep", 7: "co_search_rows: terminal leaf / full arena", 8: "sequential simulations",
            12: "groups committing 0", 13: "groups committing 1", 14: "groups committing 2", 15: "groups committing 3",
            16: "groups committing 4", 20: "co_search_rows: shared levels", 23: "co_search_rows: row-form levels",
            24: "co_search_rows: row-form turns", 25: "co_receive_eval: record rounds beyond 16 leaves",
            26: "co_receive_eval: backup batches", 27: "co_receive_eval: backup batches beyond 8 leaves",
            28: "co_prior_all: pass of 1 leaf", 29: "co_prior_all: pass of 2 leaves", 30: "co_prior_all: pass of 3 leaves",
            31: "co_prior_all: pass of 4 leaves"}


def sb_stats_lib(directory):
    """build the emulation engine with its grouped-search counters into `directory` (as tools/sb_stats.py does) and
    load it beside the normal emulation library"""
    from corintho_ai_amd import _lib

    so = os.path.join(str(directory), "libcorintho_emu_sbstats.so")
    if not os.path.exists(so):
        csrc = os.path.join(ROOT, "corintho_ai_amd", "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCO_EMU", "-DCO_SB_STATS", "-ffp-contract=off",
                               "-fno-fast-math", "-fopenmp", "-fPIC", "-Wno-unknown-pragmas", "-shared", "-o", so, "-x",
                               "c++", os.path.join(csrc, "engine.hip"), "-x", "c++",
                               os.path.join(ROOT, "tests", "emu", "nn_emu.cpp"), "-lm"])
    L = _lib.declare(C.CDLL(so))
    L.co_emu_sb_stats.restype = C.POINTER(C.c_ulonglong)
    return L


def sb_read(L):
    p = L.co_emu_sb_stats()
    return [int(p[i]) for i in range(32)]


def sb_reset(L):
    C.memset(L.co_emu_sb_stats(), 0, 32 * 8)


def run_selfplay_on_engine(L, case, trace=False):
    from corintho_ai_amd import trainer as T

    t = T.Trainer(case.G, "", case.seed, case.sims, case.spe, case.c_puct, case.eps, 0, 1, case.testing, _cdll=L,
                  trace=trace, stagger=case.stagger, game_base=case.game_base, total_games=case.total_games)
    net, pair = nets_of(case)
    r = H.play_generation(t, case.G, case.spe, net, nets_by_player=pair, record=trace)
    return t, r
