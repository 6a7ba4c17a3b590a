"""Writes tests/golden/search_paths_positions.npz: positions for the batched Analyser that sit where the search's rare
paths are (tests/test_search_paths.py), all taken from uniformly random playouts on the CPU oracle:

  before_draw      1-4 plies before a playout ended drawn (no legal move, no line)
  before_decisive  1-4 plies before one ended lost for the side to move
  one_move         exactly one legal move
  empty_reserve    the side to move has no piece left to place
  drawn_child      at least four legal moves, one of which ends the game drawn, and the oracle's 48-simulation search
                   with hash_net still weighs that drawn child when it chooses its move (the oracle's census says so)
  terminal         terminal as given, drawn and lost (the pre-result path; at most a quarter of the corpus)

    python tools/gen_search_paths_golden.py        # CPU only, a minute or two (the drawn_child positions are searched for)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "search_paths_positions.npz")
KINDS = ("before_draw", "before_decisive", "one_move", "empty_reserve", "drawn_child", "terminal")
WANT = {"before_draw": 16, "before_decisive": 16, "one_move": 10, "empty_reserve": 10, "drawn_child": 6, "terminal": 8}


def playout(O, rng):
    """-> the positions of one random game as (board, to_play, pieces, number of legal moves), the terminal one last"""
    g = O.Game()
    line = []
    while True:
        mask, _ = g.legal_mask()
        moves = [i for i in range(96) if mask >> i & 1]
        line.append((g.board, g.to_play, tuple(int(x) for x in g.pieces), len(moves)))
        if not moves:
            return line, g.terminal_result()
        g.do_move(int(rng.choice(moves)))


def weighs_a_drawn_child(O, pos):
    """does the move choice of a (48, 8) search from `pos` look at a drawn child of a root that is not decided?"""
    from tests import harness as H

    board, tp, pc, nlegal = pos
    if nlegal < 4:
        return False
    for m in range(96):
        g = O.Game(board, pc, tp)
        if g.legal_mask()[0] >> m & 1:
            g.do_move(m)
            if g.terminal_result() == 2:
                break
    else:
        return False
    mc = O.DockerMC(3, 48, 8, 1.0, 0.25, [(board >> b) & 1 for b in range(64)], tp, list(pc))
    ev, pr, gs = np.zeros(8, np.float32), np.zeros((8, 96), np.float32), np.zeros((8, 70), np.float32)
    while not mc.doIteration(ev, pr):
        n = mc.num_requests()
        if n == 0:
            break
        mc.writeRequests(gs)
        ev[:n], pr[:n] = H.hash_net(gs[:n])
    O.census_reset()
    mc.chooseMove()
    return O.census()["move_drawn_child"] > 0


def main():
    from oracle import oracle as O

    rng = np.random.default_rng(20240611)
    got = {k: [] for k in KINDS}
    seen = set()
    terminal_by_result = {1: 0, 2: 0}

    def take(kind, pos):
        if len(got[kind]) < WANT[kind] and pos[:3] not in seen:
            seen.add(pos[:3])
            got[kind].append(pos)
            return True
        return False

    games = 0
    while any(len(got[k]) < WANT[k] for k in KINDS):
        line, result = playout(O, rng)  # result: 1 lost, 2 drawn for the side to move
        games += 1
        before = "before_draw" if result == 2 else "before_decisive"
        if len(got[before]) + 4 <= WANT[before] and len(line) > 4:
            for back in (1, 2, 3, 4):
                take(before, line[-1 - back])
        elif terminal_by_result[result] < WANT["terminal"] // 2 and take("terminal", line[-1]):
            terminal_by_result[result] += 1
        else:
            if len(got["drawn_child"]) < WANT["drawn_child"]:
                for pos in line[12:-1]:
                    if pos[:3] not in seen and weighs_a_drawn_child(O, pos):
                        take("drawn_child", pos)
                        break
            for pos in line[:-5]:
                mine = pos[2][3 * pos[1]:3 * pos[1] + 3]
                if pos[3] == 1 and take("one_move", pos):
                    break
                if pos[3] > 1 and sum(mine) == 0 and take("empty_reserve", pos):
                    break
    n = sum(WANT.values())
    boards = np.zeros((n, 64), np.int8)
    to_play = np.zeros(n, np.int8)
    pieces = np.zeros((n, 6), np.int8)
    kind = np.zeros(n, np.int8)
    i = 0
    for k, name in enumerate(KINDS):
        for board, tp, pc, _ in got[name]:
            boards[i] = [(board >> b) & 1 for b in range(64)]
            to_play[i], pieces[i], kind[i] = tp, pc, k
            i += 1
    seeds = (np.arange(n, dtype=np.int32) * 7 + 3).astype(np.int32)
    np.savez_compressed(OUT, boards=boards, to_play=to_play, pieces=pieces, seeds=seeds, kind=kind,
                        kinds=np.array(KINDS))
    O.census_reset()
    print("%s: %d positions from %d playouts, %d bytes" % (OUT, n, games, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
