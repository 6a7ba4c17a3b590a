"""Sample persistence in the reference's on-disk format (corintho_ai/python/main.pyx:189-219
get_samples): three `np.savez_compressed` files whose single array is stored as `arr_0`:
    <folder>/game_states.npz         [n*8, 70] float32
    <folder>/evaluation_labels.npz   [n*8]     float32
    <folder>/probability_labels.npz  [n*8, 96] float32
so the reference's Keras training step (main.pyx:221-283) consumes them unchanged.

A training run of this package (run.py) keeps the un-augmented samples instead, `save_packed` / `load_packed`:
    <folder>/samples.npz             state_policy [n, 166], outcome [n] float32, uncompressed"""
import os
import zipfile

import numpy as np

from .trainer import GAME_STATE_SIZE, NUM_MOVES, NUM_SYMMETRIES


def get_samples(trainer):
    """main.pyx:193-198: allocate the three arrays and let the trainer fill them"""
    n = trainer.num_samples()
    gs = np.zeros((n * NUM_SYMMETRIES, GAME_STATE_SIZE), dtype=np.float32)
    ev = np.zeros(n * NUM_SYMMETRIES, dtype=np.float32)
    pr = np.zeros((n * NUM_SYMMETRIES, NUM_MOVES), dtype=np.float32)
    if n:
        trainer.writeSamples(gs, ev, pr)
    return gs, ev, pr


def save_samples(sample_folder, game_states, eval_labels, prob_labels):
    """main.pyx:200-204"""
    os.makedirs(sample_folder, exist_ok=True)
    np.savez_compressed(os.path.join(sample_folder, "game_states"), game_states)
    np.savez_compressed(os.path.join(sample_folder, "evaluation_labels"), eval_labels)
    np.savez_compressed(os.path.join(sample_folder, "probability_labels"), prob_labels)


def load_samples(sample_folder):
    """the reader side of main.pyx:208-216"""
    out = []
    for name, shape in (("game_states", (-1, GAME_STATE_SIZE)), ("evaluation_labels", (-1,)),
                        ("probability_labels", (-1, NUM_MOVES))):
        with np.load(os.path.join(sample_folder, name + ".npz")) as z:
            out.append(np.reshape(z["arr_0"], shape))
    return tuple(out)


PACKED_FILE = "samples.npz"
SAMPLE_FLOATS = GAME_STATE_SIZE + NUM_MOVES


def write_npz(path, arrays):
    """An uncompressed .npz that np.load reads, written to a temporary file and moved into place.  Unlike np.savez the
    members carry no time stamp, so equal arrays give equal bytes (a resumed run's files equal an uninterrupted run's)."""
    tmp = path + ".tmp"
    with zipfile.ZipFile(tmp, "w", zipfile.ZIP_STORED, allowZip64=True) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asarray(a), allow_pickle=False)
    os.replace(tmp, path)


def _check_packed(state_policy, outcome, where):
    sp, oc = np.asarray(state_policy), np.asarray(outcome)
    if sp.ndim != 2 or sp.shape[1] != SAMPLE_FLOATS or oc.shape != (sp.shape[0],):
        raise ValueError("%s: state_policy must be [n, %d] and outcome [n], got %s and %s"
                         % (where, SAMPLE_FLOATS, sp.shape, oc.shape))
    return np.ascontiguousarray(sp, dtype=np.float32), np.ascontiguousarray(oc, dtype=np.float32)


def save_packed(sample_folder, state_policy, outcome):
    """The un-augmented samples of Trainer.export_samples as <folder>/samples.npz (state_policy [n, 166], outcome [n]),
    uncompressed: an eighth of the bytes of the three expanded files, and no deflate on the host."""
    sp, oc = _check_packed(state_policy, outcome, "save_packed")
    os.makedirs(sample_folder, exist_ok=True)
    write_npz(os.path.join(sample_folder, PACKED_FILE), {"state_policy": sp, "outcome": oc})


def load_packed(sample_folder):
    """(state_policy, outcome) of a sample folder.  A folder that holds only the reference's three files gives their
    symmetry-0 rows: Trainer::writeSamples puts sample i under symmetry s at row 8 i + s (trainer.cpp:103-113), and
    symmetry 0 is the position as played."""
    path = os.path.join(sample_folder, PACKED_FILE)
    if os.path.exists(path):
        with np.load(path) as z:
            return _check_packed(z["state_policy"], z["outcome"], path)
    gs, ev, pr = load_samples(sample_folder)
    if gs.shape[0] % NUM_SYMMETRIES or ev.shape[0] != gs.shape[0] or pr.shape[0] != gs.shape[0]:
        raise ValueError("%s: %d, %d and %d rows are not the 8 symmetries of one sample set"
                         % (sample_folder, gs.shape[0], ev.shape[0], pr.shape[0]))
    return _check_packed(np.concatenate([gs[::NUM_SYMMETRIES], pr[::NUM_SYMMETRIES]], axis=1), ev[::NUM_SYMMETRIES],
                         sample_folder)


AUGMENTATIONS = {"reference": 0, "consistent": 1}  # CA_AUG_* of include/corintho_hip.h
_TABLES = None


def symmetry_tables():
    """(space [8, 16], move [8, 96], move_consistent [8, 96]) int32: the symmetry tables the kernels gather through,
    read from the initialisers of csrc/tables.inc that they are compiled from.  space and move are the reference's
    space_symmetries and move_symmetries.  move_consistent is move with rows 2 and 6 exchanged (row k ^ 4 where
    (k & 3) == 2): the move table that belongs to space, row for row ("Canonical orientation")."""
    global _TABLES
    if _TABLES is None:
        import re
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "tables.inc"), encoding="utf-8") as f:
            text = f.read()
        out = []
        for name, width in (("CO_SPACE_SYM_INIT", 16), ("CO_MOVE_SYM_INIT", NUM_MOVES)):
            m = re.search(r"#define %s \{(.*?)\n\}" % name, text, re.S)
            if not m:
                raise ValueError("csrc/tables.inc: no %s" % name)
            t = np.array([int(x) for x in re.findall(r"\d+", m.group(1))], np.int32)
            if t.size != NUM_SYMMETRIES * width:
                raise ValueError("csrc/tables.inc: %s has %d entries" % (name, t.size))
            out.append(t.reshape(NUM_SYMMETRIES, width))
        space, move = out
        consistent = move[[k ^ 4 if (k & 3) == 2 else k for k in range(NUM_SYMMETRIES)]]
        for t in (space, move, consistent):
            t.setflags(write=False)
        _TABLES = (space, move, consistent)
    return _TABLES


def _state_gather(space):
    """[8, 70]: where the cells of a state under symmetry k come from (cells 64..69 do not move)"""
    c = np.arange(GAME_STATE_SIZE)
    board = space[:, np.minimum(c, 63) >> 2] * 4 + (c & 3)
    return np.where(c < 64, board, c)


def _augmentation(augmentation, who):
    if augmentation not in AUGMENTATIONS:
        raise ValueError('%s: augmentation must be "reference" or "consistent", not %r' % (who, augmentation))
    return augmentation


def expand_host(state_policy, outcome, augmentation="reference"):
    """The eight symmetry copies of un-augmented samples in plain numpy: -> (game_states [8 n, 70], eval_labels [8 n],
    prob_labels [8 n, 96]) in Trainer.writeSamples' row order, sample i under symmetry k at row 8 i + k.  The state goes
    through space[k]; the policy through move[k] ("reference": what the reference, writeSamples and expand_samples do)
    or through move_consistent[k] ("consistent": rows 8 i + 2 and 8 i + 6 then carry each other's policy)."""
    sp, oc = _check_packed(state_policy, outcome, "expand_host")
    space, move, consistent = symmetry_tables()
    table = consistent if _augmentation(augmentation, "expand_host") == "consistent" else move
    n = sp.shape[0]
    states = sp[:, :GAME_STATE_SIZE][:, _state_gather(space)]  # [n, 8, 70]
    probs = sp[:, GAME_STATE_SIZE:][:, table]                  # [n, 8, 96]
    return (np.ascontiguousarray(states.reshape(n * NUM_SYMMETRIES, GAME_STATE_SIZE)), np.repeat(oc, NUM_SYMMETRIES),
            np.ascontiguousarray(probs.reshape(n * NUM_SYMMETRIES, NUM_MOVES)))


def canonicalize_host(state_policy):
    """The canonical orientation of un-augmented samples: -> (state_policy [n, 166] float32, k_star [n] int32).  This
    is the definition that Fitter.canonicalize computes on the device, bit for bit.

    Of a sample (s, p) the eight candidates are s_k[c] = s[space[k][c >> 2] * 4 + (c & 3)] for c < 64; cells 64..69 do
    not move.  k* is the k whose candidate is smallest when words 0..63 are compared in ascending order as unsigned
    32-bit patterns (so -0.0 sorts after 0.0), the lowest k on a tie.  The canonical sample is
    (s_k*, p[move_consistent[k*]]): the policy always moves through the consistent table, the only pairing with the
    space table that is a group action.  Samples that are images of one another get the same state."""
    sp = np.ascontiguousarray(state_policy, dtype=np.float32)
    if sp.ndim != 2 or sp.shape[1] != SAMPLE_FLOATS:
        raise ValueError("canonicalize_host: state_policy must be [n, %d], got %s" % (SAMPLE_FLOATS, sp.shape))
    space, _, consistent = symmetry_tables()
    n = sp.shape[0]
    if n == 0:
        return sp.copy(), np.zeros(0, np.int32)
    cand = sp[:, :GAME_STATE_SIZE][:, _state_gather(space)]  # [n, 8, 70]
    words = np.ascontiguousarray(cand[:, :, :64]).view(np.uint32)
    rows = np.arange(n)
    k_star = np.zeros(n, np.int32)
    best = words[:, 0]
    for k in range(1, NUM_SYMMETRIES):  # candidate k against the best so far: the first word that differs decides
        differs = words[:, k] != best
        at = np.argmax(differs, axis=1)
        better = differs.any(axis=1) & (words[rows, k, at] < best[rows, at])
        best = np.where(better[:, None], words[:, k], best)
        k_star[better] = k
    policy = sp[:, GAME_STATE_SIZE:][rows[:, None], consistent[k_star]]
    return np.ascontiguousarray(np.concatenate([cand[rows, k_star], policy], axis=1)), k_star


def merge_duplicates_host(state_policy, outcome, weights=None, normalize=True, symmetries=False):
    """Merge the duplicate positions of un-augmented samples: -> (state_policy, outcome, weights) float32.  This is the
    definition that Fitter.merge_duplicates computes on the device, bit for bit.  symmetries: the samples are brought
    into their canonical orientation first (canonicalize_host), so that positions which are images of one another
    under the eight symmetries merge as well; everything below then holds of the canonical samples.

    Two samples are equal when their 70 state floats have the same bit patterns.  A group of equal samples becomes one
    sample at the rank of its first member (groups keep the order of their first members).  With w_i the members'
    weights (`weights`, or 1) and every sum taken in float64 over the members in ascending index:
        W = sum w_i,   policy[m] = (sum w_i p_i[m]) / W,   outcome = (sum w_i z_i) / W,
    each rounded once to float32; the new weight is W.  A group with W = 0 has no mean: it is dropped, and its
    weight-0 members with it.  normalize: every weight is then W * (after / sum W), in float64 with the groups' W summed
    in order, rounded once, so that the weights have mean one and a weighted fit keeps an unweighted one's loss scale."""
    sp, oc = _check_packed(state_policy, outcome, "merge_duplicates_host")
    if symmetries:
        sp = canonicalize_host(sp)[0]
    n = sp.shape[0]
    if weights is None:
        w = np.ones(n, np.float64)
    else:
        w = np.ascontiguousarray(weights, dtype=np.float32).ravel().astype(np.float64)
        if w.size != n or not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("merge_duplicates_host: weights must be [n], finite and >= 0")
    if n == 0:
        return sp, oc, w.astype(np.float32)
    # groups by the states' bytes, numbered in the order of their first members
    keys = np.ascontiguousarray(sp[:, :GAME_STATE_SIZE]).view(np.dtype((np.void, 4 * GAME_STATE_SIZE))).ravel()
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    number = np.empty(order.size, np.int64)
    number[order] = np.arange(order.size)
    group = number[np.asarray(inverse).ravel()]
    first = first[order]
    # np.add.at applies its terms one by one in index order: the members in ascending index
    wsum = np.zeros(first.size, np.float64)
    acc = np.zeros((first.size, NUM_MOVES + 1), np.float64)
    np.add.at(wsum, group, w)
    terms = np.concatenate([sp[:, GAME_STATE_SIZE:], oc[:, None]], axis=1).astype(np.float64) * w[:, None]
    np.add.at(acc, group, terms)
    keep = wsum > 0
    first, wsum, acc = first[keep], wsum[keep], acc[keep]
    mean = (acc / wsum[:, None]).astype(np.float32)
    out_sp = np.concatenate([sp[first, :GAME_STATE_SIZE], mean[:, :NUM_MOVES]], axis=1)
    if normalize and wsum.size:
        total = np.cumsum(wsum)[-1]  # a running sum, in order (np.sum adds pairwise), as the device's summing thread
        wsum = wsum * (np.float64(wsum.size) / total)
    return np.ascontiguousarray(out_sp), np.ascontiguousarray(mean[:, NUM_MOVES]), wsum.astype(np.float32)


def samples_for_training(trainer, sample_folder, old_training_samples=(), mix_old=False):
    """The whole of get_samples (main.pyx:189-219): fetch this generation's samples, save them, then walk the
    replay window `old_training_samples` (folders of earlier generations, wrapper.py passes the last few).

    The reference loads every old generation and calls np.concatenate on it -- and DISCARDS the result
    (main.pyx:212-214), so what it returns, and trains on, is the current generation alone.  That is
    reproduced by default (the old files are still opened, read and shape-checked like the reference does,
    so a corrupt window fails here too).  mix_old=True returns what the code evidently meant: the current
    samples followed by the window's."""
    game_states, eval_labels, prob_labels = get_samples(trainer)
    save_samples(sample_folder, game_states, eval_labels, prob_labels)
    for cur_path in old_training_samples:
        old_gs, old_ev, old_pr = load_samples(cur_path)
        a = np.concatenate((game_states, old_gs))
        b = np.concatenate((eval_labels, old_ev))
        c = np.concatenate((prob_labels, old_pr))
        if mix_old:
            game_states, eval_labels, prob_labels = a, b, c
    return game_states, eval_labels, prob_labels
