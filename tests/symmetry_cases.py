"""Samples for the tests of the consistent augmentation and of the canonical orientation (tests/test_symmetry_aug_*.py,
tests/test_canonical_*.py): images of samples under the eight symmetries, stabilisers, planted orbits."""
import numpy as np

from corintho_ai_amd import samples_io
from tests import fit_ref

GS, NM = 70, 96


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def gather():
    """[8, 70]: the cell of the state that cell c of its image under symmetry k comes from"""
    return samples_io._state_gather(samples_io.symmetry_tables()[0])


def image(sp, j):
    """E_j of every sample of sp [n, 166] (j a number, or one per sample): the state through the space table, the policy
    through the consistent move table -- the joint action of the eight symmetries"""
    sp = np.atleast_2d(np.asarray(sp, np.float32))
    j = np.broadcast_to(np.asarray(j), (sp.shape[0],))
    rows = np.arange(sp.shape[0])[:, None]
    mc = samples_io.symmetry_tables()[2]
    return np.ascontiguousarray(np.concatenate([sp[:, :GS][rows, gather()[j]], sp[:, GS:][rows, mc[j]]], axis=1))


def stabiliser(state):
    """the symmetries that leave the state's bit patterns as they are"""
    s = np.ascontiguousarray(state, np.float32)
    return [k for k in range(8) if same(s[gather()[k]], s)]


def samples(n, seed):
    """n synthetic samples (state_policy, outcome) whose states have a trivial stabiliser and lie in n different orbits"""
    s, z, p = fit_ref.synthetic_samples(n, seed)
    sp = np.ascontiguousarray(np.concatenate([s, p], axis=1), np.float32)
    assert all(stabiliser(row[:GS]) == [0] for row in sp)
    canon = samples_io.canonicalize_host(sp)[0]
    assert np.unique(canon[:, :GS], axis=0).shape[0] == n
    return sp, np.ascontiguousarray(z, np.float32)


def start_position():
    """the state of the empty board with all pieces in hand: every symmetry leaves it as it is"""
    from oracle import oracle as O
    return O.Game().state()


def planted(orbits, count, seed, exact=0):
    """`count` samples in `orbits` orbits: sample i is a seeded image of base sample orbit_of[i], with a policy and an
    outcome of its own; every orbit occurs.  exact: that many of the samples repeat the state of the sample before
    them bit for bit (an exact duplicate).  -> (state_policy, outcome, orbit_of)"""
    rng = np.random.default_rng(seed)
    base = samples(orbits, seed + 1)[0]
    orbit_of = rng.permutation(np.concatenate([np.arange(orbits), rng.integers(0, orbits, count - orbits)]))
    _, z, p = fit_ref.synthetic_samples(count, seed + 2)
    sp = image(base[orbit_of], rng.integers(0, 8, count))
    sp[:, GS:] = p
    for i in rng.choice(np.arange(1, count), exact, replace=False):
        sp[i, :GS] = sp[i - 1, :GS]
        orbit_of[i] = orbit_of[i - 1]
    return np.ascontiguousarray(sp, np.float32), np.ascontiguousarray(z, np.float32), orbit_of


def canonical_cases():
    """the set of tests/test_canonical_gpu.py, 257 samples (state_policy, outcome) -- all eight images of three base
    samples; states that differ from an image in board word 63 alone and in board word 0 alone (the decision falls on the
    last and on the first lane); a state with a two-element stabiliser; the start position; a -0.0 word; the rest single
    samples in orientations of their own"""
    base, _ = samples(3, 71)
    rows = [image(b, k)[0] for b in base for k in range(8)]                      # 24
    for word in (63, 0):
        for k in (1, 2, 5):
            r = image(base[0], k)[0]
            r[word] = np.float32(1.0) - r[word]  # (the boards are binary)
            rows.append(r)                                                        # 6
    half = base[1].copy()                                                         # symmetric under k = 1 alone
    half[:GS] = np.maximum(half[:GS], half[:GS][gather()[1]])
    assert stabiliser(half[:GS]) == [0, 1]
    rows += [image(half, k)[0] for k in (0, 2, 7)]                                # 3
    late = half.copy()  # the symmetry broken in the last row alone: candidates 0 and 1 agree in words 0..50
    late[63] = np.float32(1.0) - late[63]
    assert int(np.flatnonzero(late[:64] != late[:GS][gather()[1]][:64])[0]) == 51
    rows += [late, image(late, 1)[0]]                                             # 2
    start = np.concatenate([start_position(), base[2][GS:]]).astype(np.float32)
    assert stabiliser(start[:GS]) == list(range(8))
    rows.append(start)                                                            # 1
    for k in (0, 3):
        r = image(base[2], k)[0]
        zero = int(np.flatnonzero(r[:64] == 0.0)[0])
        r[zero] = np.float32(-0.0)
        rows.append(r)                                                            # 2
    more, _ = samples(257 - len(rows), 72)
    rng = np.random.default_rng(73)
    sp = np.concatenate([np.stack(rows), image(more, rng.integers(0, 8, more.shape[0]))])
    sp = np.ascontiguousarray(sp[rng.permutation(257)], np.float32)
    oc = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), 257)
    return sp, oc
