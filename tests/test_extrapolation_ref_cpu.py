"""The numpy restatement of ps_set_velocity_extrapolation (extrapolation_ref.py) on the oracle's face labels, without a GPU: its properties,
and that the scenes of the GPU bit comparison (test_gpu_extrapolation.py) tell the rule from its near misses — a reference every plausible
wrong kernel agrees with would check nothing."""
from collections import deque

import numpy as np
import pytest

from polystokes_amd import _abi as abi
from polystokes_amd import scenes

import extrapolation_ref as ref

# the scenes that carry the bit comparison on the GPU, and the two that must not: spheres has a flat front on which the mutants below equal
# the rule, cavity has no invalid face at all
SCENES = {"blob0": lambda: scenes.blob(seed=0), "droplet24": lambda: scenes.droplet(24), "sliding32": lambda: scenes.sliding_block(32),
          "coil32": lambda: scenes.coil(32, tile=8)}
BIT_SCENES = ("blob0", "droplet24", "sliding32", "coil32")
_fields = {}


def fields(oracle_mod, name):
    """(valid[3], vel[3]) of scene `name`: the oracle's face labels and seeded random normal fp32 velocities; computed once, never modified"""
    if name not in _fields:
        sc, p = (SCENES[name] if name in SCENES else {"cavity32": lambda: scenes.cavity(32)}[name])()
        o = oracle_mod.Oracle()
        o.run(sc, p, solve=False)
        sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
        valid, vel = [], []
        for a in range(3):
            lab = o.array("face" + "XYZ"[a] + "Labels").reshape(sh["face" + "XYZ"[a]])
            valid.append(((lab != abi.UNSOLVED) & (lab != abi.UNASSIGNED)).astype(np.float32))
            vel.append(np.random.RandomState(7 + a).standard_normal(lab.shape).astype(np.float32))
        _fields[name] = (valid, vel)
    return _fields[name]


def bfs_distance(valid):
    """6-neighbour graph distance of every face to the nearest valid one (-1: none reachable), by a breadth-first search on flat indices"""
    nz, ny, nx = valid.shape
    dist = np.where(valid.reshape(-1) == 1, 0, -1).astype(np.int64)
    todo = deque(np.flatnonzero(dist == 0).tolist())
    sy, sz = nx, nx * ny
    while todo:
        c = todo.popleft()
        i, j, k = c % nx, (c // nx) % ny, c // sz
        for inside, f in ((i > 0, c - 1), (i + 1 < nx, c + 1), (j > 0, c - sy), (j + 1 < ny, c + sy), (k > 0, c - sz), (k + 1 < nz, c + sz)):
            if inside and dist[f] < 0:
                dist[f] = dist[c] + 1
                todo.append(f)
    return dist.reshape(valid.shape)


def test_the_table_of_the_scenes(oracle_mod):
    """what the scenes offer at 12 layers: invalid X faces, and whether every sweep finds some"""
    want = {"blob0": (11819, 14000), "droplet24": (11664, 14400), "sliding32": (13434, 33792), "coil32": (23276, 33792)}
    for name in BIT_SCENES:
        valid, vel = fields(oracle_mod, name)
        assert (int((valid[0] == 0).sum()), valid[0].size) == want[name], name
        counts = sum(ref.extrapolate(vel[a], valid[a], 12)[2] for a in range(3))
        print(name, list(counts))
        if name in ("blob0", "droplet24"):
            assert np.all(counts > 0), (name, counts)
        if name == "sliding32":
            assert np.all(counts[:11] > 0) and counts[11] == 0, counts          # saturates: the 12th sweep has nothing left
    valid, _ = fields(oracle_mod, "cavity32")
    assert all(np.all(v == 1) for v in valid)


@pytest.mark.parametrize("name", BIT_SCENES)
def test_properties(oracle_mod, name):
    valid, vel = fields(oracle_mod, name)
    layers = 5
    total = np.zeros(layers, np.int64)
    for a in range(3):
        v0, L0, c0 = ref.extrapolate(vel[a], valid[a], 0)
        assert v0.tobytes() == vel[a].tobytes() and len(c0) == 0            # 0 layers: the identity
        assert np.array_equal(L0, np.where(valid[a] == 1, 0, -1))
        v, L, counts = ref.extrapolate(vel[a], valid[a], layers)
        ok = valid[a] == 1
        assert np.array_equal(v[ok], vel[a][ok])                            # valid faces are never changed
        assert np.array_equal(v[L == -1], vel[a][L == -1])                  # nor the faces no sweep reached
        d = bfs_distance(valid[a])
        assert np.array_equal(L, np.where((d >= 0) & (d <= layers), d, -1)), a      # L: the graph distance, capped
        const = np.full(vel[a].shape, np.float32(0.1))                      # (0.1 is not a dyadic rational: a mean that rounded would show)
        vc, Lc, _ = ref.extrapolate(const, valid[a], layers)
        assert np.all(vc == np.float32(0.1)) and np.array_equal(Lc, L)
        total += np.array([(L == k).sum() for k in range(1, layers + 1)])
        assert np.array_equal(counts, [(L == k).sum() for k in range(1, layers + 1)])
    assert total.sum() > 0


def test_the_vectorised_rule_equals_the_face_by_face_rule(oracle_mod):
    valid, vel = fields(oracle_mod, "blob0")
    for a in range(3):
        want = ref.extrapolate_sequential(vel[a], valid[a], 3)
        got = ref.extrapolate(vel[a], valid[a], 3)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), a


def _differs(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@pytest.mark.parametrize("name", BIT_SCENES)
def test_the_inputs_tell_the_rule_from_its_mutants(oracle_mod, name):
    """Each mutant differs from the rule in at least one face, per scene of the bit comparison (and, for the vectorised ones, per axis).
    The one exception is a property of two scenes, not of the rule: sliding32 and coil32 are liquid on a floor under air, so no face the
    sweeps reach has a known face above it, and "+y dropped" equals the rule there (asserted, so that a change of the scenes shows);
    blob0 and droplet24, closed surfaces, catch it on every axis."""
    valid, vel = fields(oracle_mod, name)
    layers = 3
    for a in range(3):
        want = ref.extrapolate(vel[a], valid[a], layers)[0]
        for drop in range(6):                                               # one of the six directions dropped
            dirs = tuple(d for q, d in enumerate(ref.DIRECTIONS) if q != drop)
            n = _differs(ref.extrapolate(vel[a], valid[a], layers, directions=dirs)[0], want)
            if ref.DIRECTIONS[drop] == (1, +1) and name in ("sliding32", "coil32"):
                assert n == 0, (name, a)
            else:
                assert n > 0, (name, a, "direction %d dropped" % drop)
        n32 = _differs(ref.extrapolate(vel[a], valid[a], layers, acc=np.float32)[0], want)      # fp32 accumulation
        print(name, "XYZ"[a], "fp32 accumulation differs in", n32)
        assert n32 > 0, (name, a)
    # neighbours of the same sweep accepted in flat order (one sweep is enough to tell), and the X grid walked with the cell grid's extents
    want = ref.extrapolate(vel[0], valid[0], 1)[0]
    assert _differs(ref.extrapolate_sequential(vel[0], valid[0], 1, same_sweep=True)[0], want) > 0, name
    want = ref.extrapolate(vel[0], valid[0], layers)[0]
    nz, ny, nx1 = vel[0].shape
    cells = nz * ny * (nx1 - 1)
    wrong = want.copy().reshape(-1)
    wrong[:] = vel[0].reshape(-1)
    wrong[:cells] = ref.extrapolate(vel[0].reshape(-1)[:cells].reshape(nz, ny, nx1 - 1), valid[0].reshape(-1)[:cells].reshape(nz, ny, nx1 - 1),
                                    layers)[0].reshape(-1)
    assert _differs(wrong.reshape(want.shape), want) > 0, name


def test_the_two_scenes_that_do_not_discriminate(oracle_mod):
    """spheres32: a flat front, on which "+z dropped" and fp32 accumulation equal the rule (so it must not carry the bit comparison)."""
    sc, p = scenes.spheres(32, tile=8)
    o = oracle_mod.Oracle()
    o.run(sc, p, solve=False)
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    for a in range(3):
        lab = o.array("face" + "XYZ"[a] + "Labels").reshape(sh["face" + "XYZ"[a]])
        valid = ((lab != abi.UNSOLVED) & (lab != abi.UNASSIGNED)).astype(np.float32)
        vel = np.random.RandomState(7 + a).standard_normal(lab.shape).astype(np.float32)
        want = ref.extrapolate(vel, valid, 3)
        assert want[2][0] > 0 and len(set(want[2].tolist())) == 1, want[2]  # the same plane of faces in every sweep
        assert _differs(ref.extrapolate(vel, valid, 3, directions=ref.DIRECTIONS[:5])[0], want[0]) == 0
        assert _differs(ref.extrapolate(vel, valid, 3, acc=np.float32)[0], want[0]) == 0
