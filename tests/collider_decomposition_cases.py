"""Inputs shared by the tests of collider placement and painting on slab and brick ranks (test_collider_decomposition_cpu.py,
test_gpu_collider_decomposition.py), and the child process of the cull test:  python collider_decomposition_cases.py ranks <case>  prints
one digest over what a place and a paint leave on every rank of the case's group.

A rank runs both rules on its own grid, from the orig of its own upload (partition.local_orig).  rank_expected() is therefore the two
restatements (collider_shapes_ref.py, collider_motions_ref.py) run on the rank's cut arrays with the rank's orig; it is not a slice of the
global result.  test_collider_decomposition_cpu.py shows where the two agree and the one place where they do not.

Box cases: random SDF values in the world and in the volumes, tile 8, never stepped.  Lengths are given in cells: every case takes
dx = 1/64 (and half of them the dyadic orig (0.375, -1.25, 2.5)), so that orig_r + (i + 0.5) * dx is exact on a rank and in the whole grid
alike and the two results agree by arithmetic, except box_offgrid_orig (dx = 0.05, orig (0.3, -1.1, 2.7)), where they agree for the seed
noted at its entry.  Every case holds
  volume 0   large, about the crossing of the first cuts: it reaches every cell of the grid, on both sides of every cut;
  volume 1   across the first cut of the first cut axis alone;
  volume 2   small, about cell 40 along every cut axis: inside the halo block [32, 48) of the rank that owns [0, 32), owned by another;
  volume 3   wholly off the grid;
  volume 4   across the last cut of the last cut axis;
uploaded ids 0 .. 5 (5 lies outside the count), a random uploaded collisionvel, and the motions of collider_motions_cases.table("random")."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from polystokes_amd import _abi as abi  # noqa: E402
from polystokes_amd import partition  # noqa: E402
from polystokes_amd import scenes  # noqa: E402

import collider_motions_cases as motions_cases  # noqa: E402
import collider_motions_ref as motions_ref  # noqa: E402
import collider_shapes_cases as shapes_cases  # noqa: E402
import collider_shapes_ref as shapes_ref  # noqa: E402
from collider_shapes_cases import pose, rotation, sphere_volume, volume  # noqa: E402

GRID_ARRAYS = motions_cases.GRID_ARRAYS
PLACED = ("collisionField", "colliderCellIds", "colliderPlacedCells")
PAINTED = GRID_ARRAYS + ("colliderMotionFaces",)
DYADIC_ORIG = (0.375, -1.25, 2.5)
TILE = 8

# grid (nx, ny, nz), bricks (None: z-slabs), ranks, negateCollision, orig, dx, base ("random" / "ties"), volumes ("five" / "count64"),
# uploaded ids ("mod6" / "mod67" / None), seed
CASES = {
    "box_x": ((48, 12, 20), (2, 1, 1), 2, 1, (0.0, 0.0, 0.0), 1.0 / 64.0, "random", "five", "mod6", 21),
    "box_xz": ((48, 12, 48), (2, 1, 2), 4, 1, DYADIC_ORIG, 1.0 / 64.0, "random", "five", "mod6", 21),
    "box_z3": ((20, 12, 64), None, 3, 1, (0.0, 0.0, 0.0), 1.0 / 64.0, "random", "five", "mod6", 21),
    "box_xyz": ((48, 48, 48), (2, 2, 2), 8, 1, DYADIC_ORIG, 1.0 / 64.0, "random", "five", "mod6", 21),
    "box_no_negate": ((48, 12, 20), (2, 1, 1), 2, 0, DYADIC_ORIG, 1.0 / 64.0, "random", "five", "mod6", 21),
    "box_ties": ((48, 12, 48), (2, 1, 2), 4, 1, (0.0, 0.0, 0.0), 1.0 / 64.0, "ties", "five", "mod6", 21),
    "box_count64": ((48, 12, 48), (2, 1, 2), 4, 1, DYADIC_ORIG, 1.0 / 64.0, "random", "count64", "mod67", 21),
    "box_no_ids": ((48, 12, 48), (2, 1, 2), 4, 1, (0.0, 0.0, 0.0), 1.0 / 64.0, "random", "five", None, 21),
    # seed 21: the rank results equal the cuts of the global result in every cell and face outside the outer planes (the first seed tried;
    # with this dx and orig a position on a rank can differ from the global one by an ulp, so the equality is a property of the seed)
    "box_offgrid_orig": ((48, 12, 48), (2, 1, 2), 4, 1, (0.3, -1.1, 2.7), 0.05, "random", "five", "mod6", 21),
}
STEP_CASES = {"spheres64_b2x1x2": ((2, 1, 2), 4), "spheres64_w3": (None, 3)}
_built = {}


class Geometry:
    """A slab or a brick as three-axis lists (x, y, z): origin (global index of local cell 0), n (local cells), lo / hi (the owned range in
    local cells), hasLower / hasUpper."""

    def __init__(self, part, n_global):
        if isinstance(part, partition.Slab):
            nx, ny, _ = n_global
            self.origin, self.n = [0, 0, part.g0], [nx, ny, part.nz_local]
            self.lo, self.hi = [0, 0, part.zLoOwned], [nx, ny, part.zHiOwned]
            self.hasLower, self.hasUpper = [0, 0, part.hasLower], [0, 0, part.hasUpper]
        else:
            self.origin, self.n, self.lo, self.hi = list(part.origin), list(part.n_local), list(part.lo), list(part.hi)
            self.hasLower, self.hasUpper = list(part.hasLower), list(part.hasUpper)
        self.rank, self.n_global = part.rank, tuple(n_global)

    def cut(self, arr, face_axis=None):
        """the rank's part of a global (z, y, x) cell grid, or of the face grid of `face_axis`"""
        e = [int(face_axis == a) for a in range(3)]
        o, n = self.origin, self.n
        return np.ascontiguousarray(arr[o[2]:o[2] + n[2] + e[2], o[1]:o[1] + n[1] + e[1], o[0]:o[0] + n[0] + e[0]])

    def owned_cells(self):
        m = np.zeros((self.n[2], self.n[1], self.n[0]), bool)
        m[self.lo[2]:self.hi[2], self.lo[1]:self.hi[1], self.lo[0]:self.hi[0]] = True
        return m

    def owned_faces(self, a):
        """faces of axis a between the owned cells' transverse ranges; along a the planes lo .. hi - 1, and hi where the domain ends: a
        plane on a cut belongs to the rank above it"""
        shape = [self.n[2], self.n[1], self.n[0]]
        shape[2 - a] += 1
        m = np.zeros(shape, bool)
        sl = [slice(self.lo[q], self.hi[q]) for q in range(3)]
        sl[a] = slice(self.lo[a], self.hi[a] + (0 if self.hasUpper[a] else 1))
        m[sl[2], sl[1], sl[0]] = True
        return m

    def outer_planes(self, a):
        """The faces of axis a on which a rank's paint differs from the global paint by the rule itself: local i_a = 0 on a side with a
        lower neighbour (the rank sees the upper cell alone, the whole grid both cells), local i_a = n_a on a side with an upper neighbour
        — where that plane lies inside the whole grid.  Where the halo block ends with the grid, the plane is the grid's own boundary, the
        whole grid sees one cell there too, and nothing is excepted."""
        shape = [self.n[2], self.n[1], self.n[0]]
        shape[2 - a] += 1
        m = np.zeros(shape, bool)
        idx = [slice(None)] * 3
        if self.hasLower[a] and self.origin[a] > 0:
            idx[2 - a] = 0
            m[tuple(idx)] = True
        if self.hasUpper[a] and self.origin[a] + self.n[a] < self.n_global[a]:
            idx[2 - a] = self.n[a]
            m[tuple(idx)] = True
        return m


def make_parts(n, dims, world):
    if dims is None:
        return [partition.make_slab(n[2], world, r, TILE) for r in range(world)]
    return [partition.make_brick(n, dims, r, TILE) for r in range(world)]


def cut_axes(n, dims, world):
    """per axis, the global indices of its cuts"""
    d = (1, 1, world) if dims is None else dims
    return [[z0 for z0, _ in partition.slab_ranges(n[a], d[a], partition.alignment(TILE))][1:] if d[a] > 1 else [] for a in range(3)]


def _values(negate):
    """the range of a volume's random values: mostly more solid than the base's [-1, 1], in the sign convention of the field"""
    return (-1.5, 0.5) if negate else (-0.5, 1.5)


def five(rng, n, cuts, dx, orig, negate):
    lo, hi = _values(negate)
    more = -1.0 if negate else 1.0                      # the smaller volumes are more solid still
    cut_ax = [a for a in range(3) if cuts[a]]
    mid = [0.5 * n[a] for a in range(3)]
    at = lambda cells: np.asarray(orig) + np.asarray(cells, np.float64) * dx
    c0 = [cuts[a][0] if cuts[a] else mid[a] for a in range(3)]
    far = float(np.sqrt(sum(max(c0[a], n[a] - c0[a]) ** 2 for a in range(3))))      # cells from c0 to the farthest corner of the grid
    n0 = int(np.ceil(0.5 * (far + 1.0 - 4.0))) + 1      # a cube of spacing 4 dx whose inscribed sphere, 2 (n0 - 1) cells, plus the reach holds the grid
    c1 = [cuts[a][0] if a == cut_ax[0] else 0.3 * n[a] for a in range(3)]
    c2 = [40.0 if cuts[a] else mid[a] for a in range(3)]
    c4 = [cuts[a][-1] if a == cut_ax[-1] else 0.75 * n[a] for a in range(3)]
    shapes = [volume(rng, (n0, n0, n0), 4.0 * dx, lo, hi), volume(rng, (5, 4, 6), 2.0 * dx, lo + more, hi + more),
              volume(rng, (2, 2, 2), 0.5 * dx, lo + more, hi + more), volume(rng, (4, 4, 4), 2.0 * dx, lo, hi),
              volume(rng, (6, 5, 4), 1.5 * dx, lo + more, hi + more)]
    centres = [at(c0), at(c1), at(c2), at([-60.0, 90.0, 200.0]), at(c4)]
    return shapes, np.array([pose(s, rotation(rng), c) for s, c in zip(shapes, centres)])


def count64(rng, n, cuts, dx, orig, negate):
    """64 small volumes scattered over the box; every eighth lies wholly off the grid; 10 / 11 are an identical pair; volume 2 sits about
    cell 40 along every cut axis as in five()"""
    lo, hi = _values(negate)
    more = -1.0 if negate else 1.0
    at = lambda cells: np.asarray(orig) + np.asarray(cells, np.float64) * dx
    shapes, poses = [], []
    for k in range(64):
        s = volume(rng, tuple(int(q) for q in rng.randint(2, 5, 3)), rng.uniform(1.5, 3.0) * dx, lo, hi)
        c = rng.uniform((0.0, 0.0, 0.0), n)
        if k % 8 == 5:
            c = c + rng.choice([-1.0, 1.0], 3) * rng.uniform(100.0, 400.0, 3)
        if k == 2:
            s = volume(rng, (2, 2, 2), 0.5 * dx, lo + more, hi + more)
            c = [40.0 if cuts[a] else 0.5 * n[a] for a in range(3)]
        shapes.append(s)
        poses.append(pose(s, rotation(rng), at(c)))
    shapes[11], poses[11] = shapes[10], poses[10].copy()
    return shapes, np.array(poses)


def ids_field(sc, kind):
    if kind == "mod6":               # 0 .. 5: every wave holds all six, and 5 lies outside a count of 5
        n = sc.nx * sc.ny * sc.nz
        return (np.arange(n, dtype=np.int64) % 6).astype(np.int32).reshape(sc.nz, sc.ny, sc.nx)
    return motions_cases.ids_field(sc, kind)      # None; mod67: 64 .. 66 lie outside a count of 64


class Case:
    pass


def build(case):
    """The case with its global expectation; built once and shared: leave it unchanged.  Attributes: scene, params, ids, shapes, poses,
    motions, dims, world, parts, geo (a Geometry per rank), cuts, and the global restatement's col, idf, placed (counters), grids, faces
    (counters)."""
    if case not in _built:
        n, dims, world, negate, orig, dx, base, vols, kind, seed = CASES[case]
        rng = np.random.RandomState(seed)
        nx, ny, nz = n
        col = rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(np.float32)
        if base == "ties":
            col = (np.round(col * 2.0) / 2.0).astype(np.float32)
        sh = abi.grid_shapes(nx, ny, nz)
        cv = [rng.uniform(-2.0, 2.0, sh[f]).astype(np.float32) for f in ("faceX", "faceY", "faceZ")]
        c = Case()
        c.name = case
        c.scene = abi.Scene(nx, ny, nz, dx, 1.0 / 24.0, 1000.0, [0.0, 0.0, 0.0], rng.uniform(-1.0, 1.0, (nz, ny, nx)), col, 1.0,
                            collisionvel=cv, name=case)
        c.scene.orig = tuple(orig)
        c.params = abi.default_params(tileSize=TILE, tilePadding=2, preconditioner=abi.PRE_DIAGONAL, negateCollision=negate)
        c.dims, c.world, c.cuts = dims, world, cut_axes(n, dims, world)
        c.shapes, c.poses = (five if vols == "five" else count64)(rng, n, c.cuts, dx, orig, negate)
        c.ids = ids_field(c.scene, kind)
        c.motions = motions_cases.table("random", len(c.shapes))
        c.parts = make_parts(n, dims, world)
        c.geo = [Geometry(p, n) for p in c.parts]
        c.col, c.idf, c.placed = shapes_ref.place(col, c.ids, c.shapes, c.poses, orig, dx, negate)
        c.grids, c.faces = motions_ref.paint(c.col, c.idf, c.motions, orig, dx, negate, cv)
        _built[case] = c
    return _built[case]


def local(case, part):
    """the rank's Scene as the partition helper cuts it (with the rank's orig), and its cut of the uploaded ids"""
    c = build(case)
    sc = partition.local_scene(c.scene, part) if c.dims is None else partition.local_scene_brick(c.scene, part)
    return sc, (None if c.ids is None else Geometry(part, (c.scene.nx, c.scene.ny, c.scene.nz)).cut(c.ids))


def rank_expected(case, part, orig=None):
    """(collision, ids, placed counters, [gx, gy, gz], face counters) of `part`: the two restatements on the rank's cut arrays with the
    rank's orig (orig: another one in its place, for the mutants of the helper)"""
    c = build(case)
    sc, ids = local(case, part)
    o = sc.orig if orig is None else orig
    negate = c.params.negateCollision
    col, idf, placed = shapes_ref.place(sc.collision, ids, c.shapes, c.poses, o, sc.dx, negate)
    grids, faces = motions_ref.paint(col, idf, c.motions, o, sc.dx, negate, sc.collisionvel)
    return col, idf, placed, grids, faces


_expected = {}


def expected(case):
    """rank_expected of every rank of the case, computed once and shared: leave it unchanged"""
    if case not in _expected:
        _expected[case] = [rank_expected(case, part) for part in build(case).parts]
    return _expected[case]


def digest(g):
    h = hashlib.sha256()
    for v in g:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def expected_digest(case):
    out = []
    for col, idf, placed, grids, faces in expected(case):
        out += [col, idf, placed] + grids + [faces]
    return digest(out)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------
def place_and_paint(case, device_tables=None, stream=None):
    """The per_rank hook of Group.set_scene: the rank's ids, the placement, the paint.  device_tables = (poses, motions) in device memory
    (anything device_address takes), read behind what `stream` holds: the device forms."""
    c = build(case)

    def hook(s, part, sc):
        ids = None if c.ids is None else Geometry(part, (c.scene.nx, c.scene.ny, c.scene.nz)).cut(c.ids)
        if ids is not None:
            assert s.upload_collider_ids(ids) == abi.SUCCESS, s.last_error()
        if device_tables is None:
            assert s.place_colliders(c.poses) == abi.SUCCESS, s.last_error()
            assert s.paint_collider_velocities(c.motions) == abi.SUCCESS, s.last_error()
        else:
            assert s.place_colliders_device(device_tables[0], len(c.shapes), stream) == abi.SUCCESS, s.last_error()
            assert s.paint_collider_velocities_device(device_tables[1], len(c.motions), stream) == abi.SUCCESS, s.last_error()
    return hook


def run_group(case, when="after_cut", device_tables=None, stream=None):
    """a Group of the case's decomposition after upload, ids, place and paint on every rank; the caller closes it"""
    import polystokes_amd
    c = build(case)
    grp = polystokes_amd.Group(c.world, dims=c.dims)
    for s in grp.ranks:
        assert s.set_collider_shapes(c.shapes) == abi.SUCCESS, s.last_error()
    grp.set_scene(c.scene, c.params, per_rank=place_and_paint(case, device_tables, stream), when=when)
    return grp


def rank_arrays(s):
    """(collision, ids, placed counters, [gx, gy, gz], face counters) of a rank from its context's arrays, shaped like rank_expected's"""
    col, idf, placed = shapes_cases.placed(s)
    grids, faces = motions_cases.painted(s)
    return col, idf, placed, grids, faces


def group_digest(grp):
    out = []
    for s in grp.ranks:
        col, idf, placed, grids, faces = rank_arrays(s)
        out += [col, idf, placed] + grids + [faces]
    return digest(out)


# ---- the stepping cases: spheres at 64^3 and three more spheres, as volumes, in the liquid -------------------------------------------------
def step_scene():
    """(scene, params, shapes, poses, motions): three sphere volumes below the surface y = 0.5, turned by random rotations — one centred on
    the x cut of 2 x 1 x 2 bricks (x = 0.5), one on the z cut (z = 0.5, a cut of three slabs too), one inside the brick above both cuts"""
    sc, p = scenes.spheres(64, tile=TILE)
    p.preconditioner = abi.PRE_DIAGONAL
    rng = np.random.RandomState(9)
    shapes = [sphere_volume(0.08, 12, 1.0 / 48.0), sphere_volume(0.06, 10, 1.0 / 56.0), sphere_volume(0.07, 12, 1.0 / 52.0)]
    centres = [(0.5, 0.3, 0.27), (0.27, 0.36, 0.5), (0.77, 0.3, 0.8)]
    poses = np.array([pose(s, rotation(rng), c) for s, c in zip(shapes, centres)])
    motions = np.zeros((3, 9))
    motions[:, 0:3] = rng.uniform(-1.0, 1.0, (3, 3))
    motions[:, 3:6] = rng.uniform(-4.0, 4.0, (3, 3))
    motions[:, 6:9] = centres
    return sc, p, shapes, poses, motions


def step_hook(shapes, poses, motions):
    """upload of an id field that names no collider, placement, paint: on the single domain and on every rank alike"""
    def hook(s, part, sc):
        assert s.upload_collider_ids(np.full((sc.nz, sc.ny, sc.nx), -1, np.int32)) == abi.SUCCESS, s.last_error()
        assert s.place_colliders(poses) == abi.SUCCESS, s.last_error()
        assert s.paint_collider_velocities(motions) == abi.SUCCESS, s.last_error()
    return hook


def placed_step_scene():
    """step_scene() with the global restatement's collision and collisionvel in place of the uploaded ones: what run (c) cuts and uploads"""
    sc, p, shapes, poses, motions = step_scene()
    col, idf, placed = shapes_ref.place(sc.collision, None, shapes, poses, (0.0, 0.0, 0.0), sc.dx, 1)
    grids, faces = motions_ref.paint(col, idf, motions, (0.0, 0.0, 0.0), sc.dx, 1, sc.collisionvel)
    sc.collision = col
    sc.collisionvel = [g.copy() for g in grids]
    return sc, p, placed, faces


if __name__ == "__main__" and len(sys.argv) >= 3 and sys.argv[1] == "ranks":
    for case in sys.argv[2:]:
        grp = run_group(case)
        print("DIGEST", case, group_digest(grp))
        grp.close()

if __name__ == "__main__" and len(sys.argv) >= 3 and sys.argv[1] == "ranks_torch":
    import torch                      # first: the order a torch pipeline has
    assert torch.cuda.is_available(), "the device forms take their tables from torch tensors on the GPU"
    for case in sys.argv[2:]:
        c = build(case)
        dev = torch.device("cuda:0")
        tables = (torch.from_numpy(np.ascontiguousarray(c.poses, np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(c.motions, np.float64)).to(dev))
        torch.cuda.current_stream().synchronize()
        grp = run_group(case, device_tables=tables, stream=torch.cuda.current_stream())
        torch.cuda.current_stream().synchronize()
        print("DIGEST", case, group_digest(grp))
        grp.close()
