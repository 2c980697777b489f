"""Crafted weight grids and SDF scenes shared by the air-pocket tests (test_air_pockets_ref_cpu.py, test_gpu_air_pockets.py), and the child
process of the poisoned-buffer test:  python air_pockets_cases.py label <scene>  prints a digest of what the labelling leaves."""
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

import air_pockets_ref as ref  # noqa: E402

RESULT_ARRAYS = ("airPockets", "airPocketIds", "airPocketUnits", "airPocketCells", "airPocketOpen", "airPocketVolume")


# ---- weights written directly (the CPU tests of the restatement) --------------------------------------------------------------------
def liquid_weights(nx=6, ny=5, nz=4):
    """all liquid, no solid: lw = fw = 1 everywhere, every face open"""
    return {"lw": np.ones((nz, ny, nx), np.float32), "fw": np.ones((nz, ny, nx), np.float32),
            "fwx": np.ones((nz, ny, nx + 1), np.float32), "fwy": np.ones((nz, ny + 1, nx), np.float32),
            "fwz": np.ones((nz + 1, ny, nx), np.float32)}


def run_ref(w, dx=0.25, mutant=None):
    return ref.pockets(w["lw"], w["fw"], w["fwx"], w["fwy"], w["fwz"], dx, mutant)


# ---- SDF scenes (the GPU tests) -------------------------------------------------------------------------------------------------------
def _centres(nx, ny, nz):
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return i + 0.5, j + 0.5, k + 0.5       # in cells


def _scene(nx, ny, nz, surface, collision, name, tile=16, pad=2):
    from polystokes_amd import _abi as abi
    dx = 1.0 / max(nx, ny, nz)
    sc = abi.Scene(nx, ny, nz, dx, 1.0 / 24.0, 1000.0, [0.0, -1.0, 0.0], (surface * dx).astype(np.float32), (collision * dx).astype(np.float32),
                   50.0, name=name)
    return sc, abi.default_params(tileSize=tile, tilePadding=pad, preconditioner=abi.PRE_DIAGONAL)


def pool(nx, ny, nz, wall, level, bubbles, name):
    """A box open at the top (solid floor and side walls `wall` cells thick) holding liquid up to y = level cells, open air above, and
    spherical air bubbles (cx, cy, cz, r in cells) inside the liquid."""
    x, y, z = _centres(nx, ny, nz)
    collision = np.minimum.reduce([x - wall, nx - wall - x, y - wall, z - wall, nz - wall - z])   # > 0: not solid
    surface = y - level                                                                          # < 0: liquid
    for cx, cy, cz, r in bubbles:
        surface = np.maximum(surface, r - np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2))
    return _scene(nx, ny, nz, surface, collision, name)


def bubbles():
    """case 1: 40 x 24 x 20; the second bubble straddles the box border x = 16.  Three pockets, the air above the pool open."""
    return pool(40, 24, 20, 2, 16.0, [(7.5, 8.0, 10.0, 3.2), (16.3, 9.0, 9.7, 2.6)], "pockets_bubbles")


def odd19():
    return pool(19, 17, 21, 2, 11.0, [(6.0, 6.0, 8.0, 2.2), (12.5, 5.5, 14.0, 1.8)], "pockets_odd19")


def odd7():
    return pool(7, 5, 3, 1, 3.0, [], "pockets_odd7")


def bubbles_scaled(n=256):
    """case 1 scaled to n^3 (the measurement)"""
    s = n / 40.0
    return pool(n, n, n, 2, 0.66 * n, [(7.5 * s, 8.0 * s, 0.5 * n, 3.2 * s), (16.3 * s, 9.0 * s, 0.48 * n, 2.6 * s)], "pockets_bubbles%d" % n)


def _sign(mask):
    """a sign field as an SDF: +1 where mask, -1 elsewhere.  Every sub-sample of the 2x2x2 sampler lies within a quarter cell of its own
    cell's centre: its own cell has the trilinear weight 0.75^3 = 0.42, so it takes that cell's sign unless all seven other cells
    around it differ (a convex corner: that cell's weight is 7/8).  Elsewhere cell weights are 0 or 1, a face between unlike cells 0.5."""
    return np.where(mask, 1.0, -1.0)


def serpentine_mask(nx=48, ny=48):
    """a corridor one cell wide in the (x, y) plane: along x in every fourth row, joined alternately at the right and the left end"""
    m = np.zeros((ny, nx), bool)
    rows = list(range(1, ny - 1, 4))
    for q, j in enumerate(rows):
        m[j, 1:nx - 1] = True
        if q + 1 < len(rows):
            i = nx - 2 if q % 2 == 0 else 1
            m[j:rows[q + 1] + 1, i] = True
    return m


def serpentine():
    """case 3: 48 x 48 x 16.  A solid block below z = 12 holds an air corridor one cell wide and high, in the layer z = 8, that winds through
    all nine 16^3 boxes of that plane; above the block two layers of liquid and two of open air."""
    nx, ny, nz = 48, 48, 16
    fluid = np.zeros((nz, ny, nx), bool)
    fluid[8] = serpentine_mask(nx, ny)
    fluid[12:] = True
    liquid = np.zeros((nz, ny, nx), bool)
    liquid[12:14] = True
    return _scene(nx, ny, nz, _sign(~liquid), _sign(fluid), "pockets_serpentine")


def checkerboard():
    """case 4: 32 x 32 x 16, no solid; the cells with even i + j + k are air, the others liquid: 8192 single-cell pockets"""
    x, y, z = _centres(32, 32, 16)
    air = ((x + y + z - 1.5).astype(np.int64) % 2) == 0
    return _scene(32, 32, 16, _sign(air), np.ones(air.shape), "pockets_checkerboard")


def two_rooms():
    """120 x 88 x 64 = 675 840 cells, 2640 tiles of 256: more than the 1024 workgroups of the sum kernel take one each, so a workgroup walks
    three tiles and the last workgroups start beyond the grid.  A solid block below z = 40 holds two closed air rooms side by side in x
    (x in [2, 56) and [62, 118), y in [2, 86), z in [10, 14)): along the x-fastest walk their cells alternate row by row, and a row of 120
    cells does not divide a tile, so a wave changes its pocket in mid-run and meets tiles of mixed ids.  Above the block 16 layers of
    liquid and 8 of open air, where a wave carries one pocket's sums over all its tiles."""
    nx, ny, nz = 120, 88, 64
    fluid = np.zeros((nz, ny, nx), bool)
    fluid[10:14, 2:86, 2:56] = True
    fluid[10:14, 2:86, 62:118] = True
    fluid[40:] = True
    liquid = np.zeros((nz, ny, nx), bool)
    liquid[40:56] = True
    return _scene(nx, ny, nz, _sign(~liquid), _sign(fluid), "pockets_two_rooms")


def tie_weights():
    """12 x 10 x 8 with the fourteen weight grids uploaded by the caller (all liquid, no solid) and the centre liquid weights written by
    hand: skin cells tied between two different pockets in x, in y and in z (the first direction wins), one whose +x neighbour holds less
    liquid than its -x neighbour (the smaller lw wins), and one whose face towards the better neighbour is solid."""
    from polystokes_amd import _abi as abi
    nx, ny, nz = 12, 10, 8
    sh = abi.grid_shapes(nx, ny, nz)
    weights = [np.ones(sh[abi.SAMPLE_NAMES[i % 7]], np.float32) for i in range(14)]
    lw, fwx = weights[0], weights[8]
    for (i, j, k), v in {(1, 2, 1): 0.0, (2, 2, 1): 0.75, (3, 2, 1): 0.0,          # tie in x: -x
                         (6, 1, 1): 0.0, (6, 2, 1): 0.75, (6, 3, 1): 0.0,          # tie in y: -y
                         (9, 2, 1): 0.0, (9, 2, 2): 0.75, (9, 2, 3): 0.0,          # tie in z: -z
                         (1, 6, 4): 0.25, (2, 6, 4): 0.75, (3, 6, 4): 0.0,         # +x holds less liquid
                         (6, 6, 4): 0.25, (7, 6, 4): 0.75, (8, 6, 4): 0.0,         # ... but the face towards it is solid
                         (1, 8, 6): 0.0, (1, 8, 5): 0.625}.items():                # a skin cell with one neighbour, below it in z
        lw[k, j, i] = v
    fwx[4, 6, 8] = 0.0
    sc, p = _scene(nx, ny, nz, -np.ones((nz, ny, nx)), np.ones((nz, ny, nx)), "pockets_tie_weights")
    sc.weights = weights
    return sc, p


def all_air():
    return _scene(33, 17, 9, np.ones((9, 17, 33)), np.ones((9, 17, 33)), "pockets_all_air")


def all_liquid():
    return _scene(20, 12, 10, -np.ones((10, 12, 20)), np.ones((10, 12, 20)), "pockets_all_liquid")


SCENES = {"bubbles": bubbles, "odd19": odd19, "odd7": odd7, "serpentine": serpentine, "checkerboard": checkerboard, "all_air": all_air,
          "all_liquid": all_liquid, "two_rooms": two_rooms, "tie_weights": tie_weights}


def weights_of(s, sc):
    """the weight arrays of the last setup, as the restatement takes them"""
    from polystokes_amd import _abi as abi
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    return {"lw": s.array("centerLiquidWeights").reshape(sh["center"]), "fw": s.array("centerFluidWeights").reshape(sh["center"]),
            "fwx": s.array("faceXFluidWeights").reshape(sh["faceX"]), "fwy": s.array("faceYFluidWeights").reshape(sh["faceY"]),
            "fwz": s.array("faceZFluidWeights").reshape(sh["faceZ"])}


def got(s):
    """what the labelling left, in RESULT_ARRAYS order"""
    return [s.array(n) for n in RESULT_ARRAYS]


def digest(arrays):
    h = hashlib.sha256()
    for v in arrays:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


if __name__ == "__main__" and len(sys.argv) >= 3 and sys.argv[1] == "label":
    import polystokes_amd
    sc, p = SCENES[sys.argv[2]]()
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    k = s.label_air_pockets()
    vol, opn = s.air_pockets()
    print("DIGEST", k, digest(got(s) + [s.air_pocket_ids(), vol, opn]))
    s.close()
