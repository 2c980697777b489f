"""ctypes mirror of include/polystokes.h (POD structs and enums only).

The C header is the contract; this file restates it for Python harness code (tests, bench.py).
"""
import ctypes as C

import numpy as np

REDUCED_DOF = 26

# ps_result (exec/HDK_PolyStokesSolver.h:61-70)
UNSUPPORTED_SOLVER, INCOMPLETE, INVALID, FAILED, NOCONVERGE, SUCCESS, NOCHANGE = -4, -3, -2, -1, 0, 1, 2
# ps_label (exec/HDK_PolyStokesSolver.h:71-82)
UNASSIGNED, UNSOLVED, GENERICFLUID, ACTIVEFLUID, SOLID, REDUCED, UNVISITED, VISITED, BOUNDARY = (
    -1, -2, -3, -4, -5, -6, -7, -8, -9)
PCG_MATRIX_VECTOR_PRODUCTS, EIGEN = 0, 1
PRE_IDENTITY, PRE_DIAGONAL, PRE_CHEBYSHEV, PRE_CHEBYSHEV_F32 = 1, 5, 6, 7
ORDER_VOXEL_TILES, ORDER_LINEAR = 0, 1

STAGE_NAMES = ["weights", "classify", "regions", "indices", "tile_matrices", "blocks", "assemble",
               "precond", "solve", "recover", "writeback"]

SAMPLE_NAMES = ["center", "faceX", "faceY", "faceZ", "edgeYZ", "edgeXZ", "edgeXY"]


class Params(C.Structure):
    _fields_ = [
        ("mindensity", C.c_double), ("maxdensity", C.c_double),
        ("matrixSetup", C.c_int32), ("solverType", C.c_int32),
        ("doSolve", C.c_int32), ("keepNonConvergedResults", C.c_int32),
        ("exportMatrices", C.c_int32), ("exportComponentMatrices", C.c_int32),
        ("exportStats", C.c_int32), ("useWarmStart", C.c_int32),
        ("tolerance", C.c_double),
        ("maxSolverIterations", C.c_int32), ("useInputSurfaceWeights", C.c_int32),
        ("useInputCollisionWeights", C.c_int32), ("activeLiquidBoundaryLayerSize", C.c_int32),
        ("activeSolidBoundaryLayerSize", C.c_int32), ("doReducedRegions", C.c_int32),
        ("doTile", C.c_int32), ("tileSize", C.c_int32), ("tilePadding", C.c_int32),
        ("preconditioner", C.c_int32), ("indexOrder", C.c_int32), ("negateCollision", C.c_int32),
        ("preconditionerDegree", C.c_int32),
        ("exportDataPrefix", C.c_char_p),
    ]


class FieldsIn(C.Structure):
    _fields_ = [
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
        ("dx", C.c_double), ("dt", C.c_double), ("orig", C.c_double * 3),
        ("density", C.c_float), ("reserved", C.c_int32),
        ("vel", C.c_void_p * 3), ("surface", C.c_void_p), ("collision", C.c_void_p),
        ("viscosity", C.c_void_p), ("collisionvel", C.c_void_p * 3),
        ("weights", C.c_void_p * 14),
    ]


class FieldsOut(C.Structure):
    _fields_ = [("vel", C.c_void_p * 3), ("valid", C.c_void_p * 3)]


class SolutionOut(C.Structure):
    """ps_solution_out: destinations of ps_download_solution_fields (any may be NULL)"""
    _fields_ = [("pressure", C.c_void_p), ("tauDiag", C.c_void_p * 3), ("tauEdge", C.c_void_p * 3)]


# ps_warm_start
WARM_NONE, WARM_PREVIOUS_STEP = 0, 1
# ps_solid_boundary
SOLID_NO_SLIP, SOLID_FREE_SLIP = 0, 1
# ps_rheology_model
RHEOLOGY_NEWTONIAN, RHEOLOGY_HERSCHEL_BULKLEY = 0, 1
# ps_solve_precision
PRECISION_FP64, PRECISION_MIXED = 0, 1
# ps_field_layout (the ps_*_device calls): i + d0*(j + d1*k), or k + d2*(j + d1*i) — a C-contiguous array indexed [i, j, k]
LAYOUT_X_FASTEST, LAYOUT_Z_FASTEST = 0, 1
EXTRAPOLATION_MAX_LAYERS = 64      # PS_EXTRAPOLATION_MAX_LAYERS (ps_set_velocity_extrapolation)
COLLIDER_MAX = 64                  # PS_COLLIDER_MAX (ps_set_collider_loads)
CONTACT_ANGLE_SWEEPS = 6           # PS_CONTACT_ANGLE_SWEEPS (ps_set_contact_angle)


class ColliderLoads(C.Structure):
    """ps_collider_loads (ps_set_collider_loads): how many colliders' loads every later step computes, and the torques' pivots"""
    _fields_ = [("count", C.c_int32), ("pivots", C.c_void_p)]


class ColliderMotions(C.Structure):
    """ps_collider_motions (ps_paint_collider_velocities): v[3], w[3], o[3] per collider"""
    _fields_ = [("count", C.c_int32), ("motion", C.c_void_p)]


# the collider motion calls: name -> argument types; every one returns int32
COLLIDER_MOTION_CALLS = (
    ("ps_paint_collider_velocities", (C.c_void_p, C.POINTER(ColliderMotions))),
    ("ps_paint_collider_velocities_device", (C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)),
)


COLLIDER_SHAPE_REACH = 4.0         # PS_COLLIDER_SHAPE_REACH (ps_place_colliders)


class ColliderShape(C.Structure):
    """ps_collider_shape (ps_set_collider_shapes): one collider's SDF volume in the body's own frame"""
    _fields_ = [("n", C.c_int32 * 3), ("reserved", C.c_int32), ("h", C.c_double), ("orig", C.c_double * 3), ("sdf", C.c_void_p)]


class ColliderShapes(C.Structure):
    """ps_collider_shapes"""
    _fields_ = [("count", C.c_int32), ("shape", C.POINTER(ColliderShape))]


class ColliderPoses(C.Structure):
    """ps_collider_poses (ps_place_colliders): R[9] row-major (body to world), t[3] per collider"""
    _fields_ = [("count", C.c_int32), ("pose", C.c_void_p)]


# the collider shape calls: name -> argument types; every one returns int32
COLLIDER_SHAPE_CALLS = (
    ("ps_set_collider_shapes", (C.c_void_p, C.POINTER(ColliderShapes))),
    ("ps_place_colliders", (C.c_void_p, C.POINTER(ColliderPoses))),
    ("ps_place_colliders_device", (C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)),
)


ADVECT_MAX_CELL_FIELDS = 8         # PS_ADVECT_MAX_CELL_FIELDS (ps_advect_fields)


class Advection(C.Structure):
    """ps_advection (ps_advect_fields): dt, the order, the carrier's face grids (all None: the context's written velocity), the cell fields in
    and out, the velocity out (all None: not advected)"""
    _fields_ = [("dt", C.c_double), ("order", C.c_int32), ("cellFields", C.c_int32), ("carrier", C.c_void_p * 3),
                ("cellIn", C.c_void_p * ADVECT_MAX_CELL_FIELDS), ("cellOut", C.c_void_p * ADVECT_MAX_CELL_FIELDS), ("velOut", C.c_void_p * 3)]


# the advection calls: name -> argument types; every one returns int32
ADVECTION_CALLS = (
    ("ps_advect_fields", (C.c_void_p, C.POINTER(Advection))),
    ("ps_advect_fields_device", (C.c_void_p, C.POINTER(Advection), C.c_int32, C.c_void_p)),
)


ADVECT_SEMI_LAGRANGIAN, ADVECT_MACCORMACK = 0, 1                  # PS_ADVECT_* (ps_advection_scheme.scheme)
ADVECT_LIMIT_NONE, ADVECT_LIMIT_CLAMP, ADVECT_LIMIT_REVERT = 0, 1, 2   # PS_ADVECT_LIMIT_* (ps_advection_scheme.limiter)


class AdvectionScheme(C.Structure):
    """ps_advection_scheme (ps_advect_fields_scheme): the scheme and, for the MacCormack correction, its limiter"""
    _fields_ = [("scheme", C.c_int32), ("limiter", C.c_int32)]


# the advection calls that take a scheme: name -> argument types; every one returns int32
ADVECTION_SCHEME_CALLS = (
    ("ps_advect_fields_scheme", (C.c_void_p, C.POINTER(Advection), C.POINTER(AdvectionScheme))),
    ("ps_advect_fields_scheme_device", (C.c_void_p, C.POINTER(Advection), C.POINTER(AdvectionScheme), C.c_int32, C.c_void_p)),
)


# the air pocket calls (ps_label_air_pockets ...): name -> argument types; every one returns int32
AIR_POCKET_CALLS = (
    ("ps_label_air_pockets", (C.c_void_p, C.POINTER(C.c_int32))),
    ("ps_get_air_pockets", (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)),
    ("ps_download_air_pocket_ids", (C.c_void_p, C.c_void_p)),
    ("ps_download_air_pocket_ids_device", (C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)),
    ("ps_set_air_pocket_pressures", (C.c_void_p, C.c_void_p, C.c_int64)),
)


class Rheology(C.Structure):
    """ps_rheology (ps_set_rheology): the viscosity law of every later setup of a context"""
    _fields_ = [("model", C.c_int32), ("passes", C.c_int32), ("flowIndex", C.c_double), ("yieldStress", C.c_double),
                ("minShearRate", C.c_double), ("minViscosity", C.c_double), ("maxViscosity", C.c_double)]


# the grids of ps_download_solution_fields: name -> sample grid (SAMPLE_NAMES / grid_shapes), in ps_solution_out order
SOLUTION_FIELDS = [("pressure", "center"), ("txx", "center"), ("tyy", "center"), ("tzz", "center"),
                   ("tyz", "edgeYZ"), ("txz", "edgeXZ"), ("txy", "edgeXY")]


class Stats(C.Structure):
    _fields_ = [
        ("dimData", C.c_double * 27), ("solveData", C.c_double * 6),
        ("result", C.c_int32), ("usedBiCGStab", C.c_int32),
        ("stage_ms", C.c_double * 16),
    ]


class SlabStruct(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("zLoOwned", C.c_int32), ("zHiOwned", C.c_int32),
                ("hasLower", C.c_int32), ("hasUpper", C.c_int32), ("zGlobalOwned", C.c_int32)]


class SurfaceFields(C.Structure):
    """ps_surface_fields"""
    _fields_ = [("sigma", C.c_void_p), ("pressure", C.c_void_p)]


class BrickStruct(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("dims", C.c_int32 * 3), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
                ("hasLower", C.c_int32 * 3), ("hasUpper", C.c_int32 * 3), ("globalLo", C.c_int32 * 3)]


def default_params(**kw):
    """Defaults of the reference's PRM template (exec/HDK_PolyStokes.C:88-208)."""
    p = Params()
    p.mindensity, p.maxdensity = 1.0, 100000.0
    p.matrixSetup, p.solverType = 0, PCG_MATRIX_VECTOR_PRODUCTS
    p.doSolve, p.keepNonConvergedResults = 1, 1
    p.exportMatrices = p.exportComponentMatrices = p.exportStats = 0
    p.useWarmStart = 1
    p.tolerance, p.maxSolverIterations = 1e-3, 5000
    p.useInputSurfaceWeights = p.useInputCollisionWeights = 1
    p.activeLiquidBoundaryLayerSize = p.activeSolidBoundaryLayerSize = 2
    p.doReducedRegions, p.doTile, p.tileSize, p.tilePadding = 1, 1, 16, 2
    p.preconditioner, p.indexOrder, p.negateCollision = PRE_IDENTITY, ORDER_VOXEL_TILES, 1
    p.exportDataPrefix = None
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def grid_shapes(nx, ny, nz):
    """numpy shapes (z, y, x) — x fastest — of the 7 sample grids, keyed by SAMPLE_NAMES."""
    return {
        "center": (nz, ny, nx),
        "faceX": (nz, ny, nx + 1), "faceY": (nz, ny + 1, nx), "faceZ": (nz + 1, ny, nx),
        "edgeYZ": (nz + 1, ny + 1, nx), "edgeXZ": (nz + 1, ny, nx + 1), "edgeXY": (nz, ny + 1, nx + 1),
    }


class Scene:
    """Host-side input bundle: numpy float32 arrays laid out as the C ABI expects."""

    def __init__(self, nx, ny, nz, dx, dt, density, vel, surface, collision, viscosity,
                 collisionvel=None, weights=None, name="scene", density_field=None, surface_tension=None,
                 surface_sigma_field=None, surface_pressure_field=None, contact_angle=None, contact_cosine_field=None):
        self.nx, self.ny, self.nz, self.dx, self.dt, self.density = nx, ny, nz, float(dx), float(dt), float(density)
        sh = grid_shapes(nx, ny, nz)
        f32 = lambda a, s: np.array(np.broadcast_to(np.asarray(a, dtype=np.float32), s), dtype=np.float32, order="C", copy=True)
        self.vel = [f32(vel[a], sh["face" + "XYZ"[a]]) for a in range(3)]
        self.surface = f32(surface, sh["center"])
        self.collision = f32(collision, sh["center"])
        self.viscosity = f32(viscosity, sh["center"])
        if collisionvel is None:
            collisionvel = [0.0, 0.0, 0.0]
        self.collisionvel = [f32(collisionvel[a], sh["face" + "XYZ"[a]]) for a in range(3)]
        self.weights = None
        if weights is not None:
            self.weights = [f32(weights[i], sh[SAMPLE_NAMES[i % 7]]) for i in range(14)]
        self.name = name
        # optional cell density field (ps_upload_density_field); None: the scalar `density` everywhere
        self.density_field = None if density_field is None else f32(density_field, sh["center"])
        # optional surface tension coefficient sigma (ps_set_surface_tension, applied at upload / step); None: leave the context's setting
        self.surface_tension = None if surface_tension is None else float(surface_tension)
        # optional free-surface cell fields (ps_upload_surface_fields): the surface-tension coefficient (None: the scalar) and the ambient
        # pressure (None: 0)
        self.surface_sigma_field = None if surface_sigma_field is None else f32(surface_sigma_field, sh["center"])
        self.surface_pressure_field = None if surface_pressure_field is None else f32(surface_pressure_field, sh["center"])
        # optional contact angle in degrees (ps_set_contact_angle, applied at upload / step; < 0: off); None: leave the context's setting
        self.contact_angle = None if contact_angle is None else float(contact_angle)
        # optional cell field of cos(theta), painted into the solids (ps_upload_contact_cosine_field); None: the scalar angle
        self.contact_cosine_field = None if contact_cosine_field is None else f32(contact_cosine_field, sh["center"])

    def fields_in(self):
        fi = FieldsIn()
        fi.nx, fi.ny, fi.nz = self.nx, self.ny, self.nz
        fi.dx, fi.dt = self.dx, self.dt
        fi.orig[0], fi.orig[1], fi.orig[2] = (float(v) for v in getattr(self, "orig", (0.0, 0.0, 0.0)))   # (the default pivot of collider loads)
        fi.density = self.density
        for a in range(3):
            fi.vel[a] = self.vel[a].ctypes.data
            fi.collisionvel[a] = self.collisionvel[a].ctypes.data
        fi.surface = self.surface.ctypes.data
        fi.collision = self.collision.ctypes.data
        fi.viscosity = self.viscosity.ctypes.data
        for i in range(14):
            fi.weights[i] = self.weights[i].ctypes.data if self.weights is not None else None
        return fi
