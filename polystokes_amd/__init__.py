"""polystokes_amd — MI355X-native drop-in for the PolyStokes per-step reduced-viscosity Stokes solve.

The product is the C-ABI shared library `libpolystokes_hip.so` (include/polystokes.h), built from the HIP
sources in `csrc/`.  This module is only the Python harness over that ABI used by tests and bench.py.
There is no CPU fallback: loading fails loudly if the library is missing, and creating a context fails
loudly if no HIP device is present.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _abi
from ._abi import (FieldsIn, FieldsOut, Params, Scene, Stats, default_params)  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PS_LIB") or os.path.join(_HERE, "libpolystokes_hip.so")   # PS_LIB: A/B builds (scripts/build_variant.sh)
_lib = None

EXPORTED_SYMBOLS = [
    "ps_abi_version", "ps_reduced_dof", "ps_context_create", "ps_context_destroy", "ps_last_error", "ps_params_default",
    "ps_upload_fields", "ps_step_device", "ps_setup_device", "ps_solve_device", "ps_download_fields",
    "polystokes_step", "ps_apply_operator", "ps_apply_preconditioner", "ps_query_array", "ps_read_array",
    "ps_export_component_matrices", "ps_export_matrices", "ps_export_stats", "ps_bench_kernel", "ps_memory_stats", "ps_set_interrupt", "ps_solve_exported_system",
    "ps_set_slab", "ps_set_brick", "ps_comm_unique_id", "ps_comm_init_rccl", "ps_comm_selftest", "ps_comm_init_tcp", "ps_dist_stats",
    "ps_group_create", "ps_group_destroy", "ps_group_rank", "ps_group_step",
    "ps_set_warm_start", "ps_download_solution_fields", "ps_upload_density_field", "ps_set_surface_tension",
    "ps_set_solid_boundary", "ps_set_rheology", "ps_set_solve_precision",
    "ps_upload_fields_device", "ps_upload_density_field_device", "ps_download_fields_device", "ps_download_solution_fields_device",
    "ps_step_device_fields", "ps_set_velocity_extrapolation",
    "ps_upload_surface_fields", "ps_upload_surface_fields_device",
    "ps_set_collider_loads", "ps_upload_collider_ids", "ps_upload_collider_ids_device", "ps_get_collider_loads", "ps_get_collider_loads_device",
    "ps_paint_collider_velocities", "ps_paint_collider_velocities_device",
    "ps_set_collider_shapes", "ps_place_colliders", "ps_place_colliders_device",
    "ps_label_air_pockets", "ps_get_air_pockets", "ps_download_air_pocket_ids", "ps_download_air_pocket_ids_device", "ps_set_air_pocket_pressures",
    "ps_set_contact_angle", "ps_upload_contact_cosine_field", "ps_upload_contact_cosine_field_device",
    "ps_advect_fields", "ps_advect_fields_device", "ps_advect_fields_scheme", "ps_advect_fields_scheme_device",
]


def build(force=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"])
    subprocess.check_call(["make", "-C", csrc, "-j4", "-s"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C polystokes_amd/csrc` "
                "(__graft_entry__.build()).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.ps_abi_version.restype = C.c_int32
        L.ps_reduced_dof.restype = C.c_int32
        L.ps_context_create.argtypes = [C.c_int32]
        L.ps_context_create.restype = C.c_void_p
        L.ps_context_destroy.argtypes = [C.c_void_p]
        L.ps_last_error.argtypes = [C.c_void_p]
        L.ps_last_error.restype = C.c_char_p
        L.ps_params_default.argtypes = [C.POINTER(Params)]
        L.ps_upload_fields.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FieldsIn)]
        L.ps_upload_fields.restype = C.c_int32
        for fn in (L.ps_step_device, L.ps_setup_device, L.ps_solve_device):
            fn.argtypes = [C.c_void_p, C.POINTER(Stats)]
            fn.restype = C.c_int32
        L.ps_download_fields.argtypes = [C.c_void_p, C.POINTER(FieldsOut)]
        L.ps_download_fields.restype = C.c_int32
        L.polystokes_step.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FieldsIn), C.POINTER(FieldsOut),
                                      C.POINTER(Stats)]
        L.polystokes_step.restype = C.c_int32
        L.ps_apply_operator.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ps_apply_operator.restype = C.c_int32
        L.ps_apply_preconditioner.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ps_apply_preconditioner.restype = C.c_int32
        L.ps_query_array.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int32)]
        L.ps_query_array.restype = C.c_int64
        L.ps_read_array.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]
        L.ps_read_array.restype = C.c_int32
        L.ps_export_component_matrices.argtypes = [C.c_void_p, C.c_char_p]
        L.ps_export_component_matrices.restype = C.c_int32
        L.ps_export_matrices.argtypes = [C.c_void_p, C.c_char_p]
        L.ps_export_matrices.restype = C.c_int32
        L.ps_export_stats.argtypes = [C.c_void_p, C.POINTER(Stats), C.c_char_p]
        L.ps_export_stats.restype = C.c_int32
        L.ps_bench_kernel.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.ps_bench_kernel.restype = C.c_int32
        L.ps_memory_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.ps_memory_stats.restype = C.c_int32
        L.ps_solve_exported_system.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Params), C.c_double, C.c_void_p, C.c_int64, C.POINTER(Stats)]
        L.ps_solve_exported_system.restype = C.c_int32
        L.ps_set_interrupt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ps_set_interrupt.restype = C.c_int32
        L.ps_set_slab.argtypes = [C.c_void_p, C.POINTER(_abi.SlabStruct)]
        L.ps_set_slab.restype = C.c_int32
        L.ps_set_brick.argtypes = [C.c_void_p, C.POINTER(_abi.BrickStruct)]
        L.ps_set_brick.restype = C.c_int32
        L.ps_comm_unique_id.argtypes = [C.c_void_p]
        L.ps_comm_unique_id.restype = C.c_int32
        L.ps_comm_init_rccl.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.ps_comm_init_rccl.restype = C.c_int32
        L.ps_comm_init_tcp.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int32]
        L.ps_comm_init_tcp.restype = C.c_int32
        L.ps_comm_selftest.argtypes = [C.c_void_p]
        L.ps_comm_selftest.restype = C.c_int32
        L.ps_dist_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.ps_dist_stats.restype = C.c_int32
        L.ps_group_create.argtypes = [C.c_int32, C.c_int32]
        L.ps_group_create.restype = C.c_void_p
        L.ps_group_destroy.argtypes = [C.c_void_p]
        L.ps_group_rank.argtypes = [C.c_void_p, C.c_int32]
        L.ps_group_rank.restype = C.c_void_p
        L.ps_group_step.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.ps_group_step.restype = C.c_int32
        L.ps_set_warm_start.argtypes = [C.c_void_p, C.c_int32]
        L.ps_set_warm_start.restype = C.c_int32
        L.ps_download_solution_fields.argtypes = [C.c_void_p, C.POINTER(_abi.SolutionOut)]
        L.ps_download_solution_fields.restype = C.c_int32
        L.ps_upload_density_field.argtypes = [C.c_void_p, C.c_void_p]
        L.ps_upload_density_field.restype = C.c_int32
        L.ps_set_surface_tension.argtypes = [C.c_void_p, C.c_double]
        L.ps_set_surface_tension.restype = C.c_int32
        L.ps_set_solid_boundary.argtypes = [C.c_void_p, C.c_int32]
        L.ps_set_solid_boundary.restype = C.c_int32
        L.ps_set_rheology.argtypes = [C.c_void_p, C.POINTER(_abi.Rheology)]
        L.ps_set_rheology.restype = C.c_int32
        L.ps_set_solve_precision.argtypes = [C.c_void_p, C.c_int32]
        L.ps_set_solve_precision.restype = C.c_int32
        L.ps_set_velocity_extrapolation.argtypes = [C.c_void_p, C.c_int32]
        L.ps_set_velocity_extrapolation.restype = C.c_int32
        L.ps_upload_fields_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FieldsIn), C.c_int32, C.c_void_p]
        L.ps_upload_fields_device.restype = C.c_int32
        L.ps_upload_density_field_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.ps_upload_density_field_device.restype = C.c_int32
        L.ps_download_fields_device.argtypes = [C.c_void_p, C.POINTER(FieldsOut), C.c_int32, C.c_void_p]
        L.ps_download_fields_device.restype = C.c_int32
        L.ps_download_solution_fields_device.argtypes = [C.c_void_p, C.POINTER(_abi.SolutionOut), C.c_int32, C.c_void_p]
        L.ps_download_solution_fields_device.restype = C.c_int32
        L.ps_step_device_fields.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FieldsIn), C.POINTER(FieldsOut), C.POINTER(Stats),
                                            C.c_int32, C.c_void_p]
        L.ps_step_device_fields.restype = C.c_int32
        L.ps_upload_surface_fields.argtypes = [C.c_void_p, C.POINTER(_abi.SurfaceFields)]
        L.ps_upload_surface_fields.restype = C.c_int32
        L.ps_upload_surface_fields_device.argtypes = [C.c_void_p, C.POINTER(_abi.SurfaceFields), C.c_int32, C.c_void_p]
        L.ps_upload_surface_fields_device.restype = C.c_int32
        L.ps_set_collider_loads.argtypes = [C.c_void_p, C.POINTER(_abi.ColliderLoads)]
        L.ps_set_collider_loads.restype = C.c_int32
        L.ps_upload_collider_ids.argtypes = [C.c_void_p, C.c_void_p]
        L.ps_upload_collider_ids.restype = C.c_int32
        L.ps_upload_collider_ids_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.ps_upload_collider_ids_device.restype = C.c_int32
        L.ps_get_collider_loads.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.ps_get_collider_loads.restype = C.c_int32
        L.ps_get_collider_loads_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.ps_get_collider_loads_device.restype = C.c_int32
        L.ps_set_contact_angle.argtypes = [C.c_void_p, C.c_double]
        L.ps_set_contact_angle.restype = C.c_int32
        L.ps_upload_contact_cosine_field.argtypes = [C.c_void_p, C.c_void_p]
        L.ps_upload_contact_cosine_field.restype = C.c_int32
        L.ps_upload_contact_cosine_field_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.ps_upload_contact_cosine_field_device.restype = C.c_int32
        for name, argtypes in _abi.COLLIDER_MOTION_CALLS + _abi.COLLIDER_SHAPE_CALLS + _abi.AIR_POCKET_CALLS + _abi.ADVECTION_CALLS + _abi.ADVECTION_SCHEME_CALLS:
            getattr(L, name).argtypes = list(argtypes)
            getattr(L, name).restype = C.c_int32
        _lib = L
    return _lib


def device_address(a):
    """The device address behind `a`: None, an int, an object with `.ptr` (_hip.DeviceBuffer), a torch tensor (`data_ptr()`), or anything
    with `__cuda_array_interface__`."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if hasattr(a, "ptr"):
        return int(a.ptr)
    if hasattr(a, "data_ptr"):
        return int(a.data_ptr())
    if hasattr(a, "__cuda_array_interface__"):
        return int(a.__cuda_array_interface__["data"][0])
    raise TypeError(f"no device address in {type(a).__name__}")


def stream_handle(stream):
    """None (the default stream), an int, or an object with `.cuda_stream` (a torch stream, _hip.Stream)."""
    if stream is None:
        return None
    return int(stream) if isinstance(stream, int) else int(stream.cuda_stream)


def to_layout(a, layout):
    """A (z, y, x) numpy array as the flat order of `layout`: itself for LAYOUT_X_FASTEST, its [i, j, k]-indexed transpose for LAYOUT_Z_FASTEST."""
    a = np.asarray(a, dtype=np.float32)
    return np.ascontiguousarray(a if layout == _abi.LAYOUT_X_FASTEST else a.transpose(2, 1, 0))


def from_layout(flat, shape_zyx, layout):
    """Inverse of to_layout: the flat floats of a field of numpy shape (z, y, x), read back as a (z, y, x) array."""
    flat = np.asarray(flat).ravel()
    if layout == _abi.LAYOUT_X_FASTEST:
        return flat.reshape(shape_zyx)
    return np.ascontiguousarray(flat.reshape(shape_zyx[::-1]).transpose(2, 1, 0))


class DeviceScene:
    """A Scene whose arrays live on the GPU (_hip.DeviceBuffer) in one layout: what a device-resident caller hands to the ps_*_device calls."""

    def __init__(self, scene, layout=_abi.LAYOUT_X_FASTEST, pad=0):
        from . import _hip
        put = lambda a: _hip.DeviceBuffer.from_numpy(to_layout(a, layout), pad)
        self.layout, self.host = layout, scene
        for k in ("nx", "ny", "nz", "dx", "dt", "density", "name", "surface_tension"):
            setattr(self, k, getattr(scene, k))
        self.orig = tuple(getattr(scene, "orig", (0.0, 0.0, 0.0)))
        self.vel = [put(a) for a in scene.vel]
        self.collisionvel = [put(a) for a in scene.collisionvel]
        self.surface, self.collision, self.viscosity = put(scene.surface), put(scene.collision), put(scene.viscosity)
        self.weights = None if scene.weights is None else [put(a) for a in scene.weights]
        self.density_field = None if scene.density_field is None else put(scene.density_field)
        opt = lambda name: None if getattr(scene, name, None) is None else put(getattr(scene, name))
        self.surface_sigma_field, self.surface_pressure_field = opt("surface_sigma_field"), opt("surface_pressure_field")
        self.contact_angle, self.contact_cosine_field = getattr(scene, "contact_angle", None), opt("contact_cosine_field")


def device_scene(scene, layout=_abi.LAYOUT_X_FASTEST, pad=0):
    """`scene` on the device; for LAYOUT_Z_FASTEST each (z, y, x) array is stored as np.ascontiguousarray(a.transpose(2, 1, 0)).
    pad: spare floats in front of every array inside its allocation (pointers that are only 4-byte aligned)."""
    return DeviceScene(scene, layout, pad)


def fields_in_device(fields):
    """ps_fields_in from an object with Scene's attributes whose arrays are device arrays (see device_address)."""
    fi = FieldsIn()
    fi.nx, fi.ny, fi.nz = fields.nx, fields.ny, fields.nz
    fi.dx, fi.dt = fields.dx, fields.dt
    fi.orig[0], fi.orig[1], fi.orig[2] = (float(v) for v in getattr(fields, "orig", (0.0, 0.0, 0.0)))
    fi.density = fields.density
    cv = getattr(fields, "collisionvel", None)
    for a in range(3):
        fi.vel[a] = device_address(fields.vel[a])
        fi.collisionvel[a] = device_address(cv[a]) if cv is not None else None
    fi.surface, fi.collision, fi.viscosity = (device_address(fields.surface), device_address(fields.collision),
                                              device_address(fields.viscosity))
    w = getattr(fields, "weights", None)
    for i in range(14):
        fi.weights[i] = device_address(w[i]) if w is not None else None
    return fi


_DT = {(1, "i"): np.int8, (4, "i"): np.int32, (8, "i"): np.int64, (4, "f"): np.float32, (8, "f"): np.float64, (4, "u"): np.uint32}


def _kind(name):
    if name.endswith(("Labels", "Indices", ".col", ".ptr", "Region", "Perm", ".chunkInfo", ".chunkRep", ".code")) or name.startswith("faceRow"):
        return "i"
    if name in ("valuesCoded", "columns16", "diagonalsCoded", "fusedStep", "ownedRange", "streamRuns", "rowPerLane", "chebInner32", "warmStartUsed", "densityField", "launchWalk",
                "surfaceTensionReducedFaces", "surfaceFields", "solidBoundary", "solidSlipEdges", "rheologyModel", "rheologyIterations",
                "solvePrecisionUsed", "solvePassIterations",
                "velocityExtrapolation", "extrapolationLayerX", "extrapolationLayerY", "extrapolationLayerZ", "extrapolationCounts",
                "colliderLoads", "colliderLoadTerms", "colliderMotions", "colliderMotionFaces",
                "colliderShapes", "colliderPlacement", "colliderPlacedCells", "colliderCellIds",
                "airPockets", "airPocketIds", "airPocketUnits", "airPocketCells", "airPocketOpen", "airPocketPasses",
                "contactField", "contactCells", "advection", "advectionCounts", "advectionScheme", "advectionCorrection"):
        return "i"
    if name in ("ownedX", "ownedY", "ownedZ"):
        return "f"
    if False:
        return "i"
    if name == "reducedRowFace":
        return "u"
    return "f"


def process_memory_stats():
    """ps_memory_stats without a context: device bytes held through the library in this process, their peak, live contexts"""
    v = (C.c_int64 * 4)()
    lib().ps_memory_stats(None, v)
    return {"live_bytes": int(v[0]), "peak_bytes": int(v[1]), "contexts": int(v[3])}


def _has_surface_fields(scene):
    return getattr(scene, "surface_sigma_field", None) is not None or getattr(scene, "surface_pressure_field", None) is not None


class PolyStokesError(RuntimeError):
    pass


class Solver:
    """Thin object wrapper over a `ps_context` — the counterpart of `HDK_PolyStokes::Solver`
    (exec/HDK_PolyStokesSolver.h:27) as seen through the C ABI."""

    def __init__(self, device=0, _handle=None):
        self.L = lib()
        self._owned = _handle is None
        h = self.L.ps_context_create(device) if _handle is None else _handle
        if not h:
            raise PolyStokesError(self.L.ps_last_error(None).decode())
        self.h = C.c_void_p(h)
        self.stats = Stats()
        self.scene = None

    def close(self):
        if getattr(self, "h", None):
            if self._owned:
                self.L.ps_context_destroy(self.h)
            self.h = None

    def set_interrupt(self, fn):
        """fn() -> truthy stops the solve at the next CG batch boundary (UT_Interrupt equivalent)."""
        if fn is None:
            self._cb = None
            self._check(self.L.ps_set_interrupt(self.h, None, None))
            return
        self._cb = C.CFUNCTYPE(C.c_int32, C.c_void_p)(lambda user: 1 if fn() else 0)
        self._check(self.L.ps_set_interrupt(self.h, C.cast(self._cb, C.c_void_p), None))

    def set_warm_start(self, mode):
        """ps_set_warm_start: 0 (WARM_NONE) solves from zero; 1 (WARM_PREVIOUS_STEP) starts the next PCG solve from the solution this
        context carried over from its last kept step.  Every call drops the carried solution."""
        self._check(self.L.ps_set_warm_start(self.h, int(mode)))

    def set_surface_tension(self, sigma):
        """ps_set_surface_tension: sigma (force per length; 0 = off) for every later setup of this context, across uploads.  Returns the
        ps_result: INVALID for a negative or non-finite sigma (the reason in last_error(), the previous setting kept)."""
        return self._check(self.L.ps_set_surface_tension(self.h, float(sigma)), allow=(1, -2))

    def set_solid_boundary(self, mode):
        """ps_set_solid_boundary: SOLID_NO_SLIP (0, the default) or SOLID_FREE_SLIP (1: no shear stress on the edges a solid cuts) for every
        later setup of this context, across uploads.  Returns the ps_result: INVALID for another mode (the previous setting kept)."""
        return self._check(self.L.ps_set_solid_boundary(self.h, int(mode)), allow=(1, -2))

    def set_contact_angle(self, degrees):
        """ps_set_contact_angle: the angle (degrees, inside the liquid) at which the liquid surface meets every solid, for every later setup
        of this context that computes the curvature, across uploads; a negative value (the default) is off.  Returns the ps_result: INVALID
        for a NaN, an infinity or a value above 180 (the previous setting kept).  Arrays "contactAngle", "contactCosine", "contactField",
        "contactCells", "surfaceWetted" say what the last setup did."""
        return self._check(self.L.ps_set_contact_angle(self.h, float(degrees)), allow=(1, -2))

    def upload_contact_cosine_field(self, field):
        """ps_upload_contact_cosine_field: cos(theta) per cell, painted into the solid cells, for the grid of the last upload (None drops
        it); `field` is a host array or a torch tensor on the host.  Returns the ps_result (INVALID for a value outside [-1, 1], the reason
        in last_error()); FAILED raises."""
        if getattr(field, "is_cuda", False):
            raise TypeError("a device tensor goes through upload_contact_cosine_field_device")
        f = self._host_cell_field(field.numpy() if hasattr(field, "data_ptr") else field, np.float32, "the field must hold one value per cell")
        return self._check(self.L.ps_upload_contact_cosine_field(self.h, None if f is None else f.ctypes.data), allow=(1, -2))

    def upload_contact_cosine_field_device(self, field, layout=0, stream=None):
        """ps_upload_contact_cosine_field_device (None drops the field): `field` is fp32 device memory in `layout` (a DeviceBuffer, a torch
        tensor, an address).  Returns the ps_result, INVALID for a refused call."""
        return self._check(self.L.ps_upload_contact_cosine_field_device(self.h, device_address(field), int(layout), stream_handle(stream)),
                           allow=(1, -2))

    def set_rheology(self, model=_abi.RHEOLOGY_HERSCHEL_BULKLEY, flow_index=1.0, yield_stress=0.0, min_shear_rate=1e-3,
                     min_viscosity=1e-3, max_viscosity=1e6, passes=0):
        """ps_set_rheology: the uploaded viscosity becomes the consistency K of the Herschel-Bulkley law
        mu = clamp(K s^(n-1) + yield_stress / s, min_viscosity, max_viscosity), s = max(shear rate, min_shear_rate), for every later setup
        of this context, across uploads; `passes` extra Picard passes per step (0..8).  RHEOLOGY_NEWTONIAN (0) is the default.  Returns
        the ps_result: INVALID for an out-of-range value (the reason in last_error(), the previous setting kept)."""
        r = _abi.Rheology(int(model), int(passes), float(flow_index), float(yield_stress), float(min_shear_rate), float(min_viscosity),
                          float(max_viscosity))
        return self._check(self.L.ps_set_rheology(self.h, C.byref(r)), allow=(1, -2))

    def set_solve_precision(self, mode):
        """ps_set_solve_precision: PRECISION_FP64 (0, the default) or PRECISION_MIXED (1: the PCG runs in passes on fp32 vectors around the
        fp64 x, and the stop rule is decided on the fp64 residual b - A x) for every later PCG solve of this context, across uploads.  Returns
        the ps_result: INVALID for another mode (the previous setting kept).  Arrays "solvePrecisionUsed", "solvePassIterations",
        "solveTrueResidual" say what the last solve did."""
        return self._check(self.L.ps_set_solve_precision(self.h, int(mode)), allow=(1, -2))

    def set_velocity_extrapolation(self, layers):
        """ps_set_velocity_extrapolation: 0 (the default) is off; n = 1 .. EXTRAPOLATION_MAX_LAYERS carries the written velocity n faces deep
        into the invalid faces after the write-back of every later single-domain step of this context, across uploads.  Returns the
        ps_result: INVALID for a value outside 0..64 (the previous setting kept).  Arrays "velocityExtrapolation",
        "extrapolationLayerX" / Y / Z, "extrapolationCounts" say what the last step did."""
        return self._check(self.L.ps_set_velocity_extrapolation(self.h, int(layers)), allow=(1, -2))

    def set_collider_loads(self, count, pivots=None):
        """ps_set_collider_loads: 0 (the default) is off; count = 1 .. COLLIDER_MAX makes every later single-domain step of this context that
        solves and writes the velocity compute the force and torque of the liquid on colliders 0 .. count-1, across uploads.  pivots: (count, 3)
        points the torques are taken about (None: the upload's orig).  Returns the ps_result: INVALID for a count outside 0..64 or a
        non-finite pivot (the previous setting kept).  Arrays "colliderLoads", "colliderForce", "colliderTorque", "colliderLoadTerms",
        "colliderLoadScale" and collider_loads() say what the last step computed."""
        piv = None if pivots is None else np.ascontiguousarray(pivots, dtype=np.float64).ravel()
        if piv is not None and 0 <= int(count) <= _abi.COLLIDER_MAX and piv.size != 3 * int(count):
            raise ValueError("pivots must hold 3 values per collider")
        cl = _abi.ColliderLoads(int(count), None if piv is None else piv.ctypes.data)
        return self._check(self.L.ps_set_collider_loads(self.h, C.byref(cl)), allow=(1, -2))

    def upload_collider_ids(self, ids):
        """ps_upload_collider_ids: the collider of every cell (int32, shape (nz, ny, nx)) for the grid of the last upload; None drops the
        field.  Returns the ps_result (INVALID before any upload); FAILED raises."""
        f = self._host_cell_field(ids, np.int32, "ids must hold one value per cell")
        return self._check(self.L.ps_upload_collider_ids(self.h, None if f is None else f.ctypes.data), allow=(1, -2))

    def upload_collider_ids_device(self, ids, layout=0, stream=None):
        """ps_upload_collider_ids_device (None drops the field): `ids` is int32 device memory in `layout`.  Returns the ps_result, INVALID
        for a refused call."""
        return self._check(self.L.ps_upload_collider_ids_device(self.h, device_address(ids), int(layout), stream_handle(stream)), allow=(1, -2))

    def collider_loads(self):
        """ps_get_collider_loads: (count, 6) float64, Fx Fy Fz Tx Ty Tz per collider of the last step; raises when it computed none."""
        n = int(self.array("colliderLoads")[0]) if self.L.ps_query_array(self.h, b"colliderLoads", None) >= 0 else 0
        out = np.empty((max(n, 1), 6), np.float64)
        self._check(self.L.ps_get_collider_loads(self.h, out.ctypes.data, 6 * n))
        return out[:n]

    def collider_loads_device(self, out, length, stream=None):
        """ps_get_collider_loads_device into `out` (device memory of `length` doubles).  Returns the ps_result (INVALID: a refused pointer;
        the host is NOT synchronised); raises when the last step computed no loads."""
        return self._check(self.L.ps_get_collider_loads_device(self.h, device_address(out), int(length), stream_handle(stream)), allow=(1, -2))

    def paint_collider_velocities(self, motions):
        """ps_paint_collider_velocities: `motions` has shape (count, 9) — v[3], w[3], o[3] per collider; the velocity v + w x (r - o) of the
        collider each face belongs to (the more solid of its two cells, by the collision SDF and the ids of upload_collider_ids) goes into
        the collisionvel of the last upload, at once.  Returns the ps_result: INVALID before any upload, for a count outside 1..64 or a
        value that is not finite (nothing written).  Arrays "colliderMotions", "colliderMotionTable", "colliderMotionFaces" and
        "collisionVelocityX" / Y / Z say what the call left."""
        m = np.ascontiguousarray(motions, dtype=np.float64)
        if m.ndim != 2 or m.shape[1] != 9:
            raise ValueError("motions must hold 9 values per collider")
        cm = _abi.ColliderMotions(m.shape[0], m.ctypes.data)
        return self._check(self.L.ps_paint_collider_velocities(self.h, C.byref(cm)), allow=(1, -2))

    def paint_collider_velocities_device(self, ptr, count, stream=None):
        """ps_paint_collider_velocities_device: the same from 9 * count doubles of device memory, read behind what `stream` holds.  Returns
        the ps_result (INVALID: a refused pointer or count; the host is NOT synchronised).  A collider whose values are not all finite
        paints nothing: its faces are counted in the last slot of "colliderMotionFaces"."""
        return self._check(self.L.ps_paint_collider_velocities_device(self.h, device_address(ptr), int(count), stream_handle(stream)), allow=(1, -2))

    def set_collider_shapes(self, shapes):
        """ps_set_collider_shapes: `shapes` is a sequence of (sdf, h, orig) — sdf a float32 array of shape (n2, n1, n0) (x fastest, the body's
        own frame, the sign convention of the collision field), h the sample spacing, orig the body-frame low corner of the volume; None
        or an empty sequence drops the shapes.  A context setting: copied at once, kept across uploads.  Returns the ps_result: INVALID
        for a refused shape (the reason in last_error(), the previous shapes kept).  Array "colliderShapes" holds the count."""
        shapes = [] if shapes is None else list(shapes)
        if not shapes:
            return self._check(self.L.ps_set_collider_shapes(self.h, None), allow=(1, -2))
        tab = (_abi.ColliderShape * len(shapes))()
        keep = []
        for k, (sdf, h, orig) in enumerate(shapes):
            v = None if sdf is None else np.ascontiguousarray(sdf, dtype=np.float32)
            if v is not None and v.ndim != 3:
                raise ValueError("a shape's sdf must be a (n2, n1, n0) array")
            keep.append(v)
            n = (0, 0, 0) if v is None else v.shape[::-1]
            tab[k].n[0], tab[k].n[1], tab[k].n[2] = (int(q) for q in n)
            tab[k].reserved, tab[k].h = 0, float(h)
            tab[k].orig[0], tab[k].orig[1], tab[k].orig[2] = (float(q) for q in orig)
            tab[k].sdf = None if v is None else v.ctypes.data
        cs = _abi.ColliderShapes(len(shapes), tab)
        return self._check(self.L.ps_set_collider_shapes(self.h, C.byref(cs)), allow=(1, -2))

    def place_colliders(self, poses):
        """ps_place_colliders: `poses` has shape (count, 12) — R[9] row-major (body to world), t[3] per collider, count the shapes' count;
        every shape is placed into the collision field and the id field of the last upload, at once: a cell takes the largest solid
        depth among what it holds and the colliders that reach it, and the id of the winner.  Returns the ps_result: INVALID before any
        upload, without shapes, for another count or a value that is not finite (nothing written).  Arrays "colliderPlacement",
        "colliderPoseTable", "colliderPlacedCells", "collisionField" and "colliderCellIds" say what the call left."""
        m = np.ascontiguousarray(poses, dtype=np.float64)
        if m.ndim != 2 or m.shape[1] != 12:
            raise ValueError("poses must hold 12 values per collider")
        cp = _abi.ColliderPoses(m.shape[0], m.ctypes.data)
        return self._check(self.L.ps_place_colliders(self.h, C.byref(cp)), allow=(1, -2))

    def place_colliders_device(self, ptr, count, stream=None):
        """ps_place_colliders_device: the same from 12 * count doubles of device memory, read behind what `stream` holds.  Returns the
        ps_result (INVALID: a refused pointer or count; the host is NOT synchronised).  A collider whose pose is not all finite places
        nothing and is counted in the last slot of "colliderPlacedCells"."""
        return self._check(self.L.ps_place_colliders_device(self.h, device_address(ptr), int(count), stream_handle(stream)), allow=(1, -2))

    def advection(self, dt, order=2, cell_in=(), cell_out=(), carrier=None, vel_out=None):
        """The ps_advection of a call from addresses or arrays (numpy arrays by their data pointer, device arrays through device_address);
        carrier / vel_out: None or three arrays."""
        def addr(a):
            return a.ctypes.data if isinstance(a, np.ndarray) else device_address(a)
        A = _abi.Advection()
        A.dt, A.order, A.cellFields = float(dt), int(order), len(cell_in)
        if len(cell_in) != len(cell_out) or len(cell_in) > _abi.ADVECT_MAX_CELL_FIELDS:
            raise ValueError("as many outputs as inputs, at most %d" % _abi.ADVECT_MAX_CELL_FIELDS)
        for q, (i, o) in enumerate(zip(cell_in, cell_out)):
            A.cellIn[q], A.cellOut[q] = addr(i), addr(o)
        for a in range(3):
            A.carrier[a] = None if carrier is None else addr(carrier[a])
            A.velOut[a] = None if vel_out is None else addr(vel_out[a])
        return A

    def advect(self, dt, cell_fields=(), order=2, carrier=None, velocity=False, scheme=None, limiter=_abi.ADVECT_LIMIT_CLAMP):
        """ps_advect_fields on host arrays: every array of `cell_fields` (float32, shape (nz, ny, nx)) and, with `velocity`, the carrier
        itself moved semi-Lagrangian over `dt` by the carrier — three face grids, or None for the velocity the last step wrote.  order 1
        is the Euler back-trace, 2 the midpoint one.  Returns (rc, cell outputs, velocity outputs or None); INVALID for a refused call
        (the reason in last_error(), nothing written).  Arrays "advection", "advectionStep", "advectionCounts" say what the call did.
        With `scheme` (ADVECT_SEMI_LAGRANGIAN or ADVECT_MACCORMACK) the call is ps_advect_fields_scheme with that scheme and `limiter`
        (ADVECT_LIMIT_NONE / _CLAMP / _REVERT); the MacCormack correction also leaves "advectionScheme" and "advectionCorrection"."""
        sh = _abi.grid_shapes(self.scene.nx, self.scene.ny, self.scene.nz)
        cin = [np.ascontiguousarray(f, dtype=np.float32).reshape(sh["center"]) for f in cell_fields]
        car = None if carrier is None else [np.ascontiguousarray(carrier[a], dtype=np.float32).reshape(sh["face" + "XYZ"[a]]) for a in range(3)]
        cout = [np.empty(sh["center"], np.float32) for _ in cin]
        vout = [np.empty(sh["face" + a], np.float32) for a in "XYZ"] if velocity else None
        A = self.advection(dt, order, cin, cout, car, vout)
        if scheme is None:
            rc = self._check(self.L.ps_advect_fields(self.h, C.byref(A)), allow=(1, -2))
        else:
            S = _abi.AdvectionScheme(int(scheme), int(limiter))
            rc = self._check(self.L.ps_advect_fields_scheme(self.h, C.byref(A), C.byref(S)), allow=(1, -2))
        return rc, cout, vout

    def advect_device(self, dt, cell_in=(), cell_out=(), order=2, carrier=None, vel_out=None, layout=0, stream=None, scheme=None,
                      limiter=_abi.ADVECT_LIMIT_CLAMP):
        """ps_advect_fields_device: the same on device arrays in `layout`, behind what `stream` holds; `stream` then waits for the outputs
        and the host is NOT synchronised.  No output may overlap an input or another output.  Returns the ps_result (INVALID: refused).
        With `scheme` the call is ps_advect_fields_scheme_device."""
        A = self.advection(dt, order, cell_in, cell_out, carrier, vel_out)
        if scheme is None:
            return self._check(self.L.ps_advect_fields_device(self.h, C.byref(A), int(layout), stream_handle(stream)), allow=(1, -2))
        S = _abi.AdvectionScheme(int(scheme), int(limiter))
        return self._check(self.L.ps_advect_fields_scheme_device(self.h, C.byref(A), C.byref(S), int(layout), stream_handle(stream)), allow=(1, -2))

    def label_air_pockets(self):
        """ps_label_air_pockets: labels the connected air regions of the grid of the last upload (single domain) and returns their number K.
        The labels last until the next upload (or set_slab / set_brick); arrays "airPockets", "airPocketIds", "airPocketUnits",
        "airPocketCells", "airPocketOpen", "airPocketVolume", "airPocketPasses" say what the call found."""
        k = C.c_int32(-1)
        self._check(self.L.ps_label_air_pockets(self.h, C.byref(k)))
        return int(k.value)

    def _air_pocket_count(self):
        return int(self.array("airPockets")[0]) if self.L.ps_query_array(self.h, b"airPockets", None) >= 0 else 0

    def air_pockets(self):
        """ps_get_air_pockets: (volume float64[K], open int32[K]) of the current labels; raises without labels."""
        n = self._air_pocket_count()
        vol, opn = np.empty(max(n, 1), np.float64), np.empty(max(n, 1), np.int32)
        self._check(self.L.ps_get_air_pockets(self.h, vol.ctypes.data, opn.ctypes.data, n))
        return vol[:n], opn[:n]

    def air_pocket_ids(self):
        """ps_download_air_pocket_ids: the pocket of every cell (int32, shape (nz, ny, nx); -1: none); raises without labels."""
        out = np.empty(_abi.grid_shapes(self.scene.nx, self.scene.ny, self.scene.nz)["center"], np.int32)
        self._check(self.L.ps_download_air_pocket_ids(self.h, out.ctypes.data))
        return out

    def air_pocket_ids_device(self, out, layout=0, stream=None):
        """ps_download_air_pocket_ids_device into `out` (int32 device memory, one value per cell, in `layout`).  Returns the ps_result
        (INVALID: a refused pointer or layout; the host is NOT synchronised); raises without labels."""
        return self._check(self.L.ps_download_air_pocket_ids_device(self.h, device_address(out), int(layout), stream_handle(stream)), allow=(1, -2))

    def set_air_pocket_pressures(self, p):
        """ps_set_air_pocket_pressures: one pressure per pocket (K float64 values) becomes the pressure member of the free-surface fields, a
        sigma field staying; None drops the pressure member alone.  Returns the ps_result: INVALID for a length other than K or a value
        that is not finite (nothing changed); raises without labels."""
        if p is None:
            return self._check(self.L.ps_set_air_pocket_pressures(self.h, None, 0), allow=(1, -2))
        v = np.ascontiguousarray(p, dtype=np.float64).ravel()
        buf = v if v.size else np.zeros(1, np.float64)      # (K = 0: a valid pointer with len 0; NULL means "drop")
        return self._check(self.L.ps_set_air_pocket_pressures(self.h, buf.ctypes.data, v.size), allow=(1, -2))

    def solution_fields(self):
        """ps_download_solution_fields: the last solve's [p; tau] as dense fp32 grids (x fastest), keyed pressure, txx, tyy, tzz, tyz, txz, txy;
        0 where a sample has no such DOF."""
        sh = _abi.grid_shapes(self.scene.nx, self.scene.ny, self.scene.nz)
        out = {name: np.empty(sh[grid], np.float32) for name, grid in _abi.SOLUTION_FIELDS}
        so = _abi.SolutionOut()
        so.pressure = out["pressure"].ctypes.data
        for a, name in enumerate(("txx", "tyy", "tzz")):
            so.tauDiag[a] = out[name].ctypes.data
        for a, name in enumerate(("tyz", "txz", "txy")):
            so.tauEdge[a] = out[name].ctypes.data
        self._check(self.L.ps_download_solution_fields(self.h, C.byref(so)))
        return out

    def set_slab(self, slab):
        st = _abi.SlabStruct(slab.rank, slab.world, slab.zLoOwned, slab.zHiOwned, slab.hasLower, slab.hasUpper, slab.z0)
        self._check(self.L.ps_set_slab(self.h, C.byref(st)))

    def set_brick(self, b):
        """b: partition.Brick (ps_set_brick: the decomposition along all three axes)."""
        i3 = C.c_int32 * 3
        st = _abi.BrickStruct(b.rank, b.world, i3(*b.dims), i3(*b.lo), i3(*b.hi), i3(*b.hasLower), i3(*b.hasUpper), i3(*b.g0))
        self._check(self.L.ps_set_brick(self.h, C.byref(st)))

    def comm_selftest(self):
        self._check(self.L.ps_comm_selftest(self.h))

    def dist_stats(self):
        """What this rank's last distributed solve did (ps_dist_stats): dict of bytes per iteration over its cuts, owned DOFs,
        whether the exchanges overlapped, sampled transport / all-reduce times, halo cells whose label the owners' exchange changed."""
        v = (C.c_double * 8)()
        self._check(self.L.ps_dist_stats(self.h, v))
        return {"halo_bytes_per_iter": v[0], "owned_dofs": v[1], "overlap": bool(v[2]),
                "exchange_ms_per_transport": (v[3] / v[4]) if v[4] else None, "exchange_samples": int(v[4]),
                "allreduce_ms": (v[5] / v[6]) if v[6] else None, "allreduce_samples": int(v[6]), "halo_label_changes": int(v[7])}

    def memory_stats(self):
        """ps_memory_stats: device bytes held through the library in this process, their peak, bytes this context dropped that still wait for
        release, live contexts"""
        v = (C.c_int64 * 4)()
        self.L.ps_memory_stats(self.h, v)
        return {"live_bytes": int(v[0]), "peak_bytes": int(v[1]), "deferred_bytes": int(v[2]), "contexts": int(v[3])}

    def comm_init(self, uid_bytes, rank, world):
        buf = C.create_string_buffer(bytes(uid_bytes), 128)
        self._check(self.L.ps_comm_init_rccl(self.h, buf, rank, world))

    def comm_init_tcp(self, rank, world, host="127.0.0.1", base_port=29600):
        """host-staged transport (one process per rank, ranks may share a GPU); collective over the world"""
        self._check(self.L.ps_comm_init_tcp(self.h, rank, world, host.encode(), base_port))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, allow=(1,)):
        if rc == _abi.FAILED or rc not in allow:
            raise PolyStokesError(f"rc={rc}: {self.L.ps_last_error(self.h).decode()}")
        return rc

    def upload(self, scene, params):
        self.scene, self.params = scene, params
        fi = scene.fields_in()
        self._check(self.L.ps_upload_fields(self.h, C.byref(params), C.byref(fi)))
        self._scene_surface_tension(scene)
        if getattr(scene, "density_field", None) is not None:
            self._check(self.upload_density_field(scene.density_field))
        if _has_surface_fields(scene):
            self._check(self.upload_surface_fields(scene.surface_sigma_field, scene.surface_pressure_field))
        if getattr(scene, "contact_cosine_field", None) is not None:
            self._check(self.upload_contact_cosine_field(scene.contact_cosine_field))

    def _host_cell_field(self, field, dtype, wrong_size=None):
        """A host cell field as the ABI takes it: None, or a contiguous array of `dtype` with one value per cell of the last upload's grid.
        Another size raises ValueError(wrong_size), or whatever reshaping to the cell grid raises when no message is given."""
        if field is None:
            return None
        f = np.ascontiguousarray(field, dtype=dtype)
        if self.scene is None:
            return f
        sh = _abi.grid_shapes(self.scene.nx, self.scene.ny, self.scene.nz)["center"]
        if wrong_size is not None:
            if f.size != sh[0] * sh[1] * sh[2]:
                raise ValueError(wrong_size)
            return f
        return f if f.shape == sh else f.reshape(sh)

    def _scene_surface_tension(self, scene):
        """Scene.surface_tension and Scene.contact_angle (None: the context keeps its setting) -> ps_set_surface_tension,
        ps_set_contact_angle; a refused value raises."""
        sigma = getattr(scene, "surface_tension", None)
        if sigma is not None:
            self._check(self.L.ps_set_surface_tension(self.h, float(sigma)))
        angle = getattr(scene, "contact_angle", None)
        if angle is not None:
            self._check(self.L.ps_set_contact_angle(self.h, float(angle)))

    def upload_density_field(self, field):
        """ps_upload_density_field: a cell density field for the grid of the last upload (None drops it).  Returns the ps_result
        (INVALID for a refused field, the reason in last_error()); FAILED raises."""
        f = self._host_cell_field(field, np.float32)
        if f is not None:
            self._density_keep = f
        return self._check(self.L.ps_upload_density_field(self.h, None if f is None else f.ctypes.data), allow=(1, -2))

    def upload_surface_fields(self, sigma=None, pressure=None):
        """ps_upload_surface_fields: the free-surface cell fields for the grid of the last upload — the surface-tension coefficient (None:
        the scalar of set_surface_tension) and the ambient pressure (None: 0); both None drops them.  Returns the ps_result (INVALID for a
        refused field, the reason in last_error()); FAILED raises."""
        keep = self._host_cell_field(sigma, np.float32), self._host_cell_field(pressure, np.float32)
        sf = _abi.SurfaceFields(*[None if f is None else f.ctypes.data for f in keep])
        return self._check(self.L.ps_upload_surface_fields(self.h, C.byref(sf)), allow=(1, -2))

    def last_error(self):
        return self.L.ps_last_error(self.h).decode()

    # ---- device-resident fields (ps_*_device): `fields` carries Scene's attributes with device arrays (device_scene, torch tensors, ...) ----
    def upload_device(self, params, fields, layout=0, stream=None):
        """ps_upload_fields_device.  Returns the ps_result (INVALID for a refused call, the reason in last_error()); FAILED raises."""
        fi = fields_in_device(fields)
        rc = self._check(self.L.ps_upload_fields_device(self.h, C.byref(params), C.byref(fi), int(layout), stream_handle(stream)),
                         allow=(1, -2))
        if rc == 1:
            self.scene, self.params = fields, params
            self._scene_surface_tension(fields)
        return rc

    def upload_density_field_device(self, field, layout=0, stream=None):
        """ps_upload_density_field_device (None drops the field).  Returns the ps_result, INVALID for a refused field."""
        return self._check(self.L.ps_upload_density_field_device(self.h, device_address(field), int(layout), stream_handle(stream)),
                           allow=(1, -2))

    def upload_surface_fields_device(self, sigma=None, pressure=None, layout=0, stream=None):
        """ps_upload_surface_fields_device (both None drops the fields).  Returns the ps_result, INVALID for a refused field."""
        sf = _abi.SurfaceFields(device_address(sigma), device_address(pressure))
        return self._check(self.L.ps_upload_surface_fields_device(self.h, C.byref(sf), int(layout), stream_handle(stream)), allow=(1, -2))

    def _device_out(self, out):
        """(ps_fields_out, vel buffers, valid buffers): `out` = (vel[3], valid[3]) of device arrays (entries may be None), or None to allocate."""
        from . import _hip
        sh = _abi.grid_shapes(self.scene.nx, self.scene.ny, self.scene.nz)
        n = [int(np.prod(sh["face" + a])) for a in "XYZ"]
        vel, valid = out if out is not None else ([_hip.DeviceBuffer(n[a]) for a in range(3)], [_hip.DeviceBuffer(n[a]) for a in range(3)])
        fo = FieldsOut()
        for a in range(3):
            fo.vel[a], fo.valid[a] = device_address(vel[a]), device_address(valid[a])
        return fo, vel, valid

    def download_device(self, layout=0, stream=None, out=None):
        """ps_download_fields_device into `out` (see _device_out).  Returns (rc, vel, valid); the host is NOT synchronised: work queued on
        `stream` after the call sees the outputs."""
        fo, vel, valid = self._device_out(out)
        rc = self._check(self.L.ps_download_fields_device(self.h, C.byref(fo), int(layout), stream_handle(stream)), allow=(1, -2))
        return rc, vel, valid

    def solution_fields_device(self, layout=0, stream=None, out=None):
        """ps_download_solution_fields_device: dict of device arrays keyed like solution_fields() (allocated unless `out` gives them)."""
        from . import _hip
        sh = _abi.grid_shapes(self.scene.nx, self.scene.ny, self.scene.nz)
        if out is None:
            out = {name: _hip.DeviceBuffer(int(np.prod(sh[grid]))) for name, grid in _abi.SOLUTION_FIELDS}
        so = _abi.SolutionOut()
        so.pressure = device_address(out.get("pressure"))
        for a, name in enumerate(("txx", "tyy", "tzz")):
            so.tauDiag[a] = device_address(out.get(name))
        for a, name in enumerate(("tyz", "txz", "txy")):
            so.tauEdge[a] = device_address(out.get(name))
        self._check(self.L.ps_download_solution_fields_device(self.h, C.byref(so), int(layout), stream_handle(stream)))
        return out

    def step_device_fields(self, params, fields, layout=0, stream=None, out=None):
        """ps_step_device_fields: polystokes_step on device arrays.  Returns (rc, vel, valid) (see download_device; INVALID: refused)."""
        self.scene, self.params = fields, params
        self._scene_surface_tension(fields)
        fi = fields_in_device(fields)
        fo, vel, valid = self._device_out(out)
        rc = self._check(self.L.ps_step_device_fields(self.h, C.byref(params), C.byref(fi), C.byref(fo), C.byref(self.stats), int(layout),
                                                      stream_handle(stream)), allow=(0, 1, -2, -3, -4))
        return rc, vel, valid

    def setup(self):
        return self._check(self.L.ps_setup_device(self.h, C.byref(self.stats)))

    def solve(self):
        return self._check(self.L.ps_solve_device(self.h, C.byref(self.stats)), allow=(0, 1, -3, -4))

    def step_device(self):
        return self._check(self.L.ps_step_device(self.h, C.byref(self.stats)), allow=(0, 1, -3, -4))

    def step(self, scene, params):
        """solveGasSubclass equivalent on host buffers (HDK_PolyStokes.C:222-609)."""
        if (getattr(scene, "density_field", None) is not None or _has_surface_fields(scene)
                or getattr(scene, "contact_cosine_field", None) is not None):   # upload, the fields, step, download: polystokes_step has no field
            self.upload(scene, params)
            rc = self.step_device()
            self.download()
            return rc
        self.scene, self.params = scene, params
        self._scene_surface_tension(scene)
        fi = scene.fields_in()
        out, keep = self._fields_out()
        rc = self._check(self.L.polystokes_step(self.h, C.byref(params), C.byref(fi), C.byref(out), C.byref(self.stats)),
                         allow=(0, 1, -3, -4))
        self.vel, self.valid = keep[:3], keep[3:]
        return rc

    def _fields_out(self):
        sh = _abi.grid_shapes(self.scene.nx, self.scene.ny, self.scene.nz)
        keep = [np.empty(sh["face" + a], np.float32) for a in "XYZ"] + [np.empty(sh["face" + a], np.float32) for a in "XYZ"]
        out = FieldsOut()
        for a in range(3):
            out.vel[a] = keep[a].ctypes.data
            out.valid[a] = keep[3 + a].ctypes.data
        return out, keep

    def download(self):
        out, keep = self._fields_out()
        self._check(self.L.ps_download_fields(self.h, C.byref(out)))
        self.vel, self.valid = keep[:3], keep[3:]
        return self.vel, self.valid

    def array(self, name):
        eb = C.c_int32(0)
        n = self.L.ps_query_array(self.h, name.encode(), C.byref(eb))
        if n < 0:
            raise KeyError(name)
        out = np.empty(n, dtype=_DT[(eb.value, _kind(name))])
        if n:
            self._check(self.L.ps_read_array(self.h, name.encode(), out.ctypes.data, out.nbytes))
        return out

    def apply(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        self._check(self.L.ps_apply_operator(self.h, x.ctypes.data, y.ctypes.data))
        return y

    def precondition(self, r):
        """z = M^-1 r of the configured preconditioner (reference numbering)"""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.empty_like(r)
        self._check(self.L.ps_apply_preconditioner(self.h, r.ctypes.data, z.ctypes.data))
        return z

    def bench_kernel(self, name, iters=20):
        ms, by = C.c_double(0), C.c_double(0)
        self._check(self.L.ps_bench_kernel(self.h, name.encode(), iters, C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def export_component_matrices(self, prefix):
        self._check(self.L.ps_export_component_matrices(self.h, prefix.encode()))

    def export_matrices(self, prefix):
        self._check(self.L.ps_export_matrices(self.h, prefix.encode()))

    def solve_exported_system(self, prefix, params, dt, n):
        """PCG on a component set written by exportComponentMatrices (files <prefix>Mat_*.mtx, Vec_b.mtx).  Returns (rc, x); rc is INCOMPLETE
        when the interrupt callback stopped the solve at a batch end (x is then the iterate reached)."""
        x = np.zeros(n, np.float64)
        rc = self._check(self.L.ps_solve_exported_system(self.h, prefix.encode(), C.byref(params), dt, x.ctypes.data, n, C.byref(self.stats)),
                         allow=(0, 1, _abi.INCOMPLETE))
        return rc, x

    def export_stats(self, prefix):
        self._check(self.L.ps_export_stats(self.h, C.byref(self.stats), prefix.encode()))

    # convenience accessors into dimData (Solver.cpp:578-593)
    @property
    def nP(self):
        return int(self.stats.dimData[12])

    @property
    def nT(self):
        return int(self.stats.dimData[13])

    @property
    def nA(self):
        return int(self.stats.dimData[7])

    @property
    def nRegions(self):
        return int(self.stats.dimData[24])

    def S_matrices(self):
        """(S, St) as scipy CSR in REFERENCE numbering — rows of S are face rows (active faces in reference
        order, then reduced-with-entries), columns [p; tau] as in Solver.h:586-606.  On the device both are
        stored in the block-interleaved internal numbering; `sysPerm` / `rowPerm` map reference -> internal."""
        import scipy.sparse as sp
        n = self.nP + self.nT
        nA = self.nA
        sys_perm, row_perm = self.array("sysPerm"), self.array("rowPerm")
        ptr, col, val = self.array("S.ptr"), self.array("S.col"), self.array("S.val")
        nrows = len(ptr) - 1
        S = sp.csr_matrix((val, col, ptr), shape=(nrows, n))
        rows = np.concatenate([row_perm, np.arange(nA, nrows, dtype=row_perm.dtype)])
        S_ref = S[rows, :][:, sys_perm].tocsr()
        ptr, col, val = self.array("St.ptr"), self.array("St.col"), self.array("St.val")
        St = sp.csr_matrix((val, col, ptr), shape=(n, nrows))
        St_ref = St[sys_perm, :][:, rows].tocsr()
        S_ref.sort_indices()
        St_ref.sort_indices()
        return S_ref, St_ref


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 creates it, the harness broadcasts it)."""
    buf = C.create_string_buffer(128)
    if lib().ps_comm_unique_id(buf) != 1:
        raise PolyStokesError("ncclGetUniqueId failed")
    return bytes(buf.raw)


class Group:
    """`world` ranks inside one process on one GPU (device copies instead of RCCL): the distributed algorithm
    on a single-GPU box.  Same kernels, exchange lists and reduction order as the one-process-per-GPU path."""

    def __init__(self, world, device=0, dims=None):
        """dims = (dx, dy, dz) ranks per axis (bricks, dx * dy * dz == world); None: z-slabs."""
        self.L = lib()
        if dims is not None and dims[0] * dims[1] * dims[2] != world:
            raise ValueError("dims must multiply to world")
        self.dims = tuple(dims) if dims is not None else None
        g = self.L.ps_group_create(device, world)
        if not g:
            raise PolyStokesError(self.L.ps_last_error(None).decode())
        self.g = C.c_void_p(g)
        self.world = world
        self.ranks = [Solver(device, _handle=self.L.ps_group_rank(self.g, r)) for r in range(world)]
        self.stats = Stats()

    def step(self):
        rc = self.L.ps_group_step(self.g, C.byref(self.stats))
        if rc == _abi.FAILED:
            raise PolyStokesError(self.L.ps_last_error(self.ranks[0].h).decode())
        for r in self.ranks:
            r.stats = self.stats
        return rc

    def set_scene(self, scene, params, per_rank=None, when="after_cut"):
        """Partition `scene` into slabs or bricks, upload every rank's part and set its slab or brick; returns the parts (self.slabs).
        per_rank(solver, part, local_scene), if given, is called once on every rank between its upload and the step — before its
        ps_set_slab / ps_set_brick with when = "before_cut", after it with "after_cut": the place for the calls that follow an upload
        (ps_upload_collider_ids, ps_place_colliders, ps_paint_collider_velocities).  The local scene carries the rank's own orig."""
        from . import partition
        if when not in ("before_cut", "after_cut"):
            raise ValueError('when must be "before_cut" or "after_cut"')
        if self.dims is None:
            parts = [partition.make_slab(scene.nz, self.world, r, params.tileSize) for r in range(self.world)]
        else:
            parts = [partition.make_brick((scene.nx, scene.ny, scene.nz), self.dims, r, params.tileSize) for r in range(self.world)]
        for r, part in enumerate(parts):
            local = partition.local_scene(scene, part) if self.dims is None else partition.local_scene_brick(scene, part)
            self.ranks[r].upload(local, params)                                    # (with the scene's optional cell fields cut to the part)
            if per_rank is not None and when == "before_cut":
                per_rank(self.ranks[r], part, local)
            if self.dims is None:
                self.ranks[r].set_slab(part)
            else:
                self.ranks[r].set_brick(part)
            if per_rank is not None and when == "after_cut":
                per_rank(self.ranks[r], part, local)
        self.slabs = parts
        if self.dims is not None:
            self.bricks = parts
        return parts

    def solve_scene(self, scene, params, per_rank=None, when="after_cut"):
        """Partition `scene` into slabs or bricks, run the distributed step, merge the owned faces into global arrays.  per_rank, when:
        see set_scene."""
        from . import partition
        parts = self.set_scene(scene, params, per_rank, when)
        rc = self.step()
        merge = partition.merge_faces if self.dims is None else partition.merge_faces_brick
        sh = _abi.grid_shapes(scene.nx, scene.ny, scene.nz)
        vel = [np.array(scene.vel[a], copy=True) for a in range(3)]
        valid = [np.zeros(sh["face" + "XYZ"[a]], np.float32) for a in range(3)]
        for r, part in enumerate(parts):
            lv, lval = self.ranks[r].download()
            for a in range(3):
                owned = self.ranks[r].array("owned" + "XYZ"[a])
                merge(vel[a], lv[a], owned, part, a)
                merge(valid[a], lval[a], owned, part, a)
        self.vel, self.valid = vel, valid
        return rc

    def close(self):
        if getattr(self, "g", None):
            for r in self.ranks:
                r.h = None
            self.L.ps_group_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _forward_to_ranks(name, note):
    def setter(self, *args, **kw):
        return [getattr(r, name)(*args, **kw) for r in self.ranks][0]
    setter.__name__, setter.__doc__ = name, "ps_%s on every rank (%s)." % (name, note)
    return setter


for _name, _note in (("set_solid_boundary", "a context setting: it holds for every later step of the group"),
                     ("set_contact_angle", "a context setting; a rank rewrites the SDF on its own grid, the halo block covers the reach"),
                     ("set_solve_precision", 'a decomposition solves in fp64 whatever the setting: "solvePrecisionUsed" reads 0'),
                     ("set_velocity_extrapolation", 'a decomposition ignores the setting: "velocityExtrapolation" reads 0'),
                     ("set_collider_loads", 'a decomposition ignores the setting: "colliderLoads" reads 0'),
                     ("set_rheology", "a context setting: it holds for every later step of the group")):
    setattr(Group, _name, _forward_to_ranks(_name, _note))
