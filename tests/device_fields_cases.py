"""Shared by tests/test_gpu_device_fields.py and its child processes: the scenes of the device-resident field tests, one step through the
host boundary (polystokes_step) or the device boundary (ps_step_device_fields), and the exact comparison of what the two leave behind.

As a script (child process): `device_fields_cases.py release` runs the whole-step case on the library PS_LIB names;
`device_fields_cases.py torch` imports torch FIRST, then the harness, and steps on torch tensors."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARRAYS = ("valuesCoded", "diagonalsCoded", "activeRHSVector")


def smooth_collisionvel(sc):
    """blob's collisionvel is one constant per axis, which no transposition can change: replace it by a smooth field."""
    from polystokes_amd import _abi as abi
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    for a in range(3):
        z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sh["face" + "XYZ"[a]]], indexing="ij")
        sc.collisionvel[a] = (0.2 * (a - 1) + 0.05 * np.sin(0.7 * x + 0.3 * a) * np.cos(0.5 * y) + 0.03 * np.sin(0.9 * z)).astype(np.float32)
    return sc


def scene(name):
    from polystokes_amd import scenes
    if name == "blob":
        sc, p = scenes.blob()
        return smooth_collisionvel(sc), p
    if name == "blob_uniform":
        sc, p = scenes.blob(variable_viscosity=False)
        return smooth_collisionvel(sc), p
    if name == "cavity32":
        return scenes.cavity(32)
    raise KeyError(name)


def weights_scene():
    """blob with all 14 input weights, taken from a first run's weight arrays and handed in under another SDF."""
    import polystokes_amd
    from polystokes_amd import _abi as abi
    sc, p = scene("blob")
    s = polystokes_amd.Solver(0)
    s.upload(sc, p)
    s.setup()
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    w = [s.array(n + kind).reshape(sh[n]) for kind in ("LiquidWeights", "FluidWeights") for n in abi.SAMPLE_NAMES]
    s.close()
    sc2 = abi.Scene(sc.nx, sc.ny, sc.nz, sc.dx, sc.dt, sc.density, sc.vel, sc.surface + np.float32(0.01), sc.collision, sc.viscosity,
                    collisionvel=sc.collisionvel, weights=w, name="blob_weights")
    return sc2, p


def collect(s, rc, vel, valid):
    out = {"rc": np.int64(rc), "solveData": np.array(s.stats.solveData[0:2]), "dimData": np.array(s.stats.dimData[:]),
           "result": np.int64(s.stats.result)}
    for a in range(3):
        out[f"vel{a}"], out[f"valid{a}"] = np.array(vel[a], copy=True), np.array(valid[a], copy=True)
    for n in ARRAYS:
        out[n] = s.array(n)
    return out


def host_step(s, sc, p):
    rc = s.step(sc, p)
    return collect(s, rc, s.vel, s.valid)


def device_outputs(sc, vel, valid, layout):
    """Device output arrays -> (z, y, x) numpy arrays (a blocking copy on the default stream)."""
    import polystokes_amd
    from polystokes_amd import _abi as abi
    sh = abi.grid_shapes(sc.nx, sc.ny, sc.nz)
    back = lambda b, a: polystokes_amd.from_layout(b.to_numpy(), sh["face" + "XYZ"[a]], layout)
    return [back(vel[a], a) for a in range(3)], [back(valid[a], a) for a in range(3)]


def device_step(s, sc, p, layout, pad=0, alias=False):
    import polystokes_amd
    from polystokes_amd import _hip
    ds = polystokes_amd.device_scene(sc, layout, pad)
    out = None
    if alias:
        out = (list(ds.vel), [_hip.DeviceBuffer(b.count) for b in ds.vel])
    rc, vel, valid = s.step_device_fields(p, ds, layout, out=out)
    assert rc != -2, s.last_error()
    v, ok = device_outputs(sc, vel, valid, layout)
    return collect(s, rc, v, ok)


def same(a, b):
    """Names of the entries that differ in their bytes (empty: equal)."""
    bad = [k for k in a if k not in b or np.asarray(a[k]).shape != np.asarray(b[k]).shape or np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]
    return bad + [k for k in b if k not in a]


def _release():
    import polystokes_amd
    assert polystokes_amd.LIB_PATH.endswith("libpolystokes_hip_release.so"), polystokes_amd.LIB_PATH
    sc, p = scene("blob")
    s = polystokes_amd.Solver(0)
    ref = host_step(s, sc, p)
    s.close()
    for layout in (0, 1):
        s = polystokes_amd.Solver(0)
        bad = same(ref, device_step(s, sc, p, layout))
        s.close()
        assert not bad, (layout, bad)
    print("CHILD OK")


class _TorchFields:
    pass


def _torch():
    import torch                      # first: the order a torch pipeline has
    if not torch.cuda.is_available():
        print("CHILD SKIP no torch device")
        return
    import polystokes_amd
    from polystokes_amd import _abi as abi
    sc, p = scene("blob")
    s = polystokes_amd.Solver(0)
    ref = host_step(s, sc, p)
    s.close()
    dev = torch.device("cuda:0")
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).permute(2, 1, 0).contiguous()    # [nx.., ny.., nz..]-indexed: layout 1
    f = _TorchFields()
    for k in ("nx", "ny", "nz", "dx", "dt", "density"):
        setattr(f, k, getattr(sc, k))
    f.vel, f.collisionvel = [put(a) for a in sc.vel], [put(a) for a in sc.collisionvel]
    f.surface, f.collision, f.viscosity, f.weights = put(sc.surface), put(sc.collision), put(sc.viscosity), None
    vel, valid = [torch.empty_like(t) for t in f.vel], [torch.empty_like(t) for t in f.vel]
    stream = torch.cuda.current_stream().cuda_stream
    s = polystokes_amd.Solver(0)
    rc, _, _ = s.step_device_fields(p, f, abi.LAYOUT_Z_FASTEST, stream=stream, out=(vel, valid))
    assert rc != -2, s.last_error()
    torch.cuda.current_stream().synchronize()
    back = lambda t: np.ascontiguousarray(t.cpu().numpy().transpose(2, 1, 0))
    got = collect(s, rc, [back(t) for t in vel], [back(t) for t in valid])
    s.close()
    bad = same(ref, got)
    assert not bad, bad
    print("CHILD OK")


if __name__ == "__main__":
    {"release": _release, "torch": _torch}[sys.argv[1]]()
