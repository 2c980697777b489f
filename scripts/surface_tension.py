"""Surface tension (ps_set_surface_tension) measurements for profiles/surface_tension.md.
  laplace [n ...]     Laplace's law on the resting droplet (radius 0.33, sigma 1, no gravity, tolerance 1e-8): the mean pressure of the
                      cells with a pressure DOF and phi < -3 dx against 2 sigma / R, and the spurious max|u| against U = dt sigma (2/R) / (rho dx);
                      with the default layers, and with activeLiquidBoundaryLayerSize = 0, tilePadding = 1 (tiles at the surface)
  setup SCENE N       one step of `SCENE` (coil | spheres) at N^3 with sigma = 0.07 after a warm-up step: run under rocprofv3 --kernel-trace
                      --stats, the k_surface_* rows are the setup time the feature adds
  trace SIGMA N       3 steps of the N^3 cavity (Solver.step, Jacobi); SIGMA "none" never calls ps_set_surface_tension (for kernel traces)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def laplace(ns):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import test_gpu_surface_tension as t
    for n in ns:
        for layers, pad, tag in ((None, 2, "default layers"), (0, 1, "tiles at the surface")):
            pe, ur, it = t.laplace(n, liquid_layers=layers, pad=pad)
            print("laplace n %3d R/dx %5.2f %-20s pressure error %.3f %%  max|u| / U %.3f %%  iterations %d" % (
                n, 0.33 * n, tag, 100 * pe, 100 * ur, it), flush=True)


def setup(scene, n):
    import polystokes_amd
    from polystokes_amd import scenes
    sc, p = getattr(scenes, scene)(n)
    s = polystokes_amd.Solver(0)
    s.set_surface_tension(0.07)
    for _ in range(2):
        rc = s.step(sc, p)
    print("%s %d^3 rc %d setup ms %.2f reduced faces with an impulse %d" % (scene, n, rc, s.stats.solveData[5],
                                                                           int(s.array("surfaceTensionReducedFaces")[0])), flush=True)
    s.close()


def trace(sigma, n):
    import polystokes_amd
    from polystokes_amd import scenes
    sc, p = scenes.cavity(n)
    s = polystokes_amd.Solver(0)
    if sigma != "none":
        s.set_surface_tension(float(sigma))
    for _ in range(3):
        rc = s.step(sc, p)
    print("cavity %d^3 sigma %s rc %d iterations %d" % (n, sigma, rc, int(s.stats.solveData[1])), flush=True)
    s.close()


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "laplace":
        laplace([int(v) for v in sys.argv[2:]] or [32, 48, 64])
    elif cmd == "setup":
        setup(sys.argv[2], int(sys.argv[3]))
    elif cmd == "trace":
        trace(sys.argv[2], int(sys.argv[3]))
    else:
        raise SystemExit(__doc__)
