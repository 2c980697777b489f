"""The mixed-precision PCG of ps_set_solve_precision restated in numpy (include/polystokes.h, DESIGN.md "Mixed-precision PCG").

x stays fp64.  A pass solves A d = r64, r64 = b - A x formed in fp64, with the correction d, the direction p and the residual r rounded to
fp32 at every store; every product and every sum is fp64 (fsum dot products).  A pass ends when its recurrence meets the stop rule
min(r.r, r.r / x.x) < tol^2 (pcg.h:319-325) or when r.r has fallen to REDUCTION^2 of the true r.r it started from; then x += d, r64 is formed
again and the rule is evaluated on the true values, which alone decides success.  x.x inside a pass: d.d in the first pass of a cold solve
(x = d), otherwise x.x of the x the pass started from.  A pass that does not halve the true ||r|| ends the scheme ("stagnated": the
library continues in fp64 from that x).

What this restatement cannot do is round the face-row vector t inside the operator or A p in the five-kernel step: the device does both.
The caps the GPU test asserts (tests/test_gpu_mixed_precision.py) are asserted on this algorithm alone by test_mixed_precision_ref_cpu.py."""
import numpy as np

from helpers import fdot, numpy_pcg

REDUCTION = 1e-4          # MIXED_PASS_REDUCTION of ps_solve.hip
MAX_PASSES = 8            # MIXED_MAX_PASSES
ITERATION_CAP = lambda it64: 1.10 * it64 + 2      # sum of the passes' iterations against the fp64 solve's
PASS_CAP = 4
ERROR_CAP = 2.0           # ||x - x*|| against ||x64 - x*||


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def rule(r, x):
    """min(r.r, r.r / x.x) with correctly rounded sums"""
    rr, xx = fdot(r, r), fdot(x, x)
    return min(rr, rr / xx) if xx > 0 else rr


def mixed_pcg(A, M, b, x0, tol, maxit):
    """Returns dict(status: 'success' | 'stagnated' | 'maxit', x, passes: iterations run by each pass, rre: the true value of the rule at
    the last evaluation).  A(v), M(r): fp64 operator and preconditioner; x0 None: a cold start."""
    n = len(b)
    cold = x0 is None
    x = np.zeros(n) if cold else np.array(x0, np.float64)
    passes, total = [], 0
    rr_start = 0.0
    for k in range(MAX_PASSES + 1):
        have_x = (not cold) or k > 0
        r64 = b - A(x) if have_x else b.copy()
        rr_true, xx_true = fdot(r64, r64), fdot(x, x)
        rre = min(rr_true, rr_true / xx_true) if xx_true > 0 else rr_true
        if k > 0 and rre < tol * tol:
            return dict(status="success", x=x, passes=passes, rre=rre)
        if k > 0 and (not rr_true < 0.25 * rr_start or k == MAX_PASSES):
            return dict(status="stagnated", x=x, passes=passes, rre=rre)
        if total >= maxit:
            return dict(status="maxit", x=x, passes=passes, rre=rre)
        rr_start = rr_true
        floor = REDUCTION * REDUCTION * rr_true
        xx_fix = xx_true if have_x else 0.0
        r = f32(r64)
        p = f32(M(r))
        rsold = fdot(r, p)
        d = np.zeros(n)
        ran, ended = 0, False
        while total + ran < maxit:
            Ap = A(p)
            alpha = rsold / fdot(p, Ap)
            d = f32(d + alpha * p)
            r = f32(r - alpha * Ap)
            ran += 1
            rr = fdot(r, r)
            xx = xx_fix if xx_fix > 0 else fdot(d, d)
            est = min(rr, rr / xx) if xx > 0 else rr
            if est < tol * tol or rr < floor:
                ended = True
                break
            z = M(r)
            rz = fdot(r, z)
            p = f32(z + (rz / rsold) * p)
            rsold = rz
        passes.append(ran)
        total += ran
        x = x + d
        if not ended:
            r64 = b - A(x)
            return dict(status="maxit", x=x, passes=passes, rre=rule(r64, x))
    raise AssertionError("unreachable")


def fp64_pcg(A, M, b, tol, maxit):
    """the fp64 solve the library's mode 0 runs: (index of the iteration that met the rule, x)"""
    return numpy_pcg(A, M, b, np.zeros(len(b)), tol, maxit)
