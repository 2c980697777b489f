// Non-Newtonian viscosity (ps_set_rheology, an extension): the strain rate of the velocity field and the Herschel-Bulkley viscosity it
// gives, one setup kernel; and the Picard passes of a single-domain step.  Nothing here runs with the Newtonian model.
//
// The kernel writes mu_c and gammaDot_c per cell; the setup then samples mu as it samples an uploaded viscosity field (CellField::sample of
// ps_setup_util.hpp, handed out by ps_context::viscSource), so the tile matrices, the stress diagonal and every format decision after it follow unchanged.
#include "ps_context.hpp"

#include <chrono>
#include <cstring>

using namespace ps;

namespace {

constexpr int BS = 256;

struct RheoArgs {
    Grid g;
    double dx;
    const float* vel[3];        // face grids: the uploaded velocity (first solve) or the last pass's output
    const int32_t* labF[3];     // final face labels: a sample is used iff its label is neither UNSOLVED nor UNASSIGNED
    const float* K;             // cell grid: the uploaded viscosity field, the consistency of the law
    double n, tauY, minRate, minVisc, maxVisc;
    int powerOne;               // n == 1: K * s^0 without the power, so that K is exact
};

__device__ inline bool used(const RheoArgs& A, int a, int64_t f) {
    const int l = A.labF[a][f];
    return l != PS_UNSOLVED && l != PS_UNASSIGNED;
}

// du_a/dx_b at the a-face q of face grid fd: false when a sample lies outside the grid or is unused
__device__ inline bool centralDiff(const RheoArgs& A, int a, int b, const int3 fd, int3 q, double* out) {
    const int qb = comp(q, b);
    if (qb - 1 < 0 || qb + 1 >= comp(fd, b)) return false;
    int3 lo = q, hi = q;
    addc(lo, b, -1); addc(hi, b, 1);
    const int64_t fl = lin3(fd, lo.x, lo.y, lo.z), fh = lin3(fd, hi.x, hi.y, hi.z);
    if (!used(A, a, fl) || !used(A, a, fh)) return false;
    *out = ((double)A.vel[a][fh] - (double)A.vel[a][fl]) / (2. * A.dx);
    return true;
}

// G_ab(c) = du_a/dx_b at cell q: the mean over the two a-faces of q of the differences that exist, 0 if none does
__device__ inline double gradAt(const RheoArgs& A, int a, int b, const int3 q) {
    const int3 fd = A.g.dims(1 + a);
    int3 f1 = q;
    addc(f1, a, 1);
    double g0 = 0., g1 = 0.;
    const bool h0 = centralDiff(A, a, b, fd, q, &g0), h1 = centralDiff(A, a, b, fd, f1, &g1);
    if (h0 && h1) return 0.5 * (g0 + g1);
    return h0 ? g0 : (h1 ? g1 : 0.);
}

// One thread per cell, x fastest: the reads of neighbouring lanes are neighbouring words of the three face grids (the reuse between the
// stencils of adjacent cells is served by L1 / L2); the two writes are coalesced fp32 vector stores.
__global__ void __launch_bounds__(BS) k_rheology(RheoArgs A, float* __restrict__ mu, float* __restrict__ rate) {
    const int3 d = A.g.dims(0);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int3 q = unlin3(d, c);
    double Dd[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int3 fd = A.g.dims(1 + a);
        int3 f1 = q;
        addc(f1, a, 1);
        const int64_t l0 = lin3(fd, q.x, q.y, q.z), l1 = lin3(fd, f1.x, f1.y, f1.z);
        Dd[a] = (used(A, a, l0) && used(A, a, l1)) ? ((double)A.vel[a][l1] - (double)A.vel[a][l0]) / A.dx : 0.;
    }
    const double Dxy = 0.5 * (gradAt(A, 0, 1, q) + gradAt(A, 1, 0, q));
    const double Dxz = 0.5 * (gradAt(A, 0, 2, q) + gradAt(A, 2, 0, q));
    const double Dyz = 0.5 * (gradAt(A, 1, 2, q) + gradAt(A, 2, 1, q));
    const double gd = sqrt(2. * (Dd[0] * Dd[0] + Dd[1] * Dd[1] + Dd[2] * Dd[2]) + 4. * (Dxy * Dxy + Dxz * Dxz + Dyz * Dyz));
    const double s = gd > A.minRate ? gd : A.minRate;
    const double K = (double)A.K[c];
    double m = (A.powerOne ? K : K * pow(s, A.n - 1.)) + A.tauY / s;
    m = m > A.minVisc ? m : A.minVisc;
    m = m < A.maxVisc ? m : A.maxVisc;
    mu[c] = (float)m;
    rate[c] = (float)gd;
}

}  // namespace

// setupPhase(2), after constructActiveIndices (the final labels) and before the tile matrices, which sample the field viscSource() returns.
// The Newtonian model drops the buffers (deferred frees) and launches nothing.
void ps_context::computeRheology() {
    rheoModelUsed = rheoSet.model;
    if (rheoModelUsed == PS_RHEOLOGY_NEWTONIAN) {
        rheoMu.free(); rheoRate.free();
        return;
    }
    const int64_t n = g.count(0);
    rheoMu.alloc((size_t)n); rheoRate.alloc((size_t)n);
    RheoArgs A;
    A.g = g; A.dx = dx;
    for (int a = 0; a < 3; ++a) { A.vel[a] = rheoFromOut ? velOut[a].p : vel[a].p; A.labF[a] = labels[1 + a].p; }
    A.K = viscosity.p;
    A.n = rheoSet.flowIndex; A.tauY = rheoSet.yieldStress; A.minRate = rheoSet.minShearRate;
    A.minVisc = rheoSet.minViscosity; A.maxVisc = rheoSet.maxViscosity;
    A.powerOne = rheoSet.flowIndex == 1. ? 1 : 0;
    hipLaunchKernelGGL(k_rheology, dim3(gridFor(n, BS)), dim3(BS), 0, stream, A, rheoMu.p, rheoRate.p);
}

// ps_step_device / polystokes_step on a single domain: setup and solve, then with the model on and passes = k > 0, k Picard passes.  Each
// pass sets up again from the last pass's output velocity (labels, weights and numbering come out identical: they do not depend on the
// viscosity), solves from the last pass's [p; tau] through the warm-start grids, recovers and writes back.  Stats: the last pass's result,
// error and iterations, the time entries summed.
int ps_context::stepWithPasses(ps_stats* stats) {
    struct Reset {
        ps_context* c;
        ~Reset() { c->rheoPass = 0; c->rheoFromOut = false; c->rheoCarry = false; }
    } reset{this};
    const int passes = rheoSet.model != PS_RHEOLOGY_NEWTONIAN ? rheoSet.passes : 0;
    ps_stats sum{};
    int result = PS_INCOMPLETE;
    for (int k = 0; k <= passes; ++k) {
        rheoPass = k;
        rheoFromOut = k > 0;
        rheoCarry = k < passes;
        const int rc = setup(nullptr);
        if (rc != PS_SUCCESS) return rc;
        result = solveStage(nullptr);
        if (k == 0) sum = lastStats;
        else {
            for (int q = 2; q < 6; ++q) sum.solveData[q] += lastStats.solveData[q];
            for (int q = 0; q < 16; ++q) sum.stage_ms[q] += lastStats.stage_ms[q];
            sum.solveData[0] = lastStats.solveData[0]; sum.solveData[1] = lastStats.solveData[1];
            sum.result = lastStats.result; sum.usedBiCGStab = lastStats.usedBiCGStab;
            std::memcpy(sum.dimData, lastStats.dimData, sizeof(sum.dimData));
        }
        const bool kept = result == PS_SUCCESS || (result == PS_NOCONVERGE && P.keepNonConvergedResults);
        if (!kept) break;
    }
    if (passes > 0 && warmMode != PS_WARM_PREVIOUS_STEP) {   // the carried iterate served the passes only
        dropWarmStart();
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    lastStats = sum;
    if (stats) *stats = lastStats;
    return result;
}
