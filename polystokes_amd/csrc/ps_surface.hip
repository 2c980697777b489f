// Surface tension (ps_set_surface_tension, an extension): the mean curvature of the liquid SDF and the ghost-pressure impulse it adds to
// the right-hand side.  Setup only; nothing here runs with sigma = 0, and nothing here runs per iteration.
//
// The stencil of face f gives cell c the pressure coefficient gradSign wF_f liquidW_c / dx (ps_blocks.hip: faceEntriesT); the rest of the
// cell is the ghost part, whose pressure is 0 without surface tension and sigma kappa_c with it.  Its coefficient g(f,c) is
// gradSign wF_f (1 - liquidW_c) / dx for a cell with a pressure DOF (or inside a reduced tile, whose pressure the basis carries) and
// gradSign wF_f / dx for any other cell of the grid.  The impulse -dt sum_c g(f,c) sigma kappa_c goes into the active rhs of f, or through
// C_f^T into the rhs of its tile: b, the recovery and the exports follow from those two vectors ("Surface tension").
//
// Free-surface fields (ps_upload_surface_fields): the ghost pressure becomes the per-cell q_c = sigma_c kappa_c + P_c (k_surface_ghost_pressure,
// fp64), and the same two force kernels read q with scale = dt in the place of kappa_c with scale = dt sigma ("Free-surface fields").
//
// Contact angles (ps_set_contact_angle): the two curvature kernels read the SDF that ps_wetting.hip rewrote inside the solid in the place of
// the uploaded one; nothing else here changes ("Contact angles").
#include "ps_context.hpp"
#include "ps_setup_util.hpp"

using namespace ps;

namespace {

constexpr int BS = 256;

__device__ inline double phiAt(const float* __restrict__ phi, const int3 d, int i, int j, int k) {   // indices clamped to the grid
    i = i < 0 ? 0 : (i >= d.x ? d.x - 1 : i);
    j = j < 0 ? 0 : (j >= d.y ? d.y - 1 : j);
    k = k < 0 ? 0 : (k >= d.z ? d.z - 1 : k);
    return (double)phi[lin3(d, i, j, k)];
}

// kappa = div(grad phi / |grad phi|) = (phi_x^2 (phi_yy + phi_zz) + phi_y^2 (phi_xx + phi_zz) + phi_z^2 (phi_xx + phi_yy)
//          - 2 phi_x phi_y phi_xy - 2 phi_x phi_z phi_xz - 2 phi_y phi_z phi_yz) / |grad phi|^3, second-order central differences,
// the mixed terms on the 4-point diagonal stencil; 0 where |grad phi| < 1e-6 / dx.  fp64, stored as fp32.
__global__ void k_surface_curvature(Grid g, const float* __restrict__ phi, double invDx, float* __restrict__ kappa) {
    const int3 d = g.dims(0);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int3 q = unlin3(d, c);
    auto P = [&](int di, int dj, int dk) { return phiAt(phi, d, q.x + di, q.y + dj, q.z + dk); };
    const double p0 = P(0, 0, 0);
    const double h1 = 0.5 * invDx, h2 = invDx * invDx, h4 = 0.25 * invDx * invDx;
    const double px = (P(1, 0, 0) - P(-1, 0, 0)) * h1, py = (P(0, 1, 0) - P(0, -1, 0)) * h1, pz = (P(0, 0, 1) - P(0, 0, -1)) * h1;
    const double pxx = (P(1, 0, 0) - 2. * p0 + P(-1, 0, 0)) * h2;
    const double pyy = (P(0, 1, 0) - 2. * p0 + P(0, -1, 0)) * h2;
    const double pzz = (P(0, 0, 1) - 2. * p0 + P(0, 0, -1)) * h2;
    const double pxy = (P(1, 1, 0) - P(1, -1, 0) - P(-1, 1, 0) + P(-1, -1, 0)) * h4;
    const double pxz = (P(1, 0, 1) - P(1, 0, -1) - P(-1, 0, 1) + P(-1, 0, -1)) * h4;
    const double pyz = (P(0, 1, 1) - P(0, 1, -1) - P(0, -1, 1) + P(0, -1, -1)) * h4;
    const double g2 = px * px + py * py + pz * pz;
    const double gn = sqrt(g2);
    double k = 0.;
    if (gn >= 1e-6 * invDx)
        k = (px * px * (pyy + pzz) + py * py * (pxx + pzz) + pz * pz * (pxx + pyy) - 2. * (px * py * pxy + px * pz * pxz + py * pz * pyz)) / (g2 * gn);
    kappa[c] = (float)k;
}

// kappa_c: kappa sampled trilinearly (clamped to the grid) at the closest interface point x_c - phi_c grad phi_c / |grad phi_c|^2 (x_c itself
// where |grad phi| < 1e-6 / dx), clamped to [-1/dx, 1/dx].  Positions in cell-index units: the gradient per cell is (phi[i+1] - phi[i-1]) / 2.
// The step toward the interface is capped at ST_MAX_STEP cells.  A cell with a ghost term and liquidW < 1 lies within about two cells of the
// surface and never reaches the cap; a cell without a pressure DOF inside the liquid (a solid cell under a pool, next to a face on the solid's
// surface) can lie tens of cells deep, and its kappa_c is then that of the level set ST_MAX_STEP cells toward the surface.  The cap keeps every
// read within 1 + ST_MAX_STEP + 1 (trilinear) + 1 (curvature stencil) = 7 cells of a face, inside a decomposition's halo block (>= 16 layers,
// partition.py), so a slab or brick rank computes the single domain's kappa_c on every face it owns.
constexpr double ST_MAX_STEP = 4.0;
__global__ void k_surface_curvature_at_interface(Grid g, const float* __restrict__ phi, const float* __restrict__ kappa, double invDx,
                                                 float* __restrict__ kappaC) {
    const int3 d = g.dims(0);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int3 q = unlin3(d, c);
    auto P = [&](int di, int dj, int dk) { return phiAt(phi, d, q.x + di, q.y + dj, q.z + dk); };
    const double p0 = P(0, 0, 0);
    const double gi[3] = {(P(1, 0, 0) - P(-1, 0, 0)) * 0.5, (P(0, 1, 0) - P(0, -1, 0)) * 0.5, (P(0, 0, 1) - P(0, 0, -1)) * 0.5};
    const double g2 = gi[0] * gi[0] + gi[1] * gi[1] + gi[2] * gi[2];
    const double gn = sqrt(g2);
    const bool move = gn >= 1e-6;                       // |grad phi| >= 1e-6 / dx in world units
    double step = move ? -p0 / g2 : 0.;                 // x_c + step * gi (world x - phi grad phi / |grad phi|^2 with grad phi = gi / dx, over dx)
    if (move && fabs(p0) > ST_MAX_STEP * gn) step *= ST_MAX_STEP * gn / fabs(p0);   // |step * gi| = |phi| / |gi| cells, capped
    const double x[3] = {(double)q.x, (double)q.y, (double)q.z};
    // (not sampleCenterField of ps_setup_util.hpp: other arithmetic — fp64, floor, positions in cell indices, a NaN lands on 0)
    const int n[3] = {d.x, d.y, d.z};
    int i0[3], i1[3];
    double t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double u = x[a] + step * gi[a];
        u = u >= 0. ? u : 0.;                            // (a NaN lands on 0)
        u = u <= (double)(n[a] - 1) ? u : (double)(n[a] - 1);
        int b = (int)floor(u);
        if (b >= n[a] - 1) { i0[a] = i1[a] = n[a] - 1; t[a] = 0.; }
        else { i0[a] = b; i1[a] = b + 1; t[a] = u - (double)b; }
    }
    auto K = [&](int i, int j, int k) { return (double)kappa[lin3(d, i, j, k)]; };
    auto L = [](double a, double b, double tt) { return a + (b - a) * tt; };
    const double c00 = L(K(i0[0], i0[1], i0[2]), K(i1[0], i0[1], i0[2]), t[0]);
    const double c10 = L(K(i0[0], i1[1], i0[2]), K(i1[0], i1[1], i0[2]), t[0]);
    const double c01 = L(K(i0[0], i0[1], i1[2]), K(i1[0], i0[1], i1[2]), t[0]);
    const double c11 = L(K(i0[0], i1[1], i1[2]), K(i1[0], i1[1], i1[2]), t[0]);
    double v = L(L(c00, c10, t[1]), L(c01, c11, t[1]), t[2]);
    v = v < -invDx ? -invDx : (v > invDx ? invDx : v);
    kappaC[c] = (float)v;
}

struct SurfArgs {
    Grid g;
    double invDx, scale;           // scale = dt * sigma with kappa_c as the cell value, dt with q_c
    const float* lwC;              // cell liquid weights
    const float* fwF[3];           // face fluid weights
    const int32_t* labC;           // cell labels
    const int32_t* labF[3];
    const int32_t* regF[3];
    const int32_t* faceRow[3];
    int64_t nA;
};

// sum_c g(f,c) v_c of face (axis, f), v = cellVal (kappa_c in fp32, or the ghost pressure q_c in fp64): the lower cell has gradSign -1,
// the upper +1, a cell outside the grid has no term
template <class T>
__device__ inline double ghostSum(const SurfArgs& A, const T* __restrict__ cellVal, int axis, const int3 f) {
    const int3 cd = A.g.dims(0), fd = A.g.dims(1 + axis);
    const double wF = (double)A.fwF[axis][lin3(fd, f.x, f.y, f.z)];
    double s = 0.;
    if (wF == 0.) return s;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const double sign = dir == 0 ? -1. : 1.;
        int3 c = f;
        addc(c, axis, dir - 1);
        if (comp(c, axis) < 0 || comp(c, axis) >= comp(cd, axis)) continue;
        const int64_t cl = lin3(cd, c.x, c.y, c.z);
        const int l = A.labC[cl];
        const double ghost = (isActiveL(l) || l == PS_REDUCED) ? 1. - (double)A.lwC[cl] : 1.;
        if (ghost == 0.) continue;
        s += sign * wF * ghost * A.invDx * (double)cellVal[cl];
    }
    return s;
}

// active face rows: rhsA[row] -= scale sum_c g(f,c) v_c (internal row numbering, as k_S_fill wrote it)
template <class T>
__global__ void k_surface_tension_force(SurfArgs A, const T* __restrict__ cellVal, int axis, double* __restrict__ rhsA) {
    const int3 d = A.g.dims(1 + axis);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int row = A.faceRow[axis][c];
    if (row < 0 || row >= A.nA) return;
    const double s = ghostSum(A, cellVal, axis, unlin3(d, c));
    if (s != 0.) rhsA[row] -= A.scale * s;
}

// reduced faces: rhs_r += C_f^T (-scale sum_c g(f,c) v_c), one block per region over the union of its three face boxes (as k_skin),
// a fixed summation tree (deterministic).  count += faces with a non-zero impulse.
template <class T>
__global__ void __launch_bounds__(BS) k_surface_tension_tiles(SurfArgs A, const T* __restrict__ cellVal, const int32_t* __restrict__ bbox,
                                                              const double* __restrict__ COM, double dx, int3 off, double* __restrict__ rhsR,
                                                              int32_t* __restrict__ count) {
    const int r = blockIdx.x;
    const RegionBox box = RegionBox::faceUnion(bbox, r);
    const int total = (int)box.total();
    double acc[PS_RD];
#pragma unroll
    for (int n = 0; n < PS_RD; ++n) acc[n] = 0.;
    int hits = 0;
    for (int pos = threadIdx.x; pos < total; pos += BS) {
        const int3 at = box.at(pos);
        const int i = at.x, j = at.y, k = at.z;
        for (int a = 0; a < 3; ++a) {
            const int3 fd = A.g.dims(1 + a);
            if (oob3(fd, i, j, k)) continue;
            const int64_t fl = lin3(fd, i, j, k);
            if (A.labF[a][fl] != PS_REDUCED || A.regF[a][fl] != r) continue;
            const double s = ghostSum(A, cellVal, a, make_int3(i, j, k));
            if (s == 0.) continue;
            ++hits;
            const double imp = -A.scale * s;
            double o[3], row[PS_RD];
            faceOffset(COM + (int64_t)r * 3, dx, off, a, i, j, k, o);
            basisRow(o[0], o[1], o[2], a, row);
#pragma unroll
            for (int n = 0; n < PS_RD; ++n) acc[n] += imp * row[n];
        }
    }
    __shared__ double part[BS / 64][PS_RD];
    __shared__ int hitPart[BS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < PS_RD; ++n) {
        double v = acc[n];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) part[w][n] = v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) hits += __shfl_xor(hits, o, 64);
    if (lane == 0) hitPart[w] = hits;
    __syncthreads();
    if (threadIdx.x < PS_RD) {
        double v = 0.;
#pragma unroll
        for (int q = 0; q < BS / 64; ++q) v += part[q][threadIdx.x];
        if (v != 0.) rhsR[(int64_t)r * PS_RD + threadIdx.x] += v;
    }
    if (threadIdx.x == 0) {
        int h = 0;
        for (int q = 0; q < BS / 64; ++q) h += hitPart[q];
        if (h) atomicAdd(count, h);
    }
}

// q_c = s_c kappa_c + P_c in fp64 from the fp32 inputs: s_c the sigma field or (sigmaC null) the scalar, kappa_c null when neither asks for
// the curvature (the term is then absent), P_c null for 0
__global__ void k_surface_ghost_pressure(int64_t n, const float* __restrict__ sigmaC, double sigma, const float* __restrict__ kappaC,
                                         const float* __restrict__ pressureC, double* __restrict__ q) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double P = pressureC ? (double)pressureC[c] : 0.;
    if (!kappaC) { q[c] = P; return; }
    const double s = sigmaC ? (double)sigmaC[c] : sigma;
    q[c] = s * (double)kappaC[c] + P;
}

// the impulse of the cell values v into rhsA and the tiles' rhs
template <class T>
void launchSurfaceForce(ps_context* c, const SurfArgs& A, const T* cellVal) {
    if (c->nActiveVs > 0)
        for (int a = 0; a < 3; ++a) {
            const int64_t nf = c->g.count(1 + a);
            hipLaunchKernelGGL(k_surface_tension_force<T>, dim3(gridFor(nf, BS)), dim3(BS), 0, c->stream, A, cellVal, a, c->rhsA.p);
        }
    if (c->regionCount > 0)
        hipLaunchKernelGGL(k_surface_tension_tiles<T>, dim3((unsigned)c->regionCount), dim3(BS), 0, c->stream, A, cellVal, (const int32_t*)c->bbox.p,
                           (const double*)c->COM.p, c->dx, make_int3(c->gOff[0], c->gOff[1], c->gOff[2]), c->rhsR.p, c->stReduced.p);
}

}  // namespace

// After constructMatrixBlocks (rhsA) and assembleReducedBlocks (rhs_r = Mr c_fit), before b.  sigma = 0 and no free-surface field: the
// buffers are dropped (deferred frees) and nothing is launched.  With a field of ps_upload_surface_fields the cell value is q_c and the
// scale dt; without one, kappa_c and dt sigma as before the fields existed.
void ps_context::applySurfaceTension() {
    sigmaUsed = sigmaSet;
    surfFieldsUsed = (surfSigmaField ? 1 : 0) | (surfPressureField ? 2 : 0);
    const bool curvature = surfSigmaField || sigmaUsed != 0.;
    if (!curvature) { kappaRaw.free(); kappaC.free(); }
    const float* phi = applyContactAngle(curvature);   // ps_wetting.hip: the SDF rewritten inside the solid, or surface.p (the angle off: nothing launched)
    if (!curvature && surfFieldsUsed == 0) {
        stReduced.free();
        return;
    }
    const int64_t n = g.count(0);
    if (curvature) { kappaRaw.alloc((size_t)n); kappaC.alloc((size_t)n); }
    stReduced.alloc(1);
    HIP_CHECK(hipMemsetAsync(stReduced.p, 0, sizeof(int32_t), stream));
    if (curvature) {
        hipLaunchKernelGGL(k_surface_curvature, dim3(gridFor(n, BS)), dim3(BS), 0, stream, g, phi, invDx, kappaRaw.p);
        hipLaunchKernelGGL(k_surface_curvature_at_interface, dim3(gridFor(n, BS)), dim3(BS), 0, stream, g, phi, (const float*)kappaRaw.p, invDx, kappaC.p);
    }
    SurfArgs A;
    A.g = g; A.invDx = invDx; A.scale = surfFieldsUsed ? dt : dt * sigmaUsed;
    A.lwC = liquidW[0].p; A.labC = labels[0].p; A.nA = nActiveVs;
    for (int a = 0; a < 3; ++a) { A.fwF[a] = fluidW[1 + a].p; A.labF[a] = labels[1 + a].p; A.regF[a] = reducedIdx[1 + a].p; A.faceRow[a] = faceRow[a].p; }
    if (surfFieldsUsed == 0) {
        launchSurfaceForce(this, A, (const float*)kappaC.p);
        return;
    }
    surfQ.alloc((size_t)n);
    hipLaunchKernelGGL(k_surface_ghost_pressure, dim3(gridFor(n, BS)), dim3(BS), 0, stream, n, surfSigmaField ? (const float*)surfSigma.p : nullptr,
                       sigmaUsed, curvature ? (const float*)kappaC.p : nullptr, surfPressureField ? (const float*)surfPressure.p : nullptr, surfQ.p);
    launchSurfaceForce(this, A, (const double*)surfQ.p);
}
