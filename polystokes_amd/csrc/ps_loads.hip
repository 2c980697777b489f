// Collider loads (ps_set_collider_loads, an extension): the force and the torque of the liquid on every collider, summed from the solve's
// own x = [p; tau] right after the write-back (include/polystokes.h states every term).  Nothing here runs with count = 0.
//   k_loads_partial   one launch over the four sample grids that carry DOFs (cells, YZ / XZ / XY edges; blockIdx.y = grid): a thread forms the
//                     at most 6 terms of its sample and the workgroup leaves one partial per collider that occurs in it
//   k_loads_sum       sums the partials of every collider in workgroup order and writes the results
// One by-value table holds the grids (the idiom of ps_extrapolate.hip).  The result is bitwise reproducible: there is no floating-point
// atomic and every sum has one order — lanes in the tree of waveSum, waves in wave order, the tiles of a workgroup in rising order,
// workgroups in rising order — which depends on the grid's extents alone.
#include <algorithm>
#include <cstring>

#include "ps_context.hpp"

using namespace ps;

namespace {

constexpr int LBS = 256;            // threads per workgroup of k_loads_partial: four waves
constexpr int LWAVES = LBS / 64;
constexpr int LMAXGRID = 1024;      // workgroups per sample grid at most (include/polystokes.h states the partials' bytes with it)
constexpr int NV = 12;              // sums per collider: F[3], T[3], A[3], B[3]

struct LoadsTable {
    int3 d[4];                  // extents of the cell grid and of the YZ / XZ / XY edge grids
    int3 fd[3];                 // extents of the three face grids
    const int32_t* map[7];      // sample -> internal DOF (-1: none), in the order of solutionGrids() (ps_solve.hip): p, txx, tyy, tzz, tyz, txz, txy
    const float* wL[4];         // liquid weights of the sample's own grid
    const float* wF[3];         // face fluid weights
    const float* wC;            // centre fluid weights (the attribution of an edge term)
    const int32_t* ids;         // collider of every cell; null: collider 0
    const double* x;            // the solution, internal numbering
    int64_t n;                  // its length
    const double* pivots;       // 3 * count
    double dx, dx2, orig[3];
    int count;
};

__device__ inline double waveSum(double v) {    // the total in lane 0; a fixed tree
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ inline int waveSumI(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// what a thread's terms add up to: all of them belong to one collider
struct Acc {
    double v[NV];
    int terms;
    __device__ __forceinline__ void term(int a, double f, const double* arm) {   // (a: a constant after unrolling, so v[] stays in registers)
        const int a1 = a == 2 ? 0 : a + 1, a2 = a == 0 ? 2 : a - 1;
        const double t1 = arm[a2] * f, t2 = -(arm[a1] * f);
        v[a] += f; v[6 + a] += fabs(f);
        v[3 + a1] += t1; v[9 + a1] += fabs(t1);
        v[3 + a2] += t2; v[9 + a2] += fabs(t2);
        ++terms;
    }
};

// the solution entry as ps_download_solution_fields returns it: rounded to fp32, 0 without a DOF
__device__ inline double solutionValue(const LoadsTable& T, int q, int64_t s) {
    const int32_t i = T.map[q][s];
    return (i >= 0 && i < T.n) ? (double)(float)T.x[i] : 0.;
}

// The terms of cell c: pressure and normal stress on each axis, at the cell centre.  The two faces of a cell lie inside the face grid.
__device__ __forceinline__ void cellTerms(const LoadsTable& T, const int3 c, int64_t cl, const double* pivot, Acc& A) {
    const double P = solutionValue(T, 0, cl);
    const double Taa[3] = {solutionValue(T, 1, cl), solutionValue(T, 2, cl), solutionValue(T, 3, cl)};
    if (P == 0. && Taa[0] == 0. && Taa[1] == 0. && Taa[2] == 0.) return;
    const double wl = (double)T.wL[0][cl];
    const double arm[3] = {T.orig[0] + ((double)c.x + 0.5) * T.dx - pivot[0], T.orig[1] + ((double)c.y + 0.5) * T.dx - pivot[1],
                           T.orig[2] + ((double)c.z + 0.5) * T.dx - pivot[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int3 up = c;
        addc(up, a, 1);
        const double d = (double)T.wF[a][lin3(T.fd[a], up.x, up.y, up.z)] - (double)T.wF[a][lin3(T.fd[a], c.x, c.y, c.z)];
        if (d == 0.) continue;
        if (P != 0.) A.term(a, ((-T.dx2 * wl) * P) * d, arm);
        if (Taa[a] != 0.) A.term(a, ((T.dx2 * wl) * Taa[a]) * d, arm);
    }
}

// The terms of edge e of the edge grid with edge axis EA (the in-plane axes are the other two): shear on each in-plane axis a from the two
// a-faces at e and e - e_b, skipped when either lies outside the a-face grid.
template <int EA>
__device__ __forceinline__ void edgeTermsT(const LoadsTable& T, const int3 e, int64_t el, const double* pivot, Acc& A) {
    const double tau = solutionValue(T, 4 + EA, el);
    if (tau == 0.) return;
    const double wl = (double)T.wL[1 + EA][el];
    double arm[3] = {T.orig[0] + (double)e.x * T.dx - pivot[0], T.orig[1] + (double)e.y * T.dx - pivot[1], T.orig[2] + (double)e.z * T.dx - pivot[2]};
    arm[EA] = T.orig[EA] + ((double)comp(e, EA) + 0.5) * T.dx - pivot[EA];
    constexpr int p0 = EA == 0 ? 1 : 0, p1 = EA == 2 ? 1 : 2;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const int a = w == 0 ? p0 : p1, b = w == 0 ? p1 : p0;
        int3 lo = e;
        addc(lo, b, -1);
        const int3 fd = T.fd[a];
        if (oob3(fd, e.x, e.y, e.z) || oob3(fd, lo.x, lo.y, lo.z)) continue;
        const double d = (double)T.wF[a][lin3(fd, e.x, e.y, e.z)] - (double)T.wF[a][lin3(fd, lo.x, lo.y, lo.z)];
        if (d == 0.) continue;
        A.term(a, ((T.dx2 * wl) * tau) * d, arm);
    }
}

__device__ inline void edgeTerms(const LoadsTable& T, int EA, const int3 e, int64_t el, const double* pivot, Acc& A) {
    if (EA == 0) edgeTermsT<0>(T, e, el, pivot, A); else if (EA == 1) edgeTermsT<1>(T, e, el, pivot, A); else edgeTermsT<2>(T, e, el, pivot, A);
}

// the collider of an edge term: the cell with the smallest centre fluid weight among the in-grid cells around the edge, the candidates in
// rising x-fastest index so that the strict comparison keeps the lowest index of a tie
__device__ inline int edgeCollider(const LoadsTable& T, int EA, const int3 e) {
    const int p0 = EA == 0 ? 1 : 0, p1 = EA == 2 ? 1 : 2;   // p0 < p1: p1 has the longer stride
    int id = -1;
    float best = 0.f;
    bool have = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int3 c = e;
        addc(c, p1, (q >> 1) - 1);
        addc(c, p0, (q & 1) - 1);
        if (oob3(T.d[0], c.x, c.y, c.z)) continue;
        const int64_t cl = lin3(T.d[0], c.x, c.y, c.z);
        const float w = T.wC[cl];
        if (!have || w < best) { best = w; id = T.ids[cl]; have = true; }
    }
    return id;
}

// One workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of LBS consecutive samples of grid blockIdx.y.  Per tile every wave
// reduces its lanes per collider — once when its lanes share one id, else once per distinct id in the order of each id's first lane, the
// other lanes adding an exact 0 — and the waves add their totals to the workgroup's LDS bins one wave after the other: the bins see one
// order of additions.  Only lane 0 of the wave whose turn it is touches the bins: no two lanes meet on an LDS bank, and no LDS atomic is
// needed.  A tile without a term (most of a grid: a term needs a DOF next to a solid) costs one barrier.  At the end the workgroup stores
// the bins of the colliders that occurred in it, their term counts, its dropped terms and the mask of those colliders; k_loads_sum reads
// nothing else, so a partial nobody wrote is never read.
__global__ __launch_bounds__(LBS) void k_loads_partial(LoadsTable T, double* __restrict__ partial, int32_t* __restrict__ partialN,
                                                       unsigned long long* __restrict__ occurs) {
    __shared__ double bins[PS_COLLIDER_MAX][NV];
    __shared__ int32_t binN[PS_COLLIDER_MAX + 1];      // [count]: dropped terms
    __shared__ unsigned long long occ;
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = T.count;
    for (int t = tid; t < count * NV; t += LBS) bins[t / NV][t % NV] = 0.;
    for (int t = tid; t <= count; t += LBS) binN[t] = 0;
    if (tid == 0) occ = 0ull;
    __syncthreads();
    const int3 d = T.d[q];
    const int64_t n = (int64_t)d.x * d.y * d.z;
    for (int64_t base = (int64_t)blockIdx.x * LBS; base < n; base += (int64_t)gridDim.x * LBS) {
        Acc A;
#pragma unroll
        for (int v = 0; v < NV; ++v) A.v[v] = 0.;
        A.terms = 0;
        int id = 0, dropped = 0;
        const int64_t s = base + tid;
        if (s < n) {
            const int3 p = unlin3(d, s);
            // a sample without a DOF has no term: its id is not looked up (cells: any of the four maps)
            bool dof;
            if (q == 0) dof = T.map[0][s] >= 0 || T.map[1][s] >= 0 || T.map[2][s] >= 0 || T.map[3][s] >= 0;
            else dof = T.map[3 + q][s] >= 0;
            if (dof) {
                if (T.ids) id = q == 0 ? T.ids[s] : edgeCollider(T, q - 1, p);
                if (id >= 0 && id < count) {
                    const double pivot[3] = {T.pivots[3 * id], T.pivots[3 * id + 1], T.pivots[3 * id + 2]};
                    if (q == 0) cellTerms(T, p, s, pivot, A); else edgeTerms(T, q - 1, p, s, pivot, A);
                } else {   // count the terms only
                    const double zero[3] = {0., 0., 0.};
                    if (q == 0) cellTerms(T, p, s, zero, A); else edgeTerms(T, q - 1, p, s, zero, A);
                    dropped = A.terms;
                    A.terms = 0;
                }
            }
        }
        const bool has = A.terms > 0;
        if (!__syncthreads_or((has || dropped > 0) ? 1 : 0)) continue;   // (the same answer in every thread of the workgroup)
        for (int w = 0; w < LWAVES; ++w) {
            if (wave == w) {
                const int dsum = waveSumI(dropped);
                if (lane == 0 && dsum) binN[count] += dsum;
                unsigned long long m = __ballot(has);
                while (m) {
                    const int kid = __shfl(id, __ffsll((long long)m) - 1, 64);
                    const bool mine = has && id == kid;
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const double sum = waveSum(mine ? A.v[v] : 0.);
                        if (lane == 0) bins[kid][v] += sum;
                    }
                    const int tsum = waveSumI(mine ? A.terms : 0);
                    if (lane == 0) { binN[kid] += tsum; occ |= 1ull << kid; }
                    m &= ~__ballot(mine);
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned long long mask = occ;
    for (int t = tid; t < count * NV; t += LBS)
        if ((mask >> (t / NV)) & 1ull) partial[(wg * count + t / NV) * NV + t % NV] = bins[t / NV][t % NV];
    for (int t = tid; t <= count; t += LBS)
        if (t == count || ((mask >> t) & 1ull)) partialN[wg * (count + 1) + t] = binN[t];
    if (tid == 0) occurs[wg] = mask;
}

// Thread t < 13 count: collider t / 13, value t % 13 (12: its term count); thread 13 count: the dropped terms.  Each walks the workgroups
// in rising order and adds the partial where the workgroup's mask names the collider.  out: force (3 count), torque (3 count), scale
// (A_k, B_k: 6 count), then Fx Fy Fz Tx Ty Tz per collider (6 count).
__global__ __launch_bounds__(64) void k_loads_sum(const double* __restrict__ partial, const int32_t* __restrict__ partialN,
                                                   const unsigned long long* __restrict__ occurs, int64_t workgroups, int count,
                                                   double* __restrict__ out, int32_t* __restrict__ terms) {
    constexpr int SB = 16;      // workgroups per batch: their masks, then their partials, are loaded together; the additions keep the order
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t > count * (NV + 1)) return;
    if (t == count * (NV + 1)) {
        int32_t dn = 0;
#pragma unroll SB
        for (int64_t w = 0; w < workgroups; ++w) dn += partialN[w * (count + 1) + count];   // (every workgroup writes this one)
        terms[count] = dn;
        return;
    }
    const int k = t / (NV + 1), v = t % (NV + 1);
    if (v == NV) {
        int32_t tn = 0;
        for (int64_t w0 = 0; w0 < workgroups; w0 += SB) {
            bool on[SB];
            int32_t p[SB];
#pragma unroll
            for (int j = 0; j < SB; ++j) on[j] = w0 + j < workgroups && ((occurs[w0 + j] >> k) & 1ull);
#pragma unroll
            for (int j = 0; j < SB; ++j) p[j] = on[j] ? partialN[(w0 + j) * (count + 1) + k] : 0;
#pragma unroll
            for (int j = 0; j < SB; ++j) tn += p[j];
        }
        terms[k] = tn;
        return;
    }
    double sum = 0.;
    for (int64_t w0 = 0; w0 < workgroups; w0 += SB) {
        bool on[SB];
        double p[SB];
#pragma unroll
        for (int j = 0; j < SB; ++j) on[j] = w0 + j < workgroups && ((occurs[w0 + j] >> k) & 1ull);
#pragma unroll
        for (int j = 0; j < SB; ++j) p[j] = on[j] ? partial[((w0 + j) * count + k) * NV + v] : 0.;
#pragma unroll
        for (int j = 0; j < SB; ++j) if (on[j]) sum += p[j];
    }
    const int a = v % 3;
    if (v < 3) { out[3 * k + a] = sum; out[12 * (int64_t)count + 6 * k + a] = sum; }
    else if (v < 6) { out[3 * (int64_t)count + 3 * k + a] = sum; out[12 * (int64_t)count + 6 * k + 3 + a] = sum; }
    else if (v < 9) out[6 * (int64_t)count + 6 * k + a] = sum;
    else out[6 * (int64_t)count + 6 * k + 3 + a] = sum;
}

}  // namespace

// solveStage, after applySolutionToVelocity of a step that solved and whose velocity is written, inside the write-back bracket and before
// extrapolateVelocity.  Two launches and one small copy (the pivots) on the context's stream, no host synchronisation.
void ps_context::computeColliderLoads() {
    const int count = loadsCount;
    LoadsTable T{};
    int64_t most = 1;
    for (int q = 0; q < 4; ++q) {
        const int s = q == 0 ? 0 : 3 + q;
        T.d[q] = g.dims(s); T.wL[q] = liquidW[s].p;
        most = std::max(most, g.count(s));
    }
    for (int a = 0; a < 3; ++a) { T.fd[a] = g.dims(1 + a); T.wF[a] = fluidW[1 + a].p; T.orig[a] = orig[a]; }
    const int32_t* maps[7] = {sysIdx[0].p, sysIdxT[0].p, sysIdxT[1].p, sysIdxT[2].p, sysIdx[4].p, sysIdx[5].p, sysIdx[6].p};
    for (int q = 0; q < 7; ++q) T.map[q] = maps[q];
    T.wC = fluidW[0].p;
    T.ids = colliderIds.p;
    T.x = x.p; T.n = nSystem;
    T.dx = dx; T.dx2 = dx * dx; T.count = count;
    const int perGrid = (int)std::min<int64_t>(LMAXGRID, gridFor(most, LBS));
    const int64_t W = 4 * (int64_t)perGrid;
    loadsPartial.alloc((size_t)(W * count * NV));
    loadsPartialN.alloc((size_t)(W * (count + 1)));
    loadsOccurs.alloc((size_t)W);
    loadsOut.alloc((size_t)(18 * count));
    loadsTerms.alloc((size_t)(count + 1));
    loadsPivotsDev.alloc((size_t)(3 * count));
    double piv[3 * PS_COLLIDER_MAX];
    for (int q = 0; q < 3 * count; ++q) piv[q] = loadsPivots.empty() ? orig[q % 3] : loadsPivots[(size_t)q];
    HIP_CHECK(hipMemcpyAsync(loadsPivotsDev.p, piv, (size_t)(3 * count) * sizeof(double), hipMemcpyHostToDevice, stream));   // (pageable source: staged before the call returns)
    T.pivots = loadsPivotsDev.p;
    hipLaunchKernelGGL(k_loads_partial, dim3((unsigned)perGrid, 4), dim3(LBS), 0, stream, T, loadsPartial.p, loadsPartialN.p, loadsOccurs.p);
    hipLaunchKernelGGL(k_loads_sum, dim3((unsigned)gridFor((int64_t)count * (NV + 1) + 1, 64)), dim3(64), 0, stream, (const double*)loadsPartial.p,
                       (const int32_t*)loadsPartialN.p, (const unsigned long long*)loadsOccurs.p, W, count, loadsOut.p, loadsTerms.p);
    loadsUsedHost = count;
}

void ps_context::registerLoadArrays() {
    const int64_t nc = loadsUsedHost;
    const NamedArray list[] = {{"colliderForce", ArrayInfo{loadsOut.p, 3 * nc, 8}}, {"colliderTorque", ArrayInfo{loadsOut.p + 3 * nc, 3 * nc, 8}},
                               {"colliderLoadScale", ArrayInfo{loadsOut.p + 6 * nc, 6 * nc, 8}},   // A_k, B_k per collider
                               {"colliderLoadTerms", ArrayInfo{loadsTerms.p, nc + 1, 4}}};          // terms per collider, then the dropped terms
    setArrays(list, loadsUsedHost > 0);
}

void ps_context::forgetLoads() {
    loadsUsedHost = 0;
    registerLoadArrays();
}

bool ps_context::dropColliderIds() {
    const bool had = colliderIds.p != nullptr;
    colliderIds.free();
    return had;
}

// ps_upload_collider_ids / _device (the ingest of ps_fields.hip; no value is refused).  Ends with the stream idle: the input is consumed
// and whatever was dropped is released.
std::string ps_context::uploadColliderIds(const int32_t* ids, bool fromDevice, int layout, hipStream_t caller) {
    const bool dropped = dropColliderIds();
    if (ids) {
        const CellIn in = cellIn(ids, colliderIds, SCAN_BAD_NONE, "");
        ingestCellFields(&in, 1, fromDevice, layout, caller, false);
    }
    registerPlacementArrays();      // ("colliderCellIds" of ps_place_colliders follows the id field)
    releaseIdle(dropped);
    return {};
}

// Fx Fy Fz Tx Ty Tz per collider of the last step.  Host: a copy and a synchronisation.  Device: queued on our stream behind what the
// caller's stream holds, and the caller's stream then waits for it (a download: no host synchronisation).
void ps_context::copyColliderLoads(double* dst, int64_t len, bool toDevice, hipStream_t caller) {
    if (loadsUsedHost <= 0) throw Error("ps_get_collider_loads: the last step computed no loads");
    const int64_t nd = 6 * (int64_t)loadsUsedHost;
    if (len < nd) throw Error("ps_get_collider_loads: the destination holds fewer than 6 * count doubles");
    HIP_CHECK(hipSetDevice(device));
    const double* src = loadsOut.p + 12 * (int64_t)loadsUsedHost;
    if (toDevice) {
        waitForCaller(caller);
        HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)nd * sizeof(double), hipMemcpyDeviceToDevice, stream));
        releaseToCaller(caller);
    } else {
        HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)nd * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
}
