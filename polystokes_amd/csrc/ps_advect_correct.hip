// The MacCormack correction of the advection call (ps_advect_fields_scheme with scheme 1; include/polystokes.h states the rule).  The forward
// pass is k_advect itself (ps_advect.hip), launched into the library's own fp32 grids `hat`; then
//   k_advect_correct   one workgroup per 16 x 4 x 4 block of samples of one of the four grids, a thread per sample, like k_advect: the
//                      carrier at the sample once, the departure point p1 recomputed (not stored: 24 bytes per sample written and read
//                      back otherwise), the reverse trace q1 from the same U(p0), and per field eight taps of the source at p1 for the
//                      limits, eight taps of hat at q1, the corrected, limited value, or the bits of hat where the rule falls back
// A sample reads the sources and hat and writes only itself; the counts are integers: the result does not depend on the traversal.
#include <algorithm>
#include <cmath>

#include "ps_kernels_advect.hpp"

using namespace ps;

namespace {

constexpr int CSLOTS = 8;                   // counters: values the limiter changed on the four grids, fallback samples of the four grids

struct CorrectTable {
    AdvectTable A;              // the call's own table: the sources and the caller's outputs
    const float* hc[PS_ADVECT_MAX_CELL_FIELDS];   // hat of the cell fields, in the strides of A.st[0]
    const float* hv[3];         // hat of the velocity, in the strides of A.st[1 + a]
    int32_t* corr;              // CSLOTS
    int limiter;
};

// lo and hi of the eight samples a gather at t would read, in its order (x fastest, then y, then z); a NaN sample fails both comparisons
__device__ __forceinline__ void limitsAt(const float* __restrict__ F, const Taps& t, double& lo, double& hi) {
    const float* v = F + t.base;
    const int64_t ex = t.e[0], ey = t.e[1], ez = t.e[2];
    const double s[8] = {v[0], v[ex], v[ey], v[ey + ex], v[ez], v[ez + ex], v[ez + ey], v[ez + ey + ex]};
    lo = hi = s[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        if (s[k] < lo) lo = s[k];
        if (s[k] > hi) hi = s[k];
    }
}

// (no amdgpu_waves_per_eu: 98 registers and four waves per SIMD — two tap sets are live at once.  With (6) it is 78 and six, and the call
// was 1 % slower, unlike k_advect; profiles/advection_scheme.md)
__global__ __launch_bounds__(ABS) void k_advect_correct(CorrectTable C) {
    const AdvectTable& T = C.A;
    __shared__ int32_t bins[CSLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < CSLOTS) bins[tid] = 0;
    __syncthreads();
    int i[3];
    const int g = sampleOf(T, (int)blockIdx.x, tid, i);
    const int3 d = T.d[g];
    const bool live = i[0] < d.x && i[1] < d.y && i[2] < d.z;
    const int face = g - 1;                         // (-1: the cell grid)
    const int fields = g == 0 ? T.cells : 1;
    unsigned changed = 0;                           // bit q: the limiter changed field q of this sample
    bool fallback = false;
    if (live) {
        const int64_t c = (int64_t)i[0] * T.st[g][0] + (int64_t)i[1] * T.st[g][1] + (int64_t)i[2] * T.st[g][2];
        const int64_t* ss = g == 0 ? T.st[0] : T.cs[face];      // the strides of the source: the carrier may keep its own on a face grid
        const int64_t cF = (int64_t)i[0] * ss[0] + (int64_t)i[1] * ss[1] + (int64_t)i[2] * ss[2];
        double p0[3], p1[3], q1[3], U[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) p0[m] = (double)i[m] + (m == face ? 0. : 0.5);
        carrierAt(T, p0, U);
        Taps t1, t2;
        t1.clamped = t2.clamped = true;
        bool ok = traceFrom(T, p0, U, T.r, p1);
        if (ok) { t1 = tapsAt(d, ss, face, p1); ok = !t1.clamped; }
        if (ok) ok = traceFrom(T, p0, U, -T.r, q1);             // from p0, with -r: negation is exact
        if (ok) { t2 = tapsAt(d, T.st[g], face, q1); ok = !t2.clamped; }
        fallback = !ok;
        for (int q = 0; q < fields; ++q) {
            const float* F = g == 0 ? T.cin[q] : T.car[face];
            const float* H = g == 0 ? C.hc[q] : C.hv[face];
            float* out = g == 0 ? T.cout[q] : T.vout[face];
            const float hat = H[c];
            if (!ok) { out[c] = hat; continue; }    // the bits of the forward value
            const double bar = gather(H, t2);
            double v = (double)hat + 0.5 * ((double)F[cF] - bar);
            if (C.limiter != PS_ADVECT_LIMIT_NONE) {
                double lo, hi;
                limitsAt(F, t1, lo, hi);
                const bool outside = v < lo || v > hi;
                if (C.limiter == PS_ADVECT_LIMIT_CLAMP) v = v < lo ? lo : (v > hi ? hi : v);
                else v = outside ? (double)hat : v;
                changed |= outside ? 1u << q : 0u;
            }
            out[c] = stored(v);
        }
    }
    // per field one count per sample the limiter changed, and one per fallback sample (waveBinAdd; the workgroup adds its bins that are not 0)
    for (int q = 0; q < fields; ++q) waveBinAdd(bins, (changed >> q) & 1u, g, lane);
    waveBinAdd(bins, fallback, 4 + g, lane);
    __syncthreads();
    if (tid < CSLOTS && bins[tid]) atomicAdd(&C.corr[tid], bins[tid]);
}

}  // namespace

// The second launch of a scheme 1 call, on the context's stream behind the forward pass: T is the call's table, H the same with the
// outputs aimed at the forward result's grids.
void ps_context::correctAdvected(const AdvectTable& T, const AdvectTable& H, int total, int limiter) {
    CorrectTable C{};
    C.A = T;
    for (int q = 0; q < PS_ADVECT_MAX_CELL_FIELDS; ++q) C.hc[q] = H.cout[q];
    for (int m = 0; m < 3; ++m) C.hv[m] = H.vout[m];
    advectCorrection.alloc(CSLOTS);
    C.corr = advectCorrection.p;
    C.limiter = limiter;
    HIP_CHECK(hipMemsetAsync(advectCorrection.p, 0, CSLOTS * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_advect_correct, dim3((unsigned)total), dim3(ABS), 0, stream, C);
}
