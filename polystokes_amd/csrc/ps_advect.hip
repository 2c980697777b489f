// Advection (ps_advect_fields, an extension): up to eight cell fields and the MAC velocity moved semi-Lagrangian by a face velocity, the
// context's written velocity or the caller's own (include/polystokes.h states the rule).
//   k_advect    one workgroup per 16 x 4 x 4 block of samples of one of the four grids (cells, faceX, faceY, faceZ), a thread per sample: the
//               carrier at the sample, at the midpoint with order 2, the departure point, and one trilinear gather per field from there
// The table, the sampler and the trace are ps_kernels_advect.hpp, shared with the MacCormack correction (ps_advect_correct.hip), whose forward
// pass is this kernel through launchAdvect.
// One by-value table holds the four grids (the idiom of ps_extrapolate.hip and ps_shapes.hip), so one launch covers all of them.  Either
// axis order is a set of strides in the table (the context's own velocity is x fastest whatever the caller's arrays are); with z fastest
// the block lies 4 x 4 x 16, so that a wave's lanes still run along the caller's fast axis.  A sample reads the inputs and writes only itself, and the counts are integers: the result does not depend on the traversal.
#include <algorithm>
#include <cmath>

#include "ps_kernels_advect.hpp"

using namespace ps;

namespace {

constexpr int ASLOTS = 5;                   // counters: clamped samples of the four grids, samples left alone

// (amdgpu_waves_per_eu(6): 76 registers and six waves per SIMD instead of 82 and five; the call was 2.4 % quicker with it, profiles/advection.md)
__global__ __launch_bounds__(ABS) __attribute__((amdgpu_waves_per_eu(6))) void k_advect(AdvectTable T) {
    __shared__ int32_t bins[ASLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < ASLOTS) bins[tid] = 0;
    __syncthreads();
    int i[3];
    const int g = sampleOf(T, (int)blockIdx.x, tid, i);
    const int3 d = T.d[g];
    const bool live = i[0] < d.x && i[1] < d.y && i[2] < d.z;
    const int face = g - 1;                         // (-1: the cell grid)
    bool alone = false, clamped = false;
    if (live) {
        const int64_t c = (int64_t)i[0] * T.st[g][0] + (int64_t)i[1] * T.st[g][1] + (int64_t)i[2] * T.st[g][2];
        double p0[3], p1[3], U[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) p0[m] = (double)i[m] + (m == face ? 0. : 0.5);
        carrierAt(T, p0, U);
        const bool finite = traceFrom(T, p0, U, T.r, p1);
        if (finite) {
            const Taps t = tapsAt(d, g == 0 ? T.st[0] : T.cs[face], face, p1);
            clamped = t.clamped;
            if (g == 0) { for (int q = 0; q < T.cells; ++q) T.cout[q][c] = stored(gather(T.cin[q], t)); }
            else T.vout[face][c] = stored(gather(T.car[face], t));
        } else {
            alone = true;                           // nothing further is sampled: the sample keeps the bits of its own source sample
            if (g == 0) { for (int q = 0; q < T.cells; ++q) T.cout[q][c] = T.cin[q][c]; }
            else T.vout[face][c] = T.car[face][(int64_t)i[0] * T.cs[face][0] + (int64_t)i[1] * T.cs[face][1] + (int64_t)i[2] * T.cs[face][2]];
        }
    }
    // one count per sample at most: left alone, or clamped on its own grid (waveBinAdd; the workgroup adds its bins that are not 0)
    waveBinAdd(bins, alone || clamped, alone ? ASLOTS - 1 : g, lane);
    __syncthreads();
    if (tid < ASLOTS && bins[tid]) atomicAdd(&T.counts[tid], bins[tid]);
}

}  // namespace

// ps_advect_fields / _device, after the ABI's refusals.  The device form runs on the context's stream between the two event waits of a
// download and does not synchronise the host.  The host form stages every array through one device temporary, x fastest, and ends
// with the stream idle and the temporary released.  limiter < 0: the semi-Lagrangian call.  Otherwise (ps_advect_fields_scheme, scheme 1)
// the same launch writes the forward result into the library's own fp32 grids — the device form's scratch, a further piece of the host
// form's temporary — and correctAdvected (ps_advect_correct.hip) writes the caller's arrays from them.
void ps_context::advectFields(const ps_advection& a, bool fromDevice, int layout, hipStream_t caller, int limiter) {
    HIP_CHECK(hipSetDevice(device));
    const bool ownCarrier = a.carrier[0] != nullptr, vel = a.velOut[0] != nullptr;
    const int cells = a.cellFields;
    AdvectTable T{};
    T.zfast = fromDevice && layout == 1 ? 1 : 0;
    T.order = a.order; T.cells = cells;
    T.r = a.dt / dx;
    int32_t total = 0;
    for (int g4 = 0; g4 < 4; ++g4) {
        const int3 d = g.dims(g4);
        T.d[g4] = d;
        T.st[g4][0] = T.zfast ? (int64_t)d.y * d.z : 1;
        T.st[g4][1] = T.zfast ? d.z : d.x;
        T.st[g4][2] = T.zfast ? 1 : (int64_t)d.x * d.y;
        T.nb[g4][0] = gridFor(d.x, T.zfast ? ABL : ABF); T.nb[g4][1] = gridFor(d.y, ABM); T.nb[g4][2] = gridFor(d.z, T.zfast ? ABF : ABL);
        if (g4 > 0) {
            const bool zf = T.zfast && ownCarrier;
            T.cs[g4 - 1][0] = zf ? (int64_t)d.y * d.z : 1; T.cs[g4 - 1][1] = zf ? d.z : d.x; T.cs[g4 - 1][2] = zf ? 1 : (int64_t)d.x * d.y;
        }
        T.first[g4] = total;
        if (g4 == 0 ? cells > 0 : vel) total += T.nb[g4][0] * T.nb[g4][1] * T.nb[g4][2];
    }
    T.first[4] = total;
    advectCounts.alloc(ASLOTS);
    T.counts = advectCounts.p;
    const bool correct = limiter >= 0;
    const int64_t nc = g.count(0), nf = g.count(1) + g.count(2) + g.count(3);
    const int64_t hatCount = correct ? cells * nc + (vel ? nf : 0) : 0;
    float* hat = nullptr;
    DevBuf<float> stage;         // the host form's temporary: the caller's carrier, the cell fields in, then every output
    int64_t outAt = 0;
    if (fromDevice) {
        waitForCaller(caller);
        for (int m = 0; m < 3; ++m) { T.car[m] = ownCarrier ? a.carrier[m] : velOut[m].p; T.vout[m] = a.velOut[m]; }
        for (int q = 0; q < cells; ++q) { T.cin[q] = a.cellIn[q]; T.cout[q] = a.cellOut[q]; }
        if (correct) { advectScratch.alloc((size_t)hatCount); hat = advectScratch.p; }      // (grows only: the largest such call since the upload)
    } else {
        stage.alloc((size_t)((ownCarrier ? nf : 0) + 2 * cells * nc + (vel ? nf : 0) + hatCount));
        float* at = stage.p;
        auto in = [&](const float* src, int64_t n) {
            HIP_CHECK(hipMemcpyAsync(at, src, (size_t)n * sizeof(float), hipMemcpyHostToDevice, stream));
            at += n;
            return at - n;
        };
        for (int m = 0; m < 3; ++m) T.car[m] = ownCarrier ? in(a.carrier[m], g.count(1 + m)) : velOut[m].p;
        for (int q = 0; q < cells; ++q) T.cin[q] = in(a.cellIn[q], nc);
        outAt = at - stage.p;
        for (int q = 0; q < cells; ++q) { T.cout[q] = at; at += nc; }
        for (int m = 0; m < 3 && vel; ++m) { T.vout[m] = at; at += g.count(1 + m); }
        hat = at;
    }
    if (correct) {
        AdvectTable H = T;           // the forward pass, aimed at the scratch: dense grids in the call's axis order, back to back
        float* at = hat;
        for (int q = 0; q < cells; ++q) { H.cout[q] = at; at += nc; }
        for (int m = 0; m < 3 && vel; ++m) { H.vout[m] = at; at += g.count(1 + m); }
        launchAdvect(H, total);
        correctAdvected(T, H, total, limiter);
        advectSchemeHost[0] = PS_ADVECT_MACCORMACK; advectSchemeHost[1] = limiter;
    } else {
        launchAdvect(T, total);
    }
    advectOrderHost = a.order;
    advectStepHost = T.r;
    registerAdvectionArrays();
    if (fromDevice) { releaseToCaller(caller); return; }
    const float* from = stage.p + outAt;
    for (int q = 0; q < cells; ++q) { HIP_CHECK(hipMemcpyAsync(a.cellOut[q], from, (size_t)g.count(0) * sizeof(float), hipMemcpyDeviceToHost, stream)); from += g.count(0); }
    for (int m = 0; m < 3 && vel; ++m) { HIP_CHECK(hipMemcpyAsync(a.velOut[m], from, (size_t)g.count(1 + m) * sizeof(float), hipMemcpyDeviceToHost, stream)); from += g.count(1 + m); }
    HIP_CHECK(hipStreamSynchronize(stream));
    stage.free();
    drainDeferred(true);
}

// the launch of both schemes: the counters cleared, one workgroup per block of samples of the advected grids
void ps_context::launchAdvect(const AdvectTable& T, int total) {
    HIP_CHECK(hipMemsetAsync(advectCounts.p, 0, ASLOTS * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_advect, dim3((unsigned)total), dim3(ABS), 0, stream, T);
}

void ps_context::registerAdvectionArrays() {
    const NamedArray list[] = {{"advection", hostArray(&advectOrderHost, 1, 4)}, {"advectionStep", hostArray(&advectStepHost, 1, 8)},
                               {"advectionCounts", ArrayInfo{advectCounts.p, ASLOTS, 4}}};   // clamped samples per grid, then the samples left alone
    setArrays(list, advectCounts.p != nullptr);
    // ... and of the last call with the MacCormack correction: the scheme and the limiter; values the limiter changed per grid, fallback samples per grid
    const NamedArray corrected[] = {{"advectionScheme", hostArray(advectSchemeHost, 2, 4)}, {"advectionCorrection", ArrayInfo{advectCorrection.p, 8, 4}}};
    setArrays(corrected, advectCorrection.p != nullptr);
}

bool ps_context::dropAdvection() {
    const bool had = advectCounts.p != nullptr;
    advectCounts.free(); advectCorrection.free(); advectScratch.free();
    advectOrderHost = 0; advectStepHost = 0.;
    advectSchemeHost[0] = advectSchemeHost[1] = 0;
    registerAdvectionArrays();
    return had;
}
