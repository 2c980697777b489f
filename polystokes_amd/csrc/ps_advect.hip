// Advection (ps_advect_fields, an extension): up to eight cell fields and the MAC velocity moved semi-Lagrangian by a face velocity, the
// context's written velocity or the caller's own (include/polystokes.h states the rule).
//   k_advect    one workgroup per 16 x 4 x 4 block of samples of one of the four grids (cells, faceX, faceY, faceZ), a thread per sample: the
//               carrier at the sample, at the midpoint with order 2, the departure point, and one trilinear gather per field from there
// One by-value table holds the four grids (the idiom of ps_extrapolate.hip and ps_shapes.hip), so one launch covers all of them.  Either
// axis order is a set of strides in the table (the context's own velocity is x fastest whatever the caller's arrays are); with z fastest
// the block lies 4 x 4 x 16, so that a wave's lanes still run along the caller's fast axis.  A sample reads the inputs and writes only itself, and the counts are integers: the result does not depend on the traversal.
#include <algorithm>
#include <cmath>

#include "ps_context.hpp"
#include "ps_setup_util.hpp"

using namespace ps;

namespace {

constexpr int ABS = 256;                    // threads per workgroup: four waves, one per slow layer of the block
constexpr int ABF = 16, ABM = 4, ABL = 4;   // samples of a block along the fast axis, y, and the slow axis
constexpr int ASLOTS = 5;                   // counters: clamped samples of the four grids, samples left alone
static_assert(ABF * ABM == 64 && ABF * ABM * ABL == ABS, "a wave per slow layer of the block");

struct AdvectTable {
    int3 d[4];                  // extents of grid g: cells, faceX, faceY, faceZ
    int64_t st[4][3];           // the stride of grid g along x, y, z in every array of the caller
    int64_t cs[3][3];           // ... of face grid a in the carrier: the caller's strides, or x fastest for the context's velocity
    int32_t nb[4][3];           // blocks of grid g along x, y, z
    int32_t first[5];           // the first workgroup of grid g; [4]: all of them (a grid that is not advected has none)
    const float* car[3];        // the carrier's face grids
    const float* cin[PS_ADVECT_MAX_CELL_FIELDS];
    float* cout[PS_ADVECT_MAX_CELL_FIELDS];
    float* vout[3];
    int32_t* counts;            // ASLOTS
    double r;                   // dt / dx
    int order, cells, zfast;
};

// Where the sampler of grid g reads for the point p: the first of the eight samples, the steps to the upper one per axis (0 in the last
// layer: h is clamped, not l), the fractions, and whether p left the grid.  Every index lies in 0 .. d - 1 whatever the finite p.
struct Taps {
    int64_t base;
    int32_t e[3];
    double f[3];
    bool clamped;
};

__device__ __forceinline__ Taps tapsAt(const int3 d, const int64_t* st, int face, const double* p) {
    const int dd[3] = {d.x, d.y, d.z};
    Taps t;
    t.base = 0;
    t.clamped = false;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const double s = p[m] - (m == face ? 0. : 0.5);
        const double top = (double)(dd[m] - 1);
        const double c = fmin(fmax(s, 0.), top);
        const int l = (int)floor(c);
        const int h = min(l + 1, dd[m] - 1);
        t.f[m] = c - (double)l;
        t.base += (int64_t)l * st[m];
        t.e[m] = (int32_t)((int64_t)(h - l) * st[m]);      // (0 or one stride: below 2^31 for the largest grid an upload takes)
        t.clamped = t.clamped || s < 0. || s > top;
    }
    return t;
}

__device__ __forceinline__ double gather(const float* __restrict__ F, const Taps& t) {
    const float* v = F + t.base;
    const int64_t ex = t.e[0], ey = t.e[1], ez = t.e[2];
    const double v000 = v[0], v100 = v[ex], v010 = v[ey], v110 = v[ey + ex];
    const double v001 = v[ez], v101 = v[ez + ex], v011 = v[ez + ey], v111 = v[ez + ey + ex];
    const double x00 = v000 + (v100 - v000) * t.f[0], x10 = v010 + (v110 - v010) * t.f[0];
    const double x01 = v001 + (v101 - v001) * t.f[0], x11 = v011 + (v111 - v011) * t.f[0];
    const double y0 = x00 + (x10 - x00) * t.f[1], y1 = x01 + (x11 - x01) * t.f[1];
    return y0 + (y1 - y0) * t.f[2];
}

// U(p): each component from its own face grid
__device__ __forceinline__ void carrierAt(const AdvectTable& T, const double* p, double* U) {
#pragma unroll
    for (int a = 0; a < 3; ++a) U[a] = gather(T.car[a], tapsAt(T.d[1 + a], T.cs[a], a, p));
}

// the stored value: a NaN as the one quiet NaN of the rule
__device__ __forceinline__ float stored(double v) { return v != v ? __uint_as_float(0x7fc00000u) : (float)v; }

// (amdgpu_waves_per_eu(6): 76 registers and six waves per SIMD instead of 82 and five; the call was 2.4 % quicker with it, profiles/advection.md)
__global__ __launch_bounds__(ABS) __attribute__((amdgpu_waves_per_eu(6))) void k_advect(AdvectTable T) {
    __shared__ int32_t bins[ASLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < ASLOTS) bins[tid] = 0;
    __syncthreads();
    const int wg = (int)blockIdx.x;
    int g = 0;
    while (g < 3 && wg >= T.first[g + 1]) ++g;      // (the same for the whole workgroup; a grid without workgroups is passed over)
    const int b = wg - T.first[g];
    const int nbx = T.nb[g][0], nby = T.nb[g][1];
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int lf = tid & (ABF - 1), lm = (tid >> 4) & (ABM - 1), ls = tid >> 6;
    const int i[3] = {T.zfast ? bx * ABL + ls : bx * ABF + lf, by * ABM + lm, T.zfast ? bz * ABF + lf : bz * ABL + ls};
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
        bool finite = true;
        if (T.order == 2) {
            const double half = 0.5 * T.r;
            double pm[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) { pm[m] = p0[m] - half * U[m]; finite = finite && isfinite(pm[m]); }
            if (finite) carrierAt(T, pm, U);
        }
        if (finite) {
#pragma unroll
            for (int m = 0; m < 3; ++m) { p1[m] = p0[m] - T.r * U[m]; finite = finite && isfinite(p1[m]); }
        }
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
// with the stream idle and the temporary released.
void ps_context::advectFields(const ps_advection& a, bool fromDevice, int layout, hipStream_t caller) {
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
    DevBuf<float> stage;         // the host form's temporary: the caller's carrier, the cell fields in, then every output
    int64_t outAt = 0;
    if (fromDevice) {
        waitForCaller(caller);
        for (int m = 0; m < 3; ++m) { T.car[m] = ownCarrier ? a.carrier[m] : velOut[m].p; T.vout[m] = a.velOut[m]; }
        for (int q = 0; q < cells; ++q) { T.cin[q] = a.cellIn[q]; T.cout[q] = a.cellOut[q]; }
    } else {
        const int64_t nc = g.count(0), nf = g.count(1) + g.count(2) + g.count(3);
        stage.alloc((size_t)((ownCarrier ? nf : 0) + 2 * cells * nc + (vel ? nf : 0)));
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
    }
    HIP_CHECK(hipMemsetAsync(advectCounts.p, 0, ASLOTS * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_advect, dim3((unsigned)total), dim3(ABS), 0, stream, T);
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

void ps_context::registerAdvectionArrays() {
    const NamedArray list[] = {{"advection", hostArray(&advectOrderHost, 1, 4)}, {"advectionStep", hostArray(&advectStepHost, 1, 8)},
                               {"advectionCounts", ArrayInfo{advectCounts.p, ASLOTS, 4}}};   // clamped samples per grid, then the samples left alone
    setArrays(list, advectCounts.p != nullptr);
}

bool ps_context::dropAdvection() {
    const bool had = advectCounts.p != nullptr;
    advectCounts.free();
    advectOrderHost = 0; advectStepHost = 0.;
    registerAdvectionArrays();
    return had;
}
