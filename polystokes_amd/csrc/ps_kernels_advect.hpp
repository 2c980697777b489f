// The sampler of the advection kernels, one copy for k_advect (ps_advect.hip) and k_advect_correct (ps_advect_correct.hip): the by-value
// table of the four grids, the taps of a point, the trilinear gather, the carrier, the trace of a sample and the stored value
// (include/polystokes.h states the rule).  Both kernels run one workgroup per 16 x 4 x 4 block of samples of one grid, a thread per sample.
#pragma once

#include "ps_context.hpp"
#include "ps_setup_util.hpp"

namespace ps {

constexpr int ABS = 256;                    // threads per workgroup: four waves, one per slow layer of the block
constexpr int ABF = 16, ABM = 4, ABL = 4;   // samples of a block along the fast axis, y, and the slow axis
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

// The departure rule from U0 = U(p0) with the step factor r (-r: the reverse trace of the correction, which shares U0): p1, or false
// when a coordinate of the midpoint or of p1 is not finite.
__device__ __forceinline__ bool traceFrom(const AdvectTable& T, const double* p0, const double* U0, double r, double* p1) {
    double U[3] = {U0[0], U0[1], U0[2]};
    bool finite = true;
    if (T.order == 2) {
        const double half = 0.5 * r;
        double pm[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) { pm[m] = p0[m] - half * U[m]; finite = finite && isfinite(pm[m]); }
        if (finite) carrierAt(T, pm, U);
    }
    if (finite) {
#pragma unroll
        for (int m = 0; m < 3; ++m) { p1[m] = p0[m] - r * U[m]; finite = finite && isfinite(p1[m]); }
    }
    return finite;
}

// the sample of a workgroup's thread: the grid of the workgroup and the sample's indices (the blocks lie 4 x 4 x 16 with z fastest)
__device__ __forceinline__ int sampleOf(const AdvectTable& T, int wg, int tid, int* i) {
    int g = 0;
    while (g < 3 && wg >= T.first[g + 1]) ++g;      // (the same for the whole workgroup; a grid without workgroups is passed over)
    const int b = wg - T.first[g];
    const int nbx = T.nb[g][0], nby = T.nb[g][1];
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int lf = tid & (ABF - 1), lm = (tid >> 4) & (ABM - 1), ls = tid >> 6;
    i[0] = T.zfast ? bx * ABL + ls : bx * ABF + lf;
    i[1] = by * ABM + lm;
    i[2] = T.zfast ? bz * ABF + lf : bz * ABL + ls;
    return g;
}

}  // namespace ps
