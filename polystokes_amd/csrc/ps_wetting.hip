// Contact angles (ps_set_contact_angle, ps_upload_contact_cosine_field; an extension): ahead of the curvature of ps_surface.hip the liquid
// SDF inside the solid is rewritten so that its slope along the wall normal is cos(theta).  Setup only, and only in a setup that computes
// the curvature with the angle or the cosine field set; nothing here runs per iteration.
//
// The rule (include/polystokes.h states it, tests/contact_angle_ref.py restates it): with D the solid depth (the collision SDF, positive
// inside the solid), the update set U holds the cells with 0 < D <= PS_CONTACT_ANGLE_SWEEPS dx.  A Jacobi sweep gives a cell of U the
// |G_a|-weighted mean of its upwind neighbours (one per axis, toward the wall: against grad D, central differences) minus dx cos |G|: a
// first-order upwind step of grad(phi) . grad(D) = -cos |grad D|.  PS_CONTACT_ANGLE_SWEEPS sweeps carry the liquid's values that deep into
// the solid.  Cells outside U never change.
//
// Launches: k_wet_mark copies the SDF into both Jacobi iterates, writes one flag byte per 16 x 4 x 4 block of cells that holds a cell of U
// and counts |U| (one ballot and at most one integer atomic per wave); then PS_CONTACT_ANGLE_SWEEPS launches of k_wet_sweep, whose
// workgroups return after reading a clear flag, so the cost beyond the marking pass follows the wall area.  No host round trip, no
// floating-point atomics: the result does not depend on the schedule.
#include "ps_context.hpp"

using namespace ps;

namespace {

constexpr int WBX = 16, WBY = 4, WBZ = 4;   // cells per workgroup: a wave is one z-layer of the block, 4 runs of 16 cells along x
constexpr int WBS = WBX * WBY * WBZ;
static_assert(WBS == 256 && WBX * WBY == 64, "a wave covers one z-layer of the block");
static_assert(PS_CONTACT_ANGLE_SWEEPS % 2 == 0, "an even number of sweeps ends in the first iterate");

__device__ inline int3 wetCell(int t) { return make_int3((int)blockIdx.x * WBX + (t & (WBX - 1)), (int)blockIdx.y * WBY + ((t >> 4) & (WBY - 1)), (int)blockIdx.z * WBZ + (t >> 6)); }
__device__ inline int64_t wetBlock() { return blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z); }

// c in U: D_c > 0 and (double)D_c <= band (a NaN is in neither)
__device__ inline bool inBand(float D, double band) { return D > 0.f && (double)D <= band; }

__global__ void __launch_bounds__(WBS) k_wet_mark(Grid g, const float* __restrict__ collision, int negate, double band, const float* __restrict__ phi,
                                                  float* __restrict__ p0, float* __restrict__ p1, uint8_t* __restrict__ flags, int32_t* __restrict__ count) {
    const int3 d = g.dims(0);
    const int3 q = wetCell(threadIdx.x);
    bool inU = false;
    if (!oob3(d, q.x, q.y, q.z)) {
        const int64_t c = lin3(d, q.x, q.y, q.z);
        const float D = negate ? -collision[c] : collision[c];
        inU = inBand(D, band);
        const float v = phi[c];
        p0[c] = v;
        p1[c] = v;
    }
    const unsigned long long m = __ballot(inU);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));
    const int any = __syncthreads_or(inU ? 1 : 0);
    if (threadIdx.x == 0) flags[wetBlock()] = any ? 1 : 0;
}

struct WetArgs {
    Grid g;
    const float* collision;
    int negate;
    double band, dx;               // band = PS_CONTACT_ANGLE_SWEEPS dx
    const float* cosC;             // the cosine field, or null: cosS everywhere
    double cosS;
    const uint8_t* flags;
};

// one Jacobi sweep: dst = the rule applied to src on the cells of U (the other cells hold the uploaded SDF in both iterates)
__global__ void __launch_bounds__(WBS) k_wet_sweep(WetArgs A, const float* __restrict__ src, float* __restrict__ dst) {
    if (!A.flags[wetBlock()]) return;
    const int3 d = A.g.dims(0);
    const int3 q = wetCell(threadIdx.x);
    if (oob3(d, q.x, q.y, q.z)) return;
    auto Dat = [&](int i, int j, int k) {   // indices clamped to the grid
        i = i < 0 ? 0 : (i >= d.x ? d.x - 1 : i);
        j = j < 0 ? 0 : (j >= d.y ? d.y - 1 : j);
        k = k < 0 ? 0 : (k >= d.z ? d.z - 1 : k);
        const float v = A.collision[lin3(d, i, j, k)];
        return A.negate ? -v : v;
    };
    if (!inBand(Dat(q.x, q.y, q.z), A.band)) return;
    const int64_t c = lin3(d, q.x, q.y, q.z);
    const double G[3] = {((double)Dat(q.x + 1, q.y, q.z) - (double)Dat(q.x - 1, q.y, q.z)) * 0.5,
                         ((double)Dat(q.x, q.y + 1, q.z) - (double)Dat(q.x, q.y - 1, q.z)) * 0.5,
                         ((double)Dat(q.x, q.y, q.z + 1) - (double)Dat(q.x, q.y, q.z - 1)) * 0.5};
    const double gn = sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2]);
    const int pos[3] = {q.x, q.y, q.z}, ext[3] = {d.x, d.y, d.z};
    const int64_t stride[3] = {1, d.x, (int64_t)d.x * d.y};
    double N = 0., W = 0.;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int step = 0;                                   // toward the wall: against the gradient of the depth
        if (G[a] > 0.) step = -1; else if (G[a] < 0.) step = 1;
        if (step == 0) continue;                        // (a zero or a NaN)
        const int u = pos[a] + step;
        if (u < 0 || u >= ext[a]) continue;
        const double w = fabs(G[a]);
        N += w * (double)src[c + step * stride[a]];
        W += w;
    }
    if (W == 0.) { dst[c] = src[c]; return; }
    const double cosT = A.cosC ? (double)A.cosC[c] : A.cosS;
    dst[c] = (float)((N - (A.dx * cosT) * gn) / W);
}

}  // namespace

void ps_context::registerWettingArrays() {
    const NamedArray list[] = {{"contactCosine", hostArray(&contactCosUsed, 1, 8)}, {"contactField", hostArray(&contactFieldUsed, 1, 4)},
                               {"contactCells", ArrayInfo{wetCount.p, 1, 4}}, {"surfaceWetted", ArrayInfo{wetPhi[0].p, g.count(0), 4}}};
    setArrays(list, contactRan && wetPhi[0].p);
}

bool ps_context::dropWetting() {
    const bool had = wetPhi[0].p || wetPhi[1].p || wetFlags.p || wetCount.p;
    wetPhi[0].free(); wetPhi[1].free(); wetFlags.free(); wetCount.free();
    contactRan = false;
    registerWettingArrays();   // (their buffers have gone)
    return had;
}

bool ps_context::dropContactCosine() {
    const bool had = contactCos.p != nullptr;
    contactCos.free();
    contactCosField = false;
    return had;
}

// Called by applySurfaceTension with curvature = this setup computes kappa.  Returns the SDF the curvature kernels read: the rewritten one
// when the rule runs, the uploaded one otherwise (then nothing is launched and the wet buffers are dropped: deferred frees).
const float* ps_context::applyContactAngle(bool curvature) {
    const bool scalar = contactDegSet >= 0.;
    contactDegUsed = -1.; contactCosUsed = 0.; contactFieldUsed = 0;
    if (!curvature || (!scalar && !contactCosField)) {
        dropWetting();
        return surface.p;
    }
    const int3 d = g.dims(0);
    const int64_t n = g.count(0);
    const dim3 grid((unsigned)gridFor(d.x, WBX), (unsigned)gridFor(d.y, WBY), (unsigned)gridFor(d.z, WBZ));
    wetPhi[0].alloc((size_t)n); wetPhi[1].alloc((size_t)n);
    wetFlags.alloc((size_t)grid.x * grid.y * grid.z);
    wetCount.alloc(1);
    HIP_CHECK(hipMemsetAsync(wetCount.p, 0, sizeof(int32_t), stream));
    WetArgs A;
    A.g = g; A.collision = collision.p; A.negate = P.negateCollision ? 1 : 0;
    A.band = (double)PS_CONTACT_ANGLE_SWEEPS * dx; A.dx = dx;
    A.cosC = contactCosField ? (const float*)contactCos.p : nullptr;
    A.cosS = scalar ? contactCosSet : 0.;
    A.flags = wetFlags.p;
    hipLaunchKernelGGL(k_wet_mark, grid, dim3(WBS), 0, stream, g, (const float*)collision.p, A.negate, A.band, (const float*)surface.p, wetPhi[0].p,
                       wetPhi[1].p, wetFlags.p, wetCount.p);
    for (int m = 0; m < PS_CONTACT_ANGLE_SWEEPS; ++m)   // sweep m + 1 reads iterate m & 1 and writes the other: the last one writes wetPhi[0]
        hipLaunchKernelGGL(k_wet_sweep, grid, dim3(WBS), 0, stream, A, (const float*)wetPhi[m & 1].p, wetPhi[(m & 1) ^ 1].p);
    contactRan = true;
    contactDegUsed = scalar ? contactDegSet : -1.;
    contactCosUsed = A.cosS;
    contactFieldUsed = contactCosField ? 1 : 0;
    return wetPhi[0].p;
}

// ps_upload_contact_cosine_field / _device (the ingest of ps_fields.hip).  A refused value drops the field.  Ends with the stream idle and
// everything dropped released.
std::string ps_context::uploadContactCosine(const float* cosTheta, bool fromDevice, int layout, hipStream_t caller) {
    std::string why;
    bool dropped = true;   // (an ingest: the scan words at least)
    if (!cosTheta) {
        dropped = dropContactCosine();
        if (contactDegSet < 0.) dropped |= dropWetting();   // nothing asks for the rule any more
    } else {
        const CellIn in = cellIn(cosTheta, contactCos, SCAN_BAD_OUTSIDE_UNIT, "contact cosine: ");
        why = ingestCellFields(&in, 1, fromDevice, layout, caller, false);
        if (why.empty()) contactCosField = true;
        else dropContactCosine();
    }
    releaseIdle(dropped);
    return why;
}
