// Velocity extrapolation (ps_set_velocity_extrapolation, an extension): the solved velocity carried from the valid faces into the faces
// around them, layer by layer, on the three face grids.  Nothing here runs with layers = 0.
//   k_extrap_init    L = 0 on valid faces (label neither UNSOLVED nor UNASSIGNED), -1 elsewhere; the sweep counters cleared
//   k_extrap_sweep   sweep k: a face with L == -1 and a 6-neighbour of 0 <= L < k takes the mean of those neighbours and L = k
// One by-value table holds the three face grids (the FieldTable idiom of ps_fields.hip), so a launch covers all axes: 1 + layers launches
// per written step, queued on the context's stream behind the write-back with no host synchronisation between them.
#include <algorithm>

#include "ps_context.hpp"

using namespace ps;

namespace {

constexpr int EBS = 256;     // threads per workgroup of both kernels

struct ExtrapTable {
    int3 d[3];                  // extents of the face grid of axis a
    float* vel[3];              // velOut: read on known faces, written on the faces a sweep assigns
    int8_t* L[3];               // the layer of every face (array "extrapolationLayerX" / Y / Z)
    const int32_t* lab[3];      // final face labels
};

__global__ __launch_bounds__(EBS) void k_extrap_init(ExtrapTable T, int32_t* __restrict__ counts) {
    const int a = blockIdx.y;
    if (a == 0 && blockIdx.x == 0 && threadIdx.x < PS_EXTRAPOLATION_MAX_LAYERS) counts[threadIdx.x] = 0;
    const int3 d = T.d[a];
    const int64_t c = (int64_t)blockIdx.x * EBS + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int l = T.lab[a][c];
    T.L[a][c] = (l == PS_UNSOLVED || l == PS_UNASSIGNED) ? (int8_t)-1 : (int8_t)0;
}

// Sweep k, in place on velOut and L, one thread per face.  A Jacobi sweep without a second buffer: a reader takes a neighbour only if
// 0 <= L < k, and every store of this launch writes L = k on a face whose L was -1 — a reader that races with the store sees -1 or k and
// rejects both.  The velocity of a face is written only together with that store, so the velocities a reader takes (faces with
// 0 <= L < k when the launch began) are written by nobody in this launch.  sum: fp64, the neighbours in the order -x, +x, -y, +y, -z, +z,
// from 0; the face takes the fp32 rounding of sum / count (the library is built with -ffp-contract=off: no fused or reordered step).
// counts[k - 1]: faces assigned, a wave's ballot and one atomicAdd per wave.
__global__ __launch_bounds__(EBS) void k_extrap_sweep(ExtrapTable T, int k, int32_t* __restrict__ counts) {
    const int a = blockIdx.y;
    const int3 d = T.d[a];
    float* vel = T.vel[a];
    int8_t* L = T.L[a];
    const int64_t sy = d.x, sz = (int64_t)d.x * d.y, n = sz * d.z;
    const int64_t c = (int64_t)blockIdx.x * EBS + threadIdx.x;
    bool assigned = false;
    if (c < n && L[c] < 0) {
        const int3 q = unlin3(d, c);
        double sum = 0.;
        int cnt = 0;
        auto take = [&](bool inside, int64_t f) {
            if (!inside) return;
            const int l = L[f];
            if (l >= 0 && l < k) { sum += (double)vel[f]; ++cnt; }
        };
        take(q.x > 0, c - 1);
        take(q.x + 1 < d.x, c + 1);
        take(q.y > 0, c - sy);
        take(q.y + 1 < d.y, c + sy);
        take(q.z > 0, c - sz);
        take(q.z + 1 < d.z, c + sz);
        if (cnt > 0) {
            vel[c] = (float)(sum / (double)cnt);
            L[c] = (int8_t)k;
            assigned = true;
        }
    }
    const unsigned long long m = __ballot(assigned);
    if ((threadIdx.x & 63) == 0 && m != 0ull) atomicAdd(&counts[k - 1], (int32_t)__popcll(m));
}

}  // namespace

// solveStage, after applySolutionToVelocity of a step whose velocity is written, inside the write-back bracket.  The layer buffers (1 B per
// face) and the PS_EXTRAPOLATION_MAX_LAYERS counters are allocated here on first use and kept until ps_set_velocity_extrapolation(ctx, 0).
void ps_context::extrapolateVelocity(int layers) {
    ExtrapTable T;
    int64_t most = 1;
    for (int a = 0; a < 3; ++a) {
        const int64_t n = g.count(1 + a);
        extrapLayer[a].alloc((size_t)n);
        T.d[a] = g.dims(1 + a); T.vel[a] = velOut[a].p; T.L[a] = extrapLayer[a].p; T.lab[a] = labels[1 + a].p;
        most = std::max(most, n);
    }
    extrapCounts.alloc(PS_EXTRAPOLATION_MAX_LAYERS);
    const dim3 grid((unsigned)gridFor(most, EBS), 3);
    hipLaunchKernelGGL(k_extrap_init, grid, dim3(EBS), 0, stream, T, extrapCounts.p);
    for (int k = 1; k <= layers; ++k) hipLaunchKernelGGL(k_extrap_sweep, grid, dim3(EBS), 0, stream, T, k, extrapCounts.p);
    extrapUsedHost = layers;
}

void ps_context::registerExtrapolationArrays() {
    const NamedArray list[] = {{"extrapolationLayerX", ArrayInfo{extrapLayer[0].p, g.count(1), 1}}, {"extrapolationLayerY", ArrayInfo{extrapLayer[1].p, g.count(2), 1}},
                               {"extrapolationLayerZ", ArrayInfo{extrapLayer[2].p, g.count(3), 1}},
                               {"extrapolationCounts", ArrayInfo{extrapCounts.p, extrapUsedHost, 4}}};   // faces assigned by each sweep, the three axes together
    setArrays(list, extrapUsedHost > 0 && extrapCounts.p);
}

// ps_set_velocity_extrapolation(ctx, 0): the layer buffers go with the setting, and their arrays ("velocityExtrapolation" keeps what the last step ran)
bool ps_context::dropExtrapolation() {
    const bool had = extrapCounts.p != nullptr;
    for (auto& b : extrapLayer) b.free();
    extrapCounts.free();
    registerExtrapolationArrays();
    return had;
}
