// Collider shapes (ps_set_collider_shapes, ps_place_colliders, an extension): every collider's shape is a small SDF volume in the body's own
// frame, stored once; a table of rigid poses places all of them into the context's collision buffer and id field, right after an upload
// (include/polystokes.h states the rule).
//   k_place_shapes    one workgroup per 16 x 4 x 4 block of cells, a thread per cell: the union (largest solid depth) over the base value
//                     and every collider that reaches the cell, a rotated trilinear sample each, and the id of the winner
//   k_place_finish    the count of the cells left alone, from the total and the won cells
// All volumes live in one pool; one by-value table holds the grids (the idiom of ps_motions.hip).  The counts are integers and a cell
// reads and writes only itself: the result does not depend on the traversal.
#include <algorithm>
#include <cmath>

#include "ps_context.hpp"
#include "ps_setup_util.hpp"

using namespace ps;

namespace {

constexpr int SBS = 256;                    // threads per workgroup: four waves, one per z layer of the block
constexpr int SBX = 16, SBY = 4, SBZ = 4;   // cells of a block: a wave covers 16 x 4 cells of one layer, x fastest
constexpr int SP = 12;                      // doubles per pose: R[9] row-major (body to world), t[3]
static_assert(SBX * SBY == 64 && SBX * SBY * SBZ == SBS, "a wave per layer of the block");

struct ShapeTable {
    int3 d;                     // extents of the cell grid
    float* collision;           // the collision SDF, per cell: read and rewritten in place
    int32_t* ids;               // collider of every cell: rewritten where a collider wins
    const ShapeDesc* desc;      // count
    const float* pool;          // the volumes' samples
    const double* pose;         // SP * count
    int32_t* cells;             // count + 2: cells won per collider, cells left alone, colliders skipped (a pose that is not finite)
    double orig[3], dx;
    int negate, count, cull;
};

// The workgroup stages the poses and descriptors into LDS.  Wave 0 then decides, one lane per collider, whether the collider can reach the
// block at all: the block's centre goes through the collider's transform once, and the collider is out when the centre lies outside the
// volume's box by more than the reach plus the block's half extent along that sample axis (sum_m |R[m][a]| half_m: what the block's
// cells can differ from the centre by, for any R; an orthonormal R makes it at most the half diagonal) plus a margin for the rounding of
// either side.  The survivors are one 64-bit mask in LDS; every thread walks its set bits in rising order through scalar registers, so
// the loop and its trip count are the same for the whole workgroup, and a block no collider reaches ends without reading its cells.
// The per-cell test of the rule still decides every cell.
__global__ __launch_bounds__(SBS) void k_place_shapes(ShapeTable T) {
    __shared__ double pose[PS_COLLIDER_MAX * SP];
    __shared__ ShapeDesc desc[PS_COLLIDER_MAX];
    __shared__ int32_t bins[PS_COLLIDER_MAX];
    __shared__ double reachE[PS_COLLIDER_MAX];       // E of the rule, per collider
    __shared__ unsigned long long reach;
    const int tid = threadIdx.x, lane = tid & 63;
    const int count = T.count;
    for (int t = tid; t < count * SP; t += SBS) pose[t] = T.pose[t];
    for (int t = tid; t < count; t += SBS) desc[t] = T.desc[t];
    for (int t = tid; t < count; t += SBS) bins[t] = 0;
    __syncthreads();
    const int b[3] = {(int)blockIdx.x * SBX, (int)blockIdx.y * SBY, (int)blockIdx.z * SBZ};
    if (tid < 64) {
        bool ok = tid < count, finite = true;
        if (ok) {
            const double* P = pose + tid * SP;
            for (int q = 0; q < SP; ++q) finite = finite && isfinite(P[q]);
            ok = finite;
            reachE[tid] = (PS_COLLIDER_SHAPE_REACH * T.dx) / desc[tid].h;      // (the cells read it: one division per collider, not per cell)
        }
        if (ok && T.cull) {
            const double* P = pose + tid * SP;
            const ShapeDesc& S = desc[tid];
            const double half[3] = {0.5 * (SBX - 1), 0.5 * (SBY - 1), 0.5 * (SBZ - 1)};
            double r[3], dm[3], mag = 0.;
            for (int m = 0; m < 3; ++m) {
                r[m] = T.orig[m] + (((double)b[m] + half[m]) + 0.5) * T.dx;
                dm[m] = r[m] - P[9 + m];
                mag += fabs(r[m]) + fabs(P[9 + m]);
            }
            const double E = reachE[tid];
            for (int a = 0; a < 3; ++a) {
                const double q = (P[a] * dm[0] + P[3 + a] * dm[1]) + P[6 + a] * dm[2];
                const double s = (q - S.o[a]) / S.h - 0.5;
                const double ext = ((fabs(P[a]) * half[0] + fabs(P[3 + a]) * half[1] + fabs(P[6 + a]) * half[2]) * T.dx) / S.h;
                // the margin: 1e-12 of every magnitude that entered s here or enters it at a cell, in samples (their rounding is 2^-53 of it each)
                const double slack = E + ext * (1. + 1e-9) + 1e-12 * ((mag + fabs(S.o[a]) + 16. * T.dx) / S.h + (double)S.n[a] + 1.);
                if (s < -slack || s > (double)(S.n[a] - 1) + slack) ok = false;     // (a NaN compares false: the collider stays)
            }
        }
        const unsigned long long m = __ballot(ok);
        const unsigned long long skipped = __ballot(tid < count && !finite);
        if (tid == 0) {
            reach = m;
            if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && skipped) atomicAdd(&T.cells[count + 1], __popcll(skipped));
        }
    }
    __syncthreads();
    const unsigned long long mine = reach;
    unsigned long long todoK = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(mine >> 32)) << 32) |
                               (unsigned)__builtin_amdgcn_readfirstlane((int)(mine & 0xffffffffu));
    if (!todoK) return;      // no collider reaches the block (the same for every thread): its cells keep what they hold, unread
    const int i[3] = {b[0] + (tid & (SBX - 1)), b[1] + ((tid >> 4) & (SBY - 1)), b[2] + (tid >> 6)};
    const bool live = i[0] < T.d.x && i[1] < T.d.y && i[2] < T.d.z;
    const int64_t c = live ? lin3(T.d, i[0], i[1], i[2]) : 0;
    double best = 0.;
    int kbest = -1;
    if (live) { const double v = (double)T.collision[c]; best = T.negate ? -v : v; }
    double r[3];
    for (int m = 0; m < 3; ++m) r[m] = T.orig[m] + ((double)i[m] + 0.5) * T.dx;
    while (todoK) {
        const int k = __ffsll((long long)todoK) - 1;
        todoK &= todoK - 1;
        const double* P = pose + k * SP;
        const ShapeDesc& S = desc[k];
        const double dm[3] = {r[0] - P[9], r[1] - P[10], r[2] - P[11]};
        const double E = reachE[k];
        double s[3];
        bool part = live;
        for (int a = 0; a < 3; ++a) {
            const double q = (P[a] * dm[0] + P[3 + a] * dm[1]) + P[6 + a] * dm[2];
            s[a] = (q - S.o[a]) / S.h - 0.5;
            part = part && s[a] >= -E && s[a] <= (double)(S.n[a] - 1) + E;
        }
        if (!part) continue;
        int ia[3];
        double f[3], out[3];
        for (int a = 0; a < 3; ++a) {
            const double ca = fmin(fmax(s[a], 0.), (double)(S.n[a] - 1));
            ia[a] = min((int)floor(ca), S.n[a] - 2);
            f[a] = ca - (double)ia[a];
            out[a] = (s[a] - ca) * S.h;
        }
        // the eight samples: every index lies in 0 .. n - 1 (ia in 0 .. n - 2, the extents at least 2)
        const int64_t sy = S.n[0], sz = (int64_t)S.n[0] * S.n[1];
        const float* v = T.pool + S.off + (ia[0] + sy * ia[1] + sz * ia[2]);
        const double v000 = v[0], v100 = v[1], v010 = v[sy], v110 = v[sy + 1];
        const double v001 = v[sz], v101 = v[sz + 1], v011 = v[sz + sy], v111 = v[sz + sy + 1];
        const double x00 = v000 + (v100 - v000) * f[0], x10 = v010 + (v110 - v010) * f[0];
        const double x01 = v001 + (v101 - v001) * f[0], x11 = v011 + (v111 - v011) * f[0];
        const double y0 = x00 + (x10 - x00) * f[1], y1 = x01 + (x11 - x01) * f[1];
        const double val = y0 + (y1 - y0) * f[2];
        const double dist = sqrt((out[0] * out[0] + out[1] * out[1]) + out[2] * out[2]);
        const double Dk = (T.negate ? -val : val) - dist;
        if (Dk > best) { best = Dk; kbest = k; }
    }
    if (live && kbest >= 0) {
        T.collision[c] = (float)(T.negate ? -best : best);
        T.ids[c] = kbest;
    }
    // counting the won cells: waveBinAdd, and the workgroup adds its bins at the end.  The cells left alone are not counted here: one add
    // per workgroup to one address is a queue of its own (65 536 workgroups at 256^3 took 0.6 ms over it); k_place_finish takes them
    // from the total.
    waveBinAdd(bins, live && kbest >= 0, kbest, lane);
    __syncthreads();
    for (int t = tid; t < count; t += SBS)
        if (bins[t]) atomicAdd(&T.cells[t], bins[t]);
}

// the cells left alone: all that no collider won (one thread, after k_place_shapes on the same stream)
__global__ void k_place_finish(int32_t* cells, int count, int32_t total) {
    int32_t left = total;
    for (int k = 0; k < count; ++k) left -= cells[k];
    cells[count] = left;
}

}  // namespace

// ps_set_collider_shapes, after the ABI's refusals (count 0: drop).  The volumes go into one pool, back to back, and a descriptor per
// collider says where; both are copied before the call returns, and the call ends with the stream idle and the previous pair released.
void ps_context::setColliderShapes(const ps_collider_shape* shape, int count) {
    HIP_CHECK(hipSetDevice(device));
    const bool dropped = dropShapes();
    if (count > 0) {
        std::vector<ShapeDesc> desc((size_t)count);
        int64_t total = 0;
        for (int k = 0; k < count; ++k) {
            ShapeDesc& D = desc[(size_t)k];
            for (int a = 0; a < 3; ++a) { D.n[a] = shape[k].n[a]; D.o[a] = shape[k].orig[a]; }
            D.pad = 0; D.h = shape[k].h; D.off = total;
            total += (int64_t)D.n[0] * D.n[1] * D.n[2];
        }
        shapePool.alloc((size_t)total);
        shapeDesc.alloc((size_t)count);
        for (int k = 0; k < count; ++k) {
            const ShapeDesc& D = desc[(size_t)k];
            HIP_CHECK(hipMemcpyAsync(shapePool.p + D.off, shape[k].sdf, (size_t)D.n[0] * D.n[1] * D.n[2] * sizeof(float), hipMemcpyHostToDevice, stream));
        }
        HIP_CHECK(hipMemcpyAsync(shapeDesc.p, desc.data(), (size_t)count * sizeof(ShapeDesc), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));      // (desc is a local; the caller's volumes are its own again)
        shapesCount = count;
        registerShapeArrays();
    }
    releaseIdle(dropped);
}

void ps_context::registerShapeArrays() {
    const NamedArray list[] = {{"colliderShapes", hostArray(&shapesCount, 1, 4)}};
    setArrays(list, shapesCount > 0);
}

bool ps_context::dropShapes() {
    const bool had = shapePool.p != nullptr;
    shapePool.free(); shapeDesc.free();
    shapesCount = 0;
    registerShapeArrays();
    return had;
}

// ps_place_colliders / _device, after the ABI's refusals: the poses' ingest (ps_context::ingestColliderTable), the id field's creation where
// there is none, and one launch on the context's stream.  The host form ends with the stream idle; the device form synchronises the
// host only where it has something to release: a table of another size, or air-pocket labels.
void ps_context::placeColliders(const double* poses, int count, bool fromDevice, hipStream_t caller) {
    HIP_CHECK(hipSetDevice(device));
    bool dropped = dropAirPockets();                  // the labels described the solids this call moves (drops only defer: their order is free)
    dropped |= ingestColliderTable(placement, poses, count, SP, fromDevice, caller);
    if (!colliderIds.p) {            // no id field: one filled with -1, with the lifetime of an uploaded one (the loads and the paint see it)
        colliderIds.alloc((size_t)g.count(0));
        HIP_CHECK(hipMemsetAsync(colliderIds.p, 0xff, (size_t)g.count(0) * sizeof(int32_t), stream));
    }
    ShapeTable T{};
    T.d = g.dims(0);
    T.collision = collision.p; T.ids = colliderIds.p;
    T.desc = shapeDesc.p; T.pool = shapePool.p;
    T.pose = placement.table.p; T.cells = placement.counters.p;
    for (int a = 0; a < 3; ++a) T.orig[a] = orig[a];
    T.dx = dx; T.negate = P.negateCollision ? 1 : 0; T.count = count;
    // PS_DEBUG_SHAPE_CULL=0 (lab build, tests): no collider is skipped for a whole block, so that a test can show the cull changes nothing
    T.cull = envInt(PS_ENV_LOUD("PS_DEBUG_SHAPE_CULL"), 1) != 0 ? 1 : 0;
    const dim3 grid((unsigned)gridFor(T.d.x, SBX), (unsigned)gridFor(T.d.y, SBY), (unsigned)gridFor(T.d.z, SBZ));
    hipLaunchKernelGGL(k_place_shapes, grid, dim3(SBS), 0, stream, T);
    hipLaunchKernelGGL(k_place_finish, dim3(1), dim3(1), 0, stream, placement.counters.p, count, (int32_t)g.count(0));
    finishColliderTable(placement, count, fromDevice, dropped);
}

void ps_context::registerPlacementArrays() {
    const int64_t nc = placement.count;
    const NamedArray list[] = {{"colliderPlacement", hostArray(&placement.count, 1, 4)},
                               {"colliderPoseTable", ArrayInfo{placement.table.p, SP * nc, 8}},
                               {"colliderPlacedCells", ArrayInfo{placement.counters.p, nc + 2, 4}},   // cells per collider, cells left alone, colliders skipped
                               {"collisionField", ArrayInfo{collision.p, g.count(0), 4}}};         // the buffer the next setup reads
    const NamedArray idList[] = {{"colliderCellIds", ArrayInfo{colliderIds.p, g.count(0), 4}}};   // (ps_upload_collider_ids(NULL) after a call takes it away)
    setArrays(list, placement.count > 0);
    setArrays(idList, placement.count > 0 && colliderIds.p);
}
