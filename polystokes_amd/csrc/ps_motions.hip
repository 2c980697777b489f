// Collider motions (ps_paint_collider_velocities, an extension): the rigid-body velocity v + w x (r - o) of the collider a face belongs to,
// painted into the context's collisionvel buffers right after an upload (include/polystokes.h states the rule).
//   k_paint_motions   one launch over the three face grids (blockIdx.y = axis): for each of its faces a thread picks the more solid of the
//                     face's two cells, takes that cell's collider, writes the velocity of the face centre and counts the face
// One by-value table holds the grids (the idiom of ps_extrapolate.hip).  The counts are integers: the result does not depend on the traversal.
#include <algorithm>
#include <cmath>

#include "ps_context.hpp"
#include "ps_setup_util.hpp"

using namespace ps;

namespace {

constexpr int MBS = 256;            // threads per workgroup: four waves
constexpr int MU = 4;               // faces per thread and step of the walk: a face costs three dependent loads, MU faces share the waits
constexpr int MMAXGRID = 2048;      // workgroups per face grid at most: the rest is a grid-stride walk
constexpr int MV = 9;               // doubles per collider: v[3], w[3], o[3]

struct MotionTable {
    int3 d;                     // extents of the cell grid
    int3 fd[3];                 // extents of the three face grids
    float* cvel[3];             // collisionvel, per face grid
    const float* collision;     // the collision SDF, per cell
    const int32_t* ids;         // collider of every cell; null: collider 0
    const double* motion;       // MV * count
    int32_t* faces;             // count + 2: painted faces per collider, faces of an id outside 0..count-1, faces of a non-finite motion
    double orig[3], dx;
    int negate, count;
};

// p + s in the mixed radix of the grid's extents: both hold digits below the extents (the last digit is open), one carry per digit
__device__ __forceinline__ int3 addDigits(int3 p, const int3 s, const int3 fd) {
    p.x += s.x;
    if (p.x >= fd.x) { p.x -= fd.x; ++p.y; }
    p.y += s.y;
    if (p.y >= fd.y) { p.y -= fd.y; ++p.z; }
    p.z += s.z;
    return p;
}

// A workgroup stages the motions and a finite flag per collider into LDS, then walks tiles of MBS * MU consecutive faces of face grid
// blockIdx.y, x fastest: tile blockIdx.x, + gridDim.x, ...; a thread takes the faces tid, tid + MBS, ... of a tile.  The walk keeps the
// face's three indices and adds the stride's three digits with carries: no division per face.  Counting: waveBinAdd per face, and the
// workgroup adds its bins to the global counters at the end, one atomic per slot that occurred.
__global__ __launch_bounds__(MBS) void k_paint_motions(MotionTable T) {
    __shared__ double mot[PS_COLLIDER_MAX * MV];
    __shared__ int32_t finite[PS_COLLIDER_MAX];
    __shared__ int32_t bins[PS_COLLIDER_MAX + 2];
    const int a = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int count = T.count;
    for (int t = tid; t < count * MV; t += MBS) mot[t] = T.motion[t];
    for (int t = tid; t < count + 2; t += MBS) bins[t] = 0;
    __syncthreads();
    for (int t = tid; t < count; t += MBS) {
        bool ok = true;
        for (int q = 0; q < MV; ++q) ok = ok && isfinite(mot[t * MV + q]);
        finite[t] = ok ? 1 : 0;
    }
    __syncthreads();
    const int3 fd = T.fd[a];
    const int64_t n = (int64_t)fd.x * fd.y * fd.z;
    const int na = comp(T.d, a);                                                         // cells along the axis: the face index runs 0..na
    const int64_t cs = a == 0 ? 1 : (a == 1 ? (int64_t)T.d.x : (int64_t)T.d.x * T.d.y);   // the cell stride along the axis
    const int a1 = a == 2 ? 0 : a + 1, a2 = a == 0 ? 2 : a - 1;
    const int64_t stride = (int64_t)gridDim.x * (MBS * MU);
    const int3 sd = unlin3(fd, stride);      // the digits of the workgroup's stride (sd.z may exceed fd.z: the walk then ends)
    const int3 td = unlin3(fd, MBS);         // ... and of the step from one of a thread's MU faces to the next
    int3 p = unlin3(fd, (int64_t)blockIdx.x * (MBS * MU) + tid);
    for (int64_t base = (int64_t)blockIdx.x * (MBS * MU); base < n; base += stride) {
        int3 q[MU];
        int64_t cU[MU];
        bool live[MU], both[MU];
        float vu[MU], vl[MU];
        int k[MU];
        // three rounds, each over the MU faces, so that the loads of a round are in flight together: the two SDF values, the id, the rest
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            q[u] = u == 0 ? p : addDigits(q[u - 1], td, fd);
            live[u] = base + u * MBS + tid < n;
            const int ia = comp(q[u], a);
            cU[u] = lin3(T.d, q[u].x, q[u].y, q[u].z);      // the upper cell shares the face's indices (read only where it exists)
            both[u] = live[u] && ia >= 1 && ia <= na - 1;
            vu[u] = vl[u] = 0.f;
            if (both[u]) { vu[u] = T.collision[cU[u]]; vl[u] = T.collision[cU[u] - cs]; }
        }
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            const float DU = T.negate ? -vu[u] : vu[u], DL = T.negate ? -vl[u] : vl[u];
            // the only cell at the border, else the more solid one; a tie or a NaN: the lower
            const bool upper = both[u] ? DU > DL : comp(q[u], a) == 0;
            k[u] = 0;
            if (live[u] && T.ids) k[u] = T.ids[upper ? cU[u] : cU[u] - cs];
        }
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            int slot = 0;
            if (live[u]) {
                if (k[u] < 0 || k[u] >= count) slot = count;
                else if (!finite[k[u]]) slot = count + 1;
                else {
                    slot = k[u];
                    const double* m = mot + k[u] * MV;
                    const int idx[3] = {q[u].x, q[u].y, q[u].z};
                    const double r1 = T.orig[a1] + ((double)idx[a1] + 0.5) * T.dx, r2 = T.orig[a2] + ((double)idx[a2] + 0.5) * T.dx;
                    const double arm1 = r1 - m[6 + a1], arm2 = r2 - m[6 + a2];      // (the arm along the axis itself does not enter)
                    T.cvel[a][base + u * MBS + tid] = (float)(m[a] + (m[3 + a1] * arm2 - m[3 + a2] * arm1));
                }
            }
            waveBinAdd(bins, live[u], slot, lane);
        }
        p = addDigits(p, sd, fd);
    }
    __syncthreads();
    for (int t = tid; t < count + 2; t += MBS)
        if (bins[t]) atomicAdd(&T.faces[t], bins[t]);
}

}  // namespace

// ps_paint_collider_velocities / _device, after the ABI's refusals: the table's ingest (ps_context::ingestColliderTable) and one launch on the
// context's stream.  The host form ends with the stream idle; the device form synchronises the host only where a table of another size
// was dropped.
void ps_context::paintColliderVelocities(const double* motion, int count, bool fromDevice, hipStream_t caller) {
    HIP_CHECK(hipSetDevice(device));
    const bool dropped = ingestColliderTable(motions, motion, count, MV, fromDevice, caller);
    MotionTable T{};
    T.d = g.dims(0);
    int64_t most = 1;
    for (int a = 0; a < 3; ++a) {
        T.fd[a] = g.dims(1 + a); T.cvel[a] = cvel[a].p; T.orig[a] = orig[a];
        most = std::max(most, g.count(1 + a));
    }
    T.collision = collision.p;
    T.ids = colliderIds.p;
    T.motion = motions.table.p; T.faces = motions.counters.p;
    T.dx = dx; T.negate = P.negateCollision ? 1 : 0; T.count = count;
    // PS_DEBUG_MOTION_GRID=<n> (lab build, tests): at most n workgroups per face grid, so that a small grid walks several tiles per workgroup
    const int cap = std::max(1, envInt(PS_ENV_LOUD("PS_DEBUG_MOTION_GRID"), MMAXGRID));
    const int perGrid = (int)std::min<int64_t>(cap, gridFor(most, MBS * MU));
    hipLaunchKernelGGL(k_paint_motions, dim3((unsigned)perGrid, 3), dim3(MBS), 0, stream, T);
    finishColliderTable(motions, count, fromDevice, dropped);
}

void ps_context::registerMotionArrays() {
    const int64_t nc = motions.count;
    const NamedArray list[] = {{"colliderMotions", hostArray(&motions.count, 1, 4)},
                               {"colliderMotionTable", ArrayInfo{motions.table.p, MV * nc, 8}},
                               {"colliderMotionFaces", ArrayInfo{motions.counters.p, nc + 2, 4}},     // painted faces per collider, then the two left-alone counts
                               {"collisionVelocityX", ArrayInfo{cvel[0].p, g.count(1), 4}},        // the buffers the next setup reads
                               {"collisionVelocityY", ArrayInfo{cvel[1].p, g.count(2), 4}},
                               {"collisionVelocityZ", ArrayInfo{cvel[2].p, g.count(3), 4}}};
    setArrays(list, motions.count > 0);
}
