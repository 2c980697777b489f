// Air pockets (ps_label_air_pockets, an extension): the connected air regions of the uploaded grid, their volumes and open flags, and a
// pressure per pocket painted into the pressure member of the free-surface fields (include/polystokes.h states every rule).  The stage
// runs before the setup, reads the weights the setup will use and changes nothing the solve does.
//   k_pocket_init      core flag (the label is INT_MAX for a cell that is not core), label = x-fastest index, the six link bits
//   k_cc_local, k_cc_step (ps_kernels_cc.hpp, shared with the REDUCED regions)   the propagation, on a Grid whose order is linear
//   k_pocket_roots     1 where cc[c] == c; the exclusive scan of that array numbers the pockets by their smallest cell index
//   k_pocket_ids       the id of every core cell and of every skin cell
//   k_pocket_sums      units, cells and open per pocket with integer atomics: any order of additions gives the same bits
//   k_pocket_volume    units -> volume
//   k_pocket_pressure  (float)pressure[id] per cell, 0 without an id
#include <limits.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "ps_context.hpp"
#include "ps_setup_util.hpp"

using namespace ps;

namespace {

constexpr int BS = SETUP_BS;
constexpr int CC_BOX = 16;              // edge of the boxes k_cc_local closes in LDS (5 bytes per cell: 20 KB)
constexpr int SUM_MAX_BLOCKS = 1024;    // workgroups of k_pocket_sums at most: each walks one contiguous run of cells

#include "ps_kernels_cc.hpp"

struct PocketWeights {
    const float* lw;        // "centerLiquidWeights"
    const float* fw;        // "centerFluidWeights"
    const float* fwF[3];    // "faceX/Y/ZFluidWeights"
};

__device__ inline bool isCore(const PocketWeights& W, int64_t c) { return W.fw[c] > 0.f && W.lw[c] <= 0.5f; }

__global__ void __launch_bounds__(BS) k_pocket_init(Grid g, PocketWeights W, int32_t* __restrict__ cc, uint8_t* __restrict__ link) {
    const int3 d = g.dims(0);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int3 q = unlin3(d, c);
    const bool core = isCore(W, c);
    cc[c] = core ? (int32_t)c : INT_MAX;
    int m = 0;
    if (core) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int3 fd = g.dims(1 + a);
#pragma unroll
            for (int dir = 0; dir < 2; ++dir) {
                int3 nb = q;
                addc(nb, a, dir ? 1 : -1);
                if (oob3(d, nb.x, nb.y, nb.z)) continue;
                int3 f = q;
                addc(f, a, dir);
                if (!(W.fwF[a][lin3(fd, f.x, f.y, f.z)] > 0.f)) continue;
                if (!isCore(W, lin3(d, nb.x, nb.y, nb.z))) continue;
                m |= 1 << (2 * a + dir);
            }
        }
    }
    link[c] = (uint8_t)m;
}

__global__ void __launch_bounds__(BS) k_pocket_roots(const int32_t* __restrict__ cc, int32_t* __restrict__ root, int64_t n) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) root[c] = cc[c] == (int32_t)c ? 1 : 0;
}

// cc: the fix point (the smallest cell index of the cell's pocket, INT_MAX: not core); rank: the scanned root flags.  A skin cell reads core
// flags and liquid weights alone, which no thread of this launch writes.
__global__ void __launch_bounds__(BS) k_pocket_ids(Grid g, PocketWeights W, const int32_t* __restrict__ cc, const int32_t* __restrict__ rank,
                                                   int32_t* __restrict__ ids) {
    const int3 d = g.dims(0);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int mine = cc[c];
    int id = -1;
    if (mine != INT_MAX) {
        id = rank[mine];
    } else if (W.fw[c] > 0.f && W.lw[c] < 1.f) {
        const int3 q = unlin3(d, c);
        int best = INT_MAX;
        float bestLw = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int3 fd = g.dims(1 + a);
#pragma unroll
            for (int dir = 0; dir < 2; ++dir) {      // -x, +x, -y, +y, -z, +z: the strict comparison keeps the first of a tie
                int3 nb = q;
                addc(nb, a, dir ? 1 : -1);
                if (oob3(d, nb.x, nb.y, nb.z)) continue;
                const int64_t nl = lin3(d, nb.x, nb.y, nb.z);
                const int v = cc[nl];
                if (v == INT_MAX) continue;
                int3 f = q;
                addc(f, a, dir);
                if (!(W.fwF[a][lin3(fd, f.x, f.y, f.z)] > 0.f)) continue;
                const float l = W.lw[nl];
                if (best == INT_MAX || l < bestLw) { best = v; bestLw = l; }
            }
        }
        if (best != INT_MAX) id = rank[best];
    }
    ids[c] = id;
}

__device__ inline unsigned long long shflXor64(unsigned long long v, int o) {
    const int lo = __shfl_xor((int)(unsigned)v, o, 64), hi = __shfl_xor((int)(unsigned)(v >> 32), o, 64);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}

// what the lanes of a wave hold for the pocket `id` (the same in every lane): summed over the wave, one atomic per value from lane 0
__device__ inline void flushWave(int id, unsigned long long u, int cells, int open, unsigned long long* __restrict__ units,
                                 int32_t* __restrict__ cellsOut, int32_t* __restrict__ openOut) {
    if (id < 0) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        u += shflXor64(u, o);
        cells += __shfl_xor(cells, o, 64);
        open |= __shfl_xor(open, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (u) atomicAdd(&units[id], u);
        if (cells) atomicAdd(&cellsOut[id], cells);
        if (open) atomicOr(&openOut[id], 1);
    }
}

// Workgroup b walks the cells [b per, (b + 1) per) in tiles of BS; a wave sees 64 consecutive cells per tile.  In the scenes that matter
// nearly every air cell belongs to one or two large pockets: per-lane atomics would put millions of adds on one address, which a memory
// channel serves one after the other.  So a wave whose lanes with an id all hold the SAME id adds nothing to memory: every lane keeps its
// own running sums for that id in registers, across tiles, and the wave reduces and issues its three atomics when the id changes and at
// the end of its run — a few thousand atomics for a grid of one pocket, whatever its size.  A wave whose lanes hold different ids (the
// borders between pockets, a foam of small ones) falls back to one atomic per lane for that tile.  The sums are integers: the order of
// the additions does not show in the result.
__global__ void __launch_bounds__(BS) k_pocket_sums(Grid g, PocketWeights W, const int32_t* __restrict__ cc, const int32_t* __restrict__ ids,
                                                    int64_t per, unsigned long long* __restrict__ units, int32_t* __restrict__ cellsOut,
                                                    int32_t* __restrict__ openOut) {
    const int3 d = g.dims(0);
    const int64_t n = (int64_t)d.x * d.y * d.z;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    int cur = -1, accCells = 0, accOpen = 0;
    unsigned long long accU = 0ull;
    for (int64_t base = lo; base < hi; base += BS) {      // (per is a multiple of BS: every wave of the workgroup runs the same trips)
        const int64_t c = base + threadIdx.x;
        int id = -1, core = 0, open = 0;
        unsigned long long u = 0ull;
        if (c < hi) {
            id = ids[c];
            if (id >= 0) {
                u = (unsigned long long)llrint((double)W.fw[c] * (1.0 - (double)W.lw[c]) * 1048576.0);
                if (cc[c] != INT_MAX) {
                    const int3 q = unlin3(d, c);
                    core = 1;
                    open = (q.x == 0 || q.x == d.x - 1 || q.y == 0 || q.y == d.y - 1 || q.z == 0 || q.z == d.z - 1) ? 1 : 0;
                }
            }
        }
        const bool has = id >= 0;
        const unsigned long long m = __ballot(has);
        if (!m) continue;
#ifdef PS_POCKETS_PLAIN_ATOMICS      // A/B build (scripts/air_pockets_ab.py --build-plain, profiles/air_pockets.md): every lane its own atomics
        const bool uniform = false;
        const int first = -1;
#else
        const int first = __shfl(id, __ffsll((long long)m) - 1, 64);
        const bool uniform = __ballot(has && id != first) == 0ull;
#endif
        if (uniform) {
            if (first != cur) {
                flushWave(cur, accU, accCells, accOpen, units, cellsOut, openOut);
                cur = first; accU = 0ull; accCells = 0; accOpen = 0;
            }
            if (has) { accU += u; accCells += core; accOpen |= open; }
        } else if (has) {
            if (u) atomicAdd(&units[id], u);
            if (core) atomicAdd(&cellsOut[id], 1);
            if (open) atomicOr(&openOut[id], 1);
        }
    }
    flushWave(cur, accU, accCells, accOpen, units, cellsOut, openOut);
}

__global__ void __launch_bounds__(BS) k_pocket_volume(const long long* __restrict__ units, double dx3, double* __restrict__ volume, int K) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) volume[k] = ((double)units[k] * (1.0 / 1048576.0)) * dx3;
}

__global__ void __launch_bounds__(BS) k_pocket_pressure(const int32_t* __restrict__ ids, const double* __restrict__ table, float* __restrict__ out, int64_t n) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int id = ids[c];
    out[c] = id >= 0 ? (float)table[id] : 0.f;
}

}  // namespace

bool ps_context::dropAirPockets() {
    const bool had = pocketsHave || pocketIds.p != nullptr;
    pocketsHave = false;
    pocketCount = 0;
    pocketIds.free(); pocketCells.free(); pocketOpen.free(); pocketUnits.free(); pocketVolume.free();
    registerPocketArrays();
    return had;
}

void ps_context::registerPocketArrays() {
    const int64_t K = pocketCount;
    const NamedArray list[] = {{"airPockets", hostArray(&pocketCount, 1, 4)},
                               {"airPocketPasses", hostArray(&pocketPassesHost, 1, 4)},    // global propagation passes of the last call (one host round trip each)
                               {"airPocketIds", ArrayInfo{pocketIds.p, g.count(0), 4}}, {"airPocketUnits", ArrayInfo{pocketUnits.p, K, 8}},
                               {"airPocketCells", ArrayInfo{pocketCells.p, K, 4}}, {"airPocketOpen", ArrayInfo{pocketOpen.p, K, 4}},
                               {"airPocketVolume", ArrayInfo{pocketVolume.p, K, 8}}};
    setArrays(list, pocketsHave);
}

// After an upload of a single domain.  Runs the weight stage itself (the setup repeats it on the same inputs: the same bits), then labels in
// the cell scratch of the setup: cellScratch[0] the labels, [2] the link bytes, [1] the root flags and their scan.  One host round trip per
// global pass, one for the scan's total, one at the end; ends with the stream idle and everything dropped released.
void ps_context::labelAirPockets() {
    if (slabEnabled || inGroup) throw Error("air pockets need a single domain");
    HIP_CHECK(hipSetDevice(device));
    pocketsHave = false;
    registerPocketArrays();
    buildIntegrationWeightsAlt();
    Grid gl = g;
    gl.order = PS_ORDER_LINEAR;      // labels are x-fastest cell indices whatever indexOrder is: k_cc_step's pointer jump resolves them through g.order
    const int64_t n = g.count(0);
    const dim3 gr(gridFor(n, BS)), bl(BS);
    PocketWeights W{liquidW[0].p, fluidW[0].p, {fluidW[1].p, fluidW[2].p, fluidW[3].p}};
    int32_t* cc = cellScratch[0].p;
    int32_t* root = cellScratch[1].p;
    uint8_t* link = (uint8_t*)cellScratch[2].p;
    hipLaunchKernelGGL(k_pocket_init, gr, bl, 0, stream, gl, W, cc, link);
    const int B = CC_BOX;
    hipLaunchKernelGGL(k_cc_local, dim3((g.nx + B - 1) / B, (g.ny + B - 1) / B, (g.nz + B - 1) / B), dim3(256), (size_t)B * B * B * 5, stream, gl, B,
                       (const uint8_t*)link, cc);
    int passes = 0;
    for (int guard = 0; guard < 100000; ++guard) {      // a pocket that winds through many boxes needs several passes
        zeroChangeFlags();
        for (int it = 0; it < (guard == 0 ? 1 : 4); ++it)
            hipLaunchKernelGGL(k_cc_step, gr, bl, 0, stream, gl, (const uint8_t*)link, cc, counters.p + CTR_CHANGED);
        ++passes;
        if (!readCounter(CTR_CHANGED)) break;
    }
    pocketPassesHost = passes;
    hipLaunchKernelGGL(k_pocket_roots, gr, bl, 0, stream, (const int32_t*)cc, root, n);
    const int64_t K = exclusiveScanI32(root, n);
    pocketIds.alloc((size_t)n);
    pocketUnits.alloc((size_t)K); pocketCells.alloc((size_t)K); pocketOpen.alloc((size_t)K); pocketVolume.alloc((size_t)K);
    HIP_CHECK(hipMemsetAsync(pocketUnits.p, 0, (size_t)std::max<int64_t>(K, 1) * sizeof(long long), stream));
    HIP_CHECK(hipMemsetAsync(pocketCells.p, 0, (size_t)std::max<int64_t>(K, 1) * sizeof(int32_t), stream));
    HIP_CHECK(hipMemsetAsync(pocketOpen.p, 0, (size_t)std::max<int64_t>(K, 1) * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_pocket_ids, gr, bl, 0, stream, gl, W, (const int32_t*)cc, (const int32_t*)root, pocketIds.p);
    if (K > 0) {
        const int64_t tiles = gridFor(n, BS);
        const int blocks = (int)std::min<int64_t>(SUM_MAX_BLOCKS, tiles);
        const int64_t per = ((tiles + blocks - 1) / blocks) * BS;
        hipLaunchKernelGGL(k_pocket_sums, dim3((unsigned)blocks), bl, 0, stream, gl, W, (const int32_t*)cc, (const int32_t*)pocketIds.p, per,
                           (unsigned long long*)pocketUnits.p, pocketCells.p, pocketOpen.p);
        hipLaunchKernelGGL(k_pocket_volume, dim3((unsigned)gridFor(K, BS)), bl, 0, stream, (const long long*)pocketUnits.p, (dx * dx) * dx, pocketVolume.p, (int)K);
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    pocketCount = (int32_t)K;
    pocketsHave = true;
    registerPocketArrays();
    drainDeferred(true);
}

void ps_context::copyAirPockets(double* volume, int32_t* open, int64_t len) {
    if (!pocketsHave) throw Error("ps_get_air_pockets: there are no air pocket labels (ps_label_air_pockets after the last upload)");
    const int64_t K = pocketCount;
    if (len < K) throw Error("ps_get_air_pockets: len is below the pocket count " + std::to_string(K));
    if (K == 0) return;
    HIP_CHECK(hipSetDevice(device));
    if (volume) HIP_CHECK(hipMemcpyAsync(volume, pocketVolume.p, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (open) HIP_CHECK(hipMemcpyAsync(open, pocketOpen.p, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

// Host: a copy and a synchronisation.  Device: queued on our stream behind what the caller's stream holds, and the caller's stream then
// waits for it (a download: no host synchronisation); the ingest kernels move 4-byte words whatever they hold.
void ps_context::copyAirPocketIds(int32_t* dst, bool toDevice, int layout, hipStream_t caller) {
    if (!pocketsHave) throw Error("ps_download_air_pocket_ids: there are no air pocket labels (ps_label_air_pockets after the last upload)");
    const CellIn out{pocketIds.p, dst, SCAN_BAD_NONE, ""};
    moveCellFields(&out, 1, false, toDevice, layout, caller);
    if (!toDevice) HIP_CHECK(hipStreamSynchronize(stream));
}

// The pressure member of the free-surface fields from a value per pocket: what ps_upload_surface_fields_device installs for the same
// array, except that a sigma field stays.  Returns the refusal (nothing changed), or empty.
std::string ps_context::setAirPocketPressures(const double* pressure, int64_t len) {
    if (!pocketsHave) throw Error("ps_set_air_pocket_pressures: there are no air pocket labels (ps_label_air_pockets after the last upload)");
    HIP_CHECK(hipSetDevice(device));
    if (!pressure) {      // the pressure member alone goes; without a sigma field nothing of the fields is left
        bool dropped = surfPressure.p != nullptr;
        surfPressureField = false;
        surfPressure.free();
        if (!surfSigmaField) dropped |= dropSurfaceFields();
        releaseIdle(dropped);
        return {};
    }
    const int64_t K = pocketCount;
    if (len != K) return "len must equal the pocket count " + std::to_string(K);
    for (int64_t k = 0; k < K; ++k)      // as the field holds it: a double beyond the range of fp32 would paint an infinity, which the uploads refuse
        if (!std::isfinite((float)pressure[k])) return "pressure of pocket " + std::to_string(k) + " is not finite";
    const int64_t n = g.count(0);
    DevBuf<double> table;
    table.alloc((size_t)K);
    if (K > 0) HIP_CHECK(hipMemcpyAsync(table.p, pressure, (size_t)K * sizeof(double), hipMemcpyHostToDevice, stream));
    surfPressure.alloc((size_t)n);
    hipLaunchKernelGGL(k_pocket_pressure, dim3(gridFor(n, BS)), dim3(BS), 0, stream, (const int32_t*)pocketIds.p, (const double*)table.p, surfPressure.p, n);
    surfPressureField = true;
    table.free();      // (deferred: released below, once the kernel that reads it has run)
    releaseIdle(true);
    return {};
}
