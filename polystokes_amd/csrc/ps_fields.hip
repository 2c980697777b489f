// Device-resident fields (ps_*_device entry points, include/polystokes.h): the kernels that move a caller's GPU arrays into and out of the
// context's x-fastest buffers, and the scan that replaces the host loops over a cell field (fieldIsUniform, the density's finite check).
//   k_fields_copy     layout 0: every field of a call in one launch, 16-byte accesses where both ends allow them
//   k_fields_swap_xz  layout 1: the x <-> z transposition, per field and y-plane through a padded LDS tile; serves ingest and emit
//   k_field_scan      one pass over a cell field: differs from f[0] anywhere?  smallest index of a non-finite value
#include <cstring>

#include "ps_context.hpp"
#include "ps_setup_util.hpp"

using namespace ps;

namespace {

constexpr int FBS = 256;     // threads per workgroup of the three kernels
constexpr int TILE = 64;     // the swap's tile: one wave moves 64 consecutive floats (256 B) of the fast axis per access

__global__ __launch_bounds__(FBS) void k_fields_copy(FieldTable T) {
    const int q = blockIdx.y;
    const float* __restrict__ src = T.src[q];
    float* __restrict__ dst = T.dst[q];
    const int64_t n = (int64_t)T.fast[q] * T.mid[q] * T.slow[q];
    const int64_t t0 = (int64_t)blockIdx.x * FBS + threadIdx.x, step = (int64_t)gridDim.x * FBS;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const float4* __restrict__ s4 = (const float4*)src;
        float4* __restrict__ d4 = (float4*)dst;
        const int64_t n4 = n >> 2;
        for (int64_t i = t0; i < n4; i += step) d4[i] = s4[i];
        for (int64_t i = (n4 << 2) + t0; i < n; i += step) dst[i] = src[i];
    } else {
        for (int64_t i = t0; i < n; i += step) dst[i] = src[i];
    }
}

// src[f + F (j + M s)] -> dst[s + S (j + M f)] with F, M, S = T.fast, T.mid, T.slow of the field: the source's fast axis becomes the
// destination's slow one.  Ingest (z fastest -> x fastest): F = d2, S = d0; emit: F = d0, S = d2.  A work item is one 64 x 64 tile of
// one y-plane: the rows of the tile are read along f, written to the 64 x 65 LDS tile row by row (lane lx -> bank lx), and read back
// column by column (lane lx of column r -> word 65 lx + r, bank (lx + r) % 64), so both phases touch every bank once per wave.
__global__ __launch_bounds__(FBS) void k_fields_swap_xz(FieldTable T) {
    __shared__ float tile[TILE][TILE + 1];
    const int q = blockIdx.y;
    const float* __restrict__ src = T.src[q];
    float* __restrict__ dst = T.dst[q];
    const int F = T.fast[q], M = T.mid[q], S = T.slow[q];
    const int tilesF = (F + TILE - 1) / TILE, tilesS = (S + TILE - 1) / TILE;
    const int64_t tiles = (int64_t)tilesF * tilesS * M;
    const int lx = threadIdx.x & (TILE - 1), ly = threadIdx.x / TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tf = (int)(t % tilesF);
        const int64_t u = t / tilesF;
        const int ts = (int)(u % tilesS), j = (int)(u / tilesS);
        const int f0 = tf * TILE, s0 = ts * TILE;
        for (int r = ly; r < TILE; r += FBS / TILE) {
            const int f = f0 + lx, s = s0 + r;
            if (f < F && s < S) tile[r][lx] = src[f + (int64_t)F * (j + (int64_t)M * s)];
        }
        __syncthreads();
        for (int r = ly; r < TILE; r += FBS / TILE) {
            const int f = f0 + r, s = s0 + lx;
            if (f < F && s < S) dst[s + (int64_t)S * (j + (int64_t)M * f)] = tile[lx][r];
        }
        __syncthreads();   // the next tile of this workgroup overwrites the LDS tile
    }
}

// out[SCAN_BAD] = min(out[SCAN_BAD], smallest i with f[i] bad): not finite (badMode >= SCAN_BAD_NON_FINITE) or below 0
// (SCAN_BAD_NON_FINITE_OR_NEGATIVE; -0 is not) or outside [-1, 1] (SCAN_BAD_OUTSIDE_UNIT), out[SCAN_DIFFERS] |= some f[i] != f[0]
// (the comparison of fieldIsUniform: -0 == 0, a NaN differs from everything), out[SCAN_FIRST] = the bits of f[0]
__global__ __launch_bounds__(FBS) void k_field_scan(const float* __restrict__ f, int64_t n, int badMode, uint32_t* __restrict__ out) {
    const float v0 = f[0];
    bool differs = false;
    uint32_t bad = 0xffffffffu;
    for (int64_t i = (int64_t)blockIdx.x * FBS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FBS) {
        const float v = f[i];
        differs |= v != v0;
        const bool isBad = (badMode >= SCAN_BAD_NON_FINITE && (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) ||
                           (badMode == SCAN_BAD_NON_FINITE_OR_NEGATIVE && v < 0.f) ||
                           (badMode == SCAN_BAD_OUTSIDE_UNIT && !(v >= -1.f && v <= 1.f));
        if (isBad && (uint32_t)i < bad) bad = (uint32_t)i;
    }
    const bool any = __any(differs);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)bad, o, 64);
        bad = other < bad ? other : bad;
    }
    if ((threadIdx.x & 63) == 0) {
        if (any) atomicOr(&out[SCAN_DIFFERS], 1u);
        if (bad != 0xffffffffu) atomicMin(&out[SCAN_BAD], bad);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[SCAN_FIRST] = __float_as_uint(v0);
}

}  // namespace

namespace ps {

void launchFieldsCopy(const FieldTable& T, hipStream_t s) {
    if (T.count == 0) return;
    int64_t most = 1;
    for (int q = 0; q < T.count; ++q) most = std::max(most, T.entries(q));
    hipLaunchKernelGGL(k_fields_copy, dim3((unsigned)std::min<int64_t>(2048, gridFor((most + 3) / 4, FBS)), (unsigned)T.count), dim3(FBS), 0, s, T);
}

void launchFieldsSwapXZ(const FieldTable& T, hipStream_t s) {
    if (T.count == 0) return;
    int64_t most = 1;
    for (int q = 0; q < T.count; ++q)
        most = std::max(most, (int64_t)((T.fast[q] + TILE - 1) / TILE) * ((T.slow[q] + TILE - 1) / TILE) * T.mid[q]);
    hipLaunchKernelGGL(k_fields_swap_xz, dim3((unsigned)std::min<int64_t>(4096, most), (unsigned)T.count), dim3(FBS), 0, s, T);
}

// out: SCAN_WORDS device words; they are reset here, on the same stream
void launchFieldScan(const float* f, int64_t n, int bad, uint32_t* out, hipStream_t s) {
    static_assert(SCAN_BAD == 0 && SCAN_DIFFERS == 1 && SCAN_FIRST == 2 && SCAN_WORDS == 3, "the two resets below follow this order");
    HIP_CHECK(hipMemsetAsync(out + SCAN_BAD, 0xff, sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(out + SCAN_DIFFERS, 0, 2 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_field_scan, dim3((unsigned)std::min<int64_t>(1024, gridFor(n, FBS))), dim3(FBS), 0, s, f, n, bad, out);
}

}  // namespace ps

// ---- the host side of the device entry points (ps_context.hip holds the C ABI) -----------------------------------------------------

// A field the kernels will read or write `count` floats of: 4-byte aligned, device memory of this context's GPU (not host, pinned or
// managed memory, not another GPU's), inside one allocation up to its last float.  Nothing is read through the pointer.
std::string ps_context::checkDeviceField(const void* ptr, int64_t count, const char* name) const {
    const std::string who = std::string(name) + ": ";
    if ((uintptr_t)ptr & 3) return who + "the pointer is not 4-byte aligned";
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); return who + "the pointer is not device memory of the context's device"; }
    if (at.type != hipMemoryTypeDevice || at.isManaged || at.device != device) return who + "the pointer is not device memory of the context's device";
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)ptr) != hipSuccess) { (void)hipGetLastError(); return who + "the pointer is not device memory of the context's device"; }
    const uintptr_t end = (uintptr_t)base + size, need = (uintptr_t)ptr + (uintptr_t)count * sizeof(float);
    if (need > end) return who + "the allocation ends before the field does (" + std::to_string(count) + " floats needed)";
    return {};
}

const char* ps_context::layoutRefusal(int layout) { return (layout == 0 || layout == 1) ? nullptr : "layout must be 0 (x fastest) or 1 (z fastest)"; }

// every pointer of an upload that the ingest would read (the 14 weights only when all are given, as the host path uses them)
std::string ps_context::refuseFieldsIn(const ps_fields_in* in, int layout) const {
    if (const char* m = layoutRefusal(layout)) return m;
    if (!in || in->nx <= 0 || in->ny <= 0 || in->nz <= 0 || in->nx > 1022 || in->ny > 1022 || in->nz > 1022) return {};   // uploadCheck's errors
    if (const char* m = missingField(in)) return m;
    Grid gg{in->nx, in->ny, in->nz, 0};
    static const char* const velName[3] = {"vel[0]", "vel[1]", "vel[2]"}, * const cvName[3] = {"collisionvel[0]", "collisionvel[1]", "collisionvel[2]"};
    std::string why;
    for (int a = 0; a < 3 && why.empty(); ++a) {
        why = checkDeviceField(in->vel[a], gg.count(1 + a), velName[a]);
        if (why.empty() && in->collisionvel[a]) why = checkDeviceField(in->collisionvel[a], gg.count(1 + a), cvName[a]);
    }
    if (why.empty()) why = checkDeviceField(in->surface, gg.count(0), "surface");
    if (why.empty()) why = checkDeviceField(in->collision, gg.count(0), "collision");
    if (why.empty()) why = checkDeviceField(in->viscosity, gg.count(0), "viscosity");
    bool all = true;
    for (int w = 0; w < 14; ++w) if (!in->weights[w]) all = false;
    for (int w = 0; w < 14 && all && why.empty(); ++w) why = checkDeviceField(in->weights[w], gg.count(w % 7), "weights");
    return why;
}

void ps_context::waitForCaller(hipStream_t caller) {
    for (auto& e : fieldEv) if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(fieldEv[0], caller));
    HIP_CHECK(hipStreamWaitEvent(stream, fieldEv[0], 0));
}
void ps_context::releaseToCaller(hipStream_t caller) {
    for (auto& e : fieldEv) if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(fieldEv[1], stream));
    HIP_CHECK(hipStreamWaitEvent(caller, fieldEv[1], 0));
}

const uint32_t* ps_context::scanField(const float* f, int64_t n, int bad) {
    fieldScan.alloc(SCAN_WORDS);
    if (!pinnedScan) HIP_CHECK(hipHostMalloc((void**)&pinnedScan, SCAN_WORDS * sizeof(uint32_t), hipHostMallocDefault));
    launchFieldScan(f, n, bad, fieldScan.p, stream);
    HIP_CHECK(hipMemcpyAsync(pinnedScan, fieldScan.p, SCAN_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    return pinnedScan;
}

// What ingestHost does, from device arrays: the same buffers receive the same values; the viscosity's uniform flag comes from k_field_scan
// on the ingested image.  Ends, like the host ingest, with the stream synchronised: the inputs are consumed.
void ps_context::ingestDevice(const ps_fields_in* in, int layout, hipStream_t caller) {
    const int64_t nc = g.count(0);
    const bool zf = layout == 1;
    waitForCaller(caller);
    FieldTable T;
    surface.alloc((size_t)nc); collision.alloc((size_t)nc); viscosity.alloc((size_t)nc);
    T.add(in->surface, surface.p, g.dims(0), zf);
    T.add(in->collision, collision.p, g.dims(0), zf);
    T.add(in->viscosity, viscosity.p, g.dims(0), zf);
    for (int a = 0; a < 3; ++a) {
        const int64_t n = g.count(1 + a);
        vel[a].alloc((size_t)n); cvel[a].alloc((size_t)n);
        velOut[a].alloc((size_t)n); valid[a].alloc((size_t)n); faceRow[a].alloc((size_t)n);
        T.add(in->vel[a], vel[a].p, g.dims(1 + a), zf);
        if (in->collisionvel[a]) T.add(in->collisionvel[a], cvel[a].p, g.dims(1 + a), zf);
        else HIP_CHECK(hipMemsetAsync(cvel[a].p, 0, (size_t)n * sizeof(float), stream));
    }
    haveInputWeights = true;
    for (int w = 0; w < 14; ++w) if (!in->weights[w]) haveInputWeights = false;
    for (int s = 0; s < 7; ++s) {
        const int64_t n = g.count(s);
        liquidW[s].alloc((size_t)n); fluidW[s].alloc((size_t)n);
        labels[s].alloc((size_t)n); activeIdx[s].alloc((size_t)n); reducedIdx[s].alloc((size_t)n);
        if (haveInputWeights) {
            T.add(in->weights[s], liquidW[s].p, g.dims(s), zf);
            T.add(in->weights[7 + s], fluidW[s].p, g.dims(s), zf);
        }
    }
    for (int q = 0; q < 3; ++q) cellScratch[q].alloc((size_t)nc);
    counters.alloc(CTR_COUNT);
    moveFields(T, layout);
    const uint32_t* w = scanField(viscosity.p, nc, SCAN_BAD_NONE);
    std::memcpy(&viscUniformValue, &w[SCAN_FIRST], sizeof(float));
    viscUniform = !w[SCAN_DIFFERS] && std::isfinite(viscUniformValue);
}

void ps_context::upload(const ps_params* p, const ps_fields_in* in, int layout, hipStream_t caller) {
    uploadCheck(p, in);
    uploadReset(p, in);
    ingestDevice(in, layout, caller);
    uploadTail();
}

// ---- optional cell fields: one ingest, one check, one release (DESIGN.md "optional cell fields") ---------------------------------------

// Queued on our stream.  Device arrays: behind whatever the caller's stream holds so far, one launch for all fields (a z-fastest source
// is transposed on the way in); after a download the caller's stream waits for the copies (no host synchronisation).
void ps_context::moveCellFields(const CellIn* f, int count, bool in, bool fromDevice, int layout, hipStream_t caller) {
    HIP_CHECK(hipSetDevice(device));
    if (!fromDevice) {
        for (int q = 0; q < count; ++q)
            HIP_CHECK(hipMemcpyAsync(f[q].dst, f[q].src, (size_t)g.count(0) * 4, in ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, stream));
        return;
    }
    waitForCaller(caller);
    FieldTable T;
    for (int q = 0; q < count; ++q) T.add(static_cast<const float*>(f[q].src), static_cast<float*>(f[q].dst), g.dims(0), in && layout == 1);
    moveFields(T, layout);
    if (!in) releaseToCaller(caller);
}

// Every field reaches its x-fastest buffer first, then k_field_scan checks each image in list order, so the index of a refused value is
// the x-fastest one in either layout.  Ends with the stream synchronised: the inputs are consumed.
std::string ps_context::ingestCellFields(const CellIn* f, int count, bool fromDevice, int layout, hipStream_t caller, bool keepScanWords, ScanFacts* facts) {
    const bool ownScan = !fieldScan.p && !keepScanWords;   // the scan words this call allocates go with it: the fields cost their own buffers and nothing else
    moveCellFields(f, count, true, fromDevice, layout, caller);
    std::string why;
    bool scanned = false;
    for (int q = 0; q < count && why.empty(); ++q) {
        if (f[q].bad == SCAN_BAD_NONE) continue;
        const uint32_t* w = scanField(static_cast<const float*>(f[q].dst), g.count(0), f[q].bad);   // (ends synchronised)
        scanned = true;
        ScanFacts k;
        std::memcpy(&k.first, &w[SCAN_FIRST], sizeof(float));
        k.differs = w[SCAN_DIFFERS] != 0;
        k.bad = w[SCAN_BAD] == 0xffffffffu ? -1 : (int64_t)w[SCAN_BAD];
        if (k.bad >= 0) why = scanRefusal(f[q].label, f[q].bad, k.bad);
        if (facts) *facts = k;
    }
    if (!scanned) HIP_CHECK(hipStreamSynchronize(stream));
    if (ownScan) fieldScan.free();
    return why;
}

// The end of an entry point that dropped buffers.  DevBuf::free only moves memory to the deferred list, so the drops may come before the
// synchronisation; the drain must come after it (nothing queued still reads the buffers).  Nothing dropped: no synchronisation.
void ps_context::releaseIdle(bool dropped) {
    if (!dropped) return;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamSynchronize(stream));
    drainDeferred(true);
}

// ps_upload_density_field / _device.  A constant field (all values equal) runs the scalar path at its clamped value, as a constant
// viscosity skips the sampling (viscUniform); any other field is sampled per face by the setup kernels (ps_setup_util.hpp: FaceDensity,
// handed out by densSource).  The host form finds the three facts on the host and uploads nothing for a refused or constant field; the
// device form ingests first and takes them from k_field_scan on the x-fastest image (and keeps the scan words).  Returns the reason an
// input is refused (the field is then dropped), or an empty string.
std::string ps_context::uploadDensity(const float* field, bool fromDevice, int layout, hipStream_t caller) {
    static const char* const label = "ps_upload_density_field: ";
    densField = false;
    densFieldHost = 0;
    rho = rhoScalar;
    if (!field) return {};
    const double lo = P.mindensity, hi = P.maxdensity;
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo > 0.) || hi < lo)
        return std::string(label) + "mindensity must be positive and maxdensity at least mindensity, both finite";
    ScanFacts k;
    std::string why;
    if (fromDevice) {
        const CellIn in = cellIn(field, density, SCAN_BAD_NON_FINITE, label);
        why = ingestCellFields(&in, 1, true, layout, caller, true, &k);
    } else {
        const int64_t nc = g.count(0);
        for (int64_t i = 0; i < nc && k.bad < 0; ++i) if (!std::isfinite(field[i])) k.bad = i;
        k.differs = !fieldIsUniform(field, nc, &k.first);
        if (k.bad >= 0) why = scanRefusal(label, SCAN_BAD_NON_FINITE, k.bad);
    }
    if (!why.empty()) return why;
    densMin = lo; densMax = hi;
    if (!k.differs) {
        const double v = (double)k.first;
        rho = v < lo ? lo : (v > hi ? hi : v);
        return {};
    }
    if (!fromDevice) {
        const CellIn in = cellIn(field, density, SCAN_BAD_NONE, label);
        ingestCellFields(&in, 1, false, 0, nullptr, true);
    }
    densField = true;
    return {};
}

// ps_upload_surface_fields / _device: sigma is checked first; a refusal drops both fields.
void ps_context::registerSurfaceFieldArrays() {
    const NamedArray list[] = {{"surfaceGhostPressure", ArrayInfo{surfQ.p, g.count(0), 8}}};   // ("surfaceFields" keeps what the last setup used)
    setArrays(list, surfFieldsUsed != 0 && surfQ.p);
}
bool ps_context::dropSurfaceFields() {
    const bool had = surfSigma.p || surfPressure.p || surfQ.p;
    surfSigmaField = surfPressureField = false;
    surfSigma.free(); surfPressure.free(); surfQ.free();
    registerSurfaceFieldArrays();   // (its buffer has gone)
    return had;
}
std::string ps_context::uploadSurfaceFields(const ps_surface_fields* f, bool fromDevice, int layout, hipStream_t caller) {
    bool dropped = dropSurfaceFields();
    std::string why;
    CellIn in[2];
    int n = 0;
    if (f && f->sigma) in[n++] = cellIn(f->sigma, surfSigma, SCAN_BAD_NON_FINITE_OR_NEGATIVE, "sigma: ");
    if (f && f->pressure) in[n++] = cellIn(f->pressure, surfPressure, SCAN_BAD_NON_FINITE, "pressure: ");
    if (n > 0) {
        why = ingestCellFields(in, n, fromDevice, layout, caller, false);
        if (why.empty()) { surfSigmaField = f->sigma != nullptr; surfPressureField = f->pressure != nullptr; }
        else dropSurfaceFields();
        dropped = true;   // (the scan words at least)
    }
    releaseIdle(dropped);
    return why;
}

// vel / valid into the caller's device arrays: queued on our stream behind whatever the caller's stream holds so far (its earlier readers
// of these arrays), and the caller's stream then waits for the copies.  No host synchronisation.
void ps_context::downloadDevice(const ps_fields_out* out, int layout, hipStream_t caller) {
    HIP_CHECK(hipSetDevice(device));
    waitForCaller(caller);
    FieldTable T;
    for (int a = 0; a < 3; ++a) {
        if (out->vel[a]) T.add(velOut[a].p, out->vel[a], g.dims(1 + a), false);
        if (out->valid[a]) T.add(valid[a].p, out->valid[a], g.dims(1 + a), false);
    }
    moveFields(T, layout);
    releaseToCaller(caller);
}

// [p; tau] into the caller's device grids.  Layout 0: k_solution_scatter writes them in place; layout 1: into fieldScratch, back to back,
// then one swap.
void ps_context::downloadSolutionDevice(const ps_solution_out* out, int layout, hipStream_t caller) {
    HIP_CHECK(hipSetDevice(device));
    waitForCaller(caller);
    float* dst[7] = {out->pressure, out->tauDiag[0], out->tauDiag[1], out->tauDiag[2], out->tauEdge[0], out->tauEdge[1], out->tauEdge[2]};
    if (layout == 0) {
        for (int q = 0; q < 7; ++q) if (dst[q]) scatterSolution(dst[q], q, 1);
    } else {
        int64_t total = 0;
        for (int q = 0; q < 7; ++q) total += solutionGridCount(q);
        fieldScratch.alloc((size_t)total);
        scatterSolution(fieldScratch.p, 0, 7);
        FieldTable T;
        int64_t off = 0;
        for (int q = 0; q < 7; ++q) {
            if (dst[q]) T.add(fieldScratch.p + off, dst[q], g.dims(q < 4 ? 0 : q), false);
            off += solutionGridCount(q);
        }
        launchFieldsSwapXZ(T, stream);
    }
    releaseToCaller(caller);
}
