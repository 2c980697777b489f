// The host-side mirror of the reference's `HDK_PolyStokes::Solver` (exec/HDK_PolyStokesSolver.h:27-375):
// same stage methods, same state, but every field lives in HBM and every stage is a HIP kernel launch.
#pragma once
#include <map>
#include <memory>

#include "ps_common.hpp"

namespace ps {

struct DevCSR {
    int64_t rows = 0, cols = 0, nnz = 0;
    DevBuf<int32_t> ptr;   // rows+1 (nnz < 2^31 is enforced)
    DevBuf<int32_t> col;
    DevBuf<double> val;
    // Lossless value coding: every stencil value is code * scale with an integer |code| <= 127 whenever the volume
    // fractions are multiples of 1/8 (the 2x2x2 sampler): val = +-(wF*wL)/dx = +-(8wF * 8wL) * (1/(64 dx)).
    // The fill kernels verify code*scale == val bit for bit; if any entry fails, the SpMV streams `val` instead.
    DevBuf<int8_t> code;
    bool packed = false;
    // Compressed stream of the persistent SpMV kernels (with `packed`, or with val4; only if EVERY chunk fits: col16ok).
    // A chunk = up to 256 consecutive rows [chunkInfo.z, chunkInfo.z + chunkInfo.w) and a 4-entry-aligned run [chunkInfo.x,
    // chunkInfo.y) of (col16, code4) entries in CSR order; col = winBase[chunk*16 + (c16 >> 12)] + (c16 & 4095) (up to 16 windows
    // of 4096 columns per chunk); len8 = entries per row.  nv = ceil(fullest chunk / 1024) = 4-entry groups per lane.
    // Chunks start at the boundaries of the numbering's lattice blocks (and of the tiles' skin-row ranges): equivalent blocks then
    // produce byte-identical runs, and a chunk whose run equals an earlier chunk's points at THAT run (ps_blocks.hip:
    // dedupChunks) — a periodic tile structure streams one copy of each distinct run, from cache.
    DevBuf<uint16_t> col16;
    DevBuf<int8_t> code4;
    DevBuf<double> val4;         // the fp64 values in the same aligned chunk layout (only when the values are not coded)
    DevBuf<int32_t> winBase;
    DevBuf<int4> chunkInfo;      // (run begin, entries | rows << 16, first row, first row of the run's owner) — ps_kernels_spmv.hpp:Chunk
    DevBuf<uint8_t> len8;
    DevBuf<int32_t> chunkRep;    // the chunk whose run a chunk points at (itself unless shared)
    int nChunks = 0;
    int64_t uniqueLen = 0;       // entries of the runs some chunk actually points at (== streamLen without sharing)
    bool col16ok = false;
    int nv = 2;
    int64_t streamLen = 0;       // entries of col16 / code4 (multiple of 4)
    // Row-per-lane form of the same stream (coded values only; ps_blocks.hip:buildEll, ps_kernels_spmv.hpp:k_spmv_*_ell).  A chunk's
    // rows are cut into four units of 64 consecutive rows, one per wave; a unit is padded to the width W (even, <= 8) of its longest
    // row and stored lane-major: lane l of the unit finds its row's W windowed 16-bit columns at ecol[unitBegin + l*W ..] and its W
    // value codes (padded to 4 or 8 bytes) at ecode[...].  Gather instruction k of a wave then covers entry k of 64 CONSECUTIVE rows:
    // the lanes of a quad address neighbouring columns, which the CU's L1 pipeline serves per distinct line, not per lane
    // (profiles/r03_spmv_issue.md).  Each lane keeps its row's sum in a register: no LDS round trip, no row-length scan, no barrier.
    // echunk: (col begin [u16 units], code begin [bytes], first row, rows | W0 << 12 | W1 << 16 | W2 << 20 | W3 << 24).
    DevBuf<uint16_t> ecol;
    DevBuf<int8_t> ecode;
    DevBuf<int4> echunk;         // (the 16 window bases per chunk are winBase: same greedy cover, same columns)
    bool ellok = false;
    int64_t ellCols = 0, ellCodes = 0;     // sizes of ecol (u16 units) / ecode (bytes)
    int64_t ellUniqueCols = 0;             // u16 units of the runs some chunk actually points at (== ellCols without sharing)
};

// device-resident CG scalars (no host round trip inside the iteration)
struct CGScalars {
    double rsold, pAp, alpha, beta, rr, xx, rz, rre;
    int iter;        // index of the iteration that converged (pcg.h:322-325)
    int done;        // 1 once the stop rule fired (or rsold == 0)
    int maxit;
    int pend;        // the stop test of iteration `pendIter` waits for ||x||^2 of the x it updated (deferred-x step)
    double tol2;
    int pendIter;
    int vecNT;       // 1: the vector kernels use non-temporal loads / stores (ps_context::ntLevel() == 2)
    double rsold2[2];   // r.z of the previous iteration, double-buffered by iteration parity (fused-scalar step kernels)
    // a pass of the mixed-precision solve (k_cg_scal0_pass writes them, stopTest<true> reads them; the fp64 kernels touch neither): the pass
    // also ends at r.r < rrFloor, and with xxFix > 0 its stop test takes x.x = xxFix (the fp64 x at the pass's start) instead of the running sum
    double rrFloor, xxFix;
};

struct ArrayInfo {
    const void* dptr;
    int64_t count;
    int elem;
    const int32_t* perm = nullptr;   // optional: out[i] = src[perm[permOffset + i]] (reference order view)
    int64_t permOffset = 0;
    bool host = false;               // dptr is host memory of the context (no device copy behind it)
};
inline ArrayInfo hostArray(const void* p, int64_t count, int elem) { ArrayInfo a{p, count, elem}; a.host = true; return a; }
// One entry of a feature's array list (ps_context::setArrays): the feature's register...Arrays() holds the one list of its names, and
// registers or erases by it
struct NamedArray { const char* name; ArrayInfo info; };
struct AdvectTable;                  // ps_kernels_advect.hpp: the by-value table of the advection kernels
// What a call with a small table of doubles per collider keeps (ps_context::ingestColliderTable): the feature's register...Arrays(), the
// table the kernel read, count + 2 counters, the count of the last call
struct ColliderTable { void (::ps_context::*reg)(); DevBuf<double> table; DevBuf<int32_t> counters; int32_t count = 0; };

// The slots of ps_context::counters (int32 each): flags and totals that kernels write and the host reads (readCounter / fetchCounters).
// Every user clears its own slot before the launch; slots that one fetch reads are adjacent (asserted below).
enum Counter : int {
    CTR_CHANGED = 0,         // k_cc_step: a component label changed; k_fix_eval: a fix flag changed (zeroChangeFlags clears both)
    CTR_ANY_FIX = 1,         // k_fix_eval: the sweep holds a fix
    CTR_SCAN_TOTAL = 8,      // k_scan_single: the total of a synchronising scan (exclusiveScanI32, orderedIndexAssign, interleavedIndexAssignEx)
    CTR_IL_PROBE = 10,       // k_il_assign: the running prefix at the two probe positions (10, 11), fetched with CTR_SCAN_TOTAL
    CTR_CODE_FAIL = 20,      // encodeVal (k_S_fill, k_St_cells, k_St_edges): a stencil value is not code * valScale
    CTR_COL16_FAIL_S = 22,   // k_col16_build on S: a chunk needs more than 16 column windows
    CTR_COL16_FAIL_ST = 23,  // ... on St
    CTR_CHUNK_MAX = 25,      // k_chunk_len4: entries of the fullest chunk
    CTR_DICT_OVERFLOW = 26,  // k_dict_build: a diagonal takes more than 256 values
    CTR_NOT_DYADIC = 40,     // k_dyadic_check: a weight is not a multiple of 1/8
    CTR_HALO_UNMARKED = 41,  // k_count_unmarked_halo (ps_dist.hpp: decideExchangeMode)
    CTR_ACTIVE_TOTAL = 48,   // k_scan_single: the active samples of the seven grids (48 .. 54: constructActiveIndices)
    CTR_ELL_TOO_LONG = 55,   // k_ell_plan: a row is longer than the row-per-lane form holds
    CTR_ELL_COLS = 56,       // k_scan_single: column slots of the row-per-lane form (buildEll)
    CTR_ELL_CODES = 57,      // ... and its code bytes
    CTR_COUNT = 64
};
static_assert(CTR_ANY_FIX == CTR_CHANGED + 1, "constructCenterReducedIndices fetches the two flags together");
static_assert(CTR_IL_PROBE == CTR_SCAN_TOTAL + 2, "interleavedIndexAssignEx fetches the total and the two probes together");
static_assert(CTR_ELL_TOO_LONG == CTR_ACTIVE_TOTAL + 7 && CTR_ELL_COLS == CTR_ELL_TOO_LONG + 1 && CTR_ELL_CODES == CTR_ELL_COLS + 1,
              "seven totals, then buildEll's three values: each group is one fetch");

// Arrays filled with one value by ONE launch (ps_context::fillI32): the 21 label / index arrays of a setup, the ten of the internal numbering
struct FillList {
    int32_t* p[21]; int64_t n[21];
    int count = 0;
    void add(int32_t* ptr, int64_t len) { p[count] = ptr; n[count] = len; ++count; }
};

// Fields moved by ONE launch of k_fields_copy / k_fields_swap_xz (ps_fields.hip): the up to 9 + 14 inputs of an upload, the 6 outputs of a
// download.  fast / mid / slow: the extents of the SOURCE's fastest, middle (always y) and slowest axis.
struct FieldTable {
    static constexpr int MAX = 23;
    const float* src[MAX]; float* dst[MAX];
    int32_t fast[MAX], mid[MAX], slow[MAX];
    int count = 0;
    // d: the sample grid's extents along x, y, z; srcZFastest: the source is stored k + d.z (j + d.y i), else i + d.x (j + d.y k)
    void add(const float* s, float* d_, int3 d, bool srcZFastest) {
        src[count] = s; dst[count] = d_;
        fast[count] = srcZFastest ? d.z : d.x; mid[count] = d.y; slow[count] = srcZFastest ? d.x : d.z;
        ++count;
    }
    int64_t entries(int q) const { return (int64_t)fast[q] * mid[q] * slow[q]; }
};
void launchFieldsCopy(const FieldTable& T, hipStream_t s);      // ps_fields.hip: dst = src, entry by entry
void launchFieldsSwapXZ(const FieldTable& T, hipStream_t s);    // ... dst = src with the x and z axes exchanged
enum ScanWord { SCAN_BAD = 0, SCAN_DIFFERS = 1, SCAN_FIRST = 2, SCAN_WORDS = 3 };   // k_field_scan: smallest bad index (~0: none), f[i] != f[0] somewhere, bits of f[0]
enum ScanBad { SCAN_BAD_NONE = 0, SCAN_BAD_NON_FINITE = 1, SCAN_BAD_NON_FINITE_OR_NEGATIVE = 2, SCAN_BAD_OUTSIDE_UNIT = 3 };   // which values count as bad (3: outside [-1, 1], a NaN included)
void launchFieldScan(const float* f, int64_t n, int bad, uint32_t* out, hipStream_t s);
// The refusal of a cell field whose smallest bad value (by mode `bad`) sits at x-fastest index `cell`, after the caller's label
inline std::string scanRefusal(const char* label, int bad, int64_t cell) {
    const char* what = bad == SCAN_BAD_NON_FINITE ? "non-finite value" : bad == SCAN_BAD_NON_FINITE_OR_NEGATIVE ? "non-finite or negative value" : "value outside [-1, 1]";
    return std::string(label) + what + " at cell " + std::to_string(cell);
}
// What a pass over a cell field found (k_field_scan, or the host loops of ps_upload_density_field): f[0], some f[i] != f[0], the smallest bad index (-1: none)
struct ScanFacts { float first = 0.f; bool differs = false; int64_t bad = -1; };
// One cell field of 4-byte words on its way into its x-fastest buffer (ps_context::cellIn allocates it), the values that refuse it
// (SCAN_BAD_NONE: not scanned) and the label of its refusal
struct CellIn { const void* src; void* dst; int bad; const char* label; };

// One collider's volume in the pool of ps_context::shapePool (ps_set_collider_shapes): extents, first sample, spacing, body-frame low corner
struct ShapeDesc { int32_t n[3]; int32_t pad; int64_t off; double h; double o[3]; };

struct CellField;     // ps_setup_util.hpp: what the setup kernels sample
struct FaceDensity;

}  // namespace ps

struct ps_context {
    // buffers this context dropped or grew inside a step, waiting for hipFree (ps_common.hpp: DeferredFrees).  First member: alive until the
    // last DevBuf below has gone.
    ps::DeferredFrees deferred;
    ps_context() { ps::MemState& M = ps::memState(); std::lock_guard<std::mutex> lk(M.m); M.lists.push_back(&deferred); ++M.contexts; }
    ~ps_context() {
        { ps::MemState& M = ps::memState(); std::lock_guard<std::mutex> lk(M.m); --M.contexts; for (size_t q = 0; q < M.lists.size(); ++q) if (M.lists[q] == &deferred) { M.lists.erase(M.lists.begin() + (long)q); break; } }
        ps::releaseDeferred(deferred);      // (ps_context_destroy has synchronised the stream)
    }
    ps_context(const ps_context&) = delete;
    ps_context& operator=(const ps_context&) = delete;
    // Release the dropped buffers: called where the stream has just been synchronised (end of setup / solve / step: streamIsIdle) and on
    // error paths (then only if the stream really is idle).  Never inside a step of threaded ranks (ps_common.hpp).
    void drainDeferred(bool streamIsIdle) {
        if (ps::threadedRanks()) return;
        if (!streamIsIdle && (!stream || hipStreamQuery(stream) != hipSuccess)) { (void)hipGetLastError(); return; }
        ps::releaseDeferred(deferred);
        ps::releaseDeferred(ps::orphanFrees());
    }
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // ---- parameters / geometry (Solver.cpp:18-68) ----
    ps_params P{};
    ps::Grid g{0, 0, 0, 0};
    double dx = 0, invDx = 0, dt = 0, invDt = 0, rho = 0;
    double valScale = 0;      // invDx / 64
    bool forceFp64Values = false;   // env PS_FORCE_FP64_VALUES=1: never use the coded values (A/B and fallback testing)
    bool haveInputWeights = false;
    bool viscUniform = false;       // the viscosity field is one value everywhere (checked at upload): samplers return it without loads
    float viscUniformValue = 0.f;
    // Variable density (ps_upload_density_field): densField = a non-constant cell field in `density`, sampled per face and clamped to
    // [densMin, densMax]; a constant one only sets rho to its clamped value.  rhoScalar: ps_fields_in.density of the last upload.
    double rhoScalar = 0, densMin = 0, densMax = 0;
    bool densField = false;
    int32_t densFieldHost = 0;      // array "densityField": the last setup used a non-constant field
    bool uploaded = false, isSetup = false, isSolved = false;
    std::string uploadDensity(const float* field, bool device, int layout, hipStream_t caller);   // ps_fields.hip
    // Device-resident fields (ps_*_device, ps_fields.hip): the caller's arrays are GPU memory in layout 0 (x fastest) or 1 (z fastest).
    // An upload is uploadCheck, uploadReset, one of the two ingests, uploadTail; the host path's ingest is the uploadField calls.
    // fieldEv: [0] recorded on the caller's stream and waited for by ours before we touch its arrays, [1] recorded on ours after a download
    // and waited for by the caller's (created on first use, destroyed with the context).  fieldScan / pinnedScan: k_field_scan's words and
    // their page-locked mirror.  fieldScratch: the x-fastest image of a solution grid on its way to a z-fastest destination.
    hipEvent_t fieldEv[2] = {nullptr, nullptr};
    ps::DevBuf<uint32_t> fieldScan;
    uint32_t* pinnedScan = nullptr;
    ps::DevBuf<float> fieldScratch;
    void uploadCheck(const ps_params* p, const ps_fields_in* in) const;   // throws; changes nothing
    static const char* missingField(const ps_fields_in* in);              // the message for a required field that is null, or null
    void uploadReset(const ps_params* p, const ps_fields_in* in);
    void ingestHost(const ps_fields_in* in);
    void ingestDevice(const ps_fields_in* in, int layout, hipStream_t caller);
    void uploadTail();
    std::string checkDeviceField(const void* ptr, int64_t count, const char* name) const;   // empty, or why the pointer is refused
    static const char* layoutRefusal(int layout);                         // the message for a layout that is neither 0 nor 1, or null
    std::string refuseFieldsIn(const ps_fields_in* in, int layout) const;
    void waitForCaller(hipStream_t caller);      // our stream waits for everything queued on the caller's so far
    void releaseToCaller(hipStream_t caller);    // the caller's stream waits for everything queued on ours so far
    void moveFields(const ps::FieldTable& T, int layout) { if (layout == 0) ps::launchFieldsCopy(T, stream); else ps::launchFieldsSwapXZ(T, stream); }
    const uint32_t* scanField(const float* f, int64_t n, int bad);   // k_field_scan (bad: ps::ScanBad) + fetch; synchronises the stream
    void upload(const ps_params* p, const ps_fields_in* in, int layout, hipStream_t caller);   // the device upload
    // Optional cell fields (density, sigma / ambient pressure, contact cosine, collider ids; DESIGN.md "optional cell fields"), ps_fields.hip.
    // moveCellFields: `count` grids of 4-byte words between the caller's arrays (f[q].src towards us, f[q].dst away from us) and our x-fastest
    // buffers: a host array by hipMemcpyAsync, device arrays by one launch behind the caller's stream (which then waits for a download).
    // ingestCellFields: moves the fields in, scans them in list order and returns the first refusal, or empty; ends with the stream
    // synchronised.  The scan words the call allocated go with it unless keepScanWords (the density field keeps them).  facts: of the last scan.
    // releaseIdle: what an entry point that dropped buffers ends with.
    template <class T> ps::CellIn cellIn(const T* src, ps::DevBuf<T>& dst, int bad, const char* label) {
        static_assert(sizeof(T) == 4, "the ingest kernels move 4-byte words whatever they hold");
        HIP_CHECK(hipSetDevice(device));
        dst.alloc((size_t)g.count(0));
        return ps::CellIn{src, dst.p, bad, label};
    }
    void moveCellFields(const ps::CellIn* f, int count, bool in, bool device, int layout, hipStream_t caller);
    std::string ingestCellFields(const ps::CellIn* f, int count, bool device, int layout, hipStream_t caller, bool keepScanWords, ps::ScanFacts* facts = nullptr);
    void releaseIdle(bool dropped);
    void downloadDevice(const ps_fields_out* out, int layout, hipStream_t caller);
    void downloadSolutionDevice(const ps_solution_out* out, int layout, hipStream_t caller);
    // Surface tension (ps_set_surface_tension): sigmaSet is the context setting, sigmaUsed the value of the last setup (array "surfaceTension").
    // With sigma > 0 the setup adds the ghost-pressure impulse to rhsA / rhsR (ps_surface.hip); the buffers exist only then.
    double sigmaSet = 0, sigmaUsed = 0;
    ps::DevBuf<float> kappaRaw, kappaC;      // cell grids: kappa of the SDF, and kappa_c (sampled at the interface point, clamped)
    ps::DevBuf<int32_t> stReduced;           // reduced faces that received an impulse (array "surfaceTensionReducedFaces")
    void applySurfaceTension();              // ps_surface.hip: after the blocks and tile rhs, before b
    // Free-surface fields (ps_upload_surface_fields): the sigma and ambient-pressure cell fields of the last call, for the grid of the last
    // upload (every upload drops them).  With either present the setup forms q_c = sigma_c kappa_c + P_c in surfQ (array
    // "surfaceGhostPressure") and the force kernels read it; surfFieldsUsed: bit 0 / 1 = the last setup used the sigma / pressure field
    // (array "surfaceFields").  The three buffers exist only while a field is present.
    ps::DevBuf<float> surfSigma, surfPressure;
    ps::DevBuf<double> surfQ;
    bool surfSigmaField = false, surfPressureField = false;
    int32_t surfFieldsUsed = 0;
    bool dropSurfaceFields();                // ps_fields.hip: false when there was nothing to drop
    void registerSurfaceFieldArrays();       // ps_fields.hip: q_c of the last setup (none once the fields are dropped)
    std::string uploadSurfaceFields(const ps_surface_fields* f, bool device, int layout, hipStream_t caller);   // ps_fields.hip
    // Contact angles (ps_set_contact_angle, ps_upload_contact_cosine_field; ps_wetting.hip): contactDegSet / contactCosSet are the context
    // setting (degrees < 0: off) and its cosine, contactCos the cosine cell field of the last call, for the grid of the last upload (every
    // upload drops it).  A setup that computes the curvature with either set rewrites the SDF inside the solid into wetPhi[0] (array
    // "surfaceWetted"; wetPhi[1] is the other Jacobi iterate) and the curvature kernels read that; wetFlags: one byte per block of cells
    // that holds a cell of the update set, wetCount: the set's size (array "contactCells").  contactDegUsed / contactCosUsed /
    // contactFieldUsed / contactRan: what the last setup did (arrays "contactAngle", "contactCosine", "contactField").  The wet buffers
    // exist from the first setup that runs the rule to the first that does not, or to ps_set_contact_angle(-1) with no field present.
    double contactDegSet = -1., contactCosSet = 0., contactDegUsed = -1., contactCosUsed = 0.;
    ps::DevBuf<float> contactCos, wetPhi[2];
    ps::DevBuf<uint8_t> wetFlags;
    ps::DevBuf<int32_t> wetCount;
    bool contactCosField = false, contactRan = false;
    int32_t contactFieldUsed = 0;
    const float* applyContactAngle(bool curvature);   // ps_wetting.hip: the SDF the curvature reads (surface itself when the rule does not run)
    bool dropWetting();                      // ps_wetting.hip: the wet buffers and their arrays; false when there was nothing to drop
    bool dropContactCosine();                // ps_wetting.hip: false when there was nothing to drop
    void registerWettingArrays();            // ps_wetting.hip: what the last setup's rewrite left (none when it did not run)
    std::string uploadContactCosine(const float* cosTheta, bool device, int layout, hipStream_t caller);   // ps_wetting.hip
    // Solid boundary (ps_set_solid_boundary): solidBoundarySet is the context setting, solidBoundaryUsed the mode of the last setup (array
    // "solidBoundary"; constructMatrixBlocks copies it).  slipEdges: free-slip edges counted by the St count pass (array "solidSlipEdges").
    int32_t solidBoundarySet = PS_SOLID_NO_SLIP, solidBoundaryUsed = PS_SOLID_NO_SLIP;
    ps::DevBuf<int32_t> slipEdges;
    // Non-Newtonian viscosity (ps_set_rheology): rheoSet is the context setting, rheoModelUsed the model of the last setup (array
    // "rheologyModel").  With the model on, computeRheology (ps_rheology.hip) writes mu_c / gammaDot_c into rheoMu / rheoRate from the velocity
    // of rheoFromOut ? velOut : vel, and viscSource() hands rheoMu to the setup's samplers.  rheoPass / rheoCarry: the Picard pass in flight
    // (0: the step's first solve) and whether another pass follows it (stepWithPasses); rheoIters: the PCG iterations of each solve of the step.
    ps_rheology rheoSet{PS_RHEOLOGY_NEWTONIAN, 0, 1., 0., 1e-3, 1e-3, 1e6};
    int32_t rheoModelUsed = PS_RHEOLOGY_NEWTONIAN;
    ps::DevBuf<float> rheoMu, rheoRate;
    bool rheoFromOut = false, rheoCarry = false;
    int rheoPass = 0;
    std::vector<int32_t> rheoIters;
    void computeRheology();                  // ps_rheology.hip: after constructActiveIndices, before the tile matrices
    int stepWithPasses(ps_stats* stats);     // ps_rheology.hip: setup + solve, then the Picard passes of a single-domain step
    // The one viscosity field the setup samples (ps_blocks.hip / ps_tiles.hip makeArgs): the uploaded one, or mu with the model on; and the
    // one face density: the uploaded field with its clamp bounds, or the scalar rho (ps_context.hip)
    ps::CellField viscSource() const;
    ps::FaceDensity densSource() const;

    // ---- inputs (fp32 Houdini voxel arrays, HDK_PolyStokes.C:235-246) ----
    ps::DevBuf<float> surface, collision, viscosity, density, vel[3], cvel[3];
    ps::DevBuf<double> densFace[3];          // a density field's clamped face samples, per face grid (the tile mass sums read them)
    ps::DevBuf<float> velOut[3], valid[3];

    // ---- weights, labels, indices (Solver.h:316-335) ----
    ps::DevBuf<float> liquidW[7], fluidW[7];
    ps::DevBuf<int32_t> labels[7], activeIdx[7], reducedIdx[7];
    ps::DevBuf<int32_t> faceRow[3];          // face -> internal row of S (-1: none)
    // Internal (solver) numbering: DOFs and face rows interleaved by 16^3 spatial block so that the SpMV
    // gathers stay in L2.  sysIdx[0]: cell -> base (p, txx, tyy, tzz = base+0..3); sysIdx[4..6]: edge -> index.
    // permSys[ref system index] = internal index; permRow[ref active-face index] = internal row.
    ps::DevBuf<int32_t> sysIdx[7];
    ps::DevBuf<int32_t> sysIdxT[3];          // cell -> internal index of its txx / tyy / tzz (sysIdx[0]: its pressure)
    int ilPlaneMajor = 0;                    // bit 0: DOFs, bit 1: face rows numbered kind-major inside every k-plane of a lattice block (buildInternalNumbering)
    ps::DevBuf<int32_t> permSys, permRow;
    int ilBlocks = 0;                        // lattice blocks in sequence order (incl. the padding blocks of partial super-blocks)
    std::vector<int32_t> blockStartSys, blockStartRow;   // first DOF / first active row of every lattice block (+ total): host copies
    ps::DevBuf<int32_t> cellScratch[3];      // layer marks / CC labels / fix flags
    ps::DevBuf<int32_t> scanBlock;           // block sums for scans
    ps::DevBuf<int32_t> counters;            // small device counters (flags, totals)

    // ---- counts (Solver.h:272-285) ----
    int64_t nCenter = 0, nFace[3] = {0, 0, 0}, nEdge[3] = {0, 0, 0};
    int64_t nActiveVs = 0, nReducedVs = 0, nPressures = 0, nStresses = 0, nSystem = 0, nTotalDOFs = 0;
    int64_t regionCount = 0;
    int64_t nReducedRows = 0;   // reduced faces that carry at least one stencil entry
    int64_t nRows = 0;          // nActiveVs + nReducedRows

    // ---- per-region data (Solver.h:339, 705-706) ----
    ps::DevBuf<int32_t> bbox;                // R*6: min xyz, max xyz (cells)
    std::vector<int32_t> hbbox;
    ps::DevBuf<double> COM, cfit, Mr, Kv, Binv, rhsR, regionScratch;
    // Work items of the per-region dense sums (host built, small): one item = <= FB_CHUNK positions of the face box of one axis of one listed
    // region, the regions in list order, per region axis by axis, per axis by rising start; regionPtr[q] .. regionPtr[q + 1] = the items of the
    // q-th listed region (ps_tiles.hip: buildFaceBoxItems)
    struct FaceBoxItems {
        ps::DevBuf<int32_t> region, axis, start, regionPtr;
        int64_t count = 0;
    };
    FaceBoxItems fbItems;                                        // of every region
    // classes of identical tiles (ps_tiles.hip:buildTileClasses): tileRep[r] = the region whose Mr / K region r copies (itself: sums its own);
    // repList = the tileReps representatives, repItems = their face-box items alone
    ps::DevBuf<unsigned long long> tileSig; ps::DevBuf<int32_t> tileUnique, tileRep, repList;
    FaceBoxItems repItems;
    int64_t tileReps = 0;
    void buildTileClasses();
    // skin-row enumeration: items of <= FB_CHUNK positions of a region's UNION face box (ex+1)(ey+1)(ez+1); a position yields up
    // to three rows (its X, Y, Z face) — rows are ordered (region, position x-fastest, axis), so the faces hanging off one
    // voxel are adjacent rows like the active ones
    ps::DevBuf<int32_t> sbItemRegion, sbItemStart, sbItemCount, sbItemLong;   // sbItemLong: long (> 2 entries) skin rows of the item, numbered first
    std::vector<int32_t> skinCutsHost;                           // skin-row offsets where a chunk of S's stream may start (item starts, ends of the long rows)
    std::vector<int32_t> sbRegionItemPtrHost;                    // R+1
    int64_t sbItems = 0;
    int64_t maxRegionRows = 0;                                   // fullest region: decides fused / three-kernel tile apply
    ps::DevBuf<double> partials;                                  // items * 676 (or rows chunks * 26)

    // reduced rows of S: region-contiguous, deterministic order
    ps::DevBuf<uint32_t> rrowFace;           // packed (i,j,k,axis)
    ps::DevBuf<int32_t> rrowRegion;
    ps::DevBuf<int32_t> regionRowPtr;        // R+1, offsets into reduced rows
    ps::DevBuf<int32_t> rchunkRegion, rchunkStart, rchunkEnd, regionChunkPtr;  // <= RC_ROWS rows of ONE region per chunk (three-kernel tile apply)
    int64_t nRChunks = 0;
    bool bboxValid = false;      // bbox[] holds the boxes of the final regions (set by the small-region fix, cleared per setup)

    // ---- blocks (Solver.h:337-369): S = [G Dt ; Ghat Dhat] by face row, St its transpose ----
    ps::DevCSR S, St;
    ps::DevBuf<double> McInv, rhsA, uInv, rhsPT, Mc, uDiag, oldVs;
    // Value-set coding of the two diagonals the SpMV epilogues read (ps_blocks.hip:buildDiagonalCodes): when a diagonal takes at
    // most 256 distinct values (constant viscosity: uInv = invVisc * {volume fractions}; McInv = 1 / (rho * k/64)) the kernels
    // read a 1-byte code per row and look the fp64 value up in a 256-entry table held in LDS — the same bits, 7 bytes less per
    // row.  Decided per setup; any 257th value keeps the fp64 array (variable viscosity fields).  PS_NO_DIAG_CODES=1 disables.
    ps::DevBuf<uint8_t> uCode, mcCode;
    ps::DevBuf<double> uDict, mcDict;      // 256 entries each
    bool uCoded = false, mcCoded = false;
    // status arrays read from host memory (registerArrays: regHost): "valuesCoded", "columns16" (constructMatrixBlocks), "diagonalsCoded", "fusedStep"
    int32_t valuesCodedHost = 0, columns16Host = 0;
    int32_t diagFlagsHost = 0;
    int32_t fusedStepHost = 0;
    // The walks of the persistent SpMV launches of the last single-domain PCG solve (array "launchWalk", read from host memory): 5 records of
    // LAUNCH_WALK_FIELDS int32 (S, then St modes 0..3; ps_solve.hip Launch::noteWalk), written from the launch plan on the host while walkRecord is set
    static constexpr int LAUNCH_WALK_FIELDS = 8;
    int32_t launchWalkHost[5 * LAUNCH_WALK_FIELDS] = {};
    bool walkRecord = false;
    int32_t streamRunsHost[4] = {0, 0, 0, 0};
    int32_t rowPerLaneHost[2] = {0, 0};
    void buildDiagonalCodes();
    ps::DevBuf<ps::diag_t> dinvF;   // the Jacobi diagonal as the PCG kernels read it (16-bit storage: ps_common.hpp diag_t, see constructPreconditioner)
    ps::DevBuf<double> b, x, r, pvec, Ap, dinv, ts, vreg, wreg, recovered, tmp1, tmp2, tmp3, tmp4, tmp5;
    ps::DevBuf<double> chebPartials, chebPartials2;   // r.z partials of the Chebyshev polynomial's last term
    double chebLmax = 8.4;                            // upper end of the Chebyshev interval (estimateLambdaMax)
    bool chebInner32Req = false;                      // the caller asked for PS_PRE_CHEBYSHEV_F32 (P.preconditioner then holds PS_PRE_CHEBYSHEV)
    bool chebInner32 = false;                         // ... and this system runs it: the polynomial's z_j and face-row vector are stored as fp32 (ps_solve.hip: chebyshevApply)
    int32_t chebInner32Host = 0;
    ps::DevBuf<double> guess;   // [pressureGuess; stressGuess] of constructGuessVectors (Solver.cpp:512-531), internal numbering
    // Warm start (ps_set_warm_start, extension): in mode PS_WARM_PREVIOUS_STEP a kept single-domain PCG step leaves its [p; tau] in warmStore — seven
    // dense x-fastest fp32 grids (p, txx, tyy, tzz on the cell grid, then the YZ / XZ / XY edge stresses; 0 where a sample had no DOF), tagged with
    // the grid it was solved on — and the next PCG solve on the same (nx, ny, nz, dx) starts from it, gathered through that step's index maps.
    int32_t warmMode = 0;
    ps::DevBuf<float> warmStore;
    bool warmHave = false;
    int warmTag[3] = {0, 0, 0};
    double warmTagDx = 0;
    ps::DevBuf<double> warmX0;               // the x0 the last PCG solve of a mode-1 context used (array "warmStartVector"), internal numbering
    bool warmX0Valid = false;
    int32_t warmUsedHost = 0;                // 1: the last PCG solve started from the carried solution (array "warmStartUsed")
    // Mixed-precision solve (ps_set_solve_precision, extension; ps_solve.hip: solve): solvePrecisionSet is the context setting.  In mode
    // PS_PRECISION_MIXED a single-domain Jacobi / identity PCG solve on the two-unit row-per-lane kernels runs as passes on fp32 vectors — the
    // correction d32, p32, r32, the face-row vector ts32 and, in the five-kernel step, Ap32: allocated by the first such solve, dropped when
    // the mode returns to fp64 — around the fp64 x.  solvePrecisionUsedHost / passIters / trueResidualHost: arrays "solvePrecisionUsed",
    // "solvePassIterations", "solveTrueResidual" of the last PCG solve.
    int32_t solvePrecisionSet = PS_PRECISION_FP64, solvePrecisionUsedHost = 0;
    ps::DevBuf<float> d32, p32, r32, ts32, Ap32;
    std::vector<int32_t> passIters;
    double trueResidualHost = 0;
    bool dropMixedBuffers() { const bool had = d32.p != nullptr; d32.free(); p32.free(); r32.free(); ts32.free(); Ap32.free(); return had; }
    // Velocity extrapolation (ps_set_velocity_extrapolation, extension; ps_extrapolate.hip): extrapSet is the context setting, extrapUsedHost the
    // layers the last step ran (array "velocityExtrapolation": 0 when off, on a decomposition, or when the velocity was not written).
    // extrapLayer: the layer of every face, 1 B each (arrays "extrapolationLayerX" / Y / Z); extrapCounts: faces assigned per sweep (array
    // "extrapolationCounts").  Allocated by the first step that runs a layer, dropped when the setting returns to 0.
    int32_t extrapSet = 0, extrapUsedHost = 0;
    ps::DevBuf<int8_t> extrapLayer[3];
    ps::DevBuf<int32_t> extrapCounts;
    void extrapolateVelocity(int layers);               // ps_extrapolate.hip: after the write-back of a step whose velocity is written
    bool dropExtrapolation();                           // ps_extrapolate.hip: the layer buffers and their arrays; false when there was nothing to drop
    void registerExtrapolationArrays();                 // ps_extrapolate.hip: the arrays of the last step's layers (none without them)
    // Collider loads (ps_set_collider_loads, extension; ps_loads.hip): loadsCount / loadsPivots are the context setting (pivots empty: the
    // upload's orig), loadsUsedHost the count the last step computed loads for (array "colliderLoads": 0 when off, on a decomposition, or
    // when the step computed none; the getters need it > 0).  colliderIds: the id of every cell (ps_upload_collider_ids), for the grid of
    // the last upload (every upload drops it).  loadsPartial / loadsPartialN / loadsOccurs: per workgroup of k_loads_partial the 12 sums and
    // the term count of every collider that occurs in it, the dropped terms, and the bit mask of those colliders; loadsOut: force (3 count),
    // torque (3 count), scale (6 count), then Fx Fy Fz Tx Ty Tz per collider (6 count: what the getters copy); loadsTerms: count + 1.
    // Allocated by the first step that computes loads, dropped when the count returns to 0.
    int32_t loadsCount = 0, loadsUsedHost = 0;
    std::vector<double> loadsPivots;
    double orig[3] = {0., 0., 0.};                       // ps_fields_in.orig of the last upload
    ps::DevBuf<int32_t> colliderIds;
    ps::DevBuf<double> loadsPartial, loadsOut, loadsPivotsDev;
    ps::DevBuf<int32_t> loadsPartialN, loadsTerms;
    ps::DevBuf<unsigned long long> loadsOccurs;
    void computeColliderLoads();                         // ps_loads.hip: after the write-back of a step that solved and whose velocity is written
    bool dropLoadBuffers() {
        const bool had = loadsOut.p != nullptr;
        loadsPartial.free(); loadsOut.free(); loadsPivotsDev.free(); loadsPartialN.free(); loadsTerms.free(); loadsOccurs.free();
        return had;
    }
    void forgetLoads();                                  // ps_loads.hip: the last step's loads no longer stand (their arrays go)
    void registerLoadArrays();                           // ps_loads.hip: the arrays of the last step's loads (none without them)
    bool dropColliderIds();                              // ps_loads.hip: false when there was nothing to drop
    std::string uploadColliderIds(const int32_t* ids, bool device, int layout, hipStream_t caller);   // ps_loads.hip
    void copyColliderLoads(double* dst, int64_t len, bool device, hipStream_t caller);                 // ps_loads.hip: throws when there are none
    // Collider tables (ps_paint_collider_velocities, ps_place_colliders, extensions): a call brings `stride` doubles per collider, acts on the
    // grid at once and keeps a ps::ColliderTable for the arrays: the table the kernel read, count + 2 counters, and the count of the last call
    // since the last upload (0: none, and none of the feature's arrays).  Allocated by a call, as long as its count needs; dropped by every
    // upload.  ingestColliderTable: drops a pair of another length (true: something was dropped), allocates, copies the table (host
    // memory, or device memory behind what the caller's stream holds) and clears the counters.  finishColliderTable: the count, the
    // arrays, a synchronisation in the host form only (its table is pageable memory), releaseIdle(dropped).
    bool ingestColliderTable(ps::ColliderTable& C, const double* src, int count, int stride, bool device, hipStream_t caller);
    void finishColliderTable(ps::ColliderTable& C, int count, bool device, bool dropped);
    bool dropColliderTable(ps::ColliderTable& C);        // the pair and the feature's arrays; false when there was nothing to drop
    // Collider motions (ps_motions.hip): 9 doubles per collider, painted into cvel; what a call wrote lives as long as that upload's cvel.
    ps::ColliderTable motions{&ps_context::registerMotionArrays};
    void paintColliderVelocities(const double* motion, int count, bool device, hipStream_t caller);    // ps_motions.hip: after the ABI's refusals
    bool dropMotions() { return dropColliderTable(motions); }
    void registerMotionArrays();                         // ps_motions.hip: the arrays of the last call (none without one since the last upload)
    // Collider shapes (ps_shapes.hip).  The shapes are a context setting: shapesCount (array "colliderShapes"; 0: none), shapePool: every
    // volume's samples back to back, shapeDesc: a descriptor per collider; kept across uploads, dropped by a call with count 0.  A placement
    // (12 doubles per collider) rewrites collision and colliderIds at once, creating the id field where there is none; what it wrote lives
    // as long as that upload's collision.
    int32_t shapesCount = 0;
    ps::DevBuf<float> shapePool;
    ps::DevBuf<ps::ShapeDesc> shapeDesc;
    ps::ColliderTable placement{&ps_context::registerPlacementArrays};
    void setColliderShapes(const ps_collider_shape* shape, int count);                                 // ps_shapes.hip: after the ABI's refusals
    void placeColliders(const double* poses, int count, bool device, hipStream_t caller);              // ps_shapes.hip: after the ABI's refusals
    bool dropShapes();                                   // ps_shapes.hip: the pool, the descriptors and the array; false when there was nothing to drop
    bool dropPlacement() { return dropColliderTable(placement); }
    void registerShapeArrays();                          // ps_shapes.hip: "colliderShapes" while shapes are set
    void registerPlacementArrays();                      // ps_shapes.hip: the arrays of the last placement (none without one since the last upload)
    // Advection (ps_advect_fields, extension; ps_advect.hip): a call, not a setting.  It reads velOut (or the caller's carrier) and writes only
    // the caller's arrays; the context keeps the five counters (array "advectionCounts"), the order and the step factor r = dt / dx of the
    // last call since the last upload (arrays "advection", "advectionStep").  The counters are allocated by the first call and dropped
    // by every upload.
    int32_t advectOrderHost = 0;
    double advectStepHost = 0.;
    ps::DevBuf<int32_t> advectCounts;
    // The MacCormack correction (ps_advect_fields_scheme, scheme 1; ps_advect_correct.hip) adds eight counters (array "advectionCorrection"),
    // the scheme and the limiter of the last such call (array "advectionScheme") and, for the device form, the fp32 scratch of the forward
    // result, which only grows; every upload drops all three with the rest.
    int32_t advectSchemeHost[2] = {0, 0};
    ps::DevBuf<int32_t> advectCorrection;
    ps::DevBuf<float> advectScratch;
    void advectFields(const ps_advection& a, bool device, int layout, hipStream_t caller, int limiter = -1);   // ps_advect.hip: after the ABI's refusals; limiter >= 0: the correction
    void launchAdvect(const ps::AdvectTable& T, int total);                                          // ps_advect.hip: the forward pass, into the arrays T names
    void correctAdvected(const ps::AdvectTable& T, const ps::AdvectTable& H, int total, int limiter);   // ps_advect_correct.hip: the caller's arrays from the forward result in H's
    bool dropAdvection();                                // ps_advect.hip: the counters and the arrays; false when there was nothing to drop
    void registerAdvectionArrays();                      // ps_advect.hip: the arrays of the last call (none without one since the last upload)
    // The arrays that outlive a setup, solve or step (ps_context.hip states the rule); dropUploadScoped: what every upload drops
    void registerKeptArrays();
    bool dropUploadScoped();
    // Air pockets (ps_label_air_pockets, extension; ps_pockets.hip): the connected air regions of the grid of the last upload (every upload and
    // every ps_set_slab / ps_set_brick drops them; a setup, solve or step keeps them).  pocketsHave: labels exist; pocketCount: K;
    // pocketPassesHost: the global propagation passes the last call ran (array "airPocketPasses").  pocketIds: the pocket of every cell (-1:
    // none), the one cell grid held while labels exist; pocketUnits / pocketCells / pocketOpen / pocketVolume: K entries each.  The labels and
    // link bytes of the propagation live in cellScratch, which only a setup uses.
    bool inGroup = false;                                // a rank of a ps_group (ps_group_create)
    bool pocketsHave = false;
    int32_t pocketCount = 0, pocketPassesHost = 0;
    ps::DevBuf<int32_t> pocketIds, pocketCells, pocketOpen;
    ps::DevBuf<long long> pocketUnits;
    ps::DevBuf<double> pocketVolume;
    void labelAirPockets();                              // ps_pockets.hip: throws on a decomposition
    bool dropAirPockets();                               // ps_pockets.hip: false when there was nothing to drop
    void registerPocketArrays();                         // ps_pockets.hip: the arrays of the current labels (none without labels)
    void copyAirPockets(double* volume, int32_t* open, int64_t len);                                      // ps_pockets.hip: throws without labels
    void copyAirPocketIds(int32_t* dst, bool device, int layout, hipStream_t caller);                     // ps_pockets.hip: throws without labels
    std::string setAirPocketPressures(const double* pressure, int64_t len);                               // ps_pockets.hip: the refusal, or empty
    int64_t solutionGridCount(int q) const { return g.count(q < 4 ? 0 : q); }   // grid q of the store: 0..3 cell grid, 4..6 edge grids
    void scatterSolution(float* dst, int q0, int nq);   // ps_solve.hip: grids q0 .. q0+nq-1 of x, back to back in dst
    void carryWarmStart();                              // ps_solve.hip: x -> warmStore (after a kept step)
    bool gatherWarmStart();                             // ps_solve.hip: warmStore -> x, warmX0 (false: no matching store, x untouched)
    void dropWarmStart();
    // dotPartials: p.Ap partials of the St kernel; dotPartials2: their first-stage sums (one-shot St kernel only);
    // dotPartialsR: r.r / r.z partials of k_cg_update_r; dotPartials3: x.x partials of k_cg_update_xp.  Separate buffers:
    // every block of a step kernel sums its predecessor's partials while other blocks already write this kernel's.
    ps::DevBuf<double> dotPartials, dotPartials2, dotPartials3, dotPartialsR;
    ps::DevBuf<double> fusedPart;   // fused step (ps_solve.hip): S-kernel, tile, uInv p^2 and r.r/r.z partials, in that order
    ps::DevBuf<ps::CGScalars> scal;

    // ---- multi-GPU (slab decomposition; ps_dist.hip) ----
    bool slabEnabled = false;                // a decomposition is set (slab or brick) and world > 1
    int gOff[3] = {0, 0, 0};    // global index of the local cell (0, 0, 0): face positions use global indices, so a tile's matrices do not depend on the decomposition
    ps_slab slab{};             // rank / world (and the z-range when ps_set_slab was used)
    ps_brick brick{};           // the owned box in local coordinates, neighbours, global position (ps_set_slab fills it too)
    int64_t ownLo = 0, ownHi = 0;            // owned DOF range in the internal numbering (contiguous: the owned lattice blocks come first)
    int32_t ownedRangeHost[2] = {0, 0};      // the same for ps_query_array ("ownedRange")
    ps::DevBuf<int32_t> regionOwned;         // R flags
    ps::DevBuf<int32_t> blockMap;            // sequence position -> lattice block (owned blocks first); empty: lattice order
    int blockMapOwned = -1, blockMapFor = 0; // owned lattice blocks (-1: the map has to be rebuilt: ps_set_brick), blocks it was built for
    // exchange lists per LINK (internal system indices, canonical order over the cut's cross-section): the neighbour's samples my rows touch (halo)
    // and mine the neighbour's rows touch (own), below and above.  Links 0..2: the face neighbours along x, y, z.  Links 3..5 (one-round mode
    // only, r05): the DIAGONAL neighbours across two cuts — (x, y), (x, z), (y, z) — "below" = one brick down along both axes, "above" = one up along
    // both.  Only one kind of sample crosses a diagonal: the edge stress that lives on both cut planes (XY / XZ / YZ edges on the corner line), which
    // the skin rows of a tile that ends at both planes touch (a tile's rows belong to the tile's owner whatever plane they lie on) — so a diagonal
    // link has an upper halo list and a lower own list, the other two are empty.
    // One table: cut[l][side], side 0 = the neighbour below, side 1 = the one above.  Only buildHaloLists writes a list's n and hash.
    static constexpr int NLINK = 6;
    struct CutList { ps::DevBuf<int32_t> idx; int64_t n = 0; uint64_t hash = 0; };   // hash: order-sensitive, of the list's global keys
    struct Cut {
        CutList own, halo;
        ps::DevBuf<double> send, recv;
        std::vector<int32_t> hostOwn;       // host copy of own.idx: Dist::buildFixup merges them per DOF
        const CutList& list(bool ownKind) const { return ownKind ? own : halo; }
    };
    Cut cut[NLINK][2];
    ps::DevBuf<double> redbuf;
    void ensureBuffers(int l, size_t doubles) { for (Cut& k : cut[l]) k.send.alloc(doubles); for (Cut& k : cut[l]) k.recv.alloc(doubles); }
    static void linkAxes(int l, int& a, int& b) { a = l < 3 ? l : (l == 5 ? 1 : 0); b = l < 3 ? -1 : (l == 3 ? 1 : 2); }
    int axisStride(int a) const { return a == 0 ? 1 : (a == 1 ? brick.dims[0] : brick.dims[0] * brick.dims[1]); }
    bool linked(int l, int side) const { int a, b; linkAxes(l, a, b); const int32_t* has = side ? brick.hasUpper : brick.hasLower; return has[a] && (b < 0 || has[b]); }
    int nbr(int l, int side) const { int a, b; linkAxes(l, a, b); return linked(l, side) ? brick.rank + (side ? 1 : -1) * (axisStride(a) + (b >= 0 ? axisStride(b) : 0)) : -1; }
    int64_t exchangeEntries() const { int64_t n = 0; for (const auto& l : cut) for (const Cut& k : l) n += k.own.n + k.halo.n; return n; }
    // Overlap of the halo exchanges with the rows that do not need them (ps_dist.hpp: Dist::solve).  Chunk lists of the row-per-lane
    // kernels: [0] S chunks without a halo column, [1] S chunks with one; [2] St chunks holding halo rows with entries (their A p goes
    // to the neighbour), [3] St chunks of owned rows only.  St chunks of halo rows without entries are in neither: never launched.
    ps::DevBuf<int32_t> distList[5];          // [4]: the St chunks of [2] and [3] together, in chunk order — the ONE St launch of a rank whose exchanges are not overlapped
    int nDistList[5] = {0, 0, 0, 0, 0};
    bool distListsOk = false;
    hipStream_t commStream = nullptr;        // transports run here (= stream for in-process ranks: nothing to overlap on one stream)
    hipEvent_t distEv[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // what one distributed solve did (ps_dist_stats): bytes per iteration over the cuts, sampled transport / all-reduce times
    double distStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ps::DevBuf<int32_t> labelFlags;          // Dist::exchangeLabels: labels changed, REDUCED cells without a component
    ps::DevBuf<int32_t> fixDof, fixSrc;      // the merged fix-up of the fused step (k_dist_fixup_merged): DOFs that receive contributions, their sources
    ps::DevBuf<const double*> fixBufs;       // ... and the table of the twelve receive buffers
    int64_t nFix = 0;
    ps::DevBuf<unsigned char> scrMark;       // setup scratch of Dist::decideExchangeMode
    // in-process groups (all ranks of the group on one device and one stream): the rows of ALL ranks — what passes through the device's caches per
    // iteration — decide the cache policy (ntLevel), not this rank's share; and an exchange is ONE kernel for all ranks and links that gathers from
    // the senders' vectors and scatters into the receivers' (Dist::buildDirectExchange; table on rank 0: [0] values of p out, [1] contributions of A p back)
    int64_t deviceShareRows = 0;
    ps::DevBuf<unsigned char> xsegTab[2];
    int nXseg[2] = {0, 0}, xsegBlocks[2] = {0, 0};
    bool haloForward = false;                // the exchange lists carry the copies of an earlier axis's exchange (three forwarding rounds x -> y -> z); false: every
                                             // list holds the sender's OWN samples only and the three axes travel in ONE round (ps_dist.hpp: Dist::decideExchangeMode)
    int64_t haloLabelChanges = 0;            // halo cells whose label the owners' exchange changed in the last setup (both passes)
    void* rcclComm = nullptr;                // ncclComm_t when one process per GPU
    void* hostComm = nullptr;                // host-staged TCP transport (ps_comm_init_tcp): same algorithm without RCCL
    ps::DevBuf<ps::CGScalars> benchScal;     // scratch of ps_bench_kernel
    ps::DevBuf<double> benchOnes, benchZeros;
    bool ownsStream = true;
    ps::DevBuf<float> ownedFace[3];          // 1 where this rank is responsible for the output face
    ps::Own own() const {
        ps::Own o;
        o.enabled = slabEnabled ? 1 : 0;
        for (int a = 0; a < 3; ++a) { o.lo[a] = brick.lo[a]; o.hi[a] = brick.hi[a]; o.hasUpper[a] = brick.hasUpper[a]; }
        return o;
    }
    void buildHaloLists();                   // ps_grid.hip

    ps_interrupt_fn interruptCb = nullptr;   // polled between CG batches (UT_Interrupt equivalent)
    void* interruptUser = nullptr;
    bool interrupted = false;

    // ---- results ----
    int solveIterations = -1;
    double solveError = -1;
    int usedBiCGStab = 0;
    ps_stats lastStats{};

    std::map<std::string, ps::ArrayInfo> arrays;
    // a feature's arrays, by its one list: registered while the feature has them, erased otherwise
    template <size_t N> void setArrays(const ps::NamedArray (&list)[N], bool present) {
        for (const ps::NamedArray& a : list) { if (present) arrays[a.name] = a.info; else arrays.erase(a.name); }
    }
    std::map<std::string, std::vector<char>> hostArrays;   // materialised-on-demand exports

    // ---- stage methods: names follow exec/HDK_PolyStokesSolver.h:96-190 ----
    void upload(const ps_params* p, const ps_fields_in* in);
    void buildIntegrationWeightsAlt();                    // ps_grid.hip
    void classifyCells();
    void constructReducedRegions();
    void constructOnlyActiveRegions();
    void classifyFaces();
    void classifyEdges();
    void constructCenterReducedIndices(int part);         // 0: components + fixReducedRegionBoundaries, 1: fixSmallReducedRegions
    void constructFacesReducedIndices();
    void constructEdgesReducedIndices();
    void constructActiveIndices();
    void buildValidFaces();
    void computeRegionBoxes();                            // ps_tiles.hip
    void computeCenterOfMasses();
    void computeLeastSquaresFits();
    void computeReducedMassMatrices();
    void computeReducedViscosityMatricesInteriorOnly();
    void assembleReducedBlocks();                         // AssembleBlocks.cpp:147-244,356-367
    void constructMatrixBlocks();                         // ps_blocks.hip
    void buildCol16(ps::DevCSR& M, ps::Counter failSlot, const std::vector<int32_t>& cuts, const uint8_t* rowCode, int codeRows);   // ps_blocks.hip; cuts: row indices where a chunk should start
    void buildEll(ps::DevCSR& M);                         // the row-per-lane form of M's compressed stream (ps_blocks.hip)
    void buildStreams(bool share);                        // both compressed streams (ps_blocks.hip)
    bool shareRuns = true;
    ps::DevBuf<int2> scrChunkRows; ps::DevBuf<int32_t> scrSlice, scrStart4, scrVals, scrKeep, scrRemap, scrEllCol, scrEllCode, scrEllW; ps::DevBuf<unsigned long long> scrHash, scrKeys, scrUniq;   // buildCol16 scratch
    void ensureValues(ps::DevCSR& M);                    // decode the fp64 values of a coded block on demand (ps_blocks.hip)
    void buildVal4(ps::DevCSR& M);                        // fp64 values in the compressed stream's layout (fallback / A-B)
    std::vector<int32_t> regionRowPtrHost;                // R+1 offsets into the reduced rows (host copy)
    std::vector<int32_t> hostTab[20];                     // host-built tables of one setup, alive until the next: asynchronous uploads without a synchronisation
    void assembleSystemPressureStressFactored();          // ps_solve.hip
    void constructPreconditioner();
    int solve();
    void estimateLambdaMax();
    void applyPreconditionerDevice(const double* r, double* z, double* scratch);   // z = M^-1 r (parity hook, ps_apply_preconditioner)
    int chebyshevApply(const double* rvec, double* zA, double* zB, double* rzPartial, const ps::CGScalars* sc, bool firstDone = false, double** zOut = nullptr);
    double chebTheta() const;
    int ntLevel() const;
    int solveEigenCG();                                   // Solver.cpp:814-862 on the factored device operator
    void constructGuessVectors();                         // Solver.cpp:512-531
    // explicit A (AssembleSystem.cpp:351-430) in reference numbering, assembled on the host from the device blocks (export only)
    void buildExplicitA(std::vector<int64_t>& ptr, std::vector<int32_t>& col, std::vector<double>& val);
    void recoverVelocityFromPressureStress();
    void applySolutionToVelocity();
    void applyOperator(const double* x, double* y, double* dotPartialsOut);   // device pointers

    // orchestration (ps_context.hip)
    int setup(ps_stats* stats);
    void setupPhase(int phase);              // 0, 1, 2 in this order (setup() = all three); between them Dist exchanges the halo's cell labels
    std::shared_ptr<void> setupState;        // stage timer and clocks of the setup in flight
    int setupPhaseDone = -1;
    int solveStage(ps_stats* stats);
    void fillDimData(ps_stats* st) const;
    void registerArrays();

    // helpers
    int32_t orderedIndexAssign(int s, int mode, ps::DevBuf<int32_t>& out, int counterSlot = -1);   // ps_grid.hip
    int64_t interleavedIndexAssign(int ngroups, const int* samples, const int* weights, int32_t* const* outs);
    int64_t interleavedIndexAssignEx(int ngroups, const int* samples, const int* weights, int32_t* const* outs, bool ownFilter,
                                     int64_t* ownedRange);
    void buildInternalNumbering();                                            // ps_grid.hip
    int64_t exclusiveScanI32(int32_t* data, int64_t n, int counterSlot = -1);   // ps_grid.hip (counterSlot >= 0: total to counters[slot], no synchronisation)
    int32_t readCounter(ps::Counter idx);
    void fetchCounters(ps::Counter idx, int n, int32_t* out);   // counters[idx .. idx + n) in one round trip through the page-locked mirror (synchronises the stream: copies queued before it have landed too)
    int32_t* pinnedCounters = nullptr;       // page-locked mirror of `counters` (CTR_COUNT words): a count read lands there directly instead of through the runtime's staging copy
    void zeroChangeFlags();                  // CTR_CHANGED, CTR_ANY_FIX
    void fillI32(const ps::FillList& F, int32_t v);   // ps_context.hip
};

// kernel micro-benchmark dispatch (ps_solve.hip), used by ps_bench_kernel
void ps_bench_launch(ps_context* c, const std::string& kernel, const double* x, double* y);
int ps_dist_step_single(ps_context* c, ps_stats* stats);   // ps_solve.hip: distributed step of one rank (RCCL or TCP transport)
void ps_dist_release(ps_context* c);                       // ps_solve.hip: destroys the rank's communicator / sockets

namespace ps {
constexpr int FB_CHUNK = 4096;   // face-box positions per work item (per-region dense reductions)
constexpr int PS_SCAN_TILE = 2048;   // entries per workgroup of the scan kernels (ps_grid.hip: SCAN_TILE; asserted equal there): sizes their block-sum scratch
constexpr int RC_ROWS = 1280;    // reduced rows per chunk in the three-kernel tile apply (regions too large for one workgroup)
constexpr int TILE_FUSED_MAX_ROWS = 32768;   // regions up to this many skin rows: one workgroup gathers, solves and expands (k_tile_apply)
}  // namespace ps
