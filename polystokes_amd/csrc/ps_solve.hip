// The per-iteration hot loop: y = A x for the factored pressure-stress operator and the PCG around it.
//
//   A = -dt [G Dt]^T McInv [G Dt] - [JG JDt]^T BInv [JG JDt] - 1/2 diag(0, uInv)
//       (lib/include/ApplyPressureStressMatrix.h:102-179; explicit form exec/..._AssembleSystem.cpp:381-389)
// evaluated as  s = S x;  t_f = dt McInv_f s_f (active rows),  t_f = C_f . (BInv_r sum_{g in r} C_g s_g)
// (reduced rows, J evaluated on the fly);  y = -S^T t - 1/2 uInv x_tau.
//
// One translation unit, split over included parts:
//   ps_kernels_spmv.hpp  : k_spmv_S / k_spmv_St (CSR-stream one-shot kernels, fp64 or int8-coded values) and
//                          k_spmv_S_pipe / k_spmv_St_pipe (persistent, software-pipelined, compressed 3 B/nnz stream) —
//                          a 256-thread block owns 256 consecutive rows, products go through LDS, each thread sums its
//                          own short row; epilogues fuse the diagonal scalings, the -1/2 uInv x term and the p.Ap partials.
//                          k_spmv_*_ell (a lane owns a row) and k_spmv_*_ell2 / _ell2c (two units in flight per wave).  What they share exists
//                          once: the loops pipeLoop / ellLoop / ell2Loop (stream, prefetch, walk; the kernel passes its per-row loads and its
//                          row epilogue as callables), the walks chunkWalkAt / pairWalkChunk / pairWalkEnd (also called by Launch::noteWalk and
//                          pipeBlocks below), fusedPrologue (stop test, alpha), the row epilogues sRowFinish / stRowY / chebRowFinish /
//                          fusedRowFinish, and RowDiag (a diagonal as 1-byte codes into an LDS table or as the fp64 array).
//   ps_kernels_tiles.hpp : k_tile_gather / k_tile_solve / k_tile_expand — per-tile J^T, 26x26 BInv, J.
//   ps_kernels_cg.hpp    : k_cg_update_r / k_cg_update_xp (the PCG step of pcg_external_matrix_A, lib/include/pcg.h:268-340,
//                          with the scalar reductions and the stop rule folded in; scalars stay on the device), BiCGStab helpers, Jacobi
//                          diagonal, velocity recovery / write-back.  One body each — cgInit, cgUpdateR, cgUpdateXp (z from ZJacobi or ZVector;
//                          prologue sums as TwoSums, the stress diagonal as StressDiag) — takes the element type of the Krylov vectors and of the
//                          diagonal: the _f32 forms and k_cg_init_pass / k_cg_scal0_pass / k_cg_check_pass / k_cg_end_pass run the passes of the
//                          mixed-precision solve (ps_set_solve_precision: fp32 d, p, r, A p, t around the fp64 x; ps_context::solve), the _d64
//                          forms the exported system's step on its fp64 diagonal (ps_import.hpp).
//   this file            : the launch dispatch (Launch: planS / planSt choose the kernel and grid of a product, one launcher per kernel family runs it),
//                          ps_context::applyOperator / assemble / solve / recover.  The solve runs in stages (DomainSolve, as Dist's in ps_dist.hpp):
//                          solveStart, chooseStepForm, fusedStart, [mixedPasses: passStart + batches of the fp32 steps], pcgStart, batches of
//                          fourKernelStep / fiveKernelStep (one body for fp64 and fp32 vectors) or their ...ChebStep forms, bicgstabFallback; runBatches
//                          is the one batch driver (stop test, scalar read-back, interrupt), fusedSingle / fusedSlab + FusedZ build every FusedR.
//   ps_dist.hpp          : the z-slab distributed solve (RCCL or in-process ranks) and its C ABI.
//   ps_import.hpp        : MatrixMarket import + general CSR PCG (ps_solve_exported_system).
#include <algorithm>
#include <chrono>
#include <iterator>
#include <cstring>
#include <cmath>
#include <limits>
#include <ctime>

#include "ps_context.hpp"

using namespace ps;

namespace {
#include "ps_kernels_spmv.hpp"
#include "ps_kernels_tiles.hpp"
#include "ps_kernels_cg.hpp"
}  // namespace

// ---------------------------------------------------------------------------------------------------
namespace {
// A runtime value as a template argument: f gets std::integral_constant<int, V> for the first V equal to v (withOneOf; the last V
// otherwise) or not above v (withAtLeast).  Each launcher names the values its kernel is instantiated for, so no cross product is taken.
// (They return auto, so each is instantiated where it is called, depth first: the kernels it names are instantiated in the order they are written.)
template <class F> auto withBool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <int V0, int... V, class F> auto withOneOf(int v, F&& f) {
    if constexpr (sizeof...(V) == 0) f(std::integral_constant<int, V0>{}); else if (v == V0) f(std::integral_constant<int, V0>{}); else withOneOf<V...>(v, f);
}
template <int V0, int... V, class F> auto withAtLeast(int v, F&& f) {
    if constexpr (sizeof...(V) == 0) f(std::integral_constant<int, V0>{}); else if (v >= V0) f(std::integral_constant<int, V0>{}); else withAtLeast<V...>(v, f);
}
template <class F> auto withPolicy(int pol, F&& f) { withOneOf<3, 1, 0>(pol, f); }
// the pipelined kernels: the fp64-value stream (F64) with POL 3 only
template <class F> auto withPipe(bool packed, int pol, F&& f) {
    if (!packed) f(std::true_type{}, std::integral_constant<int, 3>{}); else withPolicy(pol, [&](auto POL) { f(std::false_type{}, POL); });
}
template <class T> struct Type { using type = T; };
// the element type of the Chebyshev polynomial's vectors z_j (fp32: PS_PRE_CHEBYSHEV_F32 where it runs, ps_context::chebInner32; fp64 otherwise)
template <class F> auto withZ(bool f32, F&& f) { if (f32) f(Type<float>{}); else f(Type<double>{}); }

// The kernel of one S or St product (ps_kernels_spmv.hpp).  CSR: k_spmv_S / k_spmv_St (one-shot); PIPE: k_spmv_S_pipe / k_spmv_St_pipe
// (persistent, compressed or fp64-value stream); ELL: k_spmv_S_ell / k_spmv_St_ell (FX), row-per-lane on the coded stream; two units in flight
// per wave: ELL2 = k_spmv_S_ell2 / _ell2u, or k_spmv_St_ell2 in its plain MODE 3 form, ELL2C = k_spmv_St_ell2c (a Chebyshev term), and
// k_spmv_St_ell2 with the polynomial's first term (ELL2Z), over a rank's owned rows (ELL2_OWN) or over rows that include halo rows (ELL2_HALO).
enum Kernel { CSR, PIPE, ELL, ELL2, ELL2C, ELL2Z, ELL2_OWN, ELL2_HALO };
struct Plan {
    Kernel kernel;
    int grid = 0, xcd = 0, nChunks = 0;   // workgroups (one partial sum each), ChunkWalk parameter after pipeBlocks (0: plain walk)
    int pol = 0, fx = 0;                  // Launch::policy, k_spmv_St_ell's FX
    bool run = true;                      // false: nothing to launch (no rows, an empty chunk list)
    const char* err = nullptr;            // a launch that must not happen
};

struct Launch {
    ps_context* c;
    const int* done;
    int rowsS, rowsSt, nA, nP;
    // fused residual update (DomainSolve::fusedStart: FusedR): where the S and tile kernels leave their shares of p.Ap (null: not asked for)
    double* sPart = nullptr;
    double* wvPart = nullptr;
    // chunk lists (row-per-lane kernels only; null: every chunk): ps_dist.hpp launches the chunks next to a cut and the others separately
    const int32_t* sList = nullptr; int nSList = 0;
    const int32_t* stList = nullptr; int nStList = 0;
    bool stOwnedOnly = false;        // the St chunk list holds owned rows only (the decomposition's launch under the exchange): FX bit 2
    bool cz32 = false;   // MODE 3 with the polynomial's first term: fr.cz points at floats (k_spmv_St_ell2<.., float>)
    bool v32 = false;    // a pass of the mixed-precision solve: the Krylov vectors and the face-row vector are fp32 (spmvS32 / tiles32 / spmvSt32 with the step's partials)
    bool ntSpmv = true;   // cache policy of the pipelined kernels' streams (ps_context::ntLevel >= 1)
    int pipeGrid;   // 0: one-shot kernels; >0: persistent software-pipelined kernels with this many blocks
    int stGrid = 0; // > 0: the St kernel's own cap
    int stGrid2 = 0; // > 0: the Chebyshev term's St launch alone (A/B)
    int xcdAware;   // pipelined kernels: runs of this many chunks are dealt to the XCDs round robin (ChunkWalk); 0 = plain walk
    bool dualS = true, dualT = true;   // the two-units-per-wave S / St kernels (PS_S_DUAL / PS_ST_DUAL = 0: the one-unit kernels)
    bool tileSplit = false;            // the three-kernel tile apply (PS_TILE_SPLIT)
    int tileTB = 0;                    // threads per region of the fused tile apply (PS_TILE_TB; 0: tileThreads())
    // MODE 3 of the row-per-lane St kernel in its plain form (FX = 1: no Chebyshev first term, no halo rows, coded uInv) fits 7 workgroups per CU
    bool plain3Hint = false;
    bool plain3Hint2 = false;   // the same for the Chebyshev step: single domain, coded uInv
    int32_t* walk = nullptr;    // ps_context::launchWalkHost while a solve records its walks (noteWalk), null otherwise

    // POL of the pipelined kernels (ps_kernels_spmv.hpp): 0 = default policy; 1 = non-temporal stores and epilogue streams, cached matrix
    // stream (most runs shared between chunks: read again and again); 3 = the matrix stream non-temporal too (every run read once)
    int policy(const ps::DevCSR& M) const { return !ntSpmv ? 0 : (2 * M.uniqueLen <= M.streamLen ? 1 : 3); }
    static bool ellOk(const ps::DevCSR& M) { return M.col16ok && M.packed && M.ellok; }

    // ---- the choice: which kernel runs a product, on how many workgroups.  The launchers below run it; the queries answer from it.
    Plan planS(int mode, bool list, int nList) const {
        const ps::DevCSR& M = c->S;
        Plan p{CSR};
        p.run = rowsS > 0; p.pol = policy(M); p.xcd = xcdAware;
        if (pipeGrid > 0 && ellOk(M)) {   // row-per-lane kernels on the coded stream (a chunk list: a decomposition's interior / boundary launches)
            p.nChunks = list ? nList : M.nChunks;
            p.grid = pipeBlocks(p.nChunks, p.xcd, true, sCap());
            p.run = p.run && p.nChunks > 0;
            // two units in flight per wave (k_spmv_S_ell2; r04): 256^3, same box, two interleaved rounds: S 0.2809 / 0.2816 -> 0.2672 / 0.2609 ms in
            // sequence, step 1128.6 / 1130.2 -> 1117.3 / 1118.5 ms (profiles/r04_s_dual.txt).  PS_S_DUAL=0: the one-unit kernel.
            p.kernel = (dualS && mode == 0 && (p.grid & 7) == 0) ? ELL2 : ELL;
        } else if (pipeGrid > 0 && M.col16ok && (M.packed || M.val4.p)) {
            p.kernel = PIPE; p.nChunks = M.nChunks;
            p.grid = pipeBlocks(p.nChunks, p.xcd, M.packed);
        } else
            p.grid = gridFor(rowsS, BS);
        return p;
    }
    // mode 2 (Chebyshev term fused into the epilogue, ChebArgs) exists on the pipelined kernels only: callers check stOnPipe()
    // mode 3 (residual update fused into the epilogue, FusedR): pipelined kernels on the coded stream only — callers check fusedOk()
    Plan planSt(int mode, bool list, int nList, bool ownedOnly, const FusedR& fr) const {
        const ps::DevCSR& M = c->St;
        Plan p{CSR};
        p.run = rowsSt > 0; p.pol = policy(M); p.xcd = xcdAware;
        if (pipeGrid > 0 && ellOk(M)) {   // row-per-lane kernels on the coded stream (k_spmv_St_ell)
            p.nChunks = list ? nList : M.nChunks;
            p.grid = pipeBlocks(p.nChunks, p.xcd, true, stGridFor(mode));
            p.run = p.run && p.nChunks > 0;
            p.kernel = ELL;
            // Two units in flight per wave (k_spmv_St_ell2; r04): 256^3, one box, interleaved rounds: St with the residual update 0.4251 / 0.4242 ->
            // 0.3923 / 0.3918 ms in sequence at 5 waves per SIMD on 1280 workgroups, step 1124.5 / 1122.6 -> 1098.3 / 1096.6 ms; compiled for 6 waves per
            // SIMD on 1536 workgroups another 0.6 % (profiles/r04_st_dual.txt).  PS_ST_DUAL=0: the one-unit kernel on 1792 workgroups.
            // The MODE 3 specialisations of k_spmv_St_ell (FX) take coded uInv only, without the Chebyshev term: in a single domain (3) or on a
            // slab rank (1, 5); the two-unit kernels also take the stress diagonal as the fp64 array (UC = false, r06: a viscosity field with more
            // than 256 values).
            const bool g8 = (p.grid & 7) == 0, plainFr = !fr.yOut && !fr.red && fr.rStride == 0;
            const bool coded3 = mode == 3 && c->uCoded && !fr.cz, single3 = mode == 3 && !fr.cz && plain3Hint && plainFr;
            if (mode == 2 && dualT && !list && g8 && !c->slabEnabled) p.kernel = ELL2C;
            else if (mode == 3 && dualT && plain3Hint2 && fr.cz && !fr.dinvF && plainFr && !list && g8) p.kernel = ELL2Z;
            else if (cz32 && mode == 3 && fr.cz) p.err = "internal: single-precision Chebyshev vectors without the two-unit St kernel";
            else if (single3 && stDual() && !list && g8) p.kernel = ELL2;
            else if (single3 && c->uCoded) p.fx = 3;
            else if (mode == 3 && !fr.cz && ownedOnly && list && dualT && fr.red && g8) p.kernel = ELL2_OWN;
            else if (mode == 3 && !fr.cz && dualT && fr.red && fr.yOut && !ownedOnly && g8) p.kernel = ELL2_HALO;
            else if (coded3 && ownedOnly && list) p.fx = 5;
            else if (coded3) p.fx = 1;
        } else if (pipeGrid > 0 && M.col16ok && (M.packed || M.val4.p)) {
            p.kernel = PIPE; p.nChunks = M.nChunks;
            p.grid = pipeBlocks(p.nChunks, p.xcd, M.packed, stGridFor(mode));
            if (mode == 3 && !M.packed) p.err = "internal: fused residual update on the fp64 stream";
        } else {
            p.grid = gridFor(rowsSt, BS);
            if (mode >= 2) p.err = "internal: fused St epilogue without the pipelined St kernel";
        }
        return p;
    }
    bool listsOk() const { return planS(0, false, 0).kernel >= ELL && planSt(0, false, 0, false, FusedR{}).kernel >= ELL; }
    bool stOnPipe() const { return planSt(0, false, 0, false, FusedR{}).kernel != CSR; }
    // the fused step needs both products on the persistent coded-stream kernels (their per-workgroup partials)
    bool fusedOk() const {
        const Plan s = planS(0, false, 0), t = planSt(0, false, 0, false, FusedR{});
        return rowsS > 0 && s.kernel != CSR && c->S.packed && t.kernel != CSR && c->St.packed;
    }
    // workgroups of a launch over every chunk / over a list of n chunks of S / St (the partial sums it writes)
    int sBlocks() const { return planS(0, false, 0).grid; }
    int sBlocksFor(int n) const { return planS(0, true, n).grid; }
    int stBlocks(int mode = 0) const { return planSt(mode, false, 0, false, FusedR{}).grid; }
    int stBlocksFor(int n, int mode) const { return planSt(mode, true, n, false, FusedR{}).grid; }
    // ---- the inner operator applies of the single-precision Chebyshev polynomial (PS_PRE_CHEBYSHEV_F32): z_j and the face-row vector are stored
    // as fp32 (ps_kernels_spmv.hpp: VecIO), on the pair-walking two-unit kernels only (their grid a multiple of 8 with the XCD walk on) and the
    // fused tile apply; otherwise the fp64 form runs
    bool cheb32Ok() const {
        const Plan s = planS(0, false, 0), t = planSt(2, false, 0, false, FusedR{});
        return s.run && s.kernel == ELL2 && s.xcd > 0 && t.run && t.kernel == ELL2C && t.xcd > 0 && (c->regionCount == 0 || tileFused());
    }

    // ---- the passes of the mixed-precision solve (ps_set_solve_precision): p, r, A p and the face-row vector stored as fp32, on the same kernels
    // as the fp32 polynomial — the pair-walking two-unit S kernel and the fused tile apply (cheb32Ok's condition on them) — and on the two-unit
    // St kernel of the plain single-domain step, which carries the residual update (four-kernel step) or writes A p (five-kernel step)
    bool mixedOk() const {
        const Plan s = planS(0, false, 0), t = planSt(3, false, 0, false, FusedR{});
        return s.run && s.kernel == ELL2 && s.xcd > 0 && t.run && t.kernel == ELL2 && t.xcd > 0 && (c->regionCount == 0 || tileFused());
    }

    // ---- the walk of a launch (array "launchWalk"): the first launch of each slot (0: S, 1 + mode: St) in a recording solve writes
    // {1, kernel, nChunks, grid, walk parameter, 1 if the pair walk, least / most steps with a chunk of one workgroup} — host arithmetic on the
    // plan with the kernels' own walk functions (ps_kernels_spmv.hpp): the pair walk of the two-unit kernels (pairWalkChunk: runs of 32 pairs per
    // XCD, steps l, l + per, .. below pairWalkEnd) and chunkWalkAt of the one-unit and pipelined kernels; the one-shot CSR kernels take one step
    void noteWalk(int slot, const Plan& p) const {
        if (!walk || !p.run) return;
        int32_t* w = walk + slot * ps_context::LAUNCH_WALK_FIELDS;
        if (w[0]) return;
        const bool pair = p.kernel >= ELL2;
        int lo = 1, hi = 1;
        if (p.kernel != CSR) {
            lo = INT32_MAX; hi = 0;
            const int qEnd = pairWalkEnd(p.nChunks), per = p.grid >> 3, sh = chunkWalkShift(p.xcd), rs = chunkWalkRun(p.xcd);
            for (int b = 0; b < p.grid; ++b) {
                int steps = 0;
                if (pair)   // steps whose pair exists (a chunk for the first half); the others run the loop without a chunk
                    for (int q = b >> 3; q < qEnd; q += per) steps += pairWalkChunk(q, b & 7, 0, p.nChunks) >= 0;
                else
                    while (chunkWalkAt(steps, b, p.grid, sh, rs) < p.nChunks) ++steps;
                lo = std::min(lo, steps); hi = std::max(hi, steps);
            }
        }
        const int32_t rec[ps_context::LAUNCH_WALK_FIELDS] = {1, (int32_t)p.kernel, p.nChunks, p.grid, p.xcd, pair ? 1 : 0, lo, hi};
        std::memcpy(w, rec, sizeof(rec));
    }
    // ---- launchers, one per kernel family.  (Each names its kernels in the order the dispatch has always instantiated them: the code
    // object lays the kernels out in that order.)
    // the row-per-lane kernels: the coded ELL stream of M leads every argument list
    template <class K, class... A> auto ellLaunch(K k, const Plan& p, const ps::DevCSR& M, A... a) const {
        hipLaunchKernelGGL(k, dim3(p.grid), dim3(BS), 0, c->stream, M.ecol.p, M.ecode.p, (unsigned)(M.ellCols * 2), (unsigned)M.ellCodes, M.winBase.p, M.echunk.p, c->valScale, a...);
    }
    // k_spmv_S_ell2 (the face mass McInv as 1-byte codes) / k_spmv_S_ell2u (past 256 distinct values, a density field: the fp64 array);
    // TV = float (the Chebyshev polynomial's inner applies) over every chunk only
    template <class TV> auto sEll2(const Plan& p, const TV* x, TV* out, double* part, const int32_t* list) const {
        const ps::DevCSR& M = c->S;
        const uint8_t* mc = c->mcCoded ? (const uint8_t*)c->mcCode.p : (const uint8_t*)c->McInv.p;
        withPolicy(p.pol, [&](auto POL) { withBool(c->mcCoded, [&](auto MC) {
            auto go = [&](auto LIST) {
                constexpr int pol = decltype(POL)::value; constexpr bool lst = decltype(LIST)::value;
                auto k = [] { if constexpr (decltype(MC)::value) return k_spmv_S_ell2<pol, lst, TV>; else return k_spmv_S_ell2u<pol, lst, TV>; }();
                ellLaunch(k, p, M, x, (int)M.cols, rowsS, nA, c->dt, out, done, p.nChunks, mc, c->mcDict.p, part, list);
            };
            if constexpr (std::is_same<TV, double>::value) withBool(list, go); else go(std::false_type{});
        }); });
    }
    template <class TV> auto stEll2c(const Plan& p, const TV* t, const TV* xin, TV* out, double* partial, const ChebArgs& ca) const {
        const ps::DevCSR& M = c->St;
        const uint8_t* uArg = c->uCoded ? (const uint8_t*)c->uCode.p : (const uint8_t*)c->uInv.p;
        withBool(c->uCoded, [&](auto UC) { withPolicy(p.pol, [&](auto POL) {
            ellLaunch(k_spmv_St_ell2c<POL, TV, UC>, p, M, t, (int)M.cols, rowsSt, xin, out, partial, done, p.nChunks, ca, uArg, c->uDict.p);
        }); });
    }
    void spmvS(int mode, const double* x, double* out) const {
        const Plan p = planS(mode, sList, nSList);
        if (!p.run) return;
        if (mode == 0 && !sList) noteWalk(0, p);
        const ps::DevCSR& M = c->S;
        const uint8_t* mc = c->mcCoded ? c->mcCode.p : (const uint8_t*)nullptr;
        switch (p.kernel) {
        case CSR:
            withOneOf<0, 1>(mode, [&](auto MODE) { withBool(M.packed, [&](auto PK) {
                hipLaunchKernelGGL((k_spmv_S<MODE, 8, PK>), dim3(p.grid), dim3(BS), 0, c->stream, M.ptr.p, M.col.p, M.val.p, M.code.p, c->valScale, x, rowsS, nA, c->dt, c->McInv.p, out, done);
            }); });
            return;
        case ELL2: sEll2(p, x, out, sPart, sList); return;
        case ELL:
            withOneOf<0, 1>(mode, [&](auto MODE) { withPolicy(p.pol, [&](auto POL) { withBool(sList, [&](auto LIST) {
                ellLaunch(k_spmv_S_ell<MODE, POL, LIST>, p, M, x, (int)M.cols, rowsS, nA, c->dt, c->McInv.p, out, done, p.nChunks, p.xcd, mc, c->mcDict.p, sPart, sList);
            }); }); });
            return;
        default:   // PIPE
            withOneOf<1, 2>(M.nv, [&](auto NV) { withOneOf<0, 1>(mode, [&](auto MODE) { withPipe(M.packed, p.pol, [&](auto F64, auto POL) {
                hipLaunchKernelGGL((k_spmv_S_pipe<MODE, NV, F64, POL>), dim3(p.grid), dim3(BS), 0, c->stream, M.col16.p, M.code4.p, M.val4.p, (int)M.streamLen, M.winBase.p,
                                   M.chunkInfo.p, M.len8.p, c->valScale, x, (int)M.cols, rowsS, nA, c->dt, c->McInv.p, out, done, p.nChunks, p.xcd, mc, c->mcDict.p, sPart);
            }); }); });
        }
    }
    // ---- tiles
    bool tileFused() const { return c->maxRegionRows <= TILE_FUSED_MAX_ROWS && !tileSplit; }
    // threads per region of the fused apply: enough threads in flight chip-wide (~256 K) without starving a region of work.  Measured
    // at 256^3 (4096 tiles of 3204 rows): 0.080 ms with 64 threads, 0.087 / 0.106 / 0.166 with 128 / 256 / 512; at 32^3
    // (8 tiles) one wavefront per tile serialises 50 rows per lane behind memory latency (60 us per CG iteration
    // against 43 with 256 threads per tile; 1024 threads: 50, the block reduction over 16 waves costs more than it hides).
    int tileThreads() const {
        int tb = 64;
        while (tb < 256 && (int64_t)tb * c->regionCount < 262144 && (int64_t)tb * 2 < c->maxRegionRows) tb *= 2;
        return tb;
    }
    template <int MODE, class TS, class TB> auto tileApply(TB, TS* sred, double* part) const {
        hipLaunchKernelGGL((k_tile_apply<MODE, TB::value, TS>), dim3((unsigned)c->regionCount), dim3(TB::value), 0, c->stream, c->regionRowPtr.p, c->rrowFace.p, c->COM.p,
                           c->dx, make_int3(c->gOff[0], c->gOff[1], c->gOff[2]), c->Binv.p, c->rhsR.p, c->invDt, sred, c->vreg.p, done, part);
    }
    void tiles(int mode, double* ts) const {   // ts: face-row vector; reduced part rewritten in place
        if (c->regionCount == 0) return;
        double* sred = ts + nA;
        if (tileFused()) {   // one workgroup per region: gather, 26x26 block, expand
            withOneOf<0, 1, 2>(mode, [&](auto MODE) { withAtLeast<1024, 512, 256, 128, 64>(tileTB ? tileTB : tileThreads(), [&](auto TB) {
                tileApply<MODE, double>(TB, sred, wvPart);
            }); });
            return;
        }
        if (mode != 2 && c->nRChunks > 0)
            hipLaunchKernelGGL(k_tile_gather, dim3((unsigned)c->nRChunks), dim3(64), 0, c->stream, c->rchunkRegion.p, c->rchunkStart.p, c->rchunkEnd.p,
                               c->rrowFace.p, c->COM.p, c->dx, make_int3(c->gOff[0], c->gOff[1], c->gOff[2]), sred, c->wreg.p, done);
        withOneOf<0, 1, 2>(mode, [&](auto MODE) {
            hipLaunchKernelGGL(k_tile_solve<MODE>, dim3((unsigned)c->regionCount), dim3(64), 0, c->stream, c->regionChunkPtr.p, c->wreg.p, c->Binv.p, c->rhsR.p,
                               c->invDt, c->vreg.p, done, MODE == 0 ? wvPart : (double*)nullptr);
        });
        if (mode != 1 && c->nRChunks > 0)
            hipLaunchKernelGGL(k_tile_expand, dim3((unsigned)c->nRChunks), dim3(BS), 0, c->stream, c->rchunkRegion.p, c->rchunkStart.p, c->rchunkEnd.p,
                               c->rrowFace.p, c->COM.p, c->dx, make_int3(c->gOff[0], c->gOff[1], c->gOff[2]), c->vreg.p, sred, done);
    }
    // ---- the fp32 inner applies of the Chebyshev polynomial (cheb32Ok)
    void spmvS32(const float* x, float* out) const {
        const Plan p = planS(0, false, 0);
        if (p.kernel != ELL2) throw Error("internal: single-precision S apply without the two-unit kernel");
        noteWalk(0, p);
        sEll2(p, x, out, v32 ? sPart : (double*)nullptr, (const int32_t*)nullptr);
    }
    void tiles32(float* ts) const {   // the fused apply only, at the default threads per region
        if (c->regionCount == 0) return;
        withAtLeast<256, 128, 64>(tileThreads(), [&](auto TB) { tileApply<0, float>(TB, ts + nA, v32 ? wvPart : (double*)nullptr); });
    }
    // the St product of a pass of the mixed-precision solve (mixedOk): t, p and fr.r point at floats.  ap: the plain product — A p -> fr.r,
    // the partials of p . A p -> fr.rPart (five-kernel step); otherwise the residual update of the four-kernel step.  Returns the workgroups.
    int spmvSt32(bool ap, const float* t, const float* xin, const FusedR& fr) const {
        const Plan p = planSt(3, false, 0, false, FusedR{});
        if (p.kernel != ELL2) throw Error("internal: single-precision St product without the two-unit kernel");
        noteWalk(ap ? 1 : 4, p);
        const ps::DevCSR& M = c->St;
        const uint8_t* uArg = c->uCoded ? (const uint8_t*)c->uCode.p : (const uint8_t*)c->uInv.p;
        withBool(c->uCoded, [&](auto UC) { withPolicy(p.pol, [&](auto POL) { withBool(ap, [&](auto AP) {
            ellLaunch(k_spmv_St_ell2<POL, false, false, false, double, false, UC, float, AP>, p, M, t, (int)M.cols, rowsSt, xin, done, p.nChunks, uArg, c->uDict.p, fr, (const int32_t*)nullptr);
        }); }); });
        return p.grid;
    }
    int spmvSt2c32(const float* t, const float* xin, float* out, double* partial, const ChebArgs& ca) const {   // returns the number of partials written
        const Plan p = planSt(2, false, 0, false, FusedR{});
        if (p.kernel != ELL2C) throw Error("internal: single-precision Chebyshev term without the two-unit St kernel");
        noteWalk(3, p);
        stEll2c(p, t, xin, out, partial, ca);
        return p.grid;
    }
    void spmvSt(int mode, const double* t, const double* xin, const double* add, double* out, double* partial, const ChebArgs* cheb = nullptr, const FusedR* fused = nullptr) const {
        ChebArgs ca{nullptr, nullptr, nullptr, 0., 0.};
        if (cheb) ca = *cheb;
        FusedR fr{};
        if (fused) fr = *fused;
        const Plan p = planSt(mode, stList, nStList, stOwnedOnly, fr);
        if (!p.run) return;
        if (p.err) throw Error(p.err);
        if (!stList) noteWalk(1 + mode, p);
        const ps::DevCSR& M = c->St;
        const uint8_t* uc = c->uCoded ? c->uCode.p : (const uint8_t*)nullptr;
        const uint8_t* uArg = c->uCoded ? (const uint8_t*)c->uCode.p : (const uint8_t*)c->uInv.p;
        using T = std::true_type; using F = std::false_type;
        using M3 = std::integral_constant<int, 3>;
        auto ell = [&](auto MODE, auto POL, auto FX, auto LIST) {
            ellLaunch(k_spmv_St_ell<MODE, POL, FX, LIST>, p, M, t, (int)M.cols, rowsSt, c->uInv.p, xin, add, out, partial, done, p.nChunks, p.xcd, ca, uc, c->uDict.p, fr, stList);
        };
        auto ell2 = [&](auto POL, auto CZ, auto DIST, auto LIST, auto TZ, auto HALO, auto UC) {
            ellLaunch(k_spmv_St_ell2<POL, CZ, DIST, LIST, typename decltype(TZ)::type, HALO, UC>, p, M, t, (int)M.cols, rowsSt, xin, done, p.nChunks, uArg, c->uDict.p, fr, stList);
        };
        auto pipe = [&](auto MODE, auto NV) { withPipe(M.packed, p.pol, [&](auto F64, auto POL) {
            hipLaunchKernelGGL((k_spmv_St_pipe<MODE, NV, F64, POL>), dim3(p.grid), dim3(BS), 0, c->stream, M.col16.p, M.code4.p, M.val4.p, (int)M.streamLen, M.winBase.p,
                               M.chunkInfo.p, M.len8.p, c->valScale, t, (int)M.cols, rowsSt, c->uInv.p, xin, add, out, partial, done, p.nChunks, p.xcd, ca, uc, c->uDict.p, fr);
        }); };
        if (p.kernel == CSR)
            withOneOf<0, 1>(mode, [&](auto MODE) { withBool(M.packed, [&](auto PK) {
                hipLaunchKernelGGL((k_spmv_St<MODE, 6, PK>), dim3(p.grid), dim3(BS), 0, c->stream, M.ptr.p, M.col.p, M.val.p, M.code.p, c->valScale, t, rowsSt, nP, c->uInv.p, xin, add, out, partial, done);
            }); });
        else if (p.kernel == ELL2C) stEll2c(p, t, xin, out, partial, ca);
        else if (p.kernel == ELL2Z) {
            auto z = [&](auto TZ) { withPolicy(p.pol, [&](auto POL) { withBool(c->uCoded, [&](auto UC) { ell2(POL, T{}, F{}, F{}, TZ, F{}, UC); }); }); };
            withZ(cz32, z);
        }
        else if (p.kernel == ELL2) withBool(c->uCoded, [&](auto UC) { withPolicy(p.pol, [&](auto POL) { ell2(POL, F{}, F{}, F{}, Type<double>{}, F{}, UC); }); });
        else if (p.kernel == ELL && p.fx == 3) withPolicy(p.pol, [&](auto POL) { withBool(stList, [&](auto LIST) { ell(M3{}, POL, M3{}, LIST); }); });
        else if (p.kernel == ELL2_OWN) withBool(c->uCoded, [&](auto UC) { withPolicy(p.pol, [&](auto POL) { ell2(POL, F{}, T{}, T{}, Type<double>{}, F{}, UC); }); });
        else if (p.kernel == ELL2_HALO)
            withBool(c->uCoded, [&](auto UC) { withPolicy(p.pol, [&](auto POL) { withBool(stList, [&](auto LIST) {
                ell2(POL, F{}, T{}, LIST, Type<double>{}, T{}, UC);
            }); }); });
        else if (p.kernel == ELL && p.fx == 5) withPolicy(p.pol, [&](auto POL) { ell(M3{}, POL, std::integral_constant<int, 5>{}, T{}); });
        else if (p.kernel == ELL && p.fx == 1)
            withPolicy(p.pol, [&](auto POL) { withBool(stList, [&](auto LIST) { ell(M3{}, POL, std::integral_constant<int, 1>{}, LIST); }); });
        else if (p.kernel == ELL)
            withOneOf<0, 1, 2, 3>(mode, [&](auto MODE) { withPolicy(p.pol, [&](auto POL) { withBool(stList, [&](auto LIST) {
                ell(MODE, POL, std::integral_constant<int, 0>{}, LIST);
            }); }); });
        else if (mode == 3) withOneOf<1, 2>(M.nv, [&](auto NV) { pipe(M3{}, NV); });   // PIPE
        else withOneOf<1, 2>(M.nv, [&](auto NV) { withOneOf<0, 1, 2>(mode, [&](auto MODE) { pipe(MODE, NV); }); });
    }

    // ---- grids
    // grid of a persistent kernel; the XCD-grouped walk needs a multiple of 8 blocks (workgroup b runs on XCD b & 7)
    // The fp64-value stream (10 B per entry) runs one chunk per workgroup: measured at 256^3 St 0.54 ms against 0.64 ms
    // persistent (the persistent walk pays when the stream is short and the loop is issue-bound, not when it is 3x heavier).
    int pipeBlocks(int nChunks, int& xcd, bool packed, int gridCap = 0) const {
        if (!packed) { xcd = 0; return nChunks; }
        int g = std::min(nChunks, gridCap > 0 ? gridCap : pipeGrid);
        if (xcd > 0) { if (g >= 8) g &= ~7; else xcd = 0; }
        // Balance (r06).  The two-unit kernels walk PAIRS of chunks, runs of 32 pairs per XCD: workgroup l of an XCD takes steps l, l + per, ... below
        // qEnd.  With a launch a little larger than its grid cap (a rank's 13.8 k chunks of S on 6144 workgroups) an eighth of the workgroups took
        // two steps and everybody waited for them: 59 us where two launches of half the chunks took 2 x 20.6.  Shrink the grid to the size at which every
        // workgroup takes the same number of steps (never above the cap; the 256^3 single domain keeps its 6144 / 1536: 9 / 36 steps each).
        if (xcd > 0 && g >= 8 && c->S.ellok && c->St.ellok) {
            const int qEnd = pairWalkEnd(nChunks);
            const int steps = std::max(1, (qEnd * 8 + g - 1) / g), per = (qEnd + steps - 1) / steps;
            if (per * 8 <= g) g = per * 8;
        }
        return g;
    }
    // The row-per-lane S kernel has no per-workgroup prologue and balances better on more, shorter workgroups — 256^3, same box:
    // 4096 workgroups 0.265 ms, 5120 0.260, 6144 0.257, 8192 0.258, 12288 0.250 (each is one more partial sum for every St workgroup to read)
    int sCap() const { return (ellOk(c->S) && pipeGrid == 4096) ? 6144 : 0; }
    // Workgroups of the St kernel.  With the residual update in its epilogue (mode 3) it runs best on 6 per CU — measured at 256^3,
    // rocprof average in a solve: 1280 / 1536 workgroups 415 us, 1792 489, 2048 445, 2560 / 3072 425, 4096 430 (and every workgroup
    // less is 10 K partial sums less to read in the prologue); S and the other St modes keep 16 per CU (S: 300 us at 4096, 324 at
    // 1536, 339 at 1024).  PS_PIPE_GRID_ST overrides.
    // Row-per-lane kernel, plain MODE 3: 7 per CU — 1536 workgroups 0.418 ms, 1792 0.403, 2048 0.515 (the eighth does not fit: a second round),
    // 3584 / 5376 as 1792.
    bool stDual() const { return dualT && plain3Hint && ellOk(c->St) && pipeGrid >= 1536; }
    int stGridFor(int mode) const {
        if (stGrid > 0) return stGrid;
        if (mode == 2 && stGrid2 > 0) return stGrid2;
        if (mode != 3 || pipeGrid < 1536) return 0;
        if (stDual()) return 1536;   // k_spmv_St_ell2: 80 VGPRs, six workgroups per CU
        return (plain3Hint && c->uCoded && c->St.ellok && c->St.packed && pipeGrid >= 1792) ? 1792 : 1536;
    }
};
// The lab switches of this layer, read once per process
struct LaunchSwitches {
    int pipeGrid = envInt(PS_ENV("PS_PIPE_GRID"), 4096);     // persistent pipelined kernels, 16 blocks per CU, by default; 0 = one-shot kernels
    int stGrid = envInt(PS_ENV("PS_PIPE_GRID_ST"), 0);
    int stGrid2 = envInt(PS_ENV("PS_PIPE_GRID_ST2"), 0);     // A/B: the Chebyshev term's launch alone
    // chunks per XCD run (rounded down to a power of two); 0: plain walk.  64: same kernel times as 4 / 16 / 256 on the row-per-lane kernels, a
    // fifth less HBM-side traffic than 16 (FETCH_SIZE of S 0.64 / 0.54 / 0.44 / 0.42 M KiB at 4 / 16 / 64 / 256)
    int xcd = envInt(PS_ENV("PS_XCD"), 64);
    // log2 of the consecutive chunks a workgroup takes in a row (ChunkWalk): 2 chunks on the row-per-lane kernels (256^3, same box: S 0.264 ->
    // 0.257 ms, St with the residual update 0.431 -> 0.408; 4 / 8 / 16 chunks: S 0.282 / 0.274 / 0.273, St 0.412 / 0.412 / 0.428)
    int wgRun = envInt(PS_ENV("PS_WG_RUN"), -1);
    bool dualS = envInt(PS_ENV("PS_S_DUAL"), 1) != 0;
    bool dualT = envInt(PS_ENV("PS_ST_DUAL"), 1) != 0;
    bool tileSplit = envInt(PS_ENV("PS_TILE_SPLIT"), 0) != 0;   // A/B: force the three-kernel form
    int tileTB = envInt(PS_ENV("PS_TILE_TB"), 0);
};
Launch mk(ps_context* c, const int* done) {
    static const LaunchSwitches sw;
    Launch L;
    L.c = c; L.done = done;
    L.rowsS = (int)c->nRows; L.rowsSt = (int)c->nSystem; L.nA = (int)c->nActiveVs; L.nP = (int)c->nPressures;
    L.pipeGrid = sw.pipeGrid;
    L.stGrid = sw.pipeGrid > 0 ? sw.stGrid : 0;
    L.stGrid2 = sw.stGrid2;
    L.xcdAware = sw.xcd > 0 ? sw.xcd : 0;
    const int run = sw.wgRun >= 0 ? sw.wgRun : ((c->S.ellok && c->St.ellok) ? 1 : 0);
    if (L.xcdAware > 0) L.xcdAware |= (run & 7) << 16;
    L.dualS = sw.dualS; L.dualT = sw.dualT; L.tileSplit = sw.tileSplit; L.tileTB = sw.tileTB;
    L.ntSpmv = c->ntLevel() >= 1;
    L.plain3Hint = c->P.preconditioner != PS_PRE_CHEBYSHEV && !c->slabEnabled;     // (the stress diagonal coded or not: the two-unit kernels take both, r06)
    L.plain3Hint2 = c->P.preconditioner == PS_PRE_CHEBYSHEV && !c->slabEnabled;
    L.walk = c->walkRecord ? c->launchWalkHost : nullptr;
    return L;
}
constexpr int64_t FUSED_STEP_MIN_ROWS = 1200000;   // see DomainSolve::chooseStepForm (r05: 2 M -> 1.2 M: the coil 128^3 of BASELINE config 2, 1.49 M rows, solves 3 % faster in four kernels — 10.55 against 10.86 ms,
                                                    // two rounds on one box; the 64^3 cavity, 0.8 M rows, stays faster in five: 57.3 against 58.8 us per iteration)
constexpr int64_t NT_LEVEL1_MIN_ROWS = 4000000, NT_LEVEL2_MIN_ROWS = 10000000;   // see ps_context::ntLevel
int dotBlocks(int64_t n) { return (int)std::min<int64_t>(VGRID, std::max<int64_t>(1, (n + BS - 1) / BS)); }
// entries of a partial-sums buffer over n DOFs (dotPartials, chebPartials): three sets of vector-kernel partials or one value per 256-row chunk, and the sums' slots
size_t partialsSize(int64_t n) { return (size_t)std::max<int64_t>(3 * VGRID, gridFor(std::max<int64_t>(n, 1), BS)) + 16; }
constexpr int CG_BATCH = 25;   // PCG iterations between two stop tests on the host (ps_context::solve, Dist::solve)
// The mixed-precision solve (ps_context::solve): a pass ends at the latest when r.r has fallen to MIXED_PASS_REDUCTION^2 of the true r.r it
// started from (fp32 carries 2^-24: about three digits are left for drift; profiles/mixed_precision.md), and there are at most MIXED_MAX_PASSES
constexpr double MIXED_PASS_REDUCTION = 1e-4;
constexpr int MIXED_MAX_PASSES = 8;

// More than 8192 partial sums (a one-shot kernel's: one per 256 rows) are first reduced to RED_BLOCKS sums in `red`.  Returns the sums to read, their count in cnt.
const double* reducedPartials(ps_context* c, const CGScalars* sc, const double* src, int count, double* red, int& cnt) {
    if (count > 8192) hipLaunchKernelGGL(k_reduce_partials, dim3(RED_BLOCKS), dim3(BS), 0, c->stream, sc, src, count, red);
    cnt = count > 8192 ? RED_BLOCKS : count;
    return count > 8192 ? red : src;
}
// A launch of BS-thread workgroups on the context's stream (DomainSolve::run and Dist), and the stress diagonal of the DOFs from `lo` on as the
// x, p update and k_uinv_pp take it
template <class K, class... A> void runOn(const ps_context* c, K kernel, int grid, A... a) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(BS), 0, c->stream, a...); }
StressDiag stressDiag(const ps_context* c, int64_t lo) { return {c->uCoded ? c->uCode.p + lo : nullptr, c->uDict.p, c->uInv.p + lo}; }
// a . b over n DOFs on the host: one scalar read-back per product (the BiCGStab fallback, Eigen's CG)
double hostDot(ps_context* c, const double* a, const double* b, int64_t n) {
    double out, *sum = c->dotPartials.p + 3 * VGRID;
    hipLaunchKernelGGL(k_dot, dim3(dotBlocks(n)), dim3(BS), 0, c->stream, a, b, n, c->dotPartials.p);
    hipLaunchKernelGGL(k_sumq, dim3(1), dim3(BS), 0, c->stream, (const CGScalars*)nullptr, c->dotPartials.p, dotBlocks(n), 0, 1, sum);
    HIP_CHECK(hipMemcpyAsync(&out, sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return out;
}
// the polynomial's result z (fp32 or fp64 values: chebInner32) as the fp64 vector dst — widened (dst is then another buffer), or copied unless it is there already
void zToF64(ps_context* c, double* dst, const double* z, int64_t n) {
    withZ(c->chebInner32, [&](auto TZ) {
        if constexpr (std::is_same<typename decltype(TZ)::type, float>::value) hipLaunchKernelGGL(k_widen_f32, dim3(dotBlocks(n)), dim3(BS), 0, c->stream, dst, (const float*)z, n);
        else if (dst != z) HIP_CHECK(hipMemcpyAsync(dst, z, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    });
}
// ---- FusedR (ps_kernels_spmv.hpp: the argument of the St kernel that carries the residual update) by what a site sets; the rest is null / zero.
// What forms the step's r.z: the stored Jacobi diagonal (null: the identity) OR the polynomial's first term, z_1 = dinvC r invTheta -> cz.  The
// builders below take ONE FusedZ, made by one of its two functions: no FusedR holds both.
struct FusedZ {
    const diag_t *dinvF = nullptr, *dinvC = nullptr; double invTheta = 0.; double* cz = nullptr;
    static FusedZ jacobi(const diag_t* dinvF) { FusedZ z; z.dinvF = dinvF; return z; }
    static FusedZ chebFirst(const diag_t* dinvC, double invTheta, double* cz) { FusedZ z; z.dinvC = dinvC; z.invTheta = invTheta; z.cz = cz; return z; }
};
// where the four producers of p.Ap and ||x||^2 left their partials: the S kernel, the tile kernel, uInv p^2 and x.x of the last x, p update
struct FusedPartials { const double* s; int sCount; const double* t; int tCount; const double* u; int uCount; const double* xx; int xxCount; };
// the single-domain step: the producers' partials; every row in [0, rows) is this domain's DOF
FusedR fusedSingle(CGScalars* sc, const FusedPartials& p, int it, double* r, double* rPart, int rows, const FusedZ& z) {
    FusedR f{};
    f.sc = sc; f.it = it; f.r = r; f.rPart = rPart; f.dinvF = z.dinvF; f.dinvC = z.dinvC; f.invTheta = z.invTheta; f.cz = z.cz;
    f.sPart = p.s; f.sCount = p.sCount; f.tPart = p.t; f.tCount = p.tCount; f.uPart = p.u; f.uCount = p.uCount; f.xxPart = p.xx; f.xxCount = p.xxCount; f.ownHi = rows;
    return f;
}
// a slab rank's step: red = the sums over the ranks instead of partials, its DOFs [ownLo, ownHi) of the rows, the halo rows' y -> yOut, the stride
// between the r.r and r.z partials of a step that runs as two launches
FusedR fusedSlab(CGScalars* sc, int it, double* r, double* rPart, const FusedZ& z, const double* red, int ownLo, int ownHi, double* yOut, int rStride) {
    FusedR f = fusedSingle(sc, FusedPartials{}, it, r, rPart, ownHi, z);
    f.red = red; f.ownLo = ownLo; f.yOut = yOut; f.rStride = rStride;
    return f;
}
// The batches of a PCG loop: iterations it .. min(budget, it + CG_BATCH) - 1 through step(it), then check(it - 1) — the stop test of the batch's last
// iteration — and the scalars read back; until they say done, the budget is used up or the interrupt callback asks (between batches only: sets
// ps_context::interrupted).  h0: the scalars as the caller holds them (returned as they are when the budget is empty).
struct BatchRun { int it; CGScalars h; bool interrupted; };
template <class Step, class Check> BatchRun runBatches(ps_context* c, CGScalars* sc, int budget, const CGScalars& h0, Step step, Check check) {
    BatchRun b{0, h0, false};
    for (bool finished = false; b.it < budget && !finished; ) {
        for (const int upto = std::min(budget, b.it + CG_BATCH); b.it < upto; ++b.it) step(b.it);
        check(b.it - 1);
        HIP_CHECK(hipMemcpyAsync(&b.h, sc, sizeof(b.h), hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        finished = b.h.done != 0;
        if (!finished && c->interruptCb && c->interruptCb(c->interruptUser)) { c->interrupted = b.interrupted = true; break; }
    }
    return b;
}

double chebRatio() { static const double r = PS_ENV("PS_CHEB_RATIO") ? atof(PS_ENV("PS_CHEB_RATIO")) : PS_CHEB_INTERVAL_RATIO; return r; }   // lmax / lmin (PS_CHEB_RATIO: experiments only — the oracle uses the constant)
// The Chebyshev iteration on [lmax / chebRatio(), lmax] (ps_context::chebyshevApply, Dist::chebyshevDist): z_1 = D^-1 r / theta, then
// next() gives c1, c2 of the terms 2..k in turn
struct ChebRecurrence {
    double theta, delta, sigma, rho;
    explicit ChebRecurrence(double lmax) {
        const double lmin = lmax / chebRatio();
        theta = 0.5 * (lmax + lmin); delta = 0.5 * (lmax - lmin); sigma = theta / delta; rho = 1. / sigma;
    }
    void next(double& c1, double& c2) {
        const double rhoN = 1. / (2. * sigma - rho);
        c1 = rhoN * rho; c2 = 2. * rhoN / delta;
        rho = rhoN;
    }
};

// lambda_max(D^-1 A) for the Chebyshev polynomial: 10 power iterations from the all-ones vector (`step` runs one), the Rayleigh
// quotient of the last iterate from the sums {v.v, v.w} (`sums` fills them on the host), then max(8.4, 1.25 * estimate) — same
// procedure as the oracle (ps_oracle_solve.cpp:estimateLambdaMax).
template <class Step, class Sums> double powerLambdaMax(Step step, Sums sums) {
    for (int it = 0; it < 10; ++it) step();
    double h[2] = {0., 0.};
    sums(h);
    const double lam = (h[0] > 0. && std::isfinite(h[1] / h[0])) ? h[1] / h[0] : 0.;   // A v = 0 on the way: the floor below
    return std::max(8.4, 1.25 * lam);
}

// bicgstab_external_matrix_A (pcg.h:134-200), restarted from zero (Solver.cpp:784-799): the host-driven fallback of both solves (rare
// path).  V names a vector: a device pointer, or a member of every rank's context (Dist::solve).  The caller supplies apply(in, out):
// out = A in; dot(a, b) on the host; lin(out, ca, a, cb, b, cc, c): out = ca a + cb b + cc c (b, c may be null); zero(v).
// Returns the iterations (maxit: not converged) and leaves the last relative error in `err`.
template <class V> struct BiCGVecs { V x, r, p, b, h, rhat, v, s, t, e; };
template <class V, class Apply, class Dot, class Lin, class Zero>
int bicgstab(const BiCGVecs<V>& w, int maxit, double tol, double& err, Apply apply, Dot dot, Lin lin, Zero zero) {
    zero(w.x);
    lin(w.r, 1., w.b, 0., nullptr, 0., nullptr);           // r = b - A*0
    lin(w.rhat, 1., w.r, 0., nullptr, 0., nullptr);
    zero(w.p); zero(w.v);
    double rhoCurr = 1., rhoOld = 1., alpha = 1., beta = 0., omega = 1., rre = 0.;
    int iters = maxit;
    for (int i = 0; i < maxit; ++i) {
        rhoOld = rhoCurr;
        rhoCurr = dot(w.rhat, w.r);
        beta = (rhoCurr / rhoOld) * (alpha / omega);
        lin(w.p, 1., w.r, beta, w.p, -beta * omega, w.v);  // p = r + beta (p - omega v)
        apply(w.p, w.v);
        alpha = rhoCurr / dot(w.rhat, w.v);
        lin(w.h, 1., w.x, alpha, w.p, 0., nullptr);        // h = x + alpha p
        lin(w.s, 1., w.r, -alpha, w.v, 0., nullptr);       // s = r - alpha v
        apply(w.s, w.t);
        omega = dot(w.t, w.s) / dot(w.t, w.t);
        lin(w.x, 1., w.h, omega, w.s, 0., nullptr);        // x = h + omega s
        const double xmag = std::sqrt(dot(w.x, w.x));
        apply(w.x, w.e);
        lin(w.e, 1., w.b, -1., w.e, 0., nullptr);          // err = b - A x
        const double rsnew = dot(w.e, w.e);
        rre = rsnew;
        if (std::sqrt(rsnew) / xmag < rre) rre = std::sqrt(rsnew) / xmag;
        if (rre < tol) { iters = i; break; }
        lin(w.r, 1., w.s, -omega, w.t, 0., nullptr);       // r = s - omega t
    }
    err = rre;
    return iters;
}
}  // namespace

// y = A x on device vectors (ApplyPressureStressMatrix::apply).  dotPartialsOut receives the per-block
// partials of x.y (gridFor(nSystem,256) entries).
void ps_context::applyOperator(const double* xdev, double* ydev, double* dotPartialsOut) {
    Launch L = mk(this, nullptr);
    L.spmvS(0, xdev, ts.p);
    L.tiles(0, ts.p);
    L.spmvSt(0, ts.p, xdev, nullptr, ydev, dotPartialsOut);
}

// AssembleSystem.cpp:432-470 (+ the reduced blocks of AssembleBlocks.cpp)
void ps_context::assembleSystemPressureStressFactored() {
    assembleReducedBlocks();
    applySurfaceTension();   // ps_surface.hip: the ghost-pressure impulse into rhsA / rhs_r (sigma = 0: nothing)
    const int64_t n = nSystem;
    ts.alloc((size_t)nRows + 1);
    vreg.alloc((size_t)std::max<int64_t>(1, regionCount) * PS_RD);
    wreg.alloc((size_t)std::max<int64_t>(1, nRChunks) * PS_RD);
    b.alloc((size_t)n); x.alloc((size_t)n); r.alloc((size_t)n); pvec.alloc((size_t)n); Ap.alloc((size_t)n);
    dotPartials.alloc(partialsSize(n));
    scal.alloc(1);
    dotPartials2.alloc(RED_BLOCKS);
    dotPartials3.alloc(VGRID);
    dotPartialsR.alloc(2 * VGRID);
    // t0 = McInv rhs_a on active rows, C (invDt BInv rhs_r) on reduced rows;  b = -S^T t0 + [rhs_p; rhs_tau]
    if (nActiveVs > 0)
        hipLaunchKernelGGL(k_mul<double>, dim3(dotBlocks(nActiveVs)), dim3(BS), 0, stream, ts.p, McInv.p, rhsA.p, nActiveVs);
    Launch L = mk(this, nullptr);
    L.tiles(2, ts.p);
    L.spmvSt(1, ts.p, nullptr, rhsPT.p, b.p, nullptr);
    HIP_CHECK(hipMemsetAsync(x.p, 0, (size_t)std::max<int64_t>(n, 1) * sizeof(double), stream));
}

// Preconditioners.cpp:4-9 (identity) / Jacobi extension
void ps_context::constructPreconditioner() {
    if (P.preconditioner != PS_PRE_DIAGONAL && P.preconditioner != PS_PRE_CHEBYSHEV && P.solverType != PS_EIGEN) return;   // Eigen's CG always runs its DiagonalPreconditioner
    dinv.alloc((size_t)nSystem);
    if (nSystem == 0) return;
    hipLaunchKernelGGL(k_jacobi_diag, dim3(gridFor(nSystem, 256)), dim3(256), 0, stream, St.ptr.p, St.col.p, (const double*)St.val.p, (const int8_t*)St.code.p, valScale, (int)nSystem,
                       (int)nPressures, (int)nActiveVs, dt, McInv.p, uInv.p, rrowFace.p, rrowRegion.p, COM.p, dx, make_int3(gOff[0], gOff[1], gOff[2]), Binv.p, dinv.p,
                       slabEnabled ? 0 : 1);
    // The PCG kernels read the diagonal in 16 bits (ps_common.hpp: diag_t — 2 instead of 8 bytes per DOF in both step kernels; fp32 until
    // r05).  Any diagonal of the operator's sign is a valid preconditioner; the Jacobi option itself is an extension (the reference's is a stub,
    // Preconditioners.cpp:37-41).  The fp64 array stays for export / tests / Eigen's CG / the interval estimate of the Chebyshev polynomial
    // (estimateLambdaMax: the power iteration runs on D64^-1 A while the polynomial applies D16^-1 A, whose entries differ by <= 2^-8: the
    // spectrum of D16^-1 A lies within (1 +- 0.004) of the other's, an order of magnitude inside the 1.25 x margin and the 8.4 floor of the
    // estimate — the oracle's estimate is on the fp64 diagonal too, so the two intervals agree to rounding); with a slab the conversion
    // follows the cross-rank completion of the diagonal (Dist::finishSetup).
    dinvF.alloc((size_t)nSystem);
    if (!slabEnabled) hipLaunchKernelGGL(k_to_diag, dim3(dotBlocks(nSystem)), dim3(BS), 0, stream, dinv.p, dinvF.p, nSystem);
    if (P.preconditioner == PS_PRE_CHEBYSHEV && !slabEnabled) estimateLambdaMax();   // with a slab: Dist::finishSetup, across the ranks
}

// Cache policy by system size (PS_NT_LEVEL = 0 / 1 / 2 forces): 2 = non-temporal streams in the SpMV kernels and the vector
// kernels (a 45 M-row iteration moves 6.7 GB: nothing survives to the next kernel, and keeping the once-per-launch streams out of
// the way of the gathers is worth 7 % of a step), 1 = in the SpMV kernels only, 0 = default policy everywhere (the working set of
// an iteration, ~150 B per row, fits the 256 MB memory-side cache or nearly: let it serve the next kernel).  Measured us per
// iteration at level 0 / 1 / 2 (cavity): 64^3 (0.8 M rows) 58.6 / 60.6 / 61.2; 96^3 (2.6 M) 97.9 / 104.8 / 103.4; 128^3 (5.9 M) 194.0 /
// 187.4 / 191.8; 160^3 (11.4 M) 341.7 / 337.7 / 336.0; 192^3 (19.4 M) 558 / 535 / 530; 224^3 (30.6 M) 858 / 838 / 810.
int ps_context::ntLevel() const {
    static const int env = envInt(PS_ENV("PS_NT_LEVEL"), -1);
    if (env >= 0) return env;
    const int64_t rows = std::max(nSystem, deviceShareRows);   // (ranks of an in-process group share the device's caches: ps_context::deviceShareRows)
    return rows < NT_LEVEL1_MIN_ROWS ? 0 : (rows < NT_LEVEL2_MIN_ROWS ? 1 : 2);
}

double ps_context::chebTheta() const { return ChebRecurrence(chebLmax).theta; }   // centre of the interval [lmax/250, lmax]

// lambda_max(D^-1 A) for the Chebyshev polynomial (powerLambdaMax).  The stencil part of A is a sum of rank-one face terms with <= 8
// entries, so its lambda_max(D^-1 A) <= 8 by Cauchy-Schwarz; the measurement covers the tile part.  10 applies at setup (~1 % of a 256^3 step).
void ps_context::estimateLambdaMax() {
    // The iterate is not normalised between steps (the quotient does not depend on its length and the spectrum lies in (0, ~8]: ten
    // steps grow it by < 1e10), so nothing comes back to the host until the end.
    const int64_t n = nSystem;
    chebLmax = 8.4;
    if (n == 0) return;
    const int vb = dotBlocks(n);
    tmp1.alloc((size_t)n); tmp2.alloc((size_t)n); tmp3.alloc((size_t)n);
    double* v = tmp1.p; double* w = tmp2.p; double* Av = tmp3.p;
    chebPartials.alloc(partialsSize(n));
    hipLaunchKernelGGL(k_fill_f64, dim3(vb), dim3(BS), 0, stream, v, 1., n);
    chebLmax = powerLambdaMax([&] {
        applyOperator(v, Av, dotPartials.p);
        hipLaunchKernelGGL(k_power_step, dim3(vb), dim3(BS), 0, stream, (const double*)v, (const double*)Av, (const double*)dinv.p, w, n, chebPartials.p);
        std::swap(v, w);
    }, [&](double* h) {
        hipLaunchKernelGGL(k_sumq, dim3(1), dim3(BS), 0, stream, (const CGScalars*)nullptr, (const double*)chebPartials.p, vb, 0, 1, chebPartials.p + 2 * vb);
        hipLaunchKernelGGL(k_sumq, dim3(1), dim3(BS), 0, stream, (const CGScalars*)nullptr, (const double*)chebPartials.p + vb, vb, 0, 1, chebPartials.p + 2 * vb + 1);
        HIP_CHECK(hipMemcpyAsync(h, chebPartials.p + 2 * vb, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    });
}

// z = q(D^-1 A) D^-1 r: k terms of the Chebyshev iteration on [lmax/250, lmax] (k-1 operator applies), see include/polystokes.h.
// Three-term form: z_1 = D^-1 r / theta, z_{j+1} = z_j + c1 (z_j - z_{j-1}) + c2 D^-1 (r - A z_j) — two buffers, zA and zB, taking turns
// (z_1 in zA, z_2 in zB, z_3 in zA, ...); *zOut is the one holding the final z.  Terms 2..k run as S, tiles and the St kernel with the
// update fused into its epilogue (MODE 2): per term it reads r, dinv, z_{j-1} besides its own operands and writes z_{j+1} over
// z_{j-1} — no separate vector pass.  rzPartial receives the partials of r.z of the final z (count returned); `sc` (may be null) lets
// the kernels of a converged solve exit early.
// firstDone: the caller already holds z_1 in zA (the St kernel of the four-kernel PCG step forms it on the rows it updates) — with
// a one-term polynomial nothing is launched and 0 is returned.
int ps_context::chebyshevApply(const double* rvec, double* zA, double* zB, double* rzPartial, const ps::CGScalars* sc, bool firstDone, double** zOut) {
    const int64_t n = nSystem;
    const int k = P.preconditionerDegree > 0 ? P.preconditionerDegree : 4;
    ChebRecurrence cr(chebLmax);
    const int vb = dotBlocks(n);
    const int* done = sc ? &sc->done : nullptr;
    Launch L = mk(this, done);
    // PS_PRE_CHEBYSHEV_F32 (chebInner32): the same recurrence with z_j (zA / zB) and the face-row vector of the inner applies (the first half
    // of ts) STORED as fp32; r, the diagonal, every product and sum fp64.  The two-units-per-wave kernels only (Launch::cheb32Ok decided chebInner32).
    if (!firstDone) withZ(chebInner32, [&](auto TZ) {
        using T = typename decltype(TZ)::type;
        hipLaunchKernelGGL(k_cheb_first<T>, dim3(vb), dim3(BS), 0, stream, sc, rvec, (const diag_t*)dinvF.p, 1. / cr.theta, (T*)zA, n, rzPartial);
    });
    int count = firstDone ? 0 : vb;
    double* cur = zA; double* other = zB;    // z_j, and the buffer of z_{j-1} that receives z_{j+1}
    for (int j = 1; j < k; ++j) {
        double c1, c2;
        cr.next(c1, c2);
        const double* zprev = j == 1 ? nullptr : other;            // z_0 = 0
        const ChebArgs ca{rvec, dinvF.p, zprev, c1, c2};             // (fp32: zprev points at floats, k_spmv_St_ell2c<.., float>)
        if (chebInner32) {
            float* tsF = (float*)ts.p;
            L.spmvS32((const float*)cur, tsF);
            L.tiles32(tsF);
            count = L.spmvSt2c32(tsF, (const float*)cur, (float*)other, rzPartial, ca);
        } else {
            L.spmvS(0, cur, ts.p);
            L.tiles(0, ts.p);
            if (L.stOnPipe()) {
                L.spmvSt(2, ts.p, cur, nullptr, other, rzPartial, &ca);
                count = L.stBlocks(2);   // the partials of the MODE 2 launch
            } else {
                tmp5.alloc((size_t)n);
                L.spmvSt(0, ts.p, cur, nullptr, tmp5.p, dotPartials2.p);
                hipLaunchKernelGGL(k_cheb_step, dim3(vb), dim3(BS), 0, stream, sc, rvec, (const diag_t*)dinvF.p, (const double*)tmp5.p, c1, c2, (const double*)cur, zprev, other, n, rzPartial);
                count = vb;
            }
        }
        std::swap(cur, other);
    }
    if (zOut) *zOut = cur;
    return count;
}

void ps_context::applyPreconditionerDevice(const double* rvec, double* z, double* scratch) {
    const int64_t n = nSystem;
    if (n == 0) return;
    const int vb = dotBlocks(n);
    if (P.preconditioner == PS_PRE_CHEBYSHEV) {
        chebPartials.alloc(partialsSize(n));
        double* zfin = z;
        chebInner32 = chebInner32Req && mk(this, nullptr).cheb32Ok();
        chebInner32Host = chebInner32 ? 1 : 0;   // (array "chebInner32")
        chebyshevApply(rvec, z, scratch, chebPartials.p, nullptr, false, &zfin);
        if (chebInner32) {      // the result is an fp32 vector in one of the two buffers: widen it through a third
            tmp5.alloc((size_t)n);
            zToF64(this, tmp5.p, zfin, n);
            HIP_CHECK(hipMemcpyAsync(z, tmp5.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        } else zToF64(this, z, zfin, n);
    } else if (P.preconditioner == PS_PRE_DIAGONAL) {
        hipLaunchKernelGGL(k_mul<diag_t>, dim3(vb), dim3(BS), 0, stream, z, (const diag_t*)dinvF.p, rvec, n);   // the diagonal as the PCG kernels read it
    } else {
        HIP_CHECK(hipMemcpyAsync(z, rvec, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
}

// ---------------------------------------------------------------------------------------------------
// The single-domain PCG solve in stages, named after Dist's (ps_dist.hpp: RankSolve, solveStart, chooseStepForm, fusedStart, the steps,
// bicgstabDist) where the job is the same; ps_context::solve below runs them in order.
namespace {
// The Krylov vectors of a Jacobi / identity step — the fp64 solve's x, p, r, A p and face-row vector, or a pass's fp32 ones with its correction d
// in x's place (ps_set_solve_precision; A p: the five-kernel step only) — and the vector kernels of their element type
template <class T> struct StepVecs { T *x, *p, *r, *Ap, *ts; };
template <class T> struct StepKernels { static constexpr auto updateR = k_cg_update_r; static constexpr auto updateXp = k_cg_update_xp; static constexpr auto updateXpU = k_cg_update_xp_u; };
template <> struct StepKernels<float> { static constexpr auto updateR = k_cg_update_r_f32; static constexpr auto updateXp = k_cg_update_xp_f32; static constexpr auto updateXpU = k_cg_update_xp_u_f32; };
// How the fp32 passes ended: the stop rule holds on the fp64 residual; a pass no longer halved it or the passes are used up (fp64 PCG goes on
// from this x); the iteration budget is used up (-> BiCGStab); the interrupt callback asked
enum class Passes { Converged, Stagnated, BudgetUsed, Interrupted };

struct DomainSolve {
    ps_context* c = nullptr;
    int64_t n = 0; double tol = 0.; int maxit = 0;
    int vb = 0, stBlocks = 0, stBF = 0, sBlocks = 0;              // workgroups: the vector kernels, St plain / with the residual update, S (four-kernel step)
    const diag_t* dv = nullptr; StressDiag ud{};                  // Jacobi: the stored diagonal; the stress diagonal, coded or fp64
    CGScalars *sc = nullptr, h{};                                 // the scalars on the device, and as last read back
    Launch L;
    bool cheb = false, fused = false, recording = false;
    double *fS = nullptr, *fT = nullptr, *fU = nullptr, *fR = nullptr;   // the four-kernel step's partials in fusedPart (fusedStart)
    double *zvec = nullptr, *dvec = nullptr, *rzPart = nullptr;   // the polynomial's two buffers and the r.z partials of its last term
    int itBase = 0;                                               // iterations the fp32 passes took: the fp64 loop gets the rest of the budget
    ~DomainSolve() { if (recording) c->walkRecord = false; }
    template <class K, class... A> void run(K kernel, int grid, A... a) const { runOn(c, kernel, grid, a...); }

    // Resets; false: there is nothing to iterate and rc is the solve's result (Eigen's CG ran, an unsupported solver, an empty system).
    // Otherwise the walks are being recorded, the launch dispatch stands and the polynomial has its buffers.
    bool solveStart(ps_context* ctx, int& rc) {
        c = ctx; n = c->nSystem; maxit = c->P.maxSolverIterations; tol = c->P.tolerance;
        c->usedBiCGStab = 0; c->interrupted = false; c->solvePrecisionUsedHost = 0; c->passIters.clear();
        if (c->P.solverType == PS_EIGEN) { rc = c->solveEigenCG(); return false; }
        if (c->P.solverType != PS_PCG_MATRIX_VECTOR_PRODUCTS) { c->err = "Unsupported Solver."; rc = PS_UNSUPPORTED_SOLVER; return false; }
        std::fill(std::begin(c->launchWalkHost), std::end(c->launchWalkHost), 0);
        if (n == 0) { c->solveIterations = 0; c->solveError = 0; rc = PS_SUCCESS; return false; }
        c->walkRecord = recording = true;
        cheb = c->P.preconditioner == PS_PRE_CHEBYSHEV;
        dv = (c->P.preconditioner == PS_PRE_DIAGONAL) ? c->dinvF.p : nullptr;
        vb = dotBlocks(n); sc = c->scal.p; ud = stressDiag(c, 0);
        L = mk(c, &sc->done);
        stBlocks = L.stBlocks(0); stBF = L.stBlocks(3);
        L.cz32 = c->chebInner32 = cheb && c->chebInner32Req && L.cheb32Ok();     // PS_PRE_CHEBYSHEV_F32 where the two-unit kernels run; fp64 inner vectors otherwise
        if (cheb) {
            c->tmp1.alloc((size_t)n); c->tmp2.alloc((size_t)n); c->chebPartials.alloc(partialsSize(n)); c->chebPartials2.alloc(RED_BLOCKS);
            zvec = c->tmp1.p; dvec = c->tmp2.p; rzPart = c->chebPartials.p;
        }
        return true;
    }
    // Fused step (default on the coded stream): p.Ap = -(sum_active s.t + sum_tiles w.v + 1/2 sum uInv p^2) is complete before the St kernel
    // starts, so that kernel forms alpha and updates r in its epilogue — A p is neither written nor read back (16 B per row less) and the step is
    // four launches (FusedR, ps_kernels_spmv.hpp).  Every St workgroup sums the partials of three producers in its prologue: a fixed cost per
    // iteration, which pays from 1.2 M rows (FUSED_STEP_MIN_ROWS; the figures and the rejected ticket reduction: docs/history.md).  PS_FUSED_R =
    // 0 / 1 forces it off / on (on only where the kernels exist).
    void chooseStepForm() {
        static const int fusedEnv = envInt(PS_ENV("PS_FUSED_R"), -1);
        fused = fusedEnv != 0 && (fusedEnv > 0 || n >= FUSED_STEP_MIN_ROWS) && L.fusedOk();
        c->fusedStepHost = fused ? 1 : 0;
    }
    void fusedStart() {   // the partials of the four-kernel step
        sBlocks = L.sBlocks();
        c->fusedPart.alloc((size_t)sBlocks + (size_t)c->regionCount + VGRID + 2 * (size_t)stBF + 16);
        L.sPart = fS = c->fusedPart.p; L.wvPart = fT = fS + sBlocks; fU = fT + c->regionCount; fR = fU + VGRID;
    }
    // r = b - A x (warm: x is the carried solution, pcg.h:284) or r = b, x = 0; z = M^-1 r, p = z, rsold = r.z; with the four-kernel step the first
    // direction's share of p.Ap on the diagonal
    void pcgStart(bool warm) {
        if (warm) {
            c->applyOperator(c->x.p, c->Ap.p, c->dotPartials.p);
            run(k_cg_init_warm, vb, c->b.p, c->Ap.p, dv, c->r.p, c->pvec.p, n, c->dotPartials.p);
        } else
            run(k_cg_init_f, vb, c->b.p, dv, c->x.p, c->r.p, c->pvec.p, n, c->dotPartials.p);
        if (cheb) {
            HIP_CHECK(hipMemsetAsync(sc, 0, sizeof(CGScalars), c->stream));   // `done` must read 0 inside the polynomial's kernels
            double* z0 = zvec;
            const int zCount = c->chebyshevApply(c->r.p, zvec, dvec, rzPart, nullptr, false, &z0);
            zToF64(c, c->pvec.p, z0, n);
            run(k_sumq, 1, nullptr, rzPart, zCount, 0, 1, c->dotPartials.p);
        }
        run(k_cg_scal0, 1, sc, c->dotPartials.p, cheb ? 1 : vb, tol, maxit, c->ntLevel() >= 2 ? 1 : 0);
        if (fused) run(k_uinv_pp, vb, c->pvec.p, ud, n, fU);
    }

    // ---- the steps.  (r of either element type goes through FusedR's double*.)
    StepVecs<double> v64() const { return {c->x.p, c->pvec.p, c->r.p, c->Ap.p, c->ts.p}; }
    TwoSums rrRz(const double* part, int cnt) const { return TwoSums::partials(part, cnt, dv ? part + cnt : nullptr, cnt); }   // a residual update's partials: r.r, then r.z (Jacobi)
    FusedR fusedArgs(int it, void* r, const FusedZ& z) const {
        return fusedSingle(sc, {fS, sBlocks, fT, (int)c->regionCount, fU, vb, c->dotPartials3.p, vb}, it, (double*)r, fR, (int)n, z);
    }
    template <class T> auto faceRows(const StepVecs<T>& v) const {   // ts = S p, the tiles' rows rewritten in place
        if constexpr (std::is_same<T, float>::value) { L.spmvS32(v.p, v.ts); L.tiles32(v.ts); }
        else { L.spmvS(0, v.p, v.ts); L.tiles(0, v.ts); }
    }
    // Four kernels: S, tiles, St with r -= alpha A p in its epilogue, then x, p (and the new p's share of p.Ap on the diagonal)
    template <class T> auto fourKernelStep(int it, const StepVecs<T>& v) const {
        faceRows(v);
        const FusedR fr = fusedArgs(it, v.r, FusedZ::jacobi(dv));
        if constexpr (std::is_same<T, float>::value) L.spmvSt32(false, v.ts, v.p, fr);
        else L.spmvSt(3, v.ts, v.p, nullptr, nullptr, nullptr, nullptr, &fr);
        run(StepKernels<T>::updateXpU, vb, sc, rrRz(fR, stBF), it, v.r, dv, v.x, v.p, n, c->dotPartials3.p, ud, fU);
    }
    // ... with the polynomial: the St kernel also forms its first term on the new r; then terms 2..k; then x, p
    void fourKernelChebStep(int it) {
        const StepVecs<double> v = v64();
        faceRows(v);
        const FusedR fr = fusedArgs(it, v.r, FusedZ::chebFirst(c->dinvF.p, 1. / c->chebTheta(), zvec));
        L.spmvSt(3, v.ts, v.p, nullptr, nullptr, nullptr, nullptr, &fr);
        double* zfin = zvec;
        const int zCount = c->chebyshevApply(v.r, zvec, dvec, rzPart, sc, true, &zfin);
        int cnt = stBF; const double* part = fR + stBF;         // a one-term polynomial: the St kernel's own r.z partials
        if (zCount > 0) part = reducedPartials(c, sc, rzPart, zCount, c->chebPartials2.p, cnt);
        withZ(c->chebInner32, [&](auto TZ) {
            using Z = typename decltype(TZ)::type;
            run(k_cg_update_xp_z_u<Z>, vb, sc, TwoSums::partials(fR, stBF, part, cnt), it, (const Z*)zfin, v.x, v.p, n, c->dotPartials3.p, ud, fU);
        });
    }
    // The first four kernels of the five-kernel step: A p (S, tiles, St with the partials of p.Ap), then r -= alpha A p
    template <class T> auto residualUpdate(int it, const StepVecs<T>& v) const {
        faceRows(v);
        int cnt = stBlocks;
        if constexpr (std::is_same<T, float>::value) {
            FusedR fr{}; fr.r = (double*)v.Ap; fr.rPart = c->dotPartials.p;
            cnt = L.spmvSt32(true, v.ts, v.p, fr);
        } else
            L.spmvSt(0, v.ts, v.p, nullptr, v.Ap, c->dotPartials.p);
        const double* part = reducedPartials(c, sc, c->dotPartials.p, cnt, c->dotPartials2.p, cnt);   // (the one-shot St kernel: a partial per 256 rows)
        run(StepKernels<T>::updateR, vb, sc, TwoSums::partials(part, cnt, c->dotPartials3.p, vb), it, v.Ap, dv, v.r, n, c->dotPartialsR.p);
    }
    template <class T> auto fiveKernelStep(int it, const StepVecs<T>& v) const {
        residualUpdate(it, v);
        run(StepKernels<T>::updateXp, vb, sc, rrRz(c->dotPartialsR.p, vb), it, v.r, dv, v.x, v.p, n, c->dotPartials3.p);
    }
    void fiveKernelChebStep(int it) {   // ... with the polynomial: z = M^-1 r between the residual update and x, p
        const StepVecs<double> v = v64();
        residualUpdate(it, v);
        double* zfin = zvec;
        const int zCount = c->chebyshevApply(v.r, zvec, dvec, rzPart, sc, false, &zfin);
        int cnt;
        const double* part = reducedPartials(c, sc, rzPart, zCount, c->chebPartials2.p, cnt);
        withZ(c->chebInner32, [&](auto TZ) {
            using Z = typename decltype(TZ)::type;
            run(k_cg_update_xp_z<Z>, vb, sc, TwoSums::partials(c->dotPartialsR.p, vb, part, cnt), it, (const Z*)zfin, v.x, v.p, n, c->dotPartials3.p);
        });
    }
    void step(int it) {   // one fp64 iteration
        if (cheb) { if (fused) fourKernelChebStep(it); else fiveKernelChebStep(it); }
        else if (fused) fourKernelStep(it, v64());
        else fiveKernelStep(it, v64());
    }

    // ---- mixed precision (ps_set_solve_precision; include/polystokes.h, DESIGN.md "Mixed-precision PCG"): x stays fp64; a pass runs the Jacobi /
    // identity step on fp32 vectors (d32 in x's place) for A d = b - A x, then x += d, and the stop rule is evaluated on the fp64 b - A x
    bool mixedAsked() const { return c->solvePrecisionSet == PS_PRECISION_MIXED && !cheb && !c->slabEnabled && L.mixedOk(); }
    // The true residual of the current x (fp64 operator, as k_cg_init_warm; haveX false: x = 0) rounded into the pass's r, p = z; its r.r and x.x —
    // the evaluation of the stop rule — into h
    void passStart(bool haveX) {
        if (haveX) c->applyOperator(c->x.p, c->Ap.p, c->dotPartials.p);
        run(k_cg_init_pass, vb, c->b.p, haveX ? c->Ap.p : nullptr, c->x.p, dv, c->d32.p, c->r32.p, c->p32.p, n, c->dotPartials.p);
        run(k_cg_scal0_pass, 1, sc, c->dotPartials.p, vb, tol, maxit, c->ntLevel() >= 2 ? 1 : 0, MIXED_PASS_REDUCTION * MIXED_PASS_REDUCTION, haveX ? 1 : 0);
        if (fused) run(k_uinv_pp_f32, vb, c->p32.p, ud, n, fU);
        HIP_CHECK(hipMemcpyAsync(&h, sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    // The passes.  solveError / trueResidualHost hold the last evaluation, solveIterations and itBase the iterations so far, passIters each pass's.
    Passes mixedPasses(bool warm) {
        c->solvePrecisionUsedHost = 1;
        c->d32.alloc((size_t)n); c->p32.alloc((size_t)n); c->r32.alloc((size_t)n); c->ts32.alloc((size_t)c->nRows + 1);
        if (!fused) c->Ap32.alloc((size_t)n);
        L.v32 = true;
        const StepVecs<float> v{c->d32.p, c->p32.p, c->r32.p, c->Ap32.p, c->ts32.p};
        auto toFp64 = [&](Passes how) { L.v32 = false; HIP_CHECK(hipMemsetAsync(c->dotPartials3.p, 0, VGRID * sizeof(double), c->stream)); return how; };   // the fp64 kernels take over
        double rrStart = 0.;
        for (int pass = 0; ; ++pass) {
            const bool haveX = warm || pass > 0;
            passStart(haveX);
            const double trueRR = h.rr;
            c->solveError = c->trueResidualHost = std::sqrt(h.rre);
            c->solveIterations = itBase;
            if (pass > 0 && h.rre < tol * tol) return Passes::Converged;
            if (h.done) {   // r = 0 exactly (b == 0: as the fp64 solve, x = 0)
                if (!haveX) HIP_CHECK(hipMemsetAsync(c->x.p, 0, (size_t)n * sizeof(double), c->stream));
                return Passes::Converged;
            }
            // stagnation: the pass did not halve the true ||r|| (the floor of fp32), or the passes are used up
            if (pass > 0 && (!(trueRR < 0.25 * rrStart) || pass == MIXED_MAX_PASSES)) return toFp64(Passes::Stagnated);
            if (itBase >= maxit) return toFp64(Passes::BudgetUsed);
            rrStart = trueRR;
            const BatchRun b = runBatches(c, sc, maxit - itBase, h, [&](int it) { if (fused) fourKernelStep(it, v); else fiveKernelStep(it, v); },
                                          [&](int last) { run(k_cg_check_pass, 1, sc, c->dotPartials3.p, vb, last); });
            h = b.h;
            c->passIters.push_back(h.done ? h.iter + 1 : b.it);   // the iterations whose update d holds
            c->solveIterations = itBase += c->passIters.back();
            if (b.interrupted) return Passes::Interrupted;
            run(k_cg_end_pass, vb, c->d32.p, c->x.p, n, haveX ? 0 : 1);
            if (!h.done) return toFp64(Passes::BudgetUsed);      // the budget ran out inside the pass
        }
    }
    int bicgstabFallback() {   // bicgstab (above), restarted from zero, on the factored operator: the solve's result
        c->usedBiCGStab = 1;
        c->tmp1.alloc((size_t)n); c->tmp2.alloc((size_t)n); c->tmp3.alloc((size_t)n); c->tmp4.alloc((size_t)n); c->tmp5.alloc((size_t)n);
        c->solveIterations = bicgstab(BiCGVecs<double*>{c->x.p, c->r.p, c->pvec.p, c->b.p, c->Ap.p, c->tmp1.p, c->tmp2.p, c->tmp3.p, c->tmp4.p, c->tmp5.p}, maxit, tol, c->solveError,
            [&](double* in, double* out) { c->applyOperator(in, out, c->dotPartials.p); },
            [&](const double* a, const double* bb) { return hostDot(c, a, bb, n); },
            [&](double* out, double ca, const double* a, double cb, const double* bb, double cc, const double* c3) { run(k_lin, vb, out, ca, a, cb, bb, cc, c3, n); },
            [&](double* v) { HIP_CHECK(hipMemsetAsync(v, 0, (size_t)n * sizeof(double), c->stream)); });
        return c->solveIterations == maxit ? PS_NOCONVERGE : PS_SUCCESS;
    }
};
}  // namespace

// Solver.cpp:734-812 solveSPDwithMatrixVectorPCG -> pcg_external_matrix_A (pcg.h:268-340), BiCGStab fallback (pcg.h:134-200)
int ps_context::solve() {
    DomainSolve s; int rc;
    if (!s.solveStart(this, rc)) return rc;
    s.chooseStepForm();
    if (s.fused) s.fusedStart();
    HIP_CHECK(hipMemsetAsync(dotPartials3.p, 0, VGRID * sizeof(double), stream));
    // warm start (ps_set_warm_start): x0 = the carried solution, r0 = b - A x0 (pcg.h:284); from here on the PCG is the same
    // (a Picard pass of ps_set_rheology starts from the last pass's solution the same way)
    bool warm = (warmMode == PS_WARM_PREVIOUS_STEP || rheoPass > 0) && gatherWarmStart();
    warmUsedHost = warm ? 1 : 0;
    if (s.mixedAsked())
        switch (s.mixedPasses(warm)) {
        case Passes::Converged: return PS_SUCCESS;
        case Passes::Interrupted: return PS_INCOMPLETE;
        case Passes::BudgetUsed: return s.bicgstabFallback();
        case Passes::Stagnated: solvePrecisionUsedHost = 2; warm = true;   // fp64 PCG from the passes' x, on the rest of the budget
        }
    s.pcgStart(warm);
    const BatchRun b = runBatches(this, s.sc, s.maxit - s.itBase, s.h, [&](int it) { s.step(it); },
                                  [&](int last) { s.run(k_cg_check, 1, s.sc, nullptr, dotPartials3.p, s.vb, last); });
    solveError = std::sqrt(b.h.rre);
    if (b.interrupted) { solveIterations = s.itBase + b.it; return PS_INCOMPLETE; }
    solveIterations = b.h.done ? s.itBase + b.h.iter : s.maxit;
    if (solvePrecisionUsedHost == 2) trueResidualHost = solveError;   // (the fp64 recurrence's value, as any fp64 solve reports)
    return solveIterations == s.maxit ? s.bicgstabFallback() : PS_SUCCESS;
}

// ---- warm start (ps_set_warm_start; DESIGN.md "Warm start") ----
namespace {
SolutionGrids solutionGrids(const ps_context* c, int q0, int nq, int64_t* most) {
    SolutionGrids G{};
    const int32_t* maps[7] = {c->sysIdx[0].p, c->sysIdxT[0].p, c->sysIdxT[1].p, c->sysIdxT[2].p, c->sysIdx[4].p, c->sysIdx[5].p, c->sysIdx[6].p};
    int64_t off = 0;
    *most = 1;
    for (int k = 0; k < nq; ++k) {
        G.map[k] = maps[q0 + k]; G.off[k] = off; G.cnt[k] = c->solutionGridCount(q0 + k);
        off += G.cnt[k];
        *most = std::max(*most, G.cnt[k]);
    }
    return G;
}
}  // namespace

void ps_context::scatterSolution(float* dst, int q0, int nq) {
    if (q0 < 0 || nq < 1 || q0 + nq > 7) throw Error("scatterSolution: bad grid range");
    int64_t most;
    const SolutionGrids G = solutionGrids(this, q0, nq, &most);
    hipLaunchKernelGGL(k_solution_scatter, dim3((unsigned)std::min<int64_t>(4096, gridFor(most, BS)), (unsigned)nq), dim3(BS), 0, stream, G,
                       (const double*)x.p, nSystem, dst);
}

// after a kept single-domain PCG step: x -> the store, tagged with the grid
void ps_context::carryWarmStart() {
    int64_t total = 0;
    for (int q = 0; q < 7; ++q) total += solutionGridCount(q);
    warmStore.alloc((size_t)total);
    scatterSolution(warmStore.p, 0, 7);
    warmHave = true;
    warmTag[0] = g.nx; warmTag[1] = g.ny; warmTag[2] = g.nz; warmTagDx = dx;
}

// before a PCG solve of a mode-1 context: x0 through this step's maps when the store was written on the same grid; warmX0 keeps it for
// the array "warmStartVector" (zeros when the solve starts cold).  Decompositions always start cold.
bool ps_context::gatherWarmStart() {
    const int64_t n = nSystem;
    warmX0.alloc((size_t)std::max<int64_t>(n, 1));
    warmX0Valid = true;
    const bool match = warmHave && !slabEnabled && warmTag[0] == g.nx && warmTag[1] == g.ny && warmTag[2] == g.nz && warmTagDx == dx;
    if (!match) {
        HIP_CHECK(hipMemsetAsync(warmX0.p, 0, (size_t)std::max<int64_t>(n, 1) * sizeof(double), stream));
        return false;
    }
    int64_t most;
    const SolutionGrids G = solutionGrids(this, 0, 7, &most);
    hipLaunchKernelGGL(k_warm_gather, dim3((unsigned)std::min<int64_t>(4096, gridFor(most, BS)), 7u), dim3(BS), 0, stream, G,
                       (const float*)warmStore.p, n, x.p, warmX0.p);
    return true;
}

void ps_context::dropWarmStart() {
    warmStore.free();
    warmX0.free();
    warmHave = false;
    warmX0Valid = false;
    arrays.erase("warmStartVector");
}

// initializeGuessVectors + constructGuessVectors (Solver.cpp:512-531) and the guessVector of the assemble functions
// (AssembleSystem.cpp:461-467):  pressureGuess = -G^T oldVs - JG^T cfit,  stressGuess = -2 uInv (-Dt^T oldVs - JDt^T cfit).
// With t = [oldVs ; C_f . cfit_region(f)] on the face rows this is one transposed product: g = -S^T t, stress part scaled.
void ps_context::constructGuessVectors() {
    const int64_t n = nSystem;
    guess.alloc((size_t)std::max<int64_t>(n, 1));
    HIP_CHECK(hipMemsetAsync(guess.p, 0, (size_t)std::max<int64_t>(n, 1) * sizeof(double), stream));
    if (!P.useWarmStart || n == 0 || slabEnabled) return;
    if (nActiveVs > 0) HIP_CHECK(hipMemcpyAsync(ts.p, oldVs.p, (size_t)nActiveVs * sizeof(double), hipMemcpyDeviceToDevice, stream));
    if (regionCount > 0 && nRChunks > 0)
        hipLaunchKernelGGL(k_tile_expand, dim3((unsigned)nRChunks), dim3(BS), 0, stream, rchunkRegion.p, rchunkStart.p, rchunkEnd.p, rrowFace.p,
                           COM.p, dx, make_int3(gOff[0], gOff[1], gOff[2]), cfit.p, ts.p + nActiveVs, (const int*)nullptr);
    Launch L = mk(this, nullptr);
    L.spmvSt(1, ts.p, nullptr, x.p, guess.p, nullptr);   // x is zero here (assemble): guess = -S^T t
    hipLaunchKernelGGL(k_guess_finish, dim3(dotBlocks(n)), dim3(BS), 0, stream, guess.p, uInv.p, permSys.p, nPressures, n);
}

// solveEigenCG (Solver.cpp:814-862): Eigen::ConjugateGradient<SparseMatrix, Lower|Upper> with its default diagonal
// preconditioner, solveWithGuess(b, guessVector) — extern/eigen/Eigen/src/IterativeLinearSolvers/ConjugateGradient.h:30-93,
// BasicPreconditioners.h:69-77 — run on the factored device operator instead of an assembled A (same A x; BASELINE config 1,
// a plumbing path: host-driven loop, one scalar read-back per dot product).  Stop rule ||r||^2 < tol^2 ||b||^2, returned
// count = completed iterations, error = ||r|| / ||b||, SUCCESS iff error <= tol (IterativeSolverBase::info()).
int ps_context::solveEigenCG() {
    const int64_t n = nSystem;
    const int maxit = P.maxSolverIterations;
    const double tol = P.tolerance;
    usedBiCGStab = 0;
    interrupted = false;
    if (slabEnabled) { err = "solverType EIGEN is a single-domain path"; return PS_UNSUPPORTED_SOLVER; }
    if (n == 0) { solveIterations = 0; solveError = 0; return PS_SUCCESS; }
    const int vb = dotBlocks(n);
    tmp1.alloc((size_t)n);
    double* z = tmp1.p;
    auto dotH = [&](const double* a, const double* bb) { return hostDot(this, a, bb, n); };
    auto lin = [&](double* out, double ca, const double* a, double cb, const double* bb) {
        hipLaunchKernelGGL(k_lin, dim3(vb), dim3(BS), 0, stream, out, ca, a, cb, bb, 0., (const double*)nullptr, n);
    };
    HIP_CHECK(hipMemcpyAsync(x.p, guess.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));   // solveWithGuess
    applyOperator(x.p, Ap.p, dotPartials.p);
    lin(r.p, 1., b.p, -1., Ap.p);                                   // residual = rhs - A x
    const double rhsNorm2 = dotH(b.p, b.p);
    if (rhsNorm2 == 0.) {
        HIP_CHECK(hipMemsetAsync(x.p, 0, (size_t)n * sizeof(double), stream));
        solveIterations = 0; solveError = 0.;
        return PS_SUCCESS;
    }
    const double threshold = std::max(tol * tol * rhsNorm2, std::numeric_limits<double>::min());
    double residualNorm2 = dotH(r.p, r.p);
    int i = 0;
    if (residualNorm2 >= threshold) {
        hipLaunchKernelGGL(k_mul<double>, dim3(vb), dim3(BS), 0, stream, pvec.p, dinv.p, r.p, n);   // p = precond.solve(residual)
        double absNew = dotH(r.p, pvec.p);
        while (i < maxit) {
            applyOperator(pvec.p, Ap.p, dotPartials.p);
            const double alpha = absNew / dotH(pvec.p, Ap.p);
            lin(x.p, 1., x.p, alpha, pvec.p);
            lin(r.p, 1., r.p, -alpha, Ap.p);
            residualNorm2 = dotH(r.p, r.p);
            if (residualNorm2 < threshold) break;
            hipLaunchKernelGGL(k_mul<double>, dim3(vb), dim3(BS), 0, stream, z, dinv.p, r.p, n);
            const double absOld = absNew;
            absNew = dotH(r.p, z);
            const double beta = absNew / absOld;
            lin(pvec.p, 1., z, beta, pvec.p);
            ++i;
            if ((i % 25) == 0 && interruptCb && interruptCb(interruptUser)) { interrupted = true; break; }
        }
    }
    solveIterations = i;
    solveError = std::sqrt(residualNorm2 / rhsNorm2);
    if (interrupted) return PS_INCOMPLETE;
    return solveError <= tol ? PS_SUCCESS : PS_NOCONVERGE;
}

// Solver.cpp:492-510
void ps_context::recoverVelocityFromPressureStress() {
    recovered.alloc((size_t)(nActiveVs + nReducedVs) + 1);
    Launch L = mk(this, nullptr);
    L.spmvS(1, x.p, ts.p);
    if (nActiveVs > 0)
        hipLaunchKernelGGL(k_recover_active, dim3(dotBlocks(nActiveVs)), dim3(BS), 0, stream, ts.p, McInv.p, rhsA.p, dt, invDt, nActiveVs, recovered.p);
    L.tiles(1, ts.p);
    if (regionCount > 0)
        HIP_CHECK(hipMemcpyAsync(recovered.p + nActiveVs, vreg.p, (size_t)nReducedVs * sizeof(double), hipMemcpyDeviceToDevice, stream));
}

// Solver.cpp:937-1028
void ps_context::applySolutionToVelocity() {
    for (int a = 0; a < 3; ++a) {
        const int64_t n = g.count(1 + a);
        hipLaunchKernelGGL(k_writeback, dim3(gridFor(n, BS)), dim3(BS), 0, stream, g, a, labels[1 + a].p, activeIdx[1 + a].p, reducedIdx[1 + a].p,
                           faceRow[a].p, recovered.p, recovered.p + nActiveVs, COM.p, dx, make_int3(gOff[0], gOff[1], gOff[2]), cvel[a].p, vel[a].p, velOut[a].p, 1);
    }
}

// micro-benchmark dispatch for ps_bench_kernel (bench.py roofline object)
void ps_bench_launch(ps_context* c, const std::string& k, const double* x, double* y) {
    Launch L = mk(c, nullptr);
    // "<name>_fp64": the pipelined kernels on the fp64-value form of the stream (16-bit windowed columns + fp64 values, 10 B per
    // entry: what runs when the stencil values are not code * scale);  "<name>_csr": the one-shot kernels on the plain CSR
    // (int32 columns + fp64 values, 12 B per entry: what runs when a chunk needs more than 16 column windows)
    auto endsWith = [&](const char* suf) { const size_t m = std::strlen(suf); return k.size() > m && k.compare(k.size() - m, m, suf) == 0; };
    const bool fp64 = endsWith("_fp64"), csr = endsWith("_csr");
    const std::string base = fp64 ? k.substr(0, k.size() - 5) : (csr ? k.substr(0, k.size() - 4) : k);
    const bool keepS = c->S.packed, keepT = c->St.packed, keepS16 = c->S.col16ok, keepT16 = c->St.col16ok;
    struct Restore { ps_context* c; bool a, b, d, e; ~Restore() { c->S.packed = a; c->St.packed = b; c->S.col16ok = d; c->St.col16ok = e; } } restore{c, keepS, keepT, keepS16, keepT16};
    if (fp64) {
        if (!c->S.col16ok || !c->St.col16ok) throw Error("no compressed stream on this system");
        c->buildVal4(c->S); c->buildVal4(c->St);
        c->S.packed = false; c->St.packed = false;
    }
    if (csr) { c->ensureValues(c->S); c->ensureValues(c->St); c->S.packed = c->St.packed = false; c->S.col16ok = c->St.col16ok = false; }
    if (base == "spmv_S") L.spmvS(0, x, c->ts.p);
    else if (base == "spmv_St") L.spmvSt(0, c->ts.p, x, nullptr, y, c->dotPartials.p);
    else if (base == "apply") c->applyOperator(x, y, c->dotPartials.p);
    else if (base == "tiles") L.tiles(0, c->ts.p);
    else if (base == "cg_update_r" || base == "cg_update_xp" || base == "cg_update_xp_u" || base == "spmv_St_r") {
        // streaming vector kernels on scratch vectors (alpha = beta = 0 keeps them finite over many launches)
        ps::DevBuf<CGScalars>& scratch = c->benchScal;
        scratch.alloc(1);
        CGScalars h{};
        h.tol2 = -1.;                                  // the stop test never fires
        h.vecNT = c->ntLevel() >= 2 ? 1 : 0;
        if (base == "cg_update_xp" || base == "cg_update_xp_u") h.rsold2[0] = 1.;   // beta = 0 / 1 ; (cg_update_r, spmv_St_r: alpha = 0 / p.Ap with p.Ap = +-1024 below)
        HIP_CHECK(hipMemcpyAsync(scratch.p, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
        ps::DevBuf<double>& ones = c->benchOnes;       // input partials of the fused scalar prologues
        if (ones.n < (size_t)2 * VGRID) {
            ones.alloc((size_t)2 * VGRID);
            std::vector<double> hv((size_t)2 * VGRID, 1.);
            HIP_CHECK(hipMemcpyAsync(ones.p, hv.data(), hv.size() * 8, hipMemcpyHostToDevice, c->stream));   // (the context's stream is non-blocking: nothing
            HIP_CHECK(hipStreamSynchronize(c->stream));                                                      //  orders it behind the legacy stream; hv dies here)
        }
        ps::DevBuf<double>& zeros = c->benchZeros;
        if (zeros.n < (size_t)2 * VGRID) { zeros.alloc((size_t)2 * VGRID); HIP_CHECK(hipMemsetAsync(zeros.p, 0, (size_t)2 * VGRID * 8, c->stream)); }
        const int64_t n = c->nSystem;
        const int vb = dotBlocks(n);
        const diag_t* dvf = c->P.preconditioner == PS_PRE_DIAGONAL ? c->dinvF.p : nullptr;
        c->tmp4.alloc((size_t)n); c->tmp5.alloc((size_t)n);
        c->dotPartials.alloc((size_t)std::max(3 * std::max(vb, VGRID), 2 * L.stBlocks()) + 16);
        const TwoSums rrRz = TwoSums::partials(zeros.p, VGRID, dvf ? zeros.p + VGRID : nullptr, VGRID);
        if (base == "spmv_St_r") {   // the St kernel of the four-kernel step: r (scratch) -= 0 * A x in the epilogue
            if (!L.fusedOk()) throw Error("no fused step on this system");
            const FusedR fr = fusedSingle(scratch.p, {ones.p, VGRID, zeros.p, 0, zeros.p, 0, ones.p, 0}, 0, c->tmp5.p, c->dotPartials.p, (int)n, FusedZ::jacobi(dvf));
            L.spmvSt(3, c->ts.p, x, nullptr, nullptr, nullptr, nullptr, &fr);
        }
        else if (base == "cg_update_xp_u")
            runOn(c, k_cg_update_xp_u, vb, scratch.p, rrRz, 0, x, dvf, c->tmp4.p, c->tmp5.p, n, c->dotPartials.p, stressDiag(c, 0), c->dotPartials.p + VGRID);
        else if (base == "cg_update_r")
            runOn(c, k_cg_update_r, vb, scratch.p, TwoSums::partials(ones.p, VGRID, ones.p, 0), 0, y, dvf, c->tmp5.p, n, c->dotPartials.p);
        else
            runOn(c, k_cg_update_xp, vb, scratch.p, rrRz, 0, x, dvf, c->tmp4.p, c->tmp5.p, n, c->dotPartials.p);
    }
    else throw Error("unknown kernel name: " + k);
}

#include "ps_dist.hpp"
#include "ps_import.hpp"
