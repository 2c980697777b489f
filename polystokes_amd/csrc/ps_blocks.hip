// Stencil assembly: one thread per face / cell / edge writes CSR rows directly (row length <= 8,
// so fixed slots -> count -> scan -> fill; no triplet lists, no sort).
// Reference: exec/HDK_PolyStokesSolver_ConstructMatrixBlocks.cpp:9-292 (sizes, compile), :294-868 (sweeps).
//
// Layout decision: the reference materialises JG = J^T Ghat and JDt = J^T Dhat (26 nnz per
// touched DOF per reduced face, :454-455,:524-525,:612-613).  Here only the ordinary stencils Ghat, Dhat
// of the reduced faces are stored, as extra rows of one matrix
//        S = [ G   Dt  ]   rows 0..nA-1      active faces (X,Y,Z by active index, Solver.h:628-642)
//            [ Ghat Dhat ]  rows nA..nRows-1  reduced faces with >=1 entry, region-contiguous
// and the basis row C_f (J) is evaluated on the fly in the tile kernels.  St = S^T is built by gather
// from the DOF side (deterministic, no atomics).
#include "ps_context.hpp"
#include "ps_setup_util.hpp"

using namespace ps;

namespace {

constexpr int BS = SETUP_BS;

struct BlockArgs {
    Grid g;
    double invDx;
    const float* lw[7];
    const float* fw[7];
    const int32_t* lab[7];
    const int32_t* act[7];
    const int32_t* reg[7];
    const int32_t* sys[7];     // internal system numbering (sysIdx)
    const int32_t* sysT[3];    // cell -> txx / tyy / tzz (sysIdxT)
    const int32_t* faceRow[3];
    const float* vel[3];
    const float* cvel[3];
    CellField visc;               // ps_context::viscSource
    FaceDensity dens;             // ps_context::densSource
    int64_t nP, nA, faceOff[3];
    Own own;
    const int32_t* regionOwned;   // null: all owned
    double valScale;              // invDx / 64
    int32_t* codeFail;            // set to 1 if some value is not code * valScale
    int freeSlip;                 // PS_SOLID_FREE_SLIP: an active edge with fluid weight < 1 has no stress (ps_set_solid_boundary)
    int32_t* slipEdges;           // free slip: the count pass adds such edges here (array "solidSlipEdges")
};

// Free slip drops the coupling of the edge stress at `el` of edge grid `ea`: it is cut by a solid (the `edgeSolidish` test of
// edgeColumnT).  Its entries in S and St are stored as explicit zeros and its rhs is 0; uInv keeps its value, so tau_e = 0 exactly.
// The zeros keep the pattern of no-slip: a reduced face can touch such an edge (a tile two cells from a curved solid), and dropping
// the entry would change the skin rows' length classes and hence their numbering (k_skin); no row or column becomes empty either.
__device__ inline bool slipEdge(const BlockArgs& A, int ea, int64_t el) { return A.freeSlip && A.fw[4 + ea][el] < 1.f; }

__device__ inline int8_t encodeVal(const BlockArgs& A, double v) {
    const double q = v / A.valScale;
    const double r = rint(q);
    if (!(fabs(r) <= 127.) || r * A.valScale != v) { *A.codeFail = 1; return 0; }
    return (int8_t)(int)r;
}

// The stencil row of one face in the reference's slot order: p(dir0,dir1), tau_c(dir0,dir1),
// tau_e(edgeAxis asc, dir0,dir1).  ConstructMatrixBlocks.cpp:394-421 (G), :466-491 (Dt centres), :553-579 (Dt edges).
// Entries of the row of face f: every candidate has its own slot (pressure of the two cells 0-1, their centre stress 2-3, the edge
// stresses 4-7), absent ones hold the sentinel column.  Static slots and a sorting network keep the two arrays in registers — with
// `cols[n++] = ...` and an insertion sort they lived in scratch memory (112 B per thread in k_S_fill).
constexpr int32_t NO_COL = 0x7fffffff;
template <int AXIS>
__device__ inline int faceEntriesT(const BlockArgs& A, const int3 f, int32_t (&cols)[8], double (&vals)[8]) {
    const int3 cd = A.g.dims(0);
    const int3 fd = A.g.dims(1 + AXIS);
    const double wF = (double)A.fw[1 + AXIS][lin3(fd, f.x, f.y, f.z)];
#pragma unroll
    for (int k = 0; k < 8; ++k) { cols[k] = NO_COL; vals[k] = 0.; }
    int n = 0;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const double sign = dir == 0 ? -1. : 1.;
        int3 c = f;
        addc(c, AXIS, dir - 1);
        if (comp(c, AXIS) < 0 || comp(c, AXIS) >= comp(cd, AXIS)) continue;
        const int64_t cl = lin3(cd, c.x, c.y, c.z);
        const double coeff = wF * (double)A.lw[0][cl] * A.invDx;
        if (coeff <= 0.) continue;
        const int pidx = A.sys[0][cl];   // internal index of this cell's pressure (>= 0 iff the cell is ACTIVE)
        if (pidx >= 0) { cols[dir] = pidx; vals[dir] = sign * coeff; ++n; }                                     // pressure
        if (isActiveL(A.lab[0][cl])) { cols[2 + dir] = A.sysT[AXIS][cl]; vals[2 + dir] = -1. * sign * coeff; ++n; }   // centre stress
    }
    // edge stresses
    constexpr int EA0 = AXIS == 0 ? 1 : 0, EA1 = AXIS == 2 ? 1 : 2;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const int ea = w == 0 ? EA0 : EA1;
        const int3 ed = A.g.dims(4 + ea);
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const double sign = dir == 0 ? -1. : 1.;
            int3 e = f;
            addc(e, 3 - AXIS - ea, dir);
            const int64_t el = lin3(ed, e.x, e.y, e.z);
            if (!isActiveL(A.lab[4 + ea][el])) continue;
            const double coeff = wF * (double)A.lw[4 + ea][el] * A.invDx;
            if (coeff <= 0.) continue;
            cols[4 + 2 * w + dir] = A.sys[4 + ea][el]; vals[4 + 2 * w + dir] = slipEdge(A, ea, el) ? 0. : -1. * sign * coeff; ++n;
        }
    }
    return n;
}
__device__ inline int faceEntries(const BlockArgs& A, int axis, const int3 f, int32_t (&cols)[8], double (&vals)[8]) {
    return axis == 0 ? faceEntriesT<0>(A, f, cols, vals) : (axis == 1 ? faceEntriesT<1>(A, f, cols, vals) : faceEntriesT<2>(A, f, cols, vals));
}
// ascending by column, sentinels last: Batcher's odd-even merge sort for 8 keys (19 compare-exchanges, all indices static)
__device__ inline void sortEntries(int32_t (&cols)[8], double (&vals)[8]) {
#define PS_CSWAP(i, j) { const bool sw = cols[i] > cols[j]; const int32_t ci = cols[i], cj = cols[j]; const double vi = vals[i], vj = vals[j]; \
                         cols[i] = sw ? cj : ci; cols[j] = sw ? ci : cj; vals[i] = sw ? vj : vi; vals[j] = sw ? vi : vj; }
    PS_CSWAP(0, 1) PS_CSWAP(2, 3) PS_CSWAP(4, 5) PS_CSWAP(6, 7)
    PS_CSWAP(0, 2) PS_CSWAP(1, 3) PS_CSWAP(4, 6) PS_CSWAP(5, 7)
    PS_CSWAP(1, 2) PS_CSWAP(5, 6)
    PS_CSWAP(0, 4) PS_CSWAP(1, 5) PS_CSWAP(2, 6) PS_CSWAP(3, 7)
    PS_CSWAP(2, 4) PS_CSWAP(3, 5)
    PS_CSWAP(1, 2) PS_CSWAP(3, 4) PS_CSWAP(5, 6)
#undef PS_CSWAP
}

// reduced faces with >= 1 stencil entry, enumerated per region through its face box (same work items
// as the dense reductions): count, then ordered assignment of rows nA + k.
// number of stencil entries of the reduced face (axis, i, j, k) of region r; 0: not a skin face
__device__ inline int skinFaceLen(const BlockArgs& A, int axis, int r, int i, int j, int k) {
    const int3 fd = A.g.dims(1 + axis);
    if (oob3(fd, i, j, k)) return 0;
    const int64_t c = lin3(fd, i, j, k);
    if (A.reg[1 + axis][c] != r || A.lab[1 + axis][c] != PS_REDUCED) return 0;
    int32_t cols[8];
    double vals[8];
    return faceEntries(A, axis, make_int3(i, j, k), cols, vals);
}
// blockExclusiveScan (ps_setup_util.hpp) for six 10-bit counters packed in 64 bits (each thread contributes 0 or 1 per counter: <= 256 per block)
__device__ inline unsigned long long blockScanExclPacked(unsigned long long v, unsigned long long* total) {
    __shared__ unsigned long long waveSums64[BS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned lo = __shfl_up((unsigned)(incl & 0xffffffffull), o, 64), hi = __shfl_up((unsigned)(incl >> 32), o, 64);
        if (lane >= o) incl += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 63) waveSums64[w] = incl;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < BS / 64; ++i) { if (i < w) base += waveSums64[i]; tot += waveSums64[i]; }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}
// Skin rows (reduced faces with >= 1 stencil entry) of one work item = <= FB_CHUNK positions of a region's union face box.
// ASSIGN = false counts them.  ASSIGN = true numbers them nA + (item offset) + ..., ordered by (length class, axis, position
// x-fastest): first the LONG rows (> 2 entries: the faces normal to the tile's surface, 6 entries), then the SHORT ones (tangential
// faces that touch the tile's surface with an edge: 1-2 entries), each class axis by axis.  Rows of one class and axis have the
// same shape: a 64-row unit of the row-per-lane SpMV (DevCSR::ecol) is then padded by almost nothing (in (position, axis) order
// every unit held a 6-entry row and was padded to 6: half its slots empty), and consecutive rows address consecutive DOFs of one
// kind.  itemLong[item] = number of long rows (the stream build cuts its chunks there).
constexpr int SKIN_LONG_MIN = 3;
template <bool ASSIGN>
__global__ void __launch_bounds__(BS) k_skin(BlockArgs A, const int32_t* __restrict__ bbox, const int32_t* __restrict__ itemRegion,
                                             const int32_t* __restrict__ itemStart, int32_t* __restrict__ itemCount, int32_t* __restrict__ faceRow0,
                                             int32_t* __restrict__ faceRow1, int32_t* __restrict__ faceRow2, uint32_t* __restrict__ rrowFace,
                                             int32_t* __restrict__ rrowRegion, int32_t* __restrict__ itemLong) {
    __shared__ unsigned char codes[ASSIGN ? FB_CHUNK : 1];   // per position: 2 bits per axis (0 none, 1 short, 2 long)
    const int item = blockIdx.x;
    const int r = itemRegion[item], start = itemStart[item];
    if (A.regionOwned && !A.regionOwned[r]) {   // tile of another rank (halo): no rows here
        if (!ASSIGN && threadIdx.x == 0) itemCount[item] = 0;
        if (ASSIGN && threadIdx.x == 0) itemLong[item] = 0;
        return;
    }
    const RegionBox box = RegionBox::faceUnion(bbox, r);
    const int end = min(start + FB_CHUNK, (int)box.total());
    // pass 1: classify every position; totals per (class, axis) category — category = (long ? 0 : 3) + axis
    unsigned long long mine = 0;
    for (int base = start; base < end; base += BS) {
        const int pos = base + threadIdx.x;
        if (pos < end) {
            const int3 q = box.at(pos);
            const int i = q.x, j = q.y, k = q.z;
            int code = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int n = skinFaceLen(A, a, r, i, j, k);
                if (n > 0) { const bool lg = n >= SKIN_LONG_MIN; code |= (lg ? 2 : 1) << (2 * a); mine += 1ull << (10 * ((lg ? 0 : 3) + a)); }
            }
            if (ASSIGN) codes[pos - start] = (unsigned char)code;
        }
    }
    // (`mine`: per-thread counts, <= FB_CHUNK / BS = 16 per category)
    int catBase[6] = {0, 0, 0, 0, 0, 0};
    if (ASSIGN) {
        // item totals per category from the batches (each batch total <= 256 per category)
        int itemTot[6] = {0, 0, 0, 0, 0, 0};
        for (int base = start; base < end; base += BS) {
            const int pos = base + threadIdx.x;
            unsigned long long v = 0;
            if (pos < end) {
                const int code = codes[pos - start];
#pragma unroll
                for (int a = 0; a < 3; ++a) { const int q = (code >> (2 * a)) & 3; if (q) v += 1ull << (10 * ((q == 2 ? 0 : 3) + a)); }
            }
            unsigned long long bt;
            blockScanExclPacked(v, &bt);
#pragma unroll
            for (int c = 0; c < 6; ++c) itemTot[c] += (int)((bt >> (10 * c)) & 1023ull);
        }
        int run = itemCount[item];                 // exclusive offset of this item (after the scan over the items)
#pragma unroll
        for (int c = 0; c < 6; ++c) { catBase[c] = run; run += itemTot[c]; }
        if (threadIdx.x == 0) itemLong[item] = itemTot[0] + itemTot[1] + itemTot[2];
        // pass 2: number the rows
        for (int base = start; base < end; base += BS) {
            const int pos = base + threadIdx.x;
            unsigned long long v = 0;
            int code = 0;
            if (pos < end) {
                code = codes[pos - start];
#pragma unroll
                for (int a = 0; a < 3; ++a) { const int q = (code >> (2 * a)) & 3; if (q) v += 1ull << (10 * ((q == 2 ? 0 : 3) + a)); }
            }
            unsigned long long bt;
            const unsigned long long off = blockScanExclPacked(v, &bt);
            if (code) {
                const int3 at = box.at(pos);
                const int i = at.x, j = at.y, k = at.z;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int q = (code >> (2 * a)) & 3;
                    if (!q) continue;
                    const int c = (q == 2 ? 0 : 3) + a;
                    const int rr = catBase[c] + (int)((off >> (10 * c)) & 1023ull);
                    int32_t* faceRow = a == 0 ? faceRow0 : (a == 1 ? faceRow1 : faceRow2);
                    faceRow[lin3(A.g.dims(1 + a), i, j, k)] = (int32_t)(A.nA + rr);
                    rrowFace[rr] = packFace(i, j, k, a);
                    rrowRegion[rr] = r;
                }
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) catBase[c] += (int)((bt >> (10 * c)) & 1023ull);
        }
    } else {
        // count only: total number of skin faces of the item
        int n = 0;
        unsigned long long m = mine;
#pragma unroll
        for (int c = 0; c < 6; ++c) { n += (int)(m & 1023ull); m >>= 10; }
        int totalRows;
        blockExclusiveScan(n, &totalRows);
        if (threadIdx.x == 0) itemCount[item] = totalRows;
    }
}

__global__ void k_S_count(BlockArgs A, int axis, int32_t* __restrict__ rowCount) {
    const int3 d = A.g.dims(1 + axis);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int row = A.faceRow[axis][c];
    if (row < 0) return;
    int32_t cols[8];
    double vals[8];
    rowCount[row] = faceEntries(A, axis, unlin3(d, c), cols, vals);
}
// fill S; for active rows also the diagonal mass terms and rhs (ConstructMatrixBlocks.cpp:362-391)
__global__ void k_S_fill(BlockArgs A, int axis, const int32_t* __restrict__ ptr, int32_t* __restrict__ col, double* __restrict__ val,
                         int8_t* __restrict__ code, double* __restrict__ McInv, double* __restrict__ rhsA, double* __restrict__ Mc, double* __restrict__ oldVs) {
    const int3 d = A.g.dims(1 + axis);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int row = A.faceRow[axis][c];
    if (row < 0) return;
    int32_t cols[8];
    double vals[8];
    const int n = faceEntries(A, axis, unlin3(d, c), cols, vals);
    sortEntries(cols, vals);
    const int p0 = ptr[row];
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (q < n) { col[p0 + q] = cols[q]; if (val) val[p0 + q] = vals[q]; code[p0 + q] = encodeVal(A, vals[q]); }
    if (row < A.nA) {
        double volume = (double)A.fw[1 + axis][c] * (double)A.lw[1 + axis][c];
        const double lo = 0.1 * 0.1;   // MINWEIGHT * MINWEIGHT, :365
        volume = volume < lo ? lo : (volume > 1.0 ? 1.0 : volume);
        const double u = (double)A.vel[axis][c];
        const int3 q = unlin3(d, c);
        const double rho = A.dens.at(A.g, axis, q.x, q.y, q.z);
        McInv[row] = 1. / (volume * rho);
        rhsA[row] = u * volume * rho;
        if (Mc) Mc[row] = volume * rho;
        if (oldVs) oldVs[row] = u;
    }
}

// ---- transpose by gather -----------------------------------------------------------------------
struct StEntry { int32_t row; double val; };

// entries of column j = pressure of cell c (mode 0) or centre stress (cell c, axis a) (mode 1+a)
__device__ inline int cellColumn(const BlockArgs& A, int mode, const int3 c, int32_t* rows, double* vals, double* rhsOut) {
    const int3 cd = A.g.dims(0);
    const int64_t cl = lin3(cd, c.x, c.y, c.z);
    const double wLc = (double)A.lw[0][cl];
    const bool cellSolidish = A.fw[0][cl] < 1.f;
    int n = 0;
    double rhs = 0.;
    const int a0 = mode == 0 ? 0 : mode - 1, a1 = mode == 0 ? 2 : mode - 1;
    for (int a = a0; a <= a1; ++a) {
        const int3 fd = A.g.dims(1 + a);
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            int3 f = c;
            addc(f, a, d);
            const int64_t fl = lin3(fd, f.x, f.y, f.z);
            const int row = A.faceRow[a][fl];
            if (row < 0) continue;
            const double sign = (1 - d) == 0 ? -1. : 1.;   // this cell is faceToCellMap(face, a, 1-d)
            const float wFf = A.fw[1 + a][fl];
            const double coeff = (double)wFf * wLc * A.invDx;
            if (coeff <= 0.) continue;
            rows[n] = row;
            vals[n] = mode == 0 ? sign * coeff : -1. * sign * coeff;
            ++n;
            if (row < A.nA) {   // solid-boundary rhs terms, :424-441 / :494-511 (solidCoeff unused; literal)
                const double sc = sign * coeff;
                const double svel = (double)A.cvel[a][fl];
                if (cellSolidish) rhs += -1. * sc * svel;
                if (wFf < 1.f) rhs += sc * svel;
            }
        }
    }
    *rhsOut = rhs;
    return n;
}
// entries of column tau_e: static slots (two faces per other axis), sentinel rows for the absent ones (see faceEntriesT)
template <int EA>
__device__ inline int edgeColumnT(const BlockArgs& A, const int3 e, int32_t (&rows)[4], double (&vals)[4], double* rhsOut) {
    const int3 ed = A.g.dims(4 + EA);
    const int64_t el = lin3(ed, e.x, e.y, e.z);
    const double wLe = (double)A.lw[4 + EA][el];
    const bool edgeSolidish = A.fw[4 + EA][el] < 1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { rows[k] = NO_COL; vals[k] = 0.; }
    int n = 0;
    double rhs = 0.;
    const bool slip = slipEdge(A, EA, el);   // free slip: zero values, rhs 0
    constexpr int FA0 = EA == 0 ? 1 : 0, FA1 = EA == 2 ? 1 : 2;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const int fa = w == 0 ? FA0 : FA1;
        const int third = 3 - fa - EA;
        const int3 fd = A.g.dims(1 + fa);
#pragma unroll
        for (int divDir = 0; divDir < 2; ++divDir) {
            int3 f = e;
            addc(f, third, -divDir);   // faceToEdgeMap(face, fa, ea, divDir) == e
            if (oob3(fd, f.x, f.y, f.z)) continue;
            const int64_t fl = lin3(fd, f.x, f.y, f.z);
            const int row = A.faceRow[fa][fl];
            if (row < 0) continue;
            const double sign = divDir == 0 ? -1. : 1.;
            const float wFf = A.fw[1 + fa][fl];
            const double coeff = (double)wFf * wLe * A.invDx;
            if (coeff <= 0.) continue;
            rows[2 * w + divDir] = row; vals[2 * w + divDir] = slip ? 0. : -1. * sign * coeff; ++n;
            if (row < A.nA && !slip) {   // :582-599
                const double sc = sign * coeff;
                const double svel = (double)A.cvel[fa][fl];
                if (edgeSolidish) rhs += -1. * sc * svel;
                if (wFf < 1.f) rhs += sc * svel;
            }
        }
    }
    *rhsOut = rhs;
    return n;
}
__device__ inline int edgeColumn(const BlockArgs& A, int ea, const int3 e, int32_t (&rows)[4], double (&vals)[4], double* rhsOut) {
    return ea == 0 ? edgeColumnT<0>(A, e, rows, vals, rhsOut) : (ea == 1 ? edgeColumnT<1>(A, e, rows, vals, rhsOut) : edgeColumnT<2>(A, e, rows, vals, rhsOut));
}
__device__ inline void sortRows4(int32_t (&rows)[4], double (&vals)[4]) {   // ascending, sentinels last (5 compare-exchanges)
#define PS_CSWAP(i, j) { const bool sw = rows[i] > rows[j]; const int32_t ci = rows[i], cj = rows[j]; const double vi = vals[i], vj = vals[j]; \
                         rows[i] = sw ? cj : ci; rows[j] = sw ? ci : cj; vals[i] = sw ? vj : vi; vals[j] = sw ? vi : vj; }
    PS_CSWAP(0, 1) PS_CSWAP(2, 3) PS_CSWAP(0, 2) PS_CSWAP(1, 3) PS_CSWAP(1, 2)
#undef PS_CSWAP
}

__device__ inline double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ inline void sortRows(int n, int32_t* rows, double* vals) {
    for (int i = 1; i < n; ++i) {
        const int32_t c = rows[i];
        const double v = vals[i];
        int j = i - 1;
        while (j >= 0 && rows[j] > c) { rows[j + 1] = rows[j]; vals[j + 1] = vals[j]; --j; }
        rows[j + 1] = c; vals[j + 1] = v;
    }
}

// cells: columns p, tau_xx, tau_yy, tau_zz.  FILL=false counts, FILL=true writes St rows, rhs_p/rhs_tau
// and the stress diagonals uInv (/u) (ConstructMatrixBlocks.cpp:737-867).
template <bool FILL>
__global__ void k_St_cells(BlockArgs A, int32_t* __restrict__ cnt, const int32_t* __restrict__ ptr, int32_t* __restrict__ col,
                           double* __restrict__ val, int8_t* __restrict__ code, double* __restrict__ rhsPT, double* __restrict__ uInv, double* __restrict__ uDiag) {
    const int3 d = A.g.dims(0);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int idx = A.sys[0][c];   // internal index of p; txx, tyy, tzz: sysT
    if (idx < 0) return;
    const int3 q = unlin3(d, c);
    int32_t rows[6];
    double vals[6];
    double uinvv = 0., uv = 0.;
    if (FILL) {
        const double vw = clampd((double)A.fw[0][c], 0.1, 1.0) * (double)A.lw[0][c];
        const double visc = (double)A.visc.sample(A.g, (float)q.x + 0.5f, (float)q.y + 0.5f, (float)q.z + 0.5f);
        const double invVisc = clampd(1. / visc, 0., 1.e10);
        uinvv = invVisc * clampd(vw, 1.e-2, 1.);
        uv = visc * clampd(1. / vw, 0., 1.e2);
        if (!A.own.cell(q.x, q.y, q.z)) uinvv = 0.;   // the -1/2 uInv x term belongs to the owner of the DOF
    }
    for (int mode = 0; mode < 4; ++mode) {
        double rhs;
        const int n = cellColumn(A, mode, q, rows, vals, &rhs);
        const int64_t j = mode == 0 ? idx : A.sysT[mode - 1][c];
        if (!FILL) { cnt[j] = n; continue; }
        sortRows(n, rows, vals);
        const int p0 = ptr[j];
        for (int k = 0; k < n; ++k) { col[p0 + k] = rows[k]; if (val) val[p0 + k] = vals[k]; code[p0 + k] = encodeVal(A, vals[k]); }
        rhsPT[j] = rhs;
        uInv[j] = mode > 0 ? uinvv : 0.;      // full-length diagonal, zero on pressure rows
        if (uDiag) uDiag[j] = mode > 0 ? uv : 0.;
    }
}
// edges: column tau_e (ConstructMatrixBlocks.cpp:651-735 for the diagonal)
template <bool FILL>
__global__ void k_St_edges(BlockArgs A, int ea, int32_t* __restrict__ cnt, const int32_t* __restrict__ ptr, int32_t* __restrict__ col,
                           double* __restrict__ val, int8_t* __restrict__ code, double* __restrict__ rhsPT, double* __restrict__ uInv, double* __restrict__ uDiag) {
    const int3 d = A.g.dims(4 + ea);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    if (!isActiveL(A.lab[4 + ea][c])) return;
    const int3 q = unlin3(d, c);
    int32_t rows[4];
    double vals[4];
    double rhs;
    const int n = edgeColumn(A, ea, q, rows, vals, &rhs);
    const int64_t j = A.sys[4 + ea][c];
    const int64_t t = j;
    if (!FILL) {
        cnt[j] = n;
        if (slipEdge(A, ea, c)) atomicAdd(A.slipEdges, 1);
        return;
    }
    sortRows4(rows, vals);
    const int p0 = ptr[j];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) { col[p0 + k] = rows[k]; if (val) val[p0 + k] = vals[k]; code[p0 + k] = encodeVal(A, vals[k]); }
    rhsPT[j] = rhs;
    const double vw = clampd((double)A.fw[4 + ea][c], 0.1, 1.0) * (double)A.lw[4 + ea][c];
    const float ox = ea == 0 ? 0.5f : 0.f, oy = ea == 1 ? 0.5f : 0.f, oz = ea == 2 ? 0.5f : 0.f;
    const double visc = (double)A.visc.sample(A.g, (float)q.x + ox, (float)q.y + oy, (float)q.z + oz);
    const double invVisc = clampd(1. / visc, 0., 1e10);
    uInv[t] = A.own.sample(4 + ea, q.x, q.y, q.z) ? 2. * invVisc * vw : 0.;
    if (uDiag) uDiag[t] = 0.5 * visc * clampd(1. / vw, 0., 1.e2);
}

BlockArgs makeArgs(ps_context* c) {
    BlockArgs A;
    A.g = c->g; A.invDx = c->invDx;
    for (int s = 0; s < 7; ++s) {
        A.lw[s] = c->liquidW[s].p; A.fw[s] = c->fluidW[s].p;
        A.lab[s] = c->labels[s].p; A.act[s] = c->activeIdx[s].p; A.reg[s] = c->reducedIdx[s].p; A.sys[s] = c->sysIdx[s].p;
    }
    for (int a = 0; a < 3; ++a) { A.faceRow[a] = c->faceRow[a].p; A.vel[a] = c->vel[a].p; A.cvel[a] = c->cvel[a].p; A.sysT[a] = c->sysIdxT[a].p; }
    A.visc = c->viscSource(); A.dens = c->densSource();
    A.nP = c->nPressures; A.nA = c->nActiveVs;
    A.faceOff[0] = 0; A.faceOff[1] = c->nFace[0]; A.faceOff[2] = c->nFace[0] + c->nFace[1];
    A.own = c->own();
    A.valScale = c->valScale;
    A.codeFail = c->counters.p + CTR_CODE_FAIL;
    A.regionOwned = (c->slabEnabled && c->regionCount > 0) ? c->regionOwned.p : nullptr;
    A.freeSlip = c->solidBoundaryUsed == PS_SOLID_FREE_SLIP ? 1 : 0;
    A.slipEdges = A.freeSlip ? c->slipEdges.p : nullptr;
    return A;
}

// Compressed SpMV stream, step 1: entries per chunk rounded up to a multiple of 4 (scanned into the chunk starts)
__global__ void k_chunk_len4(const int32_t* __restrict__ ptr, const int2* __restrict__ chunkRows, int nChunks, int32_t* __restrict__ len4, int32_t* __restrict__ maxLen) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch > nChunks) return;
    int n = 0;
    if (ch < nChunks) { const int2 cr = chunkRows[ch]; n = ptr[cr.x + cr.y] - ptr[cr.x]; atomicMax(maxLen, n); }
    len4[ch] = (n + 3) & ~3;
}
// step 2, one block per chunk: 16-bit windowed columns.  Greedy cover of the chunk's column set by windows
// [base, base + 4096): base = smallest column not yet covered (block min), at most 16 windows; a chunk that needs more
// raises *fail and the SpMVs keep the 32-bit CSR.  The block-interleaved numbering keeps the columns of a chunk in a
// handful of short runs (own voxels, the j/k neighbours, the 6 neighbouring blocks, skin rows of adjacent tiles), so 16
// windows are plenty.  Also copies the value codes to the aligned layout and writes the row-length bytes.
// One WAVE per chunk (four chunks per workgroup), 32 entries per lane in registers: the greedy cover needs a minimum over the chunk per
// window, which a wave forms without a barrier (the one-workgroup-per-chunk form spent its time in three barriers per window: 0.97 ms
// per matrix at 256^3, now 0.45).
__global__ void __launch_bounds__(BS) k_col16_build(const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, const int8_t* __restrict__ code,
                                                    const int2* __restrict__ chunkRows, const int32_t* __restrict__ start4, uint16_t* __restrict__ col16,
                                                    int8_t* __restrict__ code4, int32_t* __restrict__ winBase, int4* __restrict__ chunkInfo,
                                                    uint8_t* __restrict__ len8, int32_t* __restrict__ fail, int32_t* __restrict__ chunkRep, int nChunks) {
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * (BS / 64) + (int)(threadIdx.x >> 6);
    if (chunk >= nChunks) return;
    if (lane == 0) chunkRep[chunk] = chunk;                         // owner of the chunk's run (k_chunk_share redirects)
    const int2 cr = chunkRows[chunk];
    const int r0 = cr.x;
    const int p0 = ptr[r0], p1 = ptr[r0 + cr.y];
    const int q0 = start4[chunk], q1 = start4[chunk + 1];          // q1 - q0 = (p1 - p0) rounded up to 4
    if (lane == 0) chunkInfo[chunk] = make_int4(q0, (p1 - p0) | (cr.y << 16), cr.x, cr.x);   // (run begin, entries | rows << 16, first row, row source)
    for (int i = lane; i < cr.y; i += 64) len8[r0 + i] = (uint8_t)(ptr[r0 + i + 1] - ptr[r0 + i]);
    constexpr int SL = 32;                              // <= 8 entries per row: <= 2048 entries per chunk
    if (p1 - p0 > SL * 64) { if (lane == 0) *fail = 1; return; }
    int c[SL];
    unsigned open = 0u;
#pragma unroll
    for (int u = 0; u < SL; ++u) {
        const int i = lane + u * 64;
        const bool o = p0 + i < p1;
        c[u] = o ? col[p0 + i] : 0x7fffffff;
        if (o) open |= 1u << u;
        if (q0 + i < q1) { code4[q0 + i] = o ? code[p0 + i] : (int8_t)0; if (!o) col16[q0 + i] = 0; }   // incl. the padding
    }
    int used = 16;
    for (int w = 0; w < 16; ++w) {
        int m = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < SL; ++u) if ((open >> u) & 1u) m = min(m, c[u]);
        for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
        const int base = m;                             // wave-uniform
        if (base == 0x7fffffff) { used = w; break; }    // nothing left, the remaining windows get base 0
        if (lane == 0) winBase[(int64_t)chunk * 16 + w] = base;
#pragma unroll
        for (int u = 0; u < SL; ++u)
            if (((open >> u) & 1u) && c[u] - base < 4096) {
                col16[q0 + lane + u * 64] = (uint16_t)((w << 12) | (c[u] - base));
                open &= ~(1u << u);
            }
    }
    if (lane == 0) for (int w = used; w < 16; ++w) winBase[(int64_t)chunk * 16 + w] = 0;
    if (open) *fail = 1;
}
// ---- shared runs (DevCSR::chunkInfo) -----------------------------------------------------------------------------------
// A chunk's payload = its aligned run of (col16, code4) entries and the length bytes of its rows.  Equivalent lattice blocks
// (same pattern of active cells, same neighbourhood) produce byte-identical payloads — columns are window-relative, the window
// bases stay per chunk — so every chunk whose payload equals an earlier chunk's is pointed at that chunk's run: the kernels then
// stream one copy of each distinct run and find it in cache.  (1) a 64-bit hash per payload, (2) a device hash table keeps the
// smallest chunk index per hash, (3) every other chunk compares its bytes with that representative's and, if equal, takes its run.
__global__ void __launch_bounds__(64) k_chunk_hash(const int4* __restrict__ chunkInfo, const uint16_t* __restrict__ col16, const int8_t* __restrict__ code4,
                                                   const uint8_t* __restrict__ len8, unsigned long long* __restrict__ hash, int weak) {
    const int chunk = blockIdx.x;
    const int4 ci = chunkInfo[chunk];
    const int n4 = ((ci.y & 0xffff) + 3) & ~3, rows = (int)((unsigned)ci.y >> 16);
    unsigned long long h = 0;
    if (!weak)                                                      // weak (test switch): lengths only — different payloads collide, the byte compare decides
    for (int i = threadIdx.x; i < n4; i += 64)                      // position-keyed terms: the sum does not depend on the order
        h += mix64(((unsigned long long)i << 32) | ((unsigned long long)col16[ci.x + i] << 8) | (uint8_t)code4[ci.x + i]);
    if (!weak)
    for (int i = threadIdx.x; i < rows; i += 64) h += mix64(0x4000000000000000ull | ((unsigned long long)i << 32) | len8[ci.z + i]);
    for (int o = 32; o > 0; o >>= 1) h += __shfl_down(h, o, 64);
    if (threadIdx.x == 0) {
        h = mix64(h ^ (((unsigned long long)(unsigned)n4 << 32) | (unsigned)rows));
        hash[chunk] = h == HASH_EMPTY ? 0ull : h;
    }
}
__global__ void k_chunk_rep_insert(const unsigned long long* __restrict__ hash, int nChunks, unsigned long long* __restrict__ keys, int32_t* __restrict__ vals, unsigned mask) {
    const int chunk = blockIdx.x * blockDim.x + threadIdx.x;
    if (chunk >= nChunks) return;
    const unsigned long long h = hash[chunk];
    hashInsertMin(keys, vals, mask, (unsigned)(h >> 17) & mask, h, chunk);
}
// one workgroup per chunk: look the representative up, compare the payloads, redirect the run and the row-byte source.
// rowCode (may be null): the value-set codes of the kernel's diagonal (uCode per DOF; mcCode per ACTIVE face row, codeRows of them):
// read per row like the length bytes, so they have to agree too for the rows that have one.
__global__ void __launch_bounds__(64) k_chunk_share(const unsigned long long* __restrict__ hash, const unsigned long long* __restrict__ keys, const int32_t* __restrict__ vals,
                                                    unsigned mask, int4* __restrict__ chunkInfo, const uint16_t* __restrict__ col16, const int8_t* __restrict__ code4,
                                                    const uint8_t* __restrict__ len8, const uint8_t* __restrict__ rowCode, int codeRows,
                                                    unsigned long long* __restrict__ uniqueLen, int32_t* __restrict__ chunkRep) {
    const int chunk = blockIdx.x;
    const unsigned long long h = hash[chunk];
    unsigned slot = (unsigned)(h >> 17) & mask;
    while (keys[slot] != h) slot = (slot + 1) & mask;                // present: inserted by k_chunk_rep_insert
    const int rep = vals[slot];
    const int4 ci = chunkInfo[chunk];
    const int n = ci.y & 0xffff, n4 = (n + 3) & ~3, rows = (int)((unsigned)ci.y >> 16);
    bool same = rep != chunk;
    if (same) {
        const int4 cr = chunkInfo[rep];                              // a representative's entry is never rewritten (it is its own)
        same = cr.y == ci.y;
        if (same) {
            for (int i = threadIdx.x; i < n4; i += 64) same = same && col16[ci.x + i] == col16[cr.x + i] && code4[ci.x + i] == code4[cr.x + i];
            for (int i = threadIdx.x; i < rows; i += 64) {
                same = same && len8[ci.z + i] == len8[cr.z + i];
                if (rowCode) {
                    const bool a = ci.z + i < codeRows, b = cr.z + i < codeRows;
                    same = same && a == b && (!a || rowCode[ci.z + i] == rowCode[cr.z + i]);
                }
            }
        }
        same = __all(same) != 0;
        if (same && threadIdx.x == 0) { chunkInfo[chunk].x = cr.x; chunkInfo[chunk].w = cr.z; chunkRep[chunk] = rep; }
    }
    if (!same && threadIdx.x == 0) atomicAdd(uniqueLen, (unsigned long long)n4);
}
// the fp64 values of a matrix in the aligned chunk layout of its compressed stream (padding entries 0)
__global__ void __launch_bounds__(BS) k_val4_build(const int32_t* __restrict__ ptr, const double* __restrict__ val,
                                                   const int4* __restrict__ chunkInfo, double* __restrict__ val4) {
    const int chunk = blockIdx.x;
    const int4 ci = chunkInfo[chunk];
    const int p0 = ptr[ci.z], n = ci.y & 0xffff, q0 = ci.x;
    const int n4 = (n + 3) & ~3;
    for (int i = threadIdx.x; i < n4; i += BS) val4[q0 + i] = i < n ? val[p0 + i] : 0.;
}
// ---- row-per-lane form of the stream (DevCSR::ecol ...) ---------------------------------------------------------------
// A re-layout of the windowed stream above (same columns, same window bases, same codes): chunk -> four units of 64 rows, a unit
// padded to the (even) length W of its longest row, lane-major.  Only chunks that own their run get one (shared chunks point at
// their owner's: chunkRep), so a periodic tile structure stores a few MB.
__device__ inline int ellCodeWidth(int W) { return W > 4 ? 8 : (W > 0 ? 4 : 0); }
constexpr int32_t ELL_NULL_BASE = 0x1ffff000;   // (base + 12-bit offset) * 8 >= 0xffff8000: beyond any vector the kernels address (buildEll checks)
// plan, one block per chunk: unit widths -> sizes of the chunk's column / code runs (0 for a chunk that shares its owner's)
__global__ void __launch_bounds__(BS) k_ell_plan(const int4* __restrict__ chunkInfo, const uint8_t* __restrict__ len8, const int32_t* __restrict__ chunkRep,
                                                 int32_t* __restrict__ colLen, int32_t* __restrict__ codeLen, int32_t* __restrict__ wpack, int32_t* __restrict__ fail) {
    __shared__ int wmax[BS / 64];
    const int chunk = blockIdx.x;
    const int4 ci = chunkInfo[chunk];
    const int rows = (int)((unsigned)ci.y >> 16);
    int len = (int)threadIdx.x < rows ? (int)len8[ci.z + threadIdx.x] : 0;
    for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_down(len, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = len;
    __syncthreads();
    if (threadIdx.x == 0) {
        int cl = 0, vl = 0, wp = 0;
        for (int u = 0; u < BS / 64; ++u) {
            const int W = (wmax[u] + 1) & ~1;
            if (W > 8) *fail = 1;
            cl += 64 * W; vl += 64 * ellCodeWidth(W); wp |= (W & 15) << (4 * u);
        }
        const bool own = chunkRep[chunk] == chunk;
        colLen[chunk] = own ? cl : 0; codeLen[chunk] = own ? vl : 0; wpack[chunk] = wp;
    }
}
// fill, one block per chunk (thread = row): lane l of unit u writes its row's entries; slots past the end of the row hold value
// code 0 and address window 15 — which the chunk does not use (its base is still 0: windows are assigned in ascending order of
// their bases) and now gets a base beyond every vector (ELL_NULL_BASE): the gather is out of the buffer's range, returns 0 and
// costs no cache lookup; a chunk that does use 16 windows repeats the row's last column instead (a hit in the line the previous
// slot touched; the product is +-0).  Lanes past the chunk's last row repeat the last row (their results are never stored).
// Every chunk writes its record.
__global__ void __launch_bounds__(BS) k_ell_fill(const int4* __restrict__ chunkInfo, const uint8_t* __restrict__ len8, const int32_t* __restrict__ chunkRep,
                                                 const uint16_t* __restrict__ col16, const int8_t* __restrict__ code4, const int32_t* __restrict__ colBegin,
                                                 const int32_t* __restrict__ codeBegin, const int32_t* __restrict__ wpack, uint16_t* __restrict__ ecol,
                                                 int8_t* __restrict__ ecode, int4* __restrict__ echunk, int32_t* __restrict__ winBase) {
    const int chunk = blockIdx.x;
    const int rep = chunkRep[chunk];
    const bool nullOk = winBase[chunk * 16 + 15] == 0 || winBase[chunk * 16 + 15] == ELL_NULL_BASE;   // (same verdict for a chunk and the owner of its run: same window codes)
    __syncthreads();
    if (nullOk && threadIdx.x == 0) winBase[chunk * 16 + 15] = ELL_NULL_BASE;
    const int4 ci = chunkInfo[chunk];
    const int rows = (int)((unsigned)ci.y >> 16);
    const int wp = wpack[chunk];
    if (threadIdx.x == 0) echunk[chunk] = make_int4(colBegin[rep], codeBegin[rep], ci.z, rows | (wp << 12));
    if (rep != chunk) return;                                       // (block-uniform)
    const int len = (int)len8[ci.z + min((int)threadIdx.x, rows - 1)];   // rows >= 1
    int total;
    const int mine = (int)threadIdx.x < rows ? len : 0;
    const int e0 = blockExclusiveScan(mine, &total);
    __shared__ int lastE0;
    if ((int)threadIdx.x == rows - 1) lastE0 = e0;
    __syncthreads();
    const int eb = ci.x + ((int)threadIdx.x < rows ? e0 : lastE0);   // first entry of the row this lane presents
    const int u = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int W = (wp >> (4 * u)) & 15, CW = ellCodeWidth(W);
    if (W == 0 || u * 64 >= rows) return;                            // a unit without rows has no run
    int pre = 0, preC = 0;
    for (int v = 0; v < u; ++v) { const int w = (wp >> (4 * v)) & 15; pre += w; preC += ellCodeWidth(w); }
    uint16_t* oc = ecol + (size_t)colBegin[chunk] + (size_t)64 * pre + (size_t)lane * W;
    int8_t* ov = ecode + (size_t)codeBegin[chunk] + (size_t)64 * preC + (size_t)lane * CW;
    uint16_t lastc = 0;
    for (int k = 0; k < W; ++k) {
        if (k < len) lastc = col16[eb + k];
        oc[k] = (k < len || !nullOk) ? lastc : (uint16_t)0xf000;
    }
    for (int k = 0; k < CW; ++k) ov[k] = k < len ? code4[eb + k] : (int8_t)0;
}
}  // namespace
// Row-per-lane form of M's compressed stream (needs the windowed stream of buildCol16 and coded values)
void ps_context::buildEll(ps::DevCSR& M) {
    M.ellok = false;
    static const bool off = envInt(PS_ENV("PS_NO_ELL"), 0) != 0 ||  // A/B: keep the 4-entries-per-lane kernels
                            envInt(PS_ENV("PS_PIPE_GRID"), 1) == 0;   // (one-shot CSR kernels asked for)
    if (off || !M.col16ok || !M.packed || M.nChunks == 0 || (uint64_t)std::max(M.rows, M.cols) * 8 >= 0xffff8000ull) return;
    const int nChunks = M.nChunks;
    DevBuf<int32_t>& colBegin = scrEllCol; DevBuf<int32_t>& codeBegin = scrEllCode; DevBuf<int32_t>& wpack = scrEllW;
    colBegin.alloc((size_t)nChunks + 1); codeBegin.alloc((size_t)nChunks + 1); wpack.alloc((size_t)nChunks);
    HIP_CHECK(hipMemsetAsync(colBegin.p + nChunks, 0, sizeof(int32_t), stream));
    HIP_CHECK(hipMemsetAsync(codeBegin.p + nChunks, 0, sizeof(int32_t), stream));
    HIP_CHECK(hipMemsetAsync(counters.p + CTR_ELL_TOO_LONG, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_ell_plan, dim3((unsigned)nChunks), dim3(BS), 0, stream, (const int4*)M.chunkInfo.p, (const uint8_t*)M.len8.p, (const int32_t*)M.chunkRep.p,
                       colBegin.p, codeBegin.p, wpack.p, counters.p + CTR_ELL_TOO_LONG);
    scanBlock.alloc((size_t)gridFor(nChunks + 1, PS_SCAN_TILE) + 16);                   // (both unsynchronised scans below use it)
    (void)exclusiveScanI32(colBegin.p, nChunks + 1, CTR_ELL_COLS);
    (void)exclusiveScanI32(codeBegin.p, nChunks + 1, CTR_ELL_CODES);
    int32_t w[3];                                                                // one round trip for the width check and the two totals
    fetchCounters(CTR_ELL_TOO_LONG, 3, w);
    const int32_t tooLong = w[0];
    const int64_t totCol = w[1], totCode = w[2];
    if (totCol < 0 || totCode < 0 || (uint64_t)totCol * 2 >= 0xffffffffull || tooLong != 0) return;   // a row longer than 8 / 32-bit offsets: keep the other kernels
    M.ellCols = totCol; M.ellCodes = totCode; M.ellUniqueCols = totCol;
    M.ecol.alloc((size_t)totCol + 64); M.ecode.alloc((size_t)totCode + 64); M.echunk.alloc((size_t)nChunks);
    hipLaunchKernelGGL(k_ell_fill, dim3((unsigned)nChunks), dim3(BS), 0, stream, (const int4*)M.chunkInfo.p, (const uint8_t*)M.len8.p, (const int32_t*)M.chunkRep.p,
                       (const uint16_t*)M.col16.p, (const int8_t*)M.code4.p, (const int32_t*)colBegin.p, (const int32_t*)codeBegin.p, (const int32_t*)wpack.p,
                       M.ecol.p, M.ecode.p, M.echunk.p, M.winBase.p);
    M.ellok = true;
    if (PS_ENV_VERBOSE()) std::fprintf(stderr, "[polystokes] row-per-lane stream: %d chunks, %lld column slots and %lld code bytes in the distinct runs (nnz %lld)\n",
                                           nChunks, (long long)totCol, (long long)totCode, (long long)M.nnz);
}
namespace {
__global__ void k_decode_values(const int8_t* __restrict__ code, double scale, int64_t n, double* __restrict__ val) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) val[i] = (double)code[i] * scale;
}
}  // namespace
// the fp64 values of a block whose codes hold them exactly (constructMatrixBlocks does not store them then): exports, benchmarks
void ps_context::ensureValues(ps::DevCSR& M) {
    if (M.val.p || M.nnz == 0) return;
    if (!M.packed || !M.code.p) throw Error("internal: a block without values and without codes");
    M.val.alloc((size_t)M.nnz);
    hipLaunchKernelGGL(k_decode_values, dim3(2048), dim3(BS), 0, stream, (const int8_t*)M.code.p, valScale, M.nnz, M.val.p);
}
void ps_context::buildVal4(ps::DevCSR& M) {
    if (!M.col16ok || M.val4.p) return;
    ensureValues(M);
    M.val4.alloc((size_t)M.streamLen + 8);
    hipLaunchKernelGGL(k_val4_build, dim3((unsigned)M.nChunks), dim3(BS), 0, stream, M.ptr.p, M.val.p, M.chunkInfo.p, M.val4.p);
}
// Compressed SpMV stream (DevCSR::col16 ...); decided per matrix.  With coded values it is 3 B per entry; when the values are
// not code * scale (user-supplied weights, PS_FORCE_FP64_VALUES=1) the same windowed 16-bit columns go with the fp64 values
// (10 B per entry, DevCSR::val4) and the same pipelined kernels run.  PS_COL32=1 keeps the one-shot CSR kernels.
void ps_context::buildCol16(ps::DevCSR& M, Counter slot, const std::vector<int32_t>& cuts, const uint8_t* rowCode, int codeRows) {
    M.col16ok = false;
    M.ellok = false;
    M.nChunks = 0;
    M.val4.free();
    const char* e = PS_ENV("PS_COL32");
    if (M.rows == 0 || M.nnz == 0 || (e && atoi(e) != 0)) return;
    // Chunk table.  `cuts` (ascending row indices, first 0, last M.rows; may be empty) are where the numbering's lattice blocks
    // and the tiles' skin-row ranges begin.  A range of >= CHUNK_ALIGN_MIN rows starts its own chunk — equivalent blocks then
    // cut their rows into chunks the same way and produce identical runs (dedupChunks) — shorter ranges (thin layers at a
    // free surface) are packed with their neighbours so that the chunk count stays close to rows / 256.
    std::vector<int2> rowsOf;
    {
        constexpr int CHUNK_ALIGN_MIN = 512;
        static const bool plain = envInt(PS_ENV("PS_CHUNK_PLAIN"), 0) != 0;   // A/B: uniform 256-row chunks
        bool ok = !plain && cuts.size() >= 2 && cuts.front() == 0 && (int64_t)cuts.back() == M.rows;
        for (size_t i = 1; ok && i < cuts.size(); ++i) ok = cuts[i] >= cuts[i - 1];
        auto emit = [&](int64_t lo, int64_t hi) { for (int64_t r = lo; r < hi; r += BS) rowsOf.push_back(make_int2((int)r, (int)std::min<int64_t>(BS, hi - r))); };
        if (!ok) emit(0, M.rows);
        else {
            int64_t runLo = 0;
            for (size_t i = 0; i + 1 < cuts.size(); ++i) {
                const int64_t lo = cuts[i], hi = cuts[i + 1];
                if (hi - lo >= CHUNK_ALIGN_MIN) { emit(runLo, lo); emit(lo, hi); runLo = hi; }
            }
            emit(runLo, M.rows);
        }
    }
    const int nChunks = (int)rowsOf.size();
    DevBuf<int2>& chunkRows = scrChunkRows;      // setup scratch kept with the context: a hipMalloc / hipFree pair per build costs more than the kernels
    chunkRows.alloc((size_t)nChunks);
    HIP_CHECK(hipMemcpyAsync(chunkRows.p, rowsOf.data(), (size_t)nChunks * sizeof(int2), hipMemcpyHostToDevice, stream));
    DevBuf<int32_t>& start4 = scrStart4;
    start4.alloc((size_t)nChunks + 1);
    HIP_CHECK(hipMemsetAsync(counters.p + CTR_CHUNK_MAX, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_chunk_len4, dim3(gridFor(nChunks + 1, BS)), dim3(BS), 0, stream, M.ptr.p, (const int2*)chunkRows.p, nChunks, start4.p, counters.p + CTR_CHUNK_MAX);
    const int64_t total4 = exclusiveScanI32(start4.p, nChunks + 1);   // (synchronises: rowsOf may go out of scope after this)
    if (total4 < 0) return;                                           // would overflow 32 bits: keep the CSR kernels
    const int maxLen = readCounter(CTR_CHUNK_MAX);
    M.nv = std::max(1, (maxLen + 4 * BS - 1) / (4 * BS));
    if (M.nv > 2) return;
    // the kernels address everything through 32-bit buffer descriptors: every array they touch must stay below 4 GiB
    if ((uint64_t)std::max(M.rows, M.cols) * 8 >= 0xffffffffull || (uint64_t)total4 * 2 >= 0xffffffffull) return;
    M.streamLen = total4;
    M.uniqueLen = total4;
    M.nChunks = nChunks;
    M.col16.alloc((size_t)total4 + 8); M.code4.alloc((size_t)total4 + 8);
    M.winBase.alloc((size_t)nChunks * 16); M.chunkInfo.alloc((size_t)nChunks); M.len8.alloc((size_t)M.rows); M.chunkRep.alloc((size_t)nChunks);
    HIP_CHECK(hipMemsetAsync(counters.p + slot, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_col16_build, dim3((unsigned)((nChunks + BS / 64 - 1) / (BS / 64))), dim3(BS), 0, stream, M.ptr.p, M.col.p, M.code.p, (const int2*)chunkRows.p, start4.p, M.col16.p,
                       M.code4.p, M.winBase.p, M.chunkInfo.p, M.len8.p, counters.p + slot, M.chunkRep.p, nChunks);
    M.col16ok = readCounter(slot) == 0;
    if (M.col16ok && !M.packed) buildVal4(M);
    static const bool noShare = envInt(PS_ENV("PS_NO_SHARED_RUNS"), 0) != 0;
    static const bool weakHash = envInt(PS_ENV("PS_WEAK_CHUNK_HASH"), 0) != 0;   // test: force hash collisions
    if (M.col16ok && M.packed && shareRuns && !noShare && nChunks > 1) {          // coded values only: the fp64 values of equal codes need not be equal bits
        unsigned cap = 1024;
        while (cap < 4u * (unsigned)nChunks) cap <<= 1;
        DevBuf<unsigned long long>& hash = scrHash; DevBuf<unsigned long long>& keys = scrKeys; DevBuf<unsigned long long>& uniq = scrUniq;
        DevBuf<int32_t>& vals = scrVals;
        hash.alloc((size_t)nChunks); keys.alloc(cap); vals.alloc(cap); uniq.alloc(1);
        HIP_CHECK(hipMemsetAsync(keys.p, 0xff, (size_t)cap * 8, stream));
        HIP_CHECK(hipMemsetAsync(vals.p, 0x7f, (size_t)cap * 4, stream));
        HIP_CHECK(hipMemsetAsync(uniq.p, 0, 8, stream));
        hipLaunchKernelGGL(k_chunk_hash, dim3((unsigned)nChunks), dim3(64), 0, stream, (const int4*)M.chunkInfo.p, (const uint16_t*)M.col16.p, (const int8_t*)M.code4.p,
                           (const uint8_t*)M.len8.p, hash.p, weakHash ? 1 : 0);
        hipLaunchKernelGGL(k_chunk_rep_insert, dim3(gridFor(nChunks, BS)), dim3(BS), 0, stream, (const unsigned long long*)hash.p, nChunks, keys.p, vals.p, cap - 1);
        hipLaunchKernelGGL(k_chunk_share, dim3((unsigned)nChunks), dim3(64), 0, stream, (const unsigned long long*)hash.p, (const unsigned long long*)keys.p,
                           (const int32_t*)vals.p, cap - 1, M.chunkInfo.p, (const uint16_t*)M.col16.p, (const int8_t*)M.code4.p, (const uint8_t*)M.len8.p, rowCode, codeRows, uniq.p, M.chunkRep.p);
        unsigned long long u = 0;
        HIP_CHECK(hipMemcpyAsync(&u, uniq.p, 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        M.uniqueLen = (int64_t)u;
    }
    if (PS_ENV_VERBOSE()) std::fprintf(stderr, "[polystokes] compressed stream: rows %lld nnz %lld, %d chunks, fullest %d (nv %d), ok %d, distinct runs hold %lld of %lld entries\n",
                                           (long long)M.rows, (long long)M.nnz, nChunks, maxLen, M.nv, (int)M.col16ok, (long long)M.uniqueLen, (long long)M.streamLen);
}

// ---- value-set coding of the diagonals (ps_context.hpp: uCode / mcCode) ----------------------------------------------
namespace {
constexpr unsigned long long DICT_EMPTY = 0xfff8dead0000beefull;   // a NaN payload no diagonal value takes
__device__ inline int dictHash(unsigned long long k) { k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 29; return (int)(k & 255ull); }
// insert every value into a 256-slot open-addressing table (linear probing); slot index = the value's code
__global__ void __launch_bounds__(BS) k_dict_build(const double* __restrict__ v, int64_t n, unsigned long long* __restrict__ table, int32_t* __restrict__ overflow) {
    // a block works from an LDS snapshot of the table: after the first few hundred values every lookup is an LDS hit.  A value
    // missing from the snapshot takes the global probe / CAS path — ONE lane per distinct missing value of the wave (leader
    // election): with every lane probing for itself the first values of all 2048 blocks queue on the same few table slots
    // (2.5 ms at 22 M values; now 0.1 ms).  Once the table has overflowed (> 256 values) the rest of the sweep is skipped.
    __shared__ unsigned long long snap[256];
    snap[threadIdx.x] = __hip_atomic_load(&table[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounds = (n + stride - 1) / stride;
    for (int64_t k = 0; k < rounds; ++k) {                         // every lane of a wave takes every round (the election needs them)
        const int64_t i = k * stride + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const bool have = i < n;
        const unsigned long long key = have ? (unsigned long long)__double_as_longlong(v[i]) : 0ull;
        bool miss = have;
        if (have && key == DICT_EMPTY) { *overflow = 1; miss = false; }
        if (miss) {
            const int h0 = dictHash(key);
            for (int probe = 0; probe < 256; ++probe) {             // LDS snapshot first
                const unsigned long long cur = snap[(h0 + probe) & 255];
                if (cur == key) { miss = false; break; }
                if (cur == DICT_EMPTY) break;
            }
        }
        unsigned long long m = __ballot(miss);
        if (m != 0ull && __hip_atomic_load(overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;   // wave-uniform
        while (m != 0ull) {
            const int leader = __ffsll((long long)m) - 1;
            const unsigned long long lk = ((unsigned long long)(unsigned)__shfl((int)(key >> 32), leader, 64) << 32) | (unsigned)__shfl((int)(key & 0xffffffffull), leader, 64);
            if ((int)(threadIdx.x & 63) == leader) {
                int h = dictHash(lk);
                bool placed = false;
                for (int probe = 0; probe < 256 && !placed; ++probe) {
                    unsigned long long cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur == DICT_EMPTY) cur = atomicCAS(&table[h], DICT_EMPTY, lk), cur = (cur == DICT_EMPTY) ? lk : cur;
                    if (cur == lk) { placed = true; snap[h] = lk; }   // benign race: every writer of a slot writes the slot's one key
                    else h = (h + 1) & 255;
                }
                if (!placed) *overflow = 1;
            }
            if (miss && key == lk) miss = false;                    // the leader's value: done for every lane holding it
            m = __ballot(miss);
        }
    }
}
__global__ void k_dict_code(const double* __restrict__ v, int64_t n, const unsigned long long* __restrict__ table, uint8_t* __restrict__ code) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(v[i]);
        int h = dictHash(key);
        for (int probe = 0; probe < 256 && table[h] != key; ++probe) h = (h + 1) & 255;
        code[i] = (uint8_t)h;
    }
}
__global__ void k_dict_init(unsigned long long* table) { table[threadIdx.x] = DICT_EMPTY; }
__global__ void k_dict_finish(unsigned long long* table) { if (table[threadIdx.x] == DICT_EMPTY) table[threadIdx.x] = 0ull; }   // unused slots decode to 0.0
}  // namespace
void ps_context::buildDiagonalCodes() {
    uCoded = mcCoded = false;
    const char* e = PS_ENV("PS_NO_DIAG_CODES");
    if (e && atoi(e) != 0) return;
    auto build = [&](const DevBuf<double>& vals, int64_t n, DevBuf<uint8_t>& code, DevBuf<double>& dict) -> bool {
        if (n <= 0) return false;
        dict.alloc(256); code.alloc((size_t)n);
        unsigned long long* table = (unsigned long long*)dict.p;
        HIP_CHECK(hipMemsetAsync(counters.p + CTR_DICT_OVERFLOW, 0, sizeof(int32_t), stream));
        hipLaunchKernelGGL(k_dict_init, dim3(1), dim3(256), 0, stream, table);
        hipLaunchKernelGGL(k_dict_build, dim3(2048), dim3(BS), 0, stream, vals.p, n, table, counters.p + CTR_DICT_OVERFLOW);
        if (readCounter(CTR_DICT_OVERFLOW) != 0) return false;
        hipLaunchKernelGGL(k_dict_code, dim3(1024), dim3(BS), 0, stream, vals.p, n, (const unsigned long long*)table, code.p);
        hipLaunchKernelGGL(k_dict_finish, dim3(1), dim3(256), 0, stream, table);
        return true;
    };
    uCoded = build(uInv, nSystem, uCode, uDict);
    mcCoded = build(McInv, nActiveVs, mcCode, mcDict);
    if (PS_ENV_VERBOSE()) std::fprintf(stderr, "[polystokes] diagonal value sets: uInv %s, McInv %s\n", uCoded ? "coded (<= 256 values)" : "fp64", mcCoded ? "coded" : "fp64");
}

// the compressed streams of S and St.  share = false (bench.py's "_fp64" kernels: the fp64-value stream as a system with arbitrary
// weights would have it) keeps every chunk on its own run.
void ps_context::buildStreams(bool share) {
    // where chunks should start: the lattice blocks of the numbering (active rows; DOFs), then every tile's skin rows
    std::vector<int32_t> cutsS, cutsT;
    if (!blockStartRow.empty() && (int64_t)blockStartRow.back() == nActiveVs) {
        cutsS = blockStartRow;
        for (size_t r = 1; r < skinCutsHost.size(); ++r) cutsS.push_back((int32_t)(nActiveVs + skinCutsHost[r]));   // (skinCutsHost[0] = 0 = the end of the active rows)
    }
    if (!blockStartSys.empty() && (int64_t)blockStartSys.back() == nSystem) cutsT = blockStartSys;
    shareRuns = share;
    buildCol16(S, CTR_COL16_FAIL_S, cutsS, mcCoded ? mcCode.p : nullptr, (int)nActiveVs);
    buildCol16(St, CTR_COL16_FAIL_ST, cutsT, uCoded ? uCode.p : nullptr, (int)nSystem);
    if (share) { buildEll(S); buildEll(St); } else S.ellok = St.ellok = false;   // (the unshared rebuild is bench.py's fp64-value stream: the 4-entries-per-lane kernels)
}

// ConstructMatrixBlocks.cpp:9-292
void ps_context::constructMatrixBlocks() {
    nActiveVs = nFace[0] + nFace[1] + nFace[2];
    nReducedVs = regionCount * PS_RD;
    nPressures = nCenter;
    nStresses = 3 * nCenter + nEdge[0] + nEdge[1] + nEdge[2];
    nSystem = nPressures + nStresses;
    nTotalDOFs = nActiveVs + nReducedVs + nPressures + nStresses;
    if (nSystem >= 0x7fffffff || nActiveVs >= 0x7fffffff) throw Error("system too large for 32-bit DOF indices");

    valScale = invDx / 64.;
    HIP_CHECK(hipMemsetAsync(counters.p + CTR_CODE_FAIL, 0, sizeof(int32_t), stream));
    solidBoundaryUsed = solidBoundarySet;   // (ps_set_solid_boundary; read by makeArgs)
    if (solidBoundaryUsed == PS_SOLID_FREE_SLIP) {
        slipEdges.alloc(1);
        HIP_CHECK(hipMemsetAsync(slipEdges.p, 0, sizeof(int32_t), stream));
    }
    buildInternalNumbering();   // sysIdx[], faceRow[] (active rows), permSys, permRow
    haloForward = false;        // one exchange round unless Dist::decideExchangeMode finds a row that reaches a diagonal neighbour's sample
    buildHaloLists();
    BlockArgs A = makeArgs(this);
    // reduced rows
    nReducedRows = 0;
    maxRegionRows = 0;
    if (regionCount > 0 && sbItems > 0) {
        hipLaunchKernelGGL(k_skin<false>, dim3((unsigned)sbItems), dim3(BS), 0, stream, A, bbox.p, sbItemRegion.p, sbItemStart.p, sbItemCount.p,
                           faceRow[0].p, faceRow[1].p, faceRow[2].p, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
        HIP_CHECK(hipMemsetAsync(sbItemCount.p + sbItems, 0, sizeof(int32_t), stream));
        nReducedRows = exclusiveScanI32(sbItemCount.p, sbItems + 1);
        rrowFace.alloc((size_t)nReducedRows);
        rrowRegion.alloc((size_t)nReducedRows);
        sbItemLong.alloc((size_t)sbItems);
        hipLaunchKernelGGL(k_skin<true>, dim3((unsigned)sbItems), dim3(BS), 0, stream, A, bbox.p, sbItemRegion.p, sbItemStart.p, sbItemCount.p,
                           faceRow[0].p, faceRow[1].p, faceRow[2].p, rrowFace.p, rrowRegion.p, sbItemLong.p);
        // region -> row range, and equal pieces of <= RC_ROWS rows for the three-kernel tile apply (host built)
        std::vector<int32_t> itemOff((size_t)sbItems + 1), itemLong((size_t)sbItems);
        HIP_CHECK(hipMemcpyAsync(itemOff.data(), sbItemCount.p, itemOff.size() * 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(itemLong.data(), sbItemLong.p, itemLong.size() * 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        // where the stream build may start a chunk inside the skin rows: every item's first row and the end of its long rows
        skinCutsHost.clear();
        for (int64_t q = 0; q < sbItems; ++q) {
            skinCutsHost.push_back(itemOff[(size_t)q]);
            if (itemLong[(size_t)q] > 0 && itemOff[(size_t)q] + itemLong[(size_t)q] < itemOff[(size_t)q + 1]) skinCutsHost.push_back(itemOff[(size_t)q] + itemLong[(size_t)q]);
        }
        skinCutsHost.push_back(itemOff[(size_t)sbItems]);
        std::vector<int32_t>& rptr = hostTab[6]; std::vector<int32_t>& cR = hostTab[7]; std::vector<int32_t>& cS = hostTab[8]; std::vector<int32_t>& cE = hostTab[9];
        std::vector<int32_t>& cptr = hostTab[10];      // (kept with the context: their uploads need no synchronisation)
        rptr.assign((size_t)regionCount + 1, 0); cR.clear(); cS.clear(); cE.clear(); cptr.assign((size_t)regionCount + 1, 0);
        for (int64_t r = 0; r <= regionCount; ++r) rptr[(size_t)r] = itemOff[(size_t)sbRegionItemPtrHost[(size_t)r]];
        regionRowPtrHost = rptr;
        for (int64_t r = 0; r < regionCount; ++r) {
            cptr[(size_t)r] = (int32_t)cR.size();
            const int32_t lo = rptr[(size_t)r], hi = rptr[(size_t)r + 1], len = hi - lo;
            maxRegionRows = std::max<int64_t>(maxRegionRows, len);
            if (len > 0) {
                const int32_t pieces = (len + RC_ROWS - 1) / RC_ROWS;
                for (int32_t q = 0; q < pieces; ++q) {
                    cR.push_back((int32_t)r);
                    cS.push_back(lo + (int32_t)((int64_t)len * q / pieces));
                    cE.push_back(lo + (int32_t)((int64_t)len * (q + 1) / pieces));
                }
            }
        }
        cptr[(size_t)regionCount] = (int32_t)cR.size();
        nRChunks = (int64_t)cR.size();
        regionRowPtr.alloc(rptr.size()); rchunkRegion.alloc(cR.size()); rchunkStart.alloc(cS.size()); rchunkEnd.alloc(cE.size());
        regionChunkPtr.alloc(cptr.size());
        HIP_CHECK(hipMemcpyAsync(regionRowPtr.p, rptr.data(), rptr.size() * 4, hipMemcpyHostToDevice, stream));
        if (nRChunks) {
            HIP_CHECK(hipMemcpyAsync(rchunkRegion.p, cR.data(), cR.size() * 4, hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(rchunkStart.p, cS.data(), cS.size() * 4, hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(rchunkEnd.p, cE.data(), cE.size() * 4, hipMemcpyHostToDevice, stream));
        }
        HIP_CHECK(hipMemcpyAsync(regionChunkPtr.p, cptr.data(), cptr.size() * 4, hipMemcpyHostToDevice, stream));
    } else {
        nRChunks = 0;
        regionRowPtrHost.assign(1, 0);
        skinCutsHost.assign(1, 0);
    }
    nRows = nActiveVs + nReducedRows;
    if (nRows >= 0x7fffffff) throw Error("too many face rows");

    const bool wantExport = P.exportComponentMatrices != 0;
    McInv.alloc((size_t)nActiveVs); rhsA.alloc((size_t)nActiveVs);
    oldVs.alloc((size_t)nActiveVs);   // the warm-start guess needs the old face velocities themselves (constructGuessVectors)
    if (wantExport) { Mc.alloc((size_t)nActiveVs); uDiag.alloc((size_t)nSystem); }
    uInv.alloc((size_t)nSystem); rhsPT.alloc((size_t)nSystem);

    // S
    S.rows = nRows; S.cols = nSystem;
    S.ptr.alloc((size_t)nRows + 1);
    HIP_CHECK(hipMemsetAsync(S.ptr.p, 0, ((size_t)nRows + 1) * sizeof(int32_t), stream));
    for (int a = 0; a < 3; ++a) {
        const int64_t n = g.count(1 + a);
        hipLaunchKernelGGL(k_S_count, dim3(gridFor(n, BS)), dim3(BS), 0, stream, A, a, S.ptr.p);
    }
    {
        // 32-bit scan: guard against overflow with the a-priori bound 8 nnz per row
        if ((int64_t)nRows * 8 >= 0x7fffffffLL) {
            // still fine as long as the true total fits; the scan total is checked below
        }
        const int64_t tot = exclusiveScanI32(S.ptr.p, nRows + 1);
        if (tot < 0) throw Error("nnz(S) overflows 32-bit row pointers");
        S.nnz = tot;
    }
    // The fp64 values are not stored while the codes hold them exactly (every entry is checked as it is coded: CTR_CODE_FAIL): nothing on the
    // solve path reads them then, exports and the fp64-stream benchmarks decode them on demand (ensureValues) — 2 x 8 B per entry less to write
    // in setup and to keep (2.5 GB at 256^3).  They are written when the codes are refused (PS_FORCE_FP64_VALUES=1) or turn out not to fit:
    // the fill kernels then run once more with the value arrays.
    {
        const char* e = PS_ENV("PS_FORCE_FP64_VALUES");
        forceFp64Values = e && atoi(e) != 0;
    }
    auto fillS = [&](bool withValues) {
        if (withValues) S.val.alloc((size_t)S.nnz); else S.val.free();
        for (int a = 0; a < 3; ++a) {
            const int64_t n = g.count(1 + a);
            hipLaunchKernelGGL(k_S_fill, dim3(gridFor(n, BS)), dim3(BS), 0, stream, A, a, S.ptr.p, S.col.p, withValues ? S.val.p : (double*)nullptr, S.code.p, McInv.p, rhsA.p,
                               wantExport ? Mc.p : (double*)nullptr, oldVs.p);
        }
    };
    S.col.alloc((size_t)S.nnz); S.code.alloc((size_t)S.nnz);
    fillS(forceFp64Values);
    // St
    St.rows = nSystem; St.cols = nRows;
    St.ptr.alloc((size_t)nSystem + 1);
    HIP_CHECK(hipMemsetAsync(St.ptr.p, 0, ((size_t)nSystem + 1) * sizeof(int32_t), stream));
    auto fillSt = [&](bool withValues) {
        if (withValues) St.val.alloc((size_t)St.nnz); else St.val.free();
        double* v = withValues ? St.val.p : (double*)nullptr;
        const int64_t n = g.count(0);
        hipLaunchKernelGGL(k_St_cells<true>, dim3(gridFor(n, BS)), dim3(BS), 0, stream, A, (int32_t*)nullptr, St.ptr.p, St.col.p, v, St.code.p,
                           rhsPT.p, uInv.p, wantExport ? uDiag.p : (double*)nullptr);
        for (int e = 0; e < 3; ++e) {
            const int64_t ne = g.count(4 + e);
            hipLaunchKernelGGL(k_St_edges<true>, dim3(gridFor(ne, BS)), dim3(BS), 0, stream, A, e, (int32_t*)nullptr, St.ptr.p, St.col.p,
                               v, St.code.p, rhsPT.p, uInv.p, wantExport ? uDiag.p : (double*)nullptr);
        }
    };
    {
        const int64_t n = g.count(0);
        hipLaunchKernelGGL(k_St_cells<false>, dim3(gridFor(n, BS)), dim3(BS), 0, stream, A, St.ptr.p, (const int32_t*)nullptr,
                           (int32_t*)nullptr, (double*)nullptr, (int8_t*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr);
        for (int e = 0; e < 3; ++e) {
            const int64_t ne = g.count(4 + e);
            hipLaunchKernelGGL(k_St_edges<false>, dim3(gridFor(ne, BS)), dim3(BS), 0, stream, A, e, St.ptr.p, (const int32_t*)nullptr,
                               (int32_t*)nullptr, (double*)nullptr, (int8_t*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr);
        }
        St.nnz = exclusiveScanI32(St.ptr.p, nSystem + 1);
        if (St.nnz != S.nnz) throw Error("internal: nnz(S^T) != nnz(S)");
        St.col.alloc((size_t)St.nnz); St.code.alloc((size_t)St.nnz);
        fillSt(forceFp64Values);
    }
    {
        const bool ok = readCounter(CTR_CODE_FAIL) == 0;
        if (!ok && !forceFp64Values) { fillS(true); fillSt(true); }   // some value is not code * scale: the kernels will stream the values
        S.packed = St.packed = ok && !forceFp64Values;
        valuesCodedHost = S.packed ? 1 : 0;
        buildDiagonalCodes();   // before the streams: chunks that share a run also share their rows' diagonal codes
        buildStreams(true);
        columns16Host = (S.col16ok ? 1 : 0) | (St.col16ok ? 2 : 0);
    }
}
