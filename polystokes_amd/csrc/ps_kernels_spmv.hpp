// SpMV kernels: block helpers, the CSR-stream one-shot kernels and the persistent kernels on the compressed stream.
// Part of the single translation unit ps_solve.hip (included there, inside its anonymous namespace where noted).
#pragma once


constexpr int BS = 256;
constexpr int VGRID = 1024;   // capped grid for streaming vector kernels (grid-stride); 4 blocks per CU measured best

__device__ inline double waveReduceSum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// deterministic block sum (wave shuffles, then the 4 wave sums in order); result valid in thread 0
__device__ inline double blockReduceSum(double v) {
    __shared__ double ws[BS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = waveReduceSum(v);
    if (lane == 0) ws[w] = v;
    __syncthreads();
    double s = 0.;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < BS / 64; ++i) s += ws[i];
    }
    __syncthreads();
    return s;
}

// same sum (same order), valid in every thread
__device__ inline double blockSumAll(double v) {
    __shared__ double wsA[BS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = waveReduceSum(v);
    if (lane == 0) wsA[w] = v;
    __syncthreads();
    double s = 0.;
#pragma unroll
    for (int i = 0; i < BS / 64; ++i) s += wsA[i];
    __syncthreads();
    return s;
}

// Streaming phase of the CSR-stream SpMV: the block's contiguous nnz range [p0,p1) (<= BS*MAXNNZ entries)
// is read with a fixed-trip, fully unrolled loop so that all MAXNNZ (col,val) loads of a thread — and then
// all MAXNNZ gathers — are in flight together (memory-level parallelism instead of a dependent chain).
template <int SLOTS, bool PACKED>
__device__ inline void streamProducts(const int32_t* __restrict__ col, const double* __restrict__ val, const int8_t* __restrict__ code,
                                      double scale, const double* __restrict__ x, int p0, int p1, double* __restrict__ prod) {
    int c[SLOTS];
    double v[SLOTS];
#pragma unroll
    for (int u = 0; u < SLOTS; ++u) {
        const int p = p0 + threadIdx.x + u * BS;
        const bool ok = p < p1;
        c[u] = ok ? __builtin_nontemporal_load(col + p) : -1;
        if (PACKED) v[u] = ok ? (double)__builtin_nontemporal_load(code + p) * scale : 0.;   // exact: see DevCSR::code
        else v[u] = ok ? __builtin_nontemporal_load(val + p) : 0.;
    }
    double xv[SLOTS];
#pragma unroll
    for (int u = 0; u < SLOTS; ++u) xv[u] = c[u] >= 0 ? x[c[u]] : 0.;
#pragma unroll
    for (int u = 0; u < SLOTS; ++u)
        if (c[u] >= 0) prod[threadIdx.x + u * BS] = v[u] * xv[u];
}

// ---- CSR-stream SpMV ------------------------------------------------------------------------------
// One-shot variant: a block owns BS consecutive rows.  (More rows per thread was tried: 2 and 4 rows per thread are
// 5-100 % slower — registers and LDS cost more occupancy than the extra loads in flight buy.)
// MODE 0: out[row] = (row < nA ? dt*McInv[row] : 1) * (S x)[row]     (operator, forward half)
// MODE 1: out[row] = (S x)[row]                                       (velocity recovery)
template <int MODE, int MAXNNZ, bool PACKED>
__global__ void __launch_bounds__(BS) k_spmv_S(const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, const double* __restrict__ val,
                                               const int8_t* __restrict__ code, double scale, const double* __restrict__ x, int rows, int nA,
                                               double dt, const double* __restrict__ McInv, double* __restrict__ out,
                                               const int* __restrict__ done) {
    if (done && *done) return;
    constexpr int RPT = 1;
    __shared__ double prod[BS * MAXNNZ * RPT];
    const int r0 = blockIdx.x * (BS * RPT);
    const int r1 = min(r0 + BS * RPT, rows);
    const int p0 = ptr[r0], p1 = ptr[r1];
    // per-row loads that do not depend on the stream: issue them first
    int pa[RPT], pb[RPT];
    double sc[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int row = r0 + threadIdx.x + q * BS;
        const bool ok = row < rows;
        pa[q] = ok ? ptr[row] : 0;
        pb[q] = ok ? ptr[row + 1] : 0;
        sc[q] = (MODE == 0 && ok && row < nA) ? dt * McInv[row] : 1.;
    }
    streamProducts<MAXNNZ * RPT, PACKED>(col, val, code, scale, x, p0, p1, prod);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int row = r0 + threadIdx.x + q * BS;
        if (row < rows) {
            double s = 0.;
            for (int e = pa[q] - p0; e < pb[q] - p0; ++e) s += prod[e];
            out[row] = s * sc[q];
        }
    }
}
// MODE 0: out[j] = -(St t)[j] - 0.5*uInv[j]*xin[j];  partial[block] = sum xin[j]*out[j]
// MODE 1: out[j] = -(St t)[j] + add[j]                                   (right-hand side b)
template <int MODE, int MAXNNZ, bool PACKED>
__global__ void __launch_bounds__(BS) k_spmv_St(const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, const double* __restrict__ val,
                                                const int8_t* __restrict__ code, double scale, const double* __restrict__ t, int rows, int nP,
                                                const double* __restrict__ uInv, const double* __restrict__ xin, const double* __restrict__ add,
                                                double* __restrict__ out, double* __restrict__ partial, const int* __restrict__ done) {
    if (done && *done) return;
    constexpr int RPT = 1;
    __shared__ double prod[BS * MAXNNZ * RPT];
    const int r0 = blockIdx.x * (BS * RPT);
    const int r1 = min(r0 + BS * RPT, rows);
    const int p0 = ptr[r0], p1 = ptr[r1];
    int pa[RPT], pb[RPT];
    double e0[RPT], e1[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int row = r0 + threadIdx.x + q * BS;
        const bool ok = row < rows;
        pa[q] = ok ? ptr[row] : 0;
        pb[q] = ok ? ptr[row + 1] : 0;
        if (MODE == 0) { e0[q] = ok ? xin[row] : 0.; e1[q] = ok ? uInv[row] : 0.; }   // uInv is full length (0 on pressure rows)
        else { e0[q] = ok ? add[row] : 0.; e1[q] = 0.; }
    }
    streamProducts<MAXNNZ * RPT, PACKED>(col, val, code, scale, t, p0, p1, prod);
    __syncthreads();
    double d = 0.;
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int row = r0 + threadIdx.x + q * BS;
        if (row < rows) {
            double s = 0.;
            for (int e = pa[q] - p0; e < pb[q] - p0; ++e) s += prod[e];
            double y;
            if (MODE == 0) {
                y = -s;
                y -= 0.5 * e1[q] * e0[q];
                d += e0[q] * y;
            } else {
                y = -s + e0[q];
            }
            out[row] = y;
        }
    }
    if (MODE == 0) {
        const double bs = blockReduceSum(d);
        if (threadIdx.x == 0) partial[blockIdx.x] = bs;
    }
}


// ---- persistent, software-pipelined kernels on the compressed stream -----------------------------------
// PMC (SQ_WAIT_ANY / SQ_WAVE_CYCLES = 85 %) shows the one-shot kernels above are latency bound: every block walks
// three dependent memory round trips (row-pointer bounds -> (col,val) stream -> gather) at the occupancy cap of
// 8 waves/SIMD.  Here a block loops over row chunks (grid = #CUs x 16) and, while the gathers / LDS reduction of
// chunk i are in flight, the stream of chunk i+1 is already loading into a second register set and the bounds of
// chunk i+2 are being fetched.  They read the compressed form of the matrix built by ps_context::buildCol16:
//   * per chunk (<= 256 consecutive rows, starting at lattice-block / tile boundaries) a 4-entry-aligned run of (16-bit windowed
//     column, int8 value code): 3 B per entry, fetched as one 8-byte + one 4-byte load per lane for 4 consecutive entries — chunks
//     whose runs are byte-identical share ONE run (ps_blocks.hip: k_chunk_share), which then comes from cache,
//   * 16 window bases and a Chunk record (below) per chunk, one row-length byte per row (prefix-summed in the block)
// and reproduce the fp64 CSR product bit for bit (same values, same summation order within a row).
//
// chunk walk of a persistent block.  Plain: chunk = block + it * grid.  Grouped (G = xcdAware > 0): workgroups b, b+8, ...
// run on XCD b & 7 (verified with s_getreg HW_REG_XCC_ID), so runs of G consecutive chunks are dealt to the XCDs round
// robin — rows that gather the same lines of x (k-plane neighbours, a few chunks apart) then share ONE L2, while
// the chip as a whole still sweeps one compact window of memory.
// MODE 2 of the St kernel: one term of the Chebyshev preconditioner fused into the epilogue (ps_context::chebyshevApply), in its
// three-term form (no difference vector to keep):  Az = (A z_j)[row];  z_{j+1} = z_j + c1 (z_j - z_{j-1}) + c2 dinv (r - Az);
// partial += r z_{j+1}.  z_j is the kernel's x (xin), z_{j-1} is read from zprev (null: zero) and z_{j+1} goes to `out` — the
// caller passes the z_{j-1} buffer: every row is read and then written by the same thread.
struct ChebArgs { const double* r; const diag_t* dinv; const double* zprev; double c1, c2; };   // dinv: the stored diagonal (ps_common.hpp)
// MODE 3 of the St kernel: the residual update of the PCG step inside the epilogue.  x . A x is known BEFORE the kernel starts,
// from the factored form:  x.Ax = -( sum_active s_f t_f  +  sum_tiles w.v  +  1/2 sum_j uInv_j x_j^2 )  (partials of the S kernel,
// of the tile kernel and of k_cg_update_xp) — so every workgroup forms alpha itself and does r -= alpha (A p) on its rows with
// (A p)[row] still in a register: A p is never written or read back, and k_cg_update_r is not launched.
struct FusedR {
    CGScalars* sc;
    const double* sPart; int sCount;      // k_spmv_S_pipe: active-face share
    const double* tPart; int tCount;      // k_tile_apply: one value per region
    const double* uPart; int uCount;      // k_cg_update_xp / k_uinv_pp: 1/2 sum uInv p^2 is formed here (partials hold sum uInv p^2)
    const double* xxPart; int xxCount;    // ||x||^2 partials of the previous k_cg_update_xp (stop test of the previous iteration)
    int it;
    double* r; const diag_t* dinvF;       // residual (updated in place), stored Jacobi diagonal (ps_common.hpp: diag_t; null: identity)
    double* rPart;                        // out: partials of r.r at [block], of r.z at [gridDim + block]
    // Chebyshev preconditioner: the polynomial's first term on the new r, z_1 = dinv r / theta -> cz (null: not asked for; then r.z
    // above is that of the Jacobi diagonal).  At most ONE of dinvF and cz is set (every site that fills a FusedR: the Chebyshev step, the
    // Jacobi / identity step and spmv_St_r in ps_solve.hip, the rank's step in ps_dist.hpp): with cz the r.z partial is the polynomial's
    // share alone and dinvF is not read (fusedRowFinish).
    const diag_t* dinvC; double invTheta; double* cz;
    // Slab decomposition (ps_dist.hpp): red = {S + T + 1/2 U summed over the ranks, ||x||^2 over the ranks} replaces the partial
    // sums above; only rows in [ownLo, ownHi) are this rank's DOFs — the others (halo DOFs) carry contributions to a neighbour's
    // rows: their y goes to yOut and the owner subtracts alpha times it afterwards (k_dist_fixup).  Single domain: red = null,
    // [0, rows), yOut = null.
    const double* red; int ownLo, ownHi; double* yOut;
    // the kernel may run as two launches (rows next to a cut first, the rest under the exchange: ps_dist.hpp): partials of r.r at
    // rPart[block], of r.z at rPart[rStride + block]; 0 = one launch (stride = its grid)
    int rStride;
};
// Walk of a persistent workgroup over the chunk ids: runs of G = 1 << sh consecutive chunks are dealt to the 8 XCDs round robin
// (workgroup b runs on XCD b & 7), inside an XCD to its workgroups in order; sh < 0: plain grid-stride walk
// rs: a workgroup takes runs of 1 << rs CONSECUTIVE chunks (bits 16.. of the launch parameter g): its waves then find the lines the previous
// chunk gathered in the CU's L1.  Plain integers, for the kernels and for the host (ps_solve.hip: Launch::noteWalk).
__host__ __device__ inline int chunkWalkShift(int g) { return (g & 0xffff) > 0 ? 31 - __builtin_clz((unsigned)(g & 0xffff)) : -1; }
__host__ __device__ inline int chunkWalkRun(int g) { return (g >> 16) & 7; }
__host__ __device__ inline int chunkWalkAt(int it, int block, int grid, int sh, int rs) {   // step `it` of workgroup `block` of `grid` -> chunk (>= the chunk count: the walk is over)
    const int j = it >> rs, o = it & ((1 << rs) - 1);
    int run;
    if (sh < 0) run = block + j * grid;
    else {
        const int q = (block >> 3) + j * (grid >> 3);
        run = ((((q >> sh) << 3) + (block & 7)) << sh) + (q & ((1 << sh) - 1));
    }
    return (run << rs) + o;
}
struct ChunkWalk {
    int sh, rs;
    __device__ explicit ChunkWalk(int g) : sh(chunkWalkShift(g)), rs(chunkWalkRun(g)) {}
    __device__ int at(int it) const { return chunkWalkAt(it, (int)blockIdx.x, (int)gridDim.x, sh, rs); }
};
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// Every access of the loop body goes through a buffer descriptor (buffer_load/store ... offen): 32-bit byte offsets
// instead of 64-bit address arithmetic, and hardware bounds checking (a load past `bytes` returns 0, a store is dropped),
// so the body has NO branches: lanes past the end of a chunk / of the rows load and multiply harmless values into LDS
// slots no row reads.  (Arrays must be < 4 GiB: checked by ps_context::buildCol16.)
__device__ inline __amdgpu_buffer_rsrc_t bufRsrc(const void* p, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(unsigned)bytes, 0x00020000);
}
__device__ inline double bufLoadF64(__amdgpu_buffer_rsrc_t r, unsigned byteOff) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)byteOff, 0, 0));
}
template <bool NT> __device__ inline double bufLoadF64epi(__amdgpu_buffer_rsrc_t r, unsigned byteOff);
__device__ inline void bufStoreF64(__amdgpu_buffer_rsrc_t r, unsigned byteOff, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (int)byteOff, 0, 0);
}
// Cache policies of the three access classes (compile-time, scripts/build_variant.sh builds A/B copies).  Measured at 256^3
// (profiles/r02_cache_policy.txt): result stores nt (aux 2: written once, read by the NEXT kernel; St -7 %, S -3 % against
// default-policy stores; sc1 / sc0 sc1 stores +4 %); stream loads nt (sc1 / sc0 sc1 / default within 1 %); gathers default
// policy — nt gathers bypass the CU's L1 and run 2x slower: what cross-row reuse there is comes from L1.
#ifndef PS_STORE_AUX
#define PS_STORE_AUX 2
#endif
#ifndef PS_STREAM_AUX
#define PS_STREAM_AUX 2
#endif
#ifndef PS_GATHER_AUX
#define PS_GATHER_AUX 0
#endif
#ifndef PS_EPI_AUX
#define PS_EPI_AUX 2       // the per-row streams of the epilogues (row length, x, uInv / codes): read once per launch -> nt (St -3 %)
#endif
#ifndef PS_DIAG_AUX
#define PS_DIAG_AUX PS_EPI_AUX   // the stored Jacobi diagonal in the residual-update epilogue (read again by the x/p update half an iteration later)
#endif
#ifndef PS_UC_AUX
#define PS_UC_AUX PS_EPI_AUX     // the uInv codes in the two-unit St kernels (read again by the x/p update)
#endif
// POL (template parameter of the pipelined kernels), bit 0: the non-temporal policies above for the result stores and the per-row
// epilogue streams; bit 1: for the matrix stream (col16 / code4 / val4).  Chosen per system (Launch::policy): streams that are
// touched once per launch should not sweep the caches of a 45 M-row system, but a system that fits in the 256 MB memory-side
// cache (or nearly) is served from it between kernels if they are allowed to stay; and a matrix stream whose runs are SHARED
// between chunks (DevCSR::uniqueLen) is read again and again — it must stay cached (non-temporal it is 11 % slower than unshared).
// entry `row` of the stored Jacobi diagonal (diag_t: 16 bits, the upper half of an fp32 value; fp32 under -DPS_DIAG_FP32) as a float — 0 past the buffer
template <bool NT> __device__ inline float bufLoadDiag(__amdgpu_buffer_rsrc_t r, unsigned row) {
#ifdef PS_DIAG_FP32
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(row * 4u), 0, NT ? PS_DIAG_AUX : 0));
#else
    const uint32_t h = (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(r, (int)(row * 2u), 0, NT ? PS_DIAG_AUX : 0);
    return __builtin_bit_cast(float, h << 16);
#endif
}
template <bool NT> __device__ inline double bufLoadF64epi(__amdgpu_buffer_rsrc_t r, unsigned byteOff) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)byteOff, 0, NT ? PS_EPI_AUX : 0));
}
template <bool NT> __device__ inline void bufStoreF64nt(__amdgpu_buffer_rsrc_t r, unsigned byteOff, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (int)byteOff, 0, NT ? PS_STORE_AUX : 0);
}
__device__ inline double bufGatherF64(__amdgpu_buffer_rsrc_t r, unsigned byteOff) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)byteOff, 0, PS_GATHER_AUX));
}
// Element type of a vector a kernel gathers from / streams: double everywhere except the INNER vectors of the Chebyshev polynomial in its
// single-precision form (PS_PRE_CHEBYSHEV_F32: z_j and the face-row vector t of the polynomial's operator applies are STORED as fp32 — half the
// bytes of every gather and epilogue stream, half the lines a unit's gathers touch; every product, sum and recurrence stays fp64 in registers).
// Index = element index (the byte offset is formed here); loads past the buffer return 0, stores are dropped (buffer descriptors).
template <class T> struct VecIO;
template <> struct VecIO<double> {
    static constexpr unsigned BYTES = 8;
    __device__ static inline double gather(__amdgpu_buffer_rsrc_t r, unsigned i) { return bufGatherF64(r, i * 8u); }
    template <bool NT> __device__ static inline double loadEpi(__amdgpu_buffer_rsrc_t r, unsigned i) { return bufLoadF64epi<NT>(r, i * 8u); }
    __device__ static inline double load(__amdgpu_buffer_rsrc_t r, unsigned i) { return bufLoadF64(r, i * 8u); }
    template <bool NT> __device__ static inline void store(__amdgpu_buffer_rsrc_t r, unsigned i, double v) { bufStoreF64nt<NT>(r, i * 8u, v); }
    __device__ static inline double stored(double v) { return v; }              // the value a later kernel reads back
};
template <> struct VecIO<float> {
    static constexpr unsigned BYTES = 4;
    __device__ static inline double gather(__amdgpu_buffer_rsrc_t r, unsigned i) { return (double)__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(i * 4u), 0, PS_GATHER_AUX)); }
    template <bool NT> __device__ static inline double loadEpi(__amdgpu_buffer_rsrc_t r, unsigned i) { return (double)__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(i * 4u), 0, NT ? PS_EPI_AUX : 0)); }
    __device__ static inline double load(__amdgpu_buffer_rsrc_t r, unsigned i) { return (double)__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(i * 4u), 0, 0)); }
    template <bool NT> __device__ static inline void store(__amdgpu_buffer_rsrc_t r, unsigned i, double v) {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)v), r, (int)(i * 4u), 0, NT ? PS_STORE_AUX : 0);
    }
    __device__ static inline double stored(double v) { return (double)(float)v; }
};
// one lane's share of a chunk's stream: NV groups of 4 consecutive entries (non-temporal: read once)
// F64 = false: int8 value codes (3 B per entry with the column);  F64 = true: the fp64 values themselves in the same 4-aligned
// chunk layout (10 B per entry) — the form that runs when the stencil values are not code * scale (user-supplied weights)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int NV, bool F64> struct Stream4;
template <int NV> struct Stream4<NV, false> { u32x2 c[NV]; unsigned v[NV]; };
template <int NV> struct Stream4<NV, true> { u32x2 c[NV]; };   // the fp64 values are fetched for the CURRENT chunk only (below):
// double-buffering 16 more VGPR pairs per lane costs more occupancy than the prefetch buys
template <int NV> struct Vals4 { u32x4 v[NV][2]; };
template <int NV, bool NT>
__device__ inline void loadVals4(const double* val4, int p0, int p1, Vals4<NV>& s) {
    const __amdgpu_buffer_rsrc_t rVal = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(val4 + p0), 0, (int)(((unsigned)(p1 - p0 + 3) & ~3u) * 8u), 0x00020000);
#pragma unroll
    for (int w = 0; w < NV; ++w) {
        const unsigned rel = 4u * (threadIdx.x + w * BS) * 8u;                   // byte offset inside this chunk's values
        const bool in = (int)(p0 + 4 * (threadIdx.x + w * BS)) < p1;
        s.v[w][0] = __builtin_amdgcn_raw_buffer_load_b128(rVal, in ? (int)rel : -1, 0, NT ? PS_STREAM_AUX : 0);
        s.v[w][1] = __builtin_amdgcn_raw_buffer_load_b128(rVal, in ? (int)(rel + 16u) : -1, 0, NT ? PS_STREAM_AUX : 0);
    }
}
// (the fp64 value array can exceed the 4 GiB a buffer descriptor spans: its descriptor is rebuilt per chunk on the chunk's base)
template <int NV, bool F64, bool NT>
__device__ inline void loadStream4(__amdgpu_buffer_rsrc_t rCol, __amdgpu_buffer_rsrc_t rCode, const double* val4, int p0, int p1, Stream4<NV, F64>& s,
                                   unsigned tid = threadIdx.x) {               // tid: the thread's index inside its 256-thread group
#pragma unroll
    for (int w = 0; w < NV; ++w) {
        const unsigned first = (unsigned)p0 + 4u * (tid + w * BS);     // p0 is a multiple of 4
        // groups past the end of the chunk: offset 0xffffffff is out of range -> zeros without a memory access
        // (zeros decode to window 0 / offset 0 / value 0, like the padding inside the last group)
        const bool in = (int)first < p1;
        s.c[w] = __builtin_amdgcn_raw_buffer_load_b64(rCol, in ? (int)(first * 2u) : -1, 0, NT ? PS_STREAM_AUX : 0);
        if constexpr (!F64) s.v[w] = __builtin_amdgcn_raw_buffer_load_b32(rCode, in ? (int)first : -1, 0, NT ? PS_STREAM_AUX : 0);
    }
}
__device__ inline unsigned streamCol(u32x2 c, int j, int myBase) {   // window base (lane `window` of every 16-lane group) + 12-bit offset
    const unsigned w = j < 2 ? c.x : c.y;
    const unsigned raw = (w >> (16 * (j & 1))) & 0xffffu;
    return (unsigned)__shfl(myBase, (int)(raw >> 12), 16) + (raw & 4095u);
}
__device__ inline double streamVal(unsigned v, int j, double scale) {   // exact: see DevCSR::code
    return (double)((int)(v << (24 - 8 * j)) >> 24) * scale;
}
__device__ inline double streamVal(const u32x4 (&v)[2], int j, double) {
    const u32x4 q = v[j >> 1];
    const u32x2 h = (j & 1) ? u32x2{q.z, q.w} : u32x2{q.x, q.y};
    return __builtin_bit_cast(double, h);
}
template <bool F64, class S, class V>
__device__ inline double prodVal(const S& cur, const V& cv, int w, int j, double scale) {
    if constexpr (F64) return streamVal(cv.v[w], j, scale); else return streamVal(cur.v[w], j, scale);
}
// inclusive prefix sum over the 64 lanes with DPP moves (VALU only, no LDS round trips): Hillis-Steele inside each row of
// 16 lanes (row_shr 1,2,4,8; lanes without a source keep 0), then row_bcast:15 into rows 1,3 and row_bcast:31 into rows 2,3
__device__ inline int waveInclusiveScan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return v;
}
// wave sum of a double with DPP moves only (no LDS-pipe bpermutes): same row_shr / row_bcast ladder as the scan above on the two
// 32-bit halves; the total lands in lane 63 (the other lanes hold partial prefix sums)
__device__ inline double waveSumToLane63(double v) {
#define PS_DPP_STEP(CTRL, RMASK)                                                                                   \
    {                                                                                                               \
        const long long b = __double_as_longlong(v);                                                                \
        const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, RMASK, 0xf, false);            \
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, RMASK, 0xf, false);                     \
        v += __longlong_as_double(((long long)hi << 32) | (unsigned)lo);                                            \
    }
    PS_DPP_STEP(0x111, 0xf) PS_DPP_STEP(0x112, 0xf) PS_DPP_STEP(0x114, 0xf) PS_DPP_STEP(0x118, 0xf)
    PS_DPP_STEP(0x142, 0xa) PS_DPP_STEP(0x143, 0xc)
#undef PS_DPP_STEP
    return v;
}
// sum of the row's products prod[ea .. ea+len) in entry order; all (<= ML) LDS reads are issued up front
template <int ML, int PL>
__device__ inline double rowSum(const double* prod, int ea, int len) {
    double v[ML];
#pragma unroll
    for (int k = 0; k < ML; ++k) { const int e = min(ea + k, 4 * PL - 1); v[k] = prod[(e & 3) * PL + (e >> 2)]; }
    double s = 0.;
#pragma unroll
    for (int k = 0; k < ML; ++k) s = k < len ? s + v[k] : s;
    return s;
}
// ---- pieces the persistent kernels share ------------------------------------------------------------------------------------
// Each of them exists ONCE: the kernels below differ in how the stream is laid out and walked, not in what a row's epilogue computes, and the
// forced forms are compared against one oracle — the copies had to stay bit-identical to each other.
//
// Scalars of the PCG step that every workgroup forms itself (ps_kernels_cg.hpp: k_cg_update_r, k_cg_check use the same two helpers)
__device__ inline double sumLocal(const double* __restrict__ partial, int count) {   // this thread's share (fixed stride order)
    double acc = 0.;
    for (int i = threadIdx.x; i < count; i += BS) acc += partial[i];
    return acc;
}
// PASS: a pass of the mixed-precision solve (ps_solve.hip: solve, PS_PRECISION_MIXED) — x.x frozen at the pass's start where the pass does not
// build x itself (sc->xxFix > 0), and the pass also ends once r.r has fallen to sc->rrFloor; the fp64 kernels read neither field
template <bool PASS = false>
__device__ inline bool stopTest(CGScalars* sc, double xx, int iterIndex, bool writer) {
    const double rr = sc->rr;
    if (PASS && sc->xxFix > 0.) xx = sc->xxFix;
    double rre = rr;                                   // pcg.h:319-325
    if (rr / xx < rre) rre = rr / xx;
    const bool fire = rre < sc->tol2 || (PASS && rr < sc->rrFloor);
    if (writer) { sc->xx = xx; sc->rre = rre; if (fire) { sc->done = 1; sc->iter = iterIndex; } }
    return fire;
}
// Prologue of the fused residual update, as k_cg_update_r: [stop test of iteration it-1], alpha = rsold / p.Ap — identical in every
// workgroup (each sums the partials itself, in the same order), workgroup 0 records the scalars.  reduced: the sums come all-reduced in
// fr.red.  Returns false when the stop test fired (same verdict in every workgroup: the kernel returns).
template <bool PASS = false>
__device__ __forceinline__ bool fusedPrologue(const FusedR& fr, bool reduced, double& alpha) {
    CGScalars* sc = fr.sc;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    if (fr.it > 0 && stopTest<PASS>(sc, reduced ? fr.red[1] : blockSumAll(sumLocal(fr.xxPart, fr.xxCount)), fr.it - 1, writer)) return false;
    const double pAp = reduced ? -fr.red[0]
                               : -(blockSumAll(sumLocal(fr.sPart, fr.sCount)) + blockSumAll(sumLocal(fr.tPart, fr.tCount)) + 0.5 * blockSumAll(sumLocal(fr.uPart, fr.uCount)));
    alpha = sc->rsold2[fr.it & 1] / pAp;               // pcg.h:314
    if (writer) { sc->pAp = pAp; sc->alpha = alpha; }
    return true;
}

// A per-row diagonal — the face mass McInv of the S kernels, the stress diagonal uInv of the St kernels — comes as one-byte codes into a
// 256-entry table in LDS (CODED; ps_context.hpp: mcCode / uCode) or, when it takes more than 256 values (a density or viscosity FIELD), as
// the fp64 array: 7 more bytes per row.  fill: the table (first read after a barrier of the caller); load: the row's byte at `srow` (the row
// of the chunk whose run this is: the byte streams go with the runs) or its 8 bytes at `row`, AUX = the site's cache policy; value: the lookup.
struct DiagRow { int code; double v; };
template <bool CODED> struct RowDiag {
    __device__ static inline void fill(double* dict, const double* __restrict__ table) { if (CODED) dict[threadIdx.x] = table[threadIdx.x]; }
    template <int AUX> __device__ static inline DiagRow load(__amdgpu_buffer_rsrc_t r, unsigned row, unsigned srow) {
        if constexpr (CODED) return DiagRow{(int)__builtin_amdgcn_raw_buffer_load_b8(r, (int)srow, 0, AUX), 0.};
        else return DiagRow{0, __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)(row * 8u), 0, AUX))};
    }
    __device__ static inline double value(const double* dict, const DiagRow& d) { if constexpr (CODED) return dict[d.code]; else return d.v; }
};
// the form chosen at run time (the kernels that take both arrays): rc = the codes, rv = the fp64 array
template <int CAUX, int VAUX> __device__ inline DiagRow rowDiagLoad(bool coded, __amdgpu_buffer_rsrc_t rc, __amdgpu_buffer_rsrc_t rv, unsigned row, unsigned srow) {
    if (coded) return RowDiag<true>::load<CAUX>(rc, row, srow);
    return RowDiag<false>::load<VAUX>(rv, row, srow);
}
__device__ inline double rowDiagValue(bool coded, const double* dict, const DiagRow& d) { return coded ? RowDiag<true>::value(dict, d) : RowDiag<false>::value(dict, d); }

constexpr unsigned ROW_NONE = 0x1fffffffu;   // row index of an idle lane: beyond any array (rows * 8 < 4 GiB), positive as an int
// ---- row epilogues
// S: t[row] = (row < nA ? dt McInv[row] : 1) s (MODE 0; MODE 1: s), stAcc += s t on the ACTIVE rows — their share of x . A x = sum s_f t_f
// (idle lanes: row = ROW_NONE is past nA and past the output buffer: the store is dropped)
template <int MODE, bool NT, class TV>
__device__ __forceinline__ void sRowFinish(__amdgpu_buffer_rsrc_t rOut, unsigned row, int nA, double dt, double mc, double s, double& stAcc) {
    const double sc = (MODE == 0 && (int)row < nA) ? dt * mc : 1.;
    if (MODE == 0) stAcc += (int)row < nA ? s * (s * sc) : 0.;
    VecIO<TV>::template store<NT>(rOut, row, s * sc);
}
// St: (A x)[row] = -(St t)[row] - 1/2 uInv[row] x[row]
__device__ __forceinline__ double stRowY(double s, double u, double x) {
    double y = -s;
    y -= 0.5 * u * x;
    return y;
}
// MODE 2, one Chebyshev term: z_{j+1} = z_j + c1 (z_j - z_{j-1}) + c2 dinv (r - A z_j), r.z of the updated z AS STORED (TV; 0 past the
// last row: every load returned 0)
struct ChebRow { double cr, ci, cd; };   // r, dinv, z_{j-1} (0: no buffer) of the row
template <class TV>
__device__ __forceinline__ ChebRow chebLoads(__amdgpu_buffer_rsrc_t rCr, __amdgpu_buffer_rsrc_t rCi, __amdgpu_buffer_rsrc_t rCd, unsigned row) {
    return ChebRow{bufLoadF64(rCr, row * 8u), (double)bufLoadDiag<false>(rCi, row), VecIO<TV>::load(rCd, row)};
}
template <class TV>
__device__ __forceinline__ double chebRowFinish(const ChebArgs& cheb, const ChebRow& c, double az, double z, double& dacc) {
    const double y = VecIO<TV>::stored(z + (cheb.c1 * (z - c.cd) + cheb.c2 * (c.ci * (c.cr - az))));
    dacc += c.cr * y;
    return y;
}
// MODE 3, the residual update on a row whose y = (A p)[row] is still in a register (never stored).  The flags are compile-time constants
// where the kernel knows them (k_spmv_St_ell2: HALO, CZ) and run-time tests of fr.yOut / fr.cz where it does not (the _pipe and one-unit
// kernels); fr.dinvF is a run-time test everywhere.
//   ranged: rows outside [fr.ownLo, fr.ownHi) are not this rank's (false: every live row is);  halo: such a row's y goes to fr.yOut;
//   cz: the Chebyshev polynomial's first term z_1 = dinv r / theta -> fr.cz (elements TZ), r.z formed with z_1 AS STORED; without it
//   r.z is that of the Jacobi diagonal fr.dinvF (null: none asked for) — never both (FusedR).
//   TV: element type r is stored in (float: the mixed-precision solve — fr.r then points at floats, and r.r / r.z are formed with r AS STORED)
struct FusedBufs { __amdgpu_buffer_rsrc_t r, dinv, dinvC, cz, y; };
template <class TZ, class TV = double>
__device__ inline FusedBufs fusedBufs(const FusedR& fr, int rows, bool on, bool halo, bool cz) {
    return FusedBufs{bufRsrc(fr.r, on ? (size_t)rows * sizeof(TV) : 0), bufRsrc(fr.dinvF, (on && !cz && fr.dinvF) ? (size_t)rows * sizeof(diag_t) : 0),
                     bufRsrc(fr.dinvC, (on && cz) ? (size_t)rows * sizeof(diag_t) : 0), bufRsrc(fr.cz, (on && cz) ? (size_t)rows * sizeof(TZ) : 0),
                     bufRsrc(fr.yOut, (on && halo) ? (size_t)rows * 8 : 0)};
}
struct FusedRow { double cr, ci; float fd; };   // r, the polynomial's diagonal (cz), the Jacobi diagonal (1: identity) of the row
template <bool NT, class TV = double>
__device__ __forceinline__ FusedRow fusedLoads(const FusedR& fr, const FusedBufs& B, unsigned row, bool cz) {
    FusedRow L{VecIO<TV>::template loadEpi<NT>(B.r, row), 0., 1.f};
    if (cz) L.ci = (double)bufLoadDiag<NT>(B.dinvC, row);
    else if (fr.dinvF) L.fd = bufLoadDiag<NT>(B.dinv, row);
    return L;
}
template <bool NT, class TZ, class TV = double>
__device__ __forceinline__ void fusedRowFinish(const FusedR& fr, const FusedBufs& B, unsigned row, bool live, bool ranged, bool halo, bool cz, double alpha, double y,
                                               const FusedRow& L, double& dacc, double& dacc2) {
    const bool mine = ranged ? ((int)row >= fr.ownLo && (int)row < fr.ownHi) : live;   // (idle lanes: ROW_NONE is beyond ownHi)
    if (halo) bufStoreF64nt<NT>(B.y, (!mine && live) ? row * 8u : 0xfffffff8u, y);    // a neighbour's row: its share of A p
    const double rv = mine ? VecIO<TV>::stored(L.cr - alpha * y) : 0.;                // pcg.h:316
    dacc += rv * rv;
    if (cz) {                                                                          // k_cheb_first on this row
        const double v = VecIO<TZ>::stored(L.ci * rv * fr.invTheta);
        VecIO<TZ>::template store<NT>(B.cz, row, v);
        dacc2 += rv * v;
    } else if (fr.dinvF) dacc2 += (!ranged || mine) ? rv * ((double)L.fd * rv) : 0.;   // (the diagonal of a halo row is not this rank's: may be anything)
    VecIO<TV>::template store<NT>(B.r, (!ranged || mine) ? row : ROW_NONE, rv);
}
// the workgroup's partials of r.r at fr.rPart[block], of r.z at fr.rPart[stride + block]
__device__ __forceinline__ void fusedPartials(const FusedR& fr, double dacc, double dacc2, bool cz, int stride) {
    const double b0 = blockReduceSum(dacc), b1 = (cz || fr.dinvF) ? blockReduceSum(dacc2) : 0.;
    if (threadIdx.x == 0) { fr.rPart[blockIdx.x] = b0; fr.rPart[stride + blockIdx.x] = b1; }
}

// The St row of the kernels that take MODE at compile time and everything else at run time (k_spmv_St_pipe, k_spmv_St_ell):
// MODE 0: out = A x, partial of x . A x;  MODE 1: out = -(St t) + add;  MODE 2 / 3: above
struct StBufs { __amdgpu_buffer_rsrc_t e0, e1, uc, out, cr, ci, cd; FusedBufs f; };
template <int MODE>
__device__ inline StBufs stBufs(int rows, const double* uInv, const double* xin, const double* add, double* out, const ChebArgs& cheb, const uint8_t* uCode, bool coded,
                                const FusedR& fr) {
    return StBufs{bufRsrc(MODE == 1 ? add : xin, (size_t)rows * 8), bufRsrc(uInv, (size_t)rows * 8), bufRsrc(uCode, coded ? (size_t)rows : 0),
                  bufRsrc(out, (size_t)rows * 8), bufRsrc(cheb.r, MODE == 2 ? (size_t)rows * 8 : 0), bufRsrc(cheb.dinv, MODE == 2 ? (size_t)rows * sizeof(diag_t) : 0),
                  bufRsrc(cheb.zprev, (MODE == 2 && cheb.zprev) ? (size_t)rows * 8 : 0),
                  fusedBufs<double>(fr, rows, MODE == 3, fr.yOut != nullptr, fr.cz != nullptr)};
}
struct StRow { double e0; DiagRow u; ChebRow c; FusedRow f; };
template <int MODE, bool NT, int CAUX>
__device__ __forceinline__ StRow stRowLoads(const StBufs& B, const FusedR& fr, bool coded, unsigned row, unsigned srow) {
    StRow L{bufLoadF64epi<NT>(B.e0, row * 8u), DiagRow{0, 0.}, ChebRow{0., 0., 0.}, FusedRow{0., 0., 1.f}};   // e0: x (MODE 0, 2, 3) / the vector added (MODE 1)
    if (MODE != 1) L.u = rowDiagLoad<CAUX, NT ? PS_EPI_AUX : 0>(coded, B.uc, B.e1, row, srow);
    if (MODE == 2) L.c = chebLoads<double>(B.cr, B.ci, B.cd, row);
    if (MODE == 3) L.f = fusedLoads<NT>(fr, B.f, row, fr.cz != nullptr);
    return L;
}
template <int MODE, bool NT>
__device__ __forceinline__ void stRowFinish(const StBufs& B, const ChebArgs& cheb, const FusedR& fr, const double* dict, bool coded, double alpha, unsigned row, bool live,
                                            const StRow& L, double s, double& dacc, double& dacc2) {
    if (MODE == 1) { bufStoreF64nt<NT>(B.out, row * 8u, -s + L.e0); return; }
    const double y = stRowY(s, rowDiagValue(coded, dict, L.u), L.e0);
    if (MODE == 0) { dacc += L.e0 * y; bufStoreF64nt<NT>(B.out, row * 8u, y); }   // p.Ap: running sum over this block's chunks (0 past the last row)
    else if (MODE == 2) bufStoreF64nt<NT>(B.out, row * 8u, chebRowFinish<double>(cheb, L.c, y, L.e0, dacc));
    else fusedRowFinish<NT, double>(fr, B.f, row, live, true, fr.yOut != nullptr, fr.cz != nullptr, alpha, y, L.f, dacc, dacc2);
}

// chunkInfo entry (DevCSR::chunkInfo): x = first entry of the run, y = entries | rows << 16, z = first row, w = first row of the
// chunk whose run this is (== z unless the run is shared: the per-row BYTE streams — lengths, value-set codes — are read there too)
struct Chunk { int q0, q1, row0, rows, src; };
__host__ __device__ inline Chunk decodeChunk(int4 v) { return Chunk{v.x, v.x + (v.y & 0xffff), v.z, (int)((unsigned)v.y >> 16), v.w}; }
// The loop of k_spmv_S_pipe / k_spmv_St_pipe: gathers of the current chunk, prefetch of the next, products to LDS (entry e of the chunk at
// prod[(e & 3) * PL + (e >> 2)]: conflict-free writes), row offsets from the length bytes (wave scans + 4 wave totals).
// loads(row, srow): the kernel issues the per-row loads of its epilogue (before the gathers);  finish(row, live, loaded, s): the row's sum
// (at most ML entries) -> the epilogue.  Returns false when the workgroup has no chunk (nothing was done).
#define PS_INLINE_LAMBDA __attribute__((always_inline))   // the callables of the loops are called once per unit: they must vanish, or what they capture goes to memory
template <int NV, bool F64, bool SNT, bool BNT, int ML, class Loads, class Row>
__device__ __forceinline__ bool pipeLoop(const uint16_t* __restrict__ col16, const int8_t* __restrict__ code4, const double* __restrict__ val4, int streamLen,
                                         const int32_t* __restrict__ winBase, const int4* __restrict__ chunkInfo, const uint8_t* __restrict__ len8, double scale,
                                         __amdgpu_buffer_rsrc_t rX, int rows, int nChunks, int xcdAware, const Loads& loads, const Row& finish) {
    constexpr int PL = BS * NV;
    __shared__ double prod[4 * PL];
    __shared__ __align__(16) int wtot[BS / 64];
    static_assert(BS == 256, "four waves per block");
    const __amdgpu_buffer_rsrc_t rCol = bufRsrc(col16, (size_t)streamLen * 2), rCode = bufRsrc(code4, F64 ? 0 : (size_t)streamLen), rLen = bufRsrc(len8, (size_t)rows);
    const ChunkWalk W(xcdAware);
    int it = 0;
    int chunk = W.at(0);
    if (chunk >= nChunks) return false;
    Chunk pr = decodeChunk(chunkInfo[chunk]);
    Stream4<NV, F64> cur, nxt;
    loadStream4<NV, F64, SNT>(rCol, rCode, val4, pr.q0, pr.q1, cur);
    int myBase = winBase[chunk * 16 + (threadIdx.x & 15)], nBase = 0;
    int nchunk = W.at(1);
    Chunk npr{0, 0, 0, 0, 0};
    if (nchunk < nChunks) npr = decodeChunk(chunkInfo[nchunk]);
    while (true) {
        const bool live = (int)threadIdx.x < pr.rows;                                   // lanes past the chunk's rows: every access out of range
        const unsigned row = live ? (unsigned)pr.row0 + threadIdx.x : ROW_NONE, srow = live ? (unsigned)pr.src + threadIdx.x : ROW_NONE;
        const int len = (int)__builtin_amdgcn_raw_buffer_load_b8(rLen, (int)srow, 0, BNT ? PS_EPI_AUX : 0);   // 0 past the last row
        const auto L = loads(row, srow);
        double xv[4 * NV];
#pragma unroll
        for (int w = 0; w < NV; ++w) {
            if (w > 0 && pr.q0 + 4 * w * BS >= pr.q1) break;                  // block-uniform: this group of the chunk is empty
#pragma unroll
            for (int j = 0; j < 4; ++j) xv[4 * w + j] = bufGatherF64(rX, streamCol(cur.c[w], j, myBase) * 8u);
        }
        Vals4<F64 ? NV : 0> cv;
        if constexpr (F64) loadVals4<NV, SNT>(val4, pr.q0, pr.q1, cv);
        const bool hasNext = nchunk < nChunks;
        if (hasNext) {
            loadStream4<NV, F64, SNT>(rCol, rCode, val4, npr.q0, npr.q1, nxt);
            nBase = winBase[nchunk * 16 + (threadIdx.x & 15)];
        }
        const int nn = W.at(it + 2);
        Chunk nnpr{0, 0, 0, 0, 0};
        if (nn < nChunks) nnpr = decodeChunk(chunkInfo[nn]);
#pragma unroll
        for (int w = 0; w < NV; ++w) {
            if (w > 0 && pr.q0 + 4 * w * BS >= pr.q1) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) prod[j * PL + threadIdx.x + w * BS] = prodVal<F64>(cur, cv, w, j, scale) * xv[4 * w + j];
        }
        const int incl = waveInclusiveScan(len);
        if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = incl;
        __syncthreads();
        {
            const int4 wt = *reinterpret_cast<const int4*>(wtot);
            const int wv = threadIdx.x >> 6;
            const int ea = incl - len + (wv > 0 ? wt.x : 0) + (wv > 1 ? wt.y : 0) + (wv > 2 ? wt.z : 0);
            finish(row, live, L, rowSum<ML, PL>(prod, ea, len));
        }
        __syncthreads();    // protects the LDS reuse
        if (!hasNext) break;
        chunk = nchunk; pr = npr; cur = nxt; myBase = nBase;
        nchunk = nn; npr = nnpr;
        ++it;
    }
    return true;
}
// MODE 0: out[row] = (row < nA ? dt*McInv[row] : 1) * (S x)[row]  (operator, forward half);  MODE 1: out[row] = (S x)[row]  (velocity recovery)
template <int MODE, int NV, bool F64, int POL>
__global__ void __launch_bounds__(BS) k_spmv_S_pipe(const uint16_t* __restrict__ col16, const int8_t* __restrict__ code4, const double* __restrict__ val4, int streamLen,
                                                    const int32_t* __restrict__ winBase, const int4* __restrict__ chunkInfo,
                                                    const uint8_t* __restrict__ len8, double scale, const double* __restrict__ x, int cols, int rows,
                                                    int nA, double dt, const double* __restrict__ McInv, double* __restrict__ out,
                                                    const int* __restrict__ done, int nChunks, int xcdAware,
                                                    const uint8_t* __restrict__ mcCode, const double* __restrict__ mcDict, double* __restrict__ stPart) {
    // stPart (MODE 0, may be null): per workgroup, the sum over its ACTIVE rows of s_f t_f = dt McInv_f s_f^2 — the active-face
    // share of x . A x, so that the residual update can run inside the St kernel (ps_solve.hip: fused step)
    if (done && *done) return;
    constexpr bool NT = (POL & 1) != 0, SNT = (POL & 2) != 0;   // stores + per-row epilogue streams | the matrix stream
    constexpr bool BNT = NT && SNT;                               // the per-row byte streams go with the runs: cached when runs are shared
    __shared__ double dict[MODE == 0 ? 256 : 1];      // value-set coded McInv: first read after the loop's first barrier
    const bool coded = mcCode != nullptr;
    if (MODE == 0 && coded) RowDiag<true>::fill(dict, mcDict);
    const __amdgpu_buffer_rsrc_t rX = bufRsrc(x, (size_t)cols * 8), rMc = bufRsrc(McInv, (size_t)nA * 8), rMcc = bufRsrc(mcCode, coded ? (size_t)nA : 0),
                                 rOut = bufRsrc(out, (size_t)rows * 8);
    double stAcc = 0.;
    const bool any = pipeLoop<NV, F64, SNT, BNT, 8>(col16, code4, val4, streamLen, winBase, chunkInfo, len8, scale, rX, rows, nChunks, xcdAware,
        [&](unsigned row, unsigned srow) PS_INLINE_LAMBDA { return MODE == 0 ? rowDiagLoad<BNT ? PS_EPI_AUX : 0, 0>(coded, rMcc, rMc, row, srow) : DiagRow{0, 0.}; },
        [&](unsigned row, bool, const DiagRow& m, double s) PS_INLINE_LAMBDA {
            sRowFinish<MODE, NT, double>(rOut, row, nA, dt, MODE == 0 ? rowDiagValue(coded, dict, m) : 1., s, stAcc);
        });
    if (!any) { if (MODE == 0 && stPart && threadIdx.x == 0) stPart[blockIdx.x] = 0.; return; }
    if (MODE == 0 && stPart) {
        const double bs = blockReduceSum(stAcc);
        if (threadIdx.x == 0) stPart[blockIdx.x] = bs;
    }
}
// MODE 0 .. 3: stRowFinish.  (It writes its r.z partials at gridDim.x + block: fr.rStride is not looked at — the decomposition does not launch it.)
template <int MODE, int NV, bool F64, int POL>
__global__ void __launch_bounds__(BS) k_spmv_St_pipe(const uint16_t* __restrict__ col16, const int8_t* __restrict__ code4, const double* __restrict__ val4, int streamLen,
                                                     const int32_t* __restrict__ winBase, const int4* __restrict__ chunkInfo,
                                                     const uint8_t* __restrict__ len8, double scale, const double* __restrict__ t, int cols, int rows,
                                                     const double* __restrict__ uInv, const double* __restrict__ xin, const double* __restrict__ add,
                                                     double* __restrict__ out, double* __restrict__ partial, const int* __restrict__ done,
                                                     int nChunks, int xcdAware, ChebArgs cheb,
                                                     const uint8_t* __restrict__ uCode, const double* __restrict__ uDict, FusedR fr) {
    if (done && *done) return;
    constexpr bool NT = (POL & 1) != 0, SNT = (POL & 2) != 0;   // stores + per-row epilogue streams | the matrix stream
    constexpr bool BNT = NT && SNT;                               // the per-row byte streams go with the runs: cached when runs are shared
    __shared__ double dict[MODE != 1 ? 256 : 1];      // value-set coded uInv
    const bool coded = uCode != nullptr;
    if (MODE != 1 && coded) RowDiag<true>::fill(dict, uDict);
    double alpha = 0.;
    if (MODE == 3 && !fusedPrologue(fr, fr.red != nullptr, alpha)) return;
    const __amdgpu_buffer_rsrc_t rT = bufRsrc(t, (size_t)cols * 8);
    const StBufs B = stBufs<MODE>(rows, uInv, xin, add, out, cheb, uCode, coded, fr);
    double dacc = 0., dacc2 = 0.;
    const bool any = pipeLoop<NV, F64, SNT, BNT, 6>(col16, code4, val4, streamLen, winBase, chunkInfo, len8, scale, rT, rows, nChunks, xcdAware,
        [&](unsigned row, unsigned srow) PS_INLINE_LAMBDA { return stRowLoads<MODE, NT, BNT ? PS_EPI_AUX : 0>(B, fr, coded, row, srow); },
        [&](unsigned row, bool live, const StRow& L, double s) PS_INLINE_LAMBDA { stRowFinish<MODE, NT>(B, cheb, fr, dict, coded, alpha, row, live, L, s, dacc, dacc2); });
    if (!any) {
        if ((MODE == 0 || MODE == 2) && threadIdx.x == 0) partial[blockIdx.x] = 0.;
        if (MODE == 3 && threadIdx.x == 0) { fr.rPart[blockIdx.x] = 0.; fr.rPart[gridDim.x + blockIdx.x] = 0.; }
        return;
    }
    if (MODE == 0 || MODE == 2) {
        const double bs = blockReduceSum(dacc);
        if (threadIdx.x == 0) partial[blockIdx.x] = bs;   // gridDim.x partials (Launch::stBlocks)
    }
    if (MODE == 3) fusedPartials(fr, dacc, dacc2, fr.cz != nullptr, (int)gridDim.x);
}


// ---- row-per-lane kernels on DevCSR::ecol / ecode (ps_blocks.hip:buildEll) ------------------------------------------------
// Why (profiles/r03_spmv_issue.md): the CU's vector-memory path walks a gather instruction one aligned quad of lanes per cycle and
// pays one L1 tag lookup per DISTINCT 128-byte line in the quad.  With 4 consecutive stream entries per lane (kernels above) the
// lanes of a quad hold entries 16 apart — four lines, four cycles: both SpMVs sat at 0.8 lookups per cycle and CU, the L1 pipeline
// saturated while 86 % of the lookups hit.  Here a lane owns a ROW: instruction k gathers entry k of 64 consecutive rows (the three
// faces of a voxel, then the next voxel), so the lanes of a quad address the same or neighbouring lines.  The row's sum stays in a
// register: no products through LDS, no row-length scan, no barrier; the four waves of a workgroup walk the chunk list together but
// never wait for each other.  Same products, same summation order as the kernels above: bit-identical results.
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
struct EllUnit { int W, colByte, codeByte, row0, rows; };   // wave-uniform
__device__ inline EllUnit ellUnit(int4 ci, int wv) {
    const unsigned ws = (unsigned)ci.w >> 12;
    int pre = 0, preC = 0;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int w = (int)((ws >> (4 * u)) & 15u);
        if (u < wv) { pre += w; preC += w > 4 ? 8 : (w > 0 ? 4 : 0); }
    }
    EllUnit e;
    e.W = (int)((ws >> (4 * wv)) & 15u);
    e.colByte = ci.x * 2 + 128 * pre;
    e.codeByte = ci.y + 64 * preC;
    e.row0 = ci.z + 64 * wv;
    e.rows = min(64, max(0, (ci.w & 0xfff) - 64 * wv));
    if (e.rows == 0) e.W = 0;
    return e;
}
struct EllRegs { unsigned c0, c1, c2, c3, v0, v1; };   // scalars, every one written by every path: arrays written in part went to scratch memory
template <bool NT>
__device__ inline EllRegs ellLoad(__amdgpu_buffer_rsrc_t rCol, __amdgpu_buffer_rsrc_t rCode, const EllUnit& e, unsigned lane) {
    constexpr int AUX = NT ? PS_STREAM_AUX : 0;
    const int cb = e.colByte + (int)lane * 2 * e.W;
    EllRegs r{0u, 0u, 0u, 0u, 0u, 0u};
    if (e.W == 8) {
        const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(rCol, cb, 0, AUX);
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rCode, e.codeByte + (int)lane * 8, 0, AUX);
        r = EllRegs{q.x, q.y, q.z, q.w, v.x, v.y};
    } else if (e.W == 6) {
        const u32x3 q = __builtin_amdgcn_raw_buffer_load_b96(rCol, cb, 0, AUX);
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rCode, e.codeByte + (int)lane * 8, 0, AUX);
        r = EllRegs{q.x, q.y, q.z, 0u, v.x, v.y};
    } else if (e.W == 4) {
        const u32x2 q = __builtin_amdgcn_raw_buffer_load_b64(rCol, cb, 0, AUX);
        const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(rCode, e.codeByte + (int)lane * 4, 0, AUX);
        r = EllRegs{q.x, q.y, 0u, 0u, v, 0u};
    } else if (e.W == 2) {
        const unsigned q = __builtin_amdgcn_raw_buffer_load_b32(rCol, cb, 0, AUX);
        const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(rCode, e.codeByte + (int)lane * 4, 0, AUX);
        r = EllRegs{q, 0u, 0u, 0u, v, 0u};
    }
    return r;
}
template <int K> __device__ inline unsigned ellColWord(const EllRegs& r) { return K < 2 ? r.c0 : (K < 4 ? r.c1 : (K < 6 ? r.c2 : r.c3)); }
// the row's W gathers (all in flight together), and — after the caller has issued its prefetches behind them — the products in
// entry order (CSR order)
struct EllX { double x0, x1, x2, x3, x4, x5, x6, x7; };
template <int W, class T = double>
__device__ inline EllX ellGather(const EllRegs& r, int myBase, __amdgpu_buffer_rsrc_t rX) {
    const unsigned cw[4] = {r.c0, r.c1, r.c2, r.c3};
    double xv[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const unsigned raw = (cw[k >> 1] >> (16 * (k & 1))) & 0xffffu;
        const unsigned col = (unsigned)__shfl(myBase, (int)(raw >> 12), 16) + (raw & 4095u);
        xv[k] = VecIO<T>::gather(rX, col);
    }
    return EllX{xv[0], xv[1], xv[2], xv[3], xv[4], xv[5], xv[6], xv[7]};
}
template <class T = double>
__device__ inline EllX ellGatherW(int W, const EllRegs& r, int myBase, __amdgpu_buffer_rsrc_t rX) {
    if (W == 8) return ellGather<8, T>(r, myBase, rX);
    if (W == 6) return ellGather<6, T>(r, myBase, rX);
    if (W == 4) return ellGather<4, T>(r, myBase, rX);
    if (W == 2) return ellGather<2, T>(r, myBase, rX);
    return EllX{0., 0., 0., 0., 0., 0., 0., 0.};
}
template <int W>
__device__ inline double ellSum(const EllRegs& r, const EllX& X, double scale) {
    const unsigned vw[2] = {r.v0, r.v1};
    const double xv[8] = {X.x0, X.x1, X.x2, X.x3, X.x4, X.x5, X.x6, X.x7};
    double s = 0.;
#pragma unroll
    for (int k = 0; k < W; ++k) s += streamVal(vw[k >> 2], k & 3, scale) * xv[k];
    return s;
}
__device__ inline double ellSumW(int W, const EllRegs& r, const EllX& X, double scale) {
    if (W == 8) return ellSum<8>(r, X, scale);
    if (W == 6) return ellSum<6>(r, X, scale);
    if (W == 4) return ellSum<4>(r, X, scale);
    if (W == 2) return ellSum<2>(r, X, scale);
    return 0.;
}
// The loop of the one-unit kernels k_spmv_S_ell / k_spmv_St_ell: a wave owns unit `wave` of every chunk of its workgroup's ChunkWalk.
// LIST: `list` holds the chunks this launch works on, nChunks of them — the slab decomposition runs the chunks that touch no
// halo column while the halo values are still in flight, and the others afterwards (ps_dist.hpp).  A template parameter: the
// single-domain kernels must not pay registers for it (the plain MODE 3 St kernel sits at the edge of 7 waves per SIMD)
// loads(row): the per-row loads of the kernel's epilogue;  finish(row, live, loaded, s): the row's sum -> the epilogue
template <bool SNT, bool LIST, class Loads, class Row>
__device__ __forceinline__ void ellLoop(__amdgpu_buffer_rsrc_t rCol, __amdgpu_buffer_rsrc_t rCode, __amdgpu_buffer_rsrc_t rX, const int32_t* __restrict__ winBase,
                                        const int4* __restrict__ echunk, double scale, int nChunks, int xcdAware, const int32_t* __restrict__ list,
                                        const Loads& loads, const Row& finish) {
    const ChunkWalk Wk(xcdAware);
    const unsigned lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int it = 0;
    int chunk = Wk.at(0);                                               // POSITIONS in the walk (< nChunks); the chunk itself is list[position] when there is a list
    if (chunk >= nChunks) return;
    const int id0 = LIST ? list[chunk] : chunk;
    EllUnit cu = ellUnit(echunk[id0], wv);
    EllRegs cur = ellLoad<SNT>(rCol, rCode, cu, lane), nxt{0u, 0u, 0u, 0u, 0u, 0u};
    int myBase = winBase[id0 * 16 + (lane & 15)], nBase = 0;
    int nchunk = Wk.at(1), nid = 0;
    int4 nci = make_int4(0, 0, 0, 0);
    if (nchunk < nChunks) { nid = LIST ? list[nchunk] : nchunk; nci = echunk[nid]; }
    while (true) {
        // (1) the per-row streams of the epilogue and this unit's gathers first: their address arithmetic waits on nothing but the window lookups
        const bool live = (int)lane < cu.rows;
        const unsigned row = live ? (unsigned)cu.row0 + lane : ROW_NONE;
        const auto L = loads(row);
        const EllX X = ellGatherW(cu.W, cur, myBase, rX);
        // (2) behind them: the next unit's stream and the record of the chunk after it
        const bool hasNext = nchunk < nChunks;
        EllUnit nu{0, 0, 0, 0, 0};
        if (hasNext) {
            nu = ellUnit(nci, wv);
            nxt = ellLoad<SNT>(rCol, rCode, nu, lane);
            nBase = winBase[nid * 16 + (lane & 15)];
        }
        const int nn = Wk.at(it + 2);
        int nnid = 0;
        int4 nnci = make_int4(0, 0, 0, 0);
        if (nn < nChunks) { nnid = LIST ? list[nn] : nn; nnci = echunk[nnid]; }
        // (3) products, the row's sum and the epilogue
        finish(row, live, L, ellSumW(cu.W, cur, X, scale));
        if (!hasNext) break;
        chunk = nchunk; cu = nu; cur = nxt; myBase = nBase;
        nchunk = nn; nci = nnci; nid = nnid;
        ++it;
    }
}
// MODE 0 / 1 as k_spmv_S_pipe
template <int MODE, int POL, bool LIST>
__global__ void __launch_bounds__(BS) k_spmv_S_ell(const uint16_t* __restrict__ ecol, const int8_t* __restrict__ ecode, unsigned colBytes, unsigned codeBytes,
                                                   const int32_t* __restrict__ winBase, const int4* __restrict__ echunk, double scale,
                                                   const double* __restrict__ x, int cols, int rows, int nA, double dt, const double* __restrict__ McInv,
                                                   double* __restrict__ out, const int* __restrict__ done, int nChunks, int xcdAware,
                                                   const uint8_t* __restrict__ mcCode, const double* __restrict__ mcDict, double* __restrict__ stPart,
                                                   const int32_t* __restrict__ list) {
    if (done && *done) return;
    constexpr bool NT = (POL & 1) != 0, SNT = (POL & 2) != 0;
    __shared__ double dict[MODE == 0 ? 256 : 1];
    const bool coded = mcCode != nullptr;
    if (MODE == 0 && coded) RowDiag<true>::fill(dict, mcDict);
    __syncthreads();                                                    // the only barrier before the final reduction
    const __amdgpu_buffer_rsrc_t rCol = bufRsrc(ecol, colBytes), rCode = bufRsrc(ecode, codeBytes), rX = bufRsrc(x, (size_t)cols * 8),
                                 rMc = bufRsrc(McInv, (size_t)nA * 8), rMcc = bufRsrc(mcCode, coded ? (size_t)nA : 0), rOut = bufRsrc(out, (size_t)rows * 8);
    double stAcc = 0.;
    ellLoop<SNT, LIST>(rCol, rCode, rX, winBase, echunk, scale, nChunks, xcdAware, list,
        [&](unsigned row) PS_INLINE_LAMBDA { return MODE == 0 ? rowDiagLoad<NT ? PS_EPI_AUX : 0, 0>(coded, rMcc, rMc, row, row) : DiagRow{0, 0.}; },
        [&](unsigned row, bool, const DiagRow& m, double s) PS_INLINE_LAMBDA {
            sRowFinish<MODE, NT, double>(rOut, row, nA, dt, MODE == 0 ? rowDiagValue(coded, dict, m) : 1., s, stAcc);   // dropped past the chunk's last row (row = ROW_NONE)
        });
    if (MODE == 0 && stPart) {
        const double bs = blockReduceSum(stAcc);
        if (threadIdx.x == 0) stPart[blockIdx.x] = bs;
    }
}
// MODE 0 .. 3 as k_spmv_St_pipe (same prologue, same per-row epilogue, same thread <-> row assignment: bit-identical partial sums)
// FX (MODE 3 only): facts about the launch as compile-time constants, each worth buffer descriptors and branches (the generic MODE 3
// needs 100 SGPRs, spills them into VGPR lanes and fits 6 waves per SIMD).  Bit 0: value-set coded uInv and no Chebyshev first term
// (the Jacobi / identity PCG step); bit 1: a single domain (no halo rows, no all-reduced sums, one launch); bit 2: a rank's launch over
// chunks of owned rows only (ps_dist.hpp: the St launch that runs under the exchange — most of a rank's rows).
template <int MODE, int POL, int FX, bool LIST>
__global__ void __launch_bounds__(BS) k_spmv_St_ell(const uint16_t* __restrict__ ecol, const int8_t* __restrict__ ecode, unsigned colBytes, unsigned codeBytes,
                                                    const int32_t* __restrict__ winBase, const int4* __restrict__ echunk, double scale,
                                                    const double* __restrict__ t, int cols, int rows, const double* __restrict__ uInv,
                                                    const double* __restrict__ xin, const double* __restrict__ add, double* __restrict__ out,
                                                    double* __restrict__ partial, const int* __restrict__ done, int nChunks, int xcdAware, ChebArgs cheb,
                                                    const uint8_t* __restrict__ uCode, const double* __restrict__ uDict, FusedR fr, const int32_t* __restrict__ list) {
    // list: as in k_spmv_S_ell
    if (done && *done) return;
    constexpr bool NT = (POL & 1) != 0, SNT = (POL & 2) != 0;
    static_assert(FX == 0 || MODE == 3, "FX: MODE 3 only");
    if (FX & 1) { fr.cz = nullptr; fr.dinvC = nullptr; uInv = nullptr; }                                              // (the launch site guarantees uCode != null)
    if (FX & 2) { fr.yOut = nullptr; fr.rStride = 0; fr.red = nullptr; fr.ownLo = 0; fr.ownHi = rows; }
    if (FX & 4) { fr.yOut = nullptr; fr.ownLo = 0; fr.ownHi = rows; }   // a rank of a decomposition, chunks of OWNED rows only (the launch under the exchange): no halo row to hand on
    const bool coded = (FX & 1) ? true : uCode != nullptr;
    __shared__ double dict[MODE != 1 ? 256 : 1];
    if (MODE != 1 && coded) RowDiag<true>::fill(dict, uDict);
    double alpha = 0.;
    if (MODE == 3 && !fusedPrologue(fr, fr.red != nullptr, alpha)) return;
    __syncthreads();                                       // dict
    const __amdgpu_buffer_rsrc_t rCol = bufRsrc(ecol, colBytes), rCode = bufRsrc(ecode, codeBytes), rT = bufRsrc(t, (size_t)cols * 8);
    const StBufs B = stBufs<MODE>(rows, uInv, xin, add, out, cheb, uCode, coded, fr);
    double dacc = 0., dacc2 = 0.;
    ellLoop<SNT, LIST>(rCol, rCode, rT, winBase, echunk, scale, nChunks, xcdAware, list,
        [&](unsigned row) PS_INLINE_LAMBDA { return stRowLoads<MODE, NT, NT ? PS_EPI_AUX : 0>(B, fr, coded, row, row); },
        [&](unsigned row, bool live, const StRow& L, double s) PS_INLINE_LAMBDA { stRowFinish<MODE, NT>(B, cheb, fr, dict, coded, alpha, row, live, L, s, dacc, dacc2); });
    if (MODE == 0 || MODE == 2) {
        const double bs = blockReduceSum(dacc);
        if (threadIdx.x == 0) partial[blockIdx.x] = bs;   // gridDim.x partials (Launch::stBlocks)
    }
    if (MODE == 3) fusedPartials(fr, dacc, dacc2, fr.cz != nullptr, fr.rStride > 0 ? fr.rStride : (int)gridDim.x);
}

// ---- two units in flight per wave (r04; default for the single-domain operator product, PS_S_DUAL=0 switches back) -------------------
// k_spmv_S_ell with twice the memory-level parallelism per wave: a workgroup takes TWO chunks per step, waves 0-1 the first, waves 2-3 the
// second; a wave owns units 2 (w & 1) and 2 (w & 1) + 1 of its chunk and has the streams, the gathers and the epilogue loads of both in
// flight before it sums either.  Same products, same order per row: bit-identical t; the per-workgroup partials of sum s.t group differently.
//
// The walk: pairs of consecutive chunks, runs of 32 pairs dealt to the XCDs round robin (workgroup b runs on XCD b & 7); workgroup l of an
// XCD takes steps q = l, l + per, ... below pairWalkEnd.  Plain integers, for the kernels and for the host (ps_solve.hip: Launch::noteWalk, pipeBlocks).
__host__ __device__ inline int pairWalkEnd(int nChunks) { return ((((nChunks + 1) >> 1) + 255) >> 8) << 5; }   // steps beyond the last run of 32 pairs per XCD
// step q on XCD xcd -> the pair, then the wave's half of it -> the chunk, or -1
__host__ __device__ inline int pairWalkChunk(int q, int xcd, int half, int nChunks) {
    const int pair = ((((q >> 5) << 3) + xcd) << 5) + (q & 31);
    const int ch = 2 * pair + half;
    return (pair < ((nChunks + 1) >> 1) && ch < nChunks) ? ch : -1;
}
template <bool LIST> struct PairWalk {   // LIST: as ellLoop (nChunks = entries of the list)
    int nChunks, xcd, half, per, qEnd;
    const int32_t* list;
    __device__ PairWalk(int n, int half_, const int32_t* list_)
        : nChunks(n), xcd(blockIdx.x & 7), half(half_), per(gridDim.x >> 3), qEnd(pairWalkEnd(n)), list(list_) {}
    __device__ int first() const { return blockIdx.x >> 3; }
    __device__ int at(int q) const {
        const int ch = q < qEnd ? pairWalkChunk(q, xcd, half, nChunks) : -1;
        return (LIST && ch >= 0) ? list[ch] : ch;
    }
};
// The loop of the two-unit kernels.  loads(row) / finish(row, live, loaded, s) as in ellLoop, called for unit A, then for unit B: sums
// that the epilogue accumulates keep their A-then-B order.
template <bool SNT, bool LIST, class TX, class Loads, class Row>
__device__ __forceinline__ void ell2Loop(__amdgpu_buffer_rsrc_t rCol, __amdgpu_buffer_rsrc_t rCode, __amdgpu_buffer_rsrc_t rX, const int32_t* __restrict__ winBase,
                                         const int4* __restrict__ echunk, double scale, int nChunks, const int32_t* __restrict__ list, const Loads& loads, const Row& finish) {
    const unsigned lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int u0 = 2 * (wv & 1);
    const PairWalk<LIST> W(nChunks, wv >> 1, list);
    int q = W.first();
    int chunk = W.at(q);
    int4 ci = make_int4(0, 0, 0, 0);
    int myBase = 0;
    if (chunk >= 0) { ci = echunk[chunk]; myBase = winBase[chunk * 16 + (lane & 15)]; }
    while (q < W.qEnd) {
        const int qn = q + W.per;
        const int nchunk = W.at(qn);
        int4 nci = make_int4(0, 0, 0, 0);
        int nBase = 0;
        if (chunk >= 0) {
            const EllUnit ua = ellUnit(ci, u0), ub = ellUnit(ci, u0 + 1);
            const EllRegs sa = ellLoad<SNT>(rCol, rCode, ua, lane), sb = ellLoad<SNT>(rCol, rCode, ub, lane);
            if (nchunk >= 0) { nci = echunk[nchunk]; nBase = winBase[nchunk * 16 + (lane & 15)]; }     // the next step's record, behind this step's streams
            const bool liveA = (int)lane < ua.rows, liveB = (int)lane < ub.rows;
            const unsigned rowA = liveA ? (unsigned)ua.row0 + lane : ROW_NONE, rowB = liveB ? (unsigned)ub.row0 + lane : ROW_NONE;
            const auto LA = loads(rowA);
            const auto LB = loads(rowB);
            const EllX XA = ellGatherW<TX>(ua.W, sa, myBase, rX);
            const EllX XB = ellGatherW<TX>(ub.W, sb, myBase, rX);
            const double a = ellSumW(ua.W, sa, XA, scale), b = ellSumW(ub.W, sb, XB, scale);
            finish(rowA, liveA, LA, a);
            finish(rowB, liveB, LB, b);
        } else if (nchunk >= 0) { nci = echunk[nchunk]; nBase = winBase[nchunk * 16 + (lane & 15)]; }
        q = qn; chunk = nchunk; ci = nci; myBase = nBase;
    }
}
// TV: element type of x and of the output (double; float = the inner applies of the single-precision Chebyshev polynomial, VecIO)
// MC: the face mass McInv comes coded (true) or as the fp64 array itself, passed in mcCode's place and read through the same buffer policy
// (RowDiag; the St kernels' UC for the stress diagonal)
// The coded form launches as k_spmv_S_ell2, the uncoded one as k_spmv_S_ell2u (one body, spmvSEll2).
template <int POL, bool LIST, class TV, bool MC>
__device__ __forceinline__ void spmvSEll2(const uint16_t* __restrict__ ecol, const int8_t* __restrict__ ecode, unsigned colBytes, unsigned codeBytes,
                                          const int32_t* __restrict__ winBase, const int4* __restrict__ echunk, double scale,
                                          const TV* __restrict__ x, int cols, int rows, int nA, double dt, TV* __restrict__ out,
                                          const int* __restrict__ done, int nChunks, const uint8_t* __restrict__ mcCode, const double* __restrict__ mcDict,
                                          double* __restrict__ stPart, const int32_t* __restrict__ list) {
    if (done && *done) return;
    constexpr bool NT = (POL & 1) != 0, SNT = (POL & 2) != 0;
    __shared__ double dict[MC ? 256 : 1];
    RowDiag<MC>::fill(dict, mcDict);
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rCol = bufRsrc(ecol, colBytes), rCode = bufRsrc(ecode, codeBytes), rX = bufRsrc(x, (size_t)cols * sizeof(TV)),
                                 rMcc = bufRsrc(mcCode, MC ? (size_t)nA : (size_t)nA * 8), rOut = bufRsrc(out, (size_t)rows * sizeof(TV));
    double stAcc = 0.;
    ell2Loop<SNT, LIST, TV>(rCol, rCode, rX, winBase, echunk, scale, nChunks, list,
        [&](unsigned row) PS_INLINE_LAMBDA { return RowDiag<MC>::template load<NT ? PS_EPI_AUX : 0>(rMcc, row, row); },   // (rows past nA read 0 through the buffer's range; their scale is 1)
        [&](unsigned row, bool, const DiagRow& m, double s) PS_INLINE_LAMBDA { sRowFinish<0, NT, TV>(rOut, row, nA, dt, RowDiag<MC>::value(dict, m), s, stAcc); });
    if (stPart) {
        const double bs = blockReduceSum(stAcc);
        if (threadIdx.x == 0) stPart[blockIdx.x] = bs;
    }
}
#define PS_S_ELL2_PARAMS const uint16_t* __restrict__ ecol, const int8_t* __restrict__ ecode, unsigned colBytes, unsigned codeBytes, \
                         const int32_t* __restrict__ winBase, const int4* __restrict__ echunk, double scale, const TV* __restrict__ x, int cols, int rows, \
                         int nA, double dt, TV* __restrict__ out, const int* __restrict__ done, int nChunks, const uint8_t* __restrict__ mcCode, \
                         const double* __restrict__ mcDict, double* __restrict__ stPart, const int32_t* __restrict__ list
#define PS_S_ELL2_ARGS ecol, ecode, colBytes, codeBytes, winBase, echunk, scale, x, cols, rows, nA, dt, out, done, nChunks, mcCode, mcDict, stPart, list
template <int POL, bool LIST, class TV = double>
__global__ void __launch_bounds__(BS) k_spmv_S_ell2(PS_S_ELL2_PARAMS) { spmvSEll2<POL, LIST, TV, true>(PS_S_ELL2_ARGS); }
template <int POL, bool LIST, class TV = double>       // mcCode = the fp64 McInv array
__global__ void __launch_bounds__(BS) k_spmv_S_ell2u(PS_S_ELL2_PARAMS) { spmvSEll2<POL, LIST, TV, false>(PS_S_ELL2_ARGS); }
#undef PS_S_ELL2_ARGS
#undef PS_S_ELL2_PARAMS

// The same for the St kernel of the plain single-domain step (k_spmv_St_ell<3, POL, 3>: coded uInv, residual update in the epilogue): two
// units in flight per wave, two chunks per workgroup and step (r04; default, PS_ST_DUAL=0 switches back).  Compiled for six waves per SIMD
// (80 VGPRs): twelve units in flight per SIMD against the seven of the one-unit kernel.
// CZ: the Chebyshev polynomial's first term on the new r in the epilogue (z_1 = dinv r / theta -> fr.cz, r.z partials from it; fr.dinvF unused)
// DIST: a rank of a decomposition — alpha and ||x||^2 from the all-reduced sums (fr.red), partials at fr.rStride; with LIST the launch over
// the chunks of OWNED rows only that runs under the exchange (ps_dist.hpp; k_spmv_St_ell's FX bit 2)
// TZ: element type of fr.cz (CZ only; float: the single-precision Chebyshev polynomial — fr.cz then points at floats and r.z is formed
// with the value as stored)
// HALO (DIST only, r06): the launch may hold halo rows — rows outside [fr.ownLo, fr.ownHi) whose y is this rank's share of a neighbour's A p: it goes
// to fr.yOut and r is left alone there (k_spmv_St_ell's generic MODE 3 did this on one unit per wave; the rank's launch over the chunks next
// to a cut and the whole-rank launch of the sequential exchange now run two units per wave like the owned-rows launch)
// UC (r06): the stress diagonal uInv comes coded (true) or, when it takes more than 256 values — a viscosity FIELD —, as the fp64 array itself, passed
// in uCode's place (RowDiag; until r06 such scenes ran the one-unit kernels and the fp64 polynomial)
// TV: element type of the Krylov vectors the kernel gathers and streams — t, xin (p) and fr.r.  float: a pass of the mixed-precision solve
// (ps_solve.hip: PS_PRECISION_MIXED; the pointers then point at floats, r.r and r.z are formed from r AS STORED, and the stop test is the pass's)
// AP (TV = float only): the plain product of the five-kernel step instead of the residual update — no prologue, (A p)[row] -> fr.r as TV,
// the workgroup's partial of p . A p -> fr.rPart[block]; of fr only r and rPart are read
template <int POL, bool CZ, bool DIST, bool LIST, class TZ = double, bool HALO = false, bool UC = true, class TV = double, bool AP = false>
__global__ void __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(6, 6))) k_spmv_St_ell2(const uint16_t* __restrict__ ecol, const int8_t* __restrict__ ecode, unsigned colBytes, unsigned codeBytes,
                                                     const int32_t* __restrict__ winBase, const int4* __restrict__ echunk, double scale,
                                                     const TV* __restrict__ t, int cols, int rows, const TV* __restrict__ xin,
                                                     const int* __restrict__ done, int nChunks, const uint8_t* __restrict__ uCode, const double* __restrict__ uDict, FusedR fr,
                                                     const int32_t* __restrict__ list) {
    if (done && *done) return;
    constexpr bool NT = (POL & 1) != 0, SNT = (POL & 2) != 0, PASS = !std::is_same<TV, double>::value;
    static_assert(!HALO || DIST, "halo rows exist on a rank of a decomposition only");
    static_assert(!AP || (PASS && !CZ && !DIST && !HALO), "the plain product: single-domain passes of the mixed-precision solve only");
    __shared__ double dict[UC ? 256 : 1];
    RowDiag<UC>::fill(dict, uDict);
    double alpha;
    if constexpr (AP) alpha = 0.; else if (!fusedPrologue<PASS>(fr, DIST, alpha)) return;
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rCol = bufRsrc(ecol, colBytes), rCode = bufRsrc(ecode, codeBytes), rT = bufRsrc(t, (size_t)cols * sizeof(TV)),
                                 rE0 = bufRsrc(xin, (size_t)rows * sizeof(TV)), rUc = bufRsrc(uCode, UC ? (size_t)rows : (size_t)rows * 8);
    const FusedBufs B = fusedBufs<TZ, TV>(fr, rows, true, HALO, CZ);
    struct Loaded { double e; DiagRow u; FusedRow f; };
    double dacc = 0., dacc2 = 0.;
    ell2Loop<SNT, LIST, TV>(rCol, rCode, rT, winBase, echunk, scale, nChunks, list,
        [&](unsigned row) PS_INLINE_LAMBDA {
            return Loaded{VecIO<TV>::template loadEpi<NT>(rE0, row), RowDiag<UC>::template load<NT ? (UC ? PS_UC_AUX : PS_EPI_AUX) : 0>(rUc, row, row),
                          AP ? FusedRow{0., 0., 1.f} : fusedLoads<NT, TV>(fr, B, row, CZ)};
        },
        [&](unsigned row, bool live, const Loaded& L, double s) PS_INLINE_LAMBDA {
            const double y = stRowY(s, RowDiag<UC>::value(dict, L.u), L.e);
            if constexpr (AP) { dacc += L.e * y; VecIO<TV>::template store<NT>(B.r, row, y); }   // (idle lanes: e = 0, the store is dropped)
            else fusedRowFinish<NT, TZ, TV>(fr, B, row, live, HALO, HALO, CZ, alpha, y, L.f, dacc, dacc2);
        });
    if constexpr (AP) {
        const double bs = blockReduceSum(dacc);
        if (threadIdx.x == 0) fr.rPart[blockIdx.x] = bs;
    } else
    fusedPartials(fr, dacc, dacc2, CZ, (DIST && fr.rStride > 0) ? fr.rStride : (int)gridDim.x);
}

// ... and for MODE 2 (one term of the Chebyshev preconditioner in the epilogue): two units in flight per wave.
// TV: element type of t, xin (z_j), cheb.zprev (z_{j-1}) and out (z_{j+1}); r and every sum stay fp64
#ifdef PS_ST2C_WAVES      // A/B build knob (scripts/build_variant.sh): waves per SIMD the Chebyshev-term kernel is compiled for
#define PS_ST2C_ATTR __attribute__((amdgpu_waves_per_eu(PS_ST2C_WAVES, PS_ST2C_WAVES)))
#else
#define PS_ST2C_ATTR
#endif
template <int POL, class TV = double, bool UC = true>
__global__ void __launch_bounds__(BS) PS_ST2C_ATTR k_spmv_St_ell2c(const uint16_t* __restrict__ ecol, const int8_t* __restrict__ ecode, unsigned colBytes, unsigned codeBytes,
                                                      const int32_t* __restrict__ winBase, const int4* __restrict__ echunk, double scale,
                                                      const TV* __restrict__ t, int cols, int rows, const TV* __restrict__ xin, TV* __restrict__ out,
                                                      double* __restrict__ partial, const int* __restrict__ done, int nChunks, ChebArgs cheb,
                                                      const uint8_t* __restrict__ uCode, const double* __restrict__ uDict) {
    if (done && *done) return;
    constexpr bool NT = (POL & 1) != 0, SNT = (POL & 2) != 0;
    __shared__ double dict[UC ? 256 : 1];
    RowDiag<UC>::fill(dict, uDict);
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rCol = bufRsrc(ecol, colBytes), rCode = bufRsrc(ecode, codeBytes), rT = bufRsrc(t, (size_t)cols * sizeof(TV)),
                                 rE0 = bufRsrc(xin, (size_t)rows * sizeof(TV)), rUc = bufRsrc(uCode, UC ? (size_t)rows : (size_t)rows * 8), rOut = bufRsrc(out, (size_t)rows * sizeof(TV)),
                                 rCr = bufRsrc(cheb.r, (size_t)rows * 8), rCi = bufRsrc(cheb.dinv, (size_t)rows * sizeof(diag_t)),
                                 rCd = bufRsrc(cheb.zprev, cheb.zprev ? (size_t)rows * sizeof(TV) : 0);   // (cheb.zprev points at TV elements)
    struct Loaded { double e; DiagRow u; ChebRow c; };
    double dacc = 0.;
    ell2Loop<SNT, false, TV>(rCol, rCode, rT, winBase, echunk, scale, nChunks, nullptr,
        [&](unsigned row) PS_INLINE_LAMBDA {
            return Loaded{VecIO<TV>::template loadEpi<NT>(rE0, row), RowDiag<UC>::template load<NT ? (UC ? PS_UC_AUX : PS_EPI_AUX) : 0>(rUc, row, row), chebLoads<TV>(rCr, rCi, rCd, row)};
        },
        [&](unsigned row, bool, const Loaded& L, double s) PS_INLINE_LAMBDA {
            VecIO<TV>::template store<NT>(rOut, row, chebRowFinish<TV>(cheb, L.c, stRowY(s, RowDiag<UC>::value(dict, L.u), L.e), L.e, dacc));
        });
    const double bs = blockReduceSum(dacc);
    if (threadIdx.x == 0) partial[blockIdx.x] = bs;
}
#undef PS_INLINE_LAMBDA
