// PCG vector / scalar kernels, BiCGStab helpers, Jacobi diagonal, velocity recovery and write-back.
// Part of the single translation unit ps_solve.hip (included there, inside its anonymous namespace where noted).
#pragma once

// ---- CG vector kernels ---------------------------------------------------------------------------
// Cache policy of the streams these kernels touch once per iteration (compile-time, scripts/build_variant.sh builds A/B copies).
// Measured at 256^3: x, Ap and r non-temporal (read / written once per iteration, next use a whole iteration away) take
// k_cg_update_xp from 0.345 to 0.30 ms and the step from 1378 to 1319 ms; p stays default-policy (the next S gathers it).
#ifndef PS_VEC_NT_X
#define PS_VEC_NT_X 1      // x: read and written only by k_cg_update_xp
#endif
#ifndef PS_VEC_NT_AP
#define PS_VEC_NT_AP 1     // Ap: written by St, read once by k_cg_update_r
#endif
#ifndef PS_VEC_NT_R
#define PS_VEC_NT_R 1      // r in k_cg_update_r (read + written)
#endif
#ifndef PS_VEC_NT_RX
#define PS_VEC_NT_RX 1     // r as read by k_cg_update_xp
#endif
#ifndef PS_VEC_NT_P
#define PS_VEC_NT_P 0      // p as written by k_cg_update_xp (gathered by the next S)
#endif
#ifndef PS_VEC_NT_PL
#define PS_VEC_NT_PL 0     // p as read by k_cg_update_xp
#endif
#ifndef PS_VEC_NT_U
#define PS_VEC_NT_U 1      // the uInv codes as read by k_cg_update_xp_u
#endif
#ifndef PS_VEC_NT_D
#define PS_VEC_NT_D 1      // the stored Jacobi diagonal (read by both step kernels, half an iteration apart)
#endif
// two consecutive floats as doubles; i2 = index of the pair (the fp32 form of the stored diagonal; z of the single-precision polynomial, whose x
// and p are fp64: two values per 16 bytes of x, not Vec16<float>'s four)
__device__ inline double2 ldF2(const float* __restrict__ f, int64_t i2, bool nt) {
    typedef float psf2 __attribute__((ext_vector_type(2)));
    const psf2* q = reinterpret_cast<const psf2*>(f) + i2;
    const psf2 v = nt ? __builtin_nontemporal_load(q) : *q;
    return make_double2((double)v.x, (double)v.y);
}
// two consecutive entries of the stored Jacobi diagonal (ps_common.hpp: diag_t) as doubles; i2 = index of the pair
__device__ inline double2 ldDiag2(const diag_t* __restrict__ d, int64_t i2, bool nt) {
#ifdef PS_DIAG_FP32
    return ldF2(d, i2, nt);
#else
    const uint32_t* q = reinterpret_cast<const uint32_t*>(d) + i2;
    const uint32_t v = nt ? __builtin_nontemporal_load(q) : *q;
    return make_double2((double)__builtin_bit_cast(float, v << 16), (double)__builtin_bit_cast(float, v & 0xFFFF0000u));
#endif
}
constexpr uintptr_t DIAG_PAIR_MASK = 2 * sizeof(diag_t) - 1;
typedef double psd2 __attribute__((ext_vector_type(2)));
__device__ inline double2 ldD2(const double2* p, bool nt) {
    if (!nt) return *p;
    const psd2 v = __builtin_nontemporal_load(reinterpret_cast<const psd2*>(p));
    return make_double2(v.x, v.y);
}
__device__ inline void stD2(double2* p, double2 v, bool nt) {
    if (!nt) { *p = v; return; }
    psd2 q; q.x = v.x; q.y = v.y;
    __builtin_nontemporal_store(q, reinterpret_cast<psd2*>(p));
}
// 16 bytes of a Krylov vector per lane and access, as doubles: two doubles, or four floats (the mixed-precision solve, ps_solve.hip:
// PS_PRECISION_MIXED, keeps d, p, r and A p in fp32).  iv = index of the group; stored: the value a later kernel reads back.
template <class TV> struct Vec16;
template <> struct Vec16<double> {
    static constexpr int W = 2;
    __device__ static inline void load(const double* v, int64_t iv, bool nt, double (&o)[2]) { const double2 q = ldD2((const double2*)v + iv, nt); o[0] = q.x; o[1] = q.y; }
    __device__ static inline void store(double* v, int64_t iv, bool nt, const double (&o)[2]) { stD2((double2*)v + iv, make_double2(o[0], o[1]), nt); }
    __device__ static inline double stored(double v) { return v; }
};
template <> struct Vec16<float> {
    static constexpr int W = 4;
    typedef float psf4 __attribute__((ext_vector_type(4)));
    __device__ static inline void load(const float* v, int64_t iv, bool nt, double (&o)[4]) {
        const psf4* q = reinterpret_cast<const psf4*>(v) + iv;
        const psf4 f = nt ? __builtin_nontemporal_load(q) : *q;
        o[0] = (double)f.x; o[1] = (double)f.y; o[2] = (double)f.z; o[3] = (double)f.w;
    }
    __device__ static inline void store(float* v, int64_t iv, bool nt, const double (&o)[4]) {
        psf4 f; f.x = (float)o[0]; f.y = (float)o[1]; f.z = (float)o[2]; f.w = (float)o[3];
        psf4* q = reinterpret_cast<psf4*>(v) + iv;
        if (nt) __builtin_nontemporal_store(f, q); else *q = f;
    }
    __device__ static inline double stored(double v) { return (double)(float)v; }
};
// the W entries of the stored Jacobi diagonal / of an fp64 diagonal (the exported system's Jacobi diagonal, the stress diagonal) / the W one-byte
// codes that go with group iv
template <int W> __device__ inline void ldDiagW(const diag_t* __restrict__ d, int64_t iv, bool nt, double (&o)[W]) {
#pragma unroll
    for (int k = 0; k < W / 2; ++k) { const double2 q = ldDiag2(d, iv * (W / 2) + k, nt); o[2 * k] = q.x; o[2 * k + 1] = q.y; }
}
template <int W> __device__ inline void ldDiagW(const double* __restrict__ u, int64_t iv, bool nt, double (&o)[W]) {
#pragma unroll
    for (int k = 0; k < W / 2; ++k) { const double2 q = ldD2((const double2*)u + iv * (W / 2) + k, nt); o[2 * k] = q.x; o[2 * k + 1] = q.y; }
}
template <int W> __device__ inline uint32_t ldCodesW(const uint8_t* __restrict__ c, int64_t iv, bool nt) {
    if constexpr (W == 2) return nt ? __builtin_nontemporal_load((const uint16_t*)c + iv) : ((const uint16_t*)c)[iv];
    else return nt ? __builtin_nontemporal_load((const uint32_t*)c + iv) : ((const uint32_t*)c)[iv];
}
// The stress diagonal uInv as the x, p update and k_uinv_pp read it: one-byte codes into a 256-entry table (ps_context.hpp: uCode / uDict; code
// null: none) or the fp64 array.  By value at the launch sites.  fill: the table into the block's LDS, to be read after the caller's next barrier;
// value: entry i; load: the W entries of group iv (nt: PS_VEC_NT_U on the codes)
struct StressDiag {
    const uint8_t* code; const double* dict; const double* inv;
    __device__ inline const double* fill() const {
        __shared__ double lds[256];
        if (code) lds[threadIdx.x] = dict[threadIdx.x];
        return lds;
    }
    template <int W> __device__ inline bool aligned() const { return (((uintptr_t)code & (W - 1)) == 0) && (((uintptr_t)inv & 15) == 0); }
    __device__ inline double value(const double* lds, int64_t i) const { return code ? lds[code[i]] : inv[i]; }
    template <int W> __device__ inline void load(const double* lds, int64_t iv, bool nt, double (&u)[W]) const {
        if (code) {
            const uint32_t cc = ldCodesW<W>(code, iv, nt && PS_VEC_NT_U);
#pragma unroll
            for (int k = 0; k < W; ++k) u[k] = lds[(cc >> (8 * k)) & 255u];
        } else ldDiagW<W>(inv, iv, nt, u);
    }
};
// out = a .* b   (TA: double, or the stored Jacobi diagonal as the PCG kernels read it)
template <class TA> __global__ void k_mul(double* __restrict__ out, const TA* __restrict__ a, const double* __restrict__ b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = diagValue(a[i]) * b[i];
}
// Start of a solve or of a pass: r = b, or (warm) b - A x with Ax = A x from applyOperator (a warm start, whose x0 stays in x); z = pre(r);
// p = z; (clear) xd = 0 — x, or a pass's correction d; partial rsold = r.z.  warm and clear are constants at every wrapper but the pass's warm.
// DT: the diagonal's element type (diag_t, or double: the exported system).  TV = float: a pass of the mixed-precision solve
// (ps_set_solve_precision; ps_solve.hip: solve), which solves A d = r64 with r = fp32(r64), p = fp32(z).  Partials: r.z of the values as stored
// at [block]; then of the TRUE r64 . r64 at [grid + block] and of x . x (x64; warm only) at [2 grid + block] — the fp64 evaluation of the stop
// rule on b - A x (k_cg_scal0_pass)
template <class TV, class DT>
__device__ inline void cgInit(const double* __restrict__ b, const double* __restrict__ Ax, bool warm, const double* __restrict__ x64,
                              const DT* __restrict__ dinv, TV* __restrict__ xd, bool clear, TV* __restrict__ r, TV* __restrict__ p, int64_t n,
                              double* __restrict__ partial) {
    constexpr bool PASS = !std::is_same<TV, double>::value;
    double arz = 0., arr = 0., axx = 0.;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        const double r64 = warm ? b[i] - Ax[i] : b[i];
        const TV rs = (TV)r64;                                                              // as stored (Vec16<TV>::stored)
        const TV zs = (TV)(dinv ? diagValue(dinv[i]) * (double)rs : (double)rs);
        if (clear) xd[i] = (TV)0;
        r[i] = rs; p[i] = zs;
        arz += (double)rs * (double)zs;
        if (PASS) {
            arr += r64 * r64;
            if (warm) { const double xv = x64[i]; axx += xv * xv; }
        }
    }
    const double s0 = blockReduceSum(arz), s1 = PASS ? blockReduceSum(arr) : 0., s2 = PASS ? blockReduceSum(axx) : 0.;
    if (threadIdx.x != 0) return;
    partial[blockIdx.x] = s0;
    if (PASS) { partial[gridDim.x + blockIdx.x] = s1; partial[2 * gridDim.x + blockIdx.x] = s2; }
}
#define PS_CG_INIT_PARAMS(DT) const double* __restrict__ b, const DT* __restrict__ dinv, double* __restrict__ x, double* __restrict__ r, double* __restrict__ p, \
                              int64_t n, double* __restrict__ partial
__global__ void __launch_bounds__(BS) k_cg_init_f(PS_CG_INIT_PARAMS(diag_t)) { cgInit(b, nullptr, false, nullptr, dinv, x, true, r, p, n, partial); }
__global__ void __launch_bounds__(BS) k_cg_init_d64(PS_CG_INIT_PARAMS(double)) { cgInit(b, nullptr, false, nullptr, dinv, x, true, r, p, n, partial); }
#undef PS_CG_INIT_PARAMS
__global__ void __launch_bounds__(BS) k_cg_init_warm(const double* __restrict__ b, const double* __restrict__ Ax, const diag_t* __restrict__ dinv,
                                                     double* __restrict__ r, double* __restrict__ p, int64_t n, double* __restrict__ partial) {
    cgInit(b, Ax, true, nullptr, dinv, (double*)nullptr, false, r, p, n, partial);
}
__global__ void __launch_bounds__(BS) k_cg_init_pass(const double* __restrict__ b, const double* __restrict__ Ax, const double* __restrict__ x,
                                                     const diag_t* __restrict__ dinv, float* __restrict__ d, float* __restrict__ r,
                                                     float* __restrict__ p, int64_t n, double* __restrict__ partial) {
    cgInit(b, Ax, Ax != nullptr, x, dinv, d, true, r, p, n, partial);
}
// End of a pass: x += d in fp64 (cold: x = d, the first pass of a cold solve)
__global__ void __launch_bounds__(BS) k_cg_end_pass(const float* __restrict__ d, double* __restrict__ x, int64_t n, int cold) {
    const bool vec = ((((uintptr_t)d | (uintptr_t)x) & 15) == 0);
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * BS) {
        double dv[4], lo[2] = {0., 0.}, hi[2] = {0., 0.};
        Vec16<float>::load(d, i, false, dv);
        if (!cold) { Vec16<double>::load(x, 2 * i, false, lo); Vec16<double>::load(x, 2 * i + 1, false, hi); }
        lo[0] += dv[0]; lo[1] += dv[1]; hi[0] += dv[2]; hi[1] += dv[3];
        Vec16<double>::store(x, 2 * i, false, lo); Vec16<double>::store(x, 2 * i + 1, false, hi);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) x[i] = (cold ? 0. : x[i]) + (double)d[i];
}
// The solution as seven dense x-fastest grids (ps_context::warmStore): blockIdx.y = grid, its samples grid-stride; map = the grid's index
// map (sample -> internal DOF, -1: none).  Every index is checked against -1 and the system size.
struct SolutionGrids { const int32_t* map[7]; int64_t off[7]; int64_t cnt[7]; };
// store[sample] = fp32(x[map[sample]]), 0 where the sample has no DOF
__global__ void __launch_bounds__(BS) k_solution_scatter(SolutionGrids G, const double* __restrict__ x, int64_t n, float* __restrict__ store) {
    const int32_t* __restrict__ map = G.map[blockIdx.y];
    float* __restrict__ out = store + G.off[blockIdx.y];
    const int64_t cnt = G.cnt[blockIdx.y];
    for (int64_t c = (int64_t)blockIdx.x * BS + threadIdx.x; c < cnt; c += (int64_t)gridDim.x * BS) {
        const int32_t i = map[c];
        out[c] = (i >= 0 && i < n) ? (float)x[i] : 0.f;
    }
}
// x[map[sample]] = x0[map[sample]] = store[sample] widened to fp64: every DOF has exactly one sample, so x is written whole
__global__ void __launch_bounds__(BS) k_warm_gather(SolutionGrids G, const float* __restrict__ store, int64_t n, double* __restrict__ x,
                                                    double* __restrict__ x0) {
    const int32_t* __restrict__ map = G.map[blockIdx.y];
    const float* __restrict__ in = store + G.off[blockIdx.y];
    const int64_t cnt = G.cnt[blockIdx.y];
    for (int64_t c = (int64_t)blockIdx.x * BS + threadIdx.x; c < cnt; c += (int64_t)gridDim.x * BS) {
        const int32_t i = map[c];
        if (i < 0 || i >= n) continue;
        const double v = (double)in[c];
        x[i] = v; x0[i] = v;
    }
}
__global__ void k_to_diag(const double* __restrict__ a, diag_t* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = diagStore(a[i]);
}
// sum of `count` partials, valid in thread 0 (sumLocal, stopTest: ps_kernels_spmv.hpp, shared with the fused St epilogue)
__device__ inline double sumPartials(const double* __restrict__ partial, int count) { return blockReduceSum(sumLocal(partial, count)); }
// out[q] = sum of partial[q*stride .. q*stride+count)   (q < nq), one block, fixed order; sc given: nothing once the solve is done
__global__ void __launch_bounds__(BS) k_sumq(const CGScalars* __restrict__ sc, const double* __restrict__ partial, int count, int stride, int nq,
                                             double* __restrict__ out) {
    if (sc && sc->done) return;
    for (int q = 0; q < nq; ++q) {
        const double s = sumPartials(partial + (int64_t)q * stride, count);
        if (threadIdx.x == 0) out[q] = s;
        __syncthreads();
    }
}
__device__ inline void cgScalInit(CGScalars* sc, double s, double tol, int maxit, int vecNT) {   // (one thread)
    sc->rsold = s; sc->rsold2[0] = s; sc->rsold2[1] = 0.; sc->rre = 0.; sc->iter = maxit; sc->maxit = maxit; sc->tol2 = tol * tol;
    sc->done = (s == 0.) ? 1 : 0;      // deviation: b == 0 -> return at once (reference divides 0/0, pcg.h:314)
    if (s == 0.) sc->iter = 0;
    sc->alpha = sc->beta = sc->pAp = sc->rr = sc->xx = sc->rz = 0.;
    sc->pend = 0; sc->pendIter = 0; sc->vecNT = vecNT;
}
__global__ void __launch_bounds__(BS) k_cg_scal0(CGScalars* sc, const double* __restrict__ partial, int count, double tol, int maxit, int vecNT) {
    const double s = sumPartials(partial, count);
    if (threadIdx.x == 0) cgScalInit(sc, s, tol, maxit, vecNT);
}
// The same at the start of a pass of the mixed-precision solve (k_cg_init_pass wrote the partials: r.z, then the true r.r, then x.x).  The true
// values stay in rr / xx / rre for the host — the evaluation that decides the solve —; the pass ends at r.r < floor2 * (true r.r), and with
// frozenXX its stop test uses this x.x throughout (stopTest<true>)
__global__ void __launch_bounds__(BS) k_cg_scal0_pass(CGScalars* sc, const double* __restrict__ partial, int count, double tol, int maxit, int vecNT, double floor2, int frozenXX) {
    const double s = sumPartials(partial, count), rr = sumPartials(partial + count, count), xx = sumPartials(partial + 2 * count, count);
    if (threadIdx.x == 0) {
        cgScalInit(sc, s, tol, maxit, vecNT);
        double rre = rr;                              // pcg.h:319-325 on r = b - A x
        if (rr / xx < rre) rre = rr / xx;
        sc->rr = rr; sc->xx = xx; sc->rre = rre;
        sc->rrFloor = floor2 * rr; sc->xxFix = frozenXX ? xx : 0.;
    }
}
// stage A of the p.Ap reduction: RED_BLOCKS blocks each sum a contiguous slice of the SpMV block partials
constexpr int RED_BLOCKS = 256;
__global__ void __launch_bounds__(BS) k_reduce_partials(const CGScalars* __restrict__ sc, const double* __restrict__ partial, int count,
                                                        double* __restrict__ out) {
    if (sc->done) return;
    const int per = (count + RED_BLOCKS - 1) / RED_BLOCKS;
    const int lo = blockIdx.x * per, hi = min(lo + per, count);
    double acc = 0.;
    for (int i = lo + threadIdx.x; i < hi; i += BS) acc += partial[i];
    const double s = blockReduceSum(acc);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- PCG step: x update deferred into the p update, scalar reductions folded into the vector kernels ---------------
// pcg.h:311-335 updates x and r together, tests min(rr, rr/xx) < tol^2, then forms beta and the new p: 11 vector passes
// and (here) two one-block scalar kernels.  This step is 10 passes and 2 launches:
//   k_cg_update_r :  [stop test of the previous iteration]  alpha = rsold / p.Ap ;  r -= alpha Ap ;  partials r.r, r.z
//   k_cg_update_xp:  beta = r.z / rsold ;  x += alpha p ;  p = z + beta p (p read once for both) ;  partials x.x
// Every block sums the (<= 4096 + 1024) partials of the preceding kernel itself — same order in every block, so all
// blocks hold bit-identical scalars — and block 0 records them for the host and the next kernel; rsold is double-buffered
// by iteration parity so no block reads a scalar another block of the same launch writes.
// The stop test of iteration k — same rr, xx of the updated x, same iteration index as the reference — is evaluated at
// the start of iteration k+1 (or by k_cg_check before the host polls); when it fires every later kernel is a no-op and
// x already holds the iterate the reference returns.  Cost: one unused p update and one unused operator apply.
// With `red` (distributed solve) the sums come all-reduced from the ranks: red = {p.Ap, x.x} resp. {r.r, r.z}.
// One sum of a step kernel's prologue: `count` >= 0 partials that every block sums itself (none: 0), or (count = SUM_REDUCED) the value at p[0],
// all-reduced by the ranks.
// Two of them, by value at the launch sites: {p.Ap, x.x} of k_cg_update_r, {r.r, r.z} of the x, p update, where an absent second (p null) means
// r.z = r.r (identity)
constexpr int SUM_REDUCED = -1;
struct SumSrc { const double* p; int count; };
struct TwoSums {
    SumSrc a, b;
    static TwoSums partials(const double* a, int na, const double* b, int nb) { return {{a, na}, {b, nb}}; }
    static TwoSums reduced(const double* red, bool second = true) { return {{red, SUM_REDUCED}, {second ? red + 1 : nullptr, SUM_REDUCED}}; }
};
__device__ inline double sumOf(const SumSrc& s) { return s.count != SUM_REDUCED ? blockSumAll(sumLocal(s.p, s.count)) : s.p[0]; }
template <bool PASS>
__device__ inline void cgCheck(CGScalars* sc, const double* __restrict__ red, const double* __restrict__ xxPartial, int vb, int lastIter) {
    if (sc->done) return;
    const double xx = red ? red[0] : blockSumAll(sumLocal(xxPartial, vb));
    stopTest<PASS>(sc, xx, lastIter, threadIdx.x == 0);
}
__global__ void __launch_bounds__(BS) k_cg_check(CGScalars* sc, const double* __restrict__ red, const double* __restrict__ xxPartial, int vb, int lastIter) {
    cgCheck<false>(sc, red, xxPartial, vb, lastIter);
}
__global__ void __launch_bounds__(BS) k_cg_check_pass(CGScalars* sc, const double* __restrict__ xxPartial, int vb, int lastIter) {   // a pass of the mixed-precision solve
    cgCheck<true>(sc, nullptr, xxPartial, vb, lastIter);
}
// [stop test of iteration it-1] ; alpha ; r -= alpha Ap ; partials of r.r and r.z.  s = {p.Ap, x.x}
// TV: element type of Ap and r (float: a pass of the mixed-precision solve — k_cg_update_r_f32; r.r and r.z from r as stored, the pass's stop test)
// DT: element type of the Jacobi diagonal (diag_t; double: the exported system — k_cg_update_r_d64)
template <class TV, class DT>
__device__ inline void cgUpdateR(CGScalars* sc, const TwoSums& s, int it, const TV* __restrict__ Ap, const DT* __restrict__ dinv, TV* __restrict__ r,
                                 int64_t n, double* __restrict__ partial) {
    if (sc->done) return;
    constexpr bool PASS = !std::is_same<TV, double>::value;
    constexpr int W = Vec16<TV>::W;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    const double xx = it > 0 ? sumOf(s.b) : 0., pAp = sumOf(s.a);
    if (it > 0 && stopTest<PASS>(sc, xx, it - 1, writer)) return;     // same verdict in every block
    const double alpha = sc->rsold2[it & 1] / pAp;                      // pcg.h:314
    if (writer) { sc->pAp = pAp; sc->alpha = alpha; }
    double arr = 0., arz = 0.;
    const bool nt = sc->vecNT != 0;
    const bool vec = ((((uintptr_t)Ap | (uintptr_t)r) & 15) == 0) && (((uintptr_t)dinv & (W * sizeof(DT) - 1)) == 0);
    const int64_t nv = vec ? n / W : 0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * BS) {
        double av[W], rv[W];
        Vec16<TV>::load(Ap, i, nt && PS_VEC_NT_AP, av);
        Vec16<TV>::load(r, i, nt && PS_VEC_NT_R, rv);
#pragma unroll
        for (int k = 0; k < W; ++k) rv[k] = Vec16<TV>::stored(rv[k] - alpha * av[k]);
        Vec16<TV>::store(r, i, nt && PS_VEC_NT_R, rv);
#pragma unroll
        for (int k = 0; k < W; ++k) arr += rv[k] * rv[k];
        if (dinv) {
            double dv[W];
            ldDiagW<W>(dinv, i, nt && PS_VEC_NT_D, dv);
#pragma unroll
            for (int k = 0; k < W; ++k) arz += rv[k] * (dv[k] * rv[k]);
        }
    }
    for (int64_t i = W * nv + (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        const double rv = Vec16<TV>::stored((double)r[i] - alpha * (double)Ap[i]);
        r[i] = (TV)rv;
        arr += rv * rv;
        if (dinv) arz += rv * (diagValue(dinv[i]) * rv);
    }
    const double s0 = blockReduceSum(arr), s2 = dinv ? blockReduceSum(arz) : 0.;
    if (threadIdx.x == 0) { partial[blockIdx.x] = s0; partial[gridDim.x + blockIdx.x] = s2; }
}
#define PS_CG_UPDATE_R_PARAMS(TV, DT) CGScalars* sc, TwoSums s, int it, const TV* __restrict__ Ap, const DT* __restrict__ dinv, TV* __restrict__ r, int64_t n, double* __restrict__ partial
__global__ void __launch_bounds__(BS) k_cg_update_r(PS_CG_UPDATE_R_PARAMS(double, diag_t)) { cgUpdateR(sc, s, it, Ap, dinv, r, n, partial); }
__global__ void __launch_bounds__(BS) k_cg_update_r_f32(PS_CG_UPDATE_R_PARAMS(float, diag_t)) { cgUpdateR(sc, s, it, Ap, dinv, r, n, partial); }
__global__ void __launch_bounds__(BS) k_cg_update_r_d64(PS_CG_UPDATE_R_PARAMS(double, double)) { cgUpdateR(sc, s, it, Ap, dinv, r, n, partial); }
#undef PS_CG_UPDATE_R_PARAMS
// Where z = M^-1 r of the x, p update comes from.  V: element type of x and p; W values per 16-byte group of x; aligned: the 16-byte loop may run;
// load: the W values of group iv; at: entry i (the scalar tail).
// ZJacobi: z = D^-1 r with the stored diagonal (null: z = r).  TV: element type of r, x and p; DT as in cgUpdateR
template <class TV, class DT> struct ZJacobi {
    typedef TV V;
    static constexpr int W = Vec16<TV>::W;
    const TV* r; const DT* dinv;
    __device__ inline bool aligned() const { return (((uintptr_t)r & 15) == 0) && (((uintptr_t)dinv & (W * sizeof(DT) - 1)) == 0); }
    __device__ inline void load(int64_t iv, bool nt, double (&z)[W]) const {
        Vec16<TV>::load(r, iv, nt && PS_VEC_NT_RX, z);
        if (dinv) {
            double dv[W];
            ldDiagW<W>(dinv, iv, nt && PS_VEC_NT_D, dv);
#pragma unroll
            for (int k = 0; k < W; ++k) z[k] = dv[k] * z[k];
        }
    }
    __device__ inline double at(int64_t i) const { return dinv ? diagValue(dinv[i]) * (double)r[i] : (double)r[i]; }
};
// ZVector: z is a VECTOR (the polynomial preconditioner), x and p are fp64.  TZ: element type of z (float: the single-precision Chebyshev
// polynomial — still two values per group, of 8 bytes)
template <class TZ> struct ZVector {
    typedef double V;
    static constexpr int W = 2;
    const TZ* z;
    __device__ inline bool aligned() const { return ((uintptr_t)z & 15) == 0; }
    __device__ inline void load(int64_t iv, bool nt, double (&o)[2]) const {
        double2 q;
        if constexpr (std::is_same<TZ, float>::value) q = ldF2(z, iv, nt); else q = ldD2((const double2*)z + iv, nt);
        o[0] = q.x; o[1] = q.y;
    }
    __device__ inline double at(int64_t i) const { return (double)z[i]; }
};
// beta = r.z / rsold ; x += alpha p ; p = z + beta p (z from ZS) ; partials of x.x.  s = {r.r, r.z}
// UPP (fused residual update, FusedR in ps_kernels_spmv.hpp): also the partials of sum_j uInv_j p_j^2 of the NEW p — the diagonal
// share of the next p . A p — from the coded diagonal (1 B per entry + 256-entry table in LDS) or the fp64 one (StressDiag).
// ZS::V = float: a pass of the mixed-precision solve, where x is the pass's correction d — k_cg_update_xp_f32 / _u_f32; x.x and the uInv p^2
// partials are formed from the values as stored
template <bool UPP, class ZS>
__device__ inline void cgUpdateXp(CGScalars* sc, const TwoSums& s, int it, const ZS& zs, typename ZS::V* __restrict__ x, typename ZS::V* __restrict__ p,
                                  int64_t n, double* __restrict__ partial, const StressDiag& u, double* __restrict__ uPart) {
    if (sc->done) return;
    typedef typename ZS::V TV;
    constexpr int W = ZS::W;
    const double* dict = nullptr;
    if constexpr (UPP) dict = u.fill();
    const double rr = sumOf(s.a), rz = s.b.p ? sumOf(s.b) : rr;
    if (UPP && s.a.count == SUM_REDUCED) __syncthreads();                              // the table: visible after the barriers of blockSumAll otherwise
    const double alpha = sc->alpha, beta = rz / sc->rsold2[it & 1];      // pcg.h:331-335
    const bool nt = sc->vecNT != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { sc->rr = rr; sc->rz = rz; sc->beta = beta; sc->rsold2[(it + 1) & 1] = rz; sc->rsold = rz; }
    double axx = 0., aup = 0.;
    const bool vec = ((((uintptr_t)p | (uintptr_t)x) & 15) == 0) && zs.aligned() && (!UPP || u.template aligned<W>());
    const int64_t nv = vec ? n / W : 0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * BS) {
        double z[W], pv[W], xv[W];
        zs.load(i, nt, z);
        Vec16<TV>::load(p, i, nt && PS_VEC_NT_PL, pv);
        Vec16<TV>::load(x, i, nt && PS_VEC_NT_X, xv);
#pragma unroll
        for (int k = 0; k < W; ++k) xv[k] = Vec16<TV>::stored(xv[k] + alpha * pv[k]);
#pragma unroll
        for (int k = 0; k < W; ++k) pv[k] = Vec16<TV>::stored(z[k] + beta * pv[k]);
        Vec16<TV>::store(x, i, nt && PS_VEC_NT_X, xv);
        Vec16<TV>::store(p, i, nt && PS_VEC_NT_P, pv);
#pragma unroll
        for (int k = 0; k < W; ++k) axx += xv[k] * xv[k];
        if (UPP) {
            double uv[W];
            u.template load<W>(dict, i, nt, uv);
#pragma unroll
            for (int k = 0; k < W; ++k) aup += uv[k] * (pv[k] * pv[k]);
        }
    }
    for (int64_t i = W * nv + (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        const double z = zs.at(i);
        const double pv = p[i];
        const double xv = Vec16<TV>::stored((double)x[i] + alpha * pv);
        const double pn = Vec16<TV>::stored(z + beta * pv);
        x[i] = (TV)xv; p[i] = (TV)pn;
        axx += xv * xv;
        if (UPP) aup += u.value(dict, i) * (pn * pn);
    }
    const double s1 = blockReduceSum(axx);
    if (threadIdx.x == 0) partial[blockIdx.x] = s1;
    if (UPP) {
        const double s2 = blockReduceSum(aup);
        if (threadIdx.x == 0) uPart[blockIdx.x] = s2;
    }
}
#define PS_CG_XP_PARAMS(TV, DT) CGScalars* sc, TwoSums s, int it, const TV* __restrict__ r, const DT* __restrict__ dinv, TV* __restrict__ x, TV* __restrict__ p, \
                                int64_t n, double* __restrict__ partial
#define PS_CG_XP_Z_PARAMS CGScalars* sc, TwoSums s, int it, const TZ* __restrict__ z, double* __restrict__ x, double* __restrict__ p, int64_t n, double* __restrict__ partial
__global__ void __launch_bounds__(BS) k_cg_update_xp(PS_CG_XP_PARAMS(double, diag_t)) { cgUpdateXp<false>(sc, s, it, ZJacobi<double, diag_t>{r, dinv}, x, p, n, partial, StressDiag{}, nullptr); }
__global__ void __launch_bounds__(BS) k_cg_update_xp_u(PS_CG_XP_PARAMS(double, diag_t), StressDiag u, double* __restrict__ uPart) {
    cgUpdateXp<true>(sc, s, it, ZJacobi<double, diag_t>{r, dinv}, x, p, n, partial, u, uPart);
}
__global__ void __launch_bounds__(BS) k_cg_update_xp_f32(PS_CG_XP_PARAMS(float, diag_t)) { cgUpdateXp<false>(sc, s, it, ZJacobi<float, diag_t>{r, dinv}, x, p, n, partial, StressDiag{}, nullptr); }
__global__ void __launch_bounds__(BS) k_cg_update_xp_u_f32(PS_CG_XP_PARAMS(float, diag_t), StressDiag u, double* __restrict__ uPart) {
    cgUpdateXp<true>(sc, s, it, ZJacobi<float, diag_t>{r, dinv}, x, p, n, partial, u, uPart);
}
__global__ void __launch_bounds__(BS) k_cg_update_xp_d64(PS_CG_XP_PARAMS(double, double)) { cgUpdateXp<false>(sc, s, it, ZJacobi<double, double>{r, dinv}, x, p, n, partial, StressDiag{}, nullptr); }
template <class TZ> __global__ void __launch_bounds__(BS) k_cg_update_xp_z(PS_CG_XP_Z_PARAMS) { cgUpdateXp<false>(sc, s, it, ZVector<TZ>{z}, x, p, n, partial, StressDiag{}, nullptr); }
template <class TZ> __global__ void __launch_bounds__(BS) k_cg_update_xp_z_u(PS_CG_XP_Z_PARAMS, StressDiag u, double* __restrict__ uPart) {
    cgUpdateXp<true>(sc, s, it, ZVector<TZ>{z}, x, p, n, partial, u, uPart);
}
#undef PS_CG_XP_Z_PARAMS
#undef PS_CG_XP_PARAMS
// partials of sum_j uInv_j p_j^2 (the first search direction of a fused-step solve; TV = float: of a pass of the mixed-precision solve)
template <class TV>
__device__ inline void uinvPp(const TV* __restrict__ p, const StressDiag& u, int64_t n, double* __restrict__ uPart) {
    const double* dict = u.fill();
    __syncthreads();
    double acc = 0.;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        const double pv = p[i];
        acc += u.value(dict, i) * (pv * pv);
    }
    const double s = blockReduceSum(acc);
    if (threadIdx.x == 0) uPart[blockIdx.x] = s;
}
__global__ void __launch_bounds__(BS) k_uinv_pp(const double* __restrict__ p, StressDiag u, int64_t n, double* __restrict__ uPart) { uinvPp(p, u, n, uPart); }
__global__ void __launch_bounds__(BS) k_uinv_pp_f32(const float* __restrict__ p, StressDiag u, int64_t n, double* __restrict__ uPart) { uinvPp(p, u, n, uPart); }

// ---- four-kernel step across slabs (ps_dist.hpp) ---------------------------------------------------------------------------
// t = the sums of four values over a 1024-thread block, valid in thread 0 (fixed order).  The two one-block kernels below sit on the critical
// path of every rank-iteration: 1024 threads, every load of a thread issued before the sums, ONE round of wave reductions for the four values
// (k_fused_local_sum: 21 us -> a few with 256 threads walking the four arrays one after the other; k_sum_rr, r06: 12 us -> a few with 256
// threads and four block reductions in a row)
__device__ inline void blockSum4(const double (&acc)[4], double (&t)[4]) {
    __shared__ double red[4][16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) { const double v = waveReduceSum(acc[q]); if (lane == 0) red[q][w] = v; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 0; q < 4; ++q) { double a = 0.; for (int i = 0; i < 16; ++i) a += red[q][i]; t[q] = a; }
}
// this rank's share of p.Ap in its factored form and of ||x||^2: out = {sum S + sum T + 1/2 sum U, sum xx}   (one block, fixed order)
__global__ void __launch_bounds__(1024) k_fused_local_sum(const CGScalars* __restrict__ sc, const double* __restrict__ sPart, int sCount, const double* __restrict__ tPart, int tCount,
                                                         const double* __restrict__ uPart, int uCount, const double* __restrict__ xxPart, int xxCount, double* __restrict__ out) {
    if (sc && sc->done) return;
    double acc[4] = {0., 0., 0., 0.}, t[4];
    const double* arr[4] = {sPart, tPart, uPart, xxPart};
    const int cnt[4] = {sCount, tCount, uCount, xxCount};
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int i = threadIdx.x; i < cnt[q]; i += 1024) acc[q] += arr[q][i];
    blockSum4(acc, t);
    if (threadIdx.x == 0) { out[0] = t[0] + t[1] + 0.5 * t[2]; out[1] = t[3]; }
}
// The St kernel updated r on the owned DOFs with this rank's rows only.  The DOFs next to a cut also receive the neighbours' shares
// c of (A p)_j (their halo rows): r_j -= alpha c, and the partial sums of r.r / r.z are corrected by the change of r_j^2.
// fixupRow: r_j = rn (it was ro), the corrections into a0, a1; fixupPartials: the block's corrections of r.r at [block], of r.z at [grid + block]
__device__ inline void fixupRow(double* __restrict__ r, const diag_t* __restrict__ dinv, int j, double ro, double rn, double& a0, double& a1) {
    r[j] = rn;
    const double d = rn * rn - ro * ro;
    a0 += d;
    if (dinv) a1 += diagValue(dinv[j]) * d;
}
__device__ inline void fixupPartials(double a0, double a1, double* __restrict__ partial) {
    const double s0 = blockReduceSum(a0), s1 = blockReduceSum(a1);
    if (threadIdx.x == 0) { partial[blockIdx.x] = s0; partial[gridDim.x + blockIdx.x] = s1; }
}
// one link: the contributions of its two receive buffers
__global__ void __launch_bounds__(BS) k_dist_fixup(const CGScalars* __restrict__ sc, const int32_t* __restrict__ listA, int64_t nA, const double* __restrict__ bufA,
                                                   const int32_t* __restrict__ listB, int64_t nB, const double* __restrict__ bufB, double* __restrict__ r,
                                                   const diag_t* __restrict__ dinv, double* __restrict__ partial, int ownHi) {
    if (sc->done) return;
    const double alpha = sc->alpha;
    double a0 = 0., a1 = 0.;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < nA + nB; i += (int64_t)gridDim.x * BS) {
        const int j = i < nA ? listA[i] : listB[i - nA];
        if (j >= ownHi) continue;                        // a copy on its way to another rank (Dist::contributionsBack), not a DOF of this one
        const double c = i < nA ? bufA[i] : bufB[i - nA];
        const double ro = r[j];
        fixupRow(r, dinv, j, ro, ro - alpha * c, a0, a1);
    }
    fixupPartials(a0, a1, partial);
}
// out = {r.r, r.z} of this rank: the St kernel's partials plus the corrections of the fix-up ([2][fixCount] per set; r05: ONE set — the merged
// fix-up k_dist_fixup_merged — and the two corrections folded thread by thread before ONE reduction each: this one-block kernel took 17 us with
// 2 + 2 x 6 block reductions)   (one block)
__global__ void __launch_bounds__(1024) k_sum_rr(const CGScalars* __restrict__ sc, const double* __restrict__ rPart, int rCount, const double* __restrict__ fixPart, int fixCount,
                                               int fixSets, double* __restrict__ out) {
    if (sc->done) return;
    double acc[4] = {0., 0., 0., 0.}, t[4];
    for (int i = threadIdx.x; i < rCount; i += 1024) { acc[0] += rPart[i]; acc[1] += rPart[rCount + i]; }
    for (int q = 0; q < fixSets; ++q)
        for (int i = threadIdx.x; i < fixCount; i += 1024) { acc[2] += fixPart[(size_t)q * 2 * fixCount + i]; acc[3] += fixPart[(size_t)q * 2 * fixCount + fixCount + i]; }
    blockSum4(acc, t);
    if (threadIdx.x == 0) { out[0] = t[0] + t[2]; out[1] = t[1] + t[3]; }
}
// The fix-up of the fused step in ONE launch (r05): a thread owns a DOF that receives contributions — from up to MAXSRC links (a DOF next to two or
// three cuts) — and applies them in link order, each to the r the previous one left: the arithmetic of the per-link launches of k_dist_fixup, DOF by
// DOF, without the launches (3 - 6 per rank-iteration at ~6 us each).  src[k][i] = (list index << 4) | buffer (0 .. 11: 2 l + side, the receive buffers of the six
// links, a pointer table in device memory), -1 = none; built once per setup (Dist::buildFixup).
constexpr int FIX_MAXSRC = 4;
__global__ void __launch_bounds__(BS) k_dist_fixup_merged(const CGScalars* __restrict__ sc, const int32_t* __restrict__ dof, const int32_t* __restrict__ src, int64_t n, const double* const* __restrict__ bufs,
                                                          double* __restrict__ r, const diag_t* __restrict__ dinv, double* __restrict__ partial) {
    if (sc->done) return;
    __shared__ const double* sb[16];                      // the twelve receive buffers: one level less in the dependent chain src -> buffer -> value
    if (threadIdx.x < 12) sb[threadIdx.x] = bufs[threadIdx.x];
    __syncthreads();
    const double alpha = sc->alpha;
    double a0 = 0., a1 = 0.;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        const int j = dof[i];
        int e[FIX_MAXSRC];
#pragma unroll
        for (int k = 0; k < FIX_MAXSRC; ++k) e[k] = src[(size_t)k * (size_t)n + (size_t)i];
        double cv[FIX_MAXSRC];
#pragma unroll
        for (int k = 0; k < FIX_MAXSRC; ++k) cv[k] = e[k] >= 0 ? sb[e[k] & 15][e[k] >> 4] : 0.;   // all loads in flight before the sums
        const double ro = r[j];
        double rn = ro;
#pragma unroll
        for (int k = 0; k < FIX_MAXSRC; ++k)
            if (e[k] >= 0) rn -= alpha * cv[k];
        fixupRow(r, dinv, j, ro, rn, a0, a1);
    }
    fixupPartials(a0, a1, partial);
}

// ---- generic vector helpers (BiCGStab fallback, rare) -----------------------------------------------
__global__ void __launch_bounds__(BS) k_dot(const double* __restrict__ a, const double* __restrict__ b, int64_t n, double* __restrict__ partial) {
    double acc = 0.;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) acc += a[i] * b[i];
    const double s = blockReduceSum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// ---- Chebyshev-Jacobi polynomial preconditioner (PS_PRE_CHEBYSHEV) -------------------------------------------------
// first term: z_1 = dinv r / theta ; partial of r.z (used when the polynomial has this one term only)
// TZ: element type z is stored in (float: PS_PRE_CHEBYSHEV_F32; r.z is formed with the value as stored)
template <class TZ>
__global__ void __launch_bounds__(BS) k_cheb_first(const CGScalars* __restrict__ sc, const double* __restrict__ r, const diag_t* __restrict__ dinv,
                                                   double invTheta, TZ* __restrict__ z, int64_t n, double* __restrict__ partial) {
    if (sc && sc->done) return;
    double acc = 0.;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        const double rv = r[i];
        const TZ vs = (TZ)(diagValue(dinv[i]) * rv * invTheta);
        z[i] = vs;
        const double v = (double)vs;
        acc += rv * v;
    }
    const double s = blockReduceSum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// a later term, unfused form (the St kernel's MODE 2 epilogue does the same per row): Az = A z_j given; z_{j+1} -> znext, which may be
// the z_{j-1} buffer (zprev null: z_{j-1} = 0)
__global__ void __launch_bounds__(BS) k_cheb_step(const CGScalars* __restrict__ sc, const double* __restrict__ r, const diag_t* __restrict__ dinv,
                                                  const double* __restrict__ Az, double c1, double c2, const double* __restrict__ z, const double* zprev,
                                                  double* znext, int64_t n, double* __restrict__ partial) {
    if (sc && sc->done) return;
    double acc = 0.;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        const double rv = r[i], zj = z[i];
        const double zn = zj + (c1 * (zj - (zprev ? zprev[i] : 0.)) + c2 * (diagValue(dinv[i]) * (rv - Az[i])));
        znext[i] = zn;
        acc += rv * zn;
    }
    const double s = blockReduceSum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// one step of the power iteration on D^-1 A (ps_context::estimateLambdaMax): w = dinv .* Av ; partials of v.v and v.w
__global__ void __launch_bounds__(BS) k_power_step(const double* __restrict__ v, const double* __restrict__ Av, const double* __restrict__ dinv,
                                                   double* __restrict__ w, int64_t n, double* __restrict__ partial) {
    double avv = 0., avw = 0.;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        const double vi = v[i], wi = dinv[i] * Av[i];
        w[i] = wi;
        avv += vi * vi; avw += vi * wi;
    }
    const double s0 = blockReduceSum(avv), s1 = blockReduceSum(avw);
    if (threadIdx.x == 0) { partial[blockIdx.x] = s0; partial[gridDim.x + blockIdx.x] = s1; }
}
__global__ void k_widen_f32(double* __restrict__ out, const float* __restrict__ a, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (double)a[i];
}
__global__ void k_fill_f64(double* __restrict__ a, double v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) a[i] = v;
}
// constructGuessVectors (Solver.cpp:528-529): g holds -(S^T t) in the internal numbering; pressure entries stay, stress entries
// become -2 uInv g.  Indexed by REFERENCE index (pressures first) through permSys: every internal index is visited once.
__global__ void k_guess_finish(double* __restrict__ g, const double* __restrict__ uInv, const int32_t* __restrict__ permSys, int64_t nP, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < nP) continue;
        const int32_t j = permSys[i];
        g[j] = -2. * uInv[j] * g[j];
    }
}
// out = ca*a + cb*b + cc*c  (null pointers skipped)
__global__ void k_lin(double* __restrict__ out, double ca, const double* __restrict__ a, double cb, const double* __restrict__ b, double cc,
                      const double* __restrict__ c, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double v = ca * a[i];
        if (b) v += cb * b[i];
        if (c) v += cc * c[i];
        out[i] = v;
    }
}

// ---- Jacobi diagonal (extension; reference stub Preconditioners.cpp:37-41) ------------------------
// diag_j = -dt sum_f McInv_f S_fj^2 - sum_r q^T BInv_r q - 1/2 uInv_j,  q = sum_{f in r} C_f S_fj
// A lane owns DOF j.  The entries of its St row are sorted by column and a tile's skin rows are contiguous, so the entries on ONE
// tile form a run: every lane folds its next run into q (26 moments), then the wave does the quadratic forms tile by tile — the
// tile's BInv is wave-uniform, read with scalar loads into SGPRs, its upper triangle only (BInv is symmetric up to rounding; the test
// bound is 1e-9): 351 fused multiply-adds per form instead of 676 multiplies, 676 adds and 676 vector loads of one address each
// (the vector-memory path takes 16 cycles per wave for such a load: the r02 kernel took 6.3 ms of the 256^3 setup, this one 3.8;
// fetching a row's entries up front and folding them through the 3 x 10 moments was tried: 220 VGPRs, 6.2 ms).
__global__ void __launch_bounds__(256) k_jacobi_diag(const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, const double* __restrict__ val,
                              const int8_t* __restrict__ code, double valScale, int n, int nP,
                              int nA, double dt, const double* __restrict__ McInv, const double* __restrict__ uInv,
                              const uint32_t* __restrict__ rrowFace, const int32_t* __restrict__ rrowRegion, const double* __restrict__ COM,
                              double dx, int3 off, const double* __restrict__ Binv, double* __restrict__ dinv, int invert) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < n;
    double diag = 0.;
    int p = live ? ptr[j] : 0;
    const int pe = live ? ptr[j + 1] : 0;
    while (true) {
        double q[PS_RD];
#pragma unroll
        for (int m = 0; m < PS_RD; ++m) q[m] = 0.;
        int cur = -1;
        while (p < pe) {
            const int f = col[p];
            const double v = val ? val[p] : (double)code[p] * valScale;   // (coded blocks keep no fp64 values: the same bits)
            if (f < nA) { diag += -dt * McInv[f] * v * v; ++p; continue; }
            const int rr = f - nA;
            const int r = rrowRegion[rr];
            if (cur >= 0 && r != cur) break;                            // the next tile's run: next round
            cur = r;
            double o[3];
            int axis;
            rowOffset(rrowFace[rr], COM, r, dx, off, o, &axis);
            double c[PS_RD];
            basisRow(o[0], o[1], o[2], axis, c);
#pragma unroll
            for (int m = 0; m < PS_RD; ++m) q[m] += c[m] * v;
            ++p;
        }
        bool pend = cur >= 0;
        unsigned long long todo = __ballot(pend);
        if (todo == 0ull) break;                                        // wave-uniform: no lane has a run left
        while (todo != 0ull) {
            const int rl = __builtin_amdgcn_readlane(cur, __ffsll((long long)todo) - 1);
            const double* __restrict__ B = Binv + (int64_t)rl * PS_RD * PS_RD;   // wave-uniform: scalar loads
            double s = 0.;
#pragma unroll
            for (int m = 0; m < PS_RD; ++m) {
                double t = 0.;
#pragma unroll
                for (int k = m + 1; k < PS_RD; ++k) t = __builtin_fma(B[m * PS_RD + k], q[k], t);
                s = __builtin_fma(q[m], __builtin_fma(B[m * PS_RD + m], q[m], 2. * t), s);
            }
            if (pend && cur == rl) { diag -= s; pend = false; }          // (lanes of other tiles computed a value they drop)
            todo = __ballot(pend);
        }
    }
    if (!live) return;
    diag += -0.5 * uInv[j];
    dinv[j] = invert ? (diag != 0. ? 1. / diag : 1.) : diag;   // raw diagonal when halo contributions are still to be added
}

// ---- recovery and write-back ---------------------------------------------------------------------
// u_a = dt McInv (invDt rhs_a - (G p + Dt tau))      Solver.cpp:507
__global__ void k_recover_active(const double* __restrict__ s, const double* __restrict__ McInv, const double* __restrict__ rhsA, double dt,
                                 double invDt, int64_t nA, double* __restrict__ ua) {
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nA; f += (int64_t)gridDim.x * blockDim.x)
        ua[f] = dt * McInv[f] * (invDt * rhsA[f] - s[f]);
}
// applySolutionToVelocity, Solver.cpp:937-1028
__global__ void k_writeback(Grid g, int axis, const int32_t* __restrict__ lab, const int32_t* __restrict__ act, const int32_t* __restrict__ reg,
                            const int32_t* __restrict__ faceRow, const double* __restrict__ ua, const double* __restrict__ creg, const double* __restrict__ COM,
                            double dx, int3 off, const float* __restrict__ cvel, const float* __restrict__ velIn, float* __restrict__ velOut, int apply) {
    const int3 d = g.dims(1 + axis);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int l = lab[c];
    float out = velIn[c];
    if (apply && !(l == PS_UNSOLVED || l == PS_UNASSIGNED)) {
        const int r = reg[c];
        const int a = act[c];
        double v = 0.;
        if (r >= 0) {
            const int3 q = unlin3(d, c);
            // ps_common.hpp: faceOffset, written out: calling it swaps the operands of two multiplies of this kernel (profiles/region_box.md, section 1)
            double p[3] = {(double)(q.x + off.x), (double)(q.y + off.y), (double)(q.z + off.z)};
            p[axis] -= 0.5;
            const double ox = p[0] * dx - COM[(int64_t)r * 3 + 0], oy = p[1] * dx - COM[(int64_t)r * 3 + 1], oz = p[2] * dx - COM[(int64_t)r * 3 + 2];
            double C[PS_RD];
            basisRow(ox, oy, oz, axis, C);
            double s = 0.;
            for (int n = 0; n < PS_RD; ++n) s += creg[(int64_t)r * PS_RD + n] * C[n];
            v = s;
        } else if (a >= 0) {
            const int row = faceRow[c];
            v = row >= 0 ? ua[row] : (double)velIn[c];   // active face of another rank (halo): left untouched
        } else if (l == PS_SOLID) {
            v = (double)cvel[c];
        }
        out = (float)v;
    }
    velOut[c] = out;
}

