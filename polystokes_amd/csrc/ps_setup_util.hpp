// Device and host helpers shared by the setup translation units (ps_grid.hip, ps_blocks.hip, ps_tiles.hip, ps_surface.hip, ps_context.hip,
// ps_pockets.hip, ps_motions.hip, ps_shapes.hip): the cell-field sampler and the two material-field descriptions built on it, the walk over
// a region's box (RegionBox), the block scan, the 64-bit mixer, the representative insert of the two hash tables and the collider kernels'
// wave histogram.  Not included by ps_solve.hip: nothing here may reach the solver's device code.
#pragma once
#include "ps_common.hpp"

namespace ps {

// One axis of SIM_RawField::getValue(pos): the two voxel centres around pos (cell-centre coordinates, clamped to the grid: streak border)
// and the fraction between them.
struct AxisSample { int i0, i1; float t; };
__device__ inline AxisSample axisSample(float pos, int n) {
    float u = pos - 0.5f;
    if (u < 0.f) u = 0.f;
    if (u > (float)(n - 1)) u = (float)(n - 1);
    int b = (int)u;
    if (b >= n - 1) { b = n - 1; return AxisSample{b, b, 0.f}; }
    return AxisSample{b, b + 1, u - (float)b};
}
// SIM_RawField::getValue(pos) restated: trilinear between voxel centres, streak border, fp32,
// lerp(a,b,t) = a + (b-a)*t, x then y then z.  The library is built with -ffp-contract=off so the
// result is bit-identical to the CPU restatement.
__device__ inline float sampleCenterField(const float* __restrict__ f, const Grid& g, float px, float py, float pz) {
    const AxisSample X = axisSample(px, g.nx), Y = axisSample(py, g.ny), Z = axisSample(pz, g.nz);
    const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
    auto at = [&](int i, int j, int k) { return f[i + j * sy + k * sz]; };
    auto L = [](float a, float b, float tt) { return a + (b - a) * tt; };
    const float c00 = L(at(X.i0, Y.i0, Z.i0), at(X.i1, Y.i0, Z.i0), X.t);
    const float c10 = L(at(X.i0, Y.i1, Z.i0), at(X.i1, Y.i1, Z.i0), X.t);
    const float c01 = L(at(X.i0, Y.i0, Z.i1), at(X.i1, Y.i0, Z.i1), X.t);
    const float c11 = L(at(X.i0, Y.i1, Z.i1), at(X.i1, Y.i1, Z.i1), X.t);
    const float c0 = L(c00, c10, Y.t);
    const float c1 = L(c01, c11, Y.t);
    return L(c0, c1, Z.t);
}

// A cell field that may be constant (the viscosity: ps_context::viscSource).  Trilinear interpolation of a constant returns it bit for
// bit (a + (b - a) t with a == b), so a uniform field is sampled without its 8 loads.
struct CellField {
    const float* p;
    int uniform;
    float value;
    __device__ float sample(const Grid& g, float px, float py, float pz) const { return uniform ? value : sampleCenterField(p, g, px, py, pz); }
};

// Density of the face (axis, i, j, k) (ps_context::densSource): the cell field sampled at the face centre with the sampler above — an
// interior face gets the mean of its two cells as a + (b - a) * 0.5f, a face on the grid boundary its one cell — clamped to
// [mindensity, maxdensity].  Without a field (p null): the scalar rho, unclamped (ps_upload_density_field).
struct FaceDensity {
    const float* p;
    double rho, lo, hi;
    __device__ double at(const Grid& g, int axis, int i, int j, int k) const {
        if (!p) return rho;
        const float px = (float)i + (axis == 0 ? 0.f : 0.5f), py = (float)j + (axis == 1 ? 0.f : 0.5f), pz = (float)k + (axis == 2 ? 0.f : 0.5f);
        const double v = (double)sampleCenterField(p, g, px, py, pz);
        return v < lo ? lo : (v > hi ? hi : v);
    }
};

// Is the host field one value everywhere, and which (ps_context::upload, uploadDensity)?
inline bool fieldIsUniform(const float* f, int64_t n, float* value) {
    *value = f[0];
    for (int64_t i = 1; i < n; ++i) if (f[i] != f[0]) return false;
    return true;
}

// The box of positions that a per-tile kernel, or the host loop that cuts its work items, walks for region r.  bbox[r * 6 ..] holds the
// smallest and the largest cell index of the region per axis (ps_grid.hip: k_bbox); the four shapes in use grow that box.  Position
// pos in [0, total()) is x-fastest.  total() is 64 bits wide: the host refuses a box of more than 0x7fffffff positions where it cuts the
// items (ps_tiles.hip: buildFaceBoxItems), after which a walk may keep pos in an int.
struct RegionBox {
    int x0, y0, z0;   // the first position
    int ex, ey, ez;   // positions per axis
    // the positions from `below` before the region's first cell to `above` after its last one, on every axis
    __host__ __device__ static RegionBox grown(const int32_t* __restrict__ bbox, int r, int below, int above) {
        const int32_t* b = bbox + r * 6;
        RegionBox B;
        B.x0 = b[0] - below; B.y0 = b[1] - below; B.z0 = b[2] - below;
        B.ex = b[3] - B.x0 + 1 + above; B.ey = b[4] - B.y0 + 1 + above; B.ez = b[5] - B.z0 + 1 + above;
        return B;
    }
    __host__ __device__ static RegionBox cells(const int32_t* __restrict__ bbox, int r) { return grown(bbox, r, 0, 0); }
    // the faces of one axis around the region's cells: one plane more along that axis
    __host__ __device__ static RegionBox faces(const int32_t* __restrict__ bbox, int r, int axis) {
        RegionBox B = grown(bbox, r, 0, 0);
        if (axis == 0) B.ex++; else if (axis == 1) B.ey++; else B.ez++;
        return B;
    }
    // the union of the three face boxes (one position more than the cells on every axis): a position stands for up to three faces
    __host__ __device__ static RegionBox faceUnion(const int32_t* __restrict__ bbox, int r) { return grown(bbox, r, 0, 1); }
    // the face union and one sample around it, i.e. cells first - 1 .. last + 2: what a tile's Mr and K read (ps_tiles.hip: k_tile_signature)
    __host__ __device__ static RegionBox ringed(const int32_t* __restrict__ bbox, int r) { return grown(bbox, r, 1, 2); }

    __host__ __device__ int64_t total() const { return (int64_t)ex * ey * ez; }
    // position pos on the grid (I: int, or int64_t where the total is not known to fit an int)
    template <class I>
    __host__ __device__ int3 at(I pos) const { return make_int3(x0 + (int)(pos % ex), y0 + (int)((pos / ex) % ey), z0 + (int)(pos / ((I)ex * ey))); }
};

// Exclusive scan of one int per thread over a workgroup of SETUP_BS threads (all of them call it); *total = the workgroup's sum.
constexpr int SETUP_BS = 256;
__device__ inline int blockExclusiveScan(int v, int* total) {
    __shared__ int waveSums[SETUP_BS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) waveSums[w] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < SETUP_BS / 64; ++i) {
        if (i < w) base += waveSums[i];
        tot += waveSums[i];
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// The open-addressing tables of the shared chunk runs (ps_blocks.hip) and the tile classes (ps_tiles.hip): 64-bit keys, HASH_EMPTY marks a
// free slot (a key that mixes to it is stored as 0), linear probing, the value of a key = the smallest index inserted with it.
constexpr unsigned long long HASH_EMPTY = 0xffffffffffffffffull;
__device__ inline unsigned long long mix64(unsigned long long x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}
// insert (h, idx), probing from `slot` (the caller's own bits of h); keys start as HASH_EMPTY, vals as 0x7f7f7f7f
__device__ inline void hashInsertMin(unsigned long long* __restrict__ keys, int32_t* __restrict__ vals, unsigned mask, unsigned slot, unsigned long long h, int idx) {
    for (unsigned probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
        unsigned long long cur = keys[slot];
        if (cur == HASH_EMPTY) { cur = atomicCAS(&keys[slot], HASH_EMPTY, h); if (cur == HASH_EMPTY) cur = h; }
        if (cur == h) { atomicMin(&vals[slot], idx); return; }
    }
}

// The wave histogram of the collider kernels (ps_motions.hip, ps_shapes.hip): every lane that is `on` counts once into the workgroup's LDS
// bin `slot`.  The wave adds once per distinct slot among its lanes: the first live lane's slot is broadcast, the lanes that share it are
// one ballot, the first of them adds their number, and the rest repeat (one round where the lanes agree, which is the rule away from
// where two colliders meet).  Every lane of the wave calls it; the workgroup adds its bins to the global counters at its end.
__device__ __forceinline__ void waveBinAdd(int32_t* bins, bool on, int slot, int lane) {
    unsigned long long todo = __ballot(on);
    while (todo) {
        const int s = __shfl(slot, __ffsll((long long)todo) - 1, 64);
        const unsigned long long same = __ballot(on && slot == s);
        if (lane == __ffsll((long long)same) - 1) atomicAdd(&bins[s], __popcll(same));
        todo &= ~same;
    }
}

}  // namespace ps
