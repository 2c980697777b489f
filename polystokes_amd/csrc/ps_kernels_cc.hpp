// Min-label propagation of connected components over a cell grid: the two kernels that take ANY link byte plus label array.
// Included inside the anonymous namespace of ps_grid.hip (the REDUCED regions: k_cc_init there) and of ps_pockets.hip (the air pockets:
// k_pocket_init there).  cc[c]: the label of cell c — the traversal-order index (g.order) of a cell of its component, INT_MAX for a cell that
// takes no part; link[c]: bit 2 a + dir = the link of c to its neighbour along axis a (dir 0: below, 1: above) exists, both ends set it.
// Labels only decrease: the fix point is the smallest order index of each component whatever the interleaving.
// No include of its own (it is pasted into a namespace): the including file has <limits.h> (INT_MAX) and ps_common.hpp (Grid, lin3,
// orderToIjk, with `using namespace ps`) before it.
#pragma once

__global__ void k_cc_step(Grid g, const uint8_t* __restrict__ link, int32_t* cc, int32_t* __restrict__ changed) {
    const int3 d = g.dims(0);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)d.x * d.y * d.z) return;
    const int lk = link[c];
    const int mine = cc[c];
    if (mine == INT_MAX) return;                                      // not a cell of any component
    int m = mine;
    const int64_t stride[3] = {1, d.x, (int64_t)d.x * d.y};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            if (!((lk >> (2 * a + dir)) & 1)) continue;
            const int v = cc[c + (dir ? stride[a] : -stride[a])];
            if (v < m) m = v;
        }
    }
    // pointer jump through the current representative
    const int3 rq = orderToIjk(d, g.order, m);
    const int v2 = cc[lin3(d, rq.x, rq.y, rq.z)];
    if (v2 < m) m = v2;
    if (m < mine) { atomicMin(&cc[c], m); *changed = 1; }
}
// The same propagation inside one box of B^3 cells (B = tile size: with doTile a component never leaves its tile, the padding layer
// between two tiles is ACTIVE), labels in LDS, to the box's fix point — one launch instead of a dozen k_cc_step passes over the grid
// and two host round trips less.  Links that leave the box are left to k_cc_step, which runs afterwards until nothing changes
// (once, when every component is tile-local): the fix point — the smallest order index of each component — is the same.
__global__ void __launch_bounds__(256) k_cc_local(Grid g, int B, const uint8_t* __restrict__ link, int32_t* __restrict__ cc) {
    extern __shared__ int32_t shcc[];
    const int3 d = g.dims(0);
    const int x0 = blockIdx.x * B, y0 = blockIdx.y * B, z0 = blockIdx.z * B;
    const int ex = min(B, d.x - x0), ey = min(B, d.y - y0), ez = min(B, d.z - z0);
    const int nb = ex * ey * ez;
    uint8_t* shlk = (uint8_t*)(shcc + B * B * B);
    int any = 0;
    for (int i = threadIdx.x; i < nb; i += 256) {
        const int lx = i % ex, ly = (i / ex) % ey, lz = i / (ex * ey);
        const int64_t c = lin3(d, x0 + lx, y0 + ly, z0 + lz);
        const int v = cc[c];
        int lk = link[c];
        // links that leave the box: not followed here
        if (lx == 0) lk &= ~1; if (lx == ex - 1) lk &= ~2;
        if (ly == 0) lk &= ~4; if (ly == ey - 1) lk &= ~8;
        if (lz == 0) lk &= ~16; if (lz == ez - 1) lk &= ~32;
        shcc[i] = v;
        shlk[i] = (uint8_t)lk;
        any |= (v != INT_MAX && lk != 0) ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;                                  // no cell with a link inside the box
    const int st[3] = {1, ex, ex * ey};
    for (int guard = 0; guard < 4 * B * B; ++guard) {                    // (a component's longest shortest path inside the box)
        int changed = 0;
        for (int i = threadIdx.x; i < nb; i += 256) {
            const int lk = shlk[i];
            if (!lk) continue;
            // the six reads at once (a link that is not there reads the cell itself): one LDS latency per cell instead of up to seven
            int v[6];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[2 * a] = shcc[(lk & (1 << (2 * a))) ? i - st[a] : i];
                v[2 * a + 1] = shcc[(lk & (2 << (2 * a))) ? i + st[a] : i];
            }
            const int mine = shcc[i];
            int m = mine;
#pragma unroll
            for (int q = 0; q < 6; ++q) m = min(m, v[q]);
            if (m < mine) { atomicMin(&shcc[i], m); changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }
    for (int i = threadIdx.x; i < nb; i += 256) {
        if (!shlk[i]) continue;
        const int lx = i % ex, ly = (i / ex) % ey, lz = i / (ex * ey);
        cc[lin3(d, x0 + lx, y0 + ly, z0 + lz)] = shcc[i];
    }
}
