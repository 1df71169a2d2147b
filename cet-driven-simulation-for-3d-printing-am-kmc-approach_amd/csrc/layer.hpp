// layer.hpp -- layer-resolved grain structure on the device (not in the reference).
//
// One streaming pass over the label volume of the last clustering (cluster.hpp) and the state of a whole lattice (single
// slab): per plane i of the build direction (axis 0) one record of 17 integer counters (cetkmc_layer_rec, include/cetkmc.h)
// -- occupied voxels, grain starts, voxels of equiaxed grains, grain-segment starts and grain-grain cuts along the three
// axes, and per species the occupied voxels and those with a face neighbour of another label.  Nothing is written back to
// the lattice, and there is no floating point in the voxel pass: the only double expression is the aspect-ratio test of
// k_layer_class, one thread per grain.
//
// k_layer_profile: 2.5-D blocked like k_front_stats.  A block owns LAYER_TJ rows x LAYER_TK columns and marches over
// LAYER_NI planes; the labels of the planes i-1, i, i+1 of a thread's own voxel live in registers, plane i additionally in
// an LDS tile with a one-voxel face rim for the j+-1 / k+-1 neighbours (row stride TK + 2 dwords: a 32-lane half reads 32
// consecutive dwords of one row, so the b32 reads are conflict free).  The label volume has no padding, so every load is
// made inside the lattice only and "outside" is decided from the coordinates.  Every counter is a predicate of the thread's
// own voxel: per plane a wave ballots it and counts the bits, the four waves meet in LDS, and the block writes ONE partial
// record per (plane, tile).  k_layer_fold sums the tiles of a plane: no atomics, no zeroing pass, and the same bits on every
// call (integer sums).
#pragma once
#include "voxel.hpp"
#include "kernels.hpp"

namespace cetkmc {

constexpr int LAYER_TJ = 8, LAYER_TK = 32, LAYER_NI = 16;
constexpr int LAYER_NC = 18;                        // int64 words of a record: 17 counters + pad
using LayerRec = struct ::cetkmc_layer_rec;
static_assert(sizeof(LayerRec) == LAYER_NC * 8, "cetkmc_layer_rec is 18 int64 words");

// eq[id] = 1 if grain id (1..n) is equiaxed: (double)max(d) / (double)max(min(d), 1) < ar_threshold over its bounding-box
// extents d (metrics.compute_metrics_from_clusters' expression); eq[0] = 0.  stats: k_cc_stats' table.
// (variadic trailing EnsSel: replica = blockIdx.y, its clusters at entry offs[r] of the concatenated table, its class bytes
// at offs[r] + r: every replica has one more byte than clusters)
template <class... E>
__global__ __launch_bounds__(256) void k_layer_class(const int* __restrict__ stats, int n, double ar_threshold, uint8_t* eq, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        const long long* o = ens_offs(ens...);
        const long long a = o[blockIdx.y];
        stats += 8 * a; eq += a + blockIdx.y; n = (int)(o[blockIdx.y + 1] - a);
    }
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q <= n; q += gridDim.x * blockDim.x) {
        uint8_t c = 0;
        if (q > 0) {
            const int* s = stats + 8 * (int64_t)(q - 1);
            const int d0 = s[4] - s[1] + 1, d1 = s[5] - s[2] + 1, d2 = s[6] - s[3] + 1;
            const int hi = max(d0, max(d1, d2)), lo = min(d0, min(d1, d2));
            c = ((double)hi / (double)max(lo, 1)) < ar_threshold;
        }
        eq[q] = c;
    }
}

// part[i * gridDim.x + blockIdx.x] of the lattice = this block's counts of plane i.  grid: x = (j, k) tile, y = plane group,
// z = replica (variadic trailing EnsSel, as in front.hpp: labels / roots at r * stride, class bytes at offs[r] + r).
// roots[id - 1] = linear index of grain id's first voxel in row-major order (ascending).
template <class... E>
__global__ __launch_bounds__(256) void k_layer_profile(SlabView S, const int* __restrict__ labels, const int* __restrict__ roots,
                                                        const uint8_t* __restrict__ eq, LayerRec* part, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        const int64_t o = (int64_t)blockIdx.z * ens_stride(ens...);
        S = ens_rep(blockIdx.z, ens...).view[0];
        labels += o; roots += o; eq += ens_offs(ens...)[blockIdx.z] + blockIdx.z;
        part += (int64_t)blockIdx.z * gridDim.x * S.L;
    }
    constexpr int TJ = LAYER_TJ, TK = LAYER_TK, LW = TK + 2;
    static_assert(TJ * TK == 256, "one voxel of a plane per thread");
    __shared__ int tL[(TJ + 2) * LW];
    __shared__ int wcnt[4 * LAYER_NC];
    const int L = S.L;
    const int ntk = (L + TK - 1) / TK;
    const int tid = threadIdx.x, tj = tid / TK, tk = tid % TK;
    const int lane = tid & 63, w = tid >> 6;
    const int j0 = ((int)blockIdx.x / ntk) * TJ, k0 = ((int)blockIdx.x % ntk) * TK;
    const int j = j0 + tj, k = k0 + tk;
    const bool own = j < L && k < L;
    const int i0 = blockIdx.y * LAYER_NI, i1 = min(i0 + LAYER_NI, L);
    // label of the own voxel of plane i; 0 outside the lattice (never compared there: the coordinates decide)
    auto ldG = [&](int i) { return (own && i >= 0 && i < L) ? labels[((int64_t)i * L + j) * L + k] : 0; };
    // the rim cell of this thread (tid < 2 TK + 2 TJ): rows j0-1 / j0+TJ, columns k0-1 / k0+TK; no corners (faces only)
    int rcell = -1, rj = 0, rk = 0;
    if (tid < 2 * TK + 2 * TJ) {
        int tr, tc;
        if (tid < 2 * TK) { tr = (tid < TK) ? 0 : TJ + 1; tc = 1 + tid % TK; }
        else { const int f = tid - 2 * TK; tr = 1 + (f >> 1); tc = (f & 1) ? TK + 1 : 0; }
        rj = j0 + tr - 1; rk = k0 + tc - 1;
        rcell = tr * LW + tc;
    }
    const bool rin = rcell >= 0 && rj >= 0 && rj < L && rk >= 0 && rk < L;
    const int cell = (tj + 1) * LW + tk + 1;
    const bool jlo = j > 0, jhi = j < L - 1, klo = k > 0, khi = k < L - 1;      // the face neighbour is inside the lattice
    int gp = ldG(i0 - 1), gc = ldG(i0), gn;
#pragma unroll 1
    for (int i = i0; i < i1; ++i) {
        gn = ldG(i + 1);
        const int st = own ? S.state[S.sidx(i - (S.gi0 - 2), j, k)] : 0;
        tL[cell] = gc;
        if (rcell >= 0) tL[rcell] = rin ? labels[((int64_t)i * L + rj) * L + rk] : 0;
        __syncthreads();
        const int g = gc;
        const bool occ = own && g != 0;
        const int jm = tL[cell - LW], jp = tL[cell + LW], km = tL[cell - 1], kp = tL[cell + 1];
        const bool ilo = i > 0, ihi = i < L - 1;
        bool p[LAYER_NC - 1];
        p[0] = occ;
        p[3] = occ && (!ilo || gp != g);
        p[4] = occ && (!jlo || jm != g);
        p[5] = occ && (!klo || km != g);
        p[6] = occ && ilo && gp != 0 && gp != g;
        p[7] = occ && jlo && jm != 0 && jm != g;
        p[8] = occ && klo && km != 0 && km != g;
        // a grain's first voxel has no predecessor of its own label along any axis: only those look their root up
        p[1] = false;
        if (p[3] && p[4] && p[5]) p[1] = roots[g - 1] == (int)(((int64_t)i * L + j) * L + k);
        p[2] = occ && eq[g] != 0;
        const bool gb = occ && ((ilo && gp != g) || (ihi && gn != g) || (jlo && jm != g) || (jhi && jp != g) ||
                                (klo && km != g) || (khi && kp != g));
#pragma unroll
        for (int t = 1; t <= 4; ++t) { p[8 + t] = occ && st == t; p[12 + t] = gb && st == t; }
#pragma unroll
        for (int c = 0; c < LAYER_NC - 1; ++c) {
            const int n = __popcll(__ballot(p[c]));
            if (lane == 0) wcnt[w * LAYER_NC + c] = n;
        }
        __syncthreads();
        if (tid < LAYER_NC) {
            long long s = 0;
            if (tid < LAYER_NC - 1) s = (long long)wcnt[tid] + wcnt[LAYER_NC + tid] + wcnt[2 * LAYER_NC + tid] + wcnt[3 * LAYER_NC + tid];
            reinterpret_cast<long long*>(part + ((int64_t)i * gridDim.x + blockIdx.x))[tid] = s;
        }
        gp = gc; gc = gn;
    }
}

// out[r * L + i] = the nt tile partials of plane i of lattice r summed (grid: x = plane, y = lattice; one wave, one lane
// per counter)
__global__ __launch_bounds__(64) void k_layer_fold(const LayerRec* __restrict__ part, int nt, LayerRec* out)
{
    const int64_t rec = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x < LAYER_NC) {
        const long long* p = reinterpret_cast<const long long*>(part + rec * nt) + threadIdx.x;
        long long s = 0;
        for (int q = 0; q < nt; ++q) s += p[(int64_t)q * LAYER_NC];
        reinterpret_cast<long long*>(out + rec)[threadIdx.x] = s;
    }
}

}  // namespace cetkmc
