// texture.hpp -- grain-boundary misorientation and pole histograms per build plane (not in the
// reference).
//
// One streaming pass over the label volume of the last clustering (cluster.hpp) and the orientation unit vectors S.ovec of
// a whole lattice (single slab): 4 + 24 B read per voxel, nothing written to the lattice.  Per plane i of the build
// direction (axis 0) the result is one row of 4 * n_bins + 4 integer counters (include/cetkmc.h, cetkmc_texture_profile):
//   [a * n_bins + b], a = 0..2   grain-grain faces of the plane across axis a whose dot product d = o(u) . o(v) is in bin b
//   [3 * n_bins + b]             occupied voxels whose |axis . o(v)| is in bin b
//   [4 * n_bins + a], a = 0..3   faces across axis a (a = 3: voxels) whose value is not finite
// bin(x) = number of edges with x <= e[q] over n_bins - 1 strictly decreasing edges (cosines of ascending angles, from the
// host): no acos and no clamp here.  The dot products are summed left to right and the translation unit is compiled with
// -ffp-contract=off, so the counters are defined to the bit given ovec.
//
// k_texture_profile is blocked like k_layer_profile: a block owns TEX_TJ rows x TEX_TK columns (one voxel per thread) and
// marches over TEX_NI planes.  Only predecessors are read: the own voxel's label and vector of plane i - 1 stay in
// registers, plane i goes into an LDS tile with a low-side rim (row j0 - 1, column k0 - 1).  The vectors are kept as three
// component tiles of doubles: the 32 lanes of a half-wave are the 32 columns of one tile row, so a 64-bit read of a
// predecessor (the same row one column down, or the row below) touches 32 consecutive doubles = all 64 banks once,
// whatever the row stride; TEX_LW = TK + 1 holds the rim column.  The label volume has no padding and ovec's halo planes
// are never addressed: "outside" is decided from the coordinates, never by loading.  The edges go into LDS once per block,
// padded to 63 with -inf so that binning is a fixed six-step search.  Per plane the block counts into an LDS histogram of
// 32-bit counters (three faces and one pole value per voxel: at most 1024 increments per plane) with LDS integer atomics and
// flushes only its non-zero counters with 64-bit global integer atomics into the result rows, which the host zeroes on the
// stream before the launch: integer sums, so every accumulation order gives the same bits and two calls agree.  (A
// (plane, tile) partial array with a fold, as in layer.hpp, would take L * tiles * (4 * 64 + 4) * 8 B: tens of MB at L = 256.)
#pragma once
#include "voxel.hpp"
#include "kernels.hpp"

namespace cetkmc {

constexpr int TEX_TJ = 8, TEX_TK = 32, TEX_NI = 16;
constexpr int TEX_MAX_BINS = 64, TEX_NE = TEX_MAX_BINS - 1;

// by-value kernel argument: the caller's axis and the two edge arrays, padded with -inf behind the n_bins - 1 real edges
struct TexArgs {
    int n_bins, pad;
    double axis[3];
    double edges[2][TEX_NE];       // [0] boundary dot products, [1] pole cosines
};

// number of edges with x <= e[q]: e[0 .. 62] strictly decreasing, then -inf; x finite
__device__ __forceinline__ int tex_bin(const double* e, double x)
{
    int pos = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1)
        if (x <= e[pos + step - 1]) pos += step;
    return pos;
}

// out[(i * (4 n_bins + 4)) + c] += this block's count c of plane i.  grid: x = (j, k) tile, y = plane group, z = replica
// (variadic trailing EnsSel, as in layer.hpp: labels at r * stride, result rows of replica r behind those of r - 1).
template <class... E>
__global__ __launch_bounds__(256) void k_texture_profile(SlabView S, const int* __restrict__ labels, TexArgs A,
                                                          unsigned long long* out, E... ens)
{
    constexpr int TJ = TEX_TJ, TK = TEX_TK, LW = TK + 1, NCELL = (TJ + 1) * LW;
    static_assert(TJ * TK == 256, "one voxel of a plane per thread");
    const int nb = A.n_bins, nc = 4 * nb + 4;
    if constexpr (sizeof...(E) > 0) {
        S = ens_rep(blockIdx.z, ens...).view[0];
        labels += (int64_t)blockIdx.z * ens_stride(ens...);
        out += (int64_t)blockIdx.z * S.L * nc;
    }
    __shared__ double tV[3][NCELL];
    __shared__ double sE[2][TEX_NE + 1];
    __shared__ int tL[NCELL];
    __shared__ unsigned hist[4 * TEX_MAX_BINS + 4];
    const int L = S.L;
    const int ntk = (L + TK - 1) / TK;
    const int tid = threadIdx.x, tj = tid / TK, tk = tid % TK;
    const int j0 = ((int)blockIdx.x / ntk) * TJ, k0 = ((int)blockIdx.x % ntk) * TK;
    const int j = j0 + tj, k = k0 + tk;
    const bool own = j < L && k < L;
    const int i0 = blockIdx.y * TEX_NI, i1 = min(i0 + TEX_NI, L);
    const int lo = 2 - S.gi0;                          // local plane of global plane 0 (two halo planes below)
    // the rim cell of this thread (tid < TK + TJ): row j0 - 1 (tile row 0), column k0 - 1 (tile column 0); no corner
    int rcell = -1, rj = 0, rk = 0;
    if (tid < TK + TJ) {
        const int tr = tid < TK ? 0 : 1 + (tid - TK), tc = tid < TK ? 1 + tid : 0;
        rj = j0 + tr - 1; rk = k0 + tc - 1;
        rcell = tr * LW + tc;
    }
    const bool rin = rcell >= 0 && rj >= 0 && rj < L && rk >= 0 && rk < L;
    const int cell = (tj + 1) * LW + tk + 1;
    const bool jlo = j > 0, klo = k > 0;               // the predecessor is inside the lattice
    if (tid < 2 * (TEX_NE + 1)) {
        const int w = tid / (TEX_NE + 1), q = tid % (TEX_NE + 1);
        sE[w][q] = q < nb - 1 ? A.edges[w][q] : -__builtin_inf();
    }
    for (int q = tid; q < nc; q += 256) hist[q] = 0;
    // the own voxel of plane i0 - 1: label 0 outside the lattice (never compared there: the coordinates decide)
    int gp = 0;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (own && i0 > 0) {
        gp = labels[((int64_t)(i0 - 1) * L + j) * L + k];
        const double* o = S.ovec + 3 * S.tidx(i0 - 1 + lo, j, k);
        p0 = o[0]; p1 = o[1]; p2 = o[2];
    }
#pragma unroll 1
    for (int i = i0; i < i1; ++i) {
        int g = 0;
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
        if (own) {
            g = labels[((int64_t)i * L + j) * L + k];
            const double* o = S.ovec + 3 * S.tidx(i + lo, j, k);
            v0 = o[0]; v1 = o[1]; v2 = o[2];
        }
        tL[cell] = g; tV[0][cell] = v0; tV[1][cell] = v1; tV[2][cell] = v2;
        if (rcell >= 0) {
            int rg = 0;
            double r0 = 0.0, r1 = 0.0, r2 = 0.0;
            if (rin) {
                rg = labels[((int64_t)i * L + rj) * L + rk];
                const double* o = S.ovec + 3 * S.tidx(i + lo, rj, rk);
                r0 = o[0]; r1 = o[1]; r2 = o[2];
            }
            tL[rcell] = rg; tV[0][rcell] = r0; tV[1][rcell] = r1; tV[2][rcell] = r2;
        }
        __syncthreads();
        if (own && g != 0) {
            // histogram a (0..2: faces across axis a against the boundary edges, 3: the pole value against its own)
            auto count = [&](int a, double x) {
                atomicAdd(&hist[finite_d(x) ? a * nb + tex_bin(sE[a == 3], x) : 4 * nb + a], 1u);
            };
            // a face across axis a: the predecessor is inside the lattice, occupied and of another grain (layer.hpp's
            // cut[a]); only then is its vector read
            auto face = [&](int a, bool inside, int c) {
                const int gu = tL[c];
                if (inside && gu != 0 && gu != g) count(a, tV[0][c] * v0 + tV[1][c] * v1 + tV[2][c] * v2);
            };
            if (i > 0 && gp != 0 && gp != g) count(0, p0 * v0 + p1 * v1 + p2 * v2);
            face(1, jlo, cell - LW);
            face(2, klo, cell - 1);
            count(3, fabs(A.axis[0] * v0 + A.axis[1] * v1 + A.axis[2] * v2));
        }
        __syncthreads();
        for (int q = tid; q < nc; q += 256) {
            const unsigned n = hist[q];
            if (n) { atomicAdd(out + (int64_t)i * nc + q, (unsigned long long)n); hist[q] = 0; }
        }
        gp = g; p0 = v0; p1 = v1; p2 = v2;
    }
}

}  // namespace cetkmc
