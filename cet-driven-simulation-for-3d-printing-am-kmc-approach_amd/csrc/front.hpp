// front.hpp -- solidification-front diagnostics on the device (not in the reference).
//
// One streaming pass over T and state of a whole lattice (single slab): a voxel is a FRONT voxel when it is occupied
// (state != 0) and one of its six face neighbours inside the lattice is empty (the 255 sentinel outside the lattice is not
// 0, so the lattice faces need no test); at every front voxel the temperature gradient is taken by central differences
// (one-sided at the lattice faces: T has no j / k padding and its i halo planes hold no data), G = |grad T|.  A MELT voxel
// is any voxel with T >= T_melt.  Nothing is written back to the lattice.
//
// k_front_stats: 2.5-D blocked like k_thermal_march.  A block owns FRONT_TJ rows x FRONT_TK columns and marches over
// FRONT_NI planes; T and state of the planes i-1, i, i+1 of a thread's own voxel live in registers, plane i additionally in
// an LDS tile with a one-voxel rim for the j+-1 / k+-1 neighbours.  Every T value and state byte is read once per tile plus
// the rim and the two planes around a plane group.
// The f64 sums are deterministic: a thread adds its voxels in plane order, a block folds its threads by a fixed butterfly
// and its four waves in order into ONE partial record, and k_front_fold (one block per lattice) folds the partials
// strided by thread and then by the same tree.  The grid of a lattice depends on L alone, so a replica of the batched call
// gets the bits of the same lattice on a single handle.  No floating-point atomics (no atomics at all).
#pragma once
#include "voxel.hpp"
#include "kernels.hpp"

namespace cetkmc {

constexpr int FRONT_TJ = 8, FRONT_TK = 32, FRONT_NI = 16;
using FrontStats = struct ::cetkmc_front_stats;      // (the C ABI has a function of the same name: elaborated specifier)

struct FrontPart {            // partial result of one block (and the accumulator of one thread)
    long long n_front, n_skipped, pos[3], n_melt;
    double G_sum, Gi_sum, T_sum, G_min, G_max;
    int bb[6];                // melt bounding box: imin, jmin, kmin, imax, jmax, kmax
};

__device__ __forceinline__ FrontPart front_empty(int L)
{
    FrontPart a;
    a.n_front = a.n_skipped = a.n_melt = 0;
    a.pos[0] = a.pos[1] = a.pos[2] = 0;
    a.G_sum = a.Gi_sum = a.T_sum = 0.0;
    a.G_min = __builtin_huge_val(); a.G_max = -__builtin_huge_val();
    a.bb[0] = a.bb[1] = a.bb[2] = L; a.bb[3] = a.bb[4] = a.bb[5] = -1;
    return a;
}
// a := a (+) b; the sums are a + b in this order
__device__ __forceinline__ void front_merge(FrontPart& a, const FrontPart& b)
{
    a.n_front += b.n_front; a.n_skipped += b.n_skipped; a.n_melt += b.n_melt;
    a.G_sum = a.G_sum + b.G_sum; a.Gi_sum = a.Gi_sum + b.Gi_sum; a.T_sum = a.T_sum + b.T_sum;
    a.G_min = b.G_min < a.G_min ? b.G_min : a.G_min;
    a.G_max = b.G_max > a.G_max ? b.G_max : a.G_max;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.pos[c] += b.pos[c];
        a.bb[c] = min(a.bb[c], b.bb[c]);
        a.bb[3 + c] = max(a.bb[3 + c], b.bb[3 + c]);
    }
}
// Fold of the 256 threads of a block; the result is valid in thread 0.  Butterfly over the 64 lanes (both partners form
// x + y from the same two values, so every lane of a wave ends with the same bits), then the four waves in order.
__device__ __forceinline__ void front_block_fold(FrontPart& a, FrontPart* wpart)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        FrontPart b;
        b.n_front = __shfl_xor(a.n_front, m); b.n_skipped = __shfl_xor(a.n_skipped, m); b.n_melt = __shfl_xor(a.n_melt, m);
        b.G_sum = __shfl_xor(a.G_sum, m); b.Gi_sum = __shfl_xor(a.Gi_sum, m); b.T_sum = __shfl_xor(a.T_sum, m);
        b.G_min = __shfl_xor(a.G_min, m); b.G_max = __shfl_xor(a.G_max, m);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            b.pos[c] = __shfl_xor(a.pos[c], m);
            b.bb[c] = __shfl_xor(a.bb[c], m); b.bb[3 + c] = __shfl_xor(a.bb[3 + c], m);
        }
        front_merge(a, b);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wpart[w] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < 4; ++q) front_merge(a, wpart[q]);
}

// part[(blockIdx.y * gridDim.x + blockIdx.x)] of the lattice = this block's partial.  grid: x = (j, k) tile, y = plane group,
// z = replica (variadic trailing EnsSel: the replica-ensemble instantiation, as in cluster.hpp; T_melt from the replica's own
// parameters).  inv_dx = 1 / voxel edge, computed by the host like inv_dx2.
template <class... E>
__global__ __launch_bounds__(256) void k_front_stats(SlabView S, double T_melt, double inv_dx, FrontPart* part, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        const auto& e = ens_rep(blockIdx.z, ens...);
        S = e.view[0]; T_melt = e.kp.T_melt;
        part += (int64_t)blockIdx.z * gridDim.x * gridDim.y;
    }
    constexpr int TJ = FRONT_TJ, TK = FRONT_TK, LW = TK + 2;
    static_assert(TJ * TK == 256, "one voxel of a plane per thread");
    __shared__ double tT[(TJ + 2) * LW];
    __shared__ uint8_t tS[(TJ + 2) * LW];
    __shared__ FrontPart wpart[4];
    const int L = S.L;
    const int ntk = (L + TK - 1) / TK;
    const int tid = threadIdx.x, tj = tid / TK, tk = tid % TK;
    const int j0 = ((int)blockIdx.x / ntk) * TJ, k0 = ((int)blockIdx.x % ntk) * TK;
    const int j = j0 + tj, k = k0 + tk;
    const bool own = j < L && k < L;
    const int lp0 = blockIdx.y * FRONT_NI, lp1 = min(lp0 + FRONT_NI, S.nloc);
    const double half_inv_dx = 0.5 * inv_dx;
    // own voxel of global plane i: T only inside the lattice (the i halo planes of T hold nothing), state also one plane
    // outside (sentinel)
    auto ldT = [&](int i) { return (own && i >= 0 && i < L) ? S.T[S.tidx(i - (S.gi0 - 2), j, k)] : 0.0; };
    auto ldS = [&](int i) { return own ? S.state[S.sidx(i - (S.gi0 - 2), j, k)] : OOB; };
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
    FrontPart acc = front_empty(L);
    const int ig0 = S.gi0 + lp0;
    double Tp = ldT(ig0 - 1), Tc = ldT(ig0), Tn;
    uint8_t sp = ldS(ig0 - 1), sc = ldS(ig0), sn;
#pragma unroll 1
    for (int lp = lp0; lp < lp1; ++lp) {
        const int i = S.gi0 + lp, li = lp + 2;
        Tn = ldT(i + 1); sn = ldS(i + 1);
        tT[cell] = Tc; tS[cell] = sc;
        if (rcell >= 0) {
            tT[rcell] = rin ? S.T[S.tidx(li, rj, rk)] : 0.0;
            tS[rcell] = rin ? S.state[S.sidx(li, rj, rk)] : OOB;
        }
        __syncthreads();
        if (own) {
            if (Tc >= T_melt) {
                ++acc.n_melt;
                acc.bb[0] = min(acc.bb[0], i); acc.bb[1] = min(acc.bb[1], j); acc.bb[2] = min(acc.bb[2], k);
                acc.bb[3] = max(acc.bb[3], i); acc.bb[4] = max(acc.bb[4], j); acc.bb[5] = max(acc.bb[5], k);
            }
            const bool front = sc != 0 && (sp == 0 || sn == 0 || tS[cell - LW] == 0 || tS[cell + LW] == 0 ||
                                           tS[cell - 1] == 0 || tS[cell + 1] == 0);
            if (front) {
                const double jm = tT[cell - LW], jp = tT[cell + LW], km = tT[cell - 1], kp = tT[cell + 1];
                double gi, gj, gk;
                if (L == 1) { gi = gj = gk = 0.0; }
                else {
                    gi = (i == 0) ? (Tn - Tc) * inv_dx : (i == L - 1) ? (Tc - Tp) * inv_dx : (Tn - Tp) * half_inv_dx;
                    gj = (j == 0) ? (jp - Tc) * inv_dx : (j == L - 1) ? (Tc - jm) * inv_dx : (jp - jm) * half_inv_dx;
                    gk = (k == 0) ? (kp - Tc) * inv_dx : (k == L - 1) ? (Tc - km) * inv_dx : (kp - km) * half_inv_dx;
                }
                const double G = sqrt(gi * gi + gj * gj + gk * gk);
                if (finite_d(G) && finite_d(Tc)) {
                    ++acc.n_front;
                    acc.pos[0] += i; acc.pos[1] += j; acc.pos[2] += k;
                    acc.G_sum = acc.G_sum + G; acc.Gi_sum = acc.Gi_sum + gi; acc.T_sum = acc.T_sum + Tc;
                    acc.G_min = G < acc.G_min ? G : acc.G_min;
                    acc.G_max = G > acc.G_max ? G : acc.G_max;
                } else {
                    ++acc.n_skipped;
                }
            }
        }
        __syncthreads();
        Tp = Tc; Tc = Tn; sp = sc; sc = sn;
    }
    front_block_fold(acc, wpart);
    if (tid == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// out[r] = the nb partials of lattice r folded in a fixed order (one block per lattice)
__global__ __launch_bounds__(256) void k_front_fold(const FrontPart* __restrict__ part, int nb, int L, FrontStats* out)
{
    __shared__ FrontPart wpart[4];
    part += (int64_t)blockIdx.x * nb;
    FrontPart a = front_empty(L);
    for (int q = threadIdx.x; q < nb; q += 256) front_merge(a, part[q]);
    front_block_fold(a, wpart);
    if (threadIdx.x == 0) {
        FrontStats& o = out[blockIdx.x];
        o.n_front = a.n_front; o.n_skipped = a.n_skipped;
        o.G_sum = a.G_sum; o.Gi_sum = a.Gi_sum; o.T_sum = a.T_sum;
        o.G_min = a.n_front ? a.G_min : 0.0;
        o.G_max = a.n_front ? a.G_max : 0.0;
        o.n_melt = a.n_melt;
        for (int c = 0; c < 3; ++c) o.pos_sum[c] = a.pos[c];
        for (int c = 0; c < 6; ++c) o.melt_bbox[c] = a.bb[c];
    }
}

}  // namespace cetkmc
