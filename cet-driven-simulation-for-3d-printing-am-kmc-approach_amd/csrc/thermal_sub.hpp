// thermal_sub.hpp -- sub-steps 2..n of a sub-stepped temperature update, temporally blocked.
//
// A temperature update with thermal_substeps = n is n applications of the explicit step with dt / n.  The first is the
// existing launch (scrub, latent heat, prev_state := state); the others carry no scrub and no latent term, and
// k_thermal_sub<LASER, S> performs S of them per launch: the field is read once, with a rim of S cells, and written
// once (3.5-D blocking).  Same per-cell expression order as k_thermal / thermal_voxel(), same bits as S launches of them.
//
// One block owns an extended tile of SUB_EJ rows x SUB_EK columns -- the (SUB_EJ - 2 S) x (SUB_EK - 2 S) cells it writes plus
// the rim -- and marches over its plane group plus S planes on either side.  A thread owns four adjacent columns of one row
// at EVERY time level.  For each level s < S it keeps two planes of its cells in registers (i - 1 and i; plane i + 1 is the
// value it has just computed one level below), and the block keeps ONE plane per level in LDS for the j +- 1 and the outer
// k +- 1 neighbours.  When the input plane t arrives, level s computes plane t - s, so the result leaves S planes behind
// the load.  What a level computes in the outermost ring of its tile is wrong (it lacks a neighbour); the ring of
// wrong values grows by one cell per level and has reached exactly the rim when level S is stored.  Lattice edges are no
// such ring: a neighbour outside the lattice is the cell's own value AT THAT LEVEL (np.pad mode='edge' of every sub-step), in
// j, k and the plane direction alike; what a thread holds for a cell outside the lattice is never read.
//
// LDS per cell-update: 2 x 8 B (j +- 1) + 2 x 8 B / 4 (the column quad's outer k neighbours) + 8 B written = 28 B.
#pragma once
#include "kernels.hpp"

namespace cetkmc {

constexpr int SUB_EJ = 32, SUB_EK = 128, SUB_SMAX = 4;      // S * SUB_EJ * SUB_EK * 8 B of LDS: 128 KiB at S = 4
// Defaults by measurement (MI355X, n = 17, laser + latent heat, profiles/thermal_substeps.json): at 256^3 S = 3 is the fastest
// leg (1343 us per update; S = 2 1387, S = 4 1484, one launch per sub-step 1697); at 128^3 one launch per sub-step is (393 us
// against 425 / 437 / 458), so lattices up to SUB_PLAIN_L take the plain path unless option substep_block says otherwise.
constexpr int SUB_SDEFAULT = 3, SUB_PLAIN_L = 128;
constexpr int SUB_THREADS = SUB_EJ * SUB_EK / 4;

// (No ensemble instantiation: ensembles stop at L = 128, where one launch of k_thermal_march<EnsSel> per sub-step is faster.)
template <int LASER, int S>
__global__ __launch_bounds__(SUB_THREADS) void k_thermal_sub(SlabView V, const double* __restrict__ Tin, double* __restrict__ Tout,
                                                             const double* __restrict__ q_top, ThermalCfg C,
                                                             const StepState* __restrict__ ss)
{
    static_assert(S >= 1 && S <= SUB_SMAX && 2 * S < SUB_EJ, "sub-steps per launch");
    const unsigned bz = blockIdx.z;             // plane group of the block
    constexpr int EJ = SUB_EJ, EK = SUB_EK, CJ = EJ - 2 * S, CK = EK - 2 * S;
    __shared__ double lds[S][EJ][EK];
    const int L = V.L;
    const int tid = threadIdx.x;
    const int r = tid >> 5, c4 = (tid & 31) * 4;                 // row and first column inside the extended tile
    const int j = (int)blockIdx.y * CJ - S + r, k0 = (int)blockIdx.x * CK - S + c4;
    const int i0 = V.gi0 + (int)bz * C.ni, i1 = min(i0 + C.ni, V.gi0 + V.nloc);    // global planes [i0, i1) are written
    const int lofs = V.gi0 - 2;                                  // global plane -> local
    const bool jin = j >= 0 && j < L;
    bool in[4], core[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        in[h] = jin && k0 + h >= 0 && k0 + h < L;
        core[h] = in[h] && r >= S && r < EJ - S && c4 + h >= S && c4 + h < EK - S;
    }
    if (ss && ss->status) {                     // a terminated batch: the update is a copy
        for (int i = i0; i < i1; ++i)
#pragma unroll
            for (int h = 0; h < 4; ++h)
                if (core[h]) { const int64_t c = V.tidx(i - lofs, j, k0 + h); Tout[c] = Tin[c]; }
        return;
    }
    // planes that exist at level s: [lo(s), hi(s)], the plane group widened by S - s and cut at the lattice
    auto lo = [&](int s) { return max(i0 - (S - s), 0); };
    auto hi = [&](int s) { return min(i1 - 1 + (S - s), L - 1); };
    auto load = [&](int i, double (&dst)[4]) {
#pragma unroll
        for (int h = 0; h < 4; ++h) dst[h] = 0.0;
        if (i <= hi(0)) {
#pragma unroll
            for (int h = 0; h < 4; ++h)
                if (in[h]) dst[h] = Tin[V.tidx(i - lofs, j, k0 + h)];
        }
    };
    double prv[S][4], cur[S][4], inp[4];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int h = 0; h < 4; ++h) prv[s][h] = cur[s][h] = 0.0;
    load(lo(0), inp);
    const double dta = C.dt * C.alpha;
#pragma unroll 1
    for (int t = lo(0); t <= i1 - 1 + S; ++t) {
        double nv[4];                           // level s - 1, plane t - s + 1: the plane above the one level s computes
#pragma unroll
        for (int h = 0; h < 4; ++h) nv[h] = inp[h];
#pragma unroll
        for (int s = 1; s <= S; ++s) {
            const int x = t - s;                // cur[s - 1] and lds[s - 1] hold plane x of level s - 1, prv[s - 1] plane x - 1
            double out[4] = {0.0, 0.0, 0.0, 0.0};
            if (x >= lo(s) && x <= hi(s) && jin) {
                const double* row = &lds[s - 1][r][c4];
                double jm[4], jp[4];
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    jm[h] = (r > 0) ? row[h - EK] : 0.0;
                    jp[h] = (r < EJ - 1) ? row[h + EK] : 0.0;
                }
                const double kl = (c4 > 0) ? row[-1] : 0.0, kr = (c4 + 4 < EK) ? row[4] : 0.0;
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const int k = k0 + h;
                    const double tc = cur[s - 1][h];
                    const double im = (x > 0) ? prv[s - 1][h] : tc, ip = (x < L - 1) ? nv[h] : tc;
                    const double a = (j > 0) ? jm[h] : tc, b = (j < L - 1) ? jp[h] : tc;
                    const double km = (k > 0) ? (h > 0 ? cur[s - 1][h > 0 ? h - 1 : 0] : kl) : tc;
                    const double kp = (k < L - 1) ? (h < 3 ? cur[s - 1][h < 3 ? h + 1 : 3] : kr) : tc;
                    const double d0 = tc * -2.0 + (im + ip);
                    const double d1 = tc * -2.0 + (a + b);
                    const double d2 = tc * -2.0 + (km + kp);
                    const double lap = ((d0 + d1) + d2) * C.inv_dx2;
                    double nt;
                    if constexpr (!LASER) {
                        nt = tc + dta * lap;
                    } else {
                        const double qv = (x == L - 1 && in[h]) ? q_top[(int64_t)j * L + k] : 0.0;
                        const double qterm = (qv != 0.0) ? qv / C.rho_cp : 0.0;
                        const double dTdt = C.alpha * lap + qterm + C.latent_coef * 0.0;      // no latent heat behind sub-step 1
                        nt = tc + C.dt * dTdt;
                    }
                    double v = nt < C.clip_lo ? C.clip_lo : nt;
                    v = v > C.clip_hi ? C.clip_hi : v;
                    out[h] = v;
                }
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) { prv[s - 1][h] = cur[s - 1][h]; cur[s - 1][h] = nv[h]; nv[h] = out[h]; }
        }
        const int xo = t - S;                   // nv: level S, plane t - S
        if (xo >= i0 && xo < i1) {
#pragma unroll
            for (int h = 0; h < 4; ++h)
                if (core[h]) Tout[V.tidx(xo - lofs, j, k0 + h)] = nv[h];
        }
        load(t + 1, inp);                       // in flight across the barriers (issued earlier it costs the S = 4 laser kernel a spill)
        __syncthreads();                        // every read of the planes in LDS is done
#pragma unroll
        for (int s = 0; s < S; ++s) {
            double* row = &lds[s][r][c4];
#pragma unroll
            for (int h = 0; h < 4; ++h) row[h] = cur[s][h];
        }
        __syncthreads();
    }
}

}  // namespace cetkmc
