// solid.hpp -- solidification map on the device (not in the reference).
//
// The map of a lattice (single slab) records, per voxel, the thermal conditions at the moment the voxel solidified: a stamp,
// the voxel's T, the three gradient components of front.hpp and a cooling rate against a private snapshot of T
// (cetkmc_solid_*, include/cetkmc.h).  Nothing here writes a lattice field.
//
// k_solid_update: a stream over state and T of the lattice and the two snapshots.  The index space is the T layout of the
// owned planes, [L][L][pitchT], which the snapshots share: a thread owns SOLID_UP pairs of neighbouring k (k even), i.e. one
// 16-byte load of T, one 16-byte store of T_snap and a 2-byte load of state and of its snapshot per pair (rows of T are
// 64-byte multiples and k = 0 of a state row sits at the even offset KOFF, so both are aligned).  Transitions are rare (at
// most 20 voxels per Mode A update): only the rare branches read T_snap, gather the six T neighbours from global memory --
// inside the lattice only, as front.hpp does: T has no j / k padding and its halo planes hold no data -- and touch the
// dense map arrays; the snapshot byte is stored only where it differs.  The three counts go through wave ballots and one
// integer atomic per wave and counter.
//
// k_solid_profile: a stream over the dense map and the label volume of the last clustering.  A block owns SOLID_VPB
// consecutive voxels in row-major order.  Every recorded voxel contributes one vector of ten 64-bit integers in the word
// order of cetkmc_solid_rec (sums, a minimum and a maximum) to the record of its plane and, with a label, to the record of
// its grain.  Both reductions are by a run-time key and use the scheme of grain.hpp with 64-bit counters (keyed.hpp, shared
// with origin.hpp): a wave-leader loop
// over the distinct keys of a wave (butterfly over the lanes that hold the key), a direct-mapped slot table in LDS claimed
// with a compare-and-swap, and once per block integer atomics (add / min / max) into the records, which the host initialises
// on the stream before the launch.  Integer arithmetic only behind the quantisation: every order gives the same bits.
#pragma once
#include "voxel.hpp"
#include "kernels.hpp"
#include "keyed.hpp"

namespace cetkmc {

struct SolidMap {
    long long* stamp;            // [L^3] row-major; -1 = no record
    double* Ts;                  // [L^3]
    double* g;                   // [L^3][3]
    double* cool;                // [L^3]
    uint8_t* snap;               // [L][L][pitchT] state at the last update (the k padding is never read)
    double* Tsnap;               // [L][L][pitchT] T at the last update
    unsigned long long* cnt;     // [3] n_new, n_cleared, cleared voxels that had a record -- of the running update
};

constexpr int SOLID_UP = 4, SOLID_PPB = 256 * SOLID_UP;     // pairs per thread / per block of the update
constexpr int SOLID_NV = 8, SOLID_VPB = 256 * SOLID_NV;     // chunks / voxels of a profile block
constexpr int SOLID_NW = 10;                                // int64 words of a record
constexpr int SOLID_WMIN = 4, SOLID_WMAX = 5;               // the words that are a minimum / a maximum; all others are sums
constexpr int SOLID_PSLOTS = 16, SOLID_GSLOTS = 128;
constexpr long long SOLID_NONE_MIN = KEYED_NONE_MIN, SOLID_NONE_MAX = KEYED_NONE_MAX;
using SolidRec = struct ::cetkmc_solid_rec;
static_assert(sizeof(SolidRec) == SOLID_NW * 8, "cetkmc_solid_rec is 10 int64 words");
static_assert(offsetof(SolidRec, stamp_min) == SOLID_WMIN * 8 && offsetof(SolidRec, stamp_max) == SOLID_WMAX * 8, "word order of cetkmc_solid_rec");
// a block of SOLID_VPB consecutive voxels spans at most (SOLID_VPB - 1) / L^2 + 2 <= 14 planes and never more than L
// (L <= 12: L planes; L >= 13: 2047 / 169 + 2): the plane slots of a block never collide
static_assert(SOLID_VPB == 2048 && SOLID_PSLOTS >= 14, "plane slots of a profile block");

// snapshot := state, T_snap := T (cetkmc_solid_begin).  grid: x = pairs, y = replica (variadic trailing EnsSel)
template <class... E>
__global__ __launch_bounds__(256) void k_solid_snapshot(SlabView S, SolidMap M, const SolidMap* __restrict__ maps, E... ens)
{
    if constexpr (sizeof...(E) > 0) { S = ens_rep(blockIdx.y, ens...).view[0]; M = maps[blockIdx.y]; }
    const int L = S.L, half = S.pitchT >> 1;
    const int64_t npair = (int64_t)L * L * half;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npair) return;
    const int64_t row = p / half;
    const int k = 2 * (int)(p % half);
    if (k >= L) return;
    const int i = (int)(row / L), j = (int)(row % L), li = i - (S.gi0 - 2);
    const double2 t = *reinterpret_cast<const double2*>(S.T + S.tidx(li, j, k));
    const unsigned short s = *reinterpret_cast<const unsigned short*>(S.state + S.sidx(li, j, k));
    *reinterpret_cast<double2*>(M.Tsnap + row * S.pitchT + k) = t;
    *reinterpret_cast<unsigned short*>(M.snap + row * S.pitchT + k) = s;
}

// the record of voxel (i, j, k), own temperature Tc, that solidified since the last update
__device__ __forceinline__ void solid_record(const SlabView& S, const SolidMap& M, int i, int j, int k, double Tc, double T_old,
                                             long long stamp, double inv_dx, double dt)
{
    const int L = S.L, li = i - (S.gi0 - 2);
    const double half_inv_dx = 0.5 * inv_dx;
    double gi, gj, gk;
    if (L == 1) { gi = gj = gk = 0.0; }
    else {       // neighbours inside the lattice only
        const double* T = S.T;
        gi = (i == 0) ? (T[S.tidx(li + 1, j, k)] - Tc) * inv_dx : (i == L - 1) ? (Tc - T[S.tidx(li - 1, j, k)]) * inv_dx
                      : (T[S.tidx(li + 1, j, k)] - T[S.tidx(li - 1, j, k)]) * half_inv_dx;
        gj = (j == 0) ? (T[S.tidx(li, j + 1, k)] - Tc) * inv_dx : (j == L - 1) ? (Tc - T[S.tidx(li, j - 1, k)]) * inv_dx
                      : (T[S.tidx(li, j + 1, k)] - T[S.tidx(li, j - 1, k)]) * half_inv_dx;
        gk = (k == 0) ? (T[S.tidx(li, j, k + 1)] - Tc) * inv_dx : (k == L - 1) ? (Tc - T[S.tidx(li, j, k - 1)]) * inv_dx
                      : (T[S.tidx(li, j, k + 1)] - T[S.tidx(li, j, k - 1)]) * half_inv_dx;
    }
    const int64_t v = ((int64_t)i * L + j) * L + k;
    M.stamp[v] = stamp;
    M.Ts[v] = Tc;
    M.g[3 * v] = gi; M.g[3 * v + 1] = gj; M.g[3 * v + 2] = gk;
    M.cool[v] = (Tc - T_old) / dt;
}

// One update of the map (cetkmc_solid_update).  grid: x = blocks of SOLID_PPB pairs, y = replica (variadic trailing EnsSel:
// the replica's view and map from the device tables).
template <class... E>
__global__ __launch_bounds__(256) void k_solid_update(SlabView S, SolidMap M, const SolidMap* __restrict__ maps, long long stamp,
                                                      double inv_dx, double dt, E... ens)
{
    if constexpr (sizeof...(E) > 0) { S = ens_rep(blockIdx.y, ens...).view[0]; M = maps[blockIdx.y]; }
    const int L = S.L, pitchT = S.pitchT, half = pitchT >> 1;
    const int64_t npair = (int64_t)L * L * half;
    const int64_t p0 = (int64_t)blockIdx.x * SOLID_PPB + threadIdx.x;
    double2 t[SOLID_UP];
    unsigned s1[SOLID_UP], s0[SOLID_UP];
    int64_t row[SOLID_UP];
    int kk[SOLID_UP];
    bool on[SOLID_UP];
#pragma unroll
    for (int u = 0; u < SOLID_UP; ++u) {
        const int64_t p = p0 + u * 256;
        row[u] = p / half; kk[u] = 2 * (int)(p % half);
        on[u] = p < npair && kk[u] < L;
        t[u] = make_double2(0.0, 0.0); s1[u] = s0[u] = 0;
        if (on[u]) {
            const int i = (int)(row[u] / L), j = (int)(row[u] % L), li = i - (S.gi0 - 2);
            t[u] = *reinterpret_cast<const double2*>(S.T + S.tidx(li, j, kk[u]));
            s1[u] = *reinterpret_cast<const unsigned short*>(S.state + S.sidx(li, j, kk[u]));
            s0[u] = *reinterpret_cast<const unsigned short*>(M.snap + row[u] * pitchT + kk[u]);
        }
    }
    int n_new = 0, n_clr = 0, n_drop = 0;
#pragma unroll
    for (int u = 0; u < SOLID_UP; ++u) {
        const int64_t at = row[u] * pitchT + kk[u];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int k = kk[u] + e;
            const bool in = on[u] && k < L;
            const unsigned a = (s0[u] >> (8 * e)) & 0xffu, b = (s1[u] >> (8 * e)) & 0xffu;
            const bool is_new = in && a == 0 && b != 0, is_clr = in && a != 0 && b == 0;
            bool dropped = false;
            if (is_new) {
                const int i = (int)(row[u] / L), j = (int)(row[u] % L);
                solid_record(S, M, i, j, k, e ? t[u].y : t[u].x, M.Tsnap[at + e], stamp, inv_dx, dt);
            } else if (is_clr) {
                const int64_t v = row[u] * L + k;
                dropped = M.stamp[v] >= 0;
                M.stamp[v] = -1;
                M.Ts[v] = 0.0; M.g[3 * v] = 0.0; M.g[3 * v + 1] = 0.0; M.g[3 * v + 2] = 0.0; M.cool[v] = 0.0;
            }
            if (in && a != b) M.snap[at + e] = (uint8_t)b;
            n_new += __popcll(__ballot(is_new)); n_clr += __popcll(__ballot(is_clr)); n_drop += __popcll(__ballot(dropped));
        }
        if (on[u]) *reinterpret_cast<double2*>(M.Tsnap + at) = t[u];
    }
    if ((threadIdx.x & 63) == 0) {       // the wave's counts (every lane holds them)
        if (n_new) atomicAdd(M.cnt, (unsigned long long)n_new);
        if (n_clr) atomicAdd(M.cnt + 1, (unsigned long long)n_clr);
        if (n_drop) atomicAdd(M.cnt + 2, (unsigned long long)n_drop);
    }
}

// ---- profile ---------------------------------------------------------------------------------------------------------
// records := empty (sums 0, stamp_min INT64_MAX, stamp_max -1)
__global__ __launch_bounds__(256) void k_solid_rec_init(long long* rec, int64_t n_words)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_words; q += (int64_t)gridDim.x * blockDim.x) {
        const int w = (int)(q % SOLID_NW);
        rec[q] = w == SOLID_WMIN ? SOLID_NONE_MIN : w == SOLID_WMAX ? SOLID_NONE_MAX : 0;
    }
}

// the record's words for the shared keyed reduction (keyed.hpp): sums but for one minimum and one maximum
struct SolidWords {
    static constexpr int NW = SOLID_NW;
    __device__ static constexpr bool is_min(int w) { return w == SOLID_WMIN; }
    __device__ static constexpr bool is_max(int w) { return w == SOLID_WMAX; }
};

// layers[i] and grains[id - 1] get the records of the map M.  grid: x = blocks of SOLID_VPB voxels, y = replica (variadic
// trailing EnsSel: map from the device table, labels at r * stride, layers at r * L, the replica's grain records at entry
// offs[r] of the concatenated table, n = its cluster count).  labels == nullptr: no grain records.
template <class... E>
__global__ __launch_bounds__(256) void k_solid_profile(SolidMap M, const SolidMap* __restrict__ maps, int L, const int* __restrict__ labels, int n,
                                                       double q0, double q1, double q2, double q3, long long* layers, long long* grains, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        M = maps[blockIdx.y];
        layers += (int64_t)blockIdx.y * L * SOLID_NW;
        if (labels) {
            const long long* o = ens_offs(ens...);
            labels += (int64_t)blockIdx.y * ens_stride(ens...);
            grains += o[blockIdx.y] * SOLID_NW; n = (int)(o[blockIdx.y + 1] - o[blockIdx.y]);
        }
    }
    __shared__ unsigned ptag[SOLID_PSLOTS], gtag[SOLID_GSLOTS];
    __shared__ long long ptab[SOLID_PSLOTS * SOLID_NW], gtab[SOLID_GSLOTS * SOLID_NW];
    const int64_t nvox = (int64_t)L * L * L, LL = (int64_t)L * L;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int q = tid; q < SOLID_PSLOTS; q += 256) ptag[q] = 0;
    for (int q = tid; q < SOLID_GSLOTS; q += 256) gtag[q] = 0;
    for (int q = tid; q < SOLID_PSLOTS * SOLID_NW; q += 256) ptab[q] = keyed_neutral<SolidWords>(q % SOLID_NW);
    for (int q = tid; q < SOLID_GSLOTS * SOLID_NW; q += 256) gtab[q] = keyed_neutral<SolidWords>(q % SOLID_NW);
    __syncthreads();
    const double lim = 274877906944.0;                    // 2^38
    const int64_t v0 = (int64_t)blockIdx.x * SOLID_VPB;
#pragma unroll 1
    for (int it = 0; it < SOLID_NV; ++it) {
        if (v0 + it * 256 >= nvox) break;                 // block uniform
        const int64_t v = v0 + it * 256 + tid;
        const long long st = v < nvox ? M.stamp[v] : -1;
        const bool rec = st >= 0;
        if (__ballot(rec) == 0) continue;                 // wave uniform: nothing recorded among these 64 voxels
        long long c[SOLID_NW];
#pragma unroll
        for (int w = 0; w < SOLID_NW; ++w) c[w] = keyed_neutral<SolidWords>(w);
        int g = 0;
        if (rec) {
            const double gi = M.g[3 * v], gj = M.g[3 * v + 1], gk = M.g[3 * v + 2], cool = M.cool[v], Ts = M.Ts[v];
            const double G = sqrt(gi * gi + gj * gj + gk * gk);
            const double x0 = G * q0, x1 = gi * q1, x2 = cool * q2, x3 = Ts * q3;
            const bool good = finite_d(G) && finite_d(gi) && finite_d(cool) && finite_d(Ts) &&
                              fabs(x0) < lim && fabs(x1) < lim && fabs(x2) < lim && fabs(x3) < lim;
            if (good) {
                c[0] = 1; c[2] = cool < 0.0 ? 1 : 0; c[3] = st; c[SOLID_WMIN] = st; c[SOLID_WMAX] = st;
                c[6] = llrint(x0); c[7] = llrint(x1); c[8] = llrint(x2); c[9] = llrint(x3);
            } else {
                c[1] = 1;
            }
            if (labels) { g = labels[v]; if (g < 0 || g > n) g = 0; }
        }
        keyed_reduce<SolidWords, SOLID_PSLOTS>(rec, rec ? (int)(v / LL) + 1 : 0, c, ptag, ptab, layers, lane);
        if (labels && __ballot(g > 0) != 0) keyed_reduce<SolidWords, SOLID_GSLOTS>(g > 0, g, c, gtag, gtab, grains, lane);
    }
    __syncthreads();
    for (int q = tid; q < SOLID_PSLOTS * SOLID_NW; q += 256) {
        const unsigned key = ptag[q / SOLID_NW];
        if (key != 0) keyed_word<SolidWords>(layers + (int64_t)(key - 1) * SOLID_NW + q % SOLID_NW, q % SOLID_NW, ptab[q]);
    }
    for (int q = tid; q < SOLID_GSLOTS * SOLID_NW; q += 256) {
        const unsigned key = gtag[q / SOLID_NW];
        if (key != 0) keyed_word<SolidWords>(grains + (int64_t)(key - 1) * SOLID_NW + q % SOLID_NW, q % SOLID_NW, gtab[q]);
    }
}

}  // namespace cetkmc
