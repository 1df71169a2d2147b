// origin.hpp -- origin map on the device (not in the reference).
//
// The map of a lattice (single slab) records, per voxel, HOW and WHEN it was last filled or left: one 64-bit word
// ((ordinal + 1) << 3) | code, 0 = no record (cetkmc_origin_*, include/cetkmc.h), and a running census [L][5] of the absorbed
// events per build plane.  Nothing here writes a lattice field, and no stepping kernel knows of the map: the stepping calls
// leave the chosen event of every step in a device log, which is folded into the map behind the call.
//
// k_origin_absorb: one thread per log record.  Records [g * group, (g + 1) * group) share the ordinal seq + g (Mode A:
// group 1; Mode B: the D boxes of a super-step, which never touch the same voxel).  "Later wins" is a maximum over the
// encoded words, so the result does not depend on the order of the records: one 64-bit atomic max per written voxel, one
// 64-bit atomic add per census entry.
//
// k_origin_profile: a stream over the word (8 B), the label of the last clustering (4 B) and the state byte of every voxel.
// A block owns ORIGIN_VPB consecutive voxels in row-major order.  Every counted voxel contributes one vector of twelve
// 64-bit integers in the word order of cetkmc_origin_rec (sums, two minima and a maximum) to the record of its plane and,
// with a label, to the record of its grain, through the keyed reduction of keyed.hpp, which solid.hpp shares.
#pragma once
#include "voxel.hpp"
#include "kernels.hpp"
#include "keyed.hpp"

namespace cetkmc {

struct OriginMap {
    unsigned long long* words;   // [L^3] row-major; 0 = no record
    long long* census;           // [L][5] dep, diff (left here), nuc, att, diff (arrived here)
};
struct OriginRun {               // one replica's share of a batched absorb
    long long seq;               // ordinal of its record 0
    long long n;                 // records to absorb (its executed steps)
};

constexpr int ORIGIN_DEP = 1, ORIGIN_NUC = 2, ORIGIN_ATT = 3, ORIGIN_HOP = 4, ORIGIN_LEFT = 5;
constexpr int ORIGIN_NV = 8, ORIGIN_VPB = 256 * ORIGIN_NV;     // chunks / voxels of a profile block
constexpr int ORIGIN_NW = 12;                                   // int64 words of a record
constexpr int ORIGIN_WSUM = 7, ORIGIN_WMIN = 8, ORIGIN_WMAX = 9, ORIGIN_WBIRTH = 10;
constexpr int ORIGIN_PSLOTS = 16, ORIGIN_GSLOTS = 128;
using OriginRec = struct ::cetkmc_origin_rec;
static_assert(sizeof(OriginRec) == ORIGIN_NW * 8, "cetkmc_origin_rec is 12 int64 words");
static_assert(offsetof(OriginRec, ord_sum) == ORIGIN_WSUM * 8 && offsetof(OriginRec, ord_min) == ORIGIN_WMIN * 8 &&
              offsetof(OriginRec, ord_max) == ORIGIN_WMAX * 8 && offsetof(OriginRec, birth) == ORIGIN_WBIRTH * 8, "word order of cetkmc_origin_rec");
// as in solid.hpp: a block of ORIGIN_VPB consecutive voxels spans at most 14 planes, so its plane slots never collide
static_assert(ORIGIN_VPB == 2048 && ORIGIN_PSLOTS >= 14, "plane slots of a profile block");

struct OriginWords {
    static constexpr int NW = ORIGIN_NW;
    __device__ static constexpr bool is_min(int w) { return w == ORIGIN_WMIN || w == ORIGIN_WBIRTH; }
    __device__ static constexpr bool is_max(int w) { return w == ORIGIN_WMAX; }
};

__device__ __forceinline__ unsigned long long origin_enc(long long ordinal, int code)
{
    return ((unsigned long long)(ordinal + 1) << 3) | (unsigned long long)code;
}

// one record with ordinal o into the map of an L^3 lattice.  Records that name no event (idle -1, null -2), a diffusion
// without a target and anything outside the lattice are skipped.
__device__ __forceinline__ void origin_absorb_record(const cetkmc_event& ev, long long o, int L, const OriginMap& M)
{
    const int t = ev.type;
    if (t < 0 || t > 3) return;
    const unsigned uL = (unsigned)L;
    const int pi = ev.pos[0], pj = ev.pos[1], pk = ev.pos[2];
    if ((unsigned)pi >= uL || (unsigned)pj >= uL || (unsigned)pk >= uL) return;
    const int64_t vp = ((int64_t)pi * L + pj) * L + pk;
    if (t == EV_DIFF) {
        const int ti = ev.target[0], tj = ev.target[1], tk = ev.target[2];
        if (ti < 0) return;
        if ((unsigned)ti >= uL || (unsigned)tj >= uL || (unsigned)tk >= uL) return;
        const int64_t vt = ((int64_t)ti * L + tj) * L + tk;
        atomicMax(M.words + vp, origin_enc(o, ORIGIN_LEFT));
        atomicMax(M.words + vt, origin_enc(o, ORIGIN_HOP));
        atomicAdd(reinterpret_cast<unsigned long long*>(M.census + 5 * pi + 1), 1ull);
        atomicAdd(reinterpret_cast<unsigned long long*>(M.census + 5 * ti + 4), 1ull);
        return;
    }
    const int code = t == EV_DEP ? ORIGIN_DEP : t == EV_NUC ? ORIGIN_NUC : ORIGIN_ATT;
    atomicMax(M.words + vp, origin_enc(o, code));
    atomicAdd(reinterpret_cast<unsigned long long*>(M.census + 5 * pi + t), 1ull);
}

// n records of `log` into the map M, record q with ordinal seq + q / group.  grid: x = blocks of 256 records, y = replica
// (variadic trailing EnsSel: the replica's log from its EnsRep, its map, seq and n from the device tables).
template <class... E>
__global__ __launch_bounds__(256) void k_origin_absorb(const cetkmc_event* __restrict__ log, long long n, long long group, long long seq, int L,
                                                       OriginMap M, const OriginMap* __restrict__ maps, const OriginRun* __restrict__ runs, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        log = ens_rep(blockIdx.y, ens...).log_event; M = maps[blockIdx.y];
        seq = runs[blockIdx.y].seq; n = runs[blockIdx.y].n;
    }
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    origin_absorb_record(log[q], seq + (group == 1 ? q : q / group), L, M);
}

// cetkmc_apply's one event: the record travels as a kernel argument
__global__ __launch_bounds__(64) void k_origin_absorb_one(cetkmc_event ev, long long seq, int L, OriginMap M)
{
    if (threadIdx.x == 0) origin_absorb_record(ev, seq, L, M);
}

// ---- profile ---------------------------------------------------------------------------------------------------------
// records := empty (sums 0, ord_min = birth = INT64_MAX, ord_max -1)
__global__ __launch_bounds__(256) void k_origin_rec_init(long long* rec, int64_t n_words)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_words; q += (int64_t)gridDim.x * blockDim.x)
        rec[q] = keyed_neutral<OriginWords>((int)(q % ORIGIN_NW));
}

// the vector of a counted voxel with word w at linear index lin: occupied (n_occ) and classified by its word, or -- an empty
// voxel of a plane whose last event was a diffusion away -- left
__device__ __forceinline__ void origin_vector(long long (&c)[ORIGIN_NW], unsigned long long w, unsigned lin, bool occupied)
{
#pragma unroll
    for (int q = 0; q < ORIGIN_NW; ++q) c[q] = keyed_neutral<OriginWords>(q);
    if (!occupied) { c[6] = 1; return; }
    const int code = (int)(w & 7ull);
    c[0] = 1;
    if (code >= ORIGIN_DEP && code <= ORIGIN_HOP) {
        const long long o = (long long)(w >> 3) - 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) c[1 + q] = code == q + 1 ? 1 : 0;
        c[ORIGIN_WSUM] = o; c[ORIGIN_WMIN] = o; c[ORIGIN_WMAX] = o;
        c[ORIGIN_WBIRTH] = (o << 27) | ((long long)code << 24) | (long long)lin;
    } else {
        c[5] = 1;
    }
}

// layers[i] and grains[id - 1] get the records of the map M over the lattice S.  grid: x = blocks of ORIGIN_VPB voxels,
// y = replica (variadic trailing EnsSel: view and map from the device tables, labels at r * stride, layers at r * L, the
// replica's grain records at entry offs[r] of the concatenated table, n = its cluster count).  labels == nullptr: no grain
// records.
template <class... E>
__global__ __launch_bounds__(256) void k_origin_profile(SlabView S, OriginMap M, const OriginMap* __restrict__ maps, const int* __restrict__ labels, int n,
                                                        long long* layers, long long* grains, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        S = ens_rep(blockIdx.y, ens...).view[0]; M = maps[blockIdx.y];
        layers += (int64_t)blockIdx.y * S.L * ORIGIN_NW;
        if (labels) {
            const long long* o = ens_offs(ens...);
            labels += (int64_t)blockIdx.y * ens_stride(ens...);
            grains += o[blockIdx.y] * ORIGIN_NW; n = (int)(o[blockIdx.y + 1] - o[blockIdx.y]);
        }
    }
    __shared__ unsigned ptag[ORIGIN_PSLOTS], gtag[ORIGIN_GSLOTS];
    __shared__ long long ptab[ORIGIN_PSLOTS * ORIGIN_NW], gtab[ORIGIN_GSLOTS * ORIGIN_NW];
    const unsigned L = (unsigned)S.L, LL = L * L, nvox = LL * L;          // L <= 256: L^3 <= 2^24
    const int tid = threadIdx.x, lane = tid & 63;
    keyed_table_init<OriginWords, ORIGIN_PSLOTS>(ptag, ptab, tid, 256);
    keyed_table_init<OriginWords, ORIGIN_GSLOTS>(gtag, gtab, tid, 256);
    __syncthreads();
    const unsigned v0 = blockIdx.x * (unsigned)ORIGIN_VPB;
#pragma unroll 1
    for (int it = 0; it < ORIGIN_NV; ++it) {
        if (v0 + it * 256 >= nvox) break;                 // block uniform
        const unsigned v = v0 + it * 256 + tid;
        const bool in = v < nvox;
        unsigned long long w = 0;
        int g = 0;
        bool occ = false;
        unsigned plane = 0;
        if (in) {
            const unsigned row = v / L, k = v - row * L;
            plane = row / L;
            const unsigned j = row - plane * L;
            w = M.words[v];
            occ = S.state[S.sidx((int)plane - (S.gi0 - 2), (int)j, (int)k)] != 0;
            if (labels) { g = labels[v]; if (g < 0 || g > n) g = 0; }
        }
        const bool left = in && !occ && (int)(w & 7ull) == ORIGIN_LEFT;
        const bool pl = occ || left;
        if (__ballot(pl || g > 0) == 0) continue;         // wave uniform: nothing to count among these 64 voxels
        long long c[ORIGIN_NW];
        if (__ballot(pl) != 0) {
            origin_vector(c, w, v, occ);
            keyed_reduce<OriginWords, ORIGIN_PSLOTS>(pl, pl ? (int)plane + 1 : 0, c, ptag, ptab, layers, lane);
        }
        if (__ballot(g > 0) != 0) {                       // a grain's voxel is classified by its word alone
            origin_vector(c, w, v, true);
            keyed_reduce<OriginWords, ORIGIN_GSLOTS>(g > 0, g, c, gtag, gtab, grains, lane);
        }
    }
    __syncthreads();
    keyed_table_flush<OriginWords, ORIGIN_PSLOTS>(ptag, ptab, layers, tid, 256);
    keyed_table_flush<OriginWords, ORIGIN_GSLOTS>(gtag, gtab, grains, tid, 256);
}

}  // namespace cetkmc
