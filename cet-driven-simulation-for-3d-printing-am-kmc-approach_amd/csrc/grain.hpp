// grain.hpp -- per-grain table on the device (not in the reference).
//
// One streaming pass over the label volume of the last clustering (cluster.hpp) and the state of a whole lattice (single
// slab): per grain id 1..n one record of 18 integer counters (cetkmc_grain_rec, include/cetkmc.h) -- voxels, first and
// second coordinate moments, species, and the contacts of its voxels along the clustering's own 14-offset stencil -- plus
// the stored angles of the grain's first voxel.  Nothing is written back to the lattice and the voxel pass has no floating
// point: every counter is an integer sum, so every accumulation order gives the same bits.
//
// k_grain_table: a block owns GRAIN_VPB consecutive voxels in row-major order (GRAIN_NV chunks of 256; a wave reads 64
// consecutive labels) and loads the 14 neighbour labels of its voxel directly: they lie in rows the same or neighbouring
// waves read anyway, so all but the first touch of a line is a cache hit, and a tile with a two-cell rim in three directions
// would stage more cells than it owns.  The label volume has no padding: a neighbour is loaded only when its coordinates
// are inside the lattice.
//
// The reduction is by label, with 1 .. L^3 destinations known only at run time, so contributions are combined on chip
// before anything leaves the block:
//   wave:   a leader loop over the distinct labels of the wave.  Per round the first pending lane's label is broadcast, the
//           lanes that hold it are summed with wave_sum_i (18 values; 64 * 1290^2 < 2^27 fits 32 bits) and lanes 0..17 add
//           one counter each.  A wave of one grain takes one round.  After GRAIN_ROUNDS rounds the lanes left add their own
//           values (a label held by one lane skips the sum, too).
//   block:  a direct-mapped table in LDS, slot = label % GRAIN_SLOTS, its tag claimed with an LDS compare-and-swap; 32-bit
//           counters (GRAIN_VPB * 1290^2 < 2^32).  A label that finds its slot taken by another goes straight to global.
//   global: once per block, the non-zero counters of the claimed slots with returnless 64-bit integer atomic adds into the
//           records, which the host zeroes on the stream before the launch.
// k_grain_first: one thread per grain copies theta and phi of the grain's first voxel (roots[id - 1]) bit for bit.
#pragma once
#include "voxel.hpp"
#include "kernels.hpp"

namespace cetkmc {

constexpr int GRAIN_NV = 8, GRAIN_VPB = 256 * GRAIN_NV;     // chunks / voxels of a block
constexpr int GRAIN_NC = 18, GRAIN_NW = 20;                 // counters / int64 words of a record
constexpr int GRAIN_SLOTS = 128, GRAIN_ROUNDS = 4;
using GrainRec = struct ::cetkmc_grain_rec;
static_assert(sizeof(GrainRec) == GRAIN_NW * 8, "cetkmc_grain_rec is 20 int64 words");
static_assert((GRAIN_SLOTS & (GRAIN_SLOTS - 1)) == 0, "the slot is the label's low bits");

// true when label g owns (or now claims) its slot of the block's table
__device__ __forceinline__ bool grain_claim(unsigned* tag, int g)
{
    const unsigned old = atomicCAS(&tag[g & (GRAIN_SLOTS - 1)], 0u, (unsigned)g);
    return old == 0u || old == (unsigned)g;
}
// counter c of grain g += v: into the block's table, or past it into the grain's record
__device__ __forceinline__ void grain_add(bool in_lds, unsigned* tab, unsigned long long* out, int g, int c, int v)
{
    if (v == 0) return;
    if (in_lds) atomicAdd(&tab[(g & (GRAIN_SLOTS - 1)) * GRAIN_NC + c], (unsigned)v);
    else atomicAdd(out + (int64_t)(g - 1) * GRAIN_NW + c, (unsigned long long)v);
}

// out[(id - 1) * 20 + c] += the block's sum of counter c over its voxels of grain id (1..n).  grid: x = voxel chunk,
// y = replica (variadic trailing EnsSel, as in layer.hpp: labels at r * stride, the replica's records at entry offs[r] of
// the concatenated table, n = its cluster count).
template <class... E>
__global__ __launch_bounds__(256) void k_grain_table(SlabView S, const int* __restrict__ labels, int n, unsigned long long* out, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        const long long* o = ens_offs(ens...);
        S = ens_rep(blockIdx.y, ens...).view[0];
        labels += (int64_t)blockIdx.y * ens_stride(ens...);
        out += o[blockIdx.y] * GRAIN_NW; n = (int)(o[blockIdx.y + 1] - o[blockIdx.y]);
    }
    __shared__ unsigned tag[GRAIN_SLOTS];
    __shared__ unsigned tab[GRAIN_SLOTS * GRAIN_NC];
    const int L = S.L;
    const int64_t nvox = (int64_t)L * L * L;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int q = tid; q < GRAIN_SLOTS; q += 256) tag[q] = 0;
    for (int q = tid; q < GRAIN_SLOTS * GRAIN_NC; q += 256) tab[q] = 0;
    __syncthreads();
    const int64_t v0 = (int64_t)blockIdx.x * GRAIN_VPB;
#pragma unroll 1
    for (int it = 0; it < GRAIN_NV; ++it) {
        const int64_t v = v0 + it * 256 + tid;
        if (v0 + it * 256 >= nvox) break;                // block uniform
        int g = 0, val[GRAIN_NC];
#pragma unroll
        for (int c = 0; c < GRAIN_NC; ++c) val[c] = 0;
        if (v < nvox) g = labels[v];
        const bool occ = g > 0 && g <= n;                 // (labels are 0..n: the clustering made them or the import checked them)
        if (occ) {
            const int k = (int)(v % L), j = (int)((v / L) % L), i = (int)(v / ((int64_t)L * L));
            const int st = S.state[S.sidx(i - (S.gi0 - 2), j, k)];
            val[0] = 1; val[1] = i; val[2] = j; val[3] = k;
            val[4] = i * i; val[5] = j * j; val[6] = k * k; val[7] = i * j; val[8] = i * k; val[9] = j * k;
#pragma unroll
            for (int t = 1; t <= 4; ++t) val[9 + t] = st == t;
#pragma unroll
            for (int m = 0; m < 14; ++m) {
                const int ni = i + nbi_rt(m), nj = j + nbj_rt(m), nk = k + nbk_rt(m);
                if (ni < 0 || ni >= L || nj < 0 || nj >= L || nk < 0 || nk >= L) { val[17] += 1; continue; }
                const int gu = labels[((int64_t)ni * L + nj) * L + nk];
                if (gu == 0) val[16] += 1;
                else if (gu == g) val[14] += 1;
                else val[15] += 1;
            }
        }
        unsigned long long todo = __ballot(occ);
#pragma unroll 1
        for (int round = 0; todo != 0; ++round) {        // wave uniform
            if (round == GRAIN_ROUNDS) {
                if ((todo >> lane) & 1ull) {
                    const bool in_lds = grain_claim(tag, g);
#pragma unroll
                    for (int c = 0; c < GRAIN_NC; ++c) grain_add(in_lds, tab, out, g, c, val[c]);
                }
                break;
            }
            const int lead = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
            const int lbl = __builtin_amdgcn_readlane(g, lead);
            const bool mine = occ && g == lbl;
            const unsigned long long m = __ballot(mine);
            todo &= ~m;
            if (__popcll(m) == 1) {
                if (mine) {
                    const bool in_lds = grain_claim(tag, g);
#pragma unroll
                    for (int c = 0; c < GRAIN_NC; ++c) grain_add(in_lds, tab, out, g, c, val[c]);
                }
                continue;
            }
            int sel = 0;                                  // lane c < 18: the wave's sum of counter c over the lanes of lbl
#pragma unroll
            for (int c = 0; c < GRAIN_NC; ++c) {
                const int s = wave_sum_i(mine ? val[c] : 0);
                if (lane == c) sel = s;
            }
            if (lane < GRAIN_NC) grain_add(grain_claim(tag, lbl), tab, out, lbl, lane, sel);
        }
    }
    __syncthreads();
    for (int q = tid; q < GRAIN_SLOTS * GRAIN_NC; q += 256) {
        const unsigned g = tag[q / GRAIN_NC], s = tab[q];
        if (g != 0 && s != 0) atomicAdd(out + (int64_t)(g - 1) * GRAIN_NW + q % GRAIN_NC, (unsigned long long)s);
    }
}

// words 18 and 19 of record id - 1 = the bits of theta and phi at roots[id - 1], the linear index of grain id's first voxel
// (grid: x over the grains, y = replica; variadic trailing EnsSel as above, roots at r * stride)
template <class... E>
__global__ __launch_bounds__(256) void k_grain_first(SlabView S, const int* __restrict__ roots, int n, unsigned long long* out, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        const long long* o = ens_offs(ens...);
        S = ens_rep(blockIdx.y, ens...).view[0];
        roots += (int64_t)blockIdx.y * ens_stride(ens...);
        out += o[blockIdx.y] * GRAIN_NW; n = (int)(o[blockIdx.y + 1] - o[blockIdx.y]);
    }
    const int L = S.L;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        const int r = roots[q];
        const int64_t at = S.tidx(r / (L * L) - (S.gi0 - 2), (r / L) % L, r % L);
        out[(int64_t)q * GRAIN_NW + GRAIN_NC] = reinterpret_cast<const unsigned long long*>(S.theta)[at];
        out[(int64_t)q * GRAIN_NW + GRAIN_NC + 1] = reinterpret_cast<const unsigned long long*>(S.phi)[at];
    }
}

}  // namespace cetkmc
