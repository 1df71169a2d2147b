// keyed.hpp -- reduction of per-voxel vectors of 64-bit integers by a run-time key, shared by solid.hpp and origin.hpp.
//
// A record is W::NW int64 words; W says which words are a minimum (W::is_min) or a maximum (W::is_max), all others are sums.
// The scheme is the one of grain.hpp with 64-bit counters: a wave-leader loop over the distinct keys of a wave (butterfly over
// the lanes that hold the key), a direct-mapped slot table in LDS claimed with a compare-and-swap -- a key that finds its slot
// taken goes straight to global memory -- and once per block integer atomics (add / min / max) into the records, which the
// host initialises on the stream before the launch (keyed_neutral).  Integer arithmetic only: every order gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cetkmc {

constexpr long long KEYED_NONE_MIN = 0x7fffffffffffffffLL, KEYED_NONE_MAX = -1;
constexpr int KEYED_ROUNDS = 4;          // distinct keys of a wave joined by butterfly; the lanes left over go one by one

// word w of a record (+ / min / max)= x; the neutral element is skipped
template <class W>
__device__ __forceinline__ void keyed_word(long long* p, int w, long long x)
{
    if (W::is_min(w)) { if (x != KEYED_NONE_MIN) atomicMin(p, x); }
    else if (W::is_max(w)) { if (x != KEYED_NONE_MAX) atomicMax(p, x); }
    else if (x != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)x);
}
template <class W>
__device__ __forceinline__ long long keyed_join(int w, long long a, long long b)
{
    return W::is_min(w) ? (b < a ? b : a) : W::is_max(w) ? (b > a ? b : a) : (long long)((unsigned long long)a + (unsigned long long)b);
}
template <class W>
__device__ __forceinline__ long long keyed_neutral(int w) { return W::is_min(w) ? KEYED_NONE_MIN : W::is_max(w) ? KEYED_NONE_MAX : 0; }

// Key key (>= 1) of the lanes with `part` set gets their vectors c: record key - 1 of `out`, through the block's slot table
// (tag / tab, SLOTS entries) where the key owns or claims its slot.  Wave uniform: every lane of the wave calls it.
template <class W, int SLOTS>
__device__ __forceinline__ void keyed_reduce(bool part, int key, const long long (&c)[W::NW], unsigned* tag, long long* tab, long long* out, int lane)
{
    constexpr int NW = W::NW;
    auto put = [&](int kq, int w, long long x) {         // one word of key kq
        const unsigned old = atomicCAS(&tag[kq & (SLOTS - 1)], 0u, (unsigned)kq);
        long long* p = (old == 0u || old == (unsigned)kq) ? tab + (kq & (SLOTS - 1)) * NW + w : out + (int64_t)(kq - 1) * NW + w;
        keyed_word<W>(p, w, x);
    };
    unsigned long long todo = __ballot(part);
#pragma unroll 1
    for (int round = 0; todo != 0; ++round) {            // wave uniform
        if (round == KEYED_ROUNDS) {
            if ((todo >> lane) & 1ull) {
#pragma unroll
                for (int w = 0; w < NW; ++w) put(key, w, c[w]);
            }
            break;
        }
        const int lead = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const int kq = __builtin_amdgcn_readlane(key, lead);
        const bool mine = part && key == kq;
        const unsigned long long m = __ballot(mine);
        todo &= ~m;
        if (__popcll(m) == 1) {
            if (mine) {
#pragma unroll
                for (int w = 0; w < NW; ++w) put(key, w, c[w]);
            }
            continue;
        }
        long long sel = 0;                               // lane w < NW: word w joined over the lanes of kq
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            long long x = mine ? c[w] : keyed_neutral<W>(w);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) x = keyed_join<W>(w, x, __shfl_xor(x, d));
            if (lane == w) sel = x;
        }
        if (lane < NW) put(kq, lane, sel);
    }
}

// the block's slot tables: empty before the voxel pass, into the records behind it (every thread of the block, between barriers
// of the caller's)
template <class W, int SLOTS>
__device__ __forceinline__ void keyed_table_init(unsigned* tag, long long* tab, int tid, int nthreads)
{
    for (int q = tid; q < SLOTS; q += nthreads) tag[q] = 0;
    for (int q = tid; q < SLOTS * W::NW; q += nthreads) tab[q] = keyed_neutral<W>(q % W::NW);
}
template <class W, int SLOTS>
__device__ __forceinline__ void keyed_table_flush(const unsigned* tag, const long long* tab, long long* out, int tid, int nthreads)
{
    for (int q = tid; q < SLOTS * W::NW; q += nthreads) {
        const unsigned key = tag[q / W::NW];
        if (key != 0) keyed_word<W>(out + (int64_t)(key - 1) * W::NW + q % W::NW, q % W::NW, tab[q]);
    }
}

}  // namespace cetkmc
