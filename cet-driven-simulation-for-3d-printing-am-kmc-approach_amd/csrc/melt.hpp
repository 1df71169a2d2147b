// melt.hpp -- remelting on the device (not in the reference).
//
// One pass turns every occupied voxel at or above a threshold temperature into an empty one:
//   m = (state != 0) & (T >= threshold)       NaN never melts, +inf does, equality melts, a state-4 voxel melts like an atom
//   on m: state = 0, prev_state = 0, theta = phi = 0.0 (unit vector (0, 0, 1)); nothing else changes, no heat is absorbed.
// Three launches, each variadic in a trailing EnsSel (grid y = replica) like solid.hpp, each a pass-through behind an early
// stop of the batch (status != 0), as the temperature kernels are:
//
// k_melt_scan   a stream over state and T of the owned planes: 9 B per voxel read.  The index space is the T layout
//               [nloc][L][pitchT]; a thread owns MELT_UP runs of four consecutive k: one 4-byte load of state (k = 0 of a state
//               row sits at byte KOFF = 4 of a 16-byte multiple) and two 16-byte loads of T per run.  Melting is rare, so only
//               the rare branch writes: write_site() -- the reference's own "site empties" write, which also flags the row for
//               the latent-heat test -- the prev_state byte, and one byte of the per-row flag array [(nloc + 4)][L].  The count
//               goes through wave ballots and one integer atomic per wave.
// k_melt_touch  one wave per 64 voxels of an owned row.  Row (lp, j) has work iff a row (lp + di, j + dj) with dirty_offset(di, dj)
//               is flagged: at most 11 byte reads, otherwise the wave leaves.  In a row with work every voxel is encoded (ifc_encode): an
//               interface voxel that is not listed gets its membership flag and is appended (one atomic per wave, as ifc_touch
//               does without dedupe), a listed voxel stores its new neighbourhood word.  Nothing is evaluated here: in the
//               stepping loop k_interface follows, behind the direct call the interface sums go stale (Cause::apply).  The list
//               is allocated for every owned voxel and appends happen only where the flag was clear, so it cannot overflow.
// k_melt_close  clears the row flags behind the touch and folds the pass's count into the running totals.
#pragma once
#include "voxel.hpp"
#include "kernels.hpp"

namespace cetkmc {

struct MeltState {
    uint8_t* flags;              // [(nloc + 4)][L]: 1 if a voxel of row (li, j) melted in the running pass; zero at rest
    unsigned long long* cnt;     // [MELT_NC]: the words of cetkmc_remelt_info, then the running pass's count
};
constexpr int MELT_NC = 5, MELT_PASSES = 0, MELT_TOTAL = 1, MELT_LAST = 2, MELT_APPENDED = 3, MELT_RUNNING = 4;
constexpr int MELT_UP = 4, MELT_QPB = 256 * MELT_UP;      // runs of four voxels per thread / per block of the scan

// grid: x = blocks of MELT_QPB runs, y = replica
template <class... E>
__global__ __launch_bounds__(256) void k_melt_scan(SlabView S, uint8_t* prev, MeltState M, const MeltState* __restrict__ tab, double threshold,
                                                   const StepState* __restrict__ ss, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        const auto& e = ens_rep(blockIdx.y, ens...);
        S = e.view[ens_rel(ens...)]; prev = e.prev; ss = e.ss; M = tab[blockIdx.y];
    }
    if (ss && ss->status) return;
    const int L = S.L, quads = S.pitchT >> 2;
    const int64_t nquad = (int64_t)S.nloc * L * quads;
    const int64_t q0 = (int64_t)blockIdx.x * MELT_QPB + threadIdx.x;
    double2 ta[MELT_UP], tb[MELT_UP];
    unsigned st[MELT_UP];
    int64_t row[MELT_UP];
    int kk[MELT_UP];
    bool on[MELT_UP];
#pragma unroll
    for (int u = 0; u < MELT_UP; ++u) {
        const int64_t q = q0 + u * 256;
        row[u] = q / quads; kk[u] = 4 * (int)(q % quads);
        on[u] = q < nquad && kk[u] < L;
        ta[u] = tb[u] = make_double2(0.0, 0.0); st[u] = 0;
        if (on[u]) {
            const int li = (int)(row[u] / L) + 2, j = (int)(row[u] % L);
            const double2* t = reinterpret_cast<const double2*>(S.T + S.tidx(li, j, kk[u]));
            ta[u] = t[0]; tb[u] = t[1];
            st[u] = *reinterpret_cast<const unsigned*>(S.state + S.sidx(li, j, kk[u]));
        }
    }
    int n = 0;
#pragma unroll
    for (int u = 0; u < MELT_UP; ++u) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = kk[u] + c;
            const unsigned s = (st[u] >> (8 * c)) & 0xffu;
            const double Tv = c == 0 ? ta[u].x : c == 1 ? ta[u].y : c == 2 ? tb[u].x : tb[u].y;
            const bool melt = on[u] && k < L && s != 0 && s != OOB && Tv >= threshold;
            if (melt) {
                const int lp = (int)(row[u] / L), j = (int)(row[u] % L);
                write_site(S, S.gi0 + lp, j, k, 0, 0.0, 0.0);
                prev[S.sidx(lp + 2, j, k)] = 0;
                M.flags[(int64_t)(lp + 2) * L + j] = 1;
            }
            n += __popcll(__ballot(melt));
        }
    }
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(M.cnt + MELT_RUNNING, (unsigned long long)n);      // the wave's count (every lane holds it)
}

// grid: x = blocks of four waves, a wave = 64 consecutive k of an owned row; y = replica.  (No loop over k around ifc_encode: with
// one, the compiler's register allocation of k_ifc_rebuild, k_select_apply and k_sweep_stream_apply -- which inline the same
// function -- came out different from the build without this file.)
template <class... E>
__global__ __launch_bounds__(256) void k_melt_touch(SlabView S, MeltState M, const MeltState* __restrict__ tab, const StepState* __restrict__ ss, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        const auto& e = ens_rep(blockIdx.y, ens...);
        S = e.view[ens_rel(ens...)]; ss = e.ss; M = tab[blockIdx.y];
    }
    if (ss && ss->status) return;
    const int L = S.L, lane = threadIdx.x & 63, nchunk = (L + 63) >> 6;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), r = w / nchunk;
    if (r >= (int64_t)S.nloc * L) return;
    const int lp = (int)(r / L), j = (int)(r % L), li = lp + 2;
    bool work = false;
#pragma unroll
    for (int di = -2; di <= 2; ++di)
#pragma unroll
        for (int dj = -2; dj <= 2; ++dj) {
            if (!dirty_offset(di, dj)) continue;
            const int a = li + di, b = j + dj;        // 0 <= a < nloc + 4 always; the halo planes' flags are never set
            if (b >= 0 && b < L) work |= M.flags[(int64_t)a * L + b] != 0;
        }
    if (!work) return;                                // wave uniform
    const int k = (int)(w % nchunk) * 64 + lane;
    const bool in = k < L;
    const int kc = in ? k : 0;                        // (a lane past the row's end encodes voxel 0 and drops the result)
    const int64_t t = S.tidx(li, j, kc);
    bool listed = S.ifc_in[t] != 0;
    bool hit;
    const unsigned code = ifc_encode(S, li, j, kc, &hit);
    const bool want = in && hit && !listed;
    const unsigned long long m = __ballot(want);
    if (m) {
        const int leader = __builtin_ctzll(m);
        int base = 0;
        if (lane == leader) {
            base = atomicAdd(S.ifc_n, __popcll(m));
            atomicAdd(M.cnt + MELT_APPENDED, (unsigned long long)__popcll(m));
        }
        base = __shfl(base, leader);
        if (want) {
            S.ifc_in[t] = 1; listed = true;
            S.ifc_list[base + __popcll(m & ((1ull << lane) - 1ull))] = ((unsigned)lp << 20) | ((unsigned)j << 10) | (unsigned)k;
        }
    }
    if (in && listed) S.ifc_code[t] = code;
}

// grid: x = blocks over the flag array, y = replica
template <class... E>
__global__ __launch_bounds__(256) void k_melt_close(SlabView S, MeltState M, const MeltState* __restrict__ tab, const StepState* __restrict__ ss, E... ens)
{
    if constexpr (sizeof...(E) > 0) {
        const auto& e = ens_rep(blockIdx.y, ens...);
        S = e.view[ens_rel(ens...)]; ss = e.ss; M = tab[blockIdx.y];
    }
    if (ss && ss->status) return;
    const int64_t n = (int64_t)(S.nloc + 4) * S.L;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) M.flags[q] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long c = M.cnt[MELT_RUNNING];
        M.cnt[MELT_PASSES] += 1; M.cnt[MELT_TOTAL] += c; M.cnt[MELT_LAST] = c; M.cnt[MELT_RUNNING] = 0;
    }
}

// end of an ensemble call: every replica's counters into one contiguous array (one copy to the host)
__global__ void k_melt_collect(const MeltState* __restrict__ tab, int R, unsigned long long* out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < R * 4) out[q] = tab[q >> 2].cnt[q & 3];
}

}  // namespace cetkmc
