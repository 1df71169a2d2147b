// local.hpp -- Mode B with a local event loop: several events per box and super-step, up to a common time horizon.
//
// NOT in the reference.  Definition: include/cetkmc.h (cetkmc_run_supersteps_local) and DESIGN.md section 23; comparator:
// tests/local_ref.py.  Box 8 only.  Per super-step the sweep, k_domain_pick8 (every box's first pick on the frozen
// lattice) and k_domain_rmax run as in superstep.hpp; k_domain_local then replaces k_domain_apply: one wave per box
// executes the box's events one after the other until the waiting times pass the horizon tau = horizon_events / R_max, the
// box has executed max_events events, or its window holds no event any more.
//
// Independence of the boxes: a voxel's rates read state, orientation and T within +-2 of it (eval_voxel), an event writes
// its voxel and a target within +-2 of it.  A window [w0, w0 + 3] is therefore evaluated from [w0 - 2, w0 + 5] and written
// within the same range, and the next active window along an axis starts at w0 + 8, reading from w0 + 6: no box reads or
// writes what another box writes, however many events each of them executes.
//
// Inside the loop the picks m >= 1 are made from the lattice fields themselves (state, T, orientation vectors, defects):
// every lane evaluates one voxel of the window with eval_voxel() -- the arithmetic and the slot order the rate table's
// entries are summed in -- so nothing derived (rate table, class-byte counts, interface flags, neighbourhood words) is
// read or repaired there.  The lattice writes go through apply_event() as k_domain_apply's do; the upkeep of everything
// touched stays k_domain_touch, after all lattice writes of the super-step, over the D * max_events records.
#pragma once
#include "superstep.hpp"

namespace cetkmc {

constexpr uint64_t KEY_WAIT = 7ull << 40;       // waiting-time uniform of event m of box d: KEY_WAIT | m << 24 | d
constexpr int LOCAL_NL = 256;                   // leaves of a 4 x 4 x 4 window's tree: 16 blocks (12 used) x 4 x 4
constexpr int LOCAL_CAPPED = 2;                 // counter slot entry beside {executed, nucleations}: boxes stopped by max_events

struct LocalCfg {
    int32_t max_events;        // 1..64
    double horizon_events;     // > 0, may be +inf
};

// The pick of a box from its window [i0, i0 + 4) x [j0, j0 + 4) x [k0, k0 + 4) on the lattice as it stands: lane = voxel
// (ii, jj, kk) = (lane >> 4, (lane >> 2) & 3, lane & 3) evaluates its events into the three category leaves, then the
// canonical window tree, descent and slot scan of k_domain_pick (window_heap_pick, slot_scan_wave).  Every lane returns
// the same pick.
__device__ __forceinline__ DomPick local_pick(const KParams& P, const SlabView& S, const double* __restrict__ ktab_g, int i0, int j0, int k0,
                                              double u, double* hs, uint8_t* hf, uint8_t* lc, int lane)
{
    for (int q = lane; q < LOCAL_NL; q += 64) { hs[LOCAL_NL + q] = 0.0; hf[LOCAL_NL + q] = 0; lc[q] = 0; }
    __builtin_amdgcn_wave_barrier();
    const int ii = lane >> 4, jj = (lane >> 2) & 3, kk = lane & 3;
    const int i = i0 + ii, j = j0 + jj, k = k0 + kk, li = i - S.gi0 + 2;
    double s_dep = 0.0, s_diff = 0.0, s_empty = 0.0;
    int n_dep = 0, n_diff = 0, n_empty = 0, scan = 0;
    eval_voxel(P, S, ktab_g, li, i, j, k, (int)S.state[S.sidx(li, j, k)], S.T[S.tidx(li, j, k)],
               [&](int m) { return (int)S.state[S.sidx(li + nbi_rt(m), j + nbj_rt(m), k + nbk_rt(m))]; },
               [&](int cat, int type, double rate, int, int) {
                   if (cat == CAT_DEP) { s_dep = s_dep + rate; ++n_dep; }
                   else if (cat == CAT_DIFF) { s_diff = s_diff + rate; ++n_diff; }
                   else { s_empty = s_empty + rate; ++n_empty; if (type == EV_ATT) scan = 1; }
               });
    // leaf code: event count | 128 where the leaf's one event need not be the nucleation (as a listed voxel's in k_domain_pick)
    const int q0 = (3 * ii * 4 + jj) * 4 + kk;
    if (n_dep) { hs[LOCAL_NL + q0] = s_dep; hf[LOCAL_NL + q0] = 1; lc[q0] = (uint8_t)n_dep; }
    if (n_diff) { hs[LOCAL_NL + q0 + 16 * CAT_DIFF] = s_diff; hf[LOCAL_NL + q0 + 16 * CAT_DIFF] = 1; lc[q0 + 16 * CAT_DIFF] = (uint8_t)n_diff; }
    if (n_empty) {
        hs[LOCAL_NL + q0 + 16 * CAT_EMPTY] = s_empty; hf[LOCAL_NL + q0 + 16 * CAT_EMPTY] = 1;
        lc[q0 + 16 * CAT_EMPTY] = (uint8_t)(n_empty | (scan << 7));
    }
    __builtin_amdgcn_wave_barrier();
    const WinPick wp = window_heap_pick(hs, hf, lc, 16, 4, u, lane);
    DomPick pk;
    pk.i = 0; pk.j = 0; pk.k = 0; pk.type = -1; pk.m = -1; pk.atom = 0; pk.rate = 0.0; pk.R = 0.0;
    if (wp.cat >= 0) {                                           // wave-uniform
        pk.i = i0 + wp.ii; pk.j = j0 + wp.jj; pk.k = k0 + wp.kk; pk.R = wp.R;
        if (wp.simple) {
            pk.type = (wp.cat == CAT_DEP) ? EV_DEP : EV_NUC;
            pk.atom = (wp.cat == CAT_DEP) ? 0 : 1;
            pk.rate = wp.leaf_rate;
        } else {
            const SlotPick sp = slot_scan_wave(P, S, ktab_g, pk.i - S.gi0 + 2, pk.j, pk.k, wp.cat, wp.base, wp.r, lane);
            pk.type = sp.type; pk.m = sp.m; pk.atom = sp.atom; pk.rate = sp.rate;
        }
    }
    __builtin_amdgcn_wave_barrier();                             // the next pick clears the leaves this one read
    return pk;
}

// One wave per box (single slab).  Lane 0 carries the serial part -- clock, record, uniforms, lattice write -- and the whole
// wave re-picks.  The first pick and R_max come from k_domain_pick8 / k_domain_rmax.  Records: dom_events[D][K] (read by
// k_domain_touch) and, if kept, log_events[n][D][K]; the slots a box does not use hold an idle box's record.
// (207 VGPRs, 2 waves per SIMD, no scratch.  Capping the registers for 3 or 4 waves -- amdgpu_waves_per_eu -- makes the
// compiler spill 200 / 308 bytes per lane to scratch: not done.)
__global__ __launch_bounds__(64) void k_domain_local(KParams P, const SlabView* __restrict__ slabs, int L, int D, SuperCfg C, LocalCfg LC,
                                                     const StepState* __restrict__ ss, const double* __restrict__ ktab_g,
                                                     const DomPick* __restrict__ picks, const double* __restrict__ rmax,
                                                     cetkmc_event* __restrict__ dom_events, unsigned long long* counters,
                                                     cetkmc_event* log_events)
{
    __shared__ __attribute__((aligned(16))) double hs[2 * LOCAL_NL];
    __shared__ uint8_t hf[2 * LOCAL_NL];
    __shared__ uint8_t lc[LOCAL_NL];
    const int lane = threadIdx.x;
    int dl = blockIdx.x;
    if ((gridDim.x & 7) == 0) dl = (dl & 7) * (int)(gridDim.x >> 3) + (dl >> 3);      // consecutive boxes on one XCD
    if (ss->status || dl >= D) return;
    const int d = C.d0 + dl;
    const SlabView& S = slabs[0];
    const int64_t cur = ss->cur;
    const int64_t g = C.step0 + cur;
    const int sec = (int)(g & 7);
    const int nb = C.nb;
    const int di = d / (nb * nb), dj = (d / nb) % nb, dk = d % nb;
    const int i0 = di * 8 + ((sec >> 2) & 1) * 4, j0 = dj * 8 + ((sec >> 1) & 1) * 4, k0 = dk * 8 + (sec & 1) * 4;
    const int K = LC.max_events;
    const double Rmax = rmax[0];
    const double tau = Rmax > 0.0 ? LC.horizon_events / Rmax : 0.0;
    cetkmc_event* const rec = dom_events + (size_t)dl * K;
    cetkmc_event* const lrec = log_events ? log_events + ((size_t)cur * D + dl) * K : nullptr;
    DomPick pk = picks[dl];
    double t = 0.0;
    int m = 0, n_nuc = 0, capped = 0;
    while (pk.type >= 0) {                                       // wave-uniform: every lane holds the same pick
        if (m == K) { capped = 1; break; }
        const uint64_t md = ((uint64_t)m << 24) | (uint64_t)d;
        const double u = counter_uniform(C.seed, (uint64_t)g, KEY_WAIT | md);
        const double w = u > 0.0 ? -log(u) / pk.R : __builtin_inf();
        if (t + w > tau) break;
        t += w;
        if (lane == 0) {
            const cetkmc_event ev = draw_event(P, slabs, 1, L, C.seed, g, md, (uint64_t)m << 44, pk, true);
            rec[m] = ev;
            if (lrec) lrec[m] = ev;
            const int mk = (C.defect_fraction > 0.0 && counter_uniform(C.seed, (uint64_t)g, KEY_DEFECT | md) < C.defect_fraction) ? 1 : 0;
            apply_event(slabs, 1, ev, mk);
        }
        n_nuc += pk.type == EV_NUC;
        ++m;
        if (m < K) {
            // lane 0's lattice writes before the wave's reads: writer and readers are lanes of ONE wave, so work-group scope
            // is enough (they share the CU's L1; a device-scope fence would also write the XCD's L2 back on every event)
            __threadfence_block();
            pk = local_pick(P, S, ktab_g, i0, j0, k0, counter_uniform(C.seed, (uint64_t)g, KEY_PICK | ((uint64_t)m << 24) | (uint64_t)d),
                            hs, hf, lc, lane);
        }
    }
    if (lane >= m && lane < K) {                                 // unused slots: an idle box's record
        DomPick idle;
        idle.i = 0; idle.j = 0; idle.k = 0; idle.type = -1; idle.m = -1; idle.atom = 0; idle.rate = 0.0; idle.R = 0.0;
        const cetkmc_event ev = draw_event(P, slabs, 1, L, C.seed, g, 0ull, 0ull, idle, true);
        rec[lane] = ev;
        if (lrec) lrec[lane] = ev;
    }
    if (lane == 0 && m > 0) {
        unsigned long long* slot = counters + (size_t)(blockIdx.x % SUPER_CNT_SLOTS) * SUPER_CNT_STRIDE;
        atomicAdd(&slot[0], (unsigned long long)m);
        if (n_nuc) atomicAdd(&slot[1], (unsigned long long)n_nuc);
        if (capped) atomicAdd(&slot[LOCAL_CAPPED], 1ull);
    }
}

// Before k_super_commit (which sums and clears {executed, nucleations}, clears R_max and advances the batch): the capped
// boxes and the horizon of the super-step into their logs.
__global__ __launch_bounds__(64) void k_local_commit(const StepState* __restrict__ ss, unsigned long long* counters,
                                                     const double* __restrict__ rmax, LocalCfg LC, double* __restrict__ log_horizon,
                                                     int64_t* __restrict__ log_capped)
{
    if (ss->status) return;
    const int lane = threadIdx.x;
    long long cp = 0;
    for (int q = lane; q < SUPER_CNT_SLOTS; q += 64) {
        unsigned long long* slot = counters + (size_t)q * SUPER_CNT_STRIDE;
        cp += (long long)slot[LOCAL_CAPPED];
        slot[LOCAL_CAPPED] = 0;
    }
#pragma unroll
    for (int l = 0; l < 6; ++l) cp += __shfl_xor(cp, 1 << l);
    if (lane != 0) return;
    const int64_t s = ss->cur;
    const double Rmax = rmax[0];
    log_capped[s] = cp;
    log_horizon[s] = Rmax > 0.0 ? LC.horizon_events / Rmax : 0.0;
}

}  // namespace cetkmc
