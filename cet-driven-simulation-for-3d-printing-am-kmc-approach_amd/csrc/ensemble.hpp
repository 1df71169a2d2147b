// ensemble.hpp -- replica ensembles: R independent lattices of the same L stepped by the same launches.
//
// Every kernel of a Mode A step at L <= 128 (k_batch_reset, k_thermal_march, k_rate_table, k_interface, k_sweep_plane,
// k_select_apply) has an instantiation with a trailing EnsSel argument (kernels.hpp); k_clear_row_flags has its twin here.  It takes the replica index from a
// grid dimension the single-lattice kernel leaves free and reads everything that belongs to one lattice -- its slab view of
// either temperature buffer, rate constants, step state, block sums, random streams and logs -- from the replica's EnsRep.
// Replicas never interact: each keeps the trajectory a single handle would have produced.
#pragma once
#include "kernels.hpp"

namespace cetkmc {

struct EnsRep {
    KParams kp;                 // rate constants (replicas differ in impurity_c / nu_dep only: the rest is shared, kernels.hpp)
    SlabView view[2];           // [rel]: rel 0 = the T / rate-table buffer pair current at the start of the call
    StreamArgs sa[2];           // the sweep's arguments of view[rel]
    BatchCfg cfg;               // seed, defect_fraction, np_cap of this replica; step0 / rng_mode shared
    uint8_t* prev;
    StepState* ss;
    BlockEnt* blocks;
    const double* ktab;
    cetkmc_event* my_event;
    const double* u_pick;       // this replica's rows of the call's input / log arrays
    const double* u_defect;
    const double* u_np;
    double* log_total;
    cetkmc_event* log_event;
    int64_t* log_nev;
    int active;                 // 0: terminated in an earlier call -- the batch reset keeps it terminated (frozen)
    const double* q;            // thermal_mode 2: the replica's set of source planes [updates of the call][L*L] (shared by the
                                // replicas of one scan); null in the other modes, where no kernel reads a plane
};

struct EnsSel {
    const EnsRep* reps;         // device table, one entry per replica
    int rel;                    // which buffer pair is current (flips with every temperature update of the call)
    int nz;                     // k_thermal_march: plane groups per replica (the replica is folded into blockIdx.z)
    int64_t stride;             // analysis kernels (cluster.hpp): entries per replica of the label / parent arrays (L^3)
    const long long* offs;      // analysis kernels: per-replica offsets into a concatenated array (cluster stats, scatter list)
    int64_t q_off;              // k_thermal_march, laser mode: offset of the current update's plane in every plane set (u * L*L)
};

// end of a call: every replica's step state and interface-list length into contiguous arrays (one copy to the host)
__global__ void k_ens_collect(const EnsRep* __restrict__ reps, int R, StepState* ss_out, int* ifc_n_out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) {
        ss_out[r] = *reps[r].ss;
        ifc_n_out[r] = *reps[r].view[0].ifc_n;
    }
}

// k_clear_row_flags of every replica (y) behind a latent-heat temperature update: prev_state equals state again.  Not in a
// replica that has terminated or is frozen -- its update was a pass-through that left prev_state and the flags alone.
__global__ void k_ens_clear_row_flags(const EnsRep* __restrict__ reps)
{
    const EnsRep& e = reps[blockIdx.y];
    if (e.ss->status) return;
    const SlabView& S = e.view[0];
    const int64_t n = (int64_t)(S.nloc + 4) * S.L;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) S.row_chg[q] = 0;
}

// Cluster numbering of every replica without a host sort: a component's root is its first voxel in row-major order
// (cluster.hpp), so its 1-based id is 1 + the number of roots before it.  One 1024-thread block per replica scans the
// flattened parent array: cid[root] = id, roots[id - 1] = root (ascending), n_roots[r] = the replica's cluster count.
__global__ __launch_bounds__(1024) void k_ens_cc_rank(const int* __restrict__ parent, int* cid, int* roots, int* n_roots, int64_t n)
{
    __shared__ int wsum[16];
    __shared__ int base;
    const int64_t o = (int64_t)blockIdx.x * n;
    parent += o; cid += o; roots += o;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < n; c0 += 1024) {
        const int64_t v = c0 + threadIdx.x;
        const bool f = v < n && parent[v] == (int)v;
        const unsigned long long b = __ballot(f);
        const int pre = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(b);
        __syncthreads();
        int off = base;
        for (int q = 0; q < w; ++q) off += wsum[q];
        if (f) { cid[v] = off + pre + 1; roots[off + pre] = (int)v; }
        __syncthreads();
        if (threadIdx.x == 0) { int t = 0; for (int q = 0; q < 16; ++q) t += wsum[q]; base += t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) n_roots[blockIdx.x] = base;
}

// defects := 0 in every replica whose scatter list is given (offs[2r] >= 0) -- the memset of cetkmc_set_defects_sparse
__global__ void k_ens_clear_defects(const EnsRep* __restrict__ reps, const long long* __restrict__ offs)
{
    if (offs[2 * blockIdx.y] < 0) return;
    const SlabView& S = reps[blockIdx.y].view[0];
    const int64_t nS = (int64_t)(S.nloc + 4) * S.RJ * S.pitchS;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nS; q += (int64_t)gridDim.x * blockDim.x) S.defects[q] = 0;
}

}  // namespace cetkmc
