// shift.hpp -- the lattice moved on the device (cetkmc_shift; not in the reference).
//
// Voxel v of the old lattice moves to v + d; a voxel of the new lattice whose source v - d lies outside is exposed and takes a
// fill.  The move overlaps its own source in every direction, so no kernel here works in place: a gather kernel reads the old
// array and writes the shifted one into a spare of the same layout, and a second launch copies the spare back over the
// array -- the same kernel with d = 0 for the 64-bit arrays, k_shift_bytes_back for the byte arrays, which also writes what
// an upload of a state writes beside it (prev_state, the class bytes).  No pointer of the handle changes.
//
// Both gather kernels are destination centric: a lane owns 8 consecutive entries of a destination row, as the sweep does,
// loads its 8 sources (row s = (i - d0, j - d1), entries from k - d2 on, wherever that falls) and stores the run with vector
// stores where it is whole and aligned.  A source index is tested against the lattice before it is used: the 255 sentinels
// around the state rows and the halo planes are never read as data and never written.  No floating-point arithmetic: the
// f64 fields travel as 64-bit words (NaN payloads, -0.0).  The counts are integer atomics, once per block.
//
// Everything that belongs to one lattice -- its view, arrays, spares, move, fills and count record -- is a ShiftJob.  A single
// handle passes its job by value; an ensemble passes a device table of R jobs and every kernel takes its lattice from
// blockIdx.y, so the launch sequence does not depend on R.  A replica whose record has d = 0 is not active: its blocks return.
// The rest of an upload's sequence (row flags, interface flags, list, unit vectors) has its replica forms here as well.
#pragma once
#include "voxel.hpp"
#include "kernels.hpp"
#include "superstep.hpp"
#include "solid.hpp"

namespace cetkmc {

// the 64-bit arrays of a lattice, in the order of ShiftJob::arr
enum { SHIFT_THETA = 0, SHIFT_PHI, SHIFT_T, SHIFT_STAMP, SHIFT_TS, SHIFT_G, SHIFT_COOL, SHIFT_WORDS, SHIFT_CENSUS, SHIFT_NARR };
// the device record of a lattice: dropped[0..5] by old state, [6] = solidification stamps >= 0 after the move, [7] = the
// length of the rebuilt interface list
constexpr int SHIFT_NCNT = 8;

struct ShiftJob {
    SlabView S;                                  // the lattice's view (one slab that owns every plane); S.T = the current buffer
    uint8_t* prev;
    unsigned long long* arr[SHIFT_NARR];         // null: the lattice has no such array (no map)
    unsigned long long fill[3];                  // bits of fill_theta, fill_phi, fill_T
    unsigned long long* sp_w;                    // spare of the 64-bit arrays
    uint8_t *sp_st, *sp_df;                      // spares of state and defect mask (the layout of SlabView::state)
    uint8_t* snap;                               // solidification map: its snapshots
    double* Tsnap;
    unsigned long long* cnt;                     // [SHIFT_NCNT]
    int d[3];                                    // |d_a| <= L (the host clamps: any |d_a| >= L exposes everything)
    int fill_state, edge, active;
};

__device__ __forceinline__ int shift_clamp(int x, int n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }
// the job of this block's lattice; false: nothing to do for it (uniform over the block)
__device__ __forceinline__ bool shift_job(ShiftJob& J, const ShiftJob* __restrict__ jobs)
{
    if (jobs) J = jobs[blockIdx.y];
    return J.active != 0;
}

// Array `a` of every lattice into its spare (back = 0) or the spare back over it (back = 1: the move is the identity).  The
// array has n0 x n1 rows of n2 voxels with W 64-bit words each; voxel (i, j, k), component c sits at base + i * plane + j * row
// + k * W + c.  An exposed entry is the job's fill (the three fields) or `fill_const` (the maps), or with the job's edge mode
// (T only) the source clamped per axis into the array.  The census moves along axis 0 alone.  VEC: every lattice's rows start
// on 16-byte boundaries.  COUNT: the destination words that are >= 0 as signed integers are counted into cnt[6] (the stamps).
// One lattice passes what the kernel needs of its job as scalars (a run-time index into a job held in registers would put the
// job into scratch); an ensemble passes the table, which is indexed in memory.
template <bool VEC, bool COUNT>
__global__ __launch_bounds__(256) void k_shift_words(const ShiftJob* __restrict__ jobs, unsigned long long* arr, unsigned long long* sp,
                                                     unsigned long long fill, int d0, int d1, int d2, int edge_on, unsigned long long* cnt,
                                                     int a, int back, int n0, int n1, int n2, int W, long long base, long long plane,
                                                     long long row, unsigned long long fill_const)
{
    __shared__ unsigned s_n;
    if (jobs) {
        const ShiftJob& j = jobs[blockIdx.y];
        if (!j.active) return;
        arr = j.arr[a]; sp = j.sp_w; cnt = j.cnt;
        fill = a <= SHIFT_T ? j.fill[a <= SHIFT_T ? a : 0] : fill_const;
        d0 = j.d[0]; d1 = j.d[1]; d2 = j.d[2]; edge_on = j.edge;
    }
    if (!arr) return;
    if (COUNT) { if (threadIdx.x == 0) s_n = 0; __syncthreads(); }
    const unsigned long long* __restrict__ src = back ? sp : arr;
    unsigned long long* __restrict__ dst = back ? arr : sp;
    if (back) d0 = 0;
    if (back || a == SHIFT_CENSUS) { d1 = 0; d2 = 0; }
    const bool edge = a == SHIFT_T && edge_on && !back;
    const int rowlen = W * n2, nch = (rowlen + 7) >> 3;
    const long long total = (long long)n0 * n1 * nch;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < total) {
        const int c = (int)(t % nch);
        const long long r = t / nch;
        const int j = (int)(r % n1), i = (int)(r / n1);
        const int si = i - d0, sj = j - d1;
        const bool row_in = (unsigned)si < (unsigned)n0 && (unsigned)sj < (unsigned)n1;
        const unsigned long long* srow = src + base + (long long)shift_clamp(si, n0) * plane + (long long)shift_clamp(sj, n1) * row;
        unsigned long long x[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const int kw = c * 8 + w;
            const int k = kw / W, comp = kw - k * W, sk = k - d2;
            const bool in = row_in && (unsigned)sk < (unsigned)n2;
            x[w] = fill;
            if (kw < rowlen && (in || edge)) x[w] = srow[shift_clamp(sk, n2) * W + comp];
        }
        unsigned long long* drow = dst + base + (long long)i * plane + (long long)j * row + c * 8;
        if (VEC && c * 8 + 8 <= rowlen) {
            ulonglong2* q = reinterpret_cast<ulonglong2*>(drow);
            q[0] = make_ulonglong2(x[0], x[1]); q[1] = make_ulonglong2(x[2], x[3]);
            q[2] = make_ulonglong2(x[4], x[5]); q[3] = make_ulonglong2(x[6], x[7]);
        } else {
#pragma unroll
            for (int w = 0; w < 8; ++w)
                if (c * 8 + w < rowlen) drow[w] = x[w];
        }
        if (COUNT) {
            unsigned n = 0;
#pragma unroll
            for (int w = 0; w < 8; ++w) n += (c * 8 + w < rowlen && (long long)x[w] >= 0) ? 1u : 0u;
            if (n) atomicAdd(&s_n, n);
        }
    }
    if (COUNT) {
        __syncthreads();
        if (threadIdx.x == 0 && s_n) atomicAdd(&cnt[6], (unsigned long long)s_n);
    }
}

// state and defect mask of the new lattice into the spares, and the old voxels that leave the lattice counted by state into
// cnt[0..5]
__global__ __launch_bounds__(256) void k_shift_bytes(ShiftJob J, const ShiftJob* __restrict__ jobs)
{
    __shared__ unsigned s_cnt[6];
    if (!shift_job(J, jobs)) return;
    if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const SlabView& S = J.S;
    const int d0 = J.d[0], d1 = J.d[1], d2 = J.d[2];
    const int L = S.L, nch = (L + 7) >> 3;
    const long long total = (long long)L * L * nch;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < total) {
        const int k0 = (int)(t % nch) * 8;
        const long long r = t / nch;
        const int j = (int)(r % L), i = (int)(r / L);
        const int si = i - d0, sj = j - d1;
        const bool row_in = (unsigned)si < (unsigned)L && (unsigned)sj < (unsigned)L;
        const int64_t srow = S.sidx(shift_clamp(si, L) + 2, shift_clamp(sj, L), 0), drow = S.sidx(i + 2, j, k0);
        const bool row_out = (unsigned)(i + d0) >= (unsigned)L || (unsigned)(j + d1) >= (unsigned)L;
        unsigned a[8], m[8], pack = 0;      // pack: six 4-bit counters, at most 8 voxels per lane
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const int k = k0 + w, sk = k - d2;
            const bool in = row_in && k < L && (unsigned)sk < (unsigned)L;
            a[w] = (unsigned)J.fill_state; m[w] = 0;
            if (in) { a[w] = S.state[srow + sk]; m[w] = S.defects[srow + sk]; }
            if (k < L && (row_out || (unsigned)(k + d2) >= (unsigned)L)) {
                const unsigned o = S.state[drow + w];
                pack += 1u << (4 * (o <= 4u ? o : 5u));
            }
        }
        if (k0 + 8 <= L) {
            unsigned* ps = reinterpret_cast<unsigned*>(J.sp_st + drow);
            unsigned* pd = reinterpret_cast<unsigned*>(J.sp_df + drow);
            ps[0] = a[0] | a[1] << 8 | a[2] << 16 | a[3] << 24; ps[1] = a[4] | a[5] << 8 | a[6] << 16 | a[7] << 24;
            pd[0] = m[0] | m[1] << 8 | m[2] << 16 | m[3] << 24; pd[1] = m[4] | m[5] << 8 | m[6] << 16 | m[7] << 24;
        } else {
#pragma unroll
            for (int w = 0; w < 8; ++w)
                if (k0 + w < L) { J.sp_st[drow + w] = (uint8_t)a[w]; J.sp_df[drow + w] = (uint8_t)m[w]; }
        }
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const unsigned n = (pack >> (4 * b)) & 15u;
            if (n) atomicAdd(&s_cnt[b], n);
        }
    }
    __syncthreads();
    if (threadIdx.x < 6 && s_cnt[threadIdx.x]) atomicAdd(&J.cnt[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// the spares back over state and defects, and what an upload of a state writes beside it: prev_state := state, the class
// bytes class8(state) with zero count bits (the interface rebuild follows).  Lattice voxels only.
__global__ __launch_bounds__(256) void k_shift_bytes_back(ShiftJob J, const ShiftJob* __restrict__ jobs)
{
    if (!shift_job(J, jobs)) return;
    const SlabView& S = J.S;
    const int L = S.L, nch = (L + 7) >> 3;
    const long long total = (long long)L * L * nch;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int k0 = (int)(t % nch) * 8;
    const long long r = t / nch;
    const int j = (int)(r % L), i = (int)(r / L);
    const int64_t q = S.sidx(i + 2, j, k0), qc = S.cidx(i + 2, j, k0);
    if (k0 + 8 <= L) {
        const unsigned* ps = reinterpret_cast<const unsigned*>(J.sp_st + q);
        const unsigned* pd = reinterpret_cast<const unsigned*>(J.sp_df + q);
        const unsigned s0 = ps[0], s1 = ps[1], m0 = pd[0], m1 = pd[1];
        unsigned* o = reinterpret_cast<unsigned*>(S.state + q);
        o[0] = s0; o[1] = s1;
        o = reinterpret_cast<unsigned*>(J.prev + q);
        o[0] = s0; o[1] = s1;
        o = reinterpret_cast<unsigned*>(S.defects + q);
        o[0] = m0; o[1] = m1;
        unsigned long long c8 = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const unsigned st = ((w < 4 ? s0 : s1) >> (8 * (w & 3))) & 255u;
            c8 |= (unsigned long long)class8((int)st) << (8 * w);
        }
        *reinterpret_cast<unsigned long long*>(S.cls + qc) = c8;
    } else {
        for (int w = 0; k0 + w < L; ++w) {
            const uint8_t st = J.sp_st[q + w];
            S.state[q + w] = st; J.prev[q + w] = st; S.defects[q + w] = J.sp_df[q + w];
            S.cls[qc + w] = class8((int)st);
        }
    }
}

// ---- the rest of an upload of a state and of orientations, per lattice (upload_impl's sequence; grid-stride over x) ----------
// row flags := 0 (prev_state == state), interface flags := 0, list length := 0
__global__ __launch_bounds__(256) void k_shift_clear(ShiftJob J, const ShiftJob* __restrict__ jobs)
{
    if (!shift_job(J, jobs)) return;
    const SlabView& S = J.S;
    const int64_t nrow = (int64_t)(S.nloc + 4) * S.L, nin = nrow * S.pitchT / 4;       // pitchT is a multiple of 8
    unsigned* in4 = reinterpret_cast<unsigned*>(S.ifc_in);
    const int64_t step = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t q = t0; q < nin; q += step) in4[q] = 0u;
    for (int64_t q = t0; q < nrow; q += step) S.row_chg[q] = 0;
    if (t0 == 0) *S.ifc_n = 0;
}
// k_ifc_rebuild
__global__ __launch_bounds__(256) void k_shift_ifc_rebuild(ShiftJob J, const ShiftJob* __restrict__ jobs)
{
    if (!shift_job(J, jobs)) return;
    const SlabView& S = J.S;
    const int L = S.L;
    const int64_t n = (int64_t)S.nloc * L * L;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int k = (int)(idx % L);
        const int64_t r = idx / L;
        const int j = (int)(r % L), lp = (int)(r / L);
        bool hit;
        const unsigned code = ifc_encode(S, lp + 2, j, k, &hit);
        if (hit) { const int64_t t = S.tidx(lp + 2, j, k); S.ifc_in[t] = 1; S.ifc_code[t] = code; }
    }
}
// k_ifc_relist: x = blocks of RELIST_ROWS rows
__global__ __launch_bounds__(256) void k_shift_ifc_relist(ShiftJob J, const ShiftJob* __restrict__ jobs)
{
    if (!shift_job(J, jobs)) return;
    ifc_relist_body(J.S);
}
// k_orient
__global__ __launch_bounds__(256) void k_shift_orient(ShiftJob J, const ShiftJob* __restrict__ jobs)
{
    if (!shift_job(J, jobs)) return;
    const SlabView& S = J.S;
    const int64_t n = (int64_t)(S.nloc + 4) * S.L * S.pitchT;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256)
        orient_vec(S.theta[idx], S.phi[idx], S.ovec + 3 * idx);
}
// k_solid_snapshot of the lattices that moved: snapshot := state, T_snap := T.  x = pairs of neighbouring k
__global__ __launch_bounds__(256) void k_shift_snapshot(ShiftJob J, const ShiftJob* __restrict__ jobs)
{
    if (!shift_job(J, jobs) || !J.snap) return;
    const SlabView& S = J.S;
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
    *reinterpret_cast<double2*>(J.Tsnap + row * S.pitchT + k) = t;
    *reinterpret_cast<unsigned short*>(J.snap + row * S.pitchT + k) = s;
}
// the length of the rebuilt list into the count record (one copy to the host for everything)
__global__ void k_shift_finish(ShiftJob J, const ShiftJob* __restrict__ jobs, int R)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    if (jobs) J = jobs[r];
    if (J.active) J.cnt[7] = (unsigned long long)*J.S.ifc_n;
}

}  // namespace cetkmc
