// thermal_imp.hpp -- implicit temperature update: locally one-dimensional backward Euler (not in the
// reference).
//
// One implicit step of length dt:  b = scrub(T) + dt * (qterm + latent_coef * dF)  per voxel, then (I - r D) x = b along
// every line of axis 2 (k), of axis 1 (j) and of axis 0 (i), in that order, r = (alpha dt) / dx^2, D the 1-D second difference
// with the lattice edge replicated; the clip follows the third solve.  Each solve is the Thomas algorithm with the coefficient
// table inv[m], p[m] = r inv[m] the host computed in double (cetkmc_implicit_coeffs):
//   forward   y[0] = b[0] inv[0],   y[m] = (b[m] + r y[m - 1]) inv[m]
//   backward  x[L - 1] = y[L - 1],  x[m] = y[m] + p[m] x[m + 1]
// Multiplies and adds only, under -ffp-contract=off, one line strictly in order: the same bits as a sequential restatement.
// (The right-hand side keeps thermal_voxel()'s one division, qv / rho_cp, where the source plane is not zero.)
//
// Three launches per implicit step, each variadic in a trailing EnsSel (the replica rides in a grid dimension):
//
// k_imp_rows    right-hand side and k solve; reads the current buffer, writes the other.  Lines along k are contiguous, so a
//               one-wave block owns IMP_R = 64 consecutive rows and moves them in chunks of IMP_C = 64 columns through an LDS
//               tile of pitch 65 doubles: global access with the lanes along k (IMP_V row segments of 512 B in flight), LDS access
//               transposed for the sweep, where lane t owns row t (65 doubles = 130 banks of 4 B: a half-wave's 8-byte reads fall
//               on all 64 banks).  The forward sweep writes y, the backward sweep reads it back chunk by chunk in reverse; the
//               last chunk of the forward sweep is still in LDS when the backward sweep begins.
//               Bytes per voxel: 8 read + 8 (y) + 8 (y again) + 8 (x) = 32, less 16 for the chunk that stays in LDS (L <= 64: 16).
// k_imp_lines   <1>: the j solve, <0>: the i solve and the clip; in place.  A thread owns one line, the lanes run along k, so
//               every access is a row segment.  The element index m is wave-uniform: inv[m] and p[m] are uniform loads.  The
//               dependent chain is three fp64 operations per element; the loads do not depend on it and are issued IMP_U
//               elements ahead (two register sets of IMP_U).  Forward writes y, backward reads it back: 32 B per voxel.
//
// 96 B per voxel and implicit step before cache hits (92 at L = 256: one chunk in four of k_imp_rows stays in LDS; 80 up to L = 64).
// Behind an early stop of the batch (status != 0) k_imp_rows copies the field and k_imp_lines returns.
//
// Boundary form: the instantiations whose trailing pack BEGINS with an ImpBc, k_imp_rows<ImpBc>,
// k_imp_lines<AXIS, ImpBc> and the same with EnsSel behind it.  A face f with beta_f != 0 sees a ghost node x + beta_f (T_f - x):
// the end diagonals change (the host's table, [3][2][L]: one inv, p pair per axis) and the right-hand side of the end row gains
// the wave-uniform addend c_f = (r beta_f) T_f in front of everything else that row adds: y[0] = (b[0] + c_lo) inv[0],
// y[L - 1] = ((b[L - 1] + c_hi) + r y[L - 2]) inv[L - 1].  An adiabatic face adds nothing (not even + 0.0).  Every boundary
// statement stands under if constexpr: the instantiations without an ImpBc are the kernels of section 26, instruction for
// instruction.
//
// Beam form: the instantiations of k_imp_rows whose trailing pack holds an ImpBeam, behind the optional
// ImpBc and in front of the optional EnsSel.  The source is no plane but a product of factors the host tabulated:
// qv = (amp * fi[d]) * (gj[j] * gk[k]) for depth d = L - 1 - i < D, else 0: three multiplies in this order, under
// -ffp-contract=off the bits of a sequential restatement.  amp * fi[d] and gj[j] are wave-uniform; the lane's gk[k] is loaded once
// per chunk of columns, ahead of the row loop, which issues no load for the source.  A row whose uniform factors give zero gets
// the term of an unheated row, so the ballot of rows with full terms is the beam's footprint.  q_top is null.  Every beam
// statement stands under if constexpr; k_imp_lines knows no beam.
#pragma once
#include "kernels.hpp"

namespace cetkmc {

struct ImpCfg {
    double r, dt, dF;            // dF: 1 / max(dt, 1e-12), the latent-heat indicator's rate (thermal_voxel), divided on the host
    double clip_lo, clip_hi, T_nan, rho_cp, latent_coef;
    const double* coef;          // [2][L]: inv, p
    int laser, use_latent, scrub;
};
// the boundary of one implicit step: the six addends, faces in the order i_lo, i_hi, j_lo, j_hi, k_lo, k_hi (face 2 * axis + hi),
// and one bit per face with beta != 0.  With a boundary ImpCfg::coef is [3][2][L]: inv, p of axis 0, of axis 1, of axis 2.
struct ImpBc {
    double c[6];
    int on;
};
// the source of one update in the beam form: the current row of the handle's beam table (device pointers).  An ensemble's table
// holds its sets one behind the other, set_stride doubles apart; replica r reads set set_of[r] (a single handle: set_of null, the
// pointers are those of its own set).
struct ImpBeam {
    const double* amp;           // [1]
    const double* gj;            // [L]
    const double* gk;            // [L]
    const double* fi;            // [depth]
    const int32_t* set_of;       // [R], ensemble launches only
    int64_t set_stride;
    int depth;
};
template <class... E> struct imp_pack { static constexpr bool bc = false, beam = false; static constexpr int n_ens = (int)sizeof...(E); };
template <class... E> struct imp_pack<ImpBc, E...> { static constexpr bool bc = true, beam = false; static constexpr int n_ens = (int)sizeof...(E); };
template <class... E> struct imp_pack<ImpBeam, E...> { static constexpr bool bc = false, beam = true; static constexpr int n_ens = (int)sizeof...(E); };
template <class... E> struct imp_pack<ImpBc, ImpBeam, E...> { static constexpr bool bc = true, beam = true; static constexpr int n_ens = (int)sizeof...(E); };
template <class... E> __device__ __forceinline__ const ImpBc& imp_bc_of(const ImpBc& B, const E&...) { return B; }
// the replica selection of a boundary-form ensemble launch stands behind the ImpBc
template <class S> __device__ __forceinline__ const auto& ens_rep(unsigned r, const ImpBc&, const S& sel) { return ens_rep(r, sel); }
template <class S> __device__ __forceinline__ int ens_rel(const ImpBc&, const S& sel) { return ens_rel(sel); }
template <class S> __device__ __forceinline__ int64_t ens_q_off(const ImpBc&, const S& sel) { return ens_q_off(sel); }
// the beam of a beam-form launch, and its replica selection behind the ImpBeam
template <class... E> __device__ __forceinline__ const ImpBeam& imp_beam_of(const ImpBeam& M, const E&...) { return M; }
template <class... E> __device__ __forceinline__ const ImpBeam& imp_beam_of(const ImpBc&, const ImpBeam& M, const E&...) { return M; }
template <class S> __device__ __forceinline__ const auto& ens_rep(unsigned r, const ImpBeam&, const S& sel) { return ens_rep(r, sel); }
template <class S> __device__ __forceinline__ int ens_rel(const ImpBeam&, const S& sel) { return ens_rel(sel); }
template <class S> __device__ __forceinline__ const auto& ens_rep(unsigned r, const ImpBc&, const ImpBeam&, const S& sel) { return ens_rep(r, sel); }
template <class S> __device__ __forceinline__ int ens_rel(const ImpBc&, const ImpBeam&, const S& sel) { return ens_rel(sel); }
constexpr int IMP_R = 64, IMP_C = 64, IMP_PITCH = IMP_C + 1, IMP_U = 8, IMP_V = 16;   // IMP_V: rows of a chunk in flight per lane (k_imp_rows)

// the scrub of this scheme: NaN -> T_nan, +-inf -> the clip values (not +-DBL_MAX, which a solve would spread over the lattice)
__device__ __forceinline__ double imp_scrub(double x, const ImpCfg& C)
{
    if (!C.scrub) return x;
    if (x != x) return C.T_nan;
    if (__builtin_isinf(x)) return x > 0 ? C.clip_hi : C.clip_lo;
    return x;
}

// grid: x = blocks of IMP_R rows of the owned planes, y = replica
template <class... E>
__global__ __launch_bounds__(IMP_R) void k_imp_rows(SlabView S, const double* __restrict__ Tin, double* Tout, uint8_t* __restrict__ prev_state,
                                                    const double* __restrict__ q_top, ImpCfg C, const StepState* __restrict__ ss, E... ens)
{
    constexpr bool BC = imp_pack<E...>::bc, BEAM = imp_pack<E...>::beam;
    if constexpr (imp_pack<E...>::n_ens > 0) {
        const auto& e = ens_rep(blockIdx.y, ens...);
        const int rel = ens_rel(ens...);
        S = e.view[rel]; Tin = e.view[rel].T; Tout = e.view[rel ^ 1].T; prev_state = e.prev; ss = e.ss;
        if constexpr (BEAM) q_top = nullptr;
        else q_top = C.laser ? e.q + ens_q_off(ens...) : nullptr;
    }
    __shared__ double tile[IMP_R * IMP_PITCH];
    const int L = S.L, lane = threadIdx.x;
    const int64_t nrows = (int64_t)S.nloc * L, row0 = (int64_t)blockIdx.x * IMP_R;
    const int nr = (int)min((int64_t)IMP_R, nrows - row0);          // rows of this block (uniform)
    const int64_t base = ((int64_t)2 * L + row0) * S.pitchT;         // T index of (row0, k = 0): local plane = owned plane + 2
    const int pitch = S.pitchT;
    if (ss && ss->status) {                     // a terminated batch: the update is a copy
        for (int kc = 0; kc < L; kc += IMP_C) {
            const int k = kc + lane;
            if (k < L)
                for (int q = 0; q < nr; ++q) { const int64_t c = base + (int64_t)q * pitch + k; Tout[c] = Tin[c]; }
        }
        return;
    }
    const double* __restrict__ inv = C.coef + (BC ? 4 * L : 0);       // BC: the pair of axis 2
    const double* __restrict__ pc = inv + L;
    const double r = C.r;
    const bool source = C.laser != 0, latent = source && C.use_latent;
    double* mine = tile + lane * IMP_PITCH;     // the row this lane sweeps
    const int nchunk = (L + IMP_C - 1) / IMP_C;
    // beam form: this replica's set of the table; amp is read only by an update with a source (wave-uniform, as gj and fi are)
    [[maybe_unused]] const double* __restrict__ bgj = nullptr;
    [[maybe_unused]] const double* __restrict__ bgk = nullptr;
    [[maybe_unused]] const double* __restrict__ bfi = nullptr;
    [[maybe_unused]] double bamp = 0.0;
    [[maybe_unused]] int bD = 0;
    if constexpr (BEAM) {
        const ImpBeam& M = imp_beam_of(ens...);
        int64_t off = 0;
        if constexpr (imp_pack<E...>::n_ens > 0) off = (int64_t)M.set_of[blockIdx.y] * M.set_stride;
        bgj = M.gj + off; bgk = M.gk + off; bfi = M.fi + off; bD = M.depth;
        if (source) bamp = M.amp[off];
    }
    // Rows whose right-hand side needs more than the field: those of plane L - 1 (the source) and those written since the last
    // update (latent heat), one bit per row of the block.  Every other voxel of a laser-mode update gets thermal_voxel()'s
    // terms with qterm = dF = 0, which is + 0.0 for finite settings (it turns a -0.0 into +0.0, as the definition does).
    unsigned long long need = 0;
    double zero_term = 0.0;
    if (source) {
        zero_term = C.dt * (0.0 + C.latent_coef * 0.0);
        bool nd = false;
        if (lane < nr) {
            const int64_t row = row0 + lane;
            const int lp = (int)(row / L), j = (int)(row - (int64_t)lp * L);
            if constexpr (BEAM) {       // the beam's footprint: planes L - D .. L - 1, rows with non-zero uniform factors
                const int d = L - 1 - (S.gi0 + lp);
                nd = (d < bD && bamp * bfi[d] != 0.0 && bgj[j] != 0.0) || (latent && S.row_chg[(int64_t)(lp + 2) * L + j]);
            } else {
                nd = (S.gi0 + lp == L - 1) || (latent && S.row_chg[(int64_t)(lp + 2) * L + j]);
            }
        }
        need = __ballot(nd);
    }
    // global <-> tile, the lanes along k.  A load clamps its row and column into the block (no predicates: what lands in the
    // tile beyond the block's rows and the lattice's columns is never swept into a stored value); a store is predicated.
    auto load_rows = [&](const double* __restrict__ g, int kc, int q0, double (&v)[IMP_V]) {
        const double* p = g + base + min(kc + lane, L - 1);
#pragma unroll
        for (int u = 0; u < IMP_V; ++u) v[u] = p[min(q0 + u, nr - 1) * pitch];
    };
    auto store_chunk = [&](int kc) {
        if (kc + lane < L) {
            double* p = Tout + base + kc + lane;
#pragma unroll 8
            for (int q = 0; q < nr; ++q) p[q * pitch] = tile[q * IMP_PITCH + lane];
        }
    };
    // ---- forward: right-hand side in, y out ----
    double y = 0.0;
#pragma unroll 1
    for (int ch = 0; ch < nchunk; ++ch) {
        const int kc = ch * IMP_C, k = kc + lane, cn = min(IMP_C, L - kc);
#pragma unroll 1
        for (int q0 = 0; q0 < IMP_R; q0 += IMP_V) {
            double v[IMP_V];
            load_rows(Tin, kc, q0, v);
#pragma unroll
            for (int u = 0; u < IMP_V; ++u) {
                double b = imp_scrub(v[u], C);
                if (source && !((need >> (q0 + u)) & 1ull)) b = b + zero_term;
                tile[(q0 + u) * IMP_PITCH + lane] = b;
            }
        }
        if (k < L) {                // the rows with a source or a flag: thermal_voxel()'s terms in full (a lane's own tile entries)
            unsigned long long w = need;
            [[maybe_unused]] double gkv = 0.0;
            if constexpr (BEAM) { if (w) gkv = bgk[k]; }      // the lane's column factor, once per chunk
#pragma unroll 1
            while (w) {
                const int q = __ffsll(w) - 1;
                w &= w - 1;
                const int64_t row = row0 + q;
                const int lp = (int)(row / L), j = (int)(row - (int64_t)lp * L), li = lp + 2;
                double qv;
                if constexpr (BEAM) {
                    const int d = L - 1 - (S.gi0 + lp);
                    qv = d < bD ? (bamp * bfi[d]) * (bgj[j] * gkv) : 0.0;
                } else {
                    qv = (S.gi0 + lp == L - 1) ? q_top[(int64_t)j * L + k] : 0.0;
                }
                const double qterm = (qv != 0.0) ? qv / C.rho_cp : 0.0;
                double dF = 0.0;
                if (latent && S.row_chg[(int64_t)li * L + j]) {      // only rows written since the last update can differ
                    const int64_t sc = S.sidx(li, j, k);
                    const int st = S.state[sc], pv = prev_state[sc];
                    if (pv == 0 && st != 0) dF = C.dF;
                    if (pv != st) prev_state[sc] = (uint8_t)st;
                }
                tile[q * IMP_PITCH + lane] = tile[q * IMP_PITCH + lane] + C.dt * (qterm + C.latent_coef * dF);
            }
        }
        __syncthreads();
        if constexpr (BC) {         // the end addends of faces k_lo, k_hi, on the lane's own row (L = 1: (b + c_lo) + c_hi)
            const ImpBc& B = imp_bc_of(ens...);
            if (ch == 0 && (B.on & 16)) mine[0] = mine[0] + B.c[4];
            if (ch + 1 == nchunk && (B.on & 32)) mine[cn - 1] = mine[cn - 1] + B.c[5];
        }
#pragma unroll 8
        for (int c = 0; c < cn; ++c) {
            const int m = kc + c;
            const double b = mine[c];
            const double a = (m == 0) ? b : b + r * y;
            y = a * inv[m];
            mine[c] = y;
        }
        __syncthreads();
        if (ch + 1 < nchunk) {                  // (the last chunk stays in LDS for the backward sweep)
            store_chunk(kc);
            __syncthreads();
        }
    }
    // ---- backward: y in, x out ----
    double x = 0.0;
#pragma unroll 1
    for (int ch = nchunk - 1; ch >= 0; --ch) {
        const int kc = ch * IMP_C, cn = min(IMP_C, L - kc);
        if (ch + 1 < nchunk) {
#pragma unroll 1
            for (int q0 = 0; q0 < IMP_R; q0 += IMP_V) {
                double v[IMP_V];
                load_rows(Tout, kc, q0, v);
#pragma unroll
                for (int u = 0; u < IMP_V; ++u) tile[(q0 + u) * IMP_PITCH + lane] = v[u];
            }
            __syncthreads();
        }
#pragma unroll 8
        for (int c = cn - 1; c >= 0; --c) {
            const int m = kc + c;
            const double yv = mine[c];
            x = (m == L - 1) ? yv : yv + pc[m] * x;
            mine[c] = x;
        }
        __syncthreads();
        store_chunk(kc);
        __syncthreads();
    }
}

// AXIS 1: lines along j, grid y = owned plane; AXIS 0: lines along i (the whole lattice in one slab), grid y = j, and the clip.
// grid: x = segments of 64 k, z = replica
template <int AXIS, class... E>
__global__ __launch_bounds__(64) void k_imp_lines(SlabView S, double* T, ImpCfg C, const StepState* __restrict__ ss, E... ens)
{
    constexpr bool BC = imp_pack<E...>::bc;
    if constexpr (imp_pack<E...>::n_ens > 0) {
        const auto& e = ens_rep(blockIdx.z, ens...);
        S = e.view[ens_rel(ens...)]; T = S.T; ss = e.ss;
    }
    if (ss && ss->status) return;
    const int L = S.L, k = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (k >= L) return;
    const int64_t plane = (int64_t)L * S.pitchT;
    const int64_t ls = AXIS == 1 ? (int64_t)S.pitchT : plane;                            // from element m to m + 1 of the line
    double* p0 = T + 2 * plane + (int64_t)blockIdx.y * (AXIS == 1 ? plane : (int64_t)S.pitchT) + k;
    const double* __restrict__ inv = C.coef + (BC ? 2 * AXIS * L : 0);       // BC: the pair of this axis
    const double* __restrict__ pc = inv + L;
    const double r = C.r;
    bool lo_on = false, hi_on = false;             // wave-uniform
    double c_lo = 0.0, c_hi = 0.0;
    if constexpr (BC) {
        const ImpBc& B = imp_bc_of(ens...);
        lo_on = (B.on >> (2 * AXIS)) & 1; hi_on = (B.on >> (2 * AXIS + 1)) & 1;
        c_lo = B.c[2 * AXIS]; c_hi = B.c[2 * AXIS + 1];
    }
    auto clip = [&](double v) {
        if constexpr (AXIS == 0) { v = v < C.clip_lo ? C.clip_lo : v; v = v > C.clip_hi ? C.clip_hi : v; }
        return v;
    };
    double cur[IMP_U], nxt[IMP_U];
    // ---- forward ----
    double y;
    if constexpr (BC) {         // L = 1: (b + c_lo) + c_hi
        y = p0[0];
        if (lo_on) y = y + c_lo;
        if (hi_on && L == 1) y = y + c_hi;
        y = y * inv[0];
    } else {
        y = p0[0] * inv[0];
    }
    if (L > 1) p0[0] = y;
    auto load_up = [&](int m0, double (&d)[IMP_U]) {
#pragma unroll
        for (int u = 0; u < IMP_U; ++u) d[u] = (m0 + u < L) ? p0[(int64_t)(m0 + u) * ls] : 0.0;
    };
    load_up(1, cur);
#pragma unroll 1
    for (int m0 = 1; m0 < L; m0 += IMP_U) {
        load_up(m0 + IMP_U, nxt);
#pragma unroll
        for (int u = 0; u < IMP_U; ++u) {
            const int m = m0 + u;
            if (m < L) {
                if constexpr (BC) { if (hi_on && m == L - 1) cur[u] = cur[u] + c_hi; }
                y = (cur[u] + r * y) * inv[m];
                if (m < L - 1) p0[(int64_t)m * ls] = y;
            }
        }
#pragma unroll
        for (int u = 0; u < IMP_U; ++u) cur[u] = nxt[u];
    }
    // ---- backward: x[L - 1] = y[L - 1] is in the register ----
    double x = y;
    p0[(int64_t)(L - 1) * ls] = clip(x);
    auto load_down = [&](int m0, double (&d)[IMP_U]) {
#pragma unroll
        for (int u = 0; u < IMP_U; ++u) d[u] = (m0 - u >= 0) ? p0[(int64_t)(m0 - u) * ls] : 0.0;
    };
    load_down(L - 2, cur);
#pragma unroll 1
    for (int m0 = L - 2; m0 >= 0; m0 -= IMP_U) {
        load_down(m0 - IMP_U, nxt);
#pragma unroll
        for (int u = 0; u < IMP_U; ++u) {
            const int m = m0 - u;
            if (m >= 0) {
                x = cur[u] + pc[m] * x;
                p0[(int64_t)m * ls] = clip(x);
            }
        }
#pragma unroll
        for (int u = 0; u < IMP_U; ++u) cur[u] = nxt[u];
    }
}

}  // namespace cetkmc
