// vjp_tile.h -- the per-tile I/O phases of the fused adjoint (vector-Jacobian product) kernels: k_rne_vjp, k_tree_rne_vjp, k_inertia_vjp,
// k_tree_inertia_vjp, k_coriolis_vjp, k_tree_coriolis_vjp and their run-time-n forms.
//
// A tile is 64 consecutive samples = one wavefront.  The wave's (64 x n) column blocks (q, qd, qdd, gtau ...) and its (64 x n x n) block (gM, gC)
// are contiguous in memory: they are loaded coalesced -- element f = lane + 64 k of a block by lane `lane` -- and transposed into a lane-major LDS
// row per sample, lds[row * stride + slot], at an odd stride (conflict-free rows).  The lane body works on its own row and leaves the results in
// the first slots; they go out the way the inputs came in.
//
// As kin_tile.h: every phase is a __host__ __device__ function of (lane, lds, ...) with no barrier inside.  The kernel calls the phases with
// lane = threadIdx.x and keeps its __syncthreads() between them; tests/emu_vjp_tile calls them in a loop over lanes on the CPU.  A tile function:
//     geometry;  load phases;  sched_fence();  stage phases (vjp_fold: twice, a barrier between);  barrier;  lane body;  barrier;  vjp_tile_flush
// NJ > 0: a compile-time n -- every loop unrolled, the loaded values in registers (VjpCols, VjpMat) between the load and the stage phase.
// NJ = 0: run-time n -- the load phases do nothing and the stage phases read memory themselves.
#pragma once
#include "kin_device.h"
#include "vjp_device.h"

namespace rtbhip {

// tile `tile` of a batch of N samples of n columns: its first sample, its live rows (< 64 on the ragged tail), their n and n^2 element counts
struct VjpTile {
    int64_t cfg0;
    int ncfg, count, mcount;
};
RTB_HD VjpTile vjp_tile_of(int64_t tile, int64_t N, int n)
{
    VjpTile t;
    t.cfg0 = tile * kWave;
    const int64_t left = N - t.cfg0;
    t.ncfg = left < kWave ? (int)left : kWave;
    t.count = t.ncfg * n;
    t.mcount = t.count * n;
    return t;
}

template <int NJ, int A, class S> struct VjpCols { S r[A][NJ > 0 ? NJ : 1]; };
template <int NJ> struct VjpMat { double r[NJ > 0 ? NJ * NJ : 1]; };

// ---- A column blocks of n values per row -> lds[row * stride + a * n + col].  src[a]: block a of THIS tile (the caller adds cfg0 * n); with OPT
// a block may be absent (NULL): zeros.  S: the storage type, widened on the way to LDS.
// The A * NJ loads are UNCONDITIONAL -- an element past the ragged tail reads element 0 of the tile (a tile has at least one row), an absent
// block reads block 0 -- and the zeros are selected afterwards, the values still in their storage type: a load inside the bounds branch takes
// its float -> double conversion, and with it a wait for that one load, into the branch: one dependent HBM round trip per element.  As built
// the loads overlap: each wait lets the oldest load complete while a dozen or more stay in flight, and the counter never drains before the
// last one has been issued.  So: every load phase of the tile, sched_fence(), then the stage phases (select, widen, write).
template <int NJ, bool OPT, int A, class S>
RTB_HD void vjp_load_cols(const S *const (&src)[A], const VjpTile &t, int lane, VjpCols<NJ, A, S> &c)
{
    if constexpr (NJ > 0) {
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int f = lane + kWave * k, fc = f < t.count ? f : 0;
#pragma unroll
            for (int a = 0; a < A; ++a) c.r[a][k] = (!OPT || src[a] ? src[a] : src[0])[fc];
        }
    }
}
template <int NJ, bool OPT, int A, class S>
RTB_HD void vjp_stage_cols(const S *const (&src)[A], const VjpTile &t, int n_rt, int stride, int lane, VjpCols<NJ, A, S> &c, double *lds)
{
    if constexpr (NJ > 0) {
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int f = lane + kWave * k;
#pragma unroll
            for (int a = 0; a < A; ++a)
                if ((OPT && !src[a]) || f >= t.count) c.r[a][k] = S(0);
        }
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int f = lane + kWave * k;
            const int row = f / NJ;
            double *dst = lds + row * stride + (f - row * NJ);
#pragma unroll
            for (int a = 0; a < A; ++a) dst[a * NJ] = (double)c.r[a][k];
        }
    } else {
        const int n = n_rt;
        for (int f = lane; f < kWave * n; f += kWave) {
            const int row = f / n;
            double *dst = lds + row * stride + (f - row * n);
            for (int a = 0; a < A; ++a) dst[a * n] = ((!OPT || src[a]) && f < t.count) ? (double)src[a][f] : 0.0;
        }
    }
}

// ---- the (n x n) block per row.  mg: the block of THIS tile (the caller adds cfg0 * n * n).  Loaded with the column loads, before the fence
template <int NJ>
RTB_HD void vjp_load_mat(const double *mg, const VjpTile &t, int lane, VjpMat<NJ> &m)
{
    if constexpr (NJ > 0) {
#pragma unroll
        for (int k = 0; k < NJ * NJ; ++k) { const int f = lane + kWave * k; m.r[k] = mg[f < t.mcount ? f : 0]; }
    }
}
// FOLDED onto the packed triangle: S(j, i) = gM[j,i] + gM[i,j] (j > i), S(i, i) = gM[i,i] at lds[row * stride + off + j (j + 1) / 2 + i].
// Two phases with a barrier between: UPPER = false writes the lower triangle and the diagonal, UPPER = true adds the upper triangle -- each
// packed slot has exactly one element of either kind, so no two lanes touch a slot within a phase.
// Where element f of the tile's block goes: row f / n^2, entry (r, c) -> the packed slot of (max, min)
RTB_HD int vjp_fold_slot(int f, int n, int stride, int off, bool &lower)
{
    const int nn = n * n, row = f / nn, rem = f - row * nn, r = rem / n, c = rem - r * n;
    lower = r >= c;
    const int hi = lower ? r : c, lo = lower ? c : r;
    return row * stride + off + hi * (hi + 1) / 2 + lo;
}
template <int NJ, bool UPPER>
RTB_HD void vjp_fold(const double *mg, const VjpTile &t, int n_rt, int stride, int off, int lane, const VjpMat<NJ> &m, double *lds)
{
    const int n = NJ > 0 ? NJ : n_rt;
    // (the value comes through a callable: the run-time-n form reads memory for the elements of this phase's triangle only)
    auto put = [&](int f, auto value) {
        bool lower;
        const int at = vjp_fold_slot(f, n, stride, off, lower);
        if (!UPPER && lower) lds[at] = f < t.mcount ? value() : 0.0;
        if (UPPER && !lower) lds[at] = lds[at] + (f < t.mcount ? value() : 0.0);
    };
    if constexpr (NJ > 0) {
#pragma unroll
        for (int k = 0; k < NJ * NJ; ++k) put(lane + kWave * k, [&] { return m.r[k]; });
    } else {
        for (int f = lane; f < kWave * n * n; f += kWave) put(f, [&] { return mg[f]; });
    }
}

// ---- B result column blocks, lds[row * stride + b * n + col] -> dst[b] (the block of THIS tile): LDS to registers, then contiguous non-temporal
// stores at f < count (run-time n: plain stores).  With OPT an output may be NULL: not stored (wave-uniform); without, no null test is compiled in.
template <int NJ, bool OPT, int B, class S>
RTB_HD void vjp_tile_flush(S *const (&dst)[B], const VjpTile &t, int n_rt, int stride, int lane, const double *lds)
{
    if constexpr (NJ > 0) {
        double r[B][NJ];
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int f = lane + kWave * k;
            const int row = f / NJ;
            const double *src = lds + row * stride + (f - row * NJ);
#pragma unroll
            for (int b = 0; b < B; ++b) r[b][k] = src[b * NJ];
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (OPT && !dst[b]) continue;
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                const int f = lane + kWave * k;
                if (f < t.count) __builtin_nontemporal_store((S)r[b][k], dst[b] + f);
            }
        }
    } else {
        const int n = n_rt;
        for (int f = lane; f < t.count; f += kWave) {
            const int row = f / n;
            const double *src = lds + row * stride + (f - row * n);
            for (int b = 0; b < B; ++b)
                if (!OPT || dst[b]) dst[b][f] = (S)src[b * n];
        }
    }
}

#if RTB_HOST_SIDE
// the launch of one adjoint kernel, one wave per workgroup: a tile beyond 48 KB of dynamic LDS needs the attribute raised first
template <class K, class... Args>
void vjp_go(K k, dim3 grid, size_t lds, hipStream_t s, Args... args)
{
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, grid, dim3(kWave), lds, s, args...);
}
#endif

}  // namespace rtbhip
