// kin_tile.h -- the per-tile phases of the fused fkine + Jacobian (+ Hessian) kernel.
//
// A tile is 64 consecutive configurations = one wavefront; lane l owns configuration cfg0 + l.
// LDS (per wave, private -- no inter-wave traffic):
//     rows : 64 x stride doubles, lane-major ("AoS"): rows[l*stride + slot].  stride is odd, so the
//            lane stride in dwords is 2 (mod 4): ds_write_b64 (16-lane groups, 32 banks) and
//            ds_read_b64 (32-lane groups, 64 banks) are conflict-free for per-lane access.
//            Holds the Jacobian scratch (p_j, z_j), then the finished J, then (re-used) the 4x4.
//     qs   : qw x 64 doubles, column-major ("SoA"): qs[c*64 + l].
// Why LDS at all: the outputs are (N,4,4) and (N,6,n) row-major, i.e. 128 B and 48n B contiguous
// PER CONFIGURATION.  A lane-per-configuration store would scatter 16 B pieces at a 336 B stride;
// staging the wave's outputs in LDS lets the wave write its 64 x 336 B = 21 KB of J (and 8 KB of T)
// as one contiguous run, 16 B per lane per instruction -- the fully coalesced pattern.
//
// Every phase is a __host__ __device__ function of (lane, LDS pointers): the GPU kernel calls them
// with lane = threadIdx.x between s_barriers; tests/emu calls them in a loop over lanes on the CPU.
#pragma once
#include "kin_device.h"

namespace rtbhip {

struct KinParams {
    int32_t n, qw, stride, frame;
    int32_t has_base, pad;
    int64_t N;
    double base[12];  // row-major 3x4, applied to T only
    double tail[12];  // C_n * tool as {R row-major (9), t (3)}
};

RTB_HD int kin_stride(int n)
{
    int s = 6 * n;
    if (s < 16) s = 16;
    return s + 1;  // odd
}
RTB_HD size_t kin_lds_bytes(int n, int qw) { return (size_t)kWave * (kin_stride(n) + qw) * sizeof(double); }

// phase A: this lane's joint coordinates -> qs (zero for lanes past the end of the batch)
template <class S>
RTB_HD void kin_load_q(const KinParams &kp, const S *__restrict__ q, int64_t cfg, int lane,
                       double *qs)
{
    const bool live = cfg < kp.N;
    const S *src = q + cfg * kp.qw;
    int c = 0;
    for (; c + 4 <= kp.qw; c += 4) {  // 4 independent loads in flight before the first LDS write
        double a0 = live ? src[c] : 0.0, a1 = live ? src[c + 1] : 0.0;
        double a2 = live ? src[c + 2] : 0.0, a3 = live ? src[c + 3] : 0.0;
        qs[(c + 0) * kWave + lane] = a0;
        qs[(c + 1) * kWave + lane] = a1;
        qs[(c + 2) * kWave + lane] = a2;
        qs[(c + 3) * kWave + lane] = a3;
    }
    for (; c < kp.qw; ++c) qs[c * kWave + lane] = live ? src[c] : 0.0;
}

// phase B: walk the chain, leave the pose in P (tool applied) and the finished J in rows.
template <bool WANT_J, class CV>
RTB_HD void kin_walk(const KinParams &kp, const CV &cv, int lane, const double *qs, double *rows, Pose &P)
{
    double *mine = rows + lane * kp.stride;
    chain_walk<WANT_J>(cv, kp.n, kp.tail, P,
                       [&](int c) { return qs[c * kWave + lane]; },
                       [&](int slot, double v) { mine[slot] = v; });
    if (WANT_J)
        jacobian_close(cv, kp.n, P, kp.frame, [&](int s) { return mine[s]; },
                       [&](int s, double v) { mine[s] = v; });
}

// phase D: this lane's 4x4 into rows (after the J flush; the region is re-used)
RTB_HD void kin_stage_T(const KinParams &kp, int lane, double *rows, Pose P)
{
    if (kp.has_base) pose_premul(P, kp.base);
    double *mine = rows + lane * kp.stride;
    pose_store16(P, [&](int k, double v) { mine[k] = v; });
}

// Output rows are written once and never re-read by this kernel: non-temporal 16-byte stores
// (global_store_dwordx4 ... nt) measured 0.0935 vs 0.105 ms per 1e6 Panda configurations on MI355X
// (the bare access-pattern probe, scripts/roofline_probe.hip: 0.0868 vs 0.1013 ms).

// STORAGE TYPE of the per-row arrays (q in; T, J, [T | J] out): double, or float for float32 tensors (rtbhip_fkine_jacob_f32 ...).  The arithmetic is
// fp64 either way: a float is widened right after its load and a result is rounded once (round-to-nearest-even, the plain conversion) right
// before its store, so a float32 call returns exactly float(fp64 call on the widened input).  The LDS tiles stay fp64 in both forms -- the
// run-time-n walk keeps its (p_j, z_j) scratch there -- and a lane writes the same PAIR of staged values per instruction in both: 16 bytes of
// doubles or 8 bytes of floats.  The LDS side of a flush (pair reads, odd row strides, the piece bookkeeping) is therefore the fp64 one, and a
// float wave-instruction covers a contiguous 512-byte run = four whole 128-byte lines.  (Four floats per lane were weighed: the lanes of a
// ds_read_b64 would then be 8 dwords apart, 4-way on the 64 banks instead of 2-way, for half the store instructions.)  A float pointer is only
// assumed 4-byte aligned: an offset view of a float32 tensor is a legal argument.
template <bool NT>
RTB_HD void store_pair_f32(float *__restrict__ dst, double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float v2f __attribute__((ext_vector_type(2)));
    typedef v2f v2f_a4 __attribute__((aligned(4)));
    v2f w = {(float)a, (float)b};
    if (NT) __builtin_nontemporal_store(w, reinterpret_cast<v2f_a4 *>(dst));   // global_store_dwordx2 ... nt
    else *reinterpret_cast<v2f_a4 *>(dst) = w;
#else
    dst[0] = (float)a;
    dst[1] = (float)b;
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
// A FULL round of a flush whose row count and row width are compile-time numbers (the register-resident tile: kin_kernels.hip, reg_tile): the
// run's length is then a constant, a lane's pieces are unrolled, and the LDS reads run kFlushGroup pieces ahead of the stores -- each store waits
// by count for its own pair only, and the read of piece p + kFlushGroup is issued behind it.  In the rolled loop below every piece waited for its own LDS round trip: 29 in series
// per lane for the Panda's T + J, which shows where a wave has nobody to hide behind (the first and the last waves of a launch).
// Same pieces, same lanes, same addresses as the loop: piece p of lane l is the pair at f = 2 l + 128 p, present while f < total (total is even).
// src_of(f) -> the pair's place in LDS.
constexpr int kFlushGroup = 3;      // (4 cost the float32 T+J signature kernel its fourth wave: 129 VGPRs)
template <bool NT, class S>
__device__ __forceinline__ void store_piece(S *__restrict__ dst, double a, double b)
{
    if constexpr (sizeof(S) == 4) {
        store_pair_f32<NT>(dst, a, b);
    } else {
        typedef double v2d __attribute__((ext_vector_type(2)));
        v2d w = {a, b};
        if (NT) __builtin_nontemporal_store(w, reinterpret_cast<v2d *>(dst));   // global_store_dwordx4 ... nt
        else *reinterpret_cast<v2d *>(dst) = w;
    }
}
template <bool NT, int TOTAL, class S, class Src>
__device__ __forceinline__ void flush_full(S *__restrict__ dst, int lane, Src src_of)
{
    static_assert(TOTAL > 0 && TOTAL % 2 == 0, "whole pairs");
    constexpr int NP = (TOTAL + 127) / 128;
    double a[kFlushGroup], b[kFlushGroup];      // slot p % kFlushGroup holds piece p between its read and its store
    // A caller that picks the store kind by a wave-uniform flag (reg_tile's pose flush) has this body twice, the same but for the `nt` of its stores:
    // the optimiser folded the two into one and dropped the flag -- every full pose tile went out with ordinary stores.  The markers (no
    // instruction) at both ends of the non-temporal copy keep the two apart; the code object is checked for it (profiles/r08_kin_wave_latency.txt).
    if (NT) asm volatile("");
    auto has = [&](int p) { return 128 * (p + 1) <= TOTAL || 2 * lane + 128 * p < TOTAL; };      // (a whole piece: decided at compile time)
    auto read = [&](int p) {
        if (has(p)) {
            const double *src = src_of(2 * lane + 128 * p);
            a[p % kFlushGroup] = src[0];
            b[p % kFlushGroup] = src[1];
        }
    };
#pragma unroll
    for (int p = 0; p < kFlushGroup && p < NP; ++p) read(p);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (has(p)) store_piece<NT>(dst + 2 * lane + 128 * p, a[p % kFlushGroup], b[p % kFlushGroup]);
        if (p + kFlushGroup < NP) read(p + kFlushGroup);      // the slot is free again: kFlushGroup reads stay in flight ahead of the stores
    }
    if (NT) asm volatile("");
}
#endif

// phases C / E: the wave writes `ncfg` staged rows of W doubles (W even) as one contiguous run.
// Lane l writes the 16-byte pieces l, l+64, l+128, ... of the run; (cfg, e) tracks which staged
// row / element piece f falls in without a division per piece.
// FULL_ROWS, FULL_W (device code; 0: none): when the caller's rounds hold FULL_ROWS rows of FULL_W doubles and this one is full (ncfg == FULL_ROWS,
// wave-uniform) it takes the unrolled form above; a ragged round -- the last tile of a batch -- and every caller with a run-time width take the loop.
template <bool NT = true, int FULL_ROWS = 0, int FULL_W = 0, class S>
RTB_HD void kin_flush(const double *rows, int stride, int W, int ncfg, S *__restrict__ dst,
                      int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (FULL_ROWS > 0) {
        if (ncfg == FULL_ROWS) {
            flush_full<NT, FULL_ROWS * FULL_W>(dst, lane, [&](int f) { const int cfg = (unsigned)f / (unsigned)FULL_W; return rows + cfg * stride + (f - cfg * FULL_W); });
            return;
        }
    }
#endif
    const int total = ncfg * W;
    int f = 2 * lane;
    int cfg = f / W, e = f - cfg * W;
    const int da = 128 / W, db = 128 - da * W;
    for (; f < total; f += 128) {
        const double *src = rows + cfg * stride + e;
        if constexpr (sizeof(S) == 4) {
            store_pair_f32<NT>(dst + f, src[0], src[1]);
            e += db;
            cfg += da;
            if (e >= W) { e -= W; cfg += 1; }
            continue;
        }
        double2 v;
        v.x = src[0];
        v.y = src[1];
#if defined(__HIP_DEVICE_COMPILE__)
        if (NT) {
            typedef double v2d __attribute__((ext_vector_type(2)));
            v2d w = {v.x, v.y};
            __builtin_nontemporal_store(w, reinterpret_cast<v2d *>(dst + f));   // global_store_dwordx4 ... nt
        } else {
            *reinterpret_cast<double2 *>(dst + f) = v;
        }
#else
        *reinterpret_cast<double2 *>(dst + f) = v;
#endif
        e += db;
        cfg += da;
        if (e >= W) { e -= W; cfg += 1; }
    }
}

// PACKED output (SURVEY 8e's gather message: one (N, 16 + 6n) array, row = [T row-major 4x4 | J (6,n) C-order]): the wave writes `ncfg` staged
// rows of 16 + W doubles as ONE contiguous run -- a single write stream per launch, where the two-array form has two.  T and J are staged in
// separate LDS areas (rowsT: 17-double rows; rowsJ: `strideJ`-double rows); 16 and W are even, so a 16-byte piece never straddles the two.
// (FULL_ROWS, FULL_W: as kin_flush -- FULL_W is the J part's width)
template <bool NT = true, int FULL_ROWS = 0, int FULL_W = 0, class S>
RTB_HD void kin_flush_packed(const double *rowsT, const double *rowsJ, int strideJ, int W, int ncfg, S *__restrict__ dst, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (FULL_ROWS > 0) {
        if (ncfg == FULL_ROWS) {
            flush_full<NT, FULL_ROWS * (16 + FULL_W)>(dst, lane, [&](int f) {
                const int cfg = (unsigned)f / (unsigned)(16 + FULL_W), e = f - cfg * (16 + FULL_W);
                return e < 16 ? rowsT + cfg * 17 + e : rowsJ + cfg * strideJ + (e - 16);
            });
            return;
        }
    }
#endif
    const int PW = 16 + W;
    const int total = ncfg * PW;
    int f = 2 * lane;
    int cfg = f / PW, e = f - cfg * PW;
    const int da = 128 / PW, db = 128 - da * PW;
    for (; f < total; f += 128) {
        const double *src = e < 16 ? rowsT + cfg * 17 + e : rowsJ + cfg * strideJ + (e - 16);
        if constexpr (sizeof(S) == 4) {
            store_pair_f32<NT>(dst + f, src[0], src[1]);
            e += db;
            cfg += da;
            if (e >= PW) { e -= PW; cfg += 1; }
            continue;
        }
        double2 v;
        v.x = src[0];
        v.y = src[1];
#if defined(__HIP_DEVICE_COMPILE__)
        if (NT) {
            typedef double v2d __attribute__((ext_vector_type(2)));
            v2d w = {v.x, v.y};
            __builtin_nontemporal_store(w, reinterpret_cast<v2d *>(dst + f));
        } else {
            *reinterpret_cast<double2 *>(dst + f) = v;
        }
#else
        *reinterpret_cast<double2 *>(dst + f) = v;
#endif
        e += db;
        cfg += da;
        if (e >= PW) { e -= PW; cfg += 1; }
    }
}

#if defined(__HIPCC__)
// contiguous run of ncfg rows of W doubles (row stride `stride` in LDS) -> global, 16 bytes per lane per
// piece; W may be odd (a piece may then straddle two rows, and the run may end on a single double)
__device__ __forceinline__ void flush_run(const double *rows, int stride, int W, int ncfg, double *__restrict__ dst, int lane)
{
    const int total = ncfg * W;
    for (int f = 2 * lane; f < total; f += 2 * kWave) {
        const int r = f / W, e = f - r * W;
        const double a = rows[r * stride + e];
        if (f + 1 < total) {
            const double b = (e + 1 < W) ? rows[r * stride + e + 1] : rows[(r + 1) * stride];
            typedef double v2d __attribute__((ext_vector_type(2)));
            v2d w = {a, b};
            __builtin_nontemporal_store(w, reinterpret_cast<v2d *>(dst + f));
        } else {
            __builtin_nontemporal_store(a, dst + f);
        }
    }
}
#endif

// un-coalesced alternative (A/B baseline): every lane stores its own row straight from LDS
template <class S>
RTB_HD void kin_store_own(const double *rows, int stride, int W, bool live, S *__restrict__ dst_row,
                          int lane)
{
    if (!live) return;
    const double *mine = rows + lane * stride;
    for (int e = 0; e < W; e += 2) {
        if constexpr (sizeof(S) == 4) {
            store_pair_f32<false>(dst_row + e, mine[e], mine[e + 1]);
            continue;
        }
        double2 v;
        v.x = mine[e];
        v.y = mine[e + 1];
        *reinterpret_cast<double2 *>(dst_row + e) = v;
    }
}

// Hessian epilogue: straight from the finished J in rows to this lane's (n,6,n) block.
RTB_HD void kin_hessian(const KinParams &kp, int lane, const double *rows, bool live,
                        double *__restrict__ Hrow)
{
    if (!live) return;
    const double *mine = rows + lane * kp.stride;
    hessian_from_jacobian(kp.n, [&](int s) { return mine[s]; }, [&](int idx, double v) { Hrow[idx] = v; });
}

}  // namespace rtbhip
