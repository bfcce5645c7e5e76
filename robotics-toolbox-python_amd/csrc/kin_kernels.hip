// kin_kernels.hip -- gfx950 kernels for batched fkine / jacob0 / jacobe / hessian (headline path).
//
// Replaces the hot loops of core/fknm.cpp:1038-1052 (ETS_fkine trajectory loop) and the Python
// per-row loops around ETS_jacob0/ETS_jacobe/ETS_hessian0 (fknm.cpp:583-921).
//
// Launch shape: one wavefront (64 lanes) per workgroup, one configuration per lane, grid-stride
// over 64-configuration tiles.  Single-wave workgroups make every LDS hand-off wave-private (the
// s_barrier of a one-wave group is free) and let the dispatcher balance tiles across the 256 CUs.
// The chain program is read through the constant address space => s_load into SGPRs.
// Roofline: HBM-bound by construction -- 8*qw bytes in, 128 + 48n bytes out per configuration
// (520 B for the Panda), ~0.6 kflop of fp64 VALU + n sincos per configuration.
#include "kin_reg.h"
#include "kin_vjp.h"
#include "diff_device.h"
#include "servo_device.h"
#include "diff_kernel.h"
#include <algorithm>
#include <cstring>

namespace rtbhip {

// Store policy of the fused fkine + Jacobian kernels.  Both output arrays are streaming writes; written non-temporally, the pair's speed depends on
// WHERE the allocator put T and J relative to one another -- 78 or 90 us per 1e6 Panda configurations, fixed for a given pair of buffers, about
// two pairs in three slow (round 4: profiles/r04_headline_stores.txt).  When the pose array (128 B per configuration) is small enough to stay in
// the part's 256 MB memory-side cache, writing IT with ordinary stores (and first) removes the dependence: a loop that writes the same output
// arrays every step -- bench.py, a control loop with preallocated outputs -- then runs at 78 us on every pair, because the pose array is
// absorbed by that cache and rewritten in place (with three or more output sets used in rotation both forms take 90 us).  Beyond that size
// ordinary stores lose (2e6 configurations: 188-200 us against 148-171), so the launcher turns them on (KinParams.pad bit 0) only for a
// pose array of at most kPoseCacheBytes; everything else -- fkine alone, the fleet, long batches -- streams non-temporally as before.
// RTB_T_PLAIN_MAX_BYTES = 0 restores the form of rounds 1-3 (A/B).  (T after J, the order of rounds 1-3, was the other side of that measurement:
// profiles/retired_switches.md)
#ifndef RTB_T_PLAIN_MAX_BYTES
#define RTB_T_PLAIN_MAX_BYTES (136ll << 20)
#endif
constexpr long long kPoseCacheBytes = RTB_T_PLAIN_MAX_BYTES;
constexpr int kKinPosePlain = 1;      // KinParams.pad bit 0
constexpr int kKinPacked = 2;         // KinParams.pad bit 1: T is the packed (N, 16 + 6n) array [T | J], J is not written separately (run-time-n tile)

// the run-time-n tile loop; S = storage type of q, T and J (kin_tile.h: double, or float for the _f32 entry points; H is fp64 only)
template <bool WANT_T, bool WANT_J, bool WANT_H, bool COALESCED, class S>
__device__ __forceinline__ void kin_tiles(KinParams kp, DevChain dc, const S *__restrict__ q, S *__restrict__ T, S *__restrict__ J,
                                          double *__restrict__ H, double *lds)
{
    double *rows = lds;
    double *qs = lds + kWave * kp.stride;
    const ConstChain ops = const_view(dc);
    const int lane = threadIdx.x;
    const int64_t tiles = (kp.N + kWave - 1) / kWave;
    const int W = 6 * kp.n;

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t cfg0 = tile * kWave;
        const int64_t cfg = cfg0 + lane;
        const int64_t left = kp.N - cfg0;
        const int ncfg = left < kWave ? (int)left : kWave;
        const bool live = lane < ncfg;

        kin_load_q(kp, q, cfg, lane, qs);
        Pose P;
        kin_walk<(WANT_J || WANT_H)>(kp, ops, lane, qs, rows, P);
        if (WANT_H) kin_hessian(kp, lane, rows, live, H + cfg * (int64_t)(kp.n * W));
        if (WANT_T && WANT_J && !WANT_H && COALESCED && (kp.pad & kKinPacked)) {      // wave-uniform: one contiguous run of [T | J] rows
            double *rowsT = qs + kWave * kp.qw;
            if (kp.has_base) pose_premul(P, kp.base);
            pose_store16(P, [&](int k, double v) { rowsT[lane * 17 + k] = v; });
            __syncthreads();
            kin_flush_packed(rowsT, rows, kp.stride, W, ncfg, T + cfg0 * (16 + W), lane);
            __syncthreads();
            continue;
        }
        if (WANT_J) {
            if (COALESCED) {
                __syncthreads();
                kin_flush(rows, kp.stride, W, ncfg, J + cfg0 * W, lane);
            } else {
                kin_store_own(rows, kp.stride, W, live, J + cfg * W, lane);
            }
        }
        if (WANT_T) {
            if (COALESCED) __syncthreads();
            kin_stage_T(kp, lane, rows, P);
            if (COALESCED) {
                __syncthreads();
                if (kp.pad & kKinPosePlain) kin_flush<false>(rows, kp.stride, 16, ncfg, T + cfg0 * 16, lane);      // wave-uniform
                else kin_flush<true>(rows, kp.stride, 16, ncfg, T + cfg0 * 16, lane);
            } else {
                kin_store_own(rows, kp.stride, 16, live, T + cfg * 16, lane);
            }
        }
        __syncthreads();  // rows/qs are rewritten by the next tile
    }
}

template <bool WANT_T, bool WANT_J, bool WANT_H, bool COALESCED>
__global__ __launch_bounds__(kWave) void k_kin(KinParams kp, DevChain dc,
                                              const double *__restrict__ q, double *__restrict__ T,
                                              double *__restrict__ J, double *__restrict__ H)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    kin_tiles<WANT_T, WANT_J, WANT_H, COALESCED>(kp, dc, q, T, J, H, lds);
}
// float32 q, T, J (and packed [T | J] rows): the same tile loop, coalesced form
template <bool WANT_T, bool WANT_J>
__global__ __launch_bounds__(kWave) void k_kin_f32(KinParams kp, DevChain dc, const float *__restrict__ q, float *__restrict__ T, float *__restrict__ J)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    kin_tiles<WANT_T, WANT_J, false, true>(kp, dc, q, T, J, (double *)nullptr, lds);
}

// ---------------------------------------------------------------- register-resident variant (n <= 8)
#ifndef RTB_REG_WAVES
#define RTB_REG_WAVES 3   // waves per SIMD the register allocator must leave room for (<= 168 VGPRs)
#endif
// One register-resident tile (64 configurations) of a chain with NJ joints; shared by k_kin_reg and k_fleet.
// (its rounds' row counts and widths are compile-time numbers: a full round takes the unrolled flush, kin_tile.h: flush_full)
// SIG != 0: the chain's structure signature (kin_reg.h) -- the walk is straight-line code specialised for the robot's constants (k_fleet: always 0)
template <int NJ, bool WANT_T, bool WANT_J, bool PACKED = false, SegSig SIG = 0, int PIPE = 1, class S>
__device__ __forceinline__ void reg_tile(const KinParams &kp, const ConstChain &cv, const S *__restrict__ q,
                                         S *__restrict__ T, S *__restrict__ J, double *buf, int lane,
                                         int64_t tile)
{
    constexpr int W = 6 * NJ;
    const int64_t cfg0 = tile * kWave;
    const int64_t left = kp.N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    Pose P;
    double jac[6 * NJ];
    reg_compute<NJ, WANT_J, SIG>(kp, cv, q, cfg0 + lane, P, jac);
    if constexpr (PACKED) {
        // T is the packed (N, 16 + W) array: rounds of kPRound lanes stage [T | J] and the wave writes the round's rows as one contiguous run
        static_assert(!PACKED || (WANT_T && WANT_J), "packed rows carry both");
        double *bufT = buf, *bufJ = buf + kPRound * 17;
#pragma unroll
        for (int r = 0; r < kWave / kPRound; ++r) {
            if (lane / kPRound == r) reg_stage_packed<NJ>(kp, P, jac, bufT, bufJ, lane % kPRound);
            __syncthreads();
            int rows = ncfg - r * kPRound;
            rows = rows < 0 ? 0 : (rows > kPRound ? kPRound : rows);
            kin_flush_packed<true, PIPE * kPRound, W>(bufT, bufJ, W + 1, W, rows, T + (cfg0 + r * kPRound) * (16 + W), lane);
            __syncthreads();
        }
        return;
    }
    if (WANT_T) {
        reg_stage_T(kp, P, buf, lane);
        __syncthreads();
        if (kp.pad & kKinPosePlain) kin_flush<false, PIPE * kWave, 16>(buf, 17, 16, ncfg, T + cfg0 * 16, lane);      // wave-uniform
        else kin_flush<true, PIPE * kWave, 16>(buf, 17, 16, ncfg, T + cfg0 * 16, lane);
        __syncthreads();
    }
    if (WANT_J) {
#pragma unroll
        for (int r = 0; r < kWave / kJRound; ++r) {
            if (lane / kJRound == r) reg_stage_J<NJ>(jac, buf, lane % kJRound);
            __syncthreads();
            int rows = ncfg - r * kJRound;
            rows = rows < 0 ? 0 : (rows > kJRound ? kJRound : rows);
            kin_flush<true, PIPE * kJRound, W>(buf, W + 1, W, rows, J + (cfg0 + r * kJRound) * W, lane);
            __syncthreads();
        }
    }
}

// ONE tile per single-wave workgroup, no grid-stride loop: with a loop LICM hoists every segment's
// (loop-invariant) scalar loads into the preheader, where they overflow the SGPR file and come back
// as v_readlane pairs on each use.  The dispatcher balances the tiles instead.
// SIG != 0 (launch_reg: a built-in signature, no tool): every segment product is the exact specialisation of the general kernel's UNFUSED product
// for that segment's zeros and ones (kin_device.h: pose_mul_seg_sig, pose_seg_translate_sum) -- the same bits from fewer instructions, no 12-double
// segment loads, no descriptor branches, no fences; the q loads are issued together.  What that can buy is the launch's ramp, not its steady state,
// which the stores set (executed instruction counts, the N sweep and the A/B pairs: profiles/r07_kin_sig.txt).
template <int NJ, bool WANT_T, bool WANT_J, bool PACKED = false, SegSig SIG = 0>
__global__ __launch_bounds__(kWave, (NJ <= kRegMaxJoints ? RTB_REG_WAVES : 2)) void k_kin_reg(KinParams kp, DevChain dc, const double *__restrict__ q,
                                                  double *__restrict__ T, double *__restrict__ J)
{
    extern __shared__ __attribute__((aligned(16))) double buf[];
    // (the packed form writes ~30 KB runs per wave; the identity mapping the Hessian tile prefers was A/B'd for it in profiles/r05_* and not kept)
    reg_tile<NJ, WANT_T, WANT_J, PACKED, SIG>(kp, const_view(dc), q, T, J, buf, threadIdx.x, xcd_tile());
}
// float32 q, T, J (PACKED: [T | J] rows): the same tile, the same launch shape; only the widths of the row accesses differ (kin_tile.h)
template <int NJ, bool WANT_T, bool WANT_J, bool PACKED = false, SegSig SIG = 0>
__global__ __launch_bounds__(kWave, (NJ <= kRegMaxJoints ? RTB_REG_WAVES : 2)) void k_kin_reg_f32(KinParams kp, DevChain dc, const float *__restrict__ q,
                                                      float *__restrict__ T, float *__restrict__ J)
{
    extern __shared__ __attribute__((aligned(16))) double buf[];
    reg_tile<NJ, WANT_T, WANT_J, PACKED, SIG>(kp, const_view(dc), q, T, J, buf, threadIdx.x, xcd_tile());
}

static int g_hess_mode = 0;   // A/B knob (rtbhip_tune "hess_mode")

// ---------------------------------------------------------------- Hessian, register-resident (n <= 8)
// H is 48 n^2 bytes per configuration (2352 B for the Panda): the kernel is a pure HBM writer.  The
// first version wrote each lane's block with 8-byte stores at a 2352-byte stride (3.27 ms per 1e6
// Panda configurations, 9 % of the HBM peak); here the wave stages its 64 Jacobians in LDS once and
// every lane generates the 16-byte pieces of the tile's contiguous output run on the fly.
template <int NJ>
__global__ __launch_bounds__(kWave, (NJ <= kRegMaxJoints ? 2 : 1)) void k_kin_hess(KinParams kp, DevChain dc, const double *__restrict__ q,
                                                       double *__restrict__ H)
{
    extern __shared__ __attribute__((aligned(16))) double buf[];
    const ConstChain cv = const_view(dc);
    const int lane = threadIdx.x;
    const int64_t cfg0 = (int64_t)blockIdx.x * kWave;
    const int64_t left = kp.N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    constexpr int W = 6 * NJ;
    {
        Pose P;
        double jac[6 * NJ];
        reg_compute<NJ, true>(kp, cv, q, cfg0 + lane, P, jac);
        double *mine = buf + lane * (W + 1);
#pragma unroll
        for (int k = 0; k < W; ++k) mine[k] = jac[k];
    }
    __syncthreads();
    double *dst = H + cfg0 * (int64_t)(NJ * W);
    hessian_run<NJ>(buf, W + 1, ncfg, lane, [&](int f, double a, double b, bool both) {
        if (both) {
            typedef double v2d __attribute__((ext_vector_type(2)));
            v2d w = {a, b};
            __builtin_nontemporal_store(w, reinterpret_cast<v2d *>(dst + f));
        } else {
            __builtin_nontemporal_store(a, dst + f);
        }
    });
}

// The tile's Hessians from the lanes' finished Jacobians (registers): R rounds, in round r the 64/R lanes of group r
// expand theirs (compile-time indices) into whole (n,6,n) rows of the LDS tile, which the full wave writes as one
// contiguous run.  Shared by k_kin_hess_tile (J from the chain walk) and k_hess_from_jac (J supplied by the caller).
template <int NJ, int R>
__device__ __forceinline__ void hess_tile_emit(double (&jac)[6 * NJ], double *buf, int lane, int ncfg, double *__restrict__ Hrun)
{
    constexpr int HW = NJ * 6 * NJ, S = HW | 1, G = kWave / R;
    const int grp = lane / G;
    double *mine = buf + (lane - grp * G) * S;
    for (int r = 0; r < R; ++r) {
        const int cnt = ncfg - r * G < G ? ncfg - r * G : G;
        if (cnt <= 0) break;                                         // wave-uniform
        if (grp == r) {
            // the expansion must stay inside its round: hoisted out of the loop it would hold all 6 n^2 entries in registers
#pragma unroll
            for (int k = 0; k < 6 * NJ; ++k) asm volatile("" : "+v"(jac[k]));
            hessian_from_jacobian(NJ, [&](int k) { return jac[k]; }, [&](int idx, double v) { mine[idx] = v; });
        }
        __syncthreads();
        double *dst = Hrun + (int64_t)(r * G) * HW;
        flush_rows<HW>(buf, S, cnt, lane, [&](int f, double a, double b) {
            typedef double v2d __attribute__((ext_vector_type(2)));
            v2d w = {a, b};
            __builtin_nontemporal_store(w, reinterpret_cast<v2d *>(dst + f));
        });
        __syncthreads();
    }
}

// Variant B (A/B knob hess_mode = 1): every lane forms the (6,n) block H[j] of its OWN configuration in
// registers (static indexing, no per-entry LDS gathers), the wave transposes the 64 blocks through LDS and
// writes them as 64 segments of 48n bytes (2352-byte stride between configurations), one round per j.
// Hessian, tiled form (default): every lane keeps its finished Jacobian in registers; in R rounds a group of 64/R lanes
// expands its Hessians (compile-time indices: ~9 fp64 ops per (j, i) block instead of ~50 integer + select
// instructions per entry in hessian_run) into an LDS tile of whole (n,6,n) rows, which the full wave then writes as one
// contiguous run.  LDS per wave (64/R) x (6 n^2 + 1) doubles: n = 7, R = 8 -> 18.9 KB.
template <int NJ, int R>
__global__ __launch_bounds__(kWave, (NJ <= kRegMaxJoints && R >= 8 ? 2 : 1)) void k_kin_hess_tile(KinParams kp, DevChain dc, const double *__restrict__ q,
                                                                                               double *__restrict__ H)
{
    extern __shared__ __attribute__((aligned(16))) double buf[];
    const ConstChain cv = const_view(dc);
    const int lane = threadIdx.x;
    const int64_t cfg0 = (int64_t)blockIdx.x * kWave;     // (the XCD-contiguous mapping of k_kin_reg costs this kernel 3 %)
    const int64_t left = kp.N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    Pose P;
    double jac[6 * NJ];
    reg_compute<NJ, true>(kp, cv, q, cfg0 + lane, P, jac);
    hess_tile_emit<NJ, R>(jac, buf, lane, ncfg, H + cfg0 * (int64_t)(NJ * 6 * NJ));
}
template <int NJ, int R>
static hipError_t launch_hess_tile(dim3 grid, hipStream_t s, const KinParams &kp, const DevChain &dc, const double *q, double *H)
{
    const size_t lds = (size_t)(kWave / R) * ((NJ * 6 * NJ) | 1) * sizeof(double);
    auto k = k_kin_hess_tile<NJ, R>;
    if (lds > 48 * 1024) { hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(k, grid, dim3(kWave), lds, s, kp, dc, q, H);
    note_launch((int)grid.x, kWave, (int)lds);
    return hipGetLastError();
}
template <int NJ>
static hipError_t launch_hess_nj(dim3 grid, hipStream_t s, const KinParams &kp, const DevChain &dc, const double *q, double *H)
{
    // measured (Panda, 1e6, min of 10): R = 2 0.59 ms, R = 4 0.44 ms, R = 8 0.51 ms, R = 16 0.88 ms, hessian_run (mode 1) 0.61-0.64 ms
    if (g_hess_mode == 0) return launch_hess_tile<NJ, 4>(grid, s, kp, dc, q, H);
    if (g_hess_mode == 2) return launch_hess_tile<NJ, 8>(grid, s, kp, dc, q, H);
    const size_t lds = (size_t)kWave * (6 * NJ + 1) * sizeof(double);
    hipLaunchKernelGGL((k_kin_hess<NJ>), grid, dim3(kWave), lds, s, kp, dc, q, H);
    note_launch((int)grid.x, kWave, (int)lds);
    return hipGetLastError();
}

// ---------------------------------------------------------------- Hessian from a SUPPLIED Jacobian
// ETS_hessian0 / ETS_hessiane as the reference binds them take (ets, q, J, tool) and, when J is given, only run
// _ETS_hessian on it (core/fknm.cpp:583-783 -> core/methods.cpp:16-32): a pure function of J.  The tile's 64 Jacobians
// arrive as one contiguous run through LDS, every lane picks its own up into registers, then the same tile emission as
// k_kin_hess_tile.  Bytes: 48 n read + 48 n^2 written per Jacobian; HBM-bound.
template <int NJ, int R>
__global__ __launch_bounds__(kWave, 1) void k_hess_from_jac(const double *__restrict__ J, int64_t N, double *__restrict__ H)
{
    extern __shared__ __attribute__((aligned(16))) double buf[];
    constexpr int W = 6 * NJ;
    const int lane = threadIdx.x;
    const int64_t cfg0 = (int64_t)blockIdx.x * kWave;
    const int64_t left = N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    hj_load_tile(J + cfg0 * W, W, ncfg, buf, lane);
    __syncthreads();
    double jac[W];
    const double *mine = buf + lane * (W + 1);
#pragma unroll
    for (int k = 0; k < W; ++k) jac[k] = lane < ncfg ? mine[k] : 0.0;
    __syncthreads();
    hess_tile_emit<NJ, R>(jac, buf, lane, ncfg, H + cfg0 * (int64_t)(NJ * W));
}

// run-time n (chains of more than 10 joints): one lane per Jacobian, straight from and to global memory
__global__ __launch_bounds__(kWave) void k_hess_from_jac_any(int n, const double *__restrict__ J, int64_t N, double *__restrict__ H)
{
    const int64_t cfg = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (cfg >= N) return;
    const double *Jr = J + cfg * (int64_t)(6 * n);
    double *Hr = H + cfg * (int64_t)(6 * n * n);
    hessian_from_jacobian(n, [&](int k) { return Jr[k]; }, [&](int idx, double v) { Hr[idx] = v; });
}

template <int NJ>
static hipError_t launch_hess_from_jac_nj(dim3 grid, hipStream_t s, const double *J, int64_t N, double *H)
{
    constexpr int R = 4;
    const size_t a = (size_t)(kWave / R) * ((NJ * 6 * NJ) | 1), b = (size_t)kWave * (6 * NJ + 1);
    const size_t lds = (a > b ? a : b) * sizeof(double);
    auto k = k_hess_from_jac<NJ, R>;
    if (lds > 48 * 1024) { hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(k, grid, dim3(kWave), lds, s, J, N, H);
    note_launch((int)grid.x, kWave, (int)lds);
    return hipGetLastError();
}

int launch_hess_from_jac(int n, const double *J, int64_t N, double *H, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (n < 1 || n > RTBHIP_MAX_JOINTS) { set_error("hessian_from_jacobian: n must be 1..32"); return RTBHIP_ELIMIT; }
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("hessian_from_jacobian: batch too large for one launch"); return RTBHIP_ELIMIT; }
    dim3 grid((unsigned)tiles);
    hipError_t e = hipSuccess;
    switch (n) {
    case 1: e = launch_hess_from_jac_nj<1>(grid, s, J, N, H); break;
    case 2: e = launch_hess_from_jac_nj<2>(grid, s, J, N, H); break;
    case 3: e = launch_hess_from_jac_nj<3>(grid, s, J, N, H); break;
    case 4: e = launch_hess_from_jac_nj<4>(grid, s, J, N, H); break;
    case 5: e = launch_hess_from_jac_nj<5>(grid, s, J, N, H); break;
    case 6: e = launch_hess_from_jac_nj<6>(grid, s, J, N, H); break;
    case 7: e = launch_hess_from_jac_nj<7>(grid, s, J, N, H); break;
    case 8: e = launch_hess_from_jac_nj<8>(grid, s, J, N, H); break;
    case 9: e = launch_hess_from_jac_nj<9>(grid, s, J, N, H); break;
    case 10: e = launch_hess_from_jac_nj<10>(grid, s, J, N, H); break;
    default:
        hipLaunchKernelGGL(k_hess_from_jac_any, grid, dim3(kWave), 0, s, n, J, N, H);
        note_launch((int)grid.x, kWave, 0);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return hip_fail(e, "k_hess_from_jac launch");
    return RTBHIP_OK;
}

// ---------------------------------------------------------------- fknm.Angle_Axis, batched
// e[i] = angle_axis(Te[i or 0], Tep[i or 0]) (core/fknm.cpp:112-162 -> core/ik.cpp:241-286).  256 B in, 48 B out per
// pair; both tiles through LDS as contiguous runs; a broadcast operand (count 1) is read by every lane from the same
// 128 bytes.  LDS: 64 x 17 doubles per operand, the first re-used for the 64 x 7 staging of e.
// RPY = true: the same staging around servo_rpy_lane (p_servo's method "rpy", servo_device.h).
// SERVO (compile-time): the whole of tools/p_servo.py:46-117 in this launch -- after the error vector, arrived = sum|e| < threshold (one byte per
// pair, read before the gain touches e) and v = gain * e leaves in its place.  Before round 5 the wrapper ran two more elementwise kernels for that.
struct ServoTail { double gain[6]; double threshold; unsigned char *arrived; };
template <bool RPY, bool SERVO = false>
__global__ __launch_bounds__(kWave) void k_angle_axis(const double *__restrict__ Te, int te_each, const double *__restrict__ Tep, int tep_each,
                                                     int64_t N, double *__restrict__ e, ServoTail tail = ServoTail())
{
    __shared__ __attribute__((aligned(16))) double a[kWave * kAaStride];
    __shared__ __attribute__((aligned(16))) double b[kWave * kAaStride];
    const int lane = threadIdx.x;
    const int64_t cfg0 = (int64_t)xcd_tile() * kWave;
    const int64_t left = N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    {
        // both operand tiles' loads in flight together (16 x 16 B per lane), then the LDS writes (servo_device.h: aa_fetch_tile)
        AaTile ta, tb;
        aa_fetch_tile(te_each ? Te + cfg0 * 16 : Te, te_each ? ncfg : 1, lane, ta);
        aa_fetch_tile(tep_each ? Tep + cfg0 * 16 : Tep, tep_each ? ncfg : 1, lane, tb);
        aa_store_tile(ta, te_each ? ncfg : 1, a, lane);
        aa_store_tile(tb, tep_each ? ncfg : 1, b, lane);
    }
    __syncthreads();
    double te16[12], tep16[12];
    const int la = te_each ? (lane < ncfg ? lane : 0) : 0, lb = tep_each ? (lane < ncfg ? lane : 0) : 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) { te16[k] = a[la * kAaStride + k]; tep16[k] = b[lb * kAaStride + k]; }
    __syncthreads();
    if constexpr (RPY) servo_rpy_lane(te16, tep16, a + lane * 7);
    else aa_lane(te16, tep16, a + lane * 7);
    if constexpr (SERVO) {
        double *mine = a + lane * 7;
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) sum += fabs(mine[k]);                    // p_servo.py:113 `np.sum(np.abs(e)) < threshold`, on e itself
#pragma unroll
        for (int k = 0; k < 6; ++k) mine[k] = tail.gain[k] * mine[k];        // :108-111 v = k @ e (k = gain * eye(6) or diag(gain))
        if (lane < ncfg) tail.arrived[cfg0 + lane] = sum < tail.threshold ? 1 : 0;
    }
    __syncthreads();
    kin_flush(a, 7, 6, ncfg, e + cfg0 * 6, lane);
}

int launch_p_servo(const double *Te, int64_t nTe, const double *Tep, int64_t nTep, int64_t N, int method, const double *gain6, double threshold, double *v,
                   unsigned char *arrived, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("p_servo: batch too large for one launch"); return RTBHIP_ELIMIT; }
    ServoTail t;
    for (int k = 0; k < 6; ++k) t.gain[k] = gain6[k];
    t.threshold = threshold; t.arrived = arrived;
    if (method == 1) hipLaunchKernelGGL((k_angle_axis<true, true>), dim3((unsigned)tiles), dim3(kWave), 0, s, Te, nTe == N ? 1 : 0, Tep, nTep == N ? 1 : 0, N, v, t);
    else hipLaunchKernelGGL((k_angle_axis<false, true>), dim3((unsigned)tiles), dim3(kWave), 0, s, Te, nTe == N ? 1 : 0, Tep, nTep == N ? 1 : 0, N, v, t);
    note_launch((int)tiles, kWave, (int)(2 * kWave * kAaStride * sizeof(double)));
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return hip_fail(err, "k_angle_axis (servo) launch");
    return RTBHIP_OK;
}

int launch_angle_axis(const double *Te, int64_t nTe, const double *Tep, int64_t nTep, int64_t N, double *e, hipStream_t s, int method)
{
    if (N == 0) return RTBHIP_OK;
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("angle_axis: batch too large for one launch"); return RTBHIP_ELIMIT; }
    if (method == 1)
        hipLaunchKernelGGL((k_angle_axis<true, false>), dim3((unsigned)tiles), dim3(kWave), 0, s, Te, nTe == N ? 1 : 0, Tep,
                           nTep == N ? 1 : 0, N, e, ServoTail());
    else
        hipLaunchKernelGGL((k_angle_axis<false, false>), dim3((unsigned)tiles), dim3(kWave), 0, s, Te, nTe == N ? 1 : 0, Tep,
                           nTep == N ? 1 : 0, N, e, ServoTail());
    note_launch((int)tiles, kWave, (int)(2 * kWave * kAaStride * sizeof(double)));
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return hip_fail(err, "k_angle_axis launch");
    return RTBHIP_OK;
}

// ---------------------------------------------------------------- differential-kinematics consumers (n <= 8)
static int g_diff_sig = 1;     // rtbhip_tune("diff_sig", 0): k_kin_diff never takes a robot's structure instantiation (A/B, tests)
template <int NJ>
static hipError_t launch_diff_nj(int mode, dim3 grid, size_t lds, hipStream_t s, const KinParams &kp, const DevChain &dc,
                                 int axes, const double *q, const double *qd, double *out)
{
    if (mode == kDiffJdot) hipLaunchKernelGGL((k_kin_diff<NJ, kDiffJdot>), grid, dim3(kWave), lds, s, kp, dc, axes, q, qd, out);
    else if (mode == kDiffManip) hipLaunchKernelGGL((k_kin_diff<NJ, kDiffManip>), grid, dim3(kWave), lds, s, kp, dc, axes, q, qd, out);
    else if (mode == kDiffAnalytical) hipLaunchKernelGGL((k_kin_diff<NJ, kDiffAnalytical>), grid, dim3(kWave), lds, s, kp, dc, axes, q, qd, out);
    else if (mode == kDiffAnalyticalDot) hipLaunchKernelGGL((k_kin_diff<NJ, kDiffAnalyticalDot>), grid, dim3(kWave), lds, s, kp, dc, axes, q, qd, out);
    else hipLaunchKernelGGL((k_kin_diff<NJ, kDiffJacobm>), grid, dim3(kWave), lds, s, kp, dc, axes, q, qd, out);
    return hipGetLastError();
}

int launch_kin_diff(const Chain *c, const DevChain &dc, int mode, int axes, const double *q, const double *qd, int64_t N,
                    const Affine &tool, int frame, double *out, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (c->n < 1 || c->n > RTBHIP_MAX_JOINTS) { set_error("jacob_dot/manipulability/jacobm/jacob0_analytical: chains of 1..RTBHIP_MAX_JOINTS joints"); return RTBHIP_ELIMIT; }
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("jacob_dot/manipulability/jacobm: batch too large for one launch"); return RTBHIP_ELIMIT; }
    KinParams kp;
    kp.n = c->n; kp.qw = c->q_width; kp.stride = kin_stride(c->n); kp.frame = frame; kp.has_base = 0; kp.pad = 0; kp.N = N;
    for (int i = 0; i < 12; i++) kp.base[i] = 0.0;
    chain_tail(c, tool, kp.tail);
    const size_t lds = (size_t)reg_lds_doubles(c->n) * sizeof(double);
    dim3 grid((unsigned)tiles);
    hipError_t e = hipSuccess;
    // a structure instantiation of the walk for THIS robot (diff_kernel.h: k_kin_diff<NJ, MODE, SIG>), compiled at run time on first use; the general
    // kernel below serves until the code object is there and returns the same bits.  rtbhip_tune("diff_sig", 0): never.
    if (g_diff_sig && c->n <= kRegMaxJoints && !tool.used && mode != kDiffAnalyticalDot && jit_enabled()) {
        bool plain = true;
        for (int j = 0; j < c->n; ++j) plain = plain && !jm_prismatic(c->jmeta[j]) && !jm_flip(c->jmeta[j]);
        const SegSig sig = plain ? chain_signature(c->jmeta.data(), c->n) : 0;
        if (sig) {
            const int m = mode == kDiffJdot ? kDiffJdot : (mode == kDiffManip ? kDiffManip : (mode == kDiffAnalytical ? kDiffAnalytical : kDiffJacobm));
            if (hipFunction_t f = c->jit.get("diff_kernel.h", 48 + m, [&] { return "rtbhip::k_kin_diff<" + std::to_string(c->n) + ", " + std::to_string(m) + ", " + jit_hex(sig) + ">"; })) {
                void *args[] = {(void *)&kp, (void *)&dc, (void *)&axes, (void *)&q, (void *)&qd, (void *)&out};
                const int rc = jit_launch(f, grid, dim3(kWave), lds, s, args);
                if (rc != RTBHIP_OK) return rc;
                note_launch((int)grid.x, kWave, (int)lds);
                return RTBHIP_OK;
            }
        }
    }
    if (c->n > kDiffMax) {
        // a joint count without a built-in instantiation: the same k_kin_diff template, instantiated at run time (jit.cpp; seconds to a minute on first
        // use, then a file read).  The reference's loops take any n (robot/Robot.py:964-1235, robot/ETS.py:1687-1819).
        const int m = mode == kDiffJdot ? kDiffJdot : (mode == kDiffManip ? kDiffManip : (mode == kDiffAnalytical ? kDiffAnalytical : (mode == kDiffAnalyticalDot ? kDiffAnalyticalDot : kDiffJacobm)));
        hipFunction_t f = c->jit.get_wait("diff_kernel.h", 32 + m, [&] { return "rtbhip::k_kin_diff<" + std::to_string(c->n) + ", " + std::to_string(m) + ">"; });
        if (!f) return RTBHIP_ELIMIT;                         // (rtbhip_last_error says why: no hipRTC on this box, or the compiler's message)
        void *args[] = {(void *)&kp, (void *)&dc, (void *)&axes, (void *)&q, (void *)&qd, (void *)&out};
        const int rc = jit_launch(f, grid, dim3(kWave), lds, s, args);
        if (rc != RTBHIP_OK) return rc;
        note_launch((int)grid.x, kWave, (int)lds);
        return RTBHIP_OK;
    }
    switch (c->n) {
    case 1: e = launch_diff_nj<1>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 2: e = launch_diff_nj<2>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 3: e = launch_diff_nj<3>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 4: e = launch_diff_nj<4>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 5: e = launch_diff_nj<5>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 6: e = launch_diff_nj<6>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 7: e = launch_diff_nj<7>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 8: e = launch_diff_nj<8>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 9: e = launch_diff_nj<9>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 10: e = launch_diff_nj<10>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    // 11..16: one wave per SIMD, the longer ones with some scratch -- served, not fast
    case 11: e = launch_diff_nj<11>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 12: e = launch_diff_nj<12>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 13: e = launch_diff_nj<13>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 14: e = launch_diff_nj<14>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    case 15: e = launch_diff_nj<15>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    default: e = launch_diff_nj<16>(mode, grid, lds, s, kp, dc, axes, q, qd, out); break;
    }
    note_launch((int)grid.x, kWave, (int)lds);
    if (e != hipSuccess) return hip_fail(e, "k_kin_diff launch");
    return RTBHIP_OK;
}

namespace {
int g_coalesced = 1;   // tuning knobs (rtbhip_tune)
int g_tiles_per_wave = 1;
int g_use_reg = 1;
int g_kin_sig = 1;     // rtbhip_tune("kin_sig", 0): k_kin_reg never takes a structure signature's instantiation (A/B, tests)
}  // namespace

void kin_tune(const char *key, int value)
{
    std::string k(key);
    if (k == "coalesced") g_coalesced = value;
    if (k == "tiles_per_wave") g_tiles_per_wave = value < 1 ? 1 : value;
    if (k == "reg") g_use_reg = value;
    if (k == "hess_mode") g_hess_mode = value;
    if (k == "diff_sig") g_diff_sig = value != 0;
    if (k == "kin_sig") g_kin_sig = value != 0;
}

template <bool WT, bool WJ, bool WH, class S>
static hipError_t launch_variant(bool coalesced, dim3 grid, size_t lds, hipStream_t s, const KinParams &kp,
                                 const DevChain &ops, const S *q, S *T, S *J, double *H)
{
    if constexpr (sizeof(S) == 4) {
        static_assert(!WH, "the Hessian is fp64 only");
        auto k = k_kin_f32<WT, WJ>;
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k, grid, dim3(kWave), lds, s, kp, ops, q, T, J);
    } else if (coalesced) {
        auto k = k_kin<WT, WJ, WH, true>;
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k, grid, dim3(kWave), lds, s, kp, ops, q, T, J, H);
    } else {
        auto k = k_kin<WT, WJ, WH, false>;
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k, grid, dim3(kWave), lds, s, kp, ops, q, T, J, H);
    }
    return hipGetLastError();
}

// The signature of a chain that k_kin_reg has a built-in instantiation for (kin_reg.h: kSig*), else 0.  A tool is folded into the tail on the host
// (chain_tail) while a signature's last segment is the table's own: with a tool the general kernel serves.  A base is applied at staging: no matter.
static SegSig kin_reg_sig(const Chain *c, const Affine &tool)
{
    if (!g_kin_sig || tool.used || c->n < 6 || c->n > 7 || !jit_builtin_enabled()) return 0;
    for (int j = 0; j < c->n; ++j)
        if (jm_prismatic(c->jmeta[j]) || jm_flip(c->jmeta[j])) return 0;
    const SegSig sig = chain_signature(c->jmeta.data(), c->n);
    if (c->n == 7 && (sig == kSigPandaETS || sig == kSigPandaURDF)) return sig;
    if (c->n == 6 && sig == kSigUR) return sig;
    return 0;
}
// S = double: k_kin_reg, S = float: k_kin_reg_f32
template <int NJ, bool WT, bool WJ, bool PACKED, SegSig SIG, class S>
static void launch_reg_one(dim3 grid, size_t lds, hipStream_t s, const KinParams &kp, const DevChain &dc, const S *q, S *T, S *J)
{
    if constexpr (sizeof(S) == 8) hipLaunchKernelGGL((k_kin_reg<NJ, WT, WJ, PACKED, SIG>), grid, dim3(kWave), lds, s, kp, dc, q, T, J);
    else hipLaunchKernelGGL((k_kin_reg_f32<NJ, WT, WJ, PACKED, SIG>), grid, dim3(kWave), lds, s, kp, dc, q, T, J);
}
template <int NJ, SegSig SIG, class S>
static hipError_t launch_reg_sig(dim3 grid, size_t lds, hipStream_t s, const KinParams &kp, const DevChain &dc, const S *q, S *T, S *J)
{
    if (T && J) launch_reg_one<NJ, true, true, false, SIG>(grid, lds, s, kp, dc, q, T, J);
    else if (T) launch_reg_one<NJ, true, false, false, SIG>(grid, lds, s, kp, dc, q, T, J);
    else launch_reg_one<NJ, false, true, false, SIG>(grid, lds, s, kp, dc, q, T, J);
    return hipGetLastError();
}
template <int NJ, class S>
static hipError_t launch_reg(dim3 grid, size_t lds, hipStream_t s, const KinParams &kp, const DevChain &dc, const S *q, S *T, S *J, SegSig sig)
{
    if constexpr (NJ == 7) {
        if (sig == kSigPandaETS) return launch_reg_sig<7, kSigPandaETS>(grid, lds, s, kp, dc, q, T, J);
        if (sig == kSigPandaURDF) return launch_reg_sig<7, kSigPandaURDF>(grid, lds, s, kp, dc, q, T, J);
    }
    if constexpr (NJ == 6) {
        if (sig == kSigUR) return launch_reg_sig<6, kSigUR>(grid, lds, s, kp, dc, q, T, J);
    }
    return launch_reg_sig<NJ, 0>(grid, lds, s, kp, dc, q, T, J);
}

template <int NJ, SegSig SIG, class S>
static hipError_t launch_reg_packed_sig(dim3 grid, size_t lds, hipStream_t s, const KinParams &kp, const DevChain &dc, const S *q, S *TJ)
{
    launch_reg_one<NJ, true, true, true, SIG>(grid, lds, s, kp, dc, q, TJ, (S *)nullptr);
    return hipGetLastError();
}
template <int NJ, class S>
static hipError_t launch_reg_packed(dim3 grid, size_t lds, hipStream_t s, const KinParams &kp, const DevChain &dc, const S *q, S *TJ, SegSig sig)
{
    if constexpr (NJ == 7) {
        if (sig == kSigPandaETS) return launch_reg_packed_sig<7, kSigPandaETS>(grid, lds, s, kp, dc, q, TJ);
        if (sig == kSigPandaURDF) return launch_reg_packed_sig<7, kSigPandaURDF>(grid, lds, s, kp, dc, q, TJ);
    }
    if constexpr (NJ == 6) {
        if (sig == kSigUR) return launch_reg_packed_sig<6, kSigUR>(grid, lds, s, kp, dc, q, TJ);
    }
    return launch_reg_packed_sig<NJ, 0>(grid, lds, s, kp, dc, q, TJ);
}

// rtbhip_fkine_jacob_packed: rows [T (16, base applied) | J (6n)] of ONE (N, 16 + 6n) array -- a single write stream (SURVEY 8e's T||J message)
// (S: the rows' storage type, as launch_kin_s below)
template <class S>
static int launch_kin_packed_s(const Chain *c, const DevChain &ops, const S *q, int64_t N, const Affine &base,
                               const Affine &tool, int frame, S *TJ, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    KinParams kp;
    kp.n = c->n; kp.qw = c->q_width; kp.stride = kin_stride(c->n); kp.frame = frame; kp.has_base = base.used;
    kp.pad = kKinPacked; kp.N = N;
    for (int i = 0; i < 12; i++) kp.base[i] = base.v[i];
    chain_tail(c, tool, kp.tail);
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("fkine_jacob_packed: batch too large for one launch"); return RTBHIP_ELIMIT; }
    dim3 grid((unsigned)tiles);
    if (g_use_reg && c->n >= 1 && c->n <= kKinRegMax) {
        const size_t rl = (size_t)reg_lds_doubles_packed(c->n) * sizeof(double);
        const SegSig sig = kin_reg_sig(c, tool);
        hipError_t e = hipSuccess;
        switch (c->n) {
        case 1: e = launch_reg_packed<1>(grid, rl, s, kp, ops, q, TJ, sig); break;
        case 2: e = launch_reg_packed<2>(grid, rl, s, kp, ops, q, TJ, sig); break;
        case 3: e = launch_reg_packed<3>(grid, rl, s, kp, ops, q, TJ, sig); break;
        case 4: e = launch_reg_packed<4>(grid, rl, s, kp, ops, q, TJ, sig); break;
        case 5: e = launch_reg_packed<5>(grid, rl, s, kp, ops, q, TJ, sig); break;
        case 6: e = launch_reg_packed<6>(grid, rl, s, kp, ops, q, TJ, sig); break;
        case 7: e = launch_reg_packed<7>(grid, rl, s, kp, ops, q, TJ, sig); break;
        case 8: e = launch_reg_packed<8>(grid, rl, s, kp, ops, q, TJ, sig); break;
        case 9: e = launch_reg_packed<9>(grid, rl, s, kp, ops, q, TJ, sig); break;
        default: e = launch_reg_packed<10>(grid, rl, s, kp, ops, q, TJ, sig); break;
        }
        note_launch((int)grid.x, kWave, (int)rl);
        if (e != hipSuccess) return hip_fail(e, "k_kin_reg (packed) launch");
        return RTBHIP_OK;
    }
    const size_t lds = kin_lds_bytes(c->n, c->q_width) + (size_t)kWave * 17 * sizeof(double);
    if (lds > 160 * 1024) { set_error("chain too large for the per-wave LDS staging"); return RTBHIP_ELIMIT; }
    hipError_t e = launch_variant<true, true, false>(true, grid, lds, s, kp, ops, q, TJ, TJ, nullptr);
    note_launch((int)grid.x, kWave, (int)lds);
    if (e != hipSuccess) return hip_fail(e, "k_kin (packed) launch");
    return RTBHIP_OK;
}
int launch_kin_packed(const Chain *c, const DevChain &ops, const double *q, int64_t N, const Affine &base,
                      const Affine &tool, int frame, double *TJ, hipStream_t s)
{
    return launch_kin_packed_s(c, ops, q, N, base, tool, frame, TJ, s);
}
int launch_kin_packed_f32(const Chain *c, const DevChain &ops, const float *q, int64_t N, const Affine &base,
                          const Affine &tool, int frame, float *TJ, hipStream_t s)
{
    return launch_kin_packed_s(c, ops, q, N, base, tool, frame, TJ, s);
}

// S: the storage type of q, T and J -- double (every entry point of the fp64 ABI), or float (rtbhip_fkine_jacob_f32; H must then be NULL).  Same
// dispatch for both: a joint count of 1..kKinRegMax takes the register-resident tile (k_kin_reg / k_kin_reg_f32), a longer chain the run-time-n
// tile (k_kin / k_kin_f32), with the same grids and the same LDS requests -- the tiles are fp64 in both forms.
template <class S>
static int launch_kin_s(const Chain *c, const DevChain &ops, const S *q, int64_t N, const Affine &base,
                        const Affine &tool, int frame, S *T, S *J, double *H, hipStream_t s)
{
    constexpr bool kF64 = sizeof(S) == 8;
    if (N == 0) return RTBHIP_OK;
    KinParams kp;
    kp.n = c->n;
    kp.qw = c->q_width;
    kp.stride = kin_stride(c->n);
    kp.frame = frame;
    kp.has_base = base.used;
    kp.pad = (T && J && !H && (long long)N * 16 * (long long)sizeof(S) <= kPoseCacheBytes) ? kKinPosePlain : 0;      // (see the store policy at the top of this file)
    kp.N = N;
    for (int i = 0; i < 12; i++) kp.base[i] = base.v[i];
    chain_tail(c, tool, kp.tail);
    const int64_t tiles = (N + kWave - 1) / kWave;
    int64_t g = (tiles + g_tiles_per_wave - 1) / g_tiles_per_wave;
    if (g > 0x7fffffff) g = 0x7fffffff;
    dim3 grid((unsigned)g);
    if constexpr (kF64) {
    if (g_use_reg && H && !T && !J && c->n >= 1 && c->n <= kKinRegMax && tiles <= 0x7fffffff) {
        grid = dim3((unsigned)tiles);
        hipError_t e = hipSuccess;
        switch (c->n) {
        case 1: e = launch_hess_nj<1>(grid, s, kp, ops, q, H); break;
        case 2: e = launch_hess_nj<2>(grid, s, kp, ops, q, H); break;
        case 3: e = launch_hess_nj<3>(grid, s, kp, ops, q, H); break;
        case 4: e = launch_hess_nj<4>(grid, s, kp, ops, q, H); break;
        case 5: e = launch_hess_nj<5>(grid, s, kp, ops, q, H); break;
        case 6: e = launch_hess_nj<6>(grid, s, kp, ops, q, H); break;
        case 7: e = launch_hess_nj<7>(grid, s, kp, ops, q, H); break;
        case 8: e = launch_hess_nj<8>(grid, s, kp, ops, q, H); break;
        case 9: e = launch_hess_nj<9>(grid, s, kp, ops, q, H); break;
        default: e = launch_hess_nj<10>(grid, s, kp, ops, q, H); break;
        }
        if (e != hipSuccess) return hip_fail(e, "k_kin_hess launch");
        return RTBHIP_OK;
    }
    }
    if (g_use_reg && !H && c->n >= 1 && c->n <= kKinRegMax && tiles <= 0x7fffffff) {
        grid = dim3((unsigned)tiles);
        // fkine alone stages only the 64 x 17 pose tile (8.7 KB): with the Jacobian's 32 x (6n + 1) rounds left out of the request more waves fit a CU
        const size_t rl = (size_t)(J ? reg_lds_doubles(c->n) : kWave * 17) * sizeof(double);
        const SegSig sig = kin_reg_sig(c, tool);
        hipError_t e = hipSuccess;
        switch (c->n) {
        case 1: e = launch_reg<1>(grid, rl, s, kp, ops, q, T, J, sig); break;
        case 2: e = launch_reg<2>(grid, rl, s, kp, ops, q, T, J, sig); break;
        case 3: e = launch_reg<3>(grid, rl, s, kp, ops, q, T, J, sig); break;
        case 4: e = launch_reg<4>(grid, rl, s, kp, ops, q, T, J, sig); break;
        case 5: e = launch_reg<5>(grid, rl, s, kp, ops, q, T, J, sig); break;
        case 6: e = launch_reg<6>(grid, rl, s, kp, ops, q, T, J, sig); break;
        case 7: e = launch_reg<7>(grid, rl, s, kp, ops, q, T, J, sig); break;
        case 8: e = launch_reg<8>(grid, rl, s, kp, ops, q, T, J, sig); break;
        case 9: e = launch_reg<9>(grid, rl, s, kp, ops, q, T, J, sig); break;
        default: e = launch_reg<10>(grid, rl, s, kp, ops, q, T, J, sig); break;
        }
        note_launch((int)grid.x, kWave, (int)rl);
        if (e != hipSuccess) return hip_fail(e, "k_kin_reg launch");
        return RTBHIP_OK;
    }
    const size_t lds = kin_lds_bytes(c->n, c->q_width);
    if (lds > 160 * 1024) { set_error("chain too large for the per-wave LDS staging"); return RTBHIP_ELIMIT; }
    const bool co = g_coalesced != 0;
    hipError_t e;
    const bool wt = T != nullptr, wj = J != nullptr, wh = H != nullptr;
    if (wt && wj && !wh) e = launch_variant<true, true, false>(co, grid, lds, s, kp, ops, q, T, J, H);
    else if (wt && !wj && !wh) e = launch_variant<true, false, false>(co, grid, lds, s, kp, ops, q, T, J, H);
    else if (!wt && wj && !wh) e = launch_variant<false, true, false>(co, grid, lds, s, kp, ops, q, T, J, H);
    else if (kF64 && !wt && !wj && wh) { if constexpr (kF64) e = launch_variant<false, false, true>(co, grid, lds, s, kp, ops, q, T, J, H); }
    else if (kF64 && wt && wj && wh) { if constexpr (kF64) e = launch_variant<true, true, true>(co, grid, lds, s, kp, ops, q, T, J, H); }
    else { set_error("launch_kin: unsupported output combination"); return RTBHIP_EINVAL; }
    note_launch((int)grid.x, kWave, (int)lds);
    if (e != hipSuccess) return hip_fail(e, "k_kin launch");
    return RTBHIP_OK;
}
int launch_kin(const Chain *c, const DevChain &ops, const double *q, int64_t N, const Affine &base,
               const Affine &tool, int frame, double *T, double *J, double *H, hipStream_t s)
{
    return launch_kin_s(c, ops, q, N, base, tool, frame, T, J, H, s);
}
int launch_kin_f32(const Chain *c, const DevChain &ops, const float *q, int64_t N, const Affine &base,
                   const Affine &tool, int frame, float *T, float *J, hipStream_t s)
{
    return launch_kin_s(c, ops, q, N, base, tool, frame, T, J, (double *)nullptr, s);
}

// ---------------------------------------------------------------- mixed fleet (BASELINE config 5)
// One launch walks up to kFleetMax different chains, each with its own batch: the global tile index
// is mapped to (chain, local tile) by a scan over the per-chain first-tile table (wave-uniform, in
// kernarg => SGPRs); chain length, joint count and LDS row stride are then run-time values of that
// block.  Same phases as k_kin.
constexpr int kFleetMax = 32;
struct FleetArgs {
    FleetEntry e[kFleetMax];
    int32_t count, frame;
    int64_t tiles;
    int64_t tile_base;   // first global tile of this launch (launches are chunked at 2^31-1 workgroups)
};

// One tile per workgroup (no grid-stride loop, as k_kin_reg).  Three launch classes, because registers and
// dynamic LDS are per-kernel / per-launch quantities: CLS 0 chains of 1..8 joints (register-resident tile, 3
// waves per SIMD), CLS 1 chains of 9..10 joints (register-resident, 2 waves per SIMD), CLS 2 longer chains
// (LDS tile).  Inside a class the joint count of a tile is wave-uniform: a switch picks the tile body.
template <int CLS, bool PACKED = false>
__global__ __launch_bounds__(kWave, (CLS == 0 ? RTB_REG_WAVES : 2)) void k_fleet(FleetArgs fa)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t gt = (int64_t)blockIdx.x + fa.tile_base;
    int ci = 0;
    for (int i = 1; i < fa.count; ++i)
        if (gt >= fa.e[i].tile0) ci = i;
    const FleetEntry &fe = fa.e[ci];
    KinParams kp;
    kp.n = fe.n; kp.qw = fe.q_width; kp.stride = fe.stride;
    kp.frame = fa.frame; kp.has_base = 0; kp.pad = PACKED ? kKinPacked : 0; kp.N = fe.N;
    const ConstChain ops = const_view(fe.dc);
    for (int k = 0; k < 9; ++k) kp.tail[k] = ops.seg[fe.n].r[k];
    for (int k = 0; k < 3; ++k) kp.tail[9 + k] = ops.seg[fe.n].t[k];
    // The chain's tiles are dealt to the XCDs as a launch of its own would deal them (trig.h: xcd_tile_of -- XCD x walks the x-th contiguous
    // eighth of THIS chain's tiles; the hardware's round-robin is by global workgroup id, a fixed rotation of the XCD labels per chain): 1 % on the
    // 16-arm fleet (1.391 -> 1.378 ms, profiles/r05_s_fleet_xcd_ab.txt).  (Its chains launched one by one in a loop take 1.196 ms -- but only because
    // each call then rewrites the SAME 128 MB pose array, which the memory-side cache absorbs (store policy above); a fleet step writes 2 GB of poses
    // once: it streams, at 0.72-0.73 of the HBM roof against 0.745 for a plain fill of the same bytes: profiles/r05_r_fleet_probe.jsonl.)
    const int64_t local = gt - fe.tile0, ctiles = (fe.N + kWave - 1) / kWave;
    const int64_t tile = (ctiles <= 0x7fffffff) ? (int64_t)xcd_tile_of((unsigned)ctiles, (unsigned)local) : local;
    if (CLS == 0) {
        // (PIPE = 0: the unrolled flush in all ten tiles of this kernel cost it up to 28 VGPRs -- 165 -> 193, a wave per SIMD; it keeps the rolled one)
        switch (fe.n) {
        case 1: reg_tile<1, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile); return;
        case 2: reg_tile<2, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile); return;
        case 3: reg_tile<3, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile); return;
        case 4: reg_tile<4, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile); return;
        case 5: reg_tile<5, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile); return;
        case 6: reg_tile<6, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile); return;
        case 7: reg_tile<7, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile); return;
        default: reg_tile<8, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile); return;
        }
    } else if (CLS == 1) {
        if (fe.n == 9) reg_tile<9, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile);
        else reg_tile<10, true, true, PACKED, 0, 0>(kp, ops, fe.q, fe.T, fe.J, lds, lane, tile);
        return;
    }
    double *rows = lds;
    double *qs = lds + kWave * kp.stride;
    const int64_t cfg0 = tile * kWave, cfg = cfg0 + lane;
    const int64_t left = kp.N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    const int W = 6 * kp.n;
    kin_load_q(kp, fe.q, cfg, lane, qs);
    Pose P;
    kin_walk<true>(kp, ops, lane, qs, rows, P);
    if (PACKED) {
        double *rowsT = qs + kWave * kp.qw;
        pose_store16(P, [&](int k, double v) { rowsT[lane * 17 + k] = v; });
        __syncthreads();
        kin_flush_packed(rowsT, rows, kp.stride, W, ncfg, fe.T + cfg0 * (16 + W), lane);
        return;
    }
    __syncthreads();
    kin_flush(rows, kp.stride, W, ncfg, fe.J + cfg0 * W, lane);
    __syncthreads();
    kin_stage_T(kp, lane, rows, P);
    __syncthreads();
    kin_flush(rows, kp.stride, 16, ncfg, fe.T + cfg0 * 16, lane);
}

// Dynamic LDS and the register budget are per-launch quantities, so a mixed fleet is walked as (at most)
// three launches, one per class -- a single launch capped every workgroup at 4 per CU (2.32 vs 1.57 ms for the
// 16-arm fleet of BASELINE config 5).
static int fleet_class_of(int n) { return n <= kRegMaxJoints ? 0 : (n <= kKinRegMax ? 1 : 2); }
static int launch_fleet_class(int cls, const std::vector<FleetEntry> &entries, int frame, hipStream_t s, bool packed);
int launch_fleet(const std::vector<FleetEntry> &all, int frame, hipStream_t s, bool packed)
{
    std::vector<FleetEntry> by[3];
    for (const FleetEntry &e : all) by[fleet_class_of(e.n)].push_back(e);
    for (int c = 0; c < 3; ++c)
        if (!by[c].empty()) { int rc = launch_fleet_class(c, by[c], frame, s, packed); if (rc != RTBHIP_OK) return rc; }
    return RTBHIP_OK;
}

template <bool PACKED>
static void fleet_go(int cls, unsigned g, size_t lds, hipStream_t s, const FleetArgs &fa)
{
    if (cls == 0) hipLaunchKernelGGL((k_fleet<0, PACKED>), dim3(g), dim3(kWave), lds, s, fa);
    else if (cls == 1) hipLaunchKernelGGL((k_fleet<1, PACKED>), dim3(g), dim3(kWave), lds, s, fa);
    else hipLaunchKernelGGL((k_fleet<2, PACKED>), dim3(g), dim3(kWave), lds, s, fa);
}
template <bool PACKED>
static const void *fleet_fn(int cls)
{
    return cls == 0 ? (const void *)k_fleet<0, PACKED> : (cls == 1 ? (const void *)k_fleet<1, PACKED> : (const void *)k_fleet<2, PACKED>);
}

static int launch_fleet_class(int cls, const std::vector<FleetEntry> &entries, int frame, hipStream_t s, bool packed)
{
    for (size_t first = 0; first < entries.size(); first += kFleetMax) {
        FleetArgs fa;
        std::memset(&fa, 0, sizeof fa);
        fa.count = (int)std::min<size_t>(kFleetMax, entries.size() - first);
        fa.frame = frame;
        size_t lds = 0;
        int64_t tiles = 0;
        for (int i = 0; i < fa.count; i++) {
            fa.e[i] = entries[first + i];
            fa.e[i].stride = kin_stride(fa.e[i].n);
            fa.e[i].tile0 = tiles;
            tiles += (fa.e[i].N + kWave - 1) / kWave;
            lds = std::max(lds, cls < 2 ? (size_t)(packed ? reg_lds_doubles_packed(fa.e[i].n) : reg_lds_doubles(fa.e[i].n)) * sizeof(double)
                                        : kin_lds_bytes(fa.e[i].n, fa.e[i].q_width) + (packed ? (size_t)kWave * 17 * sizeof(double) : 0));
        }
        fa.tiles = tiles;
        if (lds > 160 * 1024) { set_error("fleet: chain too large for LDS staging"); return RTBHIP_ELIMIT; }
        const void *kfn = packed ? fleet_fn<true>(cls) : fleet_fn<false>(cls);
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return hip_fail(e, "k_fleet attr");
        }
        for (int64_t t0 = 0; t0 < tiles; t0 += 0x7fffffff) {
            const int64_t g = std::min<int64_t>(0x7fffffff, tiles - t0);
            fa.tile_base = t0;
            if (packed) fleet_go<true>(cls, (unsigned)g, lds, s, fa); else fleet_go<false>(cls, (unsigned)g, lds, s, fa);
            note_launch((int)g, kWave, (int)lds);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return hip_fail(e, "k_fleet launch");
        }
    }
    return RTBHIP_OK;
}

// ---------------------------------------------------------------- vector-Jacobian products of fkine / jacob0 (the backward pass of rtbhip/autograd.py)
// Given the gradients gT (N,4,4; bottom row ignored) and gJ (N,6,n) of a scalar loss with respect to T = base * P(q) and J = jacob0(q), the kernels
// below return gq (N, q_width), gq[k] = sum gT dT/dq_k + sum gJ dJ/dq_k.  No reference counterpart: the reference has no derivative of a loss; what
// is differentiated is _ETS_fkine (core/methods.cpp:318-352) and _ETS_jacob0 (:112-207), whose derivative with respect to q is _ETS_hessian (:16-32).
//   fkine   dP/dq_k is the Jacobian column acting on P: dR/dq_k = [w_k]x R, dp/dq_k = v_k, so the pose term is
//               gq_k = v_k . g_p + w_k . m,     g_p = translation column of B^T gT,   m = sum_c R_c x (B^T gT)_c     (one 6-vector per row)
//   jacob0  dJ[:,c]/dq_k = (w_k x v_c ; w_k x w_c) for k <= c and (w_c x v_k ; 0) for k > c (methods.cpp:16-32), so with a . (b x c) = b . (c x a)
//               gq_k = w_k . S_k + v_k . A_k,   S_k = sum_{c >= k} (v_c x gv_c + w_c x gw_c),   A_k = sum_{c < k} gv_c x w_c
//           one suffix and one prefix running sum over the columns: O(n), the (n,6,n) Hessian is never formed.
// Prismatic joints (w = 0, v = z) and flipped joints (the walk negated the column) need nothing extra: the finished columns carry both.
// Every sum of two products is written out (kin_device.h: mix_pp and friends).
// (vjp_pose_pullback, the pull-back of gT onto (g_p ; m): kin_vjp.h)

// The contraction.  J(r n + c) / G(r n + c): entry (r, c) of the row's finished Jacobian / of gJ; w = (g_p ; m) of the pose term (zeros without gT);
// acc(k, x): gq_k += x (the receiver starts at zero; two joints may share a q column).  n is a compile-time constant in the register tile (the
// loops unroll, every index is static) and a run-time value in k_vjp_from_jac_any.
template <bool WANT_GJ, class JGet, class GGet, class Acc>
RTB_HD void vjp_contract(int n, const double (&w)[6], JGet J, GGet G, Acc acc)
{
#pragma clang fp contract(off)
    if (!WANT_GJ) {
#pragma unroll
        for (int k = 0; k < n; ++k)
            acc(k, dot3x(J(k), w[0], J(n + k), w[1], J(2 * n + k), w[2]) + dot3x(J(3 * n + k), w[3], J(4 * n + k), w[4], J(5 * n + k), w[5]));
        return;
    }
    double sx = w[3], sy = w[4], sz = w[5];      // m + S_k
#pragma unroll
    for (int k = n - 1; k >= 0; --k) {
        const double vx = J(k), vy = J(n + k), vz = J(2 * n + k), ox = J(3 * n + k), oy = J(4 * n + k), oz = J(5 * n + k);
        const double gvx = G(k), gvy = G(n + k), gvz = G(2 * n + k), gwx = G(3 * n + k), gwy = G(4 * n + k), gwz = G(5 * n + k);
        sx = sx + (mix_pm(vy, gvz, vz, gvy) + mix_pm(oy, gwz, oz, gwy));
        sy = sy + (mix_pm(vz, gvx, vx, gvz) + mix_pm(oz, gwx, ox, gwz));
        sz = sz + (mix_pm(vx, gvy, vy, gvx) + mix_pm(ox, gwy, oy, gwx));
        acc(k, dot3x(ox, sx, oy, sy, oz, sz));
    }
    double ax = w[0], ay = w[1], az = w[2];      // g_p + A_k
#pragma unroll
    for (int k = 0; k < n; ++k) {
        const double ox = J(3 * n + k), oy = J(4 * n + k), oz = J(5 * n + k);
        const double gvx = G(k), gvy = G(n + k), gvz = G(2 * n + k);
        acc(k, dot3x(J(k), ax, J(n + k), ay, J(2 * n + k), az));
        ax = ax + mix_pm(gvy, oz, gvz, oy);
        ay = ay + mix_pm(gvz, ox, gvx, oz);
        az = az + mix_pm(gvx, oy, gvy, ox);
    }
}

// (vjp_fill / vjp_flush, the row fill and flush of the LDS tiles: kin_vjp.h)

// One register-resident tile: the walk of k_kin_reg (reg_compute: P and the finished Jacobian in registers), then the contraction in registers --
// nothing of T, J or H goes to memory.  gT rows (one round of 64), gJ rows (rounds of kJRound lanes, contracted inside their round straight from
// the staged row: no second 6 n registers) and the gq rows (rounds of floor(ldsd / (qw | 1)) lanes) pass through the one LDS buffer of
// `ldsd` doubles: reg_lds_doubles(NJ) with gJ, 64 x 17 without -- what k_kin_reg asks for.
template <int NJ, bool WANT_GT, bool WANT_GJ, class S>
__device__ __forceinline__ void vjp_tile(const KinParams &kp, const ConstChain &cv, int ldsd, const S *__restrict__ q, const S *__restrict__ gT,
                                         const S *__restrict__ gJ, S *__restrict__ gq, double *buf, int lane, int64_t tile)
{
    constexpr int W = 6 * NJ;
    const int64_t cfg0 = tile * kWave;
    const int64_t left = kp.N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    Pose P;
    double jac[6 * NJ];
    reg_compute<NJ, true>(kp, cv, q, cfg0 + lane, P, jac);
    double w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (WANT_GT) {
        vjp_fill(gT + cfg0 * 16, 16, ncfg, buf, 17, lane);
        __syncthreads();
        const double *mine = buf + (lane < ncfg ? lane : 0) * 17;
        vjp_pose_pullback(P, kp.has_base, kp.base, [&](int k) { return mine[k]; }, w);
        __syncthreads();
    }
    double g[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) g[j] = 0.0;
    if constexpr (WANT_GJ) {
#pragma unroll
        for (int r = 0; r < kWave / kJRound; ++r) {
            int rows = ncfg - r * kJRound;
            rows = rows < 0 ? 0 : (rows > kJRound ? kJRound : rows);
            vjp_fill(gJ + (cfg0 + r * kJRound) * W, W, rows, buf, W + 1, lane);
            __syncthreads();
            if (lane / kJRound == r && lane < ncfg) {
                const double *mine = buf + (lane % kJRound) * (W + 1);
                vjp_contract<true>(NJ, w, [&](int k) { return jac[k]; }, [&](int k) { return mine[k]; }, [&](int k, double x) { g[k] += x; });
            }
            __syncthreads();
        }
    } else {
        vjp_contract<false>(NJ, w, [&](int k) { return jac[k]; }, [&](int) { return 0.0; }, [&](int k, double x) { g[k] += x; });
    }
    // gq rows are q_width wide: a column no joint of the chain reads gets zero, joints sharing a column add up
    const int qw = kp.qw, so = qw | 1;
    int per = ldsd / so;
    per = per > kWave ? kWave : per;
    for (int r0 = 0; r0 < ncfg; r0 += per) {                 // wave-uniform
        if (lane >= r0 && lane < r0 + per) {
            double *mine = buf + (lane - r0) * so;
            for (int c = 0; c < qw; ++c) mine[c] = 0.0;
#pragma unroll
            for (int j = 0; j < NJ; ++j) mine[jm_jq(cv.jmeta[j])] += g[j];
        }
        __syncthreads();
        const int cnt = ncfg - r0 < per ? ncfg - r0 : per;
        vjp_flush(buf, so, qw, cnt, gq + (cfg0 + r0) * qw, lane);
        __syncthreads();
    }
}

// the launch shape of k_kin_reg: ONE tile per single-wave workgroup, no grid-stride loop (see the comment there).  Registers: the pose term alone
// fits k_kin_reg's budget (three waves per SIMD up to 8 joints); with gJ the running sums and the staged row's operands sit on top of the 6 n
// Jacobian registers, and from 6 joints up the 168-register budget sent 2..46 of them to scratch -- those variants take two waves per SIMD, no scratch.
template <int NJ, bool WANT_GT, bool WANT_GJ, class S>
__global__ __launch_bounds__(kWave, (NJ <= kRegMaxJoints && !WANT_GJ ? RTB_REG_WAVES : 2)) void k_kin_vjp(KinParams kp, DevChain dc, int ldsd, const S *__restrict__ q,
                                                                                           const S *__restrict__ gT, const S *__restrict__ gJ, S *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double buf[];
    vjp_tile<NJ, WANT_GT, WANT_GJ>(kp, const_view(dc), ldsd, q, gT, gJ, gq, buf, threadIdx.x, xcd_tile());
}

// Run-time n (1..32), from a SUPPLIED pose and Jacobian (fp64, device): the contraction alone.  Serves rtbhip_kin_vjp_from_jacobian and the chains
// beyond kKinRegMax, whose entry point runs the forward launch into scratch first.  One lane per row; a round of `per` rows passes through LDS as
// rows of [T 16 | gT 16 | J 6n | gJ 6n | gq qw] doubles (odd stride), every global access a contiguous run.  jmeta (NULL: column k is joint k)
// maps a joint to its q column; base (has_base) is pulled back from gT as in the register tile.  S: the storage type of gT, gJ and gq.
struct VjpAnyParams {
    int32_t n, qw, has_base, per;
    int64_t N;
    double base[12];
};
template <class S>
__global__ __launch_bounds__(kWave) void k_vjp_from_jac_any(VjpAnyParams vp, const int32_t *__restrict__ jmeta, const double *__restrict__ T,
                                                            const double *__restrict__ J, const S *__restrict__ gT, const S *__restrict__ gJ, S *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double buf[];
    const int lane = threadIdx.x, n = vp.n, W = 6 * n, qw = vp.qw;
    const int stride = (32 + 2 * W + qw) | 1;
    const int64_t cfg0 = (int64_t)blockIdx.x * kWave;
    const int64_t left = vp.N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    for (int r0 = 0; r0 < ncfg; r0 += vp.per) {              // wave-uniform
        const int cnt = ncfg - r0 < vp.per ? ncfg - r0 : vp.per;
        const int64_t row0 = cfg0 + r0;
        if (gT) {
            vjp_fill(T + row0 * 16, 16, cnt, buf, stride, lane);
            vjp_fill(gT + row0 * 16, 16, cnt, buf + 16, stride, lane);
        }
        vjp_fill(J + row0 * W, W, cnt, buf + 32, stride, lane);
        if (gJ) vjp_fill(gJ + row0 * W, W, cnt, buf + 32 + W, stride, lane);
        __syncthreads();
        if (lane < cnt) {
            double *mine = buf + lane * stride;
            const double *Jr = mine + 32, *Gr = mine + 32 + W;
            double *out = mine + 32 + 2 * W;
            for (int c = 0; c < qw; ++c) out[c] = 0.0;
            double w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (gT) {
                Pose P;
                P.r00 = mine[0]; P.r01 = mine[1]; P.r02 = mine[2]; P.tx = mine[3];
                P.r10 = mine[4]; P.r11 = mine[5]; P.r12 = mine[6]; P.ty = mine[7];
                P.r20 = mine[8]; P.r21 = mine[9]; P.r22 = mine[10]; P.tz = mine[11];
                vjp_pose_pullback(P, vp.has_base, vp.base, [&](int k) { return mine[16 + k]; }, w);
            }
            auto acc = [&](int k, double x) { out[jmeta ? jm_jq(jmeta[k]) : k] += x; };
            if (gJ) vjp_contract<true>(n, w, [&](int k) { return Jr[k]; }, [&](int k) { return Gr[k]; }, acc);
            else vjp_contract<false>(n, w, [&](int k) { return Jr[k]; }, [&](int) { return 0.0; }, acc);
        }
        __syncthreads();
        vjp_flush(buf + 32 + 2 * W, stride, qw, cnt, gq + row0 * qw, lane);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_widen_f32(const float *__restrict__ src, int64_t count, double *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[i] = src[i];
}

template <class S>
static int launch_vjp_from_jac_s(int n, int qw, const int32_t *jmeta, const Affine *base, const double *T, const double *J, const S *gT, const S *gJ,
                                 int64_t N, S *gq, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (n < 1 || n > RTBHIP_MAX_JOINTS) { set_error("kin_vjp_from_jacobian: n must be 1..32"); return RTBHIP_ELIMIT; }
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("kin_vjp: batch too large for one launch"); return RTBHIP_ELIMIT; }
    VjpAnyParams vp;
    vp.n = n; vp.qw = qw; vp.N = N;
    vp.has_base = base && base->used;
    for (int i = 0; i < 12; i++) vp.base[i] = base ? base->v[i] : 0.0;
    const int stride = (32 + 12 * n + qw) | 1;               // <= 673 doubles (n = 32, q_width = 256): at least 9 rows per round in 48 KB
    vp.per = std::min(kWave, (48 * 1024 / 8) / stride);
    const size_t lds = (size_t)vp.per * stride * sizeof(double);
    hipLaunchKernelGGL((k_vjp_from_jac_any<S>), dim3((unsigned)tiles), dim3(kWave), lds, s, vp, jmeta, T, J, gT, gJ, gq);
    note_launch((int)tiles, kWave, (int)lds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_vjp_from_jac_any launch");
    return RTBHIP_OK;
}
int launch_vjp_from_jac(int n, const double *T, const double *J, const double *gT, const double *gJ, int64_t N, double *gq, hipStream_t s)
{
    return launch_vjp_from_jac_s(n, n, nullptr, nullptr, T, J, gT, gJ, N, gq, s);
}

template <int NJ, class S>
static hipError_t launch_vjp_nj(dim3 grid, hipStream_t s, const KinParams &kp, const DevChain &dc, const S *q, const S *gT, const S *gJ, S *gq)
{
    // without gJ only the 64 x 17 pose tile is staged (as fkine alone in launch_kin_s); a gq row of up to 256 columns fits either request
    const int ldsd = gJ ? reg_lds_doubles(NJ) : kWave * 17;
    const size_t lds = (size_t)ldsd * sizeof(double);
    if (gT && gJ) hipLaunchKernelGGL((k_kin_vjp<NJ, true, true, S>), grid, dim3(kWave), lds, s, kp, dc, ldsd, q, gT, gJ, gq);
    else if (gT) hipLaunchKernelGGL((k_kin_vjp<NJ, true, false, S>), grid, dim3(kWave), lds, s, kp, dc, ldsd, q, gT, gJ, gq);
    else hipLaunchKernelGGL((k_kin_vjp<NJ, false, true, S>), grid, dim3(kWave), lds, s, kp, dc, ldsd, q, gT, gJ, gq);
    note_launch((int)grid.x, kWave, (int)lds);
    return hipGetLastError();
}

// S: the storage type of q, gT, gJ and gq.  1..kKinRegMax joints: the fused register tile.  Longer chains: the forward launch (run-time-n tile,
// no base: it is pulled back from gT) into stream-ordered scratch, then k_vjp_from_jac_any with the chain's joint -> q column table; float rows
// are widened into scratch first, so that the forward runs on exactly the values the fp64 call would be given.
template <class S>
static int launch_kin_vjp_s(const Chain *c, const DevChain &ops, const S *q, int64_t N, const Affine &base, const Affine &tool, const S *gT, const S *gJ,
                            S *gq, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("fkine_jacob_vjp: batch too large for one launch"); return RTBHIP_ELIMIT; }
    if (g_use_reg && c->n >= 1 && c->n <= kKinRegMax) {
        KinParams kp;
        kp.n = c->n; kp.qw = c->q_width; kp.stride = kin_stride(c->n); kp.frame = 0; kp.has_base = base.used; kp.pad = 0; kp.N = N;
        for (int i = 0; i < 12; i++) kp.base[i] = base.v[i];
        chain_tail(c, tool, kp.tail);
        dim3 grid((unsigned)tiles);
        hipError_t e = hipSuccess;
        switch (c->n) {
        case 1: e = launch_vjp_nj<1>(grid, s, kp, ops, q, gT, gJ, gq); break;
        case 2: e = launch_vjp_nj<2>(grid, s, kp, ops, q, gT, gJ, gq); break;
        case 3: e = launch_vjp_nj<3>(grid, s, kp, ops, q, gT, gJ, gq); break;
        case 4: e = launch_vjp_nj<4>(grid, s, kp, ops, q, gT, gJ, gq); break;
        case 5: e = launch_vjp_nj<5>(grid, s, kp, ops, q, gT, gJ, gq); break;
        case 6: e = launch_vjp_nj<6>(grid, s, kp, ops, q, gT, gJ, gq); break;
        case 7: e = launch_vjp_nj<7>(grid, s, kp, ops, q, gT, gJ, gq); break;
        case 8: e = launch_vjp_nj<8>(grid, s, kp, ops, q, gT, gJ, gq); break;
        case 9: e = launch_vjp_nj<9>(grid, s, kp, ops, q, gT, gJ, gq); break;
        default: e = launch_vjp_nj<10>(grid, s, kp, ops, q, gT, gJ, gq); break;
        }
        if (e != hipSuccess) return hip_fail(e, "k_kin_vjp launch");
        return RTBHIP_OK;
    }
    if (c->n < 1 || c->n > RTBHIP_MAX_JOINTS) { set_error("fkine_jacob_vjp: chains of 1..RTBHIP_MAX_JOINTS joints"); return RTBHIP_ELIMIT; }
    const int rc0 = pool_keep_cached();      // the temporaries come from the device's pool, kept cached between calls (rtbhip_partial_fkine0 does the same)
    if (rc0 != RTBHIP_OK) return rc0;
    const size_t n = (size_t)c->n, rows = (size_t)N;
    const size_t qd = std::is_same<S, float>::value ? rows * c->q_width : 0;
    void *p = nullptr;
    hipError_t e = hipMallocAsync(&p, (rows * (16 + 6 * n) + qd) * sizeof(double), s);
    if (e != hipSuccess) return hip_fail(e, "hipMallocAsync (fkine_jacob_vjp temporaries)");
    double *Ts = (double *)p, *Js = Ts + rows * 16, *qs = Js + rows * 6 * n;
    const double *q64;
    if constexpr (std::is_same<S, float>::value) {
        const int64_t count = (int64_t)qd;
        hipLaunchKernelGGL(k_widen_f32, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, q, count, qs);
        q64 = qs;
    } else {
        q64 = q;
    }
    Affine nobase;
    nobase.used = 0;
    for (int i = 0; i < 12; i++) nobase.v[i] = (i % 5 == 0) ? 1.0 : 0.0;
    int rc = launch_kin(c, ops, q64, N, nobase, tool, 0, Ts, Js, nullptr, s);
    if (rc == RTBHIP_OK) rc = launch_vjp_from_jac_s(c->n, c->q_width, ops.jmeta, &base, Ts, Js, gT, gJ, N, gq, s);
    (void)hipFreeAsync(p, s);
    return rc;
}
int launch_kin_vjp(const Chain *c, const DevChain &ops, const double *q, int64_t N, const Affine &base, const Affine &tool, const double *gT,
                   const double *gJ, double *gq, hipStream_t s)
{
    return launch_kin_vjp_s(c, ops, q, N, base, tool, gT, gJ, gq, s);
}
int launch_kin_vjp_f32(const Chain *c, const DevChain &ops, const float *q, int64_t N, const Affine &base, const Affine &tool, const float *gT,
                       const float *gJ, float *gq, hipStream_t s)
{
    return launch_kin_vjp_s(c, ops, q, N, base, tool, gT, gJ, gq, s);
}

}  // namespace rtbhip
