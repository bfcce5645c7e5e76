// kin_vjp.h -- what the kinematic adjoint kernels share: the pull-back of a pose gradient onto a 6-vector and the row fill / flush of their LDS
// tiles.  Used by k_kin_vjp / k_vjp_from_jac_any (kin_kernels.hip) and by k_ik_vjp (ikgrad_kernels.hip); every function is a
// __host__ __device__ function of (lane, lds, ...) with no barrier inside, as in kin_tile.h, so that tests/emu_* replays them on the CPU.
#pragma once
#include "kin_device.h"

namespace rtbhip {

// (g_p ; m) of a pose gradient gT at the pose P (kin_kernels.hip, "vector-Jacobian products of fkine / jacob0", has the derivation):
//     g_p = translation column of B^T gT,   m = sum_c R_c x (B^T gT)_c
// Every sum of two products is written out (kin_device.h: mix_pp and friends).
template <class G>
RTB_HD void vjp_pose_pullback(const Pose &P, int has_base, const double *base /* row-major 3x4 */, G g /* g(4 r + c): row r, column c of gT */, double (&w)[6])
{
#pragma clang fp contract(off)
    double h[12];      // B_R^T gT (top three rows)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            h[4 * i + c] = has_base ? dot3x(base[i], g(c), base[4 + i], g(4 + c), base[8 + i], g(8 + c)) : g(4 * i + c);
    w[0] = h[3]; w[1] = h[7]; w[2] = h[11];
    w[3] = (mix_pm(P.r10, h[8], P.r20, h[4]) + mix_pm(P.r11, h[9], P.r21, h[5])) + mix_pm(P.r12, h[10], P.r22, h[6]);
    w[4] = (mix_pm(P.r20, h[0], P.r00, h[8]) + mix_pm(P.r21, h[1], P.r01, h[9])) + mix_pm(P.r22, h[2], P.r02, h[10]);
    w[5] = (mix_pm(P.r00, h[4], P.r10, h[0]) + mix_pm(P.r01, h[5], P.r11, h[1])) + mix_pm(P.r02, h[6], P.r12, h[2]);
}

// kin_flush in reverse: `cnt` consecutive rows of W values (W even, contiguous in global memory) into LDS rows of `stride` doubles, widened after
// the load.  Lane l reads the pairs l, l + 64, ... of the run.  A pointer is only assumed aligned to its element (views of tensors are legal).
template <class S>
RTB_HD void vjp_fill(const S *__restrict__ src, int W, int cnt, double *rows, int stride, int lane)
{
    const int total = cnt * W;
    int f = 2 * lane;
    int r = f / W, e = f - r * W;
    const int da = 128 / W, db = 128 - da * W;
    for (; f < total; f += 128) {
        double a, b;
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (sizeof(S) == 4) {
            typedef float v2f __attribute__((ext_vector_type(2)));
            typedef v2f v2f_a4 __attribute__((aligned(4)));
            const v2f v = *reinterpret_cast<const v2f_a4 *>(src + f);
            a = v.x; b = v.y;
        } else {
            typedef double v2d __attribute__((ext_vector_type(2)));
            typedef v2d v2d_a8 __attribute__((aligned(8)));
            const v2d v = *reinterpret_cast<const v2d_a8 *>(src + f);
            a = v.x; b = v.y;
        }
#else
        a = src[f]; b = src[f + 1];
#endif
        double *dst = rows + r * stride + e;
        dst[0] = a; dst[1] = b;
        e += db; r += da;
        if (e >= W) { e -= W; r += 1; }
    }
}
// vjp_flush in reverse, for rows of ANY width W >= 1 (an odd W has no pairs to read): one element per lane per instruction
template <class S>
RTB_HD void vjp_fill_any(const S *__restrict__ src, int W, int cnt, double *rows, int stride, int lane)
{
    const int total = cnt * W;
    int f = lane;
    int r = f / W, e = f - r * W;
    const int da = kWave / W, db = kWave - da * W;
    for (; f < total; f += kWave) {
        rows[r * stride + e] = (double)src[f];
        e += db; r += da;
        if (e >= W) { e -= W; r += 1; }
    }
}
// `cnt` staged rows of W values (any W >= 1) out as one contiguous run, one element per lane per instruction, rounded once
template <class S>
RTB_HD void vjp_flush(const double *rows, int stride, int W, int cnt, S *__restrict__ dst, int lane)
{
    const int total = cnt * W;
    int f = lane;
    int r = f / W, e = f - r * W;
    const int da = kWave / W, db = kWave - da * W;
    for (; f < total; f += kWave) {
        dst[f] = (S)rows[r * stride + e];
        e += db; r += da;
        if (e >= W) { e -= W; r += 1; }
    }
}

}  // namespace rtbhip
