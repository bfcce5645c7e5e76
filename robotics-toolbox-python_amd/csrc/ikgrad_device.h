// ikgrad_device.h -- the per-lane body and the tile phases of the IMPLICIT-FUNCTION ADJOINT of the inverse kinematics (rtbhip_ik_vjp; the
// kernels are ikgrad_kernels.hip).  No reference counterpart: the reference has no derivative of a solver.  What is differentiated is the solution
// map of _angle_axis(fkine(q), Tep) = 0 (core/ik.cpp:241-286) on the rows with a non-zero mask weight, with _ETS_jacob0 (core/methods.cpp:112-217).
//
// At a converged q a change of the target by the world-frame twist nu (d t_p = nu_v, d R_p = [nu_w]x R_p) moves the solution by
//     J_a dq = nu_a,       dq = J_a^T (J_a J_a^T + d^2 I)^-1 nu_a           (a: the used rows; minimum norm; the positive weights drop out, ik_device.h)
// so a gradient gq on q pulls back to the twist
//     y_a = (J_a J_a^T + d^2 I)^-1 J_a gq,     y = 0 on the unused rows,
// the 6 x 6 symmetric system ik_pinv_step solves on every Gauss-Newton / Newton-Raphson iteration.  In the coordinates of Tep it is
//     gTep[:3, 3] = y_v,      gTep[:3, :3] = 1/2 [y_w]x R_p,      bottom row 0
// the tangent-space gradient at Tep: vjp_pose_pullback (kin_vjp.h) of it returns y, so a Tep that is itself a function (the fkine of another chain,
// a rotation parametrisation) chains correctly.  A row with success == 0 gets zeros.  A pivot that is zero or not finite leaves its row not
// finite; nothing is repaired (the damping d is the caller's remedy).
//
// As kin_tile.h / vjp_tile.h: every function here is __host__ __device__, takes (lane, lds, ...) and has no barrier inside; the kernels call the
// phases with lane = threadIdx.x and keep their __syncthreads() between them, tests/emu_ik_vjp calls them in a loop over lanes on the CPU.
#pragma once
#include "kin_reg.h"
#include "kin_vjp.h"
#include "ldl.h"
#include "vjp_tile.h"

namespace rtbhip {

// every floating-point operation as written (kin_device.h: mix_pp and friends)
#pragma clang fp contract(off)

struct IkVjpParams {
    int32_t n, rows, per, pad;      // joints; bit r set: row r of the twist is used; rows of a round (run-time-n form)
    int64_t N;
    double d2;                      // damping squared
    double tail[12];                // C_n as {R row-major (9), t (3)}: no tool in IK
};

// y = (J_a J_a^T + d2 I)^-1 J_a gq on the used rows, 0 on the others.  J(r n + k): entry (r, k) of the finished Jacobian, the slot order of
// ik_lm_step; gq(k).  An unused row is embedded as a row of the identity (ik_pinv_step does the same for a short mask), so the solve is always
// ldl_solve<6> -- with the exact division: it runs once per row and its accuracy is what the caller sees.  n is a compile-time constant in the
// register tile (every index static) and a run-time value in k_ik_vjp_any.
template <class JGet, class GGet>
RTB_HD void ik_vjp_solve(int n, JGet J, GGet gq, int rows, double d2, double (&y)[6])
{
#pragma clang fp contract(off)
    double B[6][6], b[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const bool ur = (rows >> r) & 1;
        double s = J(r * n) * gq(0);
#pragma unroll
        for (int k = 1; k < n; ++k) s = __builtin_fma(J(r * n + k), gq(k), s);
        b[r] = ur ? s : 0.0;
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            const bool uc = (rows >> c) & 1;
            double a = J(r * n) * J(c * n);
#pragma unroll
            for (int k = 1; k < n; ++k) a = __builtin_fma(J(r * n + k), J(c * n + k), a);
            B[r][c] = (ur && uc) ? (r == c ? a + d2 : a) : (r == c ? 1.0 : 0.0);
        }
    }
    sched_fence();      // J is dead from here on
    ldl_solve<6>(B, b, y);
#pragma unroll
    for (int r = 0; r < 6; ++r) y[r] = ((rows >> r) & 1) ? y[r] : 0.0;
}

// the row's results into its LDS row: gTep over the 16 slots Tep came in (T: row-major 4x4), the twist into tw[0..5].  ok == 0: zeros, selected
// (a row that did not converge may have produced anything).  An output nobody asked for is neither formed nor written.
RTB_HD void ik_vjp_emit(const double (&y)[6], int ok, bool want_T, bool want_tw, double *T, double *tw)
{
#pragma clang fp contract(off)
    if (want_T) {
        const double r00 = T[0], r01 = T[1], r02 = T[2], r10 = T[4], r11 = T[5], r12 = T[6], r20 = T[8], r21 = T[9], r22 = T[10];
        const double wx = y[3], wy = y[4], wz = y[5];
        // 1/2 [w]x R: row 0 = wy R_2 - wz R_1, row 1 = wz R_0 - wx R_2, row 2 = wx R_1 - wy R_0  (the halving is exact)
        T[0] = ok ? 0.5 * mix_pm(wy, r20, wz, r10) : 0.0; T[1] = ok ? 0.5 * mix_pm(wy, r21, wz, r11) : 0.0; T[2] = ok ? 0.5 * mix_pm(wy, r22, wz, r12) : 0.0;
        T[4] = ok ? 0.5 * mix_pm(wz, r00, wx, r20) : 0.0; T[5] = ok ? 0.5 * mix_pm(wz, r01, wx, r21) : 0.0; T[6] = ok ? 0.5 * mix_pm(wz, r02, wx, r22) : 0.0;
        T[8] = ok ? 0.5 * mix_pm(wx, r10, wy, r00) : 0.0; T[9] = ok ? 0.5 * mix_pm(wx, r11, wy, r01) : 0.0; T[10] = ok ? 0.5 * mix_pm(wx, r12, wy, r02) : 0.0;
        T[3] = ok ? y[0] : 0.0; T[7] = ok ? y[1] : 0.0; T[11] = ok ? y[2] : 0.0;
        T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 0.0;
    }
    if (want_tw) {
#pragma unroll
        for (int r = 0; r < 6; ++r) tw[r] = ok ? y[r] : 0.0;
    }
}

// ---------------------------------------------------------------- the register tile, NJ = 1..kKinRegMax
// A lane's LDS row: [q n | gq n] (at least 6 slots: the twist leaves through slots 0..5) then [Tep 16] (gTep leaves through the same slots); the
// stride is odd.  q and gq are (N, n) as rtbhip_ik_lm writes q_out: column j is joint j (k_ik reads its joint vector the same way).
RTB_HD int ik_vjp_head(int n) { return 2 * n > 6 ? 2 * n : 6; }
RTB_HD int ik_vjp_stride(int n) { return (ik_vjp_head(n) + 16) | 1; }

// phase 1: the tile's q and gq blocks (vjp_tile.h: coalesced, the loads in flight together) and its Tep rows (kin_vjp.h) into the lanes' rows
template <int NJ>
RTB_HD void ik_vjp_tile_fill(const IkVjpParams &ip, const double *__restrict__ q, const double *__restrict__ gq, const double *__restrict__ Tep,
                             int64_t tile, int lane, double *lds)
{
    const VjpTile t = vjp_tile_of(tile, ip.N, NJ);
    const double *const src[2] = {q + t.cfg0 * NJ, gq + t.cfg0 * NJ};
    VjpCols<NJ, 2, double> cols;
    vjp_load_cols<NJ, false>(src, t, lane, cols);
    vjp_fill(Tep + t.cfg0 * 16, 16, t.ncfg, lds + ik_vjp_head(NJ), ik_vjp_stride(NJ), lane);
    sched_fence();
    vjp_stage_cols<NJ, false>(src, t, NJ, ik_vjp_stride(NJ), lane, cols, lds);
}

// phase 2: the lane's own row -- the walk of k_kin_reg (P is not needed: R_p is the target's), the solve, the results over the inputs
template <int NJ, class CV>
RTB_HD void ik_vjp_lane(const IkVjpParams &ip, const CV &cv, int ok, bool want_T, bool want_tw, double *mine)
{
    double qv[NJ], g[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { qv[j] = mine[j]; g[j] = mine[NJ + j]; }
    Pose P;
    double jac[6 * NJ];
    reg_core<NJ, true>(cv, ip.tail, 0, qv, P, jac);
    double y[6];
    ik_vjp_solve(NJ, [&](int k) { return jac[k]; }, [&](int k) { return g[k]; }, ip.rows, ip.d2, y);
    ik_vjp_emit(y, ok, want_T, want_tw, mine + ik_vjp_head(NJ), mine);
}

// phase 3: the live rows out, each output one contiguous run (kin_vjp.h); a NULL output is not stored (wave-uniform)
RTB_HD void ik_vjp_tile_flush(int head, int stride, int cnt, const double *lds, double *__restrict__ gTep, double *__restrict__ gtwist, int lane)
{
    if (gTep) vjp_flush(lds + head, stride, 16, cnt, gTep, lane);
    if (gtwist) vjp_flush(lds, stride, 6, cnt, gtwist, lane);
}

// ---------------------------------------------------------------- run-time n (11..RTBHIP_MAX_JOINTS joints), from a SUPPLIED Jacobian
// A round of `per` rows passes through LDS as rows of [J 6n | gq n | Tep 16] doubles (odd stride); the twist leaves through slots 0..5 of J,
// gTep through Tep's.  J: (N, 6, n) as rtbhip_jacob writes it (frame 0, no tool).
RTB_HD int ik_vjp_any_stride(int n) { return (7 * n + 16) | 1; }

// rows row0 .. row0 + cnt - 1 in (gq rows may be odd wide: one element per lane)
RTB_HD void ik_vjp_any_fill(int n, const double *__restrict__ J, const double *__restrict__ gq, const double *__restrict__ Tep, int64_t row0, int cnt,
                            int lane, double *lds)
{
    const int stride = ik_vjp_any_stride(n);
    vjp_fill(J + row0 * 6 * n, 6 * n, cnt, lds, stride, lane);
    vjp_fill(Tep + row0 * 16, 16, cnt, lds + 7 * n, stride, lane);
    vjp_fill_any(gq + row0 * n, n, cnt, lds + 6 * n, stride, lane);
}
RTB_HD void ik_vjp_any_lane(const IkVjpParams &ip, int ok, bool want_T, bool want_tw, double *mine)
{
    const int n = ip.n;
    double y[6];
    ik_vjp_solve(n, [&](int k) { return mine[k]; }, [&](int k) { return mine[6 * n + k]; }, ip.rows, ip.d2, y);
    ik_vjp_emit(y, ok, want_T, want_tw, mine + 7 * n, mine);
}

#pragma clang fp contract(fast)
}  // namespace rtbhip
