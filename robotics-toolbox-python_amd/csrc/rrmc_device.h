// rrmc_device.h -- the per-lane body and the tile phases of RESOLVED-RATE MOTION CONTROL (rtbhip_rrmc; the kernels are rrmc_kernels.hip): the loop
// the reference's README opens with,
//     v, arrived = rtb.p_servo(robot.fkine(q), Tep, gain)          tools/p_servo.py:46-106
//     qd = pinv(robot.jacobe(q)) @ v ;  q += dt qd
// fused into one launch and, for `steps` > 1, iterated on the device.  Per row, for it = 0 .. steps - 1:
//     T, J = fkine(q), jacob(q)        method 1 "rpy": J = jacobe (the error is seen from the end-effector frame);  method 0 "angle-axis": J = jacob0
//     e    = p_servo's error (servo_device.h: servo_rpy_lane / aa_lane)
//     arr  = sum|e| < threshold        on e, before the gain (p_servo.py:104)
//     r    = gain6 * e - J qnull       qnull = 0 when not given
//     qd   = qnull + X r               X = pinv(J), applied as solves, never formed
//     q    = q + dt qd ;  its = it + 1 ;  if arr: stop      (the step of the iteration that arrives IS taken, as in the README loop)
// How X is applied (rtbhip_opspace's rule, opspace_device.h), d = damping:
//     n = 6, d = 0            J x = r by LU with partial pivoting (ops_lu_factor / ops_lu_solve)
//     n > 6, or n = 6, d > 0  x = J^T (J J^T + d^2 I)^-1 r by ldl_solve<6>
//     n < 6                   x = (J^T J + d^2 I)^-1 J^T r by an LDL^T of the n x n Gram matrix
// with exact divisions.  A zero or non-finite pivot leaves its row non-finite; nothing is repaired (rtbhip_ik_vjp's policy: the damping is the
// caller's remedy).  numpy's SVD-truncated pinv at a rank-deficient J is NOT reproduced.
//
// As ikgrad_device.h: every function here is __host__ __device__, takes (lane, lds, ...) and has no barrier inside; the kernel calls the phases
// with lane = threadIdx.x and keeps its __syncthreads() between them, tests/emu_rrmc calls them in a loop over lanes on the CPU.
#pragma once
#include "kin_reg.h"
#include "kin_vjp.h"
#include "ldl.h"
#include "vjp_tile.h"
#include "servo_device.h"
#include "opspace_device.h"

namespace rtbhip {

// every floating-point operation as written (kin_device.h: mix_pp and friends)
#pragma clang fp contract(off)

struct RrmcParams {
    int32_t n, method, steps, tep_each;     // joints; 0 angle-axis / jacob0, 1 rpy / jacobe; iterations at most; 1: a Tep per row, 0: one for all
    int64_t N;
    double gain[6], threshold, d2, dt;      // d2: damping squared
    double tail[12];                        // C_n as {R row-major (9), t (3)}: the chain's own last constant, no further tool
};

// A lane's LDS row: [q n | qnull n | Tep 16 | qd n].  q and qd LIVE there: an iteration reads q for its sines and cosines and comes back to it
// with the finished rate, so nothing but the flags crosses an iteration in registers (with q and qd there too, 6..10 joints spilled).  On the way
// out q_out is where q was, arrived and its are the first two slots of Tep.  The stride is odd.
RTB_HD int rrmc_head(int n) { return 2 * n; }
RTB_HD int rrmc_rate(int n) { return 2 * n + 16; }
RTB_HD int rrmc_stride(int n) { return (3 * n + 16) | 1; }

// phase 1: the tile's q and qnull blocks (vjp_tile.h: coalesced, the loads in flight together; an absent qnull becomes zeros) and its Tep rows
// (kin_vjp.h) into the lanes' rows.  One Tep for the whole batch: every lane copies the same 128 bytes into its own row.
template <int NJ>
RTB_HD void rrmc_tile_fill(const RrmcParams &rp, const double *__restrict__ q, const double *__restrict__ qnull, const double *__restrict__ Tep,
                           int64_t tile, int lane, double *lds)
{
    const VjpTile t = vjp_tile_of(tile, rp.N, NJ);
    const double *const src[2] = {q + t.cfg0 * NJ, qnull ? qnull + t.cfg0 * NJ : nullptr};
    VjpCols<NJ, 2, double> cols;
    vjp_load_cols<NJ, true>(src, t, lane, cols);
    if (rp.tep_each) {
        vjp_fill(Tep + t.cfg0 * 16, 16, t.ncfg, lds + rrmc_head(NJ), rrmc_stride(NJ), lane);
    } else {
        double *mine = lds + lane * rrmc_stride(NJ) + rrmc_head(NJ);
#pragma unroll
        for (int k = 0; k < 16; ++k) mine[k] = Tep[k];
    }
    sched_fence();
    vjp_stage_cols<NJ, true>(src, t, NJ, rrmc_stride(NJ), lane, cols, lds);
}

// x = X r for the finished Jacobian jac (slot r NJ + k: entry (r, k)), by the rule above
template <int NJ>
RTB_HD void rrmc_solve(const double (&jac)[6 * NJ], double (&r)[6], double d2, double (&x)[NJ])
{
#pragma clang fp contract(off)
    if constexpr (NJ < 6) {
        double S[NJ][NJ], b[NJ];
#pragma unroll
        for (int a = 0; a < NJ; ++a) {
            double s = jac[a] * r[0];
#pragma unroll
            for (int i = 1; i < 6; ++i) s = __builtin_fma(jac[i * NJ + a], r[i], s);
            b[a] = s;
#pragma unroll
            for (int c = 0; c <= a; ++c) {
                double g = jac[a] * jac[c];
#pragma unroll
                for (int i = 1; i < 6; ++i) g = __builtin_fma(jac[i * NJ + a], jac[i * NJ + c], g);
                S[a][c] = a == c ? g + d2 : g;
            }
        }
        sched_fence();
        ldl_solve<NJ>(S, b, x);
    } else {
        if (NJ == 6 && d2 == 0.0) {                      // wave-uniform
            if constexpr (NJ == 6) {
                double A[6][6];
                bool sw[6][6];
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int k = 0; k < 6; ++k) A[i][k] = jac[i * 6 + k];
                ops_lu_factor<6>(A, sw);
                ops_lu_solve<6>(A, sw, r);
#pragma unroll
                for (int k = 0; k < 6; ++k) x[k] = r[k];
            }
            return;
        }
        double B[6][6], y[6];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = 0; c <= a; ++c) {
                double g = jac[a * NJ] * jac[c * NJ];
#pragma unroll
                for (int k = 1; k < NJ; ++k) g = __builtin_fma(jac[a * NJ + k], jac[c * NJ + k], g);
                B[a][c] = a == c ? g + d2 : g;
            }
        sched_fence();
        ldl_solve<6>(B, r, y);
        sched_fence();
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            double s = jac[k] * y[0];
#pragma unroll
            for (int i = 1; i < 6; ++i) s = __builtin_fma(jac[i * NJ + k], y[i], s);
            x[k] = s;
        }
    }
}

// phase 2: the lane's own row -- the loop of the file comment, entirely in registers; Tep and qnull are read from the row where they are needed.
// live: the lane holds a row of the batch.  The loop is bounded by rp.steps and by nothing else: a lane that has arrived keeps its results and
// idles, the wave leaves when no lane is live, and a row that is not finite never arrives -- it runs out its steps.  Such a row walks the chain on
// zeros and has its rate poisoned afterwards: every output of it is non-finite either way, and the other lanes of its wave keep the sines they
// have alone (the library's sincos is a decision of the whole wave, kin_reg.h: reg_core).
template <int NJ, class CV>
RTB_HD void rrmc_lane(const RrmcParams &rp, const CV &cv, bool has_null, bool live, double *mine)
{
#pragma clang fp contract(off)
    const double *tep = mine + rrmc_head(NJ);
    const double *qn = mine + NJ;
    double *qd = mine + rrmc_rate(NJ);
#pragma unroll
    for (int j = 0; j < NJ; ++j) qd[j] = 0.0;
    int its = 0;
    bool arrived = false;
#pragma unroll 1
    for (int it = 0; it < rp.steps; ++it) {
        if (!wave_any(live)) break;
        if (live) {
            bool bad = false;
            double qs[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) { qs[j] = mine[j]; bad = bad || !(fabs(qs[j]) < __builtin_inf()); }
#pragma unroll
            for (int j = 0; j < NJ; ++j) qs[j] = bad ? 0.0 : qs[j];
            Pose P;
            double jac[6 * NJ];
            reg_core<NJ, true>(cv, rp.tail, rp.method, qs, P, jac);
            sched_fence();      // the phases of an iteration one after the other
            double e[6], r[6];
            {
                const double te[12] = {P.r00, P.r01, P.r02, P.tx, P.r10, P.r11, P.r12, P.ty, P.r20, P.r21, P.r22, P.tz};
                if (rp.method == 1) servo_rpy_lane(te, tep, e);          // wave-uniform
                else aa_lane(te, tep, e);
            }
            sched_fence();
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) sum += fabs(e[k]);
            const bool arr = !bad && sum < rp.threshold;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                r[i] = rp.gain[i] * e[i];
                if (has_null) {                                          // wave-uniform
                    double s = jac[i * NJ] * qn[0];
#pragma unroll
                    for (int k = 1; k < NJ; ++k) s = __builtin_fma(jac[i * NJ + k], qn[k], s);
                    r[i] = r[i] - s;
                }
            }
            sched_fence();
            double x[NJ];
            rrmc_solve<NJ>(jac, r, rp.d2, x);
            sched_fence();
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                double v = has_null ? qn[k] + x[k] : x[k];
                v = bad ? __builtin_nan("") : v;
                qd[k] = v;
                mine[k] = mine[k] + rp.dt * v;
            }
            its = it + 1;
            arrived = arr;
            live = !arr;
        }
    }
    mine[2 * NJ] = arrived ? 1.0 : 0.0;
    mine[2 * NJ + 1] = (double)its;
}

// phase 3: the live rows out, each output one contiguous run (kin_vjp.h); a NULL output is not stored (wave-uniform)
RTB_HD void rrmc_tile_flush(int n, int cnt, const double *lds, double *__restrict__ qd, double *__restrict__ q_out, uint8_t *__restrict__ arrived,
                            int32_t *__restrict__ its, int lane)
{
    const int stride = rrmc_stride(n);
    if (qd) vjp_flush(lds + rrmc_rate(n), stride, n, cnt, qd, lane);
    if (q_out) vjp_flush(lds, stride, n, cnt, q_out, lane);
    if (lane < cnt) {
        const double *mine = lds + lane * stride + 2 * n;
        if (arrived) arrived[lane] = mine[0] != 0.0 ? 1 : 0;
        if (its) its[lane] = (int32_t)mine[1];
    }
}

#pragma clang fp contract(fast)
}  // namespace rtbhip
