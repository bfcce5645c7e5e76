// mmc_device.h -- the per-lane body and the tile phases of the REACTIVE QP SERVO (rtbhip_mmc; the kernels are mmc_kernels.hip): the
// manipulability-maximising motion controller of the reference's examples/mmc.py (Haviland & Corke, "A purely-reactive manipulability-maximising
// motion controller") with the joint-limit velocity dampers of Robot.joint_velocity_damper (robot/Robot.py:1413-1419, IK.py:1480-1490) and the
// joint-velocity box as its constraints, one fused launch, iterated on the device.  Per row, for it = 0 .. steps - 1:
//     T, J0 = fkine(q), jacob0(q) ;  J = jacobe(q) for method 1 "rpy", J0 for method 0 "angle-axis"     (the pairing of rtbhip_rrmc)
//     e   = p_servo's error (servo_device.h) ;  s = sum|e| ;  arr = s < threshold                      (on e, before the gain)
//     v   = gain6 * e
//     qd  = argmin over (qd, delta) of  1/2 Y |qd|^2 + 1/2 (ks / s) |delta|^2 - (1 / km) jacobm(q)^T qd
//             subject to  J qd + delta = v,  lo <= qd <= hi
//     q   = q + dt qd ;  its = it + 1 ;  if arr: stop       (the step of the arriving iteration IS taken)
// jacobm is the Yoshikawa manipulability Jacobian of J0, all six axes (diff_device.h); km = 0: no linear term.  The box starts as
// [-qdlim_j, +qdlim_j] (unbounded without qdlim) and is tightened by the dampers, BOTH sides of a joint independently:
//     qlim_hi_j - q_j <= pi:   hi_j = min(hi_j,  damper_gain ((qlim_hi_j - q_j) - ps) / (pi - ps))
//     q_j - qlim_lo_j <= pi:   lo_j = max(lo_j, -damper_gain ((q_j - qlim_lo_j) - ps) / (pi - ps))
// (the reference has one matrix row per joint and lets one side override the other; the two agree whenever pi is at most half the joint's range).
//
// THE QP.  With the slack eliminated it is strictly convex in qd alone.  d^2 = Y s / ks, g = jacobm / (Y km) (0 when km = 0); with a set A of
// joints held on a bound x_A and F the free rest,
//     y = (J_F J_F^T + d^2 I)^-1 (v - J_A x_A - J_F g_F),     u = g + J^T y,     qd_F = u_F,     v - J qd = d^2 y  (the slack)
// and Y (u_k - x_k), signed towards the bound's outside, is a held joint's multiplier: the 6 x 6 solve of ik_qp_bounded (ik_device.h), with
// two-sided bounds.  The update is NOT that function's whole-set swap, which cycles here (g is ~100 times qdlim at Y = 0.01: DESIGN.md 4.20):
// ONE change per round -- hold the most violated free joint on the side it violates (lowest index on a tie); if none is violated, release the
// held joint with the most negative multiplier; neither: the KKT point, the unique minimiser.  At most 3 n + 2 rounds; every lane of the wave
// runs until a ballot shows all lanes done (a lane that is done recomputes the same numbers).
// UNSOLVABLE: an empty box (lo_j > hi_j: a damper's bound has crossed the other side's -- a joint past its limit by more than
// ps + qdlim (pi - ps) / damper_gain, or within ps of both limits; inside ps of ONE limit only makes that bound cross zero), rounds that run out,
// a q, an error or a solve that is not finite.  Such a row
// has status bit 0 set and its rate and q non-finite from there on; it never arrives and touches no other row.  Nothing is repaired.
// Status bit 1: some iteration's slack |v - J qd|inf exceeded 10 (the example's box on the slack is not imposed, only reported).
//
// As rrmc_device.h: every function here is __host__ __device__, takes (lane, lds, ...) and has no barrier inside; the kernel calls the phases
// with lane = threadIdx.x and keeps its __syncthreads() between them, tests/emu_mmc calls them in a loop over lanes on the CPU.
#pragma once
#include "kin_reg.h"
#include "kin_vjp.h"
#include "ldl.h"
#include "vjp_tile.h"
#include "servo_device.h"
#include "diff_device.h"

namespace rtbhip {

// every floating-point operation as written (kin_device.h: mix_pp and friends)
#pragma clang fp contract(off)

constexpr int kMmcMin = 6, kMmcMax = 10;        // jacobm needs a square or redundant arm; the register tile ends at kKinRegMax
constexpr int kMmcTwoWavesMax = 7;              // up to here an instantiation fits 256 VGPRs: two waves per SIMD (mmc_kernels.hip)

struct MmcParams {
    int32_t n, method, steps, tep_each;     // joints; 0 angle-axis / jacob0, 1 rpy / jacobe; iterations at most; 1: a Tep per row, 0: one for all
    int64_t N;
    double gain[6], threshold, dt;
    double Y, ks, km, ps, pi, dgain;        // dgain: damper_gain
    double tail[12];                        // C_n as {R row-major (9), t (3)}: the chain's own last constant, no further tool
    double qlo[kMmcMax], qhi[kMmcMax];      // the joint limits (an infinite one: no damper on that side)
    double vmax[kMmcMax];                   // the velocity box (infinity: none)
};

// A lane's LDS row: [q n | Tep 16 | qd n].  q and qd LIVE there between iterations (rrmc_device.h).  On the way out q_out is where q was,
// arrived, its and status are the first three slots of Tep.  The stride is odd.
RTB_HD int mmc_head(int n) { return n; }
RTB_HD int mmc_rate(int n) { return n + 16; }
RTB_HD int mmc_stride(int n) { return (2 * n + 16) | 1; }

// phase 1: the tile's q block (vjp_tile.h: coalesced, the loads in flight together) and its Tep rows (kin_vjp.h) into the lanes' rows.  One Tep
// for the whole batch: every lane copies the same 128 bytes into its own row.
template <int NJ>
RTB_HD void mmc_tile_fill(const MmcParams &mp, const double *__restrict__ q, const double *__restrict__ Tep, int64_t tile, int lane, double *lds)
{
    const VjpTile t = vjp_tile_of(tile, mp.N, NJ);
    const double *const src[1] = {q + t.cfg0 * NJ};
    VjpCols<NJ, 1, double> cols;
    vjp_load_cols<NJ, false>(src, t, lane, cols);
    if (mp.tep_each) {
        vjp_fill(Tep + t.cfg0 * 16, 16, t.ncfg, lds + mmc_head(NJ), mmc_stride(NJ), lane);
    } else {
        double *mine = lds + lane * mmc_stride(NJ) + mmc_head(NJ);
#pragma unroll
        for (int k = 0; k < 16; ++k) mine[k] = Tep[k];
    }
    sched_fence();
    vjp_stage_cols<NJ, false>(src, t, NJ, mmc_stride(NJ), lane, cols, lds);
}

// the box of one iteration: the velocity limits tightened by the dampers, both sides independently.  -> false when it is empty
template <int NJ>
RTB_HD bool mmc_box(const MmcParams &mp, const double (&qs)[NJ], double (&lo)[NJ], double (&hi)[NJ])
{
#pragma clang fp contract(off)
    const double scale = mp.dgain / (mp.pi - mp.ps);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const double up = mp.qhi[j] - qs[j], dn = qs[j] - mp.qlo[j];
        double h = mp.vmax[j], l = -mp.vmax[j];
        if (up <= mp.pi) { const double b = (up - mp.ps) * scale; h = b < h ? b : h; }
        if (dn <= mp.pi) { const double b = -((dn - mp.ps) * scale); l = b > l ? b : l; }
        lo[j] = l; hi[j] = h;
        ok = ok && !(l > h);
    }
    return ok;
}

// The active-set iteration of the file comment -> true at the KKT point.  dq: the rate; slack: |v - J dq|inf = d^2 |y|inf of the last round.
template <int NJ>
RTB_HD bool mmc_qp(const double (&jac)[6 * NJ], const double (&v)[6], double d2, const double (&g)[NJ], const double (&lo)[NJ], const double (&hi)[NJ],
                   double (&dq)[NJ], double &slack)
{
#pragma clang fp contract(off)
    unsigned act = 0, up = 0;          // bit k of act: joint k is held; of up: on its upper bound
    bool done = false;
    slack = 0.0;
#pragma unroll 1
    for (int round = 0; round < 3 * NJ + 2; ++round) {
        double B[6][6], ep[6], y[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double a = v[r];
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                const double xk = ((act >> k) & 1u) ? (((up >> k) & 1u) ? hi[k] : lo[k]) : g[k];
                a = __builtin_fma(-jac[r * NJ + k], xk, a);
            }
            ep[r] = a;
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                double b = 0.0;
#pragma unroll
                for (int k = 0; k < NJ; ++k) b = __builtin_fma(((act >> k) & 1u) ? 0.0 : jac[r * NJ + k], jac[c * NJ + k], b);
                B[r][c] = r == c ? b + d2 : b;
            }
        }
        sched_fence();
        ldl_solve<6>(B, ep, y);
        sched_fence();
        int pick = -1, rel = -1;
        bool pick_up = false;
        double worst = 0.0, most = 0.0, ym = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) ym = fabs(y[r]) > ym ? fabs(y[r]) : ym;
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            double u = g[k];
#pragma unroll
            for (int r = 0; r < 6; ++r) u = __builtin_fma(jac[r * NJ + k], y[r], u);
            const bool held = (act >> k) & 1u, upper = (up >> k) & 1u;
            const double xk = upper ? hi[k] : lo[k];
            const double over = u - hi[k], under = lo[k] - u;
            const double viol = over > under ? over : under;
            if (!held && viol > worst) { worst = viol; pick = k; pick_up = over > under; }        // (strictly: the lowest index on a tie)
            const double mult = upper ? u - xk : xk - u;
            if (held && mult < most) { most = mult; rel = k; }
            dq[k] = held ? xk : u;
        }
        slack = d2 * ym;
        if (pick >= 0) {
            act |= 1u << pick;
            up = pick_up ? (up | (1u << pick)) : (up & ~(1u << pick));
        } else if (rel >= 0) {
            act &= ~(1u << rel);
        } else {
            done = true;               // (a lane that is done comes here again: the same set, the same numbers)
        }
        if (!wave_any(!done)) break;
    }
    return done;
}

// phase 2: the lane's own row -- the loop of the file comment, entirely in registers; Tep is read from the row where it is needed.
// live: the lane holds a row of the batch.  The loop is bounded by mp.steps and by nothing else: a lane that has arrived keeps its results and
// idles, the wave leaves when no lane is live, and an unsolvable row never arrives -- it runs out its steps.  A row that is not finite walks the
// chain on zeros and has its rate poisoned afterwards (rrmc_device.h: the library's sincos is a decision of the whole wave).
template <int NJ, class CV>
RTB_HD void mmc_lane(const MmcParams &mp, const CV &cv, bool live, double *mine)
{
#pragma clang fp contract(off)
    static_assert(NJ >= kMmcMin && NJ <= kMmcMax, "jacobm needs J J^T invertible; the register tile ends at 10 joints");
    const double *tep = mine + mmc_head(NJ);
    double *qd = mine + mmc_rate(NJ);
#pragma unroll
    for (int j = 0; j < NJ; ++j) qd[j] = 0.0;
    int its = 0, status = 0;
    bool arrived = false;
#pragma unroll 1
    for (int it = 0; it < mp.steps; ++it) {
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
            reg_core<NJ, true>(cv, mp.tail, 0, qs, P, jac);            // ONE walk, for jacob0: jacobm is defined on it
            sched_fence();      // the phases of an iteration one after the other
            double e[6], v[6];
            {
                const double te[12] = {P.r00, P.r01, P.r02, P.tx, P.r10, P.r11, P.r12, P.ty, P.r20, P.r21, P.r22, P.tz};
                if (mp.method == 1) servo_rpy_lane(te, tep, e);          // wave-uniform
                else aa_lane(te, tep, e);
            }
            sched_fence();
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) sum += fabs(e[k]);
            bad = bad || !(sum < __builtin_inf());
            const bool arr = !bad && sum < mp.threshold;
#pragma unroll
            for (int i = 0; i < 6; ++i) v[i] = mp.gain[i] * e[i];
            double g[NJ];
            if (mp.km > 0.0) {                                           // wave-uniform
                double jm[NJ];
                jacobm<NJ>(jac, 63, jm);
                const double sc = 1.0 / (mp.Y * mp.km);
#pragma unroll
                for (int j = 0; j < NJ; ++j) g[j] = sc * jm[j];
            } else {
#pragma unroll
                for (int j = 0; j < NJ; ++j) g[j] = 0.0;
            }
            sched_fence();
            if (mp.method == 1) {                                        // wave-uniform: jacobe = [R^T 0; 0 R^T] jacob0, in place
#pragma unroll
                for (int k = 0; k < NJ; ++k) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const double x = jac[(3 * h) * NJ + k], y = jac[(3 * h + 1) * NJ + k], z = jac[(3 * h + 2) * NJ + k];
                        jac[(3 * h) * NJ + k] = __builtin_fma(P.r20, z, __builtin_fma(P.r10, y, P.r00 * x));
                        jac[(3 * h + 1) * NJ + k] = __builtin_fma(P.r21, z, __builtin_fma(P.r11, y, P.r01 * x));
                        jac[(3 * h + 2) * NJ + k] = __builtin_fma(P.r22, z, __builtin_fma(P.r12, y, P.r02 * x));
                    }
                }
                sched_fence();
            }
            double lo[NJ], hi[NJ], x[NJ], slack;
            const bool box = mmc_box<NJ>(mp, qs, lo, hi);
            const bool kkt = mmc_qp<NJ>(jac, v, mp.Y * sum / mp.ks, g, lo, hi, x, slack);
            sched_fence();
            bool fin = true;
#pragma unroll
            for (int k = 0; k < NJ; ++k) fin = fin && fabs(x[k]) < __builtin_inf();
            const bool solved = !bad && box && kkt && fin;
            status |= (solved ? 0 : 1) | (solved && slack > 10.0 ? 2 : 0);
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                const double r = solved ? x[k] : __builtin_nan("");
                qd[k] = r;
                mine[k] = mine[k] + mp.dt * r;
            }
            its = it + 1;
            arrived = arr && solved;
            live = !arrived;
        }
    }
    mine[NJ] = arrived ? 1.0 : 0.0;
    mine[NJ + 1] = (double)its;
    mine[NJ + 2] = (double)status;
}

// phase 3: the live rows out, each output one contiguous run (kin_vjp.h); a NULL output is not stored (wave-uniform)
RTB_HD void mmc_tile_flush(int n, int cnt, const double *lds, double *__restrict__ qd, double *__restrict__ q_out, uint8_t *__restrict__ arrived,
                           int32_t *__restrict__ its, uint8_t *__restrict__ status, int lane)
{
    const int stride = mmc_stride(n);
    if (qd) vjp_flush(lds + mmc_rate(n), stride, n, cnt, qd, lane);
    if (q_out) vjp_flush(lds, stride, n, cnt, q_out, lane);
    if (lane < cnt) {
        const double *mine = lds + lane * stride + n;
        if (arrived) arrived[lane] = mine[0] != 0.0 ? 1 : 0;
        if (its) its[lane] = (int32_t)mine[1];
        if (status) status[lane] = (uint8_t)(int)mine[2];
    }
}

#pragma clang fp contract(fast)
}  // namespace rtbhip
