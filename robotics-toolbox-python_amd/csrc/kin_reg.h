// kin_reg.h -- register-resident variant of the fused fkine + Jacobian tile for chains with a
// compile-time joint count NJ (1..8: every arm of BASELINE.json's configs except the 14-DOF YuMi).
//
// Why a second variant: the run-time-n tile (kin_tile.h) keeps the per-joint (p_j, z_j) scratch in
// LDS because a register array cannot be indexed by a run-time joint number.  That costs 8(6n+qw)
// bytes of LDS per lane -- 25 KB per wave for the Panda -- which caps a CU at 6 waves and leaves the
// kernel latency-bound (first MI355X measurement: 0.178 ms / 1e6 configs = 36 % of the HBM roof,
// ~28k cycles of mostly-stalled wave lifetime).  With NJ a template parameter the canonical
// segment walk is one straight-line block -- no branches, no interpreter -- in which
//   * all NJ sin/cos pairs are evaluated up front (NJ independent dependency chains for the
//     scheduler to interleave) before the pose-dependent products start;
//   * p_j, z_j, sin_j, cos_j are named registers; q is read straight into registers;
//   * LDS is only the output transposer, time-shared in rounds of 32 lanes for J and one round of
//     64 for T: 32*(6n+1)*8 B = 11 KB per wave for n = 7  =>  occupancy is set by VGPRs, not LDS.
#pragma once
#include "kin_tile.h"
#include "trig.h"

namespace rtbhip {

constexpr int kRegMaxJoints = 8;    // register-resident consumers (IK, Hessian, jacob_dot, manipulability ...)
constexpr int kIkMaxJoints = 16;    // IK: chains of 9..12 joints run at one wave per SIMD (the whole 512-register budget); 13..16 also compile
                                    // -- their normal equations no longer fit the register file and spill to scratch: slow, but served
constexpr int kKinRegMax = 10;      // fkine / Jacobian tiles: 9 and 10 joints still fit the register file at 2 waves per SIMD
#ifndef RTB_JROUND
#define RTB_JROUND 32
#endif
constexpr int kJRound = RTB_JROUND;  // lanes staged per J round

RTB_HD int reg_lds_doubles(int n)
{
    const int a = kJRound * (6 * n + 1), b = kWave * 17;
    return a > b ? a : b;
}

// packed (T | J) rows: lanes staged per round -- each round holds kPRound x (17 + 6n + 1) doubles of LDS (n = 7, 16 lanes: 7.7 KB per wave)
#ifndef RTB_PROUND
#define RTB_PROUND 16
#endif
constexpr int kPRound = RTB_PROUND;
RTB_HD int reg_lds_doubles_packed(int n) { return kPRound * (17 + 6 * n + 1); }

// Per-lane core: joint values qv[] (chain order, as the caller holds them) -> P = C_0 Z_0 ... tail and
// the finished Jacobian in registers.  jac slot r*NJ + j : rows 0..2 = p_j, rows 3..5 = z_j until
// the closing loop finishes them.  Used by the tile kernel (reg_compute) and by the IK loop.
// (k_ik choosing a segment's product by a RUN-TIME switch on its structure class -- kin_device.h: pose_mul_seg_cls -- measured slower than the general
// product, round 5 visit c; what ships is the COMPILE-TIME form below.  profiles/retired_switches.md)
// A chain's STRUCTURE SIGNATURE: 7 bits per constant segment C_0 .. C_n (class | translation mask << 4, rtbhip_internal.h: kSeg*), bit 63 = "present".
// reg_core<..., SIG != 0> multiplies by every segment through pose_mul_seg_sig<class, mask>: straight-line code, no descriptor is read.  A
// kernel instantiated for a signature serves exactly the chains whose table has it (ik_kernels.hip: the launcher compares).
// (SegSig and its accessors: rtbhip_internal.h)
inline SegSig chain_signature(const int32_t *jmeta, int n)      // host: from the descriptors chain.cpp wrote (n joints + the tail's word)
{
    if (n > 8) return 0;
    SegSig s = kSegSigPresent;
    for (int j = 0; j <= n; ++j) s |= seg_sig_of(j, jm_cls(jmeta[j]), jm_tmask(jmeta[j]));
    return s;
}
// The built-in structure signatures: k_kin_reg (kin_kernels.hip) and k_ik (ik_kernels.hip) have straight-line instantiations for each.  A signature is
// a property of the robot's constants; the launchers compare a chain's own with this list and fall back to the general kernel.
//   Franka Panda as the reference models it (models/ETS/Panda.py:32-54), BASELINE config 3's arm: C_0 = tz, C_1 .. C_6 quarter turns about x with
//   translations on some axes, the flange Rz(-pi/4) tz(0.103) as the tail.
constexpr SegSig kSigPandaETS = kSegSigPresent | seg_sig_of(0, kSegIdentity, 4) | seg_sig_of(1, kSegRxN, 0) | seg_sig_of(2, kSegRxP, 6) | seg_sig_of(3, kSegRxP, 1) |
                                seg_sig_of(4, kSegRxN, 7) | seg_sig_of(5, kSegRxP, 0) | seg_sig_of(6, kSegRxP, 7) | seg_sig_of(7, kSegRz, 4);
//   The same arm read from its URDF (rtb-data franka_description, to the default end effector): the constants' tiny cos(pi/2) terms fall on other entries.
constexpr SegSig kSigPandaURDF = kSegSigPresent | seg_sig_of(0, kSegIdentity, 4) | seg_sig_of(1, kSegRxN, 0) | seg_sig_of(2, kSegRxP, 2) | seg_sig_of(3, kSegRxP, 1) |
                                 seg_sig_of(4, kSegRxN, 3) | seg_sig_of(5, kSegRxP, 0) | seg_sig_of(6, kSegRxP, 1) | seg_sig_of(7, kSegRz, 4);
//   Universal Robots UR3 / UR5 / UR10 from their URDFs (ur_description, to tool0): six joints, one signature for the three sizes.
constexpr SegSig kSigUR = kSegSigPresent | seg_sig_of(0, kSegIdentity, 4) | seg_sig_of(1, kSegGeneral, 2) | seg_sig_of(2, kSegIdentity, 5) | seg_sig_of(3, kSegRzP, 1) |
                          seg_sig_of(4, kSegPermA, 4) | seg_sig_of(5, kSegPermB, 4) | seg_sig_of(6, kSegGeneral, 4);
template <SegSig SIG, int J, class CV>
RTB_HD void pose_mul_seg_by_sig(Pose &P, const CV &cv) { pose_mul_seg_sig<seg_sig_cls(SIG, J), seg_sig_tm(SIG, J)>(P, cv, J); }
// (cv_has_trig / cv_t3fma, the chain views' traits: kin_device.h)
// joint J of the walk (compile-time index: a signature picks the segment's form by it)
template <int NJ, bool WANT_J, bool PLAIN, SegSig SIG, int J, class CV>
RTB_HD void reg_walk_step(const CV &cv, Pose &P, double (&jac)[6 * NJ], const int (&jmv)[NJ], const double (&c)[NJ], const double (&s)[NJ], const double (&d)[NJ])
{
    constexpr int j = J;
    {
#if defined(__HIP_DEVICE_COMPILE__)
        // Inside k_ik's persistent loop (the chain views that carry `trig`): tie segment j's table pointer to a value of step j - 1, so that its
        // scalar loads cannot be issued before the walk gets there.  Without this the loads of the later segments were issued early and their
        // results parked in VGPR lanes (v_writelane) until needed (v_readlane): 475 -> 251 such instructions in the kernel, 253 -> 244 VGPRs,
        // -2.4 % (config 3) ... -3.6 % (notebook setting) on one box (round 4 visit l).
        CV cvj = cv;
        // (a signature kernel reads two or three scalars per segment instead of twelve: there the pin and the fences only cost -- round 5
        // visits f, k, three interleaved rounds each: config 3 0.844 -> 0.833 -> 0.830 ms without them, outputs bit-identical)
        if (PLAIN && SIG == 0 && cv_has_trig<CV>::value && j > 0) asm volatile("" : "+s"(cvj.seg), "+v"(P.tx));
        if (j == 0) pose_from_seg(P, cvj, 0);
        else if constexpr (SIG != 0) pose_mul_seg_by_sig<SIG, J>(P, cvj);                                              // k_ik for a known robot: compile-time class
        else pose_mul_seg<((PLAIN && cv_has_trig<CV>::value) || cv_t3fma<CV>::value)>(P, cvj, j);
#else
        if (j == 0) pose_from_seg(P, cv, 0);
        else if constexpr (SIG != 0) pose_mul_seg_by_sig<SIG, J>(P, cv);
        else pose_mul_seg<cv_t3fma<CV>::value>(P, cv, j);
#endif
        if (WANT_J) {
            jac[j] = P.tx; jac[NJ + j] = P.ty; jac[2 * NJ + j] = P.tz;
            jac[3 * NJ + j] = P.r02; jac[4 * NJ + j] = P.r12; jac[5 * NJ + j] = P.r22;
        }
        // revolute: rotate by (c, s); prismatic: slide d -- a wave-uniform branch on the joint descriptor (s_cbranch)
        if (jm_prismatic(jmv[j])) pose_tz(P, d[j]);
        else pose_rotz(P, c[j], s[j]);
        if (SIG == 0) sched_fence();          // (signature kernels: no fence -- visit k: 0.8337 -> 0.8302 ms, every second one 0.8337)
    }
}
// joints J .. JEND - 1
template <int NJ, bool WANT_J, bool PLAIN, SegSig SIG, int J = 0, int JEND = NJ, class CV>
RTB_HD void reg_walk_steps(const CV &cv, Pose &P, double (&jac)[6 * NJ], const int (&jmv)[NJ], const double (&c)[NJ], const double (&s)[NJ], const double (&d)[NJ])
{
    if constexpr (J < JEND) {
        reg_walk_step<NJ, WANT_J, PLAIN, SIG, J>(cv, P, jac, jmv, c, s, d);
        reg_walk_steps<NJ, WANT_J, PLAIN, SIG, J + 1, JEND>(cv, P, jac, jmv, c, s, d);
    }
}

template <int NJ, bool WANT_J>
RTB_HD void reg_close_jacobian(const Pose &P, int frame, const int (&jmv)[NJ], double (&jac)[6 * NJ])
{
    if (WANT_J) {
#pragma clang fp contract(off)
        // Jv = z x (p_e - p), Jw = z (revolute) ; Jv = z, Jw = 0 (prismatic); flip negates
        // (methods.cpp:142-195); frame 1 rotates both halves by Re^T.
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            double zx = jac[3 * NJ + j], zy = jac[4 * NJ + j], zz = jac[5 * NJ + j];
            if (jm_flip(jmv[j])) { zx = -zx; zy = -zy; zz = -zz; }          // wave-uniform
            double vx, vy, vz, wx, wy, wz;
            if (jm_prismatic(jmv[j])) {                                      // wave-uniform
                vx = zx; vy = zy; vz = zz;
                wx = 0.0; wy = 0.0; wz = 0.0;
            } else {
                const double dx = P.tx - jac[j], dy = P.ty - jac[NJ + j], dz = P.tz - jac[2 * NJ + j];
                vx = mix_pm(zy, dz, zz, dy); vy = mix_pm(zz, dx, zx, dz); vz = mix_pm(zx, dy, zy, dx);      // (written out: kin_device.h, mix_pp)
                wx = zx; wy = zy; wz = zz;
            }
            if (frame == 1) {
                double a = vx, b = vy, e = vz;
                vx = dot3x(P.r00, a, P.r10, b, P.r20, e);
                vy = dot3x(P.r01, a, P.r11, b, P.r21, e);
                vz = dot3x(P.r02, a, P.r12, b, P.r22, e);
                a = wx; b = wy; e = wz;
                wx = dot3x(P.r00, a, P.r10, b, P.r20, e);
                wy = dot3x(P.r01, a, P.r11, b, P.r21, e);
                wz = dot3x(P.r02, a, P.r12, b, P.r22, e);
            }
            jac[j] = vx; jac[NJ + j] = vy; jac[2 * NJ + j] = vz;
            jac[3 * NJ + j] = wx; jac[4 * NJ + j] = wy; jac[5 * NJ + j] = wz;
        }
    }
}

// The constants a structure signature's walk reads, as VALUES: C_0 whole (pose_from_seg), of every later segment the rotation entries its class
// leaves general and the non-zero components of its translation (pose_mul_seg_sig: the others are never read) -- 12 + 26 doubles for the Panda ETS.
// Read from the table segment by segment inside the walk, each group of scalar loads was waited for where it was issued: nine round trips in
// series, which the first wave of a launch on a CU has nobody to hide behind.  Instead:
//   sig_touch   (reg_compute, behind the q loads) one word of every 64-byte line of the table: the lines are in the scalar cache by the time the
//               sines are done -- the words themselves are waited for together with the q values and dropped;
//   sig_fetch   (reg_core, behind the library-sincos branch, so nothing is parked across it) the constants in TWO clauses with one wait each: the
//               segments before sig_split at the head of the walk, the others two products before the first of them is used -- all at once they
//               overflow the scalar registers (the Panda's 76 beside the base transform's 24: 116 spilled, 320 bytes of scratch).  The walk then
//               finds them in registers.  A chain with more than kSigFetchMax such constants (the UR arms: 65) keeps the table's view and has the
//               touch alone.
// SigSegs is a view like the table's own (seg[j].r / .t), without the traits of the fused views: both steps are for the unfused views only (k_kin_reg);
// k_ik's and k_kin_diff's walks are not touched.
template <int NJ>
struct SigSegs {
    DevSeg seg[NJ + 1];
    const int32_t *jmeta;      // (a signature's walk is PLAIN: never read)
};
constexpr bool sig_reads_entry(SegSig sig, int j, int k /* 0..8: r[k], 9..11: t[k - 9] */)
{
    const int cls = seg_sig_cls(sig, j), tm = seg_sig_tm(sig, j);
    if (j == 0 || cls == kSegGeneral || ((RTB_SIG_UNFUSED_GENERAL >> cls) & 1)) return true;
    return k < 9 ? seg_kind(cls, k) == kCA : ((tm >> (k - 9)) & 1) != 0;
}
constexpr int sig_reads_count(SegSig sig, int j0, int j1, int k1 = 0)      // entries read of segments j0 .. j1 - 1, and of the first k1 of segment j1
{
    int m = 0;
    for (int a = j0; a <= j1; ++a)
        for (int b = 0; b < (a < j1 ? 12 : k1); ++b) m += sig_reads_entry(sig, a, b) ? 1 : 0;
    return m;
}
constexpr int kSigFetchMax = 40;      // doubles in the two clauses together (each is pinned by one statement of at most 30 operands)
constexpr int sig_split(SegSig sig, int nj)      // first segment of the second clause: the first clause holds at least half
{
    int h = 1;
    while (h <= nj && 2 * sig_reads_count(sig, 0, h) < sig_reads_count(sig, 0, nj + 1)) ++h;
    return h;
}
constexpr bool sig_fetches(SegSig sig, int nj)
{
    if (sig == 0 || nj > 8) return false;
    const int h = sig_split(sig, nj);
    return sig_reads_count(sig, 0, nj + 1) <= kSigFetchMax && sig_reads_count(sig, 0, h) <= 30 && sig_reads_count(sig, h, nj + 1) <= 30;
}
// f(IntC<j>, IntC<k>, IntC<slot>) for every entry the walk reads of segments J0 .. J1 - 1, slot = 0, 1, ... in table order: all three are
// compile-time numbers in f (a loop's would be constants only after unrolling, and the slot arithmetic did not fold: the values went to scratch)
template <int V> struct IntC { static constexpr int v = V; };
template <SegSig SIG, int J0, int J1, int I = 12 * J0, class F>
RTB_HD void sig_each(F f)
{
    if constexpr (I < 12 * J1) {
        if constexpr (sig_reads_entry(SIG, I / 12, I % 12)) f(IntC<I / 12>(), IntC<I % 12>(), IntC<sig_reads_count(SIG, J0, I / 12, I % 12)>());
        sig_each<SIG, J0, J1, I + 1>(f);
    }
}
// segments J0 .. J1 - 1 of the table into the view (the entries nothing reads stay as they are)
template <SegSig SIG, int NJ, int J0, int J1, class CV>
RTB_HD void sig_fetch(const CV &cv, SigSegs<NJ> &cs)
{
    static_assert(!cv_fused_translation<CV>::value, "the unfused views' reading pattern");
    sig_each<SIG, J0, J1>([&](auto j, auto k, auto) {
        if constexpr (k.v < 9) cs.seg[j.v].r[k.v] = cv.seg[j.v].r[k.v];
        else cs.seg[j.v].t[k.v - 9] = cv.seg[j.v].t[k.v - 9];
    });
#if defined(__HIP_DEVICE_COMPILE__)
    // All of them live in scalar registers HERE, or the loads are handed out along the walk again, one by one with a wait each.  ONE statement takes
    // them all as operands (the last one again in the unused places), because a load is placed in front of the first statement that needs it: a
    // statement per value put most of the loads, and a wait each, between the statements.  The fences keep the walk's arithmetic from moving up
    // past it, which would come to the same.
    constexpr int m = sig_reads_count(SIG, J0, J1);
    static_assert(m >= 1 && m <= 30, "one statement's operands");
    double v[m];
    sig_each<SIG, J0, J1>([&](auto j, auto k, auto slot) {
        if constexpr (k.v < 9) v[slot.v] = cs.seg[j.v].r[k.v];
        else v[slot.v] = cs.seg[j.v].t[k.v - 9];
    });
#define RTB_PIN(i) "s"(v[(i) < m ? (i) : m - 1])
    sched_fence();
    asm volatile("" ::RTB_PIN(0), RTB_PIN(1), RTB_PIN(2), RTB_PIN(3), RTB_PIN(4), RTB_PIN(5), RTB_PIN(6), RTB_PIN(7), RTB_PIN(8), RTB_PIN(9), RTB_PIN(10),
                 RTB_PIN(11), RTB_PIN(12), RTB_PIN(13), RTB_PIN(14), RTB_PIN(15), RTB_PIN(16), RTB_PIN(17), RTB_PIN(18), RTB_PIN(19), RTB_PIN(20),
                 RTB_PIN(21), RTB_PIN(22), RTB_PIN(23), RTB_PIN(24), RTB_PIN(25), RTB_PIN(26), RTB_PIN(27), RTB_PIN(28), RTB_PIN(29));
    sched_fence();
#undef RTB_PIN
#endif
}
#if defined(__HIP_DEVICE_COMPILE__)
// one word of each 64-byte line of the NJ + 1 segments (the table starts a device allocation: line-aligned); nothing past the table is read
template <int NJ, class CV>
__device__ __forceinline__ void sig_touch(const CV &cv)
{
    const auto *w = (const __attribute__((address_space(4))) int32_t *)cv.seg;
    int any = 0;
#pragma unroll
    for (int b = 0; b < (NJ + 1) * (int)sizeof(DevSeg); b += 64) any |= w[b / 4];
    asm volatile("" ::"s"(any));
}
#endif

// PLAIN (compile-time): every joint is revolute and none is flipped (the caller checked the chain's descriptors): no descriptor is read, no
// wave-uniform branch splits the walk -- one straight-line block from the first sine to the last Jacobian column.
template <int NJ, bool WANT_J, bool PLAIN = false, SegSig SIG = 0, class CV, class TL>
RTB_HD void reg_core(const CV &cv, TL tail /* tail[k], k = 0..11 */, int frame, const double (&qv)[NJ], Pose &P,
                     double (&jac)[6 * NJ])
{
    static_assert(SIG == 0 || (PLAIN && NJ <= 8), "a structure signature goes with the straight-line walk");
    double c[NJ], s[NJ], d[NJ];
    // Wave-uniform per-joint blend weights instead of per-lane selects: rv = 1 for a revolute joint,
    // pv = 1 for a prismatic one, sg = -1 where the joint is flipped.  They are re-derived from the
    // one-dword joint descriptor at every use (a few SALU ops) rather than kept as 3*NJ SGPR doubles
    // across the whole walk: inside the persistent IK loop those 42 SGPRs were what overflowed the
    // scalar register file.
    int jmv[NJ];
    bool big = false;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {   // methods.cpp:363-366 for flip
        jmv[j] = PLAIN ? 0 : cv.jmeta[j];
        d[j] = PLAIN ? qv[j] : qv[j] * (jm_flip(jmv[j]) ? -1.0 : 1.0);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {   // NJ independent evaluations, one basic block
        if constexpr (cv_has_trig<CV>::value) sincos_reduced_tab(d[j], s[j], c[j], cv.trig);
        else sincos_reduced(d[j], s[j], c[j]);
        big = big || !(fabs(d[j]) < kTrigFastLimit);
    }
    if (wave_any(big)) {             // |q| >= 2^20, NaN, inf: library path for the whole wave
#pragma unroll
        for (int j = 0; j < NJ; ++j) sincos(d[j], &s[j], &c[j]);
    }
    if constexpr (sig_fetches(SIG, NJ) && !cv_fused_translation<CV>::value) {      // k_kin_reg's signature walk: its constants in two clauses (sig_fetch)
        constexpr int H = sig_split(SIG, NJ), E = H >= 2 ? H - 2 : 0;      // joint E's product is the second before segment H's
        SigSegs<NJ> cs = {};
        sig_fetch<SIG, NJ, 0, H>(cv, cs);
        reg_walk_steps<NJ, WANT_J, PLAIN, SIG, 0, E>(cs, P, jac, jmv, c, s, d);
        if constexpr (H <= NJ) sig_fetch<SIG, NJ, H, NJ + 1>(cv, cs);
        reg_walk_steps<NJ, WANT_J, PLAIN, SIG, E, NJ>(cs, P, jac, jmv, c, s, d);
        pose_mul_seg_by_sig<SIG, NJ>(P, cs);
        sched_fence();
        reg_close_jacobian<NJ, WANT_J>(P, frame, jmv, jac);
        return;
    }
    reg_walk_steps<NJ, WANT_J, PLAIN, SIG>(cv, P, jac, jmv, c, s, d);
    // k_ik's chain views: the tail IS segment NJ of the table (no tool in IK), descriptor NJ carries its class
    if constexpr (SIG != 0) pose_mul_seg_by_sig<SIG, NJ>(P, cv);
    else pose_mul_general<((PLAIN && cv_has_trig<CV>::value) || cv_t3fma<CV>::value)>(P, [&](int k) { return tail[k]; });
    sched_fence();
    reg_close_jacobian<NJ, WANT_J>(P, frame, jmv, jac);
}

// whole per-lane compute of one tile: q row in memory -> (P, J)
// SIG != 0: the chain's structure signature (all joints revolute, none flipped, no tool: the tail is segment NJ of the table) -- the straight-line walk
// S: the storage type of q (kin_tile.h): a float row is read with the same per-lane accesses, half as wide -- the wave's 64 rows are one contiguous
// run of 64 * 4 qw bytes whose lines the NJ loads of the wave consume whole between them -- and widened here; everything after is fp64
template <int NJ, bool WANT_J, SegSig SIG = 0, class CV, class S>
RTB_HD void reg_compute(const KinParams &kp, const CV &cv, const S *__restrict__ q, int64_t cfg,
                        Pose &P, double (&jac)[6 * NJ])
{
    const bool live = cfg < kp.N;
    double qv[NJ];
    if constexpr (SIG != 0) {
        // the launch's ramp is this kernel's to shorten: the NJ column words first, then NJ loads with nothing between them -- a dead lane reads
        // row 0 (N >= 1) instead of branching round its load, which put a scalar load, its wait and a branch in front of every q load
        // (the column words passed in the kernarg instead, so that the q loads wait for one scalar round trip, were not shown to gain -- nothing at a
        // resident round, one wave inside its process-to-process scatter -- and are not in: profiles/r08_kin_wave_latency.txt)
        const S *qrow = q + (live ? cfg : 0) * kp.qw;
        int jq[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) jq[j] = jm_jq(cv.jmeta[j]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) qv[j] = qrow[jq[j]];
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (!cv_fused_translation<CV>::value) sig_touch<NJ>(cv);      // the table's lines, on their way while the q values are (sig_fetch, above)
#endif
#pragma unroll
        for (int j = 0; j < NJ; ++j) qv[j] = live ? qv[j] : 0.0;
        reg_core<NJ, WANT_J, true, SIG>(cv, &cv.seg[NJ].r[0], kp.frame, qv, P, jac);
    } else {
        const S *qrow = q + cfg * kp.qw;
#pragma unroll
        for (int j = 0; j < NJ; ++j) qv[j] = live ? qrow[jm_jq(cv.jmeta[j])] : 0.0;
        reg_core<NJ, WANT_J>(cv, kp.tail, kp.frame, qv, P, jac);
    }
}

// staging: lane writes its finished J row / its 4x4 into the wave's LDS transposer
template <int NJ>
RTB_HD void reg_stage_J(const double (&jac)[6 * NJ], double *buf, int slot_lane)
{
    double *mine = buf + slot_lane * (6 * NJ + 1);
#pragma unroll
    for (int k = 0; k < 6 * NJ; ++k) mine[k] = jac[k];
}

// packed rows: the lane's 4x4 (base applied) into the T area, its J into the J area of the same round (kin_flush_packed)
template <int NJ>
RTB_HD void reg_stage_packed(const KinParams &kp, Pose P, const double (&jac)[6 * NJ], double *bufT, double *bufJ, int slot_lane)
{
    if (kp.has_base) pose_premul(P, kp.base);
    double *mt = bufT + slot_lane * 17;
    pose_store16(P, [&](int k, double v) { mt[k] = v; });
    double *mj = bufJ + slot_lane * (6 * NJ + 1);
#pragma unroll
    for (int k = 0; k < 6 * NJ; ++k) mj[k] = jac[k];
}

RTB_HD void reg_stage_T(const KinParams &kp, Pose P, double *buf, int lane)
{
    if (kp.has_base) pose_premul(P, kp.base);
    double *mine = buf + lane * 17;
    pose_store16(P, [&](int k, double v) { mine[k] = v; });
}

}  // namespace rtbhip
