// tree_coriolis_vjp_kernels.hip -- gfx950 kernels for the VECTOR-JACOBIAN PRODUCT of the batched Coriolis / centripetal matrix of an ETS / URDF
// robot (rtbhip_tree_coriolis_vjp):
//
//     gq [r,m] = sum_jk gC[r,j,k] d C[r,j,k] / d q [r,m]
//     gqd[r,m] = sum_jk gC[r,j,k] d C[r,j,k] / d qd[r,m]
//
// for robots numbered in group order (group j moves q column j: every URDF robot, every robot whose jindex was assigned automatically), every joint
// kind the forward call serves.  The forward kernel (tree_device.h: tree_bilinear_core) computes C[j,k] = 1/2 B_j(u = qd, w = e_k) from the
// TWO-FIELD spatial-vector recursion: Robot.rne without gravity and acceleration, every product of two velocities x(v) y(v) replaced by
// x(u) y(w) + x(w) y(u).  B_j is linear in w, so  sum_k gC[j,k] B_j(u, e_k) = B_j(u, gC[j,:]):  the adjoint is the sum over the ROWS j of gC of the
// reverse-mode sweep of one two-field pass whose w field has the joint rates gC[j,:] and whose only seeded torque is 1/2 on joint j (pass layout
// (b), as coriolis_vjp_kernels.hip).  gC is a constant of the differentiation; gqd is the adjoint of the u field's joint rates.
//
// The lane body is tree_rne_vjp_lane (tree_rne_vjp_kernels.hip, whose header has the single-field formulas) with both fields carried.  With qu = qd_l,
// qw = gC[j,l], p the parent group:
//     u_l = X_l u_p + s_l qu      w_l = X_l w_p + s_l qw      a_l = X_l a_p + crm(u_l) s_l qw + crm(w_l) s_l qu
//     f_l = I_l a_l + crf(u_l) I_l w_l + crf(w_l) I_l u_l + sum over children X_c^T f_c          tau_l = s_l . f_l
// and for the force adjoint fbar_l (sweep 3, unchanged) and the adjoints ubar, wbar, abar (sweep 4):
//     abar_l = I_l fbar_l + (children)
//     ubar_l = I_l crm(fbar_l) w_l - crf(fbar_l) I_l w_l + qw crf(s_l) abar_l + (children)        wbar_l: the same with u in place of w and qu for qw
//     gqd_l = s_l . ubar_l + abar_l . crm(w_l) s_l
//     gq_l  = -sigma_l [ (crm(s_l) y) . ybar  summed over  y = X_l fbar_p (with f_l), X_l u_p, X_l w_p, X_l a_p ]
// Tape: f = 6 doubles per group in registers -- and NOT u, w, a.  Taped, the two-field state is 24 doubles per group and six groups spill
// (measured: 114 spilled registers).  Sweep 4 walks tip -> base, and where group j + 1 hangs directly off group j it runs the joint of j + 1
// BACKWARDS,  X y_p = y - (joint terms),  y_p = X^-1 (X y_p),  which is the hand-down of sweep 4 itself applied to motion vectors; only the groups it
// cannot reach that way -- the last group, every leaf, every group whose children read it through a branch slot -- are KEPT: sweep 1 writes their
// 18 doubles to a per-lane store in LDS (the run-time-n form: private memory), sweep 4 reads them back in reverse order.  A serial chain keeps
// one group.  One lane = one sample; sin / cos once per lane, then a `#pragma unroll 1` loop over the passes, each kept self-contained by
// tree_opaque; gq and gqd accumulate in 2 n registers (the part of the joint variable's adjoint that sweep 3 finds goes straight into gq's).  Branch slots: the
// forward kernel's 24 doubles -- sweeps 1, 2: u, w, a of the group that saves there and the force accumulator of its children; sweeps 3, 4: its fbar
// and the accumulators of ubar, wbar, abar -- initialised at the head of every pass and again at the head of sweep 3.
// I/O as k_coriolis_vjp: lane-major LDS tile of  q (n) | qd (n) | gC (n^2)  doubles per row at an odd stride (run-time-n form: q | qd | one row of
// gC, staged per pass), then the branch slots and the kept states, [double][lane]; gq and gqd overwrite the q and qd slots and leave as contiguous non-temporal
// stores.
#include "tree_kernels.h"
#include "vjp_tile.h"

namespace rtbhip {

#pragma clang fp contract(off)      // every operation written out, as in tree_device.h

constexpr int kTreeCoriolisVjpMaxGroups = 20;      // the forward kernel's built-in sizes (tree_dyn_kernels.hip: kTreeDynMax)
constexpr int kTcSD = kTreeBilinearSlotDoubles;

RTB_HD V3 tc_zero() { return v3(0, 0, 0); }
RTB_HD V3 tc_zx(double s, V3 v, V3 acc) { return v3(__builtin_fma(-s, v.y, acc.x), __builtin_fma(s, v.x, acc.y), acc.z); }      // acc + (0, 0, s) x v
// I [l; a] = [M l + a x h; I_bar a + h x l]  (symmetric: it is its own transpose)
template <class G> RTB_HD void tc_inertia(const G &g, V3 l, V3 a, V3 &ol, V3 &oa)
{
    const V3 h = v3(g.h[0], g.h[1], g.h[2]);
    ol = cross_add(a, h, g.M * l);
    oa = cross_add(h, l, inertia_rot(g, a));
}
// xbar += I (crm(fbar) y) - crf(fbar) (I y):  the adjoint of  crf(x) I y + crf(y) I x  with respect to x
template <class G> RTB_HD void tc_bilinear_bar(const G &g, V3 fbl, V3 fba, V3 yl, V3 ya, V3 &xbl, V3 &xba)
{
    V3 tl, ta, Iyl, Iya;
    tc_inertia(g, yl, ya, Iyl, Iya);
    const V3 wl = cross_add(fbl, ya, cross(fba, yl)), wa = cross(fba, ya);
    tc_inertia(g, wl, wa, tl, ta);
    xbl = cross_add(Iyl, fba, xbl + tl);
    xba = cross_add(Iyl, fbl, cross_add(Iya, fba, xba + ta));
}

// One sample.  groups: the wave-uniform group table, group j on q column j.  qin(l), qdin(l): the joint variables and rates, readable until the
// last pass is over.  begin(j): called at the head of pass j.  gin(j, l): gC[j,l], read during pass j only.  gq(l, v), gqd(l, v): called once per
// joint, after the last pass.  slot(index) -> double& into this lane's kTreeBilinearSlotDoubles * nslots scratch; store(index) -> double& into its
// 18 doubles per kept group.  NG = 0: run-time group count
// n_rt (<= kTreeCoriolisVjpMaxGroups), the per-group arrays in private memory.
template <int NG, class GroupsP, class InQ, class InQd, class Begin, class InG, class OutQ, class OutQd, class Slot, class Store>
RTB_HD void tree_coriolis_vjp_lane(GroupsP groups, int n_rt, int nslots, InQ qin, InQd qdin, Begin begin, InG gin, OutQ gq, OutQd gqd, Slot slot,
                                   Store store)
{
#pragma clang fp contract(off)
    constexpr int CAP = NG > 0 ? NG : kTreeCoriolisVjpMaxGroups;
    const int n = NG > 0 ? NG : n_rt;
    double sn[CAP], cs[CAP], accq[CAP], accd[CAP];
    V3 FL[CAP], FA[CAP];
    if constexpr (NG > 0) {
        tree_trig<NG>(groups, qin, sn, cs);
    } else {
        for (int j = 0; j < n; ++j) {
            const auto &g = groups[j];
            const double t = jm_prismatic(g.jmeta) ? 0.0 : qin(j) * (jm_flip(g.jmeta) ? -1.0 : 1.0);
            double s, c;
            sincos(t, &s, &c);
            sn[j] = s; cs[j] = c;
        }
    }
#pragma unroll
    for (int j = 0; j < n; ++j) { accq[j] = 0.0; accd[j] = 0.0; }
    auto slide = [&](const auto &g, int j) { return jm_prismatic(g.jmeta) ? qin(j) * (jm_flip(g.jmeta) ? -1.0 : 1.0) : 0.0; };
    // group j hands its state to sweep 4 through the store unless group j + 1 hangs off it directly (then sweep 4 runs the joint of j + 1 backwards)
    auto kept = [&](int j) { return j + 1 >= n || !(groups[j + 1].parent == j && groups[j + 1].parent_slot < 0); };

#pragma unroll 1
    for (int i = 0; i < (n > 1 ? n : 0); ++i) {
        if constexpr (NG > 0) tree_opaque<NG>(sn, cs);
        begin(i);
        for (int k = 0; k < nslots; ++k)
            for (int e = 0; e < kTcSD; ++e) slot(k * kTcSD + e) = 0.0;

        // ---- 1. primal forward recursion, both fields: the group's own force (kept in registers); u, w, a of the kept groups go to the store
        int nkept = 0;
        {
            V3 ul = tc_zero(), ua = tc_zero(), wl = tc_zero(), wa = tc_zero(), al = tc_zero(), aa = tc_zero();
#pragma unroll
            for (int j = 0; j < n; ++j) {
                const auto &g = groups[j];
                const bool pris = jm_prismatic(g.jmeta) != 0;
                const double qdu = qdin(j), qdw = gin(i, j);
                V3 pul, pua, pwl, pwa, pal, paa;
                if (g.parent < 0) {
                    pul = tc_zero(); pua = tc_zero(); pwl = tc_zero(); pwa = tc_zero(); pal = tc_zero(); paa = tc_zero();
                } else if (g.parent_slot >= 0) {
                    const int b = g.parent_slot * kTcSD;
                    pul = vjp_slot_get(slot, b); pua = vjp_slot_get(slot, b + 3); pwl = vjp_slot_get(slot, b + 6); pwa = vjp_slot_get(slot, b + 9);
                    pal = vjp_slot_get(slot, b + 12); paa = vjp_slot_get(slot, b + 15);
                } else {
                    pul = ul; pua = ua; pwl = wl; pwa = wa; pal = al; paa = aa;
                }
                const V3 p = tree_origin(false, g, slide(g, j));
                const double s = sn[j], c = cs[j];
                ua = rz_t(s, c, seg_rt(g, pua));
                ul = rz_t(s, c, seg_rt(g, add_cross_ap(7, pul, pua, p)));
                wa = rz_t(s, c, seg_rt(g, pwa));
                wl = rz_t(s, c, seg_rt(g, add_cross_ap(7, pwl, pwa, p)));
                aa = rz_t(s, c, seg_rt(g, paa));
                al = rz_t(s, c, seg_rt(g, add_cross_ap(7, pal, paa, p)));
                if (pris) {
                    ul.z += qdu; wl.z += qdw;
                    al = crossz_add(wa, qdu, crossz_add(ua, qdw, al));
                } else {
                    ua.z += qdu; wa.z += qdw;
                    al = crossz_add(wl, qdu, crossz_add(ul, qdw, al));
                    aa = crossz_add(wa, qdu, crossz_add(ua, qdw, aa));
                }
                if (g.save_slot >= 0) {
                    const int b = g.save_slot * kTcSD;
                    vjp_slot_put(slot, b, ul); vjp_slot_put(slot, b + 3, ua); vjp_slot_put(slot, b + 6, wl); vjp_slot_put(slot, b + 9, wa);
                    vjp_slot_put(slot, b + 12, al); vjp_slot_put(slot, b + 15, aa);
                }
                if (kept(j)) {
                    const int b = nkept * 18;
                    vjp_slot_put(store, b, ul); vjp_slot_put(store, b + 3, ua); vjp_slot_put(store, b + 6, wl); vjp_slot_put(store, b + 9, wa);
                    vjp_slot_put(store, b + 12, al); vjp_slot_put(store, b + 15, aa);
                    ++nkept;
                }
                V3 Iul, Iua, Iwl, Iwa, Ial, Iaa;
                tc_inertia(g, ul, ua, Iul, Iua);
                tc_inertia(g, wl, wa, Iwl, Iwa);
                tc_inertia(g, al, aa, Ial, Iaa);
                FL[j] = cross_add(wa, Iul, cross_add(ua, Iwl, Ial));
                FA[j] = cross_add(wl, Iul, cross_add(ul, Iwl, cross_add(wa, Iua, cross_add(ua, Iwa, Iaa))));
                if (NG > 0) sched_fence();
            }
        }

        // ---- 2. primal backward recursion: own force -> total force f_j, in place, for the groups j > i (sweep 3 reads no force of a group <= i)
        {
            V3 cl = tc_zero(), ca = tc_zero();
#pragma unroll
            for (int jj = 0; jj < n; ++jj) {
                const int j = n - 1 - jj;
                if (j <= i) continue;
                const auto &g = groups[j];
                V3 fl = FL[j] + cl, fa = FA[j] + ca;
                if (g.save_slot >= 0) {
                    const int b = g.save_slot * kTcSD + 18;
                    fl = fl + vjp_slot_get(slot, b);
                    fa = fa + vjp_slot_get(slot, b + 3);
                }
                FL[j] = fl; FA[j] = fa;
                cl = tc_zero(); ca = tc_zero();
                if (g.parent >= 0) {
                    const V3 p = tree_origin(false, g, slide(g, j));
                    const V3 tl = seg_r(g, rz(sn[j], cs[j], fl));
                    const V3 ta = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], fa)), p, tl);
                    if (g.parent_slot >= 0) {
                        const int b = g.parent_slot * kTcSD + 18;
                        vjp_slot_add(slot, b, tl); vjp_slot_add(slot, b + 3, ta);
                    } else {
                        cl = tl; ca = ta;
                    }
                }
                if (NG > 0) sched_fence();
            }
        }

        // ---- 3. adjoint of the backward recursion, group i -> tip: f_j -> fbar_j in place.  The slots are dead by now: every one starts over as
        //         fbar = 0 (a group before i has no force adjoint) and empty accumulators for sweep 4
        for (int k = 0; k < nslots; ++k)
            for (int e = 0; e < kTcSD; ++e) slot(k * kTcSD + e) = 0.0;
        {
            V3 bl = tc_zero(), ba = tc_zero();      // fbar of the previous group
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (j < i) continue;
                const auto &g = groups[j];
                const bool pris = jm_prismatic(g.jmeta) != 0;
                V3 xl = tc_zero(), xa = tc_zero();       // X_j fbar_p
                double t = 0.0;
                if (j > i && g.parent >= 0) {            // (the parent of group i has no force adjoint)
                    V3 pbl = bl, pba = ba;
                    if (g.parent_slot >= 0) {
                        const int b = g.parent_slot * kTcSD;
                        pbl = vjp_slot_get(slot, b); pba = vjp_slot_get(slot, b + 3);
                    }
                    const V3 p = tree_origin(false, g, slide(g, j));
                    xa = rz_t(sn[j], cs[j], seg_rt(g, pba));
                    xl = rz_t(sn[j], cs[j], seg_rt(g, add_cross_ap(7, pbl, pba, p)));
                    t = pris ? -vjp_zcross(xa, FL[j]) : -(vjp_zcross(xl, FL[j]) + vjp_zcross(xa, FA[j]));
                }
                accq[j] = accq[j] + (jm_flip(g.jmeta) ? -t : t);
                if (j == i) { if (pris) xl.z += 0.5; else xa.z += 0.5; }
                FL[j] = xl; FA[j] = xa;
                if (g.save_slot >= 0) {
                    const int b = g.save_slot * kTcSD;
                    vjp_slot_put(slot, b, xl); vjp_slot_put(slot, b + 3, xa);
                }
                bl = xl; ba = xa;
                if (NG > 0) sched_fence();
            }
        }

        // ---- 4. adjoint of the forward recursion, tip -> base (the force terms of the groups j >= i; the joint and the hand-down of every group)
        {
            V3 cul = tc_zero(), cua = tc_zero(), cwl = tc_zero(), cwa = tc_zero(), cal = tc_zero(), caa = tc_zero();      // X^T (ubar, wbar, abar) from group j + 1
            V3 rul = tc_zero(), rua = tc_zero(), rwl = tc_zero(), rwa = tc_zero(), ral = tc_zero(), raa = tc_zero();      // the state of group j as group j + 1 ran it back
#pragma unroll
            for (int jj = 0; jj < n; ++jj) {
                const int j = n - 1 - jj;
                const auto &g = groups[j];
                const bool pris = jm_prismatic(g.jmeta) != 0;
                const double sigma = jm_flip(g.jmeta) ? -1.0 : 1.0;
                const double qdu = qdin(j), qdw = gin(i, j);
                V3 ul = rul, ua = rua, wl = rwl, wa = rwa, al = ral, aa = raa;
                if (kept(j)) {
                    --nkept;
                    const int b = nkept * 18;
                    ul = vjp_slot_get(store, b); ua = vjp_slot_get(store, b + 3); wl = vjp_slot_get(store, b + 6); wa = vjp_slot_get(store, b + 9);
                    al = vjp_slot_get(store, b + 12); aa = vjp_slot_get(store, b + 15);
                }
                V3 ubl = cul, uba = cua, wbl = cwl, wba = cwa, abl = cal, aba = caa;
                if (g.save_slot >= 0) {
                    const int b = g.save_slot * kTcSD + 6;
                    ubl = ubl + vjp_slot_get(slot, b); uba = uba + vjp_slot_get(slot, b + 3);
                    wbl = wbl + vjp_slot_get(slot, b + 6); wba = wba + vjp_slot_get(slot, b + 9);
                    abl = abl + vjp_slot_get(slot, b + 12); aba = aba + vjp_slot_get(slot, b + 15);
                }
                if (j >= i) {
                    // the group's own force  I a + crf(u) I w + crf(w) I u
                    const V3 fbl = FL[j], fba = FA[j];
                    V3 tl, ta;
                    tc_inertia(g, fbl, fba, tl, ta);
                    abl = abl + tl; aba = aba + ta;
                    tc_bilinear_bar(g, fbl, fba, wl, wa, ubl, uba);
                    tc_bilinear_bar(g, fbl, fba, ul, ua, wbl, wba);
                }
                // the joint:  a = X a_p + crm(u) s qw + crm(w) s qu,  u = X u_p + s qu,  w = X w_p + s qw
                double t, oqd;
                V3 xal, xaa;          // X a_p
                if (pris) {
                    uba = tc_zx(qdw, abl, uba);
                    wba = tc_zx(qdu, abl, wba);
                    oqd = ubl.z + vjp_zcross(abl, wa);
                    t = -((vjp_zcross(ua, ubl) + vjp_zcross(wa, wbl)) + vjp_zcross(aa, abl));
                    xal = v3(__builtin_fma(-qdu, wa.y, __builtin_fma(-qdw, ua.y, al.x)), __builtin_fma(qdu, wa.x, __builtin_fma(qdw, ua.x, al.y)), al.z);
                    xaa = aa;
                } else {
                    ubl = tc_zx(qdw, abl, ubl); uba = tc_zx(qdw, aba, uba);
                    wbl = tc_zx(qdu, abl, wbl); wba = tc_zx(qdu, aba, wba);
                    oqd = uba.z + (vjp_zcross(abl, wl) + vjp_zcross(aba, wa));
                    xal = v3(__builtin_fma(-qdu, wl.y, __builtin_fma(-qdw, ul.y, al.x)), __builtin_fma(qdu, wl.x, __builtin_fma(qdw, ul.x, al.y)), al.z);
                    xaa = v3(__builtin_fma(-qdu, wa.y, __builtin_fma(-qdw, ua.y, aa.x)), __builtin_fma(qdu, wa.x, __builtin_fma(qdw, ua.x, aa.y)), aa.z);
                    t = -(((vjp_zcross(ul, ubl) + vjp_zcross(ua, uba)) + (vjp_zcross(wl, wbl) + vjp_zcross(wa, wba))) + (vjp_zcross(xal, abl) + vjp_zcross(xaa, aba)));
                }
                accq[j] = accq[j] + sigma * t;
                accd[j] = accd[j] + oqd;
                cul = tc_zero(); cua = tc_zero(); cwl = tc_zero(); cwa = tc_zero(); cal = tc_zero(); caa = tc_zero();
                if (g.parent >= 0) {
                    const V3 p = tree_origin(false, g, slide(g, j));
                    const V3 hul = seg_r(g, rz(sn[j], cs[j], ubl));
                    const V3 hua = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], uba)), p, hul);
                    const V3 hwl = seg_r(g, rz(sn[j], cs[j], wbl));
                    const V3 hwa = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], wba)), p, hwl);
                    const V3 hal = seg_r(g, rz(sn[j], cs[j], abl));
                    const V3 haa = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], aba)), p, hal);
                    if (g.parent_slot >= 0) {
                        const int b = g.parent_slot * kTcSD + 6;
                        vjp_slot_add(slot, b, hul); vjp_slot_add(slot, b + 3, hua); vjp_slot_add(slot, b + 6, hwl); vjp_slot_add(slot, b + 9, hwa);
                        vjp_slot_add(slot, b + 12, hal); vjp_slot_add(slot, b + 15, haa);
                    } else {
                        cul = hul; cua = hua; cwl = hwl; cwa = hwa; cal = hal; caa = haa;
                        // ... and the joint run backwards: the state of the parent, group j - 1, from  X u_p = u - s qu,  X w_p = w - s qw,  X a_p
                        const V3 xul = pris ? v3(ul.x, ul.y, ul.z - qdu) : ul, xua = pris ? ua : v3(ua.x, ua.y, ua.z - qdu);
                        const V3 xwl = pris ? v3(wl.x, wl.y, wl.z - qdw) : wl, xwa = pris ? wa : v3(wa.x, wa.y, wa.z - qdw);
                        rua = seg_r(g, rz(sn[j], cs[j], xua));
                        rul = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], xul)), p, rua);
                        rwa = seg_r(g, rz(sn[j], cs[j], xwa));
                        rwl = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], xwl)), p, rwa);
                        raa = seg_r(g, rz(sn[j], cs[j], xaa));
                        ral = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], xal)), p, raa);
                    }
                }
                if (NG > 0) sched_fence();
            }
        }
    }
#pragma unroll
    for (int j = 0; j < n; ++j) { gq(j, accq[j]); gqd(j, accd[j]); }
}

#ifndef RTB_TREE_CORIOLIS_VJP_LANE_ONLY      // (a host-side replay of the lane body includes this file for tree_coriolis_vjp_lane alone)

constexpr int kTreeCoriolisVjpRegMax = 8;      // the largest compile-time group count (DESIGN 4.16 has the register table)

struct TreeCoriolisVjpParams {
    int32_t n, nslots;
    int64_t N;
};

// LDS row of one sample at an odd stride: q (n) | qd (n) | gC (n^2) for a compile-time group count, q | qd | one row of gC for the run-time-n form;
// then the branch slots and, for a compile-time group count, the kept states, [double][lane]
inline __host__ __device__ int tree_coriolis_vjp_stride(int n, bool rt) { return (2 * n + (rt ? n : n * n)) | 1; }

// One tile of 64 samples.  gq / gqd NULL: not stored.  The flush is vjp_tile.h's phase; the staging is this unit's own: with the staging
// phases in its place UR5's adjoint measured 3 to 5 % slower (profiles/vjp_tile_refactor_ab.json).
template <int NG>
__device__ __forceinline__ void tree_coriolis_vjp_tile(const TreeCoriolisVjpParams &tp, ConstGroups groups, int n, int64_t tile,
                                                       const double *__restrict__ q, const double *__restrict__ qd, const double *__restrict__ gC,
                                                       double *__restrict__ gq, double *__restrict__ gqd, double *lds, int lane)
{
    const int stride = tree_coriolis_vjp_stride(n, NG == 0);
    double *slots = lds + kWave * stride;
    const VjpTile t = vjp_tile_of(tile, tp.N, n);
    const int64_t cfg0 = t.cfg0;
    const int ncfg = t.ncfg;
    const int nn = n * n;
    const int count = t.count, mcount = t.mcount;
    const double *qg = q + cfg0 * n, *dg = qd + cfg0 * n, *mg = gC + cfg0 * nn;
    if constexpr (NG > 0) {
        // all 2 NG + NG^2 coalesced loads in flight before the first LDS write (vjp_tile.h tells why): unconditional -- an element past the ragged tail
        // reads element 0 of the tile -- and the zeros are selected afterwards
        double rq[NG], rd[NG], rm[NG * NG];
#pragma unroll
        for (int k = 0; k < NG; ++k) { const int f = lane + kWave * k, fc = f < count ? f : 0; rq[k] = qg[fc]; rd[k] = dg[fc]; }
#pragma unroll
        for (int k = 0; k < NG * NG; ++k) { const int f = lane + kWave * k; rm[k] = mg[f < mcount ? f : 0]; }
        sched_fence();
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int f = lane + kWave * k;
            double *dst = lds + (f / NG) * stride + (f % NG);
            dst[0] = f < count ? rq[k] : 0.0;
            dst[NG] = f < count ? rd[k] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < NG * NG; ++k) {
            const int f = lane + kWave * k;
            lds[(f / (NG * NG)) * stride + 2 * NG + (f % (NG * NG))] = f < mcount ? rm[k] : 0.0;
        }
    } else {
        for (int f = lane; f < kWave * n; f += kWave) {
            double *dst = lds + (f / n) * stride + (f % n);
            dst[0] = f < count ? qg[f] : 0.0;
            dst[n] = f < count ? dg[f] : 0.0;
        }
    }
    __syncthreads();
    if (lane < ncfg) {
        double *mine = lds + lane * stride;
        auto slot = [&](int i) -> double & { return slots[i * kWave + lane]; };
        if constexpr (NG > 0) {
            double *kept = slots + kTcSD * tp.nslots * kWave;          // the states sweep 4 cannot run back to: 18 doubles each, [double][lane]
            tree_coriolis_vjp_lane<NG>(groups, n, tp.nslots, [&](int j) { return mine[j]; }, [&](int j) { return mine[NG + j]; }, [](int) {},
                                       [&](int i, int j) { return mine[2 * NG + i * NG + j]; }, [&](int j, double v) { mine[j] = v; },
                                       [&](int j, double v) { mine[NG + j] = v; }, slot, [&](int e) -> double & { return kept[e * kWave + lane]; });
        } else {
            // row i of this lane's gC, staged at the head of pass i into the lane's own LDS row (written and read by this lane alone: no barrier)
            const double *rowg = mg + (int64_t)lane * nn;
            double kept[18 * kTreeCoriolisVjpMaxGroups];              // private memory, as the rest of this form's per-group state
            tree_coriolis_vjp_lane<0>(groups, n, tp.nslots, [&](int j) { return mine[j]; }, [&](int j) { return mine[n + j]; },
                                      [&](int i) { for (int c = 0; c < n; ++c) mine[2 * n + c] = rowg[i * n + c]; },
                                      [&](int, int j) { return mine[2 * n + j]; }, [&](int j, double v) { mine[j] = v; },
                                      [&](int j, double v) { mine[n + j] = v; }, slot, [&](int e) -> double & { return kept[e]; });
        }
    }
    __syncthreads();
    double *const gout[2] = {gq ? gq + cfg0 * n : nullptr, gqd ? gqd + cfg0 * n : nullptr};
    vjp_tile_flush<NG, true>(gout, t, n, stride, lane, lds);
}

// compile-time group count: one tile per single-wave workgroup, one wave per SIMD
template <int NG>
__global__ __launch_bounds__(kWave, 1) void k_tree_coriolis_vjp(TreeCoriolisVjpParams tp, const DevGroup *groups_g, const double *__restrict__ q,
                                                                 const double *__restrict__ qd, const double *__restrict__ gC,
                                                                 double *__restrict__ gq, double *__restrict__ gqd)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    tree_coriolis_vjp_tile<NG>(tp, (ConstGroups)groups_g, NG, blockIdx.x, q, qd, gC, gq, gqd, lds, threadIdx.x);
}

// run-time group count (more groups than the register forms serve, up to 20): grid-stride over tiles, the tape in private memory
__global__ __launch_bounds__(kWave) void k_tree_coriolis_vjp_rt(TreeCoriolisVjpParams tp, const DevGroup *groups_g, const double *__restrict__ q,
                                                                const double *__restrict__ qd, const double *__restrict__ gC,
                                                                double *__restrict__ gq, double *__restrict__ gqd)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t tiles = (tp.N + kWave - 1) / kWave;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        tree_coriolis_vjp_tile<0>(tp, (ConstGroups)groups_g, tp.n, tile, q, qd, gC, gq, gqd, lds, threadIdx.x);
        __syncthreads();
    }
}

#if RTB_HOST_SIDE
// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
int launch_tree_coriolis_vjp(const Tree *t, const DevGroup *groups, const double *q, const double *qd, int64_t N, const double *gC, double *gq,
                             double *gqd, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (t->n < 1 || t->n > kTreeCoriolisVjpMaxGroups) { set_error("tree_coriolis_vjp: robots of 1..20 joints"); return RTBHIP_ELIMIT; }
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("tree_coriolis_vjp: batch too large for one launch"); return RTBHIP_ELIMIT; }
    TreeCoriolisVjpParams tp;
    tp.n = t->n; tp.nslots = t->nslots; tp.N = N;
    // the groups whose state sweep 4 reads back instead of running the next joint backwards (tree_coriolis_vjp_lane: kept)
    int nkept = 0;
    for (int j = 0; j < t->n; ++j)
        nkept += j + 1 >= t->n || !(t->groups[j + 1].parent == j && t->groups[j + 1].parent_slot < 0);
    auto lds_of = [&](bool rt_form) {
        return (size_t)kWave * (tree_coriolis_vjp_stride(t->n, rt_form) + kTcSD * t->nslots + (rt_form ? 0 : 18 * nkept)) * sizeof(double);
    };
    const bool rt = t->n > kTreeCoriolisVjpRegMax || lds_of(false) > 160 * 1024;      // (a small tree with many branches: the register form's tile does not fit)
    const size_t lds = lds_of(rt);
    if (lds > 160 * 1024) { set_error("tree_coriolis_vjp: tree needs more LDS than a CU has"); return RTBHIP_ELIMIT; }
    dim3 grid((unsigned)(rt && tiles > 65536 ? 65536 : tiles));      // the run-time-n kernel strides over the tiles
    switch (rt ? 0 : t->n) {
    case 1: vjp_go(k_tree_coriolis_vjp<1>, grid, lds, s, tp, groups, q, qd, gC, gq, gqd); break;
    case 2: vjp_go(k_tree_coriolis_vjp<2>, grid, lds, s, tp, groups, q, qd, gC, gq, gqd); break;
    case 3: vjp_go(k_tree_coriolis_vjp<3>, grid, lds, s, tp, groups, q, qd, gC, gq, gqd); break;
    case 4: vjp_go(k_tree_coriolis_vjp<4>, grid, lds, s, tp, groups, q, qd, gC, gq, gqd); break;
    case 5: vjp_go(k_tree_coriolis_vjp<5>, grid, lds, s, tp, groups, q, qd, gC, gq, gqd); break;
    case 6: vjp_go(k_tree_coriolis_vjp<6>, grid, lds, s, tp, groups, q, qd, gC, gq, gqd); break;
    case 7: vjp_go(k_tree_coriolis_vjp<7>, grid, lds, s, tp, groups, q, qd, gC, gq, gqd); break;
    case 8: vjp_go(k_tree_coriolis_vjp<8>, grid, lds, s, tp, groups, q, qd, gC, gq, gqd); break;
    default: vjp_go(k_tree_coriolis_vjp_rt, grid, lds, s, tp, groups, q, qd, gC, gq, gqd); break;
    }
    note_launch((int)grid.x, kWave, (int)lds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_tree_coriolis_vjp launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

#endif  // RTB_TREE_CORIOLIS_VJP_LANE_ONLY

#pragma clang fp contract(fast)
}  // namespace rtbhip
