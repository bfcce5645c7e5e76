// tree_rne_vjp_kernels.hip -- gfx950 kernels for the VECTOR-JACOBIAN PRODUCT of the batched inverse dynamics of ETS / URDF robots (rtbhip_tree_rne_vjp):
//
//     gq[i,k] = sum_j gtau[i,j] d tau_j / d q_k        (likewise gqd, gqdd)
//
// the exact reverse-mode adjoint of the spatial-vector recursion tree_rne_core<NG, true, TreeNothing> evaluates (tree_device.h; Robot.rne,
// robot/Robot.py:1704-1903): the same group table (parents, flips, prismatic groups, the full symmetric inertia), the same quirk that `flip`
// negates the joint variable in the transform but not the motion subspace; gravity is a constant of the differentiation.  No reference
// counterpart: the reference has no derivative of its dynamics.
//
// With 6-vectors as pairs [linear; angular], X_j the motion transform of group j's frame  C_j Z_j(sigma_j q_j)  (sigma_j = -1 for a flipped
// joint), s_j its motion subspace ((0; z) revolute, (z; 0) prismatic) and p the parent group:
//     v_j = X_j v_p + s_j qd_j        a_j = X_j a_p + s_j qdd_j + crm(v_j) s_j qd_j        (a of the base: -gravity)
//     f_j = I_j a_j + crf(v_j) I_j v_j + sum over children X_c^T f_c                      tau_j = s_j . f_j
// The joint variable enters through X_j alone, and for a revolute and a prismatic joint alike
//     d (X_j u) / d q_j = -sigma_j crm(s_j) (X_j u)
// so no derivative of a rotation matrix is formed: every term of gq_j is  -sigma_j (crm(s_j) y) . ybar  for a transformed vector y the sweep has
// in hand and its adjoint ybar.
//
// One lane = one sample; four sweeps over the groups:
//   1. primal, base -> tip:   v_j, a_j (kept: the tape) and the group's own force
//   2. primal, tip -> base:   the total force f_j, written over the own force (kept)
//   3. adjoint of sweep 2, base -> tip:   fbar_j = X_j fbar_p + s_j gtau_j  (the force adjoint travels like a motion vector);
//      emits  -(crm(s_j) (X_j fbar_p)) . f_j  into theta_j's adjoint and leaves fbar_j in the slot of f_j (dead by then)
//   4. adjoint of sweep 1, tip -> base:   abar_j = I_j fbar_j + (children),  vbar_j = I_j crm(fbar_j) v_j - crf(fbar_j) I_j v_j
//      + qd_j crf(s_j) abar_j + (children);  gqdd_j = s_j . abar_j,  gqd_j = s_j . vbar_j + abar_j . crm(v_j) s_j,  the rest of gq_j from
//      X_j v_p = v_j - s_j qd_j  and  X_j a_p = a_j - s_j qdd_j - crm(v_j) s_j qd_j;  (vbar_j, abar_j) go to the parent through X_j^T
// Tape: 18 doubles per group (v, a, f) plus sin, cos and the partial angle adjoint -- 21 doubles, 336 VGPRs for eight groups: one wave per
// SIMD (__launch_bounds__(64, 1), the 512-entry register file).  A group whose parent is not the group before it reads fbar_p from the parent's
// per-lane LDS slot (tree_device.h: the slot the forward sweeps used for the parent's (v, a) and force accumulator; dead by sweep 3) and adds
// X^T (vbar, abar) into it: 6 + 12 = the slot's 18 doubles.  A serial chain uses no slot.
// I/O as k_rne_vjp: the wave's (64 x n) blocks of q, qd, qdd and gtau are contiguous in memory, loaded coalesced into a lane-major LDS tile
// (odd row stride); gq, gqd, gqdd overwrite the q, qd, qdd slots and leave the same way.
#include "tree_kernels.h"
#include "vjp_tile.h"

namespace rtbhip {

#pragma clang fp contract(off)      // every operation written out, as in tree_device.h

constexpr int kTreeVjpMaxGroups = 24;      // the forward kernel's built-in sizes

RTB_HD V3 tv_zero() { return v3(0, 0, 0); }
// I [l; a] = [M l + a x h; I_bar a + h x l]  (symmetric: it is its own transpose)
template <class G> RTB_HD void tv_inertia(const G &g, V3 l, V3 a, V3 &ol, V3 &oa)
{
    const V3 h = v3(g.h[0], g.h[1], g.h[2]);
    ol = cross_add(a, h, g.M * l);
    oa = cross_add(h, l, inertia_rot(g, a));
}

// One sample.  groups: the wave-uniform group table.  qin / qdin / qddin(q column), gin(tau column): per-lane readers; gq / gqd / gqdd(q column,
// value): writers.  q_j, qd_j, qdd_j must stay readable until gq_j, gqd_j, gqdd_j have been written (the kernel lets the gradients overwrite
// their slots); gtau is never written over.  slot(index) -> double& into this lane's kTreeSlotDoubles * nslots scratch.
// NG = 0: run-time group count n_rt (<= kTreeVjpMaxGroups), the per-group arrays in private memory.
template <int NG, class GroupsP, class InQ, class InQd, class InQdd, class InG, class OutQ, class OutQd, class OutQdd, class Slot>
RTB_HD void tree_rne_vjp_lane(GroupsP groups, int n_rt, int nslots, V3 gravity, InQ qin, InQd qdin, InQdd qddin, InG gin, OutQ gq, OutQd gqd,
                              OutQdd gqdd, Slot slot)
{
#pragma clang fp contract(off)
    constexpr int CAP = NG > 0 ? NG : kTreeVjpMaxGroups;
    const int n = NG > 0 ? NG : n_rt;
    double sn[CAP], cs[CAP], th[CAP];
    V3 VL[CAP], VA[CAP], AL[CAP], AA[CAP], FL[CAP], FA[CAP];
    if constexpr (NG > 0) {
        tree_trig<NG>(groups, qin, sn, cs);
    } else {
        for (int j = 0; j < n; ++j) {
            const auto &g = groups[j];
            const double t = jm_prismatic(g.jmeta) ? 0.0 : qin(jm_jq(g.jmeta)) * (jm_flip(g.jmeta) ? -1.0 : 1.0);
            double s, c;
            sincos(t, &s, &c);
            sn[j] = s; cs[j] = c;
        }
    }
    for (int k = 0; k < nslots; ++k)
        for (int e = 12; e < 18; ++e) slot(k * kTreeSlotDoubles + e) = 0.0;
    auto slide = [&](const auto &g) { return jm_prismatic(g.jmeta) ? qin(jm_jq(g.jmeta)) * (jm_flip(g.jmeta) ? -1.0 : 1.0) : 0.0; };

    // ---- 1. primal forward recursion (tree_rne_core's, the state of every group kept)
    {
        V3 vl = tv_zero(), va = tv_zero(), al = tv_zero(), aa = tv_zero();
#pragma unroll
        for (int j = 0; j < n; ++j) {
            const auto &g = groups[j];
            const bool pris = jm_prismatic(g.jmeta) != 0;
            const int col = jm_jq(g.jmeta);
            const double qdj = qdin(col), qddj = qddin(col);
            V3 pvl, pva, pal, paa;
            if (g.parent < 0) {
                pvl = tv_zero(); pva = tv_zero();
                pal = v3(-gravity.x, -gravity.y, -gravity.z); paa = tv_zero();
            } else if (g.parent_slot >= 0) {
                const int b = g.parent_slot * kTreeSlotDoubles;
                pvl = vjp_slot_get(slot, b); pva = vjp_slot_get(slot, b + 3); pal = vjp_slot_get(slot, b + 6); paa = vjp_slot_get(slot, b + 9);
            } else {
                pvl = vl; pva = va; pal = al; paa = aa;
            }
            const V3 p = tree_origin(false, g, slide(g));
            const double s = sn[j], c = cs[j];
            va = rz_t(s, c, seg_rt(g, pva));
            vl = rz_t(s, c, seg_rt(g, add_cross_ap(7, pvl, pva, p)));
            aa = rz_t(s, c, seg_rt(g, paa));
            al = rz_t(s, c, seg_rt(g, add_cross_ap(7, pal, paa, p)));
            if (pris) {
                vl.z += qdj;
                al = crossz_add(va, qdj, al);
                al.z += qddj;
            } else {
                va.z += qdj;
                al = crossz_add(vl, qdj, al);
                aa = crossz_add(va, qdj, aa);
                aa.z += qddj;
            }
            if (g.save_slot >= 0) {
                const int b = g.save_slot * kTreeSlotDoubles;
                vjp_slot_put(slot, b, vl); vjp_slot_put(slot, b + 3, va); vjp_slot_put(slot, b + 6, al); vjp_slot_put(slot, b + 9, aa);
            }
            VL[j] = vl; VA[j] = va; AL[j] = al; AA[j] = aa;
            V3 Ial, Iaa, Ivl, Iva;
            tv_inertia(g, al, aa, Ial, Iaa);
            tv_inertia(g, vl, va, Ivl, Iva);
            FL[j] = cross_add(va, Ivl, Ial);
            FA[j] = cross_add(vl, Ivl, cross_add(va, Iva, Iaa));
            if (NG > 0) sched_fence();
        }
    }

    // ---- 2. primal backward recursion: own force -> total force f_j, in place
    {
        V3 cl = tv_zero(), ca = tv_zero();
#pragma unroll
        for (int jj = 0; jj < n; ++jj) {
            const int j = n - 1 - jj;
            const auto &g = groups[j];
            V3 fl = FL[j] + cl, fa = FA[j] + ca;
            if (g.save_slot >= 0) {
                const int b = g.save_slot * kTreeSlotDoubles + 12;
                fl = fl + vjp_slot_get(slot, b);
                fa = fa + vjp_slot_get(slot, b + 3);
            }
            FL[j] = fl; FA[j] = fa;
            cl = tv_zero(); ca = tv_zero();
            if (g.parent >= 0) {
                const V3 p = tree_origin(false, g, slide(g));
                const V3 tl = seg_r(g, rz(sn[j], cs[j], fl));
                const V3 ta = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], fa)), p, tl);
                if (g.parent_slot >= 0) {
                    const int b = g.parent_slot * kTreeSlotDoubles + 12;
                    vjp_slot_add(slot, b, tl); vjp_slot_add(slot, b + 3, ta);
                } else {
                    cl = tl; ca = ta;
                }
            }
            if (NG > 0) sched_fence();
        }
    }

    // ---- 3. adjoint of the backward recursion, base -> tip: f_j -> fbar_j in place
    {
        V3 bl = tv_zero(), ba = tv_zero();      // fbar of the previous group
#pragma unroll
        for (int j = 0; j < n; ++j) {
            const auto &g = groups[j];
            const bool pris = jm_prismatic(g.jmeta) != 0;
            V3 xl = tv_zero(), xa = tv_zero();       // X_j fbar_p
            double t = 0.0;
            if (g.parent >= 0) {
                V3 pbl = bl, pba = ba;
                if (g.parent_slot >= 0) {
                    const int b = g.parent_slot * kTreeSlotDoubles;
                    pbl = vjp_slot_get(slot, b); pba = vjp_slot_get(slot, b + 3);
                }
                const V3 p = tree_origin(false, g, slide(g));
                xa = rz_t(sn[j], cs[j], seg_rt(g, pba));
                xl = rz_t(sn[j], cs[j], seg_rt(g, add_cross_ap(7, pbl, pba, p)));
                t = pris ? -vjp_zcross(xa, FL[j]) : -(vjp_zcross(xl, FL[j]) + vjp_zcross(xa, FA[j]));
            }
            th[j] = t;
            const double gt = gin(g.out_col);
            if (pris) xl.z += gt; else xa.z += gt;
            FL[j] = xl; FA[j] = xa;
            if (g.save_slot >= 0) {
                const int b = g.save_slot * kTreeSlotDoubles;
                vjp_slot_put(slot, b, xl); vjp_slot_put(slot, b + 3, xa);
                for (int e = 6; e < 18; ++e) slot(b + e) = 0.0;      // the accumulators of (vbar, abar) for sweep 4
            }
            bl = xl; ba = xa;
            if (NG > 0) sched_fence();
        }
    }

    // ---- 4. adjoint of the forward recursion, tip -> base
    {
        V3 cvl = tv_zero(), cva = tv_zero(), cal = tv_zero(), caa = tv_zero();      // X^T (vbar, abar) handed down by group j + 1 when its parent is group j
#pragma unroll
        for (int jj = 0; jj < n; ++jj) {
            const int j = n - 1 - jj;
            const auto &g = groups[j];
            const bool pris = jm_prismatic(g.jmeta) != 0;
            const int col = jm_jq(g.jmeta);
            const double sigma = jm_flip(g.jmeta) ? -1.0 : 1.0;
            const double qdj = qdin(col);
            const V3 fbl = FL[j], fba = FA[j], vl = VL[j], va = VA[j], al = AL[j], aa = AA[j];
            V3 vbl = cvl, vba = cva, abl = cal, aba = caa;
            if (g.save_slot >= 0) {
                const int b = g.save_slot * kTreeSlotDoubles + 6;
                vbl = vbl + vjp_slot_get(slot, b); vba = vba + vjp_slot_get(slot, b + 3);
                abl = abl + vjp_slot_get(slot, b + 6); aba = aba + vjp_slot_get(slot, b + 9);
            }
            // the group's own force  I a + crf(v) I v:  abar += I fbar;  vbar += I (crm(fbar) v) - crf(fbar) (I v)
            V3 tl, ta, Ivl, Iva;
            tv_inertia(g, fbl, fba, tl, ta);
            abl = abl + tl; aba = aba + ta;
            tv_inertia(g, vl, va, Ivl, Iva);
            const V3 wl = cross_add(fbl, va, cross(fba, vl)), wa = cross(fba, va);
            tv_inertia(g, wl, wa, tl, ta);
            vbl = cross_add(Ivl, fba, vbl + tl);
            vba = cross_add(Ivl, fbl, cross_add(Iva, fba, vba + ta));
            // the joint:  a = X a_p + s qdd + crm(v) s qd,  v = X v_p + s qd
            double t, oqd, oqdd;
            if (pris) {
                oqdd = abl.z;
                vba = v3(__builtin_fma(-qdj, abl.y, vba.x), __builtin_fma(qdj, abl.x, vba.y), vba.z);      // vbar += qd crf(s) abar = qd [0; z x abar_l]
                oqd = vbl.z + vjp_zcross(abl, va);
                t = -(vjp_zcross(va, vbl) + vjp_zcross(aa, abl));
            } else {
                oqdd = aba.z;
                vbl = v3(__builtin_fma(-qdj, abl.y, vbl.x), __builtin_fma(qdj, abl.x, vbl.y), vbl.z);      // qd [z x abar_l; z x abar_a]
                vba = v3(__builtin_fma(-qdj, aba.y, vba.x), __builtin_fma(qdj, aba.x, vba.y), vba.z);
                oqd = vba.z + (vjp_zcross(abl, vl) + vjp_zcross(aba, va));
                const V3 xal = v3(__builtin_fma(-qdj, vl.y, al.x), __builtin_fma(qdj, vl.x, al.y), al.z);     // X a_p up to its z parts
                const V3 xaa = v3(__builtin_fma(-qdj, va.y, aa.x), __builtin_fma(qdj, va.x, aa.y), aa.z);
                t = -((vjp_zcross(vl, vbl) + vjp_zcross(va, vba)) + (vjp_zcross(xal, abl) + vjp_zcross(xaa, aba)));
            }
            const double d = slide(g);
            gq(col, sigma * (th[j] + t));
            gqd(col, oqd);
            gqdd(col, oqdd);
            cvl = tv_zero(); cva = tv_zero(); cal = tv_zero(); caa = tv_zero();
            if (g.parent >= 0) {
                const V3 p = tree_origin(false, g, d);
                const V3 ul = seg_r(g, rz(sn[j], cs[j], vbl));
                const V3 ua = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], vba)), p, ul);
                const V3 wl2 = seg_r(g, rz(sn[j], cs[j], abl));
                const V3 wa2 = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], aba)), p, wl2);
                if (g.parent_slot >= 0) {
                    const int b = g.parent_slot * kTreeSlotDoubles + 6;
                    vjp_slot_add(slot, b, ul); vjp_slot_add(slot, b + 3, ua); vjp_slot_add(slot, b + 6, wl2); vjp_slot_add(slot, b + 9, wa2);
                } else {
                    cvl = ul; cva = ua; cal = wl2; caa = wa2;
                }
            }
            if (NG > 0) sched_fence();
        }
    }
}

#ifndef RTB_TREE_RNE_VJP_LANE_ONLY      // (a host-side replay of the lane body includes this file for tree_rne_vjp_lane alone)

struct TreeVjpParams {
    int32_t n, nslots;
    int64_t N;
    double grav[3];
};

// LDS row of one sample: q | qd | qdd | gtau, 4 n doubles at an odd stride; then the branch slots, [slot double][lane]
inline __host__ __device__ int tree_vjp_stride(int n) { return (4 * n) | 1; }

// One tile of 64 samples.  qd / qdd NULL: zeros, not read.  gq / gqd / gqdd NULL: not stored (the lane body forms all three gradients either way:
// they share the four sweeps).  The staging and the flush are vjp_tile.h's phases.
template <int NG>
__device__ __forceinline__ void tree_rne_vjp_tile(const TreeVjpParams &tp, ConstGroups groups, int n, int64_t tile, const double *__restrict__ q,
                                                  const double *__restrict__ qd, const double *__restrict__ qdd, const double *__restrict__ gtau,
                                                  double *__restrict__ gq, double *__restrict__ gqd, double *__restrict__ gqdd, double *lds, int lane)
{
    const int stride = tree_vjp_stride(n);
    double *slots = lds + kWave * stride;
    const VjpTile t = vjp_tile_of(tile, tp.N, n);
    const int64_t at = t.cfg0 * n;
    const double *const gin[4] = {q + at, qd ? qd + at : nullptr, qdd ? qdd + at : nullptr, gtau + at};
    VjpCols<NG, 4, double> cols;
    vjp_load_cols<NG, true>(gin, t, lane, cols);
    sched_fence();
    vjp_stage_cols<NG, true>(gin, t, n, stride, lane, cols, lds);
    __syncthreads();
    if (lane < t.ncfg) {
        double *mine = lds + lane * stride;
        tree_rne_vjp_lane<NG>(groups, n, tp.nslots, v3(tp.grav[0], tp.grav[1], tp.grav[2]), [&](int c) { return mine[c]; },
                              [&](int c) { return mine[n + c]; }, [&](int c) { return mine[2 * n + c]; }, [&](int c) { return mine[3 * n + c]; },
                              [&](int c, double v) { mine[c] = v; }, [&](int c, double v) { mine[n + c] = v; },
                              [&](int c, double v) { mine[2 * n + c] = v; }, [&](int i) -> double & { return slots[i * kWave + lane]; });
    }
    __syncthreads();
    double *const gout[3] = {gq ? gq + at : nullptr, gqd ? gqd + at : nullptr, gqdd ? gqdd + at : nullptr};
    vjp_tile_flush<NG, true>(gout, t, n, stride, lane, lds);
}

// compile-time group count (1..8): one tile per single-wave workgroup, one wave per SIMD
template <int NG>
__global__ __launch_bounds__(kWave, 1) void k_tree_rne_vjp(TreeVjpParams tp, const DevGroup *groups_g, const double *__restrict__ q,
                                                            const double *__restrict__ qd, const double *__restrict__ qdd,
                                                            const double *__restrict__ gtau, double *__restrict__ gq, double *__restrict__ gqd,
                                                            double *__restrict__ gqdd)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    tree_rne_vjp_tile<NG>(tp, (ConstGroups)groups_g, NG, blockIdx.x, q, qd, qdd, gtau, gq, gqd, gqdd, lds, threadIdx.x);
}

// run-time group count (9 .. 24): grid-stride over tiles, the tape in private memory
__global__ __launch_bounds__(kWave) void k_tree_rne_vjp_rt(TreeVjpParams tp, const DevGroup *groups_g, const double *__restrict__ q,
                                                           const double *__restrict__ qd, const double *__restrict__ qdd,
                                                           const double *__restrict__ gtau, double *__restrict__ gq, double *__restrict__ gqd,
                                                           double *__restrict__ gqdd)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t tiles = (tp.N + kWave - 1) / kWave;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        tree_rne_vjp_tile<0>(tp, (ConstGroups)groups_g, tp.n, tile, q, qd, qdd, gtau, gq, gqd, gqdd, lds, threadIdx.x);
        __syncthreads();
    }
}

#if RTB_HOST_SIDE
// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
int launch_tree_rne_vjp(const Tree *t, const DevGroup *groups, const double *q, const double *qd, const double *qdd, int64_t N, const double *grav3,
                        const double *gtau, double *gq, double *gqd, double *gqdd, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (t->n < 1 || t->n > kTreeVjpMaxGroups) { set_error("tree_rne_vjp: more than 24 link groups"); return RTBHIP_ELIMIT; }
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("tree_rne_vjp: batch too large for one launch"); return RTBHIP_ELIMIT; }
    TreeVjpParams tp;
    tp.n = t->n; tp.nslots = t->nslots; tp.N = N;
    for (int i = 0; i < 3; i++) tp.grav[i] = grav3[i];
    const size_t lds = (size_t)kWave * (tree_vjp_stride(t->n) + kTreeSlotDoubles * t->nslots) * sizeof(double);
    if (lds > 160 * 1024) { set_error("tree_rne_vjp: tree needs more LDS than a CU has"); return RTBHIP_ELIMIT; }
    const bool rt = t->n > 8;
    dim3 grid((unsigned)(rt && tiles > 65536 ? 65536 : tiles));      // the run-time-n kernel strides over the tiles
    switch (rt ? 0 : t->n) {
    case 1: vjp_go(k_tree_rne_vjp<1>, grid, lds, s, tp, groups, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 2: vjp_go(k_tree_rne_vjp<2>, grid, lds, s, tp, groups, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 3: vjp_go(k_tree_rne_vjp<3>, grid, lds, s, tp, groups, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 4: vjp_go(k_tree_rne_vjp<4>, grid, lds, s, tp, groups, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 5: vjp_go(k_tree_rne_vjp<5>, grid, lds, s, tp, groups, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 6: vjp_go(k_tree_rne_vjp<6>, grid, lds, s, tp, groups, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 7: vjp_go(k_tree_rne_vjp<7>, grid, lds, s, tp, groups, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 8: vjp_go(k_tree_rne_vjp<8>, grid, lds, s, tp, groups, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    default: vjp_go(k_tree_rne_vjp_rt, grid, lds, s, tp, groups, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    }
    note_launch((int)grid.x, kWave, (int)lds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_tree_rne_vjp launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

#endif  // RTB_TREE_RNE_VJP_LANE_ONLY

#pragma clang fp contract(fast)
}  // namespace rtbhip
