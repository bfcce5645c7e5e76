// tree_inertia_vjp_kernels.hip -- gfx950 kernels for the VECTOR-JACOBIAN PRODUCT of the batched joint-space inertia matrix of an ETS / URDF robot
// (rtbhip_tree_inertia_vjp):
//
//     gq[r,k] = sum_ij gM[r,i,j] d M[r,i,j] / d q[r,k]
//
// for robots numbered in group order (group j moves q column j: every URDF robot, every robot whose jindex was assigned automatically), every joint
// kind the forward call serves.  The forward kernel (tree_device.h: tree_dyn_lane) builds M from n unit-acceleration passes of the spatial-vector
// recursion at rest -- pass i = rne(q, 0, e_i) without gravity -- keeps the torques j >= i of pass i (the groups before i are no descendants of i)
// and mirrors them: the computed value P(j, i), j >= i, is both M[j,i] and M[i,j].  Its adjoint therefore takes gM FOLDED onto the triangle,
//     S(j, i) = gM[j,i] + gM[i,j]  (j > i),    S(i, i) = gM[i,i]
// and is the sum over i of the adjoint of pass i seeded with gtau_j = S(j, i) on the groups j >= i.
//
// The lane body is the SPECIALISED form of tree_rne_vjp_lane (tree_rne_vjp_kernels.hip, whose header has the formulas): with qd = 0 every velocity is
// an exact zero, so v, vbar and everything that multiplies them are left out (exact zeros there, x + 0 == x); the tape is a, f = 12 doubles per
// group plus sin, cos and the partial angle adjoint; pass i starts at group i (the branch slots are zeroed at the head of every pass, which is the
// state of the groups at rest), and M[j,i] (j >= i) depends on q_{i+1} .. q_j only: pass i emits gq_k for k > i, so the last pass is not run at all.
// One lane = one sample; sin / cos once per lane, then a `#pragma unroll 1` loop over the passes, each kept self-contained by tree_opaque
// (dyn_device.h: dyn_opaque tells why); gq accumulates in n registers.
// I/O as k_inertia_vjp: lane-major LDS tile of  q (n) | S (n (n + 1) / 2, packed: (j, i) at j (j + 1) / 2 + i)  doubles per row at an odd stride,
// then the branch slots, [slot double][lane]; gq overwrites the q slots and leaves as contiguous non-temporal stores.
#include "tree_kernels.h"
#include "vjp_tile.h"

namespace rtbhip {

#pragma clang fp contract(off)      // every operation written out, as in tree_device.h

constexpr int kTreeInertiaVjpMaxGroups = 20;      // the forward kernel's built-in sizes (tree_dyn_kernels.hip: kTreeDynMax)

RTB_HD V3 ti_zero() { return v3(0, 0, 0); }
// I [l; a] = [M l + a x h; I_bar a + h x l]  (symmetric: it is its own transpose)
template <class G> RTB_HD void ti_inertia(const G &g, V3 l, V3 a, V3 &ol, V3 &oa)
{
    const V3 h = v3(g.h[0], g.h[1], g.h[2]);
    ol = cross_add(a, h, g.M * l);
    oa = cross_add(h, l, inertia_rot(g, a));
}

// One sample.  groups: the wave-uniform group table, group j on q column j.  qin(j): the joint variables.  sym(j, i), j >= i: the folded gradient
// S(j, i).  gq(j, v): called once per joint, after the last pass.  slot(index) -> double& into this lane's kTreeSlotDoubles * nslots scratch:
// per slot  [0, 6) fbar of the group that saves there,  [6, 12) its acceleration,  [12, 18) the accumulator of its children (forces in sweep 2,
// abar in sweep 4).  NG = 0: run-time group count n_rt (<= kTreeInertiaVjpMaxGroups), the per-group arrays in private memory.
template <int NG, class GroupsP, class InQ, class InS, class OutQ, class Slot>
RTB_HD void tree_inertia_vjp_lane(GroupsP groups, int n_rt, int nslots, InQ qin, InS sym, OutQ gq, Slot slot)
{
#pragma clang fp contract(off)
    constexpr int CAP = NG > 0 ? NG : kTreeInertiaVjpMaxGroups;
    const int n = NG > 0 ? NG : n_rt;
    double sn[CAP], cs[CAP], th[CAP], acc[CAP];
    V3 AL[CAP], AA[CAP], FL[CAP], FA[CAP];
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
    for (int j = 0; j < n; ++j) acc[j] = 0.0;
    auto slide = [&](const auto &g, int j) { return jm_prismatic(g.jmeta) ? qin(j) * (jm_flip(g.jmeta) ? -1.0 : 1.0) : 0.0; };

#pragma unroll 1
    for (int i = 0; i + 1 < n; ++i) {
        if constexpr (NG > 0) tree_opaque<NG>(sn, cs);
        for (int k = 0; k < nslots; ++k)
            for (int e = 0; e < kTreeSlotDoubles; ++e) slot(k * kTreeSlotDoubles + e) = 0.0;

        // ---- 1. primal forward recursion from group i: a_j (the tape) and the group's own force I a
        {
            V3 al = ti_zero(), aa = ti_zero();
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (j < i) continue;
                const auto &g = groups[j];
                const bool pris = jm_prismatic(g.jmeta) != 0;
                const double qddj = j == i ? 1.0 : 0.0;
                V3 pal, paa;
                if (g.parent < 0) {
                    pal = ti_zero(); paa = ti_zero();
                } else if (g.parent_slot >= 0) {
                    const int b = g.parent_slot * kTreeSlotDoubles;
                    pal = vjp_slot_get(slot, b + 6); paa = vjp_slot_get(slot, b + 9);
                } else {
                    pal = al; paa = aa;
                }
                const V3 p = tree_origin(false, g, slide(g, j));
                const double s = sn[j], c = cs[j];
                aa = rz_t(s, c, seg_rt(g, paa));
                al = rz_t(s, c, seg_rt(g, add_cross_ap(7, pal, paa, p)));
                if (pris) al.z += qddj;
                else aa.z += qddj;
                if (g.save_slot >= 0) {
                    const int b = g.save_slot * kTreeSlotDoubles;
                    vjp_slot_put(slot, b + 6, al); vjp_slot_put(slot, b + 9, aa);
                }
                AL[j] = al; AA[j] = aa;
                V3 Ial, Iaa;
                ti_inertia(g, al, aa, Ial, Iaa);
                FL[j] = Ial; FA[j] = Iaa;
                if (NG > 0) sched_fence();
            }
        }

        // ---- 2. primal backward recursion: own force -> total force f_j, in place, for the groups j > i (sweep 3 reads no force of group i)
        {
            V3 cl = ti_zero(), ca = ti_zero();
#pragma unroll
            for (int jj = 0; jj < n; ++jj) {
                const int j = n - 1 - jj;
                if (j <= i) continue;
                const auto &g = groups[j];
                V3 fl = FL[j] + cl, fa = FA[j] + ca;
                if (g.save_slot >= 0) {
                    const int b = g.save_slot * kTreeSlotDoubles + 12;
                    fl = fl + vjp_slot_get(slot, b);
                    fa = fa + vjp_slot_get(slot, b + 3);
                }
                FL[j] = fl; FA[j] = fa;
                cl = ti_zero(); ca = ti_zero();
                if (g.parent >= 0) {
                    const V3 p = tree_origin(false, g, slide(g, j));
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

        // ---- 3. adjoint of the backward recursion, group i -> tip: f_j -> fbar_j in place
        {
            V3 bl = ti_zero(), ba = ti_zero();      // fbar of the previous group
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (j < i) continue;
                const auto &g = groups[j];
                const bool pris = jm_prismatic(g.jmeta) != 0;
                V3 xl = ti_zero(), xa = ti_zero();       // X_j fbar_p
                double t = 0.0;
                if (j > i && g.parent >= 0) {            // (the parent of group i is at rest and has no gradient: fbar_p = 0)
                    V3 pbl = bl, pba = ba;
                    if (g.parent_slot >= 0) {
                        const int b = g.parent_slot * kTreeSlotDoubles;
                        pbl = vjp_slot_get(slot, b); pba = vjp_slot_get(slot, b + 3);
                    }
                    const V3 p = tree_origin(false, g, slide(g, j));
                    xa = rz_t(sn[j], cs[j], seg_rt(g, pba));
                    xl = rz_t(sn[j], cs[j], seg_rt(g, add_cross_ap(7, pbl, pba, p)));
                    t = pris ? -vjp_zcross(xa, FL[j]) : -(vjp_zcross(xl, FL[j]) + vjp_zcross(xa, FA[j]));
                }
                th[j] = t;
                const double gt = sym(j, i);
                if (pris) xl.z += gt; else xa.z += gt;
                FL[j] = xl; FA[j] = xa;
                if (g.save_slot >= 0) {
                    const int b = g.save_slot * kTreeSlotDoubles;
                    vjp_slot_put(slot, b, xl); vjp_slot_put(slot, b + 3, xa);
                    for (int e = 12; e < 18; ++e) slot(b + e) = 0.0;      // the accumulator of abar for sweep 4
                }
                bl = xl; ba = xa;
                if (NG > 0) sched_fence();
            }
        }

        // ---- 4. adjoint of the forward recursion, tip -> group i + 1 (M[j,i] does not depend on q_i)
        {
            V3 cal = ti_zero(), caa = ti_zero();      // X^T abar handed down by group j + 1 when its parent is group j
#pragma unroll
            for (int jj = 0; jj < n; ++jj) {
                const int j = n - 1 - jj;
                if (j <= i) continue;
                const auto &g = groups[j];
                const bool pris = jm_prismatic(g.jmeta) != 0;
                const double sigma = jm_flip(g.jmeta) ? -1.0 : 1.0;
                const V3 fbl = FL[j], fba = FA[j], al = AL[j], aa = AA[j];
                V3 abl = cal, aba = caa;
                if (g.save_slot >= 0) {
                    const int b = g.save_slot * kTreeSlotDoubles + 12;
                    abl = abl + vjp_slot_get(slot, b); aba = aba + vjp_slot_get(slot, b + 3);
                }
                // the group's own force  I a:  abar += I fbar
                V3 tl, ta;
                ti_inertia(g, fbl, fba, tl, ta);
                abl = abl + tl; aba = aba + ta;
                // the joint:  a = X a_p + s qdd  (qdd_j = 0 for j > i: X a_p = a)
                const double t = pris ? -vjp_zcross(aa, abl) : -(vjp_zcross(al, abl) + vjp_zcross(aa, aba));
                acc[j] = acc[j] + sigma * (th[j] + t);
                cal = ti_zero(); caa = ti_zero();
                if (g.parent >= 0) {
                    const V3 p = tree_origin(false, g, slide(g, j));
                    const V3 wl2 = seg_r(g, rz(sn[j], cs[j], abl));
                    const V3 wa2 = add_cross_pa(7, seg_r(g, rz(sn[j], cs[j], aba)), p, wl2);
                    if (g.parent_slot >= 0) {
                        const int b = g.parent_slot * kTreeSlotDoubles + 12;
                        vjp_slot_add(slot, b, wl2); vjp_slot_add(slot, b + 3, wa2);
                    } else {
                        cal = wl2; caa = wa2;
                    }
                }
                if (NG > 0) sched_fence();
            }
        }
    }
#pragma unroll
    for (int j = 0; j < n; ++j) gq(j, acc[j]);
}

#ifndef RTB_TREE_INERTIA_VJP_LANE_ONLY      // (a host-side replay of the lane body includes this file for tree_inertia_vjp_lane alone)

struct TreeInertiaVjpParams {
    int32_t n, nslots;
    int64_t N;
};

// LDS row of one sample: q (n) | S (n (n + 1) / 2); then the branch slots, [slot double][lane].  An odd stride (conflict-free rows) while the tile
// with its slots stays within a CU's 160 KiB: at 20 groups the row is 230 doubles, and with five branch slots (90) only the even stride fits --
// 320 doubles per lane, exactly 160 KiB (as rne_vjp_stride gives up its odd stride at 32 joints)
__host__ __device__ constexpr int tree_inertia_vjp_stride(int n, int nslots)
{
    const int row = n + n * (n + 1) / 2, odd = row | 1;
    return (size_t)kWave * (odd + kTreeSlotDoubles * nslots) * sizeof(double) <= 160 * 1024 ? odd : row;
}
// The register forms take their stride with nslots = 0 (a compile-time constant), the launcher sizes the tile with the tree's nslots: the two
// agree while the largest register form fits at the odd stride with every slot a tree of that size can have (n - 2: a slot needs a parent with
// a child two or more groups on)
constexpr int kTreeInertiaVjpRegMax = 8;
static_assert(tree_inertia_vjp_stride(kTreeInertiaVjpRegMax, kTreeInertiaVjpRegMax - 2) == tree_inertia_vjp_stride(kTreeInertiaVjpRegMax, 0),
              "a register form of k_tree_inertia_vjp would need the even stride: pass tp.nslots to tree_inertia_vjp_stride there too");

// One tile of 64 samples.  This unit keeps its own staging, fold (as vjp_tile.h's vjp_fold) and flush: with the phases in their place UR5's adjoint
// measured 1.5 % slower in one build and 7 % faster in another, and with the flush phase alone the 13-group run-time-n form 0.3 % slower
// (profiles/vjp_tile_refactor_ab.json).
template <int NG>
__device__ __forceinline__ void tree_inertia_vjp_tile(const TreeInertiaVjpParams &tp, ConstGroups groups, int n, int64_t tile, const double *__restrict__ q,
                                                      const double *__restrict__ gM, double *__restrict__ gq, double *lds, int lane)
{
    // (a register form always fits at the odd stride -- the static_assert above -- and keeps it a compile-time constant)
    const int stride = tree_inertia_vjp_stride(n, NG > 0 ? 0 : tp.nslots);
    double *slots = lds + kWave * stride;
    const int64_t cfg0 = tile * kWave;
    const int64_t left = tp.N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    const int nn = n * n;
    const int count = ncfg * n, mcount = ncfg * nn;
    const double *qg = q + cfg0 * n, *mg = gM + cfg0 * nn;
    // where element f of the wave's gM block goes: row f / n^2 of the tile, entry (r, c) -> the packed slot of (max, min)
    auto slot_of = [&](int f, bool &lower) {
        const int row = f / nn, rem = f - row * nn, r = rem / n, c = rem - r * n;
        lower = r >= c;
        const int hi = lower ? r : c, lo = lower ? c : r;
        return row * stride + n + hi * (hi + 1) / 2 + lo;
    };
    if constexpr (NG > 0) {
        // all NG + NG^2 coalesced loads in flight before the first LDS write (vjp_tile.h tells why): unconditional -- an element past the ragged tail
        // reads element 0 of the tile -- and the zeros are selected afterwards
        double rq[NG], rm[NG * NG];
#pragma unroll
        for (int k = 0; k < NG; ++k) { const int f = lane + kWave * k; rq[k] = qg[f < count ? f : 0]; }
#pragma unroll
        for (int k = 0; k < NG * NG; ++k) { const int f = lane + kWave * k; rm[k] = mg[f < mcount ? f : 0]; }
        sched_fence();
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int f = lane + kWave * k;
            lds[(f / NG) * stride + (f % NG)] = f < count ? rq[k] : 0.0;
        }
        // the fold: the lower triangle and the diagonal are written, then the upper triangle is added -- each packed slot has exactly one element
        // of either kind, so no two lanes touch a slot within a phase
#pragma unroll
        for (int k = 0; k < NG * NG; ++k) {
            const int f = lane + kWave * k;
            bool lower;
            const int at = slot_of(f, lower);
            if (lower) lds[at] = f < mcount ? rm[k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NG * NG; ++k) {
            const int f = lane + kWave * k;
            bool lower;
            const int at = slot_of(f, lower);
            if (!lower) lds[at] = lds[at] + (f < mcount ? rm[k] : 0.0);
        }
    } else {
        for (int f = lane; f < kWave * n; f += kWave) lds[(f / n) * stride + (f % n)] = f < count ? qg[f] : 0.0;
        for (int f = lane; f < kWave * nn; f += kWave) {
            bool lower;
            const int at = slot_of(f, lower);
            if (lower) lds[at] = f < mcount ? mg[f] : 0.0;
        }
        __syncthreads();
        for (int f = lane; f < kWave * nn; f += kWave) {
            bool lower;
            const int at = slot_of(f, lower);
            if (!lower) lds[at] = lds[at] + (f < mcount ? mg[f] : 0.0);
        }
    }
    __syncthreads();
    if (lane < ncfg) {
        double *mine = lds + lane * stride;
        tree_inertia_vjp_lane<NG>(groups, n, tp.nslots, [&](int j) { return mine[j]; }, [&](int j, int i) { return mine[n + j * (j + 1) / 2 + i]; },
                                  [&](int j, double v) { mine[j] = v; }, [&](int i) -> double & { return slots[i * kWave + lane]; });
    }
    __syncthreads();
    double *out = gq + cfg0 * n;
    if constexpr (NG > 0) {
        double r[NG];
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int f = lane + kWave * k;
            r[k] = lds[(f / NG) * stride + (f % NG)];
        }
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int f = lane + kWave * k;
            if (f < count) __builtin_nontemporal_store(r[k], out + f);
        }
    } else {
        for (int f = lane; f < count; f += kWave) out[f] = lds[(f / n) * stride + (f % n)];
    }
}

// compile-time group count (1..8): one tile per single-wave workgroup, one wave per SIMD
template <int NG>
__global__ __launch_bounds__(kWave, 1) void k_tree_inertia_vjp(TreeInertiaVjpParams tp, const DevGroup *groups_g, const double *__restrict__ q,
                                                                const double *__restrict__ gM, double *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    tree_inertia_vjp_tile<NG>(tp, (ConstGroups)groups_g, NG, blockIdx.x, q, gM, gq, lds, threadIdx.x);
}

// run-time group count (9 .. 20): grid-stride over tiles, the tape in private memory
__global__ __launch_bounds__(kWave) void k_tree_inertia_vjp_rt(TreeInertiaVjpParams tp, const DevGroup *groups_g, const double *__restrict__ q,
                                                               const double *__restrict__ gM, double *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int64_t tiles = (tp.N + kWave - 1) / kWave;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        tree_inertia_vjp_tile<0>(tp, (ConstGroups)groups_g, tp.n, tile, q, gM, gq, lds, threadIdx.x);
        __syncthreads();
    }
}

#if RTB_HOST_SIDE
// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
int launch_tree_inertia_vjp(const Tree *t, const DevGroup *groups, const double *q, int64_t N, const double *gM, double *gq, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (t->n < 1 || t->n > kTreeInertiaVjpMaxGroups) { set_error("tree_inertia_vjp: robots of 1..20 joints"); return RTBHIP_ELIMIT; }
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("tree_inertia_vjp: batch too large for one launch"); return RTBHIP_ELIMIT; }
    TreeInertiaVjpParams tp;
    tp.n = t->n; tp.nslots = t->nslots; tp.N = N;
    const size_t lds = (size_t)kWave * (tree_inertia_vjp_stride(t->n, t->nslots) + kTreeSlotDoubles * t->nslots) * sizeof(double);
    if (lds > 160 * 1024) { set_error("tree_inertia_vjp: tree needs more LDS than a CU has"); return RTBHIP_ELIMIT; }
    const bool rt = t->n > kTreeInertiaVjpRegMax;
    dim3 grid((unsigned)(rt && tiles > 65536 ? 65536 : tiles));      // the run-time-n kernel strides over the tiles
    switch (rt ? 0 : t->n) {
    case 1: vjp_go(k_tree_inertia_vjp<1>, grid, lds, s, tp, groups, q, gM, gq); break;
    case 2: vjp_go(k_tree_inertia_vjp<2>, grid, lds, s, tp, groups, q, gM, gq); break;
    case 3: vjp_go(k_tree_inertia_vjp<3>, grid, lds, s, tp, groups, q, gM, gq); break;
    case 4: vjp_go(k_tree_inertia_vjp<4>, grid, lds, s, tp, groups, q, gM, gq); break;
    case 5: vjp_go(k_tree_inertia_vjp<5>, grid, lds, s, tp, groups, q, gM, gq); break;
    case 6: vjp_go(k_tree_inertia_vjp<6>, grid, lds, s, tp, groups, q, gM, gq); break;
    case 7: vjp_go(k_tree_inertia_vjp<7>, grid, lds, s, tp, groups, q, gM, gq); break;
    case 8: vjp_go(k_tree_inertia_vjp<8>, grid, lds, s, tp, groups, q, gM, gq); break;
    default: vjp_go(k_tree_inertia_vjp_rt, grid, lds, s, tp, groups, q, gM, gq); break;
    }
    note_launch((int)grid.x, kWave, (int)lds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_tree_inertia_vjp launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

#endif  // RTB_TREE_INERTIA_VJP_LANE_ONLY

#pragma clang fp contract(fast)
}  // namespace rtbhip
