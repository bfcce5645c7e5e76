// vjp_device.h -- the arithmetic the adjoint (vector-Jacobian product) lane bodies share: rne_vjp_lane, inertia_vjp_lane, coriolis_vjp_lane
// and their tree counterparts.  Per-lane functions of values the caller has in hand; the tile I/O around the lane bodies is vjp_tile.h.
#pragma once
#include "rne_device.h"

namespace rtbhip {

// every floating-point operation as written (see rne_device.h).  The kernel files switch contraction off before their own text only: this
// header is included above that line, and a helper contracted here would change the bits of every adjoint
#pragma clang fp contract(off)

RTB_HD double vjp_zcross(V3 a, V3 b) { return __builtin_fma(a.x, b.y, -(a.y * b.x)); }       // (a x b).z = ((0, 0, 1) x a) . b
RTB_HD V3 vjp_zrate_cross(double s, V3 v) { return v3(-(s * v.y), s * v.x, 0.0); }            // (0, 0, s) x v
template <class LinkT>
RTB_HD V3 vjp_inertia_t_times(const LinkT &l, V3 v)      // the transpose of inertia_times
{
    return v3(__builtin_fma(l.I[2], v.z, __builtin_fma(l.I[1], v.y, l.I[0] * v.x)), __builtin_fma(l.I[5], v.z, __builtin_fma(l.I[4], v.y, l.I[3] * v.x)),
              __builtin_fma(l.I[8], v.z, __builtin_fma(l.I[7], v.y, l.I[6] * v.x)));
}

// a V3 at doubles b .. b + 2 of a lane's branch-slot (or kept-state) area; slot(index) -> double&
template <class Slot> RTB_HD V3 vjp_slot_get(Slot &slot, int b) { return v3(slot(b + 0), slot(b + 1), slot(b + 2)); }
template <class Slot> RTB_HD void vjp_slot_put(Slot &slot, int b, V3 v) { slot(b + 0) = v.x; slot(b + 1) = v.y; slot(b + 2) = v.z; }
template <class Slot> RTB_HD void vjp_slot_add(Slot &slot, int b, V3 v) { slot(b + 0) += v.x; slot(b + 1) += v.y; slot(b + 2) += v.z; }

// Sweep 2 of the DH lane bodies, the primal backward recursion: (F_j, N_j) -> (f_j, n_j) in place, tip -> link `first` (the links before it
// are skipped: the multi-pass bodies read f and n of the links after the pass's own only).  ftip / ntip: the wrench on the tip, in its frame.
// (rne_vjp_kernels.hip's header has the formulas.)  NJ = 0: run-time n
template <int NJ, bool MDH, int CAP, class LinksP>
RTB_HD void vjp_dh_sweep2(LinksP links, int n_rt, const double (&st)[CAP], const double (&ct)[CAP], V3 (&Fq)[CAP], V3 (&Nq)[CAP], V3 ftip, V3 ntip,
                          int first)
{
#pragma clang fp contract(off)
    const int n = NJ > 0 ? NJ : n_rt;
    V3 f = ftip, nn = ntip, psn = v3(0, 0, 0);
    Rot Rn = {0, 1, 0, 1, 0};
#pragma unroll
    for (int jj = 0; jj < n; ++jj) {
        const int j = n - 1 - jj;
        if (j < first) continue;
        const auto &l = links[j];
        const V3 ps = link_offset<MDH>(l, l.d), rc = v3(l.rx, l.ry, l.rz);
        const V3 fn = jj == 0 ? f : rot_fwd<MDH>(Rn, f), gn = jj == 0 ? nn : rot_fwd<MDH>(Rn, nn);
        const V3 F = Fq[j];
        const V3 nj = MDH ? cross_add(psn, fn, cross_add(rc, F, gn + Nq[j])) : cross_add(ps, fn, cross_add(ps + rc, F, gn + Nq[j]));
        f = fn + F; nn = nj;
        Fq[j] = f; Nq[j] = nn;
        Rn = Rot{st[j], ct[j], l.sa, l.ca, 0}; psn = ps;
        if (NJ > 0) sched_fence();
    }
}

#pragma clang fp contract(fast)
}  // namespace rtbhip
