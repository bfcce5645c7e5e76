// coriolis_vjp_kernels.hip -- gfx950 kernels for the VECTOR-JACOBIAN PRODUCT of the batched Coriolis / centripetal matrix of a DH arm
// (rtbhip_coriolis_vjp):
//
//     gq [r,m] = sum_jk gC[r,j,k] d C[r,j,k] / d q [r,m]
//     gqd[r,m] = sum_jk gC[r,j,k] d C[r,j,k] / d qd[r,m]
//
// for chains whose links are all revolute.  The forward kernel (dyn_device.h: rne_bilinear_core) computes C[j,k] = 1/2 B_j(u = qd, w = e_k) from
// the TWO-FIELD Newton-Euler recursion: the pass of rne_core without gravity, acceleration and friction, in which every product of two velocities
// x(v) y(v) is replaced by x(u) y(w) + x(w) y(u).  B_j is linear in w, so
//     sum_k gC[j,k] B_j(u, e_k) = B_j(u, gC[j,:])
// and the adjoint is the sum over the ROWS j of gC of the reverse-mode sweep of one two-field pass whose w field has the joint rates gC[j,:] and
// whose only seeded torque is 1/2 on joint j (pass layout (b): one contiguous row of gC per pass, one seed, sweep 2 and sweep 3 start at link j).
// gC is a constant of the differentiation; gqd comes from the adjoint of the u field's joint rates in the same sweeps.  Both results are linear in
// qd, as C is: nothing here evaluates a general pass at qd +- e_k.
//
// The lane body is rne_vjp_lane (rne_vjp_kernels.hip, whose header has the single-field formulas) with both velocity fields carried and every
// bilinear term's adjoint taken both ways round.  With prev = (wu, ww, wd, a)_{l-1}, R = R_l, p* = p*_l, z = (0, 0, 1), qu = qd_l, qw = gC[j,l]:
//   modified DH   tu = R^T wu_prev;  tw = R^T ww_prev;  wu = tu + z qu;  ww = tw + z qw;  wd = R^T wd_prev + tu x z qw + tw x z qu
//                 a = R^T (a_prev + wd_prev x p* + wu_prev x (ww_prev x p*) + ww_prev x (wu_prev x p*))
//   standard DH   wu = R^T (wu_prev + z qu);  ww = R^T (ww_prev + z qw);  wd = R^T (wd_prev + wu_prev x z qw + ww_prev x z qu)
//                 a = R^T a_prev + wd x p* + wu x (ww x p*) + ww x (wu x p*)
//   both          F = m (a + wd x r + wu x (ww x r) + ww x (wu x r));   N = I wd + wu x I ww + ww x I wu;   the backward recursion as rne_core
// and for the adjoints Fb, Nb of F, N (acb = m Fb):
//   wub += (ww x r) x acb + r x (acb x ww) + (I ww) x Nb + I^T (Nb x ww)          wwb: the same with wu in place of ww
//   the recursion step: the single-field step with (w, wb) -> the other field's velocity and this field's adjoint, and
//   gqd_l = wub.z + (wdb x tw).z  (modified),   (R wub).z + (R wdb x ww_prev).z  (standard)
// Tape: f, n = 6 doubles per link -- and NOT wu, ww, wd, a.  Taped, the two-field state is 18 doubles per link and seven links spill (measured: 137
// to 167 spilled registers); but every forward step is a rotation plus terms of the state it produces, so sweep 4, which walks tip -> base anyway,
// runs it BACKWARDS from the tip's state:  modified DH  wu_prev = R (wu - z qu),  wd_prev = R (wd - tu x z qw - tw x z qu),  a_prev = R a - (the
// offset terms of the state just recovered);  standard DH likewise with the rotation first.  That costs a rotation and a few products more per link,
// rounds differently from the forward values by a few ulp (linear in both fields, so the homogeneity in qd stays exact) and leaves the base at
// rest exactly.  One lane = one sample; sin / cos once per lane, then a `#pragma unroll 1` loop over the passes, each kept self-contained by
// dyn_opaque (dyn_device.h tells why); gq and gqd accumulate in 2 n registers (the part of theta's adjoint that sweep 3 finds goes straight into
// gq's).  A chain of one joint has C = 0: no pass.
// I/O: the wave's (64 x n) blocks of q and qd and its (64 x n x n) block of gC are contiguous in memory, loaded coalesced -- all loads in flight
// before the first LDS write -- into a lane-major LDS tile of  q (n) | qd (n) | gC (n^2)  doubles per row at an odd stride: 63 doubles per row for
// n = 7, 31.5 KB per wave.  C is not symmetric: nothing folds.  The run-time-n form cannot keep that tile (n = 16: 147 KB): its row is
// q | qd | one row of gC, which every lane stages from memory at the head of each pass.  gq and gqd overwrite the q and qd slots and leave as
// contiguous non-temporal stores.
#include "dyn_device.h"
#include "vjp_tile.h"

namespace rtbhip {

#pragma clang fp contract(off)      // every operation as written, as rne_vjp_kernels.hip

RTB_HD V3 cv_sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }

// One sample.  links: the wave-uniform link table, every link revolute.  qin(l), qdin(l): the joint angles and rates; q is read up front, qd stays
// readable until the last pass is over.  begin(j): called at the head of pass j (the run-time-n kernel stages row j of gC there).  gin(j, l):
// gC[j,l], read during pass j only.  gq(l, v), gqd(l, v): called once per joint, after the last pass.  NJ = 0: run-time n, the per-link arrays in
// private memory.
template <int NJ, bool MDH, class LinksP, class InQ, class InQd, class Begin, class InG, class OutQ, class OutQd>
RTB_HD void coriolis_vjp_lane(LinksP links, int n_rt, InQ qin, InQd qdin, Begin begin, InG gin, OutQ gq, OutQd gqd)
{
#pragma clang fp contract(off)
    constexpr int CAP = NJ > 0 ? NJ : RTBHIP_MAX_JOINTS;
    const int n = NJ > 0 ? NJ : n_rt;
    double st[CAP], ct[CAP], accq[CAP], accd[CAP];
    V3 Fq[CAP], Nq[CAP];
    if constexpr (NJ > 0) {
        rne_trig<NJ, true>(links, qin, st, ct);
    } else {
        for (int j = 0; j < n; ++j) rtb_sincos(qin(j) + links[j].offset, &st[j], &ct[j]);
    }
#pragma unroll
    for (int j = 0; j < n; ++j) { accq[j] = 0.0; accd[j] = 0.0; }

#pragma unroll 1
    for (int i = 0; i < (n > 1 ? n : 0); ++i) {
        if constexpr (NJ > 0) dyn_opaque<NJ>(st, ct);
        begin(i);
        // ---- 1. primal forward recursion, both fields: F and N of every link (kept), wu, ww, wd, a of the tip (sweep 4 runs them back down)
        V3 wu = v3(0, 0, 0), ww = v3(0, 0, 0), wd = v3(0, 0, 0), a = v3(0, 0, 0);
        {
#pragma unroll
            for (int j = 0; j < n; ++j) {
                const auto &l = links[j];
                const Rot R = {st[j], ct[j], l.sa, l.ca, 0};
                const V3 ps = link_offset<MDH>(l, l.d), rc = v3(l.rx, l.ry, l.rz);
                const double qdu = qdin(j), qdw = gin(i, j);
                V3 wun, wwn, wdn, an;
                if (MDH) {
                    const V3 tu = rot_inv<MDH>(R, wu), tw = rot_inv<MDH>(R, ww);
                    wun = addz(tu, qdu); wwn = addz(tw, qdw);
                    wdn = rot_inv<MDH>(R, wd) + (crossz(tu, qdw) + crossz(tw, qdu));
                    an = rot_inv<MDH>(R, cross_add(wd, ps, cross_add(wu, cross(ww, ps), cross_add(ww, cross(wu, ps), a))));
                } else {
                    wun = rot_inv<MDH>(R, addz(wu, qdu)); wwn = rot_inv<MDH>(R, addz(ww, qdw));
                    wdn = rot_inv<MDH>(R, wd + (crossz(wu, qdw) + crossz(ww, qdu)));
                    an = cross_add(wdn, ps, cross_add(wun, cross(wwn, ps), cross_add(wwn, cross(wun, ps), rot_inv<MDH>(R, a))));
                }
                wu = wun; ww = wwn; wd = wdn; a = an;
                Fq[j] = l.m * cross_add(wd, rc, cross_add(wu, cross(ww, rc), cross_add(ww, cross(wu, rc), a)));
                Nq[j] = cross_add(wu, inertia_times(l, ww), cross_add(ww, inertia_times(l, wu), inertia_times(l, wd)));
                if (NJ > 0) sched_fence();
            }
        }

        // ---- 2. primal backward recursion: (F_j, N_j) -> (f_j, n_j) in place, for the links j > i (sweep 3 reads f and n of link j + 1 only)
        {
            V3 f = v3(0, 0, 0), nn = v3(0, 0, 0), psn = v3(0, 0, 0);
            Rot Rn = {0, 1, 0, 1, 0};
#pragma unroll
            for (int jj = 0; jj < n; ++jj) {
                const int j = n - 1 - jj;
                if (j <= i) continue;
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

        // ---- 3. adjoint of the backward recursion, link i -> tip (the links before i take no seed and have no adjoint): (f_j, n_j) -> the
        //         adjoints of (F_j, N_j) in place
        {
            V3 fb = v3(0, 0, 0), nb = v3(0, 0, 0);
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (j < i) continue;
                const auto &l = links[j];
                if (j == i) {
                    if (MDH) nb.z = 0.5;
                    else { nb.y = 0.5 * l.sa; nb.z = 0.5 * l.ca; }
                }
                const V3 ps = link_offset<MDH>(l, l.d), rc = v3(l.rx, l.ry, l.rz);
                V3 Fb, fnb = fb;
                if (MDH) Fb = cross_add(nb, rc, fb);
                else { Fb = cross_add(nb, ps + rc, fb); fnb = cross_add(nb, ps, fb); }
                if (j + 1 < n) {
                    const auto &l1 = links[j + 1];
                    const Rot R1 = {st[j + 1], ct[j + 1], l1.sa, l1.ca, 0};
                    if (MDH) fnb = cross_add(nb, link_offset<MDH>(l1, l1.d), fnb);
                    const V3 f1 = Fq[j + 1], n1 = Nq[j + 1];
                    const V3 fb1 = rot_inv<MDH>(R1, fnb), nb1 = rot_inv<MDH>(R1, nb);
                    if (MDH) accq[j + 1] = accq[j + 1] + (vjp_zcross(f1, fb1) + vjp_zcross(n1, nb1));
                    else accq[j + 1] = accq[j + 1] + (vjp_zcross(rot_fwd<MDH>(R1, f1), fnb) + vjp_zcross(rot_fwd<MDH>(R1, n1), nb));
                    Fq[j] = Fb; Nq[j] = nb;
                    fb = fb1; nb = nb1;
                } else {
                    Fq[j] = Fb; Nq[j] = nb;
                }
                if (NJ > 0) sched_fence();
            }
        }

        // ---- 4. adjoint of the forward recursion, tip -> base (the link terms of the links j >= i; the recursion step of every link)
        {
            V3 wub = v3(0, 0, 0), wwb = v3(0, 0, 0), wdb = v3(0, 0, 0), ab = v3(0, 0, 0);
#pragma unroll
            for (int jj = 0; jj < n; ++jj) {
                const int j = n - 1 - jj;
                const auto &l = links[j];
                const Rot R = {st[j], ct[j], l.sa, l.ca, 0};
                const V3 ps = link_offset<MDH>(l, l.d), rc = v3(l.rx, l.ry, l.rz);
                const double qdu = qdin(j), qdw = gin(i, j);
                if (j >= i) {
                    const V3 Fb = Fq[j], Nb = Nq[j];
                    // the link terms:  F = m (a + wd x r + wu x (ww x r) + ww x (wu x r)),  N = I wd + wu x (I ww) + ww x (I wu)
                    const V3 acb = l.m * Fb;
                    ab = ab + acb;
                    wdb = cross_add(rc, acb, wdb + vjp_inertia_t_times(l, Nb));
                    wub = cross_add(cross(ww, rc), acb, wub);
                    wub = cross_add(rc, cross(acb, ww), wub);
                    wub = cross_add(inertia_times(l, ww), Nb, wub);
                    wub = wub + vjp_inertia_t_times(l, cross(Nb, ww));
                    wwb = cross_add(cross(wu, rc), acb, wwb);
                    wwb = cross_add(rc, cross(acb, wu), wwb);
                    wwb = cross_add(inertia_times(l, wu), Nb, wwb);
                    wwb = wwb + vjp_inertia_t_times(l, cross(Nb, wu));
                }
                // the recursion step.  The state of link j - 1 is not taped: the forward step is run backwards from the state of link j (a rotation
                // and a few products; the base is at rest exactly)
                const V3 o = v3(0, 0, 0);
                V3 wup, wwp, wdp, ap, wubp, wwbp, wdbp, abp;
                double t, oqd;
                if (MDH) {
                    const V3 tu = addz(wu, -qdu), tw = addz(ww, -qdw);          // R^T wu_prev, R^T ww_prev
                    const V3 twd = cv_sub(wd, crossz(tu, qdw) + crossz(tw, qdu));    // R^T wd_prev
                    wup = j > 0 ? rot_fwd<MDH>(R, tu) : o;
                    wwp = j > 0 ? rot_fwd<MDH>(R, tw) : o;
                    wdp = j > 0 ? rot_fwd<MDH>(R, twd) : o;
                    ap = j > 0 ? cv_sub(rot_fwd<MDH>(R, a), cross_add(wdp, ps, cross_add(wup, cross(wwp, ps), cross(wwp, cross(wup, ps))))) : o;
                    const V3 Xb = rot_fwd<MDH>(R, ab);
                    t = -vjp_zcross(a, ab);
                    abp = Xb;
                    wdbp = cross(ps, Xb);
                    wubp = cross_add(ps, cross(Xb, wwp), cross(cross(wwp, ps), Xb));
                    wwbp = cross_add(ps, cross(Xb, wup), cross(cross(wup, ps), Xb));
                    t = t - vjp_zcross(twd, wdb);
                    wdbp = wdbp + rot_fwd<MDH>(R, wdb);
                    const V3 tub = wub + vjp_zrate_cross(qdw, wdb), twb = wwb + vjp_zrate_cross(qdu, wdb);
                    oqd = wub.z + vjp_zcross(wdb, tw);
                    t = t - (vjp_zcross(tu, tub) + vjp_zcross(tw, twb));
                    wubp = wubp + rot_fwd<MDH>(R, tub);
                    wwbp = wwbp + rot_fwd<MDH>(R, twb);
                } else {
                    wdb = cross_add(ps, ab, wdb);
                    wub = cross_add(cross(ww, ps), ab, wub);
                    wub = cross_add(ps, cross(ab, ww), wub);
                    wwb = cross_add(cross(wu, ps), ab, wwb);
                    wwb = cross_add(ps, cross(ab, wu), wwb);
                    const V3 tu = rot_fwd<MDH>(R, wu), tw = rot_fwd<MDH>(R, ww), t3 = rot_fwd<MDH>(R, wd);      // wu_prev + z qu, ww_prev + z qw, the sum wd is rotated from
                    wup = j > 0 ? addz(tu, -qdu) : o;
                    wwp = j > 0 ? addz(tw, -qdw) : o;
                    wdp = j > 0 ? cv_sub(t3, crossz(wup, qdw) + crossz(wwp, qdu)) : o;
                    ap = j > 0 ? rot_fwd<MDH>(R, cv_sub(a, cross_add(wd, ps, cross_add(wu, cross(ww, ps), cross(ww, cross(wu, ps)))))) : o;
                    abp = rot_fwd<MDH>(R, ab);
                    const V3 t3b = rot_fwd<MDH>(R, wdb), tub = rot_fwd<MDH>(R, wub), twb = rot_fwd<MDH>(R, wwb);
                    t = -(vjp_zcross(ap, abp) + (vjp_zcross(t3, t3b) + (vjp_zcross(tu, tub) + vjp_zcross(tw, twb))));
                    wdbp = t3b;
                    wubp = tub + vjp_zrate_cross(qdw, t3b);
                    wwbp = twb + vjp_zrate_cross(qdu, t3b);
                    oqd = tub.z + vjp_zcross(t3b, wwp);
                }
                accq[j] = accq[j] + t;
                accd[j] = accd[j] + oqd;
                wub = wubp; wwb = wwbp; wdb = wdbp; ab = abp;
                wu = wup; ww = wwp; wd = wdp; a = ap;
                if (NJ > 0) sched_fence();
            }
        }
    }
#pragma unroll
    for (int j = 0; j < n; ++j) { gq(j, accq[j]); gqd(j, accd[j]); }
}

#ifndef RTB_CORIOLIS_VJP_LANE_ONLY      // (a host-side replay of the lane body includes this file for coriolis_vjp_lane alone)

typedef const __attribute__((address_space(4))) DevLink *CvLinks;
constexpr int kCoriolisVjpMaxJoints = 16;      // the forward kernel's built-in sizes
constexpr int kCoriolisVjpRegMax = 7;          // the largest compile-time joint count: eight links spill (DESIGN 4.16 has the register table)

struct CoriolisVjpParams {
    int32_t n, pad_;
    int64_t N;
};

// LDS row of one sample at an odd stride (conflict-free rows): q (n) | qd (n) | gC (n^2) for a compile-time joint count, q | qd | one row of gC
// for the run-time-n form
inline __host__ __device__ int coriolis_vjp_stride(int n, bool rt) { return (2 * n + (rt ? n : n * n)) | 1; }

// One tile of 64 samples.  gq / gqd NULL: not stored.  This unit keeps its own staging and flush, and its lane body its own sweep 2: with
// vjp_tile.h's phases (or vjp_dh_sweep2) in their place the Panda's adjoint measured 0.5 to 4 % slower (profiles/vjp_tile_refactor_ab.json).
template <int NJ, bool MDH>
__device__ __forceinline__ void coriolis_vjp_tile(const CoriolisVjpParams &cp, CvLinks links, int n, int stride, int64_t tile, const double *__restrict__ q,
                                                  const double *__restrict__ qd, const double *__restrict__ gC, double *__restrict__ gq,
                                                  double *__restrict__ gqd, double *lds, int lane)
{
    const int64_t cfg0 = tile * kWave;
    const int64_t left = cp.N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    const int nn = n * n;
    const int count = ncfg * n, mcount = ncfg * nn;
    const double *qg = q + cfg0 * n, *dg = qd + cfg0 * n, *mg = gC + cfg0 * nn;
    if constexpr (NJ > 0) {
        // the 2 NJ + NJ^2 coalesced loads of the tile, UNCONDITIONAL (an element past the ragged tail reads element 0 of the tile; the zeros are
        // selected afterwards: vjp_tile.h tells why), all in flight before the first LDS write
        double rq[NJ], rd[NJ], rm[NJ * NJ];
#pragma unroll
        for (int k = 0; k < NJ; ++k) { const int f = lane + kWave * k, fc = f < count ? f : 0; rq[k] = qg[fc]; rd[k] = dg[fc]; }
#pragma unroll
        for (int k = 0; k < NJ * NJ; ++k) { const int f = lane + kWave * k; rm[k] = mg[f < mcount ? f : 0]; }
        sched_fence();
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int f = lane + kWave * k;
            double *dst = lds + (f / NJ) * stride + (f % NJ);
            dst[0] = f < count ? rq[k] : 0.0;
            dst[NJ] = f < count ? rd[k] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < NJ * NJ; ++k) {
            const int f = lane + kWave * k;
            lds[(f / (NJ * NJ)) * stride + 2 * NJ + (f % (NJ * NJ))] = f < mcount ? rm[k] : 0.0;
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
        if constexpr (NJ > 0) {
            coriolis_vjp_lane<NJ, MDH>(links, n, [&](int j) { return mine[j]; }, [&](int j) { return mine[NJ + j]; }, [](int) {},
                                       [&](int i, int j) { return mine[2 * NJ + i * NJ + j]; }, [&](int j, double v) { mine[j] = v; },
                                       [&](int j, double v) { mine[NJ + j] = v; });
        } else {
            // row i of this lane's gC, staged at the head of pass i into the lane's own LDS row (written and read by this lane alone: no barrier)
            const double *rowg = mg + (int64_t)lane * nn;
            coriolis_vjp_lane<0, MDH>(links, n, [&](int j) { return mine[j]; }, [&](int j) { return mine[n + j]; },
                                      [&](int i) { for (int c = 0; c < n; ++c) mine[2 * n + c] = rowg[i * n + c]; },
                                      [&](int, int j) { return mine[2 * n + j]; }, [&](int j, double v) { mine[j] = v; },
                                      [&](int j, double v) { mine[n + j] = v; });
        }
    }
    __syncthreads();
    double *gout[2] = {gq ? gq + cfg0 * n : nullptr, gqd ? gqd + cfg0 * n : nullptr};
    if constexpr (NJ > 0) {
        double r[2][NJ];
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int f = lane + kWave * k;
            const double *src = lds + (f / NJ) * stride + (f % NJ);
            r[0][k] = src[0]; r[1][k] = src[NJ];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (!gout[a]) continue;          // wave-uniform
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                const int f = lane + kWave * k;
                if (f < count) __builtin_nontemporal_store(r[a][k], gout[a] + f);
            }
        }
    } else {
        for (int f = lane; f < count; f += kWave) {
            const double *src = lds + (f / n) * stride + (f % n);
            if (gout[0]) gout[0][f] = src[0];
            if (gout[1]) gout[1][f] = src[n];
        }
    }
}

// compile-time joint count: one tile per single-wave workgroup, one wave per SIMD
template <int NJ, bool MDH>
__global__ __launch_bounds__(kWave, 1) void k_coriolis_vjp(CoriolisVjpParams cp, const DevLink *links_g, const double *__restrict__ q,
                                                           const double *__restrict__ qd, const double *__restrict__ gC, double *__restrict__ gq,
                                                           double *__restrict__ gqd)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    coriolis_vjp_tile<NJ, MDH>(cp, (CvLinks)links_g, NJ, coriolis_vjp_stride(NJ, false), blockIdx.x, q, qd, gC, gq, gqd, lds, threadIdx.x);
}

// run-time joint count (8 .. 16 joints, or more tiles than a grid has blocks): grid-stride over tiles, the tape
// in private memory
template <bool MDH>
__global__ __launch_bounds__(kWave) void k_coriolis_vjp_rt(CoriolisVjpParams cp, const DevLink *links_g, const double *__restrict__ q,
                                                          const double *__restrict__ qd, const double *__restrict__ gC, double *__restrict__ gq,
                                                          double *__restrict__ gqd)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int n = cp.n;
    const int stride = coriolis_vjp_stride(n, true);
    const int64_t tiles = (cp.N + kWave - 1) / kWave;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        coriolis_vjp_tile<0, MDH>(cp, (CvLinks)links_g, n, stride, tile, q, qd, gC, gq, gqd, lds, threadIdx.x);
        __syncthreads();
    }
}

#if RTB_HOST_SIDE
namespace {

template <int NJ>
void coriolis_vjp_go_nj(bool mdh, dim3 grid, size_t lds, hipStream_t s, const CoriolisVjpParams &cp, const DevLink *links, const double *q,
                        const double *qd, const double *gC, double *gq, double *gqd)
{
    if (mdh) vjp_go(k_coriolis_vjp<NJ, true>, grid, lds, s, cp, links, q, qd, gC, gq, gqd);
    else vjp_go(k_coriolis_vjp<NJ, false>, grid, lds, s, cp, links, q, qd, gC, gq, gqd);
}

}  // namespace

// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
int launch_coriolis_vjp(const Dyn *d, const DevLink *links, const double *q, const double *qd, int64_t N, const double *gC, double *gq, double *gqd,
                        hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (d->n < 1 || d->n > kCoriolisVjpMaxJoints) { set_error("coriolis_vjp: chains of 1..16 joints"); return RTBHIP_ELIMIT; }
    CoriolisVjpParams cp;
    cp.n = d->n; cp.pad_ = 0; cp.N = N;
    const int64_t tiles = (N + kWave - 1) / kWave;
    const bool mdh = d->mdh != 0;
    const bool rt = d->n > kCoriolisVjpRegMax || tiles > 0x7fffffff;
    const size_t lds = (size_t)kWave * coriolis_vjp_stride(d->n, rt) * sizeof(double);
    dim3 grid((unsigned)(rt && tiles > 65536 ? 65536 : tiles));      // the run-time-n kernel strides over the tiles
    switch (rt ? 0 : d->n) {
    case 1: coriolis_vjp_go_nj<1>(mdh, grid, lds, s, cp, links, q, qd, gC, gq, gqd); break;
    case 2: coriolis_vjp_go_nj<2>(mdh, grid, lds, s, cp, links, q, qd, gC, gq, gqd); break;
    case 3: coriolis_vjp_go_nj<3>(mdh, grid, lds, s, cp, links, q, qd, gC, gq, gqd); break;
    case 4: coriolis_vjp_go_nj<4>(mdh, grid, lds, s, cp, links, q, qd, gC, gq, gqd); break;
    case 5: coriolis_vjp_go_nj<5>(mdh, grid, lds, s, cp, links, q, qd, gC, gq, gqd); break;
    case 6: coriolis_vjp_go_nj<6>(mdh, grid, lds, s, cp, links, q, qd, gC, gq, gqd); break;
    case 7: coriolis_vjp_go_nj<7>(mdh, grid, lds, s, cp, links, q, qd, gC, gq, gqd); break;
    default:
        if (mdh) vjp_go(k_coriolis_vjp_rt<true>, grid, lds, s, cp, links, q, qd, gC, gq, gqd);
        else vjp_go(k_coriolis_vjp_rt<false>, grid, lds, s, cp, links, q, qd, gC, gq, gqd);
        break;
    }
    note_launch((int)grid.x, kWave, (int)lds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_coriolis_vjp launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

#endif  // RTB_CORIOLIS_VJP_LANE_ONLY

#pragma clang fp contract(fast)
}  // namespace rtbhip
