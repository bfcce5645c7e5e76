// rne_vjp_kernels.hip -- gfx950 kernels for the VECTOR-JACOBIAN PRODUCT of batched inverse dynamics (rtbhip_rne_vjp, rtbhip_rne_vjp_f32):
//
//     gq[i,k] = sum_j gtau[i,j] d tau_j / d q_k        (likewise gqd, gqdd)
//
// the exact reverse-mode adjoint of the Newton-Euler recursion rne_core evaluates (rne_device.h; newton_euler, core/ne.c:62-493), for chains
// whose links are all revolute.  No reference counterpart: the reference has no derivative of its dynamics.
//
// One lane = one sample (q, qd, qdd, gtau); four sweeps over the links, all in registers for a compile-time joint count:
//   1. primal, base -> tip:   w, wd, a per link (kept: the tape), F = m a_c and N = I wd + w x I w (transient)
//   2. primal, tip -> base:   f, n per link, written over F and N
//   3. adjoint, base -> tip, of sweep 2:  seeded with gtau_j * axis_j on n_j; leaves the adjoints of F_j and N_j in the slots of f_j and n_j
//      (dead by then) and the part of theta_j's adjoint that comes from  R_j f_j  and  R_j n_j
//   4. adjoint, tip -> base, of sweep 1:  the link terms (F, N -> w, wd, a), then the recursion step; emits gq_j, gqd_j, gqdd_j
// With  prev = (w, wd, a)_{j-1}  ((0, 0, gravity) for the first link),  R = R_j,  p* = p*_j,  z = (0, 0, 1)  both conventions are uniform in j:
//   modified DH   t1 = R^T w_prev;  w = t1 + z qd;  wd = R^T wd_prev + t1 x z qd + z qdd;  a = R^T (a_prev + wd_prev x p* + w_prev x (w_prev x p*))
//                 f_j = R_{j+1} f_{j+1} + F_j;   n_j = R_{j+1} n_{j+1} + N_j + r_j x F_j + p*_{j+1} x (R_{j+1} f_{j+1});   tau_j = n_j.z
//   standard DH   t1 = w_prev + z qd;  t3 = wd_prev + z qdd + w_prev x z qd;  w = R^T t1;  wd = R^T t3;  a = R^T a_prev + wd x p* + w x (w x p*)
//                 f_j = R_{j+1} f_{j+1} + F_j;   n_j = R_{j+1} n_{j+1} + N_j + (p*_j + r_j) x F_j + p*_j x (R_{j+1} f_{j+1});   tau_j = (0, sa, ca) . n_j
// (R_n = identity, f_n / n_n the external wrench, p*_n = 0) plus the joint-space terms  G^2 Jm qdd_j + G^2 B qd_j + Coulomb  (derivative zero).
// The angle enters through the rotations alone.  For y = R v with adjoint u:  modified DH  d(u . y)/d theta = (v x R^T u).z,  standard DH
// (y x u).z;  for y = R^T v:  modified DH  -(y x u).z,  standard DH  -(v x R u).z -- each from vectors the sweep has in hand anyway.
// Constants of the differentiation: gravity and the external wrench (held in the tip frame).  The exact-zero link flags are not looked at: the
// general formulas give the same values.
//
// Tape: 15 doubles per link (w, wd, a; f, n) -- 210 VGPRs for seven links, 240 for eight, plus the working set: one wave per SIMD
// (__launch_bounds__(64, 1), the 512-entry register file).  I/O as k_rne: the wave's (64 x n) blocks of q, qd, qdd and gtau are contiguous in
// memory, loaded coalesced into a lane-major LDS tile (odd row stride); gq, gqd, gqdd overwrite the q, qd, qdd slots and leave the same way.
#include "vjp_tile.h"

namespace rtbhip {

// every floating-point operation as written (see rne_device.h): the float32 instantiation must return the fp64 one's numbers, rounded once
#pragma clang fp contract(off)

// One sample.  links: the wave-uniform link table, every link revolute.  qin / qdin / qddin / gin: per-lane readers  in(j) -> double;
// gq / gqd / gqdd: writers  out(j, v).  q is read up front; qd_j, qdd_j and gtau_j must stay readable until gq_j, gqd_j, gqdd_j have been written
// (the kernel lets them overwrite the q, qd, qdd slots).  NJ = 0: run-time n, the per-link arrays in private memory.
template <int NJ, bool MDH, class LinksP, class InQ, class InQd, class InQdd, class InG, class OutQ, class OutQd, class OutQdd>
RTB_HD void rne_vjp_lane(LinksP links, int n_rt, V3 grav, V3 ftip, V3 ntip, InQ qin, InQd qdin, InQdd qddin, InG gin, OutQ gq, OutQd gqd, OutQdd gqdd)
{
#pragma clang fp contract(off)
    constexpr int CAP = NJ > 0 ? NJ : RTBHIP_MAX_JOINTS;
    const int n = NJ > 0 ? NJ : n_rt;
    double st[CAP], ct[CAP], th[CAP];
    V3 W[CAP], WD[CAP], A[CAP], Fq[CAP], Nq[CAP];
    if constexpr (NJ > 0) {
        rne_trig<NJ, true>(links, qin, st, ct);
    } else {
        for (int j = 0; j < n; ++j) rtb_sincos(qin(j) + links[j].offset, &st[j], &ct[j]);
    }

    // ---- 1. primal forward recursion
    {
        V3 w = v3(0, 0, 0), wd = v3(0, 0, 0), a = grav;
#pragma unroll
        for (int j = 0; j < n; ++j) {
            const auto &l = links[j];
            const Rot R = {st[j], ct[j], l.sa, l.ca, 0};
            const V3 ps = link_offset<MDH>(l, l.d), rc = v3(l.rx, l.ry, l.rz);
            const double qdj = qdin(j), qddj = qddin(j);
            V3 wn, wdn, an;
            if (MDH) {
                const V3 t1 = rot_inv<MDH>(R, w);
                wn = addz(t1, qdj);
                wdn = addz(rot_inv<MDH>(R, wd) + crossz(t1, qdj), qddj);
                an = rot_inv<MDH>(R, cross_add(wd, ps, cross_add(w, cross(w, ps), a)));
            } else {
                wn = rot_inv<MDH>(R, addz(w, qdj));
                wdn = rot_inv<MDH>(R, addz(wd + crossz(w, qdj), qddj));
                an = cross_add(wdn, ps, cross_add(wn, cross(wn, ps), rot_inv<MDH>(R, a)));
            }
            w = wn; wd = wdn; a = an;
            W[j] = w; WD[j] = wd; A[j] = a;
            Fq[j] = l.m * cross_add(wd, rc, cross_add(w, cross(w, rc), a));
            Nq[j] = cross_add(w, inertia_times(l, w), inertia_times(l, wd));
            if (NJ > 0) sched_fence();
        }
    }

    // ---- 2. primal backward recursion: (F_j, N_j) -> (f_j, n_j) in place
    vjp_dh_sweep2<NJ, MDH>(links, n, st, ct, Fq, Nq, ftip, ntip, 0);

    // ---- 3. adjoint of the backward recursion, base -> tip: (f_j, n_j) -> the adjoints of (F_j, N_j) in place
    {
        V3 fb = v3(0, 0, 0), nb = v3(0, 0, 0);      // adjoints of f_j, n_j as link j - 1 handed them on
        th[0] = 0.0;
#pragma unroll
        for (int j = 0; j < n; ++j) {
            const auto &l = links[j];
            const double g = gin(j);
            if (MDH) nb.z = nb.z + g;
            else { nb.y = __builtin_fma(g, l.sa, nb.y); nb.z = __builtin_fma(g, l.ca, nb.z); }
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
                if (MDH) th[j + 1] = vjp_zcross(f1, fb1) + vjp_zcross(n1, nb1);
                else th[j + 1] = vjp_zcross(rot_fwd<MDH>(R1, f1), fnb) + vjp_zcross(rot_fwd<MDH>(R1, n1), nb);
                Fq[j] = Fb; Nq[j] = nb;
                fb = fb1; nb = nb1;
            } else {
                Fq[j] = Fb; Nq[j] = nb;
            }
            if (NJ > 0) sched_fence();
        }
    }

    // ---- 4. adjoint of the forward recursion, tip -> base
    {
        V3 wb = v3(0, 0, 0), wdb = v3(0, 0, 0), ab = v3(0, 0, 0);      // adjoints of w_j, wd_j, a_j as link j + 1 handed them on
#pragma unroll
        for (int jj = 0; jj < n; ++jj) {
            const int j = n - 1 - jj;
            const auto &l = links[j];
            const Rot R = {st[j], ct[j], l.sa, l.ca, 0};
            const V3 ps = link_offset<MDH>(l, l.d), rc = v3(l.rx, l.ry, l.rz);
            const V3 w = W[j], wd = WD[j], a = A[j], Fb = Fq[j], Nb = Nq[j];
            const double qdj = qdin(j), qddj = qddin(j), g = gin(j);
            // the link terms:  F = m (a + wd x r + w x (w x r)),  N = I wd + w x (I w)
            const V3 acb = l.m * Fb;
            ab = ab + acb;
            wdb = cross_add(rc, acb, wdb + vjp_inertia_t_times(l, Nb));
            wb = cross_add(cross(w, rc), acb, wb);
            wb = cross_add(rc, cross(acb, w), wb);
            wb = cross_add(inertia_times(l, w), Nb, wb);
            wb = wb + vjp_inertia_t_times(l, cross(Nb, w));
            // the recursion step
            const V3 wp = j > 0 ? W[j > 0 ? j - 1 : 0] : v3(0, 0, 0), wdp = j > 0 ? WD[j > 0 ? j - 1 : 0] : v3(0, 0, 0), ap = j > 0 ? A[j > 0 ? j - 1 : 0] : grav;
            V3 wbp, wdbp, abp;
            double t, oqd, oqdd;
            if (MDH) {
                const V3 Xb = rot_fwd<MDH>(R, ab);
                t = -vjp_zcross(a, ab);
                abp = Xb;
                wdbp = cross(ps, Xb);
                wbp = cross_add(ps, cross(Xb, wp), cross(cross(wp, ps), Xb));
                t = t - vjp_zcross(rot_inv<MDH>(R, wdp), wdb);
                wdbp = wdbp + rot_fwd<MDH>(R, wdb);
                const V3 t1 = rot_inv<MDH>(R, wp);
                const V3 t1b = wb + vjp_zrate_cross(qdj, wdb);
                oqd = wb.z + vjp_zcross(wdb, t1);
                oqdd = wdb.z;
                t = t - vjp_zcross(t1, t1b);
                wbp = wbp + rot_fwd<MDH>(R, t1b);
            } else {
                wdb = cross_add(ps, ab, wdb);
                wb = cross_add(cross(w, ps), ab, wb);
                wb = cross_add(ps, cross(ab, w), wb);
                abp = rot_fwd<MDH>(R, ab);
                const V3 t3b = rot_fwd<MDH>(R, wdb), t1b = rot_fwd<MDH>(R, wb);
                const V3 t1 = addz(wp, qdj), t3 = addz(wdp + crossz(wp, qdj), qddj);
                t = -(vjp_zcross(ap, abp) + (vjp_zcross(t3, t3b) + vjp_zcross(t1, t1b)));
                wdbp = t3b;
                oqdd = t3b.z;
                wbp = t1b + vjp_zrate_cross(qdj, t3b);
                oqd = t1b.z + vjp_zcross(t3b, wp);
            }
            gq(j, th[j] + t);
            gqd(j, __builtin_fma(l.gb, g, oqd));
            gqdd(j, __builtin_fma(l.gjm, g, oqdd));
            wb = wbp; wdb = wdbp; ab = abp;
            if (NJ > 0) sched_fence();
        }
    }
}

#ifndef RTB_RNE_VJP_LANE_ONLY      // (a host-side replay of the lane body includes this file for rne_vjp_lane alone)

typedef const __attribute__((address_space(4))) DevLink *VjpLinks;

struct RneVjpParams {
    int32_t n, has_fext;
    int64_t N;
    double grav[3];
    double fext[6];
};

// LDS row of one sample: q | qd | qdd | gtau, 4 n doubles; an odd stride (conflict-free rows) while the tile stays within 64 KiB
inline __host__ __device__ int rne_vjp_stride(int n) { return (4 * n + 1) * kWave * 8 <= 65536 ? 4 * n + 1 : 4 * n; }

// One tile of 64 samples.  S: the storage type of q, qd, qdd, gtau and of the gradients -- double, or float (widened after the load, rounded
// once before the store).  qd / qdd NULL: zeros.  gq / gqd / gqdd NULL: not stored (the lane body forms all three gradients either way: they share
// the four sweeps, and what is particular to one of them is a handful of operations per link).  The staging and the flush are vjp_tile.h's phases.
template <int NJ, bool MDH, class S>
__device__ __forceinline__ void rne_vjp_tile(const RneVjpParams &rp, VjpLinks links, int n, int stride, int64_t tile, const S *__restrict__ q,
                                             const S *__restrict__ qd, const S *__restrict__ qdd, const S *__restrict__ gtau, S *__restrict__ gq,
                                             S *__restrict__ gqd, S *__restrict__ gqdd, double *lds, int lane)
{
    const VjpTile t = vjp_tile_of(tile, rp.N, n);
    const int64_t at = t.cfg0 * n;
    const S *const gin[4] = {q + at, qd ? qd + at : nullptr, qdd ? qdd + at : nullptr, gtau + at};
    VjpCols<NJ, 4, S> cols;
    vjp_load_cols<NJ, true>(gin, t, lane, cols);
    sched_fence();
    vjp_stage_cols<NJ, true>(gin, t, n, stride, lane, cols, lds);
    __syncthreads();
    if (lane < t.ncfg) {
        double *mine = lds + lane * stride;
        const V3 grav = v3(rp.grav[0], rp.grav[1], rp.grav[2]);
        const V3 ftip = rp.has_fext ? v3(rp.fext[0], rp.fext[1], rp.fext[2]) : v3(0, 0, 0);
        const V3 ntip = rp.has_fext ? v3(rp.fext[3], rp.fext[4], rp.fext[5]) : v3(0, 0, 0);
        rne_vjp_lane<NJ, MDH>(links, n, grav, ftip, ntip, [&](int j) { return mine[j]; }, [&](int j) { return mine[n + j]; },
                              [&](int j) { return mine[2 * n + j]; }, [&](int j) { return mine[3 * n + j]; }, [&](int j, double v) { mine[j] = v; },
                              [&](int j, double v) { mine[n + j] = v; }, [&](int j, double v) { mine[2 * n + j] = v; });
    }
    __syncthreads();
    S *const gout[3] = {gq ? gq + at : nullptr, gqd ? gqd + at : nullptr, gqdd ? gqdd + at : nullptr};
    vjp_tile_flush<NJ, true>(gout, t, n, stride, lane, lds);
}

// compile-time joint count: one tile per single-wave workgroup (as k_rne: no grid-stride loop), one wave per SIMD
template <int NJ, bool MDH, class S>
__global__ __launch_bounds__(kWave, 1) void k_rne_vjp(RneVjpParams rp, const DevLink *links_g, const S *__restrict__ q, const S *__restrict__ qd,
                                                       const S *__restrict__ qdd, const S *__restrict__ gtau, S *__restrict__ gq, S *__restrict__ gqd,
                                                       S *__restrict__ gqdd)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    rne_vjp_tile<NJ, MDH, S>(rp, (VjpLinks)links_g, NJ, rne_vjp_stride(NJ), blockIdx.x, q, qd, qdd, gtau, gq, gqd, gqdd, lds, threadIdx.x);
}

// run-time joint count (9 .. 32 joints, or more tiles than a grid has blocks): grid-stride over tiles, the tape in private memory
template <bool MDH, class S>
__global__ __launch_bounds__(kWave) void k_rne_vjp_rt(RneVjpParams rp, const DevLink *links_g, const S *__restrict__ q, const S *__restrict__ qd,
                                                      const S *__restrict__ qdd, const S *__restrict__ gtau, S *__restrict__ gq, S *__restrict__ gqd,
                                                      S *__restrict__ gqdd)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int n = rp.n;
    const int stride = rne_vjp_stride(n);
    const int64_t tiles = (rp.N + kWave - 1) / kWave;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        rne_vjp_tile<0, MDH, S>(rp, (VjpLinks)links_g, n, stride, tile, q, qd, qdd, gtau, gq, gqd, gqdd, lds, threadIdx.x);
        __syncthreads();
    }
}

#if RTB_HOST_SIDE
namespace {

template <int NJ, class S>
void vjp_launch_nj(bool mdh, dim3 grid, size_t lds, hipStream_t s, const RneVjpParams &rp, const DevLink *links, const S *q, const S *qd, const S *qdd,
                   const S *gtau, S *gq, S *gqd, S *gqdd)
{
    if (mdh) hipLaunchKernelGGL((k_rne_vjp<NJ, true, S>), grid, dim3(kWave), lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd);
    else hipLaunchKernelGGL((k_rne_vjp<NJ, false, S>), grid, dim3(kWave), lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd);
}

template <class S>
int vjp_launch(const Dyn *d, const DevLink *links, const S *q, const S *qd, const S *qdd, int64_t N, const double *grav3, const double *fext6,
               const S *gtau, S *gq, S *gqd, S *gqdd, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (d->n < 1 || d->n > RTBHIP_MAX_JOINTS) { set_error("rne_vjp: n must be 1..RTBHIP_MAX_JOINTS"); return RTBHIP_ELIMIT; }
    RneVjpParams rp;
    rp.n = d->n;
    rp.has_fext = fext6 != nullptr;
    rp.N = N;
    for (int i = 0; i < 3; i++) rp.grav[i] = grav3[i];
    for (int i = 0; i < 6; i++) rp.fext[i] = fext6 ? fext6[i] : 0.0;
    const size_t lds = (size_t)kWave * rne_vjp_stride(d->n) * sizeof(double);
    const int64_t tiles = (N + kWave - 1) / kWave;
    const bool mdh = d->mdh != 0;
    const bool rt = d->n > 8 || tiles > 0x7fffffff;
    int64_t g = tiles;
    if (rt && g > 65536) g = 65536;            // the run-time-n kernel strides over the tiles
    dim3 grid((unsigned)g);
    switch (rt ? 0 : d->n) {
    case 1: vjp_launch_nj<1, S>(mdh, grid, lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 2: vjp_launch_nj<2, S>(mdh, grid, lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 3: vjp_launch_nj<3, S>(mdh, grid, lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 4: vjp_launch_nj<4, S>(mdh, grid, lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 5: vjp_launch_nj<5, S>(mdh, grid, lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 6: vjp_launch_nj<6, S>(mdh, grid, lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 7: vjp_launch_nj<7, S>(mdh, grid, lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    case 8: vjp_launch_nj<8, S>(mdh, grid, lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd); break;
    default:
        if (mdh) hipLaunchKernelGGL((k_rne_vjp_rt<true, S>), grid, dim3(kWave), lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd);
        else hipLaunchKernelGGL((k_rne_vjp_rt<false, S>), grid, dim3(kWave), lds, s, rp, links, q, qd, qdd, gtau, gq, gqd, gqdd);
        break;
    }
    note_launch((int)grid.x, kWave, (int)lds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_rne_vjp launch");
    return RTBHIP_OK;
}

}  // namespace

// (declared in api.cpp, weakly: a library linked without this unit refuses the two entry points instead of failing to load)
int launch_rne_vjp(const Dyn *d, const DevLink *links, const double *q, const double *qd, const double *qdd, int64_t N, const double *grav3,
                   const double *fext6, const double *gtau, double *gq, double *gqd, double *gqdd, hipStream_t s)
{
    return vjp_launch<double>(d, links, q, qd, qdd, N, grav3, fext6, gtau, gq, gqd, gqdd, s);
}
int launch_rne_vjp_f32(const Dyn *d, const DevLink *links, const float *q, const float *qd, const float *qdd, int64_t N, const double *grav3,
                       const double *fext6, const float *gtau, float *gq, float *gqd, float *gqdd, hipStream_t s)
{
    return vjp_launch<float>(d, links, q, qd, qdd, N, grav3, fext6, gtau, gq, gqd, gqdd, s);
}
#endif  // RTB_HOST_SIDE

#endif  // RTB_RNE_VJP_LANE_ONLY

#pragma clang fp contract(fast)
}  // namespace rtbhip
