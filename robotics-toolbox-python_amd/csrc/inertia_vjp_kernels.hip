// inertia_vjp_kernels.hip -- gfx950 kernels for the VECTOR-JACOBIAN PRODUCT of the batched joint-space inertia matrix of a DH arm (rtbhip_inertia_vjp):
//
//     gq[r,k] = sum_ij gM[r,i,j] d M[r,i,j] / d q[r,k]
//
// for chains whose links are all revolute.  The forward kernel (dyn_device.h: dyn_lane) builds M from n unit-acceleration passes of the
// Newton-Euler recursion at rest -- pass i = rne(q, 0, e_i) without gravity -- keeps the torques j >= i of pass i (the links before i do not move)
// and mirrors them: the computed value P(j, i), j >= i, is both M[j,i] and M[i,j].  Its adjoint therefore takes gM FOLDED onto the triangle,
//     S(j, i) = gM[j,i] + gM[i,j]  (j > i),    S(i, i) = gM[i,i]
// and is the sum over i of the adjoint of pass i seeded with gtau_j = S(j, i) on the links j >= i.  The motor inertia G^2 Jm on the diagonal is a
// constant of q.
//
// The lane body is the SPECIALISED form of rne_vjp_lane (rne_vjp_kernels.hip, whose header has the formulas): with qd = 0 every angular velocity
// is an exact zero, so w, its adjoint and every product of two velocities are left out (the terms left out are exact zeros there, x + 0 == x);
// the tape is wd, a, f, n = 12 doubles per link; pass i starts at link i (the links before it are at rest, their torques are no outputs), and
// M[j,i] (j >= i) depends on q_{i+1} .. q_j only: pass i emits gq_k for k > i, so the last pass is not run at all.
// One lane = one sample; sin / cos once per lane, then a `#pragma unroll 1` loop over the passes, each kept self-contained by dyn_opaque
// (dyn_device.h tells why); gq accumulates in n registers.
// I/O: the wave's (64 x n) block of q and (64 x n x n) block of gM are contiguous in memory, loaded coalesced -- all loads in flight before the
// first LDS write -- into a lane-major LDS tile of  q (n) | S (n (n + 1) / 2, packed: (j, i) at j (j + 1) / 2 + i)  doubles per row at an odd
// stride: 45 doubles per row for n = 8, 22.5 KB per wave.  gq overwrites the q slots and leaves as contiguous non-temporal stores.
#include "dyn_device.h"
#include "vjp_tile.h"

namespace rtbhip {

#pragma clang fp contract(off)      // every operation as written, as rne_vjp_kernels.hip

// One sample.  links: the wave-uniform link table, every link revolute.  qin(j): the joint angles, read up front.  sym(j, i), j >= i: the folded
// gradient S(j, i).  gq(j, v): called once per joint, after the last pass.  NJ = 0: run-time n, the per-link arrays in private memory.
template <int NJ, bool MDH, class LinksP, class InQ, class InS, class OutQ>
RTB_HD void inertia_vjp_lane(LinksP links, int n_rt, InQ qin, InS sym, OutQ gq)
{
#pragma clang fp contract(off)
    constexpr int CAP = NJ > 0 ? NJ : RTBHIP_MAX_JOINTS;
    const int n = NJ > 0 ? NJ : n_rt;
    double st[CAP], ct[CAP], th[CAP], acc[CAP];
    V3 WD[CAP], A[CAP], Fq[CAP], Nq[CAP];
    if constexpr (NJ > 0) {
        rne_trig<NJ, true>(links, qin, st, ct);
    } else {
        for (int j = 0; j < n; ++j) rtb_sincos(qin(j) + links[j].offset, &st[j], &ct[j]);
    }
#pragma unroll
    for (int j = 0; j < n; ++j) acc[j] = 0.0;

#pragma unroll 1
    for (int i = 0; i + 1 < n; ++i) {
        if constexpr (NJ > 0) dyn_opaque<NJ>(st, ct);
        // ---- 1. primal forward recursion from link i: wd, a (the tape), F = m (a + wd x r), N = I wd
        {
            V3 wd = v3(0, 0, 0), a = v3(0, 0, 0);
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (j < i) continue;
                const auto &l = links[j];
                const Rot R = {st[j], ct[j], l.sa, l.ca, 0};
                const V3 ps = link_offset<MDH>(l, l.d), rc = v3(l.rx, l.ry, l.rz);
                const double qddj = j == i ? 1.0 : 0.0;
                V3 wdn, an;
                if (MDH) {
                    wdn = addz(rot_inv<MDH>(R, wd), qddj);
                    an = rot_inv<MDH>(R, cross_add(wd, ps, a));
                } else {
                    wdn = rot_inv<MDH>(R, addz(wd, qddj));
                    an = cross_add(wdn, ps, rot_inv<MDH>(R, a));
                }
                wd = wdn; a = an;
                WD[j] = wd; A[j] = a;
                Fq[j] = l.m * cross_add(wd, rc, a);
                Nq[j] = inertia_times(l, wd);
                if (NJ > 0) sched_fence();
            }
        }

        // ---- 2. primal backward recursion: (F_j, N_j) -> (f_j, n_j) in place, for the links j > i (sweep 3 reads f and n of link j + 1 only)
        vjp_dh_sweep2<NJ, MDH>(links, n, st, ct, Fq, Nq, v3(0, 0, 0), v3(0, 0, 0), i + 1);

        // ---- 3. adjoint of the backward recursion, link i -> tip: (f_j, n_j) -> the adjoints of (F_j, N_j) in place
        {
            V3 fb = v3(0, 0, 0), nb = v3(0, 0, 0);
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (j < i) continue;
                const auto &l = links[j];
                const double g = sym(j, i);
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

        // ---- 4. adjoint of the forward recursion, tip -> link i + 1 (M[j,i] does not depend on q_i)
        {
            V3 wdb = v3(0, 0, 0), ab = v3(0, 0, 0);
#pragma unroll
            for (int jj = 0; jj < n; ++jj) {
                const int j = n - 1 - jj;
                if (j <= i) continue;
                const auto &l = links[j];
                const Rot R = {st[j], ct[j], l.sa, l.ca, 0};
                const V3 ps = link_offset<MDH>(l, l.d), rc = v3(l.rx, l.ry, l.rz);
                const V3 a = A[j], Fb = Fq[j], Nb = Nq[j];
                const V3 acb = l.m * Fb;
                ab = ab + acb;
                wdb = cross_add(rc, acb, wdb + vjp_inertia_t_times(l, Nb));
                const V3 wdp = WD[j > 0 ? j - 1 : 0], ap = A[j > 0 ? j - 1 : 0];
                V3 wdbp, abp;
                double t;
                if (MDH) {
                    const V3 Xb = rot_fwd<MDH>(R, ab);
                    t = -vjp_zcross(a, ab);
                    abp = Xb;
                    wdbp = cross(ps, Xb);
                    t = t - vjp_zcross(rot_inv<MDH>(R, wdp), wdb);
                    wdbp = wdbp + rot_fwd<MDH>(R, wdb);
                } else {
                    wdb = cross_add(ps, ab, wdb);
                    abp = rot_fwd<MDH>(R, ab);
                    const V3 t3b = rot_fwd<MDH>(R, wdb);
                    t = -(vjp_zcross(ap, abp) + vjp_zcross(wdp, t3b));
                    wdbp = t3b;
                }
                acc[j] = acc[j] + (th[j] + t);
                wdb = wdbp; ab = abp;
                if (NJ > 0) sched_fence();
            }
        }
    }
#pragma unroll
    for (int j = 0; j < n; ++j) gq(j, acc[j]);
}

#ifndef RTB_INERTIA_VJP_LANE_ONLY      // (a host-side replay of the lane body includes this file for inertia_vjp_lane alone)

typedef const __attribute__((address_space(4))) DevLink *IvLinks;
constexpr int kInertiaVjpMaxJoints = 16;      // the forward kernel's built-in sizes

struct InertiaVjpParams {
    int32_t n, pad_;
    int64_t N;
};

// LDS row of one sample: q (n) | S (n (n + 1) / 2), at an odd stride (conflict-free rows)
inline __host__ __device__ int inertia_vjp_stride(int n) { return (n + n * (n + 1) / 2) | 1; }

// One tile of 64 samples (the staging, the fold and the flush are vjp_tile.h's phases)
template <int NJ, bool MDH>
__device__ __forceinline__ void inertia_vjp_tile(const InertiaVjpParams &ip, IvLinks links, int n, int stride, int64_t tile, const double *__restrict__ q,
                                                 const double *__restrict__ gM, double *__restrict__ gq, double *lds, int lane)
{
    const VjpTile t = vjp_tile_of(tile, ip.N, n);
    const double *const qg[1] = {q + t.cfg0 * n};
    const double *mg = gM + t.cfg0 * n * n;
    VjpCols<NJ, 1, double> cols;
    VjpMat<NJ> mat;
    vjp_load_cols<NJ, false>(qg, t, lane, cols);
    vjp_load_mat<NJ>(mg, t, lane, mat);
    sched_fence();
    vjp_stage_cols<NJ, false>(qg, t, n, stride, lane, cols, lds);
    vjp_fold<NJ, false>(mg, t, n, stride, n, lane, mat, lds);
    __syncthreads();
    vjp_fold<NJ, true>(mg, t, n, stride, n, lane, mat, lds);
    __syncthreads();
    if (lane < t.ncfg) {
        double *mine = lds + lane * stride;
        inertia_vjp_lane<NJ, MDH>(links, n, [&](int j) { return mine[j]; }, [&](int j, int i) { return mine[n + j * (j + 1) / 2 + i]; },
                                  [&](int j, double v) { mine[j] = v; });
    }
    __syncthreads();
    double *const out[1] = {gq + t.cfg0 * n};
    vjp_tile_flush<NJ, false>(out, t, n, stride, lane, lds);
}

// compile-time joint count: one tile per single-wave workgroup, one wave per SIMD
template <int NJ, bool MDH>
__global__ __launch_bounds__(kWave, 1) void k_inertia_vjp(InertiaVjpParams ip, const DevLink *links_g, const double *__restrict__ q,
                                                          const double *__restrict__ gM, double *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    inertia_vjp_tile<NJ, MDH>(ip, (IvLinks)links_g, NJ, inertia_vjp_stride(NJ), blockIdx.x, q, gM, gq, lds, threadIdx.x);
}

// run-time joint count (9 .. 16 joints, or more tiles than a grid has blocks): grid-stride over tiles, the tape in private memory
template <bool MDH>
__global__ __launch_bounds__(kWave) void k_inertia_vjp_rt(InertiaVjpParams ip, const DevLink *links_g, const double *__restrict__ q,
                                                         const double *__restrict__ gM, double *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int n = ip.n;
    const int stride = inertia_vjp_stride(n);
    const int64_t tiles = (ip.N + kWave - 1) / kWave;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        inertia_vjp_tile<0, MDH>(ip, (IvLinks)links_g, n, stride, tile, q, gM, gq, lds, threadIdx.x);
        __syncthreads();
    }
}

#if RTB_HOST_SIDE
namespace {

template <int NJ>
void inertia_vjp_go_nj(bool mdh, dim3 grid, size_t lds, hipStream_t s, const InertiaVjpParams &ip, const DevLink *links, const double *q,
                       const double *gM, double *gq)
{
    if (mdh) vjp_go(k_inertia_vjp<NJ, true>, grid, lds, s, ip, links, q, gM, gq);
    else vjp_go(k_inertia_vjp<NJ, false>, grid, lds, s, ip, links, q, gM, gq);
}

}  // namespace

// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
int launch_inertia_vjp(const Dyn *d, const DevLink *links, const double *q, int64_t N, const double *gM, double *gq, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (d->n < 1 || d->n > kInertiaVjpMaxJoints) { set_error("inertia_vjp: chains of 1..16 joints"); return RTBHIP_ELIMIT; }
    InertiaVjpParams ip;
    ip.n = d->n; ip.pad_ = 0; ip.N = N;
    const size_t lds = (size_t)kWave * inertia_vjp_stride(d->n) * sizeof(double);
    const int64_t tiles = (N + kWave - 1) / kWave;
    const bool mdh = d->mdh != 0;
    const bool rt = d->n > 8 || tiles > 0x7fffffff;
    dim3 grid((unsigned)(rt && tiles > 65536 ? 65536 : tiles));      // the run-time-n kernel strides over the tiles
    switch (rt ? 0 : d->n) {
    case 1: inertia_vjp_go_nj<1>(mdh, grid, lds, s, ip, links, q, gM, gq); break;
    case 2: inertia_vjp_go_nj<2>(mdh, grid, lds, s, ip, links, q, gM, gq); break;
    case 3: inertia_vjp_go_nj<3>(mdh, grid, lds, s, ip, links, q, gM, gq); break;
    case 4: inertia_vjp_go_nj<4>(mdh, grid, lds, s, ip, links, q, gM, gq); break;
    case 5: inertia_vjp_go_nj<5>(mdh, grid, lds, s, ip, links, q, gM, gq); break;
    case 6: inertia_vjp_go_nj<6>(mdh, grid, lds, s, ip, links, q, gM, gq); break;
    case 7: inertia_vjp_go_nj<7>(mdh, grid, lds, s, ip, links, q, gM, gq); break;
    case 8: inertia_vjp_go_nj<8>(mdh, grid, lds, s, ip, links, q, gM, gq); break;
    default:
        if (mdh) vjp_go(k_inertia_vjp_rt<true>, grid, lds, s, ip, links, q, gM, gq);
        else vjp_go(k_inertia_vjp_rt<false>, grid, lds, s, ip, links, q, gM, gq);
        break;
    }
    note_launch((int)grid.x, kWave, (int)lds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_inertia_vjp launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

#endif  // RTB_INERTIA_VJP_LANE_ONLY

#pragma clang fp contract(fast)
}  // namespace rtbhip
