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

namespace rtbhip {

#pragma clang fp contract(off)      // every operation as written, as rne_vjp_kernels.hip

RTB_HD double ivz(V3 a, V3 b) { return __builtin_fma(a.x, b.y, -(a.y * b.x)); }       // (a x b).z
template <class LinkT>
RTB_HD V3 iv_inertia_t_times(const LinkT &l, V3 v)      // the transpose of inertia_times
{
    return v3(__builtin_fma(l.I[2], v.z, __builtin_fma(l.I[1], v.y, l.I[0] * v.x)), __builtin_fma(l.I[5], v.z, __builtin_fma(l.I[4], v.y, l.I[3] * v.x)),
              __builtin_fma(l.I[8], v.z, __builtin_fma(l.I[7], v.y, l.I[6] * v.x)));
}

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
                    if (MDH) th[j + 1] = ivz(f1, fb1) + ivz(n1, nb1);
                    else th[j + 1] = ivz(rot_fwd<MDH>(R1, f1), fnb) + ivz(rot_fwd<MDH>(R1, n1), nb);
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
                wdb = cross_add(rc, acb, wdb + iv_inertia_t_times(l, Nb));
                const V3 wdp = WD[j > 0 ? j - 1 : 0], ap = A[j > 0 ? j - 1 : 0];
                V3 wdbp, abp;
                double t;
                if (MDH) {
                    const V3 Xb = rot_fwd<MDH>(R, ab);
                    t = -ivz(a, ab);
                    abp = Xb;
                    wdbp = cross(ps, Xb);
                    t = t - ivz(rot_inv<MDH>(R, wdp), wdb);
                    wdbp = wdbp + rot_fwd<MDH>(R, wdb);
                } else {
                    wdb = cross_add(ps, ab, wdb);
                    abp = rot_fwd<MDH>(R, ab);
                    const V3 t3b = rot_fwd<MDH>(R, wdb);
                    t = -(ivz(ap, abp) + ivz(wdp, t3b));
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
constexpr int kIvW = 64;
constexpr int kInertiaVjpMaxJoints = 16;      // the forward kernel's built-in sizes

struct InertiaVjpParams {
    int32_t n, pad_;
    int64_t N;
};

// LDS row of one sample: q (n) | S (n (n + 1) / 2), at an odd stride (conflict-free rows)
inline __host__ __device__ int inertia_vjp_stride(int n) { return (n + n * (n + 1) / 2) | 1; }

// One tile of 64 samples
template <int NJ, bool MDH>
__device__ __forceinline__ void inertia_vjp_tile(const InertiaVjpParams &ip, IvLinks links, int n, int stride, int64_t tile, const double *__restrict__ q,
                                                 const double *__restrict__ gM, double *__restrict__ gq, double *lds, int lane)
{
    const int64_t cfg0 = tile * kIvW;
    const int64_t left = ip.N - cfg0;
    const int ncfg = left < kIvW ? (int)left : kIvW;
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
    if constexpr (NJ > 0) {
        // the NJ + NJ^2 coalesced loads of the tile, UNCONDITIONAL (an element past the ragged tail reads element 0 of the tile; the zeros are selected
        // afterwards: k_rne_vjp tells why), all in flight before the first LDS write
        double rq[NJ], rm[NJ * NJ];
#pragma unroll
        for (int k = 0; k < NJ; ++k) { const int f = lane + kIvW * k; rq[k] = qg[f < count ? f : 0]; }
#pragma unroll
        for (int k = 0; k < NJ * NJ; ++k) { const int f = lane + kIvW * k; rm[k] = mg[f < mcount ? f : 0]; }
        sched_fence();
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int f = lane + kIvW * k;
            lds[(f / NJ) * stride + (f % NJ)] = f < count ? rq[k] : 0.0;
        }
        // the fold: the lower triangle and the diagonal are written, then the upper triangle is added -- each packed slot has exactly one element
        // of either kind, so no two lanes touch a slot within a phase
#pragma unroll
        for (int k = 0; k < NJ * NJ; ++k) {
            const int f = lane + kIvW * k;
            bool lower;
            const int at = slot_of(f, lower);
            if (lower) lds[at] = f < mcount ? rm[k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NJ * NJ; ++k) {
            const int f = lane + kIvW * k;
            bool lower;
            const int at = slot_of(f, lower);
            if (!lower) lds[at] = lds[at] + (f < mcount ? rm[k] : 0.0);
        }
    } else {
        for (int f = lane; f < kIvW * n; f += kIvW) lds[(f / n) * stride + (f % n)] = f < count ? qg[f] : 0.0;
        for (int f = lane; f < kIvW * nn; f += kIvW) {
            bool lower;
            const int at = slot_of(f, lower);
            if (lower) lds[at] = f < mcount ? mg[f] : 0.0;
        }
        __syncthreads();
        for (int f = lane; f < kIvW * nn; f += kIvW) {
            bool lower;
            const int at = slot_of(f, lower);
            if (!lower) lds[at] = lds[at] + (f < mcount ? mg[f] : 0.0);
        }
    }
    __syncthreads();
    if (lane < ncfg) {
        double *mine = lds + lane * stride;
        inertia_vjp_lane<NJ, MDH>(links, n, [&](int j) { return mine[j]; }, [&](int j, int i) { return mine[n + j * (j + 1) / 2 + i]; },
                                  [&](int j, double v) { mine[j] = v; });
    }
    __syncthreads();
    double *out = gq + cfg0 * n;
    if constexpr (NJ > 0) {
        double r[NJ];
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int f = lane + kIvW * k;
            r[k] = lds[(f / NJ) * stride + (f % NJ)];
        }
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int f = lane + kIvW * k;
            if (f < count) __builtin_nontemporal_store(r[k], out + f);
        }
    } else {
        for (int f = lane; f < count; f += kIvW) out[f] = lds[(f / n) * stride + (f % n)];
    }
}

// compile-time joint count: one tile per single-wave workgroup, one wave per SIMD
template <int NJ, bool MDH>
__global__ __launch_bounds__(kIvW, 1) void k_inertia_vjp(InertiaVjpParams ip, const DevLink *links_g, const double *__restrict__ q,
                                                          const double *__restrict__ gM, double *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    inertia_vjp_tile<NJ, MDH>(ip, (IvLinks)links_g, NJ, inertia_vjp_stride(NJ), blockIdx.x, q, gM, gq, lds, threadIdx.x);
}

// run-time joint count (9 .. 16 joints, or more tiles than a grid has blocks): grid-stride over tiles, the tape in private memory
template <bool MDH>
__global__ __launch_bounds__(kIvW) void k_inertia_vjp_rt(InertiaVjpParams ip, const DevLink *links_g, const double *__restrict__ q,
                                                         const double *__restrict__ gM, double *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int n = ip.n;
    const int stride = inertia_vjp_stride(n);
    const int64_t tiles = (ip.N + kIvW - 1) / kIvW;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        inertia_vjp_tile<0, MDH>(ip, (IvLinks)links_g, n, stride, tile, q, gM, gq, lds, threadIdx.x);
        __syncthreads();
    }
}

#if RTB_HOST_SIDE
namespace {

template <class K>
void inertia_vjp_go(K k, dim3 grid, size_t lds, hipStream_t s, const InertiaVjpParams &ip, const DevLink *links, const double *q, const double *gM,
                    double *gq)
{
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, grid, dim3(kIvW), lds, s, ip, links, q, gM, gq);
}

template <int NJ>
void inertia_vjp_go_nj(bool mdh, dim3 grid, size_t lds, hipStream_t s, const InertiaVjpParams &ip, const DevLink *links, const double *q,
                       const double *gM, double *gq)
{
    if (mdh) inertia_vjp_go(k_inertia_vjp<NJ, true>, grid, lds, s, ip, links, q, gM, gq);
    else inertia_vjp_go(k_inertia_vjp<NJ, false>, grid, lds, s, ip, links, q, gM, gq);
}

}  // namespace

// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
int launch_inertia_vjp(const Dyn *d, const DevLink *links, const double *q, int64_t N, const double *gM, double *gq, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (d->n < 1 || d->n > kInertiaVjpMaxJoints) { set_error("inertia_vjp: chains of 1..16 joints"); return RTBHIP_ELIMIT; }
    InertiaVjpParams ip;
    ip.n = d->n; ip.pad_ = 0; ip.N = N;
    const size_t lds = (size_t)kIvW * inertia_vjp_stride(d->n) * sizeof(double);
    const int64_t tiles = (N + kIvW - 1) / kIvW;
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
        if (mdh) inertia_vjp_go(k_inertia_vjp_rt<true>, grid, lds, s, ip, links, q, gM, gq);
        else inertia_vjp_go(k_inertia_vjp_rt<false>, grid, lds, s, ip, links, q, gM, gq);
        break;
    }
    note_launch((int)grid.x, kIvW, (int)lds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_inertia_vjp launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

#endif  // RTB_INERTIA_VJP_LANE_ONLY

#pragma clang fp contract(fast)
}  // namespace rtbhip
