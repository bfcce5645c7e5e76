// frames_vjp_kernels.hip -- gfx950 kernels for the VECTOR-JACOBIAN PRODUCT of the intermediate frames of a chain (rtbhip_link_frames_vjp):
//
//     gq[i, col(k)] += sum_m  G[i, m] : d T_m / d q_k          T_m = B E_1(q) ... E_marks[m],   G: (N, nmarks, 4, 4)
//
// the backward pass of rtbhip_link_frames (frames_kernels.hip, frames_device.h) for every frame at once.  No reference counterpart.
//
// With  GR_m = G_m[:3, :3],  gt_m = G_m[:3, 3]  (the bottom row of T is constant: the bottom row of G is never read) a frame contributes the wrench
//     f_m = gt_m,        n_m = sum_c R_m[:, c] x GR_m[:, c]  +  t_m x gt_m
// and joint k, with axis a_k and origin p_k in the start frame (the z column and the translation of the walk's pose at the joint; a_k negated for a
// flipped joint), collects the wrenches of the frames behind it,  jcount[m] >= k + 1:
//     revolute    gq += a_k . (Nsum_k - p_k x Fsum_k)  =  a_k . Nsum_k - (a_k x p_k) . Fsum_k
//     prismatic   gq += a_k . Fsum_k
// ONE forward walk: the running sums (Fb, Nb) over the frames emitted so far are what lies BEFORE the joint the walk has reached, so
//     Fsum_k = Ftot - Fb_k,   Nsum_k = Ntot - Nb_k
// and a joint keeps seven numbers: A = a_k, B = a_k x p_k  (prismatic: A = 0, B = -a_k) and the scalar  c_k = A . Nb_k - B . Fb_k;  after the walk
//     gq[col(k)] += (A . Ntot - B . Ftot) - c_k.
// Both brackets are the same operation sequence on different sums: a joint with no frame behind it gets exactly 0.  Nothing of size
// nmarks x n exists; the frames  T_m = P_j F_m  are recomputed by the walk (frames_device.h: the same pose arithmetic as the forward kernel).
// Every sum of two products is written out (mix_pp / mix_pm / dot3x, fp contract(off)): the result does not depend on what the compiler fuses.
//
// One lane = one configuration, 64-lane tiles, one tile per single-wave workgroup.  The kernel is bound by reading G: 128 nmarks bytes per
// configuration.  G arrives kFvChunk frames at a time: eight adjacent lanes load one 128-byte frame line, eight configurations per instruction
// (the store pattern of k_frames, reversed), into registers; the registers go to a lane-major LDS tile (odd row stride) that each lane reads
// back for its own configuration, and the next chunk's loads are issued before the walk consumes the current one.  q is loaded coalesced into a second
// lane-major tile; gq overwrites it (zeroed by the lane once the walk has read its last q) and leaves coalesced.
#include "frames_device.h"

namespace rtbhip {

#pragma clang fp contract(off)

// A . N - B . F
RTB_HD double fv_moment(double ax, double ay, double az, double bx, double by, double bz, double Nx, double Ny, double Nz, double Fx, double Fy, double Fz)
{
#pragma clang fp contract(off)
    return dot3x(ax, Nx, ay, Ny, az, Nz) - dot3x(bx, Fx, by, Fy, bz, Fz);
}

// One configuration.  cv: the wave-uniform chain view (seg, jmeta); NJ = 0: run-time n, the per-joint state in private memory.
//   qcol(c)      -> column c of this configuration's q (all reads happen during the walk)
//   need(m)      -> called once per frame, in frame order, before g(m, ..) is read: the kernel swaps G's chunks here (wave-uniform)
//   g(m, r, c)   -> G[m][r][c], r = 0..2 (the bottom row is never asked for)
//   clear()      -> called once after the walk: zero the gq row (it may be the q row)
//   add(col, v)  -> gq[col] += v, in joint order
template <int NJ, class CV, class QCol, class Need, class GIn, class Clear, class Add>
RTB_HD void frames_vjp_lane(const CV &cv, int n_rt, const FrameTable &ft, QCol qcol, Need need, GIn g, Clear clear, Add add)
{
#pragma clang fp contract(off)
    constexpr int CAP = NJ > 0 ? NJ : RTBHIP_MAX_JOINTS;
    const int n = NJ > 0 ? NJ : n_rt;
    double Ax[CAP], Ay[CAP], Az[CAP], Bx[CAP], By[CAP], Bz[CAP], Cc[CAP];
    Pose P;
    pose_identity(P);
    if (ft.has_base) {
        P.r00 = ft.base[0]; P.r01 = ft.base[1]; P.r02 = ft.base[2]; P.tx = ft.base[3];
        P.r10 = ft.base[4]; P.r11 = ft.base[5]; P.r12 = ft.base[6]; P.ty = ft.base[7];
        P.r20 = ft.base[8]; P.r21 = ft.base[9]; P.r22 = ft.base[10]; P.tz = ft.base[11];
    }
    double Fx = 0.0, Fy = 0.0, Fz = 0.0, Nx = 0.0, Ny = 0.0, Nz = 0.0;      // the wrenches of the frames emitted so far
    int m = 0;
    auto drain = [&](int jc) {
        while (m < ft.nmarks && ft.jcount[m] == jc) {
            Pose Q = P;
            if (!ft.ident[m]) pose_mul_general(Q, [&](int k) { return ft.F[m][k]; });
            need(m);
            const double g00 = g(m, 0, 0), g01 = g(m, 0, 1), g02 = g(m, 0, 2), gx = g(m, 0, 3);
            const double g10 = g(m, 1, 0), g11 = g(m, 1, 1), g12 = g(m, 1, 2), gy = g(m, 1, 3);
            const double g20 = g(m, 2, 0), g21 = g(m, 2, 1), g22 = g(m, 2, 2), gz = g(m, 2, 3);
            Fx = Fx + gx; Fy = Fy + gy; Fz = Fz + gz;
            // n = R[:, 0] x GR[:, 0] + R[:, 1] x GR[:, 1] + R[:, 2] x GR[:, 2] + t x gt, summed in that order
            const double nx = ((mix_pm(Q.r10, g20, Q.r20, g10) + mix_pm(Q.r11, g21, Q.r21, g11)) + mix_pm(Q.r12, g22, Q.r22, g12)) + mix_pm(Q.ty, gz, Q.tz, gy);
            const double ny = ((mix_pm(Q.r20, g00, Q.r00, g20) + mix_pm(Q.r21, g01, Q.r01, g21)) + mix_pm(Q.r22, g02, Q.r02, g22)) + mix_pm(Q.tz, gx, Q.tx, gz);
            const double nz = ((mix_pm(Q.r00, g10, Q.r10, g00) + mix_pm(Q.r01, g11, Q.r11, g01)) + mix_pm(Q.r02, g12, Q.r12, g02)) + mix_pm(Q.tx, gy, Q.ty, gx);
            Nx = Nx + nx; Ny = Ny + ny; Nz = Nz + nz;
            ++m;
            if (NJ > 0) sched_fence();
        }
    };
    drain(0);
#pragma unroll
    for (int j = 0; j < n; ++j) {
        pose_mul_seg(P, cv, j);
        const int jm = cv.jmeta[j];
        double eta = qcol(jm_jq(jm));
        double ax = P.r02, ay = P.r12, az = P.r22;
        if (jm_flip(jm)) { eta = -eta; ax = -ax; ay = -ay; az = -az; }
        const bool pris = jm_prismatic(jm);
        if (pris) {
            Ax[j] = 0.0; Ay[j] = 0.0; Az[j] = 0.0;
            Bx[j] = -ax; By[j] = -ay; Bz[j] = -az;
        } else {
            Ax[j] = ax; Ay[j] = ay; Az[j] = az;
            Bx[j] = mix_pm(ay, P.tz, az, P.ty); By[j] = mix_pm(az, P.tx, ax, P.tz); Bz[j] = mix_pm(ax, P.ty, ay, P.tx);      // a x p
        }
        Cc[j] = fv_moment(Ax[j], Ay[j], Az[j], Bx[j], By[j], Bz[j], Nx, Ny, Nz, Fx, Fy, Fz);      // what lies before the joint
        if (NJ > 0) sched_fence();
        if (pris) {
            pose_tz(P, eta);
        } else {
            double s, c;
            rtb_sincos(eta, &s, &c);
            pose_rotz(P, c, s);
        }
        drain(j + 1);
        if (NJ > 0) sched_fence();
    }
    clear();
#pragma unroll
    for (int j = 0; j < n; ++j)
        add(jm_jq(cv.jmeta[j]), fv_moment(Ax[j], Ay[j], Az[j], Bx[j], By[j], Bz[j], Nx, Ny, Nz, Fx, Fy, Fz) - Cc[j]);
}

#ifndef RTB_FRAMES_VJP_LANE_ONLY      // (a host-side replay of the lane body includes this file for frames_vjp_lane alone)

#define RTB_CONST __attribute__((address_space(4)))
struct ConstChainFv {
    const RTB_CONST DevSeg *seg;
    const RTB_CONST int32_t *jmeta;
};

constexpr int kFvW = 64;
constexpr int kFvChunk = 2;                          // frames of G resident in LDS at a time (and as many in flight in registers)
constexpr int kFvGStride = kFvChunk * 16 + 1;        // doubles per lane row of the G tile: odd, conflict-free
constexpr size_t kFvLdsMax = 160 * 1024;             // one CU's LDS
typedef double v2d __attribute__((ext_vector_type(2)));

inline __host__ __device__ int frames_vjp_qstride(int qw) { return qw | 1; }
inline __host__ __device__ size_t frames_vjp_lds(int qw) { return (size_t)kFvW * (kFvGStride + frames_vjp_qstride(qw)) * sizeof(double); }

struct FramesVjpParams {
    int32_t n, qw;
    int64_t N;
};

// One tile of 64 configurations.  lds: the G tile (kFvW x kFvGStride), then the q / gq tile (kFvW x qstride).
template <int NJ>
__device__ __forceinline__ void frames_vjp_tile(const FrameTable &ft, const ConstChainFv &cv, const FramesVjpParams &fp, int64_t tile,
                                                const double *__restrict__ q, const double *__restrict__ gF, double *__restrict__ gq, double *lds, int lane)
{
    const int qw = fp.qw, qs = frames_vjp_qstride(qw), nmarks = ft.nmarks;
    const int64_t cfg0 = tile * kFvW;
    const int64_t left = fp.N - cfg0;
    const int ncfg = left < kFvW ? (int)left : kFvW;
    const int count = ncfg * qw;
    double *gt = lds, *qt = lds + kFvW * kFvGStride;
    const int piece = lane & 7, sub = lane >> 3;

    // the chunk of frames m0 .. m0 + kFvChunk - 1 of the tile's 64 configurations: eight lanes per 128-byte frame line.  The loads are
    // unconditional (a configuration or frame past the end reads the tile's first frame, which exists) and the zeros are selected afterwards
    v2d pre[kFvChunk * 8];
    auto fetch = [&](int m0) {
#pragma unroll
        for (int f = 0; f < kFvChunk; ++f) {
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int c = it * 8 + sub, mm = m0 + f;
                const bool ok = c < ncfg && mm < nmarks;
                const double *src = gF + ((cfg0 + (ok ? c : 0)) * nmarks + (ok ? mm : 0)) * 16 + 2 * piece;
                const v2d v = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(src));
                const v2d z = {0.0, 0.0};
                pre[f * 8 + it] = ok ? v : z;
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int f = 0; f < kFvChunk; ++f) {
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                double *dst = gt + (it * 8 + sub) * kFvGStride + f * 16 + 2 * piece;
                dst[0] = pre[f * 8 + it].x;
                dst[1] = pre[f * 8 + it].y;
            }
        }
    };
    fetch(0);
    // q: the tile's rows are one contiguous run of ncfg * qw doubles; (row, column) advance by the wave's stride with a carry
    {
        const int dR = kFvW / qw, dE = kFvW % qw;
        int r = lane / qw, e = lane - r * qw;
        for (int f = lane; f < kFvW * qw; f += kFvW) {
            qt[r * qs + e] = f < count ? q[cfg0 * qw + f] : 0.0;
            e += dE; r += dR;
            if (e >= qw) { e -= qw; ++r; }
        }
    }
    commit();
    __syncthreads();
    if (kFvChunk < nmarks) fetch(kFvChunk);

    double *mine_q = qt + lane * qs;
    const double *mine_g = gt + lane * kFvGStride;
    // every lane walks (the walk and its chunk swaps are wave-uniform); a lane past the ragged tail works on zeros
    frames_vjp_lane<NJ>(cv, fp.n, ft, [&](int c) { return mine_q[c]; },
        [&](int m) {
            if (m > 0 && m % kFvChunk == 0) {
                __syncthreads();                                   // every lane has read the previous chunk
                commit();
                __syncthreads();
                if (m + kFvChunk < nmarks) fetch(m + kFvChunk);
            }
        },
        [&](int m, int r, int c) { return mine_g[(m % kFvChunk) * 16 + r * 4 + c]; },
        [&]() { for (int c = 0; c < qw; ++c) mine_q[c] = 0.0; },
        [&](int col, double v) { mine_q[col] = mine_q[col] + v; });
    __syncthreads();
    {
        const int dR = kFvW / qw, dE = kFvW % qw;
        int r = lane / qw, e = lane - r * qw;
        for (int f = lane; f < count; f += kFvW) {
            __builtin_nontemporal_store(qt[r * qs + e], gq + cfg0 * qw + f);
            e += dE; r += dR;
            if (e >= qw) { e -= qw; ++r; }
        }
    }
}

// compile-time joint count: one tile per single-wave workgroup, the per-joint state in registers
template <int NJ>
__global__ __launch_bounds__(kFvW, 1) void k_frames_vjp(FrameTable ft, DevChain dc, FramesVjpParams fp, const double *__restrict__ q,
                                                        const double *__restrict__ gF, double *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    ConstChainFv cv;
    cv.seg = (const RTB_CONST DevSeg *)dc.seg;
    cv.jmeta = (const RTB_CONST int32_t *)dc.jmeta;
    frames_vjp_tile<NJ>(ft, cv, fp, blockIdx.x, q, gF, gq, lds, threadIdx.x);
}

// run-time joint count (9 .. RTBHIP_MAX_JOINTS joints, or more tiles than a grid has blocks): grid-stride over the tiles, the per-joint state in private memory
__global__ __launch_bounds__(kFvW) void k_frames_vjp_rt(FrameTable ft, DevChain dc, FramesVjpParams fp, const double *__restrict__ q,
                                                        const double *__restrict__ gF, double *__restrict__ gq)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    ConstChainFv cv;
    cv.seg = (const RTB_CONST DevSeg *)dc.seg;
    cv.jmeta = (const RTB_CONST int32_t *)dc.jmeta;
    const int64_t tiles = (fp.N + kFvW - 1) / kFvW;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        frames_vjp_tile<0>(ft, cv, fp, tile, q, gF, gq, lds, threadIdx.x);
        __syncthreads();
    }
}

#if RTB_HOST_SIDE
namespace {
template <int NJ>
hipError_t fv_launch_nj(dim3 grid, size_t lds, hipStream_t s, const FrameTable &ft, const DevChain &dc, const FramesVjpParams &fp, const double *q,
                        const double *gF, double *gq)
{
    if (lds > 48 * 1024) {       // beyond the default dynamic allocation: the kernel has to be told
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_frames_vjp<NJ>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_frames_vjp<NJ>), grid, dim3(kFvW), lds, s, ft, dc, fp, q, gF, gq);
    return hipSuccess;
}
}  // namespace

// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
// q: (N, q_width), gF: (N, ft.nmarks, 4, 4), gq: (N, q_width), all on the device; ft.nmarks >= 1
int launch_frames_vjp(const Chain *c, const DevChain &dc, const FrameTable &ft, const double *q, int64_t N, const double *gF, double *gq, hipStream_t s)
{
    if (N == 0) return RTBHIP_OK;
    if (c->n < 1 || c->n > RTBHIP_MAX_JOINTS) { set_error("link_frames_vjp: chains of 1..RTBHIP_MAX_JOINTS joints"); return RTBHIP_ELIMIT; }
    if (ft.nmarks < 1 || ft.nmarks > kMaxFrames || c->q_width < 1) { set_error("link_frames_vjp: nothing to differentiate"); return RTBHIP_EINVAL; }
    const size_t lds = frames_vjp_lds(c->q_width);
    if (lds > kFvLdsMax) { set_error("link_frames_vjp: q rows too wide for the compute unit's LDS"); return RTBHIP_ELIMIT; }
    FramesVjpParams fp;
    fp.n = c->n;
    fp.qw = c->q_width;
    fp.N = N;
    const int64_t tiles = (N + kFvW - 1) / kFvW;
    const bool rt = c->n > 8 || tiles > 0x7fffffff;
    int64_t g = tiles;
    if (rt && g > 65536) g = 65536;            // the run-time-n kernel strides over the tiles
    dim3 grid((unsigned)g);
    hipError_t e = hipSuccess;
    switch (rt ? 0 : c->n) {
    case 1: e = fv_launch_nj<1>(grid, lds, s, ft, dc, fp, q, gF, gq); break;
    case 2: e = fv_launch_nj<2>(grid, lds, s, ft, dc, fp, q, gF, gq); break;
    case 3: e = fv_launch_nj<3>(grid, lds, s, ft, dc, fp, q, gF, gq); break;
    case 4: e = fv_launch_nj<4>(grid, lds, s, ft, dc, fp, q, gF, gq); break;
    case 5: e = fv_launch_nj<5>(grid, lds, s, ft, dc, fp, q, gF, gq); break;
    case 6: e = fv_launch_nj<6>(grid, lds, s, ft, dc, fp, q, gF, gq); break;
    case 7: e = fv_launch_nj<7>(grid, lds, s, ft, dc, fp, q, gF, gq); break;
    case 8: e = fv_launch_nj<8>(grid, lds, s, ft, dc, fp, q, gF, gq); break;
    default:
        if (lds > 48 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_frames_vjp_rt), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) hipLaunchKernelGGL(k_frames_vjp_rt, grid, dim3(kFvW), lds, s, ft, dc, fp, q, gF, gq);
        break;
    }
    if (e != hipSuccess) return hip_fail(e, "k_frames_vjp: hipFuncSetAttribute");
    note_launch((int)grid.x, kFvW, (int)lds);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_frames_vjp launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

#endif  // RTB_FRAMES_VJP_LANE_ONLY

#pragma clang fp contract(fast)
}  // namespace rtbhip
