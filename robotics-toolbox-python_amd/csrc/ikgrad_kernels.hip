// ikgrad_kernels.hip -- gfx950 kernels for the IMPLICIT-FUNCTION ADJOINT of the inverse kinematics (rtbhip_ik_vjp): the backward pass of
// q = ik_LM / ik_GN / ik_NR (Tep) in one launch.  ikgrad_device.h has the derivation, the lane body and the tile phases.
//
//   k_ik_vjp<NJ>   1..kKinRegMax joints.  One lane = one row, 64-lane tiles, one tile per single-wave workgroup (the launch shape of k_kin_reg /
//                  k_kin_vjp).  q, gq and Tep arrive coalesced in a lane-major LDS tile of odd stride; the lane walks the chain in registers
//                  (reg_core: the finished Jacobian never leaves them), forms J_a gq and the lower triangle of J_a J_a^T + d^2 I, solves, and writes
//                  gTep and the twist over its inputs; they leave the way the inputs came.  8 (7 + 7 + 16 + 16) + 4 = 372 bytes per Panda row.
//   k_ik_vjp_any   11..RTBHIP_MAX_JOINTS joints: jacob0 is written into stream-ordered scratch by the forward launch, and a round of rows passes
//                  through LDS as [J | gq | Tep] (launch_kin_vjp_s does the same for the kinematic adjoint).
#include <hip/hip_runtime.h>
#include "rtbhip_internal.h"
#include "diff_kernel.h"
#include "ikgrad_device.h"
#include <algorithm>

namespace rtbhip {

// Two waves per SIMD: 6 NJ Jacobian registers, the 21 of the triangle and the solve's own fit 256 VGPRs up to 10 joints without scratch
// (tests/test_code_object_notes_ik_vjp.py reads the code object's notes).
template <int NJ>
__global__ __launch_bounds__(kWave, 2) void k_ik_vjp(IkVjpParams ip, DevChain dc, const double *__restrict__ q, const double *__restrict__ Tep,
                                                     const int32_t *__restrict__ success, const double *__restrict__ gq, double *__restrict__ gTep,
                                                     double *__restrict__ gtwist)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const ConstChain cv = const_view(dc);
    const int lane = threadIdx.x;
    const int64_t tile = xcd_tile();
    const VjpTile t = vjp_tile_of(tile, ip.N, NJ);
    const int ok = success ? (lane < t.ncfg ? success[t.cfg0 + lane] : 0) : 1;      // read once per lane
    ik_vjp_tile_fill<NJ>(ip, q, gq, Tep, tile, lane, lds);
    __syncthreads();
    // every lane walks (the walk is wave-uniform); a lane past the ragged tail works on zeros and on whatever its Tep slots hold: never flushed
    ik_vjp_lane<NJ>(ip, cv, ok, gTep != nullptr, gtwist != nullptr, lds + lane * ik_vjp_stride(NJ));
    __syncthreads();
    ik_vjp_tile_flush(ik_vjp_head(NJ), ik_vjp_stride(NJ), t.ncfg, lds, gTep ? gTep + t.cfg0 * 16 : nullptr, gtwist ? gtwist + t.cfg0 * 6 : nullptr, lane);
}

__global__ __launch_bounds__(kWave) void k_ik_vjp_any(IkVjpParams ip, const double *__restrict__ J, const double *__restrict__ Tep,
                                                      const int32_t *__restrict__ success, const double *__restrict__ gq, double *__restrict__ gTep,
                                                      double *__restrict__ gtwist)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, n = ip.n, stride = ik_vjp_any_stride(n);
    const int64_t cfg0 = (int64_t)blockIdx.x * kWave;
    const int64_t left = ip.N - cfg0;
    const int ncfg = left < kWave ? (int)left : kWave;
    for (int r0 = 0; r0 < ncfg; r0 += ip.per) {              // wave-uniform
        const int cnt = ncfg - r0 < ip.per ? ncfg - r0 : ip.per;
        const int64_t row0 = cfg0 + r0;
        ik_vjp_any_fill(n, J, gq, Tep, row0, cnt, lane, lds);
        __syncthreads();
        if (lane < cnt) ik_vjp_any_lane(ip, success ? success[row0 + lane] : 1, gTep != nullptr, gtwist != nullptr, lds + lane * stride);
        __syncthreads();
        ik_vjp_tile_flush(7 * n, stride, cnt, lds, gTep ? gTep + row0 * 16 : nullptr, gtwist ? gtwist + row0 * 6 : nullptr, lane);
        __syncthreads();
    }
}

#if RTB_HOST_SIDE
namespace {
template <int NJ>
hipError_t ik_vjp_go(dim3 grid, hipStream_t s, const IkVjpParams &ip, const DevChain &dc, const double *q, const double *Tep, const int32_t *success,
                     const double *gq, double *gTep, double *gtwist)
{
    const size_t lds = (size_t)kWave * ik_vjp_stride(NJ) * sizeof(double);      // at most 64 x 37 doubles: under the default 48 KB
    hipLaunchKernelGGL((k_ik_vjp<NJ>), grid, dim3(kWave), lds, s, ip, dc, q, Tep, success, gq, gTep, gtwist);
    note_launch((int)grid.x, kWave, (int)lds);
    return hipGetLastError();
}
}  // namespace

// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
// q, gq: (N, n); Tep: (N, 4, 4); success: (N) or NULL; gTep: (N, 4, 4) or NULL; gtwist: (N, 6) or NULL -- all on the device.  rows: the used-row
// set (at most n bits: the caller checked); d2: damping squared.
int launch_ik_vjp(const Chain *c, const DevChain &dc, const double *q, int64_t N, const double *Tep, const int32_t *success, int rows, double d2,
                  const double *gq, double *gTep, double *gtwist, hipStream_t s)
{
    if (N == 0 || (!gTep && !gtwist)) return RTBHIP_OK;
    if (c->n < 1 || c->n > RTBHIP_MAX_JOINTS) { set_error("ik_vjp: chains of 1..RTBHIP_MAX_JOINTS joints"); return RTBHIP_ELIMIT; }
    const int64_t tiles = (N + kWave - 1) / kWave;
    if (tiles > 0x7fffffff) { set_error("ik_vjp: batch too large for one launch"); return RTBHIP_ELIMIT; }
    IkVjpParams ip;
    ip.n = c->n; ip.rows = rows; ip.per = kWave; ip.pad = 0; ip.N = N; ip.d2 = d2;
    Affine notool;
    notool.used = 0;
    for (int i = 0; i < 12; i++) notool.v[i] = (i % 5 == 0) ? 1.0 : 0.0;
    chain_tail(c, notool, ip.tail);
    const dim3 grid((unsigned)tiles);
    if (c->n <= kKinRegMax) {
        hipError_t e = hipSuccess;
        switch (c->n) {
        case 1: e = ik_vjp_go<1>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        case 2: e = ik_vjp_go<2>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        case 3: e = ik_vjp_go<3>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        case 4: e = ik_vjp_go<4>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        case 5: e = ik_vjp_go<5>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        case 6: e = ik_vjp_go<6>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        case 7: e = ik_vjp_go<7>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        case 8: e = ik_vjp_go<8>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        case 9: e = ik_vjp_go<9>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        default: e = ik_vjp_go<10>(grid, s, ip, dc, q, Tep, success, gq, gTep, gtwist); break;
        }
        if (e != hipSuccess) return hip_fail(e, "k_ik_vjp launch");
        return RTBHIP_OK;
    }
    // rows per round: what fits the default 48 KB of dynamic LDS (25 rows of 241 doubles at 32 joints), far below the compute unit's 160 KB
    const int stride = ik_vjp_any_stride(c->n);
    ip.per = std::min(kWave, (48 * 1024 / 8) / stride);
    if (ip.per < 1) { set_error("ik_vjp: a row of the chain's Jacobian does not fit the compute unit's LDS"); return RTBHIP_ELIMIT; }
    const size_t lds = (size_t)ip.per * stride * sizeof(double);
    const int rc0 = pool_keep_cached();      // the Jacobian comes from the device's pool, kept cached between calls (launch_kin_vjp_s does the same)
    if (rc0 != RTBHIP_OK) return rc0;
    void *p = nullptr;
    hipError_t e = hipMallocAsync(&p, (size_t)N * 6 * (size_t)c->n * sizeof(double), s);
    if (e != hipSuccess) return hip_fail(e, "hipMallocAsync (ik_vjp temporaries)");
    double *Js = (double *)p;
    int rc = launch_kin(c, dc, q, N, notool, notool, 0, nullptr, Js, nullptr, s);
    if (rc == RTBHIP_OK) {
        hipLaunchKernelGGL(k_ik_vjp_any, grid, dim3(kWave), lds, s, ip, Js, Tep, success, gq, gTep, gtwist);
        note_launch((int)grid.x, kWave, (int)lds);
        e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, "k_ik_vjp_any launch");
    }
    (void)hipFreeAsync(p, s);
    return rc;
}
#endif  // RTB_HOST_SIDE

}  // namespace rtbhip
