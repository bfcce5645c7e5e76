// rrmc_kernels.hip -- gfx950 kernels for RESOLVED-RATE MOTION CONTROL (rtbhip_rrmc): p_servo + pinv(J) as one launch, and the servo loop
// q <- q + dt pinv(J(q)) p_servo(fkine(q), Tep) iterated on the device.  rrmc_device.h has the definition, the lane body and the tile phases.
//
//   k_rrmc<NJ>   1..kKinRegMax joints.  One lane = one row, 64-lane tiles, one tile per single-wave workgroup (the launch shape of k_ik_vjp).  q,
//                qnull and Tep arrive coalesced in a lane-major LDS tile of odd stride; the lane walks the chain in registers (reg_core: neither the
//                pose nor the Jacobian ever reaches memory), forms p_servo's error, solves for the joint rate and steps -- up to `steps` times, with
//                no barrier inside the loop; q and qd live in the lane's LDS row between iterations.  q_out is where q was, arrived and its
//                take two of Tep's slots; they leave the way the inputs came.
//                8 (3 n + 16) + 5 bytes per row: 301 for the Panda.  Everything the loop needs travels in the parameter struct: no host pointer is
//                read, so a captured graph replays correctly.
// Chains of more than kKinRegMax joints are refused (RTBHIP_ELIMIT); the run-time-n form is a follow-up.
#include <hip/hip_runtime.h>
#include "rtbhip_internal.h"
#include "diff_kernel.h"
#include "rrmc_device.h"

namespace rtbhip {

// Two waves per SIMD, as k_ik_vjp (tests/test_code_object_notes_rrmc.py reads the code objects' notes)
template <int NJ>
__global__ __launch_bounds__(kWave, 2) void k_rrmc(RrmcParams rp, DevChain dc, const double *__restrict__ q, const double *__restrict__ Tep,
                                                   const double *__restrict__ qnull, double *__restrict__ qd, double *__restrict__ q_out,
                                                   uint8_t *__restrict__ arrived, int32_t *__restrict__ its)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const ConstChain cv = const_view(dc);
    const int lane = threadIdx.x;
    const int64_t tile = xcd_tile();
    const VjpTile t = vjp_tile_of(tile, rp.N, NJ);
    rrmc_tile_fill<NJ>(rp, q, qnull, Tep, tile, lane, lds);
    __syncthreads();
    // a lane past the ragged tail is not live: it never walks, and nothing of it is flushed
    rrmc_lane<NJ>(rp, cv, qnull != nullptr, lane < t.ncfg, lds + lane * rrmc_stride(NJ));
    __syncthreads();
    rrmc_tile_flush(NJ, t.ncfg, lds, qd ? qd + t.cfg0 * NJ : nullptr, q_out ? q_out + t.cfg0 * NJ : nullptr, arrived ? arrived + t.cfg0 : nullptr,
                    its ? its + t.cfg0 : nullptr, lane);
}

#if RTB_HOST_SIDE
namespace {
template <int NJ>
hipError_t rrmc_go(dim3 grid, hipStream_t s, const RrmcParams &rp, const DevChain &dc, const rtbhip_rrmc_args *a)
{
    const size_t lds = (size_t)kWave * rrmc_stride(NJ) * sizeof(double);      // at most 64 x 47 doubles: under the default 48 KB
    hipLaunchKernelGGL((k_rrmc<NJ>), grid, dim3(kWave), lds, s, rp, dc, a->q, a->Tep, a->qnull, a->qd, a->q_out, a->arrived, a->its);
    note_launch((int)grid.x, kWave, (int)lds);
    return hipGetLastError();
}
}  // namespace

// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
// a: the caller's block, checked by rtbhip_rrmc -- N > 0, 1..kKinRegMax joints, every pointer on the device
int launch_rrmc(const Chain *c, const DevChain &dc, const rtbhip_rrmc_args *a, hipStream_t s)
{
    const int64_t tiles = (a->N + kWave - 1) / kWave;
    if (a->N <= 0 || tiles > 0x7fffffff || c->n < 1 || c->n > kKinRegMax) { set_error("rrmc: launch outside the checked range"); return RTBHIP_ELIMIT; }
    RrmcParams rp;
    rp.n = c->n; rp.method = a->method; rp.steps = a->steps; rp.tep_each = a->nTep == a->N ? 1 : 0;
    rp.N = a->N;
    for (int k = 0; k < 6; ++k) rp.gain[k] = a->gain6[k];
    rp.threshold = a->threshold; rp.d2 = a->damping * a->damping; rp.dt = a->dt;
    Affine notool;
    notool.used = 0;
    for (int i = 0; i < 12; i++) notool.v[i] = (i % 5 == 0) ? 1.0 : 0.0;
    chain_tail(c, notool, rp.tail);
    const dim3 grid((unsigned)tiles);
    hipError_t e = hipSuccess;
    switch (c->n) {
    case 1: e = rrmc_go<1>(grid, s, rp, dc, a); break;
    case 2: e = rrmc_go<2>(grid, s, rp, dc, a); break;
    case 3: e = rrmc_go<3>(grid, s, rp, dc, a); break;
    case 4: e = rrmc_go<4>(grid, s, rp, dc, a); break;
    case 5: e = rrmc_go<5>(grid, s, rp, dc, a); break;
    case 6: e = rrmc_go<6>(grid, s, rp, dc, a); break;
    case 7: e = rrmc_go<7>(grid, s, rp, dc, a); break;
    case 8: e = rrmc_go<8>(grid, s, rp, dc, a); break;
    case 9: e = rrmc_go<9>(grid, s, rp, dc, a); break;
    case 10: e = rrmc_go<10>(grid, s, rp, dc, a); break;
    }
    if (e != hipSuccess) return hip_fail(e, "k_rrmc launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

}  // namespace rtbhip
