// mmc_kernels.hip -- gfx950 kernels for the REACTIVE QP SERVO (rtbhip_mmc): p_servo's error, the manipulability Jacobian, the joint-limit
// velocity dampers and a per-lane active-set QP as one launch, and the loop q <- q + dt qd iterated on the device.  mmc_device.h has the
// definition, the QP's method, the lane body and the tile phases.
//
//   k_mmc<NJ>    6..10 joints.  One lane = one row, 64-lane tiles, one tile per single-wave workgroup (the launch shape of the resolved-rate
//                kernel).  q and Tep arrive coalesced in a lane-major LDS tile of odd stride; the lane walks the chain ONCE per iteration, for
//                jacob0 (jacobm is defined on it; jacobe is its two halves rotated by R^T), forms the error, the gradient g, the box, runs
//                the QP's rounds and steps -- up to `steps` times, with no barrier inside the loop; q and qd live in the lane's LDS row
//                between iterations.  q_out is where q was, arrived, its and status take three of Tep's slots.
//                8 (2 n + 16) + 6 bytes per row: 246 for the Panda.  The joint limits and the velocity box travel in the parameter struct,
//                copied from the caller's host arrays at call time: no host pointer is read by the launch, so a captured graph replays.
#include <hip/hip_runtime.h>
#include <limits>
#include "rtbhip_internal.h"
#include "diff_kernel.h"
#include "mmc_device.h"

namespace rtbhip {

// WAVES per SIMD: 2 (256 VGPRs) where the instantiation fits, 1 (512) beyond (tests/test_code_object_notes_mmc.py reads the code objects' notes;
// DESIGN.md section 4.20 has the table)
template <int NJ> struct MmcWaves { static constexpr int v = NJ <= kMmcTwoWavesMax ? 2 : 1; };

template <int NJ>
__global__ __launch_bounds__(kWave, MmcWaves<NJ>::v) void k_mmc(MmcParams mp, DevChain dc, const double *__restrict__ q, const double *__restrict__ Tep,
                                                                 double *__restrict__ qd, double *__restrict__ q_out, uint8_t *__restrict__ arrived,
                                                                 int32_t *__restrict__ its, uint8_t *__restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const ConstChain cv = const_view(dc);
    const int lane = threadIdx.x;
    const int64_t tile = xcd_tile();
    const VjpTile t = vjp_tile_of(tile, mp.N, NJ);
    mmc_tile_fill<NJ>(mp, q, Tep, tile, lane, lds);
    __syncthreads();
    // a lane past the ragged tail is not live: it never walks, and nothing of it is flushed
    mmc_lane<NJ>(mp, cv, lane < t.ncfg, lds + lane * mmc_stride(NJ));
    __syncthreads();
    mmc_tile_flush(NJ, t.ncfg, lds, qd ? qd + t.cfg0 * NJ : nullptr, q_out ? q_out + t.cfg0 * NJ : nullptr, arrived ? arrived + t.cfg0 : nullptr,
                   its ? its + t.cfg0 : nullptr, status ? status + t.cfg0 : nullptr, lane);
}

#if RTB_HOST_SIDE
namespace {
template <int NJ>
hipError_t mmc_go(dim3 grid, hipStream_t s, const MmcParams &mp, const DevChain &dc, const rtbhip_mmc_args *a)
{
    const size_t lds = (size_t)kWave * mmc_stride(NJ) * sizeof(double);       // at most 64 x 37 doubles: under the default 48 KB
    hipLaunchKernelGGL((k_mmc<NJ>), grid, dim3(kWave), lds, s, mp, dc, a->q, a->Tep, a->qd, a->q_out, a->arrived, a->its, a->status);
    note_launch((int)grid.x, kWave, (int)lds);
    return hipGetLastError();
}
}  // namespace

// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
// a: the caller's block, checked by rtbhip_mmc -- N > 0, 6..10 joints, every array pointer on the device but qlim / qdlim, which are host arrays
// read HERE, before the launch
int launch_mmc(const Chain *c, const DevChain &dc, const rtbhip_mmc_args *a, hipStream_t s)
{
    const int64_t tiles = a->N / kWave + (a->N % kWave != 0);
    if (a->N <= 0 || tiles > 0x7fffffff || c->n < kMmcMin || c->n > kMmcMax || !a->qlim) { set_error("mmc: launch outside the checked range"); return RTBHIP_ELIMIT; }
    MmcParams mp;
    mp.n = c->n; mp.method = a->method; mp.steps = a->steps; mp.tep_each = a->nTep == a->N ? 1 : 0;
    mp.N = a->N;
    for (int k = 0; k < 6; ++k) mp.gain[k] = a->gain6[k];
    mp.threshold = a->threshold; mp.dt = a->dt;
    mp.Y = a->Y; mp.ks = a->ks; mp.km = a->km; mp.ps = a->ps; mp.pi = a->pi; mp.dgain = a->damper_gain;
    for (int j = 0; j < kMmcMax; ++j) {
        const bool in = j < c->n;
        mp.qlo[j] = in ? a->qlim[j] : -std::numeric_limits<double>::infinity();
        mp.qhi[j] = in ? a->qlim[c->n + j] : std::numeric_limits<double>::infinity();
        mp.vmax[j] = in && a->qdlim ? a->qdlim[j] : std::numeric_limits<double>::infinity();
    }
    Affine notool;
    notool.used = 0;
    for (int i = 0; i < 12; i++) notool.v[i] = (i % 5 == 0) ? 1.0 : 0.0;
    chain_tail(c, notool, mp.tail);
    const dim3 grid((unsigned)tiles);
    hipError_t e = hipSuccess;
    switch (c->n) {
    case 6: e = mmc_go<6>(grid, s, mp, dc, a); break;
    case 7: e = mmc_go<7>(grid, s, mp, dc, a); break;
    case 8: e = mmc_go<8>(grid, s, mp, dc, a); break;
    case 9: e = mmc_go<9>(grid, s, mp, dc, a); break;
    case 10: e = mmc_go<10>(grid, s, mp, dc, a); break;
    }
    if (e != hipSuccess) return hip_fail(e, "k_mmc launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

}  // namespace rtbhip
