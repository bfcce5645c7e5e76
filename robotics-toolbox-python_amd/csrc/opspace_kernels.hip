// opspace_kernels.hip -- gfx950 kernels for the OPERATIONAL-SPACE dynamics of a DH / modified-DH arm (rtbhip_opspace): the reference's
// Dynamics.inertia_x and gravload_x (robot/Dynamics.py:924-1025, 1173-1290) and Asada's manipulability measure (robot/Robot.py:871-881), which
// there are an `inertia` (n rne calls), a `gravload`, numpy.linalg.inv / pinv, two products and an eig per configuration.  Here one lane owns one
// configuration: the gravity pass (when Gx is wanted), the n unit-acceleration passes of the inertia kernel with M left in the lane's LDS row, and
// a tail that factors the supplied Jacobian once (opspace_device.h).  q (N, n) and J (N, 6, n) arrive coalesced in the wave's LDS tile, J beside M:
// held in registers across the passes its 6 n doubles (84 VGPRs at n = 7) would spill the recursion; beside M the row is 71 doubles at n = 7,
// 36 KB per wave, four waves per compute unit -- one per SIMD, hence launch bound 1 and the whole register file for the tail.  The finished rows
// (Mx 36 | Gx 6 | asada 1) overlay the tile and leave as contiguous runs; an output whose pointer is NULL is neither computed nor stored.
// Bound: fp64 VALU issue (n or n + 1 passes of ~1.5 kflop, the 2 K solves, two Jacobi eigenvalue sweeps for Asada) against 56 n bytes in and
// up to 344 bytes out per configuration.
#include "opspace_device.h"

namespace rtbhip {

typedef const __attribute__((address_space(4))) DevLink *ConstLinksO;

template <int NJ, bool MDH, bool ALLREV>
__global__ __launch_bounds__(kWave, 1) void k_opspace(OpsParams op, const DevLink *links_g, const double *__restrict__ q, const double *__restrict__ J,
                                                      double *__restrict__ Mx, double *__restrict__ Gx, double *__restrict__ asada)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr OpsLayout L = ops_layout(NJ, ALLREV, ALLREV);
    ConstLinksO links = (ConstLinksO)links_g;
    const int lane = threadIdx.x;
    const int T = op.tile;
    const int64_t cfg0 = (int64_t)blockIdx.x * T;
    const int64_t left = op.N - cfg0;
    const int ncfg = left < T ? (int)left : T;
    ops_fill<NJ>(q + cfg0 * NJ, ncfg * NJ, T, lds, L.stride, L.q_off, lane);
    ops_fill<6 * NJ>(J + cfg0 * (6 * NJ), ncfg * 6 * NJ, T, lds, L.stride, L.j_off, lane);
    __syncthreads();
    if (lane < ncfg) ops_dh_lane<NJ, MDH, ALLREV>(links, L, lds + lane * L.stride, v3(op.grav[0], op.grav[1], op.grav[2]), op.want, op.axes);
    __syncthreads();
    ops_flush_all(op, lds, L.stride, ncfg, cfg0, Mx, Gx, asada, lane);
}

#if RTB_HOST_SIDE
namespace {
template <int NJ, bool MDH, bool ALLREV>
hipError_t ops_go(hipStream_t s, OpsParams op, const DevLink *links, const double *q, const double *J, double *Mx, double *Gx, double *asada)
{
    constexpr OpsLayout L = ops_layout(NJ, ALLREV, ALLREV);
    op.tile = ops_tile_rows(L.stride);
    const size_t lds = (size_t)op.tile * L.stride * sizeof(double);
    const int64_t tiles = (op.N + op.tile - 1) / op.tile;
    if (tiles > 0x7fffffff) return hipErrorInvalidValue;
    auto k = k_opspace<NJ, MDH, ALLREV>;
    if (lds > 48 * 1024) { hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(kWave), lds, s, op, links, q, J, Mx, Gx, asada);
    note_launch((int)tiles, kWave, (int)lds);
    return hipGetLastError();
}
template <int NJ>
hipError_t ops_nj(bool mdh, bool allrev, hipStream_t s, const OpsParams &op, const DevLink *links, const double *q, const double *J, double *Mx, double *Gx,
                  double *asada)
{
    if (mdh) return allrev ? ops_go<NJ, true, true>(s, op, links, q, J, Mx, Gx, asada) : ops_go<NJ, true, false>(s, op, links, q, J, Mx, Gx, asada);
    return allrev ? ops_go<NJ, false, true>(s, op, links, q, J, Mx, Gx, asada) : ops_go<NJ, false, false>(s, op, links, q, J, Mx, Gx, asada);
}
}  // namespace

// (declared in api.cpp, weakly: a library linked without this unit refuses the entry point instead of failing to load)
// q: (N, n); J: (N, 6, n); Mx (N, 6, 6), Gx (N, 6), asada (N): each may be NULL -- all on the device
int launch_opspace(const Dyn *d, const DevLink *links, const double *q, const double *J, int64_t N, const double *grav3, int axes, double *Mx, double *Gx,
                   double *asada, hipStream_t s)
{
    if (N == 0 || (!Mx && !Gx && !asada)) return RTBHIP_OK;
    if (d->n < 1 || d->n > kOpsMaxJoints) { set_error("opspace: chains of 1..16 joints"); return RTBHIP_ELIMIT; }
    if ((N + 7) / 8 > 0x7fffffff) { set_error("opspace: batch too large for one launch"); return RTBHIP_ELIMIT; }
    OpsParams op;
    op.n = d->n; op.axes = axes & 63; op.want = (Mx ? kOpsMx : 0) | (Gx ? kOpsGx : 0) | (asada ? kOpsAsada : 0); op.tile = kWave; op.N = N;
    for (int i = 0; i < 3; i++) op.grav[i] = grav3 ? grav3[i] : 0.0;
    const bool mdh = d->mdh != 0;
    bool allrev = true;
    for (const DevLink &l : d->links) allrev = allrev && l.sigma == 0;
    hipError_t e = hipSuccess;
    switch (d->n) {
    case 1: e = ops_nj<1>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 2: e = ops_nj<2>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 3: e = ops_nj<3>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 4: e = ops_nj<4>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 5: e = ops_nj<5>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 6: e = ops_nj<6>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 7: e = ops_nj<7>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 8: e = ops_nj<8>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 9: e = ops_nj<9>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 10: e = ops_nj<10>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 11: e = ops_nj<11>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 12: e = ops_nj<12>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 13: e = ops_nj<13>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 14: e = ops_nj<14>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    case 15: e = ops_nj<15>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    default: e = ops_nj<16>(mdh, allrev, s, op, links, q, J, Mx, Gx, asada); break;
    }
    if (e != hipSuccess) return hip_fail(e, "k_opspace launch");
    return RTBHIP_OK;
}
#endif  // RTB_HOST_SIDE

}  // namespace rtbhip
