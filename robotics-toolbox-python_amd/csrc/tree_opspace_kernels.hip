// tree_opspace_kernels.hip -- gfx950 kernel for the OPERATIONAL-SPACE dynamics of an ETS / URDF robot's link tree (rtbhip_tree_opspace): what
// opspace_kernels.hip does for DH arms, on tree_device.h's recursion (Dynamics.inertia_x / gravload_x, robot/Dynamics.py:924-1025, 1173-1290, and
// Asada's measure, robot/Robot.py:871-881, over Robot.rne, robot/Robot.py:1704-1903).  A unit of its own for build time only, as tree_dyn_kernels.hip.
// The robot must be numbered in group order (the launcher's caller refuses the others): M's packed triangle is then the reference's matrix.
// LDS per lane: the packed M tile, q, J (6 n), and the tree's branch slots behind the rows.
#include "tree_kernels.h"
#include "opspace_device.h"

namespace rtbhip {

template <int NG>
__global__ __launch_bounds__(kWave, 1) void k_tree_opspace(OpsParams op, int nslots, const DevGroup *groups_g, const double *__restrict__ q,
                                                           const double *__restrict__ J, double *__restrict__ Mx, double *__restrict__ Gx,
                                                           double *__restrict__ asada)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr OpsLayout L = ops_layout(NG, true, false);
    ConstGroups groups = (ConstGroups)groups_g;
    const int lane = threadIdx.x;
    const int T = op.tile;
    double *slots = lds + T * L.stride;
    const int64_t cfg0 = (int64_t)blockIdx.x * T;
    const int64_t left = op.N - cfg0;
    const int ncfg = left < T ? (int)left : T;
    ops_fill<NG>(q + cfg0 * NG, ncfg * NG, T, lds, L.stride, L.q_off, lane);
    ops_fill<6 * NG>(J + cfg0 * (6 * NG), ncfg * 6 * NG, T, lds, L.stride, L.j_off, lane);
    __syncthreads();
    if (lane < ncfg)
        ops_tree_lane<NG>(groups, nslots, L, lds + lane * L.stride, v3(op.grav[0], op.grav[1], op.grav[2]), op.want, op.axes,
                          [&](int i) -> double & { return slots[i * T + lane]; });
    __syncthreads();
    ops_flush_all(op, lds, L.stride, ncfg, cfg0, Mx, Gx, asada, lane);
}

#if RTB_HOST_SIDE
namespace {
template <int NG>
int tree_ops_go(hipStream_t s, OpsParams op, int nslots, const DevGroup *g, const double *q, const double *J, double *Mx, double *Gx, double *asada)
{
    constexpr OpsLayout L = ops_layout(NG, true, false);
    const int per_row = L.stride + kTreeSlotDoubles * nslots;
    op.tile = ops_tile_rows(per_row);
    const size_t lds = (size_t)op.tile * per_row * sizeof(double);
    // Not reachable with kOpsMaxJoints = 16: a tree of n groups has at most n - 2 branch slots (a slot needs a parent with a child two or more
    // groups on), so a row is at most 265 + 18 * 14 = 517 doubles, which ops_tile_rows serves with 32 rows: 132352 bytes.  Kept for a larger limit.
    if (lds > 160 * 1024) { set_error("tree_opspace: the robot needs more LDS than a CU has"); return RTBHIP_ELIMIT; }
    const int64_t tiles = (op.N + op.tile - 1) / op.tile;
    if (tiles > 0x7fffffff) { set_error("tree_opspace: batch too large for one launch"); return RTBHIP_ELIMIT; }
    auto k = k_tree_opspace<NG>;
    if (lds > 48 * 1024) { hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return hip_fail(e, "k_tree_opspace attribute"); }
    hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(kWave), lds, s, op, nslots, g, q, J, Mx, Gx, asada);
    note_launch((int)tiles, kWave, (int)lds);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_tree_opspace launch");
    return RTBHIP_OK;
}
}  // namespace

// (declared in api.cpp, weakly, as launch_opspace)
int launch_tree_opspace(const Tree *t, const DevGroup *groups, const double *q, const double *J, int64_t N, const double *grav3, int axes, double *Mx,
                        double *Gx, double *asada, hipStream_t s)
{
    if (N == 0 || (!Mx && !Gx && !asada)) return RTBHIP_OK;
    if (t->n < 1 || t->n > kOpsMaxJoints) { set_error("tree_opspace: robots of 1..16 joints"); return RTBHIP_ELIMIT; }
    OpsParams op;
    op.n = t->n; op.axes = axes & 63; op.want = (Mx ? kOpsMx : 0) | (Gx ? kOpsGx : 0) | (asada ? kOpsAsada : 0); op.tile = kWave; op.N = N;
    for (int i = 0; i < 3; i++) op.grav[i] = grav3 ? grav3[i] : 0.0;
    switch (t->n) {
    case 1: return tree_ops_go<1>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 2: return tree_ops_go<2>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 3: return tree_ops_go<3>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 4: return tree_ops_go<4>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 5: return tree_ops_go<5>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 6: return tree_ops_go<6>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 7: return tree_ops_go<7>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 8: return tree_ops_go<8>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 9: return tree_ops_go<9>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 10: return tree_ops_go<10>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 11: return tree_ops_go<11>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 12: return tree_ops_go<12>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 13: return tree_ops_go<13>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 14: return tree_ops_go<14>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    case 15: return tree_ops_go<15>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    default: return tree_ops_go<16>(s, op, t->nslots, groups, q, J, Mx, Gx, asada);
    }
}
#endif  // RTB_HOST_SIDE

}  // namespace rtbhip
