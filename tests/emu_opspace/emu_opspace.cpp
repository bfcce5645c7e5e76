// tests/emu_opspace/emu_opspace.cpp -- TEST INFRASTRUCTURE: the lane body and the tile fill / flush phases of k_opspace and k_tree_opspace
// (csrc/opspace_device.h) run tile by tile, lane by lane on the CPU, in the kernels' phase order and with their LDS layout, so that
// tests/test_opspace_emu.py can hold the operational-space dynamics against the oracle where no GPU exists.  Built by that test into a library of
// its own, linked against tests/emu/libemu.so for the handle registry and the tree compiler.  Instantiated for the joint counts the cases use.
#include "../../robotics-toolbox-python_amd/csrc/rtbhip_internal.h"
#include "../../robotics-toolbox-python_amd/csrc/opspace_device.h"
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

using namespace rtbhip;

static OpsParams params_of(int n, int64_t N, const double *grav3, int axes, const double *Mx, const double *Gx, const double *asada)
{
    OpsParams op;
    op.n = n; op.axes = axes & 63; op.want = (Mx ? kOpsMx : 0) | (Gx ? kOpsGx : 0) | (asada ? kOpsAsada : 0); op.tile = kWave; op.N = N;
    for (int i = 0; i < 3; ++i) op.grav[i] = grav3 ? grav3[i] : 0.0;
    return op;
}

// k_opspace<NJ, MDH, ALLREV>: one tile at a time, a loop over the lanes where the kernel has a barrier.  The LDS tile starts as NaN: a slot read
// before it is written shows
template <int NJ, bool MDH, bool ALLREV>
static void run_dh(const Dyn *d, OpsParams op, const double *q, const double *J, double *Mx, double *Gx, double *asada)
{
    constexpr OpsLayout L = ops_layout(NJ, ALLREV, ALLREV);
    op.tile = ops_tile_rows(L.stride);
    const int T = op.tile;
    std::vector<double> lds((size_t)T * L.stride);
    const int64_t tiles = (op.N + T - 1) / T;
    for (int64_t tile = 0; tile < tiles; ++tile) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<double>::quiet_NaN());
        const int64_t cfg0 = tile * T, left = op.N - cfg0;
        const int ncfg = left < T ? (int)left : T;
        for (int lane = 0; lane < kWave; ++lane) {
            ops_fill<NJ>(q + cfg0 * NJ, ncfg * NJ, T, lds.data(), L.stride, L.q_off, lane);
            ops_fill<6 * NJ>(J + cfg0 * (6 * NJ), ncfg * 6 * NJ, T, lds.data(), L.stride, L.j_off, lane);
        }
        for (int lane = 0; lane < ncfg; ++lane)
            ops_dh_lane<NJ, MDH, ALLREV>(d->links.data(), L, lds.data() + lane * L.stride, v3(op.grav[0], op.grav[1], op.grav[2]), op.want, op.axes);
        for (int lane = 0; lane < kWave; ++lane) ops_flush_all(op, lds.data(), L.stride, ncfg, cfg0, Mx, Gx, asada, lane);
    }
}
template <int NJ>
static void run_dh_nj(const Dyn *d, const OpsParams &op, const double *q, const double *J, double *Mx, double *Gx, double *asada)
{
    bool allrev = true;
    for (const DevLink &l : d->links) allrev = allrev && l.sigma == 0;
    if (d->mdh) { if (allrev) run_dh<NJ, true, true>(d, op, q, J, Mx, Gx, asada); else run_dh<NJ, true, false>(d, op, q, J, Mx, Gx, asada); }
    else { if (allrev) run_dh<NJ, false, true>(d, op, q, J, Mx, Gx, asada); else run_dh<NJ, false, false>(d, op, q, J, Mx, Gx, asada); }
}

template <int NG>
static void run_tree(const Tree *t, OpsParams op, const double *q, const double *J, double *Mx, double *Gx, double *asada)
{
    constexpr OpsLayout L = ops_layout(NG, true, false);
    op.tile = ops_tile_rows(L.stride + kTreeSlotDoubles * t->nslots);
    const int T = op.tile;
    std::vector<double> lds((size_t)T * (L.stride + kTreeSlotDoubles * std::max(1, t->nslots)));
    double *slots = lds.data() + (size_t)T * L.stride;
    const int64_t tiles = (op.N + T - 1) / T;
    for (int64_t tile = 0; tile < tiles; ++tile) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<double>::quiet_NaN());
        const int64_t cfg0 = tile * T, left = op.N - cfg0;
        const int ncfg = left < T ? (int)left : T;
        for (int lane = 0; lane < kWave; ++lane) {
            ops_fill<NG>(q + cfg0 * NG, ncfg * NG, T, lds.data(), L.stride, L.q_off, lane);
            ops_fill<6 * NG>(J + cfg0 * (6 * NG), ncfg * 6 * NG, T, lds.data(), L.stride, L.j_off, lane);
        }
        for (int lane = 0; lane < ncfg; ++lane)
            ops_tree_lane<NG>(t->groups.data(), t->nslots, L, lds.data() + lane * L.stride, v3(op.grav[0], op.grav[1], op.grav[2]), op.want, op.axes,
                              [&](int i) -> double & { return slots[i * T + lane]; });
        for (int lane = 0; lane < kWave; ++lane) ops_flush_all(op, lds.data(), L.stride, ncfg, cfg0, Mx, Gx, asada, lane);
    }
}

// q: (N, n); J: (N, 6, n); Mx (N, 6, 6), Gx (N, 6), asada (N): each may be NULL.  -3: a joint count this replay is not instantiated for
extern "C" int emu_opspace(rtbhip_dyn_t h, const double *q, const double *J, int64_t N, const double *grav3, int axes, double *Mx, double *Gx,
                           double *asada)
{
    const std::shared_ptr<Dyn> d_owner = dyn_from_handle(h);
    const Dyn *d = d_owner.get();
    if (!d) return -1;
    const OpsParams op = params_of(d->n, N, grav3, axes, Mx, Gx, asada);
    switch (d->n) {
    case 3: run_dh_nj<3>(d, op, q, J, Mx, Gx, asada); break;
    case 6: run_dh_nj<6>(d, op, q, J, Mx, Gx, asada); break;
    case 7: run_dh_nj<7>(d, op, q, J, Mx, Gx, asada); break;
    case 8: run_dh_nj<8>(d, op, q, J, Mx, Gx, asada); break;
    case 9: run_dh_nj<9>(d, op, q, J, Mx, Gx, asada); break;
    case 16: run_dh_nj<16>(d, op, q, J, Mx, Gx, asada); break;
    default: return -3;
    }
    return 0;
}

extern "C" int emu_tree_opspace(const rtbhip_tree_group *groups, int ng, const double *q, const double *J, int64_t N, const double *grav3, int axes,
                                double *Mx, double *Gx, double *asada)
{
    Tree t;
    if (compile_tree(groups, ng, &t) != RTBHIP_OK) return -1;
    for (int j = 0; j < t.n; ++j)
        if (jm_jq(t.groups[j].jmeta) != j) return -2;          // rtbhip_tree_opspace's refusal
    const OpsParams op = params_of(t.n, N, grav3, axes, Mx, Gx, asada);
    switch (t.n) {
    case 6: run_tree<6>(&t, op, q, J, Mx, Gx, asada); break;
    case 7: run_tree<7>(&t, op, q, J, Mx, Gx, asada); break;
    default: return -3;
    }
    return 0;
}

// the row layout and tile size the kernels use (for the test's own statements about LDS)
extern "C" void emu_opspace_layout(int n, int packed, int q_in_tile, int *out5)
{
    const OpsLayout L = ops_layout(n, packed != 0, q_in_tile != 0);
    out5[0] = L.wm; out5[1] = L.q_off; out5[2] = L.j_off; out5[3] = L.g_off; out5[4] = L.stride;
}
