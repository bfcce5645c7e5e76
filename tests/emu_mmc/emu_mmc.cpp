// tests/emu_mmc/emu_mmc.cpp -- TEST INFRASTRUCTURE: the lane body and the tile fill / flush phases of k_mmc (csrc/mmc_device.h, csrc/kin_vjp.h,
// csrc/vjp_tile.h) run tile by tile, lane by lane on the CPU, in the kernel's phase order and with its LDS layout, so that tests/test_mmc_emu.py
// can hold the reactive QP servo against the oracle where no GPU exists.  Built by that test into a library of its own, linked against
// tests/emu/libemu.so for the chain compiler and the handle registry.
#include "../../robotics-toolbox-python_amd/csrc/rtbhip_internal.h"
#include "../../robotics-toolbox-python_amd/csrc/mmc_device.h"
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

using namespace rtbhip;

// (what launch_mmc does, csrc/mmc_kernels.hip)
static MmcParams params_of(const Chain *c, const rtbhip_mmc_args *a)
{
    MmcParams mp;
    mp.n = c->n; mp.method = a->method; mp.steps = a->steps; mp.tep_each = a->nTep == a->N ? 1 : 0;
    mp.N = a->N;
    for (int k = 0; k < 6; ++k) mp.gain[k] = a->gain6[k];
    mp.threshold = a->threshold; mp.dt = a->dt;
    mp.Y = a->Y; mp.ks = a->ks; mp.km = a->km; mp.ps = a->ps; mp.pi = a->pi; mp.dgain = a->damper_gain;
    const double inf = std::numeric_limits<double>::infinity();
    for (int j = 0; j < kMmcMax; ++j) {
        const bool in = j < c->n;
        mp.qlo[j] = in ? a->qlim[j] : -inf;
        mp.qhi[j] = in ? a->qlim[c->n + j] : inf;
        mp.vmax[j] = in && a->qdlim ? a->qdlim[j] : inf;
    }
    Affine notool;
    notool.used = 0;
    for (int i = 0; i < 12; i++) notool.v[i] = (i % 5 == 0) ? 1.0 : 0.0;
    chain_tail(c, notool, mp.tail);
    return mp;
}

// k_mmc<NJ>: one tile at a time, a loop over the lanes where the kernel has a barrier.  The LDS tile starts as NaN: a slot read before it is
// written shows.  (One lane at a time the wave's ballot is the lane's own flag: each lane leaves its loops when it is done.)
template <int NJ>
static void run_reg(const Chain *c, const MmcParams &mp, const rtbhip_mmc_args *a)
{
    const DevChain cv = chain_host_view(c);
    const int stride = mmc_stride(NJ);
    std::vector<double> lds((size_t)kWave * stride);
    const int64_t tiles = (mp.N + kWave - 1) / kWave;
    for (int64_t tile = 0; tile < tiles; ++tile) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<double>::quiet_NaN());
        const VjpTile t = vjp_tile_of(tile, mp.N, NJ);
        for (int lane = 0; lane < kWave; ++lane) mmc_tile_fill<NJ>(mp, a->q, a->Tep, tile, lane, lds.data());
        for (int lane = 0; lane < kWave; ++lane) mmc_lane<NJ>(mp, cv, lane < t.ncfg, lds.data() + lane * stride);
        for (int lane = 0; lane < kWave; ++lane)
            mmc_tile_flush(NJ, t.ncfg, lds.data(), a->qd ? a->qd + t.cfg0 * NJ : nullptr, a->q_out ? a->q_out + t.cfg0 * NJ : nullptr,
                           a->arrived ? a->arrived + t.cfg0 : nullptr, a->its ? a->its + t.cfg0 : nullptr, a->status ? a->status + t.cfg0 : nullptr, lane);
    }
}

// the block of rtbhip_mmc with HOST pointers; the argument checks are the entry point's, not repeated here
extern "C" int emu_mmc(const rtbhip_mmc_args *a)
{
    if (!a || a->size != sizeof(rtbhip_mmc_args)) return -1;
    const std::shared_ptr<Chain> c_owner = chain_from_handle(a->chain);
    const Chain *c = c_owner.get();
    if (!c || !a->qlim) return -1;
    if (c->n < kMmcMin || c->n > kMmcMax || c->q_width != c->n || a->steps < 1) return -3;
    const MmcParams mp = params_of(c, a);
    switch (c->n) {
    case 6: run_reg<6>(c, mp, a); break;
    case 7: run_reg<7>(c, mp, a); break;
    case 8: run_reg<8>(c, mp, a); break;
    case 9: run_reg<9>(c, mp, a); break;
    default: run_reg<10>(c, mp, a); break;
    }
    return 0;
}
