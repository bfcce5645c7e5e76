// tests/emu_opspace/emu_opspace.cpp -- TEST INFRASTRUCTURE: the lane body and the tile fill / flush phases of k_opspace and k_tree_opspace
// (csrc/opspace_device.h) run tile by tile, lane by lane on the CPU, in the kernels' phase order and with their LDS layout, so that
// tests/test_opspace_emu.py and tests/test_opspace_census.py can hold the operational-space dynamics against the oracle where no GPU exists.
// Built by tests/test_opspace_emu.py into a library of its own, linked against tests/emu/libemu.so for the handle registry and the tree compiler.
// Instantiated for every size the launchers serve: 1..16 joints, both DH conventions, all-revolute or not (64 forms), and 1..16 link groups.
// The 80 instantiations are too slow for one compiler process: this file is compiled once per value of EMU_OPS_PART (0..kParts - 1), each part
// holding the entry points (part 0) or the instantiations of a range of sizes, and the objects are linked into one library.  Without the macro
// the file is one translation unit with everything in it.
#include "../../robotics-toolbox-python_amd/csrc/rtbhip_internal.h"
#include "../../robotics-toolbox-python_amd/csrc/opspace_device.h"
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#ifndef EMU_OPS_PART
#define EMU_OPS_PART -1
#endif
#define EMU_OPS_HAS(part) (EMU_OPS_PART < 0 || EMU_OPS_PART == (part))
using namespace rtbhip;

// what the last replayed launch would have asked for: (workgroups, rows per tile, doubles per row); defined in part 0
extern int64_t emu_ops_last[3];
extern int64_t emu_ops_tile_limit;          // bytes; 0: the kernels' own limit

namespace {

// ops_tile_rows -- or, when a test has moved the limit (emu_opspace_set_tile_limit), the same statements with that limit: the seam between the two
// tile sizes then falls on other robots, and the replay must still equal the oracle
int tile_rows(int doubles_per_row)
{
    if (emu_ops_tile_limit <= 0) return ops_tile_rows(doubles_per_row);
    int t = kWave;
    while (t > 8 && (size_t)doubles_per_row * t * sizeof(double) > (size_t)emu_ops_tile_limit) t /= 2;
    return t;
}

// k_opspace<NJ, MDH, ALLREV>: one tile at a time, a loop over the lanes where the kernel has a barrier.  The LDS tile starts as NaN: a slot read
// before it is written shows
template <int NJ, bool MDH, bool ALLREV>
void run_dh(const Dyn *d, OpsParams op, const double *q, const double *J, double *Mx, double *Gx, double *asada)
{
    constexpr OpsLayout L = ops_layout(NJ, ALLREV, ALLREV);
    op.tile = tile_rows(L.stride);
    const int T = op.tile;
    std::vector<double> lds((size_t)T * L.stride);
    const int64_t tiles = (op.N + T - 1) / T;
    emu_ops_last[0] = tiles; emu_ops_last[1] = T; emu_ops_last[2] = L.stride;
    for (int64_t tile = 0; tile < tiles; ++tile) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<double>::quiet_NaN());
        const int64_t cfg0 = tile * T, left = op.N - cfg0;
        const int ncfg = left < T ? (int)left : T;
        for (int lane = 0; lane < kWave; ++lane) {
            ops_fill<NJ>(q + cfg0 * NJ, ncfg * NJ, T, lds.data(), L.stride, L.q_off, lane);
            ops_fill<6 * NJ>(J + cfg0 * (6 * NJ), ncfg * 6 * NJ, T, lds.data(), L.stride, L.j_off, lane);
        }
        for (int lane = 0; lane < kWave; ++lane)
            if (lane < ncfg)
                ops_dh_lane<NJ, MDH, ALLREV>(d->links.data(), L, lds.data() + lane * L.stride, v3(op.grav[0], op.grav[1], op.grav[2]), op.want, op.axes);
        for (int lane = 0; lane < kWave; ++lane) ops_flush_all(op, lds.data(), L.stride, ncfg, cfg0, Mx, Gx, asada, lane);
    }
}
template <int NJ>
void run_dh_nj(const Dyn *d, const OpsParams &op, const double *q, const double *J, double *Mx, double *Gx, double *asada)
{
    bool allrev = true;
    for (const DevLink &l : d->links) allrev = allrev && l.sigma == 0;
    if (d->mdh) { if (allrev) run_dh<NJ, true, true>(d, op, q, J, Mx, Gx, asada); else run_dh<NJ, true, false>(d, op, q, J, Mx, Gx, asada); }
    else { if (allrev) run_dh<NJ, false, true>(d, op, q, J, Mx, Gx, asada); else run_dh<NJ, false, false>(d, op, q, J, Mx, Gx, asada); }
}

template <int NG>
void run_tree(const Tree *t, OpsParams op, const double *q, const double *J, double *Mx, double *Gx, double *asada)
{
    constexpr OpsLayout L = ops_layout(NG, true, false);
    const int per_row = L.stride + kTreeSlotDoubles * t->nslots;
    op.tile = tile_rows(per_row);
    const int T = op.tile;
    std::vector<double> lds((size_t)T * (L.stride + kTreeSlotDoubles * std::max(1, t->nslots)));
    double *slots = lds.data() + (size_t)T * L.stride;
    const int64_t tiles = (op.N + T - 1) / T;
    emu_ops_last[0] = tiles; emu_ops_last[1] = T; emu_ops_last[2] = per_row;
    for (int64_t tile = 0; tile < tiles; ++tile) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<double>::quiet_NaN());
        const int64_t cfg0 = tile * T, left = op.N - cfg0;
        const int ncfg = left < T ? (int)left : T;
        for (int lane = 0; lane < kWave; ++lane) {
            ops_fill<NG>(q + cfg0 * NG, ncfg * NG, T, lds.data(), L.stride, L.q_off, lane);
            ops_fill<6 * NG>(J + cfg0 * (6 * NG), ncfg * 6 * NG, T, lds.data(), L.stride, L.j_off, lane);
        }
        for (int lane = 0; lane < kWave; ++lane)
            if (lane < ncfg)
                ops_tree_lane<NG>(t->groups.data(), t->nslots, L, lds.data() + lane * L.stride, v3(op.grav[0], op.grav[1], op.grav[2]), op.want, op.axes,
                                  [&](int i) -> double & { return slots[i * T + lane]; });
        for (int lane = 0; lane < kWave; ++lane) ops_flush_all(op, lds.data(), L.stride, ncfg, cfg0, Mx, Gx, asada, lane);
    }
}

}  // namespace

// one function per range of sizes, each in a part of its own: true when the size is its own
#define EMU_OPS_DH_ARGS const Dyn *d, const OpsParams &op, const double *q, const double *J, double *Mx, double *Gx, double *asada
#define EMU_OPS_TREE_ARGS const Tree *t, const OpsParams &op, const double *q, const double *J, double *Mx, double *Gx, double *asada
#define DH_CASE(K) case K: run_dh_nj<K>(d, op, q, J, Mx, Gx, asada); return true;
#define TREE_CASE(K) case K: run_tree<K>(t, op, q, J, Mx, Gx, asada); return true;
bool emu_ops_dh_1_8(EMU_OPS_DH_ARGS);
bool emu_ops_dh_9_11(EMU_OPS_DH_ARGS);
bool emu_ops_dh_12_13(EMU_OPS_DH_ARGS);
bool emu_ops_dh_14(EMU_OPS_DH_ARGS);
bool emu_ops_dh_15(EMU_OPS_DH_ARGS);
bool emu_ops_dh_16(EMU_OPS_DH_ARGS);
bool emu_ops_tree_1_9(EMU_OPS_TREE_ARGS);
bool emu_ops_tree_10_13(EMU_OPS_TREE_ARGS);
bool emu_ops_tree_14_16(EMU_OPS_TREE_ARGS);

#if EMU_OPS_HAS(1)
bool emu_ops_dh_1_8(EMU_OPS_DH_ARGS)
{
    switch (d->n) { DH_CASE(1) DH_CASE(2) DH_CASE(3) DH_CASE(4) DH_CASE(5) DH_CASE(6) DH_CASE(7) DH_CASE(8) default: return false; }
}
#endif
#if EMU_OPS_HAS(2)
bool emu_ops_dh_9_11(EMU_OPS_DH_ARGS) { switch (d->n) { DH_CASE(9) DH_CASE(10) DH_CASE(11) default: return false; } }
#endif
#if EMU_OPS_HAS(3)
bool emu_ops_dh_12_13(EMU_OPS_DH_ARGS) { switch (d->n) { DH_CASE(12) DH_CASE(13) default: return false; } }
#endif
#if EMU_OPS_HAS(4)
bool emu_ops_dh_14(EMU_OPS_DH_ARGS) { switch (d->n) { DH_CASE(14) default: return false; } }
#endif
#if EMU_OPS_HAS(5)
bool emu_ops_dh_15(EMU_OPS_DH_ARGS) { switch (d->n) { DH_CASE(15) default: return false; } }
#endif
#if EMU_OPS_HAS(6)
bool emu_ops_dh_16(EMU_OPS_DH_ARGS) { switch (d->n) { DH_CASE(16) default: return false; } }
#endif
#if EMU_OPS_HAS(7)
bool emu_ops_tree_1_9(EMU_OPS_TREE_ARGS)
{
    switch (t->n) { TREE_CASE(1) TREE_CASE(2) TREE_CASE(3) TREE_CASE(4) TREE_CASE(5) TREE_CASE(6) TREE_CASE(7) TREE_CASE(8) TREE_CASE(9) default: return false; }
}
#endif
#if EMU_OPS_HAS(8)
bool emu_ops_tree_10_13(EMU_OPS_TREE_ARGS) { switch (t->n) { TREE_CASE(10) TREE_CASE(11) TREE_CASE(12) TREE_CASE(13) default: return false; } }
#endif
#if EMU_OPS_HAS(9)
bool emu_ops_tree_14_16(EMU_OPS_TREE_ARGS) { switch (t->n) { TREE_CASE(14) TREE_CASE(15) TREE_CASE(16) default: return false; } }
#endif

#if EMU_OPS_HAS(0)
int64_t emu_ops_last[3] = {0, 0, 0};
int64_t emu_ops_tile_limit = 0;

static OpsParams params_of(int n, int64_t N, const double *grav3, int axes, const double *Mx, const double *Gx, const double *asada)
{
    OpsParams op;
    op.n = n; op.axes = axes & 63; op.want = (Mx ? kOpsMx : 0) | (Gx ? kOpsGx : 0) | (asada ? kOpsAsada : 0); op.tile = kWave; op.N = N;
    for (int i = 0; i < 3; ++i) op.grav[i] = grav3 ? grav3[i] : 0.0;
    return op;
}

// q: (N, n); J: (N, 6, n); Mx (N, 6, 6), Gx (N, 6), asada (N): each may be NULL.  -3: more joints than the launcher serves (its own refusal)
extern "C" int emu_opspace(rtbhip_dyn_t h, const double *q, const double *J, int64_t N, const double *grav3, int axes, double *Mx, double *Gx,
                           double *asada)
{
    const std::shared_ptr<Dyn> d_owner = dyn_from_handle(h);
    const Dyn *d = d_owner.get();
    if (!d) return -1;
    if (d->n < 1 || d->n > kOpsMaxJoints) return -3;
    const OpsParams op = params_of(d->n, N, grav3, axes, Mx, Gx, asada);
    const bool done = emu_ops_dh_1_8(d, op, q, J, Mx, Gx, asada) || emu_ops_dh_9_11(d, op, q, J, Mx, Gx, asada) || emu_ops_dh_12_13(d, op, q, J, Mx, Gx, asada) ||
                      emu_ops_dh_14(d, op, q, J, Mx, Gx, asada) || emu_ops_dh_15(d, op, q, J, Mx, Gx, asada) || emu_ops_dh_16(d, op, q, J, Mx, Gx, asada);
    return done ? 0 : -4;
}

extern "C" int emu_tree_opspace(const rtbhip_tree_group *groups, int ng, const double *q, const double *J, int64_t N, const double *grav3, int axes,
                                double *Mx, double *Gx, double *asada)
{
    Tree t;
    if (compile_tree(groups, ng, &t) != RTBHIP_OK) return -1;
    for (int j = 0; j < t.n; ++j)
        if (jm_jq(t.groups[j].jmeta) != j) return -2;          // rtbhip_tree_opspace's refusal
    if (t.n < 1 || t.n > kOpsMaxJoints) return -3;
    const OpsParams op = params_of(t.n, N, grav3, axes, Mx, Gx, asada);
    const bool done = emu_ops_tree_1_9(&t, op, q, J, Mx, Gx, asada) || emu_ops_tree_10_13(&t, op, q, J, Mx, Gx, asada) || emu_ops_tree_14_16(&t, op, q, J, Mx, Gx, asada);
    return done ? 0 : -4;
}

// the branch slots tree.cpp's compiler gives a group table (-1: refused)
extern "C" int emu_tree_nslots(const rtbhip_tree_group *groups, int ng)
{
    Tree t;
    return compile_tree(groups, ng, &t) == RTBHIP_OK ? t.nslots : -1;
}

// the row layout and tile size the kernels use (for the tests' own statements about LDS)
extern "C" void emu_opspace_layout(int n, int packed, int q_in_tile, int *out5)
{
    const OpsLayout L = ops_layout(n, packed != 0, q_in_tile != 0);
    out5[0] = L.wm; out5[1] = L.q_off; out5[2] = L.j_off; out5[3] = L.g_off; out5[4] = L.stride;
}
extern "C" void emu_opspace_set_tile_limit(int64_t bytes) { emu_ops_tile_limit = bytes; }
extern "C" int emu_opspace_tile_rows(int doubles_per_row) { return tile_rows(doubles_per_row); }
// (workgroups, rows per tile, doubles per row) of the last replayed launch
extern "C" void emu_opspace_last_launch(int64_t *out3) { for (int i = 0; i < 3; ++i) out3[i] = emu_ops_last[i]; }
#endif
