// tests/emu_tree_rne_vjp/emu_tree_rne_vjp.cpp -- TEST INFRASTRUCTURE: the per-lane body of k_tree_rne_vjp (csrc/tree_rne_vjp_kernels.hip:
// tree_rne_vjp_lane) run sample by sample on the CPU, so that tests/test_tree_rne_vjp_emu.py can hold the adjoint algebra against the oracle where
// no GPU exists.  Built by that test into a library of its own, linked against tests/emu/libemu.so for the group-table compiler and the handle
// registry (rtbhip_tree_create, tree_from_handle).
#define RTB_TREE_RNE_VJP_LANE_ONLY 1
#include "../../robotics-toolbox-python_amd/csrc/tree_rne_vjp_kernels.hip"

#include <algorithm>
#include <vector>

using namespace rtbhip;

template <int NG>
static void vjp_run(const Tree *t, const double *q, const double *qd, const double *qdd, int64_t N, V3 g, const double *gtau, double *gq, double *gqd,
                    double *gqdd)
{
    const DevGroup *groups = t->groups.data();
    const int n = t->n;
    std::vector<double> slots((size_t)kTreeSlotDoubles * std::max(1, t->nslots));
    std::vector<double> row(3 * (size_t)n);
    for (int64_t s = 0; s < N; ++s) {
        // as the kernel: the gradients overwrite the q, qd, qdd slots of the sample's row
        double *a = row.data(), *b = a + n, *c = b + n;
        const double *e = gtau + s * n;
        for (int j = 0; j < n; ++j) { a[j] = q[s * n + j]; b[j] = qd ? qd[s * n + j] : 0.0; c[j] = qdd ? qdd[s * n + j] : 0.0; }
        std::fill(slots.begin(), slots.end(), -7.0e300);      // nothing may be read from a slot before this sample wrote it
        tree_rne_vjp_lane<NG>(groups, n, t->nslots, g, [&](int j) { return a[j]; }, [&](int j) { return b[j]; }, [&](int j) { return c[j]; },
                              [&](int j) { return e[j]; }, [&](int j, double v) { a[j] = v; }, [&](int j, double v) { b[j] = v; },
                              [&](int j, double v) { c[j] = v; }, [&](int i) -> double & { return slots[i]; });
        for (int j = 0; j < n; ++j) { gq[s * n + j] = a[j]; gqd[s * n + j] = b[j]; gqdd[s * n + j] = c[j]; }
    }
}

// force_rt != 0: the run-time-n form whatever the group count.  gq, gqd, gqdd: (N, n) each, all three written.
extern "C" int emu_tree_rne_vjp(rtbhip_tree_t h, const double *q, const double *qd, const double *qdd, int64_t N, const double *grav3,
                                const double *gtau, double *gq, double *gqd, double *gqdd, int force_rt)
{
    const std::shared_ptr<Tree> t_owner = tree_from_handle(h);
    const Tree *t = t_owner.get();
    if (!t) return -1;
    if (t->n < 1 || t->n > kTreeVjpMaxGroups) return -2;
    const V3 g = v3(grav3[0], grav3[1], grav3[2]);
    switch (force_rt ? 0 : t->n) {
    case 1: vjp_run<1>(t, q, qd, qdd, N, g, gtau, gq, gqd, gqdd); break;
    case 2: vjp_run<2>(t, q, qd, qdd, N, g, gtau, gq, gqd, gqdd); break;
    case 3: vjp_run<3>(t, q, qd, qdd, N, g, gtau, gq, gqd, gqdd); break;
    case 4: vjp_run<4>(t, q, qd, qdd, N, g, gtau, gq, gqd, gqdd); break;
    case 5: vjp_run<5>(t, q, qd, qdd, N, g, gtau, gq, gqd, gqdd); break;
    case 6: vjp_run<6>(t, q, qd, qdd, N, g, gtau, gq, gqd, gqdd); break;
    case 7: vjp_run<7>(t, q, qd, qdd, N, g, gtau, gq, gqd, gqdd); break;
    case 8: vjp_run<8>(t, q, qd, qdd, N, g, gtau, gq, gqd, gqdd); break;
    default: vjp_run<0>(t, q, qd, qdd, N, g, gtau, gq, gqd, gqdd); break;
    }
    return 0;
}
