// tests/emu_inertia_vjp/emu_inertia_vjp.cpp -- TEST INFRASTRUCTURE: the per-lane bodies of k_inertia_vjp (csrc/inertia_vjp_kernels.hip:
// inertia_vjp_lane) and k_tree_inertia_vjp (csrc/tree_inertia_vjp_kernels.hip: tree_inertia_vjp_lane) run sample by sample on the CPU, so that
// tests/test_inertia_vjp_emu.py can hold the adjoint algebra against the oracle where no GPU exists.  Built by that test into a library of its own,
// linked against tests/emu/libemu.so for the table compilers and the handle registries (rtbhip_dyn_create, rtbhip_tree_create).
#define RTB_INERTIA_VJP_LANE_ONLY 1
#define RTB_TREE_INERTIA_VJP_LANE_ONLY 1
#include "../../robotics-toolbox-python_amd/csrc/inertia_vjp_kernels.hip"
#include "../../robotics-toolbox-python_amd/csrc/tree_inertia_vjp_kernels.hip"

#include <algorithm>
#include <vector>

using namespace rtbhip;

// as the kernel's tile: the folded gradient S(j, i) = gM[j,i] + gM[i,j] (j > i), S(i, i) = gM[i,i], packed at j (j + 1) / 2 + i
static void fold(const double *gM, int n, std::vector<double> &S)
{
    for (int j = 0; j < n; ++j)
        for (int i = 0; i <= j; ++i) S[(size_t)j * (j + 1) / 2 + i] = i == j ? gM[j * n + i] : gM[j * n + i] + gM[i * n + j];
}

template <int NJ, bool MDH>
static void dh_run(const Dyn *d, const double *q, int64_t N, const double *gM, double *gq)
{
    const DevLink *links = d->links.data();
    const int n = d->n;
    std::vector<double> S((size_t)n * (n + 1) / 2);
    for (int64_t s = 0; s < N; ++s) {
        const double *a = q + s * n;
        double *o = gq + s * n;
        fold(gM + s * n * n, n, S);
        inertia_vjp_lane<NJ, MDH>(links, n, [&](int j) { return a[j]; }, [&](int j, int i) { return S[(size_t)j * (j + 1) / 2 + i]; },
                                  [&](int j, double v) { o[j] = v; });
    }
}

template <int NJ>
static void dh_nj(const Dyn *d, const double *q, int64_t N, const double *gM, double *gq)
{
    if (d->mdh) dh_run<NJ, true>(d, q, N, gM, gq);
    else dh_run<NJ, false>(d, q, N, gM, gq);
}

// force_rt != 0: the run-time-n form whatever the joint count.  gM (N, n, n), gq (N, n)
extern "C" int emu_inertia_vjp(rtbhip_dyn_t h, const double *q, int64_t N, const double *gM, double *gq, int force_rt)
{
    const std::shared_ptr<Dyn> d_owner = dyn_from_handle(h);
    const Dyn *d = d_owner.get();
    if (!d) return -1;
    for (const DevLink &l : d->links)
        if (l.sigma != 0) return -2;
    switch (force_rt ? 0 : d->n) {
    case 1: dh_nj<1>(d, q, N, gM, gq); break;
    case 2: dh_nj<2>(d, q, N, gM, gq); break;
    case 3: dh_nj<3>(d, q, N, gM, gq); break;
    case 4: dh_nj<4>(d, q, N, gM, gq); break;
    case 5: dh_nj<5>(d, q, N, gM, gq); break;
    case 6: dh_nj<6>(d, q, N, gM, gq); break;
    case 7: dh_nj<7>(d, q, N, gM, gq); break;
    case 8: dh_nj<8>(d, q, N, gM, gq); break;
    default: dh_nj<0>(d, q, N, gM, gq); break;
    }
    return 0;
}

template <int NG>
static void tree_run(const Tree *t, const double *q, int64_t N, const double *gM, double *gq)
{
    const DevGroup *groups = t->groups.data();
    const int n = t->n;
    std::vector<double> slots((size_t)kTreeSlotDoubles * std::max(1, t->nslots));
    std::vector<double> S((size_t)n * (n + 1) / 2);
    for (int64_t s = 0; s < N; ++s) {
        const double *a = q + s * n;
        double *o = gq + s * n;
        fold(gM + s * n * n, n, S);
        std::fill(slots.begin(), slots.end(), -7.0e300);      // nothing may be read from a slot before this sample wrote it
        tree_inertia_vjp_lane<NG>(groups, n, t->nslots, [&](int j) { return a[j]; }, [&](int j, int i) { return S[(size_t)j * (j + 1) / 2 + i]; },
                                  [&](int j, double v) { o[j] = v; }, [&](int i) -> double & { return slots[i]; });
    }
}

extern "C" int emu_tree_inertia_vjp(rtbhip_tree_t h, const double *q, int64_t N, const double *gM, double *gq, int force_rt)
{
    const std::shared_ptr<Tree> t_owner = tree_from_handle(h);
    const Tree *t = t_owner.get();
    if (!t) return -1;
    if (t->n < 1 || t->n > kTreeInertiaVjpMaxGroups) return -2;
    for (int j = 0; j < t->n; ++j)
        if (jm_jq(t->groups[j].jmeta) != j) return -3;
    switch (force_rt ? 0 : t->n) {
    case 1: tree_run<1>(t, q, N, gM, gq); break;
    case 2: tree_run<2>(t, q, N, gM, gq); break;
    case 3: tree_run<3>(t, q, N, gM, gq); break;
    case 4: tree_run<4>(t, q, N, gM, gq); break;
    case 5: tree_run<5>(t, q, N, gM, gq); break;
    case 6: tree_run<6>(t, q, N, gM, gq); break;
    case 7: tree_run<7>(t, q, N, gM, gq); break;
    case 8: tree_run<8>(t, q, N, gM, gq); break;
    default: tree_run<0>(t, q, N, gM, gq); break;
    }
    return 0;
}
