// tests/emu_rne_vjp/emu_rne_vjp.cpp -- TEST INFRASTRUCTURE: the per-lane body of k_rne_vjp (csrc/rne_vjp_kernels.hip: rne_vjp_lane) run sample by
// sample on the CPU, so that tests/test_rne_vjp_emu.py can hold the adjoint algebra against the oracle where no GPU exists.  Built by that test
// into a library of its own, linked against tests/emu/libemu.so for the link-table compiler and the handle registry (rtbhip_dyn_create).
#define RTB_RNE_VJP_LANE_ONLY 1
#include "../../robotics-toolbox-python_amd/csrc/rne_vjp_kernels.hip"

using namespace rtbhip;

template <int NJ, bool MDH>
static void vjp_run(const Dyn *d, const double *q, const double *qd, const double *qdd, int64_t N, V3 g, V3 f, V3 nt, const double *gtau, double *gq,
                    double *gqd, double *gqdd)
{
    const DevLink *links = d->links.data();
    const int n = d->n;
    for (int64_t s = 0; s < N; ++s) {
        const double *a = q + s * n, *b = qd ? qd + s * n : nullptr, *c = qdd ? qdd + s * n : nullptr, *e = gtau + s * n;
        double *o0 = gq + s * n, *o1 = gqd + s * n, *o2 = gqdd + s * n;
        rne_vjp_lane<NJ, MDH>(links, n, g, f, nt, [&](int j) { return a[j]; }, [&](int j) { return b ? b[j] : 0.0; }, [&](int j) { return c ? c[j] : 0.0; },
                              [&](int j) { return e[j]; }, [&](int j, double v) { o0[j] = v; }, [&](int j, double v) { o1[j] = v; },
                              [&](int j, double v) { o2[j] = v; });
    }
}

template <int NJ>
static void vjp_nj(const Dyn *d, const double *q, const double *qd, const double *qdd, int64_t N, V3 g, V3 f, V3 nt, const double *gtau, double *gq,
                   double *gqd, double *gqdd)
{
    if (d->mdh) vjp_run<NJ, true>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd);
    else vjp_run<NJ, false>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd);
}

// force_rt != 0: the run-time-n form whatever the joint count.  gq, gqd, gqdd: (N, n) each, all three written.
extern "C" int emu_rne_vjp(rtbhip_dyn_t h, const double *q, const double *qd, const double *qdd, int64_t N, const double *grav3, const double *fext6,
                           const double *gtau, double *gq, double *gqd, double *gqdd, int force_rt)
{
    const std::shared_ptr<Dyn> d_owner = dyn_from_handle(h);
    const Dyn *d = d_owner.get();
    if (!d) return -1;
    for (const DevLink &l : d->links)
        if (l.sigma != 0) return -2;
    const V3 g = v3(grav3[0], grav3[1], grav3[2]);
    const V3 f = fext6 ? v3(fext6[0], fext6[1], fext6[2]) : v3(0, 0, 0);
    const V3 nt = fext6 ? v3(fext6[3], fext6[4], fext6[5]) : v3(0, 0, 0);
    switch (force_rt ? 0 : d->n) {
    case 1: vjp_nj<1>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd); break;
    case 2: vjp_nj<2>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd); break;
    case 3: vjp_nj<3>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd); break;
    case 4: vjp_nj<4>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd); break;
    case 5: vjp_nj<5>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd); break;
    case 6: vjp_nj<6>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd); break;
    case 7: vjp_nj<7>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd); break;
    case 8: vjp_nj<8>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd); break;
    default: vjp_nj<0>(d, q, qd, qdd, N, g, f, nt, gtau, gq, gqd, gqdd); break;
    }
    return 0;
}
