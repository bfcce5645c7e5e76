// tests/emu_frames_vjp/emu_frames_vjp.cpp -- TEST INFRASTRUCTURE: the per-lane body of k_frames_vjp (csrc/frames_vjp_kernels.hip: frames_vjp_lane)
// run configuration by configuration on the CPU, so that tests/test_link_frames_vjp_emu.py can hold the all-frame adjoint against the oracle where
// no GPU exists.  Built by that test into a library of its own, linked against tests/emu/libemu.so for the chain compiler, the lowering of the
// marks (chain.cpp: compile_frames) and the handle registry (rtbhip_chain_create).
#define RTB_FRAMES_VJP_LANE_ONLY 1
#include "../../robotics-toolbox-python_amd/csrc/frames_vjp_kernels.hip"
#include <cstring>

using namespace rtbhip;

template <int NJ>
static void fv_run(const Chain *c, const FrameTable &ft, const double *q, int64_t N, const double *gF, double *gq)
{
    const DevChain cv = chain_host_view(c);
    const int qw = c->q_width;
    for (int64_t s = 0; s < N; ++s) {
        const double *row = q + s * qw, *g = gF + s * (int64_t)ft.nmarks * 16;
        double *o = gq + s * qw;
        frames_vjp_lane<NJ>(cv, c->n, ft, [&](int k) { return row[k]; }, [](int) {}, [&](int m, int r, int k) { return g[m * 16 + r * 4 + k]; },
                            [&]() { std::memset(o, 0, sizeof(double) * qw); }, [&](int col, double v) { o[col] = o[col] + v; });
    }
}

// force_rt != 0: the run-time-n form whatever the joint count.  gF: (N, nmarks, 4, 4), gq: (N, q_width), nmarks >= 1.
extern "C" int emu_frames_vjp(rtbhip_chain_t h, const double *q, int64_t N, const double *base16, const int32_t *marks, int nmarks, const double *gF,
                              double *gq, int force_rt)
{
    const std::shared_ptr<Chain> c_owner = chain_from_handle(h);
    const Chain *c = c_owner.get();
    if (!c) return -1;
    if (c->n < 1 || c->n > RTBHIP_MAX_JOINTS || nmarks < 1) return -3;
    FrameTable ft;
    if (compile_frames(c, marks, nmarks, &ft) != RTBHIP_OK) return -2;
    ft.has_base = base16 != nullptr;
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 4; k++) ft.base[4 * r + k] = base16 ? base16[4 * r + k] : (r == k ? 1.0 : 0.0);
    switch (force_rt ? 0 : c->n) {
    case 1: fv_run<1>(c, ft, q, N, gF, gq); break;
    case 2: fv_run<2>(c, ft, q, N, gF, gq); break;
    case 3: fv_run<3>(c, ft, q, N, gF, gq); break;
    case 4: fv_run<4>(c, ft, q, N, gF, gq); break;
    case 5: fv_run<5>(c, ft, q, N, gF, gq); break;
    case 6: fv_run<6>(c, ft, q, N, gF, gq); break;
    case 7: fv_run<7>(c, ft, q, N, gF, gq); break;
    case 8: fv_run<8>(c, ft, q, N, gF, gq); break;
    default: fv_run<0>(c, ft, q, N, gF, gq); break;
    }
    return 0;
}
