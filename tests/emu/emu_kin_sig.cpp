// tests/emu/emu_kin_sig.cpp -- TEST INFRASTRUCTURE: the per-lane body of k_kin_reg (kin_reg.h: reg_compute) replayed on the CPU in its two
// forms -- the general walk, and the straight-line walk instantiated for a built-in structure signature (kSigPandaETS, kSigPandaURDF, kSigUR) --
// so that tests/test_kin_sig_emu.py can compare their outputs byte by byte where no GPU exists.  Built by that test into a library of its own
// (linked against libemu.so, whose chain registry it uses); see emu_common.h for what the replay is and is not.
#include "emu_common.h"

template <int NJ, SegSig SIG>
static void emu_sig_run(const KinParams &kp, const DevChain &cv, const double *q, int64_t N, double *T, double *J)
{
    for (int64_t cfg = 0; cfg < N; ++cfg) {
        Pose P;
        double jac[6 * NJ];
        if (J) reg_compute<NJ, true, SIG>(kp, cv, q, cfg, P, jac);
        else reg_compute<NJ, false, SIG>(kp, cv, q, cfg, P, jac);
        if (J) for (int k = 0; k < 6 * NJ; ++k) J[cfg * 6 * NJ + k] = jac[k];
        if (T) {
            double row[17];
            reg_stage_T(kp, P, row, 0);
            for (int k = 0; k < 16; ++k) T[cfg * 16 + k] = row[k];
        }
    }
}

// use_sig != 0: the signature instantiation when the chain has a built-in one.  Returns 1 when it ran, 0 when the general walk ran, < 0 on error.
extern "C" int emu_kin_reg_sig(rtbhip_chain_t h, const double *q, int64_t N, const double *base16, int frame, double *T, double *J, int use_sig)
{
    const std::shared_ptr<Chain> c_owner = chain_from_handle(h);
    Chain *c = c_owner.get();
    if (!c || c->n < 1 || c->n > 8) return -1;
    KinParams kp;
    kp.n = c->n; kp.qw = c->q_width; kp.stride = kin_stride(c->n);
    kp.frame = frame; kp.N = N; kp.pad = 0;
    Affine b = aff16(base16), t = aff16(nullptr);
    kp.has_base = b.used;
    for (int i = 0; i < 12; i++) kp.base[i] = b.v[i];
    chain_tail(c, t, kp.tail);
    const DevChain cv = chain_host_view(c);
    bool plain = true;
    for (int j = 0; j < c->n; ++j) plain = plain && !jm_prismatic(c->jmeta[j]) && !jm_flip(c->jmeta[j]);
    const SegSig sig = (use_sig && plain) ? chain_signature(c->jmeta.data(), c->n) : 0;
    if (c->n == 7 && sig == kSigPandaETS) { emu_sig_run<7, kSigPandaETS>(kp, cv, q, N, T, J); return 1; }
    if (c->n == 7 && sig == kSigPandaURDF) { emu_sig_run<7, kSigPandaURDF>(kp, cv, q, N, T, J); return 1; }
    if (c->n == 6 && sig == kSigUR) { emu_sig_run<6, kSigUR>(kp, cv, q, N, T, J); return 1; }
    if (c->n == 7) { emu_sig_run<7, 0>(kp, cv, q, N, T, J); return 0; }
    if (c->n == 6) { emu_sig_run<6, 0>(kp, cv, q, N, T, J); return 0; }
    return -2;
}
