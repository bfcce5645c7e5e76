// tests/emu_vjp_tile/emu_vjp_tile.cpp -- TEST INFRASTRUCTURE: the tile phases of the adjoint kernels (csrc/vjp_tile.h) run for lanes 0..63 in a
// loop on the CPU, one loop per stretch between two of the kernel's barriers, so that tests/test_vjp_tile_emu.py can hold their index arithmetic
// to a model of the layout where no GPU exists.  The two entry points are what a kernel's tile function does before and after its lane body; the
// lane body itself is the test's: it fills the result slots with known values between the two calls.
#include "../../robotics-toolbox-python_amd/csrc/vjp_tile.h"

using namespace rtbhip;

namespace {

enum { kMatNone = 0, kMatFolded = 2 };

// src: the A column blocks of the WHOLE batch (NULL: absent), gm its (N, n, n) block; the matrix goes behind the columns (off = A n)
template <int NJ, int A, class S, bool OPT>
void stage(int n, int mat, int64_t tile, int64_t N, int stride, const void *const *src, const double *gm, double *lds)
{
    const VjpTile t = vjp_tile_of(tile, N, n);
    const S *in[A];
    for (int a = 0; a < A; ++a) in[a] = src[a] ? (const S *)src[a] + t.cfg0 * n : nullptr;
    const S *const(&blocks)[A] = in;
    const double *mg = gm ? gm + t.cfg0 * n * n : nullptr;
    const int off = A * n;
    static VjpCols<NJ, A, S> cols[kWave];
    static VjpMat<NJ> m[kWave];
    for (int lane = 0; lane < kWave; ++lane) {
        vjp_load_cols<NJ, OPT>(blocks, t, lane, cols[lane]);
        if (mat != kMatNone) vjp_load_mat<NJ>(mg, t, lane, m[lane]);
        vjp_stage_cols<NJ, OPT>(blocks, t, n, stride, lane, cols[lane], lds);
        if (mat == kMatFolded) vjp_fold<NJ, false>(mg, t, n, stride, off, lane, m[lane], lds);
    }
    // (the kernel's barrier)
    if (mat == kMatFolded)
        for (int lane = 0; lane < kWave; ++lane) vjp_fold<NJ, true>(mg, t, n, stride, off, lane, m[lane], lds);
}

template <int NJ, int A, class S>
int stage_opt(int opt, int n, int mat, int64_t tile, int64_t N, int stride, const void *const *src, const double *gm, double *lds)
{
    if (opt) stage<NJ, A, S, true>(n, mat, tile, N, stride, src, gm, lds);
    else stage<NJ, A, S, false>(n, mat, tile, N, stride, src, gm, lds);
    return 0;
}

template <int NJ>
int stage_nj(int A, int is_float, int opt, int n, int mat, int64_t tile, int64_t N, int stride, const void *const *src, const double *gm, double *lds)
{
    if (is_float) return A == 4 ? stage_opt<NJ, 4, float>(opt, n, mat, tile, N, stride, src, gm, lds) : -1;
    switch (A) {
    case 1: return stage_opt<NJ, 1, double>(opt, n, mat, tile, N, stride, src, gm, lds);
    case 2: return stage_opt<NJ, 2, double>(opt, n, mat, tile, N, stride, src, gm, lds);
    case 4: return stage_opt<NJ, 4, double>(opt, n, mat, tile, N, stride, src, gm, lds);
    }
    return -1;
}

// dst: the B result blocks of the WHOLE batch (NULL: not wanted)
template <int NJ, int B, class S, bool OPT>
void flush(int n, int64_t tile, int64_t N, int stride, void *const *dst, const double *lds)
{
    const VjpTile t = vjp_tile_of(tile, N, n);
    S *out[B];
    for (int b = 0; b < B; ++b) out[b] = dst[b] ? (S *)dst[b] + t.cfg0 * n : nullptr;
    S *const(&blocks)[B] = out;
    for (int lane = 0; lane < kWave; ++lane) vjp_tile_flush<NJ, OPT>(blocks, t, n, stride, lane, lds);
}

template <int NJ, int B>
int flush_b(int is_float, int opt, int n, int64_t tile, int64_t N, int stride, void *const *dst, const double *lds)
{
    if (is_float) {
        if (opt) flush<NJ, B, float, true>(n, tile, N, stride, dst, lds);
        else flush<NJ, B, float, false>(n, tile, N, stride, dst, lds);
    } else {
        if (opt) flush<NJ, B, double, true>(n, tile, N, stride, dst, lds);
        else flush<NJ, B, double, false>(n, tile, N, stride, dst, lds);
    }
    return 0;
}

template <int NJ>
int flush_nj(int B, int is_float, int opt, int n, int64_t tile, int64_t N, int stride, void *const *dst, const double *lds)
{
    switch (B) {
    case 1: return flush_b<NJ, 1>(is_float, opt, n, tile, N, stride, dst, lds);
    case 2: return flush_b<NJ, 2>(is_float, opt, n, tile, N, stride, dst, lds);
    case 3: return flush_b<NJ, 3>(is_float, opt, n, tile, N, stride, dst, lds);
    }
    return -1;
}

}  // namespace

// nj: the compile-time joint count (1, 3, 8) or 0 for the run-time-n form of n joints.  Returns -1 for a form this library was not built with.
extern "C" int emu_vjp_tile_stage(int nj, int n, int A, int is_float, int opt, int mat, int64_t tile, int64_t N, int stride, const void *const *src,
                                  const double *gm, double *lds)
{
    if ((nj != 0 && nj != n) || (mat != kMatNone && mat != kMatFolded)) return -1;
    switch (nj) {
    case 0: return stage_nj<0>(A, is_float, opt, n, mat, tile, N, stride, src, gm, lds);
    case 1: return stage_nj<1>(A, is_float, opt, n, mat, tile, N, stride, src, gm, lds);
    case 3: return stage_nj<3>(A, is_float, opt, n, mat, tile, N, stride, src, gm, lds);
    case 8: return stage_nj<8>(A, is_float, opt, n, mat, tile, N, stride, src, gm, lds);
    }
    return -1;
}

extern "C" int emu_vjp_tile_flush(int nj, int n, int B, int is_float, int opt, int64_t tile, int64_t N, int stride, void *const *dst, const double *lds)
{
    if (nj != 0 && nj != n) return -1;
    switch (nj) {
    case 0: return flush_nj<0>(B, is_float, opt, n, tile, N, stride, dst, lds);
    case 1: return flush_nj<1>(B, is_float, opt, n, tile, N, stride, dst, lds);
    case 3: return flush_nj<3>(B, is_float, opt, n, tile, N, stride, dst, lds);
    case 8: return flush_nj<8>(B, is_float, opt, n, tile, N, stride, dst, lds);
    }
    return -1;
}
