// opspace_device.h -- per-lane tail and tile phases of the OPERATIONAL-SPACE kernels (opspace_kernels.hip, tree_opspace_kernels.hip): for ONE
// configuration, with the joint-space inertia matrix M(q) in the lane's LDS row (the unit-acceleration passes of dyn_device.h / tree_device.h), the
// gravity torques g(q) in registers and a supplied Jacobian J (6, n) beside M, what the reference's Dynamics.inertia_x / gravload_x
// (robot/Dynamics.py:924-1025, 1173-1290) and Asada's manipulability measure (robot/Robot.py:871-881) compute with X = pinv(J):
//     Mx = X^T M X (6, 6)        Gx = X^T g (6)        asada = lambda_min / lambda_max of the sub-block of Mx the axes mask selects, 0 without full rank
// X is never formed.  With K = min(6, n) one K x K system matrix S is factored once and applied as solves:
//     n = 6   S = J^T, LU with partial pivoting (X = J^-1):                 Mx = S^-1 M S^-T               Gx = S^-1 g
//     n > 6   S = J J^T, LDL^T (X = J^T S^-1):                              Mx = S^-1 (J M J^T) S^-T       Gx = S^-1 (J g)
//     n < 6   S = J^T J, LDL^T (X = S^-1 J^T):                              Mx = J (S^-1 M S^-T) J^T       Gx = J (S^-1 g)
// each sandwich  S^-1 B S^-T  as 2 K solves (rows of B, then columns of the result).  A zero or non-finite pivot leaves the row non-finite or huge;
// nothing is repaired (rtbhip_ik_vjp's policy): numpy's SVD-truncated pinv at a rank-deficient J is not reproduced.
// Asada's rank test: the eigenvalues of J J^T (cyclic Jacobi, ldl.h); deficient when lambda_min <= max(6, n) eps lambda_max -- the rounding floor
// of a Gram matrix, coarser than numpy.linalg.matrix_rank's test on singular values (DESIGN.md has the band and why it does not matter).  n < 6
// is always deficient, as matrix_rank(J) < 6 is.  The selected sub-block is symmetrised before its Jacobi sweeps.
// __host__ __device__ and without barriers, so tests/emu_opspace runs the same code lane by lane on the CPU.
#pragma once
#include "kin_device.h"
#include "dyn_device.h"
#include "tree_device.h"

namespace rtbhip {
#pragma clang fp contract(off)      // every operation written out, as in dyn_device.h

enum { kOpsMx = 1, kOpsGx = 2, kOpsAsada = 4 };
constexpr int kOpsMaxJoints = 16;       // compile-time pass sizes 1..16, as the forward inertia kernels
constexpr int kOpsRegMax = 8;           // the tail reads J, M and g with static indices up to here; 9..16: the run-time-n tail
constexpr int kOpsOutW = 43;            // a finished row in LDS: Mx (36) | Gx (6) | asada (1)

struct OpsParams {
    int32_t n, axes, want, tile;        // axes: bit r = row r of the task space is selected (Asada); want: kOps* bits; tile: rows per single-wave workgroup
    int64_t N;
    double grav[3];
};

// one lane's LDS row (doubles): [M: wm | q: n unless it lives in the M tile | J: 6 n | g: n, run-time-n tail only], at an odd stride that also
// holds a finished row
struct OpsLayout { int wm, q_off, j_off, g_off, stride; };
RTB_HD constexpr OpsLayout ops_layout(int n, bool packed, bool q_in_tile)
{
    OpsLayout L = {0, 0, 0, 0, 0};
    L.wm = packed ? n * (n + 1) / 2 : n * n;
    L.q_off = q_in_tile ? 0 : L.wm;
    L.j_off = L.wm + (q_in_tile ? 0 : n);
    L.g_off = L.j_off + 6 * n;
    const int used = L.g_off + (n > kOpsRegMax ? n : 0);
    L.stride = (used > kOpsOutW ? used : kOpsOutW) | 1;
    return L;
}
// rows per workgroup: 64, or fewer where 64 rows (and a tree's branch slots) exceed a compute unit's 160 KB of LDS
RTB_HD constexpr int ops_tile_rows(int doubles_per_row)
{
    int t = kWave;
    while (t > 8 && (size_t)doubles_per_row * t * sizeof(double) > 160 * 1024) t /= 2;
    return t;
}

// ---- tile phases.  src / dst: the block of THIS tile; count: its live elements (live rows x W)
// W doubles per row -> lds[row * stride + off + col], coalesced, sixteen loads in flight; rows past the ragged tail become zeros
template <int W>
RTB_HD void ops_fill(const double *__restrict__ src, int count, int tile, double *lds, int stride, int off, int lane)
{
#pragma unroll
    for (int k0 = 0; k0 < W; k0 += 16) {
        double r[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int f = lane + kWave * (k0 + k);
            r[k] = (k0 + k < W && f < count) ? src[f] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int f = lane + kWave * (k0 + k);
            const int row = f / W;
            if (k0 + k < W && row < tile) lds[row * stride + off + (f - row * W)] = r[k];
        }
    }
}
// lds[row * stride + off + col] -> one contiguous run of live rows x w doubles
RTB_HD void ops_flush(const double *lds, int stride, int off, int w, int count, double *__restrict__ dst, int lane)
{
    for (int f = lane; f < count; f += kWave) {
        const int row = f / w;
        dst[f] = lds[row * stride + off + (f - row * w)];
    }
}
RTB_HD void ops_flush_all(const OpsParams &op, const double *lds, int stride, int ncfg, int64_t cfg0, double *Mx, double *Gx, double *asada, int lane)
{
    if (Mx) ops_flush(lds, stride, 0, 36, ncfg * 36, Mx + cfg0 * 36, lane);
    if (Gx) ops_flush(lds, stride, 36, 6, ncfg * 6, Gx + cfg0 * 6, lane);
    if (asada) ops_flush(lds, stride, 42, 1, ncfg, asada + cfg0, lane);
}

// ---- K x K solvers on registers
// P A = L U with partial pivoting (what numpy.linalg.inv does through LAPACK getrf): the row exchange is det_lu's compare-and-swap chain
// (ldl.h) on WHOLE rows, so the stored multipliers travel with their rows; sw[k][i] remembers the exchanges for the right-hand sides
template <int K>
RTB_HD void ops_lu_factor(double (&a)[K][K], bool (&sw)[K][K])
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int i = k + 1; i < K; ++i) {
            const bool s = fabs(a[i][k]) > fabs(a[k][k]);
            sw[k][i] = s;
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const double u = a[k][c], v = a[i][c];
                a[k][c] = s ? v : u;
                a[i][c] = s ? u : v;
            }
        }
        const double piv = a[k][k];
#pragma unroll
        for (int i = k + 1; i < K; ++i) {
            const double f = a[i][k] / piv;
            a[i][k] = f;
#pragma unroll
            for (int c = k + 1; c < K; ++c) a[i][c] -= f * a[k][c];
        }
    }
}
template <int K>
RTB_HD void ops_lu_solve(const double (&a)[K][K], const bool (&sw)[K][K], double (&b)[K])      // b becomes the solution
{
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int i = k + 1; i < K; ++i) {
            const double u = b[k], v = b[i];
            b[k] = sw[k][i] ? v : u;
            b[i] = sw[k][i] ? u : v;
        }
#pragma unroll
    for (int i = 1; i < K; ++i)
#pragma unroll
        for (int k = 0; k < i; ++k) b[i] -= a[i][k] * b[k];
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
#pragma unroll
        for (int k = i + 1; k < K; ++k) b[i] -= a[i][k] * b[k];
        b[i] = b[i] / a[i][i];
    }
}

// B <- S^-1 B S^-T: the K rows of B solved, then the K columns of what they left
template <int K, class Solve>
RTB_HD void ops_sandwich(Solve solve, double (&B)[K][K])
{
    double b[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
#pragma unroll
        for (int c = 0; c < K; ++c) b[c] = B[r][c];
        solve(b);
#pragma unroll
        for (int c = 0; c < K; ++c) B[r][c] = b[c];
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
#pragma unroll
        for (int r = 0; r < K; ++r) b[r] = B[r][c];
        solve(b);
#pragma unroll
        for (int r = 0; r < K; ++r) B[r][c] = b[r];
    }
}

// lambda_min / lambda_max of the symmetrised sub-block of Mx the mask selects: the rows outside it are zeroed -- the Jacobi rotations leave a pair
// with a zero off-diagonal element alone (ldl.h), so their diagonal slots stay out of it and are skipped below
RTB_HD double ops_asada_ratio(const double (&Mx)[6][6], int axes)
{
    double a[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const bool in = ((axes >> r) & 1) && ((axes >> c) & 1);
            a[r][c] = in ? 0.5 * (Mx[r][c] + Mx[c][r]) : 0.0;
        }
    jacobi_eigenvalues<6>(a);
    double lo = 0.0, hi = 0.0;
    bool any = false;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        if (!((axes >> r) & 1)) continue;               // wave-uniform
        const double e = a[r][r];
        lo = any ? (e < lo ? e : lo) : e;
        hi = any ? (e > hi ? e : hi) : e;
        lo = e != e ? e : lo;                            // a non-finite row stays non-finite
        any = true;
    }
    return lo / hi;
}
// G = J J^T (full, symmetric) has full rank above the rounding floor of a Gram matrix
RTB_HD bool ops_full_rank(const double (&G)[6][6], int n)
{
    double a[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) a[r][c] = G[r][c];
    jacobi_eigenvalues<6>(a);
    double lo = a[0][0], hi = a[0][0];
#pragma unroll
    for (int r = 1; r < 6; ++r) { lo = a[r][r] < lo ? a[r][r] : lo; hi = a[r][r] > hi ? a[r][r] : hi; }
    const double floor_ = (double)(n > 6 ? n : 6) * 2.220446049250313e-16 * hi;
    return !(lo <= floor_);                              // (a NaN is not "deficient": the row stays non-finite)
}

// ---- the tail.  NJ > 0: compile-time n, every index static (g in registers through gat); NJ = 0: run-time n > 6, the contractions over the
// joints are rolled loops on the LDS row.  Mat(r, c) = M[r][c], Jat(r, c) = J[r][c], gat(c) = g[c]; out: the finished row (kOpsOutW doubles),
// which may overlay what Mat / Jat read -- it is written last.
template <int NJ, class MatF, class JatF, class GatF>
RTB_HD void ops_tail(int n_rt, MatF Mat, JatF Jat, GatF gat, int want, int axes, double *out)
{
    const int n = NJ > 0 ? NJ : n_rt;
    const bool want_m = (want & (kOpsMx | kOpsAsada)) != 0, want_g = (want & kOpsGx) != 0, want_a = (want & kOpsAsada) != 0;      // wave-uniform
    double Mx[6][6], Gx[6], ratio = 0.0;
    if constexpr (NJ > 0 && NJ < 6) {
        // left Gram path: S = J^T J (n x n)
        double S[NJ][NJ], W[NJ][NJ], w[NJ], dval[NJ], dinv[NJ];
#pragma unroll
        for (int r = 0; r < NJ; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) acc += Jat(k, r) * Jat(k, c);
                S[r][c] = acc;
                S[c][r] = acc;
            }
        ldl_factor<NJ>(S, dval, dinv);
        auto solve = [&](double (&b)[NJ]) {
            double x[NJ];
            ldl_backsolve<NJ>(S, dinv, b, x);
#pragma unroll
            for (int k = 0; k < NJ; ++k) b[k] = x[k];
        };
        if (want_m) {
#pragma unroll
            for (int r = 0; r < NJ; ++r)
#pragma unroll
                for (int c = 0; c < NJ; ++c) W[r][c] = Mat(r, c);
            ops_sandwich<NJ>(solve, W);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double t[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    double acc = 0.0;
#pragma unroll
                    for (int i = 0; i < NJ; ++i) acc += Jat(a, i) * W[i][j];
                    t[j] = acc;
                }
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc += t[j] * Jat(b, j);
                    Mx[a][b] = acc;
                }
            }
        }
        if (want_g) {
#pragma unroll
            for (int k = 0; k < NJ; ++k) w[k] = gat(k);
            solve(w);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < NJ; ++i) acc += Jat(a, i) * w[i];
                Gx[a] = acc;
            }
        }
        ratio = 0.0;                                     // matrix_rank(J) < 6 (robot/Robot.py:873)
    } else {
        // S = J^T (n = 6) or J J^T (n > 6); B = M or J M J^T; h = g or J g
        double G[6][6], B[6][6], h[6];
        const bool square = NJ == 6;
        if (want_a || !square) {
            if constexpr (NJ > 0) {
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c <= r; ++c) {
                        double acc = 0.0;
#pragma unroll
                        for (int k = 0; k < NJ; ++k) acc += Jat(r, k) * Jat(c, k);
                        G[r][c] = acc;
                        G[c][r] = acc;
                    }
            } else {
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c < 6; ++c) G[r][c] = 0.0;
#pragma unroll 1
                for (int k = 0; k < n; ++k) {
                    double col[6];
#pragma unroll
                    for (int r = 0; r < 6; ++r) col[r] = Jat(r, k);
#pragma unroll
                    for (int r = 0; r < 6; ++r)
#pragma unroll
                        for (int c = 0; c <= r; ++c) G[r][c] += col[r] * col[c];
                }
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c < r; ++c) G[c][r] = G[r][c];
            }
        }
        const bool ranked = want_a ? ops_full_rank(G, n) : true;
        if (square) {
            if constexpr (NJ == 6) {
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c < 6; ++c) { B[r][c] = want_m ? Mat(r, c) : 0.0; G[r][c] = Jat(c, r); }
#pragma unroll
                for (int r = 0; r < 6; ++r) h[r] = want_g ? gat(r) : 0.0;
            }
        } else {
            // B = (J M) J^T column by column of M: t = J M[:, c] (6 values), B += t J[:, c]^T;  h = J g
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                h[r] = 0.0;
#pragma unroll
                for (int c = 0; c < 6; ++c) B[r][c] = 0.0;
            }
            auto column = [&](int c) {
                double jc[6];
#pragma unroll
                for (int r = 0; r < 6; ++r) jc[r] = Jat(r, c);
                if (want_g) {
                    const double gc = gat(c);
#pragma unroll
                    for (int r = 0; r < 6; ++r) h[r] += jc[r] * gc;
                }
                if (want_m) {
                    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    if constexpr (NJ > 0) {
#pragma unroll
                        for (int k = 0; k < NJ; ++k) {
                            const double m = Mat(k, c);
#pragma unroll
                            for (int r = 0; r < 6; ++r) t[r] += Jat(r, k) * m;
                        }
                    } else {
#pragma unroll 1
                        for (int k = 0; k < n; ++k) {
                            const double m = Mat(k, c);
#pragma unroll
                            for (int r = 0; r < 6; ++r) t[r] += Jat(r, k) * m;
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 6; ++r)
#pragma unroll
                        for (int s = 0; s < 6; ++s) B[r][s] += t[r] * jc[s];
                }
            };
            if constexpr (NJ > 0) {
#pragma unroll
                for (int c = 0; c < NJ; ++c) column(c);
            } else {
#pragma unroll 1
                for (int c = 0; c < n; ++c) column(c);
            }
        }
        if (square) {
            bool sw[6][6];
            ops_lu_factor<6>(G, sw);
            auto solve = [&](double (&b)[6]) { ops_lu_solve<6>(G, sw, b); };
            if (want_m) ops_sandwich<6>(solve, B);
            if (want_g) solve(h);
        } else {
            double dval[6], dinv[6];
            ldl_factor<6>(G, dval, dinv);
            auto solve = [&](double (&b)[6]) {
                double x[6];
                ldl_backsolve<6>(G, dinv, b, x);
#pragma unroll
                for (int k = 0; k < 6; ++k) b[k] = x[k];
            };
            if (want_m) ops_sandwich<6>(solve, B);
            if (want_g) solve(h);
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            Gx[r] = h[r];
#pragma unroll
            for (int c = 0; c < 6; ++c) Mx[r][c] = B[r][c];
        }
        if (want_a) {
            const double e = ops_asada_ratio(Mx, axes);
            ratio = ranked ? e : 0.0;
        }
    }
    if (want & kOpsMx) {
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) out[r * 6 + c] = Mx[r][c];
    }
    if (want_g) {
#pragma unroll
        for (int r = 0; r < 6; ++r) out[36 + r] = Gx[r];
    }
    if (want_a) out[42] = ratio;
}

// the tail on a lane's LDS row.  PACKED: M as the packed lower triangle (entry (r, c), r >= c, at r (r + 1) / 2 + c), mirrored on reading
template <int NJ, bool PACKED>
RTB_HD void ops_tail_row(const OpsLayout &L, double *row, const double (&g)[NJ], int want, int axes)
{
    const double *mA = row, *Jr = row + L.j_off;
    auto Mat = [&](int r, int c) {
        if (PACKED) { const int hi = r > c ? r : c, lo = r > c ? c : r; return mA[hi * (hi + 1) / 2 + lo]; }
        return mA[r * NJ + c];
    };
    auto Jat = [&](int r, int c) { return Jr[r * NJ + c]; };
    if constexpr (NJ <= kOpsRegMax) {
        ops_tail<NJ>(NJ, Mat, Jat, [&](int c) { return g[c]; }, want, axes, row);
    } else {
        double *gr = row + L.g_off;
#pragma unroll
        for (int j = 0; j < NJ; ++j) gr[j] = g[j];
        ops_tail<0>(NJ, Mat, Jat, [&](int c) { return gr[c]; }, want, axes, row);
    }
}

// ---- one configuration of a DH / modified-DH chain: the gravity pass first, its torques kept in registers (how dyn_lane orders kDynAccel's
// full pass), then the n unit-acceleration passes of dyn_lane's inertia mode into the row's M tile, then the tail.
// row: the lane's LDS row (ops_layout(NJ, ALLREV, ALLREV)): an all-revolute chain reads q only for the sines and cosines, before the first pass
// writes over it
template <int NJ, bool MDH, bool ALLREV, class LinksP>
RTB_HD void ops_dh_lane(LinksP links, const OpsLayout &L, double *row, V3 grav, int want, int axes)
{
    const V3 zero = v3(0, 0, 0);
    const double *qsrc = row + L.q_off;
    double *mA = row;
    auto qin = [&](int j) { return qsrc[j]; };
    auto none = [&](int) { return 0.0; };
    double st[NJ], ct[NJ], g[NJ];
    rne_trig<NJ, ALLREV>(links, qin, st, ct);
#pragma unroll
    for (int j = 0; j < NJ; ++j) g[j] = 0.0;
    if (want & kOpsGx) {                                 // wave-uniform
        dyn_opaque<NJ>(st, ct);
        rne_core<NJ, MDH, true, ALLREV, true, false, false>(links, NJ, st, ct, grav, zero, zero, qin, none, none, [&](int j, double v) { g[j] = v; });
#if defined(__HIP_DEVICE_COMPILE__)
        // the pass must be over -- its link state dead -- before the passes below start (dyn_lane)
#pragma unroll
        for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(g[j]));
        sched_fence();
#endif
    }
    const int passes = (want & (kOpsMx | kOpsAsada)) ? NJ : 0;          // Gx alone needs no M (wave-uniform)
#pragma unroll 1
    for (int i = 0; i < passes; ++i) {
        dyn_opaque<NJ>(st, ct);
        if constexpr (ALLREV) {
            rne_core<NJ, MDH, false, true, true, true, false>(links, NJ, st, ct, zero, zero, zero, qin, none, [&](int j) { return j == i ? 1.0 : 0.0; },
                                                            [&](int j, double v) { mA[j * (j + 1) / 2 + i] = v; }, i);
        } else {
            rne_core<NJ, MDH, true, ALLREV, true, false, false>(links, NJ, st, ct, zero, zero, zero, qin, none, [&](int j) { return j == i ? 1.0 : 0.0; },
                                                               [&](int j, double v) { mA[i * NJ + j] = v; });
        }
    }
#if defined(__HIP_DEVICE_COMPILE__)
    sched_fence();
#endif
    ops_tail_row<NJ, ALLREV>(L, row, g, want, axes);
}

// ---- one configuration of a link tree (ETS / URDF robots), numbered in group order: the same three steps on tree_device.h's recursion.
// row: ops_layout(NG, true, false) -- q keeps slots of its own (a prismatic joint reads it in every pass); slot: the branch slots
template <int NG, class GroupsP, class Slot>
RTB_HD void ops_tree_lane(GroupsP groups, int nslots, const OpsLayout &L, double *row, V3 grav, int want, int axes, Slot slot)
{
    const V3 zero = v3(0, 0, 0);
    const double *qsrc = row + L.q_off;
    double *mA = row;
    auto qin = [&](int j) { return qsrc[j]; };
    auto none = [&](int) { return 0.0; };
    double sn[NG], cs[NG], g[NG];
    tree_trig<NG, TreeNothing>(groups, qin, sn, cs);
#pragma unroll
    for (int j = 0; j < NG; ++j) g[j] = 0.0;
    if (want & kOpsGx) {                                 // wave-uniform
        tree_opaque<NG>(sn, cs);
        tree_rne_core<NG, true, TreeNothing>(groups, nslots, sn, cs, grav, qin, none, none, [&](int j, double v) { tree_put<NG>(g, j, v); }, slot);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
        for (int j = 0; j < NG; ++j) asm volatile("" : "+v"(g[j]));
        sched_fence();
#endif
    }
    const int passes = (want & (kOpsMx | kOpsAsada)) ? NG : 0;          // Gx alone needs no M (wave-uniform)
#pragma unroll 1
    for (int i = 0; i < passes; ++i) {
        tree_opaque<NG>(sn, cs);
        tree_rne_core<NG, false, TreeNothing>(groups, nslots, sn, cs, zero, qin, none, [&](int c) { return c == i ? 1.0 : 0.0; },
                                              [&](int j, double v) { if (j >= i) mA[j * (j + 1) / 2 + i] = v; }, slot, i);
    }
#if defined(__HIP_DEVICE_COMPILE__)
    sched_fence();
#endif
    ops_tail_row<NG, true>(L, row, g, want, axes);
}

#pragma clang fp contract(fast)
}  // namespace rtbhip
