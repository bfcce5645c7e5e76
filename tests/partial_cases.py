"""tests/partial_cases.py -- TEST INFRASTRUCTURE shared by tests/test_partial_fkine0.py (not a test module).

Three things, none of which reads the product's code at run time:

  * `partial_ref`: ETS.partial_fkine0 (robot/ETS.py:1862-2013) restated once more, vectorised.  Same term bookkeeping as
    oracle.partial_fkine0 (`add_indices` / `add_pdi`), but every column of an order at once (gathers over np.indices) and
    every configuration of the batch at once, in np.longdouble, from oracle.jacob / oracle.hessian.  The loop oracle takes
    seconds per configuration beyond order 4; this takes a fraction of a second for 9 joints at order 5.
  * the launch geometry of csrc/partial_kernels.hip restated in Python (`blocks_per_group`, `partial3_geometry`, `launch`):
    which kernel a call's last launch is, its grid, its LDS bytes, how many configurations a workgroup touches.  The tests
    assert it against rtbhip.last_launch(), so a retune of the geometry fails a test instead of quietly moving a case
    off the path it was chosen for.
  * the case table: the smallest (joints, order, batch) shapes that reach each path.
"""
import functools
import math

import numpy as np

BLOCK, U_GENERAL, STAGE_DOUBLES = 256, 2, 2560          # kPartialBlock, kPartialU, kPartialStage
TILE3_BYTES, MAX_U3 = 36 * 1024, 4                      # kPartial3TileBytes, kPartial3MaxU


# ---------------------------------------------------------------- the reference
def partial_ref(ch, q, order, tool=None, dtype=np.longdouble):
    """(N, n, ..., 6, n): the order-`order` tensor of every row of q (order >= 2).  dT[c][..., l, k, :, j] from the product
    rule on H[k, :, j] = J_w[:, k] x J[:, j]; a term is (positions of the first factor's indices in the digit vector
    (j, k, l, ...), positions of the second factor's), its first position the column, the others the leading indices."""
    from oracle import oracle
    q = np.asarray(q, dtype=np.float64).reshape(-1, ch.n)
    n = ch.n
    dT = [np.asarray(oracle.jacob(ch, q, tool, 0), dtype=dtype), np.asarray(oracle.hessian(ch, q, tool, 0), dtype=dtype)]
    terms = [([1], [0])]
    while len(dT) < order:
        c = len(dT) + 1
        nxt = []
        for a, b in terms:
            nxt.append((a + [c - 1], b))
            nxt.append((a, b + [c - 1]))
        terms = nxt
        grid = np.indices((n,) * c, sparse=True)           # axis k of the grid runs over digit c-1-k: the output's own axis order
        digit = [grid[c - 1 - i] for i in range(c)]

        def columns(pos):
            # the row axis goes last first: a slice BETWEEN advanced indices would send the gathered axes to the front
            t = np.moveaxis(dT[len(pos) - 1], -2, -1)       # (N, leading ..., column, 6)
            return t[(slice(None),) + tuple(digit[i] for i in reversed(pos[1:])) + (digit[pos[0]],)]      # (N, n, ..., n, 6)
        trn = np.zeros((q.shape[0],) + (n,) * c + (3,), dtype=dtype)
        rot = np.zeros_like(trn)
        for a, b in terms:
            wa, cb = columns(a)[..., 3:6], columns(b)
            trn += np.cross(wa, cb[..., 0:3])
            rot += np.cross(wa, cb[..., 3:6])
        dT.append(np.ascontiguousarray(np.moveaxis(np.concatenate([trn, rot], axis=-1), -1, -2)))
    return dT[order - 1]


# ---------------------------------------------------------------- the launch geometry, restated
def blocks_per_group(n):
    """partial_blocks_per_group: (6, n) blocks per 256 lanes, rounded down to whole 128-byte lines of 48 n bytes per block"""
    per = BLOCK // n
    m = 8 // math.gcd(3 * n, 8)
    return per - per % m if per >= m else per


def partial3_geometry(n):
    """partial3_geometry: (G configurations per workgroup, U columns per lane); G = 0: the general kernel"""
    cols = n ** 3
    g = min(TILE3_BYTES // (48 * cols), BLOCK * MAX_U3 // cols)
    return (0, 0) if g < 1 else (g, (g * cols + BLOCK - 1) // BLOCK)


def launch(n, order, N, partial3=True):
    """What launch_partial does for the order-`order` tensor of N configurations of an n-joint chain: a dict with
    kernel ("k_partial3" / "k_partial"), grid, lds (bytes of dynamic LDS) and
      k_partial3: G, U
      k_partial:  per, perU, bpc (blocks per configuration), stage_cfgs (0: the Jacobians and Hessians are read from global
                  memory), K (the set of configuration counts its workgroups touch), idle (lanes that own no column)."""
    G, U = partial3_geometry(n)
    if order == 3 and partial3 and G > 0 and 6 * n ** 3 * G < 1 << 24:
        lds = (((G * 6 * n ** 3 + 1) & ~1) + G * (6 * n + 6 * n * n)) * 8
        return dict(kernel="k_partial3", grid=(N + G - 1) // G, lds=lds, G=G, U=U)
    per = blocks_per_group(n)
    perU = per * U_GENERAL
    bpc = n ** (order - 1)
    stage_cfgs = (perU + bpc - 2) // bpc + 1
    if stage_cfgs * (6 * n + 6 * n * n) > STAGE_DOUBLES:
        stage_cfgs = 0
    grid = (N * bpc + perU - 1) // perU
    K = set()
    for b in range(grid):
        b0 = b * perU
        nb = min(perU, N * bpc - b0)
        lb0 = b0 % bpc
        K.add((lb0 + nb - 1) // bpc + 1)
    lds = (((perU * 6 * n + 1) & ~1) + stage_cfgs * (6 * n + 6 * n * n)) * 8
    return dict(kernel="k_partial", grid=grid, lds=lds, per=per, perU=perU, bpc=bpc, stage_cfgs=stage_cfgs, K=K, idle=BLOCK - per * n)


# ---------------------------------------------------------------- the cases
def _around(w):
    return sorted({max(1, w - 1), w, w + 1, 2 * w + 1})


def _covers(n, order):
    """configurations one workgroup of the general kernel covers (rounded up: a workgroup that ends inside one touches it)"""
    g = launch(n, order, 1)
    return -(-g["perU"] // g["bpc"])


# path -> [(joints, order, batch sizes)]
TABLE = {
    # k_partial3, G > 1: a lone row, a ragged last workgroup, a full one, one row more, two workgroups and a row
    "k3_many": [(n, 3, sorted({1} | set(_around(partial3_geometry(n)[0])))) for n in (1, 2, 3, 5, 7)],
    # k_partial3, G = 1: U = 2 and U = 3 columns per lane
    "k3_one": [(8, 3, [1, 3]), (9, 3, [1, 3])],
    # k_partial<3>, staged, lanes idle (256 % n != 0)
    "gen3_staged": [(10, 3, [1, 2, 5]), (11, 3, [1, 2, 5]), (13, 3, [1, 2, 5])],
    # k_partial<3..6>, Jacobians and Hessians from global memory: long chains, and the one-joint chain's 512 configurations per workgroup
    "unstaged": [(15, 3, [1, 3]), (16, 3, [1, 3]), (15, 4, [1, 3]), (16, 4, [1, 3]), (24, 3, [1, 2])]
                + [(1, c, [1, 511, 512, 513, 1025]) for c in (4, 5, 6)],
    # k_partial<4..6>, many staged configurations per workgroup
    "many_staged": [(n, c, _around(_covers(n, c))) for n, c in ((2, 4), (2, 5), (2, 6), (3, 4), (4, 4))],
    # k_partial<4..6>, workgroups that straddle two configurations
    "straddle": [(n, c, [1, 2, 3]) for n, c in ((5, 4), (7, 4), (9, 4), (12, 4), (14, 4), (6, 5), (9, 5), (3, 6), (5, 6))],
}

CASES = [(path, n, c, N) for path, rows in TABLE.items() for n, c, Ns in rows for N in Ns]
SHAPES = sorted({(n, c) for _, n, c, _ in CASES})
CASE_IDS = ["%s-n%d-o%d-N%d" % c for c in CASES]

# one case per row of the table, at the largest batch of its row: the bit-for-bit properties
PROPERTY_CASES = [(2, 3, 193), (9, 3, 3), (11, 3, 5), (15, 4, 3), (1, 5, 1025), (3, 4, 13), (6, 5, 3)]


@functools.lru_cache(maxsize=None)
def problem(n, order):
    """-> (spec, oracle chain, tool or None, q for the largest batch of the shape): a random chain as the fuzzers build them
    (every transform kind, flips, SE3 constants), one seed per shape, a tool for every other shape, q ~ U(-2.5, 2.5)."""
    from oracle import chains
    from test_random_chains import random_spec
    rng = np.random.default_rng(77000 + 100 * n + order)
    spec = random_spec(rng, n)
    tool = None
    if (n + order) % 2:
        tool = chains.elementary("tx", rng.uniform(-0.2, 0.2)) @ chains.elementary("Rx", rng.uniform(-1, 1)) @ chains.elementary("tz", 0.15)
    Nmax = max([N for _, m, c, N in CASES if (m, c) == (n, order)] + [N for m, c, N in PROPERTY_CASES if (m, c) == (n, order)])
    q = rng.uniform(-2.5, 2.5, (Nmax, n))
    q.setflags(write=False)
    return spec, chains.Chain(spec, name="partial-n%d-o%d" % (n, order)), tool, q


@functools.lru_cache(maxsize=4)
def reference(n, order):
    """the long-double reference of problem(n, order)'s whole batch (read-only); a smaller batch of the shape is its first rows"""
    _, ch, tool, q = problem(n, order)
    ref = partial_ref(ch, q, order, tool=tool)
    ref.setflags(write=False)
    return ref
