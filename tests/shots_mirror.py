"""NumPy restatement of the finite-shot draw function of kernels_shots.hip (not a test module).

Philox4x32-10 (Random123's round function; key = the 64-bit seed, counter = (pair m, (level << 24) | block, circuit id,
epoch mod 2^32)), two 53-bit uniforms per call, and the block hierarchy: a row of 2^n entries is cut into blocks of
2^12, the block masses form the next level, the top level (one block) gets all S draws, a block with m draws picks by
rule R (`pick`; csrc/shots_dev.hpp) for each: with lo0 the first i with cdf[i] > u * cdf[last], the first i >= lo0 whose
value is positive, else the block's last positive entry; a block without a positive entry counts nothing.

Three orders of summation:
  histogram(...)                  one running sum per block (np.cumsum), block masses by np.sum.  Bit for bit the kernel
                                  wherever every partial sum is exact (dyadic rows);
  histogram(..., order="device")  device_cdf / device_mass: float64 in the kernels' own order of additions, so the kernels'
                                  own cdf, thread-boundary rounding included;
  histogram_exact(...)            masses and cdfs in extended precision, inversion on u against cdf / total, and a count of
                                  the draws too close to a boundary for float64 orders of summation to be told apart."""
import numpy as np

import hp_reference as hp

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
BLOCK_BITS = 12
BLOCK = 1 << BLOCK_BITS
DRAW_THREADS, DRAW_EPT = 512, BLOCK // 512          # draw kernel: 8 consecutive entries per thread
MASS_THREADS, MASS_EPT = 256, BLOCK // 256          # mass kernel: entries t, t + 256, ...
LD = np.longdouble if hp.HAVE_LONGDOUBLE else np.float64
MARGIN = 2.0 ** -40                                 # of u in [0, 1): the value test_gpu_mps_sampled_kernel.py uses


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over the counter words (uint32 values in any integer arrays); key words are Python ints."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & MASK32]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return c


def uniforms(seed, epoch, cid, level, block, m):
    """The m uniforms in [0, 1) of one (row, level, block): draws 2j and 2j + 1 come from call j."""
    j = np.arange((m + 1) // 2, dtype=np.uint64)
    w = philox4x32_10(j, (level << 24) | block, cid, int(epoch) & 0xFFFFFFFF, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u0 = ((w[1] << np.uint64(32)) | w[0]) >> np.uint64(11)
    u1 = ((w[3] << np.uint64(32)) | w[2]) >> np.uint64(11)
    u = np.empty(2 * len(j), dtype=np.float64)
    u[0::2] = u0.astype(np.float64) * 2.0 ** -53
    u[1::2] = u1.astype(np.float64) * 2.0 ** -53
    return u[:m]


def device_cdf(vals):
    """The draw kernel's inclusive prefix sums of blocks [..., blk <= 4096], float64 in its order of additions: thread t adds
    entries 8t .. 8t + 7 in order, the 512 thread totals are scanned with offsets 1, 2, ..., 256 (Hillis-Steele), and thread
    t > 0 adds the scanned total of thread t - 1 to each of its running sums."""
    v = np.asarray(vals, dtype=np.float64)
    blk = v.shape[-1]
    pad = np.zeros(v.shape[:-1] + (BLOCK,), dtype=np.float64)
    pad[..., :blk] = v
    run = np.cumsum(pad.reshape(v.shape[:-1] + (DRAW_THREADS, DRAW_EPT)), axis=-1)      # sequential within a thread
    ts = run[..., -1].copy()
    off = 1
    while off < DRAW_THREADS:
        nxt = ts.copy()
        nxt[..., off:] = ts[..., off:] + ts[..., :-off]
        ts = nxt
        off <<= 1
    cdf = run.copy()
    cdf[..., 1:, :] = ts[..., :-1, None] + run[..., 1:, :]
    return cdf.reshape(v.shape[:-1] + (BLOCK,))[..., :blk]


def device_mass(blocks):
    """The mass kernel's sums of blocks [..., 4096], float64 in its order of additions: thread t adds p[t + 256 i] for
    i = 0..15, the xor butterfly 32, 16, ..., 1 inside each wave of 64, then the four wave totals in order."""
    p = np.asarray(blocks, dtype=np.float64)
    lead = p.shape[:-1]
    p = p.reshape(-1, MASS_EPT, MASS_THREADS)
    s = np.zeros((p.shape[0], MASS_THREADS), dtype=np.float64)
    for i in range(MASS_EPT):
        s = s + p[:, i]
    lane = np.arange(MASS_THREADS)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ off]
    tot = np.zeros(p.shape[0], dtype=np.float64)
    for w in range(MASS_THREADS // 64):
        tot = tot + s[:, 64 * w]
    return tot.reshape(lead)


def first_greater(cdf, x):
    """lo0 of rule R: the kernel's bisection for the first i with cdf[i] > x (len(cdf) if none), probe for probe, so that
    it is defined on a cdf that is not monotone to the last bit as well."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    lo = np.zeros(x.shape, dtype=np.int64)
    hi = np.full(x.shape, len(cdf), dtype=np.int64)
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi) >> 1
        gt = cdf[np.minimum(mid, len(cdf) - 1)] > x
        hi = np.where(act & gt, mid, hi)
        lo = np.where(act & ~gt, mid + 1, lo)


def pick(cdf, positive, x):
    """Rule R for every x: the first index >= lo0 whose value is positive, else the block's last positive entry, else -1."""
    lo0 = first_greater(cdf, x)
    nz = np.nonzero(positive)[0]
    if len(nz) == 0:
        return np.full(lo0.shape, -1, dtype=np.int64)
    k = np.searchsorted(nz, lo0, side="left")
    return nz[np.minimum(k, len(nz) - 1)]


def draw_block(vals, m, seed, epoch, cid, level, block, order="sequential", x_of=None):
    """Counts [len(vals)] of the m draws of one block.  x_of(level, block, m, total), if given, replaces u * total."""
    counts = np.zeros(len(vals), dtype=np.int64)
    if m == 0:
        return counts
    cdf = device_cdf(vals) if order == "device" else np.cumsum(vals)
    x = uniforms(seed, epoch, cid, level, block, m) * cdf[-1] if x_of is None else x_of(level, block, m, cdf[-1])
    idx = pick(cdf, vals > 0, x)
    np.add.at(counts, idx[idx >= 0], 1)
    return counts


def circuit_id(r, include_base=True, p_begin=0, p_stride=1):
    if include_base:
        if r == 0:
            return 0
        r -= 1
    p = p_begin + (r >> 1) * p_stride
    return 2 * p + 1 + (r & 1)


def row_counts(row, shots, seed, epoch, cid, order="sequential", x_of=None):
    """Integer counts [2^n] of one row."""
    levels = [np.asarray(row, dtype=np.float64)]
    while len(levels[-1]) > BLOCK:
        blocks = levels[-1].reshape(-1, BLOCK)
        levels.append(device_mass(blocks) if order == "device" else blocks.sum(axis=1))
    m = np.array([shots], dtype=np.int64)                  # draws per block of the current level
    for lv in range(len(levels) - 1, -1, -1):
        vals = levels[lv]
        blk = min(len(vals), BLOCK)
        out = np.zeros(len(vals), dtype=np.int64)
        for b in range(len(vals) // blk):
            if m[b]:
                out[b * blk:(b + 1) * blk] = draw_block(vals[b * blk:(b + 1) * blk], int(m[b]), seed, epoch, cid, lv, b,
                                                        order, x_of)
        m = out
    return m


def histogram(probs, shots, seed, epoch, include_base=True, p_begin=0, p_stride=1, order="sequential"):
    """The mirror of bornvi_shots_histogram: counts [B, 2^n] (int64); frequencies are counts / shots."""
    probs = np.atleast_2d(np.asarray(probs, dtype=np.float64))
    return np.stack([row_counts(probs[r], shots, seed, epoch, circuit_id(r, include_base, p_begin, p_stride), order)
                     for r in range(probs.shape[0])])


def _draw_block_exact(vals, m, seed, epoch, cid, level, block, margin):
    """(counts, undecided) of one block whose values are already in extended precision: inversion of u on cdf / total over
    the positive entries only, so a zero entry owns nothing by construction."""
    counts = np.zeros(len(vals), dtype=np.int64)
    nz = np.nonzero(vals > 0)[0]
    assert len(nz) > 0, "a block without mass received draws"
    F = np.cumsum(vals[nz].astype(LD))
    F = F / F[-1]
    u = uniforms(seed, epoch, cid, level, block, m).astype(LD)
    j = np.minimum(np.searchsorted(F, u, side="right"), len(nz) - 1)
    below = np.where(j > 0, F[np.maximum(j - 1, 0)], LD(-1))               # the boundaries of entry j that lie between two
    above = np.where(j < len(nz) - 1, F[j], LD(2))                         # positive entries; none at either end
    undecided = int(((np.abs(u - below) <= margin) | (np.abs(u - above) <= margin)).sum())
    np.add.at(counts, nz[j], 1)
    return counts, undecided


def row_counts_exact(row, shots, seed, epoch, cid, margin=MARGIN, chunk=256):
    """(counts [2^n], undecided) of one row: block masses summed in extended precision, `chunk` blocks at a time, and draws
    made only inside blocks that received some."""
    row = np.asarray(row, dtype=np.float64)
    levels = [row]
    while len(levels[-1]) > BLOCK:
        below = levels[-1].reshape(-1, BLOCK)
        levels.append(np.concatenate([below[c:c + chunk].astype(LD).sum(axis=1) for c in range(0, len(below), chunk)]))
    m = np.array([shots], dtype=np.int64)
    undecided = 0
    for lv in range(len(levels) - 1, -1, -1):
        vals = levels[lv]
        blk = min(len(vals), BLOCK)
        out = np.zeros(len(vals), dtype=np.int64)
        for b in np.nonzero(m)[0]:
            out[b * blk:(b + 1) * blk], ud = _draw_block_exact(vals[b * blk:(b + 1) * blk], int(m[b]), seed, epoch, cid, lv,
                                                               int(b), margin)
            undecided += ud
        m = out
    return m, undecided


def histogram_exact(probs, shots, seed, epoch, include_base=True, p_begin=0, p_stride=1, margin=MARGIN):
    """The same hierarchy and uniforms in extended precision: (counts [B, 2^n], undecided).  undecided counts the draws, on
    any level, whose u lies within `margin` of a boundary between two positive entries (or two blocks with mass): only for
    those may a float64 order of summation decide otherwise.  A row without a positive entry yields zeros."""
    probs = np.atleast_2d(np.asarray(probs, dtype=np.float64))
    counts, undecided = [], 0
    for r in range(probs.shape[0]):
        if not (probs[r] > 0).any():
            counts.append(np.zeros(probs.shape[1], dtype=np.int64))
            continue
        c, ud = row_counts_exact(probs[r], shots, seed, epoch, circuit_id(r, include_base, p_begin, p_stride), margin)
        counts.append(c)
        undecided += ud
    return np.stack(counts), undecided


# ---- the non-dyadic rows of tests/test_gpu_shots.py, shared with tests/test_shots_host.py ----------------------------------
def real_row(kind, n, rng, zeros=0.5):
    """(a) sparse and peaked: r^4 with a fraction `zeros` of the entries zeroed, normalised; (b) one outcome at 1.0 and the
    rest 1e-9 r; (c) exp(6 normal), normalised, times 3.7 (an unnormalised row over 30 orders of magnitude)."""
    N = 1 << n
    if kind == "a":
        x = rng.random(N) ** 4
        x[rng.random(N) < zeros] = 0.0
        if not x.any():
            x[0] = 0.5
        return x / x.sum()
    if kind == "b":
        x = 1e-9 * rng.random(N)
        x[rng.integers(N)] = 1.0
        return x
    assert kind == "c"
    x = np.exp(6.0 * rng.standard_normal(N))
    return 3.7 * (x / x.sum())


def real_rows(kind, n, seed=0):
    """The rows of one D.1 case: one row of kind (a), B = 3 rows of kinds (b) and (c)."""
    rng = np.random.default_rng([seed, n, ord(kind)])
    return np.stack([real_row(kind, n, rng) for _ in range(1 if kind == "a" else 3)])


def dyadic_row(rng, N, zeros=0.3):
    """A row of multiples of 2^-k summing to exactly 1: every partial sum is exact in any order."""
    a = rng.integers(0, 64, N).astype(np.int64)
    a[rng.random(N) < zeros] = 0
    a[rng.integers(N)] += 1
    K = 1 << int(np.ceil(np.log2(a.sum())))
    a[np.nonzero(a)[0][-1]] += K - a.sum()
    return a / K


REAL_N = (1, 3, 8, 12, 13, 16)          # a block shorter than a thread's 8 entries (1, 3), one full block, 2 and 16 masses
REAL_SHOTS = (1, 2, 1001, 99999)        # a single draw, one pair, an odd tail pair, many draws per block
REAL_SEED, REAL_EPOCH = 12345, 7
STRIDED_IDS = dict(include_base=False, p_begin=5, p_stride=3)
SCALES = (0.0, -600.0, 600.0)           # powers of two applied to the kind-(c) row of the scale test


def level_boundary_row(kind):
    """n = 24: the top level is exactly one full block of 4096 masses.  A dyadic row, or a kind-(a) row with 99 % zeros."""
    if kind == "dyadic":
        return dyadic_row(np.random.default_rng(24), 1 << 24, zeros=0.9)[None]
    return real_row("a", 24, np.random.default_rng(2424), zeros=0.99)[None]


def scale_row():
    return real_rows("c", 13, seed=3)[:1]


def mixed_batch():
    """Five rows of every kind at n = 13 (two masses on the top level)."""
    rng = np.random.default_rng(513)
    return np.stack([real_row("a", 13, rng), real_row("b", 13, rng), real_row("c", 13, rng), real_row("a", 13, rng, zeros=0.97),
                     dyadic_row(rng, 1 << 13)])


def synthetic_cases(large=True):
    """Every synthetic input of the real-row tests of tests/test_gpu_shots.py as (name, make_probs, shots, seed, epoch,
    id keywords): what tests/test_shots_host.py shows to be free of undecided draws before a GPU test relies on it."""
    cases = []
    for n in REAL_N:
        for kind in "abc":
            for S in REAL_SHOTS:
                cases.append((f"real-n{n}-{kind}-S{S}", lambda n=n, kind=kind: real_rows(kind, n), S, REAL_SEED, REAL_EPOCH, {}))
    if large:
        cases.append(("n24-dyadic", lambda: level_boundary_row("dyadic"), 30000, 5, 2, {}))
        cases.append(("n24-sparse", lambda: level_boundary_row("sparse"), 30000, 5, 2, {}))
    for e in SCALES:
        cases.append((f"scale-2^{e:+.0f}", lambda e=e: scale_row() * 2.0 ** e, 20000, 31, 4, {}))
    for kind in "ac":
        cases.append((f"strided-{kind}", lambda kind=kind: np.concatenate([real_rows(kind, 9, seed=s) for s in (1, 2)])[:4],
                      20000, 77, 3, STRIDED_IDS))
    cases.append(("mixed-batch", mixed_batch, 20000, 99, 11, {}))
    return cases
