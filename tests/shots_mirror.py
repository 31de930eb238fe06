"""NumPy restatement of the finite-shot draw function of kernels_shots.hip (not a test module).

Philox4x32-10 (Random123's round function; key = the 64-bit seed, counter = (pair m, (level << 24) | block, circuit id,
epoch mod 2^32)), two 53-bit uniforms per call, and the block hierarchy: a row of 2^n entries is cut into blocks of
2^12, the block masses form the next level, the top level (one block) gets all S draws, a block with m draws picks
"first i with cdf[i] > u * cdf[last]" (else its last non-zero entry) for each.  The counts equal the kernel's bit for
bit wherever every partial sum is exact (dyadic rows); elsewhere they differ only through the summation order."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
BLOCK_BITS = 12
BLOCK = 1 << BLOCK_BITS


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


def draw_block(vals, m, seed, epoch, cid, level, block):
    """Counts [len(vals)] of the m draws of one block."""
    counts = np.zeros(len(vals), dtype=np.int64)
    if m == 0:
        return counts
    cdf = np.cumsum(vals)
    x = uniforms(seed, epoch, cid, level, block, m) * cdf[-1]
    idx = np.searchsorted(cdf, x, side="right")            # first i with cdf[i] > x
    nz = np.nonzero(vals > 0)[0]
    last = int(nz[-1]) if len(nz) else -1
    idx[idx >= len(vals)] = last
    idx = idx[idx >= 0]
    np.add.at(counts, idx, 1)
    return counts


def circuit_id(r, include_base=True, p_begin=0, p_stride=1):
    if include_base:
        if r == 0:
            return 0
        r -= 1
    p = p_begin + (r >> 1) * p_stride
    return 2 * p + 1 + (r & 1)


def row_counts(row, shots, seed, epoch, cid):
    """Integer counts [2^n] of one row."""
    levels = [np.asarray(row, dtype=np.float64)]
    while len(levels[-1]) > BLOCK:
        levels.append(levels[-1].reshape(-1, BLOCK).sum(axis=1))
    m = np.array([shots], dtype=np.int64)                  # draws per block of the current level
    for lv in range(len(levels) - 1, -1, -1):
        vals = levels[lv]
        blk = min(len(vals), BLOCK)
        out = np.zeros(len(vals), dtype=np.int64)
        for b in range(len(vals) // blk):
            out[b * blk:(b + 1) * blk] = draw_block(vals[b * blk:(b + 1) * blk], int(m[b]), seed, epoch, cid, lv, b)
        m = out
    return m


def histogram(probs, shots, seed, epoch, include_base=True, p_begin=0, p_stride=1):
    """The mirror of bornvi_shots_histogram: counts [B, 2^n] (int64); frequencies are counts / shots."""
    probs = np.atleast_2d(np.asarray(probs, dtype=np.float64))
    return np.stack([row_counts(probs[r], shots, seed, epoch, circuit_id(r, include_base, p_begin, p_stride))
                     for r in range(probs.shape[0])])
