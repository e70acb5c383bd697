"""The packed rows of the gradient exchange (g4splat_amd/csrc/rows.hip) restated at loop level in numpy, straight from the
words of include/g4s_rasterizer.h, with the builders of the index sets and the data that tests/test_rows_cpu.py checks and
tests/test_gpu_rows.py feeds to the kernels.

pack_rows() is g4s_pack_rows in its modes 0, 1, 2, 3, 7, 10 and 15; accumulate_rows() is g4s_accumulate_rows
(own_position 0) and g4s_accumulate_rows_ordered as an explicit sequence of float32 additions,
((0 + s_0 + ... + s_{k-1}) + own) + s_k + ... for own_position k > 0, and own + s_0 + ... for k = 0.  search() restates
the accumulate kernel's 32-ary search, so that the tests can say which source reaches which round."""
import numpy as np

f32 = np.float32
MODES = (0, 1, 2, 3, 7, 10, 15)
CHUNK = 64  # destination rows per workgroup of the accumulate kernel


# ---- the operations --------------------------------------------------------------------------------------------------
def pack_rows(segs, idx, n, packed, mode):
    """g4s_pack_rows over the float32 [P, w_s] arrays `segs` and the flat float32 array `packed`, row after row."""
    assert mode in MODES
    unpack, row_major, add, carry = mode & 1, mode & 2, mode & 4, mode & 8
    widths = [s.shape[1] for s in segs]
    W = sum(widths)
    bw = W + (1 if carry else 0)
    bits = packed.view(np.int32)  # (an index travels as int32 bits: never through a float register here)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            row = int(bits[j * bw + W]) if (carry and unpack) else int(idx[j])
            off = 0  # floats of a row before this segment
            for seg, w in zip(segs, widths):
                for c in range(w):
                    p = j * bw + off + c if row_major else off * n + j * w + c
                    if not unpack:
                        packed[p] = seg[row, c]
                    elif add:
                        seg[row, c] = f32(seg[row, c]) + f32(packed[p])
                    else:
                        seg[row, c] = packed[p]
                off += w
            if carry and not unpack:
                bits[j * bw + W] = np.int32(row)


def accumulate_rows(segs, buf, srcs, lo, hi, own_pos=0):
    """g4s_accumulate_rows (own_pos 0) / g4s_accumulate_rows_ordered over `buf` (float32 [m, W + 1], index column last)
    and srcs = [(offset, count)]: element for element one float32 addition after the other.  A row whose index lies
    outside [lo, hi) is not added anywhere."""
    widths = [s.shape[1] for s in segs]
    W = sum(widths)
    index = np.ascontiguousarray(buf[:, W]).view(np.int32)
    assert 0 <= own_pos <= len(srcs)
    held = [{int(index[j]): j for j in range(o, o + n)} for o, n in srcs]  # (a source holds a row at most once)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(lo, hi):
            off = 0
            for seg, w in zip(segs, widths):
                for c in range(w):
                    acc = f32(0.0) if own_pos else f32(seg[r, c])
                    for k in range(len(srcs) + 1):
                        if k == own_pos and k:
                            acc = f32(acc + f32(seg[r, c]))
                        if k == len(srcs):
                            break
                        if r in held[k]:
                            acc = f32(acc + f32(buf[held[k][r], off + c]))
                    seg[r, c] = acc
                off += w


def search(ix, target):
    """The accumulate kernel's search of one source for one end of a chunk: 32 probes a round, `step = (span + 31) >> 5`
    apart, valid while `pos < hi`.  -> (the first position whose index is >= target, the rounds that took)."""
    lo, hi, rounds = 0, len(ix), 0
    for _ in range(7):
        span = hi - lo
        if span <= 0:
            break
        rounds += 1
        step = (span + 31) >> 5
        pos = lo + np.arange(32) * step
        pos = pos[pos < hi]
        c, nv = int((ix[pos] < target).sum()), len(pos)
        if c == 0:
            hi = lo
        else:
            lo, hi = lo + (c - 1) * step + 1, (lo + c * step if c < nv else hi)
    assert hi == lo
    return lo, rounds


def rounds_bound(count):
    """Rounds the search can need over `count` rows: a round leaves a span of at most ceil(span / 32) - 1."""
    rounds = 0
    while count > 0:
        count, rounds = (count + 31) // 32 - 1, rounds + 1
    return rounds


# ---- data ------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan], f32)


def values(shape, rng, salt=0.04):
    """float32 normal values, none of them nor any sum of them a denormal (|x| >= 2^-10 makes every sum a multiple of
    2^-33), and a share `salt` of -0.0, +0.0, +inf, -inf and NaN."""
    x = rng.standard_normal(shape).astype(f32)
    x = np.where(np.abs(x) < f32(2.0 ** -10), np.copysign(f32(2.0 ** -10), x), x).astype(f32)
    if salt:
        hit = rng.random(shape) < salt
        x[hit] = SPECIALS[rng.integers(0, len(SPECIALS), int(hit.sum()))]
    return x


def segments(P, widths, rng, salt=0.04):
    return [values((P, w), rng, salt) for w in widths]


def source_buffer(sources, W, rng, salt=0.04):
    """-> (buf float32 [max(m, 1), W + 1] with the sources' rows back to back and their indices as int32 bits in the last
    column, srcs = [(offset, count)])."""
    counts = [len(ix) for ix in sources]
    m = sum(counts)
    buf = values((max(m, 1), W + 1), rng, salt)
    col = np.zeros(max(m, 1), np.int32)
    if m:
        col[:m] = np.concatenate(sources).astype(np.int32)
    buf[:, W] = col.view(f32)
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(int).tolist()
    return buf, list(zip(offs, counts))


def hand_placed_case(rng, widths):
    """-> (P, lo, hi, segs, buf, srcs): a shard [lo, hi) of 20 rows in 40; five sources, the first, the middle and the last
    of them without rows; rows 14 and 15 in no source; special values everywhere, and placed by hand where they decide a
    bit.  (The first segment is at least 3 floats wide.)"""
    P, lo, hi = 40, 11, 31
    segs = segments(P, widths, rng, salt=0.3)
    rows = np.setdiff1d(np.arange(lo, hi), (14, 15))
    sources = [np.zeros(0, np.int64), np.sort(rng.choice(rows, 9, replace=False)), np.zeros(0, np.int64),
               np.sort(np.concatenate([rng.choice(rows[1:-1], 6, replace=False), [lo, hi - 1]])), np.zeros(0, np.int64)]
    buf, srcs = source_buffer(sources, sum(widths), rng, salt=0.3)
    segs[0][14] = f32(-0.0)  # a row that no source holds: the ordered form behind a source makes it +0.0
    segs[0][15, :3] = (np.nan, np.inf, -np.inf)
    r = int(sources[1][0])   # -0.0 meets -0.0 and +0.0, inf meets -inf
    segs[0][r, :3] = (-0.0, np.inf, -0.0)
    buf[srcs[1][0], :3] = (-0.0, -np.inf, 0.0)
    return P, lo, hi, segs, buf, srcs


# ---- index sets of one source in the shard [lo, hi) ---------------------------------------------------------------------
def every_row(lo, hi):
    return np.arange(lo, hi, dtype=np.int64)


def every_other_row(lo, hi):
    return np.arange(lo, hi, 2, dtype=np.int64)


def chunk_ends(lo, hi):
    """The rows at offsets = 0 and = 63 (mod 64) from lo: the two ends of each chunk."""
    r = np.arange(lo, hi, dtype=np.int64)
    return r[((r - lo) % CHUNK == 0) | ((r - lo) % CHUNK == CHUNK - 1)]


def one_chunk(lo, hi, chunk):
    """All rows of chunk number `chunk`, and no other."""
    return np.arange(lo + chunk * CHUNK, min(lo + (chunk + 1) * CHUNK, hi), dtype=np.int64)


def inner_rows(lo, hi):
    """Every row but those of the first and the last chunk."""
    last = (hi - lo - 1) // CHUNK
    return np.arange(lo + CHUNK, lo + last * CHUNK, dtype=np.int64)


def last_row(lo, hi):
    return np.array([hi - 1], np.int64)


def pick(lo, hi, count, rng, must=()):
    """`count` distinct rows of [lo, hi), ascending, the rows `must` among them."""
    must = np.unique(np.asarray(must, np.int64))
    pool = np.setdiff1d(np.arange(lo, hi, dtype=np.int64), must)
    return np.sort(np.concatenate([must, rng.choice(pool, count - len(must), replace=False)]))


def with_foreign_rows(ix, lo, hi, P, below, above, rng):
    """`ix` with `below` rows of [0, lo) at its head and `above` rows of [hi, P) at its tail: still ascending."""
    return np.concatenate([pick(0, lo, below, rng), ix, pick(hi, P, above, rng)])


# ---- the search-depth cases of tests/test_gpu_rows.py ----------------------------------------------------------------------
# name -> (P, lo, hi, widths, seed).  Neither lo nor hi - lo is a multiple of 64.
DEPTH_SHARDS = {
    "to_1057": (1_200, 37, 37 + 1_057, (3, 1), 11),
    "to_1057_sets": (1_200, 37, 37 + 1_057, (3, 1), 12),
    "to_33825_product_widths": (40_200, 101, 101 + 40_003, (3, 48, 1, 2, 4, 2), 13),
    "to_1082401": (1_100_200, 77, 77 + 1_100_000, (1,), 14),
}
# The counts of each case's sources, in order.  A round of the search leaves a span of at most ceil(span / 32) - 1 rows
# (rounds_bound), so up to 32 rows take one round, up to 1 056 two, up to 33 824 three, up to 1 082 400 four, and
# 1 082 401 is the first count with a fifth: the powers of 32 and their neighbours lie inside the ranges, the last count of
# a range and the first of the next are in one launch as well.
DEPTH_COUNTS = {
    "to_1057": (1_057, 1_056, 1_025, 1_024, 1_023, 33, 32, 31),
    "to_1057_sets": (33, 64, 33, 960, 1, 0, 529, 32),
    "to_33825_product_widths": (32_769, 32_768, 32_767, 33_825, 33_824, 1_057, 33, 20_002),
    "to_1082401": (1_048_577, 33, 1_082_401, 1_082_400),
}
DEPTH_ROUNDS = {"to_1057": 3, "to_1057_sets": 2, "to_33825_product_widths": 4, "to_1082401": 5}  # the deepest search


def depth_case(name):
    """-> (P, lo, hi, widths, sources): the index sets of one launch whose eight search groups end in different rounds."""
    P, lo, hi, widths, seed = DEPTH_SHARDS[name]
    rng = np.random.default_rng(seed)
    ends = (lo, hi - 1)
    if name == "to_1057":
        sources = [every_row(lo, hi), pick(lo, hi, 1_056, rng, ends), pick(lo, hi, 1_025, rng), pick(lo, hi, 1_024, rng, ends),
                   pick(lo, hi, 1_023, rng), pick(lo, hi, 33, rng, ends), pick(lo, hi, 32, rng), pick(lo, hi, 31, rng, ends)]
    elif name == "to_1057_sets":
        sources = [chunk_ends(lo, hi), one_chunk(lo, hi, 5), one_chunk(lo, hi, 16), inner_rows(lo, hi), last_row(lo, hi),
                   np.zeros(0, np.int64), every_other_row(lo, hi), pick(lo + CHUNK, hi - CHUNK, 32, rng)]
    elif name == "to_33825_product_widths":
        sources = [pick(lo, hi, 32_769, rng, ends), pick(lo, hi, 32_768, rng), pick(lo, hi, 32_767, rng, ends),
                   pick(lo, hi, 33_825, rng), pick(lo, hi, 33_824, rng, ends), pick(lo, hi, 1_057, rng),
                   pick(lo, hi, 33, rng, ends), every_other_row(lo, hi)]
    else:
        sources = [pick(lo, hi, 1_048_577, rng, ends), pick(lo, hi, 33, rng), pick(lo, hi, 1_082_401, rng, ends),
                   pick(lo, hi, 1_082_400, rng)]
    return P, lo, hi, widths, sources
