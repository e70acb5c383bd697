"""The row kernels of the gradient exchange (g4splat_amd/csrc/rows.hip: g4s_pack_rows, g4s_accumulate_rows,
g4s_accumulate_rows_ordered) at shard size, width and depth, against parallel._HostRows run on host copies of the same
data -- the truth that tests/test_rows_cpu.py holds to the loop-level restatement of include/g4s_rasterizer.h.  Every
comparison is equality of bits (a NaN meets a NaN); whole tensors are compared, so the rows [0, row_lo) and [row_hi, P) of
every segment are sentinels, and every buffer carries PAD sentinel floats behind its rows.  The data is salted with -0.0,
+0.0, +-inf and NaN throughout and holds no denormal (rows_ref.values).

Search rounds of the accumulate kernel (a round leaves at most ceil(span / 32) - 1 rows: rows_ref.rounds_bound, and
test_rows_cpu.py runs the restated search over these very index sets):
  to_1057                  counts 31, 32 -> one round; 33, 1 023, 1 024, 1 025, 1 056 -> two; 1 057 -> three; one launch
  to_1057_sets             the index sets (chunk ends, one chunk, the last chunk, no first / last chunk, row_hi - 1, no row,
                           every other row): one and two rounds
  to_33825_product_widths  33 -> two rounds; 1 057, 32 767, 32 768, 32 769, 33 824 -> three; 33 825 -> four; one launch, the
                           widths (3, 48, 1, 2, 4, 2) of the product
  to_1082401               33 -> two rounds; 1 048 577 and 1 082 400 -> four; 1 082 401 -> five; one launch, rows of one float
Lane passes (64 floats of a row each; the pack kernel's f0 loop, the accumulate kernel's f0 and q loops):
  row widths 63 and 64 one pass, 65 and 128 two, 129 and (40, 70, 20) = 130 three, 240 four (the 60 KiB LDS tile);
  300 five (pack only).  With the index column (modes 10 and 15) a buffer row is one float longer: the column is float
  63 (lane 63 of the first pass), 64 (a second pass of its own), 65, 128 (a third pass of its own), 129, 130 and 240.  The
  eight-segment layouts (1, 5, 2, 9, 3, 7, 4, rest) put their last segment across the passes; (40, 70, 20) has its middle
  segment across float 64.
Grid cap of the pack kernel: 262 144 rows are eight per wave, 262 145 and 300 000 more than eight."""
import functools

import numpy as np
import pytest
import torch

import rows_ref as rr
from g4splat_amd import _lib, parallel
from support import DEV, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
PAD = 257            # sentinel floats behind every buffer
SENTINEL = f32(12345.0)
PRODUCT = (3, 48, 1, 2, 4, 2)
UNSUPPORTED, INVALID = -4, -1


class _Pair:
    """The same segments on the host (_HostRows: the truth) and on the device (_DeviceRows: the kernels)."""

    def __init__(self, segs):
        self.start = segs
        self.host = [torch.from_numpy(s.copy()) for s in segs]
        self.dev = [h.to(DEV) for h in self.host]
        self.H, self.D = parallel._HostRows(self.host), parallel._row_ops(self.dev)
        assert type(self.D) is parallel._DeviceRows

    def got(self):
        torch.cuda.synchronize()
        return [d.cpu().numpy() for d in self.dev]

    def same(self, what):
        for i, (d, h) in enumerate(zip(self.got(), self.host)):
            same_bits(d, h, (what, "segment", i), nan_payload=False)

    def untouched(self, what, lo=0, hi=0):
        """The device rows outside [lo, hi) are what they were."""
        for i, (d, s) in enumerate(zip(self.got(), self.start)):
            same_bits(d[:lo], s[:lo], (what, "rows below the shard", i), nan_payload=False)
            same_bits(d[hi:], s[hi:], (what, "rows above the shard", i), nan_payload=False)


def _padded(data):
    """-> (host tensor, device tensor): the floats of `data` with PAD sentinels behind them."""
    h = torch.from_numpy(np.concatenate([data.reshape(-1), np.full(PAD, SENTINEL, f32)]))
    return h, h.to(DEV)


def _same_buffer(d, h, n, bw, what):
    """Buffers equal bit for bit, the sentinels behind them included -- column by column (an index column holds int32
    bits, never a NaN's), so that a failure names the column."""
    torch.cuda.synchronize()
    got, want = d.cpu().numpy(), h.numpy()
    same_bits(got[n * bw:], np.full(PAD, SENTINEL, f32), (what, "behind the buffer"), nan_payload=False)
    same_bits(got, want, what, nan_payload=False)
    if bw <= 301:
        g, w = got[:n * bw].reshape(n, bw), want[:n * bw].reshape(n, bw)
        for c in range(bw):
            same_bits(g[:, c], w[:, c], (what, "column", c), nan_payload=False)


def _check_pack_modes(segs, idx, rng, what):
    """g4s_pack_rows in every mode over the rows `idx` (distinct) of `segs` against _HostRows."""
    n, P = len(idx), segs[0].shape[0]
    W = sum(s.shape[1] for s in segs)
    idx_h = torch.from_numpy(idx)
    idx_d = idx_h.to(DEV)
    for mode in rr.MODES:
        pair = _Pair(segs)
        row_major, carry = bool(mode & 2), bool(mode & 8)
        bw = W + (1 if carry else 0)
        if mode & 1:
            data = rr.values((n, bw), rng)
            if carry:
                data[:, W] = idx.astype(np.int32).view(f32)
        else:
            data = np.full((n, bw), f32(-777.0))
        h, d = _padded(data)
        hv, dv = (t[:n * bw].view(n, bw) if row_major else t[:n * bw] for t in (h, d))
        if mode in (0, 2, 10):
            pair.H.pack(idx_h, hv, index_col=carry, row_major=row_major)
            pair.D.pack(idx_d, dv, index_col=carry, row_major=row_major)
        elif mode in (1, 3):
            pair.H.unpack(idx_h, hv, row_major=row_major)
            pair.D.unpack(idx_d, dv, row_major=row_major)
        elif mode == 15:
            pair.H.accumulate(hv, [(0, n)], 0, P, "per_source", 0)
            pair.D.accumulate(dv, [(0, n)], 0, P, "per_source", 0)
        else:  # 7: the accumulating unpack with the indices from idx[] -- the same additions as with an index column
            with_col = torch.cat([hv, idx_h.to(torch.int32).view(torch.float32).view(n, 1)], dim=1)
            pair.H.accumulate(with_col, [(0, n)], 0, P, "per_source", 0)
            pair.D._kernel(idx_d, n, dv, 7)
        pair.same((what, "mode", mode))
        _same_buffer(d, h, n, bw, (what, "mode", mode))
        if mode == 10:
            torch.cuda.synchronize()
            col = np.ascontiguousarray(dv.cpu().numpy()[:, W]).view(np.int32)
            assert np.array_equal(col, idx.astype(np.int32)), (what, "index column")
        if mode & 1:  # (the unpack did something)
            assert any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(pair.got(), segs)), (what, mode)


def _check_accumulate(segs, buf, srcs, lo, hi, paths, what, truth_srcs=None):
    """The owner's accumulation of `buf`'s sources in each (path, own_position) against _HostRows (over `truth_srcs` where
    the kernel is to pass rows over); nothing outside [lo, hi) and nothing of the buffer changes.  -> the device rows."""
    m, bw = buf.shape
    out = {}
    for path, own_pos in paths:
        pair = _Pair(segs)
        h, d = _padded(buf)
        pair.H.accumulate(h[:m * bw].view(m, bw), truth_srcs or srcs, lo, hi, path, own_pos)
        pair.D.accumulate(d[:m * bw].view(m, bw), srcs, lo, hi, path, own_pos)
        pair.same((what, path, own_pos))
        pair.untouched((what, path, own_pos), lo, hi)
        same_bits(d, h, (what, path, own_pos, "the buffer"), nan_payload=False)  # (_HostRows only reads it)
        out[(path, own_pos)] = pair.got()
    return out


def _raw_accumulate(lib, rows, widths, srcs, buf, lo, hi, own_pos=None):
    """The entry points' status, straight from the library."""
    n = len(srcs)
    args = (len(rows), _lib.ptrs(rows), _lib.array(_lib.c_i, list(widths)), n, _lib.array(_lib.c_i, [o for o, _ in srcs]),
            _lib.array(_lib.c_i, [c for _, c in srcs]), _lib.ptr(buf), lo, hi)
    if own_pos is None:
        rc = lib.g4s_accumulate_rows(*args, _lib.stream(DEV))
    else:
        rc = lib.g4s_accumulate_rows_ordered(*args, own_pos, _lib.stream(DEV))
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def _depth(name):
    P, lo, hi, widths, sources = rr.depth_case(name)
    rng = np.random.default_rng(rr.DEPTH_SHARDS[name][4] + 100)
    buf, srcs = rr.source_buffer(sources, sum(widths), rng)
    return P, lo, hi, rr.segments(P, widths, rng), buf, srcs


# ---- search depth and count boundaries -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["to_1057", "to_1057_sets", "to_33825_product_widths", "to_1082401"])
def test_search_depth_and_counts_beside_the_powers_of_32(hip_lib, name):
    P, lo, hi, segs, buf, srcs = _depth(name)
    assert lo % 64 and (hi - lo) % 64 and tuple(c for _, c in srcs) == rr.DEPTH_COUNTS[name]
    n = len(srcs)
    paths = [("one_launch", 0), ("rank", n // 2), ("rank", n)] + ([("per_source", 0), ("rank", 1)] if P < 10 ** 6 else [])
    _check_accumulate(segs, buf, srcs, lo, hi, paths, name)


# ---- width -----------------------------------------------------------------------------------------------------------------
def _layouts():
    out = []
    for S in (63, 64, 65, 128, 129, 240):
        out.append(pytest.param((S,), id=f"w{S}_one_segment"))
        out.append(pytest.param((1, 5, 2, 9, 3, 7, 4, S - 31), id=f"w{S}_eight_segments"))
    out.append(pytest.param((40, 70, 20), id="w130_segment_across_float_64"))
    return out


@pytest.mark.parametrize("widths", _layouts())
def test_row_widths_of_one_to_four_lane_passes(hip_lib, widths):
    rng = np.random.default_rng(sum(widths) * 8 + len(widths))
    P, lo, hi = 331, 13, 13 + 150
    segs = rr.segments(P, widths, rng)
    _check_pack_modes(segs, rng.permutation(P)[:203].astype(np.int64), rng, widths)
    sources = [rr.every_row(lo, hi), rr.pick(lo, hi, 33, rng, (lo, hi - 1)), rr.chunk_ends(lo, hi), rr.one_chunk(lo, hi, 2)]
    buf, srcs = rr.source_buffer(sources, sum(widths), rng)
    _check_accumulate(segs, buf, srcs, lo, hi, [("per_source", 0), ("one_launch", 0), ("rank", 0), ("rank", 2), ("rank", 4)], widths)


def test_pack_rows_of_five_lane_passes(hip_lib):
    rng = np.random.default_rng(300)
    segs = rr.segments(150, (300,), rng)
    _check_pack_modes(segs, rng.permutation(150)[:77].astype(np.int64), rng, "width 300")


@pytest.mark.parametrize("widths", [(241,), (200, 41)])
def test_rows_of_241_floats_are_refused_and_left_alone(hip_lib, widths):
    rng = np.random.default_rng(241)
    P, lo, hi = 100, 5, 90
    pair = _Pair(rr.segments(P, widths, rng))
    buf, srcs = rr.source_buffer([rr.every_row(lo, hi)], 241, rng)
    d = torch.from_numpy(buf).to(DEV)
    for own_pos in (None, 0, 1):
        assert _raw_accumulate(hip_lib, pair.dev, widths, srcs, d, lo, hi, own_pos) == UNSUPPORTED
        assert "wider than 240" in _lib.last_error()
        pair.untouched(("241", own_pos))
    same_bits(d, buf, nan_payload=False)


# ---- grid cap of the pack kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [262_144, 262_145, 300_000])
def test_pack_rows_beyond_eight_rows_a_wave(hip_lib, n):
    rng = np.random.default_rng(n)
    P = n + 1_000
    _check_pack_modes(rr.segments(P, (3, 1), rng), rng.permutation(P)[:n].astype(np.int64), rng, n)


# ---- sources ---------------------------------------------------------------------------------------------------------------
def _all_paths(nsrc):
    return [("per_source", 0), ("one_launch", 0)] + [("rank", k) for k in range(nsrc + 1)]


def test_sources_without_rows_inside_a_launch(hip_lib):
    rng = np.random.default_rng(21)
    P, lo, hi = 300, 70, 70 + 150
    segs = rr.segments(P, PRODUCT, rng)
    none = np.zeros(0, np.int64)
    for sources in ([none, rr.pick(lo, hi, 40, rng, (lo,)), none, rr.pick(lo, hi, 25, rng, (hi - 1,)), none],
                    [none, none, rr.every_row(lo, hi)], [rr.every_other_row(lo, hi), none, none], [none, none, none], [none]):
        buf, srcs = rr.source_buffer(sources, sum(PRODUCT), rng)
        assert [c for _, c in srcs] == [len(s) for s in sources]
        _check_accumulate(segs, buf, srcs, lo, hi, _all_paths(len(srcs)), [len(s) for s in sources])


@pytest.mark.parametrize("nsrc", [16, 17])
def test_two_and_three_launches_equal_a_launch_per_source(hip_lib, nsrc):
    rng = np.random.default_rng(nsrc)
    P, lo, hi = 400, 70, 70 + 250
    segs = rr.segments(P, PRODUCT, rng)
    counts = [250, 1, 33, 0, 125, 64, 7, 200, 32, 249, 2, 31, 100, 65, 0, 180, 250][:nsrc]
    sources = [rr.pick(lo, hi, c, rng) for c in counts]
    buf, srcs = rr.source_buffer(sources, sum(PRODUCT), rng)
    got = _check_accumulate(segs, buf, srcs, lo, hi, [("per_source", 0), ("one_launch", 0)], nsrc)
    for a, b in zip(got[("per_source", 0)], got[("one_launch", 0)]):  # kernel against kernel, as the header words it
        same_bits(b, a, nsrc, nan_payload=False)


def test_ordered_form_at_every_position_of_eight_sources(hip_lib):
    rng = np.random.default_rng(8)
    P, lo, hi = 400, 70, 70 + 250
    segs = rr.segments(P, PRODUCT, rng)
    sources = [rr.pick(lo, hi, c, rng) for c in (250, 1, 33, 125, 64, 7, 200, 249)]
    buf, srcs = rr.source_buffer(sources, sum(PRODUCT), rng)
    got = _check_accumulate(segs, buf, srcs, lo, hi, [("rank", k) for k in range(9)] + [("one_launch", 0)], "ordered")
    for a, b in zip(got[("rank", 0)], got[("one_launch", 0)]):  # own_position 0 is g4s_accumulate_rows
        same_bits(a, b, "position 0", nan_payload=False)


def test_ordered_form_refuses_what_it_cannot_order(hip_lib):
    rng = np.random.default_rng(9)
    P, lo, hi = 200, 70, 70 + 100
    pair = _Pair(rr.segments(P, PRODUCT, rng))
    buf, srcs = rr.source_buffer([rr.pick(lo, hi, 10, rng) for _ in range(9)], sum(PRODUCT), rng)
    d = torch.from_numpy(buf).to(DEV)
    assert _raw_accumulate(hip_lib, pair.dev, PRODUCT, srcs, d, lo, hi, 1) == UNSUPPORTED  # nine sources behind a position
    assert "at most 8 sources" in _lib.last_error()
    pair.untouched("nine sources")
    assert _raw_accumulate(hip_lib, pair.dev, PRODUCT, srcs[:3], d, lo, hi, 4) == INVALID
    assert "own_position" in _lib.last_error()
    assert _raw_accumulate(hip_lib, pair.dev, PRODUCT, srcs[:3], d, lo, hi, -1) == INVALID
    pair.untouched("position outside 0..nsrc")
    same_bits(d, buf, nan_payload=False)
    # (nine sources with the owner's rows first are two launches)
    _check_accumulate(pair.start, buf, srcs, lo, hi, [("rank", 0), ("one_launch", 0)], "nine sources, position 0")


# ---- values -----------------------------------------------------------------------------------------------------------------
def test_special_values_and_rows_that_no_source_holds(hip_lib):
    P, lo, hi, segs, buf, srcs = rr.hand_placed_case(np.random.default_rng(2), PRODUCT)
    got = _check_accumulate(segs, buf, srcs, lo, hi, _all_paths(len(srcs)), "hand-placed")
    for (path, own_pos), rows in got.items():
        # row 14 is in no source and holds -0.0: it stays -0.0 when the owner's rows come first, and is +0.0 behind a zero
        assert (rows[0][14] == 0).all() and bool(np.signbit(rows[0][14]).all()) == (own_pos == 0), (path, own_pos)
        assert np.isnan(rows[0][15][0]) and rows[0][15][1] == np.inf and rows[0][15][2] == -np.inf


# ---- rows outside the shard -----------------------------------------------------------------------------------------------------
def test_rows_outside_the_shard_are_passed_over(hip_lib):
    rng = np.random.default_rng(31)
    P, lo, hi = 600, 150, 150 + 300
    segs = rr.segments(P, PRODUCT, rng)
    inside = [rr.pick(lo, hi, 120, rng, (lo, hi - 1)), np.zeros(0, np.int64), rr.every_row(lo, hi), rr.pick(lo, hi, 33, rng)]
    edges = [(40, 50), (7, 9), (150, 150), (0, 0)]  # rows below row_lo at the head, at and above row_hi at the tail
    sources = [rr.with_foreign_rows(ix, lo, hi, P, b, a, rng) for ix, (b, a) in zip(inside, edges)]
    assert all((np.diff(s) > 0).all() for s in sources) and sources[2][0] == 0 and sources[2][-1] == P - 1
    buf, srcs = rr.source_buffer(sources, sum(PRODUCT), rng)
    truth = [(o + b, c - b - a) for (o, c), (b, a) in zip(srcs, edges)]  # the reference never sees the foreign rows
    assert [c for _, c in truth] == [len(ix) for ix in inside]
    _check_accumulate(segs, buf, srcs, lo, hi, [("one_launch", 0)] + [("rank", k) for k in range(5)], "foreign rows", truth)


def test_unsorted_sources_write_nothing_outside_the_shard(hip_lib):
    rng = np.random.default_rng(32)
    P, lo, hi = 600, 150, 150 + 300
    segs = rr.segments(P, PRODUCT, rng)
    sources = [rng.permutation(P)[:c].astype(np.int64) for c in (500, 33, 1)]
    buf, srcs = rr.source_buffer(sources, sum(PRODUCT), rng)
    for own_pos in (None, 2):
        pair = _Pair(segs)
        h, d = _padded(buf)
        assert _raw_accumulate(hip_lib, pair.dev, PRODUCT, srcs, d, lo, hi, own_pos) == 0, _lib.last_error()
        pair.untouched(("unsorted", own_pos), lo, hi)
        same_bits(d, h, "the buffer", nan_payload=False)
