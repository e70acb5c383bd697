"""The truth of tests/test_gpu_rows.py, checked without a GPU: parallel._HostRows (torch indexing on host tensors, what the
GPU tests compare the kernels of g4splat_amd/csrc/rows.hip with) against the loop-level restatement of
include/g4s_rasterizer.h in rows_ref.py, bit for bit, in every path and layout, with -0.0, +-inf and NaN in the data, rows
that no source holds and sources without rows; and the builders of the index sets and the data the GPU tests rely on."""
import numpy as np
import pytest
import torch

import rows_ref as rr
from g4splat_amd import parallel
from support import same_bits

f32 = np.float32
WIDTHS = (3, 5, 1)
W = sum(WIDTHS)


def _host(segs):
    """_HostRows over torch copies of the numpy segments."""
    rows = [torch.from_numpy(s.copy()) for s in segs]
    return parallel._HostRows(rows), rows


def _same_rows(rows, segs, what):
    for i, (r, s) in enumerate(zip(rows, segs)):
        same_bits(r, s, (what, "segment", i), nan_payload=False)


@pytest.mark.parametrize("row_major, index_col", [(False, False), (True, False), (True, True)])
def test_pack_and_unpack_equal_the_restatement(row_major, index_col):
    rng = np.random.default_rng(1)
    P, n = 23, 9
    segs = rr.segments(P, WIDTHS, rng, salt=0.3)
    idx = rng.permutation(P)[:n].astype(np.int64)  # distinct, not ascending
    bw = W + (1 if index_col else 0)
    mode = (2 if row_major else 0) | (8 if index_col else 0)
    ops, rows = _host(segs)
    # pack: modes 0, 2, 10.  Both buffers start from the same fill and carry 7 floats more than the rows need.
    want = np.full(n * bw + 7, f32(123.0))
    rr.pack_rows([s.copy() for s in segs], idx, n, want, mode)
    flat = torch.full((n * bw + 7,), 123.0)
    ops.pack(torch.from_numpy(idx), flat[:n * bw].view(n, bw) if row_major else flat, index_col=index_col, row_major=row_major)
    if index_col:
        got = flat[:n * bw].view(n, bw).numpy()
        assert np.array_equal(np.ascontiguousarray(got[:, W]).view(np.int32), idx.astype(np.int32))
        assert np.array_equal(want.view(np.int32)[:n * bw].reshape(n, bw)[:, W], idx.astype(np.int32))
        same_bits(got[:, :W], want[:n * bw].reshape(n, bw)[:, :W], "pack", nan_payload=False)
        same_bits(flat[n * bw:], want[n * bw:], "behind the buffer", nan_payload=False)
    else:
        same_bits(flat, want, ("pack", mode), nan_payload=False)
    _same_rows(rows, segs, "pack leaves the rows alone")
    # unpack: modes 1, 3 (an index column, if any, is passed over: the indices come from idx)
    if not index_col:
        buf = rr.values(n * W, rng, salt=0.3)
        want_segs = [s.copy() for s in segs]
        rr.pack_rows(want_segs, idx, n, buf.copy(), mode | 1)
        t = torch.from_numpy(buf.copy())
        ops.unpack(torch.from_numpy(idx), t.view(n, W) if row_major else t, row_major=row_major)
        _same_rows(rows, want_segs, ("unpack", mode | 1))
        same_bits(t, buf, "unpack leaves the buffer alone", nan_payload=False)
        assert any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(want_segs, segs))


@pytest.mark.parametrize("path, own_pos", [("per_source", 0), ("one_launch", 0)] + [("rank", k) for k in range(6)])
def test_accumulate_equals_the_sequence_of_float32_additions(path, own_pos):
    P, lo, hi, segs, buf, srcs = rr.hand_placed_case(np.random.default_rng(2), WIDTHS)
    assert [c for _, c in srcs] == [0, 9, 0, 8, 0]
    want = [s.copy() for s in segs]
    rr.accumulate_rows(want, buf, srcs, lo, hi, own_pos)
    ops, rows = _host(segs)
    t = torch.from_numpy(buf.copy())
    ops.accumulate(t, srcs, lo, hi, path, own_pos)
    _same_rows(rows, want, (path, own_pos))
    same_bits(t, buf, "the buffer")
    for s, w in zip(segs, want):  # nothing outside the shard moves
        same_bits([s[:lo], s[hi:]], [w[:lo], w[hi:]], "outside the shard")
    # the row no source holds: an own -0.0 stays what it is when the owner's rows come first, and is +0.0 behind a zero
    assert (want[0][14] == 0).all() and bool(np.signbit(want[0][14]).all()) == (own_pos == 0)
    assert np.isnan(want[0][15][0]) and want[0][15][1] == np.inf and want[0][15][2] == -np.inf
    r = int(np.ascontiguousarray(buf[:, W]).view(np.int32)[srcs[1][0]])
    assert np.isnan(want[0][r][1])  # inf + -inf


def test_one_accumulating_unpack_per_source_is_the_same_sequence():
    """Modes 15 (indices from the buffer) and 7 (indices from idx[]) of the restatement, source after source, equal the
    restated accumulation with the owner's rows first, and _HostRows' "per_source" path."""
    P, lo, hi, segs, buf, srcs = rr.hand_placed_case(np.random.default_rng(3), WIDTHS)
    want = [s.copy() for s in segs]
    rr.accumulate_rows(want, buf, srcs, lo, hi, 0)
    index = np.ascontiguousarray(buf[:, W]).view(np.int32)
    m15, m7 = [s.copy() for s in segs], [s.copy() for s in segs]
    for o, c in srcs:
        rr.pack_rows(m15, None, c, buf[o:o + c].copy().reshape(-1), 15)
        rr.pack_rows(m7, index[o:o + c].astype(np.int64), c, np.ascontiguousarray(buf[o:o + c, :W]).reshape(-1), 7)
    for a, b, c_ in zip(m15, m7, want):
        same_bits(a, c_, "mode 15", nan_payload=False)
        same_bits(b, c_, "mode 7", nan_payload=False)


def test_restated_accumulation_skips_rows_outside_the_shard():
    rng = np.random.default_rng(4)
    P, lo, hi = 40, 11, 31
    segs = rr.segments(P, WIDTHS, rng)
    inside = rr.pick(lo, hi, 7, rng, (lo, hi - 1))
    foreign = rr.with_foreign_rows(inside, lo, hi, P, 3, 4, rng)
    assert len(foreign) == 14 and (np.diff(foreign) > 0).all() and (foreign[:3] < lo).all() and (foreign[-4:] >= hi).all()
    buf, srcs = rr.source_buffer([foreign], W, rng)
    got = [s.copy() for s in segs]
    rr.accumulate_rows(got, buf, srcs, lo, hi, 0)
    want = [s.copy() for s in segs]
    rr.accumulate_rows(want, buf, [(3, 7)], lo, hi, 0)
    for a, b in zip(got, want):
        same_bits(a, b, nan_payload=False)


# ---- the builders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.DEPTH_SHARDS))
def test_depth_cases_hold_what_the_gpu_tests_rely_on(name):
    P, lo, hi, widths, sources = rr.depth_case(name)
    assert lo % 64 and (hi - lo) % 64 and 0 < lo < hi < P and 1 <= len(sources) <= 8
    assert tuple(len(ix) for ix in sources) == rr.DEPTH_COUNTS[name]
    for ix in sources:
        assert ix.dtype == np.int64 and (np.diff(ix) > 0).all()  # ascending and distinct
        assert len(ix) == 0 or (lo <= ix[0] and ix[-1] < hi)
    # the deepest search of the launch, and every search against a plain binary search, at the ends of (a sample of) the chunks
    chunks = (hi - lo + 63) // 64
    sample = sorted(set(range(0, chunks, max(1, chunks // 150))) | {0, 1, chunks - 2, chunks - 1})
    deepest = 0
    for ix in sources:
        most = 0
        for c in sample:
            for target in (lo + 64 * c, min(lo + 64 * c + 64, hi)):
                pos, rounds = rr.search(ix, target)
                assert pos == np.searchsorted(ix, target, side="left")
                most = max(most, rounds)
        assert most <= rr.rounds_bound(len(ix))
        deepest = max(deepest, most)
    assert deepest == rr.DEPTH_ROUNDS[name] == rr.rounds_bound(max(rr.DEPTH_COUNTS[name]))


def test_depth_cases_put_counts_on_and_beside_the_powers_of_32_in_one_launch():
    assert [rr.rounds_bound(n) for n in (1, 32, 33, 1_024, 1_056, 1_057, 32_768, 32_769, 33_824, 33_825, 1_048_577, 1_082_400,
                                         1_082_401, 2 ** 31 - 1)] == [1, 1, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 7]
    small, big, huge = (rr.DEPTH_COUNTS[k] for k in ("to_1057", "to_33825_product_widths", "to_1082401"))
    assert {31, 32, 33, 1_023, 1_024, 1_025, 1_056, 1_057} <= set(small) and 1 in rr.DEPTH_COUNTS["to_1057_sets"]
    assert {32_767, 32_768, 32_769, 33_824, 33_825} <= set(big) and huge[:2] == (1_048_577, 33) and {1_082_400, 1_082_401} <= set(huge)
    assert {rr.rounds_bound(n) for n in small} == {1, 2, 3} and {rr.rounds_bound(n) for n in big} == {2, 3, 4}
    assert {rr.rounds_bound(n) for n in huge} == {2, 4, 5}


def test_index_sets_hold_the_stated_rows():
    lo, hi = 37, 37 + 1_057
    assert rr.every_row(lo, hi).tolist() == list(range(lo, hi))
    assert rr.every_other_row(lo, hi).tolist() == list(range(lo, hi, 2))
    ends = rr.chunk_ends(lo, hi)
    assert set((ends - lo) % 64) == {0, 63} and len(ends) == 17 + 16 and ends[0] == lo and ends[-1] == lo + 1_024
    assert rr.one_chunk(lo, hi, 5).tolist() == list(range(lo + 320, lo + 384))
    assert rr.one_chunk(lo, hi, 16).tolist() == list(range(lo + 1_024, hi))  # the last chunk holds 33 rows
    inner = rr.inner_rows(lo, hi)
    assert inner[0] == lo + 64 and inner[-1] == lo + 1_023 and len(inner) == 960
    assert rr.last_row(lo, hi).tolist() == [hi - 1]
    got = rr.pick(lo, hi, 33, np.random.default_rng(0), (lo, hi - 1))
    assert len(got) == 33 and got[0] == lo and got[-1] == hi - 1 and (np.diff(got) > 0).all()
    assert rr.depth_case("to_1057_sets")[4][4].tolist() == [hi - 1]
    _, _, _, _, sources = rr.depth_case("to_1057")
    for i in (0, 1, 3, 5, 7):
        assert sources[i][0] == lo and sources[i][-1] == hi - 1


def test_values_and_buffers():
    rng = np.random.default_rng(5)
    x = rr.values((4_000, 7), rng)
    finite = x[np.isfinite(x) & (x != 0)]
    assert x.dtype == f32 and (np.abs(finite) >= f32(2.0 ** -10)).all()
    assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
    assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
    assert np.isfinite(rr.values((50, 3), rng, salt=0)).all()
    sources = [np.array([5, 9]), np.zeros(0, np.int64), np.array([2, 5, 70_000])]
    buf, srcs = rr.source_buffer(sources, 4, rng)
    assert srcs == [(0, 2), (2, 0), (2, 3)] and buf.shape == (5, 5) and buf.dtype == f32
    assert np.ascontiguousarray(buf[:, 4]).view(np.int32).tolist() == [5, 9, 2, 5, 70_000]
    buf, srcs = rr.source_buffer([np.zeros(0, np.int64)] * 3, 4, rng)
    assert srcs == [(0, 0)] * 3 and buf.shape == (1, 5)
