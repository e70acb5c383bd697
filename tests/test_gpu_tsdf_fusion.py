"""TSDF fusion on the MI355X (g4splat_amd/csrc/tsdf/tsdf.hip: emit, key sort, unique, lookup, merge, init, integrate)
against the numpy restatement, on the cases of tests/tsdf_cases.py -- image borders, surfaces nearer than sdf_trunc,
long walks and exact DDA ties, every validity edge, keys that differ in every byte, every shape of the table merge, tiny
and thin images.  tests/test_tsdf_fusion_cpu.py shows that each case contains what it is named for and ties the
restatement to float64.  The contract is float32 in the header's order without contraction: every comparison is on bits."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_cases as tc
import tsdf_ref
from g4splat_amd import _lib
from g4splat_amd import mesh as mesh_mod
from support import DEV, dev, host, words

pytestmark = pytest.mark.gpu

NAMES = list(tc.CASES)
POISON = (float("nan"), 1.0, 1e9)  # tsdf, weight, colour of a pool slot nobody may have written


def _poison(vol, first_block=0):
    for buf, val, per in zip((vol.tsdf, vol.weight, vol.color), POISON, (512, 512, 1536)):
        buf[first_block * per:] = val


def _volume(case, initial_blocks, poison):
    vol = mesh_mod.TSDFVolume(case.voxel, case.T, case.depth_trunc, DEV, initial_blocks=initial_blocks)
    if poison:
        _poison(vol)
        grow = vol._grow

        def grow_poisoned(need):  # a grown pool's new part is poisoned as well, before the merge initialises its blocks
            old = vol.pool_blocks
            grow(need)
            _poison(vol, old)
        vol._grow = grow_poisoned
    return vol


def _pool(vol, n=None):
    """The first n slots of the pool (default: all) on the host as bits: tsdf [n,512], weight [n,512], colour [n,1536]."""
    n = vol.pool_blocks if n is None else n
    return tuple(words(host(buf[:n * per])).reshape(n, per)
                 for buf, per in zip((vol.tsdf, vol.weight, vol.color), (512, 512, 1536)))


def _poison_intact(vol, first_block):
    """Every slot from first_block on still holds the poison, bit for bit (compared on the device)."""
    for buf, val, per in zip((vol.tsdf, vol.weight, vol.color), POISON, (512, 512, 1536)):
        want = int(words(np.float32(val)).astype(np.int64).item())
        if not (buf[first_block * per:].view(torch.int32).to(torch.int64) & 0xFFFFFFFF == want).all().item():
            return False
    return True


def _fuse(name, initial_blocks=None, poison=True):
    """Fuse the case's views into a fresh volume and hold every step against the reference: the returned counts, the
    table, the voxels of the allocated blocks bit for bit (those the view did not touch are as they were), the poison in
    every slot beyond the table.  Returns the volume and per view (keys, slots, tsdf, weight, colour) as bytes."""
    case = tc.case(name)
    steps, _ref = tc.reference(name)
    vol = _volume(case, len(steps[-1].keys) + 7 if initial_blocks is None else initial_blocks, poison)
    want = [np.zeros((0, 512), np.uint32), np.zeros((0, 512), np.uint32), np.zeros((0, 1536), np.uint32)]
    out = []
    for i, (v, s) in enumerate(zip(case.views, steps)):
        table_before = (vol.keys, vol.slots)
        counts = vol.integrate(dev(v.depth)[None], dev(v.rgb), v.cam, dev(v.mask))
        torch.cuda.synchronize()
        assert counts == s.counts, (name, i)
        if counts[0] == 0:
            assert vol.keys is table_before[0] and vol.slots is table_before[1]
        keys, slots = vol.table()
        assert vol.num_blocks == len(s.keys) <= vol.pool_blocks
        assert np.array_equal(keys, s.keys) and np.array_equal(slots, s.slots), (name, i)
        n_new = s.counts[1]
        want = [np.concatenate([w, np.zeros((n_new, w.shape[1]), np.uint32)]) for w in want]
        for w, new in zip(want, (s.tsdf, s.weight, s.color)):
            w[s.touched_slots] = words(new).reshape(len(s.touched_slots), w.shape[1])
        pool = _pool(vol, vol.num_blocks)
        for what, got, w in zip(("tsdf", "weight", "colour"), pool, want):
            assert np.array_equal(got, w), (name, i, what, int((got != w).sum()))
        if poison:
            assert _poison_intact(vol, vol.num_blocks), (name, i, "a slot beyond the table was written")
        tsdf, weight, color = vol.voxels()
        assert np.array_equal(words(tsdf), want[0][slots]) and np.array_equal(words(weight), want[1][slots])
        assert np.array_equal(words(color).reshape(-1, 1536), want[2][slots])
        out.append((keys.tobytes(), slots.tobytes()) + tuple(g.tobytes() for g in pool))
    return vol, out


@pytest.mark.parametrize("name", NAMES)
def test_every_view_matches_the_restatement_bit_for_bit(hip_lib, name):
    """After every view: (touched, new), keys and slots, and tsdf, weight and colour of every allocated block equal to
    tests/tsdf_ref.py bit for bit; the pool behind the table untouched; a second fresh volume gives identical bytes."""
    _vol, first = _fuse(name)
    _vol, second = _fuse(name)
    assert first == second


@pytest.mark.parametrize("name", NAMES)
def test_blocks_per_pixel_is_the_restatements(hip_lib, name):
    case = tc.case(name)
    for v in case.views:
        H, W = v.depth.shape
        intr = (ctypes.c_float * 4)(*[float(x) for x in v.intr])
        got = hip_lib.g4s_tsdf_blocks_per_pixel(W, H, intr, case.voxel, case.T)
        assert got == tsdf_ref.blocks_per_pixel(W, H, v.intr, case.voxel, case.T)


@pytest.mark.parametrize("name", ["oblique_long", "merge_sequence"])
def test_pool_edges(hip_lib, name):
    """A pool the first view fills exactly does not grow, one block less grows once; a pool grown from one block holds
    the same table and voxels after every view as a large one.  Every run starts from a poisoned pool (tsdf NaN, weight
    1, colour 1e9) and _fuse checks after each view that the slots beyond the table still hold it and that the blocks the
    view did not touch are unchanged: tsdf_init_kernel writes the new slots only."""
    steps, _ref = tc.reference(name)
    n1 = steps[0].counts[1]
    first_view = tc.Case(name, *tc.case(name)[1:4], tc.case(name).views[:1])
    for blocks, grows in ((n1, 0), (n1 - 1, 1)):
        vol = _volume(first_view, blocks, poison=True)
        v = first_view.views[0]
        assert vol.integrate(dev(v.depth), dev(v.rgb), v.cam, dev(v.mask)) == (n1, n1)
        torch.cuda.synchronize()
        assert vol.grows == grows and vol.num_blocks == n1
        assert vol.pool_blocks == (n1 if grows == 0 else max(n1, 2 * (n1 - 1)))
        for g, new in zip(_pool(vol, n1), (steps[0].tsdf, steps[0].weight, steps[0].color)):
            assert np.array_equal(g[steps[0].touched_slots], words(new).reshape(n1, -1))
        assert _poison_intact(vol, n1)
    big_vol, big = _fuse(name)
    small_vol, small = _fuse(name, initial_blocks=1)
    assert big_vol.grows == 0 and small_vol.grows >= (1 if len(steps) == 1 else 3)
    assert big == small


@pytest.mark.parametrize("name", ["oblique_long", "small_73x2", "small_117x5"])
def test_workspace_is_enough(hip_lib, name):
    """g4s_tsdf_alloc_count, g4s_tsdf_merge and g4s_tsdf_integrate, called the way TSDFVolume.integrate calls them but
    with exactly g4s_tsdf_workspace(W, H, cap, 0) bytes: the 4096 bytes of 0xA5 behind them stay as they were and the results
    are the reference's.  The view is fused twice, so the second round runs against a table."""
    case = tc.case(name)
    steps, _ref = tc.reference(name)
    v, s = case.views[0], steps[0]
    H, W = v.depth.shape
    f4 = lambda a: (ctypes.c_float * len(a))(*[float(x) for x in a])
    intr, ext = f4(v.intr), f4(np.asarray(v.E, np.float32).reshape(-1))
    cap = hip_lib.g4s_tsdf_blocks_per_pixel(W, H, intr, case.voxel, case.T)
    assert cap == tsdf_ref.blocks_per_pixel(W, H, v.intr, case.voxel, case.T)
    nbytes = int(hip_lib.g4s_tsdf_workspace(W, H, cap, 0))
    tail = 4096
    # the workspace starts one byte into the allocation: the library aligns it to 256 itself, which uses up the slack
    # g4s_tsdf_workspace() adds for that, so its last array ends within 255 bytes of the canary
    buf = torch.full((1 + nbytes + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = buf[1:]
    depth, rgb, mask = dev(v.depth), dev(v.rgb), dev(v.mask)
    n = s.counts[0]
    pool = n + 3
    tsdf = torch.full((pool * 512,), POISON[0], device=DEV)
    weight = torch.full((pool * 512,), POISON[1], device=DEV)
    color = torch.full((pool * 1536,), POISON[2], device=DEV)
    keys = torch.zeros(1, dtype=torch.int64, device=DEV)
    slots = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = _lib.stream(DEV)
    P, size = _lib.ptr, ctypes.c_size_t(nbytes)
    n_blocks = 0
    for rnd in range(2):
        counts = (ctypes.c_int * 2)()
        rc = hip_lib.g4s_tsdf_alloc_count(W, H, P(depth), P(mask), intr, ext, case.voxel, case.T, case.depth_trunc, cap,
                                          P(keys), n_blocks, counts, P(ws), size, stream)
        assert rc == 0, _lib.last_error()
        assert (counts[0], counts[1]) == ((n, n) if rnd == 0 else (n, 0))
        keys_out = torch.empty(n_blocks + counts[1], dtype=torch.int64, device=DEV)
        slots_out = torch.empty(n_blocks + counts[1], dtype=torch.int32, device=DEV)
        rc = hip_lib.g4s_tsdf_merge(W, H, cap, P(keys), P(slots), n_blocks, counts[0], counts[1], P(keys_out), P(slots_out),
                                    P(tsdf), P(weight), P(color), pool, P(ws), size, stream)
        assert rc == 0, _lib.last_error()
        keys, slots, n_blocks = keys_out, slots_out, n_blocks + counts[1]
        rc = hip_lib.g4s_tsdf_integrate(W, H, P(depth), P(mask), P(rgb), intr, ext, case.voxel, case.T, case.depth_trunc, cap,
                                        counts[0], P(tsdf), P(weight), P(color), pool, P(ws), size, stream)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert (ws[nbytes:] == 0xA5).all().item() and buf[0].item() == 0xA5, "bytes outside the workspace were written"
        assert np.array_equal(keys.cpu().numpy(), s.keys) and np.array_equal(slots.cpu().numpy(), s.slots)
    ref = tsdf_ref.RefVolume(case.voxel, case.T, case.depth_trunc)
    for _ in range(2):
        ref.integrate(v.depth, v.rgb, v.intr, v.E, v.mask)
    for got, want, per, p in zip((tsdf, weight, color), (ref.tsdf, ref.weight, ref.color), (512, 512, 1536), POISON):
        got = words(host(got)).reshape(pool, per)
        assert np.array_equal(got[:n], words(want).reshape(n, per))
        assert (got[n:] == words(np.float32(p))).all()
