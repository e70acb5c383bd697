"""One-view-per-rank data parallelism over `gloo`, world_size 2, on CPU:
the all-reduced gradient bucket equals the sum of the single-process gradients over the same views
(no optimiser step in between), the side channel follows the per-view-norm semantics, and both
replicas stay identical after the Adam step."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _setup_paths():
    root = os.path.dirname(HERE)
    for p in (root, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)


def _views(n, W=48, H=40):
    from g4splat_amd import synthetic
    out = []
    for i in range(n):
        a = 0.5 * i
        cam = synthetic.look_at_camera((2.5 * np.sin(a), 0.2 * i, -2.5 * np.cos(a)), (0, 0, 0), (0, 1, 0), 1.0, W, H)
        out.append(SimpleNamespace(image_width=W, image_height=H, FoVx=cam.FoVx, FoVy=cam.FoVy,
                                   world_view_transform=torch.tensor(cam.world_view_transform),
                                   full_proj_transform=torch.tensor(cam.full_proj_transform),
                                   camera_center=torch.tensor(cam.camera_center), znear=0.01, zfar=100.0))
    return out


def _model(seed=0, P=150):
    from g4splat_amd.gaussian_model import GaussianModel
    rng = np.random.default_rng(seed)
    m = GaussianModel(sh_degree=3)
    m.create_from_parameters(torch.tensor(rng.uniform(-0.8, 0.8, (P, 3)).astype(np.float32)),
                             torch.tensor(rng.uniform(0.05, 0.2, (P, 2)).astype(np.float32)),
                             torch.tensor(rng.normal(size=(P, 4)).astype(np.float32)),
                             torch.tensor(rng.uniform(0, 1, (P, 3)).astype(np.float32)))
    with torch.no_grad():
        m._opacity += 2.0
        m._features_rest += torch.tensor(rng.normal(0, 0.05, tuple(m._features_rest.shape)).astype(np.float32))
    m.active_sh_degree = 2
    return m


def _step(model, views, vp):
    from cpu_rasterizer import oracle_backend
    from g4splat_amd.gaussian_renderer import render
    pipe = SimpleNamespace(depth_ratio=0.5, compute_cov3D_python=False)
    for v in views:
        with oracle_backend():
            out = render(v, model, pipe, torch.tensor([0.0, 0.1, 0.2]))
        loss = (out["render"] ** 2).mean() + 0.1 * out["rend_dist"].mean() + 0.05 * out["rend_alpha"].mean()
        loss.backward()
        vp.record_view(out["viewspace_points"], out["visibility_filter"], out["radii"])


def _worker(rank, world, port, q, compact_below, exchange="allreduce"):
    _setup_paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from g4splat_amd.parallel import ViewParallel, broadcast_parameters, shard_views
    torch.set_num_threads(1)
    model = _model(seed=rank)  # deliberately different replicas: the broadcast must fix that
    broadcast_parameters(model.parameters(), src=0)
    model.training_setup()
    vp = ViewParallel(model.parameters(), compact_below=compact_below, exchange=exchange)
    views = _views(4)
    mine = shard_views(views, rank, world)
    assert len(mine) == 4 // world
    _step(model, mine, vp)
    stats = vp.all_reduce()
    flat = vp.bucket.flat.clone()
    if exchange == "allreduce":
        assert vp._reducer.last_rows == (150 if compact_below == 0.0 else int((stats["max_radii"] > 0).sum()))
    model.optimizer.step()
    q.put((rank, flat.numpy(), stats["grad_norm_sum"].numpy(), stats["vis_count"].numpy(), stats["max_radii"].numpy(),
           torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("compact_below,exchange,world", [(0.0, "allreduce", 2), (1.1, "allreduce", 2), (0.7, "owner", 2),
                                                          (0.7, "owner", 4)])
def test_view_parallel_matches_single_process(compact_below, exchange, world):
    """dense all-reduce / visible-rows all-reduce / owner-reduce (2 and 4 ranks): the reduced bucket equals the sum of the
    single-process gradients over the same views, the statistics follow the reference's semantics, replicas stay identical."""
    _setup_paths()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + (7 if compact_below else 0) + (13 if exchange == "owner" else 0) + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, compact_below, exchange)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r = q.get(timeout=240)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    # single-process reference: all four views on one replica, gradients accumulated, no step in between
    from g4splat_amd.parallel import ViewParallel
    model = _model(seed=0)
    model.training_setup()
    vp = ViewParallel(model.parameters())
    _step(model, _views(4), vp)
    ref = vp.bucket.flat.numpy()
    for r in range(world):
        flat, gsum, cnt, rad, params = res[r]
        assert np.abs(flat - ref).max() <= 1e-3 * np.abs(ref).max()
        np.testing.assert_allclose(gsum, vp.grad_norm_sum.numpy(), rtol=1e-4, atol=1e-7)
        np.testing.assert_array_equal(cnt, vp.vis_count.numpy())
        np.testing.assert_array_equal(rad, vp.max_radii.numpy())
    # replicas identical after the step (deterministic Adam on identical reduced gradients)
    for r in range(1, world):
        np.testing.assert_array_equal(res[0][4], res[r][4])
        np.testing.assert_array_equal(res[0][0], res[r][0])  # and the reduced gradients are the same bits everywhere
    # 58 floats per Gaussian in the bucket
    assert ref.size == 150 * 58


def test_bucket_views_survive_zero_grad():
    _setup_paths()
    from g4splat_amd.parallel import GradientBucket
    ps = [torch.nn.Parameter(torch.ones(4, 3)), torch.nn.Parameter(torch.ones(4, 1))]
    b = GradientBucket(ps)
    (ps[0].sum() * 2 + ps[1].sum() * 3).backward()
    assert b.flat.tolist() == [2.0] * 12 + [3.0] * 4
    opt = torch.optim.Adam(ps)
    opt.zero_grad(set_to_none=True)
    b.zero()
    (ps[0].sum()).backward()
    assert b.flat.tolist() == [1.0] * 12 + [0.0] * 4


def _sparse_worker(rank, world, port, q):
    _setup_paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from g4splat_amd.parallel import RowSparseAllReduce
    P = 1000
    out = []
    for frac in (0.0, 0.05, 0.5, 1.0):
        g = torch.Generator().manual_seed(17)
        union = torch.rand(P, generator=g) < frac  # same mask on every rank
        mine = union & (torch.rand(P, generator=torch.Generator().manual_seed(100 + rank)) < 0.7)
        flat = torch.zeros(P * 7)
        rows = [flat[:3 * P].view(P, 3), flat[3 * P:].view(P, 4)]
        vals = torch.randn(P, 7, generator=torch.Generator().manual_seed(200 + rank))
        rows[0][mine] = vals[mine, :3]
        rows[1][mine] = vals[mine, 3:]
        dense = flat.clone()
        dist.all_reduce(dense)
        red = RowSparseAllReduce(flat, rows, compact_below=0.7)
        red.reduce(union)
        out.append((frac, bool(torch.equal(flat, dense)), red.last_rows, int(union.sum())))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_row_sparse_all_reduce_equals_dense():
    """Packed visible-rows exchange == dense all-reduce bit for bit (same two addends per row), for empty, small,
    medium and full unions (the last one takes the dense path)."""
    _setup_paths()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sparse_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        for frac, same, rows, n in res[r]:
            assert same, (r, frac)
            assert rows == (1000 if n > 700 else n), (frac, rows, n)


def _owner_worker(rank, world, port, q):
    _setup_paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from g4splat_amd.parallel import OwnerReduce
    out = []
    gathers = set()
    for P, frac, exact in ((1000, 0.3, True), (1003, 0.6, True), (257, 1.0, True), (64, 0.0, True), (1000, 0.3, False),
                           (1003, 0.05, False)):
        vis = torch.rand(P, generator=torch.Generator().manual_seed(100 + rank + 17 * P)) < frac
        flat = torch.zeros(P * 7)
        rows = [flat[:3 * P].view(P, 3), flat[3 * P:].view(P, 4)]
        g = torch.Generator().manual_seed(200 + rank)
        # exact: small integers / 8 -> every partial sum is exactly representable, so ANY summation order gives the
        # same bits and the comparison with the dense all-reduce is a bit-for-bit one at any world size
        vals = (torch.randint(-64, 64, (P, 7), generator=g).float() / 8) if exact else torch.randn(P, 7, generator=g)
        rows[0][vis] = vals[vis, :3]
        rows[1][vis] = vals[vis, 3:]
        dense = flat.clone()
        dist.all_reduce(dense)
        red = OwnerReduce(rows)
        red.debug_checks = True      # finish() verifies its precondition: unflagged rows hold zeros
        radii = vis.to(torch.int32) * 5
        red.begin(vis, radii=radii)  # (with the radii the exchange knows the union of the visible sets: sparse gather)
        red.finish()
        gathers.add(red.last_gather)
        if exact or world == 2:  # two addends commute: bit-identical for any values
            ok = bool(torch.equal(flat, dense))
        else:
            ok = bool((flat - dense).abs().max() <= 1e-6 * dense.abs().max())
        # RANK ORDER (round 6): whatever the values and whoever owns a row, the result is (((0 + g_0) + g_1) + ...) + g_{N-1} --
        # what one process accumulating the ranks' contributions one after the other computes -- bit for bit
        mine = torch.zeros(P * 7)
        mine[:3 * P].view(P, 3)[vis] = vals[vis, :3]
        mine[3 * P:].view(P, 4)[vis] = vals[vis, 3:]
        everyone = [torch.zeros(P * 7) for _ in range(world)]
        dist.all_gather(everyone, mine)
        seq = torch.zeros(P * 7)
        for g_r in everyone:
            seq += g_r
        ok = ok and bool(torch.equal(flat, seq))
        # determinism of the owner's summation order: a second exchange of the same inputs gives the same bits
        flat2 = torch.zeros(P * 7)
        rows2 = [flat2[:3 * P].view(P, 3), flat2[3 * P:].view(P, 4)]
        rows2[0][vis] = vals[vis, :3]
        rows2[1][vis] = vals[vis, 3:]
        red2 = OwnerReduce(rows2)
        red2.sparse_below = 0.0       # the dense gather, for comparison
        red2.begin(vis)
        red2.finish()
        gathers.add(red2.last_gather)
        out.append((P, frac, exact, ok, bool(torch.equal(flat, flat2)), red.last_rows_sent, int(vis.sum()), red.last_order))
    # only the radii of rows a rank FLAGS take part in the MAX (the reference updates max_radii2D under the
    # visibility filter, train_with_refine_depth.py:583), and debug_checks refuses a non-zero unflagged row
    P = 64
    rows = [torch.zeros(P, 3)]
    vis = torch.zeros(P, dtype=torch.bool)
    vis[rank::world] = True
    rows[0][vis] = 1.0
    radii = torch.full((P,), 3 + rank, dtype=torch.int32)  # also where this rank does not see the row
    red = OwnerReduce(rows)
    red.debug_checks = True
    red.begin(vis, radii=radii)
    red.finish()
    want = (torch.arange(P) % world + 3).to(red.max_radii.dtype)  # row i is seen by rank i % world only
    radii_ok = bool(torch.equal(red.max_radii, want)) and bool(torch.equal(rows[0], torch.ones(P, 3)))
    rows[0][(rank + 1) % world::world] += 0.5   # a value in a row this rank does not flag
    red.begin(vis, radii=radii)
    try:
        red.finish()
        refused = False
    except RuntimeError as e:
        refused = "not flagged visible" in str(e)
    out.append((radii_ok, refused))
    out.append(sorted(g for g in gathers if g))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_owner_reduce_equals_dense_all_reduce(world):
    """OwnerReduce (all_to_all of visible rows to index-shard owners, all_gather of the reduced shards) against the dense
    SUM all-reduce: bit-identical on exactly representable values at 2, 4 and 8 ranks (ragged last shard, empty and full
    visibility included), bit-identical on arbitrary values at 2 ranks, equal to rounding at 4 and 8, and bit-reproducible;
    and at every world size, for arbitrary values, THE SAME BITS as adding the ranks' contributions one after the other in
    rank order (`OwnerReduce.rank_order`: an N-rank step reproduces single-process gradient accumulation)."""
    _setup_paths()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_owner_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        assert res[r][-2] == (True, True), res[r][-2]
        for P, frac, exact, ok, same_again, sent, nvis, order in res[r][:-2]:
            assert ok, (r, P, frac, exact)
            assert order == "rank", (r, P, frac, order)  # (at most 7 sources: the sums are in rank order)
            assert same_again, (r, P, frac)       # (sparse gather with radii == dense gather without: the same bits)
            assert 0 <= sent <= nvis
        assert res[r][-1] == ["dense", "sparse"], res[r][-1]  # both forms of the gather ran (small and large unions)


def test_owner_addition_order_is_decided_once():
    """OwnerReduce.addition_order(), the one rule both backends follow, over every (world <= 10, rank, set of live
    sources): the rank-ordered path exactly where the device code has always taken it (rank_order on, a source below the
    owner, 2 to 8 sources), the one-launch / per-source split at ONE_LAUNCH_SOURCES otherwise, and the recorded order
    "owner" exactly when more than 8 sources arrive or rank_order is off."""
    _setup_paths()
    from itertools import combinations
    from g4splat_amd.parallel import OwnerReduce
    assert OwnerReduce.ONE_LAUNCH_SOURCES == 4 and OwnerReduce.ORDERED_SOURCES == 8
    for world in range(1, 11):
        for rank in range(world):
            others = [s for s in range(world) if s != rank]
            for k in range(len(others) + 1):
                for live in combinations(others, k):
                    for rank_order in (True, False):
                        path, order = OwnerReduce.addition_order(list(live), rank, rank_order)
                        below = any(s < rank for s in live)
                        assert (path == "rank") == (rank_order and below and 2 <= k <= 8), (world, rank, live, rank_order)
                        if path != "rank":
                            assert path == ("one_launch" if k >= 4 else "per_source"), (world, rank, live, rank_order)
                        assert order == ("owner" if (not rank_order or k > 8) else "rank"), (world, rank, live, rank_order)


def _zero1_worker(rank, world, port, q):
    _setup_paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from g4splat_amd.parallel import OwnerReduce, ShardedAdam, adam_update_
    out = []
    widths = (3, 45, 1, 2, 4)           # xyz, SH rest, opacity, scaling, rotation
    lrs = (1.6e-4, 1.25e-4, 0.05, 0.005, 0.001)
    for P in (96, 101):                 # equal shards (in-place gather) and ragged shards (staging buffer)
        gen = torch.Generator().manual_seed(7)       # the same replica everywhere
        params_a = [torch.randn(P, w, generator=gen) for w in widths]
        params_b = [p.clone() for p in params_a]
        grads_a = [torch.zeros(P, w) for w in widths]
        grads_b = [torch.zeros(P, w) for w in widths]
        side_a, side_b = torch.zeros(P, 2), torch.zeros(P, 2)
        m_full = [torch.zeros(P, w) for w in widths]
        v_full = [torch.zeros(P, w) for w in widths]
        red_a = OwnerReduce(grads_a + [side_a])
        red_b = OwnerReduce(grads_b + [side_b])
        opt = ShardedAdam(params_b, grads_b, red_b, lrs, eps=1e-15)
        allocs = None
        for it in range(4):
            g = torch.Generator().manual_seed(1000 * it + rank)
            vis = torch.rand(P, generator=g) < 0.4
            radii = (torch.rand(P, generator=g) * 50).to(torch.int32) * vis
            for ga, gb, w in zip(grads_a, grads_b, widths):
                vals = torch.randn(P, w, generator=g)
                ga.zero_(); gb.zero_()
                ga[vis] = vals[vis]; gb[vis] = vals[vis]
            for sd in (side_a, side_b):
                sd.zero_(); sd[vis, 0] = 1.0 + rank; sd[vis, 1] = 1.0
            # (A) replicated optimiser: gradients gathered, every rank steps everything
            red_a.begin(vis, radii=radii); red_a.finish()
            for p_, g_, m_, v_, lr in zip(params_a, grads_a, m_full, v_full, lrs):
                adam_update_(p_, g_, m_, v_, lr, it + 1, eps=1e-15)
            # (B) owner-applied: each rank steps its shard, the parameters (and the statistics) are gathered
            red_b.begin(vis, radii=radii); red_b.finish(gather=False); opt.step(extra=[side_b])
            if it == 1:
                allocs = (red_a.allocations, red_b.allocations)
            rmax = radii.clone(); dist.all_reduce(rmax, op=dist.ReduceOp.MAX)
            assert torch.equal(red_a.max_radii, rmax) and torch.equal(red_b.max_radii, rmax)
        same_params = all(torch.equal(a, b) for a, b in zip(params_a, params_b))
        same_side = torch.equal(side_a, side_b)
        ea, es = opt.full_state()
        same_state = all(torch.equal(a, b) for a, b in zip(ea, m_full)) and all(torch.equal(a, b) for a, b in zip(es, v_full))
        lo, hi = red_b.bounds()
        shard_only = all(t.shape[0] == hi - lo for t in opt.exp_avg)
        no_realloc = (red_a.allocations, red_b.allocations)
        # a densification changes P and with it the shard boundaries: the moments are gathered, edited like the
        # (replicated) parameters -- here: every third row pruned -- and re-sharded; one more step on each side
        keep = torch.ones(P, dtype=torch.bool)
        keep[::3] = False
        P2 = int(keep.sum())
        params_a = [p_[keep].contiguous() for p_ in params_a]
        params_b = [p_[keep].contiguous() for p_ in params_b]
        m_full = [t_[keep].contiguous() for t_ in m_full]
        v_full = [t_[keep].contiguous() for t_ in v_full]
        grads_a = [torch.zeros(P2, w) for w in widths]
        grads_b = [torch.zeros(P2, w) for w in widths]
        side_a, side_b = torch.zeros(P2, 2), torch.zeros(P2, 2)
        red_a, red_b = OwnerReduce(grads_a + [side_a]), OwnerReduce(grads_b + [side_b])
        opt.load_full_state(params_b, grads_b, red_b, [t_[keep] for t_ in ea], [t_[keep] for t_ in es])
        g = torch.Generator().manual_seed(777 + rank)
        vis = torch.rand(P2, generator=g) < 0.5
        for ga, gb, w in zip(grads_a, grads_b, widths):
            vals = torch.randn(P2, w, generator=g)
            ga[vis] = vals[vis]; gb[vis] = vals[vis]
        red_a.begin(vis); red_a.finish()
        for p_, g_, m_, v_, lr in zip(params_a, grads_a, m_full, v_full, lrs):
            adam_update_(p_, g_, m_, v_, lr, 5, eps=1e-15)
        red_b.begin(vis); red_b.finish(gather=False); opt.step(extra=[side_b])
        same_params = same_params and all(torch.equal(a, b) for a, b in zip(params_a, params_b))
        lo2, hi2 = red_b.bounds()
        shard_only = shard_only and all(t.shape[0] == hi2 - lo2 for t in opt.exp_avg)
        digest = torch.cat([p.reshape(-1) for p in params_b]).double().sum().item()
        out.append((P, same_params, same_side, same_state, shard_only, allocs, no_realloc, digest))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_owner_applied_adam_equals_the_replicated_optimiser(world):
    """ZeRO-1 behind OwnerReduce (verdict r2 item 3c): the owner steps its shard and the all_gather carries parameters.
    Against the replicated optimiser on gathered gradients, over four steps at world sizes 2 / 4 / 8, equal and ragged
    shards: parameters, statistics and (gathered) optimiser state are bit-identical, the radii MAX that rides in
    begin()'s collective equals a plain MAX all-reduce, every replica ends with the same bits, optimiser state exists
    for the rank's shard only, the exchange allocates nothing after its warm-up (persistent buffers), and after a
    densification-like row edit (moments gathered, every third row pruned, state re-sharded for the new P) the next step
    still matches bit for bit."""
    _setup_paths()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_zero1_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        for i, (P, same_params, same_side, same_state, shard_only, allocs, allocs_end, digest) in enumerate(res[r]):
            assert same_params and same_side and same_state and shard_only, (r, P)
            # (persistent buffers: after the second step at most one regrowth of a send / receive buffer, plus the two
            # buffers of the sparse gather on the first step whose union is small enough to use it)
            assert allocs_end[0] <= allocs[0] + 3 and allocs_end[1] <= allocs[1] + 1, (allocs, allocs_end)
            assert digest == res[0][i][7], (r, P)


METRIC_WIDTHS = (3, 48, 1, 2, 4, 2)  # xyz, SH, opacity, scaling, rotation, statistics: 60 floats (+ the index column = 61)


def _metric_vis(P, rank, world, step):
    """Visibility of `rank` at `step`: ~28 % of the rows, NOTHING in the shard of owner (rank + 1) % world (zero-length
    all_to_all splits), and rank world - 1 sees nothing at all in odd steps (a rank with no rows to send)."""
    g = torch.Generator().manual_seed(1000 * step + rank)
    vis = torch.rand(P, generator=g) < 0.28
    shard = (P + world - 1) // world
    d = (rank + 1) % world
    vis[d * shard:min((d + 1) * shard, P)] = False
    if rank == world - 1 and step % 2 == 1:
        vis[:] = False
    return vis


def _metric_worker(rank, world, port, q, P):
    _setup_paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from g4splat_amd.parallel import OwnerReduce
    rows = [torch.zeros(P, w) for w in METRIC_WIDTHS]
    red = OwnerReduce(rows)
    base = (torch.arange(P, dtype=torch.float32) % 251) / 8          # exactly representable, so is every partial sum
    out = []
    for step in range(3):
        vis = _metric_vis(P, rank, world, step)
        radii = ((torch.arange(P) + rank) % 97).to(torch.int32) * vis
        for r in rows:
            r.zero_()
            r[vis] = (base[vis] * (rank + 1)).unsqueeze(1).expand(-1, r.shape[1])
        red.begin(vis, radii=radii)
        red.finish()
        # what every element must be: base(i) x sum of (r + 1) over the ranks that saw row i; MAX of the radii
        sample = torch.randperm(P, generator=torch.Generator().manual_seed(step))[:20000]
        coef = torch.zeros(sample.numel())
        rmax = torch.zeros(sample.numel(), dtype=torch.int32)
        for r2 in range(world):
            v2 = _metric_vis(P, r2, world, step)[sample]
            coef += v2 * (r2 + 1.0)
            rmax = torch.maximum(rmax, (((sample + r2) % 97).to(torch.int32) * v2))
        ok = all(torch.equal(r[sample], (base[sample] * coef).unsqueeze(1).expand(-1, r.shape[1])) for r in rows)
        ok_radii = torch.equal(red.max_radii[sample], rmax)
        digest = sum(r.view(torch.int32).to(torch.int64).sum().item() for r in rows)  # the bits, not the values
        out.append((ok, ok_radii, digest, red.allocations, red.last_rows_sent, dict(red.last_bytes)))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("P", [1_500_000, 1_500_003])
def test_owner_exchange_at_the_metric_row_counts_on_eight_ranks(P):
    """Verdict r3 item 3: every collective shape of the exchange at S3's size -- 1.5 M rows x 61 floats, world 8 -- on gloo:
    the [P + 64] int32 MAX all-reduce, the uneven all_to_all with zero-length splits (every rank sees nothing of one
    owner's shard; one rank sees nothing at all in odd steps), the in-place all_gather of equal shards (P = 1.5 M) and
    the padded gather of ragged ones (P = 1.5 M + 3).  Three steps on the same persistent buffers: the sums are exact
    (checked on 20 000 sampled rows against the closed form), every rank ends with the SAME BITS, and nothing is
    allocated after the first step."""
    _setup_paths()
    world = 8
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 39500 + (os.getpid() % 2000) + (P % 7)
    procs = [ctx.Process(target=_metric_worker, args=(r, world, port, q, P)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=900) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for step in range(3):
        for r in range(world):
            ok, ok_radii, digest, allocs, sent, nbytes = res[r][step]
            assert ok and ok_radii, (r, step)
            assert digest == res[0][step][2], (r, step)          # identical bits on every rank
            assert allocs == res[r][0][3], (r, step, allocs)     # nothing (re)allocated after the first step
            assert nbytes["all_to_all_sent"] == sent * 61 * 4
    assert res[world - 1][1][4] == 0                              # the rank that saw nothing sent nothing
    assert res[0][0][5]["all_gather_received"] > 300e6            # ~315 MB in, as DESIGN.md section 5 prices it


# ---- densification under data parallelism ("identical parameters after densify_and_split") ----------------
DENSIFY_STEPS = 3          # optimiser steps before and after the densification
DENSIFY_ARGS = dict(max_grad=None, min_opacity=0.005, extent=12.0, max_screen_size=None)  # max_grad: set from the scene below


def _densify_model():
    m = _model(seed=0)
    with torch.no_grad():
        m._opacity[::7] -= 6.0        # translucent rows: pruned (opacity < 0.005)
    m.training_setup()
    return m


def _densify_pack(model, exp_avg, exp_avg_sq, history):
    c = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).numpy()
    return dict(params=c(model.parameters()), exp_avg=c(exp_avg), exp_avg_sq=c(exp_avg_sq),
                accum=model.xyz_gradient_accum.numpy().copy(), denom=model.denom.numpy().copy(),
                radii=model.max_radii2D.numpy().copy(), history=history)


def _densify_dp_worker(rank, world, port, q, zero1=True, defer=False):
    """k steps through ViewParallel (+ ShardedAdam when `zero1`, else the model's own replicated Adam behind a gathered
    exchange), ONE densify_and_prune on every replica, k more steps."""
    os.environ["OMP_NUM_THREADS"] = "1"   # the checker's backward sums with OpenMP atomics: one thread = one summation order
    _setup_paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from g4splat_amd.parallel import ReplicatedDensification, ViewParallel, shard_views
    model = _densify_model()
    vp = ViewParallel(model.parameters(), exchange="owner")
    lrs = [g["lr"] for g in model.optimizer.param_groups]
    opt = vp.sharded_adam(lrs) if zero1 else None
    dz = ReplicatedDensification(model, vp, sharded=opt, base_seed=5, defer_stats=defer)
    views = _views(2)
    history = []
    gathered = []
    for it in range(1, 2 * DENSIFY_STEPS + 1):
        _step(model, shard_views(views, rank, world), vp)
        if zero1:
            vp.reduce_to_owners()
            if defer:   # the statistics stay on their owners: only the parameters are gathered
                opt.step()
                dz.add_owner_stats()
            else:
                opt.step(extra=[vp.side])
                dz.add_stats(vp.stats_after_owner_step())
        elif defer:
            vp.all_reduce(gather_stats=False)
            dz.add_owner_stats()
            model.optimizer.step()
        else:
            dz.add_stats(vp.all_reduce())
            model.optimizer.step()
        gathered.append(vp._owner.last_bytes.get("all_gather_received"))
        vp.zero()
        if it == DENSIFY_STEPS:
            before = model._xyz.shape[0]
            dz.gather_stats()   # (defer: this test derives its threshold from the statistics, so they are replicated first)
            grads = (model.xyz_gradient_accum / model.denom).nan_to_num(0.0)
            args = dict(DENSIFY_ARGS, max_grad=float(grads[grads > 0].median()))
            dz.densify_and_prune(it, **args)
            history.append((before, model._xyz.shape[0]))
            if zero1:
                assert opt.exp_avg[0].shape[0] == opt.red.bounds()[1] - opt.red.bounds()[0]  # state exists for the shard only
    if zero1:
        ea, es = opt.full_state()
    else:
        st = [model.optimizer.state[p] for p in model.parameters()]
        ea, es = [x["exp_avg"] for x in st], [x["exp_avg_sq"] for x in st]
    dz.gather_stats()  # (defer: the last interval's statistics are still owner-local; replicate them for the comparison)
    out = _densify_pack(model, ea, es, history)
    out["gathered"] = gathered
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def _densify_single_process():
    """The same schedule in ONE process without any exchange machinery: both views accumulated into one bucket, plain Adam
    over the full tensors, the statistics taken per view, densify_and_prune with the generator of the iteration."""
    os.environ["OMP_NUM_THREADS"] = "1"
    _setup_paths()
    from g4splat_amd.parallel import ViewParallel, adam_update_, densify_generator
    model = _densify_model()
    vp = ViewParallel(model.parameters())            # no process group: a gradient bucket and the per-view statistics
    lrs = [g["lr"] for g in model.optimizer.param_groups]
    m1 = [torch.zeros_like(p) for p in model.parameters()]
    m2 = [torch.zeros_like(p) for p in model.parameters()]
    views = _views(2)
    history, steps = [], 0
    for it in range(1, 2 * DENSIFY_STEPS + 1):
        _step(model, views, vp)
        steps += 1
        with torch.no_grad():
            for p, a, b, lr in zip(model.parameters(), m1, m2, lrs):
                adam_update_(p.data, p.grad, a, b, lr, steps, eps=1e-15)
            model.xyz_gradient_accum += vp.grad_norm_sum
            model.denom += vp.vis_count
            model.max_radii2D = torch.maximum(model.max_radii2D, vp.max_radii)
        vp.zero()
        if it == DENSIFY_STEPS:
            before = model._xyz.shape[0]
            grads = (model.xyz_gradient_accum / model.denom).nan_to_num(0.0)
            args = dict(DENSIFY_ARGS, max_grad=float(grads[grads > 0].median()))
            for p, a, b in zip(model.parameters(), m1, m2):
                model.optimizer.state[p] = {"step": torch.tensor(float(steps)), "exp_avg": a, "exp_avg_sq": b}
            with torch.no_grad():
                model.densify_and_prune(generator=densify_generator("cpu", it, 5), **args)
            st = [model.optimizer.state.pop(p) for p in model.parameters()]
            m1, m2 = [s["exp_avg"] for s in st], [s["exp_avg_sq"] for s in st]
            vp.rebind(model.parameters())
            history.append((before, model._xyz.shape[0]))
    return _densify_pack(model, m1, m2, history)


def _densify_single_worker(q):
    q.put(_densify_single_process())


@pytest.mark.parametrize("zero1,defer", [(True, False), (False, False), (True, True), (False, True)])
def test_densify_and_prune_under_data_parallelism_matches_the_single_process_run(zero1, defer):
    """Verdict r5 item 3: world 2, one view per rank per step, owner exchange + ZeRO-1; after three steps every replica runs
    densify_and_prune itself (clone + split + prune; the split's children drawn from the iteration's generator), re-shards
    the moments for the new row count, and trains on.  Parameters, Adam moments and densification statistics are THE SAME
    BITS on both ranks and in the single-process run of the same schedule (two views accumulated, full-tensor Adam, no
    exchange code at all).  Reference behaviour: gaussian_model.py:586-647, train_with_refine_depth.py:583-593.
    defer=True: the statistics columns stay on their owners between densifications (ReplicatedDensification(defer_stats=True))
    and are gathered once for the edit -- same bits.  zero1=False: the same through the gathered exchange and the model's own (replicated) torch.optim.Adam -- the replicas
    hold the same bits and made the same edit; against the single-process run (whose Adam is this repository's plain
    formula, not torch's kernel) the parameters agree to rounding."""
    _setup_paths()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = 2
    port = 41500 + (os.getpid() % 2000) + (17 if zero1 else 0) + (31 if defer else 0)
    procs = [ctx.Process(target=_densify_dp_worker, args=(r, world, port, q, zero1, defer)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    q1 = ctx.Queue()
    single = ctx.Process(target=_densify_single_worker, args=(q1,))   # (its own process: OMP_NUM_THREADS has to be set before the checker loads)
    single.start()
    ref = q1.get(timeout=600)
    single.join(timeout=60)
    (before, after), = ref["history"]
    assert before == 150 and after != before
    for r in range(world):
        assert res[r]["history"] == ref["history"], (r, res[r]["history"], ref["history"])
        for key in ("params", "exp_avg", "exp_avg_sq", "accum", "denom", "radii"):
            np.testing.assert_array_equal(res[r][key], res[0][key], err_msg=f"rank {r} vs rank 0: {key}")
            if zero1:
                np.testing.assert_array_equal(res[r][key], ref[key], err_msg=f"rank {r}: {key}")
            else:
                np.testing.assert_allclose(res[r][key], ref[key], rtol=2e-4, atol=1e-6, err_msg=f"rank {r}: {key}")
    if defer and not zero1:
        # the per-step gather carried 58 of the 60 floats per row (the dense form; steps whose union of visible rows is small
        # take the sparse gather, which moves everything)
        P0 = 150
        dense_58 = [g for g in res[0]["gathered"] if g == (P0 - P0 // world) * 58 * 4]
        assert dense_58 or all(g < (P0 - P0 // world) * 58 * 4 for g in res[0]["gathered"][:DENSIFY_STEPS]), res[0]["gathered"]
    # the edit did all three things: rows were cloned and split (more rows than kept ones) and pruned
    assert after > before - (before + 6) // 7
