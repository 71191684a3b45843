"""shard_device.shard_scene_on_device on CPU tensors (the torch-op restatement of csrc/scene_shard.hip)
against the host path, dist_train.shard_device_scene / distributed.shard_scene, on the same scene.

Everything compared is an integer array or a bit copy: every comparison is torch.equal (with equal
dtypes), for every rank of world 1, 2, 3 and 8, with and without camera sharding."""
import numpy as np
import pytest
import torch

from gasfm_amd import synthetic
from gasfm_amd.attention import camera_max_piece
from gasfm_amd.dist_train import _HostEdges, shard_device_scene
from gasfm_amd.distributed import shard_scene
from gasfm_amd.scene import SceneData, SparseMat
from gasfm_amd.shard_device import shard_scene_on_device

WORLDS = (1, 2, 3, 8)
PLAN_ARRAYS = ("seg_ptr", "perm", "pos", "items", "combine", "combine_l1")
PLAN_SCALARS = ("n_slots", "num_targets", "num_edges", "src_rows", "all_partial", "max_piece")


# ------------------------------------------------------------------ scenes
def _from_edges(m, n, cam, pt, seed):
    return synthetic._sorted(m, n, np.asarray(cam), np.asarray(pt), np.random.default_rng(seed))


def sweep_scene(m=12, n=300, degrees=(2, 3, 4), seed=5, full_camera=None):
    """Point j is seen by k_j consecutive cameras starting near j * m / n: a point range touches a few
    neighbouring cameras only, so most cameras have no edge in a 1/8 shard.  full_camera: a camera that
    sees every point as well (its local segment is longer than camera_max_piece of a small shard)."""
    rng = np.random.default_rng(seed)
    k = rng.choice(np.asarray(degrees), size=n)
    start = np.minimum((np.arange(n) * m) // n, m - k)
    pairs = {(int(start[j]) + i, j) for j in range(n) for i in range(int(k[j]))}
    if full_camera is not None:
        pairs |= {(full_camera, j) for j in range(n)}
    cam, pt = zip(*sorted(pairs))
    return _from_edges(m, n, cam, pt, seed)


def block_scene(m=6, per=8, seed=7):
    """Camera c sees the points [c * per, (c + 1) * per) and no other: the cam-major edge list is
    point-sorted too (the scene's point-direction plan has no permutation)."""
    cam = np.repeat(np.arange(m), per)
    return _from_edges(m, m * per, cam, np.arange(m * per), seed)


def scene_data(sc, device="cpu"):
    """(clean scene, network input scene with other values on the same edges) with pixel measurements."""
    d = SceneData.from_synthetic(sc).to(device)
    d.pixel_xy = torch.from_numpy(sc.xy).to(device)
    inp = SceneData.__new__(SceneData)
    inp.__dict__.update(d.__dict__)
    x = d.x
    inp.x = SparseMat(x.values * 1.5 + 0.25, x.indices, x.cam_per_pts, x.pts_per_cam, x.shape)
    return d, inp


# ------------------------------------------------------------------ comparison
def same(a, b, what):
    assert (a is None) == (b is None), f"{what}: one side is None"
    if a is not None:
        assert a.dtype == b.dtype and a.shape == b.shape, \
            f"{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
        assert a.device == b.device, f"{what}: {a.device} vs {b.device}"
        assert torch.equal(a, b), what


def same_plan(p, q, what):
    for k in PLAN_ARRAYS:
        same(getattr(p, k), getattr(q, k), f"{what}.{k}")
    for k in PLAN_SCALARS:
        assert getattr(p, k) == getattr(q, k), f"{what}.{k}: {getattr(p, k)} vs {getattr(q, k)}"
    assert p.tag == q.tag, what


def same_shard(got, ref, what, loss=False):
    """One shard (network's or loss's) of the new path against the host path's."""
    same(got.x.indices, ref.x.indices, f"{what} x.indices")
    same(got.x.values, ref.x.values, f"{what} x.values")
    same(got.x.cam_per_pts, ref.x.cam_per_pts, f"{what} cam_per_pts")
    same(got.x.pts_per_cam, ref.x.pts_per_cam, f"{what} pts_per_cam")
    assert tuple(got.x.shape) == tuple(ref.x.shape), what
    assert got.point_slice == ref.point_slice, f"{what} point_slice {got.point_slice} vs {ref.point_slice}"
    assert getattr(got, "camera_slice", None) == getattr(ref, "camera_slice", None), f"{what} camera_slice"
    assert got.n_global == ref.n_global and got.n_edges_global == ref.n_edges_global, what
    assert (got.shard.rank, got.shard.world, got.shard.cams, got.shard.emulate) == \
        (ref.shard.rank, ref.shard.world, ref.shard.cams, ref.shard.emulate), what
    assert set(got.graph_wrappers) == set(ref.graph_wrappers) and set(got.partial_plans) == set(ref.partial_plans)
    for k, w in ref.graph_wrappers.items():
        same_plan(got.graph_wrappers[k].plan, w.plan, f"{what} plan {k}")
        same(got.graph_wrappers[k].valid_indices, w.valid_indices, f"{what} {k}.valid_indices")
        if k != "view2global":  # the host's keeps the edge_index of the shard's own valid views (unused)
            same(got.graph_wrappers[k].edge_index, w.edge_index, f"{what} {k}.edge_index")
    for k, p in ref.partial_plans.items():
        same_plan(got.partial_plans[k], p, f"{what} partial plan {k}")
    if loss:
        same(got.xy, ref.xy, f"{what} xy")
        assert got.Ns is ref.Ns and got.Ns_invT is ref.Ns_invT


def check_all_ranks(d, inp, worlds=WORLDS, max_piece=None, **kw):
    """Every rank of every world, cameras False and True, against shard_device_scene; returns the host
    shards' point slices and local edge counts."""
    seen = []
    for world in worlds:
        for cameras in (False, True):
            for rank in range(world):
                ref_net, ref_loss = shard_device_scene(d, rank, world, inp, cameras=cameras, max_piece=max_piece)
                sl = ref_net.point_slice
                assert sl.stop > sl.start, "choose scenes in which every rank owns a point"
                net, loss = shard_scene_on_device(d, rank, world, inp, cameras=cameras, max_piece=max_piece, **kw)
                what = f"world {world} rank {rank} cameras {cameras}"
                same_shard(net, ref_net, what + " net")
                same_shard(loss, ref_loss, what + " loss", loss=True)
                assert loss.shard is net.shard and loss.graph_wrappers is net.graph_wrappers
                assert not torch.equal(net.x.values, loss.x.values)
                seen.append((world, rank, cameras, sl, ref_net, net))
    return seen


# ------------------------------------------------------------------ tests
def test_sweep_scene_with_empty_camera_segments():
    d, inp = scene_data(sweep_scene())
    seen = check_all_ranks(d, inp)
    empty = [int((net.x.pts_per_cam == 0).sum()) for w, _, _, _, _, net in seen if w == 8]
    # 6 or 7 of the 12 cameras have no edge in a 1/8 shard: the local cam_ptr has empty segments
    assert min(empty) >= 6 and 2 * sum(e > 6 for e in empty) > len(empty)
    # camera sharding at world 8 leaves ranks 6 and 7 without camera rows: plans without any source
    last = [net for w, r, c, _, _, net in seen if w == 8 and r == 7 and c][0]
    assert last.camera_slice == slice(12, 12) and last.partial_plans["view2global"].num_edges == 0


def test_rank_boundary_exactly_on_a_point_boundary():
    """Equal degrees and n divisible by world: pt_ptr[i] * world == E * r at every boundary."""
    sc = sweep_scene(m=12, n=48, degrees=(3,), seed=11)
    d, inp = scene_data(sc)
    seen = check_all_ranks(d, inp)
    for world, rank, _, sl, _, _ in seen:
        assert (sl.start, sl.stop) == (rank * 48 // world, (rank + 1) * 48 // world)


def test_point_sorted_scene_has_no_permutation():
    d, inp = scene_data(block_scene())
    assert d.graph_wrappers["proj2scenepoint"].plan.perm is None
    seen = check_all_ranks(d, inp)  # 48 points of one view each: every rank of 8 owns six
    for _, _, _, _, _, net in seen:
        assert net.graph_wrappers["proj2scenepoint"].plan.perm is None
        assert net.graph_wrappers["scenepoint2global"].plan.num_edges == 0  # one view per point: none valid


def test_split_camera_segment():
    d, inp = scene_data(sweep_scene(full_camera=3, seed=13))
    seen = check_all_ranks(d, inp)
    split = 0
    for world, _, _, _, _, net in seen:
        plan = net.graph_wrappers["proj2view"].plan
        assert plan.max_piece == camera_max_piece(plan.num_edges)
        longest = int(net.x.pts_per_cam.max())
        assert (plan.combine.shape[0] > 0) == (longest > plan.max_piece)
        split += plan.combine.shape[0] > 0
    assert split >= 2 * (1 + 2 + 3)  # camera 3 is split in every shard of world 1, 2 and 3


def test_explicit_max_piece_and_two_level_combine():
    """max_piece = 2: the camera that sees all 300 points splits into 150 pieces, more than
    attention.L1_THRESHOLD, so the device-built plans carry a level-1 combine."""
    d, inp = scene_data(sweep_scene(full_camera=3, seed=13))
    seen = check_all_ranks(d, inp, worlds=(1, 3), max_piece=2)
    assert seen[0][5].graph_wrappers["proj2view"].plan.combine_l1 is not None
    assert seen[0][5].partial_plans["proj2view"].combine_l1 is not None


def test_explicit_point_bounds():
    d, inp = scene_data(sweep_scene())
    host = _HostEdges(d, inp.x.values)
    for bounds in ([0, 100, 101, 300], [0, 0, 250, 300], np.array([0, 7, 290, 300])):
        for cameras in (False, True):
            for rank in range(3):
                if bounds[rank + 1] == bounds[rank]:
                    continue  # an empty shard: not compared
                ref = shard_scene(host, rank, 3, cameras=cameras, point_bounds=bounds)
                net, loss = shard_scene_on_device(d, rank, 3, inp, cameras=cameras, point_bounds=bounds)
                same_shard(net, ref, f"bounds {list(bounds)} rank {rank} cameras {cameras}")
                assert net.point_slice == slice(int(bounds[rank]), int(bounds[rank + 1]))
                sel = torch.nonzero((d.x.indices[1] >= bounds[rank]) & (d.x.indices[1] < bounds[rank + 1])).view(-1)
                assert torch.equal(net.edge_ids, sel)
                assert torch.equal(loss.x.values, d.x.values[sel]) and torch.equal(loss.xy, d.pixel_xy[sel])
    for bad in ([0, 100, 300], [1, 100, 200, 300], [0, 100, 200, 299], [0, 200, 100, 300]):
        with pytest.raises(ValueError, match="point_bounds must be 4 non-decreasing"):
            shard_scene(host, 0, 3, point_bounds=bad)
        with pytest.raises(ValueError, match="point_bounds must be 4 non-decreasing"):
            shard_scene_on_device(d, 0, 3, inp, point_bounds=bad)


def test_other_edges_in_the_input_scene_are_refused():
    d, inp = scene_data(sweep_scene())
    other, _ = scene_data(sweep_scene(seed=6))
    assert other.x.indices.shape != d.x.indices.shape
    with pytest.raises(ValueError, match="other edges"):
        shard_scene_on_device(d, 0, 2, other)


def test_integer_bounds_equal_partition_points():
    """gasfm_scene_shard_bounds' rule in torch ops against distributed.partition_points' float
    searchsorted, on random degree sequences with many exact ties."""
    from gasfm_amd.distributed import partition_points
    from gasfm_amd.shard_device import _bounds_torch
    rng = np.random.default_rng(0)
    for trial in range(200):
        n = int(rng.integers(1, 60))
        deg = rng.integers(0, 4 if trial % 2 else 9, size=n)
        pt = np.repeat(np.arange(n), deg)
        ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(deg)]).astype(np.int32))
        for world in (1, 2, 3, 5, 8):
            assert _bounds_torch(ptr, world).tolist() == partition_points(pt, n, world).tolist()


def test_sharded_trainer_takes_the_keyword():
    import inspect
    from gasfm_amd.dist_train import ShardedTrainer
    assert inspect.signature(ShardedTrainer.__init__).parameters["device_shard"].default is False
