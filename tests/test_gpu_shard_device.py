"""shard_device.shard_scene_on_device on the GPU: the kernels of csrc/scene_shard.hip against the host
path (dist_train.shard_device_scene) and against their torch-op restatement on the same device
scene.  Integers and bit copies only: every comparison is torch.equal (test_shard_device_cpu.same_shard).

The end-to-end test runs one ShardedTrainer step (emulated rank 0 of 8) with the shard built either
way: equal plans and deterministic kernels make loss, our_repro, every gradient and the weights
after gasfm Adam bitwise equal."""
import copy

import numpy as np
import pytest
import torch

from test_shard_device_cpu import WORLDS, block_scene, same_shard, scene_data, sweep_scene

pytestmark = pytest.mark.gpu

SCENES = {
    "sweep": (lambda: sweep_scene(), None),
    "exact_boundary": (lambda: sweep_scene(m=12, n=48, degrees=(3,), seed=11), None),
    "point_sorted": (lambda: block_scene(), None),
    "split_camera": (lambda: sweep_scene(full_camera=3, seed=13), None),
    "two_level_combine": (lambda: sweep_scene(full_camera=3, seed=13), 2),
}


def _check_rank(d, inp, rank, world, cameras, max_piece=None, torch_path=True):
    from gasfm_amd.dist_train import shard_device_scene
    from gasfm_amd.shard_device import shard_scene_on_device
    ref = shard_device_scene(d, rank, world, inp, cameras=cameras, max_piece=max_piece)
    assert ref[0].point_slice.stop > ref[0].point_slice.start
    got = shard_scene_on_device(d, rank, world, inp, cameras=cameras, max_piece=max_piece)
    what = f"world {world} rank {rank} cameras {cameras}"
    assert got[0].x.values.is_cuda and got[0].graph_wrappers["proj2view"].plan.items.is_cuda
    same_shard(got[0], ref[0], what + " net (kernels vs host)")
    same_shard(got[1], ref[1], what + " loss (kernels vs host)", loss=True)
    if torch_path:
        alt = shard_scene_on_device(d, rank, world, inp, cameras=cameras, max_piece=max_piece, kernels=False)
        same_shard(got[0], alt[0], what + " net (kernels vs torch ops)")
        same_shard(got[1], alt[1], what + " loss (kernels vs torch ops)", loss=True)
        assert torch.equal(got[0].edge_ids, alt[0].edge_ids)
    return got


@pytest.mark.parametrize("name", list(SCENES))
def test_small_scenes_all_ranks(device, name):
    make, max_piece = SCENES[name]
    d, inp = scene_data(make(), device)
    for world in WORLDS if max_piece is None else (1, 3):
        for cameras in (False, True):
            for rank in range(world):
                _check_rank(d, inp, rank, world, cameras, max_piece)


def _device_scene(sc, device, name):
    from gasfm_amd.scene_device import scene_from_dense_device
    return scene_from_dense_device(torch.from_numpy(sc.dense_M()).to(device), torch.from_numpy(sc.Ns()).to(device),
                                   torch.from_numpy(sc.Ps_gt()).to(device), name)


def test_every_kernel_on_several_workgroups(device):
    """1,100 cameras x 2,000 points (~40 k edges) at world 8, built on the device (the scene carries the
    scene build's perm / pos): the per-camera kernel runs 5 workgroups of 256 cameras, the scan's 1,024
    threads own two cameras each, and a shard's ~5 k edges are 5 workgroups of the emit and point-CSR
    kernels (1,024 edges per workgroup)."""
    from gasfm_amd import synthetic
    from gasfm_amd.scene import SceneData, SparseMat
    d = _device_scene(synthetic.windowed_scene(1100, 2000, seed=9), device, "wide")
    assert "graph_wrappers" not in d.__dict__ and d.x.indices.shape[1] > 8 * 4 * 1024
    inp = SceneData.__new__(SceneData)
    inp.__dict__.update(d.__dict__)
    x = d.x
    inp.x = SparseMat(x.values * 1.5 + 0.25, x.indices, x.cam_per_pts, x.pts_per_cam, x.shape)
    for rank in range(8):
        net, _ = _check_rank(d, inp, rank, 8, cameras=bool(rank % 2), torch_path=rank < 2)
        assert net.x.indices.shape[1] > 4 * 1024
    assert "graph_wrappers" not in d.__dict__  # the scene's own wrappers were never needed


def _sampled(device, seed=31):
    from gasfm_amd import synthetic
    from gasfm_amd.dist_train import sample_training_scene
    full = _device_scene(synthetic.windowed_scene(40, 3000, mean_extra=6, seed=71), device, "train_c5")
    np.random.seed(seed)
    torch.manual_seed(seed)
    d, inp = sample_training_scene(full, outlier_rate=0.1)
    assert inp is not None
    return d, inp


def test_sampled_scene_with_outliers(device):
    """The network's shard carries the injected values, the loss's the clean ones, on the same edges."""
    d, inp = _sampled(device)
    assert not torch.equal(d.x.values, inp.x.values) and torch.equal(d.x.indices, inp.x.indices)
    differ = 0
    for world in (2, 8):
        for rank in range(world):
            net, loss = _check_rank(d, inp, rank, world, cameras=world == 8)
            sel = net.edge_ids
            assert torch.equal(loss.x.values, d.x.values.index_select(0, sel))
            assert torch.equal(net.x.values, inp.x.values.index_select(0, sel))
            assert net.x.indices is loss.x.indices
            differ += not torch.equal(net.x.values, loss.x.values)
    assert differ >= 8


def test_two_calls_give_equal_shards(device):
    from gasfm_amd.shard_device import shard_scene_on_device
    d, inp = _sampled(device)
    for cameras in (False, True):
        a = shard_scene_on_device(d, 3, 8, inp, cameras=cameras)
        b = shard_scene_on_device(d, 3, 8, inp, cameras=cameras)
        same_shard(a[0], b[0], "net, second call")
        same_shard(a[1], b[1], "loss, second call", loss=True)
        assert torch.equal(a[0].edge_ids, b[0].edge_ids)
        assert a[0].x.indices.data_ptr() != b[0].x.indices.data_ptr()


def test_trainer_step_is_bitwise_the_same_either_way(device):
    """One config-5 step of the emulated rank 0 of 8 from identical weights, the shard built on the
    device or on the host: loss, our_repro, every gradient and every weight after Adam are equal."""
    import gasfm_amd
    from gasfm_amd.dist_train import ShardedTrainer
    from gasfm_amd.loss import ESFMLoss
    from gasfm_amd.optim import Adam
    from test_gpu_train_step import conf_with_loss, net_for
    conf = conf_with_loss(gasfm_amd.learning_conf(num_layers=2))
    base = net_for(conf, device)
    d, inp = _sampled(device)
    out = {}
    for device_shard in (False, True):
        net = copy.deepcopy(base)
        trainer = ShardedTrainer(net, ESFMLoss(conf), optimizer=Adam(net.parameters(), lr=1e-3), emulate_world=8,
                                 device_shard=device_shard)
        loss, err = trainer.step(d, inp)
        torch.cuda.synchronize()
        out[device_shard] = (loss, err, {k: p.grad.clone() for k, p in net.named_parameters()},
                             {k: p.detach().clone() for k, p in net.named_parameters()}, trainer.last)
    (l0, e0, g0, w0, s0), (l1, e1, g1, w1, s1) = out[False], out[True]
    same_shard(s1[0], s0[0], "trainer net shard")
    same_shard(s1[1], s0[1], "trainer loss shard", loss=True)
    assert torch.isfinite(l0) and torch.equal(l0, l1), (float(l0), float(l1))
    assert torch.isfinite(e0) and torch.equal(e0, e1), (float(e0), float(e1))
    assert any(float(g.abs().max()) > 0 for g in g0.values())
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"grad {k}"
    for k in w0:
        assert torch.equal(w0[k], w1[k]), f"weight after Adam {k}"
    assert any(not torch.equal(w0[k], p.detach()) for k, p in base.named_parameters())  # Adam moved them
