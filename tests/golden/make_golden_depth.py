"""Generate tests/golden/depth_targets.npz from the REFERENCE's own depth targets (build container only).

    python tests/golden/make_golden_depth.py

Imports datasets/SceneData.py in place (tests/golden/refimport.py) and builds, with
``store_depth_targets=True``, one small calibrated scene with exact ground-truth cameras: m = 6
cameras on a circle looking at n = 60 points in [-1, 1]^3 (gasfm_amd.synthetic.rotation_look_at),
pixels = the fp64 projections rounded to float32, ragged visibility:

  points 0 .. 49   2 to 5 of the cameras 0 .. 4, drawn at random
  points 50 .. 53  cameras 1 and 4 only (dropped by any sample without both)
  point  54        cameras 0 and 5 only: camera 5 sees this one point (a camera row of length 1;
                   an empty row once camera 0 is not sampled)
  points 55 .. 57  cameras 0 and 1; 1 and 2; 3 and 4
  point  58        camera 2 only, point 59 no camera (both filtered: no edge, NaN in X)

Recorded: the inputs; the reference's triangulated X and dense ``depths``; ``sample_data(data, 4)``
after ``np.random.seed(NP_SEED)`` (views 2 .. 5: camera 5's row is empty); and
``apply_rotational_homography_aug(sampled, 15, 20)`` after ``torch.manual_seed(7)`` with its R_aug,
new M and new depths.  pytorch3d is absent offline: ``axis_angle_to_matrix`` is the restatement of
gasfm_amd.scene_device, as in make_golden_aug.py; R_aug is drawn again from the same seed by
``scene_device.rotational_homography`` and checked against the reference's new cameras.
The reference's own asserts (finite X, unit rotation rows, depths > 0 at the visible entries) run
inside its SceneData constructor.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import refimport  # noqa: E402
from gasfm_amd import synthetic  # noqa: E402  (input generation only)
from gasfm_amd.scene_device import _axis_angle_to_matrix, rotational_homography  # noqa: E402

M_CAMS, N_PTS, NUM_VIEWS, NP_SEED, TORCH_SEED, INPLANE, TILT = 6, 60, 4, 3, 7, 15.0, 20.0


def make_scene():
    rng = np.random.default_rng(11)
    ang = np.linspace(0, 2 * np.pi, M_CAMS, endpoint=False)
    ts = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), 0.3 * rng.standard_normal(M_CAMS)], 1)
    Rs = np.stack([synthetic.rotation_look_at(c) for c in ts])
    K = synthetic.K_DEFAULT
    X = rng.uniform(-1, 1, size=(N_PTS, 3))
    vis = np.zeros((M_CAMS, N_PTS), dtype=bool)
    for j in range(50):
        vis[rng.choice(5, size=int(rng.integers(2, 6)), replace=False), j] = True
    vis[[1, 4], 50:54] = True
    vis[[0, 5], 54] = True
    vis[[0, 1], 55] = vis[[1, 2], 56] = vis[[3, 4], 57] = True
    vis[2, 58] = True
    Ps = np.stack([K @ Rs[c].T @ np.concatenate([np.eye(3), -ts[c][:, None]], 1) for c in range(M_CAMS)])
    q = np.einsum("cij,nj->cni", Ps, np.concatenate([X, np.ones((N_PTS, 1))], 1))
    xy = q[:, :, :2] / q[:, :, 2:3]
    M = (xy * vis[:, :, None]).transpose(0, 2, 1).reshape(2 * M_CAMS, N_PTS).astype(np.float32)
    Ns = np.repeat(np.linalg.inv(K)[None], M_CAMS, 0).astype(np.float32)
    return torch.from_numpy(M), torch.from_numpy(Ns), torch.from_numpy(Ps.astype(np.float32)), vis


def main():
    ref = refimport.load()
    ref.SceneData.axis_angle_to_matrix = _axis_angle_to_matrix
    geo = sys.modules["utils.geo_utils"]
    M, Ns, Ps, vis = make_scene()
    data = ref.SceneData.SceneData(M, Ns, Ps, "synthetic_depth", calibrated=True, store_depth_targets=True)
    assert data.x.indices.shape[1] == int(vis[:, :58].sum())
    X = torch.tensor(geo.n_view_triangulation(Ps.numpy(), M.numpy(), Ns=Ns.numpy()), dtype=torch.float32)
    assert torch.equal((Ns @ Ps @ X)[:, 2, :].nan_to_num(-1), data.depths.nan_to_num(-1))
    np.random.seed(NP_SEED)
    s = ref.SceneData.sample_data(data, NUM_VIEWS)
    start = [i for i in range(M_CAMS - NUM_VIEWS + 1) if torch.equal(s.y, Ps[i:i + NUM_VIEWS])]
    assert start == [2], start  # views 2 .. 5: point 54 is left with camera 5 alone and is dropped
    assert int(s.x.pts_per_cam[3]) == 0
    torch.manual_seed(TORCH_SEED)
    a = ref.SceneData.apply_rotational_homography_aug(s, INPLANE, TILT)
    torch.manual_seed(TORCH_SEED)
    R = rotational_homography(NUM_VIEWS, INPLANE, TILT)
    assert torch.equal(a.y, torch.linalg.inv(s.Ns) @ R @ s.Ns @ s.y)
    assert torch.equal(a.x.indices, s.x.indices)
    out = {"M": M, "Ns": Ns, "Ps_gt": Ps, "X": X, "depths": data.depths, "indices": data.x.indices,
           "params": np.array([NUM_VIEWS, NP_SEED, TORCH_SEED, INPLANE, TILT], dtype=np.float64),
           "s_views": np.arange(start[0], start[0] + NUM_VIEWS), "R_aug": R}
    for tag, d in (("s", s), ("a", a)):
        out[f"{tag}_M"], out[f"{tag}_y"], out[f"{tag}_depths"] = d.M, d.y, d.depths
        out[f"{tag}_indices"] = d.x.indices
        e = d.depths[d.x.indices[0], d.x.indices[1]]
        print(tag, "M", tuple(d.M.shape), "edges", d.x.indices.shape[1], "depths", float(e.min()), float(e.max()))
    path = os.path.join(HERE, "depth_targets.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
