"""GPU: point-cloud voxelization (``orv_amd.voxelize`` over csrc/voxelize.hip) against the CPU restatement of tests/voxelize_ref.py and the
fixtures the reference's own CPU kernels produced (tests/golden/voxelize/).  The outputs are integers and copied floats, so every comparison
is exact equality: coordinates, voxel order, slot order, counts and zero padding.  The vote follows the reference on every voxel whose most
frequent label is unique there and takes the smallest label on a tie."""
import numpy as np
import pytest
import torch

import voxelize_cases as cases
import voxelize_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hard(points, vs, rng, max_points, max_voxels):
    from orv_amd.voxelize import voxelization
    pts = torch.from_numpy(np.ascontiguousarray(points)).to(DEV)
    keep = pts.clone()
    voxels, coors, num = voxelization(pts, vs, rng, max_points, max_voxels)
    dyn = voxelization(pts, vs, rng, -1, -1)
    torch.cuda.synchronize()
    assert torch.equal(pts.view(torch.int32), keep.view(torch.int32))              # the input is left unchanged (bitwise: NaN rows too)
    assert voxels.dtype == torch.float32 and coors.dtype == torch.int32 and num.dtype == torch.int32 and dyn.dtype == torch.int32
    return voxels.cpu().numpy(), coors.cpu().numpy(), num.cpu().numpy(), dyn.cpu().numpy()


def _same(got, want):
    voxels, coors, num, dyn = got
    w_voxels, w_coors, w_num, w_dyn = want
    assert dyn.shape == w_dyn.shape and np.array_equal(dyn, w_dyn)
    assert coors.shape == w_coors.shape and np.array_equal(coors, w_coors)
    assert np.array_equal(num, w_num)
    assert voxels.shape == w_voxels.shape and voxels.tobytes() == w_voxels.tobytes()


@pytest.mark.parametrize("name", cases.HARD)
def test_fixture_cases_equal_the_reference_and_the_restatement(name):
    """small N (1 .. 1025) at C = 3, 4, 7; both caps biting and the voxel cap lifted; the boundaries; every point invalid; one voxel."""
    fx = cases.fixture(name)
    vs, rng, mp, mv = fx["voxel_size"].tolist(), fx["coors_range"].tolist(), int(fx["max_points"]), int(fx["max_voxels"])
    got = _hard(fx["points"], vs, rng, mp, mv)
    _same(got, (fx["voxels"], fx["coors"], fx["num_points_per_voxel"], fx["dynamic_coors"]))
    _same(got, ref.hard(fx["points"], vs, rng, mp, mv) + (ref.dynamic(fx["points"], vs, rng),))


@pytest.mark.parametrize("C", [3, 4, 7])
def test_no_points_at_all(C):
    voxels, coors, num, dyn = _hard(np.zeros((0, C), np.float32), [0.05] * 3, [0, 0, 0, 0.6, 0.6, 0.6], 3, 500)
    assert voxels.shape == (0, 3, C) and coors.shape == (0, 3) and num.shape == (0,) and dyn.shape == (0, 3)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1025])
@pytest.mark.parametrize("C", [3, 4, 7])
def test_small_n_at_every_feature_width(N, C):
    pts = np.random.default_rng(1000 * C + N).uniform(-0.05, 0.65, size=(N, C)).astype(np.float32)
    vs, rng = [0.05] * 3, [0.0, 0.0, 0.0, 0.6, 0.6, 0.6]
    for mp, mv in ((3, 500), (2, 40)):
        _same(_hard(pts, vs, rng, mp, mv), ref.hard(pts, vs, rng, mp, mv) + (ref.dynamic(pts, vs, rng),))


@pytest.mark.parametrize("name", ["n70001_grid40", "real_geometry", "huge_grid"])
def test_seeded_clouds_equal_the_restatement(name):
    """70 001 points on a 40^3 grid (wave, workgroup and multi-block boundaries, both caps); the reference's 400^3 grid with 50 000 surface
    points, max_points 100, max_voxels 1e5; 2000^3 cells (keys past 32 bits)."""
    pts, vs, rng, mp, mv = cases.cloud(name)
    _same(_hard(pts, vs, rng, mp, mv), cases.cloud_ref(name))


def test_range_and_voxel_size_as_zero_d_tensors():
    from orv_amd.voxelize import voxelization
    fx = cases.fixture("caps_both")
    pts = torch.from_numpy(fx["points"]).to(DEV)
    vs = [torch.tensor(float(v), device=DEV) for v in fx["voxel_size"]]
    rng = [torch.tensor(float(v), device=DEV) for v in fx["coors_range"]]
    voxels, coors, num = voxelization(pts, vs, rng, 5, 300, True)
    assert np.array_equal(coors.cpu().numpy(), fx["coors"]) and voxels.cpu().numpy().tobytes() == fx["voxels"].tobytes()


# ---- the vote ----
def _vote(fx, **kw):
    from orv_amd.voxelize import points_to_voxels
    return points_to_voxels(fx["points"], fx["voxel_size"].tolist(), fx["labels"], point_cloud_range=cases.vote_range(fx), device=torch.device(DEV), **kw)


@pytest.mark.parametrize("name", cases.VOTE)
def test_points_to_voxels_against_the_reference(name):
    fx = cases.fixture(name)
    out = _vote(fx)                                                              # numpy inputs; the range from the data in vote_data_range
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == fx["out"].shape and out.shape[1] == 4
    ties = cases.tie_voxels(fx)
    assert np.array_equal(out[:, :3], fx["out"][:, :3])
    assert np.array_equal(out[~ties, 3], fx["out"][~ties, 3])
    counts = fx["label_counts"].astype(np.int64)[:, 1:]
    assert np.array_equal(out[:, 3], np.array([np.flatnonzero(row == row.max())[0] for row in counts], dtype=np.float64))
    assert np.array_equal(out, ref.points_to_voxels(fx["points"], fx["voxel_size"], fx["labels"], cases.vote_range(fx)))


def test_points_to_voxels_with_tensors_without_labels_and_with_lists_of_tensors():
    from orv_amd.voxelize import points_to_voxels
    fx = cases.fixture("vote_data_range")
    pts, lab = torch.from_numpy(fx["points"]).to(DEV), torch.from_numpy(fx["labels"]).to(DEV)
    keep = pts.clone()
    vs = fx["voxel_size"].tolist()
    out = points_to_voxels(pts, vs, lab)                                         # tensor inputs, integer label tensor
    assert np.array_equal(out, ref.points_to_voxels(fx["points"], vs, fx["labels"]))
    wide = torch.cat([pts, torch.rand(len(pts), 3, device=DEV)], 1)[:, :6]       # [N,6] xyz + rgb: only x y z are used
    assert np.array_equal(points_to_voxels(wide, vs, lab), out)
    none = points_to_voxels(pts, vs)                                             # labels=None: every voxel gets label 0
    assert none.dtype == np.float64 and np.array_equal(none[:, :3], out[:, :3]) and not none[:, 3].any()
    ok = pts[~torch.isnan(pts).any(1)]
    rng = [ok[:, 0].min(), ok[:, 1].min(), ok[:, 2].min(), ok[:, 0].max(), ok[:, 1].max(), ok[:, 2].max()]      # as the reference builds it
    assert np.array_equal(points_to_voxels(pts, vs, lab, point_cloud_range=rng), out)
    assert torch.equal(pts.view(torch.int32), keep.view(torch.int32))
    with pytest.raises(NotImplementedError, match=r"not integers in \[0, 255\)"):
        points_to_voxels(pts, vs, lab.float() + 0.5)
    with pytest.raises(NotImplementedError, match=r"not integers in \[0, 255\)"):
        points_to_voxels(pts, vs, torch.full_like(lab, 255))


def test_fused_vote_equals_the_vote_over_the_hard_voxels():
    """The fused path against the unfused one on the GPU: hard voxelization (max_points 100) and the restatement's vote over its buffer."""
    from orv_amd.voxelize import points_to_voxels, voxelization
    pts, vs, rng, _, _ = cases.cloud("real_geometry")
    lab = (np.random.default_rng(5).integers(0, 12, len(pts)) * (pts[:, 0] > 0)).astype(np.int64)
    out = points_to_voxels(pts[:, :3], vs, lab, point_cloud_range=rng, device=torch.device(DEV))
    four = torch.from_numpy(np.concatenate([pts[:, :3], lab[:, None].astype(np.float32) + 1], 1)).to(DEV)
    voxels, coors, num = voxelization(four, vs, rng, 100, 100000)
    assert np.array_equal(out[:, :3], coors.cpu().numpy()[:, ::-1]) and np.array_equal(out[:, 3], ref.vote(voxels.cpu().numpy()))


def test_two_runs_are_bit_identical():
    from orv_amd.voxelize import points_to_voxels, voxelization
    pts, vs, rng, mp, mv = cases.cloud("n70001_grid40")
    t = torch.from_numpy(pts).to(DEV)
    a, b = voxelization(t, vs, rng, mp, mv), voxelization(t, vs, rng, mp, mv)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    fx = cases.fixture("vote_given_range")
    assert _vote(fx).tobytes() == _vote(fx).tobytes()


def test_gpu_refusals_need_no_launch():
    from orv_amd.voxelize import voxelization
    pts = torch.zeros(8, 4, device=DEV)
    vs, rng = [0.1] * 3, [0, 0, 0, 1, 1, 1]
    with pytest.raises(NotImplementedError, match="not contiguous"):
        voxelization(torch.zeros(8, 8, device=DEV)[:, ::2], vs, rng)
    with pytest.raises(NotImplementedError, match="deterministic=False"):
        voxelization(pts, vs, rng, 35, 20000, False)
    with pytest.raises(NotImplementedError, match="float32"):
        voxelization(pts.half(), vs, rng)
    with pytest.raises(NotImplementedError, match="no backward"):
        voxelization(pts.clone().requires_grad_(), vs, rng)
    with pytest.raises(RuntimeError, match="orv_voxel_coors: the voxel size must be positive"):
        voxelization(pts, [0.1, 0.0, 0.1], rng)
    with pytest.raises(RuntimeError, match="orv_voxel_coors: the grid"):
        voxelization(pts, vs, [0, 0, 0, 1, 1, 0])
