"""Voxelization, host side (no GPU): the CPU restatement of the contract (tests/voxelize_ref.py) against every fixture the reference's own CPU
kernels produced (tests/golden/voxelize/, exact equality), the fp32 grid-size rule, the Python surface of ``orv_amd.voxelize`` (refusals, the
two import aliases) and the C ABI of the ``orv_voxel_*`` entry points (argument validation happens before any launch)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import voxelize_cases as cases
import voxelize_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement equals the reference ----
def test_there_are_fixtures():
    assert {"caps_both", "caps_points_only", "boundaries", "all_invalid", "one_voxel"} <= set(cases.HARD) and len(cases.HARD) >= 11
    assert set(cases.VOTE) == {"vote_given_range", "vote_data_range", "vote_crowded"}


@pytest.mark.parametrize("name", cases.HARD)
def test_ref_equals_the_reference_cpu_kernel_exactly(name):
    fx = cases.fixture(name)
    vs, rng, mp, mv = fx["voxel_size"], fx["coors_range"], int(fx["max_points"]), int(fx["max_voxels"])
    dyn = ref.dynamic(fx["points"], vs, rng)
    assert dyn.dtype == np.int32 and np.array_equal(dyn, fx["dynamic_coors"])
    voxels, coors, num = ref.hard(fx["points"], vs, rng, mp, mv)
    assert voxels.shape == fx["voxels"].shape and voxels.dtype == np.float32
    assert np.array_equal(coors, fx["coors"]) and coors.dtype == np.int32                  # coordinates and voxel order
    assert np.array_equal(num, fx["num_points_per_voxel"]) and num.dtype == np.int32       # counts
    assert voxels.tobytes() == fx["voxels"].tobytes()                                      # slot order and zero padding, bit for bit


def test_fixtures_cover_what_they_claim():
    both, lifted = cases.fixture("caps_both"), cases.fixture("caps_points_only")
    assert len(both["coors"]) == 300 and (both["num_points_per_voxel"] == 5).sum() > 0
    assert 900 < (both["dynamic_coors"][:, 0] < 0).sum() < 1020
    assert len(lifted["coors"]) > 300 and np.array_equal(lifted["coors"][:300], both["coors"])
    b = cases.fixture("boundaries")
    d = b["dynamic_coors"]
    assert d[0].tolist() == [0, 0, 0] and d[1].tolist() == [-1, -1, -1] and d[2].tolist() == [7, 7, 7]      # at lo, at hi, one ulp below hi
    assert d[3].tolist() == [-1, -1, -1] and d[4].tolist() == [0, 0, 0]                                    # one ulp below / above lo
    bad = ~np.isfinite(b["points"][:, :3]).all(axis=1)
    assert bad.sum() == 10 and (d[bad] == -1).all()
    for a in range(3):                                                                                     # every cell of every axis is hit
        assert set(d[d[:, 0] >= 0][:, 2 - a].tolist()) == set(range(8))
    assert len(cases.fixture("all_invalid")["coors"]) == 0
    one = cases.fixture("one_voxel")
    assert len(one["coors"]) == 1 and one["num_points_per_voxel"].tolist() == [35] and len(one["points"]) == 150
    assert (cases.fixture("vote_crowded")["num_points_per_voxel"] == 100).any()


@pytest.mark.parametrize("name", cases.VOTE)
def test_ref_vote_equals_the_reference_off_the_ties_and_takes_the_smallest_label_on_them(name):
    fx = cases.fixture(name)
    ties = cases.tie_voxels(fx)
    print(f"{name}: {len(ties)} voxels, tie share {ties.mean():.3f}")
    assert ties.mean() <= 0.20
    out = ref.points_to_voxels(fx["points"], fx["voxel_size"], fx["labels"], cases.vote_range(fx))
    assert out.dtype == np.float64 and out.shape == fx["out"].shape and str(fx["out_dtype"]) == "float64" and fx["out"].dtype == np.float64
    assert np.array_equal(out[:, :3], fx["out"][:, :3])
    assert np.array_equal(out[~ties, 3], fx["out"][~ties, 3]) and (~ties).sum() > 0
    counts = fx["label_counts"].astype(np.int64)[:, 1:]
    smallest = np.array([np.flatnonzero(row == row.max())[0] for row in counts], dtype=np.float64)
    assert np.array_equal(out[:, 3], smallest)
    if name != "vote_crowded":
        assert ties.any() and out[:, 3].max() == 254


def test_vote_tie_goes_to_the_smallest_label_by_hand():
    voxels = np.zeros((3, 6, 4), np.float32)
    voxels[0, :4, 3] = [5, 3, 5, 3]             # stored 5 and 3 twice each -> label 2
    voxels[1, :3, 3] = [9, 9, 1]                # stored 9 twice -> label 8
    voxels[2, :1, 3] = [1]                      # padding zeros outnumber the one stored label: zero never wins -> label 0
    assert ref.vote(voxels).tolist() == [2, 8, 0]


def test_grid_size_rule_is_fp32_and_gives_400_for_the_real_geometry():
    from orv_amd import ops
    assert ref.grid_size(cases.REAL_VOXEL, cases.REAL_RANGE) == (400, 400, 400)
    assert ops.voxel_grid_size(ref.f32(cases.REAL_VOXEL), ref.f32(cases.REAL_RANGE)) == (400, 400, 400)
    for vs, rng in (([0.005] * 3, [0, 0, 0, 0.04, 0.04, 0.04]), ([0.05, 0.1, 0.3], [-0.2, -0.2, 0.0, 0.2, 0.2, 0.4]), ([0.001] * 3, [0, 0, 0, 2, 2, 2]),
                    ([0.2] * 3, [-1.05, 0.0, 0.3, 1.0, 0.5, 0.61])):
        assert ops.voxel_grid_size(ref.f32(vs), ref.f32(rng)) == ref.grid_size(vs, rng), (vs, rng)
    assert ref.grid_size([0.005] * 3, [0, 0, 0, 0.04, 0.04, 0.04]) == (8, 8, 8) and ref.grid_size([0.2] * 3, [0, 0, 0, 0.5, 0.3, 0.29]) == (3, 2, 1)


def test_seeded_clouds_do_what_the_gpu_tests_need():
    v, c, n, d = cases.cloud_ref("n70001_grid40")
    assert len(c) == 20000 and (n == 3).any() and (d[:, 0] < 0).any()              # both caps bite
    v, c, n, d = cases.cloud_ref("huge_grid")
    key = (c[:, 0].astype(np.int64) * 2000 + c[:, 1]) * 2000 + c[:, 2]
    assert (key >= 2 ** 32).any() and len(c) == 500 and (n == 4).any()             # keys past 32 bits


# ---- Python surface ----
SUPPORTED = "supported: a contiguous CUDA float32 tensor points [N,C]"


def test_refusals_name_the_supported_set():
    from orv_amd import voxelize as vz
    vs, rng = [0.1] * 3, [0, 0, 0, 1, 1, 1]
    pts = torch.zeros(4, 4)
    with pytest.raises(NotImplementedError, match="not a CUDA tensor") as e:
        vz.voxelization(pts, vs, rng)
    assert SUPPORTED in str(e.value) and "there is no CPU path" in str(e.value)
    with pytest.raises(NotImplementedError, match="torch.float16, not float32") as e:
        vz.voxelization(torch.zeros(4, 4, dtype=torch.float16), vs, rng)
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="C < 3") as e:
        vz.voxelization(torch.zeros(4, 2), vs, rng)
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="no backward") as e:
        vz.voxelization(torch.zeros(4, 4, requires_grad=True), vs, rng)
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="not contiguous") as e:
        vz.voxelization(torch.zeros(4, 8)[:, ::2], vs, rng)
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="deterministic=False") as e:
        vz.voxelization(torch.zeros(4, 4), vs, rng, 35, 20000, False)
    assert SUPPORTED in str(e.value) and "not reproducible by definition" in str(e.value)
    with pytest.raises(NotImplementedError, match="is a list, not a tensor"):
        vz.voxelization([[0.0, 0.0, 0.0]], vs, rng)
    # points_to_voxels: the same set, before anything is launched
    with pytest.raises(NotImplementedError, match="not a CUDA tensor") as e:
        vz.points_to_voxels(pts)
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="not a CUDA tensor"):
        vz.points_to_voxels(np.zeros((4, 3), np.float32), device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="torch.float64, not float32"):
        vz.points_to_voxels(torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="C < 3"):
        vz.points_to_voxels(torch.zeros(4, 2))
    with pytest.raises(NotImplementedError, match="determinstic=False"):
        vz.points_to_voxels(torch.zeros(4, 3), determinstic=False)
    with pytest.raises(NotImplementedError, match="no backward"):
        vz.points_to_voxels(torch.zeros(4, 3, requires_grad=True))
    assert vz.MAX_LABEL == 255


def test_label_check_wants_integers_below_255():
    from orv_amd import voxelize as vz
    vz._check_labels(torch.tensor([0.0, 3.0, 254.0]))
    for bad in ([0.0, 255.0], [-1.0, 2.0], [1.5], [float("nan")]):
        with pytest.raises(NotImplementedError, match=r"not integers in \[0, 255\)") as e:
            vz._check_labels(torch.tensor(bad))
        assert SUPPORTED in str(e.value)


def test_signatures_are_the_references():
    from orv_amd import voxelize as vz
    sig = inspect.signature(vz.voxelization)
    assert list(sig.parameters) == ["points", "voxel_size", "coors_range", "max_points", "max_voxels", "deterministic"]
    assert [p.default for p in sig.parameters.values()][3:] == [35, 20000, True]
    sig = inspect.signature(vz.points_to_voxels)
    assert list(sig.parameters) == ["points", "voxel_size", "labels", "max_num_points", "point_cloud_range", "device", "determinstic"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["voxel_size"] == [0.2, 0.2, 0.2] and d["labels"] is None and d["max_num_points"] == -1 and d["point_cloud_range"] is None
    assert d["device"] == torch.device("cuda") and d["determinstic"] is True
    # lists of floats, of 0-d tensors, arrays: all become the same fp32 values
    want = ref.f32([0.001, 0.2, 0.3])
    for given in ([0.001, 0.2, 0.3], [torch.tensor(0.001), torch.tensor(0.2), torch.tensor(0.3)], np.array([0.001, 0.2, 0.3]), torch.tensor([0.001, 0.2, 0.3])):
        got = vz._floats(given, 3, "voxel_size")
        assert got.dtype == np.float32 and np.array_equal(got, want)
    with pytest.raises(ValueError, match="must have 6 values"):
        vz._floats([0.0] * 5, 6, "coors_range")


ALIASES = ("ivideogpt.ops.voxelize.voxelization", "orv.ops.voxelize.voxelization")


def test_install_makes_both_import_spellings_resolve_and_uninstall_removes_them():
    from orv_amd import voxelize as vz
    before = set(sys.modules)
    assert not any(k == "ivideogpt" or k.startswith("ivideogpt.") or k == "orv" or k.startswith("orv.") for k in before)
    names = vz.install()
    try:
        assert tuple(names) == ALIASES
        from ivideogpt.ops.voxelize.voxelization import voxelization as a          # the line of prepare_dataset.py:145
        from orv.ops.voxelize.voxelization import voxelization as b
        import orv.ops.voxelize.voxelization as mod
        assert a is vz.voxelization and b is vz.voxelization and mod is vz
        assert vz.install() == []                                                  # the names are taken now: nothing more to register
    finally:
        vz.uninstall()
    assert set(sys.modules) - before <= {k for k in sys.modules if k.startswith("orv_amd")}
    with pytest.raises(ImportError):
        from ivideogpt.ops.voxelize.voxelization import voxelization  # noqa: F401
    taken = type(sys)("orv")                                                       # a parent that exists already is left alone
    taken.__path__ = []
    sys.modules["orv"] = taken
    try:
        assert tuple(vz.install()) == ALIASES and sys.modules["orv"] is taken
        from orv.ops.voxelize.voxelization import points_to_voxels
        assert points_to_voxels is vz.points_to_voxels
        vz.uninstall()
        assert sys.modules.get("orv") is taken and "orv.ops" not in sys.modules and "ivideogpt" not in sys.modules
    finally:
        vz.uninstall()
        del sys.modules["orv"]
    import orv_amd
    assert "voxelize" not in inspect.getsource(orv_amd.install)                    # the package-level install() is unchanged


# ---- C ABI ----
NAMES = ("orv_voxel_grid_size", "orv_voxel_coors", "orv_voxel_segments", "orv_voxel_scatter", "orv_voxel_vote")


def test_voxel_symbols_are_declared_exported_and_bound():
    from orv_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        hdr = f.read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(_lib.lib(), name) is not None
        doc = hdr[hdr.index("Point-cloud voxelization"):hdr.index("int " + name + "(")]
        assert "prepare_dataset.py:137-198" in doc and "orv/ops/voxelize" in doc
        assert callable(getattr(ops, name[4:]))
    for name, cites in (("orv_voxel_grid_size", "voxelization_cpu.cpp:118-121"), ("orv_voxel_coors", "voxelization_kernel.cuh:9-46"),
                        ("orv_voxel_segments", "voxelization_kernel.cuh:91-132"), ("orv_voxel_scatter", "voxelization_kernel.cuh:134-163"),
                        ("orv_voxel_vote", "prepare_dataset.py:179-196")):
        end = hdr.index("int " + name + "(")
        assert cites in hdr[hdr.rindex("/*", 0, end):end], name                    # each cites the reference lines it replaces
    with open(os.path.join(ROOT, "orv_amd", "csrc", "Makefile"), "r", encoding="utf-8") as f:
        assert "voxelize.hip" in f.read()


def test_voxel_entry_points_validate_before_any_launch():
    """Null pointers, N < 0, C < 3, a non-positive voxel size or grid: nonzero with the reason in orv_last_error(), prefixed by the entry
    point's name, without a GPU (no pointer is followed)."""
    from orv_amd._lib import lib
    h = lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    err = lambda: h.orv_last_error().decode()

    def grid(vs=(0.1, 0.1, 0.1), rng=(0, 0, 0, 1, 1, 1), out=p):
        return h.orv_voxel_grid_size(*vs, *rng, out)

    def coors(points=p, N=4, C=4, vs=(0.1, 0.1, 0.1), rng=(0, 0, 0, 1, 1, 1), out=p, keys=p):
        return h.orv_voxel_coors(points, N, C, *vs, *rng, out, keys, None)

    def seg(keys=p, order=p, N=4, start=p, seglen=p, first=p):
        return h.orv_voxel_segments(keys, order, N, start, seglen, first, None)

    def sca(points=p, order=p, csum=p, N=4, C=4, mp=5, M=2, voxels=p, num=p):
        return h.orv_voxel_scatter(points, p, order, p, p, csum, N, C, mp, M, voxels, p, num, None)

    def vote(points=p, order=p, csum=p, N=4, C=4, mp=5, M=2, head_of=p, out=p):
        return h.orv_voxel_vote(points, p, order, p, p, csum, N, C, mp, M, head_of, out, None)

    for call, name in ((coors, NAMES[1]), (seg, NAMES[2]), (sca, NAMES[3]), (vote, NAMES[4])):
        assert call(N=-1) != 0 and "N must not be negative" in err() and err().startswith(name + ":"), name
    for call, name in ((coors, NAMES[1]), (sca, NAMES[3])):
        assert call(C=2) != 0 and "C = 2" in err() and "C >= 3" in err() and err().startswith(name + ":")
    assert vote(C=3) != 0 and "C = 3" in err() and "C >= 4" in err() and err().startswith(NAMES[4] + ":")
    for call, name in ((grid, NAMES[0]), (coors, NAMES[1])):
        for bad in ((0.0, 0.1, 0.1), (0.1, -0.1, 0.1), (0.1, 0.1, float("nan"))):
            assert call(vs=bad) != 0 and "voxel size must be positive" in err() and err().startswith(name + ":"), (name, bad)
        for bad in ((0, 0, 0, 1, 1, 0), (0, 0, 0, -1, 1, 1), (0, 0, 0, 1, 0.04, 1), (0, 0, 0, 1, 1e9, 1), (0, float("nan"), 0, 1, 1, 1)):
            assert call(rng=bad) != 0 and "cells on every axis" in err() and err().startswith(name + ":"), (name, bad)
    assert coors(vs=(1e-6, 1e-6, 1e-6), rng=(0, 0, 0, 2000, 2000, 2000)) != 0 and "63-bit key" in err()
    assert grid(out=None) != 0 and "null pointer" in err()
    for bad in (dict(points=None), dict(out=None)):
        assert coors(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[1] + ":"), bad
    for bad in (dict(keys=None), dict(order=None), dict(start=None), dict(seglen=None), dict(first=None)):
        assert seg(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[2] + ":"), bad
    for bad in (dict(points=None), dict(order=None), dict(csum=None), dict(voxels=None), dict(num=None)):
        assert sca(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[3] + ":"), bad
    for bad in (dict(points=None), dict(order=None), dict(csum=None), dict(head_of=None), dict(out=None)):
        assert vote(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[4] + ":"), bad
    for call in (sca, vote):
        assert call(mp=0) != 0 and "max_points must be positive" in err()
        assert call(M=-1) != 0 and "M = -1" in err()
        assert call(M=5) != 0 and "M = 5" in err()
    # nothing to do is not an error, and launches nothing
    assert coors(N=0, points=None, out=None, keys=None) == 0 and seg(N=0, keys=None) == 0
    assert sca(N=0, M=0, points=None) == 0 and sca(M=0, voxels=None) == 0 and vote(N=0, M=0, points=None) == 0 and vote(M=0, out=None) == 0
    g = (ctypes.c_int * 3)()
    assert h.orv_voxel_grid_size(*ref.f32(cases.REAL_VOXEL).tolist(), *ref.f32(cases.REAL_RANGE).tolist(), ctypes.addressof(g)) == 0
    assert tuple(g) == (400, 400, 400)
