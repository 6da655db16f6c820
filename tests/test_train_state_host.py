"""CPU: the checksum contract of orv_amd.train_state in its numpy restatement (tests/train_state_ref.py) against hand-computed pairs, the
host-only checkpoint layer (write / read / rotate / latest), the per-rank generator states over gloo, the C ABI surface of the snapshot
entry points and their refusals, and the refusals ``save_state`` makes before it touches the device."""
import ctypes
import os
import random
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import train_state_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


# ---- the contract ----
def test_restatement_against_hand_computed_pairs():
    assert R.checksum_bytes(bytes([1, 0, 0, 0, 2, 0, 0, 0, 3])) == (6, 14)                # words 1, 2, 3: 1 + 2 + 3, 1 + 4 + 9
    assert R.checksum_bytes(b"") == (0, 0)
    assert R.checksum_bytes(b"\x01") == (1, 1) and R.checksum_bytes(b"\x00\x00\x00\x00\x00\x01") == (256, 512)   # the tail is zero-padded
    # 2^17 words 0xFFFFFFFF: s1 = (2^32 - 1) 2^17 = 2^49 - 2^17; sum (i + 1) = 2^16 (2^17 + 1) = 2^33 + 2^16, so
    # s2 = (2^32 - 1)(2^33 + 2^16) = 2^65 + 2^48 - 2^33 - 2^16, which wraps to 2^48 - 2^33 - 2^16
    big = b"\xff" * (4 << 17)
    assert R.checksum_bytes(big) == ((1 << 49) - (1 << 17), (1 << 48) - (1 << 33) - (1 << 16)) == (0x0001FFFFFFFE0000, 0x0000FFFDFFFF0000)
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 3, 4, 5, 7, 4096, 4099, 70001):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert R.checksum_bytes(b) == R.checksum_exact(b), n
    assert R.checksum(torch.tensor([1, 2, 3], dtype=torch.int32)) == (6, 14)
    assert R.checksum(torch.zeros(0)) == (0, 0)


# ---- write / read ----
def _tensors(seed=0):
    g = torch.Generator().manual_seed(seed)
    opt = {"exp_avg": torch.randn(2048, generator=g), "p16": torch.randn(3, 5, generator=g).to(BF),
           "param_lo": torch.randint(-32768, 32768, (2049,), generator=g, dtype=torch.int64).to(torch.int16),
           "seg_step": torch.arange(7, dtype=torch.int32), "exp_avg8": torch.randint(0, 256, (4097,), generator=g, dtype=torch.int64).to(torch.uint8),
           "came_v": torch.zeros(0), "odd": torch.randn(3, generator=g).to(BF)}
    ema = {"shadow_params.0": torch.randn(5, generator=g), "shadow_params.1": torch.randn(2, 2, generator=g)}
    return {"optimizer": opt, "ema": ema}


def _meta(step=3):
    return {"step": step, "extra": {"epoch": 1, "note": "x"},
            "files": {"optimizer": {"values": {"step": 3, "numels": [1, 2]}, "lists": {}}, "ema": {"values": {"decay": 0.9}, "lists": {"shadow_params": 2}},
                      "scheduler": {"last_epoch": 3}, "random_states": {"ranks": [{"python": [3, [1, 2], None]}]}}}


def _sums(tensors):
    return {g: {k: R.checksum(v) for k, v in named.items()} for g, named in tensors.items()}


def test_write_read_round_trip_of_every_state_dtype(tmp_path):
    from orv_amd import train_state as T
    tensors, d = _tensors(), str(tmp_path / "checkpoint-3")
    T.write_checkpoint(d, tensors, _meta(), _sums(tensors))
    assert sorted(os.listdir(d)) == ["ema.json", "ema.safetensors", "manifest.json", "optimizer.json", "optimizer.safetensors",
                                     "random_states.json", "scheduler.json"]
    back = T.read_checkpoint(d, checksum=R.checksum)
    assert back["step"] == 3 and back["extra"] == {"epoch": 1, "note": "x"} and back["files"] == _meta()["files"]
    seen = set()
    for group, named in tensors.items():
        assert sorted(back["tensors"][group]) == sorted(named)
        for k, v in named.items():
            got = back["tensors"][group][k]
            assert got.dtype == v.dtype and got.shape == v.shape and R.tensor_bytes(got) == R.tensor_bytes(v), (group, k)
            seen.add(v.dtype)
            rec = back["manifest"]["tensors"][group][k]
            assert (int(rec["s1"], 16), int(rec["s2"], 16)) == R.checksum(v) and rec["shape"] == list(v.shape)
    assert seen == {torch.float32, BF, torch.int16, torch.int32, torch.uint8} and back["tensors"]["optimizer"]["came_v"].numel() == 0
    sd = T.join_state(back["tensors"]["ema"], back["files"]["ema"])
    assert sd["decay"] == 0.9 and [tuple(t.shape) for t in sd["shadow_params"]] == [(5,), (2, 2)]
    with pytest.raises(ValueError, match="do not name the same tensors"):
        T.write_checkpoint(str(tmp_path / "bad"), tensors, _meta(), {"optimizer": {}, "ema": {}})
    assert not os.path.exists(tmp_path / "bad" / "manifest.json")


def test_split_and_join_are_inverse_and_know_no_optimizer():
    from orv_amd import train_state as T
    a, b = torch.arange(3), torch.ones(2, 2)
    sd = {"step": 4, "t": a, "none": None, "lst": [a, b], "shapes": [[1, 2], [3]], "empty": [], "mode": "bf16", "f": 0.5}
    tensors, meta = T.split_state(sd)
    assert list(tensors) == ["t", "lst.0", "lst.1"] and meta["lists"] == {"lst": 2}
    assert meta["values"] == {"step": 4, "none": None, "shapes": [[1, 2], [3]], "empty": [], "mode": "bf16", "f": 0.5}
    back = T.join_state(tensors, meta)
    assert set(back) == set(sd) and back["t"] is a and back["lst"][1] is b and back["none"] is None and back["shapes"] == sd["shapes"]


def test_two_writes_give_byte_identical_directories(tmp_path):
    from orv_amd import train_state as T
    for name in ("a", "b"):
        tensors = _tensors()
        T.write_checkpoint(str(tmp_path / name), tensors, _meta(), _sums(tensors))
    a, b = R.tree_bytes(tmp_path / "a"), R.tree_bytes(tmp_path / "b")
    assert sorted(a) == sorted(b) and len(a) == 7 and all(a[k] == b[k] for k in a)
    text = a["manifest.json"].decode()
    assert '"format_version": 1' in text and "time" not in text and text.index('"extra"') < text.index('"files"') < text.index('"step"')


def test_one_flipped_byte_is_reported_with_the_tensors_name(tmp_path):
    from orv_amd import train_state as T
    tensors, d = _tensors(), str(tmp_path / "checkpoint-3")
    T.write_checkpoint(d, tensors, _meta(), _sums(tensors))
    R.flip_byte_of(os.path.join(d, "optimizer.safetensors"), "param_lo", at=1234)
    T.read_checkpoint(d)                                         # names, dtypes and shapes still agree
    with pytest.raises(ValueError, match=r"optimizer\.safetensors: tensor 'param_lo' has checksum"):
        T.read_checkpoint(d, checksum=R.checksum)
    R.flip_byte_of(os.path.join(d, "optimizer.safetensors"), "param_lo", at=1234)
    T.read_checkpoint(d, checksum=R.checksum)
    R.flip_byte_of(os.path.join(d, "ema.safetensors"), "shadow_params.1", at=15)
    with pytest.raises(ValueError, match=r"ema\.safetensors: tensor 'shadow_params\.1' has checksum"):
        T.read_checkpoint(d, checksum=R.checksum)
    os.remove(os.path.join(d, "manifest.json"))
    with pytest.raises(FileNotFoundError, match="not a \\(complete\\) checkpoint"):
        T.read_checkpoint(d)


# ---- rotation and 'latest' ----
@pytest.mark.parametrize("total_limit", [None, 1, 2])
@pytest.mark.parametrize("present", [[], [9], [9, 10], [2, 9, 10]])
def test_rotate_leaves_what_the_reference_rule_leaves(tmp_path, total_limit, present):
    from orv_amd import train_state as T
    before = [f"checkpoint-{n}" for n in present]
    for name in before + ["checkpoint-11", ".tmp-checkpoint-12", "checkpoint", "logs"]:           # 11 is the save that just completed
        os.makedirs(tmp_path / name)
    removed = T.rotate(str(tmp_path), total_limit, keep="checkpoint-11")
    left = sorted((n for n in os.listdir(tmp_path) if n.startswith("checkpoint-")), key=lambda x: int(x.split("-")[1]))
    assert left == R.reference_rotation(before, "checkpoint-11", total_limit)
    assert sorted(removed + left) == sorted(before + ["checkpoint-11"])
    assert all(os.path.isdir(tmp_path / n) for n in (".tmp-checkpoint-12", "checkpoint", "logs"))


def test_latest_checkpoint_is_numeric_and_wants_a_manifest(tmp_path):
    from orv_amd import train_state as T
    out = str(tmp_path)
    assert T.latest_checkpoint(out) is None and T.latest_checkpoint(os.path.join(out, "missing")) is None
    for name, manifest in ((".tmp-checkpoint-19", True), ("checkpoint-17", False), ("checkpoint", True), ("checkpoint-9", True)):
        os.makedirs(tmp_path / name)
        if manifest:
            (tmp_path / name / "manifest.json").write_text("{}")
    assert T.latest_checkpoint(out) == os.path.join(out, "checkpoint-9")
    os.makedirs(tmp_path / "checkpoint-10")
    assert T.latest_checkpoint(out) == os.path.join(out, "checkpoint-9")             # 10 is not complete yet
    (tmp_path / "checkpoint-10" / "manifest.json").write_text("{}")
    assert T.latest_checkpoint(out) == os.path.join(out, "checkpoint-10")            # numeric order: "checkpoint-10" < "checkpoint-9" as strings


# ---- generator states ----
def _draws(gen):
    return [random.random(), float(np.random.rand()), float(torch.rand(1)), float(torch.rand(1, generator=gen))]


def _seed(rank):
    random.seed(10 + rank)
    np.random.seed(20 + rank)
    torch.manual_seed(30 + rank)
    return torch.Generator().manual_seed(40 + rank)


def _rng_worker(rank, world, port, out):
    import torch.distributed as dist
    from orv_amd import train_state as T
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    gen = _seed(rank)
    _draws(gen)                                             # somewhere inside the sequences
    states = T.collect_random_states(gen)
    out.put((rank, states if rank == 0 else len(states), _draws(gen)))
    dist.destroy_process_group()


def test_two_rank_collection_of_generator_states():
    from orv_amd import train_state as T
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_rng_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    got = dict((r, (a, b)) for r, a, b in (q.get(timeout=120) for _ in range(2)))
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    states = got[0][0]
    assert len(states) == 2 and got[1][0] == 2 and states[0] != states[1]
    import json
    states = json.loads(json.dumps(states, sort_keys=True))               # as random_states.json holds them
    saved = T.random_state()
    try:
        for rank in (0, 1):
            gen = torch.Generator()
            T.set_random_state(states[rank], gen)
            assert _draws(gen) == got[rank][1], rank                       # every rank continues ITS sequences
        with pytest.raises(ValueError, match="holds no state for `generator`"):
            T.set_random_state(T.random_state(), torch.Generator())
    finally:
        T.set_random_state(saved)


# ---- C ABI ----
NAMES = ("orv_snapshot", "orv_checksum")


def test_symbols_are_declared_exported_and_bound():
    import orv_amd
    from orv_amd import _lib, ops, train_state
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        hdr = f.read()
    for name in NAMES:
        params = re.search(r"^int " + name + r"\(([^)]*)\)", hdr, re.M).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]) == 7, name
        assert getattr(_lib.lib(), name) is not None
    assert re.search(r"^long orv_snapshot_scratch_bytes\(int n, long total_bytes\);", hdr, re.M)
    assert re.search(r"^int orv_snapshot_chunk_bytes\(void\);", hdr, re.M)
    assert ctypes.sizeof(_lib.SnapshotEntry) == 24
    assert all(callable(getattr(ops, n)) for n in ("snapshot", "snapshot_into", "checksum", "snapshot_chunk_bytes", "sums_to_ints"))
    assert "snapshot.hip" in open(os.path.join(ROOT, "orv_amd", "csrc", "Makefile")).read()
    for name in ("save_state", "load_state", "latest_checkpoint"):
        assert getattr(orv_amd, name) is getattr(train_state, name)
    C = ops.snapshot_chunk_bytes()
    assert C > 0 and C % 16 == 0
    h = _lib.lib()
    assert h.orv_snapshot_scratch_bytes(1, 0) == 16 and h.orv_snapshot_scratch_bytes(3, 5 * C + 1) == 16 * 8
    assert h.orv_snapshot_scratch_bytes(0, 0) == -1 and "n=0" in h.orv_last_error().decode()
    assert h.orv_snapshot_scratch_bytes(1, -1) == -1 and "total_bytes=-1" in h.orv_last_error().decode()


def test_entry_points_validate_before_any_launch():
    """Every refusal happens on the host copy of the table, before any HIP call: no address is dereferenced, so this runs without a GPU."""
    from orv_amd import _lib, ops
    h = _lib.lib()
    C = ops.snapshot_chunk_bytes()
    DEV, SUMS, SCR = 0x7000000, 0x100000, 0x200000
    err = lambda: h.orv_last_error().decode()

    def table(*rows):
        return (_lib.SnapshotEntry * len(rows))(*rows)

    def call(fn, rows, dev=DEV, sums=SUMS, scratch=SCR, scratch_bytes=1 << 20, n=None):
        t = table(*rows)
        return fn(dev, ctypes.addressof(t), len(rows) if n is None else n, sums, scratch, scratch_bytes, None)

    ok = (0x10000, 0x20000, 100)
    for fn, who in ((h.orv_snapshot, "orv_snapshot"), (h.orv_checksum, "orv_checksum")):
        row = ok if fn is h.orv_snapshot else (0x10000, None, 100)
        t = table(row)
        assert fn(None, ctypes.addressof(t), 1, SUMS, SCR, 1 << 20, None) != 0 and who + ": null table" in err()
        assert fn(DEV, None, 1, SUMS, SCR, 1 << 20, None) != 0 and "null table" in err()
        assert call(fn, [row], n=0) != 0 and "n=0 entries" in err()
        assert call(fn, [row], sums=None) != 0 and "sums" in err()
        assert call(fn, [row], sums=SUMS + 8) != 0 and "16-byte aligned" in err()
        assert call(fn, [row, (None, None, 4)]) != 0 and "entry 1 has a null src with bytes=4" in err()
        assert call(fn, [row, (0x30000, None, -1)]) != 0 and "entry 1 has bytes=-1" in err()
        for bad in (0x10001, 0x10002, 0x10003):
            assert call(fn, [(bad, row[1], 8)]) != 0 and "entry 0: src and dst must be 4-byte aligned" in err()
        assert call(fn, [row], scratch=None) != 0 and "scratch" in err()
        assert call(fn, [row], scratch=SCR + 4) != 0 and "scratch" in err()
        assert call(fn, [(row[0], row[1], 2 * C + 1)], scratch_bytes=47) != 0 and "at least 48 bytes" in err()
    assert call(h.orv_snapshot, [(0x10000, 0x20002, 8)]) != 0 and "4-byte aligned" in err()
    assert call(h.orv_snapshot, [(0x10000, 0x10040, 100)]) != 0 and "overlap" in err()
    assert call(h.orv_checksum, [ok]) != 0 and "entry 0 has a dst" in err()
    for f, args in ((ops.snapshot, ([torch.zeros(4)],)), (ops.checksum, ([torch.zeros(4)],)), (ops.snapshot_into, ([torch.zeros(4)], [torch.zeros(4)]))):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            f(*args)
    assert ops.snapshot([]) [0] == [] and ops.checksum([]).shape == (0, 2)


# ---- save_state: what is refused before the device is touched ----
class _Bag(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.w = torch.nn.ParameterList(params)


def test_save_state_refuses_cpu_tensors_and_a_swapped_in_average(tmp_path):
    from orv_amd import FusedEMA, train_state as T
    from orv_amd.optim import FusedAdamW
    params = [torch.nn.Parameter(torch.zeros(n, dtype=BF)) for n in (3, 2049)]
    bag, opt = _Bag(params), FusedAdamW(params)
    with pytest.raises(RuntimeError, match=r"save_state: \d+ CPU tensors.*\(supported: a model and a FusedAdamW / FusedProdigy / FusedCAME"):
        T.save_state(str(tmp_path), 1, model=bag, optimizer=opt)
    ema = FusedEMA(opt)
    ema.store()
    with pytest.raises(RuntimeError, match=r"save_state: the averaged weights are swapped in.*restore\(\)"):
        T.save_state(str(tmp_path), 1, model=bag, optimizer=opt, ema=ema)
    ema.restore()
    opt._handed.add(0)
    with pytest.raises(RuntimeError, match="middle of a gradient window"):
        T.save_state(str(tmp_path), 1, model=bag, optimizer=opt)
    opt._handed.clear()
    failed = T.SaveHandle(str(tmp_path / "checkpoint-0"))
    failed.error = OSError("disk full")
    T._previous[0] = failed
    with pytest.raises(RuntimeError, match=r"the previous save \(.*checkpoint-0\) failed: OSError\('disk full'\)"):
        T.save_state(str(tmp_path), 1, model=bag, optimizer=opt)
    with pytest.raises(RuntimeError, match="failed"):
        failed.wait()
    assert T._previous[0] is None and os.listdir(tmp_path) == []
    with pytest.raises(ValueError, match="resume='newest'"):
        T.load_state(str(tmp_path), model=bag, optimizer=opt, resume="newest")
    with pytest.raises(FileNotFoundError, match="no complete checkpoint-N directory"):
        T.load_state(str(tmp_path), model=bag, optimizer=opt, resume="latest")
