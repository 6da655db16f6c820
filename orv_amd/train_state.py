"""Resumable training-state checkpoints with a device-side snapshot.

The reference saves a run every ``checkpointing_steps`` with ``accelerator.save_state(output_dir/checkpoint-{step})``, rotates to
``checkpoints_total_limit`` and resumes ``'latest'`` (train_cogvideox_control_to_video_sft.py:396-409, :1114-1143, :789-812).  Here

    handle = save_state(output_dir, step, model=m, optimizer=opt, lr_scheduler=sch, ema=ema, generator=gen, total_limit=3)
    ...                                     # training goes on; handle.wait() before the process ends
    info = load_state(output_dir, resume="latest", model=m, optimizer=opt, lr_scheduler=sch, ema=ema, generator=gen)   # info["step"]

``save_state`` holds the training stream for ONE pass over the state: ``ops.snapshot`` copies every device tensor of the walk into a second
buffer and gives each a checksum (orv_amd/csrc/snapshot.hip), an event is recorded, and a writer thread takes the copies to disk while
training goes on.  The copies stay allocated until the files are written: a second copy of the state on the device (about 22 GB for the
2B model with AdamW and an EMA).  ``load_state`` hands the files to the objects' own ``load_state_dict`` and then, with ``verify=True``,
checksums the tensors that are now on the device against the manifest: what came back through the filesystem, host memory and the upload
is what was in device memory at the save, bit for bit.

``checkpoint-{step}/`` holds ``transformer/`` (what ``model.save_pretrained`` writes; with a LoRA adapter on the model the adapter file
``pytorch_lora_weights.safetensors`` instead), ``optimizer.safetensors`` + ``optimizer.json`` (the optimizer's ``state_dict()``: tensors
in the one file, a list of tensors as ``key.0``, ``key.1`` ..., everything else as JSON - no knowledge of a particular optimizer),
``ema.safetensors`` + ``ema.json`` likewise, ``scheduler.json``, ``random_states.json`` (per rank) and ``manifest.json``, written last.
JSON is written with sorted keys and no timestamps: two saves of the same state give byte-identical directories.

The lower layer - ``write_checkpoint``, ``read_checkpoint``, ``rotate``, ``latest_checkpoint`` - touches host tensors and files only.
"""
from __future__ import annotations

import json
import os
import random
import re
import shutil
import threading
from collections import OrderedDict
from typing import Callable, Dict, List, Optional, Tuple

import torch

FORMAT_VERSION = 1
MANIFEST_NAME = "manifest.json"
CHECKPOINT_PREFIX = "checkpoint-"
TMP_PREFIX = ".tmp-checkpoint-"          # does not start with "checkpoint-": the reference's own 'latest' scan can share the directory
_NUMBERED = re.compile(r"^checkpoint-(\d+)$")
SUPPORTED = ("supported: a model and a FusedAdamW / FusedProdigy / FusedCAME whose tensors are all on one GPU, an optional FusedEMA with the "
             "training weights in place (restore() called), outside a gradient window (after step() / zero_grad()), and no failed save before")


# ---- a state_dict as (tensors, JSON) ----
def split_state(sd: dict) -> Tuple["OrderedDict[str, torch.Tensor]", dict]:
    """Generic walk of a ``state_dict()``: a tensor goes to ``tensors[key]``, a non-empty list of tensors to ``key.0``, ``key.1`` ... (its
    length recorded under ``lists``), everything else to ``values`` as it is (it must be JSON)."""
    tensors, values, lists = OrderedDict(), {}, {}
    for k, v in sd.items():
        if torch.is_tensor(v):
            tensors[k] = v
        elif isinstance(v, (list, tuple)) and len(v) > 0 and all(torch.is_tensor(x) for x in v):
            lists[k] = len(v)
            for i, x in enumerate(v):
                tensors[f"{k}.{i}"] = x
        else:
            values[k] = v
    return tensors, {"values": values, "lists": lists}


def join_state(tensors: Dict[str, torch.Tensor], meta: dict) -> dict:
    """The inverse of ``split_state``."""
    listed = {f"{k}.{i}" for k, n in meta["lists"].items() for i in range(n)}
    sd = dict(meta["values"])
    sd.update({k: v for k, v in tensors.items() if k not in listed})
    for k, n in meta["lists"].items():
        sd[k] = [tensors[f"{k}.{i}"] for i in range(n)]
    return sd


def _dump_json(obj, path):
    with open(path, "w", encoding="utf-8") as f:
        json.dump(obj, f, sort_keys=True, indent=1)
        f.write("\n")


def _load_json(path):
    with open(path, "r", encoding="utf-8") as f:
        return json.load(f)


def _hex(x: int) -> str:
    return f"0x{int(x) & 0xFFFFFFFFFFFFFFFF:016x}"


# ---- the host-only layer ----
def write_checkpoint(directory: str, tensors: Dict[str, Dict[str, torch.Tensor]], meta: dict, sums: Dict[str, Dict[str, Tuple[int, int]]],
                     writers: Optional[Dict[str, Tuple[str, Callable]]] = None) -> None:
    """Writes one checkpoint directory from host data.  ``tensors``: ``{group: {name: CPU tensor}}``, each group into ``<group>.safetensors``
    unless ``writers[group] = (relative path, write(path, tensors))`` lays it out itself (``transformer/``, the LoRA file).  ``meta``:
    ``{"step": int, "extra": JSON, "files": {stem: JSON}}``, every entry of ``files`` into ``<stem>.json``.  ``sums``:
    ``{group: {name: (s1, s2)}}`` for every tensor.  ``manifest.json`` - format version, step, extra, and for every tensor of every group its
    name, dtype, shape and checksum - is written last: a directory without it is not a checkpoint."""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    manifest = {"format_version": FORMAT_VERSION, "step": int(meta["step"]), "extra": meta.get("extra"), "files": {}, "tensors": {}}
    for group, named in tensors.items():
        if set(sums.get(group, {})) != set(named):
            raise ValueError(f"write_checkpoint: the checksums of group {group!r} do not name the same tensors as the group")
        if writers and group in writers:
            rel, write = writers[group]
            write(os.path.join(directory, rel), named)
        else:
            rel = group + ".safetensors"
            save_file({k: v.contiguous() for k, v in named.items()}, os.path.join(directory, rel), metadata={"format": "pt"})
        manifest["files"][group] = rel
        manifest["tensors"][group] = {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape), "s1": _hex(sums[group][k][0]),
                                          "s2": _hex(sums[group][k][1])} for k, v in named.items()}
    for stem, obj in meta.get("files", {}).items():
        _dump_json(obj, os.path.join(directory, stem + ".json"))
    _dump_json(manifest, os.path.join(directory, MANIFEST_NAME))


def read_checkpoint(directory: str, checksum: Optional[Callable] = None) -> dict:
    """-> ``{"step", "extra", "files": {stem: JSON}, "tensors": {group: {name: CPU tensor}}, "manifest"}``.  Every tensor's name, dtype and
    shape is compared with the manifest; with ``checksum`` (a callable, CPU tensor -> (s1, s2)) its contents too.  A difference raises a
    ValueError that names the file and the tensor."""
    from safetensors.torch import load_file

    from .checkpoint import load_state_dict_dir
    path = os.path.join(directory, MANIFEST_NAME)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{directory} holds no {MANIFEST_NAME}: not a (complete) checkpoint")
    manifest = _load_json(path)
    if manifest.get("format_version") != FORMAT_VERSION:
        raise ValueError(f"{path}: format version {manifest.get('format_version')!r}; this build reads version {FORMAT_VERSION}")
    out = {"step": manifest["step"], "extra": manifest["extra"], "files": {}, "tensors": OrderedDict(), "manifest": manifest}
    for group, rel in manifest["files"].items():
        full = os.path.join(directory, rel)
        named = load_state_dict_dir(full) if os.path.isdir(full) else load_file(full)
        want = manifest["tensors"][group]
        if set(named) != set(want):
            odd = sorted(set(named) ^ set(want))
            raise ValueError(f"{full}: the tensors differ from the manifest's (first: {odd[0]!r})")
        for name, rec in want.items():
            t = named[name]
            if str(t.dtype).replace("torch.", "") != rec["dtype"] or list(t.shape) != rec["shape"]:
                raise ValueError(f"{full}: tensor {name!r} is {t.dtype} {list(t.shape)}, the manifest says {rec['dtype']} {rec['shape']}")
            if checksum is not None:
                got = tuple(_hex(x) for x in checksum(t))
                if got != (rec["s1"], rec["s2"]):
                    raise ValueError(f"{full}: tensor {name!r} has checksum {got}, the manifest says ({rec['s1']}, {rec['s2']}): the file "
                                     "does not hold what was saved")
        out["tensors"][group] = OrderedDict((name, named[name]) for name in want)
    for name in sorted(os.listdir(directory)):
        if name.endswith(".json") and name != MANIFEST_NAME:
            out["files"][name[:-len(".json")]] = _load_json(os.path.join(directory, name))
    return out


def _numbered(output_dir: str) -> List[Tuple[int, str]]:
    if not os.path.isdir(output_dir):
        return []
    found = []
    for name in os.listdir(output_dir):
        m = _NUMBERED.match(name)
        if m and os.path.isdir(os.path.join(output_dir, name)):
            found.append((int(m.group(1)), name))
    return sorted(found)


def rotate(output_dir: str, total_limit: Optional[int], keep: Optional[str] = None) -> List[str]:
    """Called AFTER a checkpoint is complete: removes the oldest ``checkpoint-N`` directories (by N) until at most ``total_limit`` remain,
    the new one counted - the set the reference's rule leaves (:1117-1139), which removes before it saves; removing afterwards means that
    a crash during the write still leaves the old checkpoint, also with ``total_limit=1``.  ``keep`` (a directory name) is never removed.
    ``None`` removes nothing.  -> the removed names."""
    if total_limit is None:
        return []
    names = [name for _, name in _numbered(output_dir)]
    extra = len(names) - max(int(total_limit), 1 if keep in names else 0)
    removed = []
    for name in names:
        if len(removed) >= extra:
            break
        if name == keep:
            continue
        shutil.rmtree(os.path.join(output_dir, name), ignore_errors=True)
        removed.append(name)
    return removed


def latest_checkpoint(output_dir: str) -> Optional[str]:
    """The ``checkpoint-N`` directory with the largest N among those that hold a ``manifest.json`` (numeric order), or None.  ``.tmp-*``
    directories, directories without a manifest and the reference's bare ``checkpoint`` export are not candidates."""
    done = [name for _, name in _numbered(output_dir) if os.path.exists(os.path.join(output_dir, name, MANIFEST_NAME))]
    return os.path.join(output_dir, done[-1]) if done else None


# ---- random-number generators ----
def _bytes_hex(t: torch.Tensor) -> str:
    return bytes(t.cpu().numpy().tobytes()).hex()


def _hex_bytes(h: str) -> torch.Tensor:
    return torch.tensor(list(bytes.fromhex(h)), dtype=torch.uint8)


def random_state(generator: Optional[torch.Generator] = None) -> dict:
    """This process's generator states as JSON: Python ``random``, numpy, torch's CPU default generator, the default generator of the
    current GPU (where one is initialised) and ``generator`` (the one handed to ``sft_step``)."""
    import numpy as np
    ver, inner, gauss = random.getstate()
    name, keys, pos, has_gauss, cached = np.random.get_state()
    st = {"python": [ver, list(inner), gauss], "numpy": [name, [int(x) for x in keys], int(pos), int(has_gauss), float(cached)],
          "torch_cpu": _bytes_hex(torch.get_rng_state()), "torch_device": None, "generator": None}
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        st["torch_device"] = _bytes_hex(torch.cuda.get_rng_state())
    if generator is not None:
        st["generator"] = _bytes_hex(generator.get_state())
    return st


def set_random_state(st: dict, generator: Optional[torch.Generator] = None) -> None:
    import numpy as np
    ver, inner, gauss = st["python"]
    random.setstate((ver, tuple(inner), gauss))
    name, keys, pos, has_gauss, cached = st["numpy"]
    np.random.set_state((name, np.array(keys, dtype=np.uint32), pos, has_gauss, cached))
    torch.set_rng_state(_hex_bytes(st["torch_cpu"]))
    if st.get("torch_device") is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(_hex_bytes(st["torch_device"]))
    if generator is not None:
        if st.get("generator") is None:
            raise ValueError("load_state: the checkpoint holds no state for `generator` (it was saved without one)")
        generator.set_state(_hex_bytes(st["generator"]))


def _rank_world() -> Tuple[int, int]:
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def collect_random_states(generator: Optional[torch.Generator] = None) -> List[dict]:
    """``random_state`` of every rank, in rank order.  With ``torch.distributed`` initialised this is a collective (``all_gather_object``):
    every rank calls it at the same step."""
    mine = random_state(generator)
    rank, world = _rank_world()
    if world == 1:
        return [mine]
    import torch.distributed as dist
    out = [None] * world
    dist.all_gather_object(out, mine)
    return out


# ---- the walk over model, optimizer and EMA ----
def _walk(model, optimizer, ema):
    """-> (``{group: {name: (tensor, copy)}}``, ``{stem: JSON}``).  ``copy``: the tensor changes while training (it goes through the snapshot);
    False: a frozen weight or a buffer, checksummed now and written from where it lives."""
    groups, metas = OrderedDict(), {}
    adapter = getattr(model, "active_adapter", None)
    if adapter is not None:
        groups["lora"] = OrderedDict(("transformer." + k, (v.detach(), True)) for k, v in model.get_adapter_state_dict(adapter).items())
    else:
        trainable = {name for name, p in model.named_parameters() if p.requires_grad}
        groups["transformer"] = OrderedDict((k, (v.detach(), k in trainable)) for k, v in model.state_dict().items())
    for stem, obj in (("optimizer", optimizer), ("ema", ema)):
        if obj is None:
            continue
        tensors, metas[stem] = split_state(obj.state_dict())
        groups[stem] = OrderedDict((k, (v.detach(), True)) for k, v in tensors.items())
    return groups, metas


def _refuse(why: str):
    raise RuntimeError(f"save_state: {why} ({SUPPORTED})")


class SaveHandle:
    """One ``save_state`` call.  ``path``: the final ``checkpoint-{step}`` directory; ``done``: the rename has happened (or the save has
    failed: ``error``); ``wait()`` blocks until then and raises what the writer raised."""

    def __init__(self, path: str):
        self.path = path
        self.error: Optional[BaseException] = None
        self._thread: Optional[threading.Thread] = None
        self._finished = threading.Event()

    @property
    def done(self) -> bool:
        return self._finished.is_set()

    def wait(self) -> "SaveHandle":
        if self._thread is not None:
            self._thread.join()
        if self.error is not None:
            raise RuntimeError(f"save_state: writing {self.path} failed: {self.error!r}") from self.error
        return self


_previous: List[Optional[SaveHandle]] = [None]


def _write_job(handle: SaveHandle, output_dir, step, device, event, groups, copies, sums, meta, writers, total_limit):
    tmp = os.path.join(output_dir, f"{TMP_PREFIX}{step}")
    try:
        torch.cuda.set_device(device)
        event.synchronize()                              # the snapshot is complete; the training stream is not waited for again
        side = torch.cuda.Stream(device)
        with torch.cuda.stream(side):                    # device -> host on a stream of this thread's own
            host = OrderedDict()
            i = 0
            for group, named in groups.items():
                host[group] = OrderedDict()
                for name, (live, _) in named.items():
                    host[group][name] = (copies[i] if copies[i] is not None else live).cpu()
                    i += 1
            flat = [(int(a) & 0xFFFFFFFFFFFFFFFF, int(b) & 0xFFFFFFFFFFFFFFFF) for a, b in sums.cpu().tolist()]
        side.synchronize()
        copies.clear()                                   # the second copy of the state is free from here on
        it = iter(flat)
        host_sums = {group: {name: next(it) for name in named} for group, named in host.items()}
        if os.path.isdir(tmp):
            shutil.rmtree(tmp)
        write_checkpoint(tmp, host, meta, host_sums, writers)
        if os.path.isdir(handle.path):
            shutil.rmtree(handle.path)
        os.replace(tmp, handle.path)
        rotate(output_dir, total_limit, keep=os.path.basename(handle.path))
    except BaseException as e:       # noqa: BLE001 - reported through the handle; the next save_state refuses
        handle.error = e
        shutil.rmtree(tmp, ignore_errors=True)
    finally:
        copies.clear()
        handle._finished.set()


def save_state(output_dir: str, step: int, *, model, optimizer, lr_scheduler=None, ema=None, generator=None, extra=None,
               total_limit: Optional[int] = None, blocking: bool = False) -> SaveHandle:
    """Writes ``output_dir/checkpoint-{step}`` (module docstring).  The training stream is held for the snapshot only; with ``blocking=True``
    the call returns after the rename.  A second call first waits for the previous one.  Under ``torch.distributed`` every rank calls this
    at the same step (the generator states are gathered) and rank 0 writes."""
    from . import ops
    previous, _previous[0] = _previous[0], None
    if previous is not None:
        if previous._thread is not None:
            previous._thread.join()
        if previous.error is not None:
            _refuse(f"the previous save ({previous.path}) failed: {previous.error!r}")
    if ema is not None and ema._stash is not None:
        _refuse("the averaged weights are swapped in (FusedEMA.store() without restore()): the parameters are not the training weights")
    if getattr(optimizer, "_handed", None):
        _refuse("the optimizer is in the middle of a gradient window (gradient segments handed to a backward since the last step())")
    groups, metas = _walk(model, optimizer, ema)
    every = [(f"{g}:{k}", t) for g, named in groups.items() for k, (t, _) in named.items()]
    every += [(f"optimizer.params[{i}]", p) for i, p in enumerate(optimizer.params)]
    cpu = [name for name, t in every if not t.is_cuda]
    if cpu:
        _refuse(f"{len(cpu)} CPU tensors (first: {cpu[0]}); the snapshot runs on the GPU")
    saved = {t.data_ptr() for named in groups.values() for t, copy in named.values() if copy}
    lost = [i for i, p in enumerate(optimizer.params) if p.data_ptr() not in saved]
    if lost:
        _refuse(f"optimizer.params[{lost[0]}] is not a trainable parameter of `model`: its weights would not be in the checkpoint")
    path = os.path.join(output_dir, f"{CHECKPOINT_PREFIX}{int(step)}")
    handle = SaveHandle(path)
    states = collect_random_states(generator)            # a collective under torch.distributed
    rank, _ = _rank_world()
    if rank != 0:
        handle._finished.set()
        _previous[0] = handle
        return handle
    os.makedirs(output_dir, exist_ok=True)
    # host state as it is NOW (JSON text round trip: nothing the loop changes later is shared with the writer)
    files = {stem: m for stem, m in metas.items()}
    if lr_scheduler is not None:
        files["scheduler"] = lr_scheduler.state_dict()
    files["random_states"] = {"ranks": states}
    meta = json.loads(json.dumps({"step": int(step), "extra": extra, "files": files}))
    # ONE table launch over every device tensor of the walk
    tensors, flags = [], []
    for named in groups.values():
        for name, (t, copy) in list(named.items()):
            if not t.is_contiguous() or t.data_ptr() % 4:            # a strided or oddly placed frozen tensor: a compact stand-in
                t = t.contiguous().clone()
                named[name] = (t, copy)
            tensors.append(t)
            flags.append(copy)
    device = tensors[0].device
    copies, sums = ops.snapshot(tensors, copy=flags)
    event = torch.cuda.Event()
    event.record()
    writers = {}
    if "lora" in groups:
        from .lora import LORA_WEIGHT_NAME
        adapter = model.active_adapter
        strip = len("transformer.")
        writers["lora"] = (LORA_WEIGHT_NAME, lambda p, named: model.save_lora_adapter(
            os.path.dirname(p), adapter_name=adapter, state_dict=OrderedDict((k[strip:], v) for k, v in named.items())))
    elif hasattr(model, "save_pretrained"):
        writers["transformer"] = ("transformer", lambda p, named: model.save_pretrained(p, state_dict=named))
    else:
        from .checkpoint import save_state_dict_dir
        writers["transformer"] = ("transformer", lambda p, named: (os.makedirs(p, exist_ok=True), save_state_dict_dir(named, p)))
    args = (handle, output_dir, int(step), device, event, groups, copies, sums, meta, writers, total_limit)
    _previous[0] = handle
    if blocking:
        _write_job(*args)
        return handle.wait()
    handle._thread = threading.Thread(target=_write_job, args=args, name=f"orv-save-{int(step)}", daemon=False)
    handle._thread.start()
    return handle


def load_state(path: str, *, model, optimizer, lr_scheduler=None, ema=None, generator=None, verify: bool = True,
               resume: Optional[str] = None) -> dict:
    """Brings a run back: ``path`` is a ``checkpoint-N`` directory, or an ``output_dir`` with ``resume="latest"``.  The files are handed to
    the objects' own ``load_state_dict`` (another optimizer class, trainable set or flat order fails with their messages); parameters are
    copied in place into their current storage.  ``verify``: the tensors now on the device are checksummed (``ops.checksum``) against the
    manifest; a mismatch raises a ValueError naming the file and the tensor.  Then the generator states of this rank are restored and the
    weights epoch is bumped.  -> ``{"step", "extra"}``."""
    from . import _state, ops
    if resume is not None:
        if resume != "latest":
            raise ValueError(f"load_state: resume={resume!r} (supported: 'latest', or None with the checkpoint directory as path)")
        found = latest_checkpoint(path)
        if found is None:
            raise FileNotFoundError(f"load_state: no complete checkpoint-N directory under {path}")
        path = found
    ck = read_checkpoint(path)
    groups, files = ck["tensors"], ck["files"]
    adapter = getattr(model, "active_adapter", None)
    if "lora" in groups:
        if adapter is None:
            raise ValueError(f"load_state: {path} holds a LoRA adapter and no transformer/; add the adapter to the model first (add_adapter)")
        model.load_lora_adapter(path, adapter_name=adapter)               # the file itself: lora_alpha travels in its metadata
    else:
        if adapter is not None:
            raise ValueError(f"load_state: {path} holds a full transformer/, the model carries the LoRA adapter {adapter!r}")
        model.load_state_dict(groups["transformer"], strict=True)          # in place: every parameter keeps its storage
    for stem, obj in (("optimizer", optimizer), ("ema", ema)):
        if obj is None:
            continue
        if stem not in groups:
            raise ValueError(f"load_state: {path} holds no {stem}.safetensors (it was saved without one)")
        obj.load_state_dict(join_state(groups[stem], files[stem]))
    if lr_scheduler is not None:
        if "scheduler" not in files:
            raise ValueError(f"load_state: {path} holds no scheduler.json (it was saved without a schedule)")
        lr_scheduler.load_state_dict(files["scheduler"])
    if verify:
        now, _ = _walk(model, optimizer, ema)
        named = [(g, k, t) for g, group in now.items() for k, (t, _) in group.items() if k in ck["manifest"]["tensors"].get(g, {})]
        fixed = [t if t.is_contiguous() and t.data_ptr() % 4 == 0 else t.contiguous().clone() for _, _, t in named]
        got = ops.sums_to_ints(ops.checksum(fixed)) if fixed else []
        for (g, k, _), (s1, s2) in zip(named, got):
            rec = ck["manifest"]["tensors"][g][k]
            if (_hex(s1), _hex(s2)) != (rec["s1"], rec["s2"]):
                raise ValueError(f"load_state: {os.path.join(path, ck['manifest']['files'][g])}: tensor {k!r} has checksum "
                                 f"({_hex(s1)}, {_hex(s2)}) on the device, the manifest says ({rec['s1']}, {rec['s2']}): what was loaded is "
                                 "not what was saved")
    states = files["random_states"]["ranks"]
    rank, _ = _rank_world()
    if rank >= len(states):
        raise ValueError(f"load_state: {path} holds generator states of {len(states)} ranks; this is rank {rank}")
    set_random_state(states[rank], generator)
    _state.bump_weights_epoch()
    return {"step": ck["step"], "extra": ck["extra"]}
