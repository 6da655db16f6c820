"""Cascaded long-video rollouts: a 17-frame chunk, one generated frame as the reference image of the next chunk, the chunks stitched into
an episode - the reference's ``eval_config.cascaded`` (orv/pipeline/evaluation_control_to_video.py:289-379 over the slices of
``CascadedRobotDataset._load_and_process_ann_file``, orv/dataset/dataset.py:1227-1361) as one call with the chunk boundary on the device.

* ``plan_slices`` / ``stitch_ranges`` (host): which frames each chunk covers, which frame it hands to the next chunk and which of its
  positions go into the episode.  Equal to the reference's own loops, quirks included (tests/golden/rollout_plan.json is written by those
  loops, tools/gen_rollout_golden.py); the one deviation is stated at ``stitch_ranges``.
* ``rollout`` (``pipe.rollout``): per chunk one ``orv_frames_quantize`` launch per stitched range - the decoder's output to uint8 frames,
  written where they belong in the episode buffer - and one ``orv_frames_handoff`` launch that turns the hand-off frame's uint8 values
  into the channels-last tensor the VAE encoder reads.  What the loop written by hand around ``pipe(...)`` does between two chunks on
  the host (``postprocess_video('pil')``: an fp32 copy of the clip to the host and two numpy passes; ``preprocess``: a PIL frame through
  numpy and back to the device) is gone; the values are the same bit for bit.

File reading and the action arithmetic of ``CascadedRobotDataset`` stay with the caller, who supplies each slice's controls
(``conditions.encode_controls(..., frame_ids=slice.frame_ids)`` serves depth and label latents); so do the mp4 / GIF writers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Sequence, Tuple, Union

SUPPORTED = ("supported: one view (num_views = 1), a pipeline on the GPU with an orv_amd VAE, hand-off frames of the call's (height, width), "
             "controls_for_slice as a callable Slice -> dict or a sequence with one dict per slice, output_type 'u8', 'np' or 'pil'")


@dataclass(frozen=True)
class Slice:
    """One chunk of an episode: the frames it covers (``frame_ids[0]`` is the reference frame when the VAE has a first single frame),
    the frame the NEXT kept slice starts from (-1 on the last kept slice) and the reference's ``is_last`` / ``sample_index`` labels."""
    frame_ids: Tuple[int, ...]
    start_frame_idx: int
    next_start_frame_idx: int
    is_last: bool
    sample_index: int


def plan_slices(n_frames: int, sequence_length: int = 16, sequence_interval: int = 1, start_frame_interval: int = 16,
                vae_has_first_single_frame: bool = True) -> List[Slice]:
    """The slices of an episode of ``n_frames`` frames, as dataset.py:1255-1359 cuts them (without the file existence checks of
    :1321-1351).  Slices start every ``start_frame_interval * sequence_interval`` frames and take ``sequence_length`` frames
    ``sequence_interval`` apart; with ``vae_has_first_single_frame`` the frame one interval before is put in front (8 n + 1 frames).
    Quirks kept: a trailing slice that is short by more than 2 frames is regenerated backwards from the episode's last frame (so it
    overlaps its predecessor and the hand-off lands in mid-slice); one short by 1 or 2 is dropped, and then no slice carries
    ``is_last``; any other short slice is dropped too."""
    n, L, iv, stride = int(n_frames), int(sequence_length), int(sequence_interval), int(start_frame_interval)
    if L < 1 or iv < 1 or stride < 1:
        raise ValueError(f"orv_amd.rollout: sequence_length = {L}, sequence_interval = {iv}, start_frame_interval = {stride}; supported: "
                         "positive integers")
    first = iv if vae_has_first_single_frame else 0
    slices = []
    for frame_i in range(first, n, stride * iv):
        ids = list(range(frame_i, n, iv))[:L]
        is_last = ids[-1] == n - 1
        if is_last and n >= L and L - len(ids) > 2:
            ids = list(range(n - 1 - (L - 1) * iv, n, iv))
        if len(ids) != L:
            continue
        if vae_has_first_single_frame:
            ids.insert(0, ids[0] - iv)
        slices.append((tuple(ids), is_last))
    if not slices:
        need = (L - 1) * iv + 1 + first
        raise ValueError(f"orv_amd.rollout: n_frames = {n} is too short for one slice of sequence_length = {L} at sequence_interval = {iv}"
                         f"{' after the first single frame' if first else ''}; supported: n_frames >= {need}")
    starts = [ids[0] for ids, _ in slices] + [-1]
    plan = [Slice(ids, ids[0], starts[k + 1], last, k) for k, (ids, last) in enumerate(slices)]
    for s in plan:
        if s.next_start_frame_idx != -1 and s.next_start_frame_idx not in s.frame_ids:
            raise ValueError(f"orv_amd.rollout: slice {s.sample_index} covers frames {s.frame_ids[0]}..{s.frame_ids[-1]} and the next one starts "
                             f"from frame {s.next_start_frame_idx}, which it does not generate (start_frame_interval = {stride} reaches past "
                             f"the slice's {len(s.frame_ids)} frames: a stride above sequence_length, or equal to it without the first single "
                             f"frame); supported: a hand-off frame inside the current slice")
    return plan


def stitch_ranges(plan: Sequence[Slice], keep_last_frame: bool = False) -> List[Tuple[int, int, int]]:
    """``(slice_index, begin, end)`` per slice: the positions ``[begin, end)`` of that slice's frames that go into the episode.

    A slice contributes the positions in front of its hand-off frame, which opens the next slice; the last slice contributes ``[0:-1]``,
    as evaluation_control_to_video.py:366-375 does - the reference drops the episode's final frame.  ``keep_last_frame=True`` keeps it.

    Deviation from the reference, for ``sequence_interval > 1`` only: it computes ``end`` as a difference of frame IDS
    (``next_start - start``) where a list POSITION is meant, which repeats the hand-off frame (n_frames = 70 at interval 2 repeats frame
    32).  Here ``end`` is the position of ``next_start_frame_idx`` in ``frame_ids``; at ``sequence_interval == 1`` the two are the same
    number and the result equals the reference's exactly."""
    plan = list(plan)
    if not plan:
        raise ValueError("orv_amd.rollout: the plan is empty; supported: the slices plan_slices returns")
    out = []
    for k, s in enumerate(plan):
        if k < len(plan) - 1:
            if s.next_start_frame_idx not in s.frame_ids:
                raise ValueError(f"orv_amd.rollout: slice {k} hands off frame {s.next_start_frame_idx}, which is not among its frame_ids "
                                 f"{s.frame_ids[0]}..{s.frame_ids[-1]}; supported: a hand-off frame inside the current slice")
            end = s.frame_ids.index(s.next_start_frame_idx)
        else:
            end = len(s.frame_ids) if keep_last_frame else len(s.frame_ids) - 1
        out.append((k, 0, end))
    return out


def stitched_frame_ids(plan: Sequence[Slice], keep_last_frame: bool = False) -> List[int]:
    """The frame id behind every frame of the stitched episode, in order."""
    plan = list(plan)
    return [plan[k].frame_ids[p] for k, b, e in stitch_ranges(plan, keep_last_frame) for p in range(b, e)]


def handoff_table():
    """uint8 level -> the bf16 value the next chunk's encoder sees, by the statements of ``VideoProcessor.preprocess`` on a PIL frame
    (``np.float32(u) / 255.0``, then ``2.0 * x - 1.0`` in fp32) and the pipeline's ``.to(bfloat16)``: bf16 [256] on the host."""
    import numpy as np
    import torch
    x = torch.from_numpy(np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0)
    return (2.0 * x - 1.0).to(torch.bfloat16)


@dataclass
class RolloutOutput:
    """``frames``: the episode(s) - uint8 [B, N_out, H, W, 3] on the device ('u8'), the same as a numpy array ('np') or B lists of PIL
    frames ('pil'); ``slices``: the plan; ``ranges``: ``stitch_ranges`` of it."""
    frames: object
    slices: List[Slice]
    ranges: List[Tuple[int, int, int]]


def rollout(pipe, image, plan: Sequence[Slice], controls_for_slice: Union[Callable[[Slice], Dict], Sequence[Dict]], prompt_embeds=None,
            seed: int = 0, height: int = None, width: int = None, num_inference_steps: int = 50, guidance_scale: float = 1.0,
            use_dynamic_cfg: bool = False, keep_last_frame: bool = False, output_type: str = "u8", prompt=None, negative_prompt=None,
            negative_prompt_embeds=None, num_views: int = 1) -> RolloutOutput:
    """Generates the episode ``plan`` describes, one pipeline call per slice (chunk k of all B episodes at once; the reference runs
    B = 1), and returns its stitched frames.

    ``image`` is what ``pipe(...)`` takes for the first chunk (PIL, an RGB tensor, pre-encoded latents or moments); every later chunk
    starts from the frame its predecessor generated at ``next_start_frame_idx``, ROUNDED to uint8 as the reference's PIL round trip
    rounds it.  Each chunk draws from a fresh ``torch.Generator().manual_seed(seed)`` (evaluation_control_to_video.py:347) in
    ``__call__``'s order (image latents, initial noise, DPM noise); with B > 1 every episode has its own such generator, so that a batch
    equals its episodes run one at a time.  ``controls_for_slice(slice)`` (or ``controls_for_slice[k]``) is that chunk's
    ``controls_or_guidances``.  A NaN in the decoder's output becomes level 0 (the reference's numpy cast of a NaN is platform-defined).
    """
    import torch
    from . import ops
    from .cogvideox_control import ChannelsLastFrames
    plan = list(plan)
    ranges = stitch_ranges(plan, keep_last_frame)
    if output_type not in ("u8", "np", "pil"):
        raise ValueError(f"orv_amd.rollout: output_type = {output_type!r}; {SUPPORTED}")
    if num_views != 1:
        raise ValueError(f"orv_amd.rollout: num_views = {num_views}; the reference's cascade is single-view; {SUPPORTED}")
    if height is None or width is None:
        raise ValueError(f"orv_amd.rollout: height = {height}, width = {width}; supported: the frame size of every chunk, given explicitly "
                         "(there is no resize between chunks)")
    if callable(controls_for_slice):
        controls = [controls_for_slice(s) for s in plan]
    else:
        controls = list(controls_for_slice)
    if len(controls) != len(plan) or not all(isinstance(c, dict) for c in controls):
        raise ValueError(f"orv_amd.rollout: controls_for_slice gave {len(controls)} entries ({sorted({type(c).__name__ for c in controls})}) for "
                         f"{len(plan)} slices; {SUPPORTED}")
    device = pipe._execution_device
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"orv_amd.rollout: the pipeline is on {device}; there is no CPU path; {SUPPORTED}")
    if pipe.vae is None or not hasattr(pipe.vae, "encode_channels_last"):
        raise RuntimeError(f"orv_amd.rollout: the hand-off writes the input of orv_amd.vae.AutoencoderKLCogVideoX.encode_channels_last and the "
                           f"pipeline's vae is {type(pipe.vae).__name__}; {SUPPORTED}")
    lengths = {len(s.frame_ids) for s in plan}
    if len(lengths) != 1:
        raise ValueError(f"orv_amd.rollout: the slices have {sorted(lengths)} frames; supported: one length (what plan_slices returns)")
    num_frames = lengths.pop()
    if prompt is not None and prompt_embeds is None:
        # the text is encoded once for all chunks (the loop written by hand encodes it once per chunk, to the same embeddings)
        prompt_embeds, negative_prompt_embeds = pipe.encode_prompt(prompt=prompt, negative_prompt=negative_prompt,
                                                                   do_classifier_free_guidance=guidance_scale > 1.0,
                                                                   negative_prompt_embeds=negative_prompt_embeds, device=device)
        prompt = negative_prompt = None
    table = None
    n_out = sum(e - b for _, b, e in ranges)
    frames, at, handoff = None, 0, None
    for k, s in enumerate(plan):
        if k:
            table = handoff_table().to(device) if table is None else table
            image = ops.frames_handoff(handoff[0], handoff[1], table)          # bf16 [B, 1, H, W, 8]: the encoder's input
        generator = torch.Generator().manual_seed(seed)
        call = pipe._prepare_call(image, prompt=prompt, negative_prompt=negative_prompt, height=height, width=width, num_views=1,
                                  num_frames=num_frames, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                  use_dynamic_cfg=use_dynamic_cfg, generator=generator, prompt_embeds=prompt_embeds,
                                  negative_prompt_embeds=negative_prompt_embeds, controls_or_guidances=controls[k])
        if call.batch_size > 1:      # one generator per episode: a batch equals its episodes run one at a time
            call.generator = [torch.Generator().manual_seed(seed) for _ in range(call.batch_size)]
        if k == 0:
            image = pipe.video_processor.preprocess(image, height=height, width=width).to(device=device, dtype=call.dtype)
        else:
            image = ChannelsLastFrames(image)
        video = pipe._generate(image, call)                                           # [B, 3, F, H, W] on the device
        if video.dim() != 5 or video.shape[1] != 3 or video.shape[2] < num_frames:
            raise RuntimeError(f"orv_amd.rollout: chunk {k} decoded {tuple(video.shape)} for a slice of {num_frames} RGB frames")
        if tuple(video.shape[3:]) != (height, width):
            raise RuntimeError(f"orv_amd.rollout: chunk {k} generated {video.shape[3]} x {video.shape[4]} frames and the hand-off frame must be "
                               f"(height, width) = ({height}, {width}); there is no resize between chunks; {SUPPORTED}")
        if frames is None:
            frames = torch.empty(video.shape[0], n_out, height, width, 3, dtype=torch.uint8, device=video.device)
        _, b, e = ranges[k]
        if k == len(plan) - 1:
            ops.frames_quantize(video, b, e, out=frames, dst_f0=at)
        elif at + e + 1 <= n_out:
            # every frame is quantized once: the stitched range and, behind it, the hand-off frame - in the place the next chunk's first
            # frame (the same frame id, generated again) overwrites after the hand-off has read it (stream order)
            ops.frames_quantize(video, b, e + 1, out=frames, dst_f0=at)
            handoff = (frames, at + e)
        else:                        # a last slice that contributes nothing (sequence_length = 1 without a first single frame)
            ops.frames_quantize(video, b, e, out=frames, dst_f0=at)
            handoff = (ops.frames_quantize(video, e, e + 1), 0)
        at += e - b
    pipe.maybe_free_model_hooks()
    if output_type == "u8":
        out = frames
    else:
        out = frames.cpu().numpy()
        if output_type == "pil":
            import PIL.Image
            out = [[PIL.Image.fromarray(f) for f in clip] for clip in out]
    return RolloutOutput(frames=out, slices=plan, ranges=ranges)


# ``orv_amd.rollout`` is this MODULE - the import system binds a submodule to its name in the package whenever it is imported - and the
# package also exports the function of that name.  So that the name holds one object at all times, the package hands out the module for
# it (orv_amd/__init__.py) and the module is callable: ``orv_amd.rollout(pipe, ...)`` and ``from orv_amd import rollout; rollout(pipe, ...)``
# run the function below, ``orv_amd.rollout.rollout`` is the function itself.
class _CallableModule(type(__import__("sys"))):
    def __call__(self, *args, **kw):
        return rollout(*args, **kw)


__import__("sys").modules[__name__].__class__ = _CallableModule
