#!/usr/bin/env python
"""Writes tests/golden/rollout_plan.json: the reference's own slice plans and stitched frame-id lists for cascaded rollouts.

    python tools/gen_rollout_golden.py --reference /path/to/ORV [--out tests/golden/rollout_plan.json]

Neither reference module can be imported (both need packages that have nothing to do with these lines), so their syntax trees are cut
instead, at run time:
  * the planner: the statements of CascadedRobotDataset._load_and_process_ann_file (orv/dataset/dataset.py) from the assignment of
    ``start_frame`` up to its ``return``, executed with a stand-in ``self`` (a config with use_cond = filter_by_cond = False, so the
    file existence checks inside the loop never run) and an ``ann`` of ``n_frames`` states;
  * the stitch: the ``if eval_config.cascaded:`` statement of the evaluation loop (orv/pipeline/evaluation_control_to_video.py), executed
    once per planned slice with ``videos = [frame_ids]`` - the slice's frame ids stand in for its frames - and the loop's carried
    variables kept in one namespace, as the loop carries them.  What it leaves in ``videos[0]`` after the last slice is the episode.
The stitch is recorded for ``sequence_interval == 1`` only; at a larger interval the reference subtracts frame ids where it means list
positions and repeats the hand-off frame (orv_amd.rollout.stitch_ranges states the deviation), so those cases are planner-only.

Every case is asserted to keep its hand-off frame inside the current slice and to agree with orv_amd.rollout before it is written.  No
reference text is in this tool or in the fixture.  No test runs this tool; tests/test_rollout_host.py reads what it wrote.
"""
import argparse
import ast
import copy
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orv_amd import rollout  # noqa: E402


class Config(dict):
    """Attribute access and ``in`` over one dict, the two ways the reference reads its config."""
    __getattr__ = dict.__getitem__


def _targets(stmt):
    return [t.id for t in stmt.targets if isinstance(t, ast.Name)] if isinstance(stmt, ast.Assign) else []


class Reference:
    def __init__(self, root):
        path = os.path.join(root, "orv", "dataset", "dataset.py")
        with open(path, "r", encoding="utf-8") as f:
            tree = ast.parse(f.read(), filename=path)
        cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "CascadedRobotDataset")
        fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_load_and_process_ann_file")
        i0 = next(i for i, s in enumerate(fn.body) if "start_frame" in _targets(s))
        cut = fn.body[i0:]
        assert isinstance(cut[-1], ast.Return) and ast.unparse(cut[-1].value) == "samples", "the planner's return was not found"
        cut = cut[:-1]
        assert not any(isinstance(c, ast.Return) for s in cut for c in ast.walk(s))
        self.plan_code = compile(ast.Module(body=cut, type_ignores=[]), path, "exec")

        path = os.path.join(root, "orv", "pipeline", "evaluation_control_to_video.py")
        with open(path, "r", encoding="utf-8") as f:
            tree = ast.parse(f.read(), filename=path)
        hits = [n for n in ast.walk(tree) if isinstance(n, ast.If) and ast.unparse(n.test) == "eval_config.cascaded"
                and any("metainfos" in _targets(s) for s in n.body)]
        assert len(hits) == 1, "the cascade branch of the evaluation loop was not found"
        self.stitch_code = compile(ast.Module(body=[hits[0]], type_ignores=[]), path, "exec")

    def plan(self, n_frames, sequence_length, sequence_interval, start_frame_interval, vae_has_first_single_frame):
        config = Config(vae_has_first_single_frame=vae_has_first_single_frame, sequence_interval=sequence_interval,
                        sequence_length=sequence_length, caption_column="caption", use_cond=False, filter_by_cond=False, load_tensor=False)
        ns = {"self": types.SimpleNamespace(config=config, start_frame_interval=start_frame_interval), "os": os,
              "ann": {"episode_id": "0", "caption": ["a caption"], "state": [None] * n_frames}, "n_frames": n_frames, "samples": [],
              "ann_file": None, "recon_file": None, "label_file": None, "render_file": None, "episode_id": "0"}
        exec(self.plan_code, ns)
        return ns["samples"]

    def stitch(self, samples):
        ns = {"eval_config": types.SimpleNamespace(cascaded=True), "copy": copy, "all_video_slices": [], "episode_start_frame_ids": [0],
              "next_start_frame": None}
        for sample in samples:
            ns["batch"], ns["videos"] = {"metainfos": [sample]}, [list(sample["frame_ids"])]
            exec(self.stitch_code, ns)
        assert samples[-1]["next_start_frame_idx"] == -1 and ns["all_video_slices"] == []
        return list(ns["videos"][0])


KEYS = ("frame_ids", "start_frame_idx", "next_start_frame_idx", "is_last", "sample_index")

CASES = ([(n, 16, 1, 16, True) for n in (17, 18, 20, 31, 32, 33, 34, 40, 47, 48, 49, 50)]
         + [(n, 8, 1, 8, True) for n in (12, 17, 19, 20, 25)]
         # stride 4: at n = 17 and 25 the planner regenerates the slice that already ends on the last frame a second time and the
         # evaluation loop's own assertion refuses the plan (two slices carry is_last), so 16 and 24 stand in for them
         + [(n, 8, 1, 4, True) for n in (12, 16, 19, 20, 24)]
         # without the first single frame a stride equal to the length leaves the hand-off frame outside the slice: shorter strides
         + [(39, 16, 1, 8, False), (19, 8, 1, 4, False), (23, 8, 1, 7, False), (27, 8, 1, 7, False)]
         + [(70, 16, 2, 16, True), (40, 8, 2, 8, True)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds orv/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rollout_plan.json"))
    args = ap.parse_args()
    reference = Reference(args.reference)
    cases = []
    for n, length, interval, stride, first in CASES:
        samples = reference.plan(n, length, interval, stride, first)
        slices = [{k: s[k] for k in KEYS} for s in samples]
        for s in slices[:-1]:
            assert s["next_start_frame_idx"] in s["frame_ids"], f"{(n, length, interval, stride, first)}: the hand-off frame is outside the slice"
        stitched = reference.stitch(samples) if interval == 1 else None
        mine = rollout.plan_slices(n, length, interval, stride, first)
        assert [{k: (list(getattr(s, k)) if k == "frame_ids" else getattr(s, k)) for k in KEYS} for s in mine] == slices, (n, length, interval, stride, first)
        if stitched is not None:
            assert rollout.stitched_frame_ids(mine) == stitched, (n, length, interval, stride, first)
        cases.append({"inputs": {"n_frames": n, "sequence_length": length, "sequence_interval": interval, "start_frame_interval": stride,
                                 "vae_has_first_single_frame": first}, "slices": slices, "stitched": stitched})
        print(f"n = {n:3d} L = {length:2d} interval {interval} stride {stride:2d} first {int(first)}: {len(slices)} slices, starts "
              f"{[s['start_frame_idx'] for s in slices]}, is_last {[int(s['is_last']) for s in slices]}, "
              f"{'planner only' if stitched is None else str(len(stitched)) + ' stitched frames'}")
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{args.out}: {len(cases)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
