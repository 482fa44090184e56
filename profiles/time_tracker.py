"""Object tracks on the device: what a push of ObjectTracker costs at 512x1024, B = 1, M = 64, both directions, on the three masks of
profiles/time_segments.py, each moved by a smooth flow, beside pf_epi_map (one pass over the same pixels) and MovingObjects.update
(DESIGN.md section 26).  Interleaved rounds on one box, medians and the spread of the same run:

  (a) alone, one captured graph each, microseconds per replay between device events, per mask:
        begin_us, vote1_us (the forward flow alone), vote2_us (both flows: two launches), match_us, paint_us: launch by launch
        push_us        ObjectTracker.link with both flows (the five launches)
        update_us      MovingObjects.update of the second mask (eight launches): a yardstick
        accumulate_us  pf_seg_objects (five launches, of which pf_seg_objects_accumulate is the pixel pass): what the vote pass is
                       compared with
        map_us         pf_epi_map, all four outputs: the yardstick
      The vote graphs replay without a begin between them, so the matrix keeps growing (and may wrap): the same adds, the same time.
  (b) milliseconds per frame of the warm bidirectional FlowStream step (512x1024, iters 12, B = 1, occlusion "plane") with a
      MovingObjects.update of its occlusion mask behind it, and with an ObjectTracker.push behind that.
  The M > 64 path (straight global atomics) is tested (tests/test_hip_tracker.py) and not timed here.

    python profiles/time_tracker.py --out profiles/r18_tracker_time.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from prior_flow_amd import det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd.object_tracks import ObjectTracker  # noqa: E402
from prior_flow_amd.parallax import parallax_map  # noqa: E402
from prior_flow_amd.segments import MovingObjects  # noqa: E402
from prior_flow_amd.video import FlowStream  # noqa: E402
from time_pose import captured, replay_us, scene_flow, spread  # noqa: E402
from time_segments import masks  # noqa: E402

SHIFT = (2, 1)                                                              # the second mask: the first rolled by (dx, dy) pixels


def smooth_flow(B, H, W, dev, sign):
    """sign * SHIFT plus a smooth field below 0.4 px: the nearest pixel stays the rolled one."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
    u = sign * SHIFT[0] + 0.3 * torch.sin(2 * math.pi * y / H + 0.7)
    v = sign * SHIFT[1] + 0.3 * torch.cos(2 * math.pi * x / W + 0.2)
    return torch.stack([u, v])[None].repeat(B, 1, 1, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--only", default="ab")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_tracker.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, H, W, M = 1, 512, 1024, 64
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "shape": [H, W], "B": B, "max_objects": M,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; *_ms: host clock around "
                   "whole sequences that end in a synchronise; lists: interleaved rounds; spread: max - min over the rounds of the same "
                   "run; the M > 64 path is not timed", "earlier_forms": {}}
    with torch.no_grad():
        if "a" in a.only:
            fwd, bwd = smooth_flow(B, H, W, dev, 1.0), smooth_flow(B, H, W, dev, -1.0)
            flow, R_true, t_true = scene_flow(H, W, dev)
            R, t = R_true.float()[None].contiguous(), t_true.float()[None].contiguous()
            maps = tuple(torch.empty(B, H, W, device=dev) for _ in range(3)) + (torch.empty(B, H, W, dtype=torch.uint8, device=dev),)
            graphs = {"map_us": captured(lambda: parallax_map(flow, R, t, out=maps))}
            info, keep = {}, []
            for k, m0 in masks(H, W, dev).items():
                m1 = torch.roll(m0, shifts=(SHIFT[1], SHIFT[0]), dims=(1, 2)).contiguous()
                mo = MovingObjects(B, H, W, dev, max_objects=M)
                tk = ObjectTracker(mo, grid="second")
                mo.update(m0)
                tk.link(fwd, bwd)
                mo.update(m1)
                tk.link(fwd, bwd)
                torch.cuda.synchronize()
                n = min(int(mo.count[0]), M)
                info[k] = {"objects": int(mo.count[0]), "continued": int((tk.age[0, :n] > 1).sum()), "new": int((tk.age[0, :n] == 1).sum()),
                           "nonzero_cells": int((tk.votes != 0).sum())}
                # the state the timed launches see: the first mask's objects as the previous frame (a replay of match or of the whole
                # push moves the state on to the second mask's own objects, static under a flow of SHIFT: the same work)
                lib, tb = mo.lib, mo._t
                keep.append((mo, tk, m1))
                graphs[f"{k}_begin_us"] = captured(lambda tk=tk: lib.trk_begin(tk.votes))
                graphs[f"{k}_vote1_us"] = captured(lambda mo=mo, tk=tk: lib.trk_vote(tk.prev_ids, mo.ids, fwd, None, None, None, mo.rows, tk.votes))
                graphs[f"{k}_vote2_us"] = captured(lambda mo=mo, tk=tk: lib.trk_vote(tk.prev_ids, mo.ids, fwd, bwd, None, None, mo.rows, tk.votes))
                graphs[f"{k}_match_us"] = captured(lambda mo=mo, tk=tk: lib.trk_match(
                    tk.votes, mo.count, mo.sums, tk.prev_count, tk.prev_sums, tk.prev_track, tk.prev_age, tk.prev_path, tk.next_id, tk.track,
                    tk.age, tk.origin, tk.fate, tk.step, tk.path, 2, tk.min_overlap))
                graphs[f"{k}_paint_us"] = captured(lambda mo=mo, tk=tk: lib.trk_paint(mo.ids, tk.track, tk.track_map, tk.prev_ids))
                graphs[f"{k}_push_us"] = captured(lambda tk=tk: tk.link(fwd, bwd))
                graphs[f"{k}_update_us"] = captured(lambda mo=mo, m1=m1: mo.update(m1))
                graphs[f"{k}_accumulate_us"] = captured(lambda mo=mo, tb=tb: lib.seg_objects(mo.labels, None, tb.rows, tb.cols, tb.scratch, mo.ids,
                                                                                             mo.keep, mo.roots, mo.count, mo.table, mo.sums, mo.min_area))
            e = {k_: [] for k_ in graphs}
            for _ in range(a.rounds):
                for k_, (g, _) in graphs.items():
                    e[k_].append(round(replay_us(g, a.replays), 2))
            e["median"] = {k_: statistics.median(e[k_]) for k_ in graphs}
            e["spread"] = {k_: spread(e[k_]) for k_ in graphs}
            md = e["median"]
            e["over_map"] = {k_: round(md[k_] / md["map_us"], 2) for k_ in graphs if k_ != "map_us"}
            e["masks"] = info
            print(json.dumps(e), flush=True)
            res["alone"] = e
            del graphs, keep
            torch.cuda.empty_cache()
        if "b" in a.only:
            from prior_flow_amd.prior_raft import PriOr_RAFT, state_dict_shapes
            model = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
            model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
            model = model.cuda().eval()
            f0, _ = synthetic_pair(B, H, W, seed=7)
            fr = [torch.roll(f0, shifts=(t_, 3 * t_), dims=(2, 3)).cuda().contiguous() for t_ in range(a.frames)]
            stream = FlowStream(model, iters=a.iters, warm_start=True, bidirectional=True, occlusion="plane")
            mo = MovingObjects(B, H, W, dev, max_objects=M, channels=2)
            tk = ObjectTracker(mo, grid="second")

            def update(r):
                mo.update(r.occ_backward, r.backward)

            def update_push(r):
                mo.update(r.occ_backward, r.backward)
                tk.push(r)

            def ms_per_frame(after):
                def seq():
                    for f in fr:
                        r = stream(f)
                        if r is not None:
                            after(r)
                seq()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seq()
                torch.cuda.synchronize()
                reps = max(2, int(a.window / (time.perf_counter() - t0)) + 1)
                t0 = time.perf_counter()
                for _ in range(reps):
                    seq()
                torch.cuda.synchronize()
                return 1000.0 * (time.perf_counter() - t0) / (reps * len(fr))

            b = {"B": B, "iters": a.iters, "occlusion": "plane", "step_update_ms": [], "step_update_push_ms": []}
            for _ in range(a.rounds):
                b["step_update_ms"].append(round(ms_per_frame(update), 4))
                b["step_update_push_ms"].append(round(ms_per_frame(update_push), 4))
            med = {k_: statistics.median(b[k_]) for k_ in ("step_update_ms", "step_update_push_ms")}
            b["median"] = {k_: round(v, 4) for k_, v in med.items()}
            b["push_behind_step_us"] = round(1000.0 * (med["step_update_push_ms"] - med["step_update_ms"]), 2)
            b["step_update_spread_us"] = round(1000.0 * spread(b["step_update_ms"]), 2)
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
