"""Push-pull hole filling on the device: what a fill costs at 512x1024, B = 1, C = 1 and 3, on three hole maps (discs covering 5 %,
Bernoulli 0.5, one band across the seam), beside pf_epi_map and pf_splat_resolve (one pass over the same pixels each) and behind a
warm bidirectional FlowStream step with FrameInterpolator.from_bidirectional.  Interleaved rounds on one box,
medians and the spread of the same run:

  (a) alone, one captured graph each, microseconds per replay between device events, per C and hole map:
        fused_us       HoleFiller.fill (pf_fill_pushpull: three launches)
        pull_us, apex_us, push_us   its three launches alone (pf_fill_stage on the scratch a whole call left)
        levels_us      HoleFiller.fill_levels (the level-by-level entry points: 2 L + 2 = 22 launches): what the fusion is held to
      and once: map_us (pf_epi_map, all four outputs), resolve_us (pf_splat_resolve, C = 3, two jobs, on all-zero sums)
  (b) milliseconds per frame of the warm bidirectional FlowStream step (512x1024, iters 12, B = 1, occlusion "plane") with
      FrameInterpolator.from_bidirectional behind it, fill "none" and fill "pushpull".

    python profiles/time_fill.py --out profiles/r19_fill_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from prior_flow_amd import det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd.inpaint import HoleFiller  # noqa: E402
from prior_flow_amd.interp import FrameInterpolator  # noqa: E402
from prior_flow_amd.parallax import parallax_map  # noqa: E402
from prior_flow_amd.video import FlowStream  # noqa: E402
from time_pose import captured, replay_us, scene_flow, spread  # noqa: E402


def hole_maps(H, W, dev):
    """uint8 [1,H,W]: discs of radius 12 covering about 5 %, Bernoulli 0.5, a band of rows H/4..3H/4 across the seam (W/16 columns
    on either side)."""
    g = torch.Generator().manual_seed(11)
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    discs = torch.zeros(H, W, dtype=torch.bool)
    n = int(0.05 * H * W / (3.1416 * 12 * 12) * 1.1)
    for cy, cx in zip(torch.randint(0, H, (n,), generator=g).tolist(), torch.randint(0, W, (n,), generator=g).tolist()):
        dx = torch.remainder(x - cx + W // 2, W) - W // 2
        discs |= (y - cy) ** 2 + dx ** 2 <= 144
    bern = torch.rand(H, W, generator=g) < 0.5
    band = (y >= H // 4) & (y < 3 * H // 4) & ((x < W // 16) | (x >= W - W // 16))
    return {k: m.to(torch.uint8)[None].contiguous().to(dev) for k, m in (("discs", discs), ("bernoulli", bern), ("seam_band", band))}


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
    assert torch.cuda.is_available(), "time_fill.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, H, W = 1, 512, 1024
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "shape": [H, W], "B": B,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; *_ms: host clock around "
                   "whole sequences that end in a synchronise; lists: interleaved rounds; spread: max - min over the rounds of the same run"}
    with torch.no_grad():
        if "a" in a.only:
            holes = hole_maps(H, W, dev)
            flow, R_true, t_true = scene_flow(H, W, dev)
            R, t = R_true.float()[None].contiguous(), t_true.float()[None].contiguous()
            maps = tuple(torch.empty(B, H, W, device=dev) for _ in range(3)) + (torch.empty(B, H, W, dtype=torch.uint8, device=dev),)
            graphs = {"map_us": captured(lambda: parallax_map(flow, R, t, out=maps))}
            fi = FrameInterpolator(B, 3, H, W, dev)
            frame = (torch.rand(B, 3, H, W, device=dev) * 255).contiguous()
            graphs["resolve_us"] = captured(lambda: fi.lib.splat_resolve(fi.acc, fi.out, fi.hole, 2, fi.vmax, fi.cmin, frame, frame, 0.5))
            keep, info = [], {}
            for C in (1, 3):
                src = (torch.rand(B, C, H, W, device=dev) * 255).contiguous()
                for k, hole in holes.items():
                    f = HoleFiller(B, C, H, W, dev)
                    f.fill(src, hole)
                    keep.append((f, src))
                    info[k] = round(float((hole != 0).float().mean()), 4)
                    tag = f"c{C}_{k}"
                    graphs[f"{tag}_fused_us"] = captured(lambda f=f, src=src, hole=hole: f.fill(src, hole))
                    for s, name in enumerate(("pull", "apex", "push")):
                        graphs[f"{tag}_{name}_us"] = captured(
                            lambda f=f, src=src, hole=hole, s=s: f.lib.fill_pushpull(src, hole, None, f.out, f.empty, f.scratch, stage=s))
                    graphs[f"{tag}_levels_us"] = captured(lambda f=f, src=src, hole=hole: f.fill_levels(src, hole))
            e = {k_: [] for k_ in graphs}
            for _ in range(a.rounds):
                for k_, (g, _) in graphs.items():
                    e[k_].append(round(replay_us(g, a.replays), 2))
            e["median"] = {k_: statistics.median(e[k_]) for k_ in graphs}
            e["spread"] = {k_: spread(e[k_]) for k_ in graphs}
            md, sp = e["median"], e["spread"]
            e["fused_faster_by_us"] = {k_[:-9]: round(md[k_[:-9] + "_levels_us"] - md[k_], 2) for k_ in graphs if k_.endswith("_fused_us")}
            e["fused_faster_than_levels_beyond_spread"] = all(
                md[t_ + "_levels_us"] - md[t_ + "_fused_us"] > sp[t_ + "_levels_us"] + sp[t_ + "_fused_us"] for t_ in e["fused_faster_by_us"])
            e["hole_share"] = info
            e["levels"], e["launches_fused"], e["launches_levels"] = keep[0][0].L, 3, 2 * keep[0][0].L + 2
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
            interp = {k: FrameInterpolator(B, 3, H, W, dev, fill=k) for k in ("none", "pushpull")}

            def ms_per_frame(fi_):
                def seq():
                    prev = fr[-1]                                     # the stream carries on from the sequence before
                    for f in fr:
                        r = stream(f)
                        if r is not None:
                            fi_.from_bidirectional(r, prev, f, 0.5)
                        prev = f
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

            b = {"B": B, "iters": a.iters, "occlusion": "plane", "step_interp_none_ms": [], "step_interp_pushpull_ms": []}
            for _ in range(a.rounds):
                b["step_interp_none_ms"].append(round(ms_per_frame(interp["none"]), 4))
                b["step_interp_pushpull_ms"].append(round(ms_per_frame(interp["pushpull"]), 4))
            med = {k_: statistics.median(b[k_]) for k_ in ("step_interp_none_ms", "step_interp_pushpull_ms")}
            b["median"] = {k_: round(v, 4) for k_, v in med.items()}
            b["fill_behind_step_us"] = round(1000.0 * (med["step_interp_pushpull_ms"] - med["step_interp_none_ms"]), 2)
            b["step_spread_us"] = round(1000.0 * spread(b["step_interp_none_ms"]), 2)
            b["hole_share_last_frame"] = round(float((interp["pushpull"].hole != 0).float().mean()), 4)
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
