"""Forward softmax splatting on the device: what FrameInterpolator costs alone, launch by launch, beside the existing gather of
comparable bytes (FlowRenderer.warp), and behind a bidirectional FlowStream step.  Interleaved rounds on
one box, medians and the spread of the same run:

  (a) alone, one captured graph each, microseconds per replay between device events, 512x1024, C = 3, B = 1 and 8, on the
      smooth and the random flow pair of profiles/time_chain.py (a pan plus a tilt with 0.05 px of noise: a wave's taps are one
      contiguous run per plane; 6 px of white noise: every tap its own line), two jobs with the forward-backward residuals as
      the metric:
        accumulate_us  pf_splat_accumulate alone (the sums keep growing from replay to replay and wrap; integer adds cost the same)
        resolve_us     pf_splat_resolve alone (with the blend fill)
        frame_us       FrameInterpolator.frame: the two launches
        warp_us        FlowRenderer.warp of one frame along one flow (four taps gathered per pixel and channel)
      with, per case, the bytes the atomics add (2 jobs x 4 taps x (C + 2) sums x 8 bytes per pixel), that figure at the 1.3
      TB/s measured for FLOAT atomics of this shape, and the byte floor of both launches at 8 TB/s.
  (b) milliseconds per frame of the warm bidirectional FlowStream step (512x1024, iters 12, B = 1, occlusion "plane") alone and
      with one from_bidirectional call behind it on the same stream.

    python profiles/time_interp.py --out profiles/r10_interp_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from prior_flow_amd import det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd.flow_viz import FlowRenderer  # noqa: E402
from prior_flow_amd.interp import FrameInterpolator  # noqa: E402
from prior_flow_amd.video import FlowStream, forward_backward_check  # noqa: E402


def replay_us(g, n):
    for _ in range(5):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def captured(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def spread(v):
    return round(max(v) - min(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--only", default="ab")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_interp.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    H, W, C = 512, 1024, 3
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "hbm_tb_per_s": 8.0,
           "float_atomic_tb_per_s": 1.3, "shape": [H, W], "C": C,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; atomic_bytes: 2 jobs "
                   "x 4 taps x (C + 2) sums x 8 bytes per pixel; at_float_rate_us: those bytes at 1.3 TB/s; floor_us: the bytes "
                   "both launches must move at 8 TB/s (accumulate: per job C values, 2 flow and 2 metric floats read, resolve: (C + 2) sums read and "
                   "written, C floats and a byte written, 2C floats of fill read); *_ms: host clock around whole sequences that "
                   "end in a synchronise; lists: interleaved rounds; spread: max - min over the rounds of the same run"}
    with torch.no_grad():
        if "a" in a.only:
            cases = []
            yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
            smooth = torch.stack([6.0 * torch.sin(2 * torch.pi * xx / W + 0.3) + 2.0, 3.0 * torch.cos(torch.pi * yy / H)])
            for B, data in ((1, "smooth"), (1, "random"), (8, "smooth"), (8, "random")):
                gen = torch.Generator(device=dev).manual_seed(3 + B)
                if data == "smooth":
                    fw = smooth[None] + torch.randn(B, 2, H, W, device=dev, generator=gen) * 0.05
                else:
                    fw = torch.randn(B, 2, H, W, device=dev, generator=gen) * 6
                bw = -fw + torch.randn(B, 2, H, W, device=dev, generator=gen) * 0.3
                _, _, res_fw, res_bw = forward_backward_check(fw, bw, metric="plane")
                f0 = torch.rand(B, C, H, W, device=dev, generator=gen) * 255
                f1 = torch.rand(B, C, H, W, device=dev, generator=gen) * 255
                fi = FrameInterpolator(B, C, H, W, dev)
                rend = FlowRenderer(B, H, W, dev)
                rend.prepare_warp(C)
                px = B * H * W
                atomic_bytes = 2 * 4 * (C + 2) * 8 * px
                floor = (2 * (C + 2 + 2) * 4 + 2 * (C + 2) * 8 + C * 4 + 1 + 2 * C * 4) * px
                e = {"B": B, "data": data, "atomic_bytes": atomic_bytes, "at_float_rate_us": round(atomic_bytes / 1.3e12 * 1e6, 2),
                     "floor_us": round(floor / 8e12 * 1e6, 2), "keep": (fw, bw, res_fw, res_bw, f0, f1, fi, rend)}
                lib = fi.lib
                jobs = [(f0, fw, res_fw, None, 0.5, 0.5), (f1, bw, res_bw, None, 0.5, 0.5)]
                e["graphs"] = {
                    "accumulate_us": captured(lambda: lib.splat_accumulate(jobs, fi.acc, fi.alpha, fi.zmax, fi.vmax)),
                    "resolve_us": captured(lambda: lib.splat_resolve(fi.acc, fi.out, fi.hole, 2, fi.vmax, fi.cmin, f0, f1, 0.5)),
                    "frame_us": captured(lambda: fi.frame(f0, f1, fw, bw, 0.5, res_fw, res_bw)),
                    "warp_us": captured(lambda: rend.warp(f1, fw))}
                for k in e["graphs"]:
                    e[k] = []
                cases.append(e)
            for _ in range(a.rounds):
                for e in cases:
                    for k, (g, _) in e["graphs"].items():
                        e["keep"][6].reset()               # every graph starts from all-zero sums
                        e[k].append(round(replay_us(g, a.replays), 2))
            for e in cases:
                names = list(e["graphs"])
                e["keep"][6].reset()
                del e["graphs"], e["keep"]
                e["median"] = {k: statistics.median(e[k]) for k in names}
                e["spread"] = {k: spread(e[k]) for k in names}
                e["accumulate_over_float_rate"] = round(e["median"]["accumulate_us"] / e["at_float_rate_us"], 3)
                e["frame_over_floor"] = round(e["median"]["frame_us"] / e["floor_us"], 2)
                e["frame_over_warp"] = round(e["median"]["frame_us"] / e["median"]["warp_us"], 2)
                print(json.dumps(e), flush=True)
            res["alone"] = cases
            torch.cuda.empty_cache()
        if "b" in a.only:
            from prior_flow_amd.prior_raft import PriOr_RAFT, state_dict_shapes
            B = 1
            model = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
            model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
            model = model.cuda().eval()
            f0, _ = synthetic_pair(B, H, W, seed=7)
            fr = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(a.frames)]
            stream = FlowStream(model, iters=a.iters, warm_start=True, bidirectional=True, occlusion="plane")
            fi = FrameInterpolator(B, C, H, W, dev)

            def ms_per_frame(after):
                def seq():
                    prev = fr[-1]                      # the stream keeps its last frame from one sequence to the next
                    for f in fr:
                        r = stream(f)
                        if r is not None:
                            after(r, prev, f)
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

            b = {"B": B, "iters": a.iters, "occlusion": "plane", "step_ms": [], "step_interp_ms": []}
            for _ in range(a.rounds):
                b["step_ms"].append(round(ms_per_frame(lambda r, p, f: None), 4))
                b["step_interp_ms"].append(round(ms_per_frame(lambda r, p, f: fi.from_bidirectional(r, p, f, 0.5)), 4))
            med = {k: statistics.median(b[k]) for k in ("step_ms", "step_interp_ms")}
            b["median"] = {k: round(v, 4) for k, v in med.items()}
            b["interp_behind_step_us"] = round(1000.0 * (med["step_interp_ms"] - med["step_ms"]), 2)
            b["step_spread_us"] = round(1000.0 * spread(b["step_ms"]), 2)
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
