"""Flow rendering behind the video stream: what FlowRenderer.render / .warp cost alone and behind a warm FlowStream step, at
512x1024, iters=12, B = 1 and 8.  Per batch size, interleaved rounds on one box, medians:

  (a) render and warp alone: one captured graph each, replayed (5 and 3 launches), microseconds per replay;
  (b) milliseconds per frame of the warm stream step alone, the step + render, the step + render + warp (the stream replays its
      own graph; the renderer's launches follow it on the same stream, on the flow tensor the step returned);
  (c) for scale: the step + a device-to-host copy of the flow + a numpy port of the omni colour coding on the host.

The structural condition: (step + render) - step must not exceed render alone by more than the spread of the step between rounds.

    python profiles/time_flow_viz.py --out profiles/r9_flow_viz_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prior_flow_amd import det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd.flow_viz import FlowRenderer  # noqa: E402
from prior_flow_amd.prior_raft import PriOr_RAFT, state_dict_shapes  # noqa: E402
from prior_flow_amd.video import FlowStream  # noqa: E402


def frames(T, B, H, W):
    f0, _ = synthetic_pair(B, H, W, seed=7)
    return [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(T)]


def host_omni(flow):
    """numpy port of the omni colour coding (fp32 length, sort for the percentile, fp64 colour stage), one image [2,H,W]."""
    _, H, W = flow.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ex = np.mod(xx + flow[0] + 0.5, np.float32(W)) - 0.5
    ey = np.clip(yy + flow[1], -0.5, H - 0.5)
    th = lambda x: ((x + 0.5) / W - 0.5) * 2 * np.pi      # noqa: E731
    ph = lambda y: (0.5 - (y + 0.5) / H) * np.pi          # noqa: E731
    hv = np.sin((ph(ey) - ph(yy)) / 2) ** 2 + np.cos(ph(yy)) * np.cos(ph(ey)) * np.sin((th(ex) - th(xx)) / 2) ** 2
    sd = 2 * np.arcsin(np.sqrt(hv))
    clip = np.sort(sd, axis=None)[int(0.95 * sd.size)]
    rad = np.minimum(sd, clip) / (clip + 1e-5)
    seg = ((15, 0, 1, 1), (6, 1, 0, -1), (4, 1, 2, 1), (11, 2, 1, -1), (13, 2, 0, 1), (6, 0, 2, -1))
    wheel = []
    for n, full, ramp, sign in seg:
        for i in range(n):
            c = [0.0, 0.0, 0.0]
            c[full] = 255.0
            c[ramp] = np.floor(255.0 * i / n) if sign > 0 else 255.0 - np.floor(255.0 * i / n)
            wheel.append(c)
    wheel = np.array(wheel) / 255.0
    fk = (np.arctan2(-flow[1], -flow[0]) / np.pi + 1) / 2 * 54
    k0 = np.floor(fk).astype(np.int32)
    k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
    t = (fk - k0)[..., None]
    col = (1 - t) * wheel[k0] + t * wheel[k1]
    return np.floor(255 * (1 - rad[..., None] * (1 - col))).astype(np.uint8)


def replay_us(g, n):
    for _ in range(10):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def ms_per_frame(stream, fr, after, reps, window_s=0.0):
    """The warm stream over the sequence `reps` times (no reset: every timed call returns a flow), `after(flow, t)` behind it;
    more often where that is needed for a timed window of `window_s` seconds."""
    def seq():
        for t, f in enumerate(fr):
            flow = stream(f)
            if flow is not None:
                after(flow, t)
    seq()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seq()
    torch.cuda.synchronize()
    reps = max(reps, int(window_s / (time.perf_counter() - t0)) + 1)
    t0 = time.perf_counter()
    for _ in range(reps):
        seq()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / (reps * len(fr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.5, help="least length of a timed window of (b), seconds")
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    H, W = a.height, a.width
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
    model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
    model = model.cuda().eval()
    res = {"shape": [H, W], "iters": a.iters, "frames": a.frames, "reps": a.reps, "rounds": a.rounds, "window_s": a.window,
           "device": torch.cuda.get_device_name(0), "launches": {"render": 5, "warp": 3},
           "note": "alone_us: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; *_ms: ms per frame of the warm stream over whole sequences, host clock "
                   "around work that ends in a synchronise; lists: interleaved rounds; the medians are what DESIGN.md quotes",
           "runs": []}
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            fr = frames(a.frames, B, H, W)
            stream = FlowStream(model, iters=a.iters, warm_start=True)
            rend = FlowRenderer(B, H, W, "cuda")
            rend.prepare_warp(3)
            flow_in = torch.zeros(B, 2, H, W, device="cuda")
            im1, im2 = fr[0].clone(), fr[1].clone()
            for f in fr[:3]:
                got = stream(f)
            flow_in.copy_(got)
            rend.render(flow_in)
            rend.warp(im2, flow_in, image1=im1)
            torch.cuda.synchronize()
            g_r, g_w = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_r):
                rend.render(flow_in)
            with torch.cuda.graph(g_w):
                rend.warp(im2, flow_in, image1=im1)

            def with_render(flow, t):               # INTEGRATION.md's composition: launched behind the step on its stream
                rend.render(flow)

            def with_both(flow, t):
                rend.render(flow)
                rend.warp(fr[t], flow, image1=fr[t - 1])

            def with_host(flow, t):
                host_omni(flow[0].cpu().numpy())

            r = {"B": B}
            for _ in range(a.rounds):
                r.setdefault("render_alone_us", []).append(round(replay_us(g_r, 200), 2))
                r.setdefault("warp_alone_us", []).append(round(replay_us(g_w, 200), 2))
                r.setdefault("step_ms", []).append(round(ms_per_frame(stream, fr, lambda f, t: None, a.reps, a.window), 4))
                r.setdefault("step_render_ms", []).append(round(ms_per_frame(stream, fr, with_render, a.reps, a.window), 4))
                r.setdefault("step_render_warp_ms", []).append(round(ms_per_frame(stream, fr, with_both, a.reps, a.window), 4))
            r["step_host_colour_ms"] = [round(ms_per_frame(stream, fr[:6], with_host, 1), 3) for _ in range(2)]   # image 0 only
            med = {k: statistics.median(v) for k, v in r.items() if isinstance(v, list)}
            r["median"] = {k: round(v, 4) for k, v in med.items()}
            r["step_spread_pct"] = round(100.0 * (max(r["step_ms"]) - min(r["step_ms"])) / med["step_ms"], 3)
            r["render_behind_step_us"] = round(1000.0 * (med["step_render_ms"] - med["step_ms"]), 2)
            r["render_warp_behind_step_us"] = round(1000.0 * (med["step_render_warp_ms"] - med["step_ms"]), 2)
            r["structural_excess_us"] = round(r["render_behind_step_us"] - med["render_alone_us"], 2)
            r["step_spread_us"] = round(1000.0 * (max(r["step_ms"]) - min(r["step_ms"])), 2)
            r["structural_allowance_us"] = round(10.0 * med["step_ms"], 2)          # 1 % of the step
            r["structural_ok"] = bool(r["structural_excess_us"] <= r["structural_allowance_us"])
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
            del stream, rend, g_r, g_w, fr
            model._ws.clear()
            model._graphs.clear()
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
