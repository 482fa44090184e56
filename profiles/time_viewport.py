"""Perspective viewports and cube maps on the device: what ViewRenderer.image / .flow cost alone, beside the bytes they must
move and beside torch ops, and behind a FlowStream step.  Interleaved rounds on one box, medians:

  (a) alone, one captured graph each (one launch), microseconds per replay between device events:
      six 256x256 cube faces and one 512x512 view (fov 100) from a 512x1024 frame, B = 1 and 8; one 1024x1024 view from
      1920x3840, B = 1; the image form (3 channels, fp32) and the flow form of each.  Beside each:
        floor_us   the bytes the launch must move at 8 TB/s: its output plus the input pixels its taps touch (counted);
        torch_us   the same views with torch ops on the device, what a user would write today: the sample grid built with
                   torch (rays, atan2, asin), the seam handled by padding one column on either side, F.grid_sample; and
                   torch_cached_us with the grid built once.  For the flow the torch figure is the naive resampling of u and v
                   with that grid -- cheaper than anything correct, and wrong at the seam and in its meaning;
  (b) milliseconds per frame of the warm FlowStream step (512x1024, iters 12, B = 1) alone and with flow + image of the six
      faces behind it on the same stream.  The step is the parent commit's code, measured in the same process.

The structural condition: (step + views) - step exceeds the two calls' alone-time by no more than the step's own spread.

    python profiles/time_viewport.py --out profiles/r10_viewport_time.json
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

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from prior_flow_amd import det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd.projection import ViewRenderer, Viewport, cube_faces  # noqa: E402


def torch_grid(views, Rs, H, W, dev):
    """(m, n) [V,h,w] of the views' rays with torch ops (fp32); Rs: the views' rotations, already on the device."""
    out = []
    for v, R in zip(views, Rs):
        i, j = torch.meshgrid(torch.arange(v.h, device=dev, dtype=torch.float32), torch.arange(v.w, device=dev, dtype=torch.float32), indexing="ij")
        cam = torch.stack([torch.ones_like(i), (j - (v.w - 1) / 2) / v.f, -(i - (v.h - 1) / 2) / v.f], -1)
        d = cam @ R.T
        theta = torch.atan2(d[..., 1], d[..., 0])
        phi = torch.asin(d[..., 2] / d.norm(dim=-1))
        out.append(torch.stack([(theta / (2 * math.pi) + 0.5) * W - 0.5, (0.5 - phi / math.pi) * H - 0.5], -1))
    return torch.stack(out)


def torch_sample(x, mn):
    """x [B,C,H,W] at (m, n) [V,h,w,2]: wrap in x by one padded column on either side, clamp in y by border padding."""
    B, C, H, W = x.shape
    V, h, w, _ = mn.shape
    xp = torch.cat([x[..., -1:], x, x[..., :1]], -1)
    g = torch.stack([(mn[..., 0] + 1) * 2 / (W + 1) - 1, mn[..., 1] * 2 / (H - 1) - 1], -1).view(1, V * h, w, 2).expand(B, -1, -1, -1)
    return F.grid_sample(xp, g, mode="bilinear", padding_mode="border", align_corners=True).view(B, C, V, h, w).transpose(1, 2)


def touched_pixels(mn, H, W):
    m, n = torch.remainder(mn[..., 0], W).floor().long(), mn[..., 1].floor().long()
    idx = []
    for dy in (0, 1):
        for dx in (0, 1):
            idx.append((n + dy).clamp(0, H - 1) * W + (m + dx) % W)
    return int(torch.unique(torch.cat([t.reshape(-1) for t in idx])).numel())


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--only", default="ab")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "hbm_tb_per_s": 8.0,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; floor_us: output bytes plus "
                   "touched input bytes at 8 TB/s; *_ms: host clock around whole sequences that end in a synchronise; lists: interleaved rounds"}
    with torch.no_grad():
        if "a" in a.only:
            cases = []
            for name, H, W, views, Bs in (("cube 6 x 256x256", 512, 1024, cube_faces(256), (1, 8)),
                                          ("view 512x512 fov 100", 512, 1024, [Viewport(0.7, -0.4, 0.3, 100.0, 512, 512)], (1, 8)),
                                          ("view 1024x1024 fov 100", 1920, 3840, [Viewport(0.7, -0.4, 0.3, 100.0, 1024, 1024)], (1,))):
                Rs = [torch.tensor(v.R, dtype=torch.float32, device=dev) for v in views]
                mn = torch_grid(views, Rs, H, W, dev)
                touched = touched_pixels(mn, H, W)
                V, h, w = len(views), views[0].h, views[0].w
                for B in Bs:
                    r = ViewRenderer(B, H, W, views, dev)
                    r.prepare(3)
                    x = torch.rand(B, 3, H, W, device=dev) * 255
                    flow = torch.randn(B, 2, H, W, device=dev) * 10
                    e = {"case": name, "shape": [H, W], "B": B, "V": V, "view": [h, w], "touched_input_pixels": touched,
                         "image_floor_us": round((B * V * 3 * h * w * 4 + B * touched * 3 * 4) / 8e12 * 1e6, 2),
                         "flow_floor_us": round((B * V * h * w * 9 + B * touched * 8) / 8e12 * 1e6, 2), "keep": (r, x, flow, mn, Rs)}
                    e["graphs"] = {"image_us": captured(lambda: r.image(x)), "flow_us": captured(lambda: r.flow(flow)),
                                   "torch_image_us": captured(lambda: torch_sample(x, torch_grid(views, Rs, H, W, dev))),
                                   "torch_image_cached_us": captured(lambda: torch_sample(x, mn)),
                                   "torch_naive_flow_cached_us": captured(lambda: torch_sample(flow, mn))}
                    for k in e["graphs"]:
                        e[k] = []
                    cases.append(e)
            for _ in range(a.rounds):
                for e in cases:
                    for k, (g, _) in e["graphs"].items():
                        e[k].append(round(replay_us(g, a.replays), 2))
            for e in cases:
                names = list(e["graphs"])
                del e["graphs"], e["keep"]
                e["median"] = {k: statistics.median(e[k]) for k in names}
                print(json.dumps(e), flush=True)
            res["alone"] = cases
            torch.cuda.empty_cache()
        if "b" in a.only:
            from prior_flow_amd.prior_raft import PriOr_RAFT, state_dict_shapes
            from prior_flow_amd.video import FlowStream
            B, H, W = 1, 512, 1024
            model = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
            model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
            model = model.cuda().eval()
            f0, _ = synthetic_pair(B, H, W, seed=7)
            fr = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(a.frames)]
            stream = FlowStream(model, iters=a.iters, warm_start=True)
            r = ViewRenderer(B, H, W, cube_faces(256), dev)
            r.prepare(3)
            flow_in = torch.zeros(B, 2, H, W, device=dev)
            g_f, _k1 = captured(lambda: r.flow(flow_in))
            g_i, _k2 = captured(lambda: r.image(fr[0]))

            def views(flow, t):
                r.flow(flow)
                r.image(fr[t])

            def ms_per_frame(after):
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
                reps = max(2, int(a.window / (time.perf_counter() - t0)) + 1)
                t0 = time.perf_counter()
                for _ in range(reps):
                    seq()
                torch.cuda.synchronize()
                return 1000.0 * (time.perf_counter() - t0) / (reps * len(fr))

            b = {"shape": [H, W], "B": B, "iters": a.iters, "views": "cube 6 x 256x256", "flow_alone_us": [], "image_alone_us": [],
                 "step_ms": [], "step_views_ms": []}
            for _ in range(a.rounds):
                b["flow_alone_us"].append(round(replay_us(g_f, a.replays), 2))
                b["image_alone_us"].append(round(replay_us(g_i, a.replays), 2))
                b["step_ms"].append(round(ms_per_frame(lambda f, t: None), 4))
                b["step_views_ms"].append(round(ms_per_frame(views), 4))
            med = {k: statistics.median(v) for k, v in b.items() if isinstance(v, list) and k != "shape"}
            b["median"] = {k: round(v, 4) for k, v in med.items()}
            b["views_behind_step_us"] = round(1000.0 * (med["step_views_ms"] - med["step_ms"]), 2)
            b["alone_us"] = round(med["flow_alone_us"] + med["image_alone_us"], 2)
            b["step_spread_us"] = round(1000.0 * (max(b["step_ms"]) - min(b["step_ms"])), 2)
            b["structural_excess_us"] = round(b["views_behind_step_us"] - b["alone_us"], 2)
            b["structural_ok"] = bool(b["structural_excess_us"] <= b["step_spread_us"])
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
