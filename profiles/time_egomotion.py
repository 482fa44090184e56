"""Camera rotation from 360-degree flow on the device: what RotationEstimator and Stabilizer cost, launch by launch, beside an
existing gather of the same size (FlowRenderer.warp) and an existing pass over the same flow (pf_fb_check), and behind a
bidirectional FlowStream step.  Interleaved rounds on one box, medians and the spread of the same run:

  (a) alone, one captured graph each, microseconds per replay between device events, 512x1024, B = 1, C = 3, on a flow that is a
      3 degree rotation with a block of independent motion (the case the defaults were chosen on):
        accumulate_plain_us     pf_ego_accumulate, weighted = 0
        accumulate_weighted_us  pf_ego_accumulate, weighted = 1
        solve_us                pf_ego_solve (one lane per image)
        estimate_us             RotationEstimator.estimate: the fill and the 2 * passes launches
        track_us                pf_ego_track
        rotate_f32_us           pf_erp_rotate, fp32 planes
        rotate_u8_us            pf_erp_rotate, bytes channel-last
        derotate_us             pf_ego_derotate
        push_us                 Stabilizer.push: estimate, track, rotate
        warp_us                 FlowRenderer.warp of one frame along one flow (a four-tap gather of the same size)
        fb_check_us             forward_backward_check of the flow pair (a pass over the same flow, both directions)
  (b) milliseconds per frame of the warm bidirectional FlowStream step (512x1024, iters 12, B = 1, occlusion "plane") alone and
      with one Stabilizer.push_bidirectional behind it on the same stream.

    python profiles/time_egomotion.py --out profiles/r11_egomotion_time.json
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

from prior_flow_amd import det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd.egomotion import RotationEstimator, Stabilizer, derotate_flow, rotate_erp  # noqa: E402
from prior_flow_amd.flow_viz import FlowRenderer  # noqa: E402
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


def rotation_flow(H, W, dev):
    """The flow of a 3 degree rotation about (1, 2, 3) in float64 on the device, a block of it moved by a further (6, -2) px."""
    k = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device=dev)
    k = k / k.norm()
    K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64, device=dev)
    a = math.radians(3.0)
    R = torch.eye(3, dtype=torch.float64, device=dev) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    n, m = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    th, ph = ((m + 0.5) / W - 0.5) * 2 * math.pi, (0.5 - (n + 0.5) / H) * math.pi
    d = torch.stack([ph.cos() * th.cos(), ph.cos() * th.sin(), ph.sin()], -1) @ R.T
    qm = (torch.atan2(d[..., 1], d[..., 0]) / (2 * math.pi) + 0.5) * W - 0.5
    qn = (0.5 - torch.asin(d[..., 2].clamp(-1, 1)) / math.pi) * H - 0.5
    f = torch.stack([torch.remainder(qm - m + W / 2, W) - W / 2, qn - n])
    f[0, H // 4:3 * H // 4, W // 8:W // 8 + int(0.6 * W)] += 6.0
    f[1, H // 4:3 * H // 4, W // 8:W // 8 + int(0.6 * W)] -= 2.0
    return f[None].float().contiguous(), R


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
    assert torch.cuda.is_available(), "time_egomotion.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, H, W, C = 1, 512, 1024, 3
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "shape": [H, W], "B": B, "C": C,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; *_ms: host clock around "
                   "whole sequences that end in a synchronise; lists: interleaved rounds; spread: max - min over the rounds of the same run"}
    with torch.no_grad():
        if "a" in a.only:
            fw, R_true = rotation_flow(H, W, dev)
            bw = -fw
            gen = torch.Generator(device=dev).manual_seed(3)
            f1 = torch.rand(B, C, H, W, device=dev, generator=gen) * 255
            f8 = (torch.rand(B, H, W, C, device=dev, generator=gen) * 255).to(torch.uint8)
            est = RotationEstimator(B, H, W, dev)
            stab = Stabilizer(B, C, H, W, dev, smoothing=0.9)
            rend = FlowRenderer(B, H, W, dev)
            rend.prepare_warp(C)
            lib = est.lib
            Rm = R_true.float()[None].contiguous()
            o32, o8, od = torch.empty_like(f1), torch.empty_like(f8), torch.empty_like(fw)
            est.estimate(fw)
            torch.cuda.synchronize()
            M = est.R[0].double() @ R_true.T                    # its angle from the skew part: acos of the trace loses half the digits
            sin = 0.5 * math.sqrt(float((M[2, 1] - M[1, 2]) ** 2 + (M[0, 2] - M[2, 0]) ** 2 + (M[1, 0] - M[0, 1]) ** 2))
            res["estimate_off_px"] = round(math.atan2(sin, float((M.trace() - 1) / 2)) * W / (2 * math.pi), 5)
            res["stats"] = [round(float(v), 6) for v in est.stats[0].tolist()]
            graphs = {
                "accumulate_plain_us": captured(lambda: lib.ego_accumulate(fw, None, Rm, est.sums, False, 1.0)),
                "accumulate_weighted_us": captured(lambda: lib.ego_accumulate(fw, None, Rm, est.sums, True, 1.0)),
                "solve_us": captured(lambda: lib.ego_solve(est.sums, None, est.R, est.stats, H, W, 1e-3)),
                "estimate_us": captured(lambda: est.estimate(fw)),
                "track_us": captured(lambda: lib.ego_track(Rm, stab.state, stab.orientation, stab.correction, 0.9)),
                "rotate_f32_us": captured(lambda: rotate_erp(f1, Rm, out=o32)),
                "rotate_u8_us": captured(lambda: rotate_erp(f8, Rm, out=o8)),
                "derotate_us": captured(lambda: derotate_flow(fw, Rm, out=od)),
                "push_us": captured(lambda: stab.push(f1, fw)),
                "warp_us": captured(lambda: rend.warp(f1, fw)),
                "fb_check_us": captured(lambda: forward_backward_check(fw, bw, metric="plane"))}
            e = {k: [] for k in graphs}
            for _ in range(a.rounds):
                for k, (g, _) in graphs.items():
                    est.sums.zero_()
                    stab.reset()
                    e[k].append(round(replay_us(g, a.replays), 2))
            e["median"] = {k: statistics.median(e[k]) for k in graphs}
            e["spread"] = {k: spread(e[k]) for k in graphs}
            e["rotate_over_warp"] = round(e["median"]["rotate_f32_us"] / e["median"]["warp_us"], 2)
            e["accumulate_over_fb_check"] = round(e["median"]["accumulate_weighted_us"] / e["median"]["fb_check_us"], 2)
            print(json.dumps(e), flush=True)
            res["alone"] = e
            del graphs
            torch.cuda.empty_cache()
        if "b" in a.only:
            from prior_flow_amd.prior_raft import PriOr_RAFT, state_dict_shapes
            model = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
            model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
            model = model.cuda().eval()
            f0, _ = synthetic_pair(B, H, W, seed=7)
            fr = [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda().contiguous() for t in range(a.frames)]
            stream = FlowStream(model, iters=a.iters, warm_start=True, bidirectional=True, occlusion="plane")
            stab = Stabilizer(B, C, H, W, dev, smoothing=0.9)

            def ms_per_frame(after):
                def seq():
                    for f in fr:
                        r = stream(f)
                        if r is not None:
                            after(r, f)
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

            b = {"B": B, "iters": a.iters, "occlusion": "plane", "step_ms": [], "step_push_ms": []}
            for _ in range(a.rounds):
                b["step_ms"].append(round(ms_per_frame(lambda r, f: None), 4))
                b["step_push_ms"].append(round(ms_per_frame(lambda r, f: stab.push_bidirectional(r, f)), 4))
            med = {k: statistics.median(b[k]) for k in ("step_ms", "step_push_ms")}
            b["median"] = {k: round(v, 4) for k, v in med.items()}
            b["push_behind_step_us"] = round(1000.0 * (med["step_push_ms"] - med["step_ms"]), 2)
            b["step_spread_us"] = round(1000.0 * spread(b["step_ms"]), 2)
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
