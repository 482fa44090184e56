"""Camera translation from 360-degree flow on the device: what PoseEstimator and parallax_map cost, launch by launch, beside the
rotation estimate they start from (pf_ego_accumulate, RotationEstimator.estimate) and an existing pass over the same flow
(pf_fb_check), and behind a bidirectional FlowStream step.  Interleaved rounds on one box, medians and the
spread of the same run:

  (a) alone, one captured graph each, microseconds per replay between device events, 512x1024, B = 1, on the flow of a static
      scene (smooth depth 0.7..5.3, rotation 3 degrees about (1, 2, 3), |T| = 0.3 along (0.3, -0.2, 0.93)) with a block of 7.5 % of
      the pixels moved by a further (6, -2) px:
        accumulate_t_us         pf_epi_accumulate, mode PF_EPI_T, under the estimated R and t
        accumulate_t0_us        the same with t = NULL (the first pass)
        accumulate_r_us         pf_epi_accumulate, mode PF_EPI_R
        pass_t_us, pass_r_us    an accumulate and its pf_epi_solve (one lane per image) on live sums; solve_*_us is the difference
        map_us                  pf_epi_map, all four outputs
        estimate_us             PoseEstimator.estimate: the rotation estimate, the copy, the fill and the 18 launches
        ego_accumulate_us       pf_ego_accumulate, weighted = 1 (the pass every ratio is against)
        ego_estimate_us         RotationEstimator.estimate
        fb_check_us             forward_backward_check of the flow pair
  (b) milliseconds per frame of the warm bidirectional FlowStream step (512x1024, iters 12, B = 1, occlusion "plane") alone and
      with one PoseEstimator.estimate_bidirectional + parallax_map behind it on the same stream.

    python profiles/time_pose.py --out profiles/r12_pose_time.json
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

from prior_flow_amd import _lib, det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd.egomotion import RotationEstimator  # noqa: E402
from prior_flow_amd.parallax import PoseEstimator, parallax_map  # noqa: E402
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


def scene_flow(H, W, dev):
    """(flow fp32 [1,2,H,W], R_true, t_true): the exact projection of the static scene in float64 on the device, a block moved."""
    k = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device=dev)
    k = k / k.norm()
    K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64, device=dev)
    a = math.radians(3.0)
    R = torch.eye(3, dtype=torch.float64, device=dev) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    t = torch.tensor([0.3, -0.2, 0.93], dtype=torch.float64, device=dev)
    t = t / t.norm()
    n, m = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    th, ph = ((m + 0.5) / W - 0.5) * 2 * math.pi, (0.5 - (n + 0.5) / H) * math.pi
    rho = 3 + 1.5 * torch.sin(6 * math.pi * m / W) * torch.cos(2 * math.pi * n / H) + 0.8 * torch.cos(10 * math.pi * m / W + 1)
    p = torch.stack([ph.cos() * th.cos(), ph.cos() * th.sin(), ph.sin()], -1)
    d = (rho[..., None] * p) @ R.T + 0.3 * t
    d = d / d.norm(dim=-1, keepdim=True)
    qm = (torch.atan2(d[..., 1], d[..., 0]) / (2 * math.pi) + 0.5) * W - 0.5
    qn = (0.5 - torch.asin(d[..., 2].clamp(-1, 1)) / math.pi) * H - 0.5
    f = torch.stack([torch.remainder(qm - m + W / 2, W) - W / 2, qn - n])
    f[0, H // 4:H // 2, W // 8:W // 8 + int(0.3 * W)] += 6.0
    f[1, H // 4:H // 2, W // 8:W // 8 + int(0.3 * W)] -= 2.0
    return f[None].float().contiguous(), R, t


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
    assert torch.cuda.is_available(), "time_pose.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, H, W = 1, 512, 1024
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "shape": [H, W], "B": B,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; *_ms: host clock around "
                   "whole sequences that end in a synchronise; lists: interleaved rounds; spread: max - min over the rounds of the same run"}
    with torch.no_grad():
        if "a" in a.only:
            fw, R_true, t_true = scene_flow(H, W, dev)
            bw = -fw
            pose = PoseEstimator(B, H, W, dev)
            rot = RotationEstimator(B, H, W, dev)
            lib = pose.lib
            pose.estimate(fw)
            torch.cuda.synchronize()
            cross = torch.linalg.cross(pose.t[0].double(), t_true)
            res["t_off_px"] = round(math.atan2(float(cross.norm()), float(pose.t[0].double() @ t_true)) * W / (2 * math.pi), 5)
            M = pose.R[0].double() @ R_true.T
            sin = 0.5 * math.sqrt(float((M[2, 1] - M[1, 2]) ** 2 + (M[0, 2] - M[2, 0]) ** 2 + (M[1, 0] - M[0, 1]) ** 2))
            res["R_off_px"] = round(math.atan2(sin, float((M.trace() - 1) / 2)) * W / (2 * math.pi), 5)
            res["stats"] = [round(float(v), 6) for v in pose.stats[0].tolist()]
            Rm, tm = pose.R.clone(), pose.t.clone()
            R2, t2, st2 = pose.R.clone(), pose.t.clone(), pose.stats.clone()
            sums = torch.zeros_like(pose.sums)
            outs = tuple(torch.empty(B, H, W, device=dev) for _ in range(3)) + (torch.empty(B, H, W, dtype=torch.uint8, device=dev),)
            graphs = {
                "accumulate_t_us": captured(lambda: lib.epi_accumulate(fw, None, Rm, tm, sums, _lib.EPI_T, 1.0, 0.25)),
                "accumulate_t0_us": captured(lambda: lib.epi_accumulate(fw, None, Rm, None, sums, _lib.EPI_T, 1.0, 0.25)),
                "accumulate_r_us": captured(lambda: lib.epi_accumulate(fw, None, Rm, tm, sums, _lib.EPI_R, 1.0, 0.25)),
                "pass_t_us": captured(lambda: (lib.epi_accumulate(fw, None, R2, t2, sums, _lib.EPI_T, 1.0, 0.25),
                                               lib.epi_solve(sums, None, R2, t2, st2, H, W, _lib.EPI_T, 1e-3, 0.05))),
                "pass_r_us": captured(lambda: (lib.epi_accumulate(fw, None, R2, t2, sums, _lib.EPI_R, 1.0, 0.25),
                                               lib.epi_solve(sums, None, R2, t2, st2, H, W, _lib.EPI_R, 1e-3, 0.05))),
                "map_us": captured(lambda: parallax_map(fw, Rm, tm, out=outs)),
                "estimate_us": captured(lambda: pose.estimate(fw)),
                "ego_accumulate_us": captured(lambda: lib.ego_accumulate(fw, None, Rm, rot.sums, True, 1.0)),
                "ego_estimate_us": captured(lambda: rot.estimate(fw)),
                "fb_check_us": captured(lambda: forward_backward_check(fw, bw, metric="plane"))}
            e = {k: [] for k in graphs}
            for _ in range(a.rounds):
                for k, (g, _) in graphs.items():
                    sums.zero_()
                    rot.sums.zero_()
                    e[k].append(round(replay_us(g, a.replays), 2))
            e["median"] = {k: statistics.median(e[k]) for k in graphs}
            e["spread"] = {k: spread(e[k]) for k in graphs}
            for k in ("accumulate_t_us", "accumulate_t0_us", "accumulate_r_us"):
                e[k.replace("_us", "_over_ego_accumulate")] = round(e["median"][k] / e["median"]["ego_accumulate_us"], 2)
            e["solve_t_us"] = round(e["median"]["pass_t_us"] - e["median"]["accumulate_t_us"], 2)
            e["solve_r_us"] = round(e["median"]["pass_r_us"] - e["median"]["accumulate_r_us"], 2)
            e["estimate_over_ego_estimate"] = round(e["median"]["estimate_us"] / e["median"]["ego_estimate_us"], 2)
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
            pose = PoseEstimator(B, H, W, dev)
            outs = tuple(torch.empty(B, H, W, device=dev) for _ in range(3)) + (torch.empty(B, H, W, dtype=torch.uint8, device=dev),)

            def after_pose(r, f):
                R, t = pose.estimate_bidirectional(r)
                parallax_map(r.forward, R, t, mask=r.occ_forward, out=outs)

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

            b = {"B": B, "iters": a.iters, "occlusion": "plane", "step_ms": [], "step_pose_ms": []}
            for _ in range(a.rounds):
                b["step_ms"].append(round(ms_per_frame(lambda r, f: None), 4))
                b["step_pose_ms"].append(round(ms_per_frame(after_pose), 4))
            med = {k: statistics.median(b[k]) for k in ("step_ms", "step_pose_ms")}
            b["median"] = {k: round(v, 4) for k, v in med.items()}
            b["pose_behind_step_us"] = round(1000.0 * (med["step_pose_ms"] - med["step_ms"]), 2)
            b["step_spread_us"] = round(1000.0 * spread(b["step_ms"]), 2)
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
