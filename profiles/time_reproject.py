"""Depth along the trajectory on the device: what the projection, the three launches of the z-tested splat, the update, a whole
Reprojector.run and a whole DepthPropagator.push cost, launch by launch, beside the launches of sections 18 and 20 they are shaped
after, and behind a bidirectional FlowStream step.  Interleaved rounds on one box, medians and the spread
of the same run:

  (a) alone, one captured graph each, microseconds per replay between device events, 512x1024, B = 1:
        project_us                   pf_reproj_project (the depth of a static scene under a 3 degree turn and a baseline of 0.3)
        front_us                     pf_zsplat_front on that projection
        accumulate_us, _c3_us        pf_zsplat_accumulate with C = 0 and C = 3 payload planes (3 and 6 sums per tap)
        resolve_us, _c3_us           pf_zsplat_resolve with C = 0 and C = 3, on the sums of one accumulate (splat_us / splat_c3_us are
                                     front + accumulate + resolve in one graph, so the resolve sees live sums)
        update_us                    pf_depth_update (the pixel pass and the one-thread-per-image step)
        splat_accumulate_c1_us       pf_splat_accumulate, one job, C = 1 (3 sums per tap): the yardstick of front and accumulate
        splat_resolve_c1_us          pf_splat_resolve, C = 1: the yardstick of resolve
        map_us                       pf_epi_map, all four outputs: the yardstick of project and update
        run_us, run_c3_us            Reprojector.run with C = 0 and C = 3
        push_us                      DepthPropagator.push (two copies, the update, T, project, front, accumulate, resolve)
  (b) milliseconds per frame of the warm bidirectional FlowStream step (512x1024, iters 12, B = 1, occlusion "plane") with
      Odometry.push behind it, and with DepthPropagator.push behind that, on the same stream.

    python profiles/time_reproject.py --out profiles/r15_reproject_time.json
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
from prior_flow_amd.odometry import Odometry  # noqa: E402
from prior_flow_amd.parallax import parallax_map  # noqa: E402
from prior_flow_amd.reproject import DepthPropagator, Reprojector  # noqa: E402
from prior_flow_amd.video import FlowStream  # noqa: E402
from time_pose import captured, replay_us, scene_flow, spread  # noqa: E402


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
    assert torch.cuda.is_available(), "time_reproject.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, H, W = 1, 512, 1024
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "shape": [H, W], "B": B,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; *_ms: host clock around "
                   "whole sequences that end in a synchronise; lists: interleaved rounds; spread: max - min over the rounds of the same run"}
    with torch.no_grad():
        if "a" in a.only:
            fw, R_true, t_true = scene_flow(H, W, dev)
            R = R_true.float()[None].contiguous()
            t = t_true.float()[None].contiguous()
            T = (0.3 * t).contiguous()
            n, m = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
            rho = 3 + 1.5 * torch.sin(6 * torch.pi * m / W) * torch.cos(2 * torch.pi * n / H) + 0.8 * torch.cos(10 * torch.pi * m / W + 1)
            inv = (1.0 / rho).float()[None].contiguous()
            wgt = torch.ones_like(inv)
            frame = (torch.rand(B, 3, H, W, device=dev) * 255).contiguous()
            rp0, rp3 = Reprojector(B, 0, H, W, dev), Reprojector(B, 3, H, W, dev)
            lib, o = rp0.lib, rp0.o
            rp0.run(None, inv, wgt, R, T)
            rp3.run(frame, inv, wgt, R, T)
            # the yardsticks' buffers
            acc1 = torch.zeros(B, 3, H, W, dtype=torch.int64, device=dev)
            out1, hole1 = torch.empty(B, 1, H, W, device=dev), torch.empty(B, H, W, dtype=torch.uint8, device=dev)
            src1 = inv[:, None].contiguous()
            maps = tuple(torch.empty(B, H, W, device=dev) for _ in range(3)) + (torch.empty(B, H, W, dtype=torch.uint8, device=dev),)
            ds, ws = inv.clone(), wgt.clone()
            dis = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
            flags = torch.tensor([[1, 1, 1, 1]], dtype=torch.int32, device=dev)
            seg = torch.ones(B, dtype=torch.int32, device=dev)
            odo = Odometry(B, H, W, dev)
            odo.push_flows(fw, -fw)
            odo.push_flows(fw, -fw)
            prop = DepthPropagator(odo)
            prop.push()

            def splat(rp, src):
                return lambda: rp.splat(src, wgt)

            graphs = {
                "project_us": captured(lambda: lib.reproj_project(inv, wgt, None, R, T, rp0.flow, rp0.d_new, rp0.valid, o["n_min"])),
                "front_us": captured(lambda: lib.zsplat_front(None, rp0.flow, rp0.d_new, wgt, rp0.valid, rp0.front, o["b_min"])),
                "accumulate_us": captured(lambda: lib.zsplat_accumulate(None, rp0.flow, rp0.d_new, wgt, rp0.valid, rp0.front, rp0.acc, o["b_min"],
                                                                        o["ztol_log2"], o["w_max"], o["dmax"], o["vmax"])),
                "accumulate_c3_us": captured(lambda: lib.zsplat_accumulate(frame, rp3.flow, rp3.d_new, wgt, rp3.valid, rp3.front, rp3.acc,
                                                                           o["b_min"], o["ztol_log2"], o["w_max"], o["dmax"], o["vmax"])),
                "resolve_us": captured(lambda: lib.zsplat_resolve(rp0.acc, rp0.front, None, rp0.inv_depth, rp0.weight, rp0.hole, o["cmin"],
                                                                  o["w_max"], o["dmax"], o["vmax"])),
                "resolve_c3_us": captured(lambda: lib.zsplat_resolve(rp3.acc, rp3.front, rp3.out, rp3.inv_depth, rp3.weight, rp3.hole, o["cmin"],
                                                                     o["w_max"], o["dmax"], o["vmax"])),
                "splat_us": captured(splat(rp0, None)),
                "splat_c3_us": captured(splat(rp3, frame)),
                "update_us": captured(lambda: lib.depth_update(ds, ws, inv, wgt, dis, flags, seg, 0.5, 0.9, 8.0)),
                "splat_accumulate_c1_us": captured(lambda: lib.splat_accumulate([(src1, rp0.flow, None, None, 1.0, 1.0)], acc1, 0.0, 12.0, 255.0)),
                "splat_resolve_c1_us": captured(lambda: lib.splat_resolve(acc1, out1, hole1, 1, 255.0, 2.0 ** -10)),
                "map_us": captured(lambda: parallax_map(fw, R, t, out=maps)),
                "run_us": captured(lambda: rp0.run(None, inv, wgt, R, T)),
                "run_c3_us": captured(lambda: rp3.run(frame, inv, wgt, R, T)),
                "push_us": captured(prop.push)}
            e = {k_: [] for k_ in graphs}
            for _ in range(a.rounds):
                for k_, (g, _) in graphs.items():
                    for z in (rp0.acc, rp0.front, rp3.acc, rp3.front, acc1, prop.rp.acc, prop.rp.front):
                        z.zero_()
                    if k_ in ("accumulate_us", "accumulate_c3_us"):            # against the front of its own projection
                        lib.zsplat_front(None, rp0.flow, rp0.d_new, wgt, rp0.valid, rp0.front, o["b_min"])
                        lib.zsplat_front(frame, rp3.flow, rp3.d_new, wgt, rp3.valid, rp3.front, o["b_min"])
                    e[k_].append(round(replay_us(g, a.replays), 2))
            e["median"] = {k_: statistics.median(e[k_]) for k_ in graphs}
            e["spread"] = {k_: spread(e[k_]) for k_ in graphs}
            md = e["median"]
            for k_, y in (("front_us", "splat_accumulate_c1_us"), ("accumulate_us", "splat_accumulate_c1_us"),
                          ("accumulate_c3_us", "splat_accumulate_c1_us"), ("resolve_us", "splat_resolve_c1_us"),
                          ("resolve_c3_us", "splat_resolve_c1_us"), ("project_us", "map_us"), ("update_us", "map_us")):
                e[k_.replace("_us", "_over_") + y.replace("_us", "")] = round(md[k_] / md[y], 2)
            e["holes"] = round(float(rp0.hole.float().mean()), 4)
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
            fr = [torch.roll(f0, shifts=(t_, 3 * t_), dims=(2, 3)).cuda().contiguous() for t_ in range(a.frames)]
            stream = FlowStream(model, iters=a.iters, warm_start=True, bidirectional=True, occlusion="plane")
            odo = Odometry(B, H, W, dev)
            prop = DepthPropagator(odo)

            def both(r):
                odo.push(r)
                prop.push()

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

            b = {"B": B, "iters": a.iters, "occlusion": "plane", "step_odometry_ms": [], "step_odometry_depth_ms": []}
            for _ in range(a.rounds):
                b["step_odometry_ms"].append(round(ms_per_frame(odo.push), 4))
                b["step_odometry_depth_ms"].append(round(ms_per_frame(both), 4))
            med = {k_: statistics.median(b[k_]) for k_ in ("step_odometry_ms", "step_odometry_depth_ms")}
            b["median"] = {k_: round(v, 4) for k_, v in med.items()}
            b["push_behind_step_us"] = round(1000.0 * (med["step_odometry_depth_ms"] - med["step_odometry_ms"]), 2)
            b["step_spread_us"] = round(1000.0 * spread(b["step_odometry_ms"]), 2)
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
