"""Camera trajectory from 360-degree video on the device: what the scale link, the track step, the fused depth and a whole
Odometry.push cost, launch by launch, beside the launches of section 20 they are shaped after, and behind a bidirectional
FlowStream step.  Interleaved rounds on one box, medians and the spread of the same run:

  (a) alone, one captured graph each, microseconds per replay between device events, 512x1024, B = 1:
        accumulate_concentrated_us   pf_odo_accumulate on the maps of a static scene (every pixel in one or two bins)
        accumulate_spread_us         pf_odo_accumulate on maps whose ratios are spread evenly over the 512 bins
        epi_accumulate_t_us          pf_epi_accumulate, mode PF_EPI_T (the yardstick: the same outer shape, 9 B per pixel against 18)
        pass_us                      pf_odo_accumulate and pf_odo_solve on live cells (the solve leaves zeros, so the next replay
                                     starts clean); solve_us is the difference to the accumulate alone
        link_us                      ScaleLink.link: the fill of the cells and that pass; fill_us is the difference to the pass
        track_us, reverse_us         pf_odo_track, pf_odo_reverse_pose
        fuse_us                      pf_odo_fuse, all three outputs;  map_us: pf_epi_map, all four outputs (its yardstick)
        push_us                      Odometry.push_flows;  estimate_two_maps_us: PoseEstimator.estimate + two parallax_map calls
      With --lib PATH the two accumulate figures are also taken on another library's pf_odo_accumulate
      (profiles/odo_combine.hip, build line in its header: the form that combines inside the wave before it touches LDS) and reported as
      other_*, with that library's pf_version as other_lib.
  (b) milliseconds per frame of the warm bidirectional FlowStream step (512x1024, iters 12, B = 1, occlusion "plane") alone and
      with one Odometry.push behind it on the same stream.

    python profiles/time_odometry.py --out profiles/r14_odometry_time.json
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

from prior_flow_amd import _lib, det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd.odometry import Odometry, ScaleLink  # noqa: E402
from prior_flow_amd.parallax import PoseEstimator, parallax_map  # noqa: E402
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
    ap.add_argument("--lib", default="", help="another library with pf_odo_accumulate (profiles/odo_combine.hip) to time the two accumulate inputs on")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_odometry.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, H, W, bins = 1, 512, 1024, 512
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "shape": [H, W], "B": B, "bins": bins,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; *_ms: host clock around "
                   "whole sequences that end in a synchronise; lists: interleaved rounds; spread: max - min over the rounds of the same run"}
    with torch.no_grad():
        if "a" in a.only:
            fw, R_true, t_true = scene_flow(H, W, dev)
            bw = -fw
            pose = PoseEstimator(B, H, W, dev)
            lib = pose.lib
            pose.estimate(fw)
            Rm, tm = pose.R.clone(), pose.t.clone()
            outs = tuple(torch.empty(B, H, W, device=dev) for _ in range(3)) + (torch.empty(B, H, W, dtype=torch.uint8, device=dev),)
            outs2 = tuple(torch.empty(B, H, W, device=dev) for _ in range(3)) + (torch.empty(B, H, W, dtype=torch.uint8, device=dev),)
            k, _, c, m = (x.clone() for x in parallax_map(fw, Rm, tm))
            m.zero_()
            conc_a, conc_b = (k, c, m), ((k * 0.3331).contiguous(), c, m)                 # a static scene: every ratio the same
            ramp = torch.exp2(((torch.arange(H * W, device=dev) % (bins - 2) + 1.5) * (8.0 / bins) - 4.0)).reshape(B, H, W)
            spread_b = ((k.clamp_min(1e-3) * ramp).contiguous(), c, m)
            spread_a = (k.clamp_min(1e-3).contiguous(), c, m)
            link = ScaleLink(B, H, W, dev)
            hist = link.hist
            sums = torch.zeros_like(pose.sums)
            odo = Odometry(B, H, W, dev)
            odo.push_flows(fw, bw)
            state, orient, centre = odo.state.clone(), odo.orientation.clone(), odo.centre.clone()
            base, flags = odo.baseline.clone(), odo.flags.clone()
            Rr, tr = torch.empty_like(Rm), torch.empty_like(tm)
            one = torch.ones(B, device=dev)
            fz = (torch.empty(B, H, W, device=dev), torch.empty(B, H, W, device=dev), torch.empty(B, H, W, dtype=torch.uint8, device=dev))

            ratio2, stats2 = torch.empty(B, device=dev), torch.empty(B, 6, device=dev)

            def acc(l_, ma, mb):
                return lambda: l_.odo_accumulate(ma, mb, hist, bins, 4.0, 1e-4)

            def est_maps():
                R, t = pose.estimate(fw)
                parallax_map(fw, R, t, out=outs)
                parallax_map(bw, R, t, out=outs2)

            graphs = {
                "accumulate_concentrated_us": captured(acc(lib, conc_a, conc_b)),
                "accumulate_spread_us": captured(acc(lib, spread_a, spread_b)),
                "epi_accumulate_t_us": captured(lambda: lib.epi_accumulate(fw, None, Rm, tm, sums, _lib.EPI_T, 1.0, 0.25)),
                "pass_us": captured(lambda: (acc(lib, conc_a, conc_b)(), lib.odo_solve(hist, ratio2, stats2, H, W, bins, 4.0, 4, 0.05, 1.0))),
                "link_us": captured(lambda: link.link(conc_a, conc_b)),
                "track_us": captured(lambda: lib.odo_track(Rm, tm, pose.stats, link.ratio, link.stats, state, orient, centre, base, flags)),
                "reverse_us": captured(lambda: lib.odo_reverse_pose(Rm, tm, Rr, tr)),
                "fuse_us": captured(lambda: lib.odo_fuse(conc_a, conc_b, one, one, one, fz[0], fz[1], fz[2], 0.05, 1e-4, 0.5)),
                "map_us": captured(lambda: parallax_map(fw, Rm, tm, out=outs)),
                "push_us": captured(lambda: odo.push_flows(fw, bw)),
                "estimate_two_maps_us": captured(est_maps)}
            if a.lib:
                other = _lib.PfLib(a.lib, require_cuda=True, optional=tuple(_lib.EXPORTS))
                graphs["other_accumulate_concentrated_us"] = captured(acc(other, conc_a, conc_b))
                graphs["other_accumulate_spread_us"] = captured(acc(other, spread_a, spread_b))
            e = {k_: [] for k_ in graphs}
            for _ in range(a.rounds):
                for k_, (g, _) in graphs.items():
                    hist.zero_()
                    sums.zero_()
                    e[k_].append(round(replay_us(g, a.replays), 2))
            e["median"] = {k_: statistics.median(e[k_]) for k_ in graphs}
            e["spread"] = {k_: spread(e[k_]) for k_ in graphs}
            md = e["median"]
            e["concentrated_over_spread"] = round(md["accumulate_concentrated_us"] / md["accumulate_spread_us"], 2)
            if a.lib:
                e["other_concentrated_over_spread"] = round(md["other_accumulate_concentrated_us"] / md["other_accumulate_spread_us"], 2)
                e["other_lib"] = other.version()
            for k_ in ("accumulate_concentrated_us", "accumulate_spread_us"):
                e[k_.replace("_us", "_over_epi_accumulate_t")] = round(md[k_] / md["epi_accumulate_t_us"], 2)
            e["solve_us"] = round(md["pass_us"] - md["accumulate_concentrated_us"], 2)
            e["fill_us"] = round(md["link_us"] - md["pass_us"], 2)
            e["fuse_over_map"] = round(md["fuse_us"] / md["map_us"], 2)
            e["push_over_estimate_two_maps"] = round(md["push_us"] / md["estimate_two_maps_us"], 2)
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
            odo = Odometry(B, H, W, dev)

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

            b = {"B": B, "iters": a.iters, "occlusion": "plane", "step_ms": [], "step_push_ms": []}
            for _ in range(a.rounds):
                b["step_ms"].append(round(ms_per_frame(lambda r: None), 4))
                b["step_push_ms"].append(round(ms_per_frame(odo.push), 4))
            med = {k_: statistics.median(b[k_]) for k_ in ("step_ms", "step_push_ms")}
            b["median"] = {k_: round(v, 4) for k_, v in med.items()}
            b["push_behind_step_us"] = round(1000.0 * (med["step_push_ms"] - med["step_ms"]), 2)
            b["step_spread_us"] = round(1000.0 * spread(b["step_ms"]), 2)
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
