"""Chained flows on the device: what FlowChain.push costs alone, beside pf_fb_check of the same shape, and behind a
bidirectional FlowStream step.  Interleaved rounds on one box, medians and the spread of the same run:

  (a) alone, one captured graph each (one launch), microseconds per replay between device events, 512x1024, B = 1 and 8, on
      a smooth flow pair (a pan plus a tilt with 0.05 px of noise: neighbouring pixels sample neighbouring taps) and on a random
      one (6 px of white noise: every tap its own cache line):
        push_us        FlowChain.push of a BidirectionalFlow (two jobs: forward in place, backward into the other buffer)
        push_plain_us  FlowChain.push of a plain flow (one job)
        fb_check_us    pf_fb_check("plane") of the same two flows (both directions)
        floor_us       27 bytes per pixel and job at 8 TB/s (f and state in, g and occ gathered once, out and state out)
  (b) milliseconds per frame of the warm bidirectional FlowStream step (512x1024, iters 12, B = 1, occlusion "plane") alone and
      with the chain behind it on the same stream.  The step alone is the parent commit's code, measured in the same process.

    python profiles/time_chain.py --out profiles/r9_chain_time.json
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
from prior_flow_amd.tracks import FlowChain  # noqa: E402
from prior_flow_amd.video import BidirectionalFlow, FlowStream, forward_backward_check  # noqa: E402


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
    assert torch.cuda.is_available(), "time_chain.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    H, W = 512, 1024
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "hbm_tb_per_s": 8.0, "shape": [H, W],
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; floor_us: 27 bytes per "
                   "pixel and job at 8 TB/s; *_ms: host clock around whole sequences that end in a synchronise; lists: interleaved "
                   "rounds; spread: max - min over the rounds of the same run"}
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
                r = BidirectionalFlow(fw, bw, *forward_backward_check(fw, bw, metric="plane"))
                out = tuple(torch.empty_like(t) for t in r[2:])
                chain, plain = FlowChain(B, H, W, dev), FlowChain(B, H, W, dev)
                e = {"B": B, "data": data, "floor_us": {"push": round(2 * 27 * B * H * W / 8e12 * 1e6, 2), "push_plain": round(27 * B * H * W / 8e12 * 1e6, 2)},
                     "keep": (r, out, chain, plain)}
                # a replay composes onto the chain's own result: the traffic of a push, whatever the values have grown to
                e["graphs"] = {"push_us": captured(lambda: chain.push(r)), "push_plain_us": captured(lambda: plain.push(fw)),
                               "fb_check_us": captured(lambda: forward_backward_check(fw, bw, metric="plane", out=out))}
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
                e["spread"] = {k: spread(e[k]) for k in names}
                e["push_minus_fb_check_us"] = round(e["median"]["push_us"] - e["median"]["fb_check_us"], 2)
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
            chain = FlowChain(B, H, W, dev)

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

            b = {"B": B, "iters": a.iters, "occlusion": "plane", "step_ms": [], "step_chain_ms": []}
            for _ in range(a.rounds):
                b["step_ms"].append(round(ms_per_frame(lambda r: None), 4))
                b["step_chain_ms"].append(round(ms_per_frame(chain.push), 4))
            med = {k: statistics.median(b[k]) for k in ("step_ms", "step_chain_ms")}
            b["median"] = {k: round(v, 4) for k, v in med.items()}
            b["chain_behind_step_us"] = round(1000.0 * (med["step_chain_ms"] - med["step_ms"]), 2)
            b["step_spread_us"] = round(1000.0 * spread(b["step_ms"]), 2)
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
