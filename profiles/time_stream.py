"""Video inference: pairs/s of per-pair model(...) graph replay against FlowStream (cold and warm-started) over a 16-frame synthetic
sequence at 512x1024, iters=12, B = 1 and 8; plus what one stream step launches beyond a pair's work (fnet images counted in an
eager step, pf_forward_interpolate and the three slot copies timed alone with events).

    python profiles/time_stream.py --out profiles/r7_stream_time.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from prior_flow_amd import det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd import engine  # noqa: E402
from prior_flow_amd.evaluate import forward_interpolate  # noqa: E402
from prior_flow_amd.prior_raft import PriOr_RAFT, state_dict_shapes  # noqa: E402
from prior_flow_amd.video import FlowStream  # noqa: E402


def frames(T, B, H, W):
    f0, _ = synthetic_pair(B, H, W, seed=7)
    return [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda() for t in range(T)]


def per_pair(model, fr, iters, reps):
    for t in range(1, len(fr)):                                  # warm-up (capture)
        model(fr[t - 1], fr[t], iters=iters, test_mode=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        for t in range(1, len(fr)):
            model(fr[t - 1], fr[t], iters=iters, test_mode=True)
    torch.cuda.synchronize()
    return reps * (len(fr) - 1) / (time.perf_counter() - t0)


def stream(model, fr, iters, warm, reps):
    s = FlowStream(model, iters=iters, warm_start=warm)
    for f in fr:                                                 # warm-up (captures the cold and the warm graph)
        s(f)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        s.reset()                                                # every rep is a whole sequence: first frame, cold first pair
        for f in fr:
            s(f)
    torch.cuda.synchronize()
    return reps * (len(fr) - 1) / (time.perf_counter() - t0)


def event_us(fn, n=200):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def step_detail(model, B, H, W, iters):
    """fnet / cnet images of one eager stream step (counted at EncoderPlan.run), and the stream's own extra work timed alone."""
    fr = frames(3, B, H, W)
    s = FlowStream(model, iters=iters, warm_start=True, use_graph=False)
    s(fr[0])
    s(fr[1])
    seen = []
    run = engine.EncoderPlan.run

    def counted(plan, images, *a, **k):
        seen.append((plan.kind, int(images.shape[0])))
        return run(plan, images, *a, **k)
    engine.EncoderPlan.run = counted
    try:
        s(fr[2])
    finally:
        engine.EncoderPlan.run = run
    st = s._st
    low = st.flow_low
    fi = event_us(lambda: forward_interpolate(low, wrap=True, out=st.init, scratch=st.scratch))

    def copies():
        st.f4[:, 0].copy_(st.f4[:, 1])
        if st.s4 is not None:
            st.s4[:, 0].copy_(st.s4[:, 1])
        st.img_prev.copy_(st.img_new)
    cp = event_us(copies)

    def new_slot():
        st.f4[:, 1].copy_(st.fn.view(2, st.rows, 256))
        if st.s4 is not None:
            st.s4[:, 1].copy_(st.fn_split.view(2, st.rows, 8, 2, 32))
    ns = event_us(new_slot)
    return {"fnet_images_per_step": sum(n for k, n in seen if k == "instance"),
            "cnet_images_per_step": sum(n for k, n in seen if k == "batch"),
            "per_pair_fnet_images": 4 * B,
            "forward_interpolate_us": round(fi, 2), "cached_slot_copies_us": round(cp, 2), "new_slot_copies_us": round(ns, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    H, W = 512, 1024
    model = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
    model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
    model = model.cuda().eval()
    res = {"shape": [H, W], "iters": a.iters, "frames": a.frames, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "note": "pairs/s over whole sequences: a stream rep includes its first frame (fnet only) and a cold first pair",
           "runs": []}
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            fr = frames(a.frames, B, H, W)
            r = {"B": B}
            # interleaved twice: per-pair, cold stream, warm stream (same box, same clocks)
            for k in range(2):
                r.setdefault("per_pair_pairs_s", []).append(round(per_pair(model, fr, a.iters, a.reps), 2))
                r.setdefault("stream_cold_pairs_s", []).append(round(stream(model, fr, a.iters, False, a.reps), 2))
                r.setdefault("stream_warm_pairs_s", []).append(round(stream(model, fr, a.iters, True, a.reps), 2))
            best = {k: max(v) for k, v in r.items() if k.endswith("_pairs_s")}
            r["gain_cold_pct"] = round(100.0 * (best["stream_cold_pairs_s"] / best["per_pair_pairs_s"] - 1.0), 2)
            r["gain_warm_pct"] = round(100.0 * (best["stream_warm_pairs_s"] / best["per_pair_pairs_s"] - 1.0), 2)
            r.update(step_detail(model, B, H, W, a.iters))
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
            del fr
            model._ws.clear()
            model._graphs.clear()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
