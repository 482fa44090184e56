"""Bidirectional video inference: milliseconds per frame of FlowStream(bidirectional=True) against what the one-direction code
offers for the same result -- a one-direction FlowStream step plus one per-pair model(frame, previous) graph replay per frame --
over a 16-frame synthetic sequence at 512x1024, iters=12, B = 1 and 8, graph replay, runs interleaved; the forward-backward
check timed alone; what a batch of 2B costs against two batches of B (per-pair replays); the step's phases timed alone with
events; and the workspaces' sizes.

    python profiles/time_bidirectional.py --out profiles/r8_bidirectional_time.json
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
from prior_flow_amd.engine import Engine  # noqa: E402
from prior_flow_amd.prior_raft import PriOr_RAFT, state_dict_shapes  # noqa: E402
from prior_flow_amd.video import FlowStream, forward_backward_check  # noqa: E402


def frames(T, B, H, W):
    f0, _ = synthetic_pair(B, H, W, seed=7)
    return [torch.roll(f0, shifts=(t, 3 * t), dims=(2, 3)).cuda() for t in range(T)]


def timed_ms_per_frame(run_sequence, n_pairs, reps):
    run_sequence()                                               # warm-up (captures every graph the sequence uses)
    run_sequence()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run_sequence()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / (reps * n_pairs)


def baseline(model, fr, iters, warm):
    """The parent's way to both directions: a one-direction stream step and a per-pair call of the reversed pair."""
    s = FlowStream(model, iters=iters, warm_start=warm)

    def seq():
        s.reset()
        prev = None
        for f in fr:
            s(f)
            if prev is not None:
                model(f, prev, iters=iters, test_mode=True)
            prev = f
    return seq


def bidirectional(model, fr, iters, warm, occlusion):
    s = FlowStream(model, iters=iters, warm_start=warm, bidirectional=True, occlusion=occlusion)

    def seq():
        s.reset()
        for f in fr:
            s(f)
    seq.stream = s
    return seq


def per_pair(model, fr, iters):
    def seq():
        for t in range(1, len(fr)):
            model(fr[t - 1], fr[t], iters=iters, test_mode=True)
    return seq


def event_us(fn, n=100):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def phases(model, s, fr):
    """The bidirectional step's own phases, each timed alone (eager launches, device events): the encoders on the new frame's
    2B images, the cached context into the workspace + the context hoist, the corr build of the 2B batch."""
    st = s._st
    lib, P = model._lib(), model._weights()
    plans = model._encoder_plans()
    eng = Engine(lib, None)
    slot = st.t % 2
    lib.prepare_frame(fr[0], st.ws.g_a2b, st.img_new)
    out = {"cnet_2B_images_us": event_us(lambda: s._encode_context(st, plans[0], slot), 30),
           "fnet_2B_images_and_slot_copies_us": event_us(lambda: s._encode_features(st, plans[1], P, slot), 30),
           "context_copies_us": event_us(lambda: s._context_in(st, lib)),
           "context_hoist_2B_us": event_us(lambda: eng.hoist_context(st.ws, P)),
           "corr_build_2B_us": event_us(lambda: eng.build_pyramids(st.ws, Engine.encoder_precision(P)), 30)}
    return {k: round(v, 1) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    H, W = a.height, a.width
    model = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
    model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
    model = model.cuda().eval()
    res = {"shape": [H, W], "iters": a.iters, "frames": a.frames, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "note": "ms per frame over whole sequences (a sequence's first frame has no pair; T - 1 pairs per direction); "
                   "baseline = one-direction FlowStream step + one per-pair replay of the reversed pair; lists: two interleaved rounds",
           "runs": []}
    n_pairs = a.frames - 1
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            fr = frames(a.frames, B, H, W)
            r = {"B": B}
            runs = {"baseline_cold_ms": baseline(model, fr, a.iters, False),
                    "bidirectional_cold_ms": bidirectional(model, fr, a.iters, False, None),
                    "baseline_warm_ms": baseline(model, fr, a.iters, True),
                    "bidirectional_warm_ms": bidirectional(model, fr, a.iters, True, None),
                    "bidirectional_warm_sphere_ms": bidirectional(model, fr, a.iters, True, "sphere")}
            for _ in range(2):                                   # interleaved twice (same box, same clocks)
                for name, seq in runs.items():
                    r.setdefault(name, []).append(round(timed_ms_per_frame(seq, n_pairs, a.reps), 3))
            best = {k: min(v) for k, v in r.items() if k.endswith("_ms")}
            r["gain_cold_pct"] = round(100.0 * (best["baseline_cold_ms"] / best["bidirectional_cold_ms"] - 1.0), 2)
            r["gain_warm_pct"] = round(100.0 * (best["baseline_warm_ms"] / best["bidirectional_warm_ms"] - 1.0), 2)
            bi = runs["bidirectional_warm_ms"].stream
            r["bidirectional_workspace_bytes"] = bi._st.ws.nbytes()
            one = FlowStream(model, iters=a.iters)
            one(fr[0])
            r["one_direction_workspace_bytes"] = one._st.ws.nbytes()
            del one
            r["phases"] = phases(model, bi, fr)
            # the check alone, on the stream's own flows
            bi.reset()
            bi(fr[0])
            got = bi(fr[1])
            for metric in ("sphere", "plane"):
                out = forward_backward_check(got.forward, got.backward, metric=metric)
                r[f"fb_check_{metric}_us"] = round(event_us(
                    lambda: forward_backward_check(got.forward, got.backward, metric=metric, out=out), 200), 2)
            del runs, bi, got
            # what a batch of 2B costs against two batches of B: per-pair replays
            for name, n in (("per_pair_B_ms", B), ("per_pair_2B_ms", 2 * B)):
                model._ws.clear()
                model._graphs.clear()
                frn = fr if n == B else frames(a.frames, n, H, W)
                r[name] = [round(timed_ms_per_frame(per_pair(model, frn, a.iters), n_pairs, a.reps), 3) for _ in range(2)]
                del frn
            r["batch_2B_over_twice_B"] = round(min(r["per_pair_2B_ms"]) / (2.0 * min(r["per_pair_B_ms"])), 4)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
            del fr
            model._ws.clear()
            model._graphs.clear()
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
