"""mixed_precision A/B: graph-replay pairs/s of the test_mode forward at 512x1024, iters=12, with args.mixed_precision False
(bf16x3 update blocks) and True (fp16 update blocks, PF_PREC_F16), interleaved on the same box, at B = 1 and at batch 32.
Both models hold the same deterministic weights.  Rounds alternate the two modes (A B B A ...) so that clock and thermal drift
fall on both alike; per round a mode runs about `--pairs` pairs of timed replays (at least 3 forwards).  Prints and writes one
JSON object.

    python profiles/time_mixed_precision.py --out profiles/r7_mixed_precision_time.json
    # per-kernel times of the all-DMA conv launches (f16 = pf_conv_dma_kernel<..., true>):
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python profiles/time_mixed_precision.py --trace
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


def models():
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.synthetic import det_state_dict
    sd = det_state_dict(state_dict_shapes())
    out = {}
    for mixed in (False, True):
        m = PriOr_RAFT(argparse.Namespace(mixed_precision=mixed, dropout=0.0))
        m.load_state_dict(sd, strict=True)
        out[mixed] = m.cuda().eval()
    return out


def timed(m, i1, i2, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m(i1, i2, iters=12, test_mode=True)
    torch.cuda.synchronize()
    return steps * i1.shape[0] / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=320)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="a few B = 1 forwards of each mode (under rocprofv3), no timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from prior_flow_amd.synthetic import synthetic_pair
    ms = models()
    res = {"what": "graph-replay pairs/s, test_mode forward 512x1024 iters=12, mixed_precision False vs True, interleaved",
           "device": torch.cuda.get_device_name(0), "batches": {}}
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            i1, i2 = synthetic_pair(B, 512, 1024)
            i1, i2 = i1.cuda(), i2.cuda()
            for mixed in (False, True):                   # capture + warm-up
                for _ in range(a.warmup):
                    ms[mixed](i1, i2, iters=12, test_mode=True)
            if a.trace:
                for mixed in (False, True):
                    for _ in range(3):
                        ms[mixed](i1, i2, iters=12, test_mode=True)
                torch.cuda.synchronize()
                break
            runs = {False: [], True: []}
            for r in range(a.rounds):
                for mixed in ((False, True) if r % 2 == 0 else (True, False)):
                    runs[mixed].append(timed(ms[mixed], i1, i2, max(3, a.pairs // B)))
            med = {k: statistics.median(v) for k, v in runs.items()}
            res["batches"][str(B)] = {"bf16x3_pairs_s": runs[False], "f16_pairs_s": runs[True],
                                      "bf16x3_median": med[False], "f16_median": med[True],
                                      "f16_over_bf16x3": med[True] / med[False]}
            print(f"B={B}: bf16x3 {med[False]:.1f} pairs/s, f16 {med[True]:.1f} pairs/s ({med[True] / med[False]:.3f}x)", flush=True)
    if a.trace:
        return
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
