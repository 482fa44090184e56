"""alternate_corr A/B: graph-replay pairs/s of the test_mode forward, iters=12, with args.alternate_corr False (volumes and
pyramids) and True (pooled features, lookups from dot products), interleaved on the same box at 512x1024 B = 1 and B = 8;
then the alternate mode alone at 1920x3840 B = 1 (the default mode would need 141 GB of pyramids there): time per forward and
the peak allocated memory.  Rounds alternate the two modes (A B B A ...).  Prints and writes one JSON object.

    python profiles/time_alternate_corr.py --out profiles/r7_alternate_corr_time.json
    # per-kernel times (pf_lookup_feat_kernel against the default pf_elem_kernel<PfLookupArgs, ...>):
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python profiles/time_alternate_corr.py --trace
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


def model(alt):
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.synthetic import det_state_dict
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0, alternate_corr=alt))
    m.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
    return m.cuda().eval()


def timed(m, i1, i2, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m(i1, i2, iters=12, test_mode=True)
    torch.cuda.synchronize()
    return steps * i1.shape[0] / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=96)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big-steps", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="a few B = 1 512x1024 forwards of each mode (under rocprofv3), no timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from prior_flow_amd.synthetic import synthetic_pair
    ms = {False: model(False), True: model(True)}
    res = {"what": "graph-replay pairs/s, test_mode forward iters=12, alternate_corr False vs True, interleaved",
           "device": torch.cuda.get_device_name(0), "batches": {}}
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            i1, i2 = synthetic_pair(B, 512, 1024)
            i1, i2 = i1.cuda(), i2.cuda()
            for alt in (False, True):                     # capture + warm-up
                for _ in range(a.warmup):
                    ms[alt](i1, i2, iters=12, test_mode=True)
            if a.trace:
                for alt in (False, True):
                    for _ in range(3):
                        ms[alt](i1, i2, iters=12, test_mode=True)
                torch.cuda.synchronize()
                return
            runs = {False: [], True: []}
            for r in range(a.rounds):
                for alt in ((False, True) if r % 2 == 0 else (True, False)):
                    runs[alt].append(timed(ms[alt], i1, i2, max(3, a.pairs // B)))
            med = {k: statistics.median(v) for k, v in runs.items()}
            res["batches"][str(B)] = {"default_pairs_s": runs[False], "alternate_pairs_s": runs[True],
                                      "default_median": med[False], "alternate_median": med[True],
                                      "default_ms_per_pair": 1e3 / med[False], "alternate_ms_per_pair": 1e3 / med[True],
                                      "alternate_time_over_default": med[False] / med[True]}
            print(f"512x1024 B={B}: default {med[False]:.1f} pairs/s, alternate {med[True]:.1f} pairs/s "
                  f"({med[False] / med[True]:.2f}x the time)", flush=True)
        # the panorama: alternate only
        for m in ms.values():
            m._ws.clear()
            m._graphs.clear()
        del ms[False]
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        i1, i2 = synthetic_pair(1, 1920, 3840)
        i1, i2 = i1.cuda(), i2.cuda()
        for _ in range(2):
            ms[True](i1, i2, iters=12, test_mode=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.big_steps):
            ms[True](i1, i2, iters=12, test_mode=True)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.big_steps
        peak = torch.cuda.max_memory_allocated() - base
        res["1920x3840_b1"] = {"alternate_ms_per_pair": dt * 1e3, "peak_allocated_growth_gib": peak / 2 ** 30,
                               "workspace_gib": ms[True]._ws[next(iter(ms[True]._ws))].nbytes / 2 ** 30}
        print(f"1920x3840 B=1 alternate: {dt * 1e3:.1f} ms per pair, peak allocation growth {peak / 2 ** 30:.2f} GiB", flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
