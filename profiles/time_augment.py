"""The 360-degree training augmentation on the device: what it costs alone, behind a training step, and on the host
(DESIGN.md section 14).  Interleaved rounds on one box, medians:

  (a) DeviceAugmentor360 alone at 512x1024 and 384x512, B = 1 and 8: one captured graph (4 launches), 200 replays between
      device events, microseconds per replay.  The replays run on the same buffers, which stay resident in L2 / Infinity Cache:
      a lower bound for a batch that has just arrived over PCIe;
  (b) GraphedTrainStep at 384x512, iters = 12, one pair: fed with ready device tensors, against the same stepper fed through
      augmented_batches from pinned uint8 batches (copy + augmentation on the side stream, depth 2); host clock around windows
      of at least --window seconds that end in a synchronise;
  (c) the host route: tests/augment_ref.pil_chain (Pillow's ImageEnhance + HSV hue shift, what torchvision's PIL backend runs)
      plus eraser and roll in numpy, on the job's cores (--procs processes), samples / s at 512x1024.

The structural condition: (b) with augmentation exceeds (b) without it by no more than the step's own spread between the rounds
of the same run (compare with the 1 % of profiles/r8_bidirectional_time.json).

    python profiles/time_augment.py --out profiles/r10_augment_time.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o aug -- python profiles/time_augment.py --only a --rounds 1
    python profiles/time_augment.py --by-shape DIR/aug_kernel_trace.csv > profiles/r10_augment_kernels_by_shape.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402


def host_sample(args):
    """One sample through the host route (a worker process; no GPU, no torch threads)."""
    seed, H, W = args
    import augment_ref as ar
    r = np.random.RandomState(seed)
    i1, i2 = (r.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
    flow = r.standard_normal((H, W, 2)).astype(np.float32) * 20
    order = [int(v) for v in r.permutation(4)]
    f = [float(np.float32(v)) for v in r.uniform(0.6, 1.4, 3)]
    t0 = time.perf_counter()
    stack = ar.pil_chain(np.concatenate([i1, i2], axis=0), order, f[0], f[1], f[2], int(r.randint(0, 256)))
    i1, i2 = np.split(stack, 2, axis=0)
    mean = np.mean(i2.reshape(-1, 3), axis=0)
    i2 = i2.copy()
    i2[40:120, 60:150] = mean
    k = int(r.randint(-200, 200))
    out = (np.roll(i1, k, axis=1).transpose(2, 0, 1).astype(np.float32), np.roll(i2, k, axis=1).transpose(2, 0, 1).astype(np.float32),
           np.ascontiguousarray(np.roll(flow, k, axis=1).transpose(2, 0, 1)))
    return float(time.perf_counter() - t0 + 0.0 * out[0][0, 0, 0])


def host_route(procs, n, H, W):
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(host_sample, [(s, 64, 128) for s in range(procs)])           # start the workers
        t0 = time.perf_counter()
        each = pool.map(host_sample, [(s, H, W) for s in range(n)], chunksize=1)
        wall = time.perf_counter() - t0
    return {"procs": procs, "samples": n, "samples_per_s": round(n / wall, 2), "ms_per_sample_one_core": round(1e3 * statistics.median(each), 1)}


def kernels_by_shape(trace_csv):
    """Median kernel times per launch geometry from a rocprofv3 --kernel-trace csv of `--only a` (the stats file sums the four
    configurations): lines of `kernel grid(x y z) launches median_us`; grid x is work items, y the images / planes, z the batch."""
    import collections
    import csv
    g = collections.defaultdict(list)
    for r in csv.DictReader(open(trace_csv)):
        short = [k for k in ("zero", "contrast", "main", "erase") if "pf_aug_" + k in r["Kernel_Name"]]
        if short:
            g[(short[0], int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return "".join(f"pf_aug_{k[0]}_kernel grid({k[1]} {k[2]} {k[3]}) {len(v)} {statistics.median(v) / 1000:.1f}\n" for k, v in sorted(g.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--by-shape", default="", help="a rocprofv3 kernel trace csv: print median kernel times per launch geometry and exit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.5)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--host-samples", type=int, default=64)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.by_shape:
        print(kernels_by_shape(a.by_shape), end="")
        return
    res = {"rounds": a.rounds, "window_s": a.window,
           "note": "alone_us: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; step_*_ms: host clock "
                   "around windows that end in a synchronise; lists: interleaved rounds; the medians are what DESIGN.md quotes"}
    if "c" in a.only:                                          # first: worker processes are started before this process opens the GPU
        res["host_route"] = host_route(a.procs, a.host_samples, 512, 1024)
        print(json.dumps(res["host_route"]), flush=True)
    import torch
    from prior_flow_amd import augment as ag
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda", 0)
    res["device"] = torch.cuda.get_device_name(0)

    def inputs(B, H, W, seed):
        r = np.random.RandomState(seed)
        return (torch.from_numpy(r.randint(0, 256, (B, H, W, 3)).astype(np.uint8)), torch.from_numpy(r.randint(0, 256, (B, H, W, 3)).astype(np.uint8)),
                torch.from_numpy((r.standard_normal((B, H, W, 2)) * 20).astype(np.float32)))

    if "a" in a.only:
        alone = []
        for H, W in ((512, 1024), (384, 512)):
            for B in (1, 8):
                aug = ag.DeviceAugmentor360(B, H, W, dev)
                ins = [t.to(dev) for t in inputs(B, H, W, 1)]
                p = ag.sample_params_360(B, H, W, np.random.RandomState(2), torch.Generator().manual_seed(2), eraser_aug_prob=1.0,
                                         rotaton_aug_prob=1.0)
                aug(*ins, p)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    aug(*ins)
                # the graph holds raw pointers: the augmentor and its inputs must outlive it (the next capture empties the
                # allocator's cache, which would unmap the buffers of an augmentor that had been dropped)
                alone.append({"shape": [H, W], "B": B, "graph": g, "keep": (aug, ins), "us": []})
        for _ in range(a.rounds):
            for e in alone:
                for _ in range(10):
                    e["graph"].replay()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(200):
                    e["graph"].replay()
                t1.record()
                torch.cuda.synchronize()
                e["us"].append(round(t0.elapsed_time(t1) * 1000.0 / 200, 2))
        for e in alone:
            del e["graph"], e["keep"]
            e["median_us"] = statistics.median(e["us"])
            e["us_per_pair"] = round(e["median_us"] / e["B"], 2)
            print(json.dumps(e), flush=True)
        res["alone"] = alone

    if "b" in a.only:
        from prior_flow_amd import det_state_dict
        from prior_flow_amd import train as tr
        from prior_flow_amd.modules import state_dict_shapes
        from prior_flow_amd.prior_raft import PriOr_RAFT
        H, W, B = 384, 512, 1
        model = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
        model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
        model = model.to(dev).train()
        model.freeze_bn()
        opt, sched = tr.fetch_optimizer(argparse.Namespace(lr=2e-5, wdecay=5e-5, epsilon=1e-8, num_steps=1000000), model)
        crit = tr.uniform_loss(H, W, device=dev)
        stepper = tr.GraphedTrainStep(model, opt, sched, crit, iters=a.iters, clip=1.0, warmup=1)
        host = [tuple(t.pin_memory() for t in inputs(B, H, W, 10 + k)) for k in range(4)]
        kw = dict(eraser_aug_prob=1.0, rotaton_aug_prob=1.0)
        aug = ag.DeviceAugmentor360(B, H, W, dev)
        ready = [[o.clone() for o in aug(*(t.to(dev) for t in h), ag.sample_params_360(B, H, W, np.random.RandomState(k), torch.Generator().manual_seed(k), **kw))]
                 for k, h in enumerate(host)]
        feeder = ag.DeviceAugmentor360(B, H, W, dev, outputs=False)
        rng, gen = np.random.RandomState(0), torch.Generator().manual_seed(0)

        def run_ready(n):
            for k in range(n):
                stepper(*ready[k % 4])

        def run_fed(n):
            for batch in ag.augmented_batches((host[k % 4] for k in range(n)), feeder, rng, gen, depth=2, **kw):
                stepper(*batch)

        def timed(fn):
            fn(4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(8)
            torch.cuda.synchronize()
            n = max(8, int(a.window / ((time.perf_counter() - t0) / 8)) + 1)
            t0 = time.perf_counter()
            fn(n)
            torch.cuda.synchronize()
            return round(1e3 * (time.perf_counter() - t0) / n, 4)

        run_ready(4)
        r = {"shape": [H, W], "B": B, "iters": a.iters, "step_ready_ms": [], "step_fed_ms": []}
        for _ in range(a.rounds):
            r["step_ready_ms"].append(timed(run_ready))
            r["step_fed_ms"].append(timed(run_fed))
        med = {k: statistics.median(r[k]) for k in ("step_ready_ms", "step_fed_ms")}
        r["median"] = med
        r["excess_us"] = round(1e3 * (med["step_fed_ms"] - med["step_ready_ms"]), 2)
        r["step_spread_us"] = round(1e3 * (max(r["step_ready_ms"]) - min(r["step_ready_ms"])), 2)
        r["step_spread_pct"] = round(100.0 * (max(r["step_ready_ms"]) - min(r["step_ready_ms"])) / med["step_ready_ms"], 3)
        r["structural_ok"] = bool(r["excess_us"] <= r["step_spread_us"])
        print(json.dumps(r), flush=True)
        res["behind_step"] = r
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
