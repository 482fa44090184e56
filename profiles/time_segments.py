"""Moving objects on the device: what the labelling, the object table and a whole MovingObjects.update cost at 512x1024, B = 1, on
three masks, beside pf_epi_map (one pass over the same pixels), and behind a bidirectional FlowStream step.
Interleaved rounds on one box, medians and the spread of the same run:

  (a) alone, one captured graph each, microseconds per replay between device events, per mask:
        label_us       pf_seg_label: tiles, merge, flatten (three launches)
        objects_us     pf_seg_objects on those labels: count, scan, assign, accumulate, resolve (five launches), C = 3
        update_us      MovingObjects.update (the eight launches), C = 3, max_objects = 64, min_area = 4
        map_us         pf_epi_map, all four outputs: the yardstick
      masks: "balls": discs on the sphere (the blobs of a moving-ball scene: 12 balls of angular radius 0.05 .. 0.3, one across the
      seam, one over a pole); "bernoulli": independent pixels at p = 0.5 (one giant ragged cluster at 8, thousands of small ones);
      "serpentine": one snake of H W / 2 pixels through every tile border, the deep-tree case.
  (b) milliseconds per frame of the warm bidirectional FlowStream step (512x1024, iters 12, B = 1, occlusion "plane") alone and
      with one MovingObjects.update of its occlusion mask behind it, on the same stream.
  --lib PATH [PATH ...]: label_us of the three masks again on builds of pf_segments.hip alone with another tile height, beside the
      product's, after checking that they give the product's labels:
        hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -fPIC -shared -DPF_SG_STANDALONE -DPF_SG_TH=16 \
              -I prior-flow_amd/csrc prior-flow_amd/csrc/pf_segments.hip -o profiles/scratch/libpf_segments_th16.so
  --trace: each update a few times, eagerly, and nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the
      time of each launch (kernel names pf_seg_*).

    python profiles/time_segments.py --out profiles/r17_segments_time.json
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from prior_flow_amd import det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd.parallax import parallax_map  # noqa: E402
from prior_flow_amd.segments import MovingObjects  # noqa: E402
from prior_flow_amd.video import FlowStream  # noqa: E402
from time_pose import captured, replay_us, scene_flow, spread  # noqa: E402


def masks(H, W, dev):
    n, m = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    th, ph = ((m + 0.5) / W - 0.5) * 2 * math.pi, (0.5 - (n + 0.5) / H) * math.pi
    p = torch.stack([ph.cos() * th.cos(), ph.cos() * th.sin(), ph.sin()], -1)
    balls = torch.zeros(H, W, dtype=torch.bool, device=dev)
    g = torch.Generator().manual_seed(3)
    centres = [(math.pi - 0.02, 0.2, 0.3), (0.4, math.pi / 2 - 0.05, 0.2)]                      # across the seam, over a pole
    centres += [(float(torch.rand(1, generator=g)) * 2 * math.pi - math.pi, float(torch.rand(1, generator=g)) * 2.4 - 1.2,
                 0.05 + 0.25 * float(torch.rand(1, generator=g))) for _ in range(10)]
    for t0, p0, rad in centres:
        c = torch.tensor([math.cos(p0) * math.cos(t0), math.cos(p0) * math.sin(t0), math.sin(p0)], dtype=torch.float64, device=dev)
        balls |= torch.acos((p @ c).clamp(-1, 1)) <= rad
    bern = torch.rand(H, W, generator=torch.Generator().manual_seed(4)).to(dev) < 0.5
    serp = torch.zeros(H, W, dtype=torch.bool, device=dev)
    serp[0::2, :W - 1] = True
    for r in range(1, H - 1, 2):
        serp[r, W - 2 if (r // 2) % 2 == 0 else 0] = True
    return {k: v.to(torch.uint8)[None].contiguous() for k, v in (("balls", balls), ("bernoulli", bern), ("serpentine", serp))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--only", default="ab")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--lib", nargs="*", default=[])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_segments.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, H, W = 1, 512, 1024
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "shape": [H, W], "B": B,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; *_ms: host clock around "
                   "whole sequences that end in a synchronise; lists: interleaved rounds; spread: max - min over the rounds of the same run"}
    with torch.no_grad():
        mk = masks(H, W, dev)
        values = torch.randn(B, 3, H, W, device=dev).contiguous()
        if a.trace:
            mo = MovingObjects(B, H, W, dev, channels=3)
            for name, m in mk.items():
                for _ in range(5):
                    mo.update(m, values)
                torch.cuda.synchronize()
                print(name, int(mo.count[0]), flush=True)
            return
        if "a" in a.only:
            fw, R_true, t_true = scene_flow(H, W, dev)
            R, t = R_true.float()[None].contiguous(), t_true.float()[None].contiguous()
            maps = tuple(torch.empty(B, H, W, device=dev) for _ in range(3)) + (torch.empty(B, H, W, dtype=torch.uint8, device=dev),)
            objs = {k: MovingObjects(B, H, W, dev, channels=3) for k in mk}
            graphs = {"map_us": captured(lambda: parallax_map(fw, R, t, out=maps))}
            info = {}
            for k, m in mk.items():
                mo = objs[k]
                mo.update(m, values)
                torch.cuda.synchronize()
                info[k] = {"set_pixels": int(m.sum()), "components": int(torch.unique(mo.labels).numel()) - 1, "survivors": int(mo.count[0])}
                lib, tb = mo.lib, mo._t
                graphs[f"{k}_label_us"] = captured(lambda m=m, mo=mo, tb=tb: mo.lib.seg_label(m, tb.rows, mo.labels, tb.scratch, 8, False))
                graphs[f"{k}_objects_us"] = captured(lambda mo=mo, tb=tb: mo.lib.seg_objects(mo.labels, values, tb.rows, tb.cols, tb.scratch, mo.ids,
                                                                                             mo.keep, mo.roots, mo.count, mo.table, mo.sums, 4.0))
                graphs[f"{k}_update_us"] = captured(lambda m=m, mo=mo: mo.update(m, values))
            others = []
            for path in a.lib:
                from prior_flow_amd import _lib
                tag = os.path.basename(path).replace("libpf_segments_", "").replace(".so", "")
                other = _lib.PfLib(path, require_cuda=True, optional=tuple(n for n in _lib.EXPORTS if not n.startswith("pf_seg_")))
                for k, m in mk.items():
                    mo = MovingObjects(B, H, W, dev, channels=3, lib=other)
                    mo.update(m, values)
                    torch.cuda.synchronize()
                    assert torch.equal(mo.labels, objs[k].labels) and torch.equal(mo.sums, objs[k].sums), (path, k)
                    others.append(mo)
                    tb = mo._t
                    graphs[f"{k}_label_{tag}_us"] = captured(lambda m=m, mo=mo, tb=tb: mo.lib.seg_label(m, tb.rows, mo.labels, tb.scratch, 8, False))
            e = {k_: [] for k_ in graphs}
            for _ in range(a.rounds):
                for k_, (g, _) in graphs.items():
                    e[k_].append(round(replay_us(g, a.replays), 2))
            e["median"] = {k_: statistics.median(e[k_]) for k_ in graphs}
            e["spread"] = {k_: spread(e[k_]) for k_ in graphs}
            md = e["median"]
            e["over_map"] = {k_: round(md[k_] / md["map_us"], 2) for k_ in graphs if k_ != "map_us"}
            e["masks"] = info
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
            mo = MovingObjects(B, H, W, dev, channels=2)

            def ms_per_frame(after):
                def seq():
                    for f in fr:
                        r = stream(f)
                        if r is not None and after is not None:
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

            b = {"B": B, "iters": a.iters, "occlusion": "plane", "step_ms": [], "step_objects_ms": []}
            for _ in range(a.rounds):
                b["step_ms"].append(round(ms_per_frame(None), 4))
                b["step_objects_ms"].append(round(ms_per_frame(lambda r: mo.update(r.occ_forward, r.forward)), 4))
            med = {k_: statistics.median(b[k_]) for k_ in ("step_ms", "step_objects_ms")}
            b["median"] = {k_: round(v, 4) for k_, v in med.items()}
            b["update_behind_step_us"] = round(1000.0 * (med["step_objects_ms"] - med["step_ms"]), 2)
            b["step_spread_us"] = round(1000.0 * spread(b["step_ms"]), 2)
            print(json.dumps(b), flush=True)
            res["behind_step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
