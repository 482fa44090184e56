"""The self-supervised criterion on the device: what one branch's criterion call costs beside the two
launches whose traffic it has to move, and what the step built on it costs beside the supervised one.  Interleaved rounds on one
box, medians and the spread of the same run:

  (a) alone, one captured graph each, microseconds per replay between device events, 384x512, n = 12 predictions, B = 2 and 16:
        selfsup_us          SelfSupervisedLoss.__call__(lazy=True): one pf_selfsup_loss_batch and the sums of its partials
        selfsup_kernel_us   the pf_selfsup_loss_batch launch alone
        seq_loss_us         uniform_loss.__call__(lazy=True) on the same predictions: one pf_seq_loss_batch and its sums
        seq_kernel_us       the pf_seq_loss_batch launch alone
        cycle_warp_us       ONE pf_cycle_warp (C = 3) of image2 by one prediction
      selfsup_kernel_over_sum = selfsup_kernel_us / (seq_kernel_us + n * cycle_warp_us): per prediction the criterion moves what
      a warp plus a sequence-loss term move (flow in, twelve tap values and image1, gradient out).
  (b) milliseconds per step, host clock around steps that end in a synchronise, 384x512, iters 12: train_step_selfsup at B = 1
      (two pairs) beside train_step at B = 2 (two pairs), both eager.

    python profiles/time_selfsup.py --out profiles/r13_selfsup_time.json
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

from prior_flow_amd import _lib, det_state_dict, synthetic_pair  # noqa: E402
from prior_flow_amd import selfsup as ss  # noqa: E402
from prior_flow_amd import train as tr  # noqa: E402


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
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--only", default="ab")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_selfsup.py measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    H, W, n = 384, 512, 12
    res = {"rounds": a.rounds, "replays": a.replays, "device": torch.cuda.get_device_name(0), "shape": [H, W], "n": n,
           "note": "alone: graph replays on the same buffers (resident in L2 / Infinity Cache), device events; *_ms: host clock around "
                   "whole steps that end in a synchronise; lists: interleaved rounds; spread: max - min over the rounds of the same run"}
    lib = _lib.load()
    if "a" in a.only:
        with torch.no_grad():
            for B in (2, 16):
                gen = torch.Generator().manual_seed(B)
                i1, i2 = (t.cuda() for t in synthetic_pair(B, H, W, seed=5))
                preds = [(torch.rand(B, 2, H, W, generator=gen) * 12 - 6).cuda() for _ in range(n)]
                gt = (torch.rand(B, 2, H, W, generator=gen) * 12 - 6).cuda()
                valid = torch.ones(B, H, W, device=dev)
                mask = (torch.rand(B, H, W, generator=gen) < 0.1).to(torch.uint8).cuda()
                crit, sup = ss.SelfSupervisedLoss(H, W), tr.uniform_loss(H, W)
                st = crit._buffers(n, B, dev, 0.8, "", True)
                part6 = torch.empty(n, B, sup.NBLK, 6, dtype=torch.float64, device=dev)
                sgrads = [torch.empty_like(gt) for _ in range(n)]
                wts = [0.8 ** (n - i - 1) for i in range(n)]
                warped = torch.empty_like(i2)
                graphs = {
                    "selfsup_us": captured(lambda: crit(preds, i1, i2, mask, lazy=True)),
                    "selfsup_kernel_us": captured(lambda: lib.selfsup_loss_batch(
                        preds, i1, i2, crit.uniform_mask.view(-1), mask, wts, st["grads"], st["part"], st["z"], crit.w_photo, crit.w_smooth,
                        crit.eps_photo, crit.eps_smooth, crit.edge_lambda, crit.max_flow)),
                    "seq_loss_us": captured(lambda: sup(preds, gt, valid, lazy=True)),
                    "seq_kernel_us": captured(lambda: lib.seq_loss_batch(preds, gt, valid, sup.uniform_mask.view(-1), wts, 400.0, sgrads, part6)),
                    "cycle_warp_us": captured(lambda: lib.cycle_warp(i2, preds[0], warped))}
                e = {k: [] for k in graphs}
                for _ in range(a.rounds):
                    for k, (g, _) in graphs.items():
                        e[k].append(round(replay_us(g, a.replays), 2))
                med = e["median"] = {k: statistics.median(e[k]) for k in graphs}
                e["spread"] = {k: spread(e[k]) for k in graphs}
                e["nblk"] = crit.nblk
                e["selfsup_kernel_over_sum"] = round(med["selfsup_kernel_us"] / (med["seq_kernel_us"] + n * med["cycle_warp_us"]), 3)
                e["selfsup_over_sum"] = round(med["selfsup_us"] / (med["seq_loss_us"] + n * med["cycle_warp_us"]), 3)
                print(json.dumps({"B": B, **e}), flush=True)
                res[f"alone_B{B}"] = e
                del graphs
                torch.cuda.empty_cache()
    if "b" in a.only:
        from prior_flow_amd.prior_raft import PriOr_RAFT, state_dict_shapes
        args = argparse.Namespace(lr=1e-4, wdecay=5e-5, epsilon=1e-8, num_steps=100000, clip=1.0)

        def fresh():
            model = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
            model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
            model = model.cuda().train()
            model.freeze_bn()
            return (model,) + tuple(tr.fetch_optimizer(args, model))

        i1, i2 = (t.cuda() for t in synthetic_pair(2, H, W, seed=9))
        gen = torch.Generator().manual_seed(4)
        gt = (torch.rand(2, 2, H, W, generator=gen) * 6 - 3).cuda()
        valid = torch.ones(2, H, W, device=dev)
        m_sup, m_ss = fresh(), fresh()
        sup, crit = tr.uniform_loss(H, W), ss.SelfSupervisedLoss(H, W)
        steps = {"train_step_B2_ms": lambda: tr.train_step(*m_sup, sup, i1, i2, gt, valid, iters=a.iters),
                 "train_step_selfsup_B1_ms": lambda: ss.train_step_selfsup(*m_ss, crit, i1[:1], i2[:1], iters=a.iters),
                 "train_step_selfsup_B1_no_occlusion_ms": lambda: ss.train_step_selfsup(*m_ss, crit, i1[:1], i2[:1], iters=a.iters,
                                                                                       occlusion="none")}
        b = {k: [] for k in steps}
        for fn in steps.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in steps.items():
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                b[k].append(round(1000.0 * (time.perf_counter() - t0) / a.steps, 3))
        med = b["median"] = {k: statistics.median(b[k]) for k in steps}
        b["spread"] = {k: spread(b[k]) for k in steps}
        b["selfsup_over_supervised"] = round(med["train_step_selfsup_B1_ms"] / med["train_step_B2_ms"], 3)
        b["iters"] = a.iters
        print(json.dumps(b), flush=True)
        res["step"] = b
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
